"""AdamW + global-norm clipping on flat fp32 arenas (upstream trainer.py:311-312: ``clip_grad_norm_`` + ``optimizer.step()``).

Every parameter becomes a view into one parameter arena and every ``.grad`` a view into one gradient arena of the same
layout (the gradient arena is also the message of the data-parallel all-reduce); the two AdamW moments are arenas too.  The
step is then two kernel launches (``etm_grad_sqnorm``, ``etm_adamw_clip``; csrc/optim.hip) whatever the number of parameters,
with the learning rate and the step counter on the device so that a captured HIP graph replays it under changing schedules.
``state_dict`` keys, shapes and values of the model are untouched (views share storage, nothing is renamed).
"""
import struct

import torch

from . import lib as _lib


class KlGate:
    """State of the KL early stop of one update (csrc/optim.hip: etm_grad_sqnorm_gated / etm_adamw_clip_gated), handed to
    ``FlatAdamW.step``: ``limit`` (a float32 value), ``gate`` (device int64[3]: stopped, steps applied in this update, the bits of the
    kl that tripped), ``host_word`` (pinned int64[1] that receives steps applied + 1 at the first dropped step, or None) and ``kl``, the
    one-element float32 device tensor the next step compares: the caller points it at the step's own statistic before every step."""

    def __init__(self, limit, device, host_word=True):
        self.limit = float(limit)
        self.gate = torch.zeros(3, dtype=torch.int64, device=device)
        self.host_word = torch.zeros(1, dtype=torch.int64).pin_memory() if host_word else None
        self.kl = None

    def reset(self):
        """Start of an update (the previous update's launches have finished: it ended with a read-back)."""
        self.gate.zero_()
        if self.host_word is not None:
            self.host_word.zero_()

    def read(self):
        """(stopped, steps applied, kl that tripped or None) -- a device read-back."""
        stopped, applied, bits = (int(x) for x in self.gate.cpu().tolist())
        kl = struct.unpack("<f", struct.pack("<I", bits & 0xFFFFFFFF))[0] if stopped else None
        return bool(stopped), applied, kl


class AdaptiveLr:
    """The KL-adaptive learning rate (csrc/optim.hip: etm_grad_sqnorm_adaptive), handed to ``FlatAdamW.step``: ``rule``
    (utils.adaptive_lr_section: float32 values kl_low, kl_high, factor, min, max), ``state`` (device int64[2]: raises and cuts in this
    update) and ``kl``, the one-element float32 device tensor the next step's rule looks at: the caller points it at the step's own
    statistic before every step.  The learning rate itself is the optimiser's ``lr_dev``: with a rule attached the device owns it."""

    def __init__(self, rule, device):
        self.rule = dict(rule)
        self.kl_low, self.kl_high, self.factor = float(rule["kl_low"]), float(rule["kl_high"]), float(rule["factor"])
        self.lr_min, self.lr_max = float(rule["min"]), float(rule["max"])
        self.state = torch.zeros(2, dtype=torch.int64, device=device)
        self.kl = None

    def reset(self):
        """Start of an update: the counters are per update (the learning rate is never reset)."""
        self.state.zero_()

    def read(self):
        """(raises, cuts) of this update -- a device read-back."""
        raises, cuts = (int(x) for x in self.state.cpu().tolist())
        return raises, cuts


class FlatAdamW:
    N_PARTIAL = 1024

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
        self.params = [p for p in params if p.requires_grad]
        if not self.params or not self.params[0].is_cuda:
            raise RuntimeError("FlatAdamW needs parameters on the MI355X (HIP) device")
        dev = self.params[0].device
        self.device = dev
        self.total = sum(p.numel() for p in self.params)
        padded = (self.total + 3) // 4 * 4
        self.flat_params = torch.zeros(padded, dtype=torch.float32, device=dev)
        self.flat_grads = torch.zeros(padded, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(padded, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(padded, dtype=torch.float32, device=dev)
        self.grad_views = []
        off = 0
        with torch.no_grad():
            for p in self.params:
                if p.dtype != torch.float32:
                    raise TypeError("FlatAdamW: float32 parameters only")
                n = p.numel()
                view = self.flat_params[off: off + n].view(p.shape)
                view.copy_(p.data)
                p.data = view                                   # the parameter now lives in the arena
                p.grad = self.flat_grads[off: off + n].view(p.shape)
                self.grad_views.append(p.grad)
                off += n
        self.lr_dev = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        self._lr_host = float(lr)
        self.step_dev = torch.zeros((), dtype=torch.int64, device=dev)
        self.partial = torch.zeros(self.N_PARTIAL, dtype=torch.float32, device=dev)
        self.total_norm = torch.zeros((), dtype=torch.float32, device=dev)     # un-clipped gradient norm of the last step
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.adaptive = None            # an AdaptiveLr once ``attach_adaptive`` was called: lr_dev then moves on the device

    def attach_adaptive(self, adapt):
        """From here on ``lr_dev`` belongs to the device (the rule of ``adapt`` moves it inside ``step(adapt=adapt)``): ``state_dict``
        stores the device value, and ``set_lr`` is refused -- the caller's schedule must not write over what the rule decided."""
        self.adaptive = adapt

    def set_lr(self, lr):
        if self.adaptive is not None:
            raise RuntimeError("FlatAdamW.set_lr with an adaptive learning rate attached: the device owns lr_dev; do not call set_lr")
        if float(lr) != self._lr_host:
            self.lr_dev.fill_(float(lr))
            self._lr_host = float(lr)

    def zero_grad(self):
        self.flat_grads.zero_()

    def step(self, max_grad_norm=0.0, grad_scale=1.0, gate=None, adapt=None):
        """Clip the gradient arena to ``max_grad_norm`` (global L2 norm, the rule of ``clip_grad_norm_``; <= 0: no clipping) and
        apply one AdamW update.  Two launches on the current stream.  ``grad_scale``: the arena holds gradient / grad_scale
        (data parallel: the all-reduced sum, grad_scale = 1 / world); the scale rides in the clip coefficient.  A non-finite norm
        poisons the step as upstream's does (``max_grad_norm`` > 0): one NaN gradient makes every gradient, parameter and moment NaN, one
        Inf makes that element NaN and every other gradient 0; without clipping a NaN stays in its element.  ``gate`` (a ``KlGate``;
        None: exactly the two ungated calls): the step is dropped -- parameters, moments, gradients and ``step_dev`` keep every bit --
        when an earlier step under this gate was dropped or when not ``gate.kl <= gate.limit``; still two launches.  ``adapt`` (an
        ``AdaptiveLr``; None: exactly the calls above): the norm launch first moves ``lr_dev`` on ``adapt.kl`` (utils.adaptive_lr_step;
        not behind a stopped gate), then tests the gate; this step's AdamW launch -- the ungated or the gated one, as they are -- runs
        with the new rate.  Still two launches."""
        lib = _lib.load()
        st = torch.cuda.current_stream(self.device).cuda_stream
        n = self.flat_params.numel()
        if adapt is not None:
            self.adaptive = adapt           # (a step under a rule attaches it: lr_dev is the device's from here on)
            kls =[adapt.kl] + ([gate.kl] if gate is not None else [])
            for kl in kls:
                if kl is None or not kl.is_cuda or kl.dtype != torch.float32 or kl.numel() != 1:
                    raise ValueError("FlatAdamW.step: adapt.kl (and gate.kl) must be a one-element float32 device tensor (the step's own "
                                     "kl statistic)")
            if gate is not None and gate.kl.data_ptr() != adapt.kl.data_ptr():
                raise ValueError("FlatAdamW.step: adapt.kl and gate.kl must be the same element (the step's own kl statistic)")
            word = gate.host_word.data_ptr() if gate is not None and gate.host_word is not None else 0
            _lib.check(lib.etm_grad_sqnorm_adaptive(self.flat_grads.data_ptr(), n, self.partial.data_ptr(), self.N_PARTIAL,
                                                    self.step_dev.data_ptr(), adapt.kl.data_ptr(), self.lr_dev.data_ptr(), adapt.kl_low,
                                                    adapt.kl_high, adapt.factor, adapt.lr_min, adapt.lr_max, adapt.state.data_ptr(),
                                                    gate.limit if gate is not None else 0.0, gate.gate.data_ptr() if gate is not None else 0,
                                                    word, st), "etm_grad_sqnorm_adaptive")
            tail = (self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), n,
                    self.partial.data_ptr(), self.N_PARTIAL, self.lr_dev.data_ptr(), self.step_dev.data_ptr(), self.betas[0], self.betas[1],
                    self.eps, self.weight_decay, float(max_grad_norm), float(grad_scale), self.total_norm.data_ptr())
            if gate is None:
                _lib.check(lib.etm_adamw_clip(*tail, st), "etm_adamw_clip")
            else:
                _lib.check(lib.etm_adamw_clip_gated(*tail, gate.gate.data_ptr(), st), "etm_adamw_clip_gated")
            return
        if gate is not None:
            kl = gate.kl
            if kl is None or not kl.is_cuda or kl.dtype != torch.float32 or kl.numel() != 1:
                raise ValueError("FlatAdamW.step: gate.kl must be a one-element float32 device tensor (the step's own kl statistic)")
            word = gate.host_word.data_ptr() if gate.host_word is not None else 0
            _lib.check(lib.etm_grad_sqnorm_gated(self.flat_grads.data_ptr(), n, self.partial.data_ptr(), self.N_PARTIAL,
                                                 self.step_dev.data_ptr(), kl.data_ptr(), gate.limit, gate.gate.data_ptr(), word, st),
                       "etm_grad_sqnorm_gated")
            _lib.check(lib.etm_adamw_clip_gated(self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(),
                                                self.exp_avg_sq.data_ptr(), n, self.partial.data_ptr(), self.N_PARTIAL, self.lr_dev.data_ptr(),
                                                self.step_dev.data_ptr(), self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                                float(max_grad_norm), float(grad_scale), self.total_norm.data_ptr(), gate.gate.data_ptr(), st),
                       "etm_adamw_clip_gated")
            return
        _lib.check(lib.etm_grad_sqnorm(self.flat_grads.data_ptr(), n, self.partial.data_ptr(), self.N_PARTIAL, self.step_dev.data_ptr(), st),
                   "etm_grad_sqnorm")
        _lib.check(lib.etm_adamw_clip(self.flat_params.data_ptr(), self.flat_grads.data_ptr(), self.exp_avg.data_ptr(),
                                      self.exp_avg_sq.data_ptr(), n, self.partial.data_ptr(), self.N_PARTIAL, self.lr_dev.data_ptr(),
                                      self.step_dev.data_ptr(), self.betas[0], self.betas[1], self.eps, self.weight_decay,
                                      float(max_grad_norm), float(grad_scale), self.total_norm.data_ptr(), st), "etm_adamw_clip")

    # ------------------------------------------------------------------ checkpointing
    _HYPER = ("betas", "eps", "weight_decay", "total", "padded")

    def state_dict(self):
        """Everything that continues the optimiser: both moment arenas as numpy arrays (padded length), the device step counter, the
        learning rate (the python float ``lr_dev`` was last filled with; with an adaptive rule attached the device's own value, a float32
        held exactly), and the hyper-parameters and sizes ``load_state_dict`` checks."""
        if self.adaptive is not None:
            self._lr_host = float(self.lr_dev.item())
        return {"exp_avg": self.exp_avg.cpu().numpy(), "exp_avg_sq": self.exp_avg_sq.cpu().numpy(), "step": int(self.step_dev.item()),
                "lr": self._lr_host, "betas": [self.betas[0], self.betas[1]], "eps": self.eps,
                "weight_decay": self.weight_decay, "total": int(self.total), "padded": int(self.flat_params.numel())}

    def load_state_dict(self, state):
        """Copies ``state`` (of ``state_dict``) INTO the existing arenas, ``step_dev`` and ``lr_dev`` -- no tensor is rebound: captured
        graphs hold these addresses.  A different ``total`` / padded length or different hyper-parameters are refused by name."""
        mine = {"betas": [self.betas[0], self.betas[1]], "eps": self.eps, "weight_decay": self.weight_decay, "total": int(self.total),
                "padded": int(self.flat_params.numel())}
        diff = [f"{k}: saved {state.get(k)!r}, this optimiser {mine[k]!r}" for k in self._HYPER
                if (list(state[k]) if k == "betas" and k in state else state.get(k)) != mine[k]]
        if diff:
            raise ValueError("FlatAdamW.load_state_dict: the saved state does not fit this optimiser (" + "; ".join(diff) + ")")
        import numpy as np
        arenas = {}
        for name in ("exp_avg", "exp_avg_sq"):
            a = np.ascontiguousarray(state[name])
            if a.dtype != np.float32 or a.shape != (mine["padded"],):
                raise ValueError(f"FlatAdamW.load_state_dict: {name} is {a.dtype}{list(a.shape)}, expected float32[{mine['padded']}]")
            arenas[name] = torch.from_numpy(a)
        with torch.no_grad():
            self.exp_avg.copy_(arenas["exp_avg"])
            self.exp_avg_sq.copy_(arenas["exp_avg_sq"])
            self.step_dev.fill_(int(state["step"]))
            self.lr_dev.fill_(float(state["lr"]))
        self._lr_host = float(state["lr"])              # (set_lr compares against this: it stays in step with lr_dev)
