"""torch-facing wrappers (autograd glue) around the C ABI of libetm_hip.so.

PyTorch is plumbing here: it owns the device buffers and the stream; the math of the three hot ops runs in the
hand-written kernels.  Every entry point requires HIP device tensors and raises otherwise -- no CPU/eager fallback.
"""
import ctypes
import dataclasses
import itertools

import torch

from . import lib as _lib

_workspaces = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _need_dev(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("etm ops need tensors on the MI355X (HIP) device; there is no CPU path in this build "
                               "(the CPU oracle lives under oracle/ and is test-only)")


def _f32c(t, name):
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _obs_c(t, name):
    """An observation operand: float32, or uint8 where byte k stands for float32(k) / float32(255) (``bytes_to_unit``)."""
    if t is not None and t.dtype == torch.uint8:
        return t if t.is_contiguous() else t.contiguous()
    return _f32c(t, name)


def byte_unit_table():
    """The 256 fp32 values a byte observation stands for: ``np.float32(k) / np.float32(255)``, correctly rounded (numpy, host).
    The kernels form the same values from the byte (etm_byte_unit, csrc/etm_common.h); k * (1 / 255) is NOT this value."""
    import numpy as np
    return np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)


def bytes_to_unit(x, index=None, out=None):
    """uint8 device tensor [R, ...] -> float32 of the same shape with every byte k as float32(k) / 255 (etm_bytes_to_unit); with
    ``index`` (int64 device tensor [n]) the rows x[index] -> [n, ...].  The fallback in front of every float kernel that has no
    byte form.  Any row length, any storage offset of ``x``."""
    lib = _lib.load()
    _need_dev(x, index, out)
    if x.dtype != torch.uint8:
        raise TypeError(f"bytes_to_unit needs uint8, got {x.dtype}")
    if index is not None and index.dtype != torch.int64:
        raise TypeError("bytes_to_unit: index must be int64")
    if x.dim() == 0 or x.numel() == 0:
        raise ValueError("bytes_to_unit needs a non-empty tensor of at least one dimension")
    x = x if x.is_contiguous() else x.contiguous()
    rows = x.shape[0] if index is None else index.numel()
    row_bytes = x[0].numel()
    shape = (rows,) + tuple(x.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise TypeError("bytes_to_unit: out must be a contiguous float32 tensor of the result's shape")
    if rows:
        _lib.check(lib.etm_bytes_to_unit(_ptr(x), _ptr(index), _ptr(out), rows, row_bytes, _stream()), "etm_bytes_to_unit")
    return out


_frozen = set()
_retired = []


def workspace(nbytes, device, tag="ws"):
    """Scratch buffer of at least ``nbytes`` per (tag, device), grown on demand.  Once a HIP graph has captured a buffer's
    address (``freeze_workspaces``) that buffer is never freed: a later, larger request gets a NEW buffer and the old one is
    retired but kept alive, so replays of the captured graph keep writing to memory they own."""
    key = (tag, device.index)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None and key in _frozen:
            _retired.append(buf)
            _frozen.discard(key)
        buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def freeze_workspaces(device):
    """Called by the trainer right after a graph capture: the scratch buffers that exist now are referenced by the graph."""
    for key in _workspaces:
        if key[1] == device.index:
            _frozen.add(key)


class WindowSpec:
    """Where the memory-window rows of a batch live: X[n, l] = bank[ep[n], win[n, l], block, :].

    bank_ptr/ep_stride/row_stride/block_stride are in float32 elements.  ``ep`` may be None (ep[n] = n).
    """

    __slots__ = ("bank", "ep_stride", "row_stride", "block_stride", "ep", "win", "pidx", "mask", "N", "L", "pos_included", "row_stats",
                 "_gathered_stats")

    def __init__(self, bank, ep_stride, row_stride, block_stride, ep, win, pidx, mask):
        _need_dev(bank, ep, win, pidx, mask)
        if bank.dtype != torch.float32 or bank.stride(-1) != 1:
            raise TypeError("memory bank must be float32 with a contiguous feature dimension")
        for s in (ep_stride, row_stride, block_stride):
            if s % 4 != 0:
                raise ValueError("memory bank strides must be multiples of 4 floats (16-byte rows)")
        if bank.data_ptr() % 16 != 0:
            raise ValueError("memory bank must be 16-byte aligned")
        self.bank = bank
        self.ep_stride, self.row_stride, self.block_stride = int(ep_stride), int(row_stride), int(block_stride)
        self.N, self.L = int(win.shape[0]), int(win.shape[1])
        self.pos_included = False   # True: the bank rows already contain their positional rows (see Transformer.bank_with_positions)
        # round 5, pre-LN models: (mean, rstd) of every bank row [blocks, E, T, 2] (bank_row_stats; once per update: norm_kv's statistics
        # do not depend on its gain / bias) -- the window passes then gather their [N, L, 2] statistics instead of re-reading every
        # window row to compute them (472 MB per launch at config 5); None: computed per window row inside etm_window_fwd
        self.row_stats = None
        self._gathered_stats = {}
        self.ep = None if ep is None else ep.to(torch.int64).contiguous()
        self.win = win.to(torch.int64).contiguous()
        self.pidx = None if pidx is None else pidx.to(torch.int64).contiguous()
        if mask.dtype == torch.bool:
            m = mask.contiguous().view(torch.uint8)
        elif mask.dtype == torch.uint8:
            m = mask.contiguous()
        else:
            m = (mask != 0).to(torch.uint8)  # reference semantics: `mask == 0` is masked (transformer.py:66)
        self.mask = m

    @classmethod
    def from_bank(cls, bank, ep, win, pidx, mask):
        """bank: [E, T, nb, D] episode bank."""
        return cls(bank, bank.stride(0), bank.stride(1), bank.stride(2), ep, win, pidx, mask)

    @classmethod
    def from_windows(cls, memories, pidx, mask):
        """memories: pre-gathered windows [N, L, nb, D] (the reference's calling convention) or [N, L, D]."""
        n, l = memories.shape[0], memories.shape[1]
        win = torch.arange(l, device=memories.device, dtype=torch.int64).unsqueeze(0).expand(n, l)
        bstride = memories.stride(2) if memories.dim() == 4 else 0
        return cls(memories, memories.stride(0), memories.stride(1), bstride, None, win, pidx, mask)

    def block_ptr(self, block):
        return self.bank.data_ptr() + 4 * block * self.block_stride

    def window_stats(self, block):
        """[N, L, 2] LayerNorm statistics of this batch's window rows of ``block``, gathered from ``row_stats`` (None without it)."""
        if self.row_stats is None:
            return None
        got = self._gathered_stats.get("all")
        if got is None:                     # one gather for all blocks (the window indices are the same): 2 launches per step, not 2 per block
            ep = self.ep if self.ep is not None else torch.arange(self.N, device=self.win.device)
            got = self._gathered_stats["all"] = self.row_stats[:, ep.unsqueeze(1), self.win].contiguous()       # [blocks, N, L, 2]
        return got[block]


def bank_row_stats(bank, eps, out=None):
    """(mean, 1 / sqrt(var + eps)) of every row of a BLOCK-MAJOR episode bank view [E, T, blocks, D] (memory order [blocks][E][T][D],
    buffer.py) -> [blocks, E, T, 2] (etm_ln_row_stats: one pass over the used part of the bank, once per update)."""
    lib = _lib.load()
    E, T, nb, D = bank.shape
    rows = bank.permute(2, 0, 1, 3)                      # [blocks, E, T, D]: contiguous for a block-major bank
    if not rows.is_contiguous():
        rows = rows.contiguous()
    if out is None or out.shape != (nb, E, T, 2):
        out = torch.empty((nb, E, T, 2), dtype=torch.float32, device=bank.device)
    _lib.check(lib.etm_ln_row_stats(_ptr(rows), float(eps), _ptr(out), nb * E * T, D, _stream()), "etm_ln_row_stats")
    return out


class _MhaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, wk, wv, ln_g, ln_b, pos, spec, block, num_heads, ln_eps):
        lib = _lib.load()
        _need_dev(q, wk, wv, ln_g, ln_b, pos)
        q, wk, wv = _f32c(q, "q"), _f32c(wk, "wk"), _f32c(wv, "wv")
        ln_g, ln_b, pos = _f32c(ln_g, "ln_g"), _f32c(ln_b, "ln_b"), _f32c(pos, "pos")
        N, D = q.shape
        L, H = spec.L, int(num_heads)
        if N != spec.N:
            raise ValueError("query batch and window batch differ")
        need_grad = any(ctx.needs_input_grad[:6])
        ctx.set_materialize_grads(False)      # the attention weights are an output nobody differentiates: no zero tensor for them
        dev = q.device
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
        att = torch.empty((N, H, L), dtype=torch.float32, device=dev)
        k_save = v_save = None
        if need_grad:
            k_save = torch.empty((N, L, D), dtype=torch.float32, device=dev)
            v_save = torch.empty((N, L, D), dtype=torch.float32, device=dev)
        ln_stats = torch.empty((N, L, 2), dtype=torch.float32, device=dev) if ln_g is not None else None
        pidx = spec.pidx if pos is not None else None
        rc = lib.etm_mha_fwd(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                             _ptr(spec.mask), _ptr(pos), _ptr(ln_g), _ptr(ln_b), float(ln_eps), _ptr(q), _ptr(wk), _ptr(wv),
                             _ptr(out), _ptr(att), _ptr(k_save), _ptr(v_save), _ptr(ln_stats), N, L, D, H, _stream())
        _lib.check(rc, "etm_mha_fwd")
        if need_grad:
            ctx.spec, ctx.block, ctx.H = spec, block, H
            ctx.has_ln, ctx.has_pos = ln_g is not None, pos is not None
            saved = [q, wk, wv, att, k_save, v_save]
            if ln_g is not None:
                saved += [ln_g, ln_b, ln_stats]
            if pos is not None:
                saved += [pos]
            ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, d_out, _d_att):
        if d_out is None:
            return (None,) * 10
        lib = _lib.load()
        spec, block, H = ctx.spec, ctx.block, ctx.H
        saved = list(ctx.saved_tensors)
        q, wk, wv, att, k_save, v_save = saved[:6]
        rest = saved[6:]
        ln_g = ln_b = ln_stats = pos = None
        if ctx.has_ln:
            ln_g, ln_b, ln_stats = rest[:3]
            rest = rest[3:]
        if ctx.has_pos:
            pos = rest[0]
        N, D = q.shape
        L = spec.L
        dev = q.device
        d_out = _f32c(d_out, "d_ctx")
        d_q = torch.empty_like(q)
        d_e = torch.empty((N, H, L), dtype=torch.float32, device=dev)
        d_wk = torch.empty_like(wk)
        d_wv = torch.empty_like(wv)
        want_ln = ctx.has_ln and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4])
        want_pos = ctx.has_pos and ctx.needs_input_grad[5]
        d_ln_g = torch.zeros_like(ln_g) if want_ln else None
        d_ln_b = torch.zeros_like(ln_b) if want_ln else None
        d_pos = torch.zeros_like(pos) if want_pos else None
        nbytes = lib.etm_mha_bwd_workspace_bytes(N, L, D)
        ws = workspace(nbytes, dev, "mha_bwd")
        pidx = spec.pidx if pos is not None else None
        rc = lib.etm_mha_bwd(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                             _ptr(spec.mask), _ptr(pos), _ptr(ln_g), _ptr(ln_b), _ptr(q), _ptr(wk), _ptr(wv), _ptr(att),
                             _ptr(k_save), _ptr(v_save), _ptr(ln_stats), _ptr(d_out), _ptr(d_q), _ptr(d_e), _ptr(d_wk), _ptr(d_wv),
                             _ptr(d_ln_g), _ptr(d_ln_b), _ptr(d_pos), _ptr(ws), nbytes, N, L, D, H, _stream())
        _lib.check(rc, "etm_mha_bwd")
        return d_q, d_wk, d_wv, d_ln_g, d_ln_b, d_pos, None, None, None, None


class _WindowFn(torch.autograd.Function):
    """Folded window attention pass: u [H,N,D] -> (z [H,N,D], att [N,H,L]); see csrc/window_attn.hip."""

    @staticmethod
    def forward(ctx, u, ln_g, ln_b, pos, spec, block, ln_eps):
        lib = _lib.load()
        _need_dev(u, ln_g, ln_b, pos)
        u = _f32c(u, "u")
        ln_g_param, ln_b_param = ln_g, ln_b
        ln_g, ln_b, pos = _f32c(ln_g, "ln_g"), _f32c(ln_b, "ln_b"), _f32c(pos, "pos")
        H, N, D = u.shape
        L = spec.L
        if N != spec.N:
            raise ValueError("query batch and window batch differ")
        ctx.set_materialize_grads(False)      # (no zero tensor for the gradient of the attention weights)
        dev = u.device
        att = torch.empty((N, H, L), dtype=torch.float32, device=dev)
        z = torch.empty((H, N, D), dtype=torch.float32, device=dev)
        ln_stats, stats_ready = None, 0
        if ln_g is not None:
            ln_stats = spec.window_stats(block) if pos is None else None      # (row_stats were taken with the positional rows included)
            stats_ready = int(ln_stats is not None)
            if ln_stats is None:
                ln_stats = torch.empty((N, L, 2), dtype=torch.float32, device=dev)
        pidx = spec.pidx if pos is not None else None
        rc = lib.etm_window_fwd(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                                _ptr(spec.mask), _ptr(pos), _ptr(ln_g), _ptr(ln_b), float(ln_eps), _ptr(u), N * D, D, _ptr(att),
                                _ptr(z), N * D, D, _ptr(ln_stats), stats_ready, N, L, D, H, _stream())
        _lib.check(rc, "etm_window_fwd")
        if any(ctx.needs_input_grad[:4]):
            ctx.spec, ctx.block = spec, block
            ctx.has_ln, ctx.has_pos = ln_g is not None, pos is not None
            ctx.ln_params = (ln_g_param, ln_b_param) if ln_g is not None else None      # the parameters themselves (arena views by address)
            saved = [u, att]
            if ln_g is not None:
                saved += [ln_g, ln_b, ln_stats, z]      # (z: norm_kv's gradients are formed from the passes' outputs, round 6)
            if pos is not None:
                saved += [pos]
            ctx.save_for_backward(*saved)
        ctx.mark_non_differentiable(att)
        return z, att

    @staticmethod
    def backward(ctx, gz, _d_att):
        if gz is None:
            return (None,) * 7
        lib = _lib.load()
        spec, block = ctx.spec, ctx.block
        saved = list(ctx.saved_tensors)
        u, att = saved[:2]
        rest = saved[2:]
        ln_g = ln_b = ln_stats = pos = None
        z_fwd = None
        if ctx.has_ln:
            ln_g, ln_b, ln_stats, z_fwd = rest[:4]
            rest = rest[4:]
        if ctx.has_pos:
            pos = rest[0]
        H, N, D = u.shape
        L = spec.L
        dev = u.device
        gz = _f32c(gz, "d_z")
        d_e = torch.empty((N, H, L), dtype=torch.float32, device=dev)
        du = torch.empty((H, N, D), dtype=torch.float32, device=dev)
        pidx = spec.pidx if pos is not None else None
        rc = lib.etm_window_bwd(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                                _ptr(spec.mask), _ptr(pos), _ptr(ln_g), _ptr(ln_b), _ptr(ln_stats), _ptr(att), _ptr(gz), N * D, D,
                                _ptr(d_e), _ptr(du), N * D, D, N, L, D, H, _stream())
        _lib.check(rc, "etm_window_bwd")
        want_ln = ctx.has_ln and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        want_pos = ctx.has_pos and ctx.needs_input_grad[3]
        d_ln_g = d_ln_b = d_pos = None
        if _ln_grad_kernel_route(D, H, L, want_ln, want_pos):
            # norm_kv's gain / bias gradients as per-workgroup partial rows (csrc/window_ln_grad.hip), summed by the grouped column-sum
            # reduction of the step, or -- without a collector / once it is full -- by the same kernel launched here.  NOT by torch's
            # column sum: its two-stage reduction (a memset node for its semaphore + the reduce kernel) returns wrong sums in some
            # replays of a captured graph on this runtime (profiles/r05/graph_reduce_hazard.txt).
            # Round 6 ("outputs", the default): from the window passes' OUTPUTS -- u, gz, du and the forward's z -- an elementwise
            # pass over four [H, N, D] tensors; round 5 ("rows"): a third pass over the gathered window rows (8 x the bytes).
            rows = lib.etm_window_ln_grad_rows(N)
            partial = torch.empty((rows, 2 * D), dtype=torch.float32, device=dev)
            if _ln_grad_kernel == "rows":
                rc = lib.etm_window_ln_grad(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                                            _ptr(pos), _ptr(ln_stats), _ptr(att), _ptr(d_e), _ptr(u), _ptr(gz), N * D, D, _ptr(partial),
                                            N, L, D, H, _stream())
                _lib.check(rc, "etm_window_ln_grad")
            else:
                rc = lib.etm_window_ln_grad_from_outputs(_ptr(u), _ptr(gz), _ptr(du), _ptr(z_fwd), _ptr(att), _ptr(d_e), _ptr(ln_g), _ptr(ln_b),
                                                         N * D, D, _ptr(partial), N, L, D, H, _stream())
                _lib.check(rc, "etm_window_ln_grad_from_outputs")
                # the identity divides by the gain: small-gain columns (zero included) from the window rows, on the same stream
                rc = lib.etm_window_ln_grad_guarded(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win),
                                                    _ptr(pidx), _ptr(pos), _ptr(ln_stats), _ptr(att), _ptr(d_e), _ptr(u), _ptr(gz), N * D, D,
                                                    _ptr(ln_g), _ptr(ln_b), LN_GRAD_GUARD_TAU, _ptr(partial), N, L, D, H, _stream())
                _lib.check(rc, "etm_window_ln_grad_guarded")
            g_param, b_param = ctx.ln_params
            d_ln_g, d_ln_b = DeferredDw.reduce_colsums(partial, rows, 2 * D, [(0, D, g_param.data_ptr()), (D, D, b_param.data_ptr())])
            return du, d_ln_g, d_ln_b, None, None, None, None
        if want_ln or want_pos:
            d_ln_g = torch.zeros_like(ln_g) if want_ln else None
            d_ln_b = torch.zeros_like(ln_b) if want_ln else None
            d_pos = torch.zeros_like(pos) if want_pos else None
            uw = torch.empty((2, N, H, D), dtype=torch.float32, device=dev)
            uw[0].copy_(u.transpose(0, 1))
            uw[1].copy_(gz.transpose(0, 1))
            rc = lib.etm_window_dx(spec.block_ptr(block), spec.ep_stride, spec.row_stride, _ptr(spec.ep), _ptr(spec.win), _ptr(pidx),
                                   _ptr(pos), _ptr(ln_g), _ptr(ln_b), _ptr(ln_stats), _ptr(att), _ptr(d_e), _ptr(uw), _ptr(d_ln_g),
                                   _ptr(d_ln_b), _ptr(d_pos), N, L, D, H, _stream())
            _lib.check(rc, "etm_window_dx")
        return du, d_ln_g, d_ln_b, d_pos, None, None, None


def colsum_rows(partial, P, C):
    """Column sums of the first ``C`` columns of ``partial`` [P, ld] by the library's fixed-order reduction (the summation tree of the
    grouped launch a ``DeferredDw`` collector would have used: same bits with and without a collector)."""
    out = torch.empty(C, dtype=torch.float32, device=partial.device)
    _colsum_reduce([(partial, 0, P, C, partial.stride(0), out)])
    return out


# "outputs": columns with |gain| < tau max(1, |bias|) get their gain gradient from the rows kernel (etm_window_ln_grad_guarded).  The
# identity's error in such a column grows as (|g| + |b|) / |g| (tests/test_gpu_parity.py, LayerNorm value edges: measured there).
LN_GRAD_GUARD_TAU = 0.25
_ln_grad_kernel = "outputs"      # norm_kv's gain / bias gradients by csrc/window_ln_grad.hip: "outputs" (from the passes' outputs,
#                                    round 6) or "rows" (a pass over the window rows, round 5); False: the generic dX kernel, etm_window_dx


def set_ln_grad_kernel(on):
    """True / "outputs", "rows", or False (trainer.py: ``fused_ln_grad``)."""
    global _ln_grad_kernel
    if on not in (True, False, "outputs", "rows"):
        raise ValueError(f"fused_ln_grad must be true, false, 'outputs' or 'rows', got {on!r}")
    _ln_grad_kernel = "outputs" if on is True else on


ATTENTION_IMPLS = ("folded", "dense")
_default_impl = "folded"


def set_attention_impl(impl):
    """Select the kernel family behind ``mha``: 'folded' (one HBM-bound pass over the window, default) or 'dense' (the
    K/V projections of the window as fp32-MFMA contractions).  Both compute transformer.py:31-86 for a single query."""
    global _default_impl
    if impl not in ATTENTION_IMPLS:
        raise ValueError(f"attention impl must be one of {ATTENTION_IMPLS}, got {impl!r}")
    _default_impl = impl


_LDS_BYTES = 160 * 1024      # one workgroup's LDS on gfx950


def folded_supported(D, L, num_heads):
    """Shapes the folded window pass (etm_window_fwd / etm_window_bwd) runs: check_common's rules, dispatch_rows' row tilings and
    launch_pass3's LDS budget (H padded window rows of attention weights + the per-wave partial sums)."""
    H = int(num_heads)
    if H <= 0 or D % H != 0 or D % 32 != 0 or (D // H) % 2 != 0 or not ((D <= 512 and L <= 128) or (D <= 1024 and L <= 64)):
        return False
    nj = {5: 6, 7: 8}.get(-(-D // 128), -(-D // 128))
    rw, nw = (8, 4) if L <= 32 else ((8, 8) if L <= 64 else (16, 8))
    return (H * nw * rw + nw * 4 * nj * 128) * 4 <= _LDS_BYTES


def _dx_lds_ok(D, H, L):
    """bwd_dx_kernel (etm_mha_bwd step B3, etm_window_dx): 2HD + 8D + 2HL floats of LDS."""
    return (2 * H * D + 8 * D + 2 * H * L) * 4 <= _LDS_BYTES


def dense_supported(D, L, num_heads, backward=True):
    """Shapes the dense kernels run: etm_mha_fwd's rules, and with ``backward`` etm_mha_bwd's LDS checks (made for every call)."""
    H = int(num_heads)
    if H <= 0 or D % H != 0:
        return False
    hd = D // H
    if D % 32 != 0 or hd % 32 != 0 or hd > 128 or L > 128 or D > 1024:
        return False
    return not backward or (_dx_lds_ok(D, H, L) and (D + 3 * H * L) * 4 <= _LDS_BYTES)


def _ln_grad_kernel_route(D, H, L, want_ln, want_pos):
    """_WindowFn.backward: norm_kv's gradients by csrc/window_ln_grad.hip (else by etm_window_dx)."""
    return bool(_ln_grad_kernel) and want_ln and not want_pos and D % 128 == 0 and D <= 512 and H <= 8 and L <= 128


def attention_supported(D, H, L, ln=False, pos_grad=False, backward=True, impl=None):
    """The kernel family ("folded" / "dense") that ``mha`` runs for this shape, or None if neither can run it.  ``ln``: norm_kv's
    gain / bias want gradients; ``pos_grad``: a learned positional table does; ``backward``: the backward pass must run too.
    The folded forward falls back to the dense kernels when it cannot run the shape; its norm_kv / positional gradients go
    through the dX kernel unless window_ln_grad.hip takes them, and the dense backward needs that same dX kernel's LDS."""
    impl = _default_impl if impl is None else impl
    if impl not in ATTENTION_IMPLS:
        raise ValueError(f"attention impl must be one of {ATTENTION_IMPLS}, got {impl!r}")
    D, H, L = int(D), int(H), int(L)
    if impl == "folded" and folded_supported(D, L, H):
        want_dx = backward and (pos_grad or ln) and not _ln_grad_kernel_route(D, H, L, ln, pos_grad)
        return "folded" if not want_dx or _dx_lds_ok(D, H, L) else None
    return "dense" if dense_supported(D, L, H, backward) else None


# ---------------------------------------------------------------------------------------------------------------
# Deferred weight gradients: dW = dy^T x of the dense layers, collected during backward and computed by ONE grouped launch
# (csrc/grouped_dw.hip) straight into the flat gradient arena.  Inactive (no collector) every layer computes its own dW as before.
class DeferredDw:
    """Context manager around ``loss.backward()``.  ``dest``: {parameter.data_ptr(): gradient view [out, in] in the arena}.
    Inside, the autograd functions below hand their gradient problems over through the class methods (each of which answers
    False / None when no collector is active or it refuses); ``flush()`` (called on exit) runs the grouped launches and ``pack()``
    puts every other gradient into the arena.  ``written``: data_ptr()s of the parameters whose gradient now sits in its arena view
    -- a parameter's first use only: the grouped launches OVERWRITE their destinations, so a second use of the same rows (tied
    weights, a layer applied twice) is refused, autograd keeps its gradient and ``pack()`` adds it to the view."""
    active = None
    last_flops = 0.0             # 2 * N * Ma * Nb summed over the problems of the most recent grouped launch (bench.py prices it with this)

    def __init__(self, dest, tail=True):
        self.dest = dest
        self.tail = tail         # the column sums of flush() ride in the grouped launch (etm_grouped_dw_tail); False: a launch of their own
        self.rows = {}           # parameter data_ptr -> [(first row, rows)] already taken (a second use of the same rows is refused)
        self.items = []          # (A, B, C view, Ma, Nb, lda, ldb, ldc)
        self.colsums = []        # (partial sums, first column, rows P, columns C, row stride, destination view)
        self.conv_wgrads = []    # (pixel slices, slice count, dw view, db view, Cout, C, KH, KW) of the encoder layers
        self.written = set()
        self.N = None

    def __enter__(self):
        DeferredDw.active = self
        return self

    def __exit__(self, *exc):
        DeferredDw.active = None
        if exc[0] is None:
            self.flush()
        return False

    def offer(self, a, b, weight, row0=0, rows=None, a_col0=0):
        """C = weight.grad[row0 : row0 + rows] (all rows if None) = a[:, a_col0 : a_col0 + rows]^T b.  a [N, *], b [N, in] contiguous
        rows.  Returns True when the problem was taken (shape supported, destination known); else the caller multiplies itself."""
        view = self.dest.get(weight.data_ptr())
        if view is None or not (a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.dim() == 2 and b.dim() == 2):
            return False
        n, nb = b.shape
        ma = view.shape[0] if rows is None else rows
        if a.stride(1) != 1 or b.stride(1) != 1 or a.shape[0] != n or (self.N is not None and n != self.N):
            return False
        lda, ldb, ldc = a.stride(0), b.stride(0), view.stride(0)
        lib = _lib.load()
        if not lib.etm_grouped_dw_supported(n, ma, nb, lda, ldb, ldc):       # (any number of problems: flush() launches them in chunks)
            return False
        c = view[row0: row0 + ma]
        if view.shape[1] != nb or (_ptr(b) % 16) or (_ptr(c) % 16) or ((_ptr(a) + 4 * a_col0) % 4):
            return False
        taken = self.rows.setdefault(weight.data_ptr(), [])
        if any(row0 < r0 + m and r0 < row0 + ma for r0, m in taken):
            return False
        taken.append((row0, ma))
        self.N = n
        self.items.append((a, b, c, ma, nb, lda, ldb, ldc, a_col0))
        self.written.add(weight.data_ptr())
        return True

    @classmethod
    def defer(cls, a, b, weight, **kw):
        """``offer()`` to the active collector: True when it took the problem."""
        return cls.active is not None and cls.active.offer(a, b, weight, **kw)

    @classmethod
    def defer_heads(cls, a, planes, weight):
        """The rows of head h of ``weight`` [D, D] = a[:, h hd : (h + 1) hd]^T planes[h] (a [N, D], planes [H, N, D]): H problems,
        taken all together or not at all -- a refusal leaves the collector exactly as it was before the first of them."""
        col = cls.active
        if col is None or not (a.is_contiguous() and planes.is_contiguous()):
            return False
        H, ptr = planes.shape[0], weight.data_ptr()
        hd = a.shape[1] // H
        before = (len(col.items), list(col.rows.get(ptr, ())), ptr in col.written, col.N)
        if all(col.offer(a, planes[h], weight, row0=h * hd, rows=hd, a_col0=h * hd) for h in range(H)):
            return True
        n_items, col.rows[ptr], was_written, col.N = before
        del col.items[n_items:]
        if not was_written:
            col.written.discard(ptr)
        return False

    @classmethod
    def claim(cls, ptrs):
        """The arena views of the parameters ``ptrs`` when the active collector knows every one as a contiguous view and none is
        written yet; they count as written from now on (the caller fills them, at once or through ``defer_conv_wgrad``).  Else None."""
        col = cls.active
        views = None if col is None else [col.dest.get(ptr) for ptr in ptrs]
        if views is None or any(v is None or not v.is_contiguous() for v in views) or any(ptr in col.written for ptr in ptrs):
            return None
        col.written.update(ptrs)
        return views

    @classmethod
    def defer_conv_wgrad(cls, slices, count, dw, db, cout, c, kh, kw):
        """An encoder layer's weight-gradient slices [count, Cout * K + Cout] (kept alive here), reduced into the views ``dw`` / ``db``
        (from ``claim``) by the ONE slice reduction of ``flush()``."""
        cls.active.conv_wgrads.append((slices, count, dw, db, cout, c, kh, kw))

    def offer_colsum(self, partial, P, ld, parts):
        """Second stage of column-sum gradients (LayerNorm weight / bias, linear bias): ``partial`` [P, ld] per-workgroup partial sums
        (a buffer of the caller's own, kept alive here), ``parts`` = [(first column, columns, parameter data_ptr)].  True: all
        destinations are known 1-D arena views and the sums will be written by the ONE reduction launch of ``flush()``."""
        views = [self.dest.get(ptr) for _, _, ptr in parts]
        if any(v is None or v.dim() != 1 or not v.is_contiguous() for v in views):
            return False
        if len(self.colsums) + len(parts) > _lib.load().etm_colsum_reduce_max_problems():
            return False
        for (c0, cols, ptr), v in zip(parts, views):
            if v.numel() != cols or ptr in self.written:
                return False
        for (c0, cols, ptr), v in zip(parts, views):
            self.colsums.append((partial, c0, P, cols, ld, v))
            self.written.add(ptr)
        return True

    @classmethod
    def colsum_workspace(cls, nbytes, P, ld, parts, device, tag):
        """Workspace of a kernel whose second stage sums its partial rows [P, ld] into the gradients ``parts`` (see ``offer_colsum``).
        (buffer, True): a private partial buffer the active collector took -- the kernel gets no destination, ``flush()`` reduces it;
        (buffer, False): the shared ``workspace(nbytes, device, tag)`` -- the kernel reduces into a destination of the caller's."""
        if cls.active is not None:
            part = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            if cls.active.offer_colsum(part, P, ld, parts):
                return part, True
        return workspace(nbytes, device, tag), False

    @classmethod
    def reduce_colsums(cls, partial, P, ld, parts):
        """The gradients ``parts`` of the partial rows ``partial`` [P, ld]: [None] * len(parts) when the active collector took them
        (``offer_colsum``), else their column sums, reduced at once by the same fixed-order kernel (``colsum_rows``)."""
        if cls.active is not None and cls.active.offer_colsum(partial, P, ld, parts):
            return [None] * len(parts)
        sums = colsum_rows(partial, P, ld)
        return [sums[c0: c0 + cols] for c0, cols, _ in parts]

    def flush(self):
        lib = _lib.load()
        cap = lib.etm_grouped_dw_max_problems()          # problems per launch (the kernel-argument table: 84)
        tail = bool(self.tail and self.items and self.colsums and all(max(c[2], c[3], c[4]) < 65536 for c in self.colsums))
        if self.conv_wgrads:
            _conv_wgrad_reduce(self.conv_wgrads)
        if self.colsums and not tail:
            _colsum_reduce(self.colsums)
        lo = 0
        while lo < len(self.items):
            # (the tail launch carries the column-sum jobs in its argument table: fewer problems fit beside them)
            items = self.items[lo: lo + (lib.etm_grouped_dw_tail_max_problems() if tail and lo == 0 else cap)]
            dims = _c_ints([v for it in items for v in it[3:8]])
            args = (_c_ptrs([_ptr(it[0]) + 4 * it[8] for it in items]), _c_ptrs([it[1] for it in items]), _c_ptrs([it[2] for it in items]), dims,
                    len(items), self.N)
            if tail and lo == 0:
                _lib.check(lib.etm_grouped_dw_tail(*args, *_colsum_args(self.colsums), _stream()), "etm_grouped_dw_tail")
            else:
                _lib.check(lib.etm_grouped_dw(*args, _stream()), "etm_grouped_dw")
            lo += len(items)
        if self.items:
            DeferredDw.last_flops = float(sum(2.0 * self.N * it[3] * it[4] for it in self.items))
        self.items, self.colsums, self.conv_wgrads = [], [], []

    def pack(self, params, views, grads):
        """After backward: the gradients ``grads`` of ``params`` (their ``.grad`` or torch.autograd.grad's outputs; None: parameter
        outside the graph) into their arena ``views``.  A parameter in ``written`` is there already -- a refused second use is added
        to it; every other one is copied by ONE multi-tensor launch."""
        dst, src = [], []
        for p, v, g in zip(params, views, grads):
            if p.data_ptr() in self.written:
                if g is not None:
                    v.add_(g)
                continue
            dst.append(v)
            src.append(g if g is not None else torch.zeros_like(v))
        if dst:
            torch._foreach_copy_(dst, src)


def _c_ptrs(items):
    """ctypes void* array of the addresses of ``items`` (tensors, or addresses already)."""
    return (ctypes.c_void_p * len(items))(*[_ptr(t) if torch.is_tensor(t) else t for t in items])


def _c_ints(values):
    return (ctypes.c_int32 * len(values))(*values)


def _colsum_args(problems):
    """The arguments of etm_colsum_reduce_grouped for ``problems`` = [(partial sums, first column, rows P, columns C, row stride,
    destination)]."""
    partial, c0, P, C, ld, out = zip(*problems)
    return (_c_ptrs([_ptr(p) + 4 * c for p, c in zip(partial, c0)]), _c_ints(P), _c_ints(C), _c_ints(ld), _c_ptrs(out), len(problems))


def _colsum_reduce(problems):
    _lib.check(_lib.load().etm_colsum_reduce_grouped(*_colsum_args(problems), _stream()), "etm_colsum_reduce_grouped")


def _conv_wgrad_reduce(problems):
    """etm_conv_wgrad_reduce_grouped over ``problems`` = [(pixel slices, slice count, dw, db, Cout, C, KH, KW)]."""
    slices, count, dw, db, cout, c, kh, kw = zip(*problems)
    _lib.check(_lib.load().etm_conv_wgrad_reduce_grouped(_c_ptrs(slices), _c_ints(count), _c_ptrs(dw), _c_ptrs(db), _c_ints(cout), _c_ints(c),
                                                         _c_ints(kh), _c_ints(kw), len(problems), _stream()), "etm_conv_wgrad_reduce_grouped")


class _HeadFoldFn(torch.autograd.Function):
    """u[h] = q_h Wk_h ([N, hd] x [hd, D] per head): q [N, D], wk [D, D] -> u [H, N, D].  The batched library GEMMs read q and write
    dq through per-head strided views (batch stride hd, row stride D), so no head-major copy of q / dq is ever made."""

    @staticmethod
    def forward(ctx, q, wk, H):
        N, D = q.shape
        hd = D // H
        ctx.save_for_backward(q, wk)
        ctx.H = H
        return torch.bmm(q.view(N, H, hd).transpose(0, 1), wk.view(H, hd, D))

    @staticmethod
    def backward(ctx, du):
        q, wk = ctx.saved_tensors
        H = ctx.H
        N, D = q.shape
        hd = D // H
        du = du.contiguous()
        dq = dwk = None
        if ctx.needs_input_grad[0]:
            dq = torch.empty_like(q)
            torch.bmm(du, wk.view(H, hd, D).transpose(1, 2), out=dq.view(N, H, hd).transpose(0, 1))
        # dWk rows of head h = q_h^T du_h: H problems of the grouped launch (A = the head's columns of q, B = its plane of du)
        if ctx.needs_input_grad[1] and not DeferredDw.defer_heads(q, du, wk):
            dwk = torch.bmm(q.view(N, H, hd).permute(1, 2, 0), du).view(D, D)
        return dq, dwk, None


class _HeadUnfoldFn(torch.autograd.Function):
    """ctx[:, h] = z_h Wv_h^T ([N, D] x [D, hd] per head): z [H, N, D], wv [D, D] -> ctx [N, D], written straight into its
    [N, H * hd] layout through a strided view (no transpose copy forward or backward)."""

    @staticmethod
    def forward(ctx, z, wv, H):
        _, N, D = z.shape
        hd = D // H
        ctx.save_for_backward(z, wv)
        ctx.H = H
        out = torch.empty((N, D), dtype=z.dtype, device=z.device)
        torch.bmm(z, wv.view(H, hd, D).transpose(1, 2), out=out.view(N, H, hd).transpose(0, 1))
        return out

    @staticmethod
    def backward(ctx, g):
        z, wv = ctx.saved_tensors
        H = ctx.H
        _, N, D = z.shape
        hd = D // H
        g = g.contiguous()
        gh = g.view(N, H, hd).transpose(0, 1)                      # [H, N, hd], strided
        dz = torch.bmm(gh, wv.view(H, hd, D)) if ctx.needs_input_grad[0] else None
        dwv = None
        # dWv rows of head h = g_h^T z_h: H problems of the grouped launch
        if ctx.needs_input_grad[1] and not DeferredDw.defer_heads(g, z, wv):
            dwv = torch.bmm(gh.transpose(1, 2), z).view(D, D)
        return dz, dwv, None


def mha(q, wk, wv, spec, block, num_heads, ln_g=None, ln_b=None, pos=None, ln_eps=1e-5, impl=None):
    """Window attention of one block.  q [N,D] projected queries -> (ctx [N,D] before fc_out, attention [N,H,L])."""
    impl = _default_impl if impl is None else impl
    if impl not in ATTENTION_IMPLS:
        raise ValueError(f"attention impl must be one of {ATTENTION_IMPLS}, got {impl!r}")
    N, D = q.shape
    H = int(num_heads)
    grad = lambda t: t is not None and t.requires_grad
    backward = torch.is_grad_enabled() and any(grad(t) for t in (q, wk, wv, ln_g, ln_b, pos))
    want_ln, want_pos = backward and (grad(ln_g) or grad(ln_b)), backward and grad(pos)
    family = attention_supported(D, H, spec.L, want_ln, want_pos, backward, impl)
    if family is None:
        raise ValueError(f"window attention D={D} H={H} L={spec.L} (norm_kv gradients: {want_ln}, positional-table gradients: "
                         f"{want_pos}, backward: {backward}) is outside what the {impl} kernels support (ops.attention_supported)")
    if family == "dense":
        return _MhaFn.apply(q, wk, wv, ln_g, ln_b, pos, spec, block, num_heads, ln_eps)
    hd = D // H
    # u[h] = q_h Wk_h and ctx_h = z_h Wv_h^T: [N,hd] x [hd,D] per head (library GEMMs; autograd supplies d q, d Wk, d Wv)
    if q.is_cuda and q.is_contiguous() and wk.is_contiguous() and wv.is_contiguous():
        u = _HeadFoldFn.apply(q, wk, H)
        z, att = _WindowFn.apply(u, ln_g, ln_b, pos, spec, block, ln_eps)
        return _HeadUnfoldFn.apply(z, wv, H), att
    u = torch.bmm(q.view(N, H, hd).transpose(0, 1), wk.view(H, hd, D))
    z, att = _WindowFn.apply(u, ln_g, ln_b, pos, spec, block, ln_eps)
    ctx = torch.bmm(z, wv.view(H, hd, D).transpose(1, 2)).transpose(0, 1).reshape(N, D)
    return ctx, att


def attn_cached(q, kv_spec, block, num_heads, want_att=False):
    """Inference-only window attention over cached projections.  ``kv_spec`` addresses a cache [W, T, blocks, 2D]
    (K | V per row).  q [N, D] projected queries -> ctx [N, D] (and attention [N, H, L] if asked)."""
    lib = _lib.load()
    _need_dev(q)
    if torch.is_grad_enabled() and q.requires_grad:
        raise RuntimeError("attn_cached is the rollout (no-grad) path; training uses ops.mha")
    q = _f32c(q, "q")
    N, D = q.shape
    L, H = kv_spec.L, int(num_heads)
    ctx = torch.empty((N, D), dtype=torch.float32, device=q.device)
    att = torch.empty((N, H, L), dtype=torch.float32, device=q.device) if want_att else None
    rc = lib.etm_attn_cached(kv_spec.block_ptr(block), kv_spec.ep_stride, kv_spec.row_stride, _ptr(kv_spec.ep), _ptr(kv_spec.win),
                             _ptr(kv_spec.mask), _ptr(q), _ptr(ctx), _ptr(att), N, L, D, H, _stream())
    _lib.check(rc, "etm_attn_cached")
    return ctx, att


def reset_rows(dst, init, step):
    """dst[w] = init for every w with step[w] == 0 (dst [W, ...], init [...], step [W] int64), in place."""
    lib = _lib.load()
    _need_dev(dst, init, step)
    if not dst.is_contiguous() or not init.is_contiguous() or step.dtype != torch.int64:
        raise TypeError("reset_rows needs contiguous float32 tensors and an int64 step vector")
    _lib.check(lib.etm_reset_rows(_ptr(dst), _ptr(init), _ptr(step), dst.shape[0], init.numel(), _stream()), "etm_reset_rows")
    return dst


def rollout_window(step, mask_table, index_table, t_dev, mask_t, win_t, st_mask, st_idx, t_row=None, reset=None, w_off=0,
                   latch=None):
    """Window-table lookup of one rollout step + staging (all outputs preallocated, in place).  Optional riders of the same
    launch: ``t_row`` (int64 scalar tensor) receives the staging row t, ``reset = (cache [W, ...], init [...])`` performs
    ``reset_rows(cache, init, step)``, ``latch = (ss [2, W], copy [2, W])`` copies the uploaded (episode step, slot) block --
    ``step`` must be ``ss[0]`` -- into the buffer the tail of the step indexes.  Worker groups: ``mask_t`` / ``win_t`` / ``step`` (and the cache) cover the W workers of
    the group, the staging arrays ``st_mask`` / ``st_idx`` [S, W_total, L] all of them; ``w_off`` is the group's first worker."""
    lib = _lib.load()
    W, L = win_t.shape
    stage_w = st_idx.shape[1]
    rdst = rinit = None
    relems = 0
    if reset is not None:
        rdst, rinit = reset
        if not rdst.is_contiguous() or not rinit.is_contiguous() or rdst.shape[0] != W:
            raise TypeError("reset needs a contiguous cache [W, ...] and a contiguous initial row")
        relems = rinit.numel()
    lat = None
    if latch is not None:
        ss, lat = latch
        if (ss.shape != (2, W) or lat.shape != (2, W) or not ss.is_contiguous() or not lat.is_contiguous()
                or ss.dtype != torch.int64 or lat.dtype != torch.int64 or step.data_ptr() != ss.data_ptr()):
            raise TypeError("latch needs contiguous int64 [2, W] blocks and step = ss[0]")
    _lib.check(lib.etm_rollout_window(_ptr(step), _ptr(mask_table), _ptr(index_table), _ptr(t_dev), _ptr(mask_t), _ptr(win_t),
                                      st_mask.data_ptr() + w_off * L * st_mask.element_size(),
                                      st_idx.data_ptr() + w_off * L * st_idx.element_size(), _ptr(t_row), _ptr(lat), _ptr(rdst), _ptr(rinit),
                                      relems, W, L, stage_w, _stream()), "etm_rollout_window")


def _branch_sizes(branches):
    """Branch sizes of a MultiDiscrete policy as a tuple, or None for a single branch (``branches``: None, an int or a sequence)."""
    if branches is None or isinstance(branches, int):
        return None
    sizes = tuple(int(a) for a in branches)
    return sizes if len(sizes) > 1 else None


def _branch_table(sizes):
    return (ctypes.c_int32 * len(sizes))(*sizes), len(sizes)


from environments import MAX_MASKED_ACTIONS      # noqa: E402  (columns of the policy head that a 64-bit action-mask word describes)


def _mask_words(action_mask, rows, total, what, device=True):
    """The int64 word array of an ``action_mask=`` argument ([rows]; bit j = column j of the ``total`` concatenated logits is
    allowed) for the *_masked entries; ``device``: it must live on the device (else pinned host memory is fine too)."""
    if action_mask.dtype != torch.int64 or action_mask.dim() != 1 or action_mask.shape[0] != rows or not action_mask.is_contiguous():
        raise ValueError(f"{what}: action_mask must be a contiguous int64 [{rows}] word array, got {tuple(action_mask.shape)} {action_mask.dtype}")
    if total > MAX_MASKED_ACTIONS:
        raise ValueError(f"{what}: action masks describe at most {MAX_MASKED_ACTIONS} actions (all branches together), not {total}")
    if device:
        _need_dev(action_mask)
    elif not (action_mask.is_cuda or action_mask.is_pinned()):
        raise ValueError(f"{what}: action_mask must be in device or pinned host memory")
    return action_mask


def _box_bounds(low, high, A):
    """HOST float arrays of the A bounds of a Box (None: unbounded on that side) for the kernels' launch-time bound table."""
    import numpy as np
    arr = lambda b: None if b is None else (ctypes.c_float * A)(*[float(x) for x in np.broadcast_to(np.asarray(b, dtype=np.float32), (A,))])
    return arr(low), arr(high)


@dataclasses.dataclass(frozen=True, eq=False)
class _DrawCall:
    """The draw at the end of a rollout step -- sample the action, stage the step's rows -- as the 24 etm_rollout_sample* / _policy* /
    _trxl* entries take it; ``_draw_call`` makes it and validates it once.  The variant of the C entry follows from what is set:
    ``box`` -> *_gaussian (``st_means`` on top -> *_gaussian_means); else ``st_logps`` -> *_branched_logps (the mask optional),
    ``action_mask`` alone -> *_branched_masked, ``sizes`` alone -> *_branched, nothing -> the single-branch entry."""
    W: int
    A: int                              # columns of the policy head: all branches' actions, or a Box's dimensions
    draws: torch.Tensor                 # the pre-drawn uniforms [S, W_total(, B)], or a Box's normals [S, W_total, A]
    forced: torch.Tensor                # (optional) the table of forced actions, shaped like ``draws``
    t_dev: torch.Tensor
    actions: torch.Tensor
    st_actions: torch.Tensor
    st_logp: torch.Tensor
    st_values: torch.Tensor
    w_off: int = 0                      # the group's first worker: where its slice of the [S, W_total, ...] tables starts
    sizes: tuple = None                 # categorical: the branch table (a Discrete policy under a mask or with st_logps is one branch)
    box: tuple = None                   # Box: (log_std, low, high)
    action_mask: torch.Tensor = None
    st_logps: torch.Tensor = None
    st_means: torch.Tensor = None

    @property
    def suffix(self):
        """Behind etm_rollout_sample / _policy / _trxl / _trxl_group -- the scheme lib.py derives the signatures by."""
        if self.box is not None:
            return "_gaussian" + ("_means" if self.st_means is not None else "")
        return "_branched" + ("_logps" if self.st_logps is not None else "_masked" if self.action_mask is not None else "") if self.sizes else ""

    @property
    def cols(self):
        """Entries per (step, worker) of ``draws`` / ``forced`` / ``st_actions``: a Box's dimensions, or one per branch."""
        return self.A if self.box is not None else len(self.sizes) if self.sizes else 1

    def _at(self, table, cols):
        return None if table is None else table.data_ptr() + self.w_off * cols * table.element_size()

    def draw_args(self):
        """(log_std,) draws, forced, t_dev, actions, st_actions, st_logp, st_values -- the tables from the group's first worker on.
        (A categorical policy stages one log-prob per branch, a Box policy the joint one.)"""
        lead = [] if self.box is None else [_ptr(self.box[0])]
        return lead + [self._at(self.draws, self.cols), self._at(self.forced, self.cols), _ptr(self.t_dev), _ptr(self.actions),
                       self._at(self.st_actions, self.cols), self._at(self.st_logp, 1 if self.box is not None else self.cols),
                       self._at(self.st_values, 1)]

    @property
    def a_arg(self):
        """The entries with a branch table take no A."""
        return [] if self.sizes else [self.A]

    @property
    def bounds(self):
        return [] if self.box is None else list(_box_bounds(self.box[1], self.box[2], self.A))

    def tail(self):
        """The arguments behind the shape integers (behind ``stage_W``, where there is one), in the order of ``suffix``."""
        if self.box is not None:
            return [] if self.st_means is None else [self._at(self.st_means, self.A)]
        t = list(_branch_table(self.sizes)) if self.sizes else []
        if self.action_mask is not None or self.st_logps is not None:
            t.append(_ptr(self.action_mask))
        return t + ([] if self.st_logps is None else [self._at(self.st_logps, self.A)])


def _draw_call(what, W, A, tables, w_off=0, branches=None, box=None, action_mask=None, st_logps=None, st_means=None):
    """The record of the draw of the op ``what`` over ``W`` workers and ``A`` policy-head columns, its operands checked.  ``tables``:
    (draws, forced, t_dev, actions, st_actions, st_logp, st_values), the first seven fields of the record."""
    draws, forced, _, actions, st_actions, _, st_values = tables
    if st_means is not None and box is None:
        raise ValueError(f"{what}: st_means belongs to a Box policy")
    if st_logps is not None and box is not None:
        raise ValueError(f"{what}: st_logps belongs to a categorical policy")
    if action_mask is not None and box is not None:
        raise ValueError(f"{what}: a Box policy has no action mask")
    sizes = None
    if box is None:
        sizes = _branch_sizes(branches)
        if sizes is None and (action_mask is not None or st_logps is not None):
            sizes = (int(A),)              # the masked / logps entries take a Discrete policy as one branch
    c = _DrawCall(W, A, *tables, w_off, sizes, box, action_mask, st_logps, st_means)
    if sizes is not None and sum(sizes) != A:
        raise ValueError(f"{what}: branches {sizes} do not add up to the {A} " + ("logit columns" if what == "rollout_sample"
                                                                                  else "rows of the policy head"))
    if st_logps is not None:
        # next to the other staging tables: float32 [S, W_total, A] (A = all branches' columns together), contiguous, on their device
        if (st_logps.dtype != torch.float32 or tuple(st_logps.shape) != (*st_values.shape[:2], A) or not st_logps.is_contiguous()
                or st_logps.device != st_values.device):
            raise ValueError(f"st_logps: need a contiguous float32 [{st_values.shape[0]}, {st_values.shape[1]}, {A}] table on the staging "
                             f"tables' device, got {tuple(st_logps.shape)} {st_logps.dtype}")
    if action_mask is not None:
        _mask_words(action_mask, W, A, what, device=False)
    if box is not None:
        # the float tables of a Box draw hold A entries per (step, worker): the kernels index them so
        for name, t in (("normals", draws), ("forced", forced), ("st_actions", st_actions)):
            if t is not None and (t.dim() != 3 or t.shape[2] != A or t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"{name}: need a contiguous float32 [S, W, {A}] table, got {tuple(t.shape)} {t.dtype}")
        if actions.dtype != torch.float32 or tuple(actions.shape) != (W, A) or not actions.is_contiguous():
            raise ValueError(f"actions: need a contiguous float32 [{W}, {A}] tensor, got {tuple(actions.shape)} {actions.dtype}")
        if box[0].numel() != A:
            raise ValueError(f"log_std: need {A} entries, got {box[0].numel()}")
    if st_means is not None:
        # next to st_actions: same shape, float32, contiguous
        if (st_means.dtype != torch.float32 or st_means.shape != st_actions.shape or not st_means.is_contiguous()
                or st_means.device != st_actions.device):
            raise ValueError(f"st_means: need a contiguous float32 table of st_actions' shape {tuple(st_actions.shape)} on its device, "
                             f"got {tuple(st_means.shape)} {st_means.dtype}")
    return c


_policy_sync = {}


def _hand_over(host_actions, host_flag, t_dev):
    """host_actions, host_flag (pinned, optional) and the arrival counter of the launch's workgroups, one per step counter."""
    sync = _policy_sync.get(t_dev.data_ptr())
    if sync is None:
        sync = _policy_sync[t_dev.data_ptr()] = torch.zeros(1, dtype=torch.int32, device=t_dev.device)
    return [_ptr(host_actions), _ptr(host_flag), _ptr(sync)]


def _launch_draw(stem, call, *args):
    name = "etm_rollout_" + stem + call.suffix
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def _sample(head, value, name, tables, **policy):
    """The sampling launch on the policy head's outputs ``head`` [W, A]: the logits, or a Box policy's means."""
    W, A = head.shape
    call = _draw_call("rollout_sample", W, A, tables, **policy)
    head, value = _f32c(head, name), _f32c(value, "value")
    _launch_draw("sample", call, _ptr(head), _ptr(value), *call.draw_args(), *call.bounds, W, *call.a_arg, *call.tail())


def rollout_sample(logits, value, uniforms, forced, t_dev, actions, st_actions, st_logp, st_values, branches=None, action_mask=None,
                   st_logps=None):
    """Categorical sampling + staging of one rollout step (in place; increments t_dev).  ``forced`` (optional): time-major int64
    table [S, W]; entries >= 0 replace the sample of that (step, worker).  ``branches`` (optional, MultiDiscrete): the branch sizes;
    ``logits`` [W, sum] holds the branches' logits side by side, every branch is sampled on its own segment with its own uniform, and
    ``uniforms`` / ``forced`` / ``st_actions`` / ``st_logp`` are [S, W, B], ``actions`` [W, B] (etm_rollout_sample_branched).
    ``action_mask`` (optional): int64 [W], the workers' invalid-action words of this step (bit j = logit column j is allowed; no
    branch empty): every branch is drawn over its valid actions only (etm_rollout_sample_branched_masked).
    ``st_logps`` (optional, float32 [S, W, sum]): every column's log-prob of the row is staged too -- the policy's distribution,
    sampled, greedy or forced action alike; -inf at a masked-out column (etm_rollout_sample_branched_logps, masks or not); None is
    exactly the call without."""
    _sample(logits, value, "logits", (uniforms, forced, t_dev, actions, st_actions, st_logp, st_values), branches=branches,
            action_mask=action_mask, st_logps=st_logps)


def rollout_sample_gaussian(mean, value, log_std, normals, forced, t_dev, actions, st_actions, st_logp, st_values, low=None, high=None,
                            st_means=None):
    """Gaussian sampling + staging of one rollout step of a Box policy (in place; increments t_dev), etm_rollout_sample_gaussian:
    x = mean + exp(log_std) normals[t] (or ``forced[t]`` where it is not NaN), ``st_actions`` [S, W, A] = x, ``st_logp`` [S, W(, 1)]
    = log p(x), ``actions`` [W, A] = clip(x, low, high).  ``st_means`` (optional, float32 [S, W, A]): the means are staged too,
    forced action or not (etm_rollout_sample_gaussian_means); None is exactly the call without."""
    _sample(mean, value, "mean", (normals, forced, t_dev, actions, st_actions, st_logp, st_values), box=(log_std, low, high), st_means=st_means)


def _policy(h2, name, policy_head, value_head, tables, host_actions, host_flag, h_bias, w_off, **policy):
    """The heads + sampling launch on the hidden heads' outputs ``h2`` [W, 2 hid].  Worker groups: h2 / actions / forced /
    host_actions cover this group's W workers; the draws and the staging arrays are [S, W_total(, B)] and are addressed from the
    group's first worker ``w_off``."""
    W, A = h2.shape[0], policy_head.weight.shape[0]
    call = _draw_call("rollout_policy", W, A, tables, w_off, **policy)
    h2 = _f32c(h2, name)
    _launch_draw("policy", call, _ptr(h2), _ptr(h_bias), _ptr(policy_head.weight), _ptr(policy_head.bias), _ptr(value_head.weight),
                 _ptr(value_head.bias), *call.draw_args(), *_hand_over(host_actions, host_flag, call.t_dev), *call.bounds, W, *call.a_arg,
                 h2.shape[1] // 2, call.st_values.shape[1], *call.tail())


def rollout_policy(h2, policy_head, value_head, uniforms, forced, t_dev, actions, st_actions, st_logp, st_values,
                   host_actions=None, host_flag=None, h_bias=None, w_off=0, branches=None, action_mask=None, st_logps=None):
    """``rollout_heads`` + ``rollout_sample`` in one launch; ``st_logps``: as in ``rollout_sample`` ([S, W_total, sum], this group's
    slice taken as for ``st_actions``; etm_rollout_policy_branched_logps); ``host_actions`` / ``host_flag``: pinned int64 tensors that receive
    the actions and then the incremented step counter (the host spins on the flag).  ``forced`` (optional): time-major int64 table
    [S, W_total]; entries >= 0 replace the sample of that (step, worker).  ``branches`` (optional, MultiDiscrete): the branch sizes;
    ``policy_head`` is then the branches' heads concatenated ([sum, hid]) and the tables are as in ``rollout_sample``.
    ``action_mask`` (optional): int64 [W] words of THIS group's workers, device or pinned host memory (read in place), as in
    ``rollout_sample`` (etm_rollout_policy_branched_masked)."""
    _policy(h2, "h", policy_head, value_head, (uniforms, forced, t_dev, actions, st_actions, st_logp, st_values), host_actions, host_flag,
            h_bias, w_off, branches=branches, action_mask=action_mask, st_logps=st_logps)


def rollout_policy_gaussian(h2, mean_head, value_head, log_std, normals, forced, t_dev, actions, st_actions, st_logp, st_values,
                            low=None, high=None, host_actions=None, host_flag=None, h_bias=None, w_off=0, st_means=None):
    """``rollout_policy`` for a Box policy (etm_rollout_policy_gaussian): the heads, the draw of ``rollout_sample_gaussian`` and the
    hand-over of the clipped float actions (``host_actions``: pinned float32 [W, A]) in one launch.  ``st_means``: as in
    ``rollout_sample_gaussian`` ([S, W_total, A], this group's slice taken as for ``st_actions``; etm_rollout_policy_gaussian_means)."""
    _policy(h2, "h2", mean_head, value_head, (normals, forced, t_dev, actions, st_actions, st_logp, st_values), host_actions, host_flag,
            h_bias, w_off, box=(log_std, low, high), st_means=st_means)


def _supported_entry(stem, A, gaussian):
    """The *_supported entry of a policy kind and its action arguments: A dimensions of a Box policy, the number of actions, or the
    branch table of a MultiDiscrete policy."""
    lib = _lib.load()
    if gaussian:
        return getattr(lib, stem + "_gaussian"), (int(A),)
    sizes = _branch_sizes(A)
    if sizes is None:
        return getattr(lib, stem), (A if isinstance(A, int) else int(tuple(A)[0]),)
    return getattr(lib, stem + "_branched"), _branch_table(sizes)


def rollout_trxl_group_ok(fused_group, W, L, hid, A, gaussian=False):
    """Does the group form of the step kernel (etm_rollout_trxl_group, csrc/rollout_group.hip) take a worker group of W workers of
    this model?  ``fused_group``: ``ActorCriticModel._rfg`` (None: the model has no group packings).  ``A``: the number of actions,
    or the branch sizes of a MultiDiscrete policy; ``gaussian``: A dimensions of a Box policy."""
    if fused_group is None:
        return False
    entry, a = _supported_entry("etm_rollout_trxl_group_supported", A, gaussian)
    return bool(entry(fused_group["D"], fused_group["H"], L, hid, *a, fused_group["nb"], W, fused_group["gtrxl"]))


def rollout_trxl_scratch(W, D, H, nb, device, group=False):
    """Zeroed scratch of one worker group for ``rollout_trxl`` (launch counter, error word, exchange slots); ``group``: for the
    group form of the kernel."""
    lib = _lib.load()
    nbytes = lib.etm_rollout_trxl_group_scratch_bytes(nb) if group else lib.etm_rollout_trxl_scratch_bytes(W, D, H, nb)
    return torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=device)


def rollout_trxl_error(scratch):
    """Non-zero if a team member of the last launches timed out waiting for a partner (device scalar; no synchronisation)."""
    return scratch[1]


def rollout_trxl_clear_error(scratch):
    """Reset the error word of the step kernel's scratch area (after the caller has dealt with a reported time-out)."""
    scratch[1].zero_()


def rollout_trxl_supported(D, H, L, hid, A, nb, gaussian=False):
    """Does ``rollout_trxl`` handle these shapes (etm_rollout_trxl_supported)?  ``A``: the number of actions, or the branch sizes
    of a MultiDiscrete policy (etm_rollout_trxl_supported_branched); ``gaussian``: A dimensions of a Box policy
    (etm_rollout_trxl_supported_gaussian)."""
    entry, a = _supported_entry("etm_rollout_trxl_supported", A, gaussian)
    return bool(entry(D, H, L, hid, *a, nb))


def rollout_trxl(h_in, fused, kv, win_t, mask_t, items, policy_head, value_head, uniforms, forced, t_dev, actions, st_actions, st_logp,
                 st_values, scratch, host_actions=None, host_flag=None, w_off=0, tail=None, h_bias=None, window=None, branches=None, box=None,
                 action_mask=None, st_means=None, st_logps=None):
    """Transformer + hidden / output heads + sampling of one rollout step of a worker group in one launch (etm_rollout_trxl).
    ``fused``: the transposed fixed-address weight copies of ``ActorCriticModel.refresh_rollout_weights`` (dict with the host
    pointer table ``blocks``; with the group packings, ``ActorCriticModel._rfg`` with "group": True, it selects the group form of the
    kernel: same arguments); ``kv`` the group's K | V cache [W, T, blocks, 2D]; ``scratch`` from ``rollout_trxl_scratch``; the
    staging arguments as in ``rollout_policy``.  ``window`` = (ss, mask_table, index_table, st_mask, st_idx, latch, t_row, kv_init):
    the launch does the step's window lookup (and the cache reset of workers at episode step 0) itself -- no ``rollout_window``
    in front of it.  ``tail`` = (wkv [blocks, D, 2D], pos [T, D] or None, step_l [W], slot_l [W],
    bank [slots, T, blocks, D]): after the action hand-over the same launch writes the new memory items into
    ``bank[slot_l, step_l]`` and their K | V projection into ``kv[w, step_l]``.  ``branches`` (optional, MultiDiscrete): as in
    ``rollout_policy`` (etm_rollout_trxl_branched / etm_rollout_trxl_group_branched).  ``box`` (optional, Box policy): (log_std, low,
    high); ``policy_head`` is then the mean head, ``uniforms`` the normals and ``forced`` the NaN-or-action table, both float
    [S, W_total, A], ``actions`` / ``st_actions`` / ``host_actions`` float (etm_rollout_trxl_gaussian / _group_gaussian).
    ``action_mask`` (optional, categorical policies): int64 [W] words of this group's workers, device or pinned host memory (read in
    place at the start of the launch), as in ``rollout_sample`` (etm_rollout_trxl_branched_masked / _group_branched_masked).
    ``st_means`` (optional, Box policy only): the means' staging table as in ``rollout_policy_gaussian``
    (etm_rollout_trxl_gaussian_means / _group_gaussian_means).
    ``st_logps`` (optional, categorical policies only): the log-probs' staging table as in ``rollout_policy``
    (etm_rollout_trxl_branched_logps / _group_branched_logps, masks or not)."""
    h_splits = 0 if h_bias is None else h_in.shape[0]          # with h_bias, h_in = [splits, W, D] slice sums of rollout_hidden_partial
    W, D = h_in.shape[-2:]
    L = win_t.shape[1]
    A, hid = policy_head.weight.shape
    call = _draw_call("rollout_trxl", W, A, (uniforms, forced, t_dev, actions, st_actions, st_logp, st_values), w_off, branches, box,
                      action_mask, st_logps, st_means)
    h_in = _f32c(h_in, "h_in")
    w_args = [0] * 11
    if window is not None:        # (ss [2, W], mask_table, index_table, st_mask, st_idx, latch [2, W], t_row, kv_init or None)
        ss, mask_table, index_table, st_mask, st_idx, latch, t_row, kv_init = window
        w_args = [_ptr(ss), _ptr(mask_table), _ptr(index_table), st_mask.data_ptr() + w_off * L * st_mask.element_size(),
                  st_idx.data_ptr() + w_off * L * st_idx.element_size(), _ptr(latch), _ptr(t_row), _ptr(mask_t), _ptr(win_t),
                  _ptr(kv_init), index_table.shape[0]]
    t_args = [0] * 8
    if tail is not None:
        wkv, pos, step_l, slot_l, bank = tail
        if not (wkv.is_contiguous() and bank.stride(3) == 1 and (pos is None or pos.is_contiguous())):
            raise ValueError("rollout_trxl tail: wkv / pos contiguous and a bank with contiguous feature rows expected")
        # bank [slots, T, blocks, D] by STRIDES: the episode bank is block-major in memory (buffer.py), upstream's layout as a view
        t_args = [_ptr(wkv), _ptr(pos), _ptr(step_l), _ptr(slot_l), _ptr(bank), bank.stride(0), bank.stride(1), bank.stride(2)]
    _launch_draw("trxl_group" if fused.get("group") else "trxl", call,
                 _ptr(h_in), _ptr(fused["emb_t"]), _ptr(fused["emb_b"]), fused["blocks"], fused["nb"], _ptr(kv), kv.stride(0), kv.stride(1),
                 _ptr(win_t), _ptr(mask_t), _ptr(items), _ptr(fused["heads_t"]), _ptr(fused["heads_b"]), _ptr(policy_head.weight),
                 _ptr(policy_head.bias), _ptr(value_head.weight), _ptr(value_head.bias), *call.draw_args(),
                 *_hand_over(host_actions, host_flag, t_dev), float(fused["eps"]), _ptr(scratch), scratch.numel() * 8, *t_args, _ptr(h_bias),
                 h_splits, *w_args, int(fused.get("pre_ln", 0)), int(fused.get("gtrxl", 0)), W, D, fused["H"], L, hid,
                 *call.a_arg, st_values.shape[1], *call.bounds, *call.tail())


def gather_rows(fields, idx):
    """``[t.index_select(0, idx) for t in fields]`` in one launch (etm_gather_rows): the per-sample fields of a minibatch.
    Tensors whose rows are not a multiple of 4 bytes (or not contiguous) go through index_select."""
    lib = _lib.load()
    n = idx.numel()
    outs = [None] * len(fields)
    sel = []
    for k, t in enumerate(fields):
        row = t[0].numel() * t.element_size() if t.shape[0] > 0 else 0
        if t.is_contiguous() and 0 < row <= 4096 and row % 4 == 0 and t.shape[0] == fields[0].shape[0] and len(sel) < 16:
            outs[k] = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            sel.append((k, row))
        else:
            outs[k] = t.index_select(0, idx)
    if sel:
        m = len(sel)
        src = (ctypes.c_void_p * m)(*[fields[k].data_ptr() for k, _ in sel])
        dst = (ctypes.c_void_p * m)(*[outs[k].data_ptr() for k, _ in sel])
        rb = (ctypes.c_int64 * m)(*[r for _, r in sel])
        _lib.check(lib.etm_gather_rows(src, dst, rb, m, _ptr(idx), n, fields[sel[0][0]].shape[0], _stream()), "etm_gather_rows")
    return outs


def step_head(fields, idx_table, counter, idx_out=None, adv_src=None):
    """Head of a minibatch step in one launch (etm_step_head).  idx = row ``counter[0] % rows`` of ``idx_table`` [rows, n] (int64;
    ``counter`` None: row 0).  Returns (``gather_rows(fields, idx)``, ``adv_stats(adv_src[idx])`` or None when ``adv_src`` is None)
    and writes idx into ``idx_out`` [n] if given.  n must be below the split of ``adv_stats`` when ``adv_src`` is given."""
    lib = _lib.load()
    rows, n = idx_table.shape
    if idx_table.dtype != torch.int64 or not idx_table.is_contiguous() or (counter is not None and counter.dtype != torch.int64):
        raise TypeError("step_head: the index table and the counter must be contiguous int64 tensors")
    src_rows = fields[0].shape[0] if fields else adv_src.shape[0]
    outs, sel = [None] * len(fields), []
    for k, t in enumerate(fields):          # (the rule of gather_rows: other tensors go through index_select on idx_out below)
        row = t[0].numel() * t.element_size() if t.shape[0] > 0 else 0
        if t.is_contiguous() and 0 < row <= 4096 and row % 4 == 0 and t.shape[0] == src_rows and len(sel) < 16:
            outs[k] = torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)
            sel.append((k, row))
        elif idx_out is None:
            raise ValueError("step_head: a field outside the gather launch needs idx_out")
    stats = None
    if adv_src is not None:
        if adv_src.dtype != torch.float32 or not adv_src.is_contiguous() or adv_src.numel() != src_rows or lib.etm_adv_stats_workspace_bytes(n) > 0:
            raise ValueError("step_head: advantages outside the one-workgroup statistics kernel")
        stats = torch.empty(3, dtype=torch.float32, device=adv_src.device)
    m = len(sel)
    src = (ctypes.c_void_p * max(m, 1))(*[fields[k].data_ptr() for k, _ in sel])
    dst = (ctypes.c_void_p * max(m, 1))(*[outs[k].data_ptr() for k, _ in sel])
    rb = (ctypes.c_int64 * max(m, 1))(*[r for _, r in sel])
    _lib.check(lib.etm_step_head(src, dst, rb, m, _ptr(idx_table), rows, _ptr(counter) if counter is not None else None, n, src_rows,
                                 _ptr(idx_out) if idx_out is not None else None, _ptr(adv_src) if adv_src is not None else None,
                                 _ptr(stats) if stats is not None else None, _stream()), "etm_step_head")
    for k, t in enumerate(fields):
        if outs[k] is None:
            outs[k] = t.index_select(0, idx_out)
    return outs, stats


def rollout_hidden_partial(x, wt, out=None):
    """K-slice partial sums of ``x [W, F] @ wt [F, D]`` (etm_rollout_hidden_partial): [splits, W, D]; the consumer
    (``rollout_trxl(h_bias=...)``) adds the slices, the bias and the ReLU."""
    lib = _lib.load()
    x = _f32c(x, "features")
    W, F = x.shape
    D = wt.shape[1]
    splits = lib.etm_rollout_hidden_splits(F)
    if splits <= 0:
        raise ValueError(f"rollout_hidden_partial: unsupported feature size {F}")
    if out is None:
        out = torch.empty((splits, W, D), dtype=torch.float32, device=x.device)
    _lib.check(lib.etm_rollout_hidden_partial(_ptr(x), _ptr(wt), _ptr(out), W, F, D, _stream()), "etm_rollout_hidden_partial")
    return out


def rollout_conv3_hidden_supported(conv3, hi, wi, d):
    return bool(_lib.load().etm_rollout_conv3_hidden_supported(conv3.in_channels, hi, wi, conv3.out_channels, conv3.kernel_size[0],
                                                               conv3.kernel_size[1], conv3.stride[0], d))


def rollout_conv3_hidden(x2, w3k, b3, hid_t, out=None):
    """Last encoder layer + lin_hidden's partial sums of a rollout step in one launch (etm_rollout_conv3_hidden): ``x2`` [W, Hi, Wi, 64]
    NHWC, ``w3k`` [576, 64], ``hid_t`` [64 * Ho * Wo, D] -> [Ho * Wo, W, D] (``rollout_trxl(h_bias=...)`` adds the rows)."""
    lib = _lib.load()
    x2 = _f32c(x2, "x2")
    W, hi, wi, _ = x2.shape
    D = hid_t.shape[1]
    npix = (hi - 2) * (wi - 2)
    if out is None:
        out = torch.empty((npix, W, D), dtype=torch.float32, device=x2.device)
    _lib.check(lib.etm_rollout_conv3_hidden(_ptr(x2), _ptr(w3k), _ptr(b3), _ptr(hid_t), _ptr(out), W, hi, wi, D, _stream()),
               "etm_rollout_conv3_hidden")
    return out


def rollout_heads(h2, branch, value_head):
    """logits [W,A] and value [W] from h2 = [relu(lin_policy(h)) | relu(lin_value(h))] ([W, 2*hid]); no-grad path."""
    lib = _lib.load()
    h2 = _f32c(h2, "h2")
    W, hid = h2.shape[0], h2.shape[1] // 2
    A = branch.weight.shape[0]
    logits = torch.empty((W, A), dtype=torch.float32, device=h2.device)
    value = torch.empty((W,), dtype=torch.float32, device=h2.device)
    _lib.check(lib.etm_rollout_heads(_ptr(h2), _ptr(branch.weight), _ptr(branch.bias), _ptr(value_head.weight), _ptr(value_head.bias),
                                     _ptr(logits), _ptr(value), W, A, hid, _stream()), "etm_rollout_heads")
    return logits, value


def gru_gate(x, y, wy, ux, ug, bg):
    """GTrXL gate on the no-grad path: wy = [Wr;Wz;Wg] ([3D,D]), ux = [Ur;Uz] ([2D,D]), ug [D,D], bg [D].
    Three library GEMMs + two elementwise kernels."""
    lib = _lib.load()
    x, y = _f32c(x, "x"), _f32c(y, "y")
    N, D = x.shape
    a = torch.nn.functional.linear(y, wy)
    b = torch.nn.functional.linear(x, ux)
    rx = torch.empty_like(x)
    z = torch.empty_like(x)
    _lib.check(lib.etm_gru_gate_rz(_ptr(a), _ptr(b), _ptr(bg), _ptr(x), _ptr(rx), _ptr(z), N, D, _stream()), "etm_gru_gate_rz")
    c = torch.nn.functional.linear(rx, ug)
    out = torch.empty_like(x)
    _lib.check(lib.etm_gru_gate_out(_ptr(a), _ptr(c), _ptr(z), _ptr(x), _ptr(out), N, D, _stream()), "etm_gru_gate_out")
    return out


def add_layernorm(a, b, norm, out=None, bias=None, relu=False):
    """LayerNorm(act(a + bias) + b) with ``norm``'s affine parameters; forward only (rollout path).  ``bias`` / ``relu`` fold
    the epilogue of the linear layer that produced ``a`` (which then runs as a plain, per-shape tuned library GEMM)."""
    lib = _lib.load()
    _need_dev(a, b)
    a, b = _f32c(a, "a"), _f32c(b, "b")
    N, D = a.shape
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise TypeError("add_layernorm: out must be a contiguous float32 tensor of the input shape")
    _lib.check(lib.etm_add_layernorm(_ptr(a), _ptr(bias), 1 if relu else 0, _ptr(b), _ptr(norm.weight), _ptr(norm.bias), float(norm.eps),
                                     _ptr(out), N, D, _stream()), "etm_add_layernorm")
    return out


class _FusedLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(act(a + bias) + res) * gamma + beta with hand-written forward and backward (csrc/block_train.hip)."""

    @staticmethod
    def forward(ctx, a, bias, res, gamma, beta, relu, eps, fork=False):
        lib = _lib.load()
        _need_dev(a, bias, res, gamma, beta)
        a, bias, res = _f32c(a, "a"), _f32c(bias, "bias"), _f32c(res, "res")
        gamma, beta = _f32c(gamma, "gamma"), _f32c(beta, "beta")
        N, D = a.shape
        need = any(ctx.needs_input_grad[:5])
        y = torch.empty_like(a)
        s = torch.empty_like(a) if need else None
        stats = torch.empty((N, 2), dtype=torch.float32, device=a.device) if need else None
        _lib.check(lib.etm_ln_train_fwd(_ptr(a), _ptr(bias), 1 if relu else 0, _ptr(res), _ptr(gamma), _ptr(beta), float(eps), _ptr(y),
                                        _ptr(s), _ptr(stats), N, D, _stream()), "etm_ln_train_fwd")
        if need:
            ctx.relu, ctx.has_bias, ctx.has_res = bool(relu), bias is not None, res is not None
            ctx.param_ptrs = (gamma.data_ptr(), beta.data_ptr(), bias.data_ptr() if bias is not None else 0)
            ctx.save_for_backward(s, stats, gamma, a if relu else None, bias if relu else None)
        ctx.fork = bool(fork)
        if fork:         # the output twice (one storage): the gradients of its two consumers arrive separately and are added on load
            ctx.set_materialize_grads(False)
            return y, y.detach()
        return y

    @staticmethod
    def backward(ctx, dy, dy2=None):
        lib = _lib.load()
        s, stats, gamma, a, bias = ctx.saved_tensors
        if dy is None:
            dy, dy2 = dy2, None
        if dy is None:
            return (None,) * 8
        dy = _f32c(dy, "dy")
        dy2 = _f32c(dy2, "dy2")
        N, D = s.shape
        ds = torch.empty_like(s)
        da = torch.empty_like(s) if ctx.relu else None
        nbytes = lib.etm_ln_train_bwd_workspace_bytes(N, D)
        d_a = da if ctx.relu else ds
        # with a collector the three column sums go to its ONE reduction launch, straight into the parameters' arena views
        g_ptr, b_ptr, bias_ptr = ctx.param_ptrs
        parts = [(0, D, g_ptr), (D, D, b_ptr)] + ([(2 * D, D, bias_ptr)] if ctx.has_bias else [])
        ws, deferred = DeferredDw.colsum_workspace(nbytes, lib.etm_ln_train_bwd_partial_rows(N), 3 * D, parts, s.device, "ln_bwd")
        sums = None if deferred else torch.empty((3, D), dtype=torch.float32, device=s.device)
        _lib.check(lib.etm_ln_train_bwd(_ptr(dy), _ptr(dy2), _ptr(s), _ptr(stats), _ptr(gamma), _ptr(a), _ptr(bias), 1 if ctx.relu else 0, _ptr(ds),
                                        _ptr(da), _ptr(sums), _ptr(ws), nbytes, N, D, _stream()), "etm_ln_train_bwd")
        d_res = ds if ctx.has_res else None
        if deferred:
            return d_a, None, d_res, None, None, None, None, None
        return d_a, (sums[2] if ctx.has_bias else None), d_res, sums[0], sums[1], None, None, None


def fused_layernorm(a, norm, bias=None, res=None, relu=False, fork=False):
    """``norm(act(a + bias) + res)`` (``norm``: an nn.LayerNorm over the last dimension of the [N, D] input) as one forward and
    one backward kernel (+ a tiny fixed-order column-sum kernel): the bias / ReLU of the linear layer that produced ``a`` and the
    residual add ride along, so that layer runs as a plain GEMM.  Training path (differentiable); the rollout uses
    ``add_layernorm``.  ``fork``: returns the result TWICE (two tensors, one storage) for its two consumers -- the next GEMM and
    the next residual branch (transformer.py:143-149, :160-170) -- so that their gradients reach the backward kernel separately
    and are added on load, not by a launch of autograd's."""
    if fork:
        return _FusedLayerNormFn.apply(a, bias, res, norm.weight, norm.bias, relu, norm.eps, True)
    return _FusedLayerNormFn.apply(a, bias, res, norm.weight, norm.bias, relu, norm.eps)


class _GruGateFn(torch.autograd.Function):
    """GTrXL gate (transformer.py:287-298): out = (1 - z) x + z tanh(Wg y + Ug (r x)), r = sigmoid(Wr y + Ur x),
    z = sigmoid(Wz y + Uz x - bg).  Three concatenated library GEMMs + two kernels forward; six GEMMs + two kernels (+ the
    column-sum kernel for d bg) backward, instead of six small GEMMs + ~10 element-wise launches forward and twice that backward."""

    @staticmethod
    def forward(ctx, x, y, wr, ur, wz, uz, wg, ug, bg, wy=None, ux=None, fork=False):
        lib = _lib.load()
        _need_dev(x, y, wr, ur, wz, uz, wg, ug, bg)
        x, y = _f32c(x, "x"), _f32c(y, "y")
        N, D = x.shape
        if wy is None or ux is None:                   # (the caller may hand the concatenations over: transformer.py:_pack_gate_weights)
            wy = torch.cat((wr, wz, wg), dim=0)        # [3D, D]
            ux = torch.cat((ur, uz), dim=0)            # [2D, D]
        A = torch.mm(y, wy.t())
        B = torch.mm(x, ux.t())
        r, z, rx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.etm_gate_train_rz(_ptr(A), _ptr(B), _ptr(bg), _ptr(x), _ptr(r), _ptr(z), _ptr(rx), N, D, _stream()), "etm_gate_train_rz")
        C = torch.mm(rx, ug.t())
        hh, out = torch.empty_like(x), torch.empty_like(x)
        _lib.check(lib.etm_gate_train_out(_ptr(A), _ptr(C), _ptr(z), _ptr(x), _ptr(hh), _ptr(out), N, D, _stream()), "etm_gate_train_out")
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, y, r, z, rx, hh, wy, ux, ug)
            ctx.gate_weights = (wr, ur, wz, uz, wg)      # (the parameters themselves: DeferredDw looks their arena views up by address)
            ctx.bg_ptr = bg.data_ptr()
        if fork:         # the output twice (one storage) for its two consumers (pre-LN blocks: the next LayerNorm and the next gate's
            ctx.set_materialize_grads(False)   # residual input): their gradients arrive separately and gate_bwd1 adds them on load
            return out, out.detach()
        return out

    @staticmethod
    def backward(ctx, dout, dout2=None):
        lib = _lib.load()
        x, y, r, z, rx, hh, wy, ux, ug = ctx.saved_tensors
        if dout is None:
            dout, dout2 = dout2, None
        if dout is None:
            return (None,) * 12
        dout = _f32c(dout, "dout")
        dout2 = _f32c(dout2, "dout2")
        N, D = x.shape
        dev = x.device
        dA = torch.empty((N, 3 * D), dtype=torch.float32, device=dev)
        dB = torch.empty((N, 2 * D), dtype=torch.float32, device=dev)
        dx1 = torch.empty_like(x)
        nbytes = lib.etm_gate_train_bwd_workspace_bytes(N, D)
        # (with a collector: d bg's second stage rides in its one reduction launch)
        ws, deferred = DeferredDw.colsum_workspace(nbytes, lib.etm_gate_train_bwd_partial_rows(N), D, [(0, D, ctx.bg_ptr)], dev, "gate_bwd")
        dbg = None if deferred else torch.empty((D,), dtype=torch.float32, device=dev)
        _lib.check(lib.etm_gate_train_bwd1(_ptr(dout), _ptr(dout2), _ptr(z), _ptr(hh), _ptr(x), _ptr(dA), _ptr(dB), _ptr(dx1), _ptr(dbg), _ptr(ws), nbytes,
                                           N, D, _stream()), "etm_gate_train_bwd1")
        dC = dA[:, 2 * D:]                              # d pre_h, a strided view (row stride 3D): GEMM operand in place
        drx = torch.mm(dC, ug)
        dx2 = torch.empty_like(x)
        _lib.check(lib.etm_gate_train_bwd2(_ptr(drx), _ptr(x), _ptr(r), _ptr(dx1), _ptr(dA), _ptr(dB), _ptr(dx2), N, D, _stream()),
                   "etm_gate_train_bwd2")
        dy = torch.mm(dA, wy)
        dx = dx2.addmm_(dB, ux)                         # (in place: the out-of-place form first copies dx2, a 3 MB device copy per gate)
        # Weight gradients.  Round 5: with a DeferredDw collector active (the trainer's backward pass) the six D x D products go to the
        # grouped fp32-MFMA launch (csrc/grouped_dw.hip) like every other dense layer's -- column blocks of dA / dB as the left
        # operands (a_col0), written straight into the arena views.  Two reasons: 24 library GEMMs fewer per minibatch step at
        # config 5, and accuracy -- the library's [3D, N] x [N, D] product walks the N samples in ONE fp32 chain (measured 2.8e-6 of
        # the tensor norm against float64 at N = 1,686: the worst tensors of the kink-free parity test were the gate matrices), the
        # grouped kernel in four chains summed pairwise (7e-7).
        wr, ur, wz, uz, wg = ctx.gate_weights
        defer = DeferredDw.defer
        took = [defer(dA, y, wr, a_col0=0), defer(dB, x, ur, a_col0=0), defer(dA, y, wz, a_col0=D),
                defer(dB, x, uz, a_col0=D), defer(dA, y, wg, a_col0=2 * D), defer(dA, rx, ug, a_col0=2 * D)]
        dwy = torch.mm(dA.t(), y) if not (took[0] and took[2] and took[4]) else None     # [3D, D] = d [Wr; Wz; Wg]
        dux = torch.mm(dB.t(), x) if not (took[1] and took[3]) else None                 # [2D, D] = d [Ur; Uz]
        pick = lambda t, full, lo: None if t else full[lo: lo + D]
        return (dx, dy, pick(took[0], dwy, 0), pick(took[1], dux, 0), pick(took[2], dwy, D), pick(took[3], dux, D),
                pick(took[4], dwy, 2 * D), None if took[5] else torch.mm(dC.t(), rx), dbg, None, None, None)


def gru_gate_train(gate, x, y, packed=None, fork=False):
    """Differentiable GTrXL gate of ``gate`` (a transformer.GRUGate) on [N, D] inputs.  ``packed``: ([Wr; Wz; Wg], [Ur; Uz]) of the
    gate's CURRENT weights when the caller has them concatenated already.  ``fork``: returns the result TWICE (two tensors, one
    storage) for its two consumers; their gradients are added by the gate's backward kernel on load instead of by an extra launch."""
    wy, ux = packed if packed is not None else (None, None)
    return _GruGateFn.apply(x, y, gate.Wr.weight, gate.Ur.weight, gate.Wz.weight, gate.Uz.weight, gate.Wg.weight, gate.Ug.weight, gate.bg, wy, ux,
                            fork)


def conv_pack_weights(weight2d):
    """[Cout, K] (K in the order that matches the input layout) -> the MFMA-fragment order etm_conv_relu reads
    (include/etm_hip.h): packed[g, t, half, col, j] = w[t * 32 + col, g * 8 + half * 4 + j]; returned as [Cout, K]."""
    Cout, K = weight2d.shape
    if Cout % 32 or K % 8:
        raise ValueError("conv_pack_weights needs Cout % 32 == 0 and K % 8 == 0")
    w = weight2d.reshape(Cout // 32, 32, K // 8, 2, 4)          # [t, col, g, half, j]
    return w.permute(2, 0, 3, 1, 4).contiguous().view(Cout, K)   # [g, t, half, col, j]


def conv_relu(x, weight2d, bias, C, H, W, KH, KW, S, in_nhwc, out_nchw, index=None, rows=None):
    """relu(conv2d(x) + bias) on the no-grad path (see etm_conv_relu).  ``weight2d``: ``conv_pack_weights`` of the [Cout, K]
    weights in the K order that matches the input layout.  With ``index`` (int64 device scalar) ``x`` is a stack [S, N, ...]
    and the layer reads x[index] -- the row is chosen on the device, so a captured graph can walk a staging array; ``rows =
    (lo, hi)`` restricts it to images lo..hi-1 of that row (a worker group).  ``x`` may be uint8 (byte k = float32(k) / 255): the NCHW
    first layer then reads the bytes itself (etm_conv_relu_u8), any other layer gets them expanded first (``bytes_to_unit``).
    Returns NHWC [N,Ho,Wo,Cout] or NCHW [N,Cout,Ho,Wo]."""
    lib = _lib.load()
    _need_dev(x, weight2d, bias, index)
    x = _obs_c(x, "x")
    u8 = x.dtype == torch.uint8
    if index is not None and (index.dtype != torch.int64 or index.numel() != 1):
        raise TypeError("conv_relu: index must be an int64 device scalar")
    if u8 and (in_nhwc or weight2d.shape[0] != 32 or W % 4 or S % 4 or KW % 8 or x.data_ptr() % 4 or (C * H * W) % 4):
        # no byte form of this layer: the (selected row of the) input as floats, then the float kernel
        x = bytes_to_unit(x, index=None if index is None else index.reshape(1))
        if index is not None:
            x = x[0, rows[0]:rows[1]] if rows is not None else x[0]
            index = rows = None
        u8 = False
    esize = 1 if u8 else 4
    stride = 0
    if index is not None:
        stride = x[0].numel()
        N = x.shape[1]
    else:
        N = x.shape[0]
    base = x.data_ptr()
    if rows is not None:          # only images [lo, hi) of every row of the stack (a worker group)
        if index is None:
            raise TypeError("conv_relu: rows needs index (stacked input)")
        lo, hi = rows
        base += lo * x[0, 0].numel() * esize
        N = hi - lo
    Cout = weight2d.shape[0]
    Ho, Wo = (H - KH) // S + 1, (W - KW) // S + 1
    shape = (N, Cout, Ho, Wo) if out_nchw else (N, Ho, Wo, Cout)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    entry, what = (lib.etm_conv_relu_u8, "etm_conv_relu_u8") if u8 else (lib.etm_conv_relu, "etm_conv_relu")
    rc = entry(base, _ptr(index), stride, _ptr(weight2d), _ptr(bias), _ptr(out), N, C, H, W, Cout, KH, KW, S,
               1 if in_nhwc else 0, 1 if out_nchw else 0, _stream())
    _lib.check(rc, what)
    return out


def conv_pack_dgrad_weights(weight, stride):
    """conv weight [Cout, C, KH, KW] -> the S*S stride-parity class blocks etm_conv_train_dgrad reads (include/etm_hip.h):
    class (py, px) packs Wd[c][(a*T + j)*Cout + co] = w[co][c][py + S a][px + S (T-1-j)], T = KH / S."""
    Cout, C, KH, KW = weight.shape
    S = int(stride)
    T = KH // S
    blocks = []
    for py in range(S):
        for px in range(S):
            sub = weight[:, :, py::S, px::S].flip(3)                   # [Cout, C, a, j]
            blocks.append(conv_pack_weights(sub.permute(1, 2, 3, 0).reshape(C, T * T * Cout)))
    return torch.stack(blocks).contiguous()


def encoder_train_supported(obs_shape, convs, batch=None, bank=None, products=None):
    """Can the hand-written training kernels run this encoder?  (model.py:40-56 geometry with 84 x 84 or similar inputs.)
    ``batch``: images per call -- the kernels index output pixels with 24 bits (N * Ho * Wo < 2^24 per layer, padded to the
    backward-data kernel's image unit of 1024) and the source with 32-bit element offsets; larger minibatches take the library path.
    ``bank``: images of the tensor an indexed call gathers from (``encoder_train(bank, index=...)``): the fp32 first layer
    addresses the whole bank with 32-bit element offsets, so a bank of 2^31 floats or more is refused unless the call runs on the
    bf16 matrix pipe (``products`` as ``encoder_train`` takes it; those kernels form a 64-bit image base)."""
    c, h, w = obs_shape
    if bank is not None and bank * h * w * c >= 2 ** 31 and not _encoder_uses_b3(h, w, [cv.weight for cv in convs], [cv.stride[0] for cv in convs], products):
        return False
    for conv in convs:
        if batch is not None:
            kh, s = conv.kernel_size[0], conv.stride[0]
            padded = (batch + 1023) // 1024 * 1024
            if (batch * h * w * c >= 2 ** 31 or batch * ((h - kh) // s + 1) * ((w - kh) // s + 1) >= 2 ** 24      # forward / backward-weight
                    or (conv is not convs[0] and padded * (h // s) * (w // s) >= 2 ** 24)):                      # backward-data
                return False
        kh, kw = conv.kernel_size
        s = conv.stride[0]
        if (kh != kw or conv.stride[0] != conv.stride[1] or conv.padding != (0, 0) or conv.dilation != (1, 1) or conv.groups != 1
                or conv.out_channels not in (32, 64) or (kw * c) % 8 or (w * c) % 4 or (s * c) % 4 or (kh * kw * c) % 32
                or h < kh or w < kw):
            return False
        if conv is not convs[0] and (kh % s or h % s or w % s or c not in (32, 64)):     # backward-data of the layers above the first
            return False
        h, w, c = (h - kh) // s + 1, (w - kw) // s + 1, conv.out_channels
    return True


_encoder_products = "bf16x3"     # default of encoder_train for callers that name none: "bf16x3" = the encoder's products on the bf16 matrix
#                                    pipe at fp32 accuracy (csrc/conv_b3.hip, round 6); "fp32" = v_mfma_f32_32x32x2_f32 (csrc/conv_train.hip and
#                                    the LDS-resident forms).  The model passes its own ``encoder_products`` with every call.


def set_encoder_products(kind):
    """Default product form of ``encoder_train`` calls that pass none ("bf16x3" / "fp32"); tools use it, the trainer does not."""
    global _encoder_products
    if kind not in ("bf16x3", "fp32"):
        raise ValueError(f"encoder_products must be 'bf16x3' or 'fp32', got {kind!r}")
    _encoder_products = kind


_B3_LAYERS = {(3, 84, 84, 32, 8, 4), (32, 20, 20, 64, 4, 2), (64, 9, 9, 64, 3, 1)}      # (C, H, W, Cout, K, S) of model.py:29-31 on 84 x 84


def _encoder_uses_b3(h, w, weights, strides, products):
    """Does ``encoder_train`` run the three layers (weights [Cout, C, K, K], strides) on h x w images on the bf16 matrix pipe
    (csrc/conv_b3*.hip)?  Only the exact layers of _B3_LAYERS.  (``_EncoderFn`` and ``encoder_train_supported`` both ask here.)"""
    if (products or _encoder_products) != "bf16x3":
        return False
    for wt, s in zip(weights, strides):
        cout, cin, kh, kw = wt.shape
        if kh != kw or (cin, h, w, cout, kh, s) not in _B3_LAYERS:
            return False
        h, w = (h - kh) // s + 1, (w - kw) // s + 1
    return True


def conv_b3_pack(weights, dgrad, strides):
    """``weights[i]`` [Cout, C, K, K] -> the three bf16 planes of its forward (``dgrad[i]`` 0) or backward-data (1) operand in
    fragment order (etm_conv_b3_pack, one launch for all entries): int16 tensors of 3 * numel."""
    lib = _lib.load()
    outs = [torch.empty(3 * w.numel(), dtype=torch.int16, device=w.device) for w in weights]
    _lib.check(lib.etm_conv_b3_pack(_c_ptrs(weights), _c_ptrs(outs), _c_ints(dgrad), _c_ints([w.shape[0] for w in weights]),
                                    _c_ints([w.shape[1] for w in weights]), _c_ints([w.shape[2] for w in weights]), _c_ints(strides), len(weights),
                                    _stream()), "etm_conv_b3_pack")
    return outs


class _EncoderFn(torch.autograd.Function):
    """The three relu(conv2d) layers of model.py:90-92 on NHWC activations: 3 forward launches; backward = 1 mask/layout kernel,
    3 weight-gradient kernels (+ their fixed-order reductions) and 2 data-gradient kernels, with bias, ReLU, ReLU masks and
    bias gradients fused in (csrc/conv_train.hip).  Returns the features NHWC-flattened [N, Ho*Wo*Cout]: the consumer permutes
    the columns of ITS weight (a 4.8 MB copy at config 3) instead of the features being transposed to upstream's (c, h, w)
    flatten order (model.py:94) and back."""

    @staticmethod
    def forward(ctx, x_nhwc, w1, b1, w2, b2, w3, b3, strides, index=None, products=None):
        lib = _lib.load()
        _need_dev(x_nhwc, w1, b1, w2, b2, w3, b3)
        x = _obs_c(x_nhwc, "obs")
        st = _stream()
        n, h, w, c = x.shape
        u8 = x.dtype == torch.uint8
        if u8 and not (_encoder_uses_b3(h, w, [w1, w2, w3], strides, products) and x.data_ptr() % 16 == 0):
            # no byte form of this first layer (fp32 products, another geometry): the batch's images as floats, then the float kernels.
            # The byte tensor is what backward keeps; it expands them again.
            ctx.u8_fallback = (x, index)
            x, index, u8 = bytes_to_unit(x, index=index), None, False
            n = x.shape[0]
        else:
            ctx.u8_fallback = None
        acts, shapes = [x], []
        x_images = n
        if index is not None:          # batch image i = x[index[i]]: the minibatch gather rides in the first layer's loads
            n = index.numel()
        # both packings of the three layers' weights in ONE launch; the backward-data ones ride in the context
        layers = ((w1, b1, strides[0]), (w2, b2, strides[1]), (w3, b3, strides[2]))
        wts = [_f32c(wt.detach(), "conv weight") for wt, _, _ in layers]
        use_b3 = _encoder_uses_b3(h, w, wts, strides, products)
        if use_b3:      # the five operands (three forward, two backward-data) split and packed in ONE launch
            packs = conv_b3_pack(wts + wts[1:], [0, 0, 0, 1, 1], [l[2] for l in layers] + [l[2] for l in layers[1:]])
            dgrad_packs = [None] + packs[3:]
        else:
            packs = [torch.empty(wt.numel(), dtype=torch.float32, device=x.device) for wt in wts]
            dgrad_packs = [None] + [torch.empty(wt.numel(), dtype=torch.float32, device=x.device) for wt in wts[1:]]
            _lib.check(lib.etm_conv_pack_weights_grouped(_c_ptrs(wts), _c_ptrs(packs), _c_ptrs(dgrad_packs), _c_ints([wt.shape[0] for wt in wts]),
                                                         _c_ints([wt.shape[1] for wt in wts]), _c_ints([wt.shape[2] for wt in wts]),
                                                         _c_ints([wt.shape[3] for wt in wts]), _c_ints([l[2] for l in layers]), 3, st),
                       "etm_conv_pack_weights_grouped")
        ctx.b3 = use_b3
        relu_bits = []      # (b3: the ReLU pattern of every layer's output, one bit per element -- what backward-data needs of it)
        for i, (wt, bs, s) in enumerate(layers):
            cout, _, kh, kw = wt.shape
            ho, wo = (h - kh) // s + 1, (w - kw) // s + 1
            y = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
            if use_b3:
                bits = torch.empty((n, ho, wo, cout // 32), dtype=torch.int32, device=x.device)
                relu_bits.append(bits)
                fwd, what = (lib.etm_conv_b3_fwd_u8, "etm_conv_b3_fwd_u8") if (u8 and i == 0) else (lib.etm_conv_b3_fwd, "etm_conv_b3_fwd")
                _lib.check(fwd(_ptr(acts[-1]), _ptr(index) if i == 0 else None, _ptr(packs[i]), _ptr(_f32c(bs.detach(), "bias")),
                               _ptr(y), _ptr(bits), n, c, h, w, cout, kh, kw, s, st), what)
            else:
                _lib.check(lib.etm_conv_train_fwd(_ptr(acts[-1]), _ptr(index) if i == 0 else None, x_images, _ptr(packs[i]),
                                                  _ptr(_f32c(bs.detach(), "bias")), _ptr(y), n, c, h, w, cout, kh, kw, s, 0, st), "etm_conv_train_fwd")
            shapes.append((c, h, w, cout, kh, kw, s, ho, wo))
            acts.append(y)
            h, w, c = ho, wo, cout
        ctx.param_ptrs = tuple(t.data_ptr() for t in (w1, b1, w2, b2, w3, b3))
        ctx.shapes = shapes
        if ctx.u8_fallback is not None:
            acts[0], index = ctx.u8_fallback      # (the expanded copy is not kept alive between the passes)
            ctx.u8_fallback = True
        ctx.save_for_backward(acts[0], acts[1], acts[2], acts[3], dgrad_packs[1], dgrad_packs[2], index,
                              *(relu_bits if use_b3 else (None, None, None)))
        return acts[3].view(n, -1)

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x0, y1, y2, y3, pd2, pd3, index, bits1, bits2, bits3 = ctx.saved_tensors
        st = _stream()
        dev = x0.device
        n = y1.shape[0]
        if ctx.u8_fallback:
            x0, index = bytes_to_unit(x0, index=index), None
        u8 = x0.dtype == torch.uint8
        g = _f32c(g, "d_features")
        c3, h3, w3_, cout3, _, _, _, ho3, wo3 = ctx.shapes[2]
        if ctx.b3:      # the last layer's ReLU backward rides in the fills of its two consumers (pattern words of y3 from the forward pass)
            dy, dy_bits = g, bits3
        else:
            dy, dy_bits = torch.empty((n, ho3, wo3, cout3), dtype=torch.float32, device=dev), None
            _lib.check(lib.etm_relu_mask(_ptr(g), _ptr(y3), _ptr(dy), dy.numel(), st), "etm_relu_mask")
        grads = [None] * 6
        inputs = (x0, y1, y2)
        dgrad_packs = (None, pd2, pd3)
        # with a collector that knows the six parameters' arena views the three slice reductions become ONE launch at its flush
        dests = DeferredDw.claim(ctx.param_ptrs)
        for i in (2, 1, 0):
            c, h, w, cout, kh, kw, s, ho, wo = ctx.shapes[i]
            K = kh * kw * c
            if ctx.b3:
                slices = lib.etm_conv_b3_wgrad_slices(n, c, h, w, cout, kh, kw, s)
                nbytes = slices * (K * cout + cout) * 4
            else:
                slices = lib.etm_conv_train_wgrad_slices(n, c, h, w, cout, kh, kw, s)
                nbytes = lib.etm_conv_train_wgrad_workspace_bytes(n, c, h, w, cout, kh, kw, s)
            if dests is not None:
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)      # (lives until the collector's flush)
                buf = None
                DeferredDw.defer_conv_wgrad(ws, slices, dests[2 * i], dests[2 * i + 1], cout, c, kh, kw)
            else:
                ws = workspace(nbytes, dev, "conv_wgrad")
                buf = torch.empty(K * cout + cout, dtype=torch.float32, device=dev)
            if ctx.b3:      # the slices on the bf16 matrix pipe (csrc/conv_b3_wgrad.hip); without a collector their reduction follows at once
                wgrad, what = (lib.etm_conv_b3_wgrad_u8, "etm_conv_b3_wgrad_u8") if (u8 and i == 0) else (lib.etm_conv_b3_wgrad, "etm_conv_b3_wgrad")
                _lib.check(wgrad(_ptr(inputs[i]), _ptr(index) if i == 0 else None, _ptr(dy), _ptr(dy_bits), _ptr(ws), nbytes, n, c, h, w,
                                 cout, kh, kw, s, st), what)
                if buf is not None:
                    _conv_wgrad_reduce([(ws, slices, buf, buf[K * cout:], cout, c, kh, kw)])
            else:
                _lib.check(lib.etm_conv_train_wgrad(_ptr(inputs[i]), _ptr(index) if i == 0 else None, _ptr(dy), _ptr(buf), _ptr(ws), nbytes, n, c, h, w,
                                                    cout, kh, kw, s, st), "etm_conv_train_wgrad")
            if buf is not None:
                grads[2 * i] = buf[: K * cout].view(cout, c, kh, kw)
                grads[2 * i + 1] = buf[K * cout:]
            if i > 0:
                dx = torch.empty((n, h, w, c), dtype=torch.float32, device=dev)
                if ctx.b3:
                    _lib.check(lib.etm_conv_b3_dgrad(_ptr(dy), _ptr(dy_bits), _ptr(dgrad_packs[i]), None, _ptr((None, bits1, bits2)[i]), _ptr(dx), n, c, h, w,
                                                     cout, kh, kw, s, st), "etm_conv_b3_dgrad")
                else:
                    _lib.check(lib.etm_conv_train_dgrad(_ptr(dy), _ptr(dgrad_packs[i]), _ptr(inputs[i]), _ptr(dx), n, c, h, w, cout, kh, kw, s, st),
                               "etm_conv_train_dgrad")
                dy, dy_bits = dx, None      # (the data gradient comes out masked: a pre-activation gradient)
        return (None, *grads, None, None, None)


def encoder_train(obs_nhwc, conv1, conv2, conv3, index=None, products=None):
    """Differentiable encoder forward on an NHWC observation batch [N, H, W, C] -- or, with ``index`` (int64 [n]), on the images
    ``obs_nhwc[index]`` without gathering them first: features [N, Ho * Wo * Cout], NHWC-flattened
    (``linear_relu_nhwc`` is the following linear layer on that column order).  Gradients flow to the
    convolution weights and biases (observations need none).  ``obs_nhwc`` may be uint8 (byte k = float32(k) / 255): on the bf16
    matrix pipe the first layer's forward and weight-gradient kernels read the bytes; with fp32 products or another geometry the
    images are expanded (``bytes_to_unit``) in front of the float kernels, in both passes."""
    if products not in (None, "bf16x3", "fp32"):
        raise ValueError(f"products must be 'bf16x3' or 'fp32', got {products!r}")
    return _EncoderFn.apply(obs_nhwc, conv1.weight, conv1.bias, conv2.weight, conv2.bias, conv3.weight, conv3.bias,
                            (conv1.stride[0], conv2.stride[0], conv3.stride[0]), index, products)


class ReplayAfterWarmup:
    """``fn()`` -- device work on fixed-address operands without host synchronisation (a weight repacking, a cache refresh: dozens of
    small launches once per update) -- run eagerly for its first ``warm`` calls and from a captured graph afterwards (round 6:
    refresh_rollout_weights 2.3 -> 0.3 ms per update at config 5).  ``after``: host-side bookkeeping that must follow every execution,
    captured or not.  A failed capture keeps the eager form for good; ``enabled`` False never captures."""

    def __init__(self, fn, device, warm=2, after=None, enabled=True, what="refresh"):
        self.fn, self.device, self.warm, self.after, self.enabled, self.what = fn, device, warm, after, enabled, what
        self.calls, self.graph, self.failed = 0, None, False

    def __call__(self):
        if self.graph is not None:
            self.graph.replay()
        else:
            self.calls += 1
            capture = (self.enabled and not self.failed and self.calls > self.warm and torch.device(self.device).type == "cuda"
                       and not torch.cuda.is_current_stream_capturing())
            if capture:
                try:
                    torch.cuda.synchronize(self.device)
                    g = torch.cuda.CUDAGraph()
                    with torch.no_grad(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                        self.fn()
                    self.graph = g
                    g.replay()
                except Exception as exc:       # noqa: BLE001
                    import sys
                    self.failed, self.graph = True, None
                    torch.cuda.synchronize(self.device)
                    print(f"[etm] {self.what} stays eager (capture failed: {exc!r})", file=sys.stderr, flush=True)
                    self.fn()
            else:
                self.fn()
        if self.after is not None:
            self.after()


def host_view(t):
    """numpy array over the memory of the contiguous float32 (or uint8: byte observation rows) device tensor ``t`` at its HOST
    address (large-BAR systems map the device's memory into the process: the pointer is the same) -- WRITE-ONLY use: host reads
    through the BAR are uncached and slow, and the device's caches know nothing of them.  Call ``host_direct_write_ok`` first."""
    import numpy as np
    if not (t.is_cuda and t.dtype in (torch.float32, torch.uint8) and t.is_contiguous()):
        raise TypeError("host_view: a contiguous float32 or uint8 device tensor is needed")
    buf = ((ctypes.c_float if t.dtype == torch.float32 else ctypes.c_uint8) * t.numel()).from_address(t.data_ptr())
    return np.ctypeslib.as_array(buf).reshape(tuple(t.shape))


_direct_ok = {}
_direct_mode = {}      # device index -> etm_host_direct_write_init's answer (2: with an HDP flush register, 1: without, 0: not usable)


def host_direct_write_ok(device):
    """Can the host write rows straight into this device's memory (etm_host_direct_write_init: large BAR + HDP flush register),
    and does a written pattern come back through the device (self-test, once per device)?"""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _direct_ok:
        ok = False
        try:
            lib = _lib.load()
            mode = lib.etm_host_direct_write_init(idx)
            _direct_mode[idx] = mode
            if mode >= 1:
                import numpy as np
                # 48 rounds of "host rewrites a small buffer whose lines the previous kernel has just read, a kernel reads it
                # again": what a rollout does with its staging rows (tools/microbench/bar_stale.hip is the long form: 12,000
                # plain launches and graph replays, none stale)
                probe = torch.zeros(1024, dtype=torch.float32, device=device)
                view = host_view(probe)
                base = np.arange(1024, dtype=np.float32) * 0.5
                seen = []
                for k in range(48):
                    torch.cuda.synchronize(device)
                    view[:] = base + float(k + 1)
                    lib.etm_host_store_fence(idx)
                    seen.append(probe + 0.0)
                got = torch.stack(seen).cpu().numpy()
                ok = bool(all(np.array_equal(got[k], base + float(k + 1)) for k in range(48)))
        except Exception:      # noqa: BLE001 -- anything odd: keep pinned memory + uploads
            ok = False
        _direct_ok[idx] = ok
    return _direct_ok[idx]


def upload(dst, src_pinned, stream):
    """Asynchronous pinned-host -> device copy of a contiguous block on ``stream`` (a torch.cuda.Stream)."""
    lib = _lib.load()
    nbytes = src_pinned.numel() * src_pinned.element_size()
    if not (dst.is_contiguous() and src_pinned.is_contiguous()) or dst.numel() * dst.element_size() != nbytes:
        raise TypeError("upload needs contiguous blocks of equal size")
    _lib.check(lib.etm_upload(dst.data_ptr(), src_pinned.data_ptr(), nbytes, stream.cuda_stream), "etm_upload")


_fused_linear_relu = None  # None: untested, True/False after the first call


def _addmm_relu(bias, x, wt):
    """relu(bias + x wt)."""
    if _fused_linear_relu:        # bias + ReLU in the GEMM's epilogue (one launch; verified against the two-op form by linear_relu)
        return torch._addmm_activation(bias, x, wt, use_gelu=False)
    return torch.relu_(torch.addmm(bias, x, wt))


def _linear_backward(ctx, g, weight, y):
    """Backward of y = act(x W^T + b) up to the weight gradient: (dy, dx = dy W, d bias), dy = ``g`` masked by the ReLU of the
    output ``y`` (None: no ReLU).  The element-wise part is etm_relu_bwd_colsum -- the ReLU mask and the bias gradient in one pass +
    the fixed-order column-sum reduction, its second stage in the collector's one reduction launch when one is active.  nn.Linear
    leaves the bias gradient to the framework's column sum instead: two stages with a semaphore, which this runtime does not replay
    reliably from a captured graph (profiles/r05/graph_reduce_hazard.txt), and two launches."""
    g = _f32c(g, "grad")
    db = None
    if y is not None or (ctx.bias_ptr is not None and ctx.needs_input_grad[2]):
        lib = _lib.load()
        n, c = g.shape
        gm = torch.empty_like(g) if y is not None else None
        nbytes = lib.etm_relu_bwd_colsum_workspace_bytes(n, c)
        ws, deferred = DeferredDw.colsum_workspace(nbytes, lib.etm_relu_bwd_colsum_partial_rows(n), c, [(0, c, ctx.bias_ptr)], g.device, "relu_bwd")
        db = None if deferred else torch.empty(c, dtype=torch.float32, device=g.device)
        _lib.check(lib.etm_relu_bwd_colsum(_ptr(g), _ptr(y), _ptr(gm), _ptr(db), _ptr(ws), nbytes, n, c, _stream()), "etm_relu_bwd_colsum")
        g = g if gm is None else gm
    dx = g.mm(weight) if ctx.needs_input_grad[0] else None
    return g, dx, db


def _prev_input_args(table, actions, sizes, rewards, N=None):
    """Checked (R, D, N, actions pointer, row stride, branch table, branch count, rewards) of the two etm_prev_input_* entries."""
    _need_dev(table, actions)
    if rewards is not None and not (rewards.is_cuda or rewards.is_pinned()):       # (the rollout reads its pinned block in place)
        raise RuntimeError("prev_input: rewards must be in device or pinned host memory")
    if table.dim() != 2 or table.dtype != torch.float32 or not table.is_contiguous():
        raise TypeError("prev_input: the table must be a contiguous float32 [R, D] tensor")
    R, D = table.shape
    sizes = tuple(int(a) for a in sizes)
    if not _lib.load().etm_prev_input_supported(R, D):
        raise RuntimeError(f"prev_input: a table of {R} rows x {D} columns is outside the kernels (1 .. 64 rows)")
    if sizes:
        if actions is None or actions.dtype != torch.int64 or actions.dim() != 2 or actions.shape[1] != len(sizes) or actions.stride(1) != 1:
            raise TypeError(f"prev_input: actions must be int64 [N, {len(sizes)}] with unit column stride")
        N = actions.shape[0]
    if rewards is not None:
        if rewards.dtype != torch.float32 or rewards.dim() != 1 or not rewards.is_contiguous() or (sizes and rewards.shape[0] != N):
            raise TypeError("prev_input: rewards must be a contiguous float32 [N] tensor")
        N = rewards.shape[0]
    if N is None or sum(sizes) + (rewards is not None) > R or not (sizes or rewards is not None):
        raise ValueError(f"prev_input: branches {sizes}{' + the reward row' if rewards is not None else ''} do not fit a table of {R} rows")
    return (R, D, N, _ptr(actions) if sizes else None, actions.stride(0) if sizes else 0, _c_ints(sizes) if sizes else None, len(sizes),
            _ptr(rewards))


def prev_input_rows(table, actions, sizes, rewards=None, ep_step=None, bias=None, out=None):
    """The addend of ``previous_step_input`` (etm_prev_input_rows; utils.previous_step_rows is the rule, bit for bit): [N, D] =
    sum_b table[off_b + actions[:, b]] + rewards[:, None] * table[-1] (+ ``bias``), +0 (+ bias) where a sample has no previous step --
    ``ep_step`` [N] int64 (device or pinned host memory; the rollout form): where its word is 0; without it (the training form): where
    actions[:, 0] < 0.  ``actions`` [N, B] int64 (any row stride), ``sizes`` the B branch sizes (empty: the action rows are not fed
    back).  ``out``: a float32 [N, D] destination with unit column stride."""
    lib = _lib.load()
    _need_dev(bias, out)
    R, D, N, a_ptr, a_ld, c_sizes, B, r_ptr = _prev_input_args(table, actions, sizes, rewards)
    if ep_step is not None and (ep_step.dtype != torch.int64 or ep_step.dim() != 1 or ep_step.shape[0] != N or not ep_step.is_contiguous()
                                or not (ep_step.is_cuda or ep_step.is_pinned())):
        raise TypeError("prev_input_rows: ep_step must be a contiguous int64 [N] tensor in device or pinned host memory")
    if bias is not None and (bias.dtype != torch.float32 or bias.shape != (D,) or not bias.is_contiguous()):
        raise TypeError("prev_input_rows: bias must be a contiguous float32 [D] tensor")
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=table.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (N, D) or out.stride(1) != 1:
        raise TypeError("prev_input_rows: out must be a float32 [N, D] tensor with unit column stride")
    _lib.check(lib.etm_prev_input_rows(_ptr(table), R, D, a_ptr, a_ld, c_sizes, B, r_ptr, _ptr(ep_step), _ptr(bias), _ptr(out), out.stride(0), N,
                                       _stream()), "etm_prev_input_rows")
    return out


def prev_input_grad(gm, table_like, actions, sizes, rewards=None, out=None):
    """The table's gradient (etm_prev_input_grad; utils.previous_step_table_grad is the rule): [R, D] = sum_n c_n^T gm[n] over the
    samples that have a previous step (actions[:, 0] >= 0), fixed summation order, no atomics.  ``gm`` [N, D] float32 with unit column
    stride; ``table_like``: the table (its shape is what is read); ``out``: a contiguous [R, D] destination."""
    lib = _lib.load()
    _need_dev(gm, out)
    R, D, N, a_ptr, a_ld, c_sizes, B, r_ptr = _prev_input_args(table_like, actions, sizes, rewards)
    if gm.dtype != torch.float32 or tuple(gm.shape) != (N, D) or gm.stride(1) != 1:
        raise TypeError(f"prev_input_grad: gm must be a float32 [{N}, {D}] tensor with unit column stride")
    if out is None:
        out = torch.empty((R, D), dtype=torch.float32, device=gm.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != (R, D) or not out.is_contiguous():
        raise TypeError("prev_input_grad: out must be a contiguous float32 [R, D] tensor")
    nbytes = lib.etm_prev_input_grad_workspace_bytes(N, R, D)
    ws = workspace(nbytes, gm.device, "prev_input_grad")          # (fixed address once a graph has captured it: freeze_workspaces)
    _lib.check(lib.etm_prev_input_grad(_ptr(gm), gm.stride(0), a_ptr, a_ld, c_sizes, B, r_ptr, _ptr(out), R, D, N, _ptr(ws), nbytes, _stream()),
               "etm_prev_input_grad")
    return out


class _PrevInputFn(torch.autograd.Function):
    """The addend of ``previous_step_input`` under autograd, over the two kernels: forward ``prev_input_rows`` in its training form
    (with lin_hidden's bias folded in, so the layer's forward needs no pass of its own for it), backward ``prev_input_grad`` of the
    incoming gradient -- which, from _LinearFn / _LinearReluNhwcFn, is gm = g * (y > 0).  The table's gradient goes straight into the
    parameter's arena view when a DeferredDw collector knows it.  The bias gets its gradient from the linear node (column sums of gm)."""

    @staticmethod
    def forward(ctx, table, actions, rewards, sizes, bias):
        ctx.actions, ctx.rewards, ctx.sizes, ctx.table_ptr = actions, rewards, tuple(sizes), table.data_ptr()
        ctx.save_for_backward(table)
        return prev_input_rows(table.detach(), actions, sizes, rewards, bias=None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, g):
        (table,) = ctx.saved_tensors
        g = g if g.dtype == torch.float32 and g.stride(1) == 1 else _f32c(g, "grad")
        dest = DeferredDw.claim([ctx.table_ptr])
        if dest is not None and tuple(dest[0].shape) == tuple(table.shape):
            prev_input_grad(g, table, ctx.actions, ctx.sizes, ctx.rewards, out=dest[0])
            return None, None, None, None, None
        return prev_input_grad(g, table, ctx.actions, ctx.sizes, ctx.rewards), None, None, None, None


def prev_input_addend(table, actions, sizes, rewards=None, bias=None):
    """``previous_step_input``'s addend [N, D] (+ ``bias``) as an autograd node over the two kernels (see _PrevInputFn); the operand
    ``addend`` of ``linear_relu_train`` / ``linear_relu_nhwc``."""
    return _PrevInputFn.apply(table, actions, rewards, tuple(sizes), bias)


class _LinearFn(torch.autograd.Function):
    """y = x W^T, x W^T + b or (``relu``) relu(x W^T + b) for 2-D fp32 device tensors: library GEMMs for y and dx, the backward's
    element-wise part in _linear_backward, the weight gradient to the grouped launch when a DeferredDw collector is active.
    transformer.py:26-29 queries / fc_out, :115 fc without their epilogues; fc_out with its bias on the pre-LN / gated blocks.
    ``addend`` (relu form only; previous_step_input): [N, out] that already holds e + b, so y = relu(x W^T + addend); its gradient is
    gm.  None: exactly the calls without it."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, addend=None):
        if addend is not None:
            if not relu:
                raise ValueError("_LinearFn: an addend belongs to the relu form")
            y = torch.relu_(torch.addmm(addend, x, weight.t()))
        elif relu:
            y = _addmm_relu(bias, x, weight.t())
        elif bias is not None:
            y = torch.addmm(bias, x, weight.t())
        else:
            y = x.mm(weight.t())
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.bias_ptr = None if bias is None else bias.data_ptr()
        ctx.has_addend = addend is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        g, dx, db = _linear_backward(ctx, g, weight, y)
        dw = None
        if ctx.needs_input_grad[1] and not DeferredDw.defer(g, x, weight):
            dw = g.t().mm(x)
        if ctx.has_addend:
            return dx, dw, db, None, g
        return dx, dw, db, None


def linear_nobias(x, weight):
    """F.linear(x, weight) for 2-D fp32 device tensors under autograd, weight gradient deferrable (see DeferredDw)."""
    if torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous():
        return _LinearFn.apply(x, weight, None, False)
    return torch.nn.functional.linear(x, weight)


def linear_bias(lin, x):
    """``lin(x)`` (an nn.Linear with bias) for 2-D fp32 device tensors under autograd: library GEMMs for y and dx, the bias gradient by
    the library's column sums, both parameter gradients deferrable (see DeferredDw).  Anything else: ``lin(x)``."""
    if (torch.is_grad_enabled() and lin.bias is not None and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()):
        return _LinearFn.apply(x, lin.weight, lin.bias, False)
    return lin(x)


class _LinearReluNhwcFn(torch.autograd.Function):
    """relu(x Wp^T + b) for NHWC-flattened features x [N, HW * C] and a weight kept in upstream's (c, h, w) column order
    (model.py:94): Wp = the weight with its columns in (h, w, c) order.  The permutation lives INSIDE the node: one permuting copy
    of the weight forward, and backward the weight gradient is permuted straight into the parameter's arena view when a DeferredDw
    collector knows it (one permuting copy instead of a permute-back copy plus the gradient packing copy).
    ``addend`` (previous_step_input): [N, out] that already holds e + b, so y = relu(x Wp^T + addend); its gradient is gm.  None:
    exactly the calls without it."""

    @staticmethod
    def forward(ctx, x, weight, bias, channels, addend=None):
        out, feat = weight.shape
        hw = feat // channels
        wp = weight.detach().view(out, channels, hw).transpose(1, 2).reshape(out, feat)       # [out, (h, w, c)]
        y = _addmm_relu(bias, x, wp.t()) if addend is None else torch.relu_(torch.addmm(addend, x, wp.t()))
        ctx.save_for_backward(x, wp, y)
        ctx.bias_ptr, ctx.weight_ptr, ctx.channels = bias.data_ptr(), weight.data_ptr(), channels
        ctx.has_addend = addend is not None
        return y

    @staticmethod
    def backward(ctx, g):
        x, wp, y = ctx.saved_tensors
        gm, dx, db = _linear_backward(ctx, g, wp, y)
        dw = None
        if ctx.needs_input_grad[1]:
            out, feat = wp.shape
            dwp = gm.t().mm(x).view(out, feat // ctx.channels, ctx.channels).transpose(1, 2)    # [out, c, hw] view of the (h, w, c) result
            dest = DeferredDw.claim([ctx.weight_ptr])
            if dest is not None:
                dest[0].view(dwp.shape).copy_(dwp)
            else:
                dw = dwp.reshape(out, feat)
        if ctx.has_addend:
            return dx, dw, db, None, gm
        return dx, dw, db, None


def linear_relu_nhwc(x, weight, bias, channels, addend=None):
    """relu(F.linear(x, nhwc_columns(weight, channels), bias)) as one autograd node (see _LinearReluNhwcFn); with ``addend`` (of
    ``prev_input_addend`` WITH this bias) relu(F.linear(x, nhwc_columns(weight, channels)) + addend)."""
    if addend is None:
        return _LinearReluNhwcFn.apply(x, weight, bias, channels)
    return _LinearReluNhwcFn.apply(x, weight, bias, channels, addend)


def linear_relu_train(x, weight, bias, addend=None):
    """relu(F.linear(x, weight, bias)) for 2-D fp32 device tensors under autograd (see _LinearFn); with ``addend`` (of
    ``prev_input_addend`` WITH this bias) relu(F.linear(x, weight) + addend)."""
    if addend is None:
        return _LinearFn.apply(x, weight, bias, True)
    return _LinearFn.apply(x, weight, bias, True, addend)


def linear_relu(lin, x, out=None):
    """relu(lin(x)).  In the no-grad rollout path the ReLU rides in the GEMM epilogue (hipBLASLt through
    ``torch._addmm_activation``), saving one launch per layer; with autograd enabled it is the plain two-op form.
    ``out`` (no-grad only): contiguous destination."""
    global _fused_linear_relu

    def plain():
        if (torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and lin.bias is not None and out is None
                and x.is_contiguous()):
            return _LinearFn.apply(x, lin.weight, lin.bias, True)
        y = torch.relu(torch.nn.functional.linear(x, lin.weight, lin.bias))
        return y if out is None else out.copy_(y)

    if torch.is_grad_enabled() or _fused_linear_relu is False or x.dim() != 2:
        return plain()
    if _fused_linear_relu is None:
        if torch.cuda.is_current_stream_capturing():
            return plain()
        try:
            y = torch._addmm_activation(lin.bias, x, lin.weight.t(), use_gelu=False)
            ref = torch.relu(torch.nn.functional.linear(x, lin.weight, lin.bias))
            _fused_linear_relu = bool(torch.allclose(y, ref, atol=1e-5, rtol=1e-5))
        except Exception:
            _fused_linear_relu = False
        return plain()
    if out is not None:
        return torch._addmm_activation(lin.bias, x, lin.weight.t(), use_gelu=False, out=out)
    return torch._addmm_activation(lin.bias, x, lin.weight.t(), use_gelu=False)


def gae(rewards, dones, values, last_value, gamma, lamda, out=None, truncated=None, boot=None):
    """Generalized advantage estimation on device; [W,S] row-major like the reference buffer.
    ``truncated`` [W,S] bool / uint8 with ``boot`` [W,S] float32 (both or neither): where the flag is set -- only meaningful at a
    done -- the step's next value is ``boot`` instead of v_{t+1} * (1 - done) (etm_gae_truncated: a select; ``boot`` elsewhere may
    hold anything)."""
    lib = _lib.load()
    if (truncated is None) != (boot is None):
        raise TypeError("gae: truncated= and boot= come together")
    _need_dev(rewards, dones, values, last_value)
    rewards, values, last_value = _f32c(rewards, "rewards"), _f32c(values, "values"), _f32c(last_value, "last_value")
    d = dones.contiguous()
    d = d.view(torch.uint8) if d.dtype == torch.bool else d.to(torch.uint8)
    W, S = values.shape
    if out is None:
        out = torch.empty_like(values)
    elif not out.is_contiguous() or out.dtype != torch.float32:
        raise TypeError("advantages output must be contiguous float32")
    g32 = float(torch.tensor(float(gamma), dtype=torch.float32))
    gl32 = float(torch.tensor(float(gamma) * float(lamda), dtype=torch.float32))  # python-float product, then fp32 (buffer.py:111)
    if truncated is not None:
        _need_dev(truncated, boot)
        if tuple(truncated.shape) != (W, S) or tuple(boot.shape) != (W, S):
            raise ValueError(f"gae: truncated / boot must be [{W}, {S}], got {tuple(truncated.shape)} / {tuple(boot.shape)}")
        boot = _f32c(boot, "boot")
        tr = truncated.contiguous()
        tr = tr.view(torch.uint8) if tr.dtype == torch.bool else tr.to(torch.uint8)
        rc = lib.etm_gae_truncated(_ptr(rewards), _ptr(d), _ptr(tr), _ptr(values), _ptr(boot), _ptr(last_value), g32, gl32, _ptr(out),
                                   W, S, _stream())
        _lib.check(rc, "etm_gae_truncated")
        return out
    rc = lib.etm_gae(_ptr(rewards), _ptr(d), _ptr(values), _ptr(last_value), g32, gl32, _ptr(out), W, S, _stream())
    _lib.check(rc, "etm_gae")
    return out


def obs_stats_supported(features) -> bool:
    """Whether ``obs_stats_update`` takes rows of ``features`` floats (etm_obs_stats_supported: 1 to 1024)."""
    return bool(_lib.load().etm_obs_stats_supported(int(features)))


def _f64c(t, name, shape):
    if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise TypeError(f"{name} must be a contiguous float64 tensor of shape {tuple(shape)}")
    return t


def obs_stats_update(x, stats, mean, rstd, epsilon):
    """Merge the rows of ``x`` [R, F] float32 into the running per-feature triple ``stats`` [3, F] float64 (count, mean, M2) and
    refresh the fp32 table ``mean`` [F], ``rstd`` [F] = 1 / sqrt(M2 / count + epsilon) -- all three IN PLACE (etm_obs_stats_update:
    chunks of 256 rows, merged in chunk order; deterministic)."""
    lib = _lib.load()
    _need_dev(x, stats, mean, rstd)
    x = _f32c(x, "x")
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError("obs_stats_update needs a non-empty [R, F] tensor")
    R, F = x.shape
    if not lib.etm_obs_stats_supported(F):
        raise ValueError(f"obs_stats_update: {F} features (the kernel takes 1 to 1024)")
    _f64c(stats, "stats", (3, F))
    for t, name in ((mean, "mean"), (rstd, "rstd")):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (F,):
            raise TypeError(f"{name} must be a contiguous float32 tensor of shape ({F},)")
    ws_bytes = lib.etm_obs_stats_workspace_bytes(R, F)
    ws = workspace(ws_bytes, x.device, tag="obs_stats")
    _lib.check(lib.etm_obs_stats_update(_ptr(x), R, F, _ptr(stats), _ptr(mean), _ptr(rstd), float(epsilon), _ptr(ws), ws_bytes, _stream()),
               "etm_obs_stats_update")
    return stats


def obs_normalize(x, mean, rstd, clip, index=None, out=None):
    """clamp((x - mean) * rstd, -clip, +clip) in float32, subtraction and product rounded separately (etm_obs_normalize); ``x``
    [N, F] float32, or with ``index`` (int64 device tensor [n]) the rows x[index] -> [n, F].  One launch, capturable."""
    lib = _lib.load()
    _need_dev(x, mean, rstd, index, out)
    x, mean, rstd = _f32c(x, "x"), _f32c(mean, "mean"), _f32c(rstd, "rstd")
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError("obs_normalize needs a non-empty tensor")
    F = x.shape[-1]
    if mean.numel() != F or rstd.numel() != F:
        raise ValueError(f"obs_normalize: the table has {mean.numel()} / {rstd.numel()} entries, the rows {F}")
    if index is not None:
        if index.dtype != torch.int64 or x.dim() != 2:
            raise TypeError("obs_normalize: index must be int64 and x [N, F]")
        index = index.contiguous()
        shape = (index.numel(), F)
    else:
        shape = tuple(x.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous():
        raise TypeError("obs_normalize: out must be a contiguous float32 tensor of the result's shape")
    n = out.numel() // F
    if n:
        _lib.check(lib.etm_obs_normalize(_ptr(x), _ptr(index), _ptr(mean), _ptr(rstd), float(clip), _ptr(out), n, F, _stream()),
                   "etm_obs_normalize")
    return out


ATTN_STATS_WORDS = _lib.ATTN_STATS_WORDS


def attn_stats(att, mask, table_rows, workspace):
    """Add the statistics of the attention probabilities ``att`` [N, H, L] (float32, contiguous, as ``mha`` returns them) under the
    window mask ``mask`` [N, L] (uint8, non-zero = valid: ``WindowSpec.mask``) to ``table_rows`` [H, 264] float64, IN PLACE
    (etm_attn_stats; the words are listed in include/etm_hip.h).  ``workspace``: a uint8 device tensor of at least
    etm_attn_stats_workspace_bytes(N, H, L) bytes, owned by the caller.  Two launches, capturable, deterministic."""
    lib = _lib.load()
    _need_dev(att, mask, table_rows, workspace)
    if att.dtype != torch.float32 or att.dim() != 3 or not att.is_contiguous() or att.numel() == 0:
        raise TypeError("attn_stats: att must be a non-empty contiguous float32 tensor [N, H, L]")
    N, H, L = att.shape
    if mask.dtype != torch.uint8 or tuple(mask.shape) != (N, L) or not mask.is_contiguous():
        raise TypeError(f"attn_stats: mask must be a contiguous uint8 tensor [{N}, {L}]")
    _f64c(table_rows, "attn_stats: table_rows", (H, ATTN_STATS_WORDS))
    ws_bytes = lib.etm_attn_stats_workspace_bytes(N, H, L)
    if ws_bytes <= 0:
        raise ValueError(f"attn_stats: N = {N}, H = {H}, L = {L} (the kernel takes N >= 1, 1 <= H <= 32, 1 <= L <= 128)")
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < ws_bytes:
        raise TypeError(f"attn_stats: workspace must be a contiguous uint8 tensor of at least {ws_bytes} bytes")
    _lib.check(lib.etm_attn_stats(_ptr(att), _ptr(mask), _ptr(table_rows), _ptr(workspace), workspace.numel(), N, H, L, _stream()),
               "etm_attn_stats")
    return table_rows


class AttentionStatistics:
    """Owner of the accumulator of ``attn_stats`` for a model: ``table`` [blocks, heads, 264] float64 and one workspace sized for
    ``mbs``, the largest batch a pass will hand over -- both allocated once, so a captured graph can hold their addresses.
    A forward pass hands ``table[block]`` and ``workspace`` to ``attn_stats``; ``reset()`` zeroes the table; ``read()`` returns it as
    numpy (one device-to-host copy)."""

    def __init__(self, blocks, heads, mbs, L, device):
        lib = _lib.load()
        self.blocks, self.heads, self.mbs, self.L = int(blocks), int(heads), int(mbs), int(L)
        nbytes = lib.etm_attn_stats_workspace_bytes(self.mbs, self.heads, self.L)
        if self.blocks < 1 or nbytes <= 0:
            raise ValueError(f"AttentionStatistics: blocks = {blocks}, heads = {heads}, mbs = {mbs}, L = {L} (the kernel takes "
                             "1 to 32 heads, a window of 1 to 128 entries and at least one sample)")
        self.table = torch.zeros((self.blocks, self.heads, ATTN_STATS_WORDS), dtype=torch.float64, device=device)
        self.workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=device)

    def reset(self):
        self.table.zero_()

    def read(self):
        return self.table.cpu().numpy()


def return_scale_workspace(W, device):
    """A workspace of etm_return_scale for ``W`` workers, owned by the caller; its first float is the scale after a call."""
    return torch.zeros(int(_lib.load().etm_return_scale_workspace_bytes(int(W))), dtype=torch.uint8, device=device)


def return_scale(rewards, dones, ret_carry, stats, gamma, epsilon, clip, out=None, ws=None):
    """Return-based reward scaling of one rollout (etm_return_scale): the per-worker discounted returns R_t = gamma R_{t-1} + r_t
    (float64; R = 0 after a done) continue from ``ret_carry`` [W] float64 and are merged into the running triple ``stats`` [3] float64,
    both IN PLACE; -> (scaled [W, S] float32 = clamp(rewards * scale, -clip, +clip), scale: a 1-element float32 view of ``ws``) with
    scale = 1 / sqrt(M2 / count + epsilon) of the merged triple.  ``ws``: ``return_scale_workspace(W, device)`` (None: a fresh one)."""
    lib = _lib.load()
    _need_dev(rewards, dones, ret_carry, stats, out, ws)
    rewards = _f32c(rewards, "rewards")
    if rewards.dim() != 2 or rewards.numel() == 0:
        raise ValueError("return_scale needs non-empty [W, S] rewards")
    W, S = rewards.shape
    if tuple(dones.shape) != (W, S):
        raise ValueError(f"return_scale: dones must be [{W}, {S}], got {tuple(dones.shape)}")
    d = dones.contiguous()
    d = d.view(torch.uint8) if d.dtype == torch.bool else d.to(torch.uint8)
    _f64c(ret_carry, "ret_carry", (W,))
    _f64c(stats, "stats", (3,))
    if out is None:
        out = torch.empty_like(rewards)
    elif out.dtype != torch.float32 or tuple(out.shape) != (W, S) or not out.is_contiguous():
        raise TypeError("return_scale: out must be a contiguous float32 tensor [W, S]")
    ws_bytes = lib.etm_return_scale_workspace_bytes(W)
    if ws is None:
        ws = return_scale_workspace(W, rewards.device)
    elif ws.dtype != torch.uint8 or ws.numel() < ws_bytes:
        raise TypeError("return_scale: ws must come from return_scale_workspace(W, device)")
    _lib.check(lib.etm_return_scale(_ptr(rewards), _ptr(d), _ptr(ret_carry), _ptr(stats), float(gamma), float(epsilon), float(clip),
                                    _ptr(out), W, S, _ptr(ws), ws.numel(), _stream()), "etm_return_scale")
    return out, ws[:4].view(torch.float32)


def adv_stats(adv):
    """(count, mean, M2) of a flat advantage vector as a 3-element device tensor."""
    lib = _lib.load()
    _need_dev(adv)
    adv = _f32c(adv.reshape(-1), "adv")
    stats = torch.empty(3, dtype=torch.float32, device=adv.device)
    ws_bytes = lib.etm_adv_stats_workspace_bytes(adv.numel())
    if ws_bytes > 0:       # large N: per-chunk statistics on many workgroups + a fixed-order merge
        ws = workspace(ws_bytes, adv.device, tag="adv_stats")
        _lib.check(lib.etm_adv_stats_ws(_ptr(adv), adv.numel(), _ptr(stats), _ptr(ws), ws_bytes, _stream()), "etm_adv_stats_ws")
        return stats
    _lib.check(lib.etm_adv_stats(_ptr(adv), adv.numel(), _ptr(stats), _stream()), "etm_adv_stats")
    return stats


ARENA_DIGEST_PARTIALS = 1024


def arena_digest_workspace(device, n_partial=ARENA_DIGEST_PARTIALS):
    """Scratch of ``arena_digest`` (3 * n_partial 64-bit words), owned by the caller."""
    return torch.zeros(3 * int(n_partial), dtype=torch.int64, device=device)


def arena_digest(x, out=None, partial=None, n_partial=ARENA_DIGEST_PARTIALS):
    """The four 64-bit words of etm_arena_digest over the contiguous float32 device tensor ``x`` taken as raw bits (fingerprint, number
    of Inf / NaN words, bit pattern of the largest finite |x|, number of words) -> ``out`` [4] int64 on the device (the words are
    unsigned: read them through ``.view(np.uint64)`` on the host; checkpoint.digest_numpy computes the same four).  Two launches on the
    current stream; ``out`` and ``partial`` (``arena_digest_workspace``) are allocated when not given."""
    lib = _lib.load()
    _need_dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() == 0:
        raise TypeError("arena_digest needs a non-empty contiguous float32 tensor")
    if out is None:
        out = torch.zeros(4, dtype=torch.int64, device=x.device)
    if partial is None:
        partial = arena_digest_workspace(x.device, n_partial)
    if partial.dtype != torch.int64 or partial.numel() < 3 * int(n_partial) or out.dtype != torch.int64 or out.numel() != 4:
        raise TypeError("arena_digest: out is [4] int64, partial at least [3 * n_partial] int64")
    _lib.check(lib.etm_arena_digest(_ptr(x), x.numel(), _ptr(partial), int(n_partial), _ptr(out), _stream()), "etm_arena_digest")
    return out


def _check_old_logps(old_logps, N, cols, what):
    """The ``old_logps=`` argument of the loss ops: the minibatch's rows of the rollout's log-prob table, float32 [N, >= cols] on the
    device with contiguous rows (any row stride)."""
    _need_dev(old_logps)
    if (old_logps.dtype != torch.float32 or old_logps.dim() != 2 or old_logps.shape[0] != N or old_logps.shape[1] < cols
            or old_logps.stride(1) != 1):
        raise ValueError(f"{what}: old_logps must be float32 [{N}, {cols}] with contiguous rows, got {tuple(old_logps.shape)} {old_logps.dtype}")


def _check_kl_coef(kl_coef, what):
    """The ``kl_coef=`` argument of the loss ops (`kl_penalty`): ONE float32 on the device, read in place by the kernels."""
    _need_dev(kl_coef)
    if kl_coef.dtype != torch.float32 or kl_coef.numel() != 1:
        raise ValueError(f"{what}: kl_coef must be a device tensor of one float32, got {tuple(kl_coef.shape)} {kl_coef.dtype}")


@dataclasses.dataclass(frozen=True, eq=False)
class _LossCall:
    """What a loss call knows beyond the tensors that autograd sees; ``_loss_call`` makes it and validates it once.  The variant of
    the C entry follows from what is set: ``action_mask`` alone -> *_masked; the old policy (``old_logps``, or ``old_mean`` /
    ``old_log_std`` of a Box policy) -> *_kl, the mask then optional; ``kl_coef`` on top -> *_kl_penalty."""
    stats3: torch.Tensor
    clip: float
    vf_coef: float
    beta: float
    dyn: torch.Tensor = None            # float64 device (clip, beta), read by the kernels instead of the two scalars
    unit_grad: bool = False
    sizes: tuple = None                 # heads + loss: the branch sizes of a MultiDiscrete policy
    action_mask: torch.Tensor = None
    old_logps: torch.Tensor = None
    old_mean: torch.Tensor = None
    old_log_std: torch.Tensor = None
    kl_coef: torch.Tensor = None

    @property
    def kl(self):
        return self.old_logps is not None or self.old_mean is not None

    @property
    def suffix(self):
        """Behind etm_heads_loss[_gaussian | _branched] / etm_ppo_loss -- the scheme lib.py derives the signatures by."""
        return ("_kl" if self.kl else "_masked" if self.action_mask is not None else "") + ("_penalty" if self.kl_coef is not None else "")

    def tail(self, N, shift=None):
        """The arguments behind the unmasked entry's, in the order of ``suffix``.  ``shift`` (PPO loss entries): the branch's first
        column among the concatenated branches -- its mask bits and its log-prob columns start there."""
        t = []
        if self.action_mask is not None or self.old_logps is not None:
            t += [_ptr(self.action_mask)] + ([] if shift is None else [shift if self.action_mask is not None else 0])
        for rows in (self.old_logps, self.old_mean):      # rows of any stride
            if rows is not None:
                t += [rows.data_ptr(), rows.stride(0) if N > 1 else rows.shape[1]]
        if self.old_logps is not None and shift is not None:
            t.append(shift)
        if self.old_log_std is not None:
            t.append(self.old_log_std.data_ptr())
        return t + ([] if self.kl_coef is None else [self.kl_coef.data_ptr()])


def _loss_call(what, N, cols, adv, stats3, dyn, clip, vf_coef, beta, **policy):
    """The record of one call of the loss op ``what`` over ``N`` samples, its operands checked.  ``cols``: the policy head's columns --
    for ``ppo_loss`` the column at which each branch ends, every one checked as that branch's launch needs it."""
    c = _LossCall(adv_stats(adv) if stats3 is None else stats3, float(clip), float(vf_coef), float(beta), dyn, **policy)
    gauss = what == "heads_ppo_loss_gaussian"
    if (c.old_mean is None) != (c.old_log_std is None):
        raise ValueError(f"{what}: old_mean and old_log_std come together (the exact KL needs both)")
    if c.kl_coef is not None and not c.kl:
        raise ValueError(f"{what}: kl_coef without " + ("old_mean / old_log_std (the KL penalty is a term in the exact KL); pass both" if gauss
                                                        else "old_logps (the KL penalty is a term in the exact KL); pass the rollout's log-prob rows"))
    if dyn is not None and (dyn.dtype != torch.float64 or dyn.numel() != 2 or not dyn.is_cuda):
        raise TypeError(f"{what}: dyn must be a float64 device tensor (clip, beta)")
    if c.kl_coef is not None:
        _check_kl_coef(c.kl_coef, what.replace("_gaussian", ""))
    if c.old_mean is not None:
        # Box with the exact KL: old_mean [N, A] the rollout's means (rows of any stride), old_log_std [A] its log sigma
        _need_dev(c.old_mean, c.old_log_std)
        old_mean, old_log_std, A = c.old_mean, c.old_log_std, cols
        if (old_mean.dtype != torch.float32 or old_mean.dim() != 2 or tuple(old_mean.shape) != (N, A) or old_mean.stride(1) != 1
                or old_log_std.dtype != torch.float32 or old_log_std.numel() != A or not old_log_std.is_contiguous()):
            raise ValueError(f"{what}: old_mean must be float32 [{N}, {A}] with contiguous rows and old_log_std "
                             f"float32 [{A}], got {tuple(old_mean.shape)} {old_mean.dtype} / {tuple(old_log_std.shape)} {old_log_std.dtype}")
    for end in (cols if what == "ppo_loss" else (cols,)):
        if c.old_logps is not None:
            _check_old_logps(c.old_logps, N, end, what)
        if c.action_mask is not None:
            _mask_words(c.action_mask, N, end, what)
    return c


class _PpoLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, value, actions, old_logp, adv, old_value, call, branch, n_branches, shift, include_value):
        lib = _lib.load()
        _need_dev(logits, value, actions, old_logp, adv, old_value, call.stats3)
        logits = _f32c(logits, "logits")
        value = _f32c(value, "value")
        adv, old_value = _f32c(adv, "adv"), _f32c(old_value, "old_value")
        if actions.dtype != torch.int64 or old_logp.dtype != torch.float32:
            raise TypeError("actions must be int64 and old log-probs float32")
        actions, old_logp = actions.contiguous(), old_logp.contiguous()
        N, A = logits.shape
        B = actions.shape[1] if actions.dim() == 2 else 1
        dev = logits.device
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        d_logits = torch.empty_like(logits)
        d_value = torch.empty_like(value)
        nbytes = lib.etm_ppo_loss_workspace_bytes(N)
        ws = workspace(nbytes, dev, "ppo")
        # this branch's actions are bits [shift, shift + A) of the samples' words and columns [shift, shift + A) of the log-prob rows
        rc = getattr(lib, "etm_ppo_loss" + call.suffix)(
            _ptr(logits), actions.data_ptr() + 8 * branch, B, old_logp.data_ptr() + 4 * branch, B, _ptr(adv), _ptr(old_value), _ptr(value),
            _ptr(call.stats3), call.clip, call.vf_coef, call.beta, 1.0 / (N * n_branches), 1.0 / N, 1.0 / N, 1 if include_value else 0,
            _ptr(out8), _ptr(d_logits), _ptr(d_value), _ptr(ws), nbytes, _ptr(call.dyn), N, A, *call.tail(N, shift), _stream())
        _lib.check(rc, "etm_ppo_loss")
        ctx.save_for_backward(d_logits, d_value)
        ctx.include_value = include_value
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out8)
        return out8[2].clone(), out8

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        if g_loss is None:
            return (None,) * len(ctx.needs_input_grad)
        d_logits, d_value = ctx.saved_tensors
        grads = (d_logits * g_loss, d_value * g_loss if ctx.include_value else None)
        return grads + (None,) * (len(ctx.needs_input_grad) - len(grads))


class _HeadsLossFn(torch.autograd.Function):
    """Hidden heads (bias + ReLU), policy branch, value head, PPO loss and the backward pass down to the hidden heads' pre-activations
    as one kernel pass (csrc/heads_loss.hip); the two hidden GEMMs h W^T (forward) and gm W (backward) stay library GEMMs, the hidden
    heads' weight gradients go to the grouped launch.  Gradients are those of ``loss`` itself (unit upstream gradient) times
    ``g_loss``.  The inputs that receive gradients come first (``log_std``: a Box policy's, else None), then the other tensors, then
    the ``_LossCall``."""

    @staticmethod
    def forward(ctx, h, wlp, blp, wlv, blv, wb, bb, wv, bv, log_std, actions, old_logp, adv, old_value, call):
        lib = _lib.load()
        _need_dev(h, wlp, blp, wlv, blv, wb, bb, wv, bv, log_std, actions, old_logp, adv, old_value, call.stats3)
        h = _f32c(h, "h")
        N, hid, A = h.shape[0], wlp.shape[0], wb.shape[0]
        dev = h.device
        pre_p, pre_v = h.mm(wlp.t()), h.mm(wlv.t())
        gm_p, gm_v = torch.empty_like(pre_p), torch.empty_like(pre_v)
        gauss = log_std is not None
        # the row of sums: a Box policy's carries d log_std behind the statistics, the exact KL's the KL sum at its very end
        kind = ("gaussian_" if gauss else "") + ("kl_" if call.kl else "")
        row = getattr(lib, f"etm_heads_loss_{kind}row_floats")(hid, A)
        nbytes = getattr(lib, f"etm_heads_loss_{kind}workspace_bytes")(N, hid, A)
        sums = torch.empty(row, dtype=torch.float32, device=dev)
        out8 = torch.empty(8, dtype=torch.float32, device=dev)
        ws = workspace(nbytes, dev, "heads_loss")
        actions, old_logp = actions.contiguous(), old_logp.contiguous()
        if gauss:
            # Box: wb / bb the mean head, actions [N, A] the stored raw float actions, old_logp [N] (or [N, 1]) the joint log-probs
            taken = (_ptr(_f32c(actions, "actions")), A, _ptr(_f32c(log_std, "log_std")), _ptr(old_logp), 1)
        else:
            B = actions.shape[1] if actions.dim() == 2 else 1
            taken = (_ptr(actions), B, _ptr(old_logp), B)
        # MultiDiscrete: wb / bb are the branches' heads concatenated; policy term, KL and clip fraction are means over N B
        nbr = 1 if call.sizes is None else len(call.sizes)
        shape = (A,) if call.sizes is None else _branch_table(call.sizes)
        entry = "etm_heads_loss" + ("_gaussian" if gauss else "_branched" if call.sizes is not None else "") + call.suffix
        rc = getattr(lib, entry)(
            _ptr(pre_p), _ptr(pre_v), _ptr(blp), _ptr(blv), _ptr(wb), _ptr(bb), _ptr(wv), _ptr(bv), *taken, _ptr(_f32c(adv, "adv")),
            _ptr(_f32c(old_value, "old_value")), _ptr(call.stats3), call.clip, call.vf_coef, call.beta, 1.0 / (N * nbr), 1.0 / N, 1.0 / N,
            _ptr(call.dyn), _ptr(gm_p), _ptr(gm_v), _ptr(sums), _ptr(out8), 0, 0, _ptr(ws), nbytes, N, hid, *shape, *call.tail(N), _stream())
        _lib.check(rc, "etm_heads_loss")
        ctx.save_for_backward(h, wlp, wlv, gm_p, gm_v, sums)
        ctx.dims = (hid, A)
        ctx.gauss = gauss
        ctx.unit = call.unit_grad
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out8)
        return out8[2].clone(), out8

    @staticmethod
    def backward(ctx, g_loss, _g_stats):
        if g_loss is None:
            return (None,) * len(ctx.needs_input_grad)
        h, wlp, wlv, gm_p, gm_v, sums = ctx.saved_tensors
        hid, A = ctx.dims
        unit = ctx.unit                 # the caller promises loss.backward() on the returned loss itself: g_loss == 1, nothing to scale
        dh = None
        if ctx.needs_input_grad[0]:
            dh = gm_p.mm(wlp)
            dh.addmm_(gm_v, wlv)
            if not unit:
                dh = dh * g_loss
        dwlp = dwlv = None
        if ctx.needs_input_grad[1] and not (unit and DeferredDw.defer(gm_p, h, wlp)):
            dwlp = gm_p.t().mm(h) if unit else gm_p.t().mm(h) * g_loss
        if ctx.needs_input_grad[3] and not (unit and DeferredDw.defer(gm_v, h, wlv)):
            dwlv = gm_v.t().mm(h) if unit else gm_v.t().mm(h) * g_loss
        s = sums if unit else sums * g_loss
        o = (3 + A) * hid
        grads = (dh, dwlp, s[:hid], dwlv, s[hid:2 * hid], s[3 * hid:o].view(A, hid), s[o:o + A], s[2 * hid:3 * hid].view(1, hid),
                 s[o + A:o + A + 1], s[o + A + 6:o + 2 * A + 6] if ctx.gauss else None)
        return grads + (None,) * (len(ctx.needs_input_grad) - len(grads))


def _branch_list(branch):
    return list(branch) if isinstance(branch, (list, tuple, torch.nn.ModuleList)) else [branch]


def heads_loss_supported(h, lin_policy, branch):
    """Does ``heads_ppo_loss`` take this minibatch?  ``branch``: the policy branch, or the list of branches of a MultiDiscrete
    policy (etm_heads_loss_supported_branched)."""
    if not (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32):
        return False
    lib = _lib.load()
    br = _branch_list(branch)
    if len(br) == 1:
        return bool(lib.etm_heads_loss_supported(h.shape[0], lin_policy.weight.shape[0], br[0].weight.shape[0]))
    tab, nbr = _branch_table([b.weight.shape[0] for b in br])
    return bool(lib.etm_heads_loss_supported_branched(h.shape[0], lin_policy.weight.shape[0], tab, nbr))


def heads_loss_supported_gaussian(h, lin_policy, mean_head):
    """Does ``heads_ppo_loss_gaussian`` take this minibatch (etm_heads_loss_supported_gaussian: A <= 8, hid % 64 == 0, hid <= 512)?"""
    return (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32
            and bool(_lib.load().etm_heads_loss_supported_gaussian(h.shape[0], lin_policy.weight.shape[0], mean_head.weight.shape[0])))


def heads_ppo_loss_gaussian(h, lin_policy, lin_value, mean_head, log_std, value_head, actions, old_logp, adv, old_value, clip, vf_coef, beta,
                            stats3=None, dyn=None, unit_grad=False, old_mean=None, old_log_std=None, kl_coef=None):
    """``heads_ppo_loss`` for a Box policy (diagonal Gaussian, state-independent ``log_std`` [A]): ``mean_head`` gives the means,
    ``actions`` [N, A] are the stored raw float actions, ``old_logp`` [N] or [N, 1] their joint log-probs.  One ratio per sample;
    the gradients reach ``log_std`` too (etm_heads_loss_gaussian).
    ``old_mean`` [N, A] / ``old_log_std`` [A] (optional, together): the means and log sigma of the policy that drew the samples;
    stats[4] is then the exact KL(old || new) of the two Gaussians instead of the k3 sample estimate, in the same launch and with
    every other output unchanged in its bits (etm_heads_loss_gaussian_kl); None = exactly the call without.
    ``kl_coef`` (optional, `kl_penalty`; needs ``old_mean``): a device tensor of one float32 that the kernels read in place; the loss is
    then loss + coef * stats[4] and every gradient (``log_std``'s too) is that sum's (etm_heads_loss_gaussian_kl_penalty); None =
    exactly the call without."""
    A = mean_head.weight.shape[0]
    call = _loss_call("heads_ppo_loss_gaussian", h.shape[0], A, adv, stats3, dyn, clip, vf_coef, beta, unit_grad=bool(unit_grad),
                      old_mean=old_mean, old_log_std=old_log_std, kl_coef=kl_coef)
    if actions.dim() != 2 or actions.shape[1] != A or not actions.is_floating_point():
        raise ValueError(f"heads_ppo_loss_gaussian: actions must be float [N, {A}]")
    loss, st = _HeadsLossFn.apply(h, lin_policy.weight, lin_policy.bias, lin_value.weight, lin_value.bias, mean_head.weight, mean_head.bias,
                                  value_head.weight, value_head.bias, log_std, actions, old_logp, adv, old_value, call)
    return loss, st[:6]


def heads_ppo_loss(h, lin_policy, lin_value, branch, value_head, actions, old_logp, adv, old_value, clip, vf_coef, beta, stats3=None, dyn=None,
                   unit_grad=False, action_mask=None, old_logps=None, kl_coef=None):
    """model.py:101-110 + the PPO loss of ``ppo_loss``, from the transformer output ``h`` [N, D]: -> (loss scalar with grad, stats[6]).
    ``branch``: the policy branch, or the list of branches of a MultiDiscrete policy (``actions`` / ``old_logp`` [N, B]; the semantics of
    ``ppo_loss`` over branches).  ``unit_grad=True``: the caller runs ``backward()`` on the returned loss itself (upstream gradient 1):
    no scaling launches, weight gradients of the hidden heads deferrable.  See _HeadsLossFn.
    ``action_mask`` (optional): int64 [N] device words, bit j = column j of the concatenated branch heads was allowed when the sample
    was drawn: per branch the log-sum-exp, log-prob and entropy run over the valid actions only and the logits of the others get a
    zero gradient (etm_heads_loss_masked / _branched_masked); None = exactly the calls without masks.
    ``old_logps`` (optional): float32 [N, sum A_b], every column's log-prob under the policy that drew the samples (the rollout's
    ``st_logps`` rows of the minibatch); stats[4] is then the exact KL(old || new) of the categoricals, the mean over samples and
    branches, instead of the k3 sample estimate, in the same launch and with every other output unchanged in its bits
    (etm_heads_loss_kl / _branched_kl, masks or not); None = exactly the call without.
    ``kl_coef`` (optional, `kl_penalty`; needs ``old_logps``): a device tensor of one float32 that the kernels read in place; the loss
    is then loss + coef * stats[4] and every gradient is that sum's (etm_heads_loss_kl_penalty / _branched_kl_penalty); None = exactly
    the call without."""
    br = _branch_list(branch)
    if len(br) == 1:
        wb, bb, sizes = br[0].weight, br[0].bias, None
    else:
        # the kernel reads the branches' heads as one [sum A_b, hid] matrix; autograd hands each branch its rows of the gradient
        wb, bb = torch.cat([b.weight for b in br], dim=0), torch.cat([b.bias for b in br], dim=0)
        sizes = tuple(int(b.weight.shape[0]) for b in br)
    call = _loss_call("heads_ppo_loss", h.shape[0], wb.shape[0], adv, stats3, dyn, clip, vf_coef, beta, unit_grad=bool(unit_grad), sizes=sizes,
                      action_mask=action_mask, old_logps=old_logps, kl_coef=kl_coef)
    loss, st = _HeadsLossFn.apply(h, lin_policy.weight, lin_policy.bias, lin_value.weight, lin_value.bias, wb, bb,
                                  value_head.weight, value_head.bias, None, actions, old_logp, adv, old_value, call)
    return loss, st[:6]


def ppo_loss(logits_list, value, actions, old_logp, adv, old_value, clip, vf_coef, beta, stats3=None, dyn=None, action_mask=None,
             old_logps=None, kl_coef=None):
    """PPO loss over all action branches.  Returns (loss scalar with grad, stats[6] device tensor in trainer.py:318-323 order).
    ``dyn``: optional float64 device tensor (clip, beta) read by the kernels at run time instead of the two scalars.
    ``action_mask`` (optional): int64 [N] device words as in ``heads_ppo_loss``; branch b reads its bits at the offset of its logits
    among the concatenated branches (etm_ppo_loss_masked); None = exactly the calls without masks.
    ``old_logps`` (optional): float32 [N, sum A_b], every column's log-prob under the policy that drew the samples; branch b reads its
    columns at the same offset, and stats[4] is the exact KL(old || new), the mean over samples and branches, instead of the k3
    sample estimate -- every other output unchanged in its bits (etm_ppo_loss_kl, masks or not); None = exactly the calls without.
    ``kl_coef`` (optional, `kl_penalty`; needs ``old_logps``): a device tensor of one float32 read in place; every branch's loss is then
    its loss + coef * its share of stats[4], with that sum's gradient (etm_ppo_loss_kl_penalty); None = exactly the calls without."""
    nb = len(logits_list)
    ends = list(itertools.accumulate(int(lg.shape[1]) for lg in logits_list))
    shifts = [0] + ends[:-1]      # (the mask shift and the column offset of a branch are the same number)
    call = _loss_call("ppo_loss", logits_list[0].shape[0], ends, adv, stats3, dyn, clip, vf_coef, beta, action_mask=action_mask,
                      old_logps=old_logps, kl_coef=kl_coef)
    loss, st = _PpoLossFn.apply(logits_list[0], value, actions, old_logp, adv, old_value, call, 0, nb, shifts[0], True)
    if nb == 1:
        return loss, st[:6]
    pol, ent, kl, cf = st[0], st[3], st[4], st[5]
    total = loss
    for b in range(1, nb):
        l_b, s_b = _PpoLossFn.apply(logits_list[b], value, actions, old_logp, adv, old_value, call, b, nb, shifts[b], False)
        total = total + l_b
        pol, ent, kl, cf = pol + s_b[0], ent + s_b[3], kl + s_b[4], cf + s_b[5]
    return total, torch.stack([pol, st[1], total.detach(), ent, kl, cf])


# ---------------------------------------------------------------------------------------------------------------- obs_reconstruction
class _BiasReluRowsFn(torch.autograd.Function):
    """relu(x + b) over the rows of x [n, c] (an NHWC activation seen as pixels x channels): the forward is two library element-wise
    ops, the backward is etm_relu_bwd_colsum -- the ReLU mask and the bias gradient in one pass with a fixed-order column sum, its
    second stage in the collector's one reduction launch when one is active (the library's own column sum is the reduction
    ``_linear_backward`` speaks of)."""

    @staticmethod
    def forward(ctx, x, bias):
        y = torch.relu_(x + bias)
        ctx.save_for_backward(y)
        ctx.bias_ptr = bias.data_ptr()
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        lib = _lib.load()
        g = _f32c(g, "grad")
        n, c = g.shape
        gm = torch.empty_like(g)
        nbytes = lib.etm_relu_bwd_colsum_workspace_bytes(n, c)
        ws, deferred = DeferredDw.colsum_workspace(nbytes, lib.etm_relu_bwd_colsum_partial_rows(n), c, [(0, c, ctx.bias_ptr)], g.device, "relu_bwd")
        db = None if deferred else torch.empty(c, dtype=torch.float32, device=g.device)
        _lib.check(lib.etm_relu_bwd_colsum(_ptr(g), _ptr(y), _ptr(gm), _ptr(db), _ptr(ws), nbytes, n, c, _stream()), "etm_relu_bwd_colsum")
        return gm, db


def conv_transpose_wgrad(g, x, K, S):
    """dW [Cin, Cout, K, K] of y = ConvTranspose2d(Cin, Cout, K, S)(x) from g = dL/dy NHWC [N, Ho, Wo, Cout] and x NHWC [N, Hi, Wi, Cin]:
    dW[ci][co][ky][kx] = sum x[n, iy, ix, ci] g[n, S iy + ky, S ix + kx, co] is the weight gradient of the convolution (Cout -> Cin, K, S)
    with the roles exchanged, etm_conv_train_wgrad(x := g, dy := x) -- in the transposed layer's own parameter layout, summed in a fixed
    order (the library's weight gradient of these layers adds with atomics: its bits change from call to call).  That entry's trailing
    "bias gradient", the column sums of x, is discarded."""
    lib = _lib.load()
    _need_dev(g, x)
    g, x = _f32c(g, "grad"), _f32c(x, "x")
    N, Ho, Wo, C = g.shape
    cin = x.shape[3]
    if tuple(x.shape[:3]) != (N, (Ho - K) // S + 1, (Wo - K) // S + 1):
        raise ValueError(f"conv_transpose_wgrad: the gradient {tuple(g.shape)} and the input {tuple(x.shape)} do not belong to one layer")
    args = (N, C, Ho, Wo, cin, K, K, S)
    nbytes = lib.etm_conv_train_wgrad_workspace_bytes(*args)
    ws = workspace(nbytes, g.device, "conv_wgrad")
    buf = torch.empty(K * K * C * cin + cin, dtype=torch.float32, device=g.device)
    _lib.check(lib.etm_conv_train_wgrad(_ptr(g), None, _ptr(x), _ptr(buf), _ptr(ws), nbytes, *args, _stream()), "etm_conv_train_wgrad")
    return buf[: K * K * C * cin].view(cin, C, K, K)


class _ConvTransposeFn(torch.autograd.Function):
    """y = conv_transpose2d(x, w, stride) without bias on channels_last activations: the library's transposed convolution forward, the
    library's convolution for dx, and ``conv_transpose_wgrad`` for dW (fixed summation order: two runs give the same bits)."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        ctx.save_for_backward(x, weight)
        ctx.stride = int(stride)
        return torch.nn.functional.conv_transpose2d(x, weight, None, stride)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous(memory_format=torch.channels_last)
        dx = torch.nn.functional.conv2d(g, weight, None, ctx.stride) if ctx.needs_input_grad[0] else None
        dw = None
        if ctx.needs_input_grad[1]:
            dw = conv_transpose_wgrad(g.permute(0, 2, 3, 1), x.permute(0, 2, 3, 1), weight.shape[2], ctx.stride)
        return dx, dw, None


def conv_transpose_relu(deconv, x):
    """relu(deconv(x)) for an nn.ConvTranspose2d on an NCHW-shaped tensor in channels_last memory (the decoder's two middle layers):
    the library's transposed convolution without its bias (``_ConvTransposeFn``), then bias + ReLU over the pixels' rows
    (``_BiasReluRowsFn``).  A CPU tensor, or no grad: the same expression in torch."""
    if not (x.is_cuda and torch.is_grad_enabled() and x.dtype == torch.float32):
        return torch.relu(deconv(x))
    y = _ConvTransposeFn.apply(x.contiguous(memory_format=torch.channels_last), deconv.weight, deconv.stride[0])
    n, c, h, w = y.shape
    rows = y.permute(0, 2, 3, 1).contiguous().view(n * h * w, c)
    return _BiasReluRowsFn.apply(rows, deconv.bias).view(n, h, w, c).permute(0, 3, 1, 2)


def obs_recon_supported(C, Hi, Wi):
    return bool(_lib.load().etm_obs_recon_supported(int(C), int(Hi), int(Wi)))


def _obs_recon_operands(a2, w, b, obs, index, coef_word, what):
    """Checked operands of etm_obs_recon_fwd_loss: (a2, w, b, x, N, C, Hi, Wi)."""
    _need_dev(a2, w, b, obs, index, coef_word)
    a2, w, b, x = _f32c(a2, "a2"), _f32c(w, "weight"), _f32c(b, "bias"), _obs_c(obs, "obs")
    if a2.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (8, 8) or w.shape[0] != a2.shape[3] or a2.shape[3] != 32 or tuple(b.shape) != (w.shape[1],):
        raise ValueError(f"{what}: a2 NHWC [N, Hi, Wi, 32], weight [32, C, 8, 8] and bias [C] expected, got {tuple(a2.shape)}, "
                         f"{tuple(w.shape)}, {tuple(b.shape)}")
    N, Hi, Wi, _ = a2.shape
    C = w.shape[1]
    if N < 1 or not obs_recon_supported(C, Hi, Wi):
        raise ValueError(f"{what}: outside the kernel's support (1 <= C <= 4, 1 <= Hi, Wi <= 4096, N >= 1): N {N}, C {C}, Hi {Hi}, Wi {Wi}")
    if x.dim() != 4 or tuple(x.shape[1:]) != (4 * Hi + 4, 4 * Wi + 4, C):
        raise ValueError(f"{what}: the observation must be NHWC [n, {4 * Hi + 4}, {4 * Wi + 4}, {C}] (the decoder's output size), got {tuple(x.shape)}")
    if index is not None and (index.dtype != torch.int64 or index.dim() != 1 or index.numel() != N or not index.is_contiguous()):
        raise ValueError(f"{what}: the index must be a contiguous int64 vector of {N} entries")
    if index is None and x.shape[0] != N:
        raise ValueError(f"{what}: {x.shape[0]} observations for {N} samples (pass an IndexedObservations to gather)")
    if coef_word.dtype != torch.float32 or coef_word.numel() != 1:
        raise ValueError(f"{what}: the coefficient must be a device tensor of one float32, got {tuple(coef_word.shape)} {coef_word.dtype}")
    return a2, w, b, x, N, C, Hi, Wi


def obs_recon_fwd_loss(a2, w, b, obs, coef_word, index=None):
    """etm_obs_recon_fwd_loss on checked operands -> (dz [N, Ho, Wo, C], out [4] = (loss, coef, coef * loss, 0), db [C])."""
    lib = _lib.load()
    a2, w, b, x, N, C, Hi, Wi = _obs_recon_operands(a2, w, b, obs, index, coef_word, "obs_recon_fwd_loss")
    dev = a2.device
    dz = torch.empty((N, 4 * Hi + 4, 4 * Wi + 4, C), dtype=torch.float32, device=dev)
    out, db = torch.empty(4, dtype=torch.float32, device=dev), torch.empty(C, dtype=torch.float32, device=dev)
    nbytes = lib.etm_obs_recon_workspace_bytes(N, C, Hi, Wi)
    ws = workspace(nbytes, dev, "obs_recon")
    _lib.check(lib.etm_obs_recon_fwd_loss(_ptr(a2), _ptr(w), _ptr(b), _ptr(x), int(x.dtype == torch.uint8), _ptr(index), x.shape[0], _ptr(coef_word),
                                          _ptr(dz), _ptr(out), _ptr(db), _ptr(ws), nbytes, N, C, Hi, Wi, _stream()), "etm_obs_recon_fwd_loss")
    return dz, out, db


def obs_recon_dgrad(dz, w, a2):
    """etm_obs_recon_dgrad: da2 [N, Hi, Wi, 32] = (a2 > 0) * (the 8 x 8 / 4 convolution of dz with w read as [32, C, 8, 8])."""
    lib = _lib.load()
    _need_dev(dz, w, a2)
    dz, w, a2 = _f32c(dz, "dz"), _f32c(w, "weight"), _f32c(a2, "a2")
    N, Hi, Wi, _ = a2.shape
    C = w.shape[1]
    if tuple(dz.shape) != (N, 4 * Hi + 4, 4 * Wi + 4, C) or a2.shape[3] != 32 or tuple(w.shape) != (32, C, 8, 8):
        raise ValueError(f"obs_recon_dgrad: dz {tuple(dz.shape)}, weight {tuple(w.shape)}, a2 {tuple(a2.shape)} do not belong together")
    da2 = torch.empty_like(a2)
    _lib.check(lib.etm_obs_recon_dgrad(_ptr(dz), _ptr(w), _ptr(a2), _ptr(da2), N, C, Hi, Wi, _stream()), "etm_obs_recon_dgrad")
    return da2


def obs_recon_wgrad(dz, a2):
    """dW [32, C, 8, 8] of the decoder's last layer = the first encoder layer's weight gradient with the roles exchanged:
    etm_conv_train_wgrad(x := dz, dy := a2) (include/etm_hip.h states the identity).  That entry's trailing "bias gradient" -- the
    column sums of a2 -- is discarded."""
    return conv_transpose_wgrad(dz, a2, 8, 4)


class _ObsReconFn(torch.autograd.Function):
    """The decoder's last layer + sigmoid cross-entropy as one node over etm_obs_recon_fwd_loss (forward: the loss AND the gradient
    image dz = coef * dloss / dlogits), etm_obs_recon_dgrad and the reused etm_conv_train_wgrad (backward).  Returns (coef * loss, out
    [4]).  ``unit``: the caller runs backward() on a sum this term enters with weight 1, nothing is scaled."""

    @staticmethod
    def forward(ctx, a2, w, b, obs, index, coef_word, unit):
        dz, out, db = obs_recon_fwd_loss(a2.detach(), w.detach(), b.detach(), obs, coef_word, index)
        ctx.save_for_backward(a2.detach(), w.detach(), dz, db)
        ctx.unit = bool(unit)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(out)
        return out[2].clone(), out

    @staticmethod
    def backward(ctx, g_loss, _g_out):
        if g_loss is None:
            return (None,) * 7
        a2, w, dz, db = ctx.saved_tensors
        if not ctx.unit:
            dz, db = dz * g_loss, db * g_loss
        da2 = obs_recon_dgrad(dz, w, a2) if ctx.needs_input_grad[0] else None
        dw = obs_recon_wgrad(dz, a2) if ctx.needs_input_grad[1] else None
        return da2, dw, (db if ctx.needs_input_grad[2] else None), None, None, None, None


def obs_reconstruction_loss(a2, dec_conv1, obs, coef_word, unit_grad=False, with_out=False):
    """``coef * loss`` of the observation reconstruction: the decoder's last layer ``dec_conv1`` (an nn.ConvTranspose2d(32, C, 8, 4)) on
    ``a2`` NHWC [N, Hi, Wi, 32], the sigmoid cross-entropy of its logits against ``obs`` -- an NHWC tensor [N, Ho, Wo, C], float32 in
    [0, 1] or uint8 (byte k = float32(k) / 255), or an ``IndexedObservations``-like object (``.bank`` NHWC, ``.index`` int64 [N]) whose
    rows the kernel gathers -- times the one float32 of ``coef_word``, read in place (utils.obs_reconstruction_loss is the rule).
    ``unit_grad=True``: the caller runs ``backward()`` on a loss this term enters with weight 1 (the contract of the loss entries).
    ``with_out``: also the node's ``out`` [4] = (loss, coef, coef * loss, 0).  On CPU tensors the same expression in torch."""
    bank, index = (obs.bank, obs.index) if hasattr(obs, "bank") else (obs, None)
    w, b = dec_conv1.weight, dec_conv1.bias
    if a2.is_cuda:
        scaled, out = _ObsReconFn.apply(a2, w, b, bank, index, coef_word, bool(unit_grad))
        return (scaled, out) if with_out else scaled
    t = bank if index is None else bank.index_select(0, index)
    t = t.to(torch.float32) / 255 if t.dtype == torch.uint8 else t
    z = torch.nn.functional.conv_transpose2d(a2.permute(0, 3, 1, 2), w, b, stride=4).permute(0, 2, 3, 1)
    t = t.to(z.dtype)
    loss = (z.clamp_min(0) - z * t + torch.log1p(torch.exp(-z.abs()))).mean()
    coef = coef_word.reshape(()).to(z.dtype)
    scaled = coef * loss
    if with_out:
        return scaled, torch.stack([loss.detach(), coef, scaled.detach(), torch.zeros_like(coef)])
    return scaled
