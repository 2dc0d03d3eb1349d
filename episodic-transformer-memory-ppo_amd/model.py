"""Actor-critic with the episodic-memory transformer (API of upstream model.py:10-166).

``forward(obs, memory, memory_mask, memory_indices)`` keeps the upstream convention (pre-gathered memory windows);
``forward_banked(obs, spec)`` is the trainer's entry: windows are read in place from the episode bank.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.distributions import Categorical, Normal
from torch.nn import functional as F

from etm import ops
from etm import lib as etm_lib
from etm.ops import WindowSpec
from transformer import Transformer
from utils import normalization_section, obs_reconstruction_section, previous_step_input_section, previous_step_table_rows


class PreviousStep:
    """What ``previous_step_input`` feeds back for N samples: ``actions`` [N, B] int64 (the previous step's action of every branch),
    ``rewards`` [N] float32 (its raw reward; None where the key leaves the reward out), and which samples have a previous step at all
    -- ``ep_step`` [N] int64 (the rollout's form: the episode step, 0 at an episode's first step; the actions of such a row are stale
    and not read), or, without it (the buffer's form), a negative entry in column 0 of ``actions``."""

    def __init__(self, actions, rewards=None, ep_step=None):
        self.actions, self.rewards, self.ep_step = actions, rewards, ep_step


def obs_norm_table(stats, epsilon):
    """The frozen fp32 table of a running triple ``stats`` [3, F] float64 (count, mean, M2) -> (mean [F], rstd [F]) float32:
    rstd = 1 / sqrt(M2 / count + epsilon) with the population variance, formed in double and rounded once; the identity (0, 1)
    where count == 0."""
    count, mean, m2 = stats.double().unbind(0)
    seen = count > 0
    var = torch.where(seen, m2 / torch.where(seen, count, torch.ones_like(count)), torch.zeros_like(m2))
    rstd = torch.where(seen, 1.0 / torch.sqrt(var + float(epsilon)), torch.ones_like(var))
    return torch.where(seen, mean, torch.zeros_like(mean)).float(), rstd.float()


class IndexedObservations:
    """A minibatch of visual observations as (all observations of the update in NHWC memory order [n, H, W, C], int64 row
    indices): what ``buffer.samples_flat["obs"][mini_batch_indices]`` (buffer.py:84-91) denotes, without materialising it.  With
    ``normalize_observations`` also vector observations [n, F]: the normalising launch gathers the rows."""

    def __init__(self, bank_nhwc, index):
        self.bank, self.index = bank_nhwc, index


def masked_logits(logits, action_mask):
    """The branches' logits (a list of [N, A_b] tensors) with -inf at the actions that ``action_mask`` does not allow: bool [N, sum A_b]
    (the branches' actions side by side) or the packed int64 / uint64 words [N] of ``environments.pack_action_masks`` (bit j = column j)."""
    total = sum(int(l.shape[1]) for l in logits)
    dev = logits[0].device
    m = action_mask.detach().cpu().numpy() if torch.is_tensor(action_mask) else np.asarray(action_mask)
    if m.dtype != np.bool_:              # packed words, signed or unsigned: the same 64 bits
        words = torch.from_numpy(np.ascontiguousarray(m.reshape(-1)).astype(np.uint64).view(np.int64)).to(dev).reshape(-1, 1)
        valid = ((words >> torch.arange(total, device=dev)) & 1).bool()
    else:
        valid = torch.from_numpy(np.ascontiguousarray(m)).to(dev).reshape(-1, total)
    out, off = [], 0
    for l in logits:
        a = int(l.shape[1])
        out.append(l.masked_fill(~valid[:, off:off + a], float("-inf")))
        off += a
    return out


class ActorCriticModel(nn.Module):
    def __init__(self, config, observation_space, action_space_shape, max_episode_length, continuous=False):
        """``continuous``: a Box action space of A = action_space_shape[0] dimensions -- a diagonal Gaussian policy whose mean is
        ``policy_branches[0]`` and whose state-independent log standard deviation is the parameter ``policy_log_std`` [A]
        (initial value ``action_log_std_init``, default 0)."""
        super().__init__()
        self.hidden_size = config["hidden_layer_size"]
        self.memory_layer_size = config["transformer"]["embed_dim"]
        self.observation_space_shape = tuple(observation_space.shape)
        self.max_episode_length = max_episode_length
        self.visual = len(self.observation_space_shape) > 1
        self.channels_last = True          # visual observations are kept NHWC for the optimisation phase (trainer._observations_channels_last)
        self.fused_encoder = bool(config.get("fused_rollout_encoder", True))
        self.train_encoder = bool(config.get("fused_train_encoder", True))     # False: library convolutions in the optimisation phase
        # round 6: "bf16x3" = the encoder's fp32 products as six bf16 MFMA products of exactly split operands (csrc/conv_b3*.hip; error
        # against float64 below the fp32-MFMA kernels'), "fp32" = the fp32-MFMA kernels of rounds 2 - 3.  Per model, handed to every call.
        self.encoder_products = str(config.get("encoder_products", "bf16x3"))
        if self.encoder_products not in ("bf16x3", "fp32"):
            raise ValueError(f"encoder_products must be 'bf16x3' or 'fp32', got {self.encoder_products!r}")
        self.fused_rollout_block = bool(config.get("fused_rollout_block", True))   # False: one launch per GEMM / LayerNorm / attention
        # round 5: GRU-gated layouts -- the step kernel of a worker GROUP (csrc/rollout_group.hip: workers as the rows of every product,
        # every matrix read once per group and step); False keeps the per-worker teams of csrc/rollout_fused.hip
        self.rollout_group_kernel = bool(config.get("rollout_group_kernel", True))
        self._rf = None
        self._rfg = None
        self._train_encoder_ok = None
        if self.visual:
            c = self.observation_space_shape[0]
            self.conv1 = nn.Conv2d(c, 32, 8, 4)
            self.conv2 = nn.Conv2d(32, 64, 4, 2, 0)
            self.conv3 = nn.Conv2d(64, 64, 3, 1, 0)
            for conv in (self.conv1, self.conv2, self.conv3):
                nn.init.orthogonal_(conv.weight, math.sqrt(2))
            self.conv_out_size = self.get_conv_output(self.observation_space_shape)
            feat = self.conv_out_size
        else:
            feat = self.observation_space_shape[0]
        # normalize_observations (absent upstream): vector observations are standardised with a FROZEN fp32 table in front of lin_hidden,
        # derived from a running float64 triple (count, mean, M2) per feature that the trainer merges once per update.  Triple and table
        # are buffers (they travel in the state dict) and exist only with the key; they are updated in place, never rebound.
        self.obs_norm = normalization_section(config, "normalize_observations")
        if self.obs_norm is not None:
            if self.visual:
                raise ValueError("normalize_observations is for vector observations: image observations are already in [0, 1] "
                                 "(remove the key, or flatten the observation)")
            self.register_buffer("obs_norm_stats", torch.zeros((3, feat), dtype=torch.float64))
            self.register_buffer("obs_norm_mean", torch.zeros(feat, dtype=torch.float32))
            self.register_buffer("obs_norm_rstd", torch.ones(feat, dtype=torch.float32))
        self.lin_hidden = nn.Linear(feat, self.memory_layer_size)
        nn.init.orthogonal_(self.lin_hidden.weight, math.sqrt(2))
        self.transformer = Transformer(config["transformer"], self.memory_layer_size, self.max_episode_length)
        self.lin_policy = nn.Linear(self.memory_layer_size, self.hidden_size)
        nn.init.orthogonal_(self.lin_policy.weight, math.sqrt(2))
        self.lin_value = nn.Linear(self.memory_layer_size, self.hidden_size)
        nn.init.orthogonal_(self.lin_value.weight, math.sqrt(2))
        self.action_space_shape = tuple(int(a) for a in action_space_shape)   # one entry per action branch (MultiDiscrete: nvec)
        self.policy_branches = nn.ModuleList()
        for num_actions in action_space_shape:
            branch = nn.Linear(in_features=self.hidden_size, out_features=num_actions)
            nn.init.orthogonal_(branch.weight, math.sqrt(0.01))
            self.policy_branches.append(branch)
        self.value = nn.Linear(self.hidden_size, 1)
        nn.init.orthogonal_(self.value.weight, 1)
        self.continuous = bool(continuous)
        if self.continuous:
            if len(self.action_space_shape) != 1:
                raise ValueError("a Box policy has one mean head of A outputs: action_space_shape must be (A,)")
            self.policy_log_std = nn.Parameter(torch.full((self.action_space_shape[0],), float(config.get("action_log_std_init", 0.0))))
        # previous_step_input (absent upstream): the previous step's action(s) and raw reward enter lin_hidden's pre-activation through
        # a learned table [R, lin_hidden.out_features] -- branch b owns rows off_b .. off_b + A_b - 1, the reward row is the last
        # (utils.previous_step_rows is the rule).  Zeros at the start: the run begins as the function without the key.  Registered last,
        # so every other parameter keeps its place in the arena; the parameter exists only with the key.
        self.prev_cfg = previous_step_input_section(config, self.action_space_shape, box=self.continuous)
        self.prev_input = None
        if self.prev_cfg is not None:
            self.prev_input = nn.Embedding(previous_step_table_rows(self.action_space_shape, self.prev_cfg["reward"]), self.memory_layer_size)
            nn.init.zeros_(self.prev_input.weight)
        # obs_reconstruction (absent upstream's model.py; the auxiliary loss of its author's Memory Gym runs): a decoder that mirrors the
        # encoder reads h [N, D], the transformer's output, and has to reproduce the current frame (``reconstruct`` + the fused last
        # layer and loss, ops.obs_reconstruction_loss).  Optimisation phase only.  Registered last, behind prev_input, so every other
        # parameter keeps its place in the arena; the four modules exist only with the key.
        self.recon_cfg = obs_reconstruction_section(config, self.observation_space_shape)
        if self.recon_cfg is not None:
            hh, ww = self.observation_space_shape[-2:]
            self._dec_hw3 = (((hh - 8) // 4 + 1 - 4) // 2 + 1 - 2, ((ww - 8) // 4 + 1 - 4) // 2 + 1 - 2)      # the encoder's last feature map
            self.dec_hidden = nn.Linear(self.memory_layer_size, self.conv_out_size)
            self.dec_conv3 = nn.ConvTranspose2d(64, 64, 3, 1)
            self.dec_conv2 = nn.ConvTranspose2d(64, 32, 4, 2)
            self.dec_conv1 = nn.ConvTranspose2d(32, self.observation_space_shape[0], 8, 4)
            for mod in (self.dec_hidden, self.dec_conv3, self.dec_conv2, self.dec_conv1):      # (as the encoder is initialised)
                nn.init.orthogonal_(mod.weight, math.sqrt(2))

    def reconstruct(self, h):
        """``obs_reconstruction``: the decoder up to its last layer's input, h [N, D] (what ``forward_state`` returns) -> a2 NHWC
        [N, h1, w1, 32] (h1, w1: the first encoder layer's output size): dec_hidden + ReLU through the linear node, viewed as the
        encoder's last feature map (NHWC), then the two middle transposed layers on channels_last activations (library convolutions;
        bias + ReLU and their backward by ``ops.conv_transpose_relu``)."""
        if self.recon_cfg is None:
            raise ValueError("reconstruct: this model was built without obs_reconstruction")
        h3, w3 = self._dec_hw3
        x = ops.linear_relu(self.dec_hidden, h).view(h.shape[0], h3, w3, 64).permute(0, 3, 1, 2)
        x = ops.conv_transpose_relu(self.dec_conv3, x)
        x = ops.conv_transpose_relu(self.dec_conv2, x)
        return x.permute(0, 2, 3, 1).contiguous()

    def arena_parameters(self):
        """(name, parameter) pairs in the order of the optimiser's flat arena: ``named_parameters()``, except that a Box policy's
        ``policy_log_std`` -- a parameter of the model itself, which ``named_parameters()`` lists first -- goes last, so that every
        other parameter keeps the arena offset (and the 16-byte alignment the encoder kernels require) it has without it."""
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        return [x for x in named if x[0] != "policy_log_std"] + [x for x in named if x[0] == "policy_log_std"]

    # ------------------------------------------------------------------ forward
    # ------------------------------------------------------------------ rollout encoder (no grad): MFMA conv + bias + ReLU
    def _fused_encoder_ok(self, obs):
        if not (self.visual and self.fused_encoder and obs.is_cuda and not torch.is_grad_enabled()):
            return False
        _, _, hh, ww = obs.shape
        h1, w1 = (hh - 8) // 4 + 1, (ww - 8) // 4 + 1
        return ww % 4 == 0 and obs.shape[1] * 1 >= 1 and h1 >= 4 and w1 >= 4 and ((h1 - 4) // 2 + 1) >= 3 and ((w1 - 4) // 2 + 1) >= 3

    def conv2_output_hw(self):
        """Spatial size of the encoder's activations after conv1 and conv2 (the input of conv3)."""
        h, w = self.observation_space_shape[-2:]
        for cv in (self.conv1, self.conv2):
            h, w = (h - cv.kernel_size[0]) // cv.stride[0] + 1, (w - cv.kernel_size[1]) // cv.stride[1] + 1
        return h, w

    def refresh_rollout_weights(self):
        """(Re)build the weight copies / packings the rollout kernels read.  Buffers keep their address (the captured rollout graph
        reads them); called by the trainer at the start of every rollout and lazily whenever a weight's version counter moved.
        Round 6: dozens of small launches (2.3 ms per update for the gated layouts) -- from its third call on a graph replay when the
        trainer set ``graph_refresh`` (ops.ReplayAfterWarmup); the version bookkeeping follows every execution."""
        r = getattr(self, "_refresh_replay", None)
        if r is None:
            r = self._refresh_replay = ops.ReplayAfterWarmup(self._refresh_rollout_weights_now, self.lin_policy.weight.device,
                                                             after=self._mark_weight_versions, enabled=bool(getattr(self, "graph_refresh", False)),
                                                             what="refresh_rollout_weights")
        r.enabled = bool(getattr(self, "graph_refresh", False)) and r.device == self.lin_policy.weight.device
        r()

    def _mark_weight_versions(self):
        for mod in self.modules():
            if mod is not self and hasattr(mod, "_versions"):
                mod._wver = mod._versions()
        if self.visual:
            self._wver = (self.conv1.weight._version, self.conv2.weight._version, self.conv3.weight._version)

    def _refresh_rollout_weights_now(self):
        for mod in self.modules():
            if mod is not self and hasattr(mod, "refresh_rollout_weights"):
                mod.refresh_rollout_weights()
        with torch.no_grad():
            # concatenated hidden heads [lin_policy ; lin_value]: fixed-address copies read by the captured rollout graph
            w = torch.cat((self.lin_policy.weight, self.lin_value.weight), dim=0)
            b = torch.cat((self.lin_policy.bias, self.lin_value.bias), dim=0)
            if getattr(self, "_w_heads", None) is None or self._w_heads.device != w.device:
                self._w_heads, self._b_heads = w.contiguous(), b.contiguous()
                self._heads_lin = type("HeadsLinear", (), {})()
                self._heads_lin.weight, self._heads_lin.bias = self._w_heads, self._b_heads
            else:
                self._w_heads.copy_(w)
                self._b_heads.copy_(b)
            if len(self.policy_branches) > 1:
                # MultiDiscrete: the branches' heads concatenated [sum A_b, hid] -- the one policy head the rollout kernels read
                # (branch b owns rows [off_b, off_b + A_b)); fixed address, like the copies above
                wp = torch.cat([br.weight for br in self.policy_branches], dim=0)
                bp = torch.cat([br.bias for br in self.policy_branches], dim=0)
                cat = getattr(self, "_policy_cat", None)
                if cat is None or cat.weight.device != wp.device:
                    self._policy_cat = type("PolicyHeads", (), {})()
                    self._policy_cat.weight, self._policy_cat.bias = wp.contiguous(), bp.contiguous()
                else:
                    cat.weight.copy_(wp)
                    cat.bias.copy_(bp)
        self._refresh_fused_block_weights()
        if not self.visual:
            return
        with torch.no_grad():
            # encoder weights in the K order of each layer's input layout (layer 1 reads NCHW: native order; layers 2, 3 read
            # NHWC: (ky, kx, c)), packed in MFMA fragment order (ops.conv_pack_weights)
            for name, conv, nhwc in (("_w1p", self.conv1, False), ("_w2p", self.conv2, True), ("_w3p", self.conv3, True)):
                w4 = conv.weight.permute(0, 2, 3, 1) if nhwc else conv.weight
                perm = ops.conv_pack_weights(w4.reshape(conv.out_channels, -1))
                buf = getattr(self, name, None)
                if buf is None or buf.shape != perm.shape or buf.device != perm.device:
                    setattr(self, name, perm.contiguous())
                else:
                    buf.copy_(perm)
            # the last layer as [(ky, kx, c), co]: what the fused conv3 + lin_hidden launch of a rollout step reads (ops.rollout_conv3_hidden)
            w3k = self.conv3.weight.permute(2, 3, 1, 0).reshape(-1, self.conv3.out_channels)
            if getattr(self, "_w3k", None) is None or self._w3k.shape != w3k.shape or self._w3k.device != w3k.device:
                self._w3k = w3k.contiguous()
            else:
                self._w3k.copy_(w3k)
            self._wver = (self.conv1.weight._version, self.conv2.weight._version, self.conv3.weight._version)

    def rollout_policy_head(self):
        """The policy head the rollout kernels read: the branch itself for one branch, else the concatenated fixed-address copy of
        all branches (built by ``refresh_rollout_weights``)."""
        return self.policy_branches[0] if len(self.policy_branches) == 1 else getattr(self, "_policy_cat", None)

    def rollout_block_fusable(self):
        """Post- or pre-LN blocks, shapes inside etm_rollout_trxl's support (the branches' actions together): the trainer may run
        the transformer, the heads and the sampling of a rollout step as one kernel."""
        t = self.transformer
        blk = t.transformer_blocks[0]
        d = t.embed_dim
        if not (self.fused_rollout_block and blk.layer_norm in ("post", "pre") and t.linear_embedding.in_features == d):
            return False
        return ops.rollout_trxl_supported(d, t.num_heads, t.config["memory_length"], self.hidden_size,
                                          self._rollout_actions(), t.num_blocks, gaussian=self.continuous)

    def _rollout_actions(self):
        """Number of actions (one branch) or the branch sizes (MultiDiscrete): what the kernels' predicates take."""
        return self.policy_branches[0].out_features if len(self.policy_branches) == 1 else self.action_space_shape

    def _refresh_fused_block_weights(self):
        """Transposed ([in, out]) fixed-address copies of the matrices etm_rollout_trxl walks, and the host table of their
        device pointers (built once: the buffers keep their addresses, so captured graphs stay valid)."""
        if not self.lin_policy.weight.is_cuda or not self.rollout_block_fusable():
            self._rf = self._rfg = None
            return
        import ctypes
        t = self.transformer
        d = t.embed_dim
        team = etm_lib.load().etm_rollout_trxl_team(t.num_heads)
        merged = bool(etm_lib.load().etm_rollout_trxl_gate_merged(d, t.num_heads))

        def blocked(w_t):
            """[K, OUT] (transposed weight) -> member-blocked [P, K, OUT / P]: a team member's columns as one contiguous run."""
            k, out = w_t.shape
            return w_t.reshape(k, team, out // team).permute(1, 0, 2)

        with torch.no_grad():
            fresh = {"emb_t": blocked(t.linear_embedding.weight.t()),
                     "heads_t": blocked(torch.cat((self.lin_policy.weight, self.lin_value.weight), dim=0).t())}
            for i, blk in enumerate(t.transformer_blocks):
                fresh[f"wq_t{i}"] = blocked(blk.attention.queries.weight.t())
                fresh[f"wo_t{i}"] = blk.attention.fc_out.weight.t()          # K-split product: rows of a member are contiguous as they are
                fresh[f"wfc_t{i}"] = blocked(blk.fc[0].weight.t())
                if blk.use_gtrxl:    # GRU gates: [Wr | Wz | Wg]^T and [Ur | Uz]^T member-blocked, packed as the kernel expects for this shape
                    for gi, gate in ((1, blk.gate1), (2, blk.gate2)):
                        for key, names in (("wy", ("Wr", "Wz", "Wg")), ("ux", ("Ur", "Uz"))):
                            parts = torch.stack([blocked(getattr(gate, n).weight.t()) for n in names], dim=1)     # [P, j, D, DS]
                            fresh[f"g{gi}{key}_t{i}"] = parts.permute(0, 2, 1, 3) if merged else parts            # merged: [P, D, j, DS]
                        fresh[f"g{gi}ug_t{i}"] = blocked(gate.Ug.weight.t())
            if self.visual and self.lin_hidden.weight.shape[0] % 32 == 0:
                fresh["hid_t"] = self.lin_hidden.weight.t()     # [features, D]: etm_rollout_hidden_partial
            rf = getattr(self, "_rf", None)
            if rf is None or rf["emb_t"].device != self.lin_policy.weight.device:
                rf = {k: v.contiguous() for k, v in fresh.items()}
                rf["emb_b"], rf["heads_b"] = t.linear_embedding.bias, None
                ptrs = []
                for i, blk in enumerate(t.transformer_blocks):       # 19 pointers per block (include/etm_hip.h, etm_rollout_trxl)
                    ptrs += [rf[f"wq_t{i}"], rf[f"wo_t{i}"], blk.attention.fc_out.bias, blk.norm1.weight, blk.norm1.bias,
                             rf[f"wfc_t{i}"], blk.fc[0].bias, blk.norm2.weight, blk.norm2.bias]
                    for gi, gname in ((1, "gate1"), (2, "gate2")):
                        if blk.use_gtrxl:
                            ptrs += [rf[f"g{gi}wy_t{i}"], rf[f"g{gi}ux_t{i}"], rf[f"g{gi}ug_t{i}"], getattr(blk, gname).bg]
                        else:
                            ptrs += [None] * 4
                    ptrs += [blk.norm_kv.weight, blk.norm_kv.bias] if blk.layer_norm == "pre" else [None, None]
                rf["_keep"] = ptrs
                rf["blocks"] = (ctypes.c_void_p * len(ptrs))(*[None if p is None else p.data_ptr() for p in ptrs])
                rf["nb"], rf["H"], rf["eps"] = t.num_blocks, t.num_heads, t.transformer_blocks[0].norm1.eps
                rf["pre_ln"], rf["gtrxl"] = int(t.transformer_blocks[0].layer_norm == "pre"), int(t.transformer_blocks[0].use_gtrxl)
                self._rf = rf
            else:
                for k, v in fresh.items():
                    rf[k].copy_(v)
            self._rf["heads_b"] = self._b_heads          # concatenated hidden-head bias (refreshed above)
        self._refresh_group_block_weights()

    def _refresh_group_block_weights(self):
        """The packings etm_rollout_trxl_group reads (csrc/rollout_group.hip; GRU-gated blocks, groups of <= 8 workers): every
        [in, out] map transposed and COLUMN-BLOCKED over the launch's 32 workgroups -- [32][in][out / 32], a workgroup's slice of a
        map is one contiguous run --, the gates' maps of y / of x as [32][3][D][D / 32] / [32][2][D][D / 32], the hidden heads as
        [32][NCH][D][CH].  Fixed-address copies next to ``_rf`` (captured graphs read them); ``_rfg`` is None when the shape is not
        the group kernel's (the per-worker kernel then runs the gated layout as before)."""
        import ctypes
        t = self.transformer
        blk0 = t.transformer_blocks[0]
        d = t.embed_dim
        lib = etm_lib.load()
        A = sum(self.action_space_shape)
        # (the kernel's [W, D] input rows and its D x D embedding slice assume linear_embedding.in_features == embed_dim)
        if not (self.rollout_group_kernel and self._rf is not None and blk0.use_gtrxl and t.linear_embedding.in_features == d
                and lib.etm_rollout_trxl_group_supported(d, t.num_heads, t.config["memory_length"], self.hidden_size, A, t.num_blocks, 1, 1)
                and lib.etm_rollout_trxl_team(t.num_heads) == t.num_heads):
            self._rfg = None
            return
        WG = lib.etm_rollout_trxl_group_grid()

        def colblock(w_t):
            """[K, OUT] (transposed weight) -> [32][K][OUT / 32]"""
            k, out = w_t.shape
            return w_t.reshape(k, WG, out // WG).permute(1, 0, 2)

        cbh = 2 * self.hidden_size // WG
        nch = (cbh + 15) // 16
        with torch.no_grad():
            heads_t = torch.cat((self.lin_policy.weight, self.lin_value.weight), dim=0).t()               # [D, 2 hid]
            fresh = {"emb_t": colblock(t.linear_embedding.weight.t()),
                     "heads_t": heads_t.reshape(d, WG, nch, cbh // nch).permute(1, 2, 0, 3)}              # [32][NCH][D][CH]
            for i, blk in enumerate(t.transformer_blocks):
                fresh[f"wq_t{i}"] = colblock(blk.attention.queries.weight.t())
                fresh[f"wo_t{i}"] = colblock(blk.attention.fc_out.weight.t())
                fresh[f"wfc_t{i}"] = colblock(blk.fc[0].weight.t())
                # the first gate's maps of y read a = fc_out(ctx) and nothing else does: W a = (W Wo) ctx + W bo.  Folded here, in
                # float64, once per refresh; the kernel multiplies the context rows with the folded maps and adds the folded bias rows
                # (one product and one all-gather fewer per block)
                wo64, bo64 = blk.attention.fc_out.weight.double(), blk.attention.fc_out.bias.double()
                for gi, gate in ((1, blk.gate1), (2, blk.gate2)):
                    maps = [getattr(gate, n).weight for n in ("Wr", "Wz", "Wg")]
                    if gi == 1:
                        folded = torch.stack([colblock((m.double() @ wo64).float().t()) for m in maps], dim=1)          # [32][3][D][CB]
                        bias = torch.stack([(m.double() @ bo64).float() for m in maps])                               # [3][D]
                        fresh[f"g{gi}wy_t{i}"] = torch.cat((folded.reshape(-1), bias.reshape(-1)))
                    else:
                        fresh[f"g{gi}wy_t{i}"] = torch.stack([colblock(m.t()) for m in maps], dim=1)
                    fresh[f"g{gi}ux_t{i}"] = torch.stack([colblock(getattr(gate, n).weight.t()) for n in ("Ur", "Uz")], dim=1)
                    fresh[f"g{gi}ug_t{i}"] = colblock(gate.Ug.weight.t())
            rg = getattr(self, "_rfg", None)
            if rg is None or rg["emb_t"].device != self.lin_policy.weight.device:
                rg = {k: v.contiguous() for k, v in fresh.items()}
                rg["emb_b"] = t.linear_embedding.bias
                ptrs = []
                for i, blk in enumerate(t.transformer_blocks):       # the 19 pointers per block of etm_rollout_trxl, group packings
                    ptrs += [rg[f"wq_t{i}"], rg[f"wo_t{i}"], blk.attention.fc_out.bias, blk.norm1.weight, blk.norm1.bias,
                             rg[f"wfc_t{i}"], blk.fc[0].bias, blk.norm2.weight, blk.norm2.bias]
                    for gi, gname in ((1, "gate1"), (2, "gate2")):
                        ptrs += [rg[f"g{gi}wy_t{i}"], rg[f"g{gi}ux_t{i}"], rg[f"g{gi}ug_t{i}"], getattr(blk, gname).bg]
                    ptrs += [blk.norm_kv.weight, blk.norm_kv.bias] if blk.layer_norm == "pre" else [None, None]
                rg["_keep"] = ptrs
                rg["blocks"] = (ctypes.c_void_p * len(ptrs))(*[None if q is None else q.data_ptr() for q in ptrs])
                rg["nb"], rg["H"], rg["eps"], rg["D"] = t.num_blocks, t.num_heads, blk0.norm1.eps, d
                rg["pre_ln"], rg["gtrxl"], rg["group"] = int(blk0.layer_norm == "pre"), 1, True
                self._rfg = rg
            else:
                for k, v in fresh.items():
                    rg[k].copy_(v)
            self._rfg["heads_b"] = self._b_heads
            if "hid_t" in self._rf:
                self._rfg["hid_t"] = self._rf["hid_t"]

    def _prev_addend(self, prev):
        """``previous_step_input``: e + lin_hidden.bias [N, D] for the samples of ``prev`` (a PreviousStep) -- on the device the rows
        kernel (under autograd: the node over the rows and the gradient kernel), on a CPU tensor the same expression in torch."""
        if prev is None:
            raise ValueError("previous_step_input: this model was built with the key and needs the previous step on every pass "
                             "(prev=PreviousStep(actions, rewards, ep_step)); there is no pass without it")
        table, bias = self.prev_input.weight, self.lin_hidden.bias
        sizes = self.action_space_shape if self.prev_cfg["action"] else ()
        rewards = prev.rewards if self.prev_cfg["reward"] else None
        if self.prev_cfg["reward"] and rewards is None:
            raise ValueError("previous_step_input: reward: true needs PreviousStep.rewards")
        actions = prev.actions if prev.actions is None or prev.actions.dim() == 2 else prev.actions.reshape(prev.actions.shape[0], -1)
        if table.is_cuda:
            if torch.is_grad_enabled():
                if prev.ep_step is not None:      # (the rollout's form under autograd: rewritten into the buffer's form)
                    has = prev.ep_step != 0
                    actions = None if actions is None else torch.where(has.unsqueeze(1), actions, torch.full_like(actions, -1))
                    rewards = None if rewards is None else torch.where(has, rewards, torch.zeros_like(rewards))
                return ops.prev_input_addend(table, actions, sizes, rewards, bias=bias)
            return ops.prev_input_rows(table, actions, sizes, rewards, ep_step=prev.ep_step, bias=bias)
        n = actions.shape[0] if sizes else rewards.shape[0]
        has = torch.ones(n, dtype=torch.bool) if not sizes else actions[:, 0] >= 0
        if prev.ep_step is not None:
            has = prev.ep_step != 0
        e, off = torch.zeros((n, table.shape[1]), dtype=table.dtype), 0
        for b, size in enumerate(sizes):
            e = e + table[off + actions[:, b].clamp(0, size - 1)]
            off += size
        if rewards is not None:
            e = e + rewards.to(table.dtype).unsqueeze(1) * table[-1]
        return torch.where(has.unsqueeze(1), e, torch.zeros_like(e)) + bias

    def _hidden(self, x, prev=None):
        """lin_hidden on the encoder's features ``x`` [N, F]: relu(x W^T + b), or, with ``previous_step_input``, relu(x W^T + e + b)."""
        if self.prev_input is None:
            if prev is not None:
                raise ValueError("a previous step was handed to a model built without previous_step_input")
            return ops.linear_relu(self.lin_hidden, x)
        addend = self._prev_addend(prev)
        if x.is_cuda and torch.is_grad_enabled() and x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous():
            return ops.linear_relu_train(x, self.lin_hidden.weight, self.lin_hidden.bias, addend=addend)
        return torch.relu(torch.addmm(addend, x, self.lin_hidden.weight.t()))

    def rollout_features(self, obs, obs_index=None, obs_rows=None):
        """What lin_hidden reads in a no-grad rollout step, [N, F] float32 -- the (normalised) vector observation, or the fused
        encoder's features -- for a caller that forms x W^T itself (the step kernel's two-slice input with ``previous_step_input``);
        None where only ``_encode``'s road builds them (library convolutions)."""
        if self.obs_norm is not None:
            return self.normalize_observations(obs)
        if not self.visual:
            return obs if obs.dtype == torch.float32 and obs.dim() == 2 else None
        if obs_index is not None or self._fused_encoder_ok(obs):
            return self._encode_fused(obs, obs_index, obs_rows, features_only=True)
        return None

    def _hidden_nhwc(self, feats, prev=None):
        """``_hidden`` for the NHWC-flattened features of the training encoder (ops.linear_relu_nhwc)."""
        if self.prev_input is None:
            if prev is not None:
                raise ValueError("a previous step was handed to a model built without previous_step_input")
            return ops.linear_relu_nhwc(feats, self.lin_hidden.weight, self.lin_hidden.bias, self.conv3.out_channels)
        return ops.linear_relu_nhwc(feats, self.lin_hidden.weight, self.lin_hidden.bias, self.conv3.out_channels, addend=self._prev_addend(prev))

    def _encode_fused(self, obs, obs_index=None, obs_rows=None, features_only=False, prev=None):
        if getattr(self, "_w2p", None) is None or (not torch.cuda.is_current_stream_capturing()
                                                     and self._wver != (self.conv1.weight._version, self.conv2.weight._version,
                                                                        self.conv3.weight._version)):
            self.refresh_rollout_weights()
        n, c, hh, ww = obs.shape[-4:]      # with obs_index: obs is a stack [S, N, C, H, W] and the layer reads obs[obs_index]
        if obs_rows is not None:
            n = obs_rows[1] - obs_rows[0]
        x = ops.conv_relu(obs, self._w1p, self.conv1.bias, c, hh, ww, 8, 8, 4, False, False, index=obs_index, rows=obs_rows)  # -> NHWC
        h1, w1 = x.shape[1], x.shape[2]
        x = ops.conv_relu(x, self._w2p, self.conv2.bias, 32, h1, w1, 4, 4, 2, True, False)
        h2, w2 = x.shape[1], x.shape[2]
        if features_only == "conv2":          # the caller runs the last layer together with lin_hidden (ops.rollout_conv3_hidden)
            return x
        x = ops.conv_relu(x, self._w3p, self.conv3.bias, 64, h2, w2, 3, 3, 1, True, True)                                # -> NCHW
        if features_only:
            return x.reshape(n, -1)
        return self._hidden(x.reshape(n, -1), prev)

    def _encode(self, obs, obs_index=None, obs_rows=None, prev=None):
        """Observation encoder.  ``obs_index`` (int64 device scalar, fused rollout encoder only): ``obs`` is a time-major
        stack [S, N, C, H, W] and row obs[obs_index] is encoded (the row is selected on the device).  ``obs`` may be an
        ``IndexedObservations(bank_nhwc, index)``: the minibatch = bank_nhwc[index], gathered inside the first encoder layer.
        Visual observations may be uint8 on every entry: byte k stands for float32(k) / float32(255).  On the device the first
        layer's kernels read the bytes where they have a byte form (ops.conv_relu, ops.encoder_train) and ``ops.bytes_to_unit``
        expands them elsewhere; on the CPU it is ``obs.to(torch.float32) / 255``."""
        raw = obs.bank if isinstance(obs, IndexedObservations) else obs
        if self.obs_norm is not None:
            if raw.dtype != torch.float32:
                raise ValueError("normalize_observations: a vector observation must be float32")
            if obs_index is not None:
                raise RuntimeError("obs_index needs the fused rollout encoder (visual observations, no grad)")
            return self._hidden(self.normalize_observations(obs), prev)
        if raw.dtype == torch.uint8:
            if not self.visual:
                raise ValueError("uint8 observations are images (byte k = k / 255); a vector observation must be float32")
            if not raw.is_cuda:      # (IEEE division: the correctly rounded quotient)
                if isinstance(obs, IndexedObservations):
                    obs = IndexedObservations(obs.bank.index_select(0, obs.index).to(torch.float32) / 255, torch.arange(obs.index.numel()))
                else:
                    obs = obs.to(torch.float32) / 255
        if isinstance(obs, IndexedObservations):
            if self.visual and self.train_encoder and torch.is_grad_enabled():
                if self._train_encoder_ok is None:
                    self._train_encoder_ok = ops.encoder_train_supported(self.observation_space_shape, (self.conv1, self.conv2, self.conv3))
                if self._train_encoder_ok and ops.encoder_train_supported(self.observation_space_shape, (self.conv1, self.conv2, self.conv3),
                                                                            batch=int(obs.index.numel()), bank=int(obs.bank.shape[0]),
                                                                            products=self.encoder_products):
                    feats = ops.encoder_train(obs.bank, self.conv1, self.conv2, self.conv3, index=obs.index, products=self.encoder_products)
                    if getattr(self, "_keep_encoder_features", False):      # data-parallel overlap: the backward pass is cut here
                        self._encoder_features = feats                      # (trainer._train_body_a1; released by _train_body_a2)
                    return self._hidden_nhwc(feats, prev)
            if obs.bank.dtype == torch.uint8:      # (device: the gather rides in the expansion)
                obs = ops.bytes_to_unit(obs.bank, index=obs.index).permute(0, 3, 1, 2)
            else:
                obs = obs.bank.index_select(0, obs.index).permute(0, 3, 1, 2)      # NCHW view of the gathered NHWC rows
        if obs_index is not None:
            if not self._fused_encoder_ok(obs[0]):
                raise RuntimeError("obs_index needs the fused rollout encoder (visual observations, no grad)")
            return self._encode_fused(obs, obs_index, obs_rows, prev=prev)
        h = obs
        if self._fused_encoder_ok(obs):
            return self._encode_fused(obs, prev=prev)
        if self.visual and self.train_encoder and obs.is_cuda and torch.is_grad_enabled() and obs.dim() == 4:
            if self._train_encoder_ok is None:
                self._train_encoder_ok = ops.encoder_train_supported(self.observation_space_shape, (self.conv1, self.conv2, self.conv3))
            if self._train_encoder_ok and ops.encoder_train_supported(self.observation_space_shape, (self.conv1, self.conv2, self.conv3),
                                                                        batch=int(obs.shape[0])):
                # optimisation phase: the three relu(conv2d) layers forward and backward on the hand-written MFMA kernels
                # (NHWC activations; the trainer hands over an NCHW view of NHWC memory, which permutes back for free)
                feats = ops.encoder_train(obs.permute(0, 2, 3, 1), self.conv1, self.conv2, self.conv3, products=self.encoder_products)      # (h, w, c) flatten order
                return self._hidden_nhwc(feats, prev)
        if self.visual:
            if h.dtype == torch.uint8:      # library convolutions: the floats first (in the memory order the bytes have)
                nhwc = h.permute(0, 2, 3, 1)
                h = ops.bytes_to_unit(nhwc).permute(0, 3, 1, 2) if nhwc.is_contiguous() else ops.bytes_to_unit(h)
            if self.channels_last and h.is_cuda:
                # NHWC activations: MIOpen's implicit-GEMM kernels run without layout transposes (1.35 vs 2.1 ms for
                # forward+backward of the three convolutions at N = 2048); weights, logical shapes and state_dict are unchanged
                h = h.contiguous(memory_format=torch.channels_last)
            h = F.relu(self.conv1(h))
            h = F.relu(self.conv2(h))
            h = F.relu(self.conv3(h))
            h = h.reshape(h.shape[0], -1)
        return self._hidden(h, prev)

    def normalize_observations(self, obs):
        """clamp((obs - mean) * rstd, -clip, +clip) in fp32 with the frozen table, subtraction and product rounded separately: the one
        place every pass through the encoder standardises a vector observation (rollout step, get_last_value, the truncation
        bootstrap, the training forward, evaluation, enjoy.py).  On the device one launch (ops.obs_normalize; the rows of an
        ``IndexedObservations`` are gathered by it), on a CPU tensor the same expression in torch."""
        index = None
        if isinstance(obs, IndexedObservations):
            obs, index = obs.bank, obs.index
        clip = self.obs_norm["clip"]
        if obs.is_cuda:
            return ops.obs_normalize(obs, self.obs_norm_mean, self.obs_norm_rstd, clip, index=index)
        if index is not None:
            obs = obs.index_select(0, index)
        return torch.clamp((obs - self.obs_norm_mean) * self.obs_norm_rstd, -clip, clip)

    def refresh_obs_norm_table(self):
        """The table from the triple, in place (after the triple was set by hand or loaded without its table)."""
        mean, rstd = obs_norm_table(self.obs_norm_stats, self.obs_norm["epsilon"])
        with torch.no_grad():
            self.obs_norm_mean.copy_(mean)
            self.obs_norm_rstd.copy_(rstd)

    def forward_state(self, obs, spec: WindowSpec, want_items=False, prev=None):
        """Encoder + transformer: -> (h [N, D] in front of the hidden heads (model.py:100), new memory items or None)."""
        return self.transformer.forward_window(self._encode(obs, prev=prev), spec, want_items)

    def forward_logits(self, obs, spec: WindowSpec, want_items=True, prev=None):
        """-> (list of raw logits per branch, value [N], new memory items [N, blocks, D] or None).  ``prev``: the samples'
        PreviousStep, with ``previous_step_input`` (every entry below takes it and hands it to the encoder)."""
        h, memory = self.transformer.forward_window(self._encode(obs, prev=prev), spec, want_items)
        h_policy = ops.linear_relu(self.lin_policy, h)
        h_value = ops.linear_relu(self.lin_value, h)
        value = self.value(h_value).reshape(-1)
        return [branch(h_policy) for branch in self.policy_branches], value, memory

    def rollout_heads_fusable(self):
        """Concatenated hidden heads (and, with several branches, policy heads) built: the trainer may run output heads + sampling
        as one kernel on ``forward_hidden_cached``'s result."""
        return (getattr(self, "_w_heads", None) is not None and self.rollout_policy_head() is not None
                and not torch.is_grad_enabled())

    def forward_hidden_cached(self, obs, kv_spec: WindowSpec, items_out=None, obs_index=None, raw=False, obs_rows=None, prev=None):
        """Rollout path up to the hidden heads: -> (h2 [N, 2*hidden] = [relu(lin_policy(h)) | relu(lin_value(h))], memory).
        ``raw=True``: h2 are the PRE-activations (plain GEMM without epilogue); the caller applies relu(h2 + self._b_heads)
        (``ops.rollout_policy(h_bias=...)`` does it on the fly)."""
        h, memory = self.transformer.forward_cached(self._encode(obs, obs_index, obs_rows, prev=prev), kv_spec, items_out)
        if raw:
            return F.linear(h, self._w_heads), memory
        return ops.linear_relu(self._heads_lin, h), memory

    def forward_logits_cached(self, obs, kv_spec: WindowSpec, items_out=None, obs_index=None, obs_rows=None, prev=None):
        """Rollout path (no grad): like ``forward_logits`` but attention reads the per-worker K/V cache.  With ``items_out``
        [blocks, N, D] the new memory items are written there (block-major) and returned in that layout."""
        h, memory = self.transformer.forward_cached(self._encode(obs, obs_index, obs_rows, prev=prev), kv_spec, items_out)
        if self.rollout_heads_fusable():
            # [lin_policy ; lin_value] as ONE GEMM (+ReLU epilogue), then both output heads in one small kernel (several branches:
            # the concatenated policy heads, the logits split into the branches' column views)
            h2 = ops.linear_relu(self._heads_lin, h)
            logits, value = ops.rollout_heads(h2, self.rollout_policy_head(), self.value)
            if len(self.policy_branches) == 1:
                return [logits], value, memory
            return list(logits.split(list(self.action_space_shape), dim=1)), value, memory
        h_policy = ops.linear_relu(self.lin_policy, h)
        h_value = ops.linear_relu(self.lin_value, h)
        value = self.value(h_value).reshape(-1)
        return [branch(h_policy) for branch in self.policy_branches], value, memory

    def forward_banked(self, obs, spec: WindowSpec, action_mask=None, prev=None):
        """``action_mask`` (optional, categorical policies): invalid-action masks of the N samples, bool [N, sum A_b] (the branches'
        actions side by side, sb3-contrib's ``action_masks()`` layout) or the packed int64 / uint64 words [N]
        (``environments.pack_action_masks``): the logits of the invalid actions are -inf in the returned distributions."""
        if self.continuous and action_mask is not None:
            raise ValueError("a Box policy has no action mask")
        logits, value, memory = self.forward_logits(obs, spec, prev=prev)
        if self.continuous:        # Box: [Normal(mean, exp(policy_log_std))]
            return [Normal(logits[0], self.policy_log_std.exp().expand_as(logits[0]), validate_args=False)], value, memory
        if action_mask is not None:
            logits = masked_logits(logits, action_mask)
        return [Categorical(logits=l, validate_args=False) for l in logits], value, memory

    def forward(self, obs, memory, memory_mask, memory_indices, action_mask=None, prev=None):
        """Upstream signature; memory [N, L, blocks, D] is the pre-gathered window.  ``action_mask``: see ``forward_banked``."""
        return self.forward_banked(obs, WindowSpec.from_windows(memory, memory_indices, memory_mask), action_mask=action_mask, prev=prev)

    def get_conv_output(self, shape) -> int:
        with torch.no_grad():
            o = self.conv3(self.conv2(self.conv1(torch.zeros(1, *shape))))
        return int(np.prod(o.size()))

    # ------------------------------------------------------------------ gradient monitoring (keys of upstream :128-151)
    def _grad_groups(self):
        groups = {}
        if self.visual:
            groups["encoder"] = [self.conv1, self.conv2, self.conv3]
        groups["linear_layer"] = [self.lin_hidden] if self.prev_input is None else [self.lin_hidden, self.prev_input]
        for i, block in enumerate(self.transformer.transformer_blocks):
            groups["transformer_block_" + str(i)] = [block]
        for i, head in enumerate(self.policy_branches):
            groups["policy_head_" + str(i)] = [head]
        groups["lin_policy"] = [self.lin_policy]
        groups["value"] = [self.lin_value, self.value]
        if self.recon_cfg is not None:
            groups["decoder"] = [self.dec_hidden, self.dec_conv3, self.dec_conv2, self.dec_conv1]
        groups["model"] = [self, self.value]
        return groups

    def grad_norms_device(self):
        """{key: 0-dim device tensor}: no host synchronisation (the trainer syncs once per update)."""
        out = {}
        for key, modules in self._grad_groups().items():
            grads = [p.grad.reshape(-1) for m in modules for p in m.parameters() if p.grad is not None]
            out[key] = torch.linalg.norm(torch.cat(grads)) if grads else None
        return out

    def get_grad_norm(self):
        return {k: (v.item() if v is not None else None) for k, v in self.grad_norms_device().items()}
