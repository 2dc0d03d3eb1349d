"""-m gpu: the convolution encoder (model.py:29-31 / :90-92) at every admitted geometry against float64.

Training: ``ops.encoder_train`` forward and backward through the public op -- the bf16x3 kernels (csrc/conv_b3.hip,
conv_b3_wgrad.hip) at the one geometry they take, the fp32-MFMA kernels everywhere else (csrc/conv_train.hip
``conv_gemm_kernel<MT, NT, DGRAD, CLS, BLDS, EVEN>`` / ``conv_wgrad_kernel<KT, CT>`` and the LDS-resident forms
conv_fwd_lds.hip, conv_dgrad_lds.hip, conv_wgrad_lds.hip).  Each case runs the plain NHWC input, the fused minibatch gather
(``index=`` into a larger bank, bit-identical to the plain run on ``bank[index]``) and the DeferredDw hand-off (bit-identical
gradients), then every layer's backward-data through the C ABI.  Rollout: ``model._encode_fused`` (three ``etm_conv_relu``
launches, csrc/conv_encoder.hip ``conv_relu_kernel<NT, GB>``) and ``ops.rollout_conv3_hidden`` where it is supported.

The functions below restate the host dispatch of those launches; the case matrix is chosen from them, and
``test_encoder_matrix_covers_every_reachable_launch`` sweeps the restatement over the admitted geometries and batch sizes: every
launch it can reach is hit by a case, and every compiled form it cannot reach is named with the reason.

Inputs mix uniform, all-zero, constant and 0 - 255 integer-valued (unnormalised) images; some channels have biases that kill them
for whole images, so exact zeros reach the ReLU masks.  The reference is float64 on the same fp32 weights and inputs: the whole
batch on the device (``F.unfold`` + ``einsum`` / ``F.fold``, chunked over images), cross-checked against host ``F.conv2d`` on the
first, last, middle and 2^23-crossing images.  Measures: normwise relative error per tensor (``nrm``) and the worst per-image
(features, dx) or per-output-channel (dW) ``max |err| / max |ref|`` (``pix``), so that one wrong tile cannot hide in a large norm.
"""
import itertools
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CAP = {"fp32": 1e-6, "bf16x3": 3e-7, "rollout": 1e-6}          # normwise caps (fp32-MFMA 1.9 - 4.6e-7, bf16x3 at most that)
# About 4x the worst error measured over the whole matrix on the MI355X (second column: worst, and the case; every case's inputs and
# parameters come from its own seed, and repeated runs measure the same values), within the caps.  Bias gradients are plain fp32
# column sums in both product forms: fp32's cap.  "@2^24": weight / bias gradients of the two cases with over 2^23 first-layer
# pixels (N = 41,943), sums of 16.8 M random-sign terms whose cancellation grows the relative error like sqrt(pixels): no cap.
# dw/pix compares a channel's worst element with its largest, so a channel whose gradient cancels to a small result measures more.
BOUNDS = {
    ("fp32", "feat", "nrm"): 1.0e-6,            # 6.0e-7  8x84_n7 (4x would pass the cap)
    ("fp32", "feat", "pix"): 6.0e-6,            # 1.5e-6  3x84_fp32_n2048
    ("fp32", "dw", "nrm"): 1.0e-6,              # 6.9e-7  3x84_fp32_n2675/L1 (4x would pass the cap)
    ("fp32", "dw", "pix"): 3.9e-5,              # 9.8e-6  4x84_n601/L2
    ("fp32", "db", "nrm"): 1.0e-6,              # 5.6e-7  4x84_n601/L1 (4x would pass the cap)
    ("fp32", "dx", "nrm"): 1.0e-6,              # 2.9e-7  3x84_fp32_n512/L3 (4x would pass the cap)
    ("fp32", "dx", "pix"): 5.7e-6,              # 1.4e-6  3x84_fp32_limit_n41943/L3
    ("bf16x3", "feat", "nrm"): 3.0e-7,          # 1.7e-7  3x84_b3_n601 (4x would pass the cap)
    ("bf16x3", "feat", "pix"): 2.1e-6,          # 5.2e-7  3x84_b3_limit_n41943
    ("bf16x3", "dw", "nrm"): 3.0e-7,            # 1.9e-7  3x84_b3_n2048/L2 (4x would pass the cap)
    ("bf16x3", "dw", "pix"): 3.9e-6,            # 9.8e-7  3x84_b3_n601/L3
    ("bf16x3", "db", "nrm"): 1.0e-6,            # 2.8e-7  3x84_b3_n129/L1 (4x would pass fp32's cap)
    ("bf16x3", "dx", "nrm"): 3.0e-7,            # 8.9e-8  3x84_b3_n129/L3 (4x would pass the cap)
    ("bf16x3", "dx", "pix"): 2.0e-6,            # 5.1e-7  3x84_b3_limit_n41943/L3
    ("fp32@2^24", "dw", "nrm"): 7.6e-6,         # 1.9e-6  3x84_fp32_limit_n41943/L1
    ("fp32@2^24", "dw", "pix"): 2.9e-5,         # 7.3e-6  3x84_fp32_limit_n41943/L2
    ("fp32@2^24", "db", "nrm"): 5.2e-6,         # 1.3e-6  3x84_fp32_limit_n41943/L1
    ("bf16x3@2^24", "dw", "nrm"): 7.6e-6,       # 1.9e-6  3x84_b3_limit_n41943/L1
    ("bf16x3@2^24", "dw", "pix"): 1.5e-5,       # 3.9e-6  3x84_b3_limit_n41943/L2
    ("bf16x3@2^24", "db", "nrm"): 2.5e-6,       # 6.3e-7  3x84_b3_limit_n41943/L1
    ("rollout", "feat", "nrm"): 1.0e-6,         # 3.0e-7  3x36x36_w8 (4x would pass the cap)
    ("rollout", "feat", "pix"): 1.5e-6,         # 3.8e-7  3x132x132_w96
    ("rollout", "hidden", "nrm"): 1.0e-6,       # 2.9e-7  3x36x36_w8 (4x would pass the cap)
    ("rollout", "hidden", "pix"): 2.3e-6,       # 5.7e-7  1x84x84_w96
}
KINK = 1e-5     # |pre-activation| / max |pre-activation| of its image below which the device's ReLU may fall on either side

# ------------------------------------------------------------------ dispatch rules (python restatement of the host code)
CONVS = ((32, 8, 4), (64, 4, 2), (64, 3, 1))          # (Cout, kernel, stride) of model.py:29-31
B3_LAYERS = {(3, 84, 84, 32, 8, 4), (32, 20, 20, 64, 4, 2), (64, 9, 9, 64, 3, 1)}     # ops._B3_LAYERS
FWD_LDS_MASK, WGRAD_LDS_MASK = 2, 1                    # ETM_CONV_FWD_LDS_DEFAULT, ETM_CONV_WGRAD_LDS_DEFAULT (bit l - 1: layer l)
FWD_LDS = {(3, 84, 8, 4, 32): (1, 3), (32, 20, 4, 2, 64): (2, 36), (64, 9, 3, 1, 64): (4, 68)}   # (C, HW, KS, S, COUT) -> (G, CP)
WGRAD_LDS = {(3, 84, 8, 4, 32): 1, (32, 20, 4, 2, 64): 2, (64, 9, 3, 1, 64): 4}                 # -> G
DGRAD_LDS = (32, 20, 20, 64, 4, 2)                     # (C, H, W, Cout, K, S): conv_dgrad_lds<64, 9, 2, 2, 32, 4, 68>


def _cdiv(a, b):
    return -(-a // b)


def _layers(C, H, W):
    """Per layer (c, h, w, cout, k, s, ho, wo)."""
    out = []
    for cout, k, s in CONVS:
        ho, wo = (H - k) // s + 1, (W - k) // s + 1
        out.append((C, H, W, cout, k, s, ho, wo))
        C, H, W = cout, ho, wo
    return out


def _lbit(k):
    return 1 if k == 8 else 2 if k == 4 else 4


def _pick_mt(tiles, cands):
    """conv_pick_mt(prefer_large = false): fewest rounds of 256 workgroups x MT, ties to the smallest MT."""
    best, best_cost = cands[0], None
    for mt in cands:
        cost = _cdiv(_cdiv(tiles, 4 * mt), 256) * mt
        if best_cost is None or cost < best_cost or (cost == best_cost and mt < best):
            best, best_cost = mt, cost
    return best


def _uses_b3(C, H, W, products):
    return (products or "bf16x3") == "bf16x3" and all(g[:6] in B3_LAYERS for g in _layers(C, H, W))


def _fwd_key(li, g, N, indexed):
    """etm_conv_train_fwd.  Keys: (pass, kernel, template arguments, partial last k-range)."""
    c, h, w, cout, k, s, ho, wo = g
    lds = FWD_LDS.get((c, h, k, s, cout)) if h == w else None
    if _lbit(k) & FWD_LDS_MASK and N >= 512 and lds:
        G, CP = lds
        if not (G > 1 and indexed) and N * ho * wo * cout * 4 < 0xfffffff0:
            return ("fwd", "lds", (c, h, k, s, cout, G, CP), False)
    tiles = _cdiv(N * ho * wo, 32)
    if cout == 32:                                     # conv_launch<MT, 1, false>: shared fragments, no EVEN form at NT = 1
        return ("fwd", "gemm", (_pick_mt(tiles, (2, 4)), 1, False, 1, True, False), False)
    if _cdiv(tiles, 16) <= 256:                        # one round of MT = 4 workgroups: private fragments
        return ("fwd", "gemm", (4, 2, False, 1, False, False), False)
    return ("fwd", "gemm", (_pick_mt(tiles, (2, 1, 4)), 2, False, 1, True, (k * k * c // 8) % 2 == 0), False)


def _dgrad_key(g, N):
    """etm_conv_train_dgrad (layers 2 and 3: the data gradient of the layer's input)."""
    c, h, w, cout, k, s, ho, wo = g
    if N >= 512 and (c, h, w, cout, k, s) == DGRAD_LDS and N * h * h * c * 4 < 0xfffffff0:
        return ("dgrad", "lds", (64, 9, 2, 2, 32, 4, 68), False)
    merged = c == 32 and s == 2
    mt = 2
    if not merged:
        best = None
        for m in ((2, 4) if c == 32 else (1, 2, 4)):
            wu = 32 * m * 4
            t = (h // s) * (w // s) * _cdiv(N, wu) * (wu // 32)
            cost = _cdiv(_cdiv(t, 4 * m), 256) * m
            if best is None or cost < best:
                best, mt = cost, m
    nt, cls = (1 if c == 32 else 2), (4 if merged else 1)
    ch = 4 if nt * cls == 1 else 2
    return ("dgrad", "gemm", (mt, nt, True, cls, True, (cout // 8) % ch == 0), False)


def _wgrad_key(g, N, indexed):
    """etm_conv_train_wgrad."""
    c, h, w, cout, k, s, ho, wo = g
    bit = _lbit(k)
    if bit & WGRAD_LDS_MASK and N >= 512 and not (indexed and bit != 1) and h == w and (c, h, k, s, cout) in WGRAD_LDS:
        return ("wgrad", "lds", (c, h, k, s, cout, WGRAD_LDS[(c, h, k, s, cout)]), False)
    K = k * k * c
    kt = 6 if cout == 32 else (3 if K % 128 and K % 96 == 0 else 4)
    return ("wgrad", "gemm", (kt, 1 if cout == 32 else 2), K % (kt * 32) != 0)


def train_keys(C, H, W, N, products, indexed):
    layers = _layers(C, H, W)
    if _uses_b3(C, H, W, products):
        return {("fwd", "b3", l + 1, False) for l in range(3)} | {("wgrad", "b3", l + 1, False) for l in range(3)} \
            | {("dgrad", "b3", l + 1, False) for l in (1, 2)}
    keys = set()
    for li, g in enumerate(layers):
        keys.add(_fwd_key(li, g, N, indexed and li == 0))
        keys.add(_wgrad_key(g, N, indexed and li == 0))
        if li:
            keys.add(_dgrad_key(g, N))
    return keys


def rollout_keys(C, H, W, n):
    """etm_conv_relu of the three layers (layer 1 reads NCHW: K = C * 8 * 8 in rows of 8) + etm_rollout_conv3_hidden."""
    keys = set()
    for li, (c, h, w, cout, k, s, ho, wo) in enumerate(_layers(C, H, W)):
        gpw = _cdiv(k * k * c // 8, 8)
        grid = _cdiv(n * ho * wo, 32)
        if cout == 32:
            keys.add(("rollout", "conv_relu", (1, 4 if gpw <= 4 else 12), 1))
        elif 2 * grid <= 256:
            keys.add(("rollout", "conv_relu", (1, 4 if gpw <= 4 else 12), 2))
        else:
            keys.add(("rollout", "conv_relu", (2, 4 if gpw <= 4 else 8 if gpw <= 8 else 10 if gpw <= 10 else 12), 1))
    c, h, w = _layers(C, H, W)[2][:3]
    if (h - 2) * (w - 2) <= 64:
        keys.add(("rollout", "conv3_hidden", (), False))
    return keys


def _rollout_ok(C, H, W):
    """model._fused_encoder_ok on an [n, C, H, W] batch."""
    h1, w1 = (H - 8) // 4 + 1, (W - 8) // 4 + 1
    return W % 4 == 0 and h1 >= 4 and w1 >= 4 and (h1 - 4) // 2 + 1 >= 3 and (w1 - 4) // 2 + 1 >= 3


_E = (True, False)
COMPILED = ({("fwd", "gemm", (2, 1, False, 1, True, False), False), ("fwd", "gemm", (4, 1, False, 1, True, False), False),
             ("fwd", "gemm", (4, 2, False, 1, False, False), False)}
            | {("fwd", "gemm", (mt, 2, False, 1, True, e), False) for mt in (1, 2, 4) for e in _E}
            | {("fwd", "lds", (c, h, k, s, co) + FWD_LDS[(c, h, k, s, co)], False) for (c, h, k, s, co) in FWD_LDS}
            | {("dgrad", "gemm", (2, 1, True, 4, True, e), False) for e in _E}
            | {("dgrad", "gemm", (mt, 1, True, 1, True, e), False) for mt in (2, 4) for e in _E}
            | {("dgrad", "gemm", (mt, 2, True, 1, True, e), False) for mt in (1, 2, 4) for e in _E}
            | {("dgrad", "lds", (64, 9, 2, 2, 32, 4, 68), False)}
            | {("wgrad", "gemm", kc, p) for kc in ((6, 1), (4, 2), (3, 2)) for p in _E}
            | {("wgrad", "lds", key + (g,), False) for key, g in WGRAD_LDS.items()}
            | {(p, "b3", l, False) for p in ("fwd", "wgrad") for l in (1, 2, 3)} | {("dgrad", "b3", l, False) for l in (2, 3)}
            | {("rollout", "conv_relu", (1, gb), y) for gb in (4, 12) for y in (1, 2)}
            | {("rollout", "conv_relu", (2, gb), 1) for gb in (4, 8, 10, 12)}
            | {("rollout", "conv3_hidden", (), False)})

UNREACHABLE = {
    ("fwd", "gemm", (4, 1, False, 1, True, False), False): "Cout 32 forward: rounds x MT of MT 4 is never below MT 2's (ties: MT 2)",
    ("fwd", "gemm", (2, 2, False, 1, True, True), False): "Cout 64 forward past 256 workgroups: MT 1 always costs least (ties: MT 1)",
    ("fwd", "gemm", (4, 2, False, 1, True, True), False): "Cout 64 forward past 256 workgroups: MT 1 always costs least (ties: MT 1)",
    ("fwd", "gemm", (1, 2, False, 1, True, False), False): "no EVEN form: K / 8 = KH KW C / 8 is even for C in {32, 64}",
    ("fwd", "gemm", (2, 2, False, 1, True, False), False): "never picked (MT 1), and K / 8 is even",
    ("fwd", "gemm", (4, 2, False, 1, True, False), False): "never picked (MT 1), and K / 8 is even",
    ("fwd", "lds", (3, 84, 8, 4, 32, 1, 3), False): "off by default (ETM_CONV_FWD_LDS_DEFAULT = 2); test_gpu_parity sets the mask",
    ("fwd", "lds", (64, 9, 3, 1, 64, 4, 68), False): "off by default (ETM_CONV_FWD_LDS_DEFAULT = 2); test_gpu_parity sets the mask",
    ("dgrad", "gemm", (2, 1, True, 4, True, False), False): "merged C = 32 form: Cout / 8 = 8 groups per tap, a multiple of the chunk",
    ("dgrad", "gemm", (2, 1, True, 1, True, True), False): "unmerged C = 32 needs S != 2; layer 2 has S = 2",
    ("dgrad", "gemm", (2, 1, True, 1, True, False), False): "unmerged C = 32 needs S != 2; layer 2 has S = 2",
    ("dgrad", "gemm", (4, 1, True, 1, True, True), False): "unmerged C = 32 needs S != 2; layer 2 has S = 2",
    ("dgrad", "gemm", (4, 1, True, 1, True, False), False): "unmerged C = 32 needs S != 2; layer 2 has S = 2",
    ("dgrad", "gemm", (2, 2, True, 1, True, True), False): "C = 64: rounds x MT over padded image units is least at MT 1",
    ("dgrad", "gemm", (4, 2, True, 1, True, True), False): "C = 64: rounds x MT over padded image units is least at MT 1",
    ("dgrad", "gemm", (1, 2, True, 1, True, False), False): "Cout / 8 = 8 groups per tap, a multiple of the chunk",
    ("dgrad", "gemm", (2, 2, True, 1, True, False), False): "never picked (MT 1), and Cout / 8 is even",
    ("dgrad", "gemm", (4, 2, True, 1, True, False), False): "never picked (MT 1), and Cout / 8 is even",
    ("wgrad", "gemm", (4, 2), True): "<4, 2> runs layer 2 only: K = 16 * 32 = 512, a multiple of 128",
    ("wgrad", "gemm", (3, 2), True): "<3, 2> runs layer 3 only: K = 9 * 64 = 576, a multiple of 96",
    ("wgrad", "lds", (32, 20, 4, 2, 64, 2), False): "off by default (ETM_CONV_WGRAD_LDS_DEFAULT = 1); test_gpu_parity sets the mask",
    ("wgrad", "lds", (64, 9, 3, 1, 64, 4), False): "off by default (ETM_CONV_WGRAD_LDS_DEFAULT = 1); test_gpu_parity sets the mask",
    ("rollout", "conv_relu", (1, 4), 2): "Cout 64 layers have K >= 512, i.e. more than 4 groups per wave",
    ("rollout", "conv_relu", (2, 4), 1): "Cout 64 layers have K >= 512, i.e. more than 4 groups per wave",
    ("rollout", "conv_relu", (2, 12), 1): "Cout 64 layers have K <= 576, i.e. at most 9 groups per wave",
}

SWEEP_C = (1, 2, 3, 4, 8)
SWEEP_HW = tuple(range(36, 204, 8)) + (37, 39, 42, 61)
SWEEP_N = (1, 7, 127, 128, 129, 255, 256, 257, 511, 512, 513, 601, 1024, 2048, 2674, 2675, 4096, 8192, 16384, 32768)


def _convs_cpu(C):
    return [torch.nn.Conv2d(cin, cout, k, s) for cin, (cout, k, s) in zip((C, 32, 64), CONVS)]


def _max_batch(C, H, W, convs):
    """Largest N encoder_train_supported(batch=N) admits (it is monotone in N)."""
    from etm import ops
    lo, hi = 1, 1 << 22
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if ops.encoder_train_supported((C, H, W), convs, batch=mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


def reachable():
    from etm import ops
    reach = set()
    for C in SWEEP_C:
        convs = _convs_cpu(C)
        for H, W in itertools.product(SWEEP_HW, SWEEP_HW):
            if not ops.encoder_train_supported((C, H, W), convs):
                continue
            nmax = _max_batch(C, H, W, convs)
            for N in [n for n in SWEEP_N if n < nmax] + [nmax]:
                for products, indexed in itertools.product(("bf16x3", "fp32"), _E):
                    reach |= train_keys(C, H, W, N, products, indexed)
            if _rollout_ok(C, H, W):
                for n in (1, 8, 64, 84, 96, 256, 1024):
                    reach |= rollout_keys(C, H, W, n)
    return reach


# ------------------------------------------------------------------ the case matrix
def _case(name, shape, ns, products=None):
    return [dict(name=f"{name}_n{n}", shape=shape, N=n, products=products) for n in ns]


TRAIN_CASES = (_case("3x84_b3", (3, 84, 84), (1, 7, 129, 601, 2048), "bf16x3")
               + _case("3x84_fp32", (3, 84, 84), (1, 7, 127, 128, 129, 511, 512, 601, 2048, 2674, 2675), "fp32")
               + _case("1x84", (1, 84, 84), (7, 129, 512, 2048))
               + _case("4x84", (4, 84, 84), (5, 601))
               + _case("8x84", (8, 84, 84), (7, 600))
               + _case("2x38", (2, 38, 38), (1, 33, 513))
               + _case("3x36", (3, 36, 36), (7, 128, 601))
               + _case("3x44x60", (3, 44, 60), (7, 129, 512))
               + _case("3x132", (3, 132, 132), (3, 130))
               + _case("3x84_b3_limit", (3, 84, 84), (41943,), "bf16x3")
               + _case("3x84_fp32_limit", (3, 84, 84), (41943,), "fp32"))
ROLLOUT_GEOMETRIES = ((3, 84, 84), (1, 84, 84), (4, 84, 84), (8, 84, 84), (3, 36, 36), (3, 44, 60), (3, 132, 132))      # (2 x 38 x 38: W % 4 != 0, no rollout encoder)
ROLLOUT_N = (8, 64, 96)


# ------------------------------------------------------------------ helpers
def _dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda", 0)


def _record(fails, kind, what, measure, value, name):
    key = (kind, what, measure)
    print(f"[measured] {name} {key}: {value:.2e}  bound {BOUNDS[key]:.1e}")
    cap = CAP.get("fp32" if kind == "bf16x3" and what == "db" else kind, 1.0) if measure == "nrm" else 1.0
    if not value <= min(BOUNDS[key], cap):
        fails.append((name, key, value, BOUNDS[key]))


def _images(n, C, H, W, gen, nchw=False):
    """[n, H, W, C] (or NCHW): by (n - 1 - i) % 6 uniform, all-zero, constant, 0 - 255 integers, uniform, uniform -- the last image
    (the ragged tail) is always uniform."""
    x = torch.rand((n, H, W, C), generator=gen)
    kind = (n - 1 - torch.arange(n)) % 6
    x[kind == 1] = 0.0
    x[kind == 2] = 0.37
    ints = kind == 3
    x[ints] = torch.randint(0, 256, (int(ints.sum()), H, W, C), generator=gen).float()
    return x.permute(0, 3, 1, 2).contiguous() if nchw else x


def _case_params(convs, gen):
    """Weights from the case's generator (uniform in +-1 / sqrt(fan-in), the layers' default range); biases: every 5th channel
    strongly negative (dead for whole uniform / zero / constant images), every 7th positive."""
    with torch.no_grad():
        for conv in convs:
            wt = conv.weight
            wt.copy_((2 * torch.rand(wt.shape, generator=gen) - 1) / (wt[0].numel() ** 0.5))
            b = conv.bias
            b.copy_(0.05 * torch.randn(b.shape, generator=gen))
            b[::5] = -2.0
            b[3::7] = 0.5


def _fwd64(x, wt, b, s):
    """relu-free conv2d in float64 on the device: x [n, c, h, w] -> [n, cout, ho, wo] (unfold + einsum)."""
    n, _, h, w = x.shape
    cout, _, k, _ = wt.shape
    cols = F.unfold(x, k, stride=s)
    y = torch.einsum("ok,nkl->nol", wt.reshape(cout, -1), cols) + b[:, None]
    return y.reshape(n, cout, (h - k) // s + 1, (w - k) // s + 1), cols


def _dgrad64(g, wt, s, hw):
    """conv_transpose2d in float64 on the device: g [n, cout, ho, wo] -> [n, c, h, w]."""
    n, cout = g.shape[:2]
    k = wt.shape[2]
    cols = torch.einsum("ok,nol->nkl", wt.reshape(cout, -1), g.reshape(n, cout, -1))
    return F.fold(cols, hw, k, stride=s)


class _Err:
    """Normwise relative error and the worst row-wise max |err| / max |ref| over chunks of rows (dim 0 = image or channel)."""

    def __init__(self):
        self.e2, self.r2, self.pix = 0.0, 0.0, 0.0

    def add(self, got, ref):
        got, ref = got.reshape(got.shape[0], -1).double(), ref.reshape(ref.shape[0], -1).double()
        err = (got - ref).abs()
        self.e2 += float((err * err).sum())
        self.r2 += float((ref * ref).sum())
        em, rm = err.amax(1), ref.abs().amax(1)
        assert bool(((rm > 0) | (em == 0)).all()), "nonzero result where the reference row is exactly zero"
        self.pix = max(self.pix, float((em / rm.clamp_min(1e-300)).max()))

    def nrm(self):
        return (self.e2 / self.r2) ** 0.5 if self.r2 > 0 else (0.0 if self.e2 == 0 else float("inf"))


def _host_subset(N, layers):
    """First, last, middle images and those whose pixel index (N-major) crosses 2^23 in some layer."""
    sel = {0, N - 1, N // 2}
    for g in layers:
        px = g[6] * g[7]
        if N * px > 2 ** 23:
            sel.add((2 ** 23) // px)
    return sorted(sel)


# ------------------------------------------------------------------ training
def _run_train_case(case):
    from etm import lib as etm_lib
    from etm import ops
    dev = _dev()
    lib = etm_lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    P = lambda t: None if t is None else t.data_ptr()
    C, H, W = case["shape"]
    N, products = case["N"], case["products"]
    kind = "bf16x3" if _uses_b3(C, H, W, products) else "fp32"
    sums = kind + "@2^24" if N * _layers(C, H, W)[0][6] * _layers(C, H, W)[0][7] > 2 ** 23 else kind      # (see CAP)
    name = case["name"]
    fails = []
    gen = torch.Generator().manual_seed(N * 7 + C * 1000 + H)
    convs = _convs_cpu(C)
    _case_params(convs, gen)
    for c in convs:
        c.to(dev)
    params = [t for c in convs for t in (c.weight, c.bias)]
    layers = _layers(C, H, W)
    assert ops.encoder_train_supported((C, H, W), convs, batch=N)
    extra = 13
    bank = torch.empty((N + extra, H, W, C), device=dev)
    for lo in range(0, N + extra, 4096):
        hi = min(lo + 4096, N + extra)
        bank[lo:hi] = _images(hi - lo, C, H, W, gen).to(dev)
    index = torch.randperm(N + extra, generator=gen)[:N].to(dev)
    x = bank[index].contiguous()
    Fdim = layers[2][3] * layers[2][6] * layers[2][7]
    gout = torch.randn((N, Fdim), generator=gen).to(dev)

    # ---- the public op: plain, indexed (bit-identical), DeferredDw (bit-identical gradients)
    feats = ops.encoder_train(x, *convs, products=products)
    grads = torch.autograd.grad(feats, params, gout)
    feats = feats.detach()
    f_idx = ops.encoder_train(bank, *convs, index=index, products=products)
    g_idx = torch.autograd.grad(f_idx, params, gout)
    assert torch.equal(f_idx, feats), (name, "features through the index")
    assert all(torch.equal(a, b) for a, b in zip(g_idx, grads)), (name, "gradients through the index")
    del f_idx, g_idx
    views = [torch.full_like(t, float("nan")) for t in params]
    with ops.DeferredDw({t.data_ptr(): v for t, v in zip(params, views)}) as col:
        (ops.encoder_train(x, *convs, products=products) * gout).sum().backward()
    assert col.written == {t.data_ptr() for t in params} and all(t.grad is None for t in params), name
    assert all(torch.equal(v, g) for v, g in zip(views, grads)), (name, "DeferredDw gradients")
    del views, bank

    # ---- the encoder's three forward launches again through the C ABI: bit-identical activations, whose ReLU pattern is the mask of
    #      the reference backward pass (a pre-activation within rounding of 0 may fall on either side; elsewhere the patterns agree)
    ys = [x]
    for l, (c, h, w, cout, k, s, ho, wo) in enumerate(layers):
        wt, b = convs[l].weight.detach(), convs[l].bias.detach()
        y = torch.full((N, ho, wo, cout), float("nan"), device=dev)
        if kind == "bf16x3":
            pk = ops.conv_b3_pack([wt], [0], [s])[0]
            etm_lib.check(lib.etm_conv_b3_fwd(P(ys[-1]), None, P(pk), P(b), P(y), None, N, c, h, w, cout, k, k, s, st), "etm_conv_b3_fwd")
        else:
            pk = ops.conv_pack_weights(wt.permute(0, 2, 3, 1).reshape(cout, -1))
            etm_lib.check(lib.etm_conv_train_fwd(P(ys[-1]), None, N, P(pk), P(b), P(y), N, c, h, w, cout, k, k, s, 0, st), "etm_conv_train_fwd")
        ys.append(y)
    assert torch.equal(ys[3].view(N, -1), feats), (name, "per-layer forward launches")

    # ---- float64 reference over all images (device, chunked); fp32 copies of the gradients backward-data reads
    w64 = [c.weight.detach().double() for c in convs]
    b64 = [c.bias.detach().double() for c in convs]
    g32 = [None, torch.empty((N, layers[1][6], layers[1][7], 64), device=dev), torch.empty((N, layers[2][6], layers[2][7], 64), device=dev)]
    dw64 = [torch.zeros_like(w) for w in w64]
    db64 = [torch.zeros_like(b) for b in b64]
    e_feat = _Err()
    flips = 0
    host = _host_subset(N, layers)
    per = max(1, (1 << 28) // max(8 * g[4] * g[4] * g[0] * g[6] * g[7] for g in layers))      # images per chunk: <= 256 MB of columns
    for lo in range(0, N, per):
        hi = min(lo + per, N)
        a, cols, pat = [x[lo:hi].permute(0, 3, 1, 2).double()], [], [None]
        for l in range(3):
            z, cl = _fwd64(a[-1], w64[l], b64[l], layers[l][5])
            p = ys[l + 1][lo:hi].permute(0, 3, 1, 2) > 0
            off = p != (z > 0)
            assert not bool((off & (z.abs() > KINK * z.abs().amax((1, 2, 3), keepdim=True))).any()), (name, l + 1, "ReLU pattern")
            flips += int(off.sum())
            a.append(torch.relu(z))
            cols.append(cl)
            pat.append(p)
        e_feat.add(feats[lo:hi], a[3].permute(0, 2, 3, 1).reshape(hi - lo, -1))
        g = gout[lo:hi].double().reshape(hi - lo, layers[2][6], layers[2][7], 64).permute(0, 3, 1, 2) * pat[3]
        for l in (2, 1, 0):
            n_, co = g.shape[:2]
            dw64[l] += torch.einsum("nkl,nol->ok", cols[l], g.reshape(n_, co, -1)).reshape(w64[l].shape)
            db64[l] += g.sum((0, 2, 3))
            if l:
                g32[l][lo:hi] = g.permute(0, 2, 3, 1).float()
                g = _dgrad64(g, w64[l], layers[l][5], layers[l][1:3]) * pat[l]
        del a, cols, g, pat
    print(f"[{name}] ReLU pattern: {flips} pre-activations within {KINK:.0e} of 0 on the other side")
    # the device reference against the host library on the subset
    xs = x[host].permute(0, 3, 1, 2).double().cpu()
    for l in range(3):
        xs = torch.relu(F.conv2d(xs, w64[l].cpu(), b64[l].cpu(), stride=layers[l][5]))
    hs = xs.permute(0, 2, 3, 1).reshape(len(host), -1)
    assert float((feats[host].double().cpu() - hs).norm() / hs.norm().clamp_min(1e-300)) < 1e-5, (name, "host cross-check")
    _record(fails, kind, "feat", "nrm", e_feat.nrm(), name)
    _record(fails, kind, "feat", "pix", e_feat.pix, name)
    for l in range(3):
        e_w, e_b = _Err(), _Err()
        e_w.add(grads[2 * l], dw64[l])
        e_b.add(grads[2 * l + 1][None], db64[l][None])
        _record(fails, sums, "dw", "nrm", e_w.nrm(), f"{name}/L{l + 1}")
        _record(fails, sums, "dw", "pix", e_w.pix, f"{name}/L{l + 1}")
        _record(fails, sums, "db", "nrm", e_b.nrm(), f"{name}/L{l + 1}")
    del feats, grads, gout

    # ---- backward-data of layers 2 and 3 through the C ABI: mask from the layer below's output, masked elements exact zeros
    for l in (2, 1):
        c, h, w, cout, k, s = layers[l][:6]
        wt = convs[l].weight.detach()
        dx = torch.full((N, h, w, c), float("nan"), device=dev)
        if kind == "bf16x3":
            dg = ops.conv_b3_pack([wt], [1], [s])[0]
            etm_lib.check(lib.etm_conv_b3_dgrad(P(g32[l]), None, P(dg), P(ys[l]), None, P(dx), N, c, h, w, cout, k, k, s, st), "etm_conv_b3_dgrad")
        else:
            etm_lib.check(lib.etm_conv_train_dgrad(P(g32[l]), P(ops.conv_pack_dgrad_weights(wt, s)), P(ys[l]), P(dx), N, c, h, w, cout, k, k, s, st),
                          "etm_conv_train_dgrad")
        assert bool((dx[ys[l] == 0] == 0).all()), (name, l + 1, "masked elements")
        e_x = _Err()
        for lo in range(0, N, 2048):
            hi = min(lo + 2048, N)
            ref = _dgrad64(g32[l][lo:hi].permute(0, 3, 1, 2).double(), w64[l], s, (h, w)) * (ys[l][lo:hi].permute(0, 3, 1, 2) > 0)
            e_x.add(dx[lo:hi], ref.permute(0, 2, 3, 1))
        _record(fails, kind, "dx", "nrm", e_x.nrm(), f"{name}/L{l + 1}")
        _record(fails, kind, "dx", "pix", e_x.pix, f"{name}/L{l + 1}")
        del dx
    del ys, g32
    torch.cuda.empty_cache()
    assert not fails, fails


@pytest.mark.parametrize("case", TRAIN_CASES, ids=[c["name"] for c in TRAIN_CASES])
def test_encoder_train_vs_float64(case):
    _run_train_case(case)


# ------------------------------------------------------------------ rollout (no grad)
@pytest.mark.parametrize("shape", ROLLOUT_GEOMETRIES, ids=["x".join(map(str, s)) for s in ROLLOUT_GEOMETRIES])
def test_rollout_encoder_vs_float64(shape):
    from model import ActorCriticModel
    from etm import ops
    dev = _dev()
    C, H, W = shape
    D = 128
    cfg = dict(hidden_layer_size=D, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=8,
                                                     positional_encoding="", layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    gen = torch.Generator().manual_seed(C * 100 + H + W)
    torch.manual_seed(C * 100 + H + W)          # (the model's other layers, lin_hidden among them)
    m = ActorCriticModel(cfg, SimpleNamespace(shape=shape), (3,), 8)
    convs = (m.conv1, m.conv2, m.conv3)
    _case_params(convs, gen)
    m = m.to(dev)
    layers = _layers(C, H, W)
    h2, w2 = layers[2][1:3]
    assert _rollout_ok(C, H, W)
    fails = []
    hidden_ok = ops.rollout_conv3_hidden_supported(m.conv3, h2, w2, D)
    assert hidden_ok == ((h2 - 2) * (w2 - 2) <= 64), (shape, "conv3_hidden gate")
    for n in ROLLOUT_N:
        name = f"{'x'.join(map(str, shape))}_w{n}"
        obs = _images(n, C, H, W, gen, nchw=True).to(dev)
        with torch.no_grad():
            assert m._fused_encoder_ok(obs)
            got = m._encode_fused(obs, features_only=True)
            a = obs.double().cpu()
            for conv in convs:
                a = torch.relu(F.conv2d(a, conv.weight.double().cpu(), conv.bias.double().cpu(), stride=conv.stride))
            e = _Err()
            e.add(got.cpu(), a.reshape(n, -1))
            _record(fails, "rollout", "feat", "nrm", e.nrm(), name)
            _record(fails, "rollout", "feat", "pix", e.pix, name)
            if hidden_ok:
                x2 = m._encode_fused(obs, features_only="conv2")
                part = ops.rollout_conv3_hidden(x2, m._w3k, m.conv3.bias, m.lin_hidden.weight.detach().t().contiguous())
                hid = torch.relu(part.sum(dim=0) + m.lin_hidden.bias)
                ref = torch.relu(a.reshape(n, -1) @ m.lin_hidden.weight.double().cpu().t() + m.lin_hidden.bias.double().cpu())
                e = _Err()
                e.add(hid.cpu(), ref)
                _record(fails, "rollout", "hidden", "nrm", e.nrm(), name)
                _record(fails, "rollout", "hidden", "pix", e.pix, name)
    assert not fails, fails


# ------------------------------------------------------------------ the bank-size gate
def test_indexed_encoder_on_a_bank_past_the_32_bit_offsets():
    """A minibatch gathered from a bank of 2^31 floats or more at 4 x 84 x 84: the fp32 first layer addresses the whole bank with
    32-bit element offsets, so the model's indexed path must gather first (encoder_train_supported(bank=...) answers False) and
    give, bit for bit, what the encoder computes on the gathered minibatch."""
    from model import ActorCriticModel, IndexedObservations
    from etm import ops
    dev = _dev()
    C, H, W = 4, 84, 84
    n_bank = (2 ** 31) // (H * W * C) + 64
    cfg = dict(hidden_layer_size=128, transformer=dict(num_blocks=1, embed_dim=64, num_heads=2, memory_length=8,
                                                       positional_encoding="", layer_norm="post", gtrxl=False, gtrxl_bias=0.0))
    torch.manual_seed(3)
    m = ActorCriticModel(cfg, SimpleNamespace(shape=(C, H, W)), (3,), 8).to(dev)
    convs = (m.conv1, m.conv2, m.conv3)
    bank = torch.empty((n_bank, H, W, C), device=dev)          # uninitialised: only the indexed rows are written
    index = torch.cat([torch.arange(n_bank - 48, n_bank), torch.randint(0, n_bank, (48,))]).to(dev)
    bank[index] = torch.rand((96, H, W, C), device=dev)
    got = m._encode(IndexedObservations(bank, index))
    assert not ops.encoder_train_supported((C, H, W), convs, batch=96, bank=n_bank)
    assert ops.encoder_train_supported((C, H, W), convs, batch=96, bank=n_bank - 128)
    feats = ops.encoder_train(bank.index_select(0, index), *convs, products=m.encoder_products)
    want = ops.linear_relu_nhwc(feats, m.lin_hidden.weight, m.lin_hidden.bias, m.conv3.out_channels)
    assert torch.equal(got, want)
    go = torch.randn_like(got)
    params = [t for c in convs for t in (c.weight, c.bias)]
    assert all(torch.equal(a, b) for a, b in zip(torch.autograd.grad(got, params, go), torch.autograd.grad(want, params, go)))


# ------------------------------------------------------------------ coverage
def test_encoder_matrix_covers_every_reachable_launch():
    """The restated dispatch swept over the admitted geometries (C in {1, 2, 3, 4, 8}, H, W from 36 to 196, non-square included)
    and batch sizes up to the 24-bit pixel limit: every reachable launch key is hit by a case, the compiled forms it never reaches
    are exactly UNREACHABLE, and every case is a geometry the host code admits."""
    from etm import ops
    reach = reachable()
    assert reach <= COMPILED, sorted(map(str, reach - COMPILED))
    assert reach.isdisjoint(UNREACHABLE), sorted(map(str, reach & set(UNREACHABLE)))
    assert COMPILED - reach == set(UNREACHABLE), (sorted(map(str, COMPILED - reach - set(UNREACHABLE))),
                                                  sorted(map(str, set(UNREACHABLE) - (COMPILED - reach))))
    covered = set()
    for c in TRAIN_CASES:
        C, H, W = c["shape"]
        assert ops.encoder_train_supported(c["shape"], _convs_cpu(C), batch=c["N"]), c["name"]
        for indexed in _E:
            covered |= train_keys(C, H, W, c["N"], c["products"], indexed)
    for shape in ROLLOUT_GEOMETRIES:
        for n in ROLLOUT_N:
            covered |= rollout_keys(*shape, n)
    assert reach <= covered, sorted(map(str, reach - covered))
    assert max(c["N"] for c in TRAIN_CASES if c["shape"] == (3, 84, 84)) == _max_batch(3, 84, 84, _convs_cpu(3))
    for key, why in sorted(UNREACHABLE.items(), key=str):
        print(f"[unreachable] {key}: {why}")
    print(f"[coverage] {len(reach)} reachable launch keys, all covered; {len(UNREACHABLE)} compiled forms unreachable")
