"""Float64 numpy restatement of etm_attn_stats (include/etm_hip.h, csrc/attn_stats.hip) for the attention-statistics tests, the
inputs the kernel tests run on, and the error bound of the entropy words.

``attention_statistics_reference(att, mask)`` -> the table [H, 264] a call adds for ``att`` [N, H, L] and ``mask`` [N, L]: every sum
in float64 on the fp32 inputs taken as they are.  Two deliberately WRONG variants exist for the guard that the bounds are not
vacuous: ``age_shift=1`` files every probability one age too old, ``swap_halves=True`` exchanges window entries l and l + 64 (what a
kernel that confused its two lane halves would do)."""
import numpy as np

WORDS = 264
AGE0, INDEX0, MAX_L = 8, 136, 128


def row_classes(mask):
    """(v [N], counted [N], empty [N], irregular [N]) of the mask rows."""
    m = np.asarray(mask) != 0
    L = m.shape[1]
    v = m.sum(axis=1)
    prefix = (m == (np.arange(L)[None, :] < v[:, None])).all(axis=1)
    return v, prefix & (v >= 1), prefix & (v == 0), ~prefix


def attention_statistics_reference(att, mask, age_shift=0, swap_halves=False):
    att = np.asarray(att)
    N, H, L = att.shape
    assert att.dtype == np.float32 and 1 <= L <= MAX_L and np.asarray(mask).shape == (N, L)
    v, counted, empty, irregular = row_classes(mask)
    table = np.zeros((H, WORDS), dtype=np.float64)
    table[:, 0], table[:, 1], table[:, 2], table[:, 3] = counted.sum(), (counted & (v >= 2)).sum(), empty.sum(), irregular.sum()
    valid = np.arange(L)[None, :] < v[:, None]                                  # [N, L] (the mask itself on a counted row)
    p = np.where((counted[:, None] & valid)[:, None, :], att.astype(np.float64), 0.0)       # [N, H, L]
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=2)        # [N, H]
    table[:, 4] = ent.sum(axis=0)
    two = counted & (v >= 2)
    table[:, 5] = (ent[two] / np.log(v[two].astype(np.float64))[:, None]).sum(axis=0)
    table[:, 6] = p.max(axis=2).sum(axis=0)
    q = np.zeros((N, H, MAX_L), dtype=np.float64)
    q[:, :, :L] = p
    if swap_halves:
        q = np.concatenate((q[:, :, 64:], q[:, :, :64]), axis=2)
    table[:, INDEX0: INDEX0 + MAX_L] = q.sum(axis=0)
    # age a (1 .. v) of row n is entry v[n] - a
    a = np.arange(1, MAX_L + 1)[None, :]                                         # [1, 128]
    entry = v[:, None] - a                                                       # [N, 128]
    ok = (entry >= 0) & counted[:, None]
    by_age = np.where(ok[:, None, :], np.take_along_axis(q, np.broadcast_to(np.clip(entry, 0, MAX_L - 1)[:, None, :], (N, H, MAX_L)), axis=2), 0.0)
    ages = by_age.sum(axis=0)                                                    # [H, 128]
    if age_shift:
        ages = np.concatenate((np.zeros((H, age_shift)), ages[:, : MAX_L - age_shift]), axis=1)
    table[:, AGE0: AGE0 + MAX_L] = ages
    return table


def entropy_bound(rows, L):
    """Absolute error admitted on words 4 and 5: rows (L + 5) 2^-24 ln(max(L, 2)).  Derived, not measured: a term p ln p carries at
    most 3 ulp (logf at 2 ulp -- the device library documents 1 for logf, the wider figure stands -- and one for the product), an fp32
    sum of L terms whose magnitudes sum to at most ln L adds at most L - 1 ulp of that, the division of word 5 one more."""
    return float(rows) * (L + 5) * 2.0 ** -24 * np.log(max(L, 2))


def attention_statistics_inputs(N, H, L, seed):
    """(att [N, H, L] float32, mask [N, L] uint8) of a kernel test: an fp32 softmax of random logits over the valid entries with
    exact zeros elsewhere; v drawn from {0, 1, 2, L - 1, L} and uniformly, with v = 0, 1 and L each forced to occur where N allows;
    a tenth of the samples with a mask that is no prefix (L >= 2); an empty row holds the uniform 1 / L a fully masked softmax
    leaves; some rows are one-hot, some hold a subnormal probability."""
    rng = np.random.default_rng(seed)
    special = np.clip(np.array([0, 1, 2, L - 1, L]), 0, L)
    v = np.where(rng.random(N) < 0.5, rng.choice(special, size=N), rng.integers(0, L + 1, size=N))
    forced = rng.permutation(N)[: min(N, 5)]
    v[forced] = np.array([L, 1, 0, 2, L - 1])[: forced.size].clip(0, L)
    mask = (np.arange(L)[None, :] < v[:, None]).astype(np.uint8)
    if L >= 2:
        for n in np.flatnonzero(rng.random(N) < 0.1):
            if n in forced:
                continue
            m = (rng.random(L) < 0.5).astype(np.uint8)
            k = int(m.sum())
            if (m[:k] != 0).all():               # a prefix by chance: entry 0 open, the last entry set
                m[:] = 0
                m[L - 1] = 1
            mask[n] = m
    logits = 3.0 * rng.normal(size=(N, H, L))
    on = (mask != 0)[:, None, :]
    top = np.where(on, logits, -np.inf).max(axis=2, keepdims=True)
    e = np.where(on, np.exp(logits - np.where(np.isfinite(top), top, 0.0)), 0.0)
    s = e.sum(axis=2, keepdims=True)
    att = np.where(s > 0, e / np.where(s > 0, s, 1.0), 1.0 / L)
    kind = rng.random((N, H))
    for n, h in zip(*np.nonzero(kind < 0.2)):
        idx = np.flatnonzero(mask[n])
        if idx.size == 0:
            continue
        if kind[n, h] < 0.1:                      # one-hot: 0 ln 0 must add 0
            att[n, h] = 0.0
            att[n, h, rng.choice(idx)] = 1.0
        elif idx.size >= 2:                       # a subnormal probability beside the row's largest
            cand = idx[idx != np.argmax(att[n, h])]
            att[n, h, rng.choice(cand)] = 1e-40
    return att.astype(np.float32), mask
