"""previous_step_input on the device: the two kernels of csrc/prev_input.hip through etm.ops and through the C ABI, and the autograd
node that feeds lin_hidden.

Rows kernel: bit for bit utils.previous_step_rows in float32 (both forms of "is there a previous step", strided actions, with and
without the reward row and the bias), +0 rows where there is no previous step, sentinels outside the N x D block untouched.
Gradient kernel: against utils.previous_step_table_grad in float64; the bound is 4 x the error of a float32 torch one-hot product on
the same operands measured in the same run (largest absolute difference over the table), and where that product is exact, one float32
spacing of each result element.  Rows no sample touched are exactly 0, two calls give identical bits.
Refusals: ETM_EINVAL (the literal -1 of include/etm_hip.h) with every sentinel in place.
Linear node: relu(x W^T + e + b) with the addend node against the same layer written WITHOUT the feature -- the twin
relu([x | c] [W | T^T]^T + b) through the existing node, c the one-hot / reward coefficients: the error of the feature against float64
is at most 4 x the twin's own, outputs and every gradient (d table against the twin's d W[:, F:]^T).

Shapes: the smallest that reach every path -- N = 1, one wave (8, 9), more than one workgroup of the rows kernel (37 x 32 > 256
threads), and 2059 = 32 gradient chunks + 11 samples; D = 32 (half the gradient kernel's 64-column tile), 64, 384 (six tiles), 512;
the chunk size - 1 / + 1.

Trainer (4 workers x 8 steps, vector observations of 6 features, or 84 x 84 images where the step kernel's slices matter): the
buffer's fields against utils.previous_step_fields over four rollouts with episode lengths that end one worker's episode at a
rollout's last step and carry the others' over; a key-on trainer against its augmented-observation twin, each against the float64
model (oracle.ref_model) on its own samples, bound 4 x the twin's own error -- the first rollout's values and log-probs,
get_last_value, the bootstrap_truncated values of the recorded cuts (step kernel and unfused road), and the gradients of the first
optimisation step on the same minibatch indices in all three forms of the step --, Discrete and MultiDiscrete, random table; a zero
table under == against a key-absent trainer on images with the per-worker and the group step kernel; the single-episode road
(enjoy.py) replaying an episode of the fused rollout at the per-step bounds; evaluations in between; a checkpoint resumed in place
(captured graphs and eager) and by a fresh trainer; the refusals at construction."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
EINVAL = -1
LAYOUTS = ((2,), (3, 3), (2, 1, 5), (63,))
WIDTHS = (32, 64, 384, 512)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def lib():
    from etm import lib as _lib
    return _lib.load()


def _problem(rng, N, D, sizes, reward, no_prev="some"):
    """(table, actions [N, B] with -1 rows where there is no previous step, rewards or None) as numpy float32 / int64."""
    from utils import previous_step_table_rows
    R = previous_step_table_rows(sizes, reward)
    table = rng.standard_normal((R, D)).astype(np.float32)
    table[rng.random((R, D)) < 0.05] = -0.0                          # (negative zeros: the sum starts at +0)
    actions = np.stack([rng.integers(0, a, size=N) for a in sizes], axis=1).astype(np.int64)
    if no_prev == "some":
        actions[rng.random(N) < 0.3] = -1
    elif no_prev == "all":
        actions[:] = -1
    rewards = (rng.standard_normal(N) * 3).astype(np.float32) if reward else None
    return table, actions, rewards


def _strided(a, dev, pad=3, fill=-5):
    """``a`` [N, B] on the device as a view with row stride B + pad."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.int64, device=dev)
    buf[:, :a.shape[1]] = torch.from_numpy(a).to(dev)
    return buf[:, :a.shape[1]]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", WIDTHS)
def test_rows_kernel_is_the_host_rule_bit_for_bit(dev, sizes, D):
    from etm import ops
    from utils import previous_step_rows
    rng = np.random.default_rng(1000 * D + sum(sizes))
    for N in (1, 8, 9, 37, 2059):
        for reward in (False, True):
            for with_bias in (False, True):
                table, actions, rewards = _problem(rng, N, D, sizes, reward)
                bias = rng.standard_normal(D).astype(np.float32) if with_bias else None
                t_dev = torch.from_numpy(table).to(dev)
                r_dev = None if rewards is None else torch.from_numpy(rewards).to(dev)
                b_dev = None if bias is None else torch.from_numpy(bias).to(dev)
                what = (N, reward, with_bias)

                # training form: a negative action entry = no previous step; strided actions, a strided destination inside sentinels
                buf = torch.full((N + 2, D + 5), SENTINEL, dtype=torch.float32, device=dev)
                ops.prev_input_rows(t_dev, _strided(actions, dev), sizes, r_dev, bias=b_dev, out=buf[1:N + 1, 2:D + 2])
                got = buf.cpu().numpy()
                want = previous_step_rows(table, actions, rewards, sizes, bias=bias, dtype=np.float32)
                assert np.array_equal(_bits(got[1:N + 1, 2:D + 2]), _bits(want)), what
                outside = np.ones(got.shape, dtype=bool)
                outside[1:N + 1, 2:D + 2] = False
                assert (got[outside] == SENTINEL).all(), what
                none = actions[:, 0] < 0
                if not with_bias and none.any():
                    assert (_bits(got[1:N + 1, 2:D + 2][none]) == 0).all(), what          # exactly +0, not -0

                # rollout form: the episode-step word decides, the (stale) actions of such a row are valid indices and not read
                steps = rng.integers(0, 4, size=N).astype(np.int64)
                stale = np.where(actions < 0, 0, actions)
                out = ops.prev_input_rows(t_dev, torch.from_numpy(stale).to(dev), sizes, r_dev, ep_step=torch.from_numpy(steps).to(dev), bias=b_dev)
                want = previous_step_rows(table, np.where(steps[:, None] == 0, -1, stale), rewards, sizes, bias=bias, dtype=np.float32)
                assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), what


def test_rows_kernel_reads_a_pinned_step_block_and_the_reward_row_alone(dev):
    from etm import ops
    from utils import previous_step_rows
    rng = np.random.default_rng(7)
    N, D, sizes = 9, 64, (3, 3)
    table, actions, rewards = _problem(rng, N, D, sizes, True, no_prev="none")
    block = torch.zeros((2, N), dtype=torch.int64).pin_memory()                    # the step kernels' (episode step, slot) block
    block[0] = torch.from_numpy(rng.integers(0, 3, size=N))
    t_dev, r_dev = torch.from_numpy(table).to(dev), torch.from_numpy(rewards).to(dev)
    out = ops.prev_input_rows(t_dev, torch.from_numpy(actions).to(dev), sizes, r_dev, ep_step=block[0])
    want = previous_step_rows(table, np.where(block[0].numpy()[:, None] == 0, -1, actions), rewards, sizes, dtype=np.float32)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    # {action: false, reward: true}: the action rows stay in the table and are never taken
    out = ops.prev_input_rows(t_dev, None, (), r_dev)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(previous_step_rows(table, None, rewards, (), dtype=np.float32)))


def _grad_patterns(rng, N, sizes, reward):
    """name -> (actions, rewards): all samples on one row, no sample with a previous step, every row taken at least once."""
    rewards = (rng.standard_normal(N) * 3).astype(np.float32) if reward else None
    one = np.zeros((N, len(sizes)), dtype=np.int64)
    every = np.stack([(np.arange(N) + b) % a for b, a in enumerate(sizes)], axis=1).astype(np.int64)
    if N < max(sizes):
        every = None                                                 # (fewer samples than rows: the pattern does not exist)
    return {"one_row": (one, rewards), "no_previous_step": (np.full((N, len(sizes)), -1, dtype=np.int64), rewards), "every_row": (every, rewards)}


@pytest.mark.parametrize("sizes", LAYOUTS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("D", (32, 384))
def test_gradient_kernel_against_float64(dev, lib, sizes, D):
    from etm import ops
    from utils import previous_step_coefficients, previous_step_table_grad, previous_step_table_rows
    chunk = lib.etm_prev_input_grad_chunk()
    rng = np.random.default_rng(77 * D + sum(sizes))
    for N in (1, 37, 2059, chunk - 1, chunk + 1):
        for reward in (False, True):
            R = previous_step_table_rows(sizes, reward)
            like = torch.empty((R, D), dtype=torch.float32, device=dev)
            gm_full = rng.standard_normal((N, D + 3)).astype(np.float32)              # a row stride of D + 3
            gm, gm_dev = gm_full[:, :D], torch.from_numpy(gm_full).to(dev)
            for name, (actions, rewards) in _grad_patterns(rng, N, sizes, reward).items():
                if actions is None:
                    continue
                what = (name, N, reward)
                a_dev = _strided(actions, dev)
                r_dev = None if rewards is None else torch.from_numpy(rewards).to(dev)
                got_dev = ops.prev_input_grad(gm_dev[:, :D], like, a_dev, sizes, r_dev)
                got = got_dev.cpu().numpy()
                again = ops.prev_input_grad(gm_dev[:, :D], like, a_dev, sizes, r_dev, out=torch.full_like(got_dev, SENTINEL)).cpu().numpy()
                assert np.array_equal(_bits(got), _bits(again)), what
                ref = previous_step_table_grad(gm, actions, rewards, sizes, R, dtype=np.float64)
                c32 = previous_step_coefficients(actions, rewards, sizes, R, dtype=np.float32)
                torch_got = (torch.from_numpy(c32).to(dev).t() @ gm_dev[:, :D]).cpu().numpy()
                torch_err = np.abs(torch_got.astype(np.float64) - ref).max()
                err = np.abs(got.astype(np.float64) - ref)
                print(f"prev_input_grad {sizes} D={D} {what}: error {err.max():.3e}, float32 one-hot product {torch_err:.3e}")
                if torch_err == 0:
                    assert (err <= np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)).all(), (what, err.max())
                else:
                    assert err.max() <= 4 * torch_err, (what, err.max(), torch_err)
                untouched = np.abs(previous_step_coefficients(actions, rewards, sizes, R)).sum(axis=0) == 0
                if name == "no_previous_step":
                    assert untouched.all()
                assert (_bits(got[untouched]) == 0).all(), what


def _rows_call(lib, dev, **over):
    """One etm_prev_input_rows call at N = 9, D = 64, sizes (3, 3), reward row; ``over`` replaces named arguments.  -> (code, every
    output buffer)."""
    N, D, R = 9, 64, 7
    t = dict(table=torch.ones((R, D), device=dev), actions=torch.zeros((N, 2), dtype=torch.int64, device=dev),
             rewards=torch.ones(N, device=dev), ep_step=torch.ones(N, dtype=torch.int64, device=dev), bias=torch.ones(D, device=dev),
             out=torch.full((N, D), SENTINEL, device=dev))
    sizes = (ctypes.c_int32 * 2)(3, 3)
    a = dict(R=R, D=D, act_stride=2, sizes=sizes, n_branches=2, out_stride=D, N=N, **{k: v.data_ptr() for k, v in t.items()})
    for k, v in over.items():
        a[k] = a[v[1]] + 2 if isinstance(v, tuple) else v
    rc = lib.etm_prev_input_rows(a["table"], a["R"], a["D"], a["actions"], a["act_stride"], a["sizes"], a["n_branches"], a["rewards"],
                                 a["ep_step"], a["bias"], a["out"], a["out_stride"], a["N"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, [t["out"]]


def _grad_call(lib, dev, **over):
    N, D, R = 9, 64, 7
    nbytes = lib.etm_prev_input_grad_workspace_bytes(N, R, D)
    t = dict(gm=torch.ones((N, D), device=dev), actions=torch.zeros((N, 2), dtype=torch.int64, device=dev), rewards=torch.ones(N, device=dev),
             d_table=torch.full((R, D), SENTINEL, device=dev), workspace=torch.full((nbytes // 4,), SENTINEL, device=dev))
    sizes = (ctypes.c_int32 * 2)(3, 3)
    a = dict(R=R, D=D, act_stride=2, sizes=sizes, n_branches=2, gm_stride=D, N=N, workspace_bytes=nbytes, **{k: v.data_ptr() for k, v in t.items()})
    for k, v in over.items():
        a[k] = a[v[1]] + 2 if isinstance(v, tuple) else v
    rc = lib.etm_prev_input_grad(a["gm"], a["gm_stride"], a["actions"], a["act_stride"], a["sizes"], a["n_branches"], a["rewards"], a["d_table"],
                                 a["R"], a["D"], a["N"], a["workspace"], a["workspace_bytes"], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, [t["d_table"], t["workspace"]]


def _off2(name):
    return {name: ("+2", name)}


COMMON_DEFECTS = [("NULL actions", dict(actions=None)), ("actions off by 2 bytes", _off2("actions")), ("NULL sizes", dict(sizes=None)),
                  ("rewards off by 2 bytes", _off2("rewards")), ("act_stride below B", dict(act_stride=1)), ("R = 0", dict(R=0)),
                  ("R = 65", dict(R=65)), ("R below the layout", dict(R=6)), ("D = 0", dict(D=0)), ("N = 0", dict(N=0)),
                  ("17 branches", dict(n_branches=17)), ("nothing fed back", dict(n_branches=0, rewards=None))]
ROWS_DEFECTS = COMMON_DEFECTS + [("NULL table", dict(table=None)), ("table off by 2 bytes", _off2("table")), ("NULL out", dict(out=None)),
                                 ("out off by 2 bytes", _off2("out")), ("bias off by 2 bytes", _off2("bias")),
                                 ("ep_step off by 2 bytes", _off2("ep_step")), ("out_stride below D", dict(out_stride=63))]
GRAD_DEFECTS = COMMON_DEFECTS + [("NULL gm", dict(gm=None)), ("gm off by 2 bytes", _off2("gm")), ("d_table off by 2 bytes", _off2("d_table")),
                                 ("NULL workspace", dict(workspace=None)), ("workspace off by 2 bytes", _off2("workspace")),
                                 ("gm_stride below D", dict(gm_stride=63))]


def test_entry_refusals_launch_nothing(lib, dev):
    for call, defects in ((_rows_call, ROWS_DEFECTS), (_grad_call, GRAD_DEFECTS)):
        rc, outs = call(lib, dev)
        assert rc == 0 and all((o != SENTINEL).any() for o in outs[:1]), call.__name__
        for name, over in defects:
            rc, outs = call(lib, dev, **over)
            assert rc == EINVAL, (call.__name__, name, rc)
            assert all(bool((o == SENTINEL).all()) for o in outs), (call.__name__, name)
    rc, outs = _grad_call(lib, dev, workspace_bytes=4)
    assert rc == -3 and all(bool((o == SENTINEL).all()) for o in outs)          # ETM_EWORKSPACE
    assert [lib.etm_prev_input_supported(r, 64) for r in (0, 1, 64, 65)] == [0, 1, 1, 0]
    assert lib.etm_prev_input_supported(7, 0) == 0


def _twin_errors(dev, nhwc, sizes, reward):
    """(name -> (error of the feature, error of the twin)) against float64, for relu(x W^T + e + b) and its gradients."""
    from etm import ops
    from utils import previous_step_coefficients, previous_step_table_rows
    rng = np.random.default_rng(5 + sum(sizes) + reward)
    N, C, HW, D = 37, 4, 6, 64
    F = C * HW
    R = previous_step_table_rows(sizes, reward)
    table, actions, rewards = _problem(rng, N, D, sizes, reward)
    x = rng.standard_normal((N, F)).astype(np.float32)
    W = (rng.standard_normal((D, F)) / np.sqrt(F)).astype(np.float32)
    b = rng.standard_normal(D).astype(np.float32)
    gy = rng.standard_normal((N, D)).astype(np.float32)
    c = previous_step_coefficients(actions, rewards, sizes, R, dtype=np.float32)

    def perm(w):                       # the (c, h, w) -> (h, w, c) column order of the NHWC node
        return w.reshape(D, C, HW).transpose(0, 2, 1).reshape(D, F)

    # float64: y = relu(x Wp^T + c T + b)
    t64 = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, W, b, table)]
    wp64 = t64[1].view(D, C, HW).transpose(1, 2).reshape(D, F) if nhwc else t64[1]
    y64 = torch.relu(t64[0] @ wp64.t() + torch.tensor(c, dtype=torch.float64) @ t64[3] + t64[2])
    g64 = torch.autograd.grad(y64, t64, torch.tensor(gy, dtype=torch.float64))
    ref = dict(y=y64.detach().numpy(), dx=g64[0].numpy(), dW=g64[1].numpy(), db=g64[2].numpy(), dT=g64[3].numpy())

    def leaf(v):
        return torch.from_numpy(np.ascontiguousarray(v)).to(dev).requires_grad_(True)

    # the feature
    xd, wd, bd, td = leaf(x), leaf(W), leaf(b), leaf(table)
    a_dev = torch.from_numpy(actions).to(dev)
    r_dev = None if rewards is None else torch.from_numpy(rewards).to(dev)
    addend = ops.prev_input_addend(td, a_dev, sizes, r_dev, bias=bd)
    y = ops.linear_relu_nhwc(xd, wd, bd, C, addend=addend) if nhwc else ops.linear_relu_train(xd, wd, bd, addend=addend)
    g = torch.autograd.grad(y, (xd, wd, bd, td), torch.from_numpy(gy).to(dev))
    got = dict(y=y.detach(), dx=g[0], dW=g[1], db=g[2], dT=g[3])

    # the twin: the same layer without the feature, observation [x | c], weight [W | T^T]
    if nhwc:                           # (the NHWC node permutes columns by channel: the twin is written on the permuted problem)
        xa, wa = np.concatenate([x, c], axis=1), np.concatenate([perm(W), table.T], axis=1)
    else:
        xa, wa = np.concatenate([x, c], axis=1), np.concatenate([W, table.T], axis=1)
    xad, wad, bad = leaf(xa), leaf(wa), leaf(b)
    ya = ops.linear_relu_train(xad, wad, bad)
    ga = torch.autograd.grad(ya, (xad, wad, bad), torch.from_numpy(gy).to(dev))
    dwa = ga[1].cpu().numpy()
    twin_dw = dwa[:, :F]
    if nhwc:                           # back to the (c, h, w) column order
        twin_dw = twin_dw.reshape(D, HW, C).transpose(0, 2, 1).reshape(D, F)
    twin = dict(y=ya.detach().cpu().numpy(), dx=ga[0].cpu().numpy()[:, :F], dW=twin_dw, db=ga[2].cpu().numpy(), dT=dwa[:, F:].T)
    out = {}
    for k in ref:
        out[k] = (np.abs(got[k].cpu().numpy().astype(np.float64) - ref[k]).max(), np.abs(twin[k].astype(np.float64) - ref[k]).max(),
                  np.abs(ref[k]).max())
    untouched = np.abs(c).sum(axis=0) == 0
    assert (_bits(got["dT"].cpu().numpy()[untouched]) == 0).all()
    return out


@pytest.mark.parametrize("nhwc", (False, True), ids=("linear", "nhwc"))
@pytest.mark.parametrize("sizes,reward", (((3,), True), ((2, 1, 5), True), ((3, 3), False)), ids=("discrete", "multidiscrete", "no_reward"))
def test_linear_node_with_addend_against_its_twin(dev, nhwc, sizes, reward):
    for name, (err, twin_err, scale) in _twin_errors(dev, nhwc, sizes, reward).items():
        print(f"linear node {'nhwc' if nhwc else 'plain'} {sizes} reward={reward} {name}: error {err:.3e}, twin {twin_err:.3e}, ratio "
              f"{err / twin_err if twin_err else float('nan'):.2f}")
        bound = 4 * twin_err if twin_err > 0 else float(np.spacing(np.float32(scale)))
        assert err <= bound, (name, err, twin_err)


def test_linear_node_without_addend_is_unchanged(dev):
    """addend=None: the same node arguments, the same bits as the call that never knew the argument."""
    from etm import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    x, w, b = (torch.randn(s, generator=g).to(dev).requires_grad_(True) for s in ((37, 24), (64, 24), (64,)))
    gy = torch.randn((37, 64), generator=g).to(dev)
    for fn, base in ((lambda: ops.linear_relu_train(x, w, b, addend=None), lambda: ops._LinearFn.apply(x, w, b, True)),
                     (lambda: ops.linear_relu_nhwc(x, w, b, 4, addend=None), lambda: ops._LinearReluNhwcFn.apply(x, w, b, 4))):
        y0, y1 = fn(), base()
        assert torch.equal(y0, y1)
        for a, c in zip(torch.autograd.grad(y0, (x, w, b), gy), torch.autograd.grad(y1, (x, w, b), gy)):
            assert torch.equal(a, c)


# ------------------------------------------------------------------------------------------------ the trainer
class _NoisyEnv:
    """A vector environment for these tests: Gaussian observations and rewards from its own generator, episodes of a fixed length,
    Discrete or MultiDiscrete actions (which change nothing: two environments with one seed emit the same rows whatever is played).
    Every episode end is reported as a time-limit cut (``bootstrap_truncated`` then records it; without the key the flag is dropped)."""

    def __init__(self, nvec, features, episode_len, max_len, seed):
        from types import SimpleNamespace
        self.nvec, self.F, self.episode_len, self.max_episode_steps = tuple(nvec), features, episode_len, max_len
        self.observation_space = SimpleNamespace(shape=(features,), dtype=np.float32)
        self.action_space = SimpleNamespace(n=nvec[0]) if len(nvec) == 1 else SimpleNamespace(nvec=np.asarray(nvec))
        self._rng = np.random.default_rng(seed)
        self._t = 0

    def reset(self, **kw):
        self._t = 0
        return self._rng.standard_normal(self.F).astype(np.float32)

    def step(self, action):
        self._t += 1
        reward = float(np.float32(self._rng.standard_normal()))
        done = self._t >= self.episode_len
        return self._rng.standard_normal(self.F).astype(np.float32), reward, done, ({"reward": 0.0, "length": self._t, "truncated": True} if done else None)

    def close(self):
        return None


class _AugmentedEnv(_NoisyEnv):
    """The same environment with [one-hot(previous action) per branch, previous reward] appended to the observation, zeros at an
    episode's first step: what a key-absent trainer needs to be the key-on trainer's twin."""

    def __init__(self, nvec, features, episode_len, max_len, seed):
        super().__init__(nvec, features, episode_len, max_len, seed)
        from types import SimpleNamespace
        self.extra = sum(nvec) + 1
        self.observation_space = SimpleNamespace(shape=(features + self.extra,), dtype=np.float32)

    def reset(self, **kw):
        return np.concatenate([super().reset(), np.zeros(self.extra, dtype=np.float32)])

    def step(self, action):
        obs, reward, done, info = super().step(action)
        tail, off = np.zeros(self.extra, dtype=np.float32), 0
        for b, a in enumerate(np.asarray(action).reshape(-1)):
            tail[off + int(a)] = 1.0
            off += self.nvec[b]
        tail[-1] = np.float32(reward)
        return np.concatenate([obs, tail]), reward, done, info


EPISODE_LENS = (12, 8, 5, 11)            # S = 8: worker 1's episodes end at a rollout's LAST step, the others carry a live episode over
FEATURES = 6


def _vec_env(kind, nvec):
    from environments.vec_env import SerialVecEnv
    return SerialVecEnv([kind(nvec, FEATURES, n, max(EPISODE_LENS), seed=100 + w) for w, n in enumerate(EPISODE_LENS)])


def _trainer_config(key, **over):
    cfg = dict(environment=dict(type="supplied"), gamma=0.99, lamda=0.95, updates=1, epochs=1, n_workers=len(EPISODE_LENS), worker_steps=8,
               n_mini_batch=2, value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5, tunable_gemm=False,
               transformer=dict(num_blocks=2, embed_dim=64, num_heads=2, memory_length=4, positional_encoding="relative", layer_norm="post",
                                gtrxl=False, gtrxl_bias=0.0),
               learning_rate_schedule=dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10),
               beta_schedule=dict(initial=1e-3, final=1e-3, power=1.0, max_decay_steps=10),
               clip_range_schedule=dict(initial=0.1, final=0.1, power=1.0, max_decay_steps=10))
    if key is not None:
        cfg["previous_step_input"] = key
    cfg.update(over)
    return cfg


def _forced(nvec, W, S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, a, (W, S), generator=g) for a in nvec], dim=2)


@pytest.mark.parametrize("nvec", ((3,), (2, 1, 3)), ids=("discrete", "multidiscrete"))
def test_buffer_fields_follow_the_host_rule_over_rollouts(dev, nvec):
    from trainer import PPOTrainer
    from utils import previous_step_fields
    torch.manual_seed(5)
    tr = PPOTrainer(_trainer_config(True), run_id="prevfields", device=dev, tensorboard=False, env=_vec_env(_NoisyEnv, nvec))
    try:
        carry, saw_end_at_last, saw_live = (None, None, None), False, False
        for r in range(4):
            tr._sample_training_data(forced_actions=_forced(nvec, 4, 8, seed=r))
            tr.buffer.prepare_batch_dict()
            torch.cuda.synchronize()
            b = tr.buffer
            pa, pr, carry = previous_step_fields(b.actions.cpu().numpy(), b.rewards.copy(), b.dones.copy(), *carry)
            assert np.array_equal(b.prev_actions.cpu().numpy(), pa), r
            assert np.array_equal(_bits(b.prev_rewards.cpu().numpy()), _bits(pr)), r
            assert tuple(b.samples_flat["prev_actions"].shape) == (32, len(nvec)) and tuple(b.samples_flat["prev_rewards"].shape) == (32,)
            saw_end_at_last |= bool(b.dones[:, -1].any())
            saw_live |= bool((~b.dones[:, -1]).any()) and r > 0 and bool((pa[:, 0, 0] >= 0).any())
        assert saw_end_at_last and saw_live
    finally:
        tr.close()


def _steps_of(s0, dones):
    W, S = dones.shape
    steps, s = np.zeros((W, S), dtype=np.int64), s0.astype(np.int64).copy()
    for t in range(S):
        steps[:, t] = s
        s = np.where(dones[:, t], 0, s + 1)
    return steps


def _model64(tr, sd64, obs_aug, slot, rows, pidx, mask, steps):
    """The float64 model ``sd64`` (oracle.ref_model; the twin's weights) on the augmented observations ``obs_aug`` over trainer ``tr``'s
    own memory rows ``bank[slot, rows]`` (rows at or past the episode step ``steps`` are empty), positions ``pidx`` -> (logits, value)."""
    from oracle import ref_model as rm
    cfg = tr.config
    win = tr.buffer.bank[slot[:, None], rows].double()
    win = win * (rows < steps[:, None]).to(win.dtype)[:, :, None, None]
    pos = tr.model.transformer._pos()
    if pos is not None:
        win = win + pos.detach().double()[pidx].unsqueeze(2)
    ocfg = dict(cfg, transformer=dict(cfg["transformer"], positional_encoding="none"))
    logits, value, _ = rm.actor_critic(sd64, ocfg, obs_aug.double(), win, mask, pidx, tr.max_episode_length)
    return logits, value


def _rollout_samples(tr, s0):
    """(slot, rows, pidx, mask, steps) of the N = W S samples of the rollout in ``tr``'s buffer."""
    b = tr.buffer
    W, S = b.dones.shape
    flat = lambda x: x.reshape(W * S, *x.shape[2:])
    steps = torch.from_numpy(_steps_of(s0, b.dones.copy())).reshape(W * S).to(tr.device)
    return flat(b.memory_index), flat(b.memory_indices), flat(b.memory_indices), flat(b.memory_mask), steps


def _errors_against_float64(tr, sd64, obs_aug, s0):
    """Largest absolute error of the first rollout's values and log-probs of trainer ``tr`` against the float64 model."""
    b = tr.buffer
    N = b.batch_size
    flat = lambda x: x.reshape(N, *x.shape[2:])
    with torch.no_grad():
        logits, value = _model64(tr, sd64, obs_aug, *_rollout_samples(tr, s0))
    err_v = float((flat(b.values).double() - value).abs().max())
    err_lp = 0.0
    for k, lg in enumerate(logits):
        ref = torch.log_softmax(lg, dim=-1).gather(1, flat(b.actions)[:, k:k + 1])[:, 0]
        err_lp = max(err_lp, float((flat(b.log_probs)[:, k].double() - ref).abs().max()))
    return err_v, err_lp


def _last_value_error(tr, sd64, obs_aug_now):
    """get_last_value's output against the float64 model on the observation after the last step, with its window rule: rows
    [clip(step - L, 0), +L) of the worker's slot, mask row clip(step, 0, L - 1), the positions of the last stored step."""
    L, dev = tr.memory_length, tr.device
    step = torch.from_numpy(tr.worker_current_episode_step.astype(np.int64)).to(dev)
    slot = torch.from_numpy(tr.worker_episode_slot.astype(np.int64)).to(dev)
    rows = torch.clamp(step - L, min=0).unsqueeze(1) + torch.arange(L, device=dev).unsqueeze(0)
    mask = tr._mask_table[torch.clamp(step, 0, L - 1)]
    with torch.no_grad():
        _, value = _model64(tr, sd64, obs_aug_now, slot, rows, tr.buffer.memory_indices[:, -1], mask, step)
    return float((tr._lv.out.double() - value).abs().max())


def _spy_bootstrap(tr):
    """Records what the bootstrap pass of ``tr`` hands to its forward: (n, w, t, (obs, slot, rows, pidx, s, ...))."""
    seen, orig = {}, tr._bootstrap_operands

    def spy(recs, chunk):
        seen["operands"] = orig(recs, chunk)
        return seen["operands"]

    tr._bootstrap_operands = spy
    return seen


def _bootstrap_error(tr, seen, sd64, obs_aug_final):
    """The bootstrap values of the recorded cuts against the float64 model on the (augmented) final observations."""
    n, w, t, (obs, slot, rows, pidx, s) = seen["operands"][0], seen["operands"][1], seen["operands"][2], seen["operands"][3][:5]
    mask = tr._mask_table[torch.clamp(s, 0, tr.memory_length - 1)]
    with torch.no_grad():
        _, value = _model64(tr, sd64, obs_aug_final[:n], slot[:n], rows[:n], pidx[:n], mask[:n], s[:n])
    return float((tr.buffer.bootstrap_values[w[:n], t[:n]].double() - value).abs().max())


def _twin_pair(dev, nvec, **over):
    """A key-on trainer with a random table and its key-absent twin on the augmented observations, lin_hidden.weight = [W | T^T], every
    other parameter equal; ``bootstrap_truncated`` on (the test environments report every episode end as a time-limit cut)."""
    from trainer import PPOTrainer
    over = dict(over, bootstrap_truncated=True)
    torch.manual_seed(9)
    on = PPOTrainer(_trainer_config(True, **over), run_id="prevon", device=dev, tensorboard=False, env=_vec_env(_NoisyEnv, nvec))
    torch.manual_seed(9)
    twin = PPOTrainer(_trainer_config(None, **over), run_id="prevtwin", device=dev, tensorboard=False, env=_vec_env(_AugmentedEnv, nvec))
    assert "prev_input.weight" in on.model.state_dict() and "prev_input.weight" not in twin.model.state_dict()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        on.model.prev_input.weight.copy_((0.5 * torch.randn(on.model.prev_input.weight.shape, generator=g)).to(dev))
        sd_on = on.model.state_dict()
        for name, p in twin.model.named_parameters():
            if name == "lin_hidden.weight":
                p.copy_(torch.cat([sd_on[name], sd_on["prev_input.weight"].t()], dim=1))
            else:
                p.copy_(sd_on[name])
    return on, twin


def _first_rollout(on, twin, nvec):
    """The same forced actions through both trainers -> (s0, the augmented observations [32, F + extra], the bootstrap spies)."""
    forced = _forced(nvec, 4, 8, seed=1)
    s0 = on.worker_current_episode_step.copy()
    spies = [_spy_bootstrap(tr) for tr in (on, twin)]
    for tr in (on, twin):
        torch.manual_seed(11)
        tr._sample_training_data(forced_actions=forced)
        tr.buffer.prepare_batch_dict()
    torch.cuda.synchronize()
    assert torch.equal(on.buffer.actions, twin.buffer.actions) and torch.equal(on.buffer.actions.cpu(), forced)
    obs_aug = twin.buffer.obs.reshape(32, -1)
    assert torch.equal(obs_aug[:, :FEATURES], on.buffer.obs.reshape(32, -1))
    return s0, obs_aug, spies


@pytest.mark.parametrize("nvec", ((3,), (2, 1, 3)), ids=("discrete", "multidiscrete"))
@pytest.mark.parametrize("fused", (True, False), ids=("step_kernel", "unfused"))
def test_first_rollout_equals_the_augmented_observation_twin(dev, nvec, fused):
    """A key-on trainer is a key-absent trainer whose observation has [one-hot(a_prev), r_prev] appended and whose lin_hidden.weight is
    [W | T^T]: with a random table and the same forced actions, its values and log-probs, get_last_value's output and the
    ``bootstrap_truncated`` values of the recorded cuts are each at most 4 x as far from the float64 model as the twin's own (all
    measured in this run, each on its own samples)."""
    on, twin = _twin_pair(dev, nvec, fused_rollout_block=fused)
    try:
        s0, obs_aug, (spy_on, spy_twin) = _first_rollout(on, twin, nvec)
        assert (on.model._rf is not None) == fused and (twin.model._rf is not None) == fused
        if fused:      # the step kernel's two-slice input: x W^T, the previous step's term
            assert all(g.h_part is not None and g.h_part.shape[0] == 2 for g in on._groups)
        sd64 = {k: v.detach().double() for k, v in twin.model.state_dict().items()}
        road = "step kernel" if fused else "unfused"
        e_on, e_twin = _errors_against_float64(on, sd64, obs_aug, s0), _errors_against_float64(twin, sd64, obs_aug, s0)
        # the observation after the last step: the twin's pinned rows are the augmented ones
        now = twin._obs_pin.to(dev)
        assert torch.equal(now[:, :FEATURES], on._obs_pin.to(dev)) and int((on.worker_current_episode_step > 0).sum()) == 3
        e_on += (_last_value_error(on, sd64, now),)
        e_twin += (_last_value_error(twin, sd64, now),)
        # the cuts: worker 1 at its step 7 (episode length 8) and worker 2 at its step 4 (length 5)
        assert [r[:2] for r in on.last_truncations] == [r[:2] for r in twin.last_truncations] and len(on.last_truncations) == 2
        final = spy_twin["operands"][3][0]
        assert torch.equal(final[:, :FEATURES], spy_on["operands"][3][0])
        e_on += (_bootstrap_error(on, spy_on, sd64, final),)
        e_twin += (_bootstrap_error(twin, spy_twin, sd64, final),)
        for what, a, c in zip(("values", "log-probs", "last value", "bootstrap values"), e_on, e_twin):
            print(f"previous_step_input {nvec} {road} {what}: error {a:.3e}, twin {c:.3e}, ratio {a / c if c else float('nan'):.2f}")
            assert a <= (4 * c if c > 0 else float(np.spacing(np.float32(1.0)))), (what, a, c)
    finally:
        on.close()
        twin.close()


STEP_FORMS = (("tables", {}), ("ends_unfused", dict(step_ends_fused=False)), ("eager", dict(hip_graph_train=False)))


@pytest.mark.parametrize("nvec", ((3,), (2, 1, 3)), ids=("discrete", "multidiscrete"))
@pytest.mark.parametrize("form", STEP_FORMS, ids=[f[0] for f in STEP_FORMS])
def test_first_step_gradients_equal_the_twins(dev, nvec, form):
    """After the first rollout, the gradient of the PPO loss on the same minibatch indices through the trainer (samples_flat -> the
    minibatch gather -> PreviousStep -> the addend node -> the arena): ``d table`` against the float64 ``d W+[:, F:]^T`` and every other
    gradient tensor against its float64 twin, each at most 4 x the twin trainer's own error (||g - g64|| / ||g64|| per tensor; each
    trainer against float64 autograd over its own buffer rows).  In the captured step with tables, with ``step_ends_fused: false`` and
    in the eager step; an update in that form then runs and moves the table."""
    from oracle import ref_algo as ra
    on, twin = _twin_pair(dev, nvec, epochs=3, **form[1])
    try:
        s0, obs_aug, _ = _first_rollout(on, twin, nvec)
        idx = torch.arange(1, 32, 2, device=dev)
        clip, beta, F = 0.1, 1e-3, FEATURES
        names = [n for n, p in twin.model.named_parameters() if p.requires_grad]
        errors = {}
        for which, tr in (("on", on), ("twin", twin)):
            got = tr.minibatch_gradients(idx, clip, beta)
            sd = {k: v.detach().double().requires_grad_(k in names) for k, v in twin.model.state_dict().items()}
            sf = tr.buffer.samples_flat
            sel = lambda x: x.index_select(0, idx)
            logits, value = _model64(tr, sd, sel(obs_aug), *(sel(x) for x in _rollout_samples(tr, s0)))
            loss, _ = ra.ppo_loss(logits, value, sel(sf["actions"]), sel(sf["log_probs"]).double(), sel(sf["advantages"]).double(),
                                  sel(sf["values"]).double(), clip, tr.config["value_loss_coefficient"], beta)
            ref = dict(zip(names, torch.autograd.grad(loss, [sd[n] for n in names])))
            # the key-on trainer's tensors: lin_hidden.weight is W+'s first F columns, the table its other columns, transposed ...
            ref["prev_input.weight"] = ref["lin_hidden.weight"][:, F:].t()
            ref["lin_hidden.weight"] = ref["lin_hidden.weight"][:, :F]
            if which == "twin":     # ... and the twin's error is taken on the same two pieces
                got = dict(got)
                got["prev_input.weight"] = got["lin_hidden.weight"][:, F:].t()
                got["lin_hidden.weight"] = got["lin_hidden.weight"][:, :F]
            assert set(got) == set(ref)
            errors[which] = {n: float((got[n].double() - ref[n]).norm() / ref[n].norm().clamp(min=1e-300)) for n in ref}
            assert float(ref["prev_input.weight"].norm()) > 0 and float(ref["lin_hidden.bias"].norm()) > 0
        worst = max(errors["on"], key=lambda n: errors["on"][n] / max(errors["twin"][n], 1e-300))
        print(f"previous_step_input {nvec} {form[0]} gradients: d table {errors['on']['prev_input.weight']:.3e} / twin "
              f"{errors['twin']['prev_input.weight']:.3e} = {errors['on']['prev_input.weight'] / errors['twin']['prev_input.weight']:.2f}; largest "
              f"ratio {errors['on'][worst] / errors['twin'][worst]:.2f} ({worst}: {errors['on'][worst]:.3e} / {errors['twin'][worst]:.3e})")
        for n in errors["on"]:
            assert errors["on"][n] <= 4 * errors["twin"][n], (n, errors["on"][n], errors["twin"][n])
        before = on.model.prev_input.weight.detach().clone()
        stats, norms = on._train_epochs(3e-4, clip, beta)
        torch.cuda.synchronize()
        assert np.isfinite(np.asarray(stats)).all() and (on._train_graph is not None) == (form[0] != "eager") and "linear_layer" in norms
        assert not torch.equal(on.model.prev_input.weight.detach(), before)
    finally:
        on.close()
        twin.close()


IMAGE = dict(type="Synthetic", obs_shape=[3, 84, 84], num_actions=3, max_episode_steps=6, seed=0, p_done=0.05, pool=8)


@pytest.mark.parametrize("group", (False, True), ids=("worker_kernel", "group_kernel"))
def test_zero_table_is_harmless_on_images(dev, group):
    """With the table left at zero a key-on trainer's first rollout equals a key-absent trainer's under ==."""
    from trainer import PPOTrainer
    tcfg = (dict(num_blocks=2, embed_dim=128, num_heads=4, memory_length=4, positional_encoding="", layer_norm="pre", gtrxl=True, gtrxl_bias=0.0)
            if group else _trainer_config(None)["transformer"])
    got = []
    for key in (None, True):
        torch.manual_seed(21)
        cfg = _trainer_config(key, environment=dict(IMAGE), transformer=tcfg, hidden_layer_size=tcfg["embed_dim"])
        tr = PPOTrainer(cfg, run_id="prevzero", device=dev, tensorboard=False)
        try:
            torch.manual_seed(22)
            tr._sample_training_data()
            torch.cuda.synchronize()
            assert all(g.group_kernel == group and g.rf_scratch is not None for g in tr._groups)
            if key:
                assert all(g.h_part is not None and g.h_part.shape[0] in (50, 17) for g in tr._groups)       # one slice more than 49 / 16
                assert float(tr.model.prev_input.weight.detach().abs().max()) == 0.0
            b = tr.buffer
            got.append([x.clone() for x in (b.actions, b.log_probs, b.values, b.advantages, b.bank[: b.num_episodes])])
        finally:
            tr.close()
    for a, c in zip(*got):
        assert torch.equal(a, c)


def test_optimisation_step_moves_the_table_in_every_form(dev):
    """The captured step with tables, ``step_ends_fused: false`` and the eager step: the table's gradient of one minibatch is the same
    bits whether the gradient kernel writes the arena view (the collector claims it) or autograd's tensor is packed
    (``grouped_dw_train: false``) -- one deterministic kernel on the same operands --, and an update moves the table."""
    from trainer import PPOTrainer
    grads = {}
    for name, over in (("tables", {}), ("ends_unfused", dict(step_ends_fused=False)), ("eager", dict(hip_graph_train=False)),
                       ("own_products", dict(grouped_dw_train=False))):
        torch.manual_seed(31)
        tr = PPOTrainer(_trainer_config(True, epochs=3, **over), run_id="prevstep", device=dev, tensorboard=False, env=_vec_env(_NoisyEnv, (2, 1, 3)))
        try:
            torch.manual_seed(32)
            tr._sample_training_data(forced_actions=_forced((2, 1, 3), 4, 8, seed=2))
            tr.buffer.prepare_batch_dict()
            grads[name] = tr.minibatch_gradients(torch.arange(0, 32, 2), 0.1, 1e-3)["prev_input.weight"].clone()
            stats, norms = tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            assert np.isfinite(np.asarray(stats)).all()
            assert (tr._train_graph is not None) == (name != "eager")
            assert float(tr.model.prev_input.weight.detach().abs().max()) > 0
            assert "linear_layer" in norms
        finally:
            tr.close()
    assert float(grads["tables"].abs().max()) > 0
    for name in ("ends_unfused", "eager", "own_products"):
        assert torch.equal(grads[name], grads["tables"]), name


def test_trainer_refuses_what_the_feature_does_not_carry(dev):
    from trainer import PPOTrainer
    for bad, match in ((dict(previous_step_input={"action": False, "reward": False}), "at least one"),
                       (dict(previous_step_input=True, worker_processes=True), "worker_processes: false"),
                       (dict(previous_step_input=True, environment=dict(IMAGE, num_actions=64)), "65 rows"),
                       (dict(previous_step_input=True, environment=dict(type="Synthetic", obs_shape=[4], num_actions=2, max_episode_steps=8,
                                                                        seed=0, continuous_actions=2)), "Box policy")):
        with pytest.raises(ValueError, match=match):
            PPOTrainer(_trainer_config(None, **{"environment": dict(IMAGE), **bad}), run_id="prevbad", device=dev, tensorboard=False)


class _Recorded:
    """A model front that records what ``enjoy.run_episode`` hands to the model and gets back, step by step."""

    def __init__(self, model):
        self._model, self.calls = model, []

    def __getattr__(self, name):
        return getattr(self._model, name)

    def __call__(self, *args, **kw):
        policy, value, memory = self._model(*args, **kw)
        self.calls.append((kw.get("prev"), [p.logits.detach() for p in policy], value.detach()))
        return policy, value, memory


@pytest.mark.parametrize("nvec", ((3,), (2, 1, 3)), ids=("discrete", "multidiscrete"))
def test_single_episode_road_agrees_with_the_fused_rollout(dev, nvec):
    """enjoy.run_episode replays worker 1's first episode (8 steps; the environment emits the same rows whatever is played) on the
    key-on trainer's model with a random table, greedy on both roads: the same actions, the previous step handed over is the action
    and the raw reward of the step before (none at step 0), and per step the value and the taken actions' log-probs agree with the
    fused rollout's to the per-step bounds of tests/test_rollout_step_vs_float64.py.  The encoder's two device forms (the rollout's, no
    grad; the autograd node's) give the same bits, and a pass without the previous step is refused."""
    import enjoy
    from model import PreviousStep
    from test_rollout_step_vs_float64 import BOUNDS
    from trainer import PPOTrainer
    torch.manual_seed(9)
    tr = PPOTrainer(_trainer_config(True), run_id="prevenjoy", device=dev, tensorboard=False, env=_vec_env(_NoisyEnv, nvec))
    try:
        with torch.no_grad():
            tr.model.prev_input.weight.normal_(0.0, 0.5)
            for head in tr.model.policy_branches:          # (well separated logits: the greedy action is no near-tie)
                head.weight.mul_(30.0)
        tr._sample_training_data(deterministic=True)
        torch.cuda.synchronize()
        b, w, n = tr.buffer, 1, EPISODE_LENS[1]
        assert bool(b.dones[w, n - 1]) and not b.dones[w, :n - 1].any()
        front = _Recorded(tr.model)
        env = _NoisyEnv(nvec, FEATURES, n, max(EPISODE_LENS), seed=100 + w)
        rewards, info = enjoy.run_episode(front, env, tr.config, dev, deterministic=True)
        assert len(rewards) == n == len(front.calls) and info["length"] == n
        assert np.array_equal(np.asarray(rewards, dtype=np.float32), b.rewards[w, :n])
        worst_v = worst_lp = 0.0
        for t, (prev, logits, value) in enumerate(front.calls):
            assert int(prev.ep_step[0]) == t
            if t > 0:
                assert prev.actions[0].tolist() == b.actions[w, t - 1].tolist() and float(prev.rewards[0]) == float(b.rewards[w, t - 1])
            for k, lg in enumerate(logits):
                a = int(b.actions[w, t, k])
                assert int(lg.argmax(dim=-1)) == a, (t, k)
                lp, ref = float(torch.log_softmax(lg.double(), dim=-1)[0, a]), float(b.log_probs[w, t, k])
                worst_lp = max(worst_lp, abs(lp - ref) / max(1.0, abs(ref)))
            worst_v = max(worst_v, abs(float(value[0]) - float(b.values[w, t])) / max(1.0, abs(float(b.values[w, t]))))
        print(f"previous_step_input {nvec} single-episode road against the fused rollout: value {worst_v:.3e}, log-prob {worst_lp:.3e}")
        assert worst_v <= BOUNDS["value"] and worst_lp <= BOUNDS["logp"], (worst_v, worst_lp)
        model = tr.model
        obs = torch.randn((5, FEATURES), device=dev)
        B = len(nvec)
        prev = PreviousStep(torch.zeros((5, B), dtype=torch.int64, device=dev), torch.tensor([1.0, 0.0, -2.5, 0.5, 3.0], device=dev),
                            torch.tensor([0, 3, 1, 0, 2], device=dev))
        with torch.no_grad():
            x = model._encode(obs, prev=prev)
        y = model._encode(obs, prev=prev)
        assert y.requires_grad and torch.equal(x, y.detach())
        with pytest.raises(ValueError, match="needs the previous step"):
            model._encode(obs)
    finally:
        tr.close()


VECTOR = dict(type="Synthetic", obs_shape=[7], num_actions=3, max_episode_steps=12, seed=2, p_done=0.1, pool=4)


def _two_updates(dev, evaluate):
    """Two updates of a key-on trainer from a fixed seed -> the device state after each (``evaluate``: an evaluation after each)."""
    from trainer import PPOTrainer
    torch.manual_seed(41)
    tr = PPOTrainer(_trainer_config(True, environment=dict(VECTOR), epochs=2), run_id="preveval", device=dev, tensorboard=False)
    states = []
    try:
        for _ in range(2):
            tr._sample_training_data()
            tr.buffer.prepare_batch_dict()
            tr._train_epochs(3e-4, 0.1, 1e-3)
            torch.cuda.synchronize()
            opt, b = tr.optimizer, tr.buffer
            states.append([t.clone() for t in (opt.flat_params, opt.exp_avg, b.actions, b.log_probs, b.values, b.prev_actions, b.prev_rewards)])
            if evaluate:
                assert len(tr.evaluate(episodes_per_worker=1, n_workers=4, deterministic=False, worker_steps=8)["episodes"]) == 4
                assert tr._evaluator.rollout._rw_pin.data_ptr() != tr._rw_pin.data_ptr()
                assert tr._evaluator.rollout._act_dev.data_ptr() != tr._act_dev.data_ptr()
    finally:
        tr.close()
    return states


def test_evaluations_in_between_leave_the_training_bits(dev):
    """The evaluator's rollout context has its own reward block and its own act_dev: sampled evaluations after each update change no
    bit of the parameters, the moments, the rollout's rows or the previous-step fields."""
    for upd, (x, y) in enumerate(zip(_two_updates(dev, False), _two_updates(dev, True))):
        for name, p, q in zip(("parameters", "exp_avg", "actions", "log_probs", "values", "prev_actions", "prev_rewards"), x, y):
            assert torch.equal(p, q), (upd, name)


@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
def test_checkpoint_resumes_bit_for_bit(dev, tmp_path, monkeypatch, graph):
    """Two updates, a checkpoint, fresh episodes, two more updates; then the checkpoint loaded in place -- with the captured rollout and
    optimisation graphs (the default) and with eager steps --, and, with eager steps, loaded by a fresh trainer (``resume=``): the two
    updates after it repeat bit for bit -- the table travels in the arena, every worker restarts at episode step 0, nothing else of
    the previous step is state.  (A fresh trainer in graph mode warms up with eager steps where the saved run replayed: that gap is
    the subject of tests/test_resume_gpu.py, not of this key.)"""
    from trainer import PPOTrainer
    monkeypatch.chdir(tmp_path)

    def update(tr):
        lr, beta, clip = tr.schedules(tr.update_index)
        tr._sample_training_data()
        tr.buffer.prepare_batch_dict()
        tr._train_epochs(lr, clip, beta)
        tr.update_index += 1
        torch.cuda.synchronize()
        b = tr.buffer
        return [t.clone() for t in (tr.optimizer.flat_params, b.actions, b.log_probs, b.values, b.prev_actions, b.prev_rewards)]

    cfg = _trainer_config(True, environment=dict(VECTOR), epochs=2, updates=4, hip_graph_rollout=graph, hip_graph_train=graph)
    torch.manual_seed(51)
    tr = PPOTrainer(cfg, run_id="prevckpt", device=dev, tensorboard=False)
    fresh = None
    try:
        for _ in range(2):
            update(tr)
        path = tr.save_checkpoint()
        assert float(tr.model.prev_input.weight.detach().abs().max()) > 0
        tr.restart_episodes(1)
        rec_a = [update(tr) for _ in range(2)]
        tr.load_checkpoint(path)
        rec_b = [update(tr) for _ in range(2)]
        assert (tr._step_graph is not None, tr._train_graph is not None) == (graph, graph)
        rec_c = rec_a
        if not graph:
            torch.manual_seed(999)
            fresh = PPOTrainer(cfg, run_id="prevckpt_fresh", device=dev, tensorboard=False, resume=path)
            rec_c = [update(fresh) for _ in range(2)]
        for k in range(2):
            assert bool((rec_a[k][4][:, 0] == -1).all()) == (k == 0)        # every worker restarts at episode step 0, then carries
            for name, a, b, c in zip(("parameters", "actions", "log_probs", "values", "prev_actions", "prev_rewards"), rec_a[k], rec_b[k], rec_c[k]):
                assert torch.equal(a, b), ("in place", k, name)
                assert torch.equal(a, c), ("resume=", k, name)
    finally:
        tr.close()
        if fresh is not None:
            fresh.close()
