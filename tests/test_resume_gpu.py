"""-m gpu: checkpoint and resume of training -- ``etm_arena_digest`` (csrc/arena_digest.hip) and everything built on it.

1. The digest kernel against ``checkpoint.digest_numpy``, all four words bit for bit: every head / tail length, both alignments of the
   base, 1 / 7 / 1024 workgroups, NaN, +-Inf, +-0 and denormals at the first, a middle and the last index; the refusals.
2. ``FlatAdamW.state_dict`` / ``load_state_dict``: a second optimiser continues bit for bit, no arena moves.
3. In-place resume through the captured graphs: two updates, save, restart, two recorded updates; load, the same two updates again --
   equal in every bit, every fixed address and (graph mode) both captured graphs unchanged.  The trainer draws its own uniforms and
   permutations, so the generator states are under test.
4. A fresh trainer built with ``resume=``: the state right after the load equals the saved one bit for bit; the two updates equal the
   recording of 3 -- bit for bit in eager mode, and in graph mode too: the gap between an eager and a graph trainer on this config
   (identical weights, draws and permutations, two updates) was measured as 0 (profiles/r13/resume.txt), so the eager warm-up
   minibatches of the resumed trainer compute what the uninterrupted one replays.
5. ``run_training`` with ``checkpoint_interval``; without the key.
6. The non-finite guard of ``save_checkpoint``.  7. A damaged file.  8. The refusals.
"""
import gc
import os
import pickle
import shutil
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import resume_helpers as rh

pytestmark = pytest.mark.gpu

# the largest relative parameter difference between an eager and a graph trainer of the parent commit on this config after two
# updates from identical weights, draws and permutations (tools/resume_measure.py; profiles/r13/resume.txt)
PARENT_EAGER_GRAPH_GAP = 0.0


@pytest.fixture(autouse=True)
def _collect_between_tests():
    gc.collect()
    yield
    gc.collect()


def _figure(text):
    print("\n[resume] " + text, flush=True)


# ------------------------------------------------------------------ 1. etm_arena_digest
DIGEST_N = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 256 * 4096 + 3)
SPECIAL_BITS = (0x7FC00000, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0xFFC01234)


def _planted(n, variant, rng):
    """n random 32-bit words; the words ``variant`` picks (NaN, +Inf, -Inf, -0, +0, two denormals, a negative NaN with a payload) at the
    first, a middle and the last index (for n < 3 the later ones win)."""
    words = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    for k, at in enumerate((0, n // 2, n - 1)):
        words[at] = SPECIAL_BITS[(variant + 3 * k) % len(SPECIAL_BITS)]
    return words


def _device_digest(words, shift, n_partial, out, partial):
    """The kernel's four words over ``words`` placed ``shift`` floats past a 16-byte boundary."""
    from etm import ops
    n = words.size
    store = torch.zeros(n + 4, dtype=torch.int32, device=rh.dev())
    assert store.data_ptr() % 16 == 0
    x = store[shift: shift + n]
    x.copy_(torch.from_numpy(words.view(np.int32)))
    x = x.view(torch.float32)
    assert x.data_ptr() % 16 == 4 * shift and x.is_contiguous()
    out.fill_(-1)
    ops.arena_digest(x, out=out, partial=partial, n_partial=n_partial)
    got = tuple(int(w) for w in out.cpu().numpy().view(np.uint64))
    assert np.array_equal(x.view(torch.int32).cpu().numpy().view(np.uint32), words), "the input is read only"
    return got


@pytest.mark.parametrize("n", DIGEST_N)
def test_arena_digest_kernel_against_numpy(n):
    import checkpoint as ck
    rng = np.random.default_rng(n)
    out = torch.zeros(4, dtype=torch.int64, device=rh.dev())
    partial = torch.zeros(3 * 1024, dtype=torch.int64, device=rh.dev())
    for variant in range(len(SPECIAL_BITS)):
        words = _planted(n, variant, rng)
        want = ck.digest_numpy(words.view(np.float32))
        assert want[3] == n
        for shift in (0, 1, 2, 3):                 # 0: aligned; 1: the base one float past a 16-byte boundary; 2, 3: the other heads
            for n_partial in (1, 7, 1024):
                partial.fill_(-1)                  # (stale scratch must not matter)
                got = _device_digest(words, shift, n_partial, out, partial)
                assert got == want, (n, variant, shift, n_partial, got, want)


def test_arena_digest_of_plain_values():
    """No special word: nothing counted, the maximum is the largest magnitude whatever its sign."""
    import checkpoint as ck
    from etm import ops
    x = torch.linspace(-3.0, 2.0, 1000, device=rh.dev())
    got = tuple(int(w) for w in ops.arena_digest(x).cpu().numpy().view(np.uint64))
    assert got == ck.digest_numpy(x.cpu().numpy()) and got[1] == 0 and got[2] == int(np.float32(3.0).view(np.uint32)) and got[3] == 1000


def test_arena_digest_refusals():
    from etm import lib as etm_lib
    lib = etm_lib.load()
    x = torch.zeros(64, device=rh.dev())
    partial = torch.zeros(3 * 4096, dtype=torch.int64, device=rh.dev())
    out = torch.zeros(4, dtype=torch.int64, device=rh.dev())
    st = torch.cuda.current_stream().cuda_stream
    ok = (x.data_ptr(), 64, partial.data_ptr(), 8, out.data_ptr(), st)
    assert lib.etm_arena_digest(*ok) == 0
    EINVAL = -1
    for i, bad in ((0, None), (2, None), (4, None), (1, 0), (1, -5), (3, 0), (3, -1), (3, 4097), (0, x.data_ptr() + 2)):
        args = list(ok)
        args[i] = bad
        assert lib.etm_arena_digest(*args) == EINVAL, (i, bad)
    assert lib.etm_arena_digest(*(ok[:3] + (4096,) + ok[4:])) == 0 and lib.etm_arena_digest(*(ok[:3] + (1,) + ok[4:])) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 2. FlatAdamW
def _adamw(seed, like=None):
    from etm.optim import FlatAdamW
    g = torch.Generator().manual_seed(seed)
    shapes = ((3, 5), (7,), (2, 2, 3), (1,), (13,), (1,))           # 49 floats: the arena is padded to 52
    if like is None:
        params = [torch.nn.Parameter(torch.randn(s, generator=g).to(rh.dev())) for s in shapes]
    else:
        params = [torch.nn.Parameter(p.detach().clone()) for p in like]
    return FlatAdamW(params, lr=1e-2, weight_decay=0.05), params


def _adamw_step(opt, seed):
    g = torch.Generator().manual_seed(seed)
    opt.flat_grads[: opt.total].copy_(torch.randn(opt.total, generator=g).to(rh.dev()))
    opt.step(max_grad_norm=0.5)


def test_flat_adamw_state_round_trip():
    a, pa = _adamw(0)
    assert a.total == 49 and a.flat_params.numel() == 52
    for s in range(3):
        _adamw_step(a, 100 + s)
    a.set_lr(5e-3)
    sd = a.state_dict()
    assert sd["step"] == 3 and sd["lr"] == 5e-3 and sd["total"] == 49 and sd["padded"] == 52 and sd["betas"] == [0.9, 0.999]
    assert sd["eps"] == 1e-8 and sd["weight_decay"] == 0.05
    assert isinstance(sd["exp_avg"], np.ndarray) and sd["exp_avg"].dtype == np.float32 and sd["exp_avg_sq"].shape == (52,)
    b, pb = _adamw(1, like=pa)
    ptrs = [t.data_ptr() for t in (b.flat_params, b.flat_grads, b.exp_avg, b.exp_avg_sq, b.step_dev, b.lr_dev)] + [p.data_ptr() for p in pb]
    b.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in (b.flat_params, b.flat_grads, b.exp_avg, b.exp_avg_sq, b.step_dev, b.lr_dev)] + [p.data_ptr() for p in pb]
    assert b._lr_host == 5e-3 and float(b.lr_dev.item()) == float(np.float32(5e-3))
    for opt in (a, b):
        opt.set_lr(5e-3)                      # (in step with the device value: no refill)
        _adamw_step(opt, 200)
    for name in ("flat_params", "exp_avg", "exp_avg_sq", "step_dev", "lr_dev"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(b.step_dev.item()) == 4
    for x, y in zip(pa, pb):
        assert torch.equal(x, y)
    # a state that does not fit is refused, and the difference is named
    for key, value in (("total", 50), ("padded", 56), ("betas", [0.8, 0.999]), ("eps", 1e-6), ("weight_decay", 0.01)):
        with pytest.raises(ValueError, match=key):
            b.load_state_dict(dict(sd, **{key: value}))
    with pytest.raises(ValueError, match="exp_avg_sq"):
        b.load_state_dict(dict(sd, exp_avg_sq=sd["exp_avg_sq"][:48]))
    assert int(b.step_dev.item()) == 4, "a refused state touches nothing"


# ------------------------------------------------------------------ 3 / 4. resume through the trainer
_SCENARIOS = {}


def _scenario(graph, tmp_path_factory):
    """Test 3's run, once per mode: two updates, save_checkpoint, restart_episodes(1), two recorded updates (A); load_checkpoint, the
    same two updates again (B).  -> everything tests 3 and 4 assert on; the checkpoint stays on disk for test 4."""
    if graph in _SCENARIOS:
        return _SCENARIOS[graph]
    work = tmp_path_factory.mktemp("resume_graph" if graph else "resume_eager")
    cwd = os.getcwd()
    os.chdir(work)
    tr = None
    try:
        tr = rh.trainer(rh.config(**rh.modes(graph)), run_id="scenario")
        for _ in range(2):
            rh.update(tr)
        path = tr.save_checkpoint()
        saved, saved_digest = rh.state(tr), tr.state_digest()
        tr.restart_episodes(1)
        rec_a = [rh.update(tr) for _ in range(2)]
        assert tr.update_index == 4
        graphs = (tr._step_graph, tr._train_graph, tr._lv.graph, tr._kv_refresh_replay.graph)
        addresses = tr._fixed_addresses()
        tr.load_checkpoint(path)
        loaded, loaded_digest, index_after_load, segment_after_load = rh.state(tr), tr.state_digest(), tr.update_index, tr.segment
        addresses_after = tr._fixed_addresses()
        rec_b = [rh.update(tr) for _ in range(2)]
        same_graphs = [x is y for x, y in zip(graphs, (tr._step_graph, tr._train_graph, tr._lv.graph, tr._kv_refresh_replay.graph))]
        out = dict(path=os.path.join(str(work), path), saved=saved, saved_digest=saved_digest, rec_a=rec_a, rec_b=rec_b, loaded=loaded,
                   loaded_digest=loaded_digest, index_after_load=index_after_load, segment_after_load=segment_after_load,
                   addresses=addresses, addresses_after=addresses_after, addresses_end=tr._fixed_addresses(), graphs=graphs,
                   same_graphs=same_graphs, captured=(tr._step_graph is not None, tr._train_graph is not None))
    finally:
        os.chdir(cwd)
        rh.release(tr)
    _SCENARIOS[graph] = out
    return out


@pytest.mark.parametrize("graph", (True, False), ids=["graph", "eager"])
def test_in_place_resume_reproduces_the_run(graph, tmp_path_factory):
    sc = _scenario(graph, tmp_path_factory)
    assert rh.differing(sc["saved"], sc["loaded"]) == [] and sc["saved_digest"] == sc["loaded_digest"]
    assert sc["index_after_load"] == 2 and sc["segment_after_load"] == 1
    a0, a1 = sc["rec_a"]
    assert rh.differing(a0, a1) != [] and rh.differing(sc["saved"], {k: a0[k] for k in sc["saved"]}) != [], "the updates do something"
    assert not np.array_equal(a0["obs_norm_stats"], sc["saved"]["obs_norm_stats"]) and not np.array_equal(a0["ret_stats"], sc["saved"]["ret_stats"])
    assert int(a1["step"]) == 4 * 4 and a0["lr"] != a1["lr"], "four minibatch steps per update, a decaying learning rate"
    for k, (a, b) in enumerate(zip(sc["rec_a"], sc["rec_b"])):
        assert rh.differing(a, b) == [], f"update {2 + k} after the load differs from the uninterrupted run"
    assert sc["addresses"] == sc["addresses_after"] == sc["addresses_end"]
    assert sc["captured"] == (graph, graph)
    if graph:
        assert all(g is not None for g in sc["graphs"][:2]) and all(sc["same_graphs"]), "the captured graphs survive the load"


@pytest.mark.parametrize("graph", (True, False), ids=["graph", "eager"])
def test_fresh_trainer_resumes_from_the_file(graph, tmp_path_factory):
    sc = _scenario(graph, tmp_path_factory)
    tr = None
    try:
        torch.manual_seed(999)                 # (the generator states come from the file, not from here)
        tr = rh.trainer(rh.config(**rh.modes(graph)), seed=999, run_id="fresh", resume=sc["path"])
        assert tr.update_index == 2 and tr.segment == 1
        assert rh.differing(sc["saved"], rh.state(tr)) == [] and tr.state_digest() == sc["saved_digest"], "the state right after the load"
        rec = [rh.update(tr) for _ in range(2)]
        for k, (a, b) in enumerate(zip(sc["rec_a"], rec)):
            gap = rh.largest_relative_parameter_difference(a, b)
            _figure(f"fresh resume graph={graph} update {2 + k}: largest relative parameter difference {gap:.3e}; keys that differ {rh.differing(a, b)}")
            if not graph or PARENT_EAGER_GRAPH_GAP == 0.0:
                assert rh.differing(a, b) == [], f"update {2 + k} of the resumed trainer differs from the uninterrupted run"
            else:
                assert gap <= 3 * PARENT_EAGER_GRAPH_GAP
        assert (tr._step_graph is not None, tr._train_graph is not None) == (graph, graph)
    finally:
        rh.release(tr)


# ------------------------------------------------------------------ 5. run_training
def test_run_training_writes_checkpoints_and_resumes(tmp_path, monkeypatch):
    from evaluation import Evaluator
    from trainer import PPOTrainer
    monkeypatch.chdir(tmp_path)
    cfg = rh.config(updates=4, checkpoint_interval=2)
    tr = resumed = ev = None
    try:
        tr = rh.trainer(cfg, run_id="e2e")
        saves = []
        inner = tr.save_checkpoint

        def spy():
            path = inner()
            assert os.path.exists("models/e2e.nn") and os.path.exists(path) and not [f for f in os.listdir("models") if f.endswith(".tmp")]
            shutil.copy(path, f"models/at_{tr.update_index}.ckpt")
            saves.append(tr.update_index)
            return path
        tr.save_checkpoint = spy
        tr.run_training()
        assert saves == [2, 4] and tr.update_index == 4
        final = rh.state(tr)
        with open("models/e2e.nn", "rb") as f:               # evaluate.py's loader
            state_dict, config = pickle.load(f)
        assert config == cfg and all(torch.is_tensor(v) for v in state_dict.values())
        ev = Evaluator(config, rh.dev(), run_id="evaluate")
        ev.load_state_dict(state_dict)
        assert len(ev.run(episodes_per_worker=1, n_workers=4, worker_steps=8)["episodes"]) == 4
        for n, p in ev.rollout.model.named_parameters():
            assert np.array_equal(rh.bits(p.detach().cpu().numpy()), rh.bits(final["param:" + n])), n
        ev.close()
        ev = None
        rh.release(tr)
        tr = None
        # resumed from the update-2 file: exactly updates 2 and 3, under their schedules
        resumed = rh.trainer(cfg, seed=5, run_id="e2e_resumed", resume="models/at_2.ckpt")
        seen = []
        inner_epochs = resumed._train_epochs
        resumed._train_epochs = lambda lr, clip, beta, **kw: (seen.append((lr, beta, clip)), inner_epochs(lr, clip, beta, **kw))[1]
        resumed.run_training()
        assert seen == [resumed.schedules(2), resumed.schedules(3)] and resumed.schedules(2) != resumed.schedules(3) != resumed.schedules(0)
        assert resumed.update_index == 4 and int(resumed.optimizer.step_dev.item()) == 16 and resumed.segment == 1
        with open("models/e2e_resumed.ckpt", "rb") as f:
            last = pickle.load(f)
        assert last["update"] == 4 and last["segment"] == 1 and last["format"] == 1 and len(last["episode_infos"]) <= 100
    finally:
        if ev is not None:
            ev.close()
        rh.release(tr, resumed)


def test_run_training_without_the_key_writes_the_model_file_once(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr = None
    try:
        tr = rh.trainer(rh.config(updates=2), run_id="plain")
        calls = []
        inner = tr._save_model
        tr._save_model = lambda: (calls.append(tr.update_index), inner())[1]
        tr.save_checkpoint = lambda *a, **k: pytest.fail("save_checkpoint without checkpoint_interval")
        tr.run_training()
        assert calls == [2] and sorted(os.listdir("models")) == ["plain.nn"]
        assert getattr(tr, "_digest_out", None) is None, "nothing of the checkpoint path was allocated"
    finally:
        rh.release(tr)


# ------------------------------------------------------------------ 6 / 7. the guard, a damaged file
def test_non_finite_state_is_not_saved_and_a_damaged_file_is_not_loaded(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr = None
    try:
        tr = rh.trainer(rh.config(**rh.modes(False)), run_id="guard")
        rh.update(tr)
        path = tr.save_checkpoint()
        good = {f: open(os.path.join("models", f), "rb").read() for f in ("guard.nn", "guard.ckpt")}
        rh.update(tr)
        # 7. one element of the parameter array flipped inside the file
        with open(path, "rb") as f:
            damaged = pickle.load(f)
        damaged["params"] = damaged["params"].copy()
        damaged["params"][17] = -damaged["params"][17] if damaged["params"][17] != 0 else np.float32(1.0)
        with open("models/damaged.ckpt", "wb") as f:
            pickle.dump(damaged, f)
        before, before_state, index = tr.state_digest(), rh.state(tr), tr.update_index
        with pytest.raises(ValueError, match="params arena does not match its stored digest"):
            tr.load_checkpoint("models/damaged.ckpt")
        assert tr.state_digest() == before and rh.differing(rh.state(tr), before_state) == [] and tr.update_index == index
        # 6. one NaN in the second moment: neither file is written
        assert before["exp_avg_sq"][1] == 0
        tr.optimizer.exp_avg_sq[5] = float("nan")
        assert tr.state_digest()["exp_avg_sq"][1] == 1
        with pytest.raises(FloatingPointError, match=r"1 non-finite value\(s\) in the exp_avg_sq arena after update 2"):
            tr.save_checkpoint()
        assert {f: open(os.path.join("models", f), "rb").read() for f in sorted(os.listdir("models")) if f.startswith("guard")} == good
        # the good file still loads, and the run continues from it
        tr.load_checkpoint(path)
        assert tr.update_index == 1 and tr.state_digest()["exp_avg_sq"][1] == 0
    finally:
        rh.release(tr)


# ------------------------------------------------------------------ 8. refusals
def test_data_parallel_runs_refuse_checkpoints_before_anything_is_built(monkeypatch):
    import trainer as trainer_module
    from trainer import PPOTrainer
    built = []
    monkeypatch.setattr(trainer_module, "make_vec_env", lambda *a, **k: built.append(a) or pytest.fail("an environment was built"))
    dp = SimpleNamespace(world=2, rank=0)
    plain = {k: v for k, v in rh.config().items() if not k.startswith("normalize_")}
    with pytest.raises(ValueError, match="checkpoint_interval in a data-parallel run"):
        PPOTrainer(dict(plain, checkpoint_interval=2), device=rh.dev(), dp=dp, tensorboard=False)
    with pytest.raises(ValueError, match="resume in a data-parallel run"):
        PPOTrainer(plain, device=rh.dev(), dp=dp, tensorboard=False, resume="/nonexistent/run.ckpt")
    with pytest.raises(ValueError, match="checkpoint_interval: 0"):
        PPOTrainer(dict(plain, checkpoint_interval=0), device=rh.dev(), tensorboard=False)
    assert built == []


def test_worker_processes_resume_through_the_constructor_only(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    plain = {k: v for k, v in rh.config(**rh.modes(False)).items() if not k.startswith("normalize_")}
    a = b = None
    try:
        a = rh.trainer(plain, run_id="inproc")
        rh.update(a)
        path = a.save_checkpoint()
        saved, digest = rh.state(a), a.state_digest()
        rh.release(a)
        a = None
        b = rh.trainer(dict(plain, worker_processes=True, envs_per_process=4), seed=3, run_id="procs", resume=path)
        assert b._shm_env is not None and b.update_index == 1 and b.segment == 1
        assert rh.differing(saved, rh.state(b)) == [] and b.state_digest() == digest
        with pytest.raises(ValueError, match=r"resume=path"):
            b.load_checkpoint(path)
        with pytest.raises(ValueError, match="worker_processes"):
            b.restart_episodes(2)
        assert b.state_digest() == digest
        rh.update(b)
        assert int(b.optimizer.step_dev.item()) == 8
    finally:
        rh.release(a, b)


class _SuppliedEnv:
    """An environment handed to the trainer through ``env=``: the synthetic front-end behind a wrapper that can ``restart`` on other
    worker ids (``restartable``) or can only be ``reset``."""

    def __init__(self, cfg, restartable):
        self._cfg, self.restarts, self.resets = cfg, [], 0
        self._build(0)
        if restartable:
            self.restart = self._restart

    def _build(self, first):
        from environments.vec_env import make_vec_env
        self._env = make_vec_env(dict(self._cfg["environment"]), self._cfg["n_workers"], first, groups=1)

    def _restart(self, first_worker_id):
        self.restarts.append(first_worker_id)
        self._env.close()
        self._build(first_worker_id)

    def reset(self, *a, **k):
        self.resets += 1
        return self._env.reset(*a, **k)

    def __getattr__(self, name):
        return getattr(self._env, name)


def test_supplied_environment_is_restarted_or_reset(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    cfg = rh.config(**rh.modes(False))
    a = b = c = None
    try:
        env_a = _SuppliedEnv(cfg, restartable=True)
        a = rh.trainer(cfg, run_id="supplied", env=env_a)
        rh.update(a)
        path = a.save_checkpoint()
        assert env_a.restarts == [] and env_a.resets == 1
        a.restart_episodes(1)
        assert env_a.restarts == [1_000_000] and env_a.resets == 2 and a.segment == 1
        rec_a = rh.update(a)
        env_b = _SuppliedEnv(cfg, restartable=True)
        b = rh.trainer(cfg, seed=4, run_id="supplied_b", env=env_b, resume=path)
        assert env_b.restarts == [1_000_000] and env_b.resets == 1 and b.segment == 1
        assert rh.differing(rec_a, rh.update(b)) == [], "the constructor and restart_episodes put a supplied environment on the same ids"
        env_c = _SuppliedEnv(cfg, restartable=False)
        c = rh.trainer(cfg, seed=4, run_id="supplied_c", env=env_c)
        rh.update(c)
        c.load_checkpoint(path)
        assert env_c.resets == 2 and not hasattr(env_c, "restart") and c.segment == 1 and c.update_index == 1
        assert (c.worker_current_episode_step == 0).all() and c.buffer.num_episodes == rh.W_T and not c.buffer.ret_carry.any()
        rh.update(c)
    finally:
        rh.release(a, b, c)
