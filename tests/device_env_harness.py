"""What the GPU tests of the device-resident environments share, whatever the task: the kernel call object behind the C ABI with its
sentinels, the walk over everything an entry refuses, the front-end against a SerialVecEnv of host twins, and the trainer compared
bit for bit between ``device: true`` and the host twin.  A task's test files hold its case tables, its reference module
(cue_room_reference.py, command_room_reference.py: the oracles, independent of this module) and what only it checks."""
import gc

import numpy as np
import pytest
import torch

SEED, FIRST = 11, 5
SENTINEL = 0xA5
EINVAL = -1


# ---------------------------------------------------------------------------------------------------------------- the kernel
class Call:
    """Device and pinned operands of one sequence of kernel calls: the frame destination is rows [2, 2 + W) of a block of W + 4 rows
    with a pitch above the frame size, everything else filled with the sentinel.  ``entry``: the prefix of the task's C entries;
    ``rule``: the words its reset and step take behind ``W`` (G, P, ...), before the stream word."""

    def __init__(self, lib, entry, W, rule, pinned_words=True):
        G, P = rule[:2]
        self.rule = (W,) + tuple(rule) + (SEED + FIRST,)
        self._reset, self._step = getattr(lib, entry + "_reset"), getattr(lib, entry + "_step")
        self.W, self.fb = W, 3 * G * P * G * P
        self.pitch = self.fb + 16
        dev = torch.device("cuda", 0)
        self.state = torch.zeros(int(getattr(lib, entry + "_state_bytes")(W)) // 8, dtype=torch.int64, device=dev)
        self.block = torch.full((W + 4, self.pitch), SENTINEL, dtype=torch.uint8, device=dev)
        self.actions = torch.zeros((W, 3), dtype=torch.int64, device=dev)       # (a row stride of 3: the action is column 0)

        def words(dtype):
            t = torch.zeros(W + 2, dtype=dtype)
            return t.pin_memory() if pinned_words else t.to(dev)
        self.rewards, self.flags, self.returns = words(torch.float32), words(torch.uint8), words(torch.float32)
        self.lengths, self.masks = words(torch.int32), words(torch.int64)
        self.done = torch.zeros(1, dtype=torch.int64).pin_memory()
        self.fill_words()

    def fill_words(self):
        for t, v in ((self.rewards, -7.0), (self.flags, SENTINEL), (self.returns, -7.0), (self.lengths, -7), (self.masks, -7)):
            t.fill_(v)

    def ptrs(self, **replace):
        # the words' destinations start at entry 1: entries 0 and W + 1 are sentinels
        p = dict(state=self.state.data_ptr(), actions=self.actions.data_ptr(), frames=self.block[2].data_ptr(), pitch=self.pitch,
                 rewards=self.rewards[1:].data_ptr(), flags=self.flags[1:].data_ptr(), returns=self.returns[1:].data_ptr(),
                 lengths=self.lengths[1:].data_ptr(), masks=self.masks[1:].data_ptr(), done=self.done.data_ptr(), value=0)
        p.update(replace)
        return p

    def reset(self, rule=None, **replace):
        p = self.ptrs(**replace)
        return self._reset(p["state"], p["frames"], p["pitch"], p["rewards"], p["flags"], p["returns"], p["lengths"], p["masks"],
                           p["done"], p["value"], *(rule or self.rule), None)

    def step(self, table=None, rule=None, act_stride=3, **replace):
        if table is not None:
            self.actions[:, 0] = torch.from_numpy(np.array(table, dtype=np.int64)).to(self.actions.device)
        p = self.ptrs(**replace)
        return self._step(p["state"], p["actions"], act_stride, p["frames"], p["pitch"], p["rewards"], p["flags"], p["returns"],
                          p["lengths"], p["masks"], p["done"], p["value"], *(rule or self.rule), None)

    def read(self):
        """(frames [W, fb], rewards, flags, returns, lengths, masks) of the last call; asserts every sentinel."""
        torch.cuda.synchronize()
        block = self.block.cpu().numpy()
        W = self.W
        assert (block[:2] == SENTINEL).all() and (block[2 + W:] == SENTINEL).all(), "a frame row outside [lo, hi) was written"
        assert (block[2:2 + W, self.fb:] == SENTINEL).all(), "bytes between a frame's end and the pitch were written"
        outs = [t.cpu().numpy() for t in (self.rewards, self.flags, self.returns, self.lengths, self.masks)]
        for o, v in zip(outs, (-7.0, SENTINEL, -7.0, -7, -7)):
            assert o[0] == v and o[-1] == v, "a result word outside [0, W) was written"
        return (block[2:2 + W, :self.fb].copy(),) + tuple(o[1:-1].copy() for o in outs)

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.block.cpu().numpy() == SENTINEL).all()
        for t, v in ((self.rewards, -7.0), (self.flags, SENTINEL), (self.returns, -7.0), (self.lengths, -7), (self.masks, -7)):
            assert (t.cpu().numpy() == v).all()
        assert int(self.done[0]) == 0 and (self.state.cpu().numpy() == 0).all()


def run(call, raw, S):
    """reset + S steps -> per step (frames, rewards, flags, returns, lengths, masks); the completion word counts the calls."""
    assert call.reset(value=100) == 0
    out = [call.read()]
    assert int(call.done[0]) == 100
    for t in range(S):
        assert call.step(raw[t], value=t + 1) == 0
        out.append(call.read())
        assert int(call.done[0]) == t + 1
    return out


def assert_kernel_equals_the_rule(make_call, raw, want, S, W, side):
    """``make_call(pinned_words=...)`` -> a fresh Call; ``want``: the reference's frames / masks per observation and rewards / flags /
    returns / lengths per step."""
    got = run(make_call(), raw, S)
    for t, (frames, rewards, flags, returns, lengths, masks) in enumerate(got):
        assert np.array_equal(frames.reshape(W, 3, side, side), want["frames"][t]), f"frames of step {t}"
        assert np.array_equal(masks.view(np.uint64), want["masks"][t]), f"mask words of step {t}"
        if t == 0:
            assert not rewards.any() and not flags.any() and not returns.any() and not lengths.any()
            continue
        assert np.array_equal(rewards.view(np.uint32), want["rewards"][t - 1].view(np.uint32)), f"rewards of step {t}"
        assert np.array_equal(flags, want["flags"][t - 1]), f"flags of step {t}"
        assert np.array_equal(returns.view(np.uint32), want["returns"][t - 1].view(np.uint32)), f"returns of step {t}"
        assert np.array_equal(lengths, want["lengths"][t - 1]), f"lengths of step {t}"
    # two runs from equal state are equal -- with the result words in device memory this time
    again = run(make_call(pinned_words=False), raw, S)
    for a, b in zip(got, again):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def assert_step_advances_the_state_exactly_once(call, raw, want):
    # two steps from one reset: the second call continues from the first one's state (not from the reset's)
    assert call.reset() == 0
    first = call.read()
    assert call.step(raw[0]) == 0 and call.step(raw[1]) == 0
    frames = call.read()[0]
    assert np.array_equal(frames.reshape(want["frames"][2].shape), want["frames"][2])
    assert not np.array_equal(first[0], frames)


def assert_einval_leaves_every_sentinel_in_place(call, own_bad_rules):
    """Every class of argument the entries refuse, each at reset and step; ``own_bad_rules``: the task's own bad rule tuples, beside
    the bad ``W`` / ``G`` / ``P`` every task refuses.  Nothing was written, and a good call still runs."""
    W, G, P, *tail = call.rule[:-1]
    bad_rules = [(0, G, P, *tail, 0), (-3, G, P, *tail, 0), (W, 4, P, *tail, 0), (W, 1, P, *tail, 0), (W, 33, P, *tail, 0),
                 (W, G, 6, *tail, 0), (W, G, 0, *tail, 0), (W, G, 68, *tail, 0)] + list(own_bad_rules)
    good = call.ptrs()
    for rule in bad_rules:
        assert call.reset(rule=rule) == EINVAL, rule
        assert call.step(rule=rule) == EINVAL, rule
    for name in ("state", "frames", "rewards", "flags", "returns", "lengths", "masks"):
        assert call.reset(**{name: None}) == EINVAL, name
        assert call.step(**{name: None}) == EINVAL, name
    assert call.step(actions=None) == EINVAL
    for name, off in (("state", 4), ("frames", 2), ("rewards", 2), ("returns", 1), ("lengths", 2), ("masks", 4), ("done", 4)):
        assert call.reset(**{name: good[name] + off}) == EINVAL, name
        assert call.step(**{name: good[name] + off}) == EINVAL, name
    assert call.step(actions=good["actions"] + 4) == EINVAL
    assert call.step(act_stride=0) == EINVAL
    for pitch in (call.fb - 4, call.fb + 2, 0, -call.pitch):
        assert call.reset(pitch=pitch) == EINVAL, pitch
        assert call.step(pitch=pitch) == EINVAL, pitch
    call.untouched()
    # and the calls above left no error behind: a good call still runs, without a completion word too
    assert call.reset(pitch=call.fb) == 0
    assert call.reset(pitch=call.fb, done=None) == 0
    torch.cuda.synchronize()
    assert int(call.done[0]) == 0


# ---------------------------------------------------------------------------------------------------------------- the front-end
def host_vec(cfg, W, first):
    from environments.vec_env import make_vec_env
    return make_vec_env(dict(cfg, device=False, vectorize="serial"), W, first_worker_id=first)


def _host_infos(infos):
    # (SerialVecEnv hands a CUT episode's last frame over in its info; the front-end keeps none)
    return [{k: v for k, v in i.items() if k != "final_observation"} if i and i.get("truncated") else i for i in infos]


def front_end_against_host_twins(groups, cfg, front_end, num_actions, max_episode_steps, choose, tail):
    """``cfg``: the environment section with ``device: true`` (grid 3, cell 12); ``choose(t, host)`` -> the actions [W] of step t
    (``host``: the SerialVecEnv of twins, before the step); ``tail``: two more action vectors, for a plain (unpinned) destination and
    none at all.  -> (episodes ended, successes)."""
    from environments.device_env import DeviceVecEnv
    from environments.vec_env import CompositeVecEnv, make_vec_env
    W, S, first = 5, 30, 4
    if groups == 1:
        dev = make_vec_env(cfg, W, first_worker_id=first)
        assert isinstance(dev, front_end) and isinstance(dev, DeviceVecEnv)
    else:           # parts of 2 and 3 workers with consecutive worker ids: the streams of a single front-end
        dev = CompositeVecEnv([make_vec_env(cfg, 2, first_worker_id=first), make_vec_env(cfg, 3, first_worker_id=first + 2)])
        assert all(isinstance(p, front_end) and p.device_resident for p in dev.parts)
    host = host_vec(cfg, W, first)
    assert dev.observation_dtype == np.uint8 and dev.observation_space_shape == host.observation_space_shape == (3, 36, 36)
    assert tuple(dev.action_space_shape) == tuple(host.action_space_shape) == (num_actions,)
    assert dev.num_actions == host.num_actions == num_actions
    assert dev.max_episode_steps == host.max_episode_steps == max_episode_steps and dev.num_envs == W
    rows = torch.zeros((W, 3, 36, 36), dtype=torch.uint8).pin_memory().numpy()
    assert np.array_equal(dev.reset(out=rows), host.reset())
    assert np.array_equal(dev.action_masks(), host.action_masks())
    ended = succeeded = 0
    for t in range(S):
        acts = choose(t, host)
        seen = []
        obs, rewards, dones, infos = dev.step(acts, out=rows, on_rows=lambda a, b: seen.append((a, b)))
        h_obs, h_rewards, h_dones, h_infos = host.step(acts)
        assert obs is rows and np.array_equal(obs, h_obs), t
        assert rewards.dtype == np.float32 and np.array_equal(rewards, h_rewards) and dones.dtype == bool and np.array_equal(dones, h_dones)
        assert list(infos) == _host_infos(h_infos), t
        assert seen and seen[0][0] == 0 and seen[-1][1] == W and all(a[1] == b[0] for a, b in zip(seen, seen[1:]))
        words = np.zeros(W, dtype=np.int64)
        assert dev.action_masks(out=words) is words and np.array_equal(words.view(np.uint64), host.action_masks())
        ended += int(dones.sum())
        succeeded += sum(i["success"] for i in infos if i)
    assert ended >= W
    # a plain (unpinned) destination and none at all
    assert np.array_equal(dev.step(tail[0], out=np.zeros_like(rows))[0], host.step(tail[0])[0])
    assert np.array_equal(dev.step(tail[1])[0], host.step(tail[1])[0])
    with pytest.raises(ValueError, match="outside Discrete"):
        dev.step(np.full(W, num_actions))
    with pytest.raises(ValueError, match="outside Discrete"):
        dev.step(np.full(W, -1))
    dev.close()
    return ended, succeeded


def step_device_writes_the_rows_it_is_given(cfg, front_end, num_actions):
    """``cfg``: the environment section without ``device`` (grid 3, cell 12); its keys are the front-end's keyword arguments."""
    W, first = 3, 2
    dev = front_end(W, first_worker_id=first, **{k: v for k, v in cfg.items() if k != "type"})
    host = host_vec(cfg, W, first)
    dev.reset(), host.reset()
    stage = torch.full((4, W + 2, 3, 36, 36), SENTINEL, dtype=torch.uint8, device="cuda")      # rows [1, 1 + W) of row t + 1
    act_dev = torch.zeros((W, 1), dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    acts = np.random.default_rng(3).integers(0, num_actions, size=(3, W)).astype(np.int64)
    for t in range(3):
        act_dev[:, 0] = torch.from_numpy(acts[t]).cuda()
        torch.cuda.synchronize()
        if t == 1:
            rewards, dones, infos = dev.step_device(act_dev, stage[t + 1, 1:1 + W].data_ptr(), side)
        else:
            rewards, dones, infos = dev.step_device(act_dev, stage[t + 1, 1:1 + W])
        h_obs, h_rewards, h_dones, h_infos = host.step(acts[t])
        got = stage.cpu().numpy()
        assert np.array_equal(got[t + 1, 1:1 + W], h_obs) and np.array_equal(rewards, h_rewards) and np.array_equal(dones, h_dones)
        assert list(infos) == _host_infos(h_infos)
        assert np.array_equal(dev.action_masks(), host.action_masks())
        assert (got[t + 1, 0] == SENTINEL).all() and (got[t + 1, W + 1] == SENTINEL).all() and (got[t + 2:] == SENTINEL).all()
    assert dev.device_steps == 3 and dev.protocol_steps == 0
    # the protocol path continues from the same state
    assert np.array_equal(dev.step(acts[0])[0], host.step(acts[0])[0]) and dev.protocol_steps == 1


# ---------------------------------------------------------------------------------------------------------------- the trainer
W, S, EPOCHS, N_MB = 4, 8, 2, 2
FORMS = {
    "captured": {},
    "protocol": {"hip_graph_rollout": False},
    "two groups": {"rollout_groups": 2, "rollout_min_group_size": 2},
    "action masks": {"action_masks": True},
    "previous step": {"previous_step_input": True},
}
TRANSFORMER = dict(num_blocks=1, embed_dim=64, num_heads=1, memory_length=4, positional_encoding="relative", layer_norm="post",
                   gtrxl=False, gtrxl_bias=0.0)
FIELDS = ("obs", "actions", "log_probs", "values", "rewards", "dones", "memory_index", "advantages")


def config(env, device, **over):
    """``env``: the task's environment section without ``device`` and ``vectorize``."""
    sched = dict(initial=3e-4, final=3e-4, power=1.0, max_decay_steps=10)
    cfg = dict(environment=dict(env, device=bool(device), vectorize="serial"), gamma=0.99, lamda=0.95, updates=2, epochs=EPOCHS,
               n_workers=W, worker_steps=S, n_mini_batch=N_MB, value_loss_coefficient=0.5, hidden_layer_size=64, max_grad_norm=0.5,
               tunable_gemm=False, rollout_groups=1, transformer=dict(TRANSFORMER),
               learning_rate_schedule=dict(sched), beta_schedule=dict(sched, initial=1e-3, final=1e-3),
               clip_range_schedule=dict(sched, initial=0.1, final=0.1))
    cfg.update(over)
    return cfg


def trainer(cfg, run_id, **kw):
    from trainer import PPOTrainer
    torch.manual_seed(11)
    return PPOTrainer(cfg, run_id=run_id, device=torch.device("cuda", 0), tensorboard=False, **kw)


def _release(*trainers):
    for tr in trainers:
        tr.close()
    del trainers
    gc.collect()
    torch.cuda.synchronize()


def _front_ends(tr):
    return list(getattr(tr.env, "parts", None) or [tr.env])


def _eq(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _field(buf, name):
    # (the host array is what the rollout writes; the device field is uploaded from it when the batch is prepared)
    return buf.memory_index_host if name == "memory_index" else getattr(buf, name)


def trains_bit_for_bit_like_the_host_twin(form, env, run_id, front_end):
    from environments.vec_env import SerialVecEnv
    dev, host = trainer(config(env, True, **FORMS[form]), run_id), trainer(config(env, False, **FORMS[form]), run_id)
    try:
        assert all(isinstance(e, front_end) for e in _front_ends(dev))
        assert all(isinstance(e, SerialVecEnv) for e in _front_ends(host))
        assert len(_front_ends(dev)) == len(_front_ends(host)) == (2 if form == "two groups" else 1)
        assert dev.observation_dtype == torch.uint8 and _eq(dev.obs, host.obs)
        rng = np.random.default_rng(3)
        for update in range(2):
            uniforms = rng.random((W, S), dtype=np.float32)
            perms = [np.random.default_rng(40 + 10 * update + e).permutation(W * S) for e in range(EPOCHS)]
            infos = []
            for tr in (dev, host):
                lr, beta, clip = tr.schedules(update)
                infos.append(tr._sample_training_data(uniforms=uniforms))
                torch.cuda.synchronize()
            for name in FIELDS:
                assert _eq(_field(dev.buffer, name), _field(host.buffer, name)), f"update {update}: buffer.{name} differs"
            assert infos[0] == infos[1], f"update {update}: the finished episodes' infos differ"
            assert _eq(dev.obs, host.obs), "the rows after the last step (the bootstrap observation) differ"
            if form == "action masks":
                assert _eq(dev.buffer.action_masks_host, host.buffer.action_masks_host)
                assert dev.last_valid_action_share == host.last_valid_action_share < 1.0
            # which path stepped the environments: in a plan that streams observations every step but the rollout's last one is
            # the kernel writing into the staging row; else the protocol path alone
            fast = sum(e.device_steps for e in _front_ends(dev))
            slow = sum(e.protocol_steps for e in _front_ends(dev))
            n = len(_front_ends(dev))
            if form == "protocol":
                assert dev._plan is None and (fast, slow) == (0, (update + 1) * S)
            else:
                assert dev._plan is not None and dev._plan.stream_obs and host._plan == dev._plan
                assert (fast, slow) == ((update + 1) * (S - 1) * n, (update + 1) * n), "the fast path was not taken"
            for tr in (dev, host):
                tr.buffer.prepare_batch_dict()
                tr._train_epochs(lr, clip, beta, perms=perms)
                tr.update_index += 1
            torch.cuda.synchronize()
            assert _eq(dev.optimizer.flat_params, host.optimizer.flat_params), f"update {update}: the parameter arenas differ"
        assert len(infos[0]) >= W and all(set(i) == {"reward", "length", "success"} for i in infos[0])
    finally:
        _release(dev, host)


def evaluation_returns_the_host_twins_result(env, run_id):
    dev, host = trainer(config(env, True), run_id), trainer(config(env, False), run_id)
    try:
        a = dev.evaluate(episodes_per_worker=2, n_workers=4, deterministic=True, seed=700, worker_steps=8)
        b = host.evaluate(episodes_per_worker=2, n_workers=4, deterministic=True, seed=700, worker_steps=8)
        assert a["episodes"] == b["episodes"] and a["result"] == b["result"] and a["steps"] == b["steps"]
        assert len(a["episodes"]) == 8
        a = dev.evaluate(episodes_per_worker=1, n_workers=4, deterministic=False, seed=701, worker_steps=8)
        b = host.evaluate(episodes_per_worker=1, n_workers=4, deterministic=False, seed=701, worker_steps=8)
        assert a["episodes"] == b["episodes"] and a["result"] == b["result"]
    finally:
        _release(dev, host)


REFUSED = [(dict(worker_processes=True), "worker_processes: false"), (dict(bootstrap_truncated=True), "bootstrap_truncated")]


def refused_at_construction(env, run_id, over, match):
    with pytest.raises(ValueError, match=match):
        trainer(config(env, True, **over), run_id)


def worker_processes_are_refused_for_the_host_twin_too(env, run_id):
    # the shared segment's rows are float32 and these types have no float form
    with pytest.raises(ValueError, match="uint8"):
        trainer(config(env, False, worker_processes=True), run_id)


def refused_in_a_data_parallel_run(env, run_id):
    class _Dp:
        world, rank = 2, 0
    with pytest.raises(ValueError, match="data-parallel"):
        trainer(config(env, True), run_id + "_dp", dp=_Dp())
