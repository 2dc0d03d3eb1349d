"""Hidden-arm task: the demonstration environment of ``previous_step_input``.

Each episode draws one of ``arms`` arms uniformly and hides it; the observation is a constant vector, so nothing the agent sees says
which arm it is, which arm it pulled or what it was paid.  The reward of a step is 1 when the action equals the hidden arm, else 0;
an episode lasts ``max_episode_steps`` steps.  A policy that is not told its previous action and reward cannot beat 1 / ``arms`` per
step (0.5 with two arms); one that is can learn win-stay / lose-shift, which with two arms earns 1 from the second step on at the
latest.  Uses its own ``numpy.random.Generator`` (seedable).
"""
from types import SimpleNamespace

import numpy as np


class HiddenArmEnv:
    def __init__(self, arms: int = 2, max_episode_steps: int = 16, seed=None):
        if int(arms) < 2 or int(max_episode_steps) < 1:
            raise ValueError("HiddenArmEnv needs at least two arms and one step per episode")
        self.arms, self.max_episode_steps = int(arms), int(max_episode_steps)
        self._rng = np.random.default_rng(seed)
        self._obs = np.ones(2, dtype=np.float32)
        self._arm, self._t, self._total = 0, 0, 0.0

    @property
    def observation_space(self):
        return SimpleNamespace(shape=(2,), low=0.0, high=1.0, dtype=np.float32)

    @property
    def action_space(self):
        return SimpleNamespace(n=self.arms)

    def reset(self, **kwargs):
        self._arm = int(self._rng.integers(self.arms))
        self._t, self._total = 0, 0.0
        return self._obs.copy()

    def step(self, action):
        a = int(np.asarray(action).reshape(-1)[0])
        reward = 1.0 if a == self._arm else 0.0
        self._total += reward
        self._t += 1
        done = self._t >= self.max_episode_steps
        info = {"reward": float(self._total), "length": self._t} if done else None
        return self._obs.copy(), reward, bool(done), info

    def close(self):
        return None
