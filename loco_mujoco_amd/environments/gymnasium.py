"""
Gymnasium front-end (reference: ``loco_mujoco/environments/gymnasium.py:11-173``): 5-tuple ``step``
with ``truncated`` always False, ``reset(seed, options) -> (obs, {})``, float64 Box spaces.
``gymnasium`` itself is optional: without it the wrapper is a plain class with the same methods and
``make("LocoMujoco", env_name=...)`` below stands in for ``gym.make``. The batched surface on device tensors is
:class:`loco_mujoco_amd.vector.LocoVectorEnv` (``make_vec`` below / the registration's ``vector_entry_point``).
"""

import numpy as np

from .base import LocoEnv

try:                                    # pragma: no cover - depends on the installation
    import gymnasium as _gym
    from gymnasium import spaces as _spaces
    _Env = _gym.Env
except ImportError:                     # gymnasium is not part of this image
    _gym = None

    class _Env:                         # minimal stand-in for gymnasium.Env
        metadata = {}

    class _Box:
        def __init__(self, low, high, shape=None, dtype=np.float64):
            self.low, self.high, self.shape, self.dtype = np.asarray(low, dtype), np.asarray(high, dtype), shape, dtype

        def sample(self):
            lo = np.where(np.isfinite(self.low), self.low, -1.0)
            hi = np.where(np.isfinite(self.high), self.high, 1.0)
            return np.random.uniform(lo, hi).astype(self.dtype)

    class _spaces:
        Box = _Box


class GymnasiumWrapper(_Env):
    """Wraps a :class:`LocoEnv` (``n_envs=1``) in the Gymnasium API."""

    metadata = {"render_modes": ["human", "rgb_array"], "render_fps": 100}

    def __init__(self, env_name, render_mode=None, **kwargs):
        self.spec = None
        self.render_mode = render_mode
        self._env = LocoEnv.make(env_name, **kwargs)
        self.metadata = dict(self.metadata, render_fps=1.0 / self._env.dt)
        self.observation_space = self._convert_space(self._env.info.observation_space)
        self.action_space = self._convert_space(self._env.info.action_space)

    def step(self, action):
        obs, reward, absorbing, info = self._env.step(action)
        return obs, reward, absorbing, False, info

    def reset(self, *, seed=None, options=None):
        # like the reference (environments/gymnasium.py:73-77): a passed seed initialises the wrapper's OWN generator (gymnasium's
        # `np_random`); the environment draws from the global `np.random`, which this call does not touch
        if seed is not None:
            self._np_random = np.random.default_rng(seed)
        return self._env.reset(), {}

    def render(self):
        return self._env.render()

    def close(self):
        self._env.stop()

    def create_dataset(self, **kwargs):
        return self._env.create_dataset(**kwargs)

    def play_trajectory(self, **kwargs):
        return self._env.play_trajectory(**kwargs)

    def play_trajectory_from_velocity(self, **kwargs):
        return self._env.play_trajectory_from_velocity(**kwargs)

    def _set_observation_space(self):
        self.observation_space = self._convert_space(self._env.info.observation_space)
        return self.observation_space

    def _set_action_space(self):
        self.action_space = self._convert_space(self._env.info.action_space)
        return self.action_space

    @property
    def unwrapped(self):
        return self._env

    @staticmethod
    def _convert_space(space):
        low = np.min(space.low)
        high = np.max(space.high)
        return _spaces.Box(low, high, shape=space.shape, dtype=space.low.dtype)


def make(env_id, env_name=None, **kwargs):
    """Stand-in for ``gymnasium.make("LocoMujoco", env_name=...)`` when gymnasium is absent."""
    assert env_id == "LocoMujoco"
    return GymnasiumWrapper(env_name, **kwargs)


def make_vec(env_id, env_name=None, num_envs=1, **kwargs):
    """Stand-in for ``gymnasium.make_vec("LocoMujoco", env_name=..., num_envs=...)`` when gymnasium is absent: the batched surface on
    device tensors (:class:`loco_mujoco_amd.vector.LocoVectorEnv`)."""
    assert env_id == "LocoMujoco"
    from ..vector import LocoVectorEnv
    return LocoVectorEnv(env_name, num_envs, **kwargs)


if _gym is not None:                    # pragma: no cover
    try:
        try:
            _gym.register("LocoMujoco", entry_point="loco_mujoco_amd.environments.gymnasium:GymnasiumWrapper",
                          vector_entry_point="loco_mujoco_amd.vector:LocoVectorEnv")
        except TypeError:               # a gymnasium from before vector entry points: the single-environment registration as it was
            _gym.register("LocoMujoco", entry_point="loco_mujoco_amd.environments.gymnasium:GymnasiumWrapper")
    except Exception:
        pass
