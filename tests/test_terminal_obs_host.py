"""
Terminal observations (include/locohip.h lm_set_terminal_obs), the parts that need no GPU: the C-ABI names, the error path of an
unusable handle, and what LocoEnv.step() puts into `info` — on the fp64 oracle stand-in the host tests use (tests/oracle_backend.py),
extended by the few calls `enable_auto_reset` makes on a batch.
"""

import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

from loco_mujoco_amd import LocoEnv

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_backend import OracleBatch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lm_set_terminal_obs", "lm_get_terminal_obs", "lm_pinned_terminal_obs"]


def test_abi_names_are_declared_exported_and_listed():
    from loco_mujoco_amd import backend
    header = open(os.path.join(ROOT, "include", "locohip.h")).read()
    declared = set(re.findall(r"\b(lm_[a-z_]+)\s*\(", header))
    lib = backend.load_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", backend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lm_[a-z_0-9]+)$", syms, flags=re.M))
    for name in NAMES:
        assert name in declared and name in exported and name in backend.EXPORTS and hasattr(lib, name), name


def test_entry_points_refuse_a_null_batch_with_a_message():
    """Without a device no batch can exist; the entry points still fail cleanly (the GPU suite checks "not enabled" on a real one)."""
    from loco_mujoco_amd import backend
    lib = backend.load_library()
    buf = np.zeros(4, dtype=np.float32)
    ptr = C.POINTER(C.c_double)()
    for rc in (lib.lm_get_terminal_obs(None, buf.ctypes.data_as(C.POINTER(C.c_float))), lib.lm_set_terminal_obs(None, 1, None),
               lib.lm_pinned_terminal_obs(None, 0, C.byref(ptr))):
        assert rc != 0 and b"null batch" in lib.lm_last_error()


class _RestartingOracle(OracleBatch):
    """The oracle stand-in with the calls of a batch that restarts on the device: it ends every episode at the horizon WITHOUT
    restarting it (the host logic under test only routes flags and rows), and keeps the observation of that step as the terminal one."""

    def set_reset_table(self, rows, seed=0, global_env_offset=0):
        self.table = np.asarray(rows)

    def set_auto_reset(self, enabled, horizon=0):
        self.horizon, self.t = int(horizon), 0

    def enable_terminal_obs(self, out=None):
        self._term_on = True
        self._term = None

    def disable_terminal_obs(self):
        self._term_on = False

    def terminal_obs(self):
        return self._term.astype(np.float32)

    def step(self, action):
        obs, rew, done = super().step(action)
        self.t += 1
        ended = np.full(self.n, self.horizon > 0 and self.t % self.horizon == 0) | done
        self.last_restarted = ended
        if getattr(self, "_term_on", False):
            if self._term is None:
                self._term = np.zeros_like(obs)
            self._term[ended] = obs[ended]
        return obs, rew, done


def _env(n_envs):
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=n_envs, copy_outputs=True)
    env._backend = _RestartingOracle(env)
    env.reset()
    return env


def test_info_keys_without_the_keyword_are_unchanged():
    env = _env(2)
    env.enable_auto_reset(seed=1, horizon=2)
    keys = [set(env.step(np.zeros((2, 12)))[3].keys()) for _ in range(2)]
    assert keys == [{"episode_restarted"}, {"episode_restarted"}]
    assert not getattr(env._backend, "_term_on", False)


def test_terminal_observation_shapes_for_one_and_several_environments():
    env = _env(1)
    env.enable_auto_reset(seed=1, horizon=2, terminal_observations=True)
    obs, _, _, info = env.step(np.zeros(12))
    assert info["episode_restarted"] is False and info["terminal_observation"] is None
    obs, _, _, info = env.step(np.zeros(12))
    term = info["terminal_observation"]
    assert info["episode_restarted"] is True and term.shape == obs.shape == (37,) and term.dtype == np.float64
    assert np.allclose(term, obs, atol=1e-6)              # the stand-in does not restart: the step's observation, through float32
    env = _env(2)
    env.enable_auto_reset(seed=1, horizon=1, terminal_observations=True)
    obs, _, _, info = env.step(np.zeros((2, 12)))
    assert set(info.keys()) == {"episode_restarted", "terminal_observation"}
    assert info["terminal_observation"].shape == obs.shape == (2, 37) and info["terminal_observation"].dtype == np.float64
    # switching the keyword off again removes the key
    env.enable_auto_reset(seed=1, horizon=1)
    assert set(env.step(np.zeros((2, 12)))[3].keys()) == {"episode_restarted"}
