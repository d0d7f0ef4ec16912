"""
Action tapes (include/locohip.h lm_rollout_tape), the parts that need no GPU: the C-ABI name, the argument checks of
HipBatch.rollout_tape (backend.check_tape_args, which runs without a device) and the conditions under which LocoEnv.step_chunk refuses.
"""

import os
import re
import subprocess

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv
from loco_mujoco_amd.backend import check_tape_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NU, NOBS, T = 5, 3, 4, 7


class _Buf:
    """What the checker looks at in a torch tensor: shape, dtype, contiguity, where it lives."""

    def __init__(self, shape, dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = tuple(shape), dtype, contiguous, is_cuda

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 0


def _ok(**kw):
    args = dict(actions=_Buf((T, N, NU)), obs=_Buf((T, N, NOBS)), reward=_Buf((T, N)), done=_Buf((T, N), "torch.uint8"),
                terminal=_Buf((T, N, NOBS)))
    args.update(kw)
    return check_tape_args(N, NU, NOBS, **args)


def test_abi_name_is_declared_exported_and_listed():
    from loco_mujoco_amd import backend
    header = open(os.path.join(ROOT, "include", "locohip.h")).read()
    declared = set(re.findall(r"\b(lm_[a-z_]+)\s*\(", header))
    lib = backend.load_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", backend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lm_[a-z_0-9]+)$", syms, flags=re.M))
    name = "lm_rollout_tape"
    assert name in declared and name in exported and name in backend.EXPORTS and hasattr(lib, name)
    assert lib.lm_rollout_tape(None, 1, 1, None, 0, None, None, None, None, None, 1, None) != 0 and b"null batch" in lib.lm_last_error()


def test_checker_accepts_tapes_and_action_repeat():
    assert _ok() == (T, N * NU, T)                                      # steps_per_launch defaults to T
    assert _ok(steps_per_launch=3) == (T, N * NU, 3)
    assert _ok(obs=None, reward=None, terminal=None) == (T, N * NU, T)    # every output is optional
    assert _ok(actions=_Buf((N, NU)), repeat=T) == (T, 0, T)            # [N, nu] with repeat: stride 0
    rep5 = dict(obs=_Buf((5, N, NOBS)), reward=_Buf((5, N)), done=_Buf((5, N), "torch.uint8"), terminal=None)
    assert _ok(actions=_Buf((N, NU)), repeat=5, steps_per_launch=2, **rep5) == (5, 0, 2)
    # raw device pointers are taken as given, with the number of steps stated
    assert check_tape_args(N, NU, NOBS, 0x1000, obs=0x2000, n_steps=T) == (T, N * NU, T)
    assert check_tape_args(N, NU, NOBS, 0x1000, repeat=4) == (4, 0, 4)


@pytest.mark.parametrize("kw,word", [
    (dict(actions=_Buf((T, N * NU))), "actions must be"),                          # wrong rank
    (dict(actions=_Buf((N, NU))), "actions must be"),                              # [N, nu] without repeat
    (dict(actions=_Buf((T, N, NU)), repeat=T), "with repeat"),                     # a tape with repeat
    (dict(actions=_Buf((T, N + 1, NU))), "actions must be"),
    (dict(actions=_Buf((T, N, NU), "torch.float64")), "actions must be float32"),  # wrong dtype
    (dict(done=_Buf((T, N), "torch.bool")), "done must be uint8"),
    (dict(obs=_Buf((T, N, NOBS), "torch.float16")), "obs must be float32"),
    (dict(obs=_Buf((T, N, NOBS), contiguous=False)), "obs must be contiguous"),    # non-contiguous
    (dict(actions=_Buf((T, N, NU), contiguous=False)), "actions must be contiguous"),
    (dict(obs=_Buf((T - 1, N, NOBS))), "obs tape holds 6 steps"),                  # T mismatches between tapes
    (dict(reward=_Buf((T + 1, N))), "reward tape holds 8 steps"),
    (dict(terminal=_Buf((1, N, NOBS))), "terminal tape holds 1 steps"),
    (dict(obs=_Buf((T, N, NOBS + 1))), "obs must be"),
    (dict(reward=_Buf((T, N, 1))), "reward must be"),
    (dict(obs=_Buf((T, N, NOBS), is_cuda=False)), "must live on the device"),
    (dict(actions=None), "actions is None"),
    (dict(actions=0x1000), "needs n_steps"),
    (dict(steps_per_launch=0), "steps_per_launch"),
    (dict(actions=_Buf((N, NU)), repeat=0, obs=None, reward=None, done=None, terminal=None), "T must be"),
    (dict(terminal_enabled=False), "terminal observations enabled"),
    (dict(n_steps=T + 1), "n_steps"),
    (dict(actions=np.zeros((T, N, NU), dtype=np.float32)), "actions must be a device tensor"),   # a host array is no device buffer
    (dict(obs=np.zeros((T, N, NOBS), dtype=np.float32)), "obs must be a device tensor"),
    (dict(done=[0] * N), "done must be a device tensor"),
])
def test_checker_rejects(kw, word):
    with pytest.raises(ValueError, match=word):
        _ok(**kw)


def test_checker_takes_real_tensors():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError, match="must live on the device"):
        check_tape_args(N, NU, NOBS, torch.zeros((T, N, NU)))
    with pytest.raises(ValueError, match="actions must be contiguous"):
        check_tape_args(N, NU, NOBS, torch.zeros((T, NU, N)).transpose(1, 2))
    with pytest.raises(ValueError, match="actions must be float32"):
        check_tape_args(N, NU, NOBS, torch.zeros((T, N, NU), dtype=torch.float64))


def test_step_chunk_refusals_decided_without_a_batch():
    np.random.seed(0)
    assert LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=4)._step_chunk_refusal() is None
    assert LocoEnv.make("UnitreeA1.simple", debug=True)._step_chunk_refusal() is None
    # the reward reads foot-force columns: evaluated on the host after every step
    assert "reward runs on the host" in LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=4, use_foot_forces=True)._step_chunk_refusal()
    cfg = os.path.join(ROOT, "tests", "golden", "dr_talos_inertial.yaml")
    assert "model compiler" in LocoEnv.make("Talos.walk", debug=True, n_envs=4, domain_randomization_config=cfg)._step_chunk_refusal()
    assert "several models" in LocoEnv.make("HumanoidTorque4Ages.run.all", debug=True, n_envs=8)._step_chunk_refusal()
    env = LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=4, use_foot_forces=True)
    with pytest.raises(RuntimeError, match="reset"):
        env.step_chunk(np.zeros((2, 4, 12)))              # before reset(), like step()
    env._obs = np.zeros((4, env.info.observation_space.shape[0]))
    with pytest.raises(NotImplementedError, match="reward runs on the host"):
        env.step_chunk(np.zeros((2, 4, 12)))
