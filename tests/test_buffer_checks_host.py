"""
The device-buffer checks of the backend, the host side (no GPU): for every public entry that takes device buffers and every buffer
argument of it, what each fault is answered with — the WHOLE message, so that the wording, and which of two faults is reported, stay what
they are. Device tensors are stood in for by the description object of tests/test_policy_rollout_host.py. Also here: the list of
exports, in its order, and that each has its prototype declared.
"""

import types

import numpy as np
import pytest

from loco_mujoco_amd import backend
from loco_mujoco_amd.backend import (HipBatch, MlpPolicy, check_gae_args, check_obs_norm_args, check_policy_args, check_restore_args,
                                     check_tape_args)
from test_policy_rollout_host import NOBS, NU, N, T, Dev, _count, _policy

SIZES = (NOBS, 40, NU)
COUNT = _count(SIZES)

# entry, buffer argument, its shape, its dtype
PAIRS = [
    ("check_tape_args", "actions", (T, N, NU), "float32"), ("check_tape_args", "obs", (T, N, NOBS), "float32"),
    ("check_tape_args", "reward", (T, N), "float32"), ("check_tape_args", "done", (T, N), "uint8"),
    ("check_tape_args", "terminal", (T, N, NOBS), "float32"),
    ("check_policy_args", "obs0", (N, NOBS), "float32"), ("check_policy_args", "actions", (T, N, NU), "float32"),
    ("check_policy_args", "obs", (T, N, NOBS), "float32"), ("check_policy_args", "reward", (T, N), "float32"),
    ("check_policy_args", "done", (T, N), "uint8"), ("check_policy_args", "terminal", (T, N, NOBS), "float32"),
    ("MlpPolicy", "params", (COUNT,), "float32"), ("MlpPolicy", "log_std", (NU,), "float32"),
    ("check_obs_norm_args", "mean", (NOBS,), "float32"), ("check_obs_norm_args", "inv_std", (NOBS,), "float32"),
    ("check_gae_args", "reward", (T, N), "float32"), ("check_gae_args", "done", (T, N), "uint8"), ("check_gae_args", "value", (T, N), "float32"),
    ("check_gae_args", "last_value", (N,), "float32"), ("check_gae_args", "term_value", (T, N), "float32"),
    ("check_gae_args", "adv", (T, N), "float32"), ("check_gae_args", "ret", (T, N), "float32"),
    ("check_restore_args", "src", (N,), "int32"), ("check_restore_args", "mask", (N,), "bool"),
    ("enable_terminal_obs", "out", (N, NOBS), "float32"),
]
FAULTS = ("neither", "shape", "dtype", "strided", "host", "raw")
WRONG_DTYPE = {"float32": "torch.float64", "uint8": "torch.bool", "int32": "torch.int64", "bool": "torch.uint8"}


def _faulty(fault, shape, dtype):
    """The argument with one fault: neither a pointer nor a tensor (a host array), one column too many, another dtype, not contiguous,
    on the host — and `raw`, a raw device pointer, which has no fault to find."""
    if fault == "neither":
        return np.zeros(shape, dtype=np.float32)
    if fault == "raw":
        return 0x1000
    return Dev(shape[:-1] + (shape[-1] + 1,) if fault == "shape" else shape, WRONG_DTYPE[dtype] if fault == "dtype" else "torch." + dtype,
               contiguous=fault != "strided", cuda=fault != "host")


def _terminal(out):
    b = object.__new__(HipBatch)          # the check runs before the library is called: no library, no device
    b.n, b.nobs, b._h, calls = N, NOBS, None, []
    b._lib = types.SimpleNamespace(lm_set_terminal_obs=lambda *a: calls.append(a) or 0)
    try:
        b.enable_terminal_obs(out)
    except Exception:
        assert not calls                  # refused: nothing reached the library
        raise
    assert len(calls) == 1 and b._term_on and b._term_out is out


def _gae(**kw):
    args = dict(reward=Dev((T, N)), done=Dev((T, N), "torch.uint8"), value=Dev((T, N)), last_value=Dev((N,)))
    args.update(kw)
    return check_gae_args(N, **args)


def _mlp(**kw):
    args = dict(params=Dev((COUNT,)), log_std=Dev((NU,)))
    args.update(kw)
    return MlpPolicy(SIZES, "tanh", **args)


def _norm(clip=5.0, **kw):
    args = dict(mean=Dev((NOBS,)), inv_std=Dev((NOBS,)))
    args.update(kw)
    return check_obs_norm_args(NOBS, clip=clip, **args)


def _tape(**kw):
    args = dict(actions=Dev((T, N, NU)))
    args.update(kw)
    return check_tape_args(N, NU, NOBS, **args)


ENTRIES = {
    "check_tape_args": _tape,
    "check_policy_args": lambda **kw: check_policy_args(N, NU, NOBS, _policy(), T, **kw),
    "MlpPolicy": _mlp,
    "check_obs_norm_args": _norm,
    "check_gae_args": _gae,
    "check_restore_args": lambda **kw: check_restore_args(N, **kw),
    "enable_terminal_obs": _terminal,
}


def _answer(call, **kw):
    """What a call is answered with: None (accepted), the ValueError's whole message, or another exception's class."""
    try:
        call(**kw)
    except ValueError as e:
        return str(e)
    except Exception as e:
        return type(e)
    return None


# entry, argument, fault, the answer. None: accepted — a raw pointer is taken as given, restore takes host values for what is no
# tensor; TypeError: enable_terminal_obs hands what is no tensor to int(), whose wording is Python's
ROWS = [
    ("check_tape_args", "actions", "neither", 'rollout_tape: actions must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", "actions", "shape", 'rollout_tape: actions must be [7, 5, 12], not [7, 5, 13]'),
    ("check_tape_args", "actions", "dtype", 'rollout_tape: actions must be float32, not torch.float64'),
    ("check_tape_args", "actions", "strided", 'rollout_tape: actions must be contiguous'),
    ("check_tape_args", "actions", "host", 'rollout_tape: actions must live on the device'),
    ("check_tape_args", "actions", "raw", 'rollout_tape: a raw action pointer needs n_steps (a tape) or repeat'),
    ("check_tape_args", "obs", "neither", 'rollout_tape: obs must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", "obs", "shape", 'rollout_tape: obs must be [7, 5, 37], not [7, 5, 38]'),
    ("check_tape_args", "obs", "dtype", 'rollout_tape: obs must be float32, not torch.float64'),
    ("check_tape_args", "obs", "strided", 'rollout_tape: obs must be contiguous'),
    ("check_tape_args", "obs", "host", 'rollout_tape: obs must live on the device'),
    ("check_tape_args", "obs", "raw", None),
    ("check_tape_args", "reward", "neither", 'rollout_tape: reward must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", "reward", "shape", 'rollout_tape: reward must be [7, 5], not [7, 6]'),
    ("check_tape_args", "reward", "dtype", 'rollout_tape: reward must be float32, not torch.float64'),
    ("check_tape_args", "reward", "strided", 'rollout_tape: reward must be contiguous'),
    ("check_tape_args", "reward", "host", 'rollout_tape: reward must live on the device'),
    ("check_tape_args", "reward", "raw", None),
    ("check_tape_args", "done", "neither", 'rollout_tape: done must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", "done", "shape", 'rollout_tape: done must be [7, 5], not [7, 6]'),
    ("check_tape_args", "done", "dtype", 'rollout_tape: done must be uint8, not torch.bool'),
    ("check_tape_args", "done", "strided", 'rollout_tape: done must be contiguous'),
    ("check_tape_args", "done", "host", 'rollout_tape: done must live on the device'),
    ("check_tape_args", "done", "raw", None),
    ("check_tape_args", "terminal", "neither", 'rollout_tape: terminal must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", "terminal", "shape", 'rollout_tape: terminal must be [7, 5, 37], not [7, 5, 38]'),
    ("check_tape_args", "terminal", "dtype", 'rollout_tape: terminal must be float32, not torch.float64'),
    ("check_tape_args", "terminal", "strided", 'rollout_tape: terminal must be contiguous'),
    ("check_tape_args", "terminal", "host", 'rollout_tape: terminal must live on the device'),
    ("check_tape_args", "terminal", "raw", None),
    ("check_policy_args", "obs0", "neither", 'rollout_policy: obs0 must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "obs0", "shape", 'rollout_policy: obs0 must be [5, 37], not [5, 38]'),
    ("check_policy_args", "obs0", "dtype", 'rollout_policy: obs0 must be float32, not torch.float64'),
    ("check_policy_args", "obs0", "strided", 'rollout_policy: obs0 must be contiguous'),
    ("check_policy_args", "obs0", "host", 'rollout_policy: obs0 must live on the device'),
    ("check_policy_args", "obs0", "raw", None),
    ("check_policy_args", "actions", "neither", 'rollout_policy: actions must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "actions", "shape", 'rollout_policy: actions must be [7, 5, 12], not [7, 5, 13]'),
    ("check_policy_args", "actions", "dtype", 'rollout_policy: actions must be float32, not torch.float64'),
    ("check_policy_args", "actions", "strided", 'rollout_policy: actions must be contiguous'),
    ("check_policy_args", "actions", "host", 'rollout_policy: actions must live on the device'),
    ("check_policy_args", "actions", "raw", None),
    ("check_policy_args", "obs", "neither", 'rollout_policy: obs must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "obs", "shape", 'rollout_policy: obs must be [7, 5, 37], not [7, 5, 38]'),
    ("check_policy_args", "obs", "dtype", 'rollout_policy: obs must be float32, not torch.float64'),
    ("check_policy_args", "obs", "strided", 'rollout_policy: obs must be contiguous'),
    ("check_policy_args", "obs", "host", 'rollout_policy: obs must live on the device'),
    ("check_policy_args", "obs", "raw", None),
    ("check_policy_args", "reward", "neither", 'rollout_policy: reward must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "reward", "shape", 'rollout_policy: reward must be [7, 5], not [7, 6]'),
    ("check_policy_args", "reward", "dtype", 'rollout_policy: reward must be float32, not torch.float64'),
    ("check_policy_args", "reward", "strided", 'rollout_policy: reward must be contiguous'),
    ("check_policy_args", "reward", "host", 'rollout_policy: reward must live on the device'),
    ("check_policy_args", "reward", "raw", None),
    ("check_policy_args", "done", "neither", 'rollout_policy: done must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "done", "shape", 'rollout_policy: done must be [7, 5], not [7, 6]'),
    ("check_policy_args", "done", "dtype", 'rollout_policy: done must be uint8, not torch.bool'),
    ("check_policy_args", "done", "strided", 'rollout_policy: done must be contiguous'),
    ("check_policy_args", "done", "host", 'rollout_policy: done must live on the device'),
    ("check_policy_args", "done", "raw", None),
    ("check_policy_args", "terminal", "neither", 'rollout_policy: terminal must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_policy_args", "terminal", "shape", 'rollout_policy: terminal must be [7, 5, 37], not [7, 5, 38]'),
    ("check_policy_args", "terminal", "dtype", 'rollout_policy: terminal must be float32, not torch.float64'),
    ("check_policy_args", "terminal", "strided", 'rollout_policy: terminal must be contiguous'),
    ("check_policy_args", "terminal", "host", 'rollout_policy: terminal must live on the device'),
    ("check_policy_args", "terminal", "raw", None),
    ("MlpPolicy", "params", "neither", 'MlpPolicy: params must be a device tensor (data_ptr()), not ndarray'),
    ("MlpPolicy", "params", "shape", 'MlpPolicy: params must be a flat tensor of 2012 elements, not [2013]'),
    ("MlpPolicy", "params", "dtype", 'MlpPolicy: params must be float32, not torch.float64'),
    ("MlpPolicy", "params", "strided", 'MlpPolicy: params must be contiguous'),
    ("MlpPolicy", "params", "host", 'MlpPolicy: params must live on the device'),
    ("MlpPolicy", "params", "raw", 'MlpPolicy: params must be a device tensor (data_ptr()), not int'),
    ("MlpPolicy", "log_std", "neither", 'MlpPolicy: log_std must be a device tensor (data_ptr()), not ndarray'),
    ("MlpPolicy", "log_std", "shape", 'MlpPolicy: log_std must be a flat tensor of 12 elements, not [13]'),
    ("MlpPolicy", "log_std", "dtype", 'MlpPolicy: log_std must be float32, not torch.float64'),
    ("MlpPolicy", "log_std", "strided", 'MlpPolicy: log_std must be contiguous'),
    ("MlpPolicy", "log_std", "host", 'MlpPolicy: log_std must live on the device'),
    ("MlpPolicy", "log_std", "raw", 'MlpPolicy: log_std must be a device tensor (data_ptr()), not int'),
    ("check_obs_norm_args", "mean", "neither", 'set_policy_obs_norm: mean must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_obs_norm_args", "mean", "shape", 'set_policy_obs_norm: mean must be [37], not [38]'),
    ("check_obs_norm_args", "mean", "dtype", 'set_policy_obs_norm: mean must be float32, not torch.float64'),
    ("check_obs_norm_args", "mean", "strided", 'set_policy_obs_norm: mean must be contiguous'),
    ("check_obs_norm_args", "mean", "host", 'set_policy_obs_norm: mean must live on the device'),
    ("check_obs_norm_args", "mean", "raw", None),
    ("check_obs_norm_args", "inv_std", "neither", 'set_policy_obs_norm: inv_std must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_obs_norm_args", "inv_std", "shape", 'set_policy_obs_norm: inv_std must be [37], not [38]'),
    ("check_obs_norm_args", "inv_std", "dtype", 'set_policy_obs_norm: inv_std must be float32, not torch.float64'),
    ("check_obs_norm_args", "inv_std", "strided", 'set_policy_obs_norm: inv_std must be contiguous'),
    ("check_obs_norm_args", "inv_std", "host", 'set_policy_obs_norm: inv_std must live on the device'),
    ("check_obs_norm_args", "inv_std", "raw", None),
    ("check_gae_args", "reward", "neither", 'gae: reward must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "reward", "shape", 'gae: reward must be [7, 5], not [7, 6]'),
    ("check_gae_args", "reward", "dtype", 'gae: reward must be float32, not torch.float64'),
    ("check_gae_args", "reward", "strided", 'gae: reward must be contiguous'),
    ("check_gae_args", "reward", "host", 'gae: reward must live on the device'),
    ("check_gae_args", "reward", "raw", None),
    ("check_gae_args", "done", "neither", 'gae: done must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "done", "shape", 'gae: done must be [7, 5], not [7, 6]'),
    ("check_gae_args", "done", "dtype", 'gae: done must be uint8, not torch.bool'),
    ("check_gae_args", "done", "strided", 'gae: done must be contiguous'),
    ("check_gae_args", "done", "host", 'gae: done must live on the device'),
    ("check_gae_args", "done", "raw", None),
    ("check_gae_args", "value", "neither", 'gae: value must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "value", "shape", 'gae: value must be [7, 5], not [7, 6]'),
    ("check_gae_args", "value", "dtype", 'gae: value must be float32, not torch.float64'),
    ("check_gae_args", "value", "strided", 'gae: value must be contiguous'),
    ("check_gae_args", "value", "host", 'gae: value must live on the device'),
    ("check_gae_args", "value", "raw", None),
    ("check_gae_args", "last_value", "neither", 'gae: last_value must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "last_value", "shape", 'gae: last_value must be [5], not [6]'),
    ("check_gae_args", "last_value", "dtype", 'gae: last_value must be float32, not torch.float64'),
    ("check_gae_args", "last_value", "strided", 'gae: last_value must be contiguous'),
    ("check_gae_args", "last_value", "host", 'gae: last_value must live on the device'),
    ("check_gae_args", "last_value", "raw", None),
    ("check_gae_args", "term_value", "neither", 'gae: term_value must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "term_value", "shape", 'gae: term_value must be [7, 5], not [7, 6]'),
    ("check_gae_args", "term_value", "dtype", 'gae: term_value must be float32, not torch.float64'),
    ("check_gae_args", "term_value", "strided", 'gae: term_value must be contiguous'),
    ("check_gae_args", "term_value", "host", 'gae: term_value must live on the device'),
    ("check_gae_args", "term_value", "raw", None),
    ("check_gae_args", "adv", "neither", 'gae: adv must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "adv", "shape", 'gae: adv must be [7, 5], not [7, 6]'),
    ("check_gae_args", "adv", "dtype", 'gae: adv must be float32, not torch.float64'),
    ("check_gae_args", "adv", "strided", 'gae: adv must be contiguous'),
    ("check_gae_args", "adv", "host", 'gae: adv must live on the device'),
    ("check_gae_args", "adv", "raw", None),
    ("check_gae_args", "ret", "neither", 'gae: ret must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_gae_args", "ret", "shape", 'gae: ret must be [7, 5], not [7, 6]'),
    ("check_gae_args", "ret", "dtype", 'gae: ret must be float32, not torch.float64'),
    ("check_gae_args", "ret", "strided", 'gae: ret must be contiguous'),
    ("check_gae_args", "ret", "host", 'gae: ret must live on the device'),
    ("check_gae_args", "ret", "raw", None),
    ("check_restore_args", "src", "neither", 'restore: src must hold integers, not float32'),
    ("check_restore_args", "src", "shape", 'restore: src must be [5], not [6]'),
    ("check_restore_args", "src", "dtype", 'restore: a src tensor must be int32, not torch.int64'),
    ("check_restore_args", "src", "strided", 'restore: src must be contiguous'),
    ("check_restore_args", "src", "host", 'restore: a src tensor must live on the device (host values: a numpy array or a list)'),
    ("check_restore_args", "src", "raw", 'restore: src must be a sequence of 5 entries, not int'),
    ("check_restore_args", "mask", "neither", 'restore: mask must hold booleans, not float32'),
    ("check_restore_args", "mask", "shape", 'restore: mask must be [5], not [6]'),
    ("check_restore_args", "mask", "dtype", 'restore: a mask tensor must be bool, not torch.uint8'),
    ("check_restore_args", "mask", "strided", 'restore: mask must be contiguous'),
    ("check_restore_args", "mask", "host", 'restore: a mask tensor must live on the device (host values: a numpy array or a list)'),
    ("check_restore_args", "mask", "raw", 'restore: mask must be a sequence of 5 entries, not int'),
    ("enable_terminal_obs", "out", "neither", TypeError),
    ("enable_terminal_obs", "out", "shape", 'terminal observations: the buffer must be [5, 37], not (5, 38)'),
    ("enable_terminal_obs", "out", "dtype", 'terminal observations: the buffer must be float32, not torch.float64'),
    ("enable_terminal_obs", "out", "strided", 'terminal observations: the buffer must be contiguous'),
    ("enable_terminal_obs", "out", "host", 'terminal observations: the buffer must live on the device'),
    ("enable_terminal_obs", "out", "raw", None),
]


def test_every_pair_is_in_the_table_with_every_fault():
    assert [r[:3] for r in ROWS] == [(entry, arg, fault) for entry, arg, _, _ in PAIRS for fault in FAULTS]


@pytest.mark.parametrize("entry,arg,fault,answer", ROWS, ids=["%s-%s-%s" % r[:3] for r in ROWS])
def test_one_fault_in_one_buffer(entry, arg, fault, answer):
    shape, dtype = next(p[2:] for p in PAIRS if p[:2] == (entry, arg))
    assert _answer(ENTRIES[entry], **{arg: _faulty(fault, shape, dtype)}) == answer


F64, HOST_ARRAY = "torch.float64", np.zeros((T, N, NOBS), dtype=np.float32)


# an input with two faults: which of them is reported is behaviour
@pytest.mark.parametrize("entry,kw,answer", [
    # every buffer is looked at for being one before "actions is None", and that comes before any dtype
    ("check_tape_args", dict(actions=None, obs=HOST_ARRAY), 'rollout_tape: obs must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray'),
    ("check_tape_args", dict(actions=None, done=Dev((T, N))), 'rollout_tape: actions is None (policy-free rollouts: rollout())'),
    # a tape's length before its dtype; the actions before the other tapes, those in the order obs, reward, done, terminal
    ("check_tape_args", dict(obs=Dev((T - 1, N, NOBS), F64)), 'rollout_tape: the obs tape holds 6 steps, the actions T = 7'),
    ("check_tape_args", dict(actions=Dev((T, N, NU), F64), obs=Dev((T - 1, N, NOBS))), 'rollout_tape: actions must be float32, not torch.float64'),
    ("check_tape_args", dict(actions=Dev((T, N, NU), F64), n_steps=T + 1), 'rollout_tape: n_steps = 8, but the action tape holds T = 7 steps'),
    ("check_tape_args", dict(actions=Dev((T, N, NU)), repeat=T, n_steps=T + 1), 'rollout_tape: n_steps and repeat disagree'),
    ("check_tape_args", dict(actions=Dev((N, NU + 1), F64), repeat=T), 'rollout_tape: actions must be [5, 12], not [5, 13]'),
    ("check_tape_args", dict(reward=Dev((T, N), cuda=False), done=Dev((T, N))), 'rollout_tape: reward must live on the device'),
    # of one buffer: shape, dtype, contiguous, device
    ("check_tape_args", dict(obs=Dev((T, N, NOBS + 1), F64)), 'rollout_tape: obs must be [7, 5, 37], not [7, 5, 38]'),
    ("check_tape_args", dict(obs=Dev((T, N, NOBS), F64, contiguous=False)), 'rollout_tape: obs must be float32, not torch.float64'),
    ("check_tape_args", dict(obs=Dev((T, N, NOBS), contiguous=False, cuda=False)), 'rollout_tape: obs must be contiguous'),
    # the buffers, then terminal observations enabled, then steps_per_launch
    ("check_tape_args", dict(terminal=Dev((T, N, NOBS + 1)), terminal_enabled=False), 'rollout_tape: terminal must be [7, 5, 37], not [7, 5, 38]'),
    ("check_tape_args", dict(terminal=Dev((T, N, NOBS)), terminal_enabled=False, steps_per_launch=0),
     'rollout_tape: a terminal tape needs terminal observations enabled (enable_terminal_obs)'),
    ("check_policy_args", dict(obs0=Dev((N, NOBS + 1), F64)), 'rollout_policy: obs0 must be [5, 37], not [5, 38]'),
    ("check_policy_args", dict(obs0=Dev((N, NOBS), cuda=False), actions=Dev((T, N, NU), F64)), 'rollout_policy: obs0 must live on the device'),
    ("check_policy_args", dict(actions=Dev((T, N, NU), F64, contiguous=False)), 'rollout_policy: actions must be float32, not torch.float64'),
    ("check_policy_args", dict(obs=HOST_ARRAY, actions=Dev((T, N, NU + 1))), 'rollout_policy: actions must be [7, 5, 12], not [7, 5, 13]'),
    ("check_policy_args", dict(terminal=Dev((T, N, NOBS + 1)), terminal_enabled=False), 'rollout_policy: terminal must be [7, 5, 37], not [7, 5, 38]'),
    ("check_policy_args", dict(terminal=Dev((T, N, NOBS)), terminal_enabled=False, steps_per_launch=0),
     'rollout_policy: a terminal tape needs terminal observations enabled (enable_terminal_obs)'),
    # MlpPolicy alone looks at the dtype before the shape
    ("MlpPolicy", dict(params=Dev((COUNT + 1,), F64)), 'MlpPolicy: params must be float32, not torch.float64'),
    ("MlpPolicy", dict(params=Dev((COUNT + 1,), contiguous=False)), 'MlpPolicy: params must be a flat tensor of 2012 elements, not [2013]'),
    ("MlpPolicy", dict(params=Dev((COUNT,), contiguous=False, cuda=False)), 'MlpPolicy: params must be contiguous'),
    ("MlpPolicy", dict(params=Dev((COUNT,), cuda=False), log_std=HOST_ARRAY), 'MlpPolicy: params must live on the device'),
    ("MlpPolicy", dict(params=Dev((COUNT, 1))), 'MlpPolicy: params must be a flat tensor of 2012 elements, not [2012, 1]'),
    # "go together", then clip, then the buffers
    ("check_obs_norm_args", dict(mean=HOST_ARRAY, clip="5"), 'set_policy_obs_norm: clip must be a number, not str'),
    ("check_obs_norm_args", dict(mean=None, clip=-1.0), 'set_policy_obs_norm: mean and inv_std go together (both None: off)'),
    ("check_obs_norm_args", dict(mean=Dev((NOBS,), cuda=False), inv_std=Dev((NOBS + 1,))), 'set_policy_obs_norm: mean must live on the device'),
    # None, then the tapes' lengths, then the buffers in the order of the arguments, then gamma and lam
    ("check_gae_args", dict(reward=None, done=HOST_ARRAY), 'gae: reward is None'),
    ("check_gae_args", dict(value=Dev((T + 1, N), F64)), 'gae: the value tape holds 8 steps, the others T = 7'),
    ("check_gae_args", dict(reward=Dev((T, N + 1), F64)), 'gae: reward must be [7, 5], not [7, 6]'),
    ("check_gae_args", dict(ret=Dev((T, N), F64), reward=Dev((T, N), cuda=False)), 'gae: reward must live on the device'),
    ("check_gae_args", dict(last_value=Dev((N,), F64), gamma=2.0), 'gae: last_value must be float32, not torch.float64'),
    ("check_gae_args", dict(gamma=2.0, lam="1"), 'gae: gamma must be in [0, 1], not 2.0'),
    ("check_restore_args", dict(src=Dev((N + 1,), "torch.int64")), 'restore: src must be [5], not [6]'),
    ("check_restore_args", dict(src=Dev((N,), "torch.int64", contiguous=False)), 'restore: a src tensor must be int32, not torch.int64'),
    ("check_restore_args", dict(mask=Dev((N,), "torch.bool", contiguous=False, cuda=False)), 'restore: mask must be contiguous'),
    ("check_restore_args", dict(src=Dev((N + 1,), "torch.int32"), mask=HOST_ARRAY), 'restore: give src or mask, not both'),
    ("enable_terminal_obs", dict(out=Dev((N, NOBS + 1), F64)), 'terminal observations: the buffer must be [5, 37], not (5, 38)'),
    ("enable_terminal_obs", dict(out=Dev((N * NOBS,), cuda=False)), 'terminal observations: the buffer must be [5, 37], not (185,)'),
    ("enable_terminal_obs", dict(out=Dev((N, NOBS), F64, contiguous=False)), 'terminal observations: the buffer must be float32, not torch.float64'),
])
def test_which_of_two_faults_is_reported(entry, kw, answer):
    assert _answer(ENTRIES[entry], **kw) == answer


def test_exports_are_the_same_list_and_each_has_its_prototype():
    assert list(backend.EXPORTS) == [
        "lm_device_count", "lm_last_error", "lm_toolchain", "lm_lds_bytes", "lm_model_create", "lm_model_destroy", "lm_model_dims",
        "lm_batch_create", "lm_batch_destroy", "lm_batch_set_layout", "lm_batch_set_replay", "lm_batch_set_active", "lm_get_replay_marks",
        "lm_set_state", "lm_get_state", "lm_set_activation", "lm_get_activation",
        "lm_set_dof_params", "lm_get_dof_params", "lm_set_dof_randomization", "lm_set_goal", "lm_step", "lm_step_device",
        "lm_pinned_slot", "lm_set_obs_order", "lm_step_pinned",
        "lm_set_terminal_obs", "lm_get_terminal_obs", "lm_pinned_terminal_obs",
        "lm_set_reset_table", "lm_set_auto_reset", "lm_rollout", "lm_rollout_fused", "lm_rollout_tape", "lm_rollout_policy",
        "lm_set_policy_obs_norm", "lm_tape_gae", "lm_forward_debug", "lm_get_stats", "lm_sync",
        "lm_get_flags", "lm_set_model_variants", "lm_set_variant_index", "lm_get_variant_index", "lm_set_variant_rows",
        "lm_set_model_compiler", "lm_compile_models", "lm_get_model_draws", "lm_get_model_tables",
        "lm_snapshot_create", "lm_snapshot_destroy", "lm_snapshot_save", "lm_snapshot_restore", "lm_snapshot_bytes",
        "lm_snapshot_export", "lm_snapshot_import"]
    lib = backend.load_library()
    # an export without argtypes converts its arguments by ctypes' defaults and nothing notices; the three that take no argument have none
    no_arguments = {"lm_device_count", "lm_last_error", "lm_toolchain"}
    assert [name for name in backend.EXPORTS if name not in no_arguments and getattr(lib, name).argtypes is None] == []
