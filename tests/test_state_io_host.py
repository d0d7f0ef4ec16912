"""
State on device buffers (include/locostate.h ls_get_state_device / ls_set_state_device / ls_restart_device), the parts that need no GPU:
the three C-ABI names, the argument checks of HipBatch.get_state_device / set_state_device / restart_device (backend.check_*_args, which
run without a device), the per-unit work of csrc/lm_state_io.h on the host under the address and undefined-behaviour sanitizers as a
stand-alone program (tests/state_io_main.cpp) with its restart draws against tests/step_bookkeeping_model.py, and the dof ->
observation-column maps of csrc/lm_model_parse.h (tests/obs_maps_main.cpp) against the tasks' own index lists.
"""

import os
import re
import subprocess

import numpy as np
import pytest

import step_bookkeeping_model as M
from loco_mujoco_amd import LocoEnv
from loco_mujoco_amd.backend import check_get_state_device_args, check_restart_device_args, check_state_device_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, NV, NA, NGOAL, NOBS = 5, 18, 3, 2, 37
NAMES = ["ls_get_state_device", "ls_set_state_device", "ls_restart_device"]
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


class _Buf:
    """What the checkers look at in a torch tensor: shape, dtype, contiguity, where it lives."""

    def __init__(self, shape, dtype="torch.float32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = tuple(shape), dtype, contiguous, is_cuda

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 0


def _get(**kw):
    return check_get_state_device_args(N, NV, NA, NGOAL, **kw)


def _set(qpos=_Buf((N, NV)), qvel=_Buf((N, NV)), **kw):
    return check_state_device_args(N, NV, NA, NGOAL, NOBS, qpos, qvel, **kw)


def _restart(**kw):
    return check_restart_device_args(N, NOBS, **kw)


def test_abi_names_are_declared_exported_and_listed():
    from loco_mujoco_amd import backend
    header = open(os.path.join(ROOT, "include", "locostate.h")).read()
    declared = set(re.findall(r"\b(ls_[a-z_]+)\s*\(", header))
    lib = backend.load_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", backend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (ls_[a-z_0-9]+)$", syms, flags=re.M))
    # the header's names, the library's ls_ symbols and the binding's table are one list; each has its prototype declared
    assert declared == exported == set(backend.STATE_EXPORTS) == set(NAMES)
    assert not set(backend.STATE_EXPORTS) & set(backend.EXPORTS)
    for name in NAMES:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None, name
    # a null batch is refused with a message before anything touches a device
    assert lib.ls_get_state_device(None, None, None, None, None, None, None, None, 1) != 0 and b"null" in lib.lm_last_error()
    assert lib.ls_set_state_device(None, None, None, None, None, None, None, None, 1) != 0 and b"null" in lib.lm_last_error()
    assert lib.ls_restart_device(None, None, None, None, 1) != 0 and b"null" in lib.lm_last_error()


def test_checkers_accept_described_tensors_and_raw_pointers():
    _get(qpos=_Buf((N, NV)), qvel=_Buf((N, NV)), act=_Buf((N, NA)), goal=_Buf((N, NGOAL)), ep_step=_Buf((N,), "torch.int32"),
         ep_count=_Buf((N,), "torch.int32"))
    _get(ep_count=_Buf((N,), "torch.uint32"))
    _get(qpos=0x7f0000000000, ep_step=np.int64(4096))
    _get()                                                   # no output at all: the library's refusal, not this layer's
    _set()
    _set(act=_Buf((N, NA)), goal=_Buf((N, NGOAL)), mask=_Buf((N,), "torch.bool"), obs=_Buf((N, NOBS)))
    _set(mask=_Buf((N,), "torch.uint8"))
    _set(qpos=1 << 40, qvel=1 << 41, act=1 << 42, goal=1 << 43, mask=1 << 44, obs=1 << 45)
    _restart()
    _restart(mask=_Buf((N,), "torch.bool"), obs=_Buf((N, NOBS)))
    _restart(mask=_Buf((N,), "torch.uint8"))
    _restart(mask=1 << 40, obs=1 << 41)
    # act for a model without activations is the library's refusal as well (na = 0: no shape to hold it to)
    check_state_device_args(N, NV, 0, NGOAL, NOBS, _Buf((N, NV)), _Buf((N, NV)), act=_Buf((N, 4)))


@pytest.mark.parametrize("call,kw,answer", [
    # a wrong dtype
    (_get, dict(qpos=_Buf((N, NV), "torch.float64")), "get_state_device: qpos must be float32, not torch.float64"),
    (_get, dict(ep_step=_Buf((N,), "torch.int64")), "get_state_device: ep_step must be int32, not torch.int64"),
    (_get, dict(ep_count=_Buf((N,), "torch.float32")), "get_state_device: ep_count must be int32, not torch.float32"),
    (_set, dict(qvel=_Buf((N, NV), "torch.float16")), "set_state_device: qvel must be float32, not torch.float16"),
    (_set, dict(mask=_Buf((N,), "torch.int32")), "set_state_device: mask must be uint8 or bool, not torch.int32"),
    (_restart, dict(mask=_Buf((N,), "torch.float32")), "restart_device: mask must be uint8 or bool, not torch.float32"),
    (_restart, dict(obs=_Buf((N, NOBS), "torch.float64")), "restart_device: obs must be float32, not torch.float64"),
    # a wrong shape
    (_get, dict(qvel=_Buf((NV, N))), "get_state_device: qvel must be [5, 18], not [18, 5]"),
    (_get, dict(act=_Buf((N, NA + 1))), "get_state_device: act must be [5, 3], not [5, 4]"),
    (_get, dict(goal=_Buf((N,))), "get_state_device: goal must be [5, 2], not [5]"),
    (_set, dict(qpos=_Buf((N, NV + 1))), "set_state_device: qpos must be [5, 18], not [5, 19]"),
    (_set, dict(obs=_Buf((N, NOBS - 1))), "set_state_device: obs must be [5, 37], not [5, 36]"),
    (_set, dict(mask=_Buf((N + 1,), "torch.bool")), "set_state_device: mask must be [5], not [6]"),
    (_restart, dict(mask=_Buf((N, 1), "torch.uint8")), "restart_device: mask must be [5], not [5, 1]"),
    (_restart, dict(obs=_Buf((N * NOBS,))), "restart_device: obs must be [5, 37], not [185]"),
    # a wrong device
    (_get, dict(qpos=_Buf((N, NV), is_cuda=False)), "get_state_device: qpos must live on the device"),
    (_set, dict(goal=_Buf((N, NGOAL), is_cuda=False)), "set_state_device: goal must live on the device"),
    (_restart, dict(mask=_Buf((N,), "torch.bool", is_cuda=False)), "restart_device: mask must live on the device"),
    # non-contiguity
    (_get, dict(ep_step=_Buf((N,), "torch.int32", contiguous=False)), "get_state_device: ep_step must be contiguous"),
    (_set, dict(qpos=_Buf((N, NV), contiguous=False)), "set_state_device: qpos must be contiguous"),
    (_restart, dict(obs=_Buf((N, NOBS), contiguous=False)), "restart_device: obs must be contiguous"),
    # a missing qpos / qvel
    (_set, dict(qpos=None), "set_state_device: qpos is None (a state is positions and velocities)"),
    (_set, dict(qvel=None), "set_state_device: qvel is None (a state is positions and velocities)"),
    # no buffer at all
    (_get, dict(qpos=[0.0] * 4), "get_state_device: qpos must be a device tensor (data_ptr()) or a raw device pointer (int), not list"),
    (_set, dict(mask=True), "set_state_device: mask must be a device tensor (data_ptr()) or a raw device pointer (int), not bool"),
    (_restart, dict(mask=np.ones(N, dtype=bool)), "restart_device: mask must be a device tensor (data_ptr()) or a raw device pointer (int), not ndarray"),
])
def test_checkers_refuse_with_the_projects_wording(call, kw, answer):
    with pytest.raises(ValueError) as err:
        call(**kw)
    assert str(err.value) == answer


@pytest.fixture(scope="module")
def state_io(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("state_io") / "state_io")
    subprocess.check_call(SANITIZE + ["-o", exe, os.path.join(ROOT, "tests", "state_io_main.cpp")])

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        return r.stdout.splitlines()

    return run


def test_gather_scatter_and_restart_on_the_host_under_sanitizers(state_io):
    """tests/state_io_main.cpp: the header's host/device functions over arrays of N = 37 and N = 1 against naive loops — the gather with
    every subset of outputs it is written for, the scatter and the restart under no mask byte set, all set, a NULL mask and a sparse
    one, with and without activations, goal, a variant pool (own draw / the row's block), the compiler's flag and the joint-parameter
    redraw. A stand-alone program with its own main: nothing sanitised is loaded into this interpreter."""
    assert state_io("walk")[-1] == "state io: ok"


def test_rows_the_header_draws_are_the_host_models(state_io):
    """(seed, global id, episode count before the restart, table rows): the row lm_state_io.h's restart_row draws equals
    step_bookkeeping_model.restart_row — a global id beyond 2^32, a negative one (an offset below zero), and an episode count whose
    increment wraps at 32 bits among them."""
    cases = [(5, 1000 + e, c, 257) for e in (0, 1, 36) for c in (0, 1, 2)]
    cases += [(5, (1 << 32) + 7, 3, 257), (5, (1 << 40) + 123456789, 0, 5), (2 ** 64 - 1, (1 << 33), 9, 1000003),
              (5, 12, 0xFFFFFFFF, 257), (0x123456789ABCDEF, (1 << 35) + 1, 0xFFFFFFFF, 5), (5, -3, 4, 257), (0, 0, 0, 1)]
    args = [x for c in cases for x in c]
    got = [int(ln.split()[1]) for ln in state_io("rows", *args)]
    want = [int(M.restart_row(seed, gid, (count + 1) & 0xFFFFFFFF, rows)) for seed, gid, count, rows in cases]
    assert got == want
    assert len(set(got[:9])) >= 5                                               # not vacuous: the draws differ
    assert int(M.restart_row(5, 12, 0, 257)) == got[cases.index((5, 12, 0xFFFFFFFF, 257))]      # the wrapped count is episode 0's key


@pytest.mark.parametrize("task", ["UnitreeA1.simple", "Atlas.walk"])
def test_observation_maps_of_the_parser_are_the_tasks(task, tmp_path):
    """csrc/lm_model_parse.h's qobs / vobs for the task's chain-model blob: dof d sits at the column the task's qpos_obs_idx / qvel_obs_idx
    lists put it (positions first, velocities behind them), -1 for a dof no column shows — the root's horizontal position among them."""
    exe = str(tmp_path / "obs_maps")
    subprocess.check_call(SANITIZE + ["-o", exe, os.path.join(ROOT, "tests", "obs_maps_main.cpp")])
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    blob = str(tmp_path / (task + ".bin"))
    np.ascontiguousarray(env._chain_model(), dtype=np.float64).tofile(blob)
    r = subprocess.run([exe, blob], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "obs maps: ok"
    got = {ln.split()[1]: [int(x) for x in ln.split()[2:]] for ln in lines[:-1]}
    t = env._device_task()
    qi, vi = list(t["qpos_obs_idx"]), list(t["qvel_obs_idx"])
    nv = env._model.nv
    want_q = [qi.index(d) if d in qi else -1 for d in range(nv)]
    want_v = [len(qi) + vi.index(d) if d in vi else -1 for d in range(nv)]
    assert got["qobs"] == want_q and got["vobs"] == want_v
    assert want_q[0] == -1 and want_q[1] == -1 and -1 not in want_v              # root x / y: in no observation column
