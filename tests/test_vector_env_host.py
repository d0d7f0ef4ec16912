"""
The vector environment, the host side (no GPU): liblocovec.so builds for gfx950, loads and exports exactly what include/locovec.h
declares; every refusal of the C-ABI (they come before the first HIP call) and of vector.check_finish_args gives its reason; the numpy
model of tests/vector_finish_model.py agrees with a naive loop over environments; the column mapping of environments whose reference
order is not the kernel's; construction refusals and make_vec without gymnasium. Device tensors are stood in for by the description
object of tests/test_policy_rollout_host.py.
"""

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vector_finish_model as M
from loco_mujoco_amd import LocoEnv, LocoVectorEnv, vector
from loco_mujoco_amd.backend import BackendError
from loco_mujoco_amd.vector import VEC_EXPORTS, check_finish_args
from test_policy_rollout_host import Dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loco_mujoco_amd", "csrc")
LIB = os.path.join(CSRC, "liblocovec.so")
N, NOBS = 5, 37


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", CSRC, "liblocovec.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return vector.load_vec_library()


def test_library_builds_and_exports_what_the_header_declares(lib):
    header = open(os.path.join(ROOT, "include", "locovec.h")).read()
    declared = set(re.findall(r"\b(lv_[a-z_]+)\s*\(", header))
    assert declared == set(VEC_EXPORTS) == {"lv_last_error", "lv_finish_step"} and len(VEC_EXPORTS) == 2
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lv_[a-z_0-9]+)$", syms, flags=re.M))
    assert exported == declared, sorted(exported ^ declared)
    assert not re.findall(r" T (l[mt]_[a-z_0-9]+)$", syms, flags=re.M)          # a library of its own: no lm_ / lt_ name
    for name in VEC_EXPORTS:
        fn = getattr(lib, name)
        restype, argtypes = vector._PROTOTYPES[name]
        assert fn.restype is restype
        if argtypes is None:
            assert name == "lv_last_error"                       # the one export without arguments
        else:
            assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes) == 15
    assert vector.VEC_LIB_PATH == LIB


def test_the_library_is_built_with_plain_ieee_arithmetic():
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    rule = re.search(r"^liblocovec\.so:.*\n\t(.*)$", makefile, flags=re.M).group(1)
    for flag in ("--offload-arch=$(ARCH)", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared"):
        assert flag in rule.split(), (flag, rule)
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in rule and "-fgpu-flush-denormals-to-zero" not in rule
    assert "-ffast-math" not in rule and "-ffp-contract=fast" not in rule
    assert "liblocovec.so" in re.search(r"^clean:\n\t(.*)$", makefile, flags=re.M).group(1)


def test_a_missing_library_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setattr(vector, "_lib", None)
    monkeypatch.setattr(vector, "VEC_LIB_PATH", str(tmp_path / "liblocovec.so"))
    with pytest.raises(BackendError, match="vector library not built.*no torch fallback"):
        vector.load_vec_library()


P = 0x1000          # stands for a device pointer: a refused call reads none of them
Q = 0x2000


def _finish(lib, n_envs=37, nobs=NOBS, obs=P, reward=P, done=P, term=None, terminated=P, truncated=P, final_obs=None, run_return=None,
            run_length=None, ep_return=None, ep_length=None):
    return lib.lv_finish_step(n_envs, nobs, obs, reward, done, term, terminated, truncated, final_obs, run_return, run_length, ep_return,
                              ep_length, None, 1)


@pytest.mark.parametrize("kw,word", [
    (dict(n_envs=0), "n_envs must be >= 1"), (dict(n_envs=-37), "n_envs must be >= 1"),
    (dict(nobs=0), "nobs must be >= 1"), (dict(nobs=-1), "nobs must be >= 1"),
    (dict(obs=None), "d_obs is null"), (dict(reward=None), "d_reward is null"), (dict(done=None), "d_done is null"),
    (dict(terminated=None), "d_terminated is null"), (dict(truncated=None), "d_truncated is null"),
    (dict(run_return=P), "d_run_return and d_run_length are given together"),
    (dict(run_length=P), "d_run_return and d_run_length are given together"),
    (dict(ep_return=P), "d_ep_return needs the accumulators"), (dict(ep_length=P), "d_ep_length needs the accumulators"),
    (dict(ep_return=P, run_length=P), "d_run_return and d_run_length are given together"),
    (dict(final_obs=P), "d_final_obs must not be d_obs"), (dict(final_obs=Q, term=Q), "d_final_obs must not be d_term"),
])
def test_c_refusals_name_the_call_and_the_argument(lib, kw, word):
    assert _finish(lib, **kw) != 0
    assert re.search("lv_finish_step: " + word, lib.lv_last_error().decode()), lib.lv_last_error()


def _args(**kw):
    u8 = "torch.uint8"
    a = dict(obs=Dev((N, NOBS)), reward=Dev((N,)), done=Dev((N,), u8), terminated=Dev((N,), u8), truncated=Dev((N,), u8))
    a.update(kw)
    return a


def test_a_valid_call_passes():
    assert check_finish_args(N, NOBS, **_args()) == (N, NOBS)
    assert check_finish_args(N, NOBS, **_args(term=Dev((N, NOBS)), final_obs=Dev((N, NOBS)), run_return=Dev((N,)),
                                              run_length=Dev((N,), "torch.int32"), ep_return=Dev((N,)),
                                              ep_length=Dev((N,), "torch.int32"))) == (N, NOBS)
    assert check_finish_args(np.int64(N), NOBS, P, P, P, P, P, final_obs=Q) == (N, NOBS)           # raw pointers are taken as given
    assert check_finish_args(N, NOBS, **_args(obs=P, run_return=P, run_length=Dev((N,), "torch.int32"))) == (N, NOBS)


FIN = Dev((N, NOBS))


@pytest.mark.parametrize("kw,reason", [
    (dict(obs=None), "obs is None"), (dict(reward=None), "reward is None"), (dict(done=None), "done is None"),
    (dict(terminated=None), "terminated is None"), (dict(truncated=None), "truncated is None"),
    (dict(obs=torch.zeros(N, NOBS)), "obs must live on the device"),                   # a host tensor
    (dict(obs=np.zeros((N, NOBS), dtype=np.float32)), "device tensor"),
    (dict(obs=Dev((N, NOBS), "torch.float64")), "obs must be float32"),
    (dict(obs=Dev((N, NOBS + 1))), r"obs must be \[%d, %d\]" % (N, NOBS)),
    (dict(obs=Dev((N, NOBS), contiguous=False)), "obs must be contiguous"),
    (dict(reward=Dev((N, 1))), r"reward must be \[%d\]" % N),
    (dict(done=Dev((N,))), "done must be uint8"), (dict(done=Dev((N,), "torch.bool")), "done must be uint8"),
    (dict(terminated=Dev((N,), "torch.bool")), "terminated must be uint8"),
    (dict(truncated=Dev((N + 1,), "torch.uint8")), r"truncated must be \[%d\]" % N),
    (dict(term=Dev((N, NOBS), cuda=False)), "term must live on the device"),
    (dict(final_obs=Dev((NOBS, N))), r"final_obs must be \[%d, %d\]" % (N, NOBS)),
    (dict(run_return=Dev((N,))), "run_return and run_length are given together"),
    (dict(run_length=Dev((N,), "torch.int32")), "run_return and run_length are given together"),
    (dict(ep_return=Dev((N,))), "ep_return needs the accumulators"),
    (dict(ep_length=Dev((N,), "torch.int32")), "ep_length needs the accumulators"),
    (dict(run_return=Dev((N,)), run_length=Dev((N,))), "run_length must be int32"),
    (dict(run_return=Dev((N,)), run_length=Dev((N,), "torch.int32"), ep_length=Dev((N,), "torch.int64")), "ep_length must be int32"),
    (dict(final_obs=FIN, obs=FIN), "final_obs must not be obs"), (dict(final_obs=FIN, term=FIN), "final_obs must not be term"),
    (dict(obs=Q, final_obs=Q), "final_obs must not be obs"),
])
def test_refusals_give_their_reason(kw, reason):
    with pytest.raises(ValueError, match="finish_step: .*" + reason):
        check_finish_args(N, NOBS, **_args(**kw))


@pytest.mark.parametrize("n,nobs,word", [(0, NOBS, "n_envs"), (True, NOBS, "n_envs"), (N, 0, "nobs"), (N, 2.0, "nobs")])
def test_sizes_are_integers_of_at_least_one(n, nobs, word):
    with pytest.raises(ValueError, match="finish_step: %s must be an integer >= 1" % word):
        check_finish_args(n, nobs, **_args())


@pytest.mark.parametrize("n,nobs", [(1, 1), (7, 3), (257, 37)])
def test_the_model_agrees_with_the_naive_loop(n, nobs):
    """Three calls in a row, the accumulators carried; with and without the terminal buffer, final_obs and the accumulators. A NaN
    reward in the second call ends with its episode: the environment's return is NaN where that episode ends, and finite afterwards."""
    nan_env = min(2, n - 1)
    for with_term in (True, False):
        run_r, run_l = np.zeros(n, np.float32), np.zeros(n, np.int32)
        nan_r, nan_l = run_r.copy(), run_l.copy()
        fin = np.full((n, nobs), M.SENTINEL, np.float32)
        nan_seen = False
        for call in range(1, 7):
            obs, rew, done, term = M.synthetic_step(n, nobs, seed=call, nan_at=nan_env if call == 2 else None)
            kw = dict(term=term if with_term else None, final_obs=fin, run_return=run_r, run_length=run_l)
            m, ref = M.finish(obs, rew, done, **kw), M.naive_finish(obs, rew, done, **kw)
            for key in ref:
                assert m[key].dtype == ref[key].dtype and np.array_equal(m[key], ref[key], equal_nan=True), (call, key)
            ended = done != 0
            assert np.array_equal(m["terminated"] | m["truncated"], ended.astype(np.uint8)) and not (m["terminated"] & m["truncated"]).any()
            assert (m["ep_length"][~ended] == 0).all() and (m["ep_return"][~ended] == 0).all() and (m["ep_length"][ended] >= 1).all()
            assert (m["run_length"][ended] == 0).all() and (m["run_return"][ended] == 0).all()
            assert np.array_equal(m["final_obs"][~ended], fin[~ended])                    # rows that did not end: untouched
            src = np.where((((done & 2) != 0) & with_term)[:, None], term, obs)
            assert np.array_equal(m["final_obs"][ended], src[ended])
            if call >= 2 and not nan_seen:
                # the NaN stays in the running return until the episode ends, is reported there, and is gone afterwards
                if ended[nan_env]:
                    assert np.isnan(m["ep_return"][nan_env]) and m["run_return"][nan_env] == 0
                    nan_seen = True
                else:
                    assert np.isnan(m["run_return"][nan_env])
            elif nan_seen:
                assert np.isfinite(m["run_return"][nan_env]) and np.isfinite(m["ep_return"][nan_env])
            run_r, run_l, fin = m["run_return"], m["run_length"], m["final_obs"]
        assert nan_seen
    # without accumulators / final_obs nothing of them is returned; without want_ep the accumulators still run
    obs, rew, done, term = M.synthetic_step(n, nobs, seed=3)
    bare = M.finish(obs, rew, done)
    assert all(bare[k] is None for k in ("final_obs", "run_return", "run_length", "ep_return", "ep_length"))
    quiet = M.finish(obs, rew, done, run_return=np.ones(n, np.float32), run_length=np.ones(n, np.int32), want_ep=False)
    assert quiet["ep_return"] is None and quiet["ep_length"] is None
    assert np.array_equal(quiet["run_length"], np.where(done != 0, 0, 2))


def test_the_models_done_bytes_cover_every_value():
    for n in M.N_CASES:
        seen = set()
        for seed in (1, 2, 3):
            seen |= set(M.synthetic_step(n, 1, seed=seed)[2].tolist())
        assert seen == ({0, 1, 2, 3} if n > 1 else {1, 2, 3})


def test_the_column_mapping_is_the_environments():
    """Atlas carrying a weight with foot forces: the kernel's observation is [q, v, weight, foot forces], the reference's
    [q, v, foot forces, weight]. The index_select that step() applies is LocoEnv.step's `obs[:, perm]`."""
    env = LocoEnv.make("Atlas.carry", debug=True, use_foot_forces=True)
    perm = env._obs_perm()
    nobs, g = env.info.observation_space.shape[0], env._get_grf_size()
    assert perm is not None and sorted(perm.tolist()) == list(range(nobs)) and g > 0
    x = np.arange(3 * nobs, dtype=np.float32).reshape(3, nobs)
    want = M.column_map(x, perm)
    assert np.array_equal(want[0], np.concatenate([np.arange(nobs - g - 1), np.arange(nobs - g, nobs), [nobs - g - 1]]))
    assert np.array_equal(x[:, perm], want) and M.column_map(x, None) is x                 # (LocoEnv.step's own expression)
    out = torch.empty(3, nobs)
    torch.index_select(torch.from_numpy(x), 1, torch.as_tensor(np.asarray(perm), dtype=torch.int64), out=out)
    assert np.array_equal(out.numpy(), want)
    assert LocoEnv.make("UnitreeA1.simple", debug=True)._obs_perm() is None


def test_construction_refusals_give_their_reason():
    """Before anything touches a device: these run on a machine without one."""
    with pytest.raises(NotImplementedError, match="LocoVectorEnv: the reward is evaluated on the host"):
        LocoVectorEnv("UnitreeA1.simple", 4, debug=True, use_foot_forces=True)
    with pytest.raises(NotImplementedError, match="LocoVectorEnv: several models in one batch"):
        LocoVectorEnv("HumanoidTorque4Ages.walk.all", 8, debug=True)
    for bad in (0, -3, 2.0, True):
        with pytest.raises(ValueError, match="LocoVectorEnv: num_envs must be an integer >= 1"):
            LocoVectorEnv("UnitreeA1.simple", bad, debug=True)


def test_make_vec_without_gymnasium(monkeypatch):
    from loco_mujoco_amd.environments import gymnasium as G
    seen = {}

    class Recorder:
        def __init__(self, env_name, num_envs, **kw):
            seen.update(env_name=env_name, num_envs=num_envs, **kw)

    monkeypatch.setattr(vector, "LocoVectorEnv", Recorder)
    v = G.make_vec("LocoMujoco", env_name="UnitreeA1.simple", num_envs=7, seed=3, debug=True)
    assert isinstance(v, Recorder) and seen == dict(env_name="UnitreeA1.simple", num_envs=7, seed=3, debug=True)
    with pytest.raises(AssertionError):
        G.make_vec("CartPole-v1", env_name="UnitreeA1.simple")
    monkeypatch.undo()
    # the real class: its refusals come through make_vec, and the metadata names the autoreset mode
    with pytest.raises(ValueError, match="num_envs must be an integer >= 1"):
        G.make_vec("LocoMujoco", env_name="UnitreeA1.simple", num_envs=0)
    if G._gym is None:
        assert LocoVectorEnv.metadata["autoreset_mode"] == "SameStep"
    else:
        assert LocoVectorEnv.metadata["autoreset_mode"] == G._gym.vector.AutoresetMode.SAME_STEP
    assert vector.LocoVectorEnv is LocoVectorEnv
