"""
Episode returns and lengths from the tapes, the host side (no GPU): liblocotape.so builds for gfx950, loads and exports exactly what
include/locotape.h declares; every refusal of the C-ABI (they come before the first HIP call) and of tapes.check_episode_args gives its
reason; the float64 model of tests/episode_tape_model.py agrees with a second, naive computation. Device tensors are stood in for by
the description object of tests/test_policy_rollout_host.py.
"""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import episode_tape_model as M
from loco_mujoco_amd import tapes
from loco_mujoco_amd.tapes import TAPE_EXPORTS, check_episode_args
from test_policy_rollout_host import N, T, Dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "loco_mujoco_amd", "csrc")
LIB = os.path.join(CSRC, "liblocotape.so")


@pytest.fixture(scope="module")
def lib():
    subprocess.check_call(["make", "-C", CSRC, "liblocotape.so"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return tapes.load_tape_library()


def test_library_builds_and_exports_what_the_header_declares(lib):
    header = open(os.path.join(ROOT, "include", "locotape.h")).read()
    declared = set(re.findall(r"\b(lt_[a-z_]+)\s*\(", header))
    assert declared == set(TAPE_EXPORTS) and len(TAPE_EXPORTS) == 4
    syms = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lt_[a-z_0-9]+)$", syms, flags=re.M))
    assert exported == declared, sorted(exported ^ declared)
    for name in TAPE_EXPORTS:
        fn = getattr(lib, name)
        restype, argtypes = tapes._PROTOTYPES[name]
        assert fn.restype is restype
        if argtypes is None:
            assert name == "lt_last_error"                       # the one export without arguments
        else:
            assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes) > 0
    assert "#define LT_CARRY_ROWS %d\n" % tapes.CARRY_ROWS in header and "#define LT_SUMMARY_FIELDS %d\n" % tapes.SUMMARY_FIELDS in header
    assert tuple(M.SUMMARY) == tuple(tapes.SUMMARY_LAYOUT) and len(M.SUMMARY) == tapes.SUMMARY_FIELDS


def test_the_library_is_built_with_plain_ieee_arithmetic():
    rule = re.search(r"^liblocotape\.so:.*\n\t(.*)$", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M).group(1)
    for flag in ("--offload-arch=$(ARCH)", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off"):
        assert flag in rule.split(), (flag, rule)
    assert "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in rule and "-fgpu-flush-denormals-to-zero" not in rule


def test_work_size_is_host_arithmetic(lib):
    assert [lib.lt_episode_work_doubles(n) for n in (-3, 0, 1, 256, 257, 300, 4096)] == [0, 0, 10, 10, 20, 20, 160]


P = 0x1000          # stands for a device pointer: a refused call reads none of them


def _episodes(lib, n_steps=7, n_envs=37, reward=P, done=P, mask=None, gamma=0.99, carry=P, length=P, summary=None, work=None):
    return lib.lt_tape_episodes(n_steps, n_envs, reward, done, mask, gamma, carry, length, None, None, None, None, summary, 1, work, None, 1)


@pytest.mark.parametrize("kw,word", [
    (dict(reward=None), "d_reward is null"), (dict(done=None), "d_done is null"), (dict(carry=None), "d_carry is null"),
    (dict(length=None), "d_len is null"), (dict(n_steps=0), "n_steps must be >= 1"), (dict(n_steps=-2), "n_steps must be >= 1"),
    (dict(n_envs=0), "n_envs must be >= 1"), (dict(n_envs=-37), "n_envs must be >= 1"),
    (dict(gamma=1.5), r"gamma must be in \[0, 1\]"), (dict(gamma=-0.1), r"gamma must be in \[0, 1\]"),
    (dict(gamma=float("nan")), r"gamma must be in \[0, 1\]"), (dict(gamma=float("inf")), r"gamma must be in \[0, 1\]"),
    (dict(summary=P), "d_summary needs d_work"),
])
def test_c_refusals_name_the_call_and_the_argument(lib, kw, word):
    assert _episodes(lib, **kw) != 0
    assert re.search("lt_tape_episodes: " + word, lib.lt_last_error().decode()), lib.lt_last_error()


@pytest.mark.parametrize("args,word", [((0, P, P), "n_envs must be >= 1"), ((37, None, P), "d_carry is null"), ((37, P, None), "d_len is null")])
def test_c_refusals_of_the_carry_reset(lib, args, word):
    assert lib.lt_episode_carry_reset(args[0], args[1], args[2], None, None, 1) != 0
    assert re.search("lt_episode_carry_reset: " + word, lib.lt_last_error().decode()), lib.lt_last_error()


def _args(**kw):
    a = dict(reward=Dev((T, N)), done=Dev((T, N), "torch.uint8"))
    a.update(kw)
    return a


def test_a_valid_call_passes():
    assert check_episode_args(N, **_args()) == (T, 0.99)
    assert check_episode_args(N, **_args(gamma=1, mask=Dev((N,), "torch.uint8"), ep_return=Dev((T, N)), ep_disc_return=Dev((T, N)),
                                         ep_length=Dev((T, N), "torch.int32"), trace=Dev((T, N)))) == (T, 1.0)
    assert check_episode_args(N, 0x1000, 0x2000, gamma=np.float32(0.5), n_steps=3) == (3, 0.5)          # raw pointers are taken as given
    assert check_episode_args(N, **_args(reward=0x1000)) == (T, 0.99)


@pytest.mark.parametrize("kw,reason", [
    (dict(reward=None), "reward is None"),
    (dict(done=None), "done is None"),
    (dict(reward=torch.zeros(T, N)), "reward must live on the device"),                # a host tensor
    (dict(reward=np.zeros((T, N), dtype=np.float32)), "device tensor"),
    (dict(reward=Dev((T, N), "torch.float64")), "reward must be float32"),
    (dict(reward=Dev((T, N + 1))), r"reward must be \[%d, %d\]" % (T, N)),
    (dict(reward=Dev((T * N,))), r"reward must be \[%d, %d\]" % (T, N)),
    (dict(reward=Dev((T, N), contiguous=False)), "reward must be contiguous"),
    (dict(done=Dev((T, N))), "done must be uint8"),
    (dict(done=Dev((T, N), "torch.bool")), "done must be uint8"),
    (dict(done=Dev((T + 1, N), "torch.uint8")), "the done tape holds %d steps, the others T = %d" % (T + 1, T)),
    (dict(n_steps=T - 1), "the reward tape holds %d steps, the others T = %d" % (T, T - 1)),
    (dict(mask=Dev((N,))), "mask must be uint8"),
    (dict(mask=Dev((N + 1,), "torch.uint8")), r"mask must be \[%d\]" % N),
    (dict(mask=Dev((N,), "torch.uint8", cuda=False)), "mask must live on the device"),
    (dict(ep_length=Dev((T, N))), "ep_length must be int32"),
    (dict(trace=Dev((T, N), "torch.float16")), "trace must be float32"),
    (dict(ep_return=Dev((N, T))), "the ep_return tape holds %d steps" % N),
    (dict(gamma=-0.01), r"gamma must be in \[0, 1\]"),
    (dict(gamma=1.01), r"gamma must be in \[0, 1\]"),
    (dict(gamma=float("nan")), r"gamma must be in \[0, 1\]"),
    (dict(gamma="0.9"), "gamma must be a number"),
    (dict(gamma=True), "gamma must be a number"),
])
def test_refusals_give_their_reason(kw, reason):
    with pytest.raises(ValueError, match="episodes: .*" + reason):
        check_episode_args(N, **_args(**kw))


def test_raw_pointers_need_the_number_of_steps():
    with pytest.raises(ValueError, match="episodes: raw pointers need n_steps"):
        check_episode_args(N, 0x1000, 0x2000)
    with pytest.raises(ValueError, match="episodes: T must be >= 1"):
        check_episode_args(N, 0x1000, 0x2000, n_steps=0)
    with pytest.raises(ValueError, match="episodes: n_envs must be an integer >= 1"):
        check_episode_args(0, 0x1000, 0x2000, n_steps=3)


@pytest.mark.parametrize("gamma", [0.0, 0.99, 1.0])
def test_the_model_agrees_with_the_naive_computation(gamma):
    """Two float64 computations of the same values: they differ by float64 roundings, far inside the float32 bound the model returns."""
    r, d = M.synthetic_tapes(37)
    m = M.episodes64(r, d, gamma)
    ret, disc, length, trace = M.naive_episodes(r, d, gamma)
    ended = d != 0
    assert np.array_equal(m["length"], length) and np.array_equal(length >= 0, ended)
    assert (length[:, M.NO_END] == -1).all() and (length[:, M.EVERY_STEP] == 1).all() and m["carry_length"][M.NO_END] == M.T
    assert ended[0].any() and ended[M.T - 1].any()
    assert np.array_equal(np.isnan(m["ret"]), ~ended) and np.array_equal(np.isnan(ret), ~ended)
    for got, ref, bound in ((m["ret"], ret, m["b_ret"]), (m["disc"], disc, m["b_disc"])):
        assert (np.abs(got - ref)[ended] <= bound[ended]).all()
        assert (bound[ended] <= 2 * M.T * M.U * np.abs(r).sum(0).max()).all()        # (the bound is a rounding bound, not a loose one)
    assert (np.abs(m["trace"] - trace) <= m["b_trace"]).all()
    # an unfinished episode is not counted: it is the carry. Split anywhere, the model continues it to the same values
    for k in (1, 3):
        a = M.episodes64(r[:k], d[:k], gamma)
        b = M.episodes64(r[k:], d[k:], gamma, carry=a["carry"], length=a["carry_length"])
        for key in ("ret", "disc", "length", "trace"):
            assert np.array_equal(np.concatenate([a[key], b[key]]), m[key], equal_nan=True), key
        assert np.array_equal(b["carry"], m["carry"]) and np.array_equal(b["carry_length"], m["carry_length"])


def test_the_summary_of_returned_values():
    r, d = M.synthetic_tapes(37)
    m = M.episodes64(r, d, 0.99)
    values, bounds = M.summary_of(m["ret"].astype(np.float32), m["disc"].astype(np.float32), m["length"], d)
    assert values["episodes"] == (d != 0).sum() and values["absorbing"] == ((d & 1) != 0).sum() and values["L_min"] == 1
    assert values["L_sum"] == m["length"][d != 0].sum() and all(bounds[f] == 0 for f in M.EXACT)
    mask = np.zeros(37, dtype=np.uint8)
    assert M.summary_of(m["ret"], m["disc"], m["length"], d, mask=mask)[0] == dict(zip(M.SUMMARY, tapes._EMPTY_SUMMARY))
