"""
Input normalisation of the in-kernel policy (include/locohip.h lm_set_policy_obs_norm, HipBatch.set_policy_obs_norm; `-m gpu`): the MLP of
lm_rollout_policy reads clamp((obs - mean) * inv_std, -clip, clip), the tensors in place. Batches, policies, shapes and the comparisons
are those of tests/test_policy_rollout_gpu.py (imported): n in {1, 5, 37}, T = 7, launches of 1, 3 (3 + 3 + 1) and 7 control steps.
Cases: the quadruped (fused path, tanh 40/24), Atlas (relu 256) and the generic family (one step per launch: policy_kernel).
"""

import functools
import os
import types

import numpy as np
import pytest

import test_policy_rollout_gpu as pr
import test_rollout_tape_gpu as tp
from test_rollout_tape_gpu import OBS_FILL, T, _same

pytestmark = pytest.mark.gpu

CASES = {k: pr.CASES[k] for k in ("a1", "atlas", "generic")}
SPLS = pr.SPLS
INV_STD, CLIP = 4.0, 1.0          # angles beyond 0.25 rad are clamped, the small ones are not


def _tensors(b, mean=0.0, inv_std=INV_STD):
    torch, dev = pr._torch()
    return (torch.full((b.nobs,), float(mean), dtype=torch.float32, device=dev),
            torch.full((b.nobs,), float(inv_std), dtype=torch.float32, device=dev))


def _start(make, mean=0.0, inv_std=INV_STD, clip=CLIP):
    """tests/test_policy_rollout_gpu.py's start, the normaliser set: (batch, obs0, (mean, inv_std))."""
    b, obs0 = pr._start(make)
    ts = _tensors(b, mean, inv_std)
    b.set_policy_obs_norm(ts[0], ts[1], clip)
    return b, obs0, ts


def _expression(prev, mean, inv_std, clip):
    """The stated expression in numpy float32, operation by operation."""
    t = (prev.astype(np.float32) - np.float32(mean)) * np.float32(inv_std)
    assert t.dtype == np.float32
    if clip > 0:
        c = np.float32(clip)
        t = np.where(t < -c, -c, np.where(t > c, c, t))
    return t


def _inputs(out, obs0):
    return np.concatenate([obs0[None], out["obs"][:-1]])          # [T, n, nobs]: what each step's action was computed from


def _check_actions_are_the_mlps_of(policy, out, x, label):
    """tests/test_policy_rollout_gpu.py's float64 evaluation and running bound, with x [T, n, nobs] in place of the raw rows."""
    shifted = dict(out, obs=np.concatenate([x[1:], x[-1:]]))
    return pr._check_actions_are_the_mlps(policy, shifted, x[0], label)


@functools.lru_cache(maxsize=None)
def _unset(case, spl=3, log_std=None):
    """The rollout with the setting off, computed once per case and shared (read-only)."""
    task, n, widths, act = CASES[case]
    b, obs0 = pr._start(lambda: pr._batch(task, n))
    return pr._run(b, pr._policy(b, widths, act, log_std), spl, obs0, noise_seed=9)


def _same_rollout(out, ref, what):
    for k in ("actions", "obs", "reward", "done"):
        _same(out[k], ref[k], "%s: %s tape" % (what, k))
    _same(out["state"][0], ref["state"][0], what + ": final qpos")
    _same(out["state"][1], ref["state"][1], what + ": final qvel")


# ---- 1. the identity is bitwise the rollout without the setting, and so is the setting taken back
@pytest.mark.parametrize("case", list(CASES))
def test_identity_and_off_again_are_bitwise_the_unset_rollout(case):
    task, n, widths, act = CASES[case]
    ref = _unset(case)
    make = lambda: pr._batch(task, n)
    b, obs0, _ = _start(make, 0.0, 1.0, 0.0)
    _same_rollout(pr._run(b, pr._policy(b, widths, act), 3, obs0, noise_seed=9), ref, "mean 0, inv_std 1, no clip")
    b, obs0, _ = _start(make)
    b.set_policy_obs_norm(None, None)
    _same_rollout(pr._run(b, pr._policy(b, widths, act), 3, obs0, noise_seed=9), ref, "set and taken back")
    # (and the setting DOES something: the shared run below differs from the unset one)
    assert not np.array_equal(_normalised(case, 3)["actions"], ref["actions"])


@functools.lru_cache(maxsize=None)
def _normalised(case, spl, log_std=None):
    task, n, widths, act = CASES[case]
    b, obs0, _ = _start(lambda: pr._batch(task, n))
    out = pr._run(b, pr._policy(b, widths, act, log_std), spl, obs0, noise_seed=9)
    out["obs0"] = obs0.cpu().numpy()
    return out


# ---- 2. the actions are the MLP's on the normalised inputs
@pytest.mark.parametrize("spl", [1, T])
@pytest.mark.parametrize("case", list(CASES))
def test_actions_are_the_mlps_on_normalised_inputs(case, spl):
    task, n, widths, act = CASES[case]
    out = _normalised(case, spl)
    prev = _inputs(out, out["obs0"])
    assert np.isfinite(prev).all()
    scaled = np.abs(prev * np.float32(INV_STD))
    assert (scaled > CLIP).any() and (scaled < CLIP).any()              # at least one input was clamped, at least one was not
    print("%s: %.1f %% of the inputs clamped" % (case, 100.0 * (scaled > CLIP).mean()))
    x = _expression(prev, 0.0, INV_STD, CLIP)
    assert np.abs(x).max() == CLIP
    dims = types.SimpleNamespace(nobs=out["obs"].shape[-1], nu=out["actions"].shape[-1])
    _check_actions_are_the_mlps_of(pr._policy(dims, widths, act), out, x, "%s, %d per launch, normalised" % (case, spl))
    assert out["actions"].std(axis=(0, 1)).min() > 1e-4


def test_a_mean_and_no_clip():
    """mean != 0 and clip 0 (no clamp): the subtraction is there, the selects are not."""
    task, n, widths, act = CASES["a1"]
    b, obs0, _ = _start(lambda: pr._batch(task, n), 0.3, 2.5, 0.0)
    policy = pr._policy(b, widths, act)
    out = pr._run(b, policy, 3, obs0)
    x = _expression(_inputs(out, obs0.cpu().numpy()), 0.3, 2.5, 0.0)
    assert np.abs(x).max() > 2.5
    _check_actions_are_the_mlps_of(policy, out, x, "a1, mean 0.3, inv_std 2.5, no clip")


# ---- 3. the launch split and the batch do not matter
@pytest.mark.parametrize("log_std", [None, -1.0])
@pytest.mark.parametrize("case", ["a1", "atlas"])
def test_launch_split_and_batch_size_do_not_change_an_action(case, log_std):
    task, n, widths, act = CASES[case]
    env, _, tab = tp._task(task)
    tapes = [_normalised(case, spl, log_std) for spl in SPLS]
    for other in tapes[1:]:
        _same(other["actions"], tapes[0]["actions"], "action tape")
        _same(other["obs"], tapes[0]["obs"], "observation tape")
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)]          # (the rows of pr._batch)
    e = 3
    for m, first, spl in ((1, e, 3), (5, 0, T)):
        def make():
            b = pr._batch(task, m, rows=rows[first:first + m])
            b.set_reset_table(tab[:4], seed=0, global_env_offset=first)          # (no auto-reset: the offset only)
            return b
        b, obs0, _ = _start(make)
        out = pr._run(b, pr._policy(b, widths, act, log_std), spl, obs0, noise_seed=9)
        _same(out["actions"][:, e - first], tapes[0]["actions"][:, e], "actions of environment %d in a batch of %d" % (e, m))


# ---- 4. replaying the recorded actions is bitwise the same rollout
@pytest.mark.parametrize("case", list(CASES))
def test_recorded_actions_replay_the_rollout_bitwise(case):
    task, n, widths, act = CASES[case]
    make = lambda: pr._batch(task, n)
    b, obs0, _ = _start(make)
    out = pr._run(b, pr._policy(b, widths, act), 3, obs0, noise_seed=9)
    _same(out["actions"], _normalised(case, 3)["actions"], "the shared run")
    assert out["stats"]["env_steps"] == T * n
    pr._replayed_by_tape(make, out, 3)


# ---- 5. the tensors are read in place
def test_tensors_are_read_in_place():
    torch, dev = pr._torch()
    task, n, widths, act = CASES["a1"]
    make = lambda: pr._batch(task, n)
    runs = {}
    for key in ("halved", "kept"):
        b, obs0, (mean, inv_std) = _start(make)
        policy = pr._policy(b, widths, act)
        first = pr._run(b, policy, 3, obs0, steps=3)
        if key == "halved":
            inv_std.mul_(0.5)                                     # in place: no further call
            torch.cuda.synchronize(dev)
        mid = torch.from_numpy(first["obs"][-1]).to(dev)
        runs[key] = (first, pr._run(b, policy, 3, mid, steps=4), mid)
    _same(runs["halved"][0]["actions"], runs["kept"][0]["actions"], "the first call")
    assert not np.array_equal(runs["halved"][1]["actions"][0], runs["kept"][1]["actions"][0])
    # a twin that was given the halved tensor from the start: the same action from the same observation
    b, _, _ = _start(make, 0.0, INV_STD * 0.5, CLIP)
    got = pr._run(b, pr._policy(b, widths, act), 1, runs["halved"][2], steps=1)
    _same(got["actions"][0], runs["halved"][1]["actions"][0], "the action under the halved tensor")


# ---- 6. refused calls change nothing and launch nothing
def test_refused_calls_change_nothing():
    import ctypes as C
    torch, dev = pr._torch()
    task, n, widths, act = CASES["a1"]
    b, obs0 = pr._start(lambda: pr._batch(task, n))
    mean, inv_std = _tensors(b)
    pm, pi = C.c_void_p(mean.data_ptr()), C.c_void_p(inv_std.data_ptr())
    for args, word in (((pm, None, 1.0), b"go together"), ((None, pi, 1.0), b"go together"), ((pm, pi, -1.0), b"clip"),
                       ((pm, pi, float("nan")), b"clip"), ((pm, pi, float("inf")), b"clip")):
        assert b._lib.lm_set_policy_obs_norm(b._h, *args) != 0
        assert word in b._lib.lm_last_error(), b._lib.lm_last_error()
    for kw, reason in ((dict(mean=mean, inv_std=None), "go together"), (dict(mean=mean, inv_std=inv_std, clip=-1.0), "clip"),
                       (dict(mean=mean, inv_std=inv_std, clip=float("nan")), "clip"),
                       (dict(mean=mean.cpu(), inv_std=inv_std, clip=1.0), "mean must live on the device"),
                       (dict(mean=mean, inv_std=inv_std[:-1], clip=1.0), "inv_std must be")):
        with pytest.raises(ValueError, match=reason):
            b.set_policy_obs_norm(**kw)
    assert b.stats()["env_steps"] == 0
    _same_rollout(pr._run(b, pr._policy(b, widths, act), 3, obs0, noise_seed=9), _unset("a1"), "after the refusals")


# ---- 7. under the replay kernel; restarts inside a launch and the terminal tape
def test_replay_kernel_under_a_normalised_policy():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ht_folded_states.npz"))
    task, n = "HumanoidTorque.run", 37
    env, _, tab = tp._task(task)
    nv = env._model.nv
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)].copy()
    k = min(len(d["q"]), n - 5)
    rows[:k, :nv], rows[:k, nv:2 * nv] = d["q"][:k], d["v"][:k]
    make = lambda: pr._batch(task, n, rows=rows, replay=2)
    b, obs0, _ = _start(make)
    policy = pr._policy(b, (40, 24), "tanh")
    out = pr._run(b, policy, 3, obs0)
    assert out["stats"]["replayed_env_steps"] == T * n
    pr._replayed_by_tape(make, out, 3)
    x = _expression(_inputs(out, obs0.cpu().numpy()), 0.0, INV_STD, CLIP)
    _check_actions_are_the_mlps_of(policy, out, x, "HumanoidTorque through the replay kernel, normalised")
    # (the regular fused kernel on the same observation: the same function of the same inputs)
    b2, _, _ = _start(lambda: pr._batch(task, n, rows=rows))
    _same(pr._run(b2, policy, 2, obs0, steps=2)["actions"][0], out["actions"][0], "step 0 under the regular kernel")


@pytest.mark.parametrize("spl", [3, T])
def test_restarts_inside_a_launch_and_raw_terminal_rows(spl):
    task, n, widths, act = CASES["a1"]
    table = pr._restart_table(task)
    make = lambda: pr._batch(task, n, restarts=(table, 3), terminal=True)
    b, obs0, _ = _start(make)
    policy = pr._policy(b, widths, act)
    out = pr._run(b, policy, spl, obs0, terminal=True)
    # the twin knows nothing of the normaliser: its observation and terminal tapes are raw, and bitwise these
    pr._replayed_by_tape(make, out, spl, terminal=True)
    ended = (out["done"] & 2) != 0
    assert ended.sum() >= n and (out["term"][~ended] == OBS_FILL).all() and not (out["term"][ended] == OBS_FILL).all(1).any()
    assert np.abs(out["term"][ended]).max() > CLIP and np.abs(out["obs"]).max() > CLIP
    x = _expression(_inputs(out, obs0.cpu().numpy()), 0.0, INV_STD, CLIP)
    _check_actions_are_the_mlps_of(policy, out, x, "restarts, %d per launch, normalised" % spl)
