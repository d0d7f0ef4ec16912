"""
The line search's slot loop in two (lm_families.h LM_LS_FLOOR_SPLIT, lm_core.h kLsFloorSplit: floor slots with an opaque weight of 1.0f,
self-contact slots with slot_weight as before) on the device: not a bit may move. No fixture of its own — what the libraries before
the split computed on an MI355X is the reference (tests/golden/a1_collapse_rollout_gpu.npz, test_newton_passes_gpu.py;
tests/golden/a1_newton_hard_states_gpu.npz, test_hessian_paths_gpu.py).

Case 1: the collapse roll-out (reset rows, zero action, 40 control steps) as ONE ragged batch of five, and as a batch of eight in which
environments 2 and 5 start from the two self-contact states of a1_newton_hard_states.npz (with their warm starts), so that floor-only
and pair-slot environments share a wave: per-step launches, the fused roll-out (8 x 5) and the replay pass. The rows that are in the
fixture must equal it (the replay pass its `replay_*` tapes: over this roll-out the replay kernel's numbers are its own); the
self-contact environments, which are not, must come out of the fused roll-out as they come out of the per-step launches.
Case 2: one control step from each state of a1_newton_hard_states.npz equals the recorded one — the self-contact states are the pair loop.
"""

import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROLLOUT = os.path.join(HERE, "golden", "a1_collapse_rollout_gpu.npz")
STATES = os.path.join(HERE, "golden", "a1_newton_hard_states.npz")
STATES_GPU = os.path.join(HERE, "golden", "a1_newton_hard_states_gpu.npz")
N, T = 8, 40
PAIR_ENVS = (2, 5)                  # of the batch of eight: the self-contact states
KEYS = ("obs", "reward", "done", "q", "v", "w")


def _rows(x, key, rows):
    return x[key][:, rows] if key in ("obs", "reward", "done") else x[key][rows]


def _rollout(hm, start, n, steps_per_launch=1, replay=None):
    """T control steps of the first n start states (qpos, qvel, warm) under zero action; tapes [T, n, ...], final state, warm start, counters."""
    import torch
    from loco_mujoco_amd.backend import HipBatch
    from test_hessian_paths_gpu import _load, _read_warm
    b = HipBatch(hm, n)
    if replay is not None:
        b.set_replay(replay)
    _load(b, start, list(range(n)))
    b.stats(reset=True)
    obs = torch.zeros((T, n, b.nobs), dtype=torch.float32, device="cuda")
    reward = torch.zeros((T, n), dtype=torch.float32, device="cuda")
    done = torch.zeros((T, n), dtype=torch.uint8, device="cuda")
    b.rollout_tape(torch.zeros((n, b.nu), dtype=torch.float32, device="cuda"), obs=obs, reward=reward, done=done,
                   steps_per_launch=steps_per_launch, repeat=T)
    q, v = b.get_state()
    w = _read_warm(b)
    st = b.stats()
    b.close()
    out = dict(obs=obs.cpu().numpy(), reward=reward.cpu().numpy(), done=done.cpu().numpy(), q=q, v=v, w=w)
    out.update({key: st[key] for key in ("solver_iters", "linesearch_evals", "replayed_env_steps", "nan_resets", "self_contacts")})
    return out


@pytest.fixture(scope="module")
def setup():
    from loco_mujoco_amd import LocoEnv
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True)
    hm = HipModel(env._chain_model())
    table = np.asarray(env._reset_table(), dtype=np.float64)
    E, S, G = np.load(ROLLOUT), np.load(STATES), np.load(STATES_GPU)
    nq, nv = hm.dims.nq, hm.dims.nv
    q0, v0 = table[:N, :nq].astype(np.float32), table[:N, nq:nq + nv].astype(np.float32)
    assert np.array_equal(q0, E["q0"]) and np.array_equal(v0, E["v0"])          # the reset table's rows are the recorded start
    names = [str(x) for x in S["names"]]
    assert names == [str(x) for x in G["names"]]
    pair_states = [i for i, name in enumerate(names) if name.startswith("self_contact")]
    assert len(pair_states) == len(PAIR_ENVS)
    floor = dict(qpos=q0.astype(np.float64), qvel=v0.astype(np.float64), warm=np.zeros((N, nv)))
    mixed = {key: val.copy() for key, val in floor.items()}
    for e, i in zip(PAIR_ENVS, pair_states):
        for key in mixed:
            mixed[key][e] = S[key][i]
    return hm, floor, mixed, E, S, G


@pytest.fixture(scope="module")
def per_step(setup):
    """The per-step launches of both batches, computed once."""
    hm, floor, mixed, _, _, _ = setup
    return _rollout(hm, floor, 5), _rollout(hm, mixed, N)


def _same_as_fixture(got, E, batch_rows, fixture_rows, prefix=""):
    for key in KEYS:
        a, want = _rows(got, key, batch_rows), _rows({k: E[prefix + k] for k in KEYS}, key, fixture_rows)
        assert a.shape == want.shape and np.array_equal(a, want), (prefix, key, np.abs(a.astype(np.float64) - want).max())


def _same_as_each_other(got, ref):
    for key in KEYS:
        assert got[key].shape == ref[key].shape and np.array_equal(got[key], ref[key]), (key, np.abs(got[key].astype(np.float64) - ref[key]).max())
    for key in ("solver_iters", "linesearch_evals"):
        assert got[key] == ref[key], (key, got[key], ref[key])


FLOOR_ENVS = [e for e in range(N) if e not in PAIR_ENVS]


def test_ragged_batch_of_five_per_step_launches(setup, per_step):
    _, _, _, E, _, _ = setup
    got = per_step[0]
    assert got["nan_resets"] == 0 and got["replayed_env_steps"] == 0
    assert got["linesearch_evals"] > got["solver_iters"] > 0
    _same_as_fixture(got, E, list(range(5)), list(range(5)))


def test_ragged_batch_of_five_fused(setup, per_step):
    hm, floor, _, E, _, _ = setup
    got = _rollout(hm, floor, 5, steps_per_launch=8)
    _same_as_each_other(got, per_step[0])
    _same_as_fixture(got, E, list(range(5)), list(range(5)))


def test_ragged_batch_of_five_replay_pass(setup):
    hm, floor, _, E, _, _ = setup
    got = _rollout(hm, floor, 5, replay=2)            # 2: every environment through the replay kernel
    assert got["replayed_env_steps"] == 5 * T and got["nan_resets"] == 0
    _same_as_fixture(got, E, list(range(5)), list(range(5)), prefix="replay_")


def test_floor_and_pair_environments_in_one_wave_per_step_launches(setup, per_step):
    _, _, _, E, _, _ = setup
    got = per_step[1]
    assert got["nan_resets"] == 0 and np.isfinite(got["obs"]).all()
    assert got["self_contacts"] > 0                   # the pair loop ran
    _same_as_fixture(got, E, FLOOR_ENVS, FLOOR_ENVS)      # an environment's numbers do not depend on its wave mates


def test_floor_and_pair_environments_in_one_wave_fused(setup, per_step):
    hm, _, mixed, E, _, _ = setup
    got = _rollout(hm, mixed, N, steps_per_launch=8)
    _same_as_each_other(got, per_step[1])
    _same_as_fixture(got, E, FLOOR_ENVS, FLOOR_ENVS)


def test_floor_and_pair_environments_in_one_wave_replay_pass(setup):
    hm, _, mixed, E, _, _ = setup
    got = _rollout(hm, mixed, N, replay=2)
    assert got["replayed_env_steps"] == N * T and got["nan_resets"] == 0 and np.isfinite(got["obs"]).all()
    assert got["self_contacts"] > 0
    _same_as_fixture(got, E, FLOOR_ENVS, FLOOR_ENVS, prefix="replay_")


def test_one_control_step_from_each_hard_state(setup):
    from test_hessian_paths_gpu import run_states
    hm, _, _, _, S, G = setup
    for i, name in enumerate(S["names"]):
        got = run_states(hm, S, [i])
        for key in "qvw":
            want = G["n1_step1_" + key][i]
            assert np.array_equal(got[key].reshape(want.shape), want), (str(name), key, np.abs(got[key].reshape(want.shape) - want).max())
        for key in ("solver_iters", "linesearch_evals", "replayed"):
            assert got[key] == G["n1_step1_" + key][i], (str(name), key, got[key], G["n1_step1_" + key][i])
        if str(name).startswith("self_contact"):
            again = run_states(hm, S, [i], replay=2)          # ... nor on which kernel ran it
            assert again["replayed"] == 1
            for key in "qvw":
                assert np.array_equal(again[key], got[key]), (str(name), "replay", key)
