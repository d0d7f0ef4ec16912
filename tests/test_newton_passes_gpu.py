"""
The exchanges between the replicas of an environment and between the lanes of a quad as DPP moves (lm_families.h LM_DPP_BCAST: the line
search's four points, the floor pass's contact counts, the pair pass's shared numbers) must not move a bit: a roll-out of a collapsing
robot through the quadruped's regular, fused and replay kernels, against what the library of the commit BEFORE that switch computed on
an MI355X (tests/golden/a1_collapse_rollout_gpu.npz: recorded once with `record()` below; `python tests/test_newton_passes_gpu.py
OUT.npz`). Building a floor slot's line-search polynomials in the visit that computes its direction rows was measured against this file
too and left it (profiles/newton_passes_notes.md): it is not in the source.

The roll-out: eight environments from rows 0-7 of the reset table, zero action, 40 control steps, one launch per control step. Row 0
collapses at control steps 28-31 (profiles/newton_hessian_paths_notes.md §1: 60-80 Newton iterations and 90-200 line-search rounds per
control step, condim-6 feet and condim-3 shins together): several geoms of one link group within reach of the floor (the floor pass's
replica counts), line searches of several rounds (the four points' exchange) and dozens of consecutive Newton iterations. Stored: the observation, reward and done tapes and the final qpos, qvel and warm start — of the regular
kernels (the ragged and the fused run are bitwise that) and, as `replay_*`, of the replay kernel, whose roll-out is its own.
"""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "golden", "a1_collapse_rollout_gpu.npz")
N, T = 8, 40
KEYS = ("obs", "reward", "done", "q", "v", "w")


def _model():
    from loco_mujoco_amd import LocoEnv
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True)
    return HipModel(env._chain_model()), np.asarray(env._reset_table(), dtype=np.float64)


def _start(hm, table):
    """qpos and qvel of reset rows 0 .. N-1, as float32 (what the device holds)."""
    nq, nv = hm.dims.nq, hm.dims.nv
    return table[:N, :nq].astype(np.float32), table[:N, nq:nq + nv].astype(np.float32)


def rollout(hm, start, n, steps_per_launch=1, replay=None):
    """T control steps of the first n start states under zero action, steps_per_launch of them per launch. Returns the tapes [T, n, ...],
    the final state and warm start [n, nv] and the batch's counters."""
    import torch
    from loco_mujoco_amd.backend import HipBatch
    from test_hessian_paths_gpu import _read_warm
    b = HipBatch(hm, n)
    if replay is not None:
        b.set_replay(replay)
    b.set_state(start[0][:n], start[1][:n])
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
    return dict(obs=obs.cpu().numpy(), reward=reward.cpu().numpy(), done=done.cpu().numpy(), q=q, v=v, w=w,
                solver_iters=st["solver_iters"], linesearch_evals=st["linesearch_evals"], replayed=st["replayed_env_steps"],
                nan_resets=st["nan_resets"])


def record(out):
    """The expected values, from the library that is loaded. Run twice: the recorder must reproduce itself; and the roll-out must be
    the hard one the test is about."""
    hm, table = _model()
    table = _start(hm, table)
    a, b = rollout(hm, table, N), rollout(hm, table, N)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert np.isfinite(a["obs"]).all() and a["nan_resets"] == 0
    assert a["solver_iters"] > 0 and a["linesearch_evals"] > a["solver_iters"]        # line searches of more than one round
    for name, got in (("ragged", rollout(hm, table, 5)), ("fused", rollout(hm, table, N, steps_per_launch=8))):
        n = got["q"].shape[0]
        for key in KEYS:
            want = a[key][:, :n] if key in ("obs", "reward", "done") else a[key][:n]
            assert np.array_equal(got[key], want), (name, key)
        if n == N:
            assert got["solver_iters"] == a["solver_iters"] and got["linesearch_evals"] == a["linesearch_evals"], name
    # the replay kernel is another instantiation (more slots, another pair pass): over 40 control steps of a collapsing robot its
    # roll-out is not bitwise the regular kernels', so it has expected values of its own
    r, r2 = rollout(hm, table, N, replay=2), rollout(hm, table, N, replay=2)
    for key in r:
        assert np.array_equal(r[key], r2[key]), ("replay", key)
    assert r["replayed"] == N * T and np.isfinite(r["obs"]).all() and r["nan_resets"] == 0
    for key in KEYS:
        d = np.abs(r[key].astype(np.float64) - a[key])
        print("replay against regular: %-6s largest difference %.3g, first control step that differs %s" % (
            key, d.max(), (np.nonzero(d.reshape(T, -1).max(axis=1))[0][:1] if d.ndim > 2 or key in ("reward", "done") else "-")))
    print("Newton iterations", a["solver_iters"], "line-search rounds", a["linesearch_evals"], "replayed", a["replayed"],
          "| replay kernel:", r["solver_iters"], r["linesearch_evals"])
    a.update({"replay_" + key: val for key, val in r.items()})
    np.savez_compressed(out, q0=table[0], v0=table[1], **a)
    print("wrote", out, os.path.getsize(out), "bytes")


@pytest.fixture(scope="module")
def setup():
    hm, table = _model()
    E = np.load(EXPECTED)
    q0, v0 = _start(hm, table)
    assert np.array_equal(q0, E["q0"]) and np.array_equal(v0, E["v0"])          # the reset table's rows are the recorded start
    return hm, (q0, v0), E


def _same(got, E, n=N, counters=True, prefix=""):
    for key in KEYS:
        want = E[prefix + key][:, :n] if key in ("obs", "reward", "done") else E[prefix + key][:n]
        assert got[key].shape == want.shape and np.array_equal(got[key], want), (key, np.abs(got[key].astype(np.float64) - want).max())
    if counters:
        for key in ("solver_iters", "linesearch_evals"):
            assert got[key] == E[prefix + key], (key, got[key], E[prefix + key])


def test_one_launch_per_control_step(setup):
    hm, table, E = setup
    got = rollout(hm, table, N)
    _same(got, E)
    assert got["replayed"] == E["replayed"]


def test_two_waves_the_second_ragged(setup):
    hm, table, E = setup
    _same(rollout(hm, table, 5), E, n=5, counters=False)


def test_fused_eight_control_steps_per_launch(setup):
    hm, table, E = setup
    _same(rollout(hm, table, N, steps_per_launch=8), E)


def test_the_replay_kernel(setup):
    hm, table, E = setup
    got = rollout(hm, table, N, replay=2)            # 2: every environment through the replay kernel
    assert got["replayed"] == N * T
    _same(got, E, prefix="replay_")


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    import torch  # noqa: F401  (before the library, as tests/conftest.py does: torch finds its GPUs only with its own HIP runtime)
    record(sys.argv[1])
