"""
The paths of the Newton iteration's Hessian pass (lm_core.h hess_slot: one instantiation of `accumulate` per environment and iteration)
on the device: the states of tests/golden/a1_newton_hard_states.npz (test_hessian_paths_host.py describes them) through the quadruped's
regular, fused and replay kernels, bit for bit against what the library of the commit BEFORE the one-path vote computed on an MI355X
(tests/golden/a1_newton_hard_states_gpu.npz: recorded once with `record()` below; `python tests/test_hessian_paths_gpu.py OUT.npz`).

A batch has no call that sets or reads the solver's warm start, but a snapshot holds it: the third segment of the blob of
Snapshot.to_bytes() (lm_snapshot.h: [rows][N] float32 segments qpos, qvel, warm, each starting at a multiple of 256 bytes behind the
64-byte header). The warm start of a state is put in place by restoring a patched blob and read back the same way; the test checks
its reading of the layout on the qpos and qvel segments.
"""

import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
STATES = os.path.join(HERE, "golden", "a1_newton_hard_states.npz")
EXPECTED = os.path.join(HERE, "golden", "a1_newton_hard_states_gpu.npz")
GROUPS5 = ((0, 1, 2, 3, 4), (3, 4, 5, 6, 7))      # N = 5: two waves (four environments each), the second ragged; together every state


def _segments(n, nv):
    """Byte offsets of the qpos, qvel and warm segments in a snapshot blob of n environments."""
    from loco_mujoco_amd.backend import SNAPSHOT_BLOB_HEADER
    size = 4 * nv * n
    off, offs = 0, []
    for _ in range(3):
        off = (off + 255) // 256 * 256
        offs.append(SNAPSHOT_BLOB_HEADER + off)
        off += size
    return offs, size


def _read_warm(b):
    snap = b.snapshot()
    blob = np.frombuffer(snap.to_bytes(), dtype=np.uint8)
    snap.close()
    offs, size = _segments(b.n, b.nv)
    seg = [blob[o:o + size].view(np.float32).reshape(b.nv, b.n).T.copy() for o in offs]
    q, v = b.get_state()
    assert np.array_equal(seg[0], q) and np.array_equal(seg[1], v)          # the layout is what this file takes it to be
    return seg[2]


def _load(b, S, idx):
    """States idx of the fixture into the batch: positions and velocities, then the warm start through a patched snapshot."""
    b.set_state(S["qpos"][idx], S["qvel"][idx])
    snap = b.snapshot()
    blob = np.frombuffer(snap.to_bytes(), dtype=np.uint8).copy()
    snap.close()
    offs, size = _segments(b.n, b.nv)
    blob[offs[2]:offs[2] + size] = np.ascontiguousarray(S["warm"][idx].astype(np.float32).T).view(np.uint8).reshape(-1)
    snap = b.snapshot_from_bytes(blob.tobytes())
    b.restore(snap)
    snap.close()
    assert np.array_equal(_read_warm(b), S["warm"][idx].astype(np.float32))


def run_states(hm, S, idx, fused=False, replay=None):
    """One control step (fused: three control steps in one launch) of the states idx in one batch, under each state's action.
    Returns qpos, qvel, warm start [len(idx), nv] and the batch's counters."""
    import torch
    from loco_mujoco_amd.backend import HipBatch
    idx = list(idx)
    b = HipBatch(hm, len(idx))
    if replay is not None:
        b.set_replay(replay)
    _load(b, S, idx)
    b.stats(reset=True)
    act = np.ascontiguousarray(S["action"][idx], dtype=np.float32)
    if fused:
        b.rollout_tape(torch.from_numpy(act).cuda(), repeat=3, steps_per_launch=3)
    else:
        b.step(act)
    q, v = b.get_state()
    w = _read_warm(b)
    st = b.stats()
    b.close()
    return dict(q=q, v=v, w=w, solver_iters=st["solver_iters"], linesearch_evals=st["linesearch_evals"], replayed=st["replayed_env_steps"],
                nan_resets=st["nan_resets"])


def record(out):
    """The expected values, from the library that is loaded: every state alone (N = 1) and in the two groups of five, one control step
    and three fused ones. Run twice: the recorder must reproduce itself."""
    from loco_mujoco_amd import LocoEnv
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    hm = HipModel(LocoEnv.make("UnitreeA1.simple", debug=True)._chain_model())
    S = np.load(STATES)
    res = []
    for _ in range(2):
        r = {}
        for fused in (False, True):
            tag = "fused3" if fused else "step1"
            one = [run_states(hm, S, [i], fused) for i in range(len(S["names"]))]
            for key in one[0]:
                r["n1_%s_%s" % (tag, key)] = np.array([np.asarray(x[key]).reshape(-1) if key in "qvw" else x[key] for x in one])
            for g, idx in enumerate(GROUPS5):
                for key, val in run_states(hm, S, idx, fused).items():
                    r["n5g%d_%s_%s" % (g, tag, key)] = np.asarray(val)
        res.append(r)
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), key
    r = res[0]
    names = [str(x) for x in S["names"]]
    for tag in ("step1", "fused3"):
        assert not r["n1_%s_nan_resets" % tag].any()
        for i, name in enumerate(names):
            if tag == "step1" and not name.startswith("self_contact"):
                assert r["n1_%s_replayed" % tag][i] == 0, name          # the floor-contact states fit the regular kernel (the robot on its
                                                                        # back leaves it in its second control step)
        for g, idx in enumerate(GROUPS5):           # an environment's numbers do not depend on its wave mates
            for key in "qvw":
                assert np.array_equal(r["n5g%d_%s_%s" % (g, tag, key)], r["n1_%s_%s" % (tag, key)][list(idx)]), (g, tag, key)
        print(tag, "Newton iterations", r["n1_%s_solver_iters" % tag], "line-search rounds", r["n1_%s_linesearch_evals" % tag], "replayed",
              r["n1_%s_replayed" % tag])
    for g, idx in enumerate(GROUPS5):               # ... nor on which kernel ran it
        got = run_states(hm, S, idx, replay=2)
        assert got["replayed"] == len(idx), got["replayed"]
        for key in ("q", "v", "w", "solver_iters", "linesearch_evals"):
            assert np.array_equal(got[key], r["n5g%d_step1_%s" % (g, key)]), ("replay", g, key)
    np.savez_compressed(out, names=S["names"], **r)
    print("wrote", out, os.path.getsize(out), "bytes")


@pytest.fixture(scope="module")
def setup():
    from loco_mujoco_amd import LocoEnv
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    hm = HipModel(LocoEnv.make("UnitreeA1.simple", debug=True)._chain_model())
    S, E = np.load(STATES), np.load(EXPECTED)
    assert [str(x) for x in S["names"]] == [str(x) for x in E["names"]]
    return hm, S, E


def _same(got, E, prefix, rows=None):
    for key in "qvw":
        want = E["%s_%s" % (prefix, key)]
        want = want if rows is None else want[rows]
        assert np.array_equal(got[key].reshape(want.shape), want), (prefix, key, np.abs(got[key].reshape(want.shape) - want).max())
    for key in ("solver_iters", "linesearch_evals"):
        want = E["%s_%s" % (prefix, key)]
        want = want if rows is None else want[rows]
        assert got[key] == want, (prefix, key, got[key], want)


@pytest.mark.parametrize("fused", [False, True])
def test_one_environment_in_a_wave(setup, fused):
    hm, S, E = setup
    tag = "fused3" if fused else "step1"
    for i in range(len(S["names"])):
        got = run_states(hm, S, [i], fused)
        _same(got, E, "n1_" + tag, rows=i)
        if E["n1_%s_replayed" % tag][i] == 0:          # the states that fit the regular kernel stay in it
            assert got["replayed"] == 0, str(S["names"][i])


@pytest.mark.parametrize("fused", [False, True])
def test_two_waves_the_second_ragged(setup, fused):
    hm, S, E = setup
    tag = "fused3" if fused else "step1"
    for g, idx in enumerate(GROUPS5):
        got = run_states(hm, S, idx, fused)
        _same(got, E, "n5g%d_%s" % (g, tag))
        if E["n5g%d_%s_replayed" % (g, tag)] == 0:
            assert got["replayed"] == 0, g


def test_the_replay_kernel_gives_the_regular_kernels_numbers(setup):
    hm, S, E = setup
    for g, idx in enumerate(GROUPS5):
        got = run_states(hm, S, idx, replay=2)            # 2: every environment through the replay kernel
        assert got["replayed"] == len(idx)
        _same(got, E, "n5g%d_step1" % g)


if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]
    import torch  # noqa: F401  (before the library, as tests/conftest.py does: torch finds its GPUs only with its own HIP runtime)
    record(sys.argv[1])
