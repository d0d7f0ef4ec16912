"""
Mesh-foot HumanoidTorque on the MI355X: kernel family 11 (seven-link chains, RK4, condim-3 pyramids, the pair pass and the convex
collider, joint equality rows). The fp64 oracle has no equality rows, so every comparison of a whole step runs the "twin" (the fixture
without its four equality constraints) on both sides; the equality rows themselves are pinned against an independent fp64 restatement
of MuJoCo's primal problem with the four rows appended to the oracle's (tests/mesh_feet_common.py).
"""

import copy

import numpy as np
import pytest

from loco_mujoco_amd import lowering
from oracle.model_blob import pack_model
from oracle.pyoracle import Oracle
from mesh_feet_common import EQ_JOINTS, equality_rows, make_env, oracle_rows, primal_solve, twin

pytestmark = pytest.mark.gpu

QTOL, VTOL = 1e-4, 1e-2


@pytest.fixture(scope="module")
def mesh():
    from loco_mujoco_amd.backend import HipBatch, HipModel
    env = make_env()
    m = env._model
    t = twin(m)
    task = env._device_task()
    full_cm, twin_cm = lowering.lower(m, task)[0], lowering.lower(t, task)[0]
    assert int(full_cm[lowering.H_NEQ]) == 4 and int(twin_cm[lowering.H_NEQ]) == 0
    return env, m, t, HipModel(full_cm), HipModel(twin_cm), Oracle(pack_model(t)), HipBatch


def _states(env, n, seed):
    tab = env._reset_table()
    rs = np.random.RandomState(seed)
    rows = tab[rs.randint(0, len(tab), n)]
    return rows, rs


def _ctrl(env, m, act):
    c = np.zeros(m.nu)
    c[env._action_indices] = env._preprocess_action(act)
    return c


def test_mesh_feet_forward_stages(mesh):
    """forward_debug of the twin against the oracle (M, bias, qacc_smooth, qacc, ncon), and of the full model against the primal
    solver with the four equality rows appended to the oracle's rows."""
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    n = 32
    rows, rs = _states(env, n, 11)
    acts = rs.uniform(-1, 1, (n, 17))
    q32, v32 = rows[:, :m.nv].astype(np.float32).astype(np.float64), rows[:, m.nv:2 * m.nv].astype(np.float32).astype(np.float64)
    dd = {}
    for name, hm in (("twin", htwin), ("full", hfull)):
        b = HipBatch(hm, n)
        b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
        dd[name] = b.forward_debug(acts)
    used, worst_eq = 0, 0.0
    for k in range(n):
        f = oracle.forward(q32[k], v32[k], _ctrl(env, m, acts[k]).astype(np.float32).astype(np.float64))
        if f["unhandled_pairs"]:
            continue
        used += 1
        d = dd["twin"]
        assert d["ncon"][k] == f["ncon"], k
        assert np.abs(d["M"][k] - f["M"]).max() < 2e-5
        assert np.abs(d["qfrc_bias"][k] - f["bias"]).max() < 2e-4
        scale = max(1.0, np.abs(f["qacc_smooth"]).max())
        assert np.abs(d["qacc_smooth"][k] - f["qacc_smooth"]).max() < 2e-5 * scale + 1e-3
        scale = max(1.0, np.abs(f["qacc"]).max())
        assert np.abs(d["qacc"][k] - f["qacc"]).max() < 1e-4 * scale, (k, np.abs(d["qacc"][k] - f["qacc"]).max())
        # the full model: the oracle's rows + the four equality rows
        J, aref, R, always = oracle_rows(f)
        Je, arefe, Re = equality_rows(m, q32[k], v32[k])
        a = primal_solve(f["M"], f["qacc_smooth"], np.vstack([J, Je]), np.concatenate([aref, arefe]), np.concatenate([R, Re]),
                         np.concatenate([always, np.ones(len(Re), dtype=bool)]))
        scale = max(1.0, np.abs(a).max())
        err = np.abs(dd["full"]["qacc"][k] - a).max()
        worst_eq = max(worst_eq, err / scale)
        assert err < 1e-4 * scale, (k, err, scale)
        # the rows act: the full model's qacc differs from the twin's on the constrained dofs
    print("mesh feet forward stages: %d/%d states compared, worst full-model qacc error %.2e x scale" % (used, n, worst_eq))
    assert used >= n // 2


def test_mesh_feet_twin_control_step_vs_oracle(mesh):
    """The twin: one control step of 128 dataset states under random actions against the oracle, the states where the oracle's
    proximity counter finds an unhandled pair set aside (the rule of test_humanoid_torque_random_states_vs_oracle)."""
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    n = 128
    rows, rs = _states(env, n, 3)
    acts = rs.uniform(-1, 1, (n, 17))
    b = HipBatch(htwin, n)
    b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
    b.step(acts)
    q, v = b.get_state()
    eq, ev, used = [], [], 0
    for i in range(n):
        qo, vo, _, st = oracle.step(rows[i, :m.nv].astype(np.float32).astype(np.float64),
                                    rows[i, m.nv:2 * m.nv].astype(np.float32).astype(np.float64), _ctrl(env, m, acts[i]), nsub=10)
        if st["unhandled_pairs"]:
            continue
        used += 1
        eq.append(np.abs(q[i] - qo).max())
        ev.append(np.abs(v[i] - vo).max())
    eq, ev = np.array(eq), np.array(ev)
    beyond = int(((eq >= QTOL) | (ev >= VTOL)).sum())
    print("mesh feet twin control step: %d/%d compared, qpos max %.2e median %.2e, qvel max %.2e median %.2e, %d beyond QTOL/VTOL"
          % (used, n, eq.max(), np.median(eq), ev.max(), np.median(ev), beyond))
    assert np.isfinite(q).all() and np.isfinite(v).all()
    # frozen at the measured counts (MI355X, the library of this change): 128 of 128 states compared, none beyond the tolerance
    assert used >= 120 and beyond == 0


def test_mesh_feet_twin_per_environment_damping_vs_oracle(mesh):
    """The per-environment joint damping kernels (part 1: DR) of family 11: 16 dataset states with their own damping of every dof,
    one control step of the twin against the oracle run on a copy of the model with that damping."""
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    n = 16
    rows, rs = _states(env, n, 7)
    acts = rs.uniform(-1, 1, (n, 17))
    damp = t.dof_damping[None, :] * rs.uniform(0.5, 2.0, (n, m.nv))
    b = HipBatch(htwin, n)
    b.set_dof_params(damping=damp)
    b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
    b.step(acts)
    q, v = b.get_state()
    used = 0
    for i in range(n):
        mi = copy.copy(t)
        mi.dof_damping = damp[i].copy()
        qo, vo, _, st = Oracle(pack_model(mi)).step(rows[i, :m.nv].astype(np.float32).astype(np.float64),
                                                    rows[i, m.nv:2 * m.nv].astype(np.float32).astype(np.float64), _ctrl(env, m, acts[i]), nsub=10)
        if st["unhandled_pairs"]:
            continue
        used += 1
        assert np.abs(q[i] - qo).max() < QTOL and np.abs(v[i] - vo).max() < VTOL, i
    assert used >= n // 2


def test_mesh_feet_foot_forces_vs_oracle(mesh, tmp_path):
    """use_foot_forces=True: 56 observations, the 12 foot-force entries (r_foot, r_bofoot, l_foot, l_bofoot) against the oracle's
    contact forces under the reference's rule (tests/oracle_backend.py), the twin on both sides."""
    import sys, os
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from loco_mujoco_amd import LocoEnv
    from oracle_backend import attach
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    path = tmp_path / "twin.model.npz"
    t.save(path)
    mk = lambda: LocoEnv.make("HumanoidTorque.walk", use_box_feet=False, model_path=path, debug=True, use_foot_forces=True)
    np.random.seed(0)
    dev = mk()
    np.random.seed(0)
    ora = attach(mk())
    np.random.seed(0)
    o_dev = dev.reset()
    np.random.seed(0)
    o_ora = ora.reset()
    assert o_dev.shape == (56,) and np.array_equal(o_dev, o_ora)
    rs = np.random.RandomState(4)
    fmax, steps = 0.0, 0
    for k in range(6):
        a = rs.randn(17) * 0.1
        o_dev, _, d_dev, _ = dev.step(a)
        o_ora, _, d_ora, _ = ora.step(a)
        steps += 1
        assert np.abs(o_dev[:-12] - o_ora[:-12]).max() < VTOL
        assert np.abs(o_dev[-12:] - o_ora[-12:]).max() < 2e-2 * max(1e-3, np.abs(o_ora[-12:]).max()), (k, o_dev[-12:], o_ora[-12:])
        fmax = max(fmax, np.abs(o_ora[-12:]).max())
        if d_ora or d_dev:
            break
        dev._backend.set_state(ora._backend.qpos, ora._backend.qvel)
    assert fmax > 1e-3


def test_mesh_feet_replay_and_fused_are_bitwise(mesh):
    """The full model: the replay kernel (every control step abandoned to it) gives the regular kernel's bits, and a fused rollout
    (launches of 7 + 7 + 6 control steps) the single-step rollout's."""
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    n = 128
    rows, rs = _states(env, n, 5)
    acts = rs.uniform(-1, 1, (3, n, 17))
    out = []
    for mode in (1, 2):
        b = HipBatch(hfull, n)
        b.set_replay(mode)
        b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
        obs = [b.step(a)[0] for a in acts]
        q, v = b.get_state()
        out.append((q, v, obs[-1], b.stats()))
    (q1, v1, o1, s1), (q2, v2, o2, s2) = out
    assert s2["replayed_env_steps"] == 3 * n and s1["overflow_contacts"] == 0 and s2["overflow_contacts"] == 0
    assert np.isfinite(q1).all() and np.array_equal(q1, q2) and np.array_equal(v1, v2) and np.array_equal(o1, o2)
    tab = env._reset_table()
    out = []
    for fuse in (1, 7):
        b = HipBatch(hfull, n)
        b.set_reset_table(tab, seed=3)
        b.set_auto_reset(True, horizon=15)
        b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
        st = b.rollout(20, action_mode=1, seed=9, steps_per_launch=fuse)
        q, v = b.get_state()
        out.append((q, v, st, b.replay_marks()))
    (q1, v1, s1, m1), (q7, v7, s7, m7) = out
    same = ~(m1 | m7)
    assert same.sum() >= 0.9 * n
    assert np.array_equal(q1[same], q7[same]) and np.array_equal(v1[same], v7[same])
    assert s1["overflow_contacts"] == 0 and s7["overflow_contacts"] == 0 and s1["env_steps"] == n * 20


def test_mesh_feet_rollout_with_auto_reset(mesh):
    """512 environments, 200 control steps under a random policy with the device's auto-reset: finite, nothing dropped, and the
    equality rows hold the subtalar / mtp joints near their reference where the twin lets them swing."""
    env, m, t, hfull, htwin, oracle, HipBatch = mesh
    n = 512
    rows, _ = _states(env, n, 0)
    tab = env._reset_table()
    dofs = [m.jnt_id(j) for j in EQ_JOINTS]
    peak = {}
    for name, hm in (("full", hfull), ("twin", htwin)):
        b = HipBatch(hm, n)
        b.set_reset_table(tab, seed=1)
        b.set_auto_reset(True, horizon=1000)
        b.set_state(rows[:, :m.nv], rows[:, m.nv:2 * m.nv])
        pk = 0.0
        for _ in range(10):
            st = b.rollout(20, action_mode=1, seed=5)
            q, v = b.get_state()
            assert np.isfinite(q).all() and np.isfinite(v).all()
            assert st["nan_resets"] == 0 and st["overflow_contacts"] == 0
            pk = max(pk, np.abs(q[:, dofs]).max())
        peak[name] = pk
    print("mesh feet rollout 512 x 200: max |q| of subtalar / mtp: %.3g with the equality rows, %.3g in the twin" % (peak["full"], peak["twin"]))
    # frozen from the measured run (MI355X, the library of this change): 0.736 rad with the rows, 2.36 rad without
    assert peak["full"] < 1.0 and peak["twin"] > 2.0
