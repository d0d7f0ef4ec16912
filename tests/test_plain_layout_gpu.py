"""
The plain layout (lm_batch_set_layout: 8 or 16 environments per workgroup, no replicas; `-m gpu`). It selects another compiled kernel
for every family and part — QuadDppT<1>, the one-point line search, (4 epb + 15) / 16 groups of lane memory, padding quads of another
shape — so every family's plain kernels are held to what the replicated ones are held to:
  a. one control step against the fp64 oracle, 37 states (ragged last workgroup) and a single one, at both widths;
  b. environment i comes out bitwise the same whatever batch it sits in, across device-side restarts;
  c. the kernels with per-environment joint parameters and with model variants against each environment's oracle;
  d. a control step handed from a plain launch to the replay kernel is bitwise the replicated layout's;
  e. (tests/test_terminal_obs_gpu.py: the terminal row of a pair family in the plain layout)
  f. a layout whose kernels need more LDS than a compute unit has is refused at the call, with the byte counts: the muscle humanoid
     with pair tables at 16 per workgroup (13 400 B static + 155 648 B dynamic against 163 840 B). That launch was made once and ended
     in an illegal memory access; NO test here runs a muscle kernel at 16 per workgroup with pair tables.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv, lowering
from oracle.model_blob import pack_model
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.gpu

QTOL, VTOL = 1e-4, 1e-2      # the stated fp32 tolerance of one control step (tests/test_gpu_parity.py)
N = 37                       # at 16 per workgroup: two full workgroups and one of 5 environments + 11 padding quads; at 8: four and 5 + 3
MAX_LEFT_OUT = 2             # knife-edge states per task (a condition of the test, not a measurement)
LDS_CU = 160 * 1024          # LDS of a gfx950 compute unit
MESH, MUSCLE, MUSCLE_NOPAIRS = "HumanoidTorque.mesh_feet", "HumanoidMuscle.run", "HumanoidMuscle.run.nopairs"
# one task per kernel family (lm_kernels.hip family_of)
FAMILY = {"UnitreeA1.simple": 0, "Atlas.walk": 2, "Talos.walk": 4, "HumanoidTorque.run": 8, "UnitreeH1.run": 9, "UnitreeG1.walk": 7, MESH: 11,
          MUSCLE: 10, MUSCLE_NOPAIRS: 5}
CASES = [(t, w) for t in FAMILY for w in (8, 16) if (t, w) != (MUSCLE, 16)]      # (f: that layout is refused, and never launched)
KIND_PLAIN = 2               # include/locohip.h lm_lds_bytes


@functools.lru_cache(maxsize=None)
def _case(name):
    """One lowering, one set of inputs and ONE oracle pass per task for the whole module (read-only): the 37 states and actions of the
    issue, the oracle's result for each and whether the oracle itself jumps there (the rule of
    test_error_distribution_three_control_steps_vs_oracle: its result moves by more than 3x the tolerance under a 1e-6 / 1e-5
    perturbation of its input, RandomState(1000 + i), four probes)."""
    np.random.seed(0)
    if name == MESH:
        # the fp64 oracle has no equality rows: the twin on both sides (tests/test_mesh_feet_gpu.py); b runs the full model
        from mesh_feet_common import make_env, twin
        env = make_env()
        om = twin(env._model)
        cm, cm_full = lowering.lower(om, env._device_task())[0], lowering.lower(env._model, env._device_task())[0]
    else:
        env = LocoEnv.make(name.replace(".nopairs", ""), debug=True)
        om = env._model
        cm = env._chain_model() if name != MUSCLE_NOPAIRS else lowering.lower(om, dict(env._device_task(), self_collisions=False))[0]
        cm_full = cm
    oracle = Oracle(pack_model(om))
    if name == MUSCLE_NOPAIRS:
        oracle.set_option("disable_self_collision", 1)          # the same robot without its pair tables, on both sides
    tab = env._reset_table()
    rs = np.random.RandomState(11)
    rows = np.ascontiguousarray(tab[rs.randint(0, len(tab), N)], dtype=np.float32)
    acts = rs.uniform(-0.3, 0.3, (N, len(env._action_indices)))
    c = dict(name=name, env=env, m=om, cm=cm, cm_full=cm_full, tab=tab, rows=rows, acts=acts, rs=rs)
    qo, vo, ao, left_out, unhandled = _oracle_pass(c, [oracle] * N)
    c.update(qo=qo, vo=vo, ao=ao, left_out=left_out)
    assert unhandled == 0 and left_out.sum() <= MAX_LEFT_OUT, (name, unhandled, int(left_out.sum()))
    return c


def _oracle_pass(c, oracles):
    """(qpos, qvel, activations, knife-edge mask, unhandled pairs) of one control step of c's states under oracles[i]."""
    env, m, rows, acts = c["env"], c["m"], c["rows"], c["acts"]
    nv = m.nv

    def run(o, q, v, ctrl):
        if m.na:
            r = o.step_act(q, v, np.zeros(m.na), ctrl, 10, np.zeros(nv))
            return r[0], r[1], r[2], r[4]
        r = o.step(q, v, ctrl, 10, np.zeros(nv))
        return r[0], r[1], np.zeros(0), r[3]

    qo, vo, ao, jump, unhandled = [], [], [], [], 0
    for i in range(len(rows)):
        q0, v0 = rows[i, :nv].astype(np.float64), rows[i, nv:2 * nv].astype(np.float64)
        ctrl = np.zeros(m.nu)
        ctrl[env._action_indices] = env._preprocess_action(acts[i])
        q, v, a, st = run(oracles[i], q0, v0, ctrl)
        unhandled += int(st["unhandled_pairs"] != 0)
        prs = np.random.RandomState(1000 + i)
        j = False
        for e in (1e-6, 1e-6, 1e-5, 1e-5):
            qp, vp, _, _ = run(oracles[i], q0 + e * prs.uniform(-1, 1, nv), v0 + e * prs.uniform(-1, 1, nv), ctrl)
            j = j or np.abs(qp - q).max() > 3 * QTOL or np.abs(vp - v).max() > 3 * VTOL
        qo.append(q); vo.append(v); ao.append(a); jump.append(j)
    return np.stack(qo), np.stack(vo), np.stack(ao), np.array(jump), unhandled


@functools.lru_cache(maxsize=None)
def _model(name, full=False):
    from loco_mujoco_amd.backend import HipModel
    c = _case(name)
    return HipModel(c["cm_full"] if full else c["cm"])


def _load(b, c, rows):
    nv = c["m"].nv
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    if rows.shape[1] > 2 * nv:
        b.set_goal(rows[:, 2 * nv:])


def _raw_step(b, act):
    from test_terminal_obs_gpu import _raw_step as raw
    return raw(b, act)


def _lds(name, width, kind=KIND_PLAIN):
    """(static, dynamic) LDS bytes of the kernel the task's family launches at `width` per workgroup, from the library's own arithmetic."""
    from loco_mujoco_amd.backend import load_library
    cm = np.asarray(_case(name)["cm"])
    used = (int(cm[lowering.H_CM_USED]) + 63) & ~63
    s, d = C.c_int(0), C.c_int(0)
    assert load_library().lm_lds_bytes(FAMILY[name], kind, width, used, C.byref(s), C.byref(d)) == 0
    return s.value, d.value


def _plain_batch(name, n, width, full=False):
    """A batch of the task in the plain layout — or None where the library refuses the layout, with the refusal checked: only a model
    whose kernels exceed the compute unit's LDS (by the byte counts of lm_lds_bytes) may be refused. (No task here is served by the
    generic family, which has one layout only: tests/test_generic_family_gpu.py.)"""
    from loco_mujoco_amd.backend import BackendError, HipBatch
    s, d = _lds(name, width)
    try:
        b = HipBatch(_model(name, full), n, envs_per_workgroup=width)
    except BackendError as e:
        assert s + d > LDS_CU and "LDS" in str(e) and str(s) in str(e) and str(d) in str(e), (name, width, s, d, str(e))
        print("%s at %d per workgroup refused: %s" % (name, width, e))
        return None
    assert s + d <= LDS_CU, (name, width, s, d)              # what was accepted fits
    return b


def _check_against_oracle(name, label, q, v, qr, vr, left_out, qo, vo):
    """Every state the rule does not leave out within QTOL / VTOL of the oracle, worst case; and where the replicated layout (qr, vr) is
    within tolerance of the oracle the plain layout must be too, left-out states included."""
    eq, ev = np.abs(q - qo).max(1), np.abs(v - vo).max(1)
    rq, rv = np.abs(qr - qo).max(1), np.abs(vr - vo).max(1)
    keep = ~left_out
    print("%s %s: %d of %d states (%d knife-edge states left out): qpos Linf max %.2e qvel Linf max %.2e (replicated layout: %.2e / %.2e)"
          % (name, label, keep.sum(), len(q), left_out.sum(), eq[keep].max(), ev[keep].max(), rq[keep].max(), rv[keep].max()))
    assert np.isfinite(q).all() and np.isfinite(v).all()
    assert left_out.sum() <= MAX_LEFT_OUT
    assert eq[keep].max() < QTOL and ev[keep].max() < VTOL, (name, label, np.nonzero(keep & ((eq >= QTOL) | (ev >= VTOL)))[0])
    rep_ok = (rq < QTOL) & (rv < VTOL)
    assert (eq[rep_ok] < QTOL).all() and (ev[rep_ok] < VTOL).all(), (name, label, np.nonzero(rep_ok & ((eq >= QTOL) | (ev >= VTOL)))[0])


@functools.lru_cache(maxsize=None)
def _replicated_step(name):
    """The same batch in the replicated layout (computed once per task, read-only)."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(name)
    b = HipBatch(_model(name), N)
    _load(b, c, c["rows"])
    _raw_step(b, c["acts"])
    return b.get_state()


# ------------------------------------------------------------------------------------------------------------------------------
# a. one control step against the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,width", CASES)
def test_plain_layout_one_control_step_vs_oracle(name, width):
    """37 dataset states under actions from U(-0.3, 0.3), one control step in the plain layout against the fp64 oracle: every state the
    oracle itself does not jump at (at most 2 of 37) within qpos 1e-4 / qvel 1e-2, worst case; a state the replicated layout gets
    within tolerance the plain layout gets within tolerance; no contact dropped, no state reset as non-finite. Muscle activations
    within 1e-5 (test_humanoid_muscle_one_control_step_kats' bound)."""
    c = _case(name)
    b = _plain_batch(name, N, width)
    if b is None:
        return
    _load(b, c, c["rows"])
    _raw_step(b, c["acts"])
    q, v = b.get_state()
    qr, vr = _replicated_step(name)
    _check_against_oracle(name, "plain layout, %d per workgroup" % width, q, v, qr, vr, c["left_out"], c["qo"], c["vo"])
    if b.na:
        ea = np.abs(b.get_activation() - c["ao"]).max()
        print("%s %d per workgroup: activations max %.2e" % (name, width, ea))
        assert ea < 1e-5
    st = b.stats()
    assert st["overflow_contacts"] == 0 and st["nan_resets"] == 0 and st["env_steps"] == N


@pytest.mark.parametrize("name", [t for t in FAMILY if t != MUSCLE])
def test_plain_layout_single_environment_vs_oracle(name):
    """n = 1 at 16 per workgroup: one environment and fifteen padding quads. Environment 0 of the 37, against the oracle and bitwise
    the 37-batch's (what a padding quad computes is stored nowhere)."""
    c = _case(name)
    b1, b = _plain_batch(name, 1, 16), _plain_batch(name, N, 16)
    if b1 is None:
        assert b is None
        return
    _load(b1, c, c["rows"][:1])
    _raw_step(b1, c["acts"][:1])
    q, v = b1.get_state()
    if not c["left_out"][0]:
        eq, ev = np.abs(q[0] - c["qo"][0]).max(), np.abs(v[0] - c["vo"][0]).max()
        print("%s n = 1 at 16 per workgroup: qpos %.2e qvel %.2e" % (name, eq, ev))
        assert eq < QTOL and ev < VTOL
    _load(b, c, c["rows"])
    _raw_step(b, c["acts"])
    qa, va = b.get_state()
    assert np.array_equal(q[0], qa[0]) and np.array_equal(v[0], va[0])
    assert b1.stats()["overflow_contacts"] == 0 and b1.stats()["nan_resets"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# b. batch-composition invariance inside the plain layout
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,width", CASES)
def test_plain_layout_environment_is_bitwise_the_same_in_any_batch(name, width):
    """Four control steps under the random policy (seed 3) with device-side restarts (reset table under seed 7, horizon 2): environment
    offset + i of the 37-batch and of the sub-batches (1, 0), (1, 36), (5, 20), (17, 3) — other workgroup counts, other numbers of
    padding quads — ends in bitwise the same state, after the same number of steps and episodes. Compared after the third step too:
    at horizon 2 the fourth step ends every episode, so the final state is a reset-table row (the draw); the state after three steps
    is one control step of physics behind a restart."""
    c = _case(name)

    def run(n, off):
        b = _plain_batch(name, n, width, full=True)
        if b is None:
            return None
        b.set_reset_table(c["tab"], seed=7, global_env_offset=off)
        b.set_auto_reset(True, horizon=2)
        _load(b, c, c["rows"][off:off + n])
        b.rollout(3, action_mode=1, seed=3, steps_per_launch=1)
        mid = b.get_state() + ((b.get_activation(),) if b.na else ())
        b.rollout(1, action_mode=1, seed=3, steps_per_launch=1)
        return mid, b.get_state() + ((b.get_activation(),) if b.na else ()), b.stats()

    whole = run(N, 0)
    if whole is None:
        return
    mid_a, end_a, sa = whole
    assert sa["env_steps"] == 4 * N and sa["episodes"] >= 2 * N and sa["nan_resets"] == 0 and sa["overflow_contacts"] == 0
    assert all(np.isfinite(x).all() for x in mid_a + end_a)
    nv = c["m"].nv
    # (not vacuous: after three steps three quarters of the environments and more carry a control step of physics — they sit on no
    # reset row, as one that fell in the third step would — and no two of those are alike)
    tab32 = c["tab"].astype(np.float32)
    moved = np.array([not (tab32[:, :nv] == mid_a[0][e]).all(1).any() for e in range(N)])
    assert moved.sum() >= 3 * N // 4 and len(np.unique(mid_a[0][moved], axis=0)) == moved.sum()
    for n, off in ((1, 0), (1, 36), (5, 20), (17, 3)):
        mid, end, st = run(n, off)
        for x, xa in zip(mid + end, mid_a + end_a):
            assert np.array_equal(x, xa[off:off + n]), (name, width, n, off)
        assert st["env_steps"] == 4 * n and st["episodes"] >= 2 * n and st["nan_resets"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# c. the plain kernels with per-environment joint parameters (DR) and with model variants (DRV)
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task", ["UnitreeA1.simple", "Atlas.walk", "Talos.walk"])
def test_plain_layout_per_environment_joint_parameters_vs_oracle(task):
    """37 environments at 16 per workgroup, each with its own damping / stiffness / friction loss (drawn as in
    test_per_environment_joint_parameters_vs_oracle), one control step against the oracle compiled with that environment's numbers:
    a's tolerance and a's rule, and the replicated layout's kernel of the same part beside it."""
    from loco_mujoco_amd.backend import HipBatch, HipModel
    from test_gpu_parity import _with_dof_params
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, **(dict(disable_back_joint=False) if task.startswith("Atlas") else {}))
    m = env._model
    tab = env._reset_table()
    rs = np.random.RandomState(11)
    rows = np.ascontiguousarray(tab[rs.randint(0, len(tab), N)], dtype=np.float32)
    acts = rs.uniform(-0.3, 0.3, (N, len(env._action_indices)))
    damp = np.tile(m.dof_damping, (N, 1)) * rs.uniform(0.5, 2.0, (N, m.nv)) + (m.dof_damping > 0) * rs.uniform(0, 1, (N, m.nv))
    stiff = np.tile(m.jnt_stiffness, (N, 1)) * rs.uniform(0.5, 1.5, (N, m.nv))
    floss = np.tile(m.dof_frictionloss, (N, 1)) * rs.uniform(0.5, 1.5, (N, m.nv))
    c = dict(env=env, m=m, rows=rows, acts=acts)
    oracles = [Oracle(pack_model(_with_dof_params(m, damp[i].astype(np.float32), stiff[i].astype(np.float32), floss[i].astype(np.float32)))) for i in range(N)]
    qo, vo, _, left_out, unhandled = _oracle_pass(c, oracles)
    assert unhandled == 0
    hm = HipModel(env._chain_model())
    out = []
    for width in (16, None):
        b = HipBatch(hm, N, envs_per_workgroup=width)
        _load(b, c, rows)
        b.set_dof_params(damping=damp, stiffness=stiff, frictionloss=floss)
        _raw_step(b, acts)
        out.append(b.get_state())
        assert b.stats()["overflow_contacts"] == 0 and b.stats()["nan_resets"] == 0
    (q, v), (qr, vr) = out
    _check_against_oracle(task, "joint parameters, 16 per workgroup", q, v, qr, vr, left_out, qo, vo)
    # the nominal kernel on the same states differs (the parameters matter)
    b2 = HipBatch(hm, N, envs_per_workgroup=16)
    _load(b2, c, rows)
    _raw_step(b2, acts)
    assert np.abs(b2.get_state()[1] - v).max() > 1e-3


def test_plain_layout_model_variants_vs_oracle():
    """test_model_variants_one_control_step_vs_oracle at 16 per workgroup, 37 environments: every environment on the variant it drew
    (a pool of five) with its own joint damping, against the oracle of that variant's compiled model."""
    from test_gpu_parity import _talos_variant_env, _with_dof_params
    env = _talos_variant_env(N, 5)
    m = env._model
    env.reset()
    variants, prm = env._pending_variants.copy(), env._pending_dof_params.copy()
    assert len(set(variants)) >= 3
    q0 = np.stack([h.qpos for h in env._host]).astype(np.float32)
    v0 = np.stack([h.qvel for h in env._host]).astype(np.float32)
    acts = np.random.RandomState(2).uniform(-0.3, 0.3, (N, 12))
    env.backend.set_layout(16)
    env.step(acts)
    assert np.array_equal(env.backend.get_variant_index(), variants) and env.backend.n_variants == 5
    q, v = env.backend.get_state()
    c = dict(env=env, m=m, rows=np.concatenate([q0, v0], axis=1), acts=acts)
    oracles = [Oracle(pack_model(_with_dof_params(env._variant_models[0][variants[i]], *(prm[p][i].astype(np.float32) for p in range(3))))) for i in range(N)]
    qo, vo, _, left_out, unhandled = _oracle_pass(c, oracles)
    assert unhandled == 0
    qn, vn, _, _, _ = _oracle_pass(c, [Oracle(pack_model(_with_dof_params(m, *(prm[p][i].astype(np.float32) for p in range(3))))) for i in range(N)])
    _check_against_oracle("Talos.walk", "model variants, 16 per workgroup", q, v, q, v, left_out, qo, vo)
    assert np.abs(v - vn).max() > 10 * VTOL                      # the variants are different robots
    st = env.backend.stats()
    assert st["overflow_contacts"] == 0 and st["nan_resets"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# d. hand-over to the replay kernel from a plain launch
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["HumanoidTorque.run", "Atlas.walk"])
def test_plain_launch_hands_over_to_the_replay_kernel_bitwise(name):
    """set_replay(2): every control step is abandoned by the regular kernel before its first substep — nothing of it is stored (lm_step.h:
    `gone`) — and run by the family's replay kernel on four replicas (kReplayRep) from the untouched state. The regular kernel's
    layout therefore cannot show: three control steps from a plain launch at 16 per workgroup are bitwise those of the replicated
    layout under set_replay(2), observations included, and every replay mark is set."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(name)
    rs = np.random.RandomState(4)
    acts = rs.uniform(-0.3, 0.3, (3,) + c["acts"].shape)
    out = []
    for width in (16, None):
        b = HipBatch(_model(name), N, envs_per_workgroup=width)
        b.set_replay(2)
        _load(b, c, c["rows"])
        obs = [_raw_step(b, a)[0] for a in acts]
        st = b.stats()
        assert b.replay_marks().all() and st["replayed_env_steps"] == 3 * N and st["overflow_contacts"] == 0 and st["nan_resets"] == 0
        out.append((b.get_state(), obs))
    ((q, v), o), ((qr, vr), orr) = out
    assert np.array_equal(q, qr) and np.array_equal(v, vr) and all(np.array_equal(x, y) for x, y in zip(o, orr))
    assert np.isfinite(q).all() and np.abs(q - c["rows"][:, :c["m"].nv]).max() > 1e-3          # (the robots moved)


# ------------------------------------------------------------------------------------------------------------------------------
# f. the refusal
# ------------------------------------------------------------------------------------------------------------------------------

def test_layout_beyond_the_compute_units_lds_is_refused_at_the_call():
    """HumanoidMuscle.run with pair tables (family 10), n = 5: set_layout(16) raises with the byte counts — 13 400 B static + 155 648 B
    dynamic = 169 048 B against the compute unit's 163 840 B — and launches nothing: the batch then steps once in its default layout
    and equals, bitwise, a fresh batch that never received the call. set_layout(8) (95 704 B) is accepted and steps."""
    from loco_mujoco_amd.backend import BackendError, HipBatch
    c = _case(MUSCLE)
    s, d = _lds(MUSCLE, 16)
    assert (s, d) == (13400, 155648) and s + d > LDS_CU
    s8, d8 = _lds(MUSCLE, 8)
    assert s8 + d8 == 95704
    n = 5
    a, fresh = HipBatch(_model(MUSCLE), n), HipBatch(_model(MUSCLE), n)
    for b in (a, fresh):
        _load(b, c, c["rows"][:n])
    with pytest.raises(BackendError) as err:
        a.set_layout(16)
    msg = str(err.value)
    print(msg)
    assert "169048 B" in msg and "13400 B static" in msg and "155648 B dynamic" in msg and "compute unit has" in msg
    assert a.stats()["env_steps"] == 0                             # nothing ran
    with pytest.raises(BackendError, match="169048 B"):
        HipBatch(_model(MUSCLE), n, envs_per_workgroup=16)
    oa, of = _raw_step(a, c["acts"][:n]), _raw_step(fresh, c["acts"][:n])
    assert all(np.array_equal(x, y) for x, y in zip(oa, of))
    assert all(np.array_equal(x, y) for x, y in zip(a.get_state(), fresh.get_state())) and np.array_equal(a.get_activation(), fresh.get_activation())
    assert a.stats()["env_steps"] == n
    a.set_layout(8)
    _raw_step(a, c["acts"][:n])
    assert a.stats()["env_steps"] == 2 * n and np.isfinite(a.get_state()[0]).all()
