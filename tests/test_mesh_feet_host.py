"""
Mesh-foot HumanoidTorque (``use_box_feet=False``) on the host: joint equality constraints in the MJCF compiler, seven-link chains and
equality records in the lowering, the environment surface, the unchanged tables of every other configuration, and the fp64 primal
solver the GPU tests pin the equality rows against (tests/mesh_feet_common.py). No GPU.
"""

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv, lowering as L, mjcf
from mesh_feet_common import EQ_JOINTS, FIXTURE, equality_rows, impedance, make_env, oracle_rows, primal_solve, twin

GOLDEN = Path(__file__).resolve().parent / "golden"

_MJCF = """
<mujoco>
  <compiler angle="radian"/>
  <default>{default}</default>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 0.1"/>
    <body name="base" pos="0 0 1">
      <joint name="root_z" type="slide" axis="0 0 1"/>
      <geom type="sphere" size="0.1" mass="1"/>
      <body name="l1"><joint name="j1" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 0 0 -0.3" size="0.03" mass="0.5"/>
        <body name="l2" pos="0 0 -0.3"><joint name="j2" axis="0 1 0"/><geom type="capsule" fromto="0 0 0 0 0 -0.3" size="0.03" mass="0.5"/></body>
      </body>
    </body>
  </worldbody>
  <equality>{equality}</equality>
</mujoco>
"""


def _compile(equality, default=""):
    return mjcf.compile_mjcf(mjcf.MjcfHandle.from_string(_MJCF.format(equality=equality, default=default)))


def test_joint_equality_parses_with_mujoco_defaults():
    m = _compile('<joint name="e" joint1="j1"/><joint name="off" joint1="j2" active="false"/><weld body1="base" active="false"/>')
    assert m.eq_names == ["e"] and list(m.eq_type) == [mjcf.EQ_JOINT]
    assert m.eq_obj1id[0] == m.jnt_id("j1") and m.eq_obj2id[0] == -1
    assert np.allclose(m.eq_data[0], [0, 1, 0, 0, 0])
    assert np.allclose(m.eq_solref[0], [0.02, 1.0]) and np.allclose(m.eq_solimp[0], [0.9, 0.95, 0.001, 0.5, 2.0])
    m = _compile('<joint joint1="j1" joint2="j2" polycoef="0.1 2" solref="0.05 0.5" solimp="0.8 0.9"/>',
                 default='<equality solref="0.03 2" solimp="0.7 0.8 0.01"/>')
    assert m.eq_obj2id[0] == m.jnt_id("j2") and np.allclose(m.eq_data[0], [0.1, 2, 0, 0, 0])
    assert np.allclose(m.eq_solref[0], [0.05, 0.5]) and np.allclose(m.eq_solimp[0], [0.8, 0.9, 0.001, 0.5, 2.0])
    m = _compile('<joint joint1="j2"/>', default='<equality solref="0.03 2" solimp="0.7 0.8 0.01"/>')
    assert np.allclose(m.eq_solref[0], [0.03, 2]) and np.allclose(m.eq_solimp[0], [0.7, 0.8, 0.01, 0.5, 2.0])


def test_compiled_model_round_trips_the_equality_arrays(tmp_path):
    m = _compile('<joint name="e" joint1="j1" polycoef="0.2"/>')
    m.save(tmp_path / "m.model.npz")
    m2 = mjcf.CompiledModel.load(tmp_path / "m.model.npz")
    assert m2.eq_names == ["e"] and np.array_equal(m2.eq_data, m.eq_data) and np.array_equal(m2.eq_obj1id, m.eq_obj1id)


@pytest.fixture(scope="module")
def env():
    return make_env()


def test_fixture_lowers_to_seven_link_chains_with_four_equality_records(env):
    m = env._model
    assert m.nv == 23 and m.nu == 17 and sorted(m.eq_names) == sorted(j + "_constraint" for j in EQ_JOINTS)
    cmod, info = L.lower(m, env._device_task())
    assert info["n_chains"] == 3 and info["max_links"] == 7 and info["equality_rows"] == 4
    nl = [int(cmod[L.HEADER_SIZE + L.CM_CHAINS + L.C_NLINKS * L.NCHAIN + c]) for c in range(3)]
    assert sorted(nl) == [3, 7, 7]
    assert info["self_collision_tables"]["geom_pairs"] == 850 and info["mesh_vertices"] == 6407
    neq, off = int(cmod[L.H_NEQ]), int(cmod[L.H_OFF_EQ])
    assert neq == 4 and off > 0
    recs = cmod[L.HEADER_SIZE + off:L.HEADER_SIZE + off + neq * L.EQ_SIZE].reshape(neq, L.EQ_SIZE)
    for i, r in enumerate(recs):
        d = m.jnt_id(m.eq_names[i].replace("_constraint", ""))
        assert int(r[L.EQ_LANE]) == info["dof_to_lane"][d]
        # the record's link holds that dof
        blk = L.HEADER_SIZE + L.CM_CHAINS + (L.C_LINKS + int(r[L.EQ_LINK]) * L.LINK_SIZE + L.D_DOF) * L.NCHAIN + int(r[L.EQ_LANE])
        assert int(cmod[blk]) == d
        # k and b from solref (MuJoCo's mj_makeImpedance with the engine's defaults), solimp, dof_invweight0
        dmax = 0.95
        tc = max(0.02, 2 * m.timestep)
        assert np.isclose(r[L.EQ_K], 1.0 / (dmax * dmax * tc * tc)) and np.isclose(r[L.EQ_B], 2.0 / (dmax * tc))
        assert r[L.EQ_REF] == 0.0 and np.allclose(r[L.EQ_S0:L.EQ_S0 + 5], [0.9, 0.95, 0.001, 0.5, 2.0])
        assert r[L.EQ_INVW] == m.dof_invweight0[d] > 0
    # R = (1 - imp) / imp * invweight0 at a state: the restatement against numpy
    q = np.zeros(m.nv)
    q[[m.jnt_id(j) for j in EQ_JOINTS]] = [0.01, -0.2, 0.0005, 0.5]
    J, aref, R = equality_rows(m, q, np.zeros(m.nv))
    for i, j in enumerate(m.eq_obj1id):
        imp = impedance([0.9, 0.95, 0.001, 0.5, 2.0], abs(q[j]))
        assert np.isclose(R[i], (1 - imp) / imp * m.dof_invweight0[j]) and J[i, j] == 1.0
    assert np.isclose(impedance([0.9, 0.95, 0.001, 0.5, 2.0], 0.0005), 0.925)


def test_lowering_refuses_what_the_device_lacks(env):
    task = env._device_task()
    m = env._model
    for mutate, msg in ((lambda t: t.eq_obj2id.__setitem__(0, t.jnt_id("mtp_angle_r")), "joint2"),
                        (lambda t: t.eq_type.__setitem__(0, mjcf.EQ_WELD), "weld"),
                        (lambda t: t.eq_type.__setitem__(0, mjcf.EQ_CONNECT), "connect"),
                        (lambda t: t.eq_obj1id.__setitem__(0, t.jnt_id("pelvis_tilt")), "root dof")):
        t = twin(m)
        for k in ("eq_type", "eq_obj1id", "eq_obj2id", "eq_data", "eq_solref", "eq_solimp"):
            setattr(t, k, getattr(m, k).copy())
        t.eq_names = list(m.eq_names)
        mutate(t)
        with pytest.raises(L.UnsupportedModel, match=msg):
            L.lower(t, task)
    # the twin lowers without records
    cmod, info = L.lower(twin(m), task)
    assert int(cmod[L.H_NEQ]) == 0 and int(cmod[L.H_OFF_EQ]) == 0 and "equality_rows" not in info


def test_environment_surface():
    env = make_env()
    obs = env.reset()
    assert env.info.observation_space.shape == (44,) and env.info.action_space.shape == (17,) and obs.shape == (44,)
    assert np.isfinite(obs).all()
    keys = [k for k, _, _ in env.obs_helper.observation_spec]
    for j in EQ_JOINTS:
        assert "q_" + j in keys and "dq_" + j in keys
    env = make_env(use_foot_forces=True)
    assert env.info.observation_space.shape == (56,) and env._grf_group_names() == ["foot_r", "front_foot_r", "foot_l", "front_foot_l"]
    # still refused: muscles / 4Ages with mesh feet, free arms, and mesh feet without a model
    from loco_mujoco_amd.environments.humanoids import HumanoidMuscle, HumanoidTorque, HumanoidTorque4Ages
    for cls, kw in ((HumanoidTorque, dict(use_box_feet=False)), (HumanoidTorque, dict(disable_arms=False)),
                    (HumanoidMuscle, dict(use_box_feet=False, model_path=FIXTURE)),
                    (HumanoidTorque4Ages, dict(use_box_feet=False, model_path=FIXTURE))):
        with pytest.raises(NotImplementedError):
            cls(**kw)
    with pytest.raises(NotImplementedError, match="model_path"):
        HumanoidTorque(use_box_feet=False)


def table_digest(cm):
    """sha256 of a lowered table without its capacity fields: the header with H_CM_SIZE cleared and the offsets behind the constant
    table taken relative to its end, the part of the constant table the model uses (H_CM_USED), and everything behind the table."""
    cm = np.asarray(cm, dtype=np.float64).copy()
    tail0 = L.HEADER_SIZE + int(cm[L.H_CM_SIZE])
    h = cm[:L.HEADER_SIZE].copy()
    h[L.H_CM_SIZE] = 0
    for f in (L.H_OFF_GPT, L.H_OFF_MESHV, L.H_OFF_MESHN, L.H_OFF_BPT, L.H_OFF_MESHADJ):
        h[f] -= tail0
    parts = [h, cm[L.HEADER_SIZE:L.HEADER_SIZE + int(cm[L.H_CM_USED])], cm[tail0:]]
    return hashlib.sha256(b"".join(p.tobytes() for p in parts)).hexdigest()


def test_tables_of_every_existing_configuration_are_unchanged():
    """Digests recorded with the six-link layout (before seven-link chains and equality records): every configuration lowers to the
    same table apart from the capacity fields."""
    want = json.loads((GOLDEN / "lowered_table_digests.json").read_text())
    for task, digest in want.items():
        np.random.seed(0)
        assert table_digest(LocoEnv.make(task, debug=True)._chain_model()) == digest, task


def test_primal_solver_reproduces_the_oracle_on_twin_states(env):
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    m = twin(env._model)
    o = Oracle(pack_model(m))
    tab = env._reset_table()
    rs = np.random.RandomState(1)
    n_rows = 0
    for i in rs.randint(0, len(tab), 12):
        q, v = tab[i, :m.nv], tab[i, m.nv:2 * m.nv]
        ctrl = rs.uniform(-1, 1, m.nu)
        f = o.forward(q, v, ctrl)
        J, aref, R, always = oracle_rows(f)
        n_rows += len(R)
        a = primal_solve(f["M"], f["qacc_smooth"], J, aref, R, always)
        assert np.abs(a - f["qacc"]).max() <= 1e-8 * max(1.0, np.abs(f["qacc"]).max()), i
    assert n_rows > 0
