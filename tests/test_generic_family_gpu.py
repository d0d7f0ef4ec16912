"""
The generic kernel family (lm_families.h LM_GENERIC_FAMILY, lm_family.hip; `-m gpu`): what a model gets that no specialised family fits —
a model of the user's own, a shipped robot under another cone or integrator. Cone and chain length are read at run time, the layout is
the plain one at four environments per workgroup, there is no replay kernel: a contact beyond the slots is dropped and counted. One
case per instance a model reaches (generic_family_common.CASES), each held to what the specialised families are held to:
  a. the model is served by family 6: one layout only, and its kernels fit a compute unit's LDS;
  b. one control step against the fp64 oracle, 37 states and a single one, no contact dropped;
  c. the stages of lm_forward_debug against the oracle's forward pass;
  d. environment i comes out bitwise the same whatever batch it sits in;
  e. (tests/test_terminal_obs_gpu.py: the terminal row of a generic model; tests/test_step_bookkeeping_gpu.py: restarts, rollouts, rewards)
  f. the models no kernel is compiled for are refused when the model is created, with the reason.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import generic_family_common as GF
from loco_mujoco_amd import LocoEnv, lowering, mjcf
from test_plain_layout_gpu import KIND_PLAIN, LDS_CU, MAX_LEFT_OUT, N, QTOL, VTOL, _check_against_oracle, _load, _oracle_pass, _raw_step

pytestmark = pytest.mark.gpu

KEYS = list(GF.CASES)
N_STAGES = 8
A1_BIAS_BOUND = 2e-4         # tests/test_gpu_parity.py test_forward_stages_match_oracle: the quadruped's bound on the bias force


@functools.lru_cache(maxsize=None)
def _case(key):
    """The inputs of the case and ONE oracle pass for the whole module (read-only): test_plain_layout_gpu._case's rule."""
    c = dict(GF.inputs(key))
    oracle = GF.oracle_for(key, c["m"])
    qo, vo, _, left_out, unhandled = _oracle_pass(c, [oracle] * N)
    assert unhandled == 0 and left_out.sum() <= MAX_LEFT_OUT, (key, unhandled, int(left_out.sum()))
    c.update(oracle=oracle, qo=qo, vo=vo, left_out=left_out)
    return c


@functools.lru_cache(maxsize=None)
def _model(key):
    from loco_mujoco_amd.backend import HipModel
    return HipModel(_case(key)["cm"])


@functools.lru_cache(maxsize=None)
def _whole_batch_step(key):
    """One control step of the 37 states (computed once per case, read-only): (qpos, qvel, stats)."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(key)
    b = HipBatch(_model(key), N)
    _load(b, c, c["rows"])
    _raw_step(b, c["acts"])
    return b.get_state() + (b.stats(),)


# ------------------------------------------------------------------------------------------------------------------------------
# a. the family
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_model_is_served_by_the_generic_family(key):
    """The plain layouts of the specialised families are refused ("one layout only": only the generic family answers so), per-environment
    joint parameters too, and what lm_lds_bytes reports for family 6 — the five-link instance, the larger one — fits a compute unit at
    the one layout it has. (Which family the same edit of the shipped model file gets: tests/test_model_parse_host.py EDITED.)"""
    from loco_mujoco_amd.backend import BackendError, HipBatch, load_library
    c = _case(key)
    for width in (8, 16):
        with pytest.raises(BackendError, match="the generic kernel family has one layout only"):
            HipBatch(_model(key), N, envs_per_workgroup=width)
    b = HipBatch(_model(key), 4)
    with pytest.raises(BackendError, match="not compiled for this model's kernel family"):
        b.set_dof_params(damping=np.ones((4, c["m"].nv)))
    used = (int(np.asarray(c["cm"])[lowering.H_CM_USED]) + 63) & ~63
    s, d = C.c_int(0), C.c_int(0)
    assert load_library().lm_lds_bytes(GF.GENERIC_FAMILY, KIND_PLAIN, 4, used, C.byref(s), C.byref(d)) == 0
    print("%s: %d B static + %d B dynamic LDS per workgroup" % (key, s.value, d.value))
    assert 0 < s.value + d.value <= LDS_CU and d.value > 4 * used


# ------------------------------------------------------------------------------------------------------------------------------
# b. one control step against the fp64 oracle
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_generic_family_one_control_step_vs_oracle(key):
    """37 dataset states under actions from U(-0.3, 0.3) (the inputs of test_plain_layout_one_control_step_vs_oracle), one control step
    against the fp64 oracle of the edited model: every state the oracle itself does not jump at (at most 2 of 37) within qpos 1e-4 /
    qvel 1e-2, worst case. The generic kernels drop a contact beyond their slots: overflow_contacts == 0 keeps a drop from hiding."""
    c = _case(key)
    q, v, st = _whole_batch_step(key)
    _check_against_oracle(key, "generic family", q, v, q, v, c["left_out"], c["qo"], c["vo"])
    assert st["overflow_contacts"] == 0 and st["nan_resets"] == 0 and st["env_steps"] == N
    assert np.abs(q - c["rows"][:, :c["m"].nv]).max() > 1e-3          # (the robots moved)


@pytest.mark.parametrize("key", KEYS)
def test_generic_family_single_environment_vs_oracle(key):
    """n = 1: one environment and three padding quads. Environment 0 of the 37 against the oracle, and bitwise the 37-batch's."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(key)
    b1 = HipBatch(_model(key), 1)
    _load(b1, c, c["rows"][:1])
    _raw_step(b1, c["acts"][:1])
    q, v = b1.get_state()
    if not c["left_out"][0]:
        eq, ev = np.abs(q[0] - c["qo"][0]).max(), np.abs(v[0] - c["vo"][0]).max()
        print("%s n = 1: qpos %.2e qvel %.2e" % (key, eq, ev))
        assert eq < QTOL and ev < VTOL
    qa, va, _ = _whole_batch_step(key)
    assert np.array_equal(q[0], qa[0]) and np.array_equal(v[0], va[0])
    assert b1.stats()["overflow_contacts"] == 0 and b1.stats()["nan_resets"] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# c. the stages
# ------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _specialised_bias_error(task, disable_self_collision):
    """The largest error of the bias force of the SPECIALISED family's lm_forward_debug against the oracle, on the same robot as
    shipped and the same eight states (the bias force does not depend on the cone or the integrator)."""
    from loco_mujoco_amd.backend import HipBatch, HipModel
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    key = next(k for k, v in GF.CASES.items() if v[0] == task)
    c = _case(key)
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    o = Oracle(pack_model(env._model))
    if disable_self_collision:
        o.set_option("disable_self_collision", 1)
    b = HipBatch(HipModel(env._chain_model()), N_STAGES)
    _load(b, c, c["rows"][:N_STAGES])
    d = b.forward_debug(c["acts"][:N_STAGES])
    nv = c["m"].nv
    return max(np.abs(d["qfrc_bias"][k] - o.forward(c["rows"][k, :nv].astype(np.float64), c["rows"][k, nv:2 * nv].astype(np.float64), GF.ctrl_of(c, k))["bias"]).max()
               for k in range(N_STAGES))


@pytest.mark.parametrize("key", KEYS)
def test_generic_family_forward_stages_match_oracle(key):
    """lm_forward_debug on the first 8 of the 37 states against the oracle's forward pass under the edited cone / integrator: the
    contact count is the oracle's; the inertia matrix within 2e-5, qacc_smooth within 2e-5 scale + 1e-3 and qacc within 1e-4 scale
    (test_forward_stages_match_oracle's bounds). The bias force: the quadruped's bound of that test, 2e-4; for the humanoids, which
    have no project bound, twice the largest error of the specialised family's lm_forward_debug on the same robot as shipped and
    the same states. Measured on an MI355X, generic kernel / specialised kernel (the bound is twice the latter): Talos 8.28e-5 /
    8.28e-5, Atlas 1.60e-4 / 1.60e-4, HumanoidTorque 1.47e-4 / 1.47e-4, UnitreeH1 7.90e-5 / 7.90e-5 — the same code computes both; the
    quadruped 8.59e-6 under both edits."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(key)
    task, nv = GF.CASES[key][0], c["m"].nv
    b = HipBatch(_model(key), N_STAGES)
    _load(b, c, c["rows"][:N_STAGES])
    d = b.forward_debug(c["acts"][:N_STAGES])
    spec = _specialised_bias_error(task, GF.CASES[key][4])
    bias_bound = A1_BIAS_BOUND if task.startswith("UnitreeA1") else 2 * spec
    worst = dict(M=0.0, bias=0.0, qacc_smooth=0.0, qacc=0.0)
    ncon = 0
    for k in range(N_STAGES):
        f = c["oracle"].forward(c["rows"][k, :nv].astype(np.float64), c["rows"][k, nv:2 * nv].astype(np.float64), GF.ctrl_of(c, k))
        assert d["ncon"][k] == f["ncon"], (key, k, d["ncon"][k], f["ncon"])
        ncon += f["ncon"]
        e = dict(M=np.abs(d["M"][k] - f["M"]).max(), bias=np.abs(d["qfrc_bias"][k] - f["bias"]).max(),
                 qacc_smooth=np.abs(d["qacc_smooth"][k] - f["qacc_smooth"]).max() / (2e-5 * max(1.0, np.abs(f["qacc_smooth"]).max()) + 1e-3),
                 qacc=np.abs(d["qacc"][k] - f["qacc"]).max() / (1e-4 * max(1.0, np.abs(f["qacc"]).max())))
        worst = dict((n, max(worst[n], e[n])) for n in worst)
    print("%s stages, %d states, %d contacts: M %.2e, bias %.2e (specialised family %.2e, bound %.2e), qacc_smooth %.2f and qacc %.2f of their bounds"
          % (key, N_STAGES, ncon, worst["M"], worst["bias"], spec, bias_bound, worst["qacc_smooth"], worst["qacc"]))
    assert ncon > 0                                                   # (not vacuous: the contact stage ran)
    assert worst["M"] < 2e-5 and worst["qacc_smooth"] < 1.0 and worst["qacc"] < 1.0
    assert worst["bias"] <= bias_bound, (key, worst["bias"], spec)


# ------------------------------------------------------------------------------------------------------------------------------
# d. batch composition
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS)
def test_generic_family_environment_is_bitwise_the_same_in_any_batch(key):
    """One control step: environment offset + i of the 37-batch, alone ((1, 0), (1, 36): three padding quads) and in the sub-batch
    (5, 20) — another workgroup count, another number of padding quads — ends in bitwise the same state."""
    from loco_mujoco_amd.backend import HipBatch
    c = _case(key)
    qa, va, _ = _whole_batch_step(key)
    assert len(np.unique(qa, axis=0)) == N                            # (no two environments alike)
    for n, off in ((1, 0), (1, 36), (5, 20)):
        b = HipBatch(_model(key), n)
        _load(b, c, c["rows"][off:off + n])
        _raw_step(b, c["acts"][off:off + n])
        q, v = b.get_state()
        assert np.array_equal(q, qa[off:off + n]) and np.array_equal(v, va[off:off + n]), (key, n, off)


# ------------------------------------------------------------------------------------------------------------------------------
# f. the refusals
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task,reason", [("HumanoidMuscle.run", "the generic kernels that serve other cones and integrators have no muscles"),
                                         ("UnitreeG1.walk", "chains of six links are compiled for Euler")])
def test_models_without_a_kernel_are_refused_when_the_model_is_created(task, reason):
    """Under an elliptic cone the muscle humanoid fits no muscle family and the generic kernels are compiled without muscles — they
    would step it with its muscles slack; six-link chains have no run-time-cone kernel either. lm_model_create refuses both with the
    reason, before a batch exists; the same robots as shipped are created."""
    from loco_mujoco_amd.backend import BackendError, HipModel
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    HipModel(env._chain_model())
    env._model.cone = mjcf.CONE_ELLIPTIC
    with pytest.raises(BackendError) as err:
        HipModel(env._chain_model())
    print(str(err.value))
    assert "no kernel is compiled for this model" in str(err.value) and reason in str(err.value)
