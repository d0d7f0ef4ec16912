"""
The generic kernel family without a GPU: the device code of its instances (lm_core.h with the cone read at run time, chosen by the
lane emulator through pick_family like the library does) against the fp64 oracle, and how much the edited option moves the oracle —
the cases of tests/test_generic_family_gpu.py (generic_family_common.CASES). Test tooling only.
"""

import numpy as np
import pytest

import generic_family_common as GF
import test_plain_layout_gpu as G
from emu import pyemu
from loco_mujoco_amd import LocoEnv, lowering, mjcf

KEYS = list(GF.CASES)
N_EMU, N_EMU_STAGES = 4, 2            # the emulator plays one quad with four OS threads: a few states


@pytest.mark.parametrize("key", KEYS)
def test_emulator_runs_the_librarys_instance(key):
    """The lowering of every case is a family-6 model, and the emulator runs the instance lm_family.hip launches for it: links and slots
    per chain, integrator, cone read at run time (-1), no muscles, no pair pass."""
    import ctypes as C
    c = GF.inputs(key)
    out = (C.c_int * 8)()
    blob = np.ascontiguousarray(c["cm"], dtype=np.float64)
    C.CDLL(pyemu.build()).emu_instance(blob.ctypes.data_as(C.c_void_p), 0, out)
    mc, ns, rk4 = GF.CASES[key][3]
    assert list(out) == [GF.GENERIC_FAMILY, 1, mc, ns, int(rk4), -1, 0, 0]
    # (the lowering builds no self-collision tables for these models — the generic kernels have no pair pass: what the oracle is switched
    # to in the two cases whose robot has colliding links)
    assert int(blob[lowering.H_NGPAIR]) == 0


@pytest.mark.parametrize("key", KEYS)
def test_emulator_one_control_step_and_stages_vs_oracle(key):
    """Four of the 37 states, one control step (ten substeps) on the emulator against the oracle of the edited model: within qpos 1e-4 /
    qvel 1e-2 wherever the oracle itself does not jump (test_plain_layout_gpu._oracle_pass), no contact dropped. Stages of the first
    substep on two states: the contact count is the oracle's (the emulator counts every forward pass: four under RK4), M within 2e-5,
    qacc_smooth within 2e-5 scale + 1e-3, qacc within 1e-4 scale (tests/test_gpu_parity.py test_forward_stages_match_oracle)."""
    c = dict(GF.inputs(key))
    c.update(rows=c["rows"][:N_EMU], acts=c["acts"][:N_EMU])
    m, nv = c["m"], c["m"].nv
    o = GF.oracle_for(key, m)
    qo, vo, _, left_out, unhandled = G._oracle_pass(c, [o] * N_EMU)
    assert unhandled == 0 and left_out.sum() <= 1
    q0, v0 = c["rows"][:, :nv].astype(np.float64), c["rows"][:, nv:2 * nv].astype(np.float64)
    q, v, _, cnt, _ = pyemu.run(c["cm"], q0, v0, c["acts"], nsub=10)
    keep = ~left_out
    eq, ev = np.abs(q - qo).max(1), np.abs(v - vo).max(1)
    print("%s emulator vs oracle: qpos %.2e qvel %.2e (%d of %d states)" % (key, eq[keep].max(), ev[keep].max(), keep.sum(), N_EMU))
    assert cnt["overflow"] == 0 and cnt["unhandled"] == 0 and cnt["replayed"] == 0 and cnt["ncon"] > 0
    assert eq[keep].max() < G.QTOL and ev[keep].max() < G.VTOL
    passes = 4 if GF.CASES[key][3][2] else 1
    for k in range(N_EMU_STAGES):
        f = o.forward(q0[k], v0[k], GF.ctrl_of(c, k))
        _, _, _, c1, d = pyemu.run(c["cm"], q0[k], v0[k], c["acts"][k], nsub=1, debug_env=0)
        assert c1["ncon"] == passes * f["ncon"], (key, k, c1["ncon"], f["ncon"])
        assert np.abs(d["M"] - f["M"]).max() < 2e-5
        assert np.abs(d["qacc_smooth"] - f["qacc_smooth"]).max() < 2e-5 * max(1.0, np.abs(f["qacc_smooth"]).max()) + 1e-3
        assert np.abs(d["qacc"] - f["qacc"]).max() < 1e-4 * max(1.0, np.abs(f["qacc"]).max()), (key, k)


@pytest.mark.parametrize("key", KEYS)
def test_edited_option_moves_the_oracle(key):
    """A kernel that ignored the run-time cone or integrator could not pass the parity cases: on the 37 states the oracle of the edited
    model and the oracle of the model as shipped differ by more than the tolerance (qpos 1e-4 or qvel 1e-2) in at least 15 states."""
    c = GF.inputs(key)
    m, nv = c["m"], c["m"].nv
    edited, shipped = GF.oracle_for(key, m), GF.shipped_oracle(key)
    moved = 0
    for i in range(GF.N):
        q0, v0 = c["rows"][i, :nv].astype(np.float64), c["rows"][i, nv:2 * nv].astype(np.float64)
        (qa, va), (qb, vb) = edited.step(q0, v0, GF.ctrl_of(c, i), 10)[:2], shipped.step(q0, v0, GF.ctrl_of(c, i), 10)[:2]
        moved += bool(np.abs(qa - qb).max() > G.QTOL or np.abs(va - vb).max() > G.VTOL)
    print("%s: the edit moves %d of %d states beyond the tolerance" % (key, moved, GF.N))
    assert moved >= 15


def test_muscle_model_under_an_elliptic_cone_lowers_but_has_no_family():
    """The lowering accepts it (92 muscles, an elliptic header) — the refusal is lm_model_create's (pick_family: -1, tests/test_model_parse_host.py
    EDITED; on the GPU tests/test_generic_family_gpu.py) — and the emulator, which chooses like the library, runs nothing for it."""
    np.random.seed(0)
    env = LocoEnv.make("HumanoidMuscle.run", debug=True)
    env._model.cone = mjcf.CONE_ELLIPTIC
    cm = env._chain_model()
    assert int(cm[lowering.H_NMUSCLE]) == 92 and int(cm[lowering.H_CONE]) == mjcf.CONE_ELLIPTIC
    nv = env._model.nv
    row = env._reset_table()[0]
    with pytest.raises(AssertionError, match="emulator returned -1"):
        pyemu.run(cm, row[:nv], row[nv:2 * nv], np.zeros(len(env._action_indices)), nsub=1, act=np.zeros(92))
