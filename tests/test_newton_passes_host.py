"""
The slot passes of the quadruped's Newton iteration on the CPU lane emulator, and the assembly fingerprint tool.

* lm_families.h LM_DPP_BCAST leaves the emulator alone: its policy has no DPP members, lm_core.h's detection helper must fall back to
  rep_bcast / quad_read, and 40 control steps of reset-table row 0 under zero action with the warm start carried (the robot collapses
  at control steps 28-31) on the four-replica emulator built from this tree are bitwise those of the emulator built with the switch
  at 0. The emulator also checks the replicas' protocol (two replicas changing one lane-memory word to different values end the run).
* tools/isa_arith_fingerprint.py on two hand-written kernels: the same arithmetic with other registers, moves and waits is "equal";
  a multiply + subtract against a fused multiply-add is found, in the region (loop) where it stands.
"""

import io
import os
import subprocess
import sys

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv, lowering
from emu import pyemu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = 40


def _emu_switched_off():
    """The four-replica emulator of this tree with the switch at 0 (pyemu.build's command, plus the define)."""
    emu_dir = os.path.join(HERE, "emu")
    lib = os.path.join(emu_dir, "libemu4_rep4_passes_off.so")
    srcs = [os.path.join(emu_dir, "emu.cpp"), os.path.join(ROOT, "loco_mujoco_amd", "csrc", "lm_core.h"),
            os.path.join(ROOT, "loco_mujoco_amd", "csrc", "lm_families.h"), os.path.join(ROOT, "include", "lm_layout.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in srcs):
        tmp = lib + ".tmp%d" % os.getpid()
        subprocess.check_call(["g++", "-O2", "-std=c++20", "-pthread", "-fPIC", "-shared", "-ffp-contract=off", "-DEMU_LS_POINTS=4", "-DEMU_REP=4",
                               "-DEMU_PYRAMID_ONLY", "-DLM_DPP_BCAST=0", "-o", tmp, srcs[0]])
        os.replace(tmp, lib)
    return lib


def _rollout(cmod, q, v, lib=None):
    """STEPS control steps under zero action, warm start carried; lib: another emulator library in place of pyemu's own."""
    real_build = pyemu.build
    if lib is not None:
        pyemu.build = lambda *a, **k: lib
    try:
        nv = q.shape[0]
        w, a = np.zeros(nv), np.zeros(12)
        tape, iters, evals = [], 0, 0
        for _ in range(STEPS):
            qe, ve, we, cnt, _dbg = pyemu.run(cmod, q, v, a, nsub=10, warm=w, ls_points=4, rep=4)
            q, v, w = qe[0], ve[0], we[0]
            tape.append(np.concatenate([q, v, w]))
            iters += cnt["solver_iters"]; evals += cnt["ls_evals"]
        return np.array(tape), iters, evals
    finally:
        pyemu.build = real_build


def test_forty_control_steps_of_the_collapsing_robot_are_bitwise_the_unswitched_passes():
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True)
    cmod = lowering.lower(env._model, env._device_task())[0]
    nv = env._model.nv
    assert len(env._action_indices) == 12
    table = env._reset_table()
    q0, v0 = table[0, :nv].copy(), table[0, nv:2 * nv].copy()
    got, iters, evals = _rollout(cmod, q0, v0)
    want, iters0, evals0 = _rollout(cmod, q0, v0, lib=_emu_switched_off())
    assert np.isfinite(got).all()
    # the hard roll-out (profiles/newton_hessian_paths_notes.md §1): 65 + 78 + 43 Newton iterations in control steps 28-30 alone, about
    # ten in each of the standing ones in front of them, and line searches of more than one round
    assert iters >= 400 and evals > iters, (iters, evals)
    assert (iters, evals) == (iters0, evals0)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:1]


# ---- the fingerprint tool -------------------------------------------------------------------------------------------------------------
_KERNEL_A = """
	.text
	.globl	_Z6kernelPf
_Z6kernelPf:                            ; @_Z6kernelPf
; %bb.0:
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_mov_b32_e32 v1, 0
	s_waitcnt lgkmcnt(0)
	v_mul_f32_e32 v2, v0, v0
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	ds_bpermute_b32 v3, v4, v2
	s_waitcnt lgkmcnt(0)
	v_pk_mul_f32 v[6:7], v[2:3], v[4:5]
	v_sub_f32_e32 v8, v6, v7
	v_fma_f32 v9, -v8, v2, v1
	s_add_i32 s2, s2, -1
	s_cmp_lg_u32 s2, 0
	s_cbranch_scc1 .LBB0_1
; %bb.2:
	v_rcp_f32_e32 v10, v9
	v_max_f32_e64 v10, |v10|, v2
	global_store_dword v1, v10, s[0:1]
	s_endpgm
.Lfunc_end0:
	.size	_Z6kernelPf, .Lfunc_end0-_Z6kernelPf
"""
# the same arithmetic: other registers, a DPP move in place of the LDS permute and its wait, another encoding of the multiply
_KERNEL_SAME = _KERNEL_A.replace("ds_bpermute_b32 v3, v4, v2\n\ts_waitcnt lgkmcnt(0)", "v_mov_b32_dpp v3, v2 row_newbcast:4 row_mask:0xf bank_mask:0xf bound_ctrl:1") \
                        .replace("v_mul_f32_e32 v2, v0, v0", "v_mul_f32_e64 v12, v0, v0").replace("v_sub_f32_e32 v8, v6, v7", "v_sub_f32_e32 v18, v16, v17")
# the product and the difference of the loop fused the other way: v_mul + v_fma instead of a packed multiply + an unfused subtract
_KERNEL_FUSED = _KERNEL_A.replace("v_pk_mul_f32 v[6:7], v[2:3], v[4:5]\n\tv_sub_f32_e32 v8, v6, v7", "v_mul_f32_e32 v7, v3, v5\n\tv_fma_f32 v8, v2, v4, -v7")


@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_arith_fingerprint
    finally:
        sys.path.pop(0)
    return isa_arith_fingerprint


def _compare(tool, tmp_path, a, b):
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(a); pb.write_text(b)
    na, fa = tool.fingerprint(str(pa), "kernel")
    nb, fb = tool.fingerprint(str(pb), "kernel")
    assert na == nb == "_Z6kernelPf"
    out = io.StringIO()
    return tool.report(na, fa, nb, fb, out=out), out.getvalue(), fa, fb


def test_fingerprint_ignores_registers_moves_and_waits(tool, tmp_path):
    same, text, fa, fb = _compare(tool, tmp_path, _KERNEL_A, _KERNEL_SAME)
    assert same, text
    assert [len(r["fp"]) for r in fa] == [1, 3, 2]                      # in front of the loop, the loop, behind it
    assert fa[1]["fp"] == ["v_pk_mul_f32(++)", "v_sub_f32(++)", "v_fma_f32(-++)"] and fa[2]["fp"] == ["v_rcp_f32(+)", "v_max_f32(+a+)"]
    assert fa[1]["counts"]["lds_permute"] == 1 and fb[1]["counts"]["lds_permute"] == 0
    assert fb[1]["counts"]["move"] == fa[1]["counts"]["move"] + 1 and fb[1]["counts"]["wait"] == fa[1]["counts"]["wait"] - 1


def test_fingerprint_finds_a_pair_fused_the_other_way(tool, tmp_path):
    same, text, fa, fb = _compare(tool, tmp_path, _KERNEL_A, _KERNEL_FUSED)
    assert not same
    assert "FIRST DIFFERENCE: region 1" in text and ".LBB0_1" in text, text
    assert fb[1]["fp"] == ["v_mul_f32(++)", "v_fma_f32(++-)", "v_fma_f32(-++)"]
    assert fa[0]["fp"] == fb[0]["fp"] and fa[2]["fp"] == fb[2]["fp"]
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    assert tool.main([str(pa), str(pb), "kernel"]) == 1 and tool.main([str(pa), str(pa), "kernel"]) == 0
    assert tool.main([str(pa), str(pb), "no_such_kernel"]) == 2
