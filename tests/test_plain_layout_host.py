"""
The plain layout without a device: the LDS arithmetic behind lm_batch_set_layout's refusal (lm_lds_bytes: the launch code asked what
it would request, nothing launched), and that the oracle check of tests/test_plain_layout_gpu.py tells one dataset state from the next.
"""

import ctypes as C

import numpy as np
import pytest

import test_plain_layout_gpu as G
from loco_mujoco_amd import lowering

LDS_CU = 160 * 1024
KINDS = {"forward": 0, "replicated": 1, "plain": 2, "plain DR": 4, "plain DRV": 8, "replay": 10}


def _lds(family, kind, width, cm_floats):
    from loco_mujoco_amd.backend import load_library
    s, d = C.c_int(0), C.c_int(0)
    rc = load_library().lm_lds_bytes(family, kind, width, cm_floats, C.byref(s), C.byref(d))
    return None if rc else (s.value, d.value)


def test_lds_of_every_family_and_width_and_the_one_that_does_not_fit():
    """Static + dynamic LDS per workgroup of every family's kernels at 4 (replicated), 8 and 16 (plain) environments per workgroup, with
    the constant table of the model the GPU tests run (and with a full table, LM_CM_SIZE): only the muscle humanoid with pair tables at
    16 exceeds the 160 KB of a compute unit with its own table — 13 400 + 155 648 = 169 048 B; at 8 it takes 95 704 B."""
    over = []
    for name, fam in sorted(G.FAMILY.items(), key=lambda kv: kv[1]):
        cm = np.asarray(G._case(name)["cm"])
        used = (int(cm[lowering.H_CM_USED]) + 63) & ~63
        full = (int(cm[lowering.H_CM_SIZE]) + 63) & ~63
        for width, kind in ((4, 1), (8, 2), (16, 2)):
            s, d = _lds(fam, kind, width, used)
            sf, df = _lds(fam, kind, width, full)
            assert (s, d) == _lds(fam, kind + 2, width, used) == _lds(fam, kind + 6, width, used)      # the DR / DRV parts: the same lane memory
            print("family %2d (%s) at %2d per workgroup: static %6d B + dynamic %6d B = %6d B of %d B%s | with a full constant table %6d B%s"
                  % (fam, name, width, s, d, s + d, LDS_CU, "  OVER" if s + d > LDS_CU else "", sf + df, "  OVER" if sf + df > LDS_CU else ""))
            if s + d > LDS_CU:
                over.append((fam, width))
            assert d == 4 * used + df - 4 * full
        s, d = _lds(fam, 10, 4, used)
        print("family %2d replay kernel: static %d B + dynamic %d B" % (fam, s, d))
        assert s + d <= LDS_CU
    assert over == [(10, 16)]
    assert _lds(10, 2, 16, 2240) == (13400, 155648) and _lds(10, 2, 8, 2240) == (13400, 82304) and _lds(5, 2, 16, 2176) == (13400, 119552)
    assert _lds(8, 2, 16, 0) == (60, 122112) and _lds(11, 2, 16, 0) == (60, 140544)
    # no such kernel: the generic family has no part with model variants, families 1 and 3 are gone
    assert _lds(6, 8, 16, 0) is None and _lds(1, 2, 16, 0) is None and _lds(12, 2, 16, 0) is None and _lds(0, 13, 16, 0) is None


def test_swapping_one_state_for_its_neighbours_fails_the_oracle_check():
    """The tolerance separates one dataset state from the next: the GPU test's check passes on the oracle's own results rounded to
    float32 and FAILS when one environment's row is replaced by its neighbour's."""
    for name in ("UnitreeA1.simple", "HumanoidTorque.run"):
        c = G._case(name)
        q, v = c["qo"].astype(np.float32), c["vo"].astype(np.float32)
        G._check_against_oracle(name, "oracle rounded to float32", q, v, q, v, c["left_out"], c["qo"], c["vo"])
        i = int(np.nonzero(~c["left_out"])[0][3])
        q2, v2 = q.copy(), v.copy()
        q2[i], v2[i] = q[i + 1], v[i + 1]
        with pytest.raises(AssertionError):
            G._check_against_oracle(name, "row %d swapped" % i, q2, v2, q, v, c["left_out"], c["qo"], c["vo"])
