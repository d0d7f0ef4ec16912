"""
The paths of the Newton iteration's Hessian pass (lm_core.h hess_slot: the 6-wide and the 3-wide instantiation of `accumulate`, one per
environment and iteration) on the CPU lane emulator: a change of path must not change a bit.

tests/golden/a1_newton_hard_states.npz (written by tools/probes/newton_hard_states.py) holds quadruped states (qpos, qvel, warm start,
action) and what the emulator of the commit BEFORE the one-path vote computed from each in one control step:
  reset_row        a row of the reset table, no contact
  standing         foot contacts only (condim 6: the 6-wide path alone)
  collapsed        the control step of the zero-action roll-out with the most Newton iterations (78): condim-6 feet and condim-3 shins in
                   every one of its 88 Hessian passes, 66 of which also mix the quadratic and the cone zone
  zones_mixed_*    two more steps of the same roll-out whose passes mix the two zones
  turned_*         the robot on its back: condim-3 contacts only — the 3-wide path still runs
  self_contact_*   states of tests/golden/a1_self_contact_states.npz: self-contact slots between two legs beside the floor contacts
in three configurations: four line-search points per round with one replica and with four, and one point per round.
"""

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv, lowering
from emu import pyemu

GOLD = np.load(__file__.replace("test_hessian_paths_host.py", "golden/a1_newton_hard_states.npz"))
NAMES = [str(x) for x in GOLD["names"]]


@pytest.fixture(scope="module")
def cmod():
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True)
    return lowering.lower(env._model, env._device_task())[0]


def test_the_fixture_holds_the_states_it_promises():
    for kind in ("reset_row", "standing", "collapsed", "zones_mixed", "turned", "self_contact"):
        assert any(n.startswith(kind) for n in NAMES), kind
    assert 6 <= len(NAMES) <= 10
    k = next(i for i, n in enumerate(NAMES) if n.startswith("collapsed"))
    assert GOLD["ls4_rep1_solver_iters"][k] >= 60 and GOLD["ls4_rep1_ls_evals"][k] >= 150


@pytest.mark.parametrize("tag,kw", [("ls4_rep1", dict(ls_points=4, rep=1)), ("ls4_rep4", dict(ls_points=4, rep=4)), ("ls1_rep1", dict(ls_points=1, rep=1))])
def test_one_control_step_is_bitwise_the_recorded_one(cmod, tag, kw):
    for i, name in enumerate(NAMES):
        q, v, w, cnt, _ = pyemu.run(cmod, GOLD["qpos"][i], GOLD["qvel"][i], GOLD["action"][i], nsub=10, warm=GOLD["warm"][i], **kw)
        for key, got in (("q", q[0]), ("v", v[0]), ("w", w[0])):
            assert np.array_equal(got, GOLD["%s_%s" % (tag, key)][i]), (name, tag, key, np.abs(got - GOLD["%s_%s" % (tag, key)][i]).max())
        for key in ("solver_iters", "ls_evals", "ncon"):
            assert cnt[key] == GOLD["%s_%s" % (tag, key)][i], (name, tag, key, cnt[key], GOLD["%s_%s" % (tag, key)][i])
