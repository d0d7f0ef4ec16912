"""
The line search's slot loop in two (lm_families.h LM_LS_FLOOR_SPLIT, lm_core.h kLsFloorSplit: floor slots with a weight of 1.0f that is
not read from lane memory, self-contact slots with slot_weight as before) on the CPU lane emulator: the split must not change a bit.

The states are those of tests/golden/a1_newton_hard_states.npz (test_hessian_paths_host.py describes them), compared with what the
emulator of the commit BEFORE the one-path vote computed from each in one control step:
  self_contact_*            slots between two legs beside the floor contacts: their weight in the line search is 0.5 (the pair loop)
  collapsed, zones_mixed_*  floor contacts only, 43-78 Newton iterations and 89-199 line-search rounds (the floor loop, every zone)
with four replicas and with one. And an environment's numbers do not depend on the batch it is evaluated in.
"""

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv, lowering
from emu import pyemu

GOLD = np.load(__file__.replace("test_line_search_slots_host.py", "golden/a1_newton_hard_states.npz"))
NAMES = [str(x) for x in GOLD["names"]]
PAIR = [i for i, n in enumerate(NAMES) if n.startswith("self_contact")]
FLOOR = [i for i, n in enumerate(NAMES) if n.startswith(("collapsed", "zones_mixed"))]
CONFIGS = [("ls4_rep4", dict(ls_points=4, rep=4)), ("ls4_rep1", dict(ls_points=4, rep=1))]


@pytest.fixture(scope="module")
def cmod():
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True)
    return lowering.lower(env._model, env._device_task())[0]


def _step(cmod, idx, **kw):
    idx = list(idx)
    q, v, w, cnt, _ = pyemu.run(cmod, GOLD["qpos"][idx], GOLD["qvel"][idx], GOLD["action"][idx], nsub=10, warm=GOLD["warm"][idx], **kw)
    return dict(q=q, v=v, w=w), cnt


def _same_as_recorded(cmod, idx, tag, kw):
    for i in idx:
        got, cnt = _step(cmod, [i], **kw)
        for key in "qvw":
            want = GOLD["%s_%s" % (tag, key)][i]
            assert np.array_equal(got[key][0], want), (NAMES[i], tag, key, np.abs(got[key][0] - want).max())
        for key in ("solver_iters", "ls_evals", "ncon"):
            assert cnt[key] == GOLD["%s_%s" % (tag, key)][i], (NAMES[i], tag, key, cnt[key], GOLD["%s_%s" % (tag, key)][i])


def test_the_fixture_holds_both_kinds_of_slots(cmod):
    assert len(PAIR) == 2 and len(FLOOR) == 3
    for i in PAIR:              # self-contacts, and line searches of more than one round
        _, cnt = _step(cmod, [i], ls_points=4, rep=1)
        assert cnt["selfcon"] > 0 and cnt["ls_evals"] > cnt["solver_iters"], (NAMES[i], cnt)
    for i in FLOOR:
        assert GOLD["ls4_rep1_solver_iters"][i] >= 40 and GOLD["ls4_rep1_ls_evals"][i] >= 2 * GOLD["ls4_rep1_solver_iters"][i], NAMES[i]


@pytest.mark.parametrize("tag,kw", CONFIGS)
def test_self_contact_states_are_bitwise_the_recorded_ones(cmod, tag, kw):
    _same_as_recorded(cmod, PAIR, tag, kw)


@pytest.mark.parametrize("tag,kw", CONFIGS)
def test_collapsed_floor_contact_states_are_bitwise_the_recorded_ones(cmod, tag, kw):
    _same_as_recorded(cmod, FLOOR, tag, kw)


def test_an_environment_alone_and_in_a_batch_of_five(cmod):
    """A self-contact state between floor-only ones: the batch of five gives every environment the numbers it has alone (and the fixture's)."""
    idx = [FLOOR[0], PAIR[0], FLOOR[1], PAIR[1], FLOOR[2]]
    kw = dict(ls_points=4, rep=4)
    batch, cnt = _step(cmod, idx, **kw)
    iters = evals = 0
    for row, i in enumerate(idx):
        alone, c1 = _step(cmod, [i], **kw)
        iters += c1["solver_iters"]; evals += c1["ls_evals"]
        for key in "qvw":
            assert np.array_equal(batch[key][row], alone[key][0]), (NAMES[i], key)
            assert np.array_equal(batch[key][row], GOLD["ls4_rep4_%s" % key][i]), (NAMES[i], key)
    assert (cnt["solver_iters"], cnt["ls_evals"]) == (iters, evals)
