"""
The models of the generic kernel family (lm_families.h LM_GENERIC_FAMILY: cone and chain length read at run time, plain layout, no
replay kernel), shared by tests/test_generic_family_host.py and tests/test_generic_family_gpu.py: a shipped task whose compiled model
is edited in memory — another integrator, another cone — so that no specialised family fits it. One case per instance a model reaches.
"""

import functools

import numpy as np

from loco_mujoco_amd import LocoEnv, lowering, mjcf

GENERIC_FAMILY = 6
N = 37                        # tests/test_plain_layout_gpu.py: the states, actions and rule of its _case


def _rk4(m):
    m.integrator = 1


def _elliptic(m):
    m.cone = mjcf.CONE_ELLIPTIC


def _pyramidal_condim3(m):
    m.cone = mjcf.CONE_PYRAMIDAL
    m.geom_condim = np.full_like(m.geom_condim, 3)


# key: (task, edit of the compiled model, the option the edit changes, instance <links, slots, RK4>, oracle without self-collisions)
# The lowering carries no self-collision tables under an elliptic cone (lowering.py: the pair tables are built for condim-3 pyramids),
# so HumanoidTorque and UnitreeH1 are compared with the oracle's self-collisions switched off, as HumanoidMuscle.run.nopairs is.
CASES = {
    "UnitreeA1.rk4": ("UnitreeA1.simple", _rk4, "integrator", (3, 4, True), False),
    "UnitreeA1.pyramidal3": ("UnitreeA1.simple", _pyramidal_condim3, "cone", (3, 4, False), False),
    "Talos.elliptic": ("Talos.walk", _elliptic, "cone", (5, 8, False), False),
    "Atlas.elliptic": ("Atlas.walk", _elliptic, "cone", (5, 8, True), False),
    "HumanoidTorque.elliptic": ("HumanoidTorque.run", _elliptic, "cone", (5, 8, True), True),
    "UnitreeH1.elliptic": ("UnitreeH1.run", _elliptic, "cone", (5, 8, False), True),
}


def edited_env(key):
    """The task's environment with its compiled model edited in memory (tests/test_gpu_parity.py
    test_joint_parameters_on_a_generic_kernel_family_fail_at_the_call)."""
    task, edit = CASES[key][:2]
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    edit(env._model)
    return env


def oracle_for(key, model):
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    o = Oracle(pack_model(model))
    if CASES[key][4]:
        o.set_option("disable_self_collision", 1)
    return o


@functools.lru_cache(maxsize=None)
def inputs(key):
    """The edited environment, its lowering and the 37 states and actions of test_plain_layout_gpu._case (dataset rows under
    RandomState(11), actions from U(-0.3, 0.3)) — no oracle pass. Read-only."""
    env = edited_env(key)
    cm = env._chain_model()
    tab = env._reset_table()
    rs = np.random.RandomState(11)
    rows = np.ascontiguousarray(tab[rs.randint(0, len(tab), N)], dtype=np.float32)
    acts = rs.uniform(-0.3, 0.3, (N, len(env._action_indices)))
    return dict(name=key, env=env, m=env._model, cm=cm, cm_full=cm, tab=tab, rows=rows, acts=acts)


def shipped_oracle(key):
    """The oracle of the same task as shipped (the edit not made), with the same self-collision switch."""
    task = CASES[key][0]
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    return oracle_for(key, env._model)


def ctrl_of(c, i):
    env, m = c["env"], c["m"]
    ctrl = np.zeros(m.nu)
    ctrl[env._action_indices] = env._preprocess_action(c["acts"][i])
    return ctrl
