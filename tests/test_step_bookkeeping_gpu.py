"""
The step kernel's bookkeeping against its host model (tests/step_bookkeeping_model.py; `-m gpu`), at tiny shapes and exact wherever the
rule is integer arithmetic:
  a. which reset-table row a device-side restart draws (lm_step, the replay kernel, the plain layout, active lists, lm_rollout,
     lm_rollout_fused);
  b. which model variant it draws, independently of the row and as the row's block;
  c. the joint parameters it draws, every kind, dof and parameter, to a derived number of float32 ulps;
  d. lm_rollout's random policy: the same simulation as lm_step fed the model's numbers, and its statistics;
  e. reward (taken on the previous observation, across restarts) and the absorbing bit on those per-step outputs;
  f. actions beyond [-1, 1]: the kernel's ctrl clamp against the fp64 oracle.
"""

import functools

import numpy as np
import pytest

import step_bookkeeping_model as M
from loco_mujoco_amd import LocoEnv
from test_terminal_obs_gpu import GENERIC, N_PUSHED, _load, _raw_step, _start_rows, _task

pytestmark = pytest.mark.gpu

# (GENERIC: the quadruped under RK4 — the generic kernel family: one layout, no fused kernels, a rollout runs one control step per launch)
FAMILIES = ["UnitreeA1.simple", "Atlas.walk", "Talos.walk", "HumanoidTorque.run", "HumanoidMuscle.run", "UnitreeG1.walk", GENERIC]
N = 37                       # nine full workgroups of four environments and a padded one
OFFSET = 1000                # global_env_offset: the draws are keyed by OFFSET + e
SEED = 5
N_ROWS = 257
T_RESTART = 5
QTOL, VTOL = 1e-4, 1e-2      # the stated fp32 tolerance of one control step (test_gpu_parity.py)


def _gids(n):
    return OFFSET + np.arange(n)


def _obs_columns(env):
    """(dofs behind the qpos columns, dofs behind the qvel columns, goal columns) of the kernel's observation [q | v | goal]."""
    t = env._device_task()
    return np.array(t["qpos_obs_idx"]), np.array(t["qvel_obs_idx"]), int(t["n_goal"])


def _obs_of_rows(env, rows):
    """The observation of the states in `rows` [qpos | qvel | goal] (no foot forces), float32 like the kernel's."""
    qi, vi, ng = _obs_columns(env)
    nv = env._model.nv
    r = np.asarray(rows, dtype=np.float32)
    return np.concatenate([r[:, qi], r[:, nv + vi], r[:, 2 * nv:2 * nv + ng]], axis=1)


def _table257(env, tab):
    """A reset table of 257 pairwise distinct rows (257 is prime: no power of two, no multiple of a workgroup). The datasets the tests
    run on are short — 100 samples for the humanoids, 300 for the quadruped with repeated ones among the first 257 — so the task's
    rows are cycled to 257 and row k gets k millimetres as its root x position (dof 0, which no observation column shows; at horizon 1
    every check is a copy of the row, so the tag's effect on a step does not matter): a row identifies itself."""
    qi = _obs_columns(env)[0]
    assert 0 not in qi                                      # root x is not observed: the observation checks below do not see the tag
    rows = np.ascontiguousarray(tab[np.arange(N_ROWS) % len(tab)], dtype=np.float32)
    rows[:, 0] = (0.001 * np.arange(N_ROWS)).astype(np.float32)
    assert len(rows) == N_ROWS and len(np.unique(rows, axis=0)) == N_ROWS
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# a. the restart row
# ------------------------------------------------------------------------------------------------------------------------------

def _restart_batch(task, mode):
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task(task)
    table = _table257(env, tab)
    start = tab[(N_ROWS + 3 * np.arange(N)) % len(tab)]
    b = HipBatch(hm, N, envs_per_workgroup=int(mode[5:]) if mode.startswith("plain") else None)      # "plain16" / "plain8": the width
    if mode == "replay":
        b.set_replay(2)
    _load(b, env, start)
    b.set_reset_table(table, seed=SEED, global_env_offset=OFFSET)
    b.set_auto_reset(True, horizon=1)
    return env, b, table, start.astype(np.float32)


def _wanted_rows(seed_eff):
    want = np.stack([M.restart_row(seed_eff, _gids(N), t, N_ROWS) for t in range(1, T_RESTART + 1)]).astype(np.int64)      # [t][e]
    assert min(len(set(want[:, e])) for e in range(N)) >= 3                            # not vacuous: three different rows per environment
    return want


# (HumanoidMuscle.run at 16 environments per workgroup is not here: its plain kernel needs 13 400 B of static LDS (the muscle table) +
# 155 648 B of dynamic LDS = 169 048 B, a compute unit has 163 840 B. The launch asked for the dynamic part alone, was made, and ended in
# an illegal memory access; lm_batch_set_layout now refuses that layout with these numbers — tests/test_plain_layout_gpu.py — and
# no test launches it. At 8 per workgroup the kernel takes 95 704 B: "plain8")
_STEP_CASES = ([(t, "step") for t in FAMILIES] + [(t, "replay") for t in ("HumanoidTorque.run", "HumanoidMuscle.run")]
               + [(t, "plain16") for t in FAMILIES if t not in (GENERIC, "HumanoidMuscle.run")] + [("HumanoidMuscle.run", "plain8")]
               + [(t, "active") for t in FAMILIES if t != "UnitreeA1.simple"])              # (the quadruped family's kernels have no active lists; the generic ones do)


@pytest.mark.parametrize("task,mode", _STEP_CASES)
def test_restart_row_is_the_models(task, mode):
    """horizon 1: every control step ends every episode. After step t environment e holds row restart_row(seed, OFFSET + e, t, 257) of
    the float32 table, bit for bit: state, goal and q / v columns of the observation; done bit 1 is set; muscle activations are zero.
    Through lm_step's regular kernel, the replay kernel, the plain layout (16 environments per workgroup; the muscle humanoid: 8) and an active list of
    every third environment — the listed ones draw by their global id, the others keep their state bitwise."""
    env, b, table, start = _restart_batch(task, mode)
    nv = env._model.nv
    ng = _obs_columns(env)[2]
    active = np.arange(0, N, 3) if mode == "active" else np.arange(N)
    rest = np.setdiff1d(np.arange(N), active)
    if mode == "active":
        b.set_active(active)
    want = _wanted_rows(SEED)
    rs = np.random.RandomState(1)
    for t in range(1, T_RESTART + 1):
        obs, rew, done = _raw_step(b, rs.uniform(-0.3, 0.3, (N, b.nu)))
        q, v = b.get_state()
        rows = table[want[t - 1]]
        assert np.array_equal(q[active], rows[active, :nv]) and np.array_equal(v[active], rows[active, nv:2 * nv]), (task, mode, t)
        assert np.array_equal(q[rest], start[rest, :nv]) and np.array_equal(v[rest], start[rest, nv:2 * nv])      # inactive: untouched
        if b.na:
            assert not b.get_activation()[active].any()
        assert ((done[active] & 2) != 0).all()
        assert np.array_equal(obs[active], _obs_of_rows(env, rows)[active]), (task, mode, t)
        if ng:
            assert np.array_equal(obs[active, b.nobs - ng:], rows[active, 2 * nv:])    # the goal columns are the row's goal
    if mode == "replay":
        assert b.replay_marks().all()


@pytest.mark.parametrize("spl", [1, 3])
@pytest.mark.parametrize("task", FAMILIES)
def test_restart_row_after_a_rollout_is_the_models(task, spl):
    """lm_rollout and lm_rollout_fused (three control steps per launch; the generic family runs them one by one) draw under
    rollout_seed(batch seed, 9): the state after five control steps at horizon 1 is that model's fifth row."""
    env, b, table, _ = _restart_batch(task, "rollout")
    nv = env._model.nv
    want = _wanted_rows(M.rollout_seed(SEED, 9))
    assert not np.array_equal(want, _wanted_rows(SEED))
    st = b.rollout(T_RESTART, action_mode=1, seed=9, steps_per_launch=spl)
    q, v = b.get_state()
    rows = table[want[T_RESTART - 1]]
    assert np.array_equal(q, rows[:, :nv]) and np.array_equal(v, rows[:, nv:2 * nv]), (task, spl)
    if b.na:
        assert not b.get_activation().any()
    assert st["episodes"] == N * T_RESTART and st["env_steps"] == N * T_RESTART


# ------------------------------------------------------------------------------------------------------------------------------
# b. the variant redraw
# ------------------------------------------------------------------------------------------------------------------------------

def test_variant_redraw_is_the_models():
    """A pool of three variants (no power of two), horizon 1: after each of four steps every environment is on variant
    variant_draw(seed, OFFSET + e, t, 3) — a draw of its own beside the row draw."""
    import os
    from loco_mujoco_amd.backend import HipBatch
    cfg = os.path.join(os.path.dirname(__file__), "golden", "dr_talos_inertial.yaml")
    np.random.seed(0)
    env = LocoEnv.make("Talos.walk", debug=True, n_envs=N, domain_randomization_config=cfg, n_model_variants=3)
    env.reset()
    nv = env._model.nv
    tab = env._reset_table()
    env.backend                                             # (creates the HipModel)
    b = HipBatch(env._hip_model, N)
    b.set_model_variants(env._build_model_variants(env._chain_model())[1])
    assert b.n_variants == 3
    rows = tab[(np.arange(N) * 7) % len(tab)]
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    b.set_reset_table(tab, seed=SEED, global_env_offset=OFFSET)
    b.set_auto_reset(True, horizon=1)
    seen = []
    for t in range(1, 5):
        _raw_step(b, np.zeros((N, b.nu)))
        want = np.asarray(M.variant_draw(SEED, _gids(N), t, 3)).astype(np.int64)
        assert np.array_equal(b.get_variant_index().astype(np.int64), want), t
        seen.append(want)
    seen = np.stack(seen)
    assert set(seen.ravel()) == {0, 1, 2} and (seen[1:] != seen[:-1]).mean() > 0.4      # (a fresh draw of three differs with p = 2/3)


def test_variant_follows_the_restart_row():
    """Talos.carry: four weights as four variants, the reset table one block of rows per weight (lm_set_variant_rows). After each
    step at horizon 1 the variant is restart_row(...) // rows_per_variant and the observed weight column is that variant's."""
    np.random.seed(0)
    env = LocoEnv.make("Talos.carry", debug=True, n_envs=N)
    env.reset()
    assert env._pooled
    env._select_model(0)
    rpv = len(env._reset_table())
    weights = np.array([0.1, 1.0, 5.0, 10.0])
    env.enable_auto_reset(seed=SEED, horizon=1, global_env_offset=OFFSET)
    rs = np.random.RandomState(3)
    seen = set()
    for t in range(1, 5):
        o = env.step(rs.uniform(-0.3, 0.3, (N, 12)))[0]
        row = np.asarray(M.restart_row(SEED, _gids(N), t, 4 * rpv)).astype(np.int64)
        want = np.asarray(M.variant_of_row(row, rpv)).astype(np.int64)
        assert np.array_equal(env.backend.get_variant_index().astype(np.int64), want), t
        assert np.array_equal(o[:, -1].astype(np.float32), weights[want].astype(np.float32)), t
        seen.update(want.tolist())
    assert seen == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------------------------------------
# c. the joint-parameter redraw
# ------------------------------------------------------------------------------------------------------------------------------

_AB_CLIPS, _AB_CLEAR, _AB_UNIFORM = (0.1, 1.0), (2.0, 0.05), (0.2, 0.7)
ULP32 = 2.0 ** -23


def _redraw_spec(nv):
    """spec[3][nv][3] written by hand: the four kinds in turn over (dof, parameter) so that every dof — the six root dofs, every link
    of every chain — and every parameter meets each kind across the pattern; the normal kinds alternate between (0.1, 1.0), where the
    clip at 0 fires for 46 % of the draws, and (2.0, 0.05), 40 sigma above it."""
    spec = np.zeros((3, nv, 3), dtype=np.float32)
    for p in range(3):
        for d in range(nv):
            kind = (d + 2 * p + d // 4) % 4
            a, b = (0.0, 0.0) if kind == 0 else _AB_UNIFORM if kind == 2 else (_AB_CLIPS if (d + p) % 2 == 0 else _AB_CLEAR)
            spec[p, d] = (kind, a, b)
    return spec


def _redraw_bound(kind, a, b):
    """Derived, not measured: the device evaluates b * sqrt(-2 ln u1) * cos(2 pi u2) + a in float32 — logf, sqrtf and cosf at a few
    ulps each, one possible fma contraction, and |z| reaches 6 with a 24-bit u1 — 16 ulps of the largest magnitude in play,
    max(|a|, |b|, 6 |b|); the uniform kind is one multiply-add: 4 ulps of max(|a|, |b|)."""
    return 4 * ULP32 * max(abs(a), abs(b)) if kind == 2 else 16 * ULP32 * max(abs(a), abs(b), 6 * abs(b))


@pytest.mark.parametrize("task,kw", [("UnitreeA1.simple", {}), ("Atlas.walk", dict(disable_back_joint=False))])
def test_joint_parameter_redraw_is_the_models(task, kw):
    """n = 64, horizon 1, three steps; after each: kind-0 entries are bitwise what set_dof_params uploaded, every other entry is
    dof_redraw(seed, OFFSET + e, t, dof, p, ...) within the derived bound, and exactly 0.0 where the model's unclipped value lies
    below minus that bound (within the bound of 0 it may be either)."""
    from loco_mujoco_amd.backend import HipBatch, HipModel
    n = 64
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, **kw)
    nv = env._model.nv
    tab = env._reset_table()
    b = HipBatch(HipModel(env._chain_model()), n)
    _load(b, env, tab[(np.arange(n) * 3) % len(tab)])
    rs = np.random.RandomState(6)
    up = [rs.uniform(0.05, 0.5, (n, nv)).astype(np.float32) for _ in range(3)]
    b.set_dof_params(damping=up[0], stiffness=up[1], frictionloss=up[2])
    spec = _redraw_spec(nv)
    kinds = spec[:, :, 0].astype(int)
    assert all((kinds[:, :6] == k).any() and (kinds[p] == k).any() for k in range(4) for p in range(3))
    b.set_dof_randomization(spec)
    b.set_reset_table(tab, seed=SEED, global_env_offset=OFFSET)
    b.set_auto_reset(True, horizon=1)
    worst = 0.0
    n_clipped = n_drawn = 0
    for t in range(1, 4):
        _raw_step(b, np.zeros((n, b.nu)))
        got = b.get_dof_params()
        for p, name in enumerate(("damping", "stiffness", "frictionloss")):
            for d in range(nv):
                kind, a, bb = int(spec[p, d, 0]), float(spec[p, d, 1]), float(spec[p, d, 2])
                g = got[name][:, d]
                if kind == 0:
                    assert np.array_equal(g, up[p][:, d]), (t, name, d)
                    continue
                raw = np.asarray(M.dof_redraw(SEED, _gids(n), t, d, p, kind, a, bb, clip=False))
                bound = _redraw_bound(kind, a, bb)
                want = raw if kind == 2 else np.maximum(raw, 0.0)
                err = np.abs(g.astype(np.float64) - want)
                worst = max(worst, err.max() / bound)
                assert err.max() <= bound, (t, name, d, kind, float(err.max()), bound)
                if kind != 2:
                    assert (g[raw < -bound] == 0.0).all() and (g >= 0.0).all()
                    n_clipped += int((raw < -bound).sum())
                n_drawn += n
    print("%s joint-parameter redraw: %d draws, largest error %.3f of the bound, %d clipped to 0" % (task, n_drawn, worst, n_clipped))
    assert n_clipped > 0.1 * n_drawn / 3              # the clip fired: (0.1, 1.0) clips 46 % of about a quarter of the draws


# ------------------------------------------------------------------------------------------------------------------------------
# d, e. the random policy is lm_step fed the model's numbers; reward and absorbing bit of those steps
# ------------------------------------------------------------------------------------------------------------------------------

N_POLICY = 45


@functools.lru_cache(maxsize=None)
def _policy_runs(task, restarts):
    """Batch B: lm_steps fed random_action(effective seed, OFFSET + e, step, column) — computed once per (task, run) and shared by the
    tests below, which leave it unchanged. Without restarts: four steps under rollout_seed(SEED, 9), auto-reset off; with: six steps
    at horizon 2 under the batch's own seed (a rollout with seed argument 0). Returns what B saw and, for one and three control steps
    per launch, what a batch A left behind after rollout(...)."""
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task(task)
    n = N_POLICY
    rows, _ = _start_rows(env, tab, n)
    steps, rseed = (6, 0) if restarts else (4, 9)

    def batch():
        b = HipBatch(hm, n)
        _load(b, env, rows)
        b.set_reset_table(tab, seed=SEED, global_env_offset=OFFSET)
        b.set_auto_reset(bool(restarts), horizon=2 if restarts else 1000)
        return b

    B = batch()
    seed_eff = M.rollout_seed(SEED, rseed)
    g, k = np.meshgrid(_gids(n), np.arange(B.nu), indexing="ij")
    acts = [np.asarray(M.random_action(seed_eff, g, t, k), dtype=np.float32) for t in range(steps)]
    out = [_raw_step(B, a) for a in acts]
    res = dict(env=env, rows=rows, acts=acts, obs=[o for o, _, _ in out], rew=[r for _, r, _ in out], done=[d for _, _, d in out],
               state=B.get_state(), act=B.get_activation() if B.na else None, marks=B.replay_marks(), A={})
    for spl in (1, 3):
        A = batch()
        st = A.rollout(steps, action_mode=1, seed=rseed, steps_per_launch=spl)
        res["A"][spl] = dict(stats=st, state=A.get_state(), act=A.get_activation() if A.na else None, marks=A.replay_marks())
    return res


@pytest.mark.parametrize("spl", [1, 3])
@pytest.mark.parametrize("restarts", [False, True])
@pytest.mark.parametrize("task", FAMILIES)
def test_random_policy_rollout_is_lm_step_fed_the_models_actions(task, restarts, spl):
    """State and activations of A (rollout under the random policy) and B (lm_step fed the model's actions) are bitwise equal for every
    environment no control step of which went through the replay kernel in either batch (the rule of
    test_fused_rollout_is_bitwise_the_single_step_rollout), at least 90 % of them; B's last observation is the observation of A's
    final state. With restarts A's statistics are B's per-step outputs added up."""
    r = _policy_runs(task, restarts)
    env, n, A = r["env"], N_POLICY, r["A"][spl]
    acts = np.stack(r["acts"])
    assert acts.min() >= -1.0 and acts.max() < 1.0 and abs(acts.mean()) < 0.05 and len(np.unique(acts)) > 0.95 * acts.size
    same = ~(A["marks"] | r["marks"])
    print("%s restarts=%d steps_per_launch=%d: %d of %d environments unmarked" % (task, restarts, spl, same.sum(), n))
    assert same.sum() >= 0.9 * n
    (qa, va), (qb, vb) = A["state"], r["state"]
    assert np.array_equal(qa[same], qb[same]) and np.array_equal(va[same], vb[same])
    if A["act"] is not None:
        assert np.array_equal(A["act"][same], r["act"][same]) and (restarts or A["act"].any())
    qi, vi, ng = _obs_columns(env)
    last = r["obs"][-1]
    assert np.array_equal(last[same][:, :len(qi)], qa[same][:, qi]) and np.array_equal(last[same][:, len(qi):len(qi) + len(vi)], va[same][:, vi])
    st = A["stats"]
    steps = len(r["acts"])
    assert st["env_steps"] == n * steps and st["nan_resets"] == 0
    if restarts:
        ended = int(sum(((d & 2) != 0).sum() for d in r["done"]))
        assert ended >= n * (steps // 2)                       # horizon 2: every environment ended at least three episodes
        assert st["episodes"] == ended
        total = float(np.sum([x.astype(np.float64).sum() for x in r["rew"]]))
        assert abs(st["reward_sum"] - total) <= 1e-3 * abs(total), (st["reward_sum"], total)      # float32 block sums


@pytest.mark.parametrize("restarts", [False, True])
@pytest.mark.parametrize("task", FAMILIES)
def test_reward_and_absorbing_bit_of_the_steps(task, restarts):
    """On B's per-step outputs: reward_t is the environment's reward of the observation the PREVIOUS step returned (the start rows'
    before the first) within 1e-5 — after a restart that is the fresh episode's first observation, the quadruped's goal-velocity
    reward with the goal of the restart row. Without restarts done bit 0 is _has_fallen of the step's own observation, for twelve
    rows pushed across a termination bound and 33 dataset rows: both outcomes occur."""
    r = _policy_runs(task, restarts)
    env, n = r["env"], N_POLICY
    prev = _obs_of_rows(env, r["rows"])
    worst = 0.0
    fallen = upright = 0
    restarted = 0
    for t, (obs, rew, done) in enumerate(zip(r["obs"], r["rew"], r["done"])):
        want = np.array([env.reward(prev[e].astype(np.float64), None, None, False) for e in range(n)])
        worst = max(worst, np.abs(rew - want).max())
        assert np.abs(rew - want).max() < 1e-5, (task, t)
        if t > 0:
            restarted += int(((r["done"][t - 1] & 2) != 0).sum())
        if not restarts:
            has = np.array([bool(env._has_fallen(obs[e].astype(np.float64))) for e in range(n)])
            assert np.array_equal((done & 1) != 0, has), (task, t)
            fallen += int(has.sum()); upright += int((~has).sum())
        prev = obs
    print("%s restarts=%d: reward error %.2e; %d fallen / %d upright; %d rewards right after a restart" % (task, restarts, worst, fallen, upright, restarted))
    if restarts:
        assert restarted >= 2 * n
    else:
        assert fallen >= 8 and upright >= 8 and N_PUSHED == 12


# ------------------------------------------------------------------------------------------------------------------------------
# f. actions beyond the range
# ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task,kw", [("UnitreeA1.simple", {}), ("UnitreeA1.simple", dict(action_mode="position")), ("Atlas.walk", {})])
def test_actions_beyond_the_range_are_clamped_like_the_references(task, kw):
    """16 dataset states, actions from U(-3, 3) with column 0 exactly +-1, one control step against the fp64 oracle on the ctrl the
    reference's un-normalise-then-ctrlrange-clamp gives: the existing QTOL / VTOL."""
    from loco_mujoco_amd.backend import HipBatch, HipModel
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    n = 16
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, **kw)
    m = env._model
    oracle = Oracle(pack_model(m))
    tab = env._reset_table()
    rs = np.random.RandomState(8)
    rows = tab[rs.randint(0, len(tab), n)]
    acts = rs.uniform(-3, 3, (n, len(env._action_indices)))
    acts[:, 0] = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    lo, hi = m.act_ctrlrange[env._action_indices, 0], m.act_ctrlrange[env._action_indices, 1]
    assert np.asarray(m.act_ctrllimited)[env._action_indices].all()
    raw = np.stack([env._preprocess_action(a) for a in acts])
    assert ((raw < lo) | (raw > hi)).mean() >= 0.25 and (np.abs(acts) > 1).mean() >= 0.25       # a quarter and more reaches the clamp
    b = HipBatch(HipModel(env._chain_model()), n)
    _load(b, env, rows)
    _raw_step(b, acts)
    q, v = b.get_state()
    eq, ev = [], []
    for i in range(n):
        q0, v0 = rows[i, :m.nv].astype(np.float32).astype(np.float64), rows[i, m.nv:2 * m.nv].astype(np.float32).astype(np.float64)
        ctrl = np.zeros(m.nu)
        ctrl[env._action_indices] = np.clip(raw[i], lo, hi)
        qo, vo = oracle.step(q0, v0, ctrl, nsub=10)[:2]
        eq.append(np.abs(q[i] - qo).max()); ev.append(np.abs(v[i] - vo).max())
    print("%s %s, actions in [-3, 3] vs the oracle on clamped ctrl: qpos max %.2e qvel max %.2e" % (task, kw, max(eq), max(ev)))
    assert max(eq) < QTOL and max(ev) < VTOL
