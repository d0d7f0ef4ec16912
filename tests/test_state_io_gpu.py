"""
State on device buffers (include/locostate.h ls_get_state_device / ls_set_state_device / ls_restart_device, HipBatch.get_state_device /
set_state_device / restart_device; `-m gpu`): environments read, set and restarted from device memory, on a stream. 37 environments
(a partial last workgroup, state rows at multiples of 148 bytes), one case at n = 1. Every comparison is BITWISE unless it says
otherwise: a restart on request against a twin batch whose step kernel restarted the same environments itself and against the host
model of the draws (tests/step_bookkeeping_model.py); a set against a twin that took the host's lm_set_state / lm_set_goal /
lm_set_activation.
"""

import functools
import os

import numpy as np
import pytest

import step_bookkeeping_model as M
import test_rollout_tape_gpu as tp
import test_snapshot_gpu as sn
import test_step_bookkeeping_gpu as sb
import test_terminal_obs_gpu as tt
from loco_mujoco_amd import LocoEnv

pytestmark = pytest.mark.gpu

N, OFFSET, SEED = 37, 1000, 5
HORIZON = sn.RESTARTS["horizon"]
SCALE = 0.3                 # actions from U(-0.3, 0.3): three control steps from a dataset state leave nearly every robot upright
FILL = tp.OBS_FILL
FORCES = "HumanoidTorque.walk+forces"      # foot forces in the observation (the task of tests/test_terminal_obs_gpu.py)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _task(task):
    return tt._task(task[:-len("+forces")], True) if task.endswith("+forces") else tp._task(task)


def _gids(n=N):
    return OFFSET + np.arange(n)


def _table5(task):
    _, _, tab = _task(task)
    return np.ascontiguousarray(tab[np.linspace(0, len(tab) - 1, sn.RESTARTS["table_rows"]).astype(int)], dtype=np.float32)


def _start(task, n=N):
    _, _, tab = _task(task)
    return tab[np.random.RandomState(3).randint(0, len(tab), n)]


def _new(task, n=N, table=None, horizon=None):
    """A batch on the start rows; `table`: a reset table under (SEED, OFFSET); `horizon` not None: device-side restarts on."""
    from loco_mujoco_amd.backend import HipBatch
    env, hm, _ = _task(task)
    b = HipBatch(hm, n)
    tt._load(b, env, _start(task, n))
    if table is not None:
        b.set_reset_table(table, seed=SEED, global_env_offset=OFFSET)
    if horizon is not None:
        b.set_auto_reset(True, horizon=horizon)
    return b


def _acts(task, n, steps):
    env, _, _ = _task(task)
    return np.random.default_rng(1234).uniform(-SCALE, SCALE, (steps, n, len(env._action_indices))).astype(np.float32)


def _step(b, act, stream=None, sync=True):
    """One lm_step_device into fresh sentinel-filled tensors; returns them (torch)."""
    torch, dev = _torch()
    obs = torch.full((b.n, b.nobs), FILL, dtype=torch.float32, device=dev)
    rew = torch.full((b.n,), FILL, dtype=torch.float32, device=dev)
    done = torch.full((b.n,), tp.DONE_FILL, dtype=torch.uint8, device=dev)
    if sync:
        torch.cuda.synchronize(dev)
    b.step_device(action=act, obs=obs, reward=rew, done=done, stream=stream, sync=sync)
    return obs, rew, done


def _state_tensors(b, stream=None, sync=True):
    torch, dev = _torch()
    f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
    out = dict(qpos=torch.full((b.n, b.nv), FILL, **f32), qvel=torch.full((b.n, b.nv), FILL, **f32), ep_step=torch.full((b.n,), -7, **i32),
               ep_count=torch.full((b.n,), -7, **i32))
    if b.ngoal:
        out["goal"] = torch.full((b.n, b.ngoal), FILL, **f32)
    if b.na:
        out["act"] = torch.full((b.n, b.na), FILL, **f32)
    if sync:
        torch.cuda.synchronize(dev)
    b.get_state_device(stream=stream, sync=sync, **out)
    return out


def _state(b):
    """The whole state through ls_get_state_device, on the host; qpos / qvel also against lm_get_state."""
    out = {k: v.cpu().numpy() for k, v in _state_tensors(b).items()}
    q, v = b.get_state()
    tp._same(out["qpos"], q, "get_state_device qpos vs get_state")
    tp._same(out["qvel"], v, "get_state_device qvel vs get_state")
    return out


def _same_state(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        tp._same(a[k], b[k], "%s: %s" % (what, k))


# ---- 1. a restart on request is the kernel's restart
@functools.lru_cache(maxsize=None)
def _restart_twins(task):
    """Twin A restarts on the device at horizon 3, twin B only where a robot falls (horizon 0); both take the same three steps. The
    environments whose episode A's kernel ended and B's did not are then restarted in B on request. A continues under B's setting
    (horizon 0) for two more steps: an environment that fell in both twins before would otherwise reach A's horizon inside them."""
    torch, dev = _torch()
    env, _, _ = _task(task)
    table = _table5(task)
    acts = _dev(_acts(task, N, 5))
    A, B = _new(task, table=table, horizon=HORIZON), _new(task, table=table, horizon=0)
    for t in range(3):
        oa, ra, da = _step(A, acts[t])
        ob, rb, db = _step(B, acts[t])
    mask = ((da & 2) != 0) & ((db & 2) == 0)
    before = _state(B)
    obs_b = torch.full((N, B.nobs), FILL, dtype=torch.float32, device=dev)
    B.restart_device(mask, obs=obs_b)
    out = dict(env=env, table=table, mask=mask.cpu().numpy(), before=before, state_a=_state(A), state_b=_state(B), obs_a3=oa.cpu().numpy(),
               obs_b=obs_b.cpu().numpy(), later=[])
    A.set_auto_reset(True, horizon=0)
    for t in (3, 4):
        sa, sb_ = _step(A, acts[t]), _step(B, acts[t])
        out["later"].append(([x.cpu().numpy() for x in sa], [x.cpu().numpy() for x in sb_], _state(A), _state(B)))
    A.close(); B.close()
    return out


@pytest.mark.parametrize("task", ["UnitreeA1.simple", "Atlas.walk"])
def test_restart_on_request_is_the_kernels_restart(task):
    r = _restart_twins(task)
    mask, nv = r["mask"], r["env"]._model.nv
    print("%s: %d of %d environments restarted on request" % (task, mask.sum(), N))
    assert mask.sum() >= 30                                   # not vacuous: at this action scale nearly every episode runs into the horizon
    _same_state(r["state_b"], r["state_a"], "after the restart")
    tp._same(r["obs_b"][mask], r["obs_a3"][mask], "observation rows of the restarted environments")
    assert (r["obs_b"][~mask] == FILL).all()
    # ... and what the host model of the draws says: episode count + 1, the row drawn under (seed, global id, that count)
    count = r["before"]["ep_count"].astype(np.int64)
    row = np.asarray(M.restart_row(SEED, _gids(), count + 1, len(r["table"]))).astype(np.int64)
    rows = r["table"][row]
    got = r["state_b"]
    assert np.array_equal(got["qpos"][mask], rows[mask, :nv]) and np.array_equal(got["qvel"][mask], rows[mask, nv:2 * nv])
    if "goal" in got:
        assert np.array_equal(got["goal"][mask], rows[mask, 2 * nv:])
    assert np.array_equal(got["ep_count"][mask], count[mask] + 1) and not got["ep_step"][mask].any()
    assert len(set(row[mask])) >= 3                           # several rows of the five were drawn
    for k in got:                                             # the others keep everything
        tp._same(got[k][~mask], r["before"][k][~mask], "unmasked " + k)
    for (oa, ra, da), (ob, rb, db), sa, sb_ in r["later"]:
        tp._same(ob, oa, "obs of a later step"); tp._same(rb, ra, "reward of a later step"); tp._same(db, da, "done of a later step")
        _same_state(sb_, sa, "after a later step")
    assert not np.array_equal(r["later"][0][0][0], r["obs_a3"])          # the later steps moved


# ---- 2. rows decide the model
def test_restart_on_request_puts_the_environment_on_the_rows_model():
    """Talos.carry: four weights as four variants, the reset table one block of rows per weight (lm_set_variant_rows). After
    restart_device the variant of a masked environment is restart_row(...) // rows_per_variant; the others keep theirs."""
    np.random.seed(0)
    env = LocoEnv.make("Talos.carry", debug=True, n_envs=N)
    env.reset()
    assert env._pooled
    env._select_model(0)
    rpv = len(env._reset_table())
    env.enable_auto_reset(seed=SEED, horizon=1000, global_env_offset=OFFSET)
    env.step(np.zeros((N, 12)))                               # (uploads the host's pending state)
    b = env.backend
    before, count = b.get_variant_index().astype(np.int64), _state(b)["ep_count"].astype(np.int64)
    mask = np.arange(N) % 3 != 1
    b.restart_device(_dev(mask))
    row = np.asarray(M.restart_row(SEED, _gids(), count + 1, 4 * rpv)).astype(np.int64)
    want = np.asarray(M.variant_of_row(row, rpv)).astype(np.int64)
    after = b.get_variant_index().astype(np.int64)
    assert np.array_equal(after[mask], want[mask]) and np.array_equal(after[~mask], before[~mask])
    assert len(set(want[mask])) >= 3 and (want[mask] != before[mask]).any()
    assert np.array_equal(_state(b)["ep_count"], np.where(mask, count + 1, count))
    env.stop()


# ---- 3. joint parameters are redrawn
@pytest.mark.parametrize("task", ["UnitreeA1.simple", "Atlas.walk"])
def test_restart_on_request_redraws_the_joint_parameters(task):
    """The spec of test_step_bookkeeping_gpu._redraw_spec: on the mask every drawn entry is dof_redraw(seed, OFFSET + e, 1, dof, p, ...)
    within that file's _redraw_bound (the bound the in-kernel redraw is held to; contraction may differ between two kernels), kind-0
    entries and everything off the mask are bitwise what was uploaded. Printed, not asserted: whether the values are bitwise those of
    a twin whose step kernel restarted (horizon 1)."""
    env, _, tab = _task(task)
    nv = env._model.nv
    rs = np.random.RandomState(6)
    up = [rs.uniform(0.05, 0.5, (N, nv)).astype(np.float32) for _ in range(3)]
    spec = sb._redraw_spec(nv)
    table = np.ascontiguousarray(tab, dtype=np.float32)

    def batch(horizon):
        b = _new(task, table=table, horizon=horizon)
        b.set_dof_params(damping=up[0], stiffness=up[1], frictionloss=up[2])
        b.set_dof_randomization(spec)
        return b

    b = batch(None)
    mask = np.arange(N) % 4 != 2
    b.restart_device(_dev(mask))
    got = b.get_dof_params()
    twin = batch(1)
    tt._raw_step(twin, np.zeros((N, twin.nu)))
    kernel = twin.get_dof_params()
    worst, drawn, bitwise = 0.0, 0, True
    for p, name in enumerate(("damping", "stiffness", "frictionloss")):
        assert np.array_equal(got[name][~mask], up[p][~mask]), name
        for d in range(nv):
            kind, a, bb = int(spec[p, d, 0]), float(spec[p, d, 1]), float(spec[p, d, 2])
            g = got[name][mask, d]
            if kind == 0:
                assert np.array_equal(g, up[p][mask, d]), (name, d)
                continue
            raw = np.asarray(M.dof_redraw(SEED, _gids()[mask], 1, d, p, kind, a, bb, clip=False))
            bound = sb._redraw_bound(kind, a, bb)
            err = np.abs(g.astype(np.float64) - (raw if kind == 2 else np.maximum(raw, 0.0)))
            assert err.max() <= bound, (name, d, kind, float(err.max()), bound)
            if kind != 2:
                assert (g[raw < -bound] == 0.0).all() and (g >= 0.0).all()
            worst, drawn = max(worst, err.max() / bound), drawn + len(g)
            bitwise = bitwise and np.array_equal(g, kernel[name][mask, d])
    print("%s joint-parameter redraw on request: %d draws, largest error %.3f of the bound; bitwise the step kernel's: %s" % (task, drawn, worst, bitwise))
    assert drawn > N * nv


# ---- 4. the model compiler
def test_restart_on_request_compiles_the_models_the_kernels_restart_would():
    """Talos.walk under tests/golden/dr_talos_inertial.yaml (the configuration of test_variant_redraw_is_the_models) with the model
    compiler: after restart_device of the environments twin A's kernel restarted, draws and generations equal A's."""
    from loco_mujoco_amd import lowering
    from loco_mujoco_amd.backend import HipBatch, HipModel
    from loco_mujoco_amd.utils.domain_randomization import JointRandomization
    np.random.seed(0)
    env = LocoEnv.make("Talos.walk", debug=True)
    jr = JointRandomization(env._model, os.path.join(os.path.dirname(__file__), "golden", "dr_talos_inertial.yaml"))
    ib, db, _ = lowering.model_compiler_tables(env._model, env._device_task(), *jr.model_draw_ops())
    nominal = env._chain_model()
    tabs = lowering.variant_tables(nominal, nominal)
    hm = HipModel(nominal)
    tab, nv = env._reset_table(), env._model.nv
    rows = tab[(np.arange(N) * 7) % len(tab)]

    def batch(horizon):
        b = HipBatch(hm, N)
        b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
        b.set_reset_table(tab, seed=SEED, global_env_offset=OFFSET)
        b.set_auto_reset(True, horizon=horizon)
        b.set_model_compiler((ib, db), tabs, seed=3)
        return b

    A, B = batch(HORIZON), batch(0)
    for t in range(HORIZON):
        da = tt._raw_step(A, np.zeros((N, A.nu)))[2]
        db_ = tt._raw_step(B, np.zeros((N, B.nu)))[2]
    mask = ((da & 2) != 0) & ((db_ & 2) == 0)
    assert mask.sum() >= 30
    d0, g0 = B.get_model_draws()
    B.restart_device(_dev(mask))
    (da_, ga), (dd, gb) = A.get_model_draws(), B.get_model_draws()
    assert np.array_equal(dd, da_) and np.array_equal(gb, ga)
    assert np.array_equal(gb[mask], g0[mask] + 1) and np.array_equal(gb[~mask], g0[~mask])
    assert (dd[mask] != d0[mask]).any(1).all() and np.array_equal(dd[~mask], d0[~mask])
    _same_state(_state(B), _state(A), "after the restart")
    A.set_auto_reset(True, horizon=0)                          # (B's setting, as in _restart_twins)
    oa, ob = tt._raw_step(A, np.zeros((N, A.nu))), tt._raw_step(B, np.zeros((N, B.nu)))      # the fresh models step alike
    for x, y, what in zip(ob, oa, ("obs", "reward", "done")):
        tp._same(x, y, what + " of the step on the fresh models")


# ---- 5. set equals the host's set
def _set_case(task, with_act):
    """X takes set_state_device, its twin Y the host's set_state / set_goal / set_activation with the same mask, both after two steps."""
    torch, dev = _torch()
    env, _, tab = _task(task)
    nv = env._model.nv
    acts = _dev(_acts(task, N, 3))
    X, Y = _new(task), _new(task)
    for t in range(2):
        _step(X, acts[t]); _step(Y, acts[t])
    rs = np.random.RandomState(7)
    mask = rs.rand(N) < 0.5
    rows = np.ascontiguousarray(tab[rs.randint(0, len(tab), N)], dtype=np.float32)
    q, v, g = rows[:, :nv], rows[:, nv:2 * nv], rows[:, 2 * nv:]
    a = rs.uniform(0.1, 0.9, (N, X.na)).astype(np.float32) if with_act else None
    old = _state(X)
    obs = torch.full((N, X.nobs), FILL, dtype=torch.float32, device=dev)
    X.set_state_device(_dev(q), _dev(v), act=_dev(a) if with_act else None, goal=_dev(g) if X.ngoal else None, mask=_dev(mask), obs=obs)
    Y.set_state(q, v, mask)
    if Y.ngoal:
        Y.set_goal(g, mask)
    if with_act:
        Y.set_activation(a, mask)
    return env, X, Y, mask, rows, a, old, obs.cpu().numpy(), acts[2]


@pytest.mark.parametrize("task,with_act", [("UnitreeA1.simple", False), ("HumanoidMuscle.run", False), ("HumanoidMuscle.run", True), (FORCES, False)])
def test_set_from_device_rows_is_the_hosts_set(task, with_act):
    env, X, Y, mask, rows, a, old, obs, act = _set_case(task, with_act)
    assert 8 <= mask.sum() <= N - 8
    nv, ngrf = env._model.nv, (env._get_grf_size() if task == FORCES else 0)
    new = _state(X)
    _same_state(new, _state(Y), "after the set")
    assert np.array_equal(new["qpos"][mask], rows[mask, :nv]) and np.array_equal(new["qvel"][mask], rows[mask, nv:2 * nv])
    if "goal" in new:
        assert np.array_equal(new["goal"][mask], rows[mask, 2 * nv:])
    assert not new["ep_step"][mask].any() and old["ep_step"].all() and np.array_equal(new["ep_count"], old["ep_count"])
    for k in new:
        tp._same(new[k][~mask], old[k][~mask], "unmasked " + k)
    assert not np.array_equal(new["qpos"][mask], old["qpos"][mask])
    if X.na:
        assert old["act"].any(1).all()                           # two steps in: every environment has activations
        assert np.array_equal(new["act"][mask], a[mask]) if with_act else not new["act"][mask].any()
    # the observation written: the columns of the rows, foot forces 0; only the masked rows
    want = sb._obs_of_rows(env, rows)
    assert X.nobs == want.shape[1] + ngrf and (task != FORCES or ngrf > 0)
    assert np.array_equal(obs[mask, :X.nobs - ngrf], want[mask]) and not obs[mask, X.nobs - ngrf:].any()
    assert (obs[~mask] == FILL).all()
    sx, sy = _step(X, act), _step(Y, act)
    for x, y, what in zip(sx, sy, ("obs", "reward", "done")):
        tp._same(x.cpu().numpy(), y.cpu().numpy(), what + " of the step after the set")
    _same_state(_state(X), _state(Y), "after the step after the set")
    tp._same(X.flags(), Y.flags(), "flags")
    X.close(); Y.close()


def test_set_without_obs_writes_the_batchs_own_row():
    """obs None: the observation rows go to the batch's own last-step row (the convention of lm_step_device), which a policy
    rollout with obs0 None starts from — here read back by a rollout of zero-weight layers whose first action is a bias of the row."""
    torch, dev = _torch()
    from loco_mujoco_amd.backend import MlpPolicy
    task = "UnitreeA1.simple"
    env, _, tab = _task(task)
    nv = env._model.nv
    b = _new(task)
    b.step_device(action=None)                                 # the own row now holds a step's observation
    rows = np.ascontiguousarray(tab[np.random.RandomState(9).randint(0, len(tab), N)], dtype=np.float32)
    b.set_state_device(_dev(rows[:, :nv]), _dev(rows[:, nv:2 * nv]), goal=_dev(rows[:, 2 * nv:]) if b.ngoal else None)
    # a one-layer policy: action k = observation column k (identity block, zero bias)
    w = np.zeros((b.nu, b.nobs), dtype=np.float32)
    w[np.arange(b.nu), np.arange(b.nu)] = 1.0
    params = _dev(np.concatenate([w.ravel(), np.zeros(b.nu, dtype=np.float32)]))
    actions = b.rollout_policy(MlpPolicy((b.nobs, b.nu), "tanh", params), 1)
    want = sb._obs_of_rows(env, rows)[:, :b.nu]
    tp._same(actions[0].cpu().numpy(), want, "the first action = the own row's first columns")
    b.close()


# ---- 6. stream order
def test_calls_queued_on_a_stream_equal_the_synchronous_sequence():
    """step -> restart -> step -> get on a non-default torch stream with sync=False throughout and ONE synchronise at the end,
    against the same sequence run synchronously on a twin."""
    torch, dev = _torch()
    task = "UnitreeA1.simple"
    table = _table5(task)
    acts = _dev(_acts(task, N, 2))
    mask = _dev(np.arange(N) % 2 == 0)
    A, B = _new(task, table=table), _new(task, table=table)
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        s = side.cuda_stream
        _step(A, acts[0], stream=s, sync=False)
        ra = torch.full((N, A.nobs), FILL, dtype=torch.float32, device=dev)
        A.restart_device(mask, obs=ra, stream=s, sync=False)
        sa = _step(A, acts[1], stream=s, sync=False)
        got = _state_tensors(A, stream=s, sync=False)
    side.synchronize()
    _step(B, acts[0])
    rb = torch.full((N, B.nobs), FILL, dtype=torch.float32, device=dev)
    B.restart_device(mask, obs=rb)
    sb_ = _step(B, acts[1])
    want = _state_tensors(B)
    tp._same(ra.cpu().numpy(), rb.cpu().numpy(), "restart observation")
    for x, y, what in zip(sa, sb_, ("obs", "reward", "done")):
        tp._same(x.cpu().numpy(), y.cpu().numpy(), what)
    _same_state({k: v.cpu().numpy() for k, v in got.items()}, {k: v.cpu().numpy() for k, v in want.items()}, "queued vs synchronous")
    assert not (got["ep_step"].cpu().numpy() == -7).any()
    A.close(); B.close()


# ---- 7. masks
def test_mask_of_zeros_changes_nothing_and_null_is_all():
    torch, dev = _torch()
    task = "UnitreeA1.simple"
    env, _, tab = _task(task)
    nv = env._model.nv
    table = _table5(task)
    acts = _dev(_acts(task, N, 2))
    A, B, C = _new(task, table=table), _new(task, table=table), _new(task, table=table)
    for b in (A, B, C):
        _step(b, acts[0])
    before = _state(A)
    obs = torch.full((N, A.nobs), FILL, dtype=torch.float32, device=dev)
    none = torch.zeros(N, dtype=torch.uint8, device=dev)
    rows = np.ascontiguousarray(tab[:N], dtype=np.float32)
    A.restart_device(none, obs=obs)
    A.set_state_device(_dev(rows[:, :nv]), _dev(rows[:, nv:2 * nv]), goal=_dev(rows[:, 2 * nv:]) if A.ngoal else None, mask=none, obs=obs)
    _same_state(_state(A), before, "no mask byte set")
    assert (obs.cpu().numpy() == FILL).all()
    # NULL = every byte set (uint8 255 and bool alike)
    ob, oc = torch.full_like(obs, FILL), torch.full_like(obs, FILL)
    B.restart_device(None, obs=ob)
    C.restart_device(torch.full((N,), 255, dtype=torch.uint8, device=dev), obs=oc)
    _same_state(_state(B), _state(C), "NULL mask vs all set")
    tp._same(ob.cpu().numpy(), oc.cpu().numpy(), "NULL mask vs all set: observation")
    assert not (ob.cpu().numpy() == FILL).any() and np.array_equal(_state(B)["ep_count"], before["ep_count"] + 1)
    # ... and A, which the zero masks left untouched, restarted now (a bool mask) steps on as B
    A.restart_device(torch.ones(N, dtype=torch.bool, device=dev))
    for x, y, what in zip(_step(A, acts[1]), _step(B, acts[1]), ("obs", "reward", "done")):
        tp._same(x.cpu().numpy(), y.cpu().numpy(), what)
    for b in (A, B, C):
        b.close()


def test_a_batch_of_one_environment():
    torch, dev = _torch()
    task = "UnitreeA1.simple"
    env, _, tab = _task(task)
    nv = env._model.nv
    table = _table5(task)
    b = _new(task, n=1, table=table)
    obs = torch.full((1, b.nobs), FILL, dtype=torch.float32, device=dev)
    for ec in (1, 2, 3):
        b.restart_device(torch.ones(1, dtype=torch.bool, device=dev), obs=obs)
        st = _state(b)
        row = table[int(M.restart_row(SEED, OFFSET, ec, len(table)))][None]
        assert np.array_equal(st["qpos"], row[:, :nv]) and np.array_equal(st["qvel"], row[:, nv:2 * nv]) and st["ep_count"][0] == ec
        tp._same(obs.cpu().numpy(), sb._obs_of_rows(env, row), "observation of the row")
    q = _dev(tab[7:8, :nv].astype(np.float32))
    b.set_state_device(q, _dev(tab[7:8, nv:2 * nv].astype(np.float32)))
    assert np.array_equal(_state(b)["qpos"], tab[7:8, :nv].astype(np.float32)) and _state(b)["ep_count"][0] == 3
    b.close()


# ---- 8. refusals
def test_refused_calls_leave_the_batch_as_it_was():
    from loco_mujoco_amd.backend import BackendError
    torch, dev = _torch()
    task = "UnitreeA1.simple"
    acts = _dev(_acts(task, N, 2))
    A, B = _new(task), _new(task)
    for b in (A, B):
        _step(b, acts[0])
    before = _state(A)
    q, v = _dev(before["qpos"] + 1.0), _dev(before["qvel"])
    with pytest.raises(BackendError, match="reset table"):
        A.restart_device(torch.ones(N, dtype=torch.bool, device=dev))
    assert A.na == 0
    with pytest.raises(BackendError, match="no activation states"):
        A.set_state_device(q, v, act=torch.zeros((N, 3), dtype=torch.float32, device=dev))
    with pytest.raises(BackendError, match="no activation states"):
        A.get_state_device(qpos=q, act=torch.zeros((N, 3), dtype=torch.float32, device=dev))
    with pytest.raises(BackendError, match="every output is null"):
        A.get_state_device()
    with pytest.raises(ValueError, match="qvel is None"):
        A.set_state_device(q, None)
    _same_state(_state(A), before, "after the refused calls")
    for x, y, what in zip(_step(A, acts[1]), _step(B, acts[1]), ("obs", "reward", "done")):
        tp._same(x.cpu().numpy(), y.cpu().numpy(), what)
    _same_state(_state(A), _state(B), "the step after the refused calls")
    A.close(); B.close()
