"""
Device-side snapshots (include/locohip.h lm_snapshot_*, HipBatch.snapshot / restore / fork, LocoEnv.save_state / load_state; `-m gpu`):
save, rewind and fork the environments of a batch without leaving the device. Every comparison is BITWISE: a restored batch has to
continue exactly as the batch that was saved did, and exactly as a twin batch that never saved. Shapes and helpers are those of
tests/test_rollout_tape_gpu.py: 37 environments (a partial last workgroup, state rows that start at multiples of 148 bytes) or 64,
T = 7 control steps with 3 per launch, tapes from a fixed generator.
"""

import functools
import os

import numpy as np
import pytest

import test_rollout_tape_gpu as tp
from loco_mujoco_amd import LocoEnv

pytestmark = pytest.mark.gpu

T = tp.T
PRE = 3                                   # control steps before the save


def _rows(task, n):
    """Start rows; HumanoidTorque's first rows are robots folded on the floor (more contacts than the regular kernel has slots:
    the replay kernel, its prediction marks and the convex collider's cache are in use from the first step)."""
    env, _, tab = tp._task(task)
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)].copy()
    if task == "HumanoidTorque.run":
        d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ht_folded_states.npz"))
        nv = env._model.nv
        k = min(len(d["q"]), n - 5)
        rows[:k, :nv], rows[:k, nv:2 * nv] = d["q"][:k], d["v"][:k]
    return rows


def _acts(task, n, which):
    """pre: the steps before the save; A / B: the two tapes (A hits the ctrl clamp)."""
    if which == "pre":
        return tp._tape_of(task, n, 2.0, PRE)
    return tp._tape_of(task, n, 3.0 if which == "A" else 1.0)


def _span(b, acts, **kw):
    """One recorded span with the event counters of that span alone."""
    b.stats(reset=True)
    return tp._tape(b, acts, 3, **kw)


RESTARTS = {"table_rows": 5, "horizon": 3}


def _fresh(task, n, restarts=False):
    if not restarts:
        return tp._batch(task, n, rows=_rows(task, n))
    _, _, tab = tp._task(task)
    table = tab[np.linspace(0, len(tab) - 1, RESTARTS["table_rows"]).astype(int)]
    return tp._batch(task, n, rows=_rows(task, n), restarts=(table, RESTARTS["horizon"]), terminal=True)


@functools.lru_cache(maxsize=None)
def _rewind(task, n, restarts=False):
    """PRE steps; save; tape A; restore; tape A; restore; tape B — and the twin that never saved: PRE steps, then A step by step."""
    kw = dict(terminal=True) if restarts else {}
    b = _fresh(task, n, restarts)
    _span(b, _acts(task, n, "pre"))
    snap = b.snapshot()
    first = _span(b, _acts(task, n, "A"), **kw)
    b.restore(snap)
    second = _span(b, _acts(task, n, "A"), **kw)
    b.restore(snap)
    third = _span(b, _acts(task, n, "B"), **kw)
    twin_b = _fresh(task, n, restarts)
    tp._single_steps(twin_b, _acts(task, n, "pre"))
    twin_b.stats(reset=True)
    twin = tp._single_steps(twin_b, _acts(task, n, "A"), terminal=restarts)
    out = dict(first=first, second=second, third=third, twin=twin, nbytes=snap.nbytes)
    if restarts:
        # the count of control steps keys the random actions of rollout(): rewound with the rest
        finals = []
        for _ in range(2):
            b.restore(snap)
            b.rollout(T, action_mode=1)
            finals.append(b.get_state())
        out["finals"] = finals
    snap.close()
    b.close()
    twin_b.close()
    return out


REWIND_CASES = [("UnitreeA1.simple", 37), ("Atlas.walk", 37), ("HumanoidMuscle.run", 37), ("HumanoidTorque.run", 64)]


# ---- 1. rewind
@pytest.mark.parametrize("task,n", REWIND_CASES)
def test_rewind_repeats_the_span_bitwise(task, n):
    """save -> tape A -> restore -> tape A: the second recording, the final qpos / qvel / activations and the event counters of the
    span are the first's. restore -> tape B differs: the restore did not just freeze the batch."""
    r = _rewind(task, n)
    tp._check(r["second"], r["first"])
    assert r["nbytes"] > 0
    assert not np.array_equal(r["third"]["obs"], r["first"]["obs"])
    assert not np.array_equal(r["third"]["state"][0], r["first"]["state"][0])
    if task == "HumanoidTorque.run":
        assert r["first"]["stats"]["replayed_env_steps"] >= 1 and r["first"]["stats"]["self_contacts"] >= 1      # replay and the pair pass ran


# ---- 2. restore equals a twin
@pytest.mark.parametrize("task,n", REWIND_CASES)
def test_restored_batch_is_the_twin_that_never_saved(task, n):
    """The twin takes the same PRE + T steps with step_device and never saves: the first pass equals it (saving changes nothing) and so
    does the second (a restored batch cannot be told from one that simply lived that history)."""
    r = _rewind(task, n)
    tp._check(r["first"], r["twin"])
    tp._check(r["second"], r["twin"])


# ---- 3. restarts inside the span
@pytest.mark.parametrize("task,n", [("UnitreeA1.simple", 37), ("Atlas.walk", 37)])
def test_rewind_across_device_side_restarts(task, n):
    """Reset table of 5 rows, horizon 3, terminal observations on: the rewound pass restarts the same environments at the same steps
    to the same rows, with the same terminal rows; random-action rollouts from one snapshot agree (the count of control steps)."""
    r = _rewind(task, n, True)
    tp._check(r["second"], r["first"])
    tp._check(r["second"], r["twin"])
    done = r["first"]["done"]
    ended = (done & 2) != 0
    fell = ((done & 1) != 0).any(0)
    assert ended.sum() >= 2 * n and (~fell).sum() >= n // 2          # horizon 3, T = 7: every environment's episode ends at least twice
    tp._same(r["second"]["term"][ended], r["first"]["term"][ended], "terminal rows")
    assert (r["second"]["term"][~ended] == tp.OBS_FILL).all()
    tp._same(r["finals"][0][0], r["finals"][1][0], "qpos after rollout(action_mode=1) from the same snapshot")
    tp._same(r["finals"][0][1], r["finals"][1][1], "qvel after rollout(action_mode=1) from the same snapshot")


# ---- 4. fork
def _fork_src(n):
    src = np.random.RandomState(11).permutation(n).astype(np.int32)
    src[[1, 8, 20, 33]] = 5                # several environments take environment 5's state
    src[[2, 9, n - 1]] = -1                # these keep what they have
    src[12] = n                            # ... and so does an entry beyond the batch
    return src


@pytest.mark.parametrize("how", ["torch_async", "numpy"])
@pytest.mark.parametrize("task,n", [("UnitreeA1.simple", 37), ("HumanoidTorque.run", 64)])
def test_fork_continues_from_the_source(task, n, how):
    """fork(src), then every environment gets the action row of its source: environment e is bitwise environment src[e] of a twin that
    was not forked, in every tape row and in the final state; entries outside [0, n) leave the environment itself."""
    torch, dev = tp._torch()
    src = _fork_src(n)
    who = np.where((src >= 0) & (src < n), src, np.arange(n))
    b, twin_b = _fresh(task, n), _fresh(task, n)
    for x in (b, twin_b):
        tp._tape(x, _acts(task, n, "pre"), 3)
    if how == "numpy":
        b.fork(src)
    else:
        side = torch.cuda.Stream(dev)
        with torch.cuda.stream(side):
            d_src = torch.from_numpy(src).to(dev)
            b.fork(d_src, stream=torch.cuda.current_stream(dev).cuda_stream, sync=False)      # nothing waits on the host
    acts = _acts(task, n, "A")
    twin = tp._tape(twin_b, acts, 3)
    fork = tp._tape(b, np.ascontiguousarray(acts[:, who]), 3)        # (the library's stream is ordered behind the fork)
    for k in ("obs", "reward", "done"):
        tp._same(fork[k], twin[k][:, who], k + " tape of the forked batch")
    tp._same(fork["state"][0], twin["state"][0][who], "final qpos")
    tp._same(fork["state"][1], twin["state"][1][who], "final qvel")
    assert not np.array_equal(fork["state"][0], twin["state"][0])      # the fork did move environments
    b.close()
    twin_b.close()


# ---- 5. masked restore
def test_masked_restore_rewinds_the_masked_environments_only():
    task, n = "UnitreeA1.simple", 37
    mask = np.random.RandomState(5).rand(n) < 0.4
    assert 5 <= mask.sum() <= n - 5
    b, rewound, straight = _fresh(task, n), _fresh(task, n), _fresh(task, n)
    for x in (b, rewound, straight):
        tp._tape(x, _acts(task, n, "pre"), 3)
    snap = b.snapshot()
    tp._tape(b, _acts(task, n, "A"), 3)
    tp._tape(straight, _acts(task, n, "A"), 3)
    b.restore(snap, mask=mask)
    got = tp._tape(b, _acts(task, n, "B"), 3)
    want_m, want_o = tp._tape(rewound, _acts(task, n, "B"), 3), tp._tape(straight, _acts(task, n, "B"), 3)
    for k in ("obs", "reward", "done"):
        tp._same(got[k][:, mask], want_m[k][:, mask], k + " of the rewound environments")
        tp._same(got[k][:, ~mask], want_o[k][:, ~mask], k + " of the environments that went on")
    for i in (0, 1):
        tp._same(got["state"][i][mask], want_m["state"][i][mask], "final state of the rewound environments")
        tp._same(got["state"][i][~mask], want_o["state"][i][~mask], "final state of the environments that went on")
    assert not np.array_equal(want_m["obs"][:, mask], want_o["obs"][:, mask])


# ---- 6. per-environment models (the model compiler)
def test_rewind_and_fork_with_per_environment_models():
    n = 37
    env = tp._compiler_env(n)
    b = env.backend
    assert b.n_variants == n
    acts = tp._tape_of("Talos.walk", n, 1.0)
    snap = b.snapshot()
    d0, g0 = b.get_model_draws()
    first = _span(b, acts)
    d1, g1 = b.get_model_draws()
    assert ((first["done"] & 2) != 0).sum() >= 2 * n - 4 and (g1 >= g0 + 2).sum() >= n - 2      # two restarts, two fresh models each
    b.restore(snap)
    d, g = b.get_model_draws()
    assert np.array_equal(d, d0) and np.array_equal(g, g0)
    second = _span(b, acts)
    tp._check(second, first)
    d2, g2 = b.get_model_draws()
    assert np.array_equal(d2, d1) and np.array_equal(g2, g1)
    src = _fork_src(n)
    who = np.where((src >= 0) & (src < n), src, np.arange(n))
    before = [b.get_model_tables(e) for e in range(n)]
    b.fork(src)
    for e in range(n):
        for got, want in zip(b.get_model_tables(e), before[who[e]]):
            assert np.array_equal(got, want), e
    d3, g3 = b.get_model_draws()
    assert np.array_equal(d3, d2[who]) and np.array_equal(g3, g2[who])
    assert not np.array_equal(before[1][0], before[5][0])             # the models did differ


# ---- 7. export / import, refusals
def test_blob_round_trip_and_refusals():
    from loco_mujoco_amd.backend import BackendError, SNAPSHOT_BLOB_HEADER
    task, n = "UnitreeA1.simple", 37
    b = _fresh(task, n)
    tp._tape(b, _acts(task, n, "pre"), 3)
    snap = b.snapshot()
    blob = snap.to_bytes()
    assert len(blob) == SNAPSHOT_BLOB_HEADER + snap.nbytes
    want = _span(b, _acts(task, n, "A"))
    c = tp._batch(task, n)                                  # a fresh batch of the same model, other start rows
    s2 = c.snapshot_from_bytes(blob)
    c.restore(s2)
    tp._check(_span(c, _acts(task, n, "A")), want)

    def refused(call, word):
        q0, v0 = c.get_state()
        with pytest.raises((BackendError, ValueError), match=word):
            call()
        q, v = c.get_state()
        assert np.array_equal(q, q0) and np.array_equal(v, v0)

    refused(lambda: c.snapshot_from_bytes(blob[:len(blob) // 2]), "cut short")
    refused(lambda: c.snapshot_from_bytes(blob[:10]), "shorter than its header")
    refused(lambda: c.snapshot_from_bytes(b"\0" * len(blob)), "magic")
    other = tp._batch("Atlas.walk", n)
    refused(lambda: c.snapshot_from_bytes(other.snapshot().to_bytes()), "another configuration: nv")
    wide = tp._batch(task, 41)
    wide_snap = wide.snapshot()
    refused(lambda: c.restore(wide_snap), "another batch")
    assert c._lib.lm_snapshot_restore(c._h, wide_snap._h, None, None, 1) != 0          # ... and the library itself
    assert b"n_envs = 41, the batch has 37" in c._lib.lm_last_error(), c._lib.lm_last_error()
    old = c.snapshot()
    c.set_dof_params(damping=np.full((n, c.nv), 0.5, dtype=np.float32))
    refused(lambda: c.restore(old), "dof_params")
    refused(lambda: old.save(), "dof_params")
    # ... and the batch still steps, bitwise like one that went the same way and was never refused anything
    d = tp._batch(task, n)
    d.restore(d.snapshot_from_bytes(blob))
    tp._tape(d, _acts(task, n, "A"), 3)
    d.set_dof_params(damping=np.full((n, c.nv), 0.5, dtype=np.float32))
    tp._check(_span(c, _acts(task, n, "B")), _span(d, _acts(task, n, "B")))
    # closing the batch closes its snapshots
    c.close()
    assert s2.closed and old.closed
    with pytest.raises(ValueError, match="closed"):
        s2.to_bytes()


def test_snapshot_without_the_collider_cache_is_smaller():
    task, n = "HumanoidTorque.run", 64
    b = _fresh(task, n)
    tp._tape(b, _acts(task, n, "pre"), 3)
    full, lean = b.snapshot(), b.snapshot(keep_collider_cache=False)
    assert lean.nbytes < full.nbytes // 10
    q0, v0 = b.get_state()
    tp._tape(b, _acts(task, n, "A"), 3)
    b.restore(lean)
    q, v = b.get_state()
    tp._same(q, q0, "qpos after a restore without the cache")
    tp._same(v, v0, "qvel after a restore without the cache")
    assert b.snapshot_from_bytes(lean.to_bytes()).keep_collider_cache is False


# ---- 8. LocoEnv
@pytest.mark.parametrize("task,n,reset", [("UnitreeA1.simple", 1, {}), ("UnitreeA1.simple", 37, {}),
                                          ("Atlas.walk", 37, dict(seed=0, horizon=3, terminal_observations=True))])
def test_env_load_state_repeats_the_chunk(task, n, reset):
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, n_envs=n)
    env.reset()
    if reset:
        env.enable_auto_reset(**reset)
    nu = len(env._action_indices)
    acts = np.random.default_rng(7).uniform(-1, 1, (T, n, nu))
    acts = acts if n > 1 else acts[:, 0]
    env.step(acts[0])
    state = env.save_state()
    first = env.step_chunk(acts)
    env.step(acts[1])
    env.load_state(state)
    second = env.step_chunk(acts)
    for x, y in zip(first[:3], second[:3]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert first[0].dtype == np.float64 and set(first[3].keys()) == set(second[3].keys())
    for k in first[3]:
        assert np.array_equal(first[3][k], second[3][k]), k
    if reset:
        assert first[3]["episode_restarted"].sum() >= 2 * n - 4
    # ... and step() after load_state is step() after save_state
    env.load_state(state)
    o1 = [np.array(x) for x in env.step(acts[2])[:3]]
    env.load_state(state)
    o2 = [np.array(x) for x in env.step(acts[2])[:3]]
    for x, y in zip(o1, o2):
        assert np.array_equal(x, y)
    state.close()


def test_env_save_state_refuses_several_models():
    np.random.seed(0)
    env = LocoEnv.make("HumanoidTorque4Ages.run.all", debug=True, n_envs=8)
    env.reset()
    with pytest.raises(NotImplementedError, match="several models"):
        env.save_state()
