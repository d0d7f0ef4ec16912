"""
Action tapes (include/locohip.h lm_rollout_tape, HipBatch.rollout_tape, LocoEnv.step_chunk; `-m gpu`): T control steps under given
actions, several per kernel launch, every step's observation, reward, done byte and terminal observation recorded. Every comparison
is BITWISE against a twin batch that takes the same T steps one lm_step_device call at a time from the same initial state.
Shapes: 37 environments (a partial last workgroup at 4 per workgroup) or 64, T = 7 with 3 steps per launch (launches of 3, 3, 1).
"""

import functools
import os

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv

pytestmark = pytest.mark.gpu

T = 7
OBS_FILL, DONE_FILL = -7.0, 0x80          # sentinels of rows that must not be written
COUNTERS = ("env_steps", "episodes", "nan_resets", "solver_iters", "overflow_contacts", "unhandled_geoms", "linesearch_evals",
            "linesearch_capped", "steps_with_8plus_iters", "self_proximity", "self_contacts", "own_manifold_contacts")
# (not among them: replayed_env_steps counts where a control step RAN, not what happened in it — an environment handed to the replay kernel
# finishes the launch's remaining control steps there, so the figure grows with steps_per_launch; as under lm_rollout_fused)


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _task(task):
    """(env, HipModel, reset table): one lowering per task for the whole module (read-only)."""
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True)
    return env, HipModel(env._chain_model()), env._reset_table()


@functools.lru_cache(maxsize=None)
def _tape_of(task, n, scale, steps=T):
    """The action tape: a fixed generator, U(-scale, scale) — 1: inside the action range, 3: the ctrl clamp is hit."""
    env, _, _ = _task(task)
    a = np.random.default_rng(1234).uniform(-scale, scale, (steps, n, len(env._action_indices))).astype(np.float32)
    a.setflags(write=False)
    return a


def _batch(task, n, rows=None, layout=None, replay=None, restarts=None, terminal=False, active=None):
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task(task)
    nv = env._model.nv
    if rows is None:
        rows = tab[np.random.RandomState(3).randint(0, len(tab), n)]
    b = HipBatch(hm, n, envs_per_workgroup=layout)
    if replay is not None:
        b.set_replay(replay)
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    if rows.shape[1] > 2 * nv:
        b.set_goal(rows[:, 2 * nv:])
    if restarts is not None:
        table, horizon = restarts
        b.set_reset_table(table, seed=5)
        b.set_auto_reset(True, horizon=horizon)
    if terminal:
        b.enable_terminal_obs()
    if active is not None:
        b.set_active(active)
    return b


def _single_steps(b, acts, terminal=False):
    """The twin: one lm_step_device call per tape row, into sentinel-filled rows of its own. Returns the stacked results."""
    torch, dev = _torch()
    steps, n = acts.shape[0], b.n
    d_a = torch.from_numpy(np.array(acts)).to(dev)
    obs = torch.full((steps, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev)
    rew = torch.full((steps, n), OBS_FILL, dtype=torch.float32, device=dev)
    done = torch.full((steps, n), DONE_FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    term = []
    for t in range(steps):
        b.step_device(action=d_a[t], obs=obs[t], reward=rew[t], done=done[t])
        if terminal:
            term.append(b.terminal_obs())
    return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), done=done.cpu().numpy(), term=np.stack(term) if terminal else None,
                state=b.get_state(), act=b.get_activation() if b.na else None, stats=b.stats(), marks=b.replay_marks())


def _tape(b, acts, spl, repeat=None, want=("obs", "reward", "done"), terminal=False):
    torch, dev = _torch()
    steps, n = (repeat if repeat is not None else acts.shape[0]), b.n
    d_a = torch.from_numpy(np.array(acts)).to(dev)
    bufs = dict(obs=torch.full((steps, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev) if "obs" in want else None,
                reward=torch.full((steps, n), OBS_FILL, dtype=torch.float32, device=dev) if "reward" in want else None,
                done=torch.full((steps, n), DONE_FILL, dtype=torch.uint8, device=dev) if "done" in want else None,
                terminal=torch.full((steps, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev) if terminal else None)
    torch.cuda.synchronize(dev)
    b.rollout_tape(d_a, steps_per_launch=spl, repeat=repeat, **bufs)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in bufs.items()}
    out["term"] = out.pop("terminal")
    out.update(state=b.get_state(), act=b.get_activation() if b.na else None, stats=b.stats(), marks=b.replay_marks())
    return out


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), \
        "%s differs at %s" % (what, np.argwhere(~((a == b) | ((a != a) & (b != b))))[:4].tolist())


def _check(tape, twin, keys=("obs", "reward", "done")):
    for k in keys:
        _same(tape[k], twin[k], k + " tape")
    _same(tape["state"][0], twin["state"][0], "final qpos")
    _same(tape["state"][1], twin["state"][1], "final qvel")
    if twin["act"] is not None:
        _same(tape["act"], twin["act"], "final activations")
    for k in COUNTERS:
        assert tape["stats"][k] == twin["stats"][k], (k, tape["stats"][k], twin["stats"][k])
    assert twin["stats"]["env_steps"] > 0
    # reward_sum counts no event: a float32 sum per workgroup whose grouping follows the launches (a fused launch adds its control
    # steps' rewards up before they join the slot). <= 4 environments x T terms per slot: a few float32 roundings, 1e-5 relative is
    # ~30 of them; every single reward is compared bitwise in the reward tape above
    assert np.isclose(tape["stats"]["reward_sum"], twin["stats"]["reward_sum"], rtol=1e-5, atol=0)


@functools.lru_cache(maxsize=None)
def _twin(task, n, scale):
    """The plain twin run of a task (no restarts), computed once and shared."""
    return _single_steps(_batch(task, n), _tape_of(task, n, scale))


# ---- 1. tape = single steps
@pytest.mark.parametrize("spl", [1, 3, T])
@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("task,n", [("UnitreeA1.simple", 37), ("Atlas.walk", 37), ("HumanoidTorque.run", 64)])
def test_tape_is_bitwise_the_single_steps(task, n, scale, spl):
    """Every row of the observation, reward and done tapes, the final state and the event counters, for launches of 1, 3 (3 + 3 + 1)
    and T control steps: Euler without an active list (the quadruped), RK4 (Atlas), the pair pass with the convex collider."""
    twin = _twin(task, n, scale)
    tape = _tape(_batch(task, n), _tape_of(task, n, scale), spl)
    _check(tape, twin)
    assert not (twin["obs"] == OBS_FILL).all(2).any() and not (twin["done"] == DONE_FILL).any()      # the twin did write every row


# ---- 2. hand-over to the replay kernel inside a launch
@pytest.mark.parametrize("replay", [None, 2])
def test_replay_hand_over_inside_a_launch(replay):
    """HumanoidTorque robots folded on the floor (tests/golden/ht_folded_states.npz: more contacts on a chain than the regular kernel
    has slots) under the U(-3,3) tape: the regular kernel hands them to the replay kernel in the middle of a fused launch, which has
    to go on reading and writing at the hand-over step's rows. replay=2: EVERY control step through the replay kernel."""
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ht_folded_states.npz"))
    env, _, tab = _task("HumanoidTorque.run")
    nv = env._model.nv
    n = 37
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)].copy()
    k = min(len(d["q"]), n - 5)
    rows[:k, :nv], rows[:k, nv:2 * nv] = d["q"][:k], d["v"][:k]
    acts = _tape_of("HumanoidTorque.run", n, 3.0)
    twin = _single_steps(_batch("HumanoidTorque.run", n, rows=rows, replay=replay), acts)
    for spl in (3, T):
        b = _batch("HumanoidTorque.run", n, rows=rows, replay=replay)
        b.replay_marks(reset=True)
        tape = _tape(b, acts, spl)
        print("steps per launch %d: %d of %d environments replayed, %d env-steps" % (spl, tape["marks"].sum(), n, tape["stats"]["replayed_env_steps"]))
        assert tape["marks"].sum() >= 1 and tape["stats"]["replayed_env_steps"] >= 1      # the replay kernel DID run during the tape call
        if replay == 2:
            assert tape["marks"].all() and tape["stats"]["replayed_env_steps"] == T * n
        _check(tape, twin)
        assert tape["marks"][twin["marks"]].all()          # whatever needed the replay kernel step by step needs it in a fused launch
        assert tape["stats"]["replayed_env_steps"] >= twin["stats"]["replayed_env_steps"]


# ---- 3. restarts in the middle of a launch
@pytest.mark.parametrize("task,n", [("UnitreeA1.simple", 37), ("Atlas.walk", 37)])
def test_restarts_inside_one_launch(task, n):
    """Reset table of 5 distinct rows, horizon 3, all T = 7 steps in ONE launch: every environment restarts twice inside it."""
    env, _, tab = _task(task)
    table = tab[np.linspace(0, len(tab) - 1, 5).astype(int)]
    assert len(np.unique(table, axis=0)) == 5
    acts = _tape_of(task, n, 1.0)
    twin = _single_steps(_batch(task, n, restarts=(table, 3), terminal=True), acts, terminal=True)
    tape = _tape(_batch(task, n, restarts=(table, 3), terminal=True), acts, T, terminal=True)
    _check(tape, twin)
    done = tape["done"]
    fell = ((done & 1) != 0).any(0)
    assert (~fell).sum() >= n // 2
    expect = np.zeros((T, n), dtype=bool)
    expect[[2, 5]] = True
    _same(((done & 2) != 0)[:, ~fell], expect[:, ~fell], "bit 1 of the done tape")
    ended = (done & 2) != 0
    # rows of steps that ended an episode: the twin's terminal buffer read after that step; every other row: the sentinel
    _same(tape["term"][ended], twin["term"][ended], "terminal tape")
    assert (tape["term"][~ended] == OBS_FILL).all()
    assert not np.array_equal(tape["term"][ended], tape["obs"][ended])          # ... not the restarted episode's first observation
    assert tape["stats"]["episodes"] >= 2 * (~fell).sum()


def test_terminal_tape_stands_in_for_the_terminal_buffer():
    """With a terminal tape the rows go to the tape and the buffer of lm_set_terminal_obs keeps what it held (include/locohip.h);
    without one the buffer is written as by lm_step_device: after T steps it is the twin's."""
    task, n = "UnitreeA1.simple", 37
    env, _, tab = _task(task)
    table = tab[np.linspace(0, len(tab) - 1, 5).astype(int)]
    acts = _tape_of(task, n, 1.0)
    twin_b = _batch(task, n, restarts=(table, 3), terminal=True)
    twin = _single_steps(twin_b, acts, terminal=True)
    assert np.abs(twin["term"][-1]).max() > 0
    b = _batch(task, n, restarts=(table, 3), terminal=True)
    tape = _tape(b, acts, 3, terminal=True)
    _check(tape, twin)
    assert not b.terminal_obs().any()                       # still the zero-filled buffer
    b = _batch(task, n, restarts=(table, 3), terminal=True)
    tape = _tape(b, acts, 3)
    _check(tape, twin)
    _same(b.terminal_obs(), twin["term"][-1], "terminal buffer without a terminal tape")


# ---- 4. action repeat
def test_action_repeat_is_a_tape_of_the_same_action():
    task, n = "UnitreeA1.simple", 37
    one = _tape_of(task, n, 3.0)[0]
    ref = _tape(_batch(task, n), np.broadcast_to(one, (5,) + one.shape).copy(), 3)
    rep = _tape(_batch(task, n), one, 3, repeat=5)
    assert rep["obs"].shape[0] == 5
    _check(rep, ref)
    _check(rep, _single_steps(_batch(task, n), np.broadcast_to(one, (5,) + one.shape).copy()))


# ---- 5. null outputs
@pytest.mark.parametrize("only", ["done", "obs"])
def test_partial_recording_leaves_the_same_state(only):
    task, n = "Atlas.walk", 37
    twin = _twin(task, n, 1.0)
    tape = _tape(_batch(task, n), _tape_of(task, n, 1.0), 3, want=(only,))
    _check(tape, twin, keys=(only,))


# ---- 6. active list
def test_active_list_leaves_inactive_rows_alone():
    task, n = "HumanoidTorque.run", 64
    ids = np.arange(1, n, 2, dtype=np.int32)
    acts = _tape_of(task, n, 1.0)
    twin = _single_steps(_batch(task, n, active=ids), acts)
    tape = _tape(_batch(task, n, active=ids), acts, 3)
    _check(tape, twin)
    off = np.setdiff1d(np.arange(n), ids)
    assert (tape["obs"][:, off] == OBS_FILL).all() and (tape["reward"][:, off] == OBS_FILL).all() and (tape["done"][:, off] == DONE_FILL).all()
    assert not (tape["obs"][:, ids] == OBS_FILL).all(2).any() and not (tape["done"][:, ids] == DONE_FILL).any()
    assert tape["stats"]["env_steps"] == T * len(ids)


# ---- 7. fallback paths: one step per launch with host-side offsets
def test_fallback_sixteen_environments_per_workgroup():
    task, n = "Atlas.walk", 37
    acts = _tape_of(task, n, 1.0)
    twin = _single_steps(_batch(task, n, layout=16), acts)
    _check(_tape(_batch(task, n, layout=16), acts, 3), twin)


def _compiler_env(n):
    np.random.seed(0)
    cfg = os.path.join(os.path.dirname(__file__), "golden", "dr_talos_inertial.yaml")
    env = LocoEnv.make("Talos.walk", debug=True, n_envs=n, domain_randomization_config=cfg)
    env.reset()
    env.enable_auto_reset(seed=3, horizon=3)
    env.step(np.zeros((n, 12)))
    return env


def test_fallback_with_the_model_compiler():
    """A batch with the on-device model compiler (a fresh model per restart, compiled BETWEEN launches): restarts every 3 steps."""
    n = 37
    A, B = _compiler_env(n).backend, _compiler_env(n).backend
    assert A.n_variants == n
    acts = _tape_of("Talos.walk", n, 1.0)
    twin = _single_steps(B, acts)
    tape = _tape(A, acts, 3)
    _check(tape, twin)
    assert ((tape["done"] & 2) != 0).sum() >= 2 * n - 4
    da, ga = A.get_model_draws()
    db, gb = B.get_model_draws()
    assert np.array_equal(da, db) and np.array_equal(ga, gb)


# ---- 8. errors: nothing launched
def test_refused_calls_launch_nothing():
    from loco_mujoco_amd.backend import BackendError
    import ctypes as C
    torch, dev = _torch()
    task, n = "UnitreeA1.simple", 37
    b = _batch(task, n)
    q0, v0 = b.get_state()
    acts = torch.from_numpy(np.array(_tape_of(task, n, 1.0))).to(dev)
    term = torch.zeros((T, n, b.nobs), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def raw(actions, stride, d_term=None):
        return b._lib.lm_rollout_tape(b._h, T, 3, None if actions is None else C.c_void_p(actions.data_ptr()), stride, None, None, None,
                                      None if d_term is None else C.c_void_p(d_term.data_ptr()), None, 1, None)
    for call, word in ((lambda: raw(acts, n * b.nu, term), b"d_term"), (lambda: raw(acts, n * b.nu - 1), b"action_step_stride"),
                       (lambda: raw(acts, b.nu), b"action_step_stride"), (lambda: raw(None, n * b.nu), b"d_actions")):
        assert call() != 0
        assert word in b._lib.lm_last_error(), b._lib.lm_last_error()
        q, v = b.get_state()
        assert np.array_equal(q, q0) and np.array_equal(v, v0)
    with pytest.raises(ValueError, match="terminal"):
        b.rollout_tape(acts, terminal=term)
    assert b.stats()["env_steps"] == 0
    assert raw(acts, n * b.nu) == 0                      # the batch is still usable
    assert b.stats()["env_steps"] == T * n


# ---- 9. LocoEnv.step_chunk
def _env_pair(task, n, **reset):
    envs = []
    for _ in range(2):
        np.random.seed(0)
        env = LocoEnv.make(task, debug=True, n_envs=n)
        env.reset()
        if reset:
            env.enable_auto_reset(**reset)
        envs.append(env)
    return envs


@pytest.mark.parametrize("task,n,reset", [("UnitreeA1.simple", 1, {}), ("UnitreeA1.simple", 37, {}),
                                          ("Atlas.walk", 37, dict(seed=0, horizon=3, terminal_observations=True))])
def test_step_chunk_is_k_calls_of_step(task, n, reset):
    A, B = _env_pair(task, n, **reset)
    nu = len(A._action_indices)
    acts = np.random.default_rng(7).uniform(-1, 1, (T + 1, n, nu))
    obs, rew, absorbing, info = A.step_chunk(acts[:T] if n > 1 else acts[:T, 0])
    assert obs.shape == (T, n, A.info.observation_space.shape[0]) and obs.dtype == np.float64 and rew.shape == (T, n) and absorbing.shape == (T, n)
    for t in range(T):
        o, r, d, inf = B.step(acts[t] if n > 1 else acts[t, 0])
        assert np.array_equal(obs[t], np.reshape(o, (n, -1))) and np.array_equal(rew[t], np.reshape(r, n)) and np.array_equal(absorbing[t], np.reshape(d, n))
        assert set(inf.keys()) == set(info.keys()), (inf.keys(), info.keys())
        if "episode_restarted" in inf:
            restarted = np.reshape(inf["episode_restarted"], n)
            assert np.array_equal(info["episode_restarted"][t], restarted)
        if "terminal_observation" in inf:
            # both define these rows where episode_restarted is set; the others are unspecified (step(): whatever its buffer held)
            assert np.array_equal(info["terminal_observation"][t][restarted], inf["terminal_observation"][restarted])
            assert not info["terminal_observation"][t][~restarted].any()          # step_chunk: zeros
    if reset:
        assert info["episode_restarted"].sum() >= 2 * n - 4 and info["terminal_observation"].shape == obs.shape
    # the two alternate: one more step() on both
    oa, ra, da, ia = A.step(acts[T] if n > 1 else acts[T, 0])
    ob, rb, db, ib = B.step(acts[T] if n > 1 else acts[T, 0])
    assert np.array_equal(oa, ob) and np.array_equal(ra, rb) and np.array_equal(da, db) and set(ia.keys()) == set(ib.keys())
    if reset:
        # T = 7, horizon 3: this eighth step is not an episode's last; step T + 2 (below) is, and reports the same rows on both
        assert np.array_equal(ia["episode_restarted"], ib["episode_restarted"])
        oa, _, _, ia = A.step(acts[0])
        ob, _, _, ib = B.step(acts[0])
        ended = ib["episode_restarted"]
        assert ended.sum() >= n // 2 and np.array_equal(ia["episode_restarted"], ended) and np.array_equal(oa, ob)
        assert np.array_equal(ia["terminal_observation"][ended], ib["terminal_observation"][ended])
    # ... and a chunk after a step
    oc = A.step_chunk(acts[:2] if n > 1 else acts[:2, 0])[0]
    for t in range(2):
        assert np.array_equal(oc[t], np.reshape(B.step(acts[t] if n > 1 else acts[t, 0])[0], (n, -1)))


def test_step_chunk_refusals_give_their_reason():
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=4, use_foot_forces=True)      # its reward reads foot-force columns: host
    env.reset()
    assert env._reward_device_spec() is None
    with pytest.raises(NotImplementedError, match="reward runs on the host"):
        env.step_chunk(np.zeros((2, 4, 12)))
    with pytest.raises(NotImplementedError, match="model compiler"):
        _compiler_env(4).step_chunk(np.zeros((2, 4, 12)))
    np.random.seed(0)
    env = LocoEnv.make("HumanoidTorque4Ages.run.all", debug=True, n_envs=8)
    env.reset()
    assert env._blocks
    with pytest.raises(NotImplementedError, match="several models"):
        env.step_chunk(np.zeros((2, 8, len(env._action_indices))))


# ---- 10. a caller's stream with nothing waiting on the host; a refused call
SIDE_N, SIDE_STEPS = 5, 6      # one full workgroup and one of a single environment; step_device + a tape of 4 (launches of 3 and 1) + step_device
SIDE_CASES = [("UnitreeA1.simple", None), ("HumanoidTorque.run", 2)]


def _six_steps(b, acts, stream, sync):
    """step_device, rollout_tape of 4 with 3 steps per launch, step_device — then get_state(), which runs on the library's stream."""
    torch, dev = _torch()
    n = b.n
    d_a = torch.from_numpy(np.array(acts)).to(dev)
    obs = torch.full((SIDE_STEPS, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev)
    rew = torch.full((SIDE_STEPS, n), OBS_FILL, dtype=torch.float32, device=dev)
    done = torch.full((SIDE_STEPS, n), DONE_FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    kw = dict(stream=stream, sync=sync)
    b.step_device(action=d_a[0], obs=obs[0], reward=rew[0], done=done[0], **kw)
    b.rollout_tape(d_a[1:5], obs=obs[1:5], reward=rew[1:5], done=done[1:5], steps_per_launch=3, **kw)
    b.step_device(action=d_a[5], obs=obs[5], reward=rew[5], done=done[5], **kw)
    state = b.get_state()                     # no host wait in front of it: the library orders its stream behind the caller's
    torch.cuda.synchronize(dev)
    return dict(state=state, obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), done=done.cpu().numpy())


@pytest.mark.parametrize("task,replay", SIDE_CASES)
def test_calls_on_a_side_stream_without_host_waits(task, replay):
    """Six control steps queued on a torch side stream (not the current one) with sync=False, then get_state() on the library's
    stream: state and every recorded row are bitwise those of a twin that ran the same six steps synchronously on the library's
    stream. The quadruped: no replay pass. HumanoidTorque with set_replay(2): every control step goes through the replay kernel —
    its pollers run on the batch's second stream, and each launch is ordered behind the previous one's drain pass."""
    torch, dev = _torch()
    acts = _tape_of(task, SIDE_N, 1.0, steps=SIDE_STEPS)
    twin = _six_steps(_batch(task, SIDE_N, replay=replay), acts, None, True)
    side = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    out = _six_steps(_batch(task, SIDE_N, replay=replay), acts, side.cuda_stream, False)
    for k in ("obs", "reward", "done"):
        _same(out[k], twin[k], k + " rows")
    _same(out["state"][0], twin["state"][0], "final qpos")
    _same(out["state"][1], twin["state"][1], "final qvel")
    assert not (twin["obs"] == OBS_FILL).all(2).any() and not (twin["done"] == DONE_FILL).any()      # every row was written


def test_a_refused_forward_debug_changes_nothing():
    """forward_debug at 16 environments per workgroup is refused on the host with its LDS byte counts (nothing is launched): the
    state stays, and so does the count of control steps that keys the random policy — a random-action rollout afterwards leaves
    the state of a twin batch that was never refused."""
    from loco_mujoco_amd.backend import BackendError
    task = "HumanoidTorque.run"
    a, twin = _batch(task, SIDE_N, replay=2), _batch(task, SIDE_N, replay=2)
    q0, v0 = a.get_state()
    a.set_layout(16)
    with pytest.raises(BackendError, match="LDS") as err:
        a.forward_debug(np.zeros((SIDE_N, a.nu)))
    assert "16 environments per workgroup" in str(err.value) and "forward" in str(err.value), str(err.value)
    q, v = a.get_state()
    _same(q, q0, "qpos after the refusal")
    _same(v, v0, "qvel after the refusal")
    a.set_layout(4)
    for b in (a, twin):
        b.rollout(3, action_mode=1, seed=7)
    _same(a.get_state()[0], twin.get_state()[0], "qpos after the rollout")
    _same(a.get_state()[1], twin.get_state()[1], "qvel after the rollout")
    assert not np.array_equal(a.get_state()[0], q0)
