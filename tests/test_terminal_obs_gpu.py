"""
Terminal observations under device-side restarts (include/locohip.h lm_set_terminal_obs; `-m gpu`): a control step that ends an
episode on the device writes the observation of the state it REACHED into a buffer of its own, before the restart replaces state and
goal. Checked bitwise against a twin batch that does not restart (its observation of that step IS the terminal one), for every
launch mode that shares the kernel source, and through LocoEnv.step()'s `info["terminal_observation"]`.
"""

import ctypes as C
import functools

import numpy as np
import pytest

from loco_mujoco_amd import LocoEnv

pytestmark = pytest.mark.gpu

H = 3            # horizon of the twin runs: H + 1 control steps
GENERIC = "UnitreeA1.simple.rk4"      # the quadruped under RK4: no specialised family fits it, the generic kernels serve it (lm_families.h)
N_PUSHED = 12    # environments started just inside a termination bound with a velocity that crosses it


@functools.lru_cache(maxsize=None)
def _task(task, foot_forces=False):
    """(env, HipModel, reset table): one lowering per task for the whole module (read-only). GENERIC: UnitreeA1.simple with the compiled
    model's integrator set to RK4 in memory."""
    from loco_mujoco_amd.backend import HipModel
    np.random.seed(0)
    env = LocoEnv.make(task[:-len(".rk4")] if task == GENERIC else task, debug=True, **(dict(use_foot_forces=True) if foot_forces else {}))
    if task == GENERIC:
        env._model.integrator = 1
    return env, HipModel(env._chain_model()), env._reset_table()


def _start_rows(env, tab, n, seed=3):
    """n dataset rows; the first N_PUSHED are put just inside the upper end of the first bounded termination entry, moving out of it
    (pelvis height of the humanoids, trunk list of the quadruped), and — where the robot has a one-sided height bound (the quadruped) —
    lifted off the floor so that nothing holds the root back: they end absorbing in the first control step."""
    rs = np.random.RandomState(seed)
    rows = tab[rs.randint(0, len(tab), n)].copy()
    nv = env._model.nv
    spec = env.obs_helper.observation_spec[2:]
    term = env._termination_spec()
    i, lo, hi = next(t for t in term if np.isfinite(t[2]))
    j = env._model.jnt_id(spec[i][1])
    rows[:N_PUSHED, j] = hi - 0.005
    rows[:N_PUSHED, nv + j] = 3.0
    for i2, lo2, hi2 in term:
        if not np.isfinite(hi2):
            rows[:N_PUSHED, env._model.jnt_id(spec[i2][1])] += 0.3
    return rows, rs


def _load(b, env, rows):
    nv = env._model.nv
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    if rows.shape[1] > 2 * nv:
        b.set_goal(rows[:, 2 * nv:])


def _raw_step(b, act):
    """lm_step with the whole done byte."""
    a = np.ascontiguousarray(act, dtype=np.float32)
    obs = np.zeros((b.n, b.nobs), dtype=np.float32); rew = np.zeros(b.n, dtype=np.float32); done = np.zeros(b.n, dtype=np.uint8)
    f = C.POINTER(C.c_float)
    assert b._lib.lm_step(b._h, a.ctypes.data_as(f), obs.ctypes.data_as(f), rew.ctypes.data_as(f), done.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    return obs, rew, done


def _twin_run(task, n, foot_forces=False, replay=None, layout=None, terminal=True):
    """Batch A restarts on the device (reset table, horizon H, terminal observations on unless `terminal` is False); batch B runs the
    same states and actions without restarts. Returns per step (A's obs, reward, done byte, terminal buffer, B's obs) and A itself."""
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task(task, foot_forces)
    rows, rs = _start_rows(env, tab, n)
    acts = rs.uniform(-0.3, 0.3, (H + 1, n, len(env._action_indices)))
    A, B = HipBatch(hm, n, envs_per_workgroup=layout), HipBatch(hm, n, envs_per_workgroup=layout)
    for b in (A, B):
        if replay is not None:
            b.set_replay(replay)
        _load(b, env, rows)
    A.set_reset_table(tab, seed=5)
    A.set_auto_reset(True, horizon=H)
    B.set_auto_reset(False, horizon=H)
    if terminal:
        A.enable_terminal_obs()
        assert not A.terminal_obs().any()                  # zero-filled
    steps = []
    for a in acts:
        oa, ra, da = _raw_step(A, a)
        ob, _, _ = _raw_step(B, a)
        steps.append((oa, ra, da, A.terminal_obs() if terminal else None, ob))
    return env, A, steps


def _check_twin(env, steps, n, ngrf=0):
    ended = np.zeros(n, dtype=bool)
    n_abs = n_trunc = n_force = 0
    for t, (oa, ra, da, term, ob) in enumerate(steps, start=1):
        first = ((da & 2) != 0) & ~ended
        for e in np.nonzero(first)[0]:
            # B did not restart: its observation of this step is the observation A's episode ended in
            assert np.array_equal(term[e], ob[e]), (t, e, term[e], ob[e])
            assert not np.array_equal(term[e], oa[e])          # ... and not the restarted episode's first
        n_abs += int((first & ((da & 1) != 0) & (t < H)).sum())
        n_trunc += int((first & ((da & 1) == 0) & (t == H)).sum())
        if ngrf:
            # this step's mean foot force (bitwise the twin's, above), where the fresh episode's running mean starts at zero
            n_force += int((np.abs(term[first, -ngrf:]).max(1) > 0).sum())
            assert not oa[first, -ngrf:].any()
        ended |= first
        assert not term[~ended].any()                            # environments that have not ended: still the zero fill
    print("%d environments: %d ended absorbing before step %d, %d by truncation at it" % (n, n_abs, H, n_trunc))
    assert n_abs >= 8 and n_trunc >= 8                           # not vacuous: both kinds of episode end were seen
    assert ended.all()
    if ngrf:
        assert n_force >= 8                                      # the robots that walked into the horizon stand on the floor


@pytest.mark.parametrize("task,n,kw", [("UnitreeA1.simple", 37, {}), ("HumanoidTorque.run", 64, {}), ("HumanoidMuscle.run", 64, {}),
                                       ("HumanoidTorque.walk", 64, dict(foot_forces=True)),
                                       ("UnitreeA1.simple", 37, dict(replay=2)), ("UnitreeA1.simple", 37, dict(layout=16)),
                                       ("HumanoidTorque.run", 64, dict(layout=16)), (GENERIC, 37, {})])
def test_terminal_row_is_the_twin_batchs_observation_bitwise(task, n, kw):
    """At the first step in which A's done byte has bit 1, A's terminal row equals the observation of the twin that did not restart,
    bit for bit: dataset rows (n = 37: a ragged last workgroup) of which twelve leave a termination bound in the first step, the others
    run into the horizon. With foot forces the terminal row carries this step's mean force, the fresh observation zeros. GENERIC: the
    terminal-observation instance of the generic family's kernels (lm_family.hip launch_term)."""
    env, A, steps = _twin_run(task, n, **kw)
    ngrf = env._get_grf_size() if kw.get("foot_forces") else 0
    _check_twin(env, steps, n, ngrf)
    if kw.get("replay") == 2:
        assert A.replay_marks().all()                            # every control step went through the replay kernel


@pytest.mark.parametrize("task,n", [("UnitreeA1.simple", 37), ("HumanoidTorque.run", 64)])
def test_feature_changes_nothing_else(task, n):
    """The same run with the feature on and off: observations, rewards, done bytes, states and statistics are bitwise the same."""
    _, A1, on = _twin_run(task, n, terminal=True)
    _, A0, off = _twin_run(task, n, terminal=False)
    for (o1, r1, d1, _, _), (o0, r0, d0, _, _) in zip(on, off):
        assert np.array_equal(o1, o0) and np.array_equal(r1, r0) and np.array_equal(d1, d0)
    (q1, v1), (q0, v0) = A1.get_state(), A0.get_state()
    assert np.array_equal(q1, q0) and np.array_equal(v1, v0)
    s1, s0 = A1.stats(), A0.stats()
    s1.pop("kernel_ms"); s0.pop("kernel_ms")
    assert s1 == s0 and s1["episodes"] >= n


def test_get_before_enabling_is_an_error_and_disable_restores_it():
    from loco_mujoco_amd.backend import BackendError, HipBatch
    env, hm, tab = _task("UnitreeA1.simple")
    b = HipBatch(hm, 8)
    with pytest.raises(BackendError, match="not enabled"):
        b.terminal_obs()
    b.enable_terminal_obs()
    assert b.terminal_obs().shape == (8, b.nobs)
    b.disable_terminal_obs()
    with pytest.raises(BackendError, match="not enabled"):
        b.terminal_obs()


def _locoenv(copy_outputs, n=64):
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=n, copy_outputs=copy_outputs)
    env.reset()
    env.enable_auto_reset(seed=2, horizon=4, terminal_observations=True)
    return env


def test_locoenv_reports_terminal_observations_over_later_episodes():
    """LocoEnv.step() over 20 steps with horizon 4 (at least five episodes per environment): wherever `episode_restarted` is set the
    terminal observation has fallen exactly when the step was absorbing and differs from the returned (new episode's) observation; the
    pinned ring's view and the `copy_outputs=True` array agree; a view stays intact for three more steps; the columns are the
    reference's (the device buffer through the environment's column permutation)."""
    n = 64
    env, env_c = _locoenv(False), _locoenv(True)
    perm = env._obs_perm()
    rs = np.random.RandomState(4)
    seen = 0
    kept = []
    for t in range(20):
        act = rs.uniform(-1, 1, (n, 12))
        obs, rew, done, info = env.step(act)
        obs_c, _, done_c, info_c = env_c.step(act)
        assert set(info.keys()) == set(info_c.keys()) == {"episode_restarted", "terminal_observation"}
        r, term, term_c = info["episode_restarted"], info["terminal_observation"], info_c["terminal_observation"]
        assert term.shape == obs.shape and term.dtype == np.float64 and term_c.shape == obs.shape and term_c.dtype == np.float64
        assert np.array_equal(obs, obs_c) and np.array_equal(done, done_c) and np.array_equal(r, info_c["episode_restarted"])
        assert np.array_equal(term[r], term_c[r])
        buf = env.backend.terminal_obs()
        assert np.array_equal(term[r], (buf if perm is None else buf[:, perm]).astype(np.float64)[r])
        for e in np.nonzero(r)[0]:
            assert bool(env._has_fallen(term[e])) == bool(done[e]), (t, e)
            assert not np.array_equal(term[e], obs[e])
        seen += int(r.sum())
        kept.append((term, term[r].copy(), r.copy()))
        if t >= 3:
            view, rows, rr = kept[t - 3]
            assert np.array_equal(view[rr], rows)            # what step t - 3 returned is intact after three more steps
    assert seen >= 5 * n


def test_rollout_fused_and_unfused_leave_the_same_terminal_buffer():
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task("UnitreeA1.simple")
    n = 128
    rows, _ = _start_rows(env, tab, n)
    bufs = []
    for spl in (1, 5):
        b = HipBatch(hm, n)
        _load(b, env, rows)
        b.set_reset_table(tab, seed=5)
        b.set_auto_reset(True, horizon=H)
        b.enable_terminal_obs()
        st = b.rollout(10, action_mode=1, seed=3, steps_per_launch=spl)
        assert st["episodes"] >= 3 * n
        bufs.append(b.terminal_obs())
    assert np.array_equal(bufs[0], bufs[1])
    assert (np.abs(bufs[0]).max(1) > 0).all()                # every environment's last episode end is there


def test_active_list_and_caller_owned_buffer():
    """A caller-owned torch tensor handed to `enable_terminal_obs` receives, through `step_device`, the rows the library-owned buffer
    of a twin receives; under an active list the rows of inactive environments keep what they held."""
    import torch
    from loco_mujoco_amd.backend import HipBatch
    env, hm, tab = _task("HumanoidTorque.run")
    n = 37
    rows, rs = _start_rows(env, tab, n)
    acts = rs.uniform(-0.3, 0.3, (H, n, len(env._action_indices))).astype(np.float32)
    active = np.arange(0, n, 2)
    dev = torch.device("cuda", 0)
    out = torch.full((n, hm.dims.nobs), 7.0, dtype=torch.float32, device=dev)
    own, ext = HipBatch(hm, n), HipBatch(hm, n)
    for b in (own, ext):
        _load(b, env, rows)
        b.set_reset_table(tab, seed=5)
        b.set_auto_reset(True, horizon=H)
        b.set_active(active)
    own.enable_terminal_obs()
    with pytest.raises(ValueError):
        ext.enable_terminal_obs(out[:, :-1])
    with pytest.raises(ValueError):
        ext.enable_terminal_obs(out.double())
    ext.enable_terminal_obs(out)
    torch.cuda.synchronize()
    for a in acts:
        own.step(a)
        ext.step_device(torch.from_numpy(a).to(dev), sync=True)
    got, ref = out.cpu().numpy(), own.terminal_obs()
    inactive = np.setdiff1d(np.arange(n), active)
    assert np.array_equal(got[active], ref[active]) and (np.abs(ref[active]).max(1) > 0).all()
    assert (got[inactive] == 7.0).all() and not ref[inactive].any()
    assert np.array_equal(ext.terminal_obs(), got)           # lm_get_terminal_obs reads whichever buffer is in use


def test_grouped_models_take_the_row_from_the_batch_the_episode_ran_on():
    """HumanoidTorque4Ages "all": one batch per size, an environment changes size (and batch) when its episode ends and the host redraws
    model and start row. The terminal observation is the one of the size the episode RAN on: its size bits are those the environment
    had before the step, and it has fallen exactly when the step was absorbing."""
    n = 64
    np.random.seed(0)
    env = LocoEnv.make("HumanoidTorque4Ages.walk.all", debug=True, n_envs=n)
    prev = env.reset()
    env.enable_auto_reset(seed=7, horizon=4, terminal_observations=True)
    rs = np.random.RandomState(1)
    seen = 0
    for k in range(6):
        before = env._env_model.copy()
        obs, rew, done, info = env.step(rs.uniform(-0.3, 0.3, (n, 13)))
        r, term = info["episode_restarted"], info["terminal_observation"]
        assert term.shape == obs.shape and term.dtype == np.float64
        if k == 3:
            assert r.sum() >= n // 2                          # horizon 4
        bits = term[r][:, -2:]
        assert np.array_equal(bits[:, 0] * 2 + bits[:, 1], before[r].astype(float))
        for e in np.nonzero(r)[0]:
            assert bool(env._has_fallen(term[e])) == bool(done[e]), (k, e)
            assert not np.array_equal(term[e], obs[e])
        seen += int(r.sum())
    assert seen >= n


def test_block_models_report_each_blocks_rows(tmp_path):
    """Domain randomisation over the humanoid's four sizes: contiguous blocks of environments, one device batch per size (`_blocks`,
    not grouped). `info["terminal_observation"]` is the blocks' buffers one after the other: in every block the rows with
    `episode_restarted` are that batch's terminal rows (reference column order), carry the block's size bits, have fallen exactly when
    the step was absorbing and differ from the new episode's observation; at horizon 2 every environment of every block ends."""
    n, m = 64, 4
    y = tmp_path / "dr.yaml"
    y.write_text("Joints:\n  knee_angle_r:\n    damping:\n      sigma: 0.01\n")
    np.random.seed(0)
    env = LocoEnv.make("HumanoidTorque4Ages.walk.all", debug=True, n_envs=n, domain_randomization_config=str(y))
    assert env._blocks and not env._grouped and env._n_models == m
    env.reset()
    env.enable_auto_reset(seed=7, horizon=2, terminal_observations=True)
    perm = env._obs_perm()
    rs = np.random.RandomState(1)
    for k in range(4):
        obs, rew, done, info = env.step(rs.uniform(-0.3, 0.3, (n, 13)))
        assert set(info.keys()) == {"episode_restarted", "terminal_observation"}
        r, term = info["episode_restarted"], info["terminal_observation"]
        assert term.shape == obs.shape and term.dtype == np.float64 and r.shape == (n,)
        if k % 2 == 1:
            assert r.all()                                    # horizon 2: every block's environments end here
        for idx in range(m):
            envs = env._model_envs(idx)
            assert len(envs) == n // m
            env._select_model(idx)
            assert np.array_equal(r[envs], env.backend.last_restarted)
            buf = env.backend.terminal_obs()
            assert buf.shape == (len(envs), obs.shape[1])
            buf = (buf if perm is None else buf[:, perm]).astype(np.float64)
            rb = r[envs]
            assert np.array_equal(term[envs][rb], buf[rb])
            bits = term[envs][rb][:, -2:]
            assert (bits[:, 0] * 2 + bits[:, 1] == idx).all()
        for e in np.nonzero(r)[0]:
            assert bool(env._has_fallen(term[e])) == bool(done[e]), (k, e)
            assert not np.array_equal(term[e], obs[e])
