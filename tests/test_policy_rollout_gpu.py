"""
Closed-loop policy rollouts (include/locohip.h lm_rollout_policy, HipBatch.rollout_policy; `-m gpu`): a small MLP evaluated on the
device at the top of every control step, its action recorded in a tape. Batches, states and the bitwise comparisons are those of
tests/test_rollout_tape_gpu.py (imported); shapes: n in {1, 5, 37}, T = 7, launches of 1, 3 (3 + 3 + 1) and 7 control steps.
"""

import functools
import os

import numpy as np
import pytest

import generic_family_common as GF
import test_rollout_tape_gpu as tp
from test_rollout_tape_gpu import COUNTERS, DONE_FILL, OBS_FILL, T, _same

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SPLS = [1, 3, T]
# task (or a key of generic_family_common.CASES), n, hidden widths, activation
CASES = {
    "a1": ("UnitreeA1.simple", 37, (40, 24), "tanh"),
    "atlas": ("Atlas.walk", 37, (256,), "relu"),
    "torque": ("HumanoidTorque.run", 37, (), "tanh"),
    "muscle": ("HumanoidMuscle.run", 5, (40, 24), "tanh"),            # nu = 92: the muscle-control path reads the action
    "generic": ("UnitreeA1.rk4", 37, (256,), "tanh"),                 # the generic family: one control step per launch
}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _generic_model(key):
    from loco_mujoco_amd.backend import HipModel
    return HipModel(GF.inputs(key)["cm"])


def _batch(task, n, rows=None, **kw):
    """tests/test_rollout_tape_gpu.py's batch; for a generic-family key the edited model with the states of its own tests."""
    if task not in GF.CASES:
        return tp._batch(task, n, rows=rows, **kw)
    from loco_mujoco_amd.backend import HipBatch
    assert not kw
    c = GF.inputs(task)
    rows = c["rows"][:n] if rows is None else rows
    nv = c["m"].nv
    b = HipBatch(_generic_model(task), n)
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    if rows.shape[1] > 2 * nv:
        b.set_goal(rows[:, 2 * nv:])
    return b


def _first_obs(b):
    """One zero-action step into a tensor of the caller's: the observation the first action is computed from."""
    torch, dev = _torch()
    obs0 = torch.zeros((b.n, b.nobs), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    b.step_device(obs=obs0)
    return obs0


@functools.lru_cache(maxsize=None)
def _module(nobs, nu, widths, act, seed=0):
    """A seeded torch Sequential on the device. The first layer is scaled up (observations are O(1): some hidden units saturate), the
    last one down (actions inside the actuators' range most of the time)."""
    torch, dev = _torch()
    torch.manual_seed(1000 + seed)
    sizes = (nobs,) + tuple(widths) + (nu,)
    mods = []
    for a, c in zip(sizes[:-1], sizes[1:]):
        mods += [torch.nn.Linear(a, c), torch.nn.Tanh() if act == "tanh" else torch.nn.ReLU()]
    seq = torch.nn.Sequential(*mods[:-1])
    with torch.no_grad():
        seq[0].weight.mul_(3.0)
        if len(widths):
            seq[-1].weight.mul_(0.5)
    return seq.to(dev)


def _policy(b, widths, act, log_std=None, seed=0):
    from loco_mujoco_amd.backend import MlpPolicy
    torch, dev = _torch()
    if log_std is not None:
        log_std = torch.full((b.nu,), float(log_std), dtype=torch.float32, device=dev)
    return MlpPolicy.from_torch(_module(b.nobs, b.nu, tuple(widths), act, seed), log_std)


def _run(b, policy, spl, obs0, steps=T, noise_seed=0, terminal=False, **kw):
    torch, dev = _torch()
    n = b.n
    bufs = dict(obs=torch.full((steps, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev),
                reward=torch.full((steps, n), OBS_FILL, dtype=torch.float32, device=dev),
                done=torch.full((steps, n), DONE_FILL, dtype=torch.uint8, device=dev),
                terminal=torch.full((steps, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev) if terminal else None)
    torch.cuda.synchronize(dev)
    acts = b.rollout_policy(policy, steps, obs0=obs0, steps_per_launch=spl, noise_seed=noise_seed, **bufs, **kw)
    torch.cuda.synchronize(dev)
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in bufs.items()}
    out["term"] = out.pop("terminal")
    out.update(actions=acts.cpu().numpy(), state=b.get_state(), act=b.get_activation() if b.na else None, stats=b.stats(), marks=b.replay_marks())
    return out


def _replayed_by_tape(make, out, spl, terminal=False):
    """Test 1: the recorded actions fed to rollout_tape on a twin batch are bitwise the same rollout."""
    twin_b = make()
    _first_obs(twin_b)
    twin_b.stats(reset=True); twin_b.replay_marks(reset=True)
    twin = tp._tape(twin_b, out["actions"], spl, terminal=terminal)
    assert np.isfinite(out["actions"]).all()
    tp._check(out, twin)
    if terminal:
        _same(out["term"], twin["term"], "terminal tape")
    return twin


def _start(make):
    b = make()
    obs0 = _first_obs(b)
    b.stats(reset=True); b.replay_marks(reset=True)
    return b, obs0


# ---- 1. replaying the recorded actions is bitwise the same rollout
@pytest.mark.parametrize("spl", SPLS)
@pytest.mark.parametrize("case", list(CASES))
def test_recorded_actions_replay_the_rollout_bitwise(case, spl):
    task, n, widths, act = CASES[case]
    make = lambda: _batch(task, n)
    b, obs0 = _start(make)
    out = _run(b, _policy(b, widths, act), spl, obs0)
    assert not (out["obs"] == OBS_FILL).all(2).any() and not (out["done"] == DONE_FILL).any()
    assert out["stats"]["env_steps"] == T * n
    _replayed_by_tape(make, out, spl)


# ---- 2. the launch split and the batch do not matter
@pytest.mark.parametrize("log_std", [None, -1.0])
@pytest.mark.parametrize("case", ["a1", "atlas"])
def test_launch_split_and_batch_size_do_not_change_an_action(case, log_std):
    task, n, widths, act = CASES[case]
    env, _, tab = tp._task(task)
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)]
    tapes = []
    for spl in SPLS:
        b, obs0 = _start(lambda: _batch(task, n, rows=rows))
        tapes.append(_run(b, _policy(b, widths, act, log_std), spl, obs0, noise_seed=9))
    for other in tapes[1:]:
        _same(other["actions"], tapes[0]["actions"], "action tape")
        _same(other["obs"], tapes[0]["obs"], "observation tape")
    # environment 3 alone (a workgroup with three padding quads; the same global id through the offset) and among five
    e = 3
    for m, first, spl in ((1, e, 3), (5, 0, T)):
        b = _batch(task, m, rows=rows[first:first + m])
        b.set_reset_table(tab[:4], seed=0, global_env_offset=first)          # (no auto-reset: the offset only)
        obs0 = _first_obs(b)
        out = _run(b, _policy(b, widths, act, log_std), spl, obs0, noise_seed=9)
        _same(out["actions"][:, e - first], tapes[0]["actions"][:, e], "actions of environment %d in a batch of %d" % (e, m))


# ---- 3. the actions are the MLP's
def _mlp64(policy, x, tanh_allowance=0.0):
    """float64 evaluation on float32 inputs x [m, nobs] beside the standard running error bound per layer:
    gamma_{n+2} (sum |w||x| + |b|) + sum |w| err_in — n products, n additions in sequence starting from the bias, each fmaf one
    rounding (gamma_{n+2} covers it with room); relu adds nothing (1-Lipschitz, exact), tanh (1-Lipschitz) its per-unit allowance.
    Returns (mean64, bound, pre-activations of the hidden layers)."""
    flat = policy.params.detach().cpu().numpy().astype(np.float64)
    h, err, at, pres = x.astype(np.float64), np.zeros(x.shape), 0, []
    for layer, (a, c) in enumerate(zip(policy.sizes[:-1], policy.sizes[1:])):
        W, bias = flat[at:at + a * c].reshape(c, a), flat[at + a * c:at + a * c + c]
        at += a * c + c
        k = a + 2
        gamma = k * U / (1 - k * U)
        z = h @ W.T + bias
        err = gamma * (np.abs(h) @ np.abs(W).T + np.abs(bias)) + err @ np.abs(W).T
        if layer < policy.n_layers - 1:
            pres.append(z)
            if policy.activation == 0:
                h, err = np.tanh(z), err + tanh_allowance
            else:
                h = np.maximum(z, 0)
        else:
            h = z
    return h, err, pres


def _tanh_allowance(pres):
    """Four times the largest |float32 torch.tanh on the device - float64 tanh| over the same pre-activations (rounded to float32)."""
    torch, dev = _torch()
    worst = 0.0
    for z in pres:
        z32 = z.astype(np.float32)
        t = torch.tanh(torch.from_numpy(z32).to(dev)).cpu().numpy().astype(np.float64)
        worst = max(worst, np.abs(t - np.tanh(z32.astype(np.float64))).max())
    return 4.0 * worst


def _check_actions_are_the_mlps(policy, out, obs0, label):
    prev = np.concatenate([obs0[None], out["obs"][:-1]])                      # [T, n, nobs]: what each step's action was computed from
    x = prev.reshape(-1, prev.shape[-1])
    _, _, pres = _mlp64(policy, x)
    allow = _tanh_allowance(pres) if (policy.activation == 0 and pres) else 0.0
    mean, bound, pres = _mlp64(policy, x, allow)
    err = np.abs(out["actions"].reshape(mean.shape).astype(np.float64) - mean)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print("%s: largest |action - float64 MLP| %.3e (its bound %.3e), largest bound %.3e, tanh allowance %.3e"
          % (label, err.max(), bound[np.unravel_index(np.argmax(err), err.shape)], bound.max(), allow))
    assert (err <= bound).all(), (label, err[worst], bound[worst])
    return mean, pres


@pytest.mark.parametrize("spl", [1, T])
@pytest.mark.parametrize("case", ["a1", "atlas", "torque", "muscle"])
def test_actions_are_the_mlps(case, spl):
    task, n, widths, act = CASES[case]
    b, obs0 = _start(lambda: _batch(task, n))
    policy = _policy(b, widths, act)
    out = _run(b, policy, spl, obs0)
    mean, pres = _check_actions_are_the_mlps(policy, out, obs0.cpu().numpy(), "%s, %d per launch" % (case, spl))
    assert out["actions"].std(axis=(0, 1)).min() > 1e-3                         # not constant, in any output
    if act == "tanh" and pres:
        assert max(np.abs(z).max() for z in pres) > 2.0                         # some hidden tanh unit is out of its linear range


# ---- 4. noise
def test_noise_is_seeded_and_off_without_log_std():
    task, n, widths, act = CASES["a1"]
    runs = {}
    for key, log_std, seed in (("a", -1.0, 5), ("b", -1.0, 5), ("c", -1.0, 6), ("none", None, 5), ("zero", -np.inf, 5)):
        b, obs0 = _start(lambda: _batch(task, n))
        runs[key] = _run(b, _policy(b, widths, act, log_std), 3, obs0, noise_seed=seed)["actions"]
    _same(runs["a"], runs["b"], "the same seed")
    assert (runs["a"] != runs["c"]).mean() > 0.99
    assert (runs["a"] != runs["none"]).mean() > 0.99
    _same(runs["zero"], runs["none"], "standard deviation 0 against no log_std: mean + 0 * z")


def test_noise_statistics():
    """z = (a - mean64) / exp(log_std) over 7 * 33 steps of 37 quadrupeds x 12 outputs = 102 564 samples (restarts every 20 steps keep
    the robots on their feet's side of the state space): mean, variance and the lag-1 correlations along step, environment and output."""
    task, n, widths, act = CASES["a1"]
    steps, log_std = 7 * 33, -1.0
    env, _, tab = tp._task(task)
    b, obs0 = _start(lambda: _batch(task, n, restarts=(tab, 20)))
    policy = _policy(b, widths, act, log_std)
    out = _run(b, policy, T, obs0, steps=steps, noise_seed=77)
    prev = np.concatenate([obs0.cpu().numpy()[None], out["obs"][:-1]])
    assert np.isfinite(prev).all()
    mean = _mlp64(policy, prev.reshape(-1, b.nobs))[0].reshape(out["actions"].shape)
    z = (out["actions"].astype(np.float64) - mean) / np.exp(log_std)
    m = z.size
    assert m >= 100000
    print("noise: m = %d, mean %.4f, var %.4f" % (m, z.mean(), z.var()))
    assert abs(z.mean()) < 5 / np.sqrt(m)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / m)
    for axis, name in ((0, "step"), (1, "environment"), (2, "output")):
        a, c = np.moveaxis(z, axis, 0)[1:], np.moveaxis(z, axis, 0)[:-1]
        corr = (a * c).mean() / z.var()
        print("noise: lag-1 correlation along %s %.5f" % (name, corr))
        assert abs(corr) < 5 / np.sqrt(m), (name, corr)
    per_env = z.transpose(1, 0, 2).reshape(n, -1)
    assert len(np.unique(per_env, axis=0)) == n


def test_noise_is_keyed_by_the_global_environment_id():
    task, n, widths, act = CASES["a1"]
    env, _, tab = tp._task(task)
    g, m = 11, 5
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)]
    whole = _batch(task, n, rows=rows)
    obs0 = _first_obs(whole)
    ref = _run(whole, _policy(whole, widths, act, -1.0), T, obs0, noise_seed=4)["actions"]
    part = _batch(task, m, rows=rows[g:g + m])
    part.set_reset_table(tab[:4], seed=0, global_env_offset=g)
    _first_obs(part)                                        # the same count of control steps as the whole batch: it is part of the key
    got =_run(part, _policy(part, widths, act, -1.0), T, obs0[g:g + m].contiguous(), noise_seed=4)["actions"]
    _same(got[0], ref[0, g:g + m], "step 0 of environments g .. g + 4")
    assert (got[0] != ref[0, :m]).all()


# ---- 5. hand-over to the replay kernel
@pytest.mark.parametrize("replay", [None, 2])
def test_replay_kernel_under_a_policy(replay):
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "ht_folded_states.npz"))
    task, n = "HumanoidTorque.run", 37
    env, _, tab = tp._task(task)
    nv = env._model.nv
    rows = tab[np.random.RandomState(3).randint(0, len(tab), n)].copy()
    k = min(len(d["q"]), n - 5)
    rows[:k, :nv], rows[:k, nv:2 * nv] = d["q"][:k], d["v"][:k]
    make = lambda: _batch(task, n, rows=rows, replay=replay)
    for spl in (3, T):
        b, obs0 = _start(make)
        out = _run(b, _policy(b, (40, 24), "tanh"), spl, obs0)
        print("steps per launch %d: %d env-steps replayed" % (spl, out["stats"]["replayed_env_steps"]))
        assert out["stats"]["replayed_env_steps"] >= 1
        if replay == 2:
            assert out["stats"]["replayed_env_steps"] == T * n
        _replayed_by_tape(make, out, spl)


# ---- 6. restarts, terminal rows, per-environment parameters, the model compiler
def _restart_table(task):
    env, _, tab = tp._task(task)
    table = tab[np.linspace(0, len(tab) - 1, 5).astype(int)]
    return table


@pytest.mark.parametrize("spl", [3, T])
@pytest.mark.parametrize("kind", ["plain", "joint parameters"])
def test_restarts_inside_a_launch_and_terminal_rows(kind, spl):
    """Horizon 3: restarts at steps 2 and 5, in the middle of a launch. The action after a restart is the MLP of the NEW episode's first
    observation (the row the step wrote), the terminal tape holds the observation the old one ended in."""
    task, n, widths, act = CASES["a1"]
    table = _restart_table(task)

    def make():
        b = _batch(task, n, restarts=(table, 3), terminal=True)
        if kind != "plain":
            b.set_dof_params(damping=np.full((n, b.nv), 0.5, dtype=np.float32))
        return b
    b, obs0 = _start(make)
    policy = _policy(b, widths, act)
    out = _run(b, policy, spl, obs0, terminal=True)
    _replayed_by_tape(make, out, spl, terminal=True)
    ended = (out["done"] & 2) != 0
    assert ended.sum() >= n and (out["term"][~ended] == OBS_FILL).all() and not (out["term"][ended] == OBS_FILL).all(1).any()
    assert not np.array_equal(out["term"][ended], out["obs"][ended])
    _check_actions_are_the_mlps(policy, out, obs0.cpu().numpy(), "restarts, %s, %d per launch" % (kind, spl))
    # without a terminal tape the batch's own buffer is written, as by rollout_tape
    b, obs0 = _start(make)
    out2 = _run(b, policy, spl, obs0)
    _same(out2["actions"], out["actions"], "action tape without a terminal tape")
    last = np.where(ended.any(0), T - 1 - np.argmax(ended[::-1], axis=0), -1)
    for e in np.nonzero(last >= 0)[0][:8]:
        _same(b.terminal_obs()[e], out["term"][last[e], e], "terminal buffer row %d" % e)


def _variant_batch(n):
    from loco_mujoco_amd import LocoEnv
    from loco_mujoco_amd.backend import HipBatch
    cfg = os.path.join(os.path.dirname(__file__), "golden", "dr_talos_inertial.yaml")
    np.random.seed(0)
    env = LocoEnv.make("Talos.walk", debug=True, n_envs=n, domain_randomization_config=cfg, n_model_variants=3)
    env.reset()
    nv = env._model.nv
    tab = env._reset_table()
    env.backend
    b = HipBatch(env._hip_model, n)
    b._keep_env = env
    b.set_model_variants(env._build_model_variants(env._chain_model())[1])
    rows = tab[(np.arange(n) * 7) % len(tab)]
    b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
    b.set_reset_table(tab, seed=5)
    b.set_auto_reset(True, horizon=3)
    return b


@pytest.mark.parametrize("spl", [3, T])
def test_model_variant_pool_under_a_policy(spl):
    n = 37
    make = lambda: _variant_batch(n)
    b, obs0 = _start(make)
    assert b.n_variants == 3
    out = _run(b, _policy(b, (40, 24), "tanh"), spl, obs0)
    _replayed_by_tape(make, out, spl)
    assert ((out["done"] & 2) != 0).sum() >= n


def test_model_compiler_runs_one_step_per_launch():
    n = 37
    make = lambda: tp._compiler_env(n).backend
    b, obs0 = _start(make)
    out = _run(b, _policy(b, (40, 24), "tanh"), 3, obs0)
    _replayed_by_tape(make, out, 3)
    assert ((out["done"] & 2) != 0).sum() >= 2 * n - 4


# ---- 7. a caller's stream, nothing waiting on the host
@pytest.mark.parametrize("task,replay", tp.SIDE_CASES)
def test_policy_rollout_on_a_side_stream_without_host_waits(task, replay):
    torch, dev = _torch()
    n = tp.SIDE_N

    def go(stream, sync):
        b = _batch(task, n, replay=replay)
        policy = _policy(b, (40, 24), "tanh", -1.0)
        obs = torch.full((T, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev)
        acts = torch.full((T, n, b.nu), OBS_FILL, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        kw = dict(stream=stream, sync=sync)
        b.step_device(**kw)                                       # the batch's own row: obs0 = None below
        b.rollout_policy(policy, 4, actions=acts[:4], obs=obs[:4], steps_per_launch=3, noise_seed=2, **kw)
        b.rollout_policy(policy, 3, obs0=obs[3], actions=acts[4:], obs=obs[4:], steps_per_launch=3, noise_seed=2, **kw)
        state = b.get_state()
        torch.cuda.synchronize(dev)
        return dict(state=state, obs=obs.cpu().numpy(), actions=acts.cpu().numpy())
    twin = go(None, True)
    side = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    out = go(side.cuda_stream, False)
    for k in ("obs", "actions"):
        _same(out[k], twin[k], k + " rows")
        assert not (twin[k] == OBS_FILL).all(2).any()
    _same(out["state"][0], twin["state"][0], "final qpos")
    _same(out["state"][1], twin["state"][1], "final qvel")


# ---- 8. refused calls launch nothing
def test_refused_calls_launch_nothing():
    import ctypes as C
    from loco_mujoco_amd.backend import MlpPolicyStruct
    torch, dev = _torch()
    task, n, widths, act = CASES["a1"]
    b, obs0 = _start(lambda: _batch(task, n))
    q0, v0 = b.get_state()
    policy = _policy(b, widths, act)
    acts = torch.full((T, n, b.nu), OBS_FILL, dtype=torch.float32, device=dev)
    term = torch.zeros((T, n, b.nobs), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)

    def raw(edit=None, actions=acts, d_term=None, spl=3, steps=T, null_policy=False):
        st = policy.struct()
        if edit:
            edit(st)
        return b._lib.lm_rollout_policy(b._h, None if null_policy else C.byref(st), steps, spl, 0, C.c_void_p(obs0.data_ptr()),
                                        None if actions is None else C.c_void_p(actions.data_ptr()), None, None, None,
                                        None if d_term is None else C.c_void_p(d_term.data_ptr()), None, 1, None)

    def sizes(i, v):
        def edit(st):
            st.sizes[i] = v
        return edit

    def field(name, v):
        def edit(st):
            setattr(st, name, v)
        return edit
    for call, word in ((lambda: raw(sizes(0, b.nobs + 1)), b"nobs"), (lambda: raw(sizes(3, b.nu - 1)), b"nu"), (lambda: raw(sizes(1, 0)), b"hidden width 0"),
                       (lambda: raw(sizes(2, 257)), b"hidden width 257"), (lambda: raw(field("n_layers", 4)), b"n_layers"),
                       (lambda: raw(field("n_layers", 0)), b"n_layers"), (lambda: raw(field("activation", 2)), b"activation"),
                       (lambda: raw(field("d_params", None)), b"d_params"), (lambda: raw(actions=None), b"d_actions"),
                       (lambda: raw(d_term=term), b"d_term"), (lambda: raw(spl=0), b"steps_per_launch"), (lambda: raw(steps=-1), b"n_steps"),
                       (lambda: raw(null_policy=True), b"policy is null")):
        assert call() != 0
        assert word in b._lib.lm_last_error(), b._lib.lm_last_error()
        q, v = b.get_state()
        assert np.array_equal(q, q0) and np.array_equal(v, v0)
    with pytest.raises(ValueError, match="terminal"):
        b.rollout_policy(policy, T, obs0=obs0, terminal=term)
    assert b.stats()["env_steps"] == 0 and (acts == OBS_FILL).all()
    # the count of control steps stayed: the batch runs what a twin that was never refused runs
    twin, obs0_t = _start(lambda: _batch(task, n))
    noisy = _policy(b, widths, act, -1.0)
    _same(_run(b, noisy, 3, obs0, noise_seed=1)["actions"], _run(twin, noisy, 3, obs0_t, noise_seed=1)["actions"], "actions after the refusals")
