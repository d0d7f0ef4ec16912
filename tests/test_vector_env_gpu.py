"""
The vector environment on the device (`-m gpu`): lv_finish_step (include/locovec.h) BITWISE against the numpy model of
tests/vector_finish_model.py at the smallest shapes that can go wrong — 1, 255 and 257 environments (one short of and one past a
workgroup of 256 lanes), rows of 1 and 37 columns, done bytes 0 to 3, every optional buffer present and absent — and LocoVectorEnv
against the numpy surface: a twin LocoEnv made under the same seeds takes the same eight steps, with horizon 3 so that every environment
ends at least two episodes (A1, Atlas, and Atlas carrying a weight with foot forces, whose reference column order is not the kernel's).
"""

import functools

import numpy as np
import pytest

import vector_finish_model as M
from loco_mujoco_amd import LocoEnv, LocoVectorEnv, vector

pytestmark = pytest.mark.gpu

STEPS, HORIZON, SEED = 8, 3, 11
TASKS = (("UnitreeA1.simple", 5), ("Atlas.walk", 37))
# a carried weight with foot forces: the reference's column order is not the kernel's (LocoEnv._obs_perm), and the four weights share
# one batch as model variants
PERMUTED = ("Atlas.carry", 6)
MAKE_KW = {"Atlas.carry": dict(use_foot_forces=True)}


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _dev(a):
    torch, dev = _torch()
    return None if a is None else torch.from_numpy(np.array(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%s differs at %s" % (what, np.argwhere(_bits(got) != _bits(want))[:4].tolist())


def _call(n, nobs, inputs, state, with_term, with_final, with_acc, with_ep):
    """One lv_finish_step call on fresh device copies of `inputs` and `state`; returns what the model returns, from the device."""
    torch, dev = _torch()
    obs, rew, done, term = inputs
    d = dict(obs=_dev(obs), reward=_dev(rew), done=_dev(done), term=_dev(term) if with_term else None,
             terminated=torch.full((n,), 9, dtype=torch.uint8, device=dev), truncated=torch.full((n,), 9, dtype=torch.uint8, device=dev),
             final_obs=_dev(state["final_obs"]) if with_final else None,
             run_return=_dev(state["run_return"]) if with_acc else None, run_length=_dev(state["run_length"]) if with_acc else None,
             ep_return=torch.full((n,), -3.0, dtype=torch.float32, device=dev) if with_ep else None,
             ep_length=torch.full((n,), -3, dtype=torch.int32, device=dev) if with_ep else None)
    vector.finish_step(n, nobs, **d)               # the null stream, behind torch's copies on it; waits
    keys = ("terminated", "truncated", "final_obs", "run_return", "run_length", "ep_return", "ep_length")
    got = {k: None if d[k] is None else d[k].cpu().numpy() for k in keys}
    for k, x in (("obs", obs), ("reward", rew), ("done", done)) + ((("term", term),) if with_term else ()):
        _same_bits(d[k].cpu().numpy(), x, "the input " + k)          # inputs are read only
    return got


@pytest.mark.parametrize("nobs", M.NOBS_CASES)
@pytest.mark.parametrize("n", M.N_CASES)
def test_the_kernel_is_bitwise_the_model(n, nobs):
    """Three calls in a row carry the accumulators and the sentinel-filled final_obs; a NaN reward in the second call. Every
    combination of the optional buffers; the same call on fresh copies twice gives the same bits."""
    nan_env = min(2, n - 1)
    for with_term in (True, False):
        for with_final, with_acc, with_ep in ((True, True, True), (False, True, True), (True, True, False), (True, False, False),
                                              (False, False, False)):
            state = dict(final_obs=np.full((n, nobs), M.SENTINEL, np.float32), run_return=np.zeros(n, np.float32),
                         run_length=np.zeros(n, np.int32))
            ended_rows = kept_rows = 0
            for call in (1, 2, 3):
                inputs = M.synthetic_step(n, nobs, seed=call, nan_at=nan_env if call == 2 else None)
                obs, rew, done, term = inputs
                want = M.finish(obs, rew, done, term=term if with_term else None, final_obs=state["final_obs"] if with_final else None,
                                run_return=state["run_return"] if with_acc else None,
                                run_length=state["run_length"] if with_acc else None, want_ep=with_ep)
                got = _call(n, nobs, inputs, state, with_term, with_final, with_acc, with_ep)
                label = "n=%d nobs=%d term=%d final=%d acc=%d ep=%d call %d: " % (n, nobs, with_term, with_final, with_acc, with_ep, call)
                for k, w in want.items():
                    assert (got[k] is None) == (w is None), label + k
                    if w is not None:
                        _same_bits(got[k], w, label + k)
                if call == 2 and (with_final or with_acc):
                    again = _call(n, nobs, inputs, state, with_term, with_final, with_acc, with_ep)
                    for k, g in got.items():
                        if g is not None:
                            _same_bits(again[k], g, label + k + " (the same call again)")
                if with_final:
                    ended_rows += int((done != 0).sum())
                    kept_rows += int((got["final_obs"] == M.SENTINEL).all(1).sum())
                for k in state:
                    if want[k] is not None:
                        state[k] = want[k]
            if with_final:
                assert ended_rows >= 1 and (kept_rows >= 1 or n == 1)           # both kinds of rows were there
            if with_acc and with_ep and n > 1:
                assert np.isnan(want["ep_return"]).any() or np.isnan(state["run_return"]).any()      # the NaN was carried


@functools.lru_cache(maxsize=None)
def _actions(task, n):
    nu = len(LocoEnv.make(task, debug=True, **MAKE_KW.get(task, {}))._action_indices)
    a = np.random.default_rng(77).uniform(-1, 1, (STEPS, n, nu)).astype(np.float32)
    a.setflags(write=False)
    return a


def _vec_run(task, n, side=False, copy=False, steps=STEPS, ring=False):
    """`steps` steps of a fresh LocoVectorEnv; every step's results copied into stacks ON THE DEVICE (no host wait between the steps),
    brought to the host after one synchronise. `ring`: the checks of the result ring, between the steps (they wait for the device)."""
    torch, dev = _torch()
    acts = _dev(_actions(task, n))
    np.random.seed(0)
    venv = LocoVectorEnv(task, n, seed=SEED, horizon=HORIZON, copy=copy, debug=True, **MAKE_KW.get(task, {}))
    nobs = venv.single_observation_space.shape[0]
    assert venv.num_envs == n and venv.observation_space.shape == (n, nobs) and venv.action_space.shape == (n, acts.shape[2])
    assert venv.device == dev and venv.unwrapped.n_envs == n and venv.metadata["autoreset_mode"] in ("SameStep", vector.SAME_STEP)
    with pytest.raises(RuntimeError, match="reset"):
        venv.step(acts[0])
    stream = torch.cuda.Stream(device=dev) if side else torch.cuda.current_stream(dev)
    shapes = dict(obs=((nobs,), torch.float32), reward=((), torch.float32), terminated=((), torch.bool), truncated=((), torch.bool),
                  final_obs=((nobs,), torch.float32), ended=((), torch.bool), ep_r=((), torch.float32), ep_l=((), torch.int32))
    stacks = {k: torch.zeros((steps, n) + s, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}
    torch.cuda.synchronize(dev)
    kept = []
    with torch.cuda.stream(stream):
        obs0, info0 = venv.reset()
        assert info0 == {} and obs0.shape == (n, nobs) and obs0.dtype == torch.float32 and obs0.device == dev
        for t in range(steps):
            obs, rew, term, trunc, info = venv.step(acts[t])
            assert set(info) == {"final_obs", "_final_obs", "episode", "_episode"} and set(info["episode"]) == {"r", "l"}
            assert info["_episode"] is info["_final_obs"] or copy
            res = dict(obs=obs, reward=rew, terminated=term, truncated=trunc, final_obs=info["final_obs"], ended=info["_final_obs"],
                       ep_r=info["episode"]["r"], ep_l=info["episode"]["l"])
            for k, x in res.items():
                assert x.shape == stacks[k][t].shape and x.dtype == stacks[k].dtype and x.device == dev, k
                stacks[k][t].copy_(x)
            if ring or copy:
                kept.append((res, {k: x.clone() for k, x in res.items()}))
            if ring and t >= 2:
                # step t - 1 is intact after step t; step t - 2 has been overwritten by step t (the same memory, this step's values)
                for k in res:
                    assert torch.equal(kept[t - 1][0][k], kept[t - 1][1][k]), (t, k)
                    assert kept[t - 2][0][k].data_ptr() == res[k].data_ptr() and torch.equal(kept[t - 2][0][k], res[k]), (t, k)
                assert not torch.equal(kept[t - 2][0]["obs"], kept[t - 2][1]["obs"])
    if side:
        assert stream.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    if copy:
        ptrs = [x.data_ptr() for res, _ in kept for x in res.values()]
        assert len(set(ptrs)) == len(ptrs)                      # fresh tensors every step
        for res, clone in kept:
            for k in res:
                assert torch.equal(res[k], clone[k]), k           # ... which no later step has written
    out = {k: x.cpu().numpy() for k, x in stacks.items()}
    out["obs0"] = obs0.cpu().numpy()
    venv.close()
    return out


@functools.lru_cache(maxsize=None)
def _vec(task, n):
    return _vec_run(task, n, ring=True)


@functools.lru_cache(maxsize=None)
def _twin(task, n):
    """The numpy surface: LocoEnv.step under the same seeds and actions."""
    acts = _actions(task, n)
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, n_envs=n, **MAKE_KW.get(task, {}))
    obs0 = env.reset()
    env.enable_auto_reset(seed=SEED, horizon=HORIZON, terminal_observations=True)
    out = dict(obs0=obs0.copy(), obs=[], reward=[], absorbing=[], restarted=[], term=[])
    for t in range(STEPS):
        obs, rew, absorbing, info = env.step(acts[t].astype(np.float64))
        for k, x in (("obs", obs), ("reward", rew), ("absorbing", absorbing), ("restarted", info["episode_restarted"]),
                     ("term", info["terminal_observation"])):
            out[k].append(np.array(x))
    return {k: np.stack(v) if isinstance(v, list) else v for k, v in out.items()}


@pytest.mark.parametrize("task,n", TASKS + (PERMUTED,))
def test_against_the_numpy_surface(task, n):
    v, w = _vec(task, n), _twin(task, n)
    if (task, n) == PERMUTED:
        assert LocoEnv.make(task, debug=True, **MAKE_KW[task])._obs_perm() is not None
    assert np.array_equal(v["obs0"], w["obs0"].astype(np.float32))
    assert v["obs"].dtype == np.float32 and w["obs"].dtype == np.float64
    assert np.array_equal(v["obs"].astype(np.float64), w["obs"]) and np.array_equal(v["reward"].astype(np.float64), w["reward"])
    assert np.array_equal(v["terminated"], w["absorbing"])
    ended = v["terminated"] | v["truncated"]
    assert np.array_equal(ended, w["restarted"]) and np.array_equal(v["ended"], ended) and not (v["terminated"] & v["truncated"]).any()
    # no episode is longer than 3 steps, so every environment ends at least twice in 8: the comparison cannot pass empty
    assert ended.sum(0).min() >= 2 and ended.sum() >= 2 * n and v["truncated"][HORIZON - 1].any()
    assert np.array_equal(v["final_obs"][ended].astype(np.float64), w["term"][ended])
    assert not np.array_equal(v["final_obs"][ended], v["obs"][ended])         # (the new episode's first observation is another)


@pytest.mark.parametrize("task,n", TASKS)
def test_episode_statistics(task, n):
    """Lengths: 3 at every truncation. Returns: bitwise what EpisodeMeter.update reports from the stacked reward and done of the run —
    both add in float32, in step order."""
    from loco_mujoco_amd.tapes import EpisodeMeter
    v = _vec(task, n)
    ended = v["ended"]
    assert ended.sum() >= 2 * n and (v["ep_l"][v["truncated"]] == HORIZON).all() and v["truncated"].any()
    assert (v["ep_l"][~ended] == 0).all() and (v["ep_r"][~ended] == 0).all() and (v["ep_l"][ended] >= 1).all()
    done = (v["terminated"].astype(np.uint8) | (v["truncated"].astype(np.uint8) << 1)).astype(np.uint8)
    ep = EpisodeMeter(n, device="cuda:0").update(_dev(v["reward"]), _dev(done), want=("ret", "length"))
    ret, length = ep.ret.cpu().numpy(), ep.length.cpu().numpy()
    assert np.array_equal(~np.isnan(ret), ended) or np.isnan(v["reward"]).any()
    _same_bits(v["ep_r"][ended], ret[ended], "episode returns")
    assert np.array_equal(v["ep_l"][ended], length[ended])


def test_results_are_views_of_a_ring_of_two():
    """Step t's results are unchanged after step t + 1 and overwritten by step t + 2 (checked between the steps of the shared run);
    copy=True returns tensors of their own that no later step writes, with the same values."""
    task, n = TASKS[0]
    v = _vec(task, n)
    c = _vec_run(task, n, copy=True, steps=4)
    for k in ("obs", "reward", "terminated", "truncated", "ended", "ep_r", "ep_l"):
        _same_bits(c[k], v[k][:4], k)
    ended = v["ended"][:4]
    _same_bits(c["final_obs"][ended], v["final_obs"][:4][ended], "final_obs")


def test_steps_on_a_side_stream_without_host_waits():
    """Eight steps queued on a torch side stream (not the current one), every result copied on that stream, then ONE synchronise: the
    results are bitwise those of the run on the current stream."""
    task, n = TASKS[0]
    v, s = _vec(task, n), _vec_run(task, n, side=True)
    for k in ("obs0", "obs", "reward", "terminated", "truncated", "ended", "ep_r", "ep_l"):
        _same_bits(s[k], v[k], k)
    _same_bits(s["final_obs"][v["ended"]], v["final_obs"][v["ended"]], "final_obs")


def test_actions_are_checked():
    torch, dev = _torch()
    task, n = TASKS[0]
    np.random.seed(0)
    venv = LocoVectorEnv(task, n, seed=SEED, debug=True)
    venv.reset()
    nu = venv.single_action_space.shape[0]
    for bad, word in ((torch.zeros(n, nu), "must live on the device"), (torch.zeros(n, nu, dtype=torch.float64, device=dev), "must be float32"),
                      (torch.zeros(n + 1, nu, device=dev), r"must be \[%d, %d\]" % (n, nu)), (np.zeros((n, nu), np.float32), "must be a device tensor")):
        with pytest.raises(ValueError, match="LocoVectorEnv.step: actions " + word):
            venv.step(bad)
    venv.close()


def test_construction_refusals_launch_nothing(monkeypatch):
    from loco_mujoco_amd import backend
    made = []
    for cls in (backend.HipModel, backend.HipBatch):
        init = cls.__init__
        monkeypatch.setattr(cls, "__init__", lambda self, *a, _init=init, **kw: (made.append(type(self).__name__), _init(self, *a, **kw))[1])
    with pytest.raises(NotImplementedError, match="LocoVectorEnv: the reward is evaluated on the host"):
        LocoVectorEnv("UnitreeA1.simple", 4, debug=True, use_foot_forces=True)
    with pytest.raises(NotImplementedError, match="LocoVectorEnv: several models in one batch"):
        LocoVectorEnv("HumanoidTorque4Ages.walk.all", 8, debug=True)
    assert made == []                                            # no model, no batch: nothing reached the device
