"""
LocoVectorEnv's partial reset and state() (`-m gpu`): ``reset(options={"reset_mask": m})`` restarts chosen environments on the device
(HipBatch.restart_device) without a host wait, and ``state()`` reads qpos / qvel / ep_step as device tensors. 37 environments, horizon
3; A1, Atlas, and Atlas carrying a weight with foot forces, whose reference column order is not the kernel's.
"""

import numpy as np
import pytest

from loco_mujoco_amd import LocoVectorEnv

pytestmark = pytest.mark.gpu

N, HORIZON, SEED = 37, 3, 11
FILL = -7.0
MAKE_KW = {"Atlas.carry": dict(use_foot_forces=True)}
TASKS = ["UnitreeA1.simple", "Atlas.walk", "Atlas.carry"]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _venv(task, copy=False):
    np.random.seed(0)
    return LocoVectorEnv(task, N, seed=SEED, horizon=HORIZON, copy=copy, debug=True, **MAKE_KW.get(task, {}))


def _actions(venv, steps):
    torch, dev = _torch()
    nu = venv.single_action_space.shape[0]
    return torch.from_numpy(np.random.default_rng(77).uniform(-0.3, 0.3, (steps, N, nu)).astype(np.float32)).to(dev)


def _same(got, want, what):
    got, want = got.cpu().numpy(), want.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=True), \
        "%s differs at %s" % (what, np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("how", ["bool", "uint8", "numpy"])
@pytest.mark.parametrize("task", TASKS)
def test_partial_reset_replaces_the_masked_rows_and_waits_for_nothing(task, how, monkeypatch):
    """After a full reset and two steps: the observation returned has the rows of the masked environments replaced by what a
    backend-level restart_device writes on a twin (through the reference's column order where the task has one), the other rows are
    the previous step's; torch.cuda.synchronize is not called."""
    torch, dev = _torch()
    A, B = _venv(task), _venv(task)
    acts = _actions(A, 3)
    for v in (A, B):
        np.random.seed(1)                                       # the host reset draws from np.random: the twins start alike
        v.reset()
        for t in range(2):
            prev = v.step(acts[t])[0]
        prev = prev.clone()
    mask = np.arange(N) % 3 != 0
    m = torch.from_numpy(mask).to(dev)
    given = {"bool": m, "uint8": m.to(torch.uint8), "numpy": mask}[how]
    # the twin: the backend's call, raw columns
    bb = B.unwrapped.backend
    raw = torch.full((N, bb.nobs), FILL, dtype=torch.float32, device=dev)
    bb.restart_device(m, obs=raw)
    want_rows = raw if B._perm is None else raw.index_select(1, B._perm)
    torch.cuda.synchronize(dev)

    def refuse(*a, **kw):
        raise AssertionError("torch.cuda.synchronize was called")

    monkeypatch.setattr(torch.cuda, "synchronize", refuse)
    obs, info = A.reset(options={"reset_mask": given})
    monkeypatch.undo()
    assert info == {} and tuple(obs.shape) == (N, bb.nobs)
    _same(obs[m], want_rows[m], "rows of the restarted environments")
    _same(obs[~m], prev[~m], "rows of the others")
    assert not (obs[m] == prev[m]).all(1).any()
    if task == "Atlas.carry":
        assert A._perm is not None                              # the case is the permuted one
    # both continue alike: the partial reset is the twin's restart, nothing else
    oa, ob = A.step(acts[2]), B.step(acts[2])
    for x, y, what in zip(oa[:4], ob[:4], ("obs", "reward", "terminated", "truncated")):
        _same(x, y, what + " of the step after the partial reset")
    A.close(); B.close()


def test_episode_statistics_count_from_the_partial_reset():
    """Horizon 3: one step, a partial reset, three more steps. The environments that were not reset run into the horizon at step 3
    with length 3; the reset ones at step 4, with length 3 — counted from the partial reset — and the float32 sum of the three rewards
    since it as their return."""
    torch, dev = _torch()
    venv = _venv("UnitreeA1.simple", copy=True)
    acts = _actions(venv, 4)
    venv.reset()
    mask = torch.from_numpy(np.arange(N) % 2 == 0).to(dev)
    out = [venv.step(acts[0])]
    venv.reset(options={"reset_mask": mask})
    out += [venv.step(acts[t]) for t in (1, 2, 3)]
    rew = [o[1] for o in out]
    fell = torch.stack([o[2] for o in out]).any(0)
    # step 3 (index 2): the environments that were not reset reach the horizon
    trunc3, info3 = out[2][3], out[2][4]
    assert (trunc3[~mask] | fell[~mask]).all() and not trunc3[mask].any()
    up = ~mask & ~fell
    assert up.sum() >= N // 4 and (info3["episode"]["l"][up] == 3).all()
    # step 4 (index 3): the reset ones do, three steps after the partial reset
    trunc4, info4 = out[3][3], out[3][4]
    up = mask & ~fell
    assert up.sum() >= N // 4 and trunc4[up].all() and info4["_episode"][up].all()
    assert (info4["episode"]["l"][up] == 3).all()
    _same(info4["episode"]["r"][up], ((rew[1] + rew[2]) + rew[3])[up], "return since the partial reset")
    venv.close()


def test_partial_reset_right_after_a_full_reset_keeps_its_rows():
    torch, dev = _torch()
    venv = _venv("UnitreeA1.simple")
    first = venv.reset()[0].clone()
    mask = torch.from_numpy(np.arange(N) % 5 == 1).to(dev)
    obs = venv.reset(options={"reset_mask": mask})[0]
    _same(obs[~mask], first[~mask], "rows of the full reset")
    assert (obs[mask] != first[mask]).any(1).sum() > mask.sum() // 2      # (a drawn row may be the dataset row the host reset drew)
    kept = obs[mask].clone()                                    # (obs is a view of the result set: the next call writes into it)
    again = venv.reset(options={"reset_mask": ~mask})[0]
    _same(again[mask], kept, "rows of the first partial reset")
    assert (again[~mask] != first[~mask]).any(1).sum() > (~mask).sum() // 2
    with pytest.raises(ValueError, match="reset_mask must be"):
        venv.reset(options={"reset_mask": torch.zeros(N + 1, dtype=torch.bool, device=dev)})
    with pytest.raises(ValueError, match="takes no seed"):
        venv.reset(seed=3, options={"reset_mask": mask})
    venv.close()


@pytest.mark.parametrize("task", ["UnitreeA1.simple", "Atlas.carry"])
def test_two_partial_resets_before_any_step_keep_the_uncovered_rows(task):
    """reset(), reset(mask1), reset(mask2) with no step in between, the masks overlapping and together leaving rows out — also where the
    reference's column order is not the kernel's (Atlas.carry): the rows in neither mask are the full reset's, the rows only the first
    mask covers keep what the first partial reset gave them, and a twin that takes the same three calls at the backend gives the rows
    of the second mask."""
    torch, dev = _torch()
    A, B = _venv(task), _venv(task)
    np.random.seed(1)                                           # the host reset draws from np.random: the twins start alike
    B.reset()
    np.random.seed(1)
    first = A.reset()[0].clone()
    if task == "Atlas.carry":
        assert A._perm is not None
    idx = np.arange(N)
    m1, m2 = torch.from_numpy(idx % 3 == 0).to(dev), torch.from_numpy((idx % 3 == 1) | (idx % 6 == 0)).to(dev)
    neither, only1 = ~(m1 | m2), m1 & ~m2
    assert neither.sum() >= 8 and only1.sum() >= 4 and (m1 & m2).sum() >= 4
    one = A.reset(options={"reset_mask": m1})[0].clone()
    _same(one[~m1], first[~m1], "after the first partial reset: rows of the full reset")
    two = A.reset(options={"reset_mask": m2})[0].clone()
    _same(two[neither], first[neither], "after the second partial reset: rows in neither mask")
    _same(two[only1], one[only1], "after the second partial reset: rows of the first mask alone")
    # the twin: the same restarts at the backend, raw columns brought into the reference's order
    env, bb = B.unwrapped, B.unwrapped.backend
    if env._pending_state:
        env._upload_state()
    raw = torch.full((N, bb.nobs), FILL, dtype=torch.float32, device=dev)
    bb.restart_device(m1, obs=raw)
    bb.restart_device(m2, obs=raw)
    want = raw if B._perm is None else raw.index_select(1, B._perm)
    _same(two[m2], want[m2], "rows of the second mask")
    _same(one[only1], want[only1], "rows of the first mask alone")
    assert (two[m2] != first[m2]).any(1).sum() > m2.sum() // 2
    A.close(); B.close()


def test_state_is_the_batchs_state_on_the_device():
    torch, dev = _torch()
    venv = _venv("UnitreeA1.simple")
    acts = _actions(venv, 2)
    venv.reset()
    for t in range(2):
        venv.step(acts[t])
    st = venv.state()
    b = venv.unwrapped.backend
    q, v = b.get_state()
    assert sorted(st) == ["ep_step", "qpos", "qvel"] and all(x.is_cuda for x in st.values())
    assert tuple(st["qpos"].shape) == (N, b.nv) and st["qpos"].dtype == torch.float32 and st["ep_step"].dtype == torch.int32
    torch.cuda.synchronize(dev)
    assert np.array_equal(st["qpos"].cpu().numpy(), q) and np.array_equal(st["qvel"].cpu().numpy(), v)
    assert (st["ep_step"] <= 2).all() and (st["ep_step"] == 2).sum() >= N // 2
    assert st["qpos"][:, 0].abs().max() > 0                     # the root's horizontal position: in no observation column
    venv.close()
