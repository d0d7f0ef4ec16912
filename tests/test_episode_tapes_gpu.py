"""
Episode returns and lengths from the tapes (include/locotape.h lt_tape_episodes, tapes.EpisodeMeter; `-m gpu`). T = 7; n = 37 is one
partial workgroup of 256 lanes, n = 300 two workgroups (the cross-workgroup sum of the summary). The tapes are those of
tests/episode_tape_model.py (done bytes from {0, 1, 2, 3}, a column without an end, a column ending in every step, ends at t = 0 and
t = T - 1); the reference is its float64 loop with its own rounding bound, and the summary is held to float64 numpy sums of the float32
episode values the call returned. Everything that is promised not to depend on the split, the place or the batch is compared BITWISE.
"""

import ctypes as C
import functools

import numpy as np
import pytest

import episode_tape_model as M
import test_policy_rollout_gpu as pr
import test_rollout_tape_gpu as tp
from episode_tape_model import T

pytestmark = pytest.mark.gpu

GAMMA = 0.99
FILL, LEN_FILL = -7.0, -9                      # sentinels of rows that must not be written (raw calls)
KEYS = ("ret", "disc", "length", "trace")


def _meter(n, gamma=GAMMA):
    from loco_mujoco_amd.tapes import EpisodeMeter
    return EpisodeMeter(n, device=pr._torch()[1], gamma=gamma)


def _dev(a):
    torch, dev = pr._torch()
    return torch.from_numpy(np.array(a)).to(dev)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), \
        "%s differs at %s" % (what, np.argwhere(_bits(a) != _bits(b))[:4].tolist())


def _state(meter):
    return dict(carry=meter.carry.cpu().numpy(), carry_length=meter.length.cpu().numpy(), summary=meter.summary_raw())


def _scan(r, d, gamma=GAMMA, splits=(T,), mask=None):
    """The tapes through EpisodeMeter.update, one call per entry of ``splits``: the episode tapes and the trace stacked, the final carry
    and the accumulated device summary."""
    torch, dev = pr._torch()
    assert sum(splits) == r.shape[0]
    meter = _meter(r.shape[1], gamma)
    dr, dd, dm = _dev(r), _dev(d), (None if mask is None else _dev(mask))
    parts, at = [], 0
    for k in splits:
        parts.append(meter.update(dr[at:at + k], dd[at:at + k], want=("ret", "disc", "length"), trace=True, mask=dm))
        at += k
    out = {key: torch.cat([getattr(p, key) for p in parts]).cpu().numpy() for key in KEYS}
    out.update(_state(meter), meter=meter)
    return out


@functools.lru_cache(maxsize=None)
def _result(n, gamma=GAMMA):
    r, d = M.synthetic_tapes(n)
    return _scan(r, d, gamma)


def _raw(meter, dr, dd, outs, n_steps=None, n_envs=None, gamma=None, accumulate=1, null=(), mask=None):
    """lt_tape_episodes through ctypes on the meter's carry, scratch and summary, with the caller's (sentinel-filled) output tensors."""
    p = dict(reward=dr, done=dd, carry=meter.carry, len=meter.length, summary=meter._summary, work=meter._work, **outs)
    q = {k: (None if (k in null or x is None) else C.c_void_p(x.data_ptr())) for k, x in p.items()}
    return meter._lib.lt_tape_episodes(dr.shape[0] if n_steps is None else n_steps, meter.n if n_envs is None else n_envs, q["reward"], q["done"],
                                       None if mask is None else C.c_void_p(mask.data_ptr()), meter.gamma if gamma is None else gamma,
                                       q["carry"], q["len"], q["ret"], q["disc"], q["length"], q["trace"], q["summary"], accumulate, q["work"], None, 1)


def _sentinels(steps, n):
    torch, dev = pr._torch()
    outs = dict(ret=torch.full((steps, n), FILL, dtype=torch.float32, device=dev), disc=torch.full((steps, n), FILL, dtype=torch.float32, device=dev),
                length=torch.full((steps, n), LEN_FILL, dtype=torch.int32, device=dev), trace=torch.full((steps, n), FILL, dtype=torch.float32, device=dev))
    torch.cuda.synchronize(dev)
    return outs


def _raw_scan(r, d, gamma=GAMMA):
    meter = _meter(r.shape[1], gamma)
    outs = _sentinels(*r.shape)
    rc = _raw(meter, _dev(r), _dev(d), outs, accumulate=0)
    assert rc == 0, meter._lib.lt_last_error()
    meter._fresh = False
    out = {k: v.cpu().numpy() for k, v in outs.items()}
    out.update(_state(meter))
    return out


def _check_values(out, r, d, gamma, label, mask=None):
    m = M.episodes64(r, d, gamma, mask=mask)
    ended = (d != 0) if mask is None else (d != 0) & (np.asarray(mask) != 0)[None, :]
    assert np.array_equal(out["length"], m["length"]) and np.array_equal(out["carry_length"], m["carry_length"])
    assert np.array_equal(np.isnan(out["ret"]), ~ended) and np.array_equal(np.isnan(out["disc"]), ~ended)
    tiny = np.finfo(np.float64).tiny
    worst = {}
    for key, bound in (("ret", "b_ret"), ("disc", "b_disc"), ("trace", "b_trace"), ("carry", "b_carry")):
        where = ended if key in ("ret", "disc") else ~np.isnan(m[key])
        err = np.abs(out[key].astype(np.float64) - m[key])[where]
        worst[key] = (err / np.maximum(m[bound][where], tiny)).max() if err.size else 0.0
    print("%s: worst |error| / bound %s" % (label, {k: round(float(v), 3) for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values()), (label, worst)


def _check_summary(raw, out, d, label, mask=None):
    values, bounds = M.summary_of(out["ret"], out["disc"], out["length"], d, mask=mask)
    for f, got in zip(M.SUMMARY, raw):
        print("%s: summary %s = %r, numpy %r, bound %.3g" % (label, f, float(got), float(values[f]), bounds[f]))
    for f, got in zip(M.SUMMARY, raw):
        if f in M.EXACT:
            assert got == values[f], (label, f, got, values[f])
        else:
            assert abs(got - values[f]) <= bounds[f], (label, f, got, values[f], bounds[f])
    return values


# ---- 1. against the float64 model, with the summary
@pytest.mark.parametrize("gamma", [0.0, GAMMA, 1.0])
@pytest.mark.parametrize("n", [37, 300])
def test_values_against_the_float64_model(n, gamma):
    r, d = M.synthetic_tapes(n)
    out = _result(n, gamma)
    label = "n %d, gamma %g" % (n, gamma)
    _check_values(out, r, d, gamma, label)
    values = _check_summary(out["summary"], out, d, label)
    assert values["episodes"] >= T + 9 and values["absorbing"] > 0 and values["L_max"] > values["L_min"] == 1
    # the dict a logger reads: the same numbers; reset starts a new summary at the next update, the carry stays
    meter = out["meter"]
    s = meter.summary(reset=False)
    k = values["episodes"]
    assert set(s) == {"episodes", "R_mean", "R_std", "R_min", "R_max", "J_mean", "L_mean", "L_min", "L_max", "absorbing_share"}
    assert s["episodes"] == k and s["R_mean"] == out["summary"][1] / k and s["J_mean"] == out["summary"][5] / k
    assert s["L_mean"] == values["L_sum"] / k and s["absorbing_share"] == values["absorbing"] / k and (s["R_min"], s["R_max"]) == (values["R_min"], values["R_max"])
    assert np.isclose(s["R_std"], np.std(out["ret"][d != 0].astype(np.float64)), rtol=1e-9, atol=1e-12)


def test_update_returns_what_was_asked_for_and_summary_resets():
    r, d = M.synthetic_tapes(37)
    meter = _meter(37)
    empty = meter.summary()
    assert empty["episodes"] == 0 and np.isnan(empty["R_mean"]) and np.isnan(empty["L_mean"]) and empty["R_min"] == np.inf and empty["L_max"] == -np.inf
    dr, dd = _dev(r), _dev(d)
    ep = meter.update(dr[:3], dd[:3])
    assert set(vars(ep)) == {"ret", "length"} and ep.ret.shape == (3, 37) and str(ep.length.dtype) == "torch.int32"
    _same_bits(ep.ret.cpu().numpy(), _result(37)["ret"][:3], "ret of the first three steps")
    first = meter.summary(reset=True)
    assert first["episodes"] == (d[:3] != 0).sum()
    ep = meter.update(dr[3:], dd[3:], want="disc", trace=True)
    assert set(vars(ep)) == {"disc", "trace"}
    _same_bits(ep.disc.cpu().numpy(), _result(37)["disc"][3:], "disc of the last four steps")        # the carry ran on over the reset
    assert meter.summary(reset=False)["episodes"] == (d[3:] != 0).sum()                             # ... and the summary started anew
    assert meter.summary()["episodes"] == (d[3:] != 0).sum() and meter.summary()["episodes"] == 0


# ---- 2. the split over calls changes nothing
@pytest.mark.parametrize("n", [37, 300])
def test_split_invariance_is_bitwise(n):
    r, d = M.synthetic_tapes(n)
    whole = _result(n)
    for splits in ((3, 4), (1,) * T):
        out = _scan(r, d, splits=splits)
        for key in KEYS + ("carry", "carry_length"):
            _same_bits(out[key], whole[key], "%s under the split %s" % (key, splits))
        _check_summary(out["summary"], out, d, "n %d, split %s" % (n, splits))


# ---- 3. nor does the place in the batch
def test_a_column_is_independent_of_its_place_and_of_the_batch():
    r37, d37 = M.synthetic_tapes(37)
    r, d = (np.array(a) for a in M.synthetic_tapes(300, seed=7))
    pairs = [(5, 280), (M.EVERY_STEP, 0), (M.NO_END, 299), (2, 255), (11, 256)]
    for e, at in pairs:
        r[:, at], d[:, at] = r37[:, e], d37[:, e]
    out, small = _scan(r, d), _result(37)
    for e, at in pairs:
        for key in KEYS:
            _same_bits(out[key][:, at], small[key][:, e], "%s of column %d at %d" % (key, e, at))
        _same_bits(out["carry"][:, at], small["carry"][:, e], "carry")
        assert out["carry_length"][at] == small["carry_length"][e]


# ---- 4. a NaN ends with its episode
def test_a_poisoned_reward_stays_inside_its_episode():
    r, d = M.synthetic_tapes(37)
    ends = [np.nonzero(d[:, e] != 0)[0] for e in range(37)]
    c = next(e for e in range(37) if e != M.EVERY_STEP and len(ends[e]) >= 2 and ends[e][0] >= 1)
    t1 = ends[c][0]
    bad = np.array(r)
    bad[0, c] = bad[2, M.EVERY_STEP] = np.nan
    clean, out = _raw_scan(r, d), _raw_scan(bad, d)
    for key, fill in (("ret", FILL), ("disc", FILL), ("length", LEN_FILL)):          # the raw call is update()'s, on sentinels of its own
        _same_bits(clean[key], np.where(d != 0, _result(37)[key], np.array(fill, dtype=clean[key].dtype)), key + " of the raw call")
    _same_bits(clean["trace"], _result(37)["trace"], "trace of the raw call")
    hit = np.zeros((T, 37), dtype=bool)                  # the steps of the two poisoned episodes
    hit[:t1 + 1, c] = True
    hit[2, M.EVERY_STEP] = True
    assert np.isnan(out["trace"][hit]).all() and np.isnan(out["ret"][t1, c]) and np.isnan(out["disc"][t1, c])
    assert np.isnan(out["ret"][2, M.EVERY_STEP]) and np.isnan(out["disc"][2, M.EVERY_STEP])
    for key in ("ret", "disc", "trace"):
        assert np.array_equal(_bits(out[key])[~hit], _bits(clean[key])[~hit]), key         # the next episode of c, and every other environment
    _same_bits(out["length"], clean["length"], "lengths")
    _same_bits(out["carry"], clean["carry"], "carry")
    # sentinel-filled rows without an episode end stay sentinels
    assert (out["ret"][d == 0] == FILL).all() and (out["disc"][d == 0] == FILL).all() and (out["length"][d == 0] == LEN_FILL).all()
    # the summary: the counts and lengths are exact, the sums show the NaN, min / max pass over it
    values, _ = M.summary_of(out["ret"], out["disc"], out["length"], d)
    for f, got in zip(M.SUMMARY, out["summary"]):
        if f in M.EXACT:
            assert got == values[f], (f, got, values[f])
    assert np.isnan(out["summary"][1]) and np.isnan(out["summary"][2]) and np.isnan(out["summary"][5])


# ---- 5. masked-out environments are not there
def test_mask_skips_environments_and_reset_touches_the_masked_carries():
    torch, dev = pr._torch()
    r, d = M.synthetic_tapes(300)
    mask = (np.random.default_rng(5).random(300) < 0.5).astype(np.uint8)
    mask[[M.NO_END, M.EVERY_STEP, 299]] = (1, 0, 0)
    on = mask != 0
    meter = _meter(300)
    dr, dd, dm = _dev(r), _dev(d), _dev(mask)
    meter.update(dr[:3], dd[:3])
    before = _state(meter)
    meter.summary(reset=True)
    ep = meter.update(dr[3:], dd[3:], want=("ret", "disc", "length"), trace=True, mask=dm)
    out = {k: getattr(ep, k).cpu().numpy() for k in KEYS}
    after = _state(meter)
    whole = _result(300)
    for key in KEYS:
        _same_bits(out[key][:, on], whole[key][3:][:, on], key + " of the environments in the mask")
    _same_bits(after["carry"][:, on], whole["carry"][:, on], "carry in the mask")
    # outside the mask: the carry stays, the rows keep what update() filled them with, nothing is counted
    _same_bits(after["carry"][:, ~on], before["carry"][:, ~on], "carry outside the mask")
    assert np.array_equal(after["carry_length"][~on], before["carry_length"][~on]) and (before["carry_length"][~on] > 0).any()
    assert np.isnan(out["ret"][:, ~on]).all() and np.isnan(out["disc"][:, ~on]).all() and np.isnan(out["trace"][:, ~on]).all() and (out["length"][:, ~on] == -1).all()
    _check_summary(after["summary"], out, d[3:], "masked", mask=mask)
    assert after["summary"][0] == (d[3:][:, on] != 0).sum() < (d[3:] != 0).sum()
    # a bool mask is its bytes; reset(mask) writes a fresh carry exactly there
    meter.reset(mask=torch.from_numpy(on).to(dev))
    reset = _state(meter)
    assert (reset["carry"][:, on] == np.array(M.FRESH, dtype=np.float32)[:, None]).all() and (reset["carry_length"][on] == 0).all()
    _same_bits(reset["carry"][:, ~on], after["carry"][:, ~on], "carry outside the reset's mask")
    assert np.array_equal(reset["carry_length"][~on], after["carry_length"][~on])
    _same_bits(reset["summary"], after["summary"], "the summary under a carry reset")
    meter.reset()
    assert (meter.carry.cpu().numpy() == np.array(M.FRESH, dtype=np.float32)[:, None]).all() and (meter.length.cpu().numpy() == 0).all()


# ---- 6. refused calls write nothing
def test_refused_calls_write_nothing():
    torch, dev = pr._torch()
    r, d = M.synthetic_tapes(37)
    meter = _meter(37)
    dr, dd = _dev(r), _dev(d)
    meter.update(dr[:3], dd[:3])
    before = _state(meter)
    outs = _sentinels(4, 37)
    lib = meter._lib
    for kw, word in ((dict(null=("reward",)), b"d_reward"), (dict(null=("done",)), b"d_done"), (dict(null=("carry",)), b"d_carry"),
                     (dict(null=("len",)), b"d_len"), (dict(null=("work",)), b"d_work"), (dict(n_steps=0), b"n_steps"), (dict(n_steps=-4), b"n_steps"),
                     (dict(n_envs=0), b"n_envs"), (dict(gamma=1.5), b"gamma"), (dict(gamma=-0.5), b"gamma"), (dict(gamma=float("nan")), b"gamma")):
        assert _raw(meter, dr[3:], dd[3:], outs, **kw) != 0
        assert b"lt_tape_episodes: " in lib.lt_last_error() and word in lib.lt_last_error(), lib.lt_last_error()
    assert lib.lt_episode_carry_reset(37, None, C.c_void_p(meter.length.data_ptr()), None, None, 1) != 0 and b"d_carry" in lib.lt_last_error()
    assert lib.lt_episode_carry_reset(0, C.c_void_p(meter.carry.data_ptr()), C.c_void_p(meter.length.data_ptr()), None, None, 1) != 0
    for kw, reason in ((dict(rew=dr[3:].cpu()), "reward must live on the device"), (dict(done=dd[3:].bool()), "done must be uint8"),
                       (dict(done=dd[2:]), "the done tape holds 5 steps"), (dict(rew=dr[3:, :36]), r"reward must be \[4, 37\]"),
                       (dict(mask=torch.ones(36, dtype=torch.uint8, device=dev)), r"mask must be \[37\]"), (dict(want=("ret", "steps")), "want names")):
        args = dict(rew=dr[3:], done=dd[3:])
        args.update(kw)
        with pytest.raises(ValueError, match="episodes: .*" + reason):
            meter.update(**args)
    meter.gamma = 2.0                                    # (tampered with after the constructor's check)
    with pytest.raises(ValueError, match="gamma must be in"):
        meter.update(dr[3:], dd[3:])
    with pytest.raises(ValueError, match=r"mask must be \[37\]"):
        meter.reset(mask=torch.ones(36, dtype=torch.uint8, device=dev))
    meter.gamma = GAMMA
    torch.cuda.synchronize(dev)
    for k, fill in (("ret", FILL), ("disc", FILL), ("trace", FILL), ("length", LEN_FILL)):
        assert (outs[k] == fill).all(), k
    after = _state(meter)
    for k in before:
        _same_bits(after[k], before[k], k + " after the refused calls")
    # ... and the meter goes on as if nothing had been tried
    ep = meter.update(dr[3:], dd[3:], want=("ret", "disc", "length"), trace=True)
    for key in KEYS:
        _same_bits(getattr(ep, key).cpu().numpy(), _result(37)[key][3:], key + " after the refused calls")
    _same_bits(meter.summary_raw(), _scan(r, d, splits=(3, 4))["summary"], "summary after the refused calls")


# ---- 7. no atomics: the same call twice gives the same bits
def test_two_identical_calls_give_a_bitwise_identical_summary():
    r, d = M.synthetic_tapes(300)
    a, b = _scan(r, d), _scan(r, d)
    _same_bits(a["summary"], _result(300)["summary"], "summary of a second run")
    _same_bits(a["summary"], b["summary"], "summary of a third run")
    a2, b2 = _scan(r, d, splits=(3, 4)), _scan(r, d, splits=(3, 4))
    _same_bits(a2["summary"], b2["summary"], "accumulated summary")
    assert a["summary"].view(np.uint64).tolist() == b["summary"].view(np.uint64).tolist()


# ---- 8. on real tapes, across two rollouts
def test_end_to_end_over_two_rollouts_with_device_restarts():
    """UnitreeA1.simple, n = 64, device restarts with horizon 3: two rollout_tape calls of 7 zero-action steps, meter.update after each,
    compared with the model over all 14 steps. An episode that ended by truncation alone and started inside the recording has length 3,
    and the meter counts the episodes the step kernel counted."""
    torch, dev = pr._torch()
    task, n = "UnitreeA1.simple", 64
    b = pr._batch(task, n, restarts=(pr._restart_table(task), 3))
    counted = b.stats()["episodes"]
    meter = _meter(n)
    acts = torch.zeros((T, n, b.nu), dtype=torch.float32, device=dev)
    tapes, eps = [], []
    for _ in range(2):
        rew = torch.full((T, n), FILL, dtype=torch.float32, device=dev)
        done = torch.full((T, n), tp.DONE_FILL, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        b.rollout_tape(acts, reward=rew, done=done)
        eps.append(meter.update(rew, done, want=("ret", "disc", "length"), trace=True))
        tapes.append((rew.cpu().numpy(), done.cpu().numpy()))
    counted = b.stats()["episodes"] - counted
    r, d = np.concatenate([t[0] for t in tapes]), np.concatenate([t[1] for t in tapes])
    assert not (d == tp.DONE_FILL).any() and np.isfinite(r).all()
    print("real tapes: done bytes", {int(k): int((d == k).sum()) for k in np.unique(d)})
    out = {key: torch.cat([getattr(e, key) for e in eps]).cpu().numpy() for key in KEYS}
    out.update(_state(meter))
    _check_values(out, r, d, GAMMA, "real tapes")
    _check_summary(out["summary"], out, d, "real tapes")
    seen = 0
    for e in range(n):
        ends = np.nonzero(d[:, e] != 0)[0]
        for prev, t in zip(ends[:-1], ends[1:]):
            if d[t, e] == 2:
                assert out["length"][t, e] == 3 == t - prev, (e, t)
                seen += 1
    assert seen >= n
    # an episode crossed the boundary between the two rollouts: counted once, in the second call, with its whole length
    assert ((out["length"][T:] > np.arange(1, T + 1)[:, None]) & (d[T:] != 0)).any()
    s = meter.summary()
    print("real tapes: meter %d episodes, step kernel %d, done != 0 in %d steps" % (s["episodes"], counted, (d != 0).sum()))
    assert s["episodes"] == (d != 0).sum() == counted
    assert s["L_max"] <= 3 and 0.0 <= s["absorbing_share"] <= 1.0
