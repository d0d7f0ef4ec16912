"""
Advantage estimation over the tapes (include/locohip.h lm_tape_gae, HipBatch.gae; `-m gpu`): one launch, the done byte's bits told apart.
T = 7, n = 37 (two wave-sized groups of lanes, the second partial). The reference is a float64 numpy loop of the header's formula,
written here, that carries a running rounding bound per step, as tests/test_policy_rollout_gpu.py's _mlp64 does per layer.
"""

import functools

import numpy as np
import pytest

import test_policy_rollout_gpu as pr
import test_rollout_tape_gpu as tp
from test_rollout_tape_gpu import OBS_FILL, T

pytestmark = pytest.mark.gpu

N = 37
U = 2.0 ** -24
GAMMA, LAM = 0.99, 0.95
FILL = -7.0


def _gae64(r, d, v, last_v, term_v, gamma, lam):
    """(adv, ret, bound on |adv32 - adv|, bound on |ret32 - ret|) in float64 from float32 tapes; gamma / lam are the float32 values the
    library receives. The kernel rounds four times per step — fmaf(gamma, next_v, r); - v; the product gamma * lam (relative, so
    u * gamma * lam * |adv[t+1]| in the result); fmaf(gamma * lam, adv[t+1], delta) — each by at most u = 2^-24 times a magnitude that
    s = gamma |next_v| + |r| + |v| + gamma lam |adv[t+1]| covers; with 5 in place of 4 the second-order terms (u^2, and the inherited
    error inside |adv[t+1]|, which is added to it below) have room. The inherited error itself passes with the factor gamma * lam.
    ret = adv + v: one more rounding of at most u (|adv| + |v|)."""
    g, l = float(np.float32(gamma)), float(np.float32(lam))
    r, v, last_v = r.astype(np.float64), v.astype(np.float64), last_v.astype(np.float64)
    term_v = np.zeros_like(r) if term_v is None else term_v.astype(np.float64)
    steps, n = r.shape
    adv, err = np.zeros((steps, n)), np.zeros((steps, n))
    for e in range(n):
        adv_next = err_next = 0.0
        for t in range(steps - 1, -1, -1):
            last = t == steps - 1
            if d[t, e] & 1:
                next_v = 0.0
            elif d[t, e] & 2:
                next_v = term_v[t, e]
            else:
                next_v = last_v[e] if last else v[t + 1, e]
            cut = d[t, e] != 0 or last
            delta = r[t, e] + g * next_v - v[t, e]
            trace = 0.0 if cut else g * l * adv_next
            inherited = 0.0 if cut else g * l * err_next
            adv[t, e] = delta + trace
            s = abs(g * next_v) + abs(r[t, e]) + abs(v[t, e]) + (0.0 if cut else g * l * (abs(adv_next) + err_next))
            err[t, e] = 5 * U * s + inherited
            adv_next, err_next = adv[t, e], err[t, e]
    ret = adv + v
    return adv, ret, err, err + U * (np.abs(adv) + err + np.abs(v))


def _within(got_adv, got_ret, ref, label):
    adv, ret, b_adv, b_ret = ref
    e_adv, e_ret = np.abs(got_adv.astype(np.float64) - adv), np.abs(got_ret.astype(np.float64) - ret)
    assert np.isfinite(got_adv).all() and np.isfinite(got_ret).all()
    tiny = np.finfo(np.float64).tiny
    print("%s: worst |adv error| / bound %.3f, worst |ret error| / bound %.3f, largest |adv| %.3f"
          % (label, (e_adv / np.maximum(b_adv, tiny)).max(), (e_ret / np.maximum(b_ret, tiny)).max(), np.abs(adv).max()))
    assert (e_adv <= b_adv).all(), (label, np.argwhere(e_adv > b_adv)[:4].tolist())
    assert (e_ret <= b_ret).all(), (label, np.argwhere(e_ret > b_ret)[:4].tolist())


@functools.lru_cache(maxsize=None)
def _tapes():
    """Synthetic tapes from a seeded generator (read-only): every done byte of {0, 1, 2, 3} at t = 0, in the middle and at t = T - 1."""
    rng = np.random.default_rng(2024)
    r = rng.standard_normal((T, N)).astype(np.float32)
    v = (rng.standard_normal((T, N)) * 3).astype(np.float32)
    last_v = (rng.standard_normal(N) * 3).astype(np.float32)
    term_v = (rng.standard_normal((T, N)) * 3).astype(np.float32)
    d = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 3], dtype=np.uint8), (T, N))
    for i, t in enumerate((0, T // 2, T - 1)):
        d[t, 4 * i:4 * i + 4] = (0, 1, 2, 3)
    d[:, 12] = 0                                          # one trace that runs through all T steps
    for t in (0, T // 2, T - 1):
        assert set(d[t]) == {0, 1, 2, 3}
    out = dict(reward=r, done=d, value=v, last_value=last_v, term_value=term_v)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _a_batch(n=N):
    return tp._batch("UnitreeA1.simple", n)


def _gae(tapes, b=None, gamma=GAMMA, lam=LAM, **kw):
    torch, dev = pr._torch()
    b = _a_batch() if b is None else b
    dev_t = {k: (None if a is None else torch.from_numpy(np.array(a)).to(dev)) for k, a in tapes.items()}
    steps = tapes["reward"].shape[0]
    adv = torch.full((steps, b.n), FILL, dtype=torch.float32, device=dev)
    ret = torch.full((steps, b.n), FILL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    got = b.gae(dev_t["reward"], dev_t["done"], dev_t["value"], dev_t["last_value"], dev_t.get("term_value"), gamma=gamma, lam=lam,
                adv=adv, ret=ret, **kw)
    assert got[0] is adv and got[1] is ret
    return adv.cpu().numpy(), ret.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _result():
    return _gae(_tapes())


# ---- 1. against the float64 loop
@pytest.mark.parametrize("gamma,lam", [(GAMMA, LAM), (1.0, 1.0), (0.9, 0.0)])
def test_against_the_float64_loop(gamma, lam):
    t = _tapes()
    adv, ret = _result() if (gamma, lam) == (GAMMA, LAM) else _gae(t, gamma=gamma, lam=lam)
    assert not (adv == FILL).any() and not (ret == FILL).any()
    _within(adv, ret, _gae64(t["reward"], t["done"], t["value"], t["last_value"], t["term_value"], gamma, lam), "gamma %g, lam %g" % (gamma, lam))


def test_outputs_are_optional_and_allocated_when_not_given():
    torch, dev = pr._torch()
    t = {k: torch.from_numpy(np.array(a)).to(dev) for k, a in _tapes().items()}
    adv, ret = _a_batch().gae(t["reward"], t["done"], t["value"], t["last_value"], t["term_value"], gamma=GAMMA, lam=LAM)
    assert np.array_equal(adv.cpu().numpy(), _result()[0]) and np.array_equal(ret.cpu().numpy(), _result()[1])
    # the C-ABI: either output may be NULL
    import ctypes as C
    b = _a_batch()
    for which in (0, 1):
        outs = [torch.full((T, N), FILL, dtype=torch.float32, device=dev) for _ in range(2)]
        torch.cuda.synchronize(dev)
        ptrs = [C.c_void_p(o.data_ptr()) for o in outs]
        ptrs[1 - which] = None
        rc = b._lib.lm_tape_gae(b._h, T, C.c_void_p(t["reward"].data_ptr()), C.c_void_p(t["done"].data_ptr()), C.c_void_p(t["value"].data_ptr()),
                                C.c_void_p(t["last_value"].data_ptr()), C.c_void_p(t["term_value"].data_ptr()), GAMMA, LAM, ptrs[0], ptrs[1], None, 1)
        assert rc == 0, b._lib.lm_last_error()
        assert np.array_equal(outs[which].cpu().numpy(), _result()[which]) and (outs[1 - which] == FILL).all()


# ---- 2. no terminal values = zeros
def test_no_terminal_values_is_bitwise_zeros_there():
    t = dict(_tapes())
    zeros = _gae(dict(t, term_value=np.zeros((T, N), dtype=np.float32)))
    none = _gae(dict(t, term_value=None))
    assert np.array_equal(zeros[0], none[0]) and np.array_equal(zeros[1], none[1])
    assert not np.array_equal(none[0], _result()[0])


# ---- 3. gamma = lam = 0: r - v
def test_gamma_and_lam_zero_reduce_to_r_minus_v():
    t = _tapes()
    adv, ret = _gae(t, gamma=0.0, lam=0.0)
    assert np.array_equal(adv, t["reward"] - t["value"])
    assert np.array_equal(ret, (t["reward"] - t["value"]) + t["value"])


# ---- 4. what must not be read is not read
def test_poisoned_unreachable_values_stay_out():
    """NaN in term_value wherever done != 2 and in last_value wherever the last step ended an episode: the result is finite and bitwise
    the unpoisoned one. value[t + 1] cannot be poisoned in place — it is step t + 1's own v whatever step t's done byte says — so the
    cut is shown on the tapes cut short: for the environments whose step k - 1 ended an episode, rows 0 .. k - 1 computed from the
    first k rows alone, with NaN as last_value, are finite and bitwise the full run's."""
    t = dict(_tapes())
    term = np.where(t["done"] == 2, t["term_value"], np.float32(np.nan)).astype(np.float32)
    last = np.where(t["done"][T - 1] == 0, t["last_value"], np.float32(np.nan)).astype(np.float32)
    assert np.isnan(term).any() and np.isnan(last).any()
    adv, ret = _gae(dict(t, term_value=term, last_value=last))
    assert np.isfinite(adv).all() and np.isfinite(ret).all()
    assert np.array_equal(adv, _result()[0]) and np.array_equal(ret, _result()[1])
    seen = 0
    for k in range(1, T):
        cut = t["done"][k - 1] != 0
        short = {key: np.ascontiguousarray(t[key][:k]) for key in ("reward", "done", "value")}
        short.update(term_value=np.ascontiguousarray(term[:k]), last_value=np.full(N, np.nan, dtype=np.float32))
        a_k, r_k = _gae(short)
        assert np.isfinite(a_k[:, cut]).all() and np.isnan(a_k[k - 1, ~cut]).all()
        assert np.array_equal(a_k[:, cut], adv[:k, cut]) and np.array_equal(r_k[:, cut], ret[:k, cut])
        seen += cut.sum()
    assert seen >= 6


# ---- 5. a row does not depend on n or on its place
def test_a_row_is_independent_of_the_batch():
    t = _tapes()
    e = 3
    one = {k: np.ascontiguousarray(a[..., e:e + 1]) for k, a in t.items()}
    adv, ret = _gae(one, b=_a_batch(1))
    assert adv.shape == (T, 1)
    assert np.array_equal(adv[:, 0], _result()[0][:, e]) and np.array_equal(ret[:, 0], _result()[1][:, e])


# ---- 6. on real tapes, queued behind the rollout on a side stream
def test_real_tapes_on_a_side_stream_without_host_waits():
    torch, dev = pr._torch()
    task, n, widths, act = pr.CASES["a1"]
    assert n == N
    table = pr._restart_table(task)
    b, obs0 = pr._start(lambda: pr._batch(task, n, restarts=(table, 3), terminal=True))
    policy = pr._policy(b, widths, act, -1.0)
    torch.manual_seed(7)
    critic = torch.nn.Sequential(torch.nn.Linear(b.nobs, 32), torch.nn.Tanh(), torch.nn.Linear(32, 1)).to(dev)
    obs = torch.full((T, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev)
    term = torch.full((T, n, b.nobs), OBS_FILL, dtype=torch.float32, device=dev)
    reward = torch.full((T, n), FILL, dtype=torch.float32, device=dev)
    done = torch.full((T, n), tp.DONE_FILL, dtype=torch.uint8, device=dev)
    adv = torch.full((T, n), FILL, dtype=torch.float32, device=dev)
    ret = torch.full((T, n), FILL, dtype=torch.float32, device=dev)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(side), torch.no_grad():
        s = side.cuda_stream
        b.rollout_policy(policy, T, obs0=obs0, obs=obs, reward=reward, done=done, terminal=term, steps_per_launch=3, noise_seed=3, stream=s, sync=False)
        prev = torch.cat([obs0[None], obs[:-1]])
        values = critic(torch.cat([prev, obs[-1:], term])).squeeze(-1).contiguous()          # one batched pass: [2 T + 1, n]
        value, last_value, term_value = values[:T], values[T], values[T + 1:]
        b.gae(reward, done, value, last_value, term_value, gamma=GAMMA, lam=LAM, adv=adv, ret=ret, stream=s, sync=False)
    side.synchronize()
    d = done.cpu().numpy()
    assert (d == 2).any() and (d == 0).any() and not (d == tp.DONE_FILL).any()
    print("real tapes: done bytes", {int(k): int((d == k).sum()) for k in np.unique(d)})
    ref = _gae64(reward.cpu().numpy(), d, value.cpu().numpy(), last_value.cpu().numpy(), term_value.cpu().numpy(), GAMMA, LAM)
    _within(adv.cpu().numpy(), ret.cpu().numpy(), ref, "real tapes")
    # the bootstrap at a truncation did come from the terminal rows: zeros there give another result
    z = _gae(dict(reward=reward.cpu().numpy(), done=d, value=value.cpu().numpy(), last_value=last_value.cpu().numpy(), term_value=None), b=b)
    assert not np.array_equal(z[0], adv.cpu().numpy())


# ---- 7. refused calls write nothing
def test_refused_calls_write_nothing():
    import ctypes as C
    torch, dev = pr._torch()
    b = _a_batch()
    t = {k: torch.from_numpy(np.array(a)).to(dev) for k, a in _tapes().items()}
    adv = torch.full((T, N), FILL, dtype=torch.float32, device=dev)
    ret = torch.full((T, N), FILL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    p = {k: C.c_void_p(x.data_ptr()) for k, x in t.items()}
    pa, pr_ = C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr())

    def raw(steps=T, gamma=GAMMA, lam=LAM, adv_p=pa, ret_p=pr_, **null):
        q = {k: (None if k in null else x) for k, x in p.items()}
        return b._lib.lm_tape_gae(b._h, steps, q["reward"], q["done"], q["value"], q["last_value"], q["term_value"], gamma, lam, adv_p, ret_p, None, 1)
    for call, word in ((lambda: raw(reward=1), b"d_reward"), (lambda: raw(done=1), b"d_done"), (lambda: raw(value=1), b"d_value"),
                       (lambda: raw(last_value=1), b"d_last_value"), (lambda: raw(adv_p=None, ret_p=None), b"both null"),
                       (lambda: raw(steps=0), b"n_steps"), (lambda: raw(steps=-3), b"n_steps"),
                       (lambda: raw(gamma=1.5), b"gamma"), (lambda: raw(gamma=-0.1), b"gamma"), (lambda: raw(gamma=float("nan")), b"gamma"),
                       (lambda: raw(lam=1.5), b"lam"), (lambda: raw(lam=float("nan")), b"lam"), (lambda: raw(lam=float("inf")), b"lam")):
        assert call() != 0
        assert word in b._lib.lm_last_error(), b._lib.lm_last_error()
    for kw, reason in ((dict(gamma=2.0), "gamma"), (dict(lam=float("nan")), "lam"), (dict(reward=t["reward"].cpu()), "reward must live on the device"),
                       (dict(last_value=t["value"]), "last_value must be"), (dict(done=t["done"].bool()), "done must be uint8")):
        args = dict(reward=t["reward"], done=t["done"], value=t["value"], last_value=t["last_value"], adv=adv, ret=ret)
        args.update(kw)
        with pytest.raises(ValueError, match=reason):
            b.gae(**args)
    torch.cuda.synchronize(dev)
    assert (adv == FILL).all() and (ret == FILL).all()
