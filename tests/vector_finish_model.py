"""
The contract of lv_finish_step (include/locovec.h) restated in numpy float32: the bookkeeping of one control step, vectorised over the
environments — and, beside it, a naive loop over single environments that the host tests compare it with. Every operation is a float32
operation rounded once, so the device's results are compared BITWISE.
"""

import numpy as np

NOBS_CASES = (1, 37)
N_CASES = (1, 255, 257)                     # one short of and one past a workgroup of 256 lanes
SENTINEL = -7.0                             # what final_obs holds before the call: rows that did not end keep it


def finish(obs, reward, done, term=None, final_obs=None, run_return=None, run_length=None, want_ep=True):
    """One call. ``obs`` / ``term`` / ``final_obs`` float32 [n, nobs], ``reward`` / ``run_return`` float32 [n], ``done`` uint8 [n],
    ``run_length`` int32 [n]. Returns a dict of NEW arrays: terminated, truncated (uint8), final_obs (or None), run_return, run_length,
    ep_return, ep_length (None without accumulators / with ``want_ep`` False). The inputs are not changed."""
    obs, reward, done = np.asarray(obs, np.float32), np.asarray(reward, np.float32), np.asarray(done, np.uint8)
    ended = done != 0
    out = dict(terminated=(done & 1).astype(np.uint8), truncated=(((done & 2) != 0) & ((done & 1) == 0)).astype(np.uint8),
               final_obs=None, run_return=None, run_length=None, ep_return=None, ep_length=None)
    if run_return is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            ret = (np.asarray(run_return, np.float32) + reward).astype(np.float32)
        length = (np.asarray(run_length, np.int32) + np.int32(1)).astype(np.int32)
        if want_ep:
            out["ep_return"] = np.where(ended, ret, np.float32(0)).astype(np.float32)
            out["ep_length"] = np.where(ended, length, np.int32(0)).astype(np.int32)
        ret, length = ret.copy(), length.copy()
        ret[ended] = 0.0                     # by assignment: a NaN ends with its episode
        length[ended] = 0
        out["run_return"], out["run_length"] = ret, length
    if final_obs is not None:
        fin = np.array(final_obs, dtype=np.float32)
        from_term = ((done & 2) != 0) if term is not None else np.zeros(len(done), dtype=bool)
        fin[ended & ~from_term] = obs[ended & ~from_term]
        if term is not None:
            fin[from_term] = np.asarray(term, np.float32)[from_term]
        out["final_obs"] = fin
    return out


def naive_finish(obs, reward, done, term=None, final_obs=None, run_return=None, run_length=None):
    """The same, one environment after the other, in the words of the header."""
    n = len(done)
    out = dict(terminated=np.zeros(n, np.uint8), truncated=np.zeros(n, np.uint8),
               final_obs=None if final_obs is None else np.array(final_obs, dtype=np.float32),
               run_return=None if run_return is None else np.array(run_return, dtype=np.float32),
               run_length=None if run_length is None else np.array(run_length, dtype=np.int32),
               ep_return=None if run_return is None else np.zeros(n, np.float32),
               ep_length=None if run_return is None else np.zeros(n, np.int32))
    for e in range(n):
        d = int(done[e])
        out["terminated"][e] = d & 1
        out["truncated"][e] = 1 if (d & 2) and not (d & 1) else 0
        if run_return is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                out["run_return"][e] = np.float32(out["run_return"][e]) + np.float32(reward[e])
            out["run_length"][e] += 1
            if d != 0:
                out["ep_return"][e], out["ep_length"][e] = out["run_return"][e], out["run_length"][e]
                out["run_return"][e], out["run_length"][e] = 0.0, 0
        if final_obs is not None and d != 0:
            out["final_obs"][e] = term[e] if (d & 2) and term is not None else obs[e]
    return out


def synthetic_step(n, nobs, seed=0, nan_at=None):
    """Inputs of one call: done bytes that cover 0, 1, 2 and 3 (cyclically from a seeded offset, so that every n >= 1 has an ended
    environment in some call of three), rewards of mixed sign and magnitude, observation and terminal rows that differ everywhere."""
    rs = np.random.RandomState(1000 + seed)
    done = ((np.arange(n) + seed) % 5).astype(np.uint8)
    done[done == 4] = 0
    obs = rs.standard_normal((n, nobs)).astype(np.float32)
    term = (rs.standard_normal((n, nobs)) + 10.0).astype(np.float32)
    reward = (rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, n)).astype(np.float32)
    if nan_at is not None:
        reward[nan_at] = np.nan
    return obs, reward, done, term


def column_map(x, perm):
    """The reference's column order from the kernel's: column j of the result is column perm[j] of x (LocoEnv.step's `obs[:, perm]`)."""
    return x if perm is None else np.stack([x[:, int(p)] for p in perm], axis=1)
