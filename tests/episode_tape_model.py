"""
Host model of lt_tape_episodes (include/locotape.h; not a test file): a float64 numpy loop of the header's per-environment formulas
that returns every value together with a bound on what float32 may make of it, and the summary recomputed from RETURNED float32 values.

The bound is built like the one of tests/test_tape_gae_gpu.py's _gae64: every float32 rounding contributes at most u = 2^-24 times the
magnitude it rounds, and the errors inherited through the recurrences are carried along — per step and environment

    ret' = fl(ret + r)               e_ret'  = e_ret + u (|ret'| + e_ret)
    disc' = fl(w r + disc)  (fmaf)   e_disc' = |r| e_w + e_disc + u (|disc'| + |r| e_w + e_disc)
    w' = fl(w gamma)                 e_w'    = gamma e_w + u (gamma (|w| + e_w))
    g' = fl(gamma g + r)    (fmaf)   e_g'    = gamma e_g + u (|g'| + gamma e_g)

(the magnitude a rounding sees is at most the model's value plus the error inherited so far; primes are the model's float64 values).
The model's own float64 arithmetic rounds too, at most twice per line (a product and a sum) by 2^-53 of the same magnitudes: u below is
2^-24 + 2 * 2^-53, so that the bound also holds against the model as computed. No other constant. Lengths and counts are exact.
"""

import numpy as np

U = 2.0 ** -24 + 2 * 2.0 ** -53
FRESH = (0.0, 0.0, 1.0, 0.0)                  # ret, disc, w, g of a fresh carry; len 0
SUMMARY = ("episodes", "R_sum", "RR_sum", "R_min", "R_max", "J_sum", "L_sum", "L_min", "L_max", "absorbing")
EXACT = ("episodes", "R_min", "R_max", "L_sum", "L_min", "L_max", "absorbing")     # (L_sum: integers below 2^53)


T = 7
NO_END, EVERY_STEP = 12, 13                   # columns of synthetic_tapes: no episode end at all / one in every step


def synthetic_tapes(n, seed=2025):
    """(reward float32 [T, n], done uint8 [T, n]) from a seeded generator, read-only: done bytes drawn from {0, 1, 2, 3}, each of them at
    t = 0, in the middle and at t = T - 1 (columns 0..11), column NO_END without an end, column EVERY_STEP ending in every step."""
    assert n > EVERY_STEP
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((T, n)).astype(np.float32)
    d = rng.choice(np.array([0, 0, 0, 0, 0, 1, 2, 3], dtype=np.uint8), (T, n))
    for i, t in enumerate((0, T // 2, T - 1)):
        d[t, 4 * i:4 * i + 4] = (0, 1, 2, 3)
    d[:, NO_END] = 0
    d[:, EVERY_STEP] = 1 + np.arange(T) % 3
    r.setflags(write=False)
    d.setflags(write=False)
    return r, d


def episodes64(reward, done, gamma, carry=None, length=None, mask=None):
    """``reward`` float32 [T, n], ``done`` uint8 [T, n], ``gamma`` (rounded to float32 as the library receives it); ``carry`` float32
    [4, n] / ``length`` int [n]: what the scan starts from (exact values; None: fresh); ``mask`` [n]: environments with 0 are skipped.
    Returns a dict: ``ret`` / ``disc`` float64 [T, n] (NaN where no episode ended) with bounds ``b_ret`` / ``b_disc``, ``length`` int64
    [T, n] (-1 there), ``trace`` float64 [T, n] with ``b_trace`` (NaN for skipped environments), the final ``carry`` float64 [4, n]
    with ``b_carry`` and ``carry_length`` int64 [n]."""
    g32 = float(np.float32(gamma))
    T, n = reward.shape
    r64 = reward.astype(np.float64)
    out = dict(ret=np.full((T, n), np.nan), disc=np.full((T, n), np.nan), b_ret=np.zeros((T, n)), b_disc=np.zeros((T, n)),
               length=np.full((T, n), -1, dtype=np.int64), trace=np.full((T, n), np.nan), b_trace=np.zeros((T, n)),
               carry=np.zeros((4, n)), b_carry=np.zeros((4, n)), carry_length=np.zeros(n, dtype=np.int64))
    for e in range(n):
        ret, disc, w, g = FRESH if carry is None else (float(carry[k, e]) for k in range(4))
        ln = 0 if length is None else int(length[e])
        e_ret = e_disc = e_w = e_g = 0.0
        if mask is None or mask[e]:
            for t in range(T):
                r = r64[t, e]
                ret = ret + r
                e_ret = e_ret + U * (abs(ret) + e_ret)
                disc = w * r + disc
                inherited = abs(r) * e_w + e_disc
                e_disc = inherited + U * (abs(disc) + inherited)
                e_w = g32 * e_w + U * (g32 * (abs(w) + e_w))
                w = w * g32
                g = g32 * g + r
                e_g = g32 * e_g + U * (abs(g) + g32 * e_g)
                ln += 1
                out["trace"][t, e], out["b_trace"][t, e] = g, e_g
                if done[t, e] != 0:
                    out["ret"][t, e], out["b_ret"][t, e] = ret, e_ret
                    out["disc"][t, e], out["b_disc"][t, e] = disc, e_disc
                    out["length"][t, e] = ln
                    ret, disc, w, g = FRESH
                    ln = 0
                    e_ret = e_disc = e_w = e_g = 0.0
        out["carry"][:, e], out["b_carry"][:, e], out["carry_length"][e] = (ret, disc, w, g), (e_ret, e_disc, e_w, e_g), ln
    return out


def naive_episodes(reward, done, gamma):
    """The same values the plain way, from a fresh carry: every column split at ``done != 0`` with np.split, the complete pieces summed
    in float64 (the trailing piece is the unfinished episode: not counted). Returns (ret, disc, length, trace) shaped as above."""
    g32 = float(np.float32(gamma))
    T, n = reward.shape
    ret, disc = np.full((T, n), np.nan), np.full((T, n), np.nan)
    length, trace = np.full((T, n), -1, dtype=np.int64), np.zeros((T, n))
    for e in range(n):
        ends = np.nonzero(done[:, e] != 0)[0]
        pieces = np.split(reward[:, e].astype(np.float64), ends + 1)
        start = 0
        for i, piece in enumerate(pieces):
            k = np.arange(len(piece))
            for j in range(len(piece)):                    # g at step start + j: the rewards so far, the latest undiscounted
                trace[start + j, e] = np.sum(piece[:j + 1] * g32 ** (j - k[:j + 1]))
            if i < len(ends):
                ret[ends[i], e], disc[ends[i], e], length[ends[i], e] = piece.sum(), np.sum(piece * g32 ** k), len(piece)
            start += len(piece)
    return ret, disc, length, trace


def summary_of(ep_ret, ep_disc, ep_length, done, mask=None):
    """The summary from the float32 episode tapes a call RETURNED (rows with ``done != 0`` of unmasked environments), as float64 numpy
    sums: ``(values, bounds)``, dicts over SUMMARY. Sums of k terms in any order differ from the exact sum by at most (k - 1) 2^-53 of
    the sum of magnitudes, the library's and numpy's alike: the bound is k 2^-53 sum |x| for the sums of R, R*R (float32 squares are
    exact in float64) and J, and 0 for counts, lengths, min and max. NaN returns are passed over by min / max, as by the library."""
    ended = done != 0
    if mask is not None:
        ended = ended & (np.asarray(mask) != 0)[None, :]
    R, J, L = ep_ret[ended].astype(np.float64), ep_disc[ended].astype(np.float64), ep_length[ended].astype(np.float64)
    k = int(ended.sum())
    fin = R[~np.isnan(R)]
    values = dict(episodes=float(k), R_sum=R.sum(), RR_sum=(R * R).sum(), R_min=fin.min() if len(fin) else np.inf,
                  R_max=fin.max() if len(fin) else -np.inf, J_sum=J.sum(), L_sum=L.sum(), L_min=L.min() if k else np.inf,
                  L_max=L.max() if k else -np.inf, absorbing=float(((done & 1) != 0)[ended].sum()))
    bounds = dict.fromkeys(SUMMARY, 0.0)
    bounds.update(R_sum=k * 2.0 ** -53 * np.abs(R).sum(), RR_sum=k * 2.0 ** -53 * (R * R).sum(), J_sum=k * 2.0 ** -53 * np.abs(J).sum())
    return values, bounds
