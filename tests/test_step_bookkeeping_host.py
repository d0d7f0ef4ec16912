"""
The host model of the step kernel's bookkeeping (tests/step_bookkeeping_model.py) on its own: the mixer against SplitMix64's published
outputs and against a restatement in Python ints, and the statistical properties the draw rules of include/locohip.h promise, over
2^18 (global environment id, episode) pairs under one fixed seed — nothing here can flake. No GPU: tests/test_step_bookkeeping_gpu.py
holds the kernels to this model.
"""

import math

import numpy as np
from scipy import stats

import step_bookkeeping_model as M

SEED = 0x5EED0123456789AB
OFFSET = 1000
G, E = 512, 512                       # 2^18 (gid, episode) pairs
GID = (OFFSET + np.arange(G))[:, None]
EP = (1 + np.arange(E))[None, :]


def _mix64_ints(x):
    x = (x + 0x9E3779B97F4A7C15) & M.MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M.MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M.MASK64
    return x ^ (x >> 31)


def _corr(a, b):
    return float(np.corrcoef(np.ravel(a).astype(np.float64), np.ravel(b).astype(np.float64))[0, 1])


def test_mixer_is_splitmix64():
    g = M.GOLDEN
    assert M.mix64(0) == 0xE220A8397B1DCDAF and M.mix64(g) == 0x6E789E6AA1B965F4 and M.mix64(2 * g) == 0x06C45D188009454F
    rs = np.random.RandomState(0)
    xs = [int(a) << 32 | int(b) for a, b in rs.randint(0, 2 ** 32, (256, 2), dtype=np.int64)] + [0, 1, M.MASK64, M.MASK64 - g + 1]
    got = M.mix64(np.array(xs, dtype=np.uint64))
    assert [int(v) for v in got] == [_mix64_ints(x) for x in xs]
    assert all(M.mix64(x) == _mix64_ints(x) for x in xs[:8])


def test_draw_rules_in_python_ints():
    """Every draw rule once more with wrapping Python ints, scalar by scalar, at ids past 2^31 and 2^32, a negative offset's id and a
    64-bit seed: the array code and this restatement agree."""
    for seed, gid, ec in [(SEED, 1003, 1), (0, 0, 1), (9, 2 ** 31 + 5, 7), (M.MASK64, 2 ** 32 + 1, 2 ** 31), (5, -3, 4)]:
        key = (seed ^ _mix64_ints(((gid & M.MASK64) * 2 + 1) & M.MASK64) ^ ((ec & 0xFFFFFFFF) << 32)) & M.MASK64
        assert M.restart_row(seed, gid, ec, 257) == _mix64_ints(key) % 257
        assert M.variant_draw(seed, gid, ec, 3) == _mix64_ints(key ^ M.K_VARIANT) % 3
        for dof, p in [(0, 0), (5, 2), (17, 1)]:
            assert M.dof_redraw_bits(seed, gid, ec, dof, p) == _mix64_ints(key ^ ((dof * 3 + p + 1) * M.K_STREAM & M.MASK64))
        for step, k in [(0, 0), (3, 11), (2 ** 32 - 1, 91)]:
            r = _mix64_ints(seed ^ _mix64_ints(((gid & M.MASK64) * M.K_GID_STEP + step) & M.MASK64) ^ ((k + 1) * M.K_STREAM & M.MASK64))
            assert M.random_action_bits(seed, gid, step, k) == r >> 40
            assert float(M.random_action(seed, gid, step, k)) == (r >> 40) * 2.0 ** -23 - 1.0
    assert M.variant_of_row(255, 128) == 1 and M.variant_of_row(256, 128) == 2 and M.variant_of_row(0, 128) == 0
    assert M.rollout_seed(5, 0) == 5 and M.rollout_seed(0, 1) == M.GOLDEN
    assert M.rollout_seed(5, 9) == 5 ^ ((9 * M.GOLDEN) % 2 ** 64)
    # an id is not truncated to 32 bits, and the episode counter is not off by one
    assert not np.array_equal(M.restart_row(SEED, 2 ** 32 + np.arange(64), 1, 2 ** 20), M.restart_row(SEED, np.arange(64), 1, 2 ** 20))
    assert not np.array_equal(M.restart_row(SEED, np.arange(64), 1, 2 ** 20), M.restart_row(SEED, np.arange(64), 2, 2 ** 20))


def test_restart_rows_are_uniform_and_uncorrelated():
    for n_rows in (3, 257, 300):
        rows = M.restart_row(SEED, GID, EP, n_rows)
        assert rows.shape == (G, E) and rows.min() == 0 and rows.max() == n_rows - 1
        chi2, p = stats.chisquare(np.bincount(rows.ravel().astype(np.int64), minlength=n_rows))
        print("n_rows %d: chi-square %.1f, p = %.3g" % (n_rows, chi2, p))
        assert p > 1e-4
        r_gid, r_ep = _corr(rows[:-1], rows[1:]), _corr(rows[:, :-1], rows[:, 1:])
        print("n_rows %d: correlation of neighbouring ids %.4f, of successive episodes %.4f" % (n_rows, r_gid, r_ep))
        assert abs(r_gid) < 0.01 and abs(r_ep) < 0.01


def test_row_and_variant_of_one_restart_are_uncorrelated():
    rows = M.restart_row(SEED, GID, EP, 257)
    for nvar in (3, 4):
        var = M.variant_draw(SEED, GID, EP, nvar)
        assert var.min() == 0 and var.max() == nvar - 1
        assert stats.chisquare(np.bincount(var.ravel().astype(np.int64), minlength=nvar))[1] > 1e-4
        r = _corr(rows, var)
        print("%d variants: correlation with the row %.4f" % (nvar, r))
        assert abs(r) < 0.01


def test_random_action_is_uniform_on_minus_one_to_one():
    a = M.random_action(SEED, GID, np.arange(E)[None, :], 0)
    assert a.dtype == np.float32 and a.shape == (G, E)
    a64 = a.astype(np.float64)
    print("random_action: mean %.5f variance %.5f" % (a64.mean(), a64.var()))
    assert abs(a64.mean()) < 0.01 and abs(a64.var() - 1.0 / 3.0) < 0.01
    # neighbouring ids, successive steps and neighbouring action entries are uncorrelated
    b = M.random_action(SEED, GID, np.arange(E)[None, :], 1)
    assert abs(_corr(a[:-1], a[1:])) < 0.01 and abs(_corr(a[:, :-1], a[:, 1:])) < 0.01 and abs(_corr(a, b)) < 0.01


def test_random_action_range_and_float32_exactness():
    """All 2^24 values of r >> 40: the kernel's float32 expression (float)(r >> 40) * (2.0f / 16777216.0f) - 1.0f is exact, never
    reaches +1 and gives -1 for 0 alone."""
    top = np.arange(2 ** 24, dtype=np.uint64)
    exact = top.astype(np.float64) * 2.0 ** -23 - 1.0
    f32 = top.astype(np.float32) * np.float32(2.0 / 16777216.0) - np.float32(1.0)
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), exact)
    assert exact.max() < 1.0 and exact[0] == -1.0 and (exact[1:] > -1.0).all()
    # ... and random_action is that map of its bits
    bits = np.asarray(M.random_action_bits(SEED, GID[:64], np.arange(64)[None, :], 3))
    assert np.array_equal(M.random_action(SEED, GID[:64], np.arange(64)[None, :], 3), f32[bits.astype(np.int64)])
    assert int(bits.max()) < 2 ** 24


def test_normal_kinds_have_the_specs_moments_and_clip_at_zero():
    a, b = 0.1, 1.0
    share = 0.5 * math.erfc(0.1 / math.sqrt(2.0))              # Phi(-0.1)
    for kind in (M.KIND_NORMAL_CLIPPED, M.KIND_NORMAL):
        raw = M.dof_redraw(SEED, GID, EP, 4, 1, kind, a, b, clip=False)
        v = M.dof_redraw(SEED, GID, EP, 4, 1, kind, a, b)
        print("kind %d: mean %.5f std %.5f before the clip, %.5f clipped to 0 (Phi(-0.1) = %.5f)" % (kind, raw.mean(), raw.std(), (v == 0).mean(), share))
        assert abs(raw.mean() - float(np.float32(a))) < 0.01 and abs(raw.std() - b) < 0.01
        assert np.isfinite(raw).all() and v.min() == 0.0 and np.array_equal(v, np.maximum(raw, 0.0))
        assert abs((v == 0).mean() - share) < 0.01
    # both normal kinds draw the same numbers (kind 3 is clipped like kind 1); the uniform kind stays inside [a, b]
    assert np.array_equal(M.dof_redraw(SEED, GID, EP, 4, 1, 1, a, b), M.dof_redraw(SEED, GID, EP, 4, 1, 3, a, b))
    u = M.dof_redraw(SEED, GID, EP, 4, 1, M.KIND_UNIFORM, 0.25, 0.75)
    assert u.min() > 0.25 and u.max() <= 0.75 and abs(u.mean() - 0.5) < 0.01 and abs(u.std() - 0.5 / math.sqrt(12.0)) < 0.01
    # keyed per dof and per parameter: neighbouring keys are uncorrelated draws
    base = M.dof_redraw(SEED, GID, EP, 4, 1, M.KIND_UNIFORM, 0.0, 1.0)
    for dof, p in ((4, 2), (5, 1), (4, 0), (3, 1)):
        assert abs(_corr(base, M.dof_redraw(SEED, GID, EP, dof, p, M.KIND_UNIFORM, 0.0, 1.0))) < 0.01
