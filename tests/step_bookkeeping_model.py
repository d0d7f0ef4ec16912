"""
Host model of the step kernel's bookkeeping (not a test file): the counter-based draws that decide which episode an environment is
in and which actions a policy-free rollout feeds it, restated from include/locohip.h (lm_set_reset_table, lm_set_dof_randomization,
lm_set_model_variants, lm_set_variant_rows, lm_rollout, lm_rollout_fused) and loco_mujoco_amd/csrc/lm_step.h (mix64; the actuation
block; the restart block of step_kernel) with 64-bit integers that wrap, and float64 on the float32 inputs the device uses.

Every function takes Python ints or integer arrays (broadcast against each other) and returns a Python scalar for scalar arguments,
an array otherwise. Plain numpy; nothing here touches the GPU.
"""

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15          # SplitMix64's increment; lm_rollout_fused multiplies its seed argument by it
K_STREAM = 0xD6E8FEB86659FD93        # separates the draws of one (environment, episode) / (environment, step)
K_VARIANT = 0xA24BAED4963EE407       # the variant draw beside the row draw
K_GID_STEP = 0x100000001B3           # global environment id -> the step counter's stream

KIND_KEEP, KIND_NORMAL_CLIPPED, KIND_UNIFORM, KIND_NORMAL = 0, 1, 2, 3
TWO_PI_F32 = float(np.float32(6.2831853))


def _u64(x):
    """Integers (negative ones as the C cast to unsigned long long gives them) -> uint64 array."""
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object or a.dtype.kind not in "iu":
        return np.array([int(v) & MASK64 for v in np.ravel(a)], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).view(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64)


def _c(v):
    return np.uint64(v & MASK64)


def _ret(a):
    a = np.asarray(a)
    return a.item() if a.ndim == 0 else a


def _mix(x):
    with np.errstate(over="ignore"):
        x = x + _c(GOLDEN)
        x = (x ^ (x >> _c(30))) * _c(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _c(27))) * _c(0x94D049BB133111EB)
        return x ^ (x >> _c(31))


def mix64(x):
    """lm_step.h mix64: SplitMix64's output function applied to x + GOLDEN."""
    return _ret(_mix(_u64(x)))


def _episode_key(seed, gid, ep_count_after):
    """seed ^ mix64(gid * 2 + 1) ^ (ec << 32): `ec` is the kernel's 32-bit episode counter AFTER the increment of this restart."""
    with np.errstate(over="ignore"):
        ec = _u64(ep_count_after) & _c(0xFFFFFFFF)
        return _u64(seed) ^ _mix(_u64(gid) * _c(2) + _c(1)) ^ (ec << _c(32))


def restart_row(seed, gid, ep_count_after, n_rows):
    """Row of the reset table from which environment `gid` (global id: the batch's offset + its index) starts the episode that makes
    its episode counter `ep_count_after` (1 at the first device-side restart of a fresh batch)."""
    return _ret(_mix(_episode_key(seed, gid, ep_count_after)) % _c(n_rows))


def variant_draw(seed, gid, ep_count_after, nvar):
    """Model variant drawn with that episode when the variants do not follow the rows (lm_set_variant_rows 0)."""
    return _ret(_mix(_episode_key(seed, gid, ep_count_after) ^ _c(K_VARIANT)) % _c(nvar))


def variant_of_row(row, rows_per_variant):
    """Model variant under lm_set_variant_rows(rows_per_variant): the block of the reset table the row lies in."""
    return _ret(_u64(row) // _c(rows_per_variant))


def dof_redraw_bits(seed, gid, ep_count_after, dof, p):
    """The 64 random bits behind parameter p (0 damping, 1 stiffness, 2 frictionloss) of dof `dof`."""
    with np.errstate(over="ignore"):
        return _ret(_mix(_episode_key(seed, gid, ep_count_after) ^ (_u64(np.asarray(dof) * 3 + np.asarray(p) + 1) * _c(K_STREAM))))


def dof_redraw(seed, gid, ep_count_after, dof, p, kind, a, b, clip=True):
    """Joint parameter drawn with that episode, in float64 from the float32 inputs the device uses: u1 = (float32(r >> 40) + 0.5f) * 2^-24
    (the sum rounded to float32 as on the device), u2 = ((r >> 16) & 0xFFFFFF) * 2^-24, the float32 constant 6.2831853f and the spec's
    float32 (a, b). kind 2: a + (b - a) * u1; kinds 1 and 3: b * sqrt(-2 ln u1) * cos(2 pi u2) + a, clipped at 0 unless clip=False."""
    if kind == KIND_KEEP:
        raise ValueError("kind 0 keeps the value: nothing is drawn")
    r = _u64(dof_redraw_bits(seed, gid, ep_count_after, dof, p))
    a, b = float(np.float32(a)), float(np.float32(b))
    hi = (r >> _c(40)).astype(np.float32) + np.float32(0.5)            # float32 sum: 25 significant bits round to 24
    u1 = hi.astype(np.float64) * 2.0 ** -24
    u2 = ((r >> _c(16)) & _c(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    if kind == KIND_UNIFORM:
        return _ret(a + (b - a) * u1)
    z = np.sqrt(-2.0 * np.log(u1)) * np.cos(TWO_PI_F32 * u2)
    v = b * z + a
    return _ret(np.maximum(v, 0.0) if clip else v)


def random_action_bits(seed_eff, gid, step_index, k):
    """The 24 bits (r >> 40) behind action entry k of environment `gid` in the batch's `step_index`-th control step."""
    with np.errstate(over="ignore"):
        step = _u64(step_index) & _c(0xFFFFFFFF)
        r = _mix(_u64(seed_eff) ^ _mix(_u64(gid) * _c(K_GID_STEP) + step) ^ (_u64(np.asarray(k) + 1) * _c(K_STREAM)))
        return _ret(r >> _c(40))


def random_action(seed_eff, gid, step_index, k):
    """Action entry k of lm_rollout's random policy (action_mode 1): (r >> 40) * 2^-23 - 1, exact in float32, in [-1, 1).
    `seed_eff` is rollout_seed(batch seed, the rollout's seed argument); `step_index` counts the batch's control steps from 0."""
    top = np.asarray(random_action_bits(seed_eff, gid, step_index, k), dtype=np.uint64)
    return _ret((top.astype(np.float64) * 2.0 ** -23 - 1.0).astype(np.float32))


def rollout_seed(batch_seed, rollout_seed):
    """The seed lm_rollout / lm_rollout_fused run under: the batch's (lm_set_reset_table; 0 without a table) xor the call's seed argument
    times GOLDEN. It keys the rollout's actions AND its restart draws; seed argument 0 leaves the batch's seed as lm_step uses it."""
    return ((int(batch_seed) & MASK64) ^ ((int(rollout_seed) * GOLDEN) & MASK64)) & MASK64
