"""
Policy input normalisation, the host side (no GPU): every refusal of backend.check_obs_norm_args with its reason, ObsNorm's running
moments against float64 numpy, and ObsNorm.normalize as the stated expression, bit for bit. Device tensors are stood in for by the
description object of tests/test_policy_rollout_host.py; ObsNorm itself runs on CPU torch tensors here.
"""

import numpy as np
import pytest
import torch

from loco_mujoco_amd.backend import EXPORTS, ObsNorm, check_obs_norm_args
from test_policy_rollout_host import NOBS, Dev


def test_a_valid_call_passes():
    assert check_obs_norm_args(NOBS, Dev((NOBS,)), Dev((NOBS,)), 5) == 5.0
    assert check_obs_norm_args(NOBS, Dev((NOBS,)), Dev((NOBS,)), 0.0) == 0.0          # no clamp
    assert check_obs_norm_args(NOBS, None, None, 0.0) == 0.0                          # off
    assert check_obs_norm_args(NOBS, 0x1000, 0x2000, np.float32(2.5)) == 2.5          # raw pointers are taken as given
    assert "lm_set_policy_obs_norm" in EXPORTS


@pytest.mark.parametrize("mean,inv_std,clip,reason", [
    (Dev((NOBS,)), None, 1.0, "mean and inv_std go together"),
    (None, Dev((NOBS,)), 1.0, "mean and inv_std go together"),
    (Dev((NOBS,)), Dev((NOBS,)), -1.0, "clip must be finite and >= 0"),
    (Dev((NOBS,)), Dev((NOBS,)), float("nan"), "clip must be finite and >= 0"),
    (Dev((NOBS,)), Dev((NOBS,)), float("inf"), "clip must be finite and >= 0"),
    (None, None, -1.0, "clip must be finite and >= 0"),
    (Dev((NOBS,)), Dev((NOBS,)), "1", "clip must be a number"),
    (Dev((NOBS,)), Dev((NOBS,)), True, "clip must be a number"),
    (Dev((NOBS + 1,)), Dev((NOBS,)), 1.0, r"mean must be \[%d\]" % NOBS),
    (Dev((NOBS,)), Dev((NOBS - 1,)), 1.0, r"inv_std must be \[%d\]" % NOBS),
    (Dev((1, NOBS)), Dev((NOBS,)), 1.0, r"mean must be \[%d\]" % NOBS),
    (Dev((NOBS,), "torch.float64"), Dev((NOBS,)), 1.0, "mean must be float32"),
    (Dev((NOBS,)), Dev((NOBS,), "torch.float16"), 1.0, "inv_std must be float32"),
    (Dev((NOBS,), contiguous=False), Dev((NOBS,)), 1.0, "mean must be contiguous"),
    (Dev((NOBS,)), Dev((NOBS,), cuda=False), 1.0, "inv_std must live on the device"),
    (torch.zeros(NOBS), torch.ones(NOBS), 1.0, "mean must live on the device"),       # a host tensor
    (np.zeros(NOBS, dtype=np.float32), Dev((NOBS,)), 1.0, "device tensor"),
    (Dev((NOBS,)), [1.0] * NOBS, 1.0, "device tensor"),
])
def test_refusals_give_their_reason(mean, inv_std, clip, reason):
    with pytest.raises(ValueError, match="set_policy_obs_norm: .*" + reason):
        check_obs_norm_args(NOBS, mean, inv_std, clip)


def test_update_over_three_chunks_is_the_moments_of_the_concatenation():
    rng = np.random.RandomState(0)
    scale, shift = rng.uniform(0.01, 30.0, NOBS), rng.uniform(-50.0, 50.0, NOBS)
    chunks = [(rng.standard_normal(shape + (NOBS,)) * scale + shift).astype(np.float32) for shape in ((7, 5), (1,), (3, 2, 4))]
    norm = ObsNorm(NOBS, "cpu", clip=5.0, eps=1e-8)
    assert norm.mean.dtype == torch.float32 and norm.inv_std.dtype == torch.float32
    assert (norm.mean == 0).all() and (norm.inv_std == 1).all()                         # the identity until the first update
    at = norm.mean.data_ptr(), norm.inv_std.data_ptr()
    for c in chunks:
        norm.update(torch.from_numpy(c))
        assert (norm.mean.data_ptr(), norm.inv_std.data_ptr()) == at                    # rewritten in place
    every = np.concatenate([c.reshape(-1, NOBS) for c in chunks]).astype(np.float64)
    assert norm.count == len(every) == 35 + 1 + 24
    assert norm.mean64.dtype == torch.float64 and norm.m2.dtype == torch.float64
    np.testing.assert_allclose(norm.mean64.numpy(), every.mean(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose((norm.m2 / norm.count).numpy(), every.var(0), rtol=1e-12, atol=0)
    # the float32 tensors the kernel reads are the float64 state rounded once
    assert np.array_equal(norm.mean.numpy(), norm.mean64.numpy().astype(np.float32))
    np.testing.assert_allclose(norm.inv_std.numpy(), 1.0 / np.sqrt(every.var(0) + 1e-8), rtol=2.0 ** -23)
    with pytest.raises(ValueError, match="nobs"):
        norm.update(torch.zeros(4, NOBS + 1))
    norm.update(torch.zeros(0, NOBS))                                                   # nothing to merge
    assert norm.count == len(every)


@pytest.mark.parametrize("clip", [0.0, 1.0, 5.0])
def test_normalize_is_the_stated_expression_bit_for_bit(clip):
    rng = np.random.RandomState(1)
    norm = ObsNorm(NOBS, "cpu", clip=clip)
    norm.update(torch.from_numpy((rng.standard_normal((64, NOBS)) * 3 + 1).astype(np.float32)))
    x = torch.from_numpy((rng.standard_normal((9, 4, NOBS)) * 6).astype(np.float32))
    x[0, 0, 0], x[3, 2, 5], x[8, 3, NOBS - 1] = float("nan"), float("inf"), -float("inf")
    got = norm.normalize(x)
    want = (x - norm.mean) * norm.inv_std
    if clip > 0:
        want = want.clamp(-clip, clip)
    assert got.dtype == torch.float32
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    # the same in numpy float32, operation by operation: what the kernel's subtraction, multiplication and two selects compute
    t = (x.numpy() - norm.mean.numpy()) * norm.inv_std.numpy()
    if clip > 0:
        t = np.where(t < -np.float32(clip), -np.float32(clip), np.where(t > np.float32(clip), np.float32(clip), t))
    assert t.dtype == np.float32
    assert np.array_equal(np.isnan(t), np.isnan(got.numpy())) and bool(got[0, 0, 0].isnan())        # a NaN stays a NaN
    assert np.array_equal(t[~np.isnan(t)], got.numpy()[~np.isnan(t)])
    if clip > 0:
        assert got[3, 2, 5] == clip and got[8, 3, NOBS - 1] == -clip and (got[~got.isnan()].abs() <= clip).all()
        assert (got.abs() == clip).any() and (got.abs() < clip).any()
    else:
        assert got[3, 2, 5] == float("inf")
