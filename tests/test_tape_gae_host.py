"""
Advantage estimation over the tapes, the host side (no GPU): every refusal of backend.check_gae_args with its reason. Device tensors
are stood in for by the description object of tests/test_policy_rollout_host.py.
"""

import numpy as np
import pytest
import torch

from loco_mujoco_amd.backend import EXPORTS, check_gae_args
from test_policy_rollout_host import N, T, Dev


def _args(**kw):
    a = dict(reward=Dev((T, N)), done=Dev((T, N), "torch.uint8"), value=Dev((T, N)), last_value=Dev((N,)))
    a.update(kw)
    return a


def test_a_valid_call_passes():
    assert check_gae_args(N, **_args()) == (T, 0.99, 0.95)
    assert check_gae_args(N, **_args(term_value=Dev((T, N)), adv=Dev((T, N)), ret=Dev((T, N)), gamma=1, lam=0)) == (T, 1.0, 0.0)
    assert check_gae_args(N, **_args(gamma=np.float32(0.5), lam=np.float64(1.0))) == (T, 0.5, 1.0)
    assert check_gae_args(N, 0x1000, 0x2000, 0x3000, 0x4000, n_steps=3) == (3, 0.99, 0.95)          # raw pointers are taken as given
    assert check_gae_args(N, **_args(reward=0x1000)) == (T, 0.99, 0.95)                            # T from the described tapes
    assert check_gae_args(N, **_args(n_steps=T)) == (T, 0.99, 0.95)
    assert "lm_tape_gae" in EXPORTS


@pytest.mark.parametrize("kw,reason", [
    (dict(reward=None), "reward is None"),
    (dict(done=None), "done is None"),
    (dict(value=None), "value is None"),
    (dict(last_value=None), "last_value is None"),
    (dict(reward=Dev((T, N + 1))), r"reward must be \[%d, %d\]" % (T, N)),
    (dict(reward=Dev((T * N,))), r"reward must be \[%d, %d\]" % (T, N)),
    (dict(done=Dev((T, N))), "done must be uint8"),
    (dict(done=Dev((T, N), "torch.bool")), "done must be uint8"),
    (dict(value=Dev((T, N), "torch.float64")), "value must be float32"),
    (dict(value=Dev((T + 1, N))), "the value tape holds %d steps, the others T = %d" % (T + 1, T)),
    (dict(n_steps=T - 1), "the reward tape holds %d steps, the others T = %d" % (T, T - 1)),
    (dict(last_value=Dev((N, 1))), r"last_value must be \[%d\]" % N),
    (dict(last_value=Dev((T, N))), r"last_value must be \[%d\]" % N),
    (dict(last_value=Dev((N,), cuda=False)), "last_value must live on the device"),
    (dict(term_value=Dev((T, N), contiguous=False)), "term_value must be contiguous"),
    (dict(term_value=Dev((T, N, 1))), r"term_value must be \[%d, %d\]" % (T, N)),
    (dict(adv=Dev((T, N), "torch.float16")), "adv must be float32"),
    (dict(ret=Dev((N, T))), "the ret tape holds %d steps" % N),
    (dict(reward=torch.zeros(T, N)), "reward must live on the device"),                # a host tensor
    (dict(reward=np.zeros((T, N), dtype=np.float32)), "device tensor"),
    (dict(gamma=-0.01), r"gamma must be in \[0, 1\]"),
    (dict(gamma=1.01), r"gamma must be in \[0, 1\]"),
    (dict(gamma=float("nan")), r"gamma must be in \[0, 1\]"),
    (dict(lam=float("inf")), r"lam must be in \[0, 1\]"),
    (dict(lam=-1), r"lam must be in \[0, 1\]"),
    (dict(lam="0.9"), "lam must be a number"),
    (dict(gamma=True), "gamma must be a number"),
])
def test_refusals_give_their_reason(kw, reason):
    with pytest.raises(ValueError, match="gae: .*" + reason):
        check_gae_args(N, **_args(**kw))


def test_raw_pointers_need_the_number_of_steps():
    with pytest.raises(ValueError, match="raw pointers need n_steps"):
        check_gae_args(N, 0x1000, 0x2000, 0x3000, 0x4000)
    with pytest.raises(ValueError, match="T must be >= 1"):
        check_gae_args(N, 0x1000, 0x2000, 0x3000, 0x4000, n_steps=0)
