"""
Closed-loop policy rollouts, the host side (no GPU): every refusal of backend.check_policy_args, MlpPolicy and MlpPolicy.from_torch with
its reason, and the parameter layout of include/locohip.h lm_mlp_policy against torch.nn.utils.parameters_to_vector.
Device tensors are stood in for by a small description object (shape / dtype / is_contiguous / data_ptr / is_cuda), as the checks
read nothing else; CPU torch tensors are "host tensors" and are refused.
"""

import numpy as np
import pytest
import torch

from loco_mujoco_amd.backend import MlpPolicy, MlpPolicyStruct, check_policy_args

N, NU, NOBS, T = 5, 12, 37, 7


class Dev:
    """What the checks read of a device tensor."""

    def __init__(self, shape, dtype="torch.float32", contiguous=True, cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = tuple(shape), dtype, contiguous, cuda

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 0x1000


def _count(sizes):
    return sum(a * b + b for a, b in zip(sizes[:-1], sizes[1:]))


def _policy(sizes=(NOBS, 40, 24, NU), activation="tanh", log_std=None, **kw):
    return MlpPolicy(sizes, activation, Dev((_count(sizes),), **kw), log_std)


def test_a_valid_call_passes():
    p = _policy(log_std=Dev((NU,)))
    assert check_policy_args(N, NU, NOBS, p, T) == (T, T)
    assert check_policy_args(N, NU, NOBS, p, T, obs0=Dev((N, NOBS)), actions=Dev((T, N, NU)), obs=Dev((T, N, NOBS)), reward=Dev((T, N)),
                             done=Dev((T, N), "torch.uint8"), terminal=Dev((T, N, NOBS)), steps_per_launch=3) == (T, 3)
    assert check_policy_args(N, NU, NOBS, _policy((NOBS, NU)), T, actions=0x2000) == (T, T)          # one linear layer; a raw pointer
    assert check_policy_args(N, NU, NOBS, _policy((NOBS, 256, NU), "relu"), 1) == (1, 1)
    for w in (1, 17, 255):                                  # any width, not only multiples of 16
        _policy((NOBS, w, NU))


@pytest.mark.parametrize("make,reason", [
    (lambda: _policy((NOBS, 0, NU)), "hidden width 0"),
    (lambda: _policy((NOBS, 257, NU)), "hidden width 257"),
    (lambda: _policy((NOBS, 8, 8, 8, NU)), "4 linear layers"),
    (lambda: _policy((NOBS,)), "0 linear layers"),
    (lambda: _policy(activation="gelu"), "activation"),
    (lambda: _policy(activation=2), "activation"),
    (lambda: _policy(dtype="torch.float64"), "params must be float32"),
    (lambda: _policy(contiguous=False), "params must be contiguous"),
    (lambda: _policy(cuda=False), "params must live on the device"),
    (lambda: MlpPolicy((NOBS, 40, NU), "tanh", Dev((_count((NOBS, 40, NU)) - 1,))), "flat tensor of %d elements" % _count((NOBS, 40, NU))),
    (lambda: MlpPolicy((NOBS, 40, NU), "tanh", np.zeros(_count((NOBS, 40, NU)), dtype=np.float32)), "device tensor"),
    (lambda: _policy(log_std=Dev((NU + 1,))), "log_std must be a flat tensor of %d" % NU),
    (lambda: _policy(log_std=Dev((NU,), "torch.float64")), "log_std must be float32"),
    (lambda: _policy(log_std=Dev((NU,), cuda=False)), "log_std must live on the device"),
])
def test_policy_refusals_give_their_reason(make, reason):
    with pytest.raises(ValueError, match=reason):
        make()


@pytest.mark.parametrize("kw,reason", [
    (dict(policy=_policy((NOBS + 1, 40, NU))), "reads 38 inputs, the model's observation has nobs = 37"),
    (dict(policy=_policy((NOBS, 40, NU - 1))), "writes 11 outputs, the model's action has nu = 12"),
    (dict(policy="mlp"), "must be an MlpPolicy"),
    (dict(n_steps=0), "n_steps"),
    (dict(n_steps=2.5), "n_steps"),
    (dict(steps_per_launch=0), "steps_per_launch"),
    (dict(obs0=Dev((N, NOBS + 1))), "obs0 must be"),
    (dict(obs0=Dev((N, NOBS), cuda=False)), "obs0 must live on the device"),
    (dict(actions=Dev((T - 1, N, NU))), "actions must be"),
    (dict(actions=Dev((T, N, NU), "torch.float64")), "actions must be float32"),
    (dict(actions=Dev((T, N, NU), contiguous=False)), "actions must be contiguous"),
    (dict(actions=np.zeros((T, N, NU), dtype=np.float32)), "actions must be a device tensor"),
    (dict(obs=Dev((T, N, NOBS - 1))), "obs must be"),
    (dict(reward=Dev((T, N, 1))), "reward must be"),
    (dict(done=Dev((T, N))), "done must be uint8"),
    (dict(terminal=Dev((T, N, NOBS)), terminal_enabled=False), "terminal observations enabled"),
])
def test_call_refusals_give_their_reason(kw, reason):
    args = dict(policy=_policy(), n_steps=T)
    args.update(kw)
    with pytest.raises(ValueError, match=reason):
        check_policy_args(N, NU, NOBS, args.pop("policy"), args.pop("n_steps"), **args)


def _seq(widths, act=torch.nn.Tanh, nobs=NOBS, nu=NU):
    sizes = (nobs,) + tuple(widths) + (nu,)
    mods = []
    for a, b in zip(sizes[:-1], sizes[1:]):
        mods += [torch.nn.Linear(a, b), act()]
    return torch.nn.Sequential(*mods[:-1])


@pytest.mark.parametrize("make,reason", [
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.Tanh()), "expected Linear"),
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.Linear(8, NU), torch.nn.Linear(NU, NU)), "activations must be"),
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.GELU(), torch.nn.Linear(8, NU)), "activations must be"),
    (lambda: torch.nn.Sequential(torch.nn.Tanh(), torch.nn.Tanh(), torch.nn.Tanh()), "expected a Linear layer"),
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.Tanh(), torch.nn.Linear(8, 8), torch.nn.ReLU(), torch.nn.Linear(8, NU)), "one kind of activation"),
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8, bias=False), torch.nn.Tanh(), torch.nn.Linear(8, NU)), "need a bias"),
    (lambda: torch.nn.Sequential(torch.nn.Linear(NOBS, 8), torch.nn.Tanh(), torch.nn.Linear(9, NU)), "do not chain"),
    (lambda: _seq((8,)).double(), "must be float32"),
    (lambda: _seq((8,)), "must live on the device"),              # a host (CPU) module
    (lambda: _seq((8, 8, 8)), "4 linear layers"),
    (lambda: _seq((300,)), "hidden width 300"),
])
def test_from_torch_refusals_give_their_reason(make, reason, monkeypatch):
    seq = make()
    if reason not in ("must live on the device", "must be float32"):
        # the structure is judged before the tensors: let the CPU parameters pass for device ones
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    if reason == "must be float32":
        monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    with pytest.raises(ValueError, match=reason):
        MlpPolicy.from_torch(seq)


@pytest.mark.parametrize("widths,act", [((40, 24), torch.nn.Tanh), ((256,), torch.nn.ReLU), ((), torch.nn.Tanh)])
def test_parameter_layout_is_parameters_to_vector(widths, act, monkeypatch):
    """sizes, activation and the flat vector of from_torch; and a float64 evaluation that walks the vector the way the header says
    (per layer W [out][in] row-major, then b [out]) gives the module's own output."""
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    torch.manual_seed(0)
    seq = _seq(widths, act)
    p = MlpPolicy.from_torch(seq)
    assert p.sizes == (NOBS,) + tuple(widths) + (NU,) and p.n_layers == len(widths) + 1
    assert p.activation == (1 if act is torch.nn.ReLU else 0)
    vec = torch.nn.utils.parameters_to_vector(seq.parameters()).detach()
    assert torch.equal(p.params, vec) and p.params.numel() == MlpPolicy.n_params(p.sizes)
    st = p.struct()
    assert isinstance(st, MlpPolicyStruct) and st.n_layers == p.n_layers and list(st.sizes)[:len(p.sizes)] == list(p.sizes)
    assert st.d_params == p.params.data_ptr() and st.d_log_std is None
    x = torch.randn(3, NOBS)
    flat, at, h = vec.double().numpy(), 0, x.double().numpy()
    for layer, (a, b) in enumerate(zip(p.sizes[:-1], p.sizes[1:])):
        W = flat[at:at + a * b].reshape(b, a)
        bias = flat[at + a * b:at + a * b + b]
        at += a * b + b
        h = h @ W.T + bias
        if layer < p.n_layers - 1:
            h = np.tanh(h) if p.activation == 0 else np.maximum(h, 0)
    assert at == len(flat)
    assert np.allclose(h, seq(x).detach().numpy(), rtol=0, atol=1e-5)


def test_parameters_that_are_views_of_one_flat_tensor_are_used_in_place(monkeypatch):
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    torch.manual_seed(1)
    seq = _seq((40, 24))
    flat = torch.nn.utils.parameters_to_vector(seq.parameters()).detach().clone()
    at = 0
    for q in seq.parameters():
        q.data = flat[at:at + q.numel()].view_as(q)
        at += q.numel()
    p = MlpPolicy.from_torch(seq)
    assert p.params.data_ptr() == flat.data_ptr() and torch.equal(p.params, flat)
    flat.mul_(0.5)                                  # "an optimiser step": the policy sees it
    assert torch.equal(p.params, flat)
    # separately allocated parameters: one flattened copy
    q = MlpPolicy.from_torch(_seq((40, 24)))
    assert q.params.numel() == MlpPolicy.n_params(q.sizes)
