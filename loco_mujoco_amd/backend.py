"""
ctypes loader for ``liblocohip.so`` (C-ABI: ``include/locohip.h``) — the ONLY physics path of the
product. There is no CPU fallback: if the library or a GPU is missing this module raises.
"""

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOCOHIP_LIB", os.path.join(_HERE, "csrc", "liblocohip.so"))   # override: kernel A/B builds

_F = C.POINTER(C.c_float)
_U8 = C.POINTER(C.c_uint8)
_D = C.POINTER(C.c_double)
_I32 = C.POINTER(C.c_int32)


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nq", "nv", "nu", "nobs", "ngoal", "n_substeps", "n_chains", "max_chain_dofs", "na")]


class Stats(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("env_steps", "episodes", "reward_sum", "nan_resets", "solver_iters",
                                          "overflow_contacts", "unhandled_geoms", "linesearch_evals", "linesearch_capped", "steps_with_8plus_iters", "kernel_ms",
                                          "self_proximity", "self_contacts", "replayed_env_steps", "own_manifold_contacts")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class MlpPolicyStruct(C.Structure):
    """``lm_mlp_policy`` of include/locohip.h."""
    _fields_ = [("n_layers", C.c_int), ("sizes", C.c_int * 4), ("activation", C.c_int), ("d_params", C.c_void_p), ("d_log_std", C.c_void_p)]


class ForwardOut(C.Structure):
    _fields_ = [(n, _F) for n in ("M", "qfrc_bias", "qfrc_smooth", "qacc_smooth", "qacc", "qfrc_constraint")] + \
               [("ncon", C.POINTER(C.c_int)), ("solver_iter", C.POINTER(C.c_int))]


# THE prototypes of include/locohip.h, stated once: name -> (restype, argtypes). load_library() declares every one of them and EXPORTS
# is the key list, so an export cannot be listed and left to ctypes' default conversions. argtypes None: the function takes no argument
_P, _I, _LL, _U64, _FL, _ST = C.c_void_p, C.c_int, C.c_longlong, C.c_uint64, C.c_float, C.POINTER(Stats)
_PROTOTYPES = {
    "lm_device_count": (_I, None), "lm_last_error": (C.c_char_p, None), "lm_toolchain": (C.c_char_p, None),
    "lm_lds_bytes": (_I, [_I, _I, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "lm_model_create": (_I, [_D, C.c_size_t, _I, C.POINTER(_P)]), "lm_model_destroy": (None, [_P]), "lm_model_dims": (_I, [_P, C.POINTER(Dims)]),
    "lm_batch_create": (_I, [_P, _I, C.POINTER(_P)]), "lm_batch_destroy": (None, [_P]),
    "lm_batch_set_layout": (_I, [_P, _I]), "lm_batch_set_replay": (_I, [_P, _I]), "lm_batch_set_active": (_I, [_P, _I32, _I]),
    "lm_get_replay_marks": (_I, [_P, _U8, _I]),
    "lm_set_state": (_I, [_P, _F, _F, _U8]), "lm_get_state": (_I, [_P, _F, _F]),
    "lm_set_activation": (_I, [_P, _F, _U8]), "lm_get_activation": (_I, [_P, _F]),
    "lm_set_dof_params": (_I, [_P, _F, _F, _F, _U8]), "lm_get_dof_params": (_I, [_P, _F, _F, _F]), "lm_set_dof_randomization": (_I, [_P, _F]),
    "lm_set_goal": (_I, [_P, _F, _U8]),
    "lm_step": (_I, [_P, _F, _F, _F, _U8]), "lm_step_device": (_I, [_P, _P, _P, _P, _P, _P, _I]),
    "lm_pinned_slot": (_I, [_P, _I, C.POINTER(_D), C.POINTER(_D), C.POINTER(_U8)]), "lm_set_obs_order": (_I, [_P, _I32, _I]),
    "lm_step_pinned": (_I, [_P, _D, _I]),
    "lm_set_terminal_obs": (_I, [_P, _I, _P]), "lm_get_terminal_obs": (_I, [_P, _F]), "lm_pinned_terminal_obs": (_I, [_P, _I, C.POINTER(_D)]),
    "lm_set_reset_table": (_I, [_P, _F, _I, _U64, C.c_int64]), "lm_set_auto_reset": (_I, [_P, _I, _I]),
    "lm_rollout": (_I, [_P, _I, _I, _U64, _ST]), "lm_rollout_fused": (_I, [_P, _I, _I, _I, _U64, _ST]),
    "lm_rollout_tape": (_I, [_P, _I, _I, _P, _LL, _P, _P, _P, _P, _P, _I, _ST]),
    "lm_rollout_policy": (_I, [_P, C.POINTER(MlpPolicyStruct), _I, _I, _U64, _P, _P, _P, _P, _P, _P, _P, _I, _ST]),
    "lm_set_policy_obs_norm": (_I, [_P, _P, _P, _FL]),
    "lm_tape_gae": (_I, [_P, _I, _P, _P, _P, _P, _P, _FL, _FL, _P, _P, _P, _I]),
    "lm_forward_debug": (_I, [_P, _F, C.POINTER(ForwardOut)]), "lm_get_stats": (_I, [_P, _ST, _I]), "lm_sync": (_I, [_P]),
    "lm_get_flags": (_I, [_P, _U8]),
    "lm_set_model_variants": (_I, [_P, _F, _F, _F, _I, _I]), "lm_set_variant_index": (_I, [_P, _I32, _U8]),
    "lm_get_variant_index": (_I, [_P, _I32]), "lm_set_variant_rows": (_I, [_P, _I]),
    "lm_set_model_compiler": (_I, [_P, _I32, _LL, _D, _LL, _F, _F, _F, _I, _U64]), "lm_compile_models": (_I, [_P, _U8]),
    "lm_get_model_draws": (_I, [_P, _D, C.POINTER(C.c_uint32)]), "lm_get_model_tables": (_I, [_P, _I, _F, _F, _F]),
    "lm_snapshot_create": (_I, [_P, _I, C.POINTER(_P)]), "lm_snapshot_destroy": (None, [_P]),
    "lm_snapshot_save": (_I, [_P, _P, _P, _I]), "lm_snapshot_restore": (_I, [_P, _P, _P, _P, _I]), "lm_snapshot_bytes": (_LL, [_P]),
    "lm_snapshot_export": (_I, [_P, _P, _P, _LL]), "lm_snapshot_import": (_I, [_P, _P, _P, _LL]),
}
EXPORTS = list(_PROTOTYPES)
# THE prototypes of include/locostate.h (state on device buffers; the same library, a header and a prefix of its own), stated once
_STATE_PROTOTYPES = {
    "ls_get_state_device": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I]), "ls_set_state_device": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I]),
    "ls_restart_device": (_I, [_P, _P, _P, _P, _I]),
}
STATE_EXPORTS = list(_STATE_PROTOTYPES)

_lib = None


class BackendError(RuntimeError):
    pass


def load_library():
    """Load liblocohip.so and declare its prototypes. Raises BackendError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendError("HIP library not built: %s is missing (run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C loco_mujoco_amd/csrc`). There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in list(_PROTOTYPES.items()) + list(_STATE_PROTOTYPES.items()):
        fn = getattr(lib, name)
        fn.restype = restype          # (c_int is also what ctypes assumes)
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise BackendError("liblocohip: %s (code %d)" % (load_library().lm_last_error().decode(), rc))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def _ptr(a, ctype=_F):
    """A host array as the C pointer a prototype asks for."""
    return a.ctypes.data_as(ctype)


def _mask(mask, n):
    if mask is None:
        return None, None
    m = np.ascontiguousarray(mask, dtype=np.uint8).reshape(n)
    return m, _ptr(m, _U8)


# THE device-buffer check's wording per fault; a caller whose messages read differently passes its own templates over the same values
_BUFFER_FAULTS = {"pointer": "%(who)s: %(name)s must be a device tensor (data_ptr()) or a raw device pointer (int), not %(type)s",
                  "shape": "%(who)s: %(name)s must be %(shape)s, not %(got)s",
                  "dtype": "%(who)s: %(name)s must be %(dtype)s, not %(got)s",
                  "contiguous": "%(who)s: %(name)s must be contiguous",
                  "device": "%(who)s: %(name)s must live on the device"}


def _check_device_buffer(who, name, x, shape, dtype, raw=True, faults=("shape", "dtype", "contiguous", "device"), say=None):
    """``x``: a raw device pointer (int), taken as given (``raw`` False: refused), or a described object (torch tensor, anything with
    ``shape`` / ``dtype`` / ``is_contiguous()`` / ``data_ptr()``): ``shape``, ``dtype``, contiguous, on the device, looked at in the order
    of ``faults`` (empty: only that ``x`` is a buffer at all). ``say``: the caller's own wording of some faults (_BUFFER_FAULTS)."""
    def refuse(fault, **found):
        raise ValueError((say or {}).get(fault, _BUFFER_FAULTS[fault]) % dict(found, who=who, name=name, dtype=dtype))

    if not hasattr(x, "data_ptr"):
        if not raw or isinstance(x, bool) or not isinstance(x, (int, np.integer)):
            refuse("pointer", type=type(x).__name__)
        return
    for fault in faults:
        if fault == "shape" and tuple(x.shape) != tuple(shape):
            refuse(fault, shape=list(shape), got=list(x.shape), got_tuple=tuple(x.shape))
        if fault == "dtype" and dtype not in str(x.dtype):
            refuse(fault, got=x.dtype)
        if fault == "contiguous" and not x.is_contiguous():
            refuse(fault)
        if fault == "device" and hasattr(x, "is_cuda") and not x.is_cuda:
            refuse(fault)


def _number(who, name, v):
    """``v`` as a float: a real number, not a bool."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s: %s must be a number, not %s" % (who, name, type(v).__name__))
    return float(v)


def _tape_table(n, nobs):
    """The tapes a rollout records, [T] in front of each: (name, shape of one step, dtype)."""
    return (("obs", (n, nobs), "float32"), ("reward", (n,), "float32"), ("done", (n,), "uint8"), ("terminal", (n, nobs), "float32"))


def check_tape_args(n, nu, nobs, actions, obs=None, reward=None, done=None, terminal=None, steps_per_launch=None, repeat=None,
                    n_steps=None, terminal_enabled=True):
    """The argument checks of :meth:`HipBatch.rollout_tape`, without a device: returns ``(T, action_step_stride, steps_per_launch)``
    or raises ValueError. Buffers are objects with ``shape`` / ``dtype`` / ``is_contiguous()`` / ``data_ptr()`` (torch tensors), which
    are checked, or raw device pointers (ints), which are taken as given and need ``n_steps`` (a tape) or ``repeat``."""
    who = "rollout_tape"
    given = dict(actions=actions, obs=obs, reward=reward, done=done, terminal=terminal)
    for name, x in given.items():          # what is no buffer at all is refused before anything is said about any of them
        if x is not None:
            _check_device_buffer(who, name, x, None, None, faults=())
    if actions is None:
        raise ValueError("rollout_tape: actions is None (policy-free rollouts: rollout())")
    described = hasattr(actions, "data_ptr")
    if repeat is not None:
        T, stride = int(repeat), 0
        if n_steps is not None and int(n_steps) != T:
            raise ValueError("rollout_tape: n_steps and repeat disagree")
        if described and len(actions.shape) != 2:
            raise ValueError("rollout_tape: with repeat, actions must be [%d, %d], not %s" % (n, nu, list(actions.shape)))
        _check_device_buffer(who, "actions", actions, (n, nu), "float32")
    else:
        if described:
            if len(actions.shape) != 3:
                raise ValueError("rollout_tape: actions must be [T, %d, %d] (or [%d, %d] with repeat=T), not %s" % (n, nu, n, nu, list(actions.shape)))
            T = int(actions.shape[0])
            if n_steps is not None and int(n_steps) != T:
                raise ValueError("rollout_tape: n_steps = %d, but the action tape holds T = %d steps" % (int(n_steps), T))
        elif n_steps is None:
            raise ValueError("rollout_tape: a raw action pointer needs n_steps (a tape) or repeat")
        else:
            T = int(n_steps)
        stride = n * nu
        _check_device_buffer(who, "actions", actions, (T, n, nu), "float32")
    if T < 1:
        raise ValueError("rollout_tape: T must be >= 1, not %d" % T)
    for name, step, dtype in _tape_table(n, nobs):
        x = given[name]
        if x is None:
            continue
        if hasattr(x, "data_ptr") and len(x.shape) >= 1 and int(x.shape[0]) != T:
            raise ValueError("rollout_tape: the %s tape holds %d steps, the actions T = %d" % (name, int(x.shape[0]), T))
        _check_device_buffer(who, name, x, (T,) + step, dtype)
    if terminal is not None and not terminal_enabled:
        raise ValueError("rollout_tape: a terminal tape needs terminal observations enabled (enable_terminal_obs)")
    spl = T if steps_per_launch is None else int(steps_per_launch)
    if spl < 1:
        raise ValueError("rollout_tape: steps_per_launch must be >= 1, not %d" % spl)
    return T, stride, spl


POLICY_MAX_LAYERS, POLICY_MAX_WIDTH = 3, 256          # include/locohip.h lm_mlp_policy
POLICY_ACTIVATIONS = {"tanh": 0, "relu": 1}


def _check_policy_tensor(name, x, count):
    """A tensor of :class:`MlpPolicy`: float32, ``count`` elements, contiguous, on the device, and no raw pointer (``struct()`` asks it for
    its ``data_ptr()``). Its dtype is looked at before its shape, and its shape is worded as a count."""
    _check_device_buffer("MlpPolicy", name, x, (count,), "float32", raw=False, faults=("dtype", "shape", "contiguous", "device"),
                         say={"pointer": "%(who)s: %(name)s must be a device tensor (data_ptr()), not %(type)s",
                              "shape": "%%(who)s: %%(name)s must be a flat tensor of %d elements, not %%(got)s" % count})


class MlpPolicy:
    """A small MLP policy for :meth:`HipBatch.rollout_policy` (``lm_mlp_policy``): ``sizes`` = (nobs, hidden widths ..., nu) with one
    to three linear layers and hidden widths 1..256, ``activation`` "tanh" or "relu" after every layer but the last, ``params`` ONE
    flat float32 device tensor — per layer W [out, in] row-major, then b [out]: ``torch.nn.utils.parameters_to_vector`` of a
    ``Sequential(Linear, act, Linear, act, Linear)`` — and ``log_std`` None (deterministic) or a float32 device tensor [nu]. The
    kernel reads both tensors in place at every step: an optimiser that updates them in place needs no further call. The object keeps
    references to the tensors and nothing else."""

    def __init__(self, sizes, activation, params, log_std=None):
        self.sizes = tuple(int(v) for v in sizes)
        if isinstance(activation, str):
            if activation not in POLICY_ACTIVATIONS:
                raise ValueError("MlpPolicy: activation must be 'tanh' or 'relu', not %r" % (activation,))
            activation = POLICY_ACTIVATIONS[activation]
        self.activation = int(activation)
        if self.activation not in (0, 1):
            raise ValueError("MlpPolicy: activation must be 0 (tanh) or 1 (relu), not %d" % self.activation)
        n_layers = len(self.sizes) - 1
        if n_layers < 1 or n_layers > POLICY_MAX_LAYERS:
            raise ValueError("MlpPolicy: %d linear layers; one to %d are supported" % (n_layers, POLICY_MAX_LAYERS))
        for w in self.sizes[1:-1]:
            if w < 1 or w > POLICY_MAX_WIDTH:
                raise ValueError("MlpPolicy: hidden width %d is outside 1..%d" % (w, POLICY_MAX_WIDTH))
        for name, w in (("nobs", self.sizes[0]), ("nu", self.sizes[-1])):
            if w < 1 or w > POLICY_MAX_WIDTH:
                raise ValueError("MlpPolicy: %s = %d is outside 1..%d" % (name, w, POLICY_MAX_WIDTH))
        _check_policy_tensor("params", params, self.n_params(self.sizes))
        if log_std is not None:
            _check_policy_tensor("log_std", log_std, self.sizes[-1])
        self.params, self.log_std = params, log_std

    @staticmethod
    def n_params(sizes):
        return sum(int(a) * int(b) + int(b) for a, b in zip(sizes[:-1], sizes[1:]))

    @property
    def n_layers(self):
        return len(self.sizes) - 1

    @classmethod
    def from_torch(cls, sequential, log_std=None):
        """From a ``torch.nn.Sequential`` of Linear layers (with bias) separated by ONE kind of activation, ``nn.Tanh`` or ``nn.ReLU``,
        and ending in a Linear layer; anything else is refused. Where the module's parameters are already consecutive views of one flat
        float32 tensor (as after ``p.data = flat[a:b].view_as(p)``), that storage is used in place; otherwise they are flattened ONCE
        (``parameters_to_vector``) and the copy is kept in ``policy.params`` — re-create the policy after an optimiser step then."""
        import torch
        mods = list(sequential)
        if not mods or len(mods) % 2 != 1:
            raise ValueError("MlpPolicy.from_torch: expected Linear (, activation, Linear)*, got %d modules" % len(mods))
        linears, acts = mods[0::2], mods[1::2]
        for m in linears:
            if not isinstance(m, torch.nn.Linear):
                raise ValueError("MlpPolicy.from_torch: expected a Linear layer, found %s" % type(m).__name__)
            if m.bias is None:
                raise ValueError("MlpPolicy.from_torch: Linear layers need a bias")
        kinds = {type(m) for m in acts}
        if not kinds <= {torch.nn.Tanh, torch.nn.ReLU}:
            raise ValueError("MlpPolicy.from_torch: activations must be nn.Tanh or nn.ReLU, found %s" % sorted(k.__name__ for k in kinds))
        if len(kinds) > 1:
            raise ValueError("MlpPolicy.from_torch: one kind of activation per policy, found Tanh and ReLU")
        for a, b in zip(linears[:-1], linears[1:]):
            if a.out_features != b.in_features:
                raise ValueError("MlpPolicy.from_torch: layer widths do not chain: %d -> %d" % (a.out_features, b.in_features))
        sizes = [linears[0].in_features] + [m.out_features for m in linears]
        activation = 1 if kinds == {torch.nn.ReLU} else 0
        ps = [p for m in linears for p in (m.weight, m.bias)]
        for p in ps:
            if p.dtype != torch.float32:
                raise ValueError("MlpPolicy.from_torch: parameters must be float32, not %s" % p.dtype)
            if not p.is_contiguous():
                raise ValueError("MlpPolicy.from_torch: parameters must be contiguous")
            if not p.is_cuda:
                raise ValueError("MlpPolicy.from_torch: parameters must live on the device")
        flat, at = None, ps[0].data_ptr()
        in_place = True
        for p in ps:
            in_place = in_place and p.data_ptr() == at and p.untyped_storage().data_ptr() == ps[0].untyped_storage().data_ptr()
            at += 4 * p.numel()
        if in_place:
            flat = torch.as_strided(ps[0].detach(), (cls.n_params(sizes),), (1,))
        else:
            flat = torch.nn.utils.parameters_to_vector(ps).detach().contiguous()
        policy = cls(sizes, activation, flat, log_std.detach() if hasattr(log_std, "detach") else log_std)
        policy.module = sequential
        return policy

    def struct(self):
        st = MlpPolicyStruct()
        st.n_layers = self.n_layers
        for i, w in enumerate(self.sizes):
            st.sizes[i] = w
        st.activation = self.activation
        st.d_params = int(self.params.data_ptr())
        st.d_log_std = int(self.log_std.data_ptr()) if self.log_std is not None else None
        return st


def check_policy_args(n, nu, nobs, policy, n_steps, obs0=None, actions=None, obs=None, reward=None, done=None, terminal=None,
                      steps_per_launch=None, terminal_enabled=True):
    """The argument checks of :meth:`HipBatch.rollout_policy`, without a device: returns ``(T, steps_per_launch)`` or raises ValueError.
    Buffers are described objects (torch tensors), which are checked, or raw device pointers (ints), which are taken as given."""
    who = "rollout_policy"
    if not isinstance(policy, MlpPolicy):
        raise ValueError("rollout_policy: policy must be an MlpPolicy, not %s" % type(policy).__name__)
    if policy.sizes[0] != nobs:
        raise ValueError("rollout_policy: the policy reads %d inputs, the model's observation has nobs = %d" % (policy.sizes[0], nobs))
    if policy.sizes[-1] != nu:
        raise ValueError("rollout_policy: the policy writes %d outputs, the model's action has nu = %d" % (policy.sizes[-1], nu))
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or int(n_steps) < 1:
        raise ValueError("rollout_policy: n_steps must be an integer >= 1, not %r" % (n_steps,))
    T = int(n_steps)
    given = dict(obs=obs, reward=reward, done=done, terminal=terminal)
    for name, x, shape, dtype in [("obs0", obs0, (n, nobs), "float32"), ("actions", actions, (T, n, nu), "float32")] + \
                                 [(name, given[name], (T,) + step, dtype) for name, step, dtype in _tape_table(n, nobs)]:
        if x is not None:
            _check_device_buffer(who, name, x, shape, dtype)
    if terminal is not None and not terminal_enabled:
        raise ValueError("rollout_policy: a terminal tape needs terminal observations enabled (enable_terminal_obs)")
    spl = T if steps_per_launch is None else int(steps_per_launch)
    if spl < 1:
        raise ValueError("rollout_policy: steps_per_launch must be >= 1, not %d" % spl)
    return T, spl


def check_obs_norm_args(nobs, mean, inv_std, clip):
    """The argument checks of :meth:`HipBatch.set_policy_obs_norm`, without a device: returns ``clip`` as a float or raises ValueError.
    ``mean`` / ``inv_std``: both None (off), or both float32 [nobs], contiguous, on the device — described objects (torch tensors), which
    are checked, or raw device pointers (ints), which are taken as given. ``clip``: finite and >= 0 (0: no clamp)."""
    who = "set_policy_obs_norm"
    if (mean is None) != (inv_std is None):
        raise ValueError("%s: mean and inv_std go together (both None: off)" % who)
    clip = _number(who, "clip", clip)
    if not np.isfinite(clip) or clip < 0:
        raise ValueError("%s: clip must be finite and >= 0 (0: no clamp), not %r" % (who, clip))
    if mean is not None:
        _check_device_buffer(who, "mean", mean, (nobs,), "float32")
        _check_device_buffer(who, "inv_std", inv_std, (nobs,), "float32")
    return clip


def check_gae_args(n, reward, done, value, last_value, term_value=None, gamma=0.99, lam=0.95, adv=None, ret=None, n_steps=None):
    """The argument checks of :meth:`HipBatch.gae`, without a device: returns ``(T, gamma, lam)`` or raises ValueError. Buffers are
    described objects (torch tensors), which are checked — ``reward`` / ``value`` / ``term_value`` / ``adv`` / ``ret`` float32 [T, n],
    ``done`` uint8 [T, n], ``last_value`` float32 [n] — or raw device pointers (ints), which are taken as given; T comes from the
    first described tape, or from ``n_steps`` when every tape is a raw pointer."""
    who = "gae"
    for name, x in (("reward", reward), ("done", done), ("value", value), ("last_value", last_value)):
        if x is None:
            raise ValueError("%s: %s is None" % (who, name))
    tapes = (("reward", reward, "float32"), ("done", done, "uint8"), ("value", value, "float32"), ("term_value", term_value, "float32"),
             ("adv", adv, "float32"), ("ret", ret, "float32"))
    T = None if n_steps is None else int(n_steps)
    for name, x, _ in tapes:
        if x is not None and hasattr(x, "data_ptr") and len(x.shape) == 2:
            if T is None:
                T = int(x.shape[0])
            elif int(x.shape[0]) != T:
                raise ValueError("%s: the %s tape holds %d steps, the others T = %d" % (who, name, int(x.shape[0]), T))
    if T is None:
        raise ValueError("%s: raw pointers need n_steps" % who)
    if T < 1:
        raise ValueError("%s: T must be >= 1, not %d" % (who, T))
    for name, x, dtype in tapes:
        if x is not None:
            _check_device_buffer(who, name, x, (T, n), dtype)
    _check_device_buffer(who, "last_value", last_value, (n,), "float32")
    out = []
    for name, g in (("gamma", gamma), ("lam", lam)):
        g = _number(who, name, g)
        if not (0.0 <= g <= 1.0):
            raise ValueError("%s: %s must be in [0, 1], not %r" % (who, name, g))
        out.append(g)
    return T, out[0], out[1]




class ObsNorm:
    """The running observation normaliser of :meth:`HipBatch.set_policy_obs_norm`: owns the two float32 device tensors ``mean`` and
    ``inv_std`` [nobs] that the policy kernels read in place, and the float64 running count / mean / M2 behind them.
    :meth:`update` merges the moments of a chunk of observations and rewrites both tensors in place; :meth:`normalize` is the expression
    the kernel evaluates, so ``pi(norm.normalize(prev))`` sees bit for bit the inputs the recorded actions were computed from."""

    def __init__(self, nobs, device, clip=10.0, eps=1e-8):
        import torch
        self.nobs, self.clip, self.eps = int(nobs), float(clip), float(eps)
        if not np.isfinite(self.clip) or self.clip < 0:
            raise ValueError("ObsNorm: clip must be finite and >= 0 (0: no clamp), not %r" % self.clip)
        if not np.isfinite(self.eps) or self.eps < 0:
            raise ValueError("ObsNorm: eps must be finite and >= 0, not %r" % self.eps)
        self.mean = torch.zeros(self.nobs, dtype=torch.float32, device=device)
        self.inv_std = torch.ones(self.nobs, dtype=torch.float32, device=device)
        self.count = 0
        self.mean64 = torch.zeros(self.nobs, dtype=torch.float64, device=device)
        self.m2 = torch.zeros(self.nobs, dtype=torch.float64, device=device)

    def update(self, obs):
        """Merge the moments of ``obs`` [..., nobs] (Chan's parallel merge, float64) and rewrite ``mean`` / ``inv_std`` in place."""
        import torch
        if int(obs.shape[-1]) != self.nobs:
            raise ValueError("ObsNorm.update: the last dimension must be nobs = %d, not %d" % (self.nobs, int(obs.shape[-1])))
        x = obs.detach().reshape(-1, self.nobs).to(device=self.mean64.device, dtype=torch.float64)
        m = int(x.shape[0])
        if m == 0:
            return
        var, mean = torch.var_mean(x, dim=0, unbiased=False)
        total = self.count + m
        delta = mean - self.mean64
        self.mean64 += delta * (m / total)
        self.m2 += var * m + delta * delta * (self.count * m / total)
        self.count = total
        self.mean.copy_(self.mean64)
        self.inv_std.copy_(1.0 / torch.sqrt(self.m2 / total + self.eps))

    def normalize(self, x):
        y = (x - self.mean) * self.inv_std
        return y.clamp(-self.clip, self.clip) if self.clip > 0 else y


def check_terminal_obs_args(n, nobs, out):
    """The argument check of :meth:`HipBatch.enable_terminal_obs`, without a device: ``out`` None (the batch's own buffer), a described
    object (torch tensor), which is checked — float32 [n, nobs], contiguous, on the device — or anything else, which ``int()`` makes the
    raw device pointer. Raises ValueError."""
    if hasattr(out, "data_ptr"):
        _check_device_buffer("terminal observations", "the buffer", out, (n, nobs), "float32",
                             say={"shape": "%(who)s: %(name)s must be %(shape)s, not %(got_tuple)s"})


def _check_device_mask(who, mask, n):
    """An environment mask on the device: uint8 or bool [n] (a non-zero byte selects), or a raw device pointer."""
    dtype = "bool" if "bool" in str(getattr(mask, "dtype", "")) else "uint8"
    _check_device_buffer(who, "mask", mask, (n,), dtype, say={"dtype": "%(who)s: %(name)s must be uint8 or bool, not %(got)s"})


def check_get_state_device_args(n, nv, na, ngoal, qpos=None, qvel=None, act=None, goal=None, ep_step=None, ep_count=None):
    """The argument checks of :meth:`HipBatch.get_state_device`, without a device: raises ValueError. Every output is optional and is a
    described object (torch tensor), which is checked — ``qpos`` / ``qvel`` float32 [n, nv], ``act`` float32 [n, na], ``goal`` float32
    [n, ngoal], ``ep_step`` / ``ep_count`` int32 [n] (uint32 passes as well), contiguous, on the device — or a raw device pointer (int),
    which is taken as given. What only the library can know (no output at all, ``act`` for a model without activations) is left to it."""
    who = "get_state_device"
    for name, x, shape, dtype in (("qpos", qpos, (n, nv), "float32"), ("qvel", qvel, (n, nv), "float32"), ("act", act, (n, na), "float32"),
                                  ("goal", goal, (n, ngoal), "float32"), ("ep_step", ep_step, (n,), "int32"), ("ep_count", ep_count, (n,), "int32")):
        if x is not None and not (name == "act" and na == 0):
            _check_device_buffer(who, name, x, shape, dtype)


def check_state_device_args(n, nv, na, ngoal, nobs, qpos, qvel, act=None, goal=None, mask=None, obs=None):
    """The argument checks of :meth:`HipBatch.set_state_device`, without a device: raises ValueError. ``qpos`` and ``qvel`` are both
    needed; buffers are described objects (torch tensors), which are checked — ``qpos`` / ``qvel`` float32 [n, nv], ``act`` float32
    [n, na], ``goal`` float32 [n, ngoal], ``mask`` uint8 or bool [n], ``obs`` float32 [n, nobs], contiguous, on the device — or raw device
    pointers (ints), which are taken as given. ``act`` for a model without activations is left to the library to refuse."""
    who = "set_state_device"
    for name, x in (("qpos", qpos), ("qvel", qvel)):
        if x is None:
            raise ValueError("%s: %s is None (a state is positions and velocities)" % (who, name))
    for name, x, shape in (("qpos", qpos, (n, nv)), ("qvel", qvel, (n, nv)), ("act", act, (n, na)), ("goal", goal, (n, ngoal)), ("obs", obs, (n, nobs))):
        if x is not None and not (name == "act" and na == 0):
            _check_device_buffer(who, name, x, shape, "float32")
    if mask is not None:
        _check_device_mask(who, mask, n)


def check_restart_device_args(n, nobs, mask=None, obs=None):
    """The argument checks of :meth:`HipBatch.restart_device`, without a device: raises ValueError. ``mask`` uint8 or bool [n], ``obs``
    float32 [n, nobs] — described objects (torch tensors), which are checked, or raw device pointers (ints), which are taken as given."""
    who = "restart_device"
    if mask is not None:
        _check_device_mask(who, mask, n)
    if obs is not None:
        _check_device_buffer(who, "obs", obs, (n, nobs), "float32")


SNAPSHOT_BLOB_HEADER = 64       # bytes in front of the payload of lm_snapshot_export (include/locohip.h)


def check_restore_args(n, src=None, mask=None, snapshot=None, batch=None):
    """The argument checks of :meth:`HipBatch.restore` / :meth:`HipBatch.fork`, without a device. ``src``: None, an object with
    ``data_ptr()`` (a torch tensor: int32, [n], contiguous, on the device) or integers on the host (numpy array / list, [n]); ``mask``:
    booleans [n], sugar for ``src[e] = e if mask[e] else -1``; not both. ``snapshot`` (with ``batch``): an open snapshot of THIS batch,
    taken under the batch's present configuration. Returns ``(kind, value)``: ``("all", None)``, ``("device", tensor)``,
    ``("host", int32 array)`` — entries outside [0, n) folded to -1 — or ``("device_mask", tensor)``. Raises ValueError."""
    if snapshot is not None:
        if getattr(snapshot, "closed", False):
            raise ValueError("restore: the snapshot is closed (its batch was closed, or close() was called)")
        if batch is not None and getattr(snapshot, "batch", None) is not batch:
            raise ValueError("restore: the snapshot belongs to another batch")
        if batch is not None and tuple(snapshot.signature) != tuple(batch.snapshot_signature()):
            raise ValueError("restore: the snapshot was taken under another configuration of the batch: %s, now %s"
                             % (tuple(snapshot.signature), tuple(batch.snapshot_signature())))
    if src is not None and mask is not None:
        raise ValueError("restore: give src or mask, not both")
    if src is None and mask is None:
        return "all", None
    name, x = ("src", src) if src is not None else ("mask", mask)
    if hasattr(x, "data_ptr"):
        _check_device_buffer("restore", name, x, (n,), "int32" if src is not None else "bool",
                             say={"dtype": "%(who)s: a %(name)s tensor must be %(dtype)s, not %(got)s",
                                  "device": "%(who)s: a %(name)s tensor must live on the device (host values: a numpy array or a list)"})
        return ("device" if src is not None else "device_mask"), x
    if isinstance(x, (str, bytes)) or np.ndim(x) == 0:
        raise ValueError("restore: %s must be a sequence of %d entries, not %s" % (name, n, type(x).__name__))
    a = np.asarray(x)
    if a.shape != (n,):
        raise ValueError("restore: %s must be [%d], not %s" % (name, n, list(a.shape)))
    if src is not None:
        if a.dtype.kind not in "iu":
            raise ValueError("restore: src must hold integers, not %s" % a.dtype)
        a = a.astype(np.int64)
        return "host", np.ascontiguousarray(np.where((a < 0) | (a >= n), -1, a), dtype=np.int32)
    if a.dtype.kind != "b":
        raise ValueError("restore: mask must hold booleans, not %s" % a.dtype)
    return "host", np.ascontiguousarray(np.where(a, np.arange(n), -1), dtype=np.int32)


def _dev_ptr(x):
    """A device buffer as a C pointer: None, a raw address (int), or an object with ``data_ptr()`` such as a torch tensor."""
    if x is None:
        return None
    return C.c_void_p(int(x.data_ptr()) if hasattr(x, "data_ptr") else int(x))


def _stream_ptr(stream):
    """A raw hipStream_t (int) as a C pointer; None: the library's own stream."""
    return None if stream is None else C.c_void_p(int(stream))


class HipModel:
    def __init__(self, chain_model, device=0):
        self.device = int(device)
        lib = load_library()
        if lib.lm_device_count() <= 0:
            raise BackendError("no HIP device visible: the batched simulator needs an MI355X (no CPU fallback)")
        cm = np.ascontiguousarray(chain_model, dtype=np.float64)
        h = C.c_void_p()
        _check(lib.lm_model_create(_ptr(cm, _D), len(cm), device, C.byref(h)))
        self._h = h
        self._lib = lib                      # kept on the object: module globals are gone when __del__ runs at interpreter exit
        d = Dims()
        _check(lib.lm_model_dims(h, C.byref(d)))
        self.dims = d

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lm_model_destroy(self._h)
            self._h = None

    __del__ = close


class Snapshot:
    """The state of every environment of a :class:`HipBatch`, in device memory (``lm_snapshot_*``). Made by
    :meth:`HipBatch.snapshot`; holds a reference to its batch, whose ``close()`` closes it."""

    def __init__(self, batch, keep_collider_cache=True):
        self.batch = batch
        self._lib = batch._lib
        self._h = None
        self.keep_collider_cache = bool(keep_collider_cache)
        self.signature = batch.snapshot_signature()
        h = C.c_void_p()
        _check(self._lib.lm_snapshot_create(batch._h, 0 if keep_collider_cache else 1, C.byref(h)))
        self._h = h
        batch._snapshots.add(self)

    @property
    def closed(self):
        return self._h is None

    @property
    def nbytes(self):
        return int(self._lib.lm_snapshot_bytes(self._h)) if self._h else 0

    def save(self, stream=None, sync=True):
        """Save the batch's present state into this snapshot's storage (one kernel launch)."""
        check_restore_args(self.batch.n, snapshot=self, batch=self.batch)
        _check(self._lib.lm_snapshot_save(self.batch._h, self._h, _stream_ptr(stream), int(bool(sync))))
        return self

    def to_bytes(self):
        """The snapshot as a self-describing blob (``lm_snapshot_export``), for files; :meth:`HipBatch.snapshot_from_bytes` reads it."""
        if self.closed:
            raise ValueError("to_bytes: the snapshot is closed")
        buf = np.empty(SNAPSHOT_BLOB_HEADER + self.nbytes, dtype=np.uint8)
        _check(self._lib.lm_snapshot_export(self.batch._h, self._h, C.c_void_p(buf.ctypes.data), len(buf)))
        return buf.tobytes()

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lm_snapshot_destroy(self._h)
            self._h = None

    __del__ = close


class HipBatch:
    """A batch of ``n_envs`` lock-step environments resident on one GPU."""

    def __init__(self, model, n_envs, envs_per_workgroup=None):
        """``envs_per_workgroup``: None / 4 = the replicated layout (default), 8 or 16 = the plain layout (lm_batch_set_layout)."""
        self.model = model
        self.n = int(n_envs)
        self._lib = load_library()
        import weakref
        self._snapshots = weakref.WeakSet()
        self._fork_snapshot = self._src_keep = None
        h = C.c_void_p()
        _check(self._lib.lm_batch_create(model._h, self.n, C.byref(h)))
        self._h = h
        if envs_per_workgroup is not None:
            _check(self._lib.lm_batch_set_layout(self._h, int(envs_per_workgroup)))
        d = model.dims
        self.nq, self.nv, self.nu, self.nobs, self.ngoal = d.nq, d.nv, d.nu, d.nobs, d.ngoal
        self.na = d.na
        self._term_on, self._term_out = False, None              # terminal observations: enabled; a caller's tensor, kept alive
        self._pinned = self._pinned_term = None                  # views of the pinned ring (step_pinned)
        self._obs_norm = None                                    # the policy's input normalisation: the caller's tensors, kept alive
        self._compiler_on, self.n_variants, self.n_model_draws, self._table_sizes = False, 0, 0, None

    def close(self):
        for snap in list(getattr(self, "_snapshots", ())):      # the batch's snapshots die with it (their storage first)
            snap.close()
        self._fork_snapshot = self._src_keep = None
        if getattr(self, "_h", None):
            self._lib.lm_batch_destroy(self._h)
            self._h = None
        self._term_out = None              # a caller's terminal-observation tensor, the pinned ring's views
        self._pinned = self._pinned_term = None
        self._obs_norm = None

    __del__ = close

    def set_layout(self, envs_per_workgroup):
        """Environments per workgroup (``lm_batch_set_layout``): 4 = the replicated layout, 8 or 16 = the plain layout. A layout whose
        kernels need more LDS than a compute unit has is refused with the byte counts; the batch keeps the layout it had."""
        _check(self._lib.lm_batch_set_layout(self._h, int(envs_per_workgroup)))

    def set_replay(self, enabled):
        """Speculate / replay (``lm_batch_set_replay``): on by default; off = the regular kernels alone, contacts beyond their slots
        are dropped and counted (A/B measurements)."""
        # 2 (tests): everything through the replay kernel; 3 / 4: like 1 / 2 without the concurrent pollers (profilers)
        _check(self._lib.lm_batch_set_replay(self._h, int(enabled) if enabled in (2, 3, 4) else int(bool(enabled))))

    def replay_marks(self, reset=False):
        """Per environment: did the replay kernel run one of its control steps since the marks were last cleared?"""
        out = np.empty(self.n, dtype=np.uint8)
        _check(self._lib.lm_get_replay_marks(self._h, _ptr(out, _U8), int(bool(reset))))
        return out != 0

    def set_state(self, qpos, qvel, mask=None):
        q, v = _f32(qpos, (self.n, self.nq)), _f32(qvel, (self.n, self.nv))
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_set_state(self._h, _ptr(q), _ptr(v), mp))

    def get_state(self):
        q = np.empty((self.n, self.nq), dtype=np.float32)
        v = np.empty((self.n, self.nv), dtype=np.float32)
        _check(self._lib.lm_get_state(self._h, _ptr(q), _ptr(v)))
        return q, v

    def step_device(self, action=None, obs=None, reward=None, done=None, stream=None, sync=True):
        """One control step on DEVICE buffers: arguments are device pointers (ints) or objects with ``data_ptr()`` such as
        torch tensors — float32 action [n, nu], obs [n, nobs], reward [n], uint8 done [n]; None = zero action / library
        buffers. ``stream``: raw hipStream_t (e.g. ``torch.cuda.current_stream().cuda_stream``).

        The done byte is a bit field, NOT a boolean: bit 0 (``done & 1``) = absorbing state, what the reference's ``step()``
        returns; bit 1 (``done & 2``) = the episode ended on the device in this step (restarted from the reset table — ``obs``
        is then the first observation of the new episode — or, without auto-reset, the step that reached the horizon).
        ``done.bool()`` mixes truncation and restarts into the terminal flag; mask the bits."""
        _check(self._lib.lm_step_device(self._h, _dev_ptr(action), _dev_ptr(obs), _dev_ptr(reward), _dev_ptr(done),
                                        _stream_ptr(stream), int(bool(sync))))

    def get_state_device(self, qpos=None, qvel=None, act=None, goal=None, ep_step=None, ep_count=None, stream=None, sync=True):
        """The state of every environment into DEVICE buffers, one launch (``ls_get_state_device``): ``qpos`` / ``qvel`` float32
        [n, nv], ``act`` float32 [n, na], ``goal`` float32 [n, ngoal], ``ep_step`` int32 [n], ``ep_count`` int32 / uint32 [n] — torch
        tensors or raw device pointers, each optional, not all None. ``stream`` / ``sync`` as in :meth:`step_device`: queued behind
        whatever the batch has in flight; ``sync=False`` waits for nothing."""
        check_get_state_device_args(self.n, self.nv, self.na, self.ngoal, qpos, qvel, act, goal, ep_step, ep_count)
        _check(self._lib.ls_get_state_device(self._h, _dev_ptr(qpos), _dev_ptr(qvel), _dev_ptr(act), _dev_ptr(goal), _dev_ptr(ep_step),
                                             _dev_ptr(ep_count), _stream_ptr(stream), int(bool(sync))))

    def set_state_device(self, qpos, qvel, act=None, goal=None, mask=None, obs=None, stream=None, sync=True):
        """:meth:`set_state` from DEVICE rows, one launch (``ls_set_state_device``): for every environment whose ``mask`` byte (uint8 or
        bool [n]; None: all) is non-zero, ``qpos`` / ``qvel`` float32 [n, nv] are written, warm start, self-collision slack and the
        episode's step are cleared and the activations zeroed — or set from ``act`` [n, na]; ``goal`` [n, ngoal] sets the goal. The
        observation of the new state is written for those environments into ``obs`` float32 [n, nobs] (the kernel's column order,
        foot-force columns 0), or into the batch's own last-step row when None, so ``rollout_policy(obs0=None)`` is valid afterwards.
        The episode count, the flags and the reward / done rows stay. ``stream`` / ``sync`` as in :meth:`step_device`."""
        check_state_device_args(self.n, self.nv, self.na, self.ngoal, self.nobs, qpos, qvel, act, goal, mask, obs)
        _check(self._lib.ls_set_state_device(self._h, _dev_ptr(qpos), _dev_ptr(qvel), _dev_ptr(act), _dev_ptr(goal), _dev_ptr(mask),
                                             _dev_ptr(obs), _stream_ptr(stream), int(bool(sync))))

    def restart_device(self, mask=None, obs=None, stream=None, sync=True):
        """Restart the masked environments (uint8 or bool [n] on the device; None: all) exactly as the step kernel restarts an episode
        that ended (``ls_restart_device``): the episode count advances, the reset-table row is the one drawn from (seed, global
        environment id, episode count), state and goal come from it, the model variant / the compiler's model and the randomised
        joint parameters are redrawn. Needs :meth:`set_reset_table`; :meth:`set_auto_reset` need not be on. ``obs`` as in
        :meth:`set_state_device`. Not touched: the collider's cache, the flags, the reward / done rows, the count of control steps,
        the statistics. ``stream`` / ``sync`` as in :meth:`step_device`."""
        check_restart_device_args(self.n, self.nobs, mask, obs)
        _check(self._lib.ls_restart_device(self._h, _dev_ptr(mask), _dev_ptr(obs), _stream_ptr(stream), int(bool(sync))))

    def set_dof_params(self, damping=None, stiffness=None, frictionloss=None, mask=None):
        """Per-environment joint parameters [n, nv] (domain randomisation); None leaves a parameter as it is."""
        arrs = [None if x is None else _f32(x, (self.n, self.nv)) for x in (damping, stiffness, frictionloss)]
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_set_dof_params(self._h, *[None if x is None else _ptr(x) for x in arrs], mp))

    def get_dof_params(self):
        out = [np.empty((self.n, self.nv), dtype=np.float32) for _ in range(3)]
        _check(self._lib.lm_get_dof_params(self._h, *[_ptr(x) for x in out]))
        return dict(damping=out[0], stiffness=out[1], frictionloss=out[2])

    def set_dof_randomization(self, spec):
        """Device-side redraw rule at episode restarts: spec[3, nv, 3] = (kind, a, b); None disables."""
        if spec is None:
            _check(self._lib.lm_set_dof_randomization(self._h, None))
            return
        s = _f32(spec, (3, self.nv, 3))
        _check(self._lib.lm_set_dof_randomization(self._h, _ptr(s)))

    def set_model_variants(self, tables):
        """``tables``: list of (record, geom table, geom-pair table) from ``lowering.variant_tables`` — the pool of randomised
        models of this batch (None / empty removes it). Every environment starts on variant 0; a device-side restart redraws."""
        if not tables:
            _check(self._lib.lm_set_model_variants(self._h, None, None, None, 0, 0))
            self.n_variants = 0
            self._compiler_on = False
            return
        rec = np.ascontiguousarray(np.stack([t[0] for t in tables]), dtype=np.float32)
        gt = np.ascontiguousarray(np.stack([t[1] for t in tables]), dtype=np.float32)
        npair = len(tables[0][2])
        gpt = np.ascontiguousarray(np.stack([t[2] for t in tables]), dtype=np.float32) if npair else None
        _check(self._lib.lm_set_model_variants(self._h, _ptr(rec), _ptr(gt), _ptr(gpt) if gpt is not None else None, npair, len(tables)))
        self.n_variants = len(tables)
        self._compiler_on = False

    def set_model_compiler(self, program, nominal_tables, seed=0):
        """The model compiler on the device: ``program`` = (int32, float64) of ``lowering.model_compiler_tables``, ``nominal_tables`` =
        ``lowering.variant_tables(nominal, nominal)``. Every environment gets a slot and a freshly drawn model of its own, now and at
        every device-side restart; :meth:`compile_models` is the host-side reset."""
        ib = np.ascontiguousarray(program[0], dtype=np.int32)
        db = np.ascontiguousarray(program[1], dtype=np.float64)
        # the library checks the program's sizes and where its gather / contact ops write; what its draws and drawn bodies index is
        # checked here (the kernel's tables in LDS are sized by the header's counts)
        if len(ib) < 16:
            raise BackendError("model-compiler program: header missing")
        nv, nrb, ngs, nd, nslot, nbody = int(ib[1]), int(ib[2]), int(ib[3]), int(ib[4]), int(ib[5]), int(ib[8])
        if len(ib) < 16 + 4 * nd + 4 * nrb:
            raise BackendError("model-compiler program: draw / body tables cut short")
        draws = ib[16:16 + 4 * nd].reshape(nd, 4)
        rb = ib[16 + 4 * nd:16 + 4 * nd + 4 * nrb].reshape(nrb, 4)
        limit = {0: (nv, 1), 1: (nrb, 1), 2: (nrb, 3), 3: (nrb, 3), 4: (ngs, 3)}
        for kind, target, idx, comp in draws:
            if kind not in (1, 2, 3) or target not in limit or not (0 <= idx < limit[int(target)][0] and 0 <= comp < limit[int(target)][1]):
                raise BackendError("model-compiler program: a draw outside its table (kind %d target %d index %d component %d)" % (kind, target, idx, comp))
        for body, kind, slot, has_sv in rb:
            if not (0 < body < nbody and kind in (1, 2) and 0 <= slot < nslot and has_sv in (0, 1)):
                raise BackendError("model-compiler program: a drawn body outside the model (body %d kind %d slot %d)" % (body, kind, slot))
        rec, gt = _f32(nominal_tables[0], (len(nominal_tables[0]),)), _f32(nominal_tables[1], (len(nominal_tables[1]),))
        npair = len(nominal_tables[2])
        gpt = _f32(nominal_tables[2], (npair,)) if npair else None
        _check(self._lib.lm_set_model_compiler(self._h, _ptr(ib, _I32), len(ib), _ptr(db, _D),
                                               len(db), _ptr(rec), _ptr(gt), _ptr(gpt) if gpt is not None else None, npair, int(seed) & (2 ** 64 - 1)))
        self.n_variants = self.n
        self._compiler_on = True
        self.n_model_draws = int(ib[4])
        self._table_sizes = (len(rec), len(gt), npair)

    def compile_models(self, mask=None):
        """A fresh model for the masked environments (None: all), drawn and compiled on the device."""
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_compile_models(self._h, mp))

    def get_model_draws(self):
        """(draws [n, n_draw] float64 of every environment's CURRENT model, models each environment has had [n])."""
        d = np.empty((self.n, self.n_model_draws), dtype=np.float64)
        g = np.empty(self.n, dtype=np.uint32)
        _check(self._lib.lm_get_model_draws(self._h, _ptr(d, _D), _ptr(g, C.POINTER(C.c_uint32))))
        return d, g

    def get_model_tables(self, env, sizes=None):
        """(record, geom table, geom-pair table) environment ``env`` runs on."""
        nr, ng, npair = sizes if sizes is not None else self._table_sizes
        rec, gt, gpt = np.empty(nr, dtype=np.float32), np.empty(ng, dtype=np.float32), np.empty(npair, dtype=np.float32)
        _check(self._lib.lm_get_model_tables(self._h, int(env), _ptr(rec), _ptr(gt), _ptr(gpt) if npair else None))
        return rec, gt, gpt

    def set_variant_index(self, index, mask=None):
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(index, dtype=np.int32), (self.n,)))
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_set_variant_index(self._h, _ptr(idx, _I32), mp))

    def set_variant_rows(self, rows_per_variant):
        """The reset table is n_variants blocks of ``rows_per_variant`` rows: a device-side restart from row i puts the environment
        on variant i // rows_per_variant (0: variants are redrawn independently of the row)."""
        _check(self._lib.lm_set_variant_rows(self._h, int(rows_per_variant)))

    def get_variant_index(self):
        idx = np.zeros(self.n, dtype=np.int32)
        _check(self._lib.lm_get_variant_index(self._h, _ptr(idx, _I32)))
        return idx

    def set_activation(self, act, mask=None):
        """Muscle activations [n, na] (set_state zeroes them like mj_resetData; this is for checkpoints and tests)."""
        a = _f32(act, (self.n, self.na))
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_set_activation(self._h, _ptr(a), mp))

    def get_activation(self):
        a = np.empty((self.n, self.na), dtype=np.float32)
        _check(self._lib.lm_get_activation(self._h, _ptr(a)))
        return a

    def set_goal(self, goal, mask=None):
        if self.ngoal == 0:
            return
        g = _f32(goal, (self.n, self.ngoal))
        keep, mp = _mask(mask, self.n)
        _check(self._lib.lm_set_goal(self._h, _ptr(g), mp))

    def step(self, action):
        a = _f32(action, (self.n, self.nu))
        obs = np.empty((self.n, self.nobs), dtype=np.float32)
        rew = np.empty(self.n, dtype=np.float32)
        done = np.empty(self.n, dtype=np.uint8)
        _check(self._lib.lm_step(self._h, _ptr(a), _ptr(obs), _ptr(rew), _ptr(done, _U8)))
        # done byte: bit 0 = absorbing state, bit 1 = the device ended the episode in this step (restarted it from the
        # reset table, or the horizon was reached)
        self.last_restarted = (done & 2) != 0
        return obs, rew, (done & 1) != 0

    def set_active(self, env_ids):
        """Run only the listed environments from now on (``lm_batch_set_active``); None: all of them again."""
        if env_ids is None:
            _check(self._lib.lm_batch_set_active(self._h, None, 0))
            return
        ids = np.ascontiguousarray(env_ids, dtype=np.int32).reshape(-1)
        _check(self._lib.lm_batch_set_active(self._h, _ptr(ids, _I32), len(ids)))

    PINNED_SLOTS = 4

    def set_obs_order(self, perm):
        """Column order of the float64 observation of step_pinned (None: the kernel's own)."""
        if perm is None:
            _check(self._lib.lm_set_obs_order(self._h, None, 0))
        else:
            p = np.ascontiguousarray(perm, dtype=np.int32)
            _check(self._lib.lm_set_obs_order(self._h, _ptr(p, _I32), len(p)))

    def _pinned_views(self):
        views = []
        for slot in range(self.PINNED_SLOTS):
            o, r, d = _D(), _D(), _U8()
            _check(self._lib.lm_pinned_slot(self._h, slot, C.byref(o), C.byref(r), C.byref(d)))
            arrs = []
            for ptr, ct, dt, shape in ((o, C.c_double, np.float64, (self.n, self.nobs)), (r, C.c_double, np.float64, (self.n,)), (d, C.c_uint8, np.uint8, (self.n,))):
                buf = (ct * int(np.prod(shape))).from_address(C.addressof(ptr.contents))
                buf._owner = self          # a view handed to the caller keeps the batch (and with it the pinned memory) alive
                arrs.append(np.frombuffer(buf, dtype=dt).reshape(shape))
            views.append(tuple(arrs))
        return views

    def step_pinned(self, action64):
        """One control step through the library's float64 host surface (lm_step_pinned): ``action64`` is a C-contiguous float64
        array [n, nu]; returns (obs float64 [n, nobs], reward float64 [n], absorbing bool [n]). obs and reward are VIEWS of a ring of
        PINNED_SLOTS pinned result sets owned by the batch: what a call returned stays intact for the next PINNED_SLOTS - 1 calls.
        With terminal observations enabled a fourth view follows: float64 [n, nobs] in the order of set_obs_order, whose rows with
        ``last_restarted`` set hold this step's terminal observation (the other rows: whatever the slot held)."""
        if self._pinned is None:
            self._pinned = self._pinned_views()
            self._slot = -1
        self._slot = (self._slot + 1) % self.PINNED_SLOTS
        _check(self._lib.lm_step_pinned(self._h, _ptr(action64, _D), self._slot))
        obs, rew, done = self._pinned[self._slot]
        self.last_restarted = (done & 2) != 0
        if self._term_on:
            if self._pinned_term is None:
                self._pinned_term = self._pinned_term_views()
            return obs, rew, (done & 1) != 0, self._pinned_term[self._slot]
        return obs, rew, (done & 1) != 0

    def enable_terminal_obs(self, out=None):
        """Terminal observations (``lm_set_terminal_obs``): a step that ends an episode on the device (done byte, bit 1) writes the
        observation of the state it reached — not the restarted episode's first — into row e of a float32 buffer [n, nobs].
        ``out`` None: a zero-filled buffer owned by the batch, read with :meth:`terminal_obs`; otherwise a device pointer (int) or a
        torch tensor [n, nobs], float32, contiguous, which the batch keeps alive until :meth:`disable_terminal_obs` / :meth:`close`."""
        check_terminal_obs_args(self.n, self.nobs, out)
        _check(self._lib.lm_set_terminal_obs(self._h, 1, _dev_ptr(out)))
        self._term_out = out
        self._term_on = True

    def disable_terminal_obs(self):
        _check(self._lib.lm_set_terminal_obs(self._h, 0, None))
        self._term_out = None
        self._term_on = False

    def terminal_obs(self):
        """The terminal-observation buffer as a host float32 array [n, nobs] (the kernel's column order), after the last step."""
        out = np.empty((self.n, self.nobs), dtype=np.float32)
        _check(self._lib.lm_get_terminal_obs(self._h, _ptr(out)))
        return out

    def _pinned_term_views(self):
        views = []
        for slot in range(self.PINNED_SLOTS):
            t = _D()
            _check(self._lib.lm_pinned_terminal_obs(self._h, slot, C.byref(t)))
            buf = (C.c_double * (self.n * self.nobs)).from_address(C.addressof(t.contents))
            buf._owner = self
            views.append(np.frombuffer(buf, dtype=np.float64).reshape(self.n, self.nobs))
        return views

    def set_reset_table(self, rows, seed=0, global_env_offset=0):
        r = _f32(rows)
        assert r.ndim == 2 and r.shape[1] == self.nq + self.nv + self.ngoal
        _check(self._lib.lm_set_reset_table(self._h, _ptr(r), r.shape[0], int(seed), int(global_env_offset)))

    def set_auto_reset(self, enabled, horizon=0):
        _check(self._lib.lm_set_auto_reset(self._h, int(bool(enabled)), int(horizon)))

    def rollout(self, n_steps, action_mode=0, seed=0, steps_per_launch=1):
        """n_steps control steps on the device with zero (0) or uniform random (1) actions. steps_per_launch > 1 fuses that
        many control steps into one launch (same results, no device-wide join between control steps)."""
        st = Stats()
        _check(self._lib.lm_rollout_fused(self._h, int(n_steps), int(steps_per_launch), int(action_mode), int(seed), C.byref(st)))
        return st.as_dict()

    def rollout_tape(self, actions, obs=None, reward=None, done=None, terminal=None, steps_per_launch=None, repeat=None, stream=None,
                     sync=True, n_steps=None):
        """T control steps under GIVEN actions, ``steps_per_launch`` (default: T) of them per kernel launch, every step recorded
        (``lm_rollout_tape``). Buffers are torch tensors or raw device pointers, as in :meth:`step_device`: ``actions`` float32
        [T, n, nu] — or [n, nu] with ``repeat=T``, the same action T times — and, each optional, ``obs`` float32 [T, n, nobs],
        ``reward`` float32 [T, n], ``done`` uint8 [T, n] (the bit field of :meth:`step_device`) and ``terminal`` float32 [T, n, nobs]
        (needs :meth:`enable_terminal_obs`; row [t, e] is written where ``done[t, e] & 2``, the others are left as they were).
        Bitwise what T calls of ``step_device`` produce. Returns the statistics (``sync=True``) or None."""
        T, stride, spl = check_tape_args(self.n, self.nu, self.nobs, actions, obs, reward, done, terminal, steps_per_launch, repeat, n_steps,
                                         terminal_enabled=self._term_on)
        st = Stats()
        _check(self._lib.lm_rollout_tape(self._h, T, spl, _dev_ptr(actions), stride, _dev_ptr(obs), _dev_ptr(reward), _dev_ptr(done), _dev_ptr(terminal),
                                         _stream_ptr(stream), int(bool(sync)), C.byref(st) if sync else None))
        return st.as_dict() if sync else None

    def rollout_policy(self, policy, n_steps, obs0=None, actions=None, obs=None, reward=None, done=None, terminal=None,
                       steps_per_launch=None, noise_seed=0, stream=None, sync=True):
        """``n_steps`` control steps in closed loop under an :class:`MlpPolicy`, evaluated on the device at the top of every step from
        the observation the step before wrote (``lm_rollout_policy``). ``obs0`` float32 [n, nobs]: what the FIRST action is computed
        from, in the kernel's column order (what :meth:`step_device` writes); None = the batch's own last-step row, valid after any
        step but not after :meth:`set_state`. ``actions`` float32 [T, n, nu] receives every step's action (the raw one, before the
        actuator's clamp) and is allocated when not given (needs a policy of torch tensors); ``obs`` / ``reward`` / ``done`` /
        ``terminal``, ``steps_per_launch``, ``stream`` and ``sync`` as in :meth:`rollout_tape`. With ``policy.log_std`` the action is
        mean + exp(log_std) * z, z keyed by (``noise_seed``, global environment id, the batch's step count, output index). Feeding the
        returned tape to :meth:`rollout_tape` repeats the rollout bit for bit. Returns the action tape; the statistics of a
        synchronous call are in ``self.last_policy_stats``."""
        T, spl = check_policy_args(self.n, self.nu, self.nobs, policy, n_steps, obs0, actions, obs, reward, done, terminal, steps_per_launch,
                                   terminal_enabled=self._term_on)
        if actions is None:
            import torch
            actions = torch.empty((T, self.n, self.nu), dtype=torch.float32, device=policy.params.device)
        st, ps = Stats(), policy.struct()
        _check(self._lib.lm_rollout_policy(self._h, C.byref(ps), T, spl, int(noise_seed) & 0xFFFFFFFFFFFFFFFF, _dev_ptr(obs0), _dev_ptr(actions),
                                           _dev_ptr(obs), _dev_ptr(reward), _dev_ptr(done), _dev_ptr(terminal),
                                           _stream_ptr(stream), int(bool(sync)), C.byref(st) if sync else None))
        self.last_policy_stats = st.as_dict() if sync else None
        return actions

    def set_policy_obs_norm(self, mean=None, inv_std=None, clip=0.0):
        """Input normalisation of the policy of :meth:`rollout_policy` (``lm_set_policy_obs_norm``): the MLP reads
        ``((obs - mean) * inv_std).clamp(-clip, clip)`` (``clip`` 0: no clamp) in place of the raw observation row. ``mean`` /
        ``inv_std``: float32 device tensors [nobs] in the kernel's column order, read in place at every evaluation — an in-place update
        (:meth:`ObsNorm.update`) is seen by the next call; the batch keeps references to them. Both None: off (the default). The
        observation, terminal and action tapes are not affected: only what the policy reads. A setting, not part of a snapshot."""
        clip = check_obs_norm_args(self.nobs, mean, inv_std, clip)
        _check(self._lib.lm_set_policy_obs_norm(self._h, _dev_ptr(mean), _dev_ptr(inv_std), clip))
        self._obs_norm = (mean, inv_std)

    def gae(self, reward, done, value, last_value, term_value=None, gamma=0.99, lam=0.95, adv=None, ret=None, stream=None, sync=True,
            n_steps=None):
        """Generalised advantage estimation over the tapes of :meth:`rollout_tape` / :meth:`rollout_policy` in one launch
        (``lm_tape_gae``), the done byte's bits told apart: no bootstrap at an absorbing state (``done & 1``), a bootstrap from
        ``term_value[t, e]`` = V(terminal tape row) at a truncation (``done == 2``; None: 0), the trace cut at every restart.
        ``reward`` / ``value`` float32 [T, n], ``done`` uint8 [T, n], ``last_value`` float32 [n] = V(obs[T-1]); ``value[t]`` = V of the
        observation step t's action was computed from (obs0, then obs[t-1]). ``adv`` / ``ret`` float32 [T, n] are allocated with torch
        when not given. ``stream`` / ``sync`` as in :meth:`rollout_tape`: queued behind the rollout that fills the tapes. Returns
        ``(adv, ret)``."""
        T, gamma, lam = check_gae_args(self.n, reward, done, value, last_value, term_value, gamma, lam, adv, ret, n_steps)
        if adv is None or ret is None:
            import torch
            if not hasattr(value, "device"):
                raise ValueError("gae: adv and ret can only be allocated beside a value tensor; pass both with raw pointers")
            adv = torch.empty((T, self.n), dtype=torch.float32, device=value.device) if adv is None else adv
            ret = torch.empty((T, self.n), dtype=torch.float32, device=value.device) if ret is None else ret
        _check(self._lib.lm_tape_gae(self._h, T, _dev_ptr(reward), _dev_ptr(done), _dev_ptr(value), _dev_ptr(last_value), _dev_ptr(term_value),
                                     gamma, lam, _dev_ptr(adv), _dev_ptr(ret), _stream_ptr(stream), int(bool(sync))))
        return adv, ret

    # ---- snapshots (include/locohip.h lm_snapshot_*)
    def snapshot_signature(self):
        """What a snapshot must agree on with the batch, as far as this layer knows it (the library compares its own, fuller list —
        the joint-parameter arrays and the collider cache among it — and refuses with the field's name)."""
        compiler = self.n_model_draws if self._compiler_on else 0
        return (self.n, self.nv, self.na, self.nobs, int(self.n_variants), int(compiler))

    def snapshot(self, keep_collider_cache=True, stream=None, sync=True):
        """Save the state of every environment on the device and return the :class:`Snapshot`: everything a later control step reads,
        so that :meth:`restore` continues bit for bit. ``keep_collider_cache=False`` leaves the convex collider's warm-start cache out
        (88 KB per HumanoidTorque environment); only the default is promised bitwise."""
        return Snapshot(self, keep_collider_cache).save(stream=stream, sync=sync)

    def restore(self, snap, src=None, stream=None, sync=True, mask=None):
        """Put the batch back to ``snap``. ``src`` None: every environment takes its own saved state, and the count of control steps
        is rewound. Otherwise environment e takes the saved state of environment ``src[e]`` — an int32 CUDA tensor [n] (nothing is
        copied, nothing waits with ``sync=False``), or a numpy array / list of ints, which is uploaded; entries outside [0, n) mean
        "keep what it has". ``mask`` (booleans [n]) is sugar for ``src[e] = e if mask[e] else -1``.
        A forked environment copies its source's episode step and episode count, but random numbers stay keyed by the environment's
        own id: it equals its source until one of them restarts on the device."""
        kind, val = check_restore_args(self.n, src, mask, snapshot=snap, batch=self)
        ptr = None
        if kind != "all":
            import torch
            if kind == "host":
                val = torch.from_numpy(val).to(torch.device("cuda", self.model.device))      # (blocking: on the device when it returns)
            elif kind == "device_mask":
                ids = torch.arange(self.n, dtype=torch.int32, device=val.device)
                val = torch.where(val, ids, torch.full_like(ids, -1))
                if stream is None or int(stream) != int(torch.cuda.current_stream(val.device).cuda_stream):
                    torch.cuda.current_stream(val.device).synchronize()                          # made on torch's stream, read on another
            self._src_keep = val          # alive until the next restore: with sync=False the copy may still be queued
            ptr = C.c_void_p(int(val.data_ptr()))
        _check(self._lib.lm_snapshot_restore(self._h, snap._h, ptr, _stream_ptr(stream), int(bool(sync))))

    def fork(self, src=None, stream=None, sync=True, mask=None):
        """Environment e continues from the PRESENT state of environment ``src[e]``: a save into a scratch snapshot owned by the batch,
        then :meth:`restore` with ``src`` (same forms, same ``mask``)."""
        check_restore_args(self.n, src, mask)
        snap = self._fork_snapshot
        if snap is None or snap.closed or tuple(snap.signature) != tuple(self.snapshot_signature()):
            if snap is not None:
                snap.close()
            snap = self._fork_snapshot = Snapshot(self)
        try:
            snap.save(stream=stream, sync=False)
        except BackendError:
            # the library's configuration changed where this layer does not see it (joint parameters allocated since): a fresh scratch
            snap.close()
            snap = self._fork_snapshot = Snapshot(self)
            snap.save(stream=stream, sync=False)
        self.restore(snap, src=src, stream=stream, sync=sync, mask=mask)

    def snapshot_from_bytes(self, blob):
        """A :class:`Snapshot` of THIS batch filled from ``Snapshot.to_bytes()`` of a batch of the same configuration. A blob that is
        cut short, foreign or of another configuration is refused (BackendError) and nothing changes."""
        buf = np.frombuffer(bytes(blob), dtype=np.uint8)
        keep = True
        if len(buf) >= SNAPSHOT_BLOB_HEADER:
            keep = not (int(np.frombuffer(buf[48:52].tobytes(), dtype=np.int32)[0]) & 1)      # the header's flags word
        snap = Snapshot(self, keep_collider_cache=keep)
        try:
            _check(self._lib.lm_snapshot_import(self._h, snap._h, C.c_void_p(buf.ctypes.data), len(buf)))
        except BackendError:
            snap.close()
            raise
        return snap

    def forward_debug(self, action):
        a = _f32(action, (self.n, self.nu))
        nv = self.nv
        res = dict(M=np.zeros((self.n, nv, nv), np.float32), qfrc_bias=np.zeros((self.n, nv), np.float32),
                   qfrc_smooth=np.zeros((self.n, nv), np.float32), qacc_smooth=np.zeros((self.n, nv), np.float32),
                   qacc=np.zeros((self.n, nv), np.float32), qfrc_constraint=np.zeros((self.n, nv), np.float32))
        ncon = np.zeros(self.n, np.int32)
        it = np.zeros(self.n, np.int32)
        out = ForwardOut()
        for k, arr in res.items():
            setattr(out, k, _ptr(arr))
        out.ncon = _ptr(ncon, C.POINTER(C.c_int))
        out.solver_iter = _ptr(it, C.POINTER(C.c_int))
        _check(self._lib.lm_forward_debug(self._h, _ptr(a), C.byref(out)))
        res["ncon"], res["solver_iter"] = ncon, it
        return res

    def stats(self, reset=False):
        st = Stats()
        _check(self._lib.lm_get_stats(self._h, C.byref(st), int(reset)))
        return st.as_dict()

    def flags(self):
        """Validity flags of the last control step per environment (``lm_get_flags``): 1 dropped contact, 2 self pair without a
        collider in reach, 4 collider-less geom at the floor."""
        out = np.empty(self.n, dtype=np.uint8)
        _check(self._lib.lm_get_flags(self._h, _ptr(out, _U8)))
        return out

    def sync(self):
        _check(self._lib.lm_sync(self._h))
