"""
The vector environment on device tensors: :class:`LocoVectorEnv`, Gymnasium's ``VectorEnv`` contract (SAME_STEP autoreset) over
:meth:`HipBatch.step_device`, and the ctypes loader of ``liblocovec.so`` (C-ABI: ``include/locovec.h``) — the bookkeeping of a control
step as ONE launch behind the step kernel: the done byte taken apart into ``terminated`` / ``truncated``, the observation every finished
episode ended in, running returns and lengths. The library reads what a step wrote: no batch, no model. There is no torch fallback: if
the library is missing this module raises.

Out of scope: NEXT_STEP autoreset; observation / reward normalisation wrappers (:class:`backend.ObsNorm` stays the per-rollout tool);
partial HOST resets (``reset()`` restarts every environment on the host; ``reset(options={"reset_mask": m})`` restarts chosen ones on the
device, from the reset table).
"""

import ctypes as C
import os

import numpy as np

from .backend import BackendError, _check_device_buffer, _dev_ptr, _stream_ptr
from .environments.base import LocoEnv
from .environments.gymnasium import GymnasiumWrapper, _gym, _spaces

_HERE = os.path.dirname(os.path.abspath(__file__))
VEC_LIB_PATH = os.path.join(_HERE, "csrc", "liblocovec.so")

# THE prototypes of include/locovec.h, stated once: name -> (restype, argtypes), as backend._PROTOTYPES
_P, _I, _LL = C.c_void_p, C.c_int, C.c_longlong
_PROTOTYPES = {
    "lv_last_error": (C.c_char_p, None),
    "lv_finish_step": (_I, [_LL, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I]),
}
VEC_EXPORTS = list(_PROTOTYPES)

_lib = None


def load_vec_library():
    """Load liblocovec.so and declare its prototypes. Raises BackendError if it is not built. (With torch in the process, import
    torch first: whichever HIP runtime is loaded first serves both.)"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(VEC_LIB_PATH):
        raise BackendError("vector library not built: %s is missing (run `python -c 'import __graft_entry__ as g; g.build()'` or "
                           "`make -C loco_mujoco_amd/csrc liblocovec.so`). There is no torch fallback." % VEC_LIB_PATH)
    lib = C.CDLL(VEC_LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise BackendError("liblocovec: %s (code %d)" % (load_vec_library().lv_last_error().decode(), rc))


def _same_buffer(a, b):
    """The same object, or the same raw address (two described tensors at one address are left to the C check)."""
    if a is None or b is None:
        return False
    return a is b or (not hasattr(a, "data_ptr") and not hasattr(b, "data_ptr") and int(a) == int(b))


def check_finish_args(n, nobs, obs, reward, done, terminated, truncated, term=None, final_obs=None, run_return=None, run_length=None,
                      ep_return=None, ep_length=None):
    """The argument checks of ``lv_finish_step``, without a device: returns ``(n, nobs)`` or raises ValueError. Buffers are described
    objects (torch tensors), which are checked — ``obs`` / ``term`` / ``final_obs`` float32 [n, nobs], ``reward`` / ``run_return`` /
    ``ep_return`` float32 [n], ``done`` / ``terminated`` / ``truncated`` uint8 [n], ``run_length`` / ``ep_length`` int32 [n] — or raw
    device pointers (ints), which are taken as given."""
    who = "finish_step"
    for name, v in (("n_envs", n), ("nobs", nobs)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
            raise ValueError("%s: %s must be an integer >= 1, not %r" % (who, name, v))
    n, nobs = int(n), int(nobs)
    for name, x in (("obs", obs), ("reward", reward), ("done", done), ("terminated", terminated), ("truncated", truncated)):
        if x is None:
            raise ValueError("%s: %s is None" % (who, name))
    if (run_return is None) != (run_length is None):
        raise ValueError("%s: run_return and run_length are given together or not at all" % who)
    for name, x in (("ep_return", ep_return), ("ep_length", ep_length)):
        if x is not None and run_return is None:
            raise ValueError("%s: %s needs the accumulators run_return and run_length" % (who, name))
    for name, x in (("obs", obs), ("term", term)):
        if _same_buffer(final_obs, x):
            raise ValueError("%s: final_obs must not be %s" % (who, name))
    for name, x, shape, dtype in (("obs", obs, (n, nobs), "float32"), ("reward", reward, (n,), "float32"), ("done", done, (n,), "uint8"),
                                  ("term", term, (n, nobs), "float32"), ("terminated", terminated, (n,), "uint8"),
                                  ("truncated", truncated, (n,), "uint8"), ("final_obs", final_obs, (n, nobs), "float32"),
                                  ("run_return", run_return, (n,), "float32"), ("run_length", run_length, (n,), "int32"),
                                  ("ep_return", ep_return, (n,), "float32"), ("ep_length", ep_length, (n,), "int32")):
        if x is not None:
            _check_device_buffer(who, name, x, shape, dtype)
    return n, nobs


def finish_step(n, nobs, obs, reward, done, terminated, truncated, term=None, final_obs=None, run_return=None, run_length=None,
                ep_return=None, ep_length=None, stream=None, sync=True):
    """``lv_finish_step`` on checked arguments (:func:`check_finish_args`). ``stream``: a raw hipStream_t (None: the device's null
    stream), ``sync`` as in :meth:`EpisodeMeter.update`. The launch goes to the calling thread's current device."""
    n, nobs = check_finish_args(n, nobs, obs, reward, done, terminated, truncated, term, final_obs, run_return, run_length, ep_return,
                                ep_length)
    p = _dev_ptr
    _check(load_vec_library().lv_finish_step(n, nobs, p(obs), p(reward), p(done), p(term), p(terminated), p(truncated), p(final_obs),
                                             p(run_return), p(run_length), p(ep_return), p(ep_length), _stream_ptr(stream), int(bool(sync))))


def _vector_env_refusal(env):
    """Why :class:`LocoVectorEnv` cannot serve this environment (a reason), or None."""
    if env._blocks or env._grouped:
        return ("several models in one batch (block / grouped batches) step one device batch per model, with host work between them: "
                "there is no single step launch to queue behind — use LocoEnv.step()")
    if env._reward_device_spec() is None:
        return ("the reward is evaluated on the host after every step (custom functor / foot-force columns): a step cannot stay on "
                "the device — use LocoEnv.step()")
    return None


if _gym is not None:                    # pragma: no cover - depends on the installation
    _VectorEnv = _gym.vector.VectorEnv
    try:
        SAME_STEP = _gym.vector.AutoresetMode.SAME_STEP
    except AttributeError:
        SAME_STEP = "SameStep"
else:
    SAME_STEP = "SameStep"

    class _VectorEnv:                   # minimal stand-in for gymnasium.vector.VectorEnv
        metadata = {}


class _ResultSet:
    """One set of a step's results on the device."""

    def __init__(self, torch, n, nobs, dev):
        f32 = dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.obs, self.reward = torch.zeros((n, nobs), **f32), torch.zeros(n, **f32)
        self.done, self.terminated, self.truncated = torch.zeros(n, **u8), torch.zeros(n, **u8), torch.zeros(n, **u8)
        self.final_obs, self.ended = torch.zeros((n, nobs), **f32), torch.zeros(n, dtype=torch.bool, device=dev)
        self.ep_return, self.ep_length = torch.zeros(n, **f32), torch.zeros(n, dtype=torch.int32, device=dev)
        self.terminated_b, self.truncated_b = self.terminated.view(torch.bool), self.truncated.view(torch.bool)


class LocoVectorEnv(_VectorEnv):
    """``num_envs`` lock-step environments of one task behind Gymnasium's ``VectorEnv`` contract, on torch DEVICE tensors and in
    SAME_STEP autoreset mode: an environment whose episode ends in a step restarts inside the step kernel; ``obs`` is then the first
    observation of its new episode and ``info["final_obs"]`` the one the old episode ended in.

    ``step(actions)`` queues two launches on torch's current stream and waits for nothing: the step kernel
    (:meth:`HipBatch.step_device`) and ``lv_finish_step`` behind it. ``actions``: float32 device tensor [num_envs, nu], the reference's
    normalised action (what ``LocoEnv.step`` takes). Returns ``obs`` float32 [n, nobs] in the reference's column order, ``reward``
    float32 [n], ``terminated`` / ``truncated`` bool [n] (absorbing state / ended otherwise: horizon) and ``info``: ``final_obs``
    [n, nobs], meaningful where ``_final_obs`` (bool [n], ``terminated | truncated``) — the other rows hold earlier episode ends or
    zeros; ``episode``: ``{"r": float32 [n], "l": int32 [n]}``, return and length of the episodes that ended in this step, 0
    elsewhere, with ``_episode`` the same mask. Returns are summed in float32 in step order.

    The tensors returned are VIEWS of a ring of two result sets: what a step returned stays intact through the next ``step()`` — so
    ``(obs, next_obs)`` pairs are valid — and is overwritten by the one after it. A partial reset (``reset(options={"reset_mask": m})``) is the exception: it replaces the
    masked rows of the ``obs`` the last ``step()`` returned IN PLACE, so a caller that still needs that tensor as the successor of a
    transition clones it first. ``copy=True`` returns clones.

    ``seed`` keys the device-side restart draws, ``horizon`` (None: the task's) truncates episodes; ``make_kwargs`` go to
    ``LocoEnv.make``. Refused, with the reason: several models in one batch, a reward evaluated on the host, ``num_envs < 1``."""

    metadata = {"render_modes": [], "autoreset_mode": SAME_STEP}

    def __init__(self, env_name, num_envs, device=0, seed=0, horizon=None, copy=False, **make_kwargs):
        if isinstance(num_envs, bool) or not isinstance(num_envs, (int, np.integer)) or int(num_envs) < 1:
            raise ValueError("LocoVectorEnv: num_envs must be an integer >= 1, not %r" % (num_envs,))
        self.num_envs = int(num_envs)
        self._device_index = self._index_of(device)
        self._env = LocoEnv.make(env_name, n_envs=self.num_envs, device=self._device_index, **make_kwargs)
        why = _vector_env_refusal(self._env)
        if why is not None:
            raise NotImplementedError("LocoVectorEnv: " + why)
        self.spec = None
        self.render_mode = None
        self.metadata = dict(self.metadata, render_fps=1.0 / self._env.dt)
        self.single_observation_space = GymnasiumWrapper._convert_space(self._env.info.observation_space)
        self.single_action_space = GymnasiumWrapper._convert_space(self._env.info.action_space)
        self.observation_space = self._batched(self.single_observation_space)
        self.action_space = self._batched(self.single_action_space)
        self._copy, self._horizon = bool(copy), horizon
        self._lib = load_vec_library()

        import torch
        self.device = dev = torch.device("cuda", self._device_index)
        b = self._env.backend
        n, nobs = self.num_envs, b.nobs
        self._term = torch.zeros((n, nobs), dtype=torch.float32, device=dev)       # the step kernel's terminal-observation buffer
        self._arm(seed)
        self._ring = [_ResultSet(torch, n, nobs, dev) for _ in range(2)]
        self._slot = 0
        self._run_return = torch.zeros(n, dtype=torch.float32, device=dev)
        self._run_length = torch.zeros(n, dtype=torch.int32, device=dev)
        perm = self._env._obs_perm()
        # (rare) the reference's column order is not the kernel's: the step and the bookkeeping run on raw buffers, and one
        # index_select each brings observation and final observation into the result set
        self._perm = None if perm is None else torch.as_tensor(np.asarray(perm), dtype=torch.int64, device=dev)
        self._raw_obs = self._raw_final = None
        if self._perm is not None:
            self._raw_obs = torch.zeros((n, nobs), dtype=torch.float32, device=dev)
            self._raw_final = torch.zeros((n, nobs), dtype=torch.float32, device=dev)
        self._started = False
        self._reset_obs = None          # the observation of a full reset() until the first step() replaces it

    @staticmethod
    def _index_of(device):
        if isinstance(device, (int, np.integer)) and not isinstance(device, bool):
            return int(device)
        import torch
        d = torch.device(device)
        if d.type != "cuda":
            raise ValueError("LocoVectorEnv: device must be a GPU (an index, 'cuda' or 'cuda:i'), not %r" % (device,))
        return torch.cuda.current_device() if d.index is None else d.index

    def _batched(self, space):
        return _spaces.Box(space.low.min(), space.high.max(), shape=(self.num_envs,) + tuple(space.shape), dtype=space.dtype)

    def _arm(self, seed):
        """Device-side restarts keyed by ``seed``, and the terminal observations into this object's tensor (enable_auto_reset
        switches a batch's terminal observations off unless it is asked for the host form)."""
        self._env.enable_auto_reset(seed=seed, horizon=self._horizon)
        self._env.backend.enable_terminal_obs(self._term)

    @property
    def unwrapped(self):
        return self._env

    def reset(self, *, seed=None, options=None):
        """The wrapped environment's host ``reset()``: every environment starts a new episode; returns ``(obs, {})`` with the
        observation uploaded once as float32 [num_envs, nobs]. A given ``seed`` re-keys the device-side restart draws; like the
        single-environment wrapper's, it does not touch ``np.random``, which the host reset draws from.

        ``options={"reset_mask": m}`` is Gymnasium's PARTIAL reset, and stays on the device: ``m`` is a bool / uint8 device tensor
        [num_envs] (a numpy mask is uploaded); the masked environments restart as the step kernel restarts an episode that ended
        (:meth:`HipBatch.restart_device`: the next row of the reset table under the environment's own draw, episode count + 1), queued
        on torch's current stream; their running return and length start from zero. Nothing waits on the host and there is no host
        reset. Returns ``(obs, {})``: the current result set's observation — what the last ``step()`` returned (after a full
        ``reset()``: what that returned) — with the masked rows replaced IN PLACE by the new episodes' first observations. Like
        ``step()`` it bypasses ``LocoEnv``'s host mirrors of the state. Takes no ``seed``."""
        import torch
        if options is not None and options.get("reset_mask") is not None:
            return self._reset_masked(options["reset_mask"], seed)
        torch.cuda.synchronize(self.device)          # THE host wait of this class: steps still queued finish before the host restarts everything
        if seed is not None:
            self._arm(int(seed))
        self._env.reset()
        obs = torch.from_numpy(np.ascontiguousarray(self._env._obs, dtype=np.float32)).to(self.device)
        with torch.cuda.device(self.device):
            self._run_return.zero_()
            self._run_length.zero_()
        self._started = True
        self._reset_obs = obs
        return obs, {}

    def _reset_masked(self, m, seed):
        import torch
        if seed is not None:
            raise ValueError("LocoVectorEnv.reset: a partial reset takes no seed (the restart draws stay keyed as they are)")
        if not self._started:
            raise RuntimeError("call reset() before a partial reset")
        env, b = self._env, self._env.backend
        n = self.num_envs
        if not hasattr(m, "data_ptr"):
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(m).reshape(-1) != 0)).to(self.device)
        if tuple(m.shape) != (n,) or m.dtype not in (torch.bool, torch.uint8) or not m.is_cuda or not m.is_contiguous():
            raise ValueError("LocoVectorEnv.reset: reset_mask must be a contiguous bool or uint8 device tensor [%d], not %s %s"
                             % (n, m.dtype, list(m.shape)))
        if env._pending_state:
            env._upload_state()
        r = self._ring[self._slot]
        raw_obs = r.obs if self._perm is None else self._raw_obs
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            mb = m if m.dtype == torch.bool else m != 0
            b.restart_device(m, obs=raw_obs, stream=stream, sync=False)
            if self._perm is not None:
                torch.index_select(raw_obs, 1, self._perm, out=r.obs)
            if self._reset_obs is not None:
                # no step since the full reset: the rows that no partial reset has replaced are the full reset's. They are kept in a
                # tensor of their own, outside the ring (torch.where makes a new one), so the next partial reset finds them again
                self._reset_obs = torch.where(mb[:, None], r.obs, self._reset_obs)
                r.obs.copy_(self._reset_obs)
            self._run_return.masked_fill_(mb, 0.0)
            self._run_length.masked_fill_(mb, 0)
            obs = r.obs.clone() if self._copy else r.obs
        return obs, {}

    def state(self):
        """The full state of every environment as device tensors, queued on torch's current stream and waiting for nothing
        (:meth:`HipBatch.get_state_device`): ``{"qpos": float32 [n, nv], "qvel": float32 [n, nv], "ep_step": int32 [n]}`` — the root's
        horizontal position included, which no observation shows. Fresh tensors at every call. Read from the device batch, not from
        ``LocoEnv``'s host mirrors (as ``step()``)."""
        import torch
        env, b = self._env, self._env.backend
        if env._pending_state:
            env._upload_state()
        n = self.num_envs
        with torch.cuda.device(self.device):
            out = {"qpos": torch.empty((n, b.nv), dtype=torch.float32, device=self.device),
                   "qvel": torch.empty((n, b.nv), dtype=torch.float32, device=self.device),
                   "ep_step": torch.empty(n, dtype=torch.int32, device=self.device)}
            b.get_state_device(stream=torch.cuda.current_stream(self.device).cuda_stream, sync=False, **out)
        return out

    def step(self, actions):
        import torch
        if not self._started:
            raise RuntimeError("call reset() before step()")
        env, b = self._env, self._env.backend
        n, nobs = self.num_envs, b.nobs
        _check_device_buffer("LocoVectorEnv.step", "actions", actions, (n, b.nu), "float32", raw=False)
        if env._pending_state:
            env._upload_state()
        self._reset_obs = None
        self._slot ^= 1
        r = self._ring[self._slot]
        raw_obs, raw_final = (r.obs, r.final_obs) if self._perm is None else (self._raw_obs, self._raw_final)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            b.step_device(actions, raw_obs, r.reward, r.done, stream=stream, sync=False)
            p = _dev_ptr
            _check(self._lib.lv_finish_step(n, nobs, p(raw_obs), p(r.reward), p(r.done), p(self._term), p(r.terminated), p(r.truncated),
                                            p(raw_final), p(self._run_return), p(self._run_length), p(r.ep_return), p(r.ep_length),
                                            _stream_ptr(stream), 0))
            torch.bitwise_or(r.terminated_b, r.truncated_b, out=r.ended)
            if self._perm is not None:
                torch.index_select(raw_obs, 1, self._perm, out=r.obs)
                torch.index_select(raw_final, 1, self._perm, out=r.final_obs)
            out = (r.obs, r.reward, r.terminated_b, r.truncated_b, r.final_obs, r.ended, r.ep_return, r.ep_length)
            if self._copy:
                out = tuple(x.clone() for x in out)
        obs, reward, terminated, truncated, final_obs, ended, ep_r, ep_l = out
        info = {"final_obs": final_obs, "_final_obs": ended, "episode": {"r": ep_r, "l": ep_l}, "_episode": ended}
        return obs, reward, terminated, truncated, info

    def close(self, **kwargs):
        env = getattr(self, "_env", None)
        if env is not None:
            b = env._backend
            if b is not None and getattr(b, "_h", None) and b._term_out is self._term:
                b.disable_terminal_obs()
            env.stop()
        self._started = False

    def create_dataset(self, **kwargs):
        return self._env.create_dataset(**kwargs)
