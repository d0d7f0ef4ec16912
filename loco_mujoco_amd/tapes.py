"""
ctypes loader for ``liblocotape.so`` (C-ABI: ``include/locotape.h``) — the learner's side of the tapes: episode returns, discounted
returns and lengths from the reward and done tapes of :meth:`HipBatch.rollout_tape` / :meth:`HipBatch.rollout_policy`, carried across
rollouts. The library reads tapes only: no batch, no model. There is no torch fallback: if the library is missing this module raises.
"""

import ctypes as C
import os
import types

import numpy as np

from .backend import BackendError, _check_device_buffer, _dev_ptr, _number, _stream_ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
TAPE_LIB_PATH = os.path.join(_HERE, "csrc", "liblocotape.so")

CARRY_ROWS, SUMMARY_FIELDS = 4, 10            # include/locotape.h LT_CARRY_ROWS, LT_SUMMARY_FIELDS
# the summary's fields in the order of the header
SUMMARY_LAYOUT = ("episodes", "R_sum", "RR_sum", "R_min", "R_max", "J_sum", "L_sum", "L_min", "L_max", "absorbing")
_EMPTY_SUMMARY = (0.0, 0.0, 0.0, float("inf"), float("-inf"), 0.0, 0.0, float("inf"), float("-inf"), 0.0)

# THE prototypes of include/locotape.h, stated once: name -> (restype, argtypes), as backend._PROTOTYPES
_P, _I, _LL, _FL = C.c_void_p, C.c_int, C.c_longlong, C.c_float
_PROTOTYPES = {
    "lt_last_error": (C.c_char_p, None),
    "lt_episode_work_doubles": (_LL, [_LL]),
    "lt_episode_carry_reset": (_I, [_LL, _P, _P, _P, _P, _I]),
    "lt_tape_episodes": (_I, [_I, _LL, _P, _P, _P, _FL, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _I]),
}
TAPE_EXPORTS = list(_PROTOTYPES)

_lib = None


def load_tape_library():
    """Load liblocotape.so and declare its prototypes. Raises BackendError if it is not built. (With torch in the process, import
    torch first: whichever HIP runtime is loaded first serves both.)"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(TAPE_LIB_PATH):
        raise BackendError("tape library not built: %s is missing (run `python -c 'import __graft_entry__ as g; g.build()'` or "
                           "`make -C loco_mujoco_amd/csrc liblocotape.so`). There is no torch fallback." % TAPE_LIB_PATH)
    lib = C.CDLL(TAPE_LIB_PATH)
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise BackendError("liblocotape: %s (code %d)" % (load_tape_library().lt_last_error().decode(), rc))


def check_episode_args(n, reward, done, gamma=0.99, mask=None, ep_return=None, ep_disc_return=None, ep_length=None, trace=None, n_steps=None):
    """The argument checks of :meth:`EpisodeMeter.update`, without a device: returns ``(T, gamma)`` or raises ValueError. Buffers are
    described objects (torch tensors), which are checked — ``reward`` / ``ep_return`` / ``ep_disc_return`` / ``trace`` float32 [T, n],
    ``done`` uint8 [T, n], ``ep_length`` int32 [T, n], ``mask`` uint8 [n] — or raw device pointers (ints), which are taken as given; T
    comes from the first described tape, or from ``n_steps`` when every tape is a raw pointer."""
    who = "episodes"
    for name, x in (("reward", reward), ("done", done)):
        if x is None:
            raise ValueError("%s: %s is None" % (who, name))
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) < 1:
        raise ValueError("%s: n_envs must be an integer >= 1, not %r" % (who, n))
    n = int(n)
    tapes = (("reward", reward, "float32"), ("done", done, "uint8"), ("ep_return", ep_return, "float32"),
             ("ep_disc_return", ep_disc_return, "float32"), ("ep_length", ep_length, "int32"), ("trace", trace, "float32"))
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
    if mask is not None:
        _check_device_buffer(who, "mask", mask, (n,), "uint8")
    return T, _check_gamma(who, gamma)


def _check_gamma(who, gamma):
    g = _number(who, "gamma", gamma)
    if not (0.0 <= g <= 1.0):
        raise ValueError("%s: gamma must be in [0, 1], not %r" % (who, g))
    return g


class EpisodeMeter:
    """Episode statistics of ``n_envs`` environments from their reward and done tapes (``lt_tape_episodes``): owns the carry — what
    every running episode has accumulated, so that episodes run across :meth:`update` calls — the scratch of the summary and the device
    summary itself. An episode ends where ``done != 0`` (absorbing, restarted on the device, or at the horizon), and the reward of that
    step belongs to it; an unfinished episode is never counted.

    ``carry`` (float32 [4, n]: return, discounted return, the next reward's weight, the running discounted return) and ``length``
    (int32 [n]) are plain tensors: save them beside a :class:`Snapshot` with ``clone()``, put them back with ``copy_()``, and after
    ``fork(src)`` gather them by the same ``src`` (``carry.index_select(1, src)``, ``length.index_select(0, src)`` where ``src >= 0``)."""

    def __init__(self, n_envs, device="cuda", gamma=0.99):
        import torch
        if isinstance(n_envs, bool) or not isinstance(n_envs, (int, np.integer)) or int(n_envs) < 1:
            raise ValueError("EpisodeMeter: n_envs must be an integer >= 1, not %r" % (n_envs,))
        self.n, self.gamma = int(n_envs), _check_gamma("EpisodeMeter", gamma)
        self._lib = load_tape_library()
        dev = torch.device(device)
        self.device = dev if dev.index is not None else torch.device(dev.type, torch.cuda.current_device())
        self.carry = torch.empty((CARRY_ROWS, self.n), dtype=torch.float32, device=self.device)
        self.length = torch.empty(self.n, dtype=torch.int32, device=self.device)
        self._work = torch.empty(int(self._lib.lt_episode_work_doubles(self.n)), dtype=torch.float64, device=self.device)
        self._summary = torch.empty(SUMMARY_FIELDS, dtype=torch.float64, device=self.device)
        self._fresh = True                    # the device summary holds nothing yet: the next update overwrites it
        self.reset()

    def _stream(self, stream):
        """(torch stream to allocate under, raw hipStream_t): the caller's, or torch's current one on the meter's device."""
        import torch
        s = torch.cuda.current_stream(self.device) if stream is None else torch.cuda.ExternalStream(int(stream), device=self.device)
        return s, s.cuda_stream

    @staticmethod
    def _mask(mask):
        """A bool tensor is its bytes."""
        if mask is not None and "bool" in str(getattr(mask, "dtype", "")):
            import torch
            return mask.view(torch.uint8)
        return mask

    def reset(self, mask=None, stream=None, sync=True):
        """A fresh carry for every environment, or where ``mask`` (uint8 or bool device tensor [n]) is set (``lt_episode_carry_reset``):
        after a host-side ``reset()`` / ``set_state`` that drops running episodes. The summary is not touched."""
        import torch
        mask = self._mask(mask)
        if mask is not None:
            _check_device_buffer("episodes", "mask", mask, (self.n,), "uint8")
        _, raw = self._stream(stream)
        with torch.cuda.device(self.device):
            _check(self._lib.lt_episode_carry_reset(self.n, _dev_ptr(self.carry), _dev_ptr(self.length), _dev_ptr(mask), _stream_ptr(raw), int(bool(sync))))

    def update(self, rew, done, stream=None, sync=True, want=("ret", "length"), trace=False, mask=None):
        """Scan the tapes ``rew`` float32 [K, n] and ``done`` uint8 [K, n] of one rollout: ONE call of ``lt_tape_episodes``, the summary
        accumulated on the device. ``stream``: a raw hipStream_t (None: torch's current stream), ``sync`` as in
        :meth:`HipBatch.rollout_tape`; the call is ordered like a torch op on the tapes. Returns an object with only what was asked
        for: ``want`` names among ``ret`` / ``disc`` float32 [K, n] (NaN where no episode ended), ``length`` int32 [K, n] (-1 there),
        and with ``trace=True`` ``trace`` float32 [K, n], the running discounted return including each step's reward. ``mask`` (uint8 or
        bool device tensor [n]): environments whose byte is 0 are skipped — pass the active list as a mask, their tape rows are stale."""
        import torch
        want = (want,) if isinstance(want, str) else tuple(want)
        for w in want:
            if w not in ("ret", "disc", "length"):
                raise ValueError("episodes: want names ret, disc or length, not %r" % (w,))
        mask = self._mask(mask)
        T, _ = check_episode_args(self.n, rew, done, self.gamma, mask=mask)
        ts, raw = self._stream(stream)
        out = types.SimpleNamespace()
        with torch.cuda.device(self.device), torch.cuda.stream(ts):
            for name in ("ret", "disc"):
                if name in want:
                    setattr(out, name, torch.full((T, self.n), float("nan"), dtype=torch.float32, device=self.device))
            if "length" in want:
                out.length = torch.full((T, self.n), -1, dtype=torch.int32, device=self.device)
            if trace:
                out.trace = torch.empty((T, self.n), dtype=torch.float32, device=self.device)
                if mask is not None:
                    out.trace.fill_(float("nan"))           # the rows of skipped environments are not written
            g = vars(out).get
            _check(self._lib.lt_tape_episodes(T, self.n, _dev_ptr(rew), _dev_ptr(done), _dev_ptr(mask), self.gamma,
                                              _dev_ptr(self.carry), _dev_ptr(self.length),
                                              _dev_ptr(g("ret")), _dev_ptr(g("disc")), _dev_ptr(g("length")), _dev_ptr(g("trace")),
                                              _dev_ptr(self._summary), 0 if self._fresh else 1, _dev_ptr(self._work),
                                              _stream_ptr(raw), int(bool(sync))))
        self._fresh = False
        return out

    def summary_raw(self):
        """The device summary as a float64 numpy array [10] in the header's order (waits for the device)."""
        import torch
        if self._fresh:
            return np.array(_EMPTY_SUMMARY, dtype=np.float64)
        torch.cuda.synchronize(self.device)
        return self._summary.cpu().numpy()

    def summary(self, reset=True):
        """THE host read: waits for the device and returns ``episodes``, ``R_mean``, ``R_std``, ``R_min``, ``R_max`` (undiscounted
        returns: the reference's ``compute_J(dataset)``), ``J_mean`` (``compute_J(dataset, gamma)``), ``L_mean``, ``L_min``, ``L_max``
        (``compute_episodes_length``) and ``absorbing_share`` of the episodes finished since the last reset of the summary. The means
        are NaN at 0 episodes (min +inf, max -inf). ``reset``: the next :meth:`update` starts a new summary; the carry stays."""
        s = dict(zip(SUMMARY_LAYOUT, (float(v) for v in self.summary_raw())))
        k = s["episodes"]
        nan = float("nan")
        r_mean = s["R_sum"] / k if k else nan
        out = dict(episodes=int(k), R_mean=r_mean, R_std=float(np.sqrt(max(s["RR_sum"] / k - r_mean * r_mean, 0.0))) if k else nan,
                   R_min=s["R_min"], R_max=s["R_max"], J_mean=s["J_sum"] / k if k else nan, L_mean=s["L_sum"] / k if k else nan,
                   L_min=s["L_min"], L_max=s["L_max"], absorbing_share=s["absorbing"] / k if k else nan)
        if reset:
            self._fresh = True
        return out
