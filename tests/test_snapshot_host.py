"""
Device-side snapshots (include/locohip.h lm_snapshot_*), the parts that need no GPU: the seven C-ABI names, the argument checks of
HipBatch.restore / fork (backend.check_restore_args, which runs without a device) and the index walks of csrc/lm_snapshot.h, run on
the host under the address and undefined-behaviour sanitizers as a stand-alone program (tests/snapshot_walk_main.cpp).
"""

import os
import re
import subprocess
import types

import numpy as np
import pytest

from loco_mujoco_amd.backend import check_restore_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5
NAMES = ["lm_snapshot_create", "lm_snapshot_destroy", "lm_snapshot_save", "lm_snapshot_restore", "lm_snapshot_bytes",
         "lm_snapshot_export", "lm_snapshot_import"]


class _Buf:
    """What the checker looks at in a torch tensor: shape, dtype, contiguity, where it lives."""

    def __init__(self, shape, dtype="torch.int32", contiguous=True, is_cuda=True):
        self.shape, self.dtype, self._c, self.is_cuda = tuple(shape), dtype, contiguous, is_cuda

    def is_contiguous(self):
        return self._c

    def data_ptr(self):
        return 0


def test_abi_names_are_declared_exported_and_listed():
    from loco_mujoco_amd import backend
    header = open(os.path.join(ROOT, "include", "locohip.h")).read()
    declared = set(re.findall(r"\b(lm_[a-z_]+)\s*\(", header))
    lib = backend.load_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", backend.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lm_[a-z_0-9]+)$", syms, flags=re.M))
    for name in NAMES:
        assert name in declared and name in exported and name in backend.EXPORTS and hasattr(lib, name), name
    # null handles are refused with a message before anything touches a device
    assert lib.lm_snapshot_create(None, 0, None) != 0 and b"null" in lib.lm_last_error()
    assert lib.lm_snapshot_save(None, None, None, 1) != 0 and b"null" in lib.lm_last_error()
    assert lib.lm_snapshot_restore(None, None, None, None, 1) != 0 and b"null" in lib.lm_last_error()
    assert lib.lm_snapshot_export(None, None, None, 0) != 0 and lib.lm_snapshot_import(None, None, None, 0) != 0
    assert lib.lm_snapshot_bytes(None) == 0
    lib.lm_snapshot_destroy(None)


def test_checker_accepts_none_device_tensors_and_host_integers():
    assert check_restore_args(N) == ("all", None)
    t = _Buf((N,))
    assert check_restore_args(N, src=t) == ("device", t)
    m = _Buf((N,), "torch.bool")
    assert check_restore_args(N, mask=m) == ("device_mask", m)
    kind, a = check_restore_args(N, src=[4, 4, -1, N, 0])
    assert kind == "host" and a.dtype == np.int32 and a.tolist() == [4, 4, -1, -1, 0]          # outside [0, n): "keep", folded to -1
    kind, a = check_restore_args(N, src=np.array([0, 1, 2, 2 ** 40, -2 ** 40]))
    assert a.dtype == np.int32 and a.tolist() == [0, 1, 2, -1, -1]
    kind, a = check_restore_args(N, mask=np.array([True, False, False, True, False]))
    assert kind == "host" and a.dtype == np.int32 and a.tolist() == [0, -1, -1, 3, -1]
    assert check_restore_args(N, mask=[False] * N)[1].tolist() == [-1] * N


@pytest.mark.parametrize("kw,word", [
    (dict(src=_Buf((N,), "torch.int64")), "int32"),                       # wrong dtype
    (dict(src=_Buf((N,), "torch.float32")), "int32"),
    (dict(src=np.zeros(N, dtype=np.float32)), "integers"),
    (dict(src=_Buf((N + 1,))), r"must be \[5\]"),                         # wrong length
    (dict(src=list(range(N - 1))), r"must be \[5\]"),
    (dict(src=np.zeros((N, 1), dtype=np.int32)), r"must be \[5\]"),
    (dict(src=_Buf((N,), is_cuda=False)), "on the device"),               # a CPU tensor where a CUDA one is needed
    (dict(mask=_Buf((N,), "torch.bool", is_cuda=False)), "on the device"),
    (dict(src=_Buf((N,), contiguous=False)), "contiguous"),
    (dict(src=_Buf((N,)), mask=np.ones(N, dtype=bool)), "not both"),      # a mask together with src
    (dict(src=[0] * N, mask=[True] * N), "not both"),
    (dict(mask=np.ones(N, dtype=np.int32)), "booleans"),
    (dict(mask=_Buf((N,), "torch.uint8")), "bool"),
    (dict(src=3), "sequence"),
    (dict(src="01234"), "sequence"),
])
def test_checker_rejects(kw, word):
    with pytest.raises(ValueError, match=word):
        check_restore_args(N, **kw)


def test_checker_refuses_foreign_stale_and_closed_snapshots():
    sig = (N, 18, 0, 37, 0, 0)
    batch = types.SimpleNamespace(snapshot_signature=lambda: sig)
    snap = types.SimpleNamespace(batch=batch, signature=sig, closed=False)
    assert check_restore_args(N, snapshot=snap, batch=batch) == ("all", None)
    other = types.SimpleNamespace(snapshot_signature=lambda: sig)
    with pytest.raises(ValueError, match="another batch"):
        check_restore_args(N, snapshot=snap, batch=other)
    stale = types.SimpleNamespace(batch=batch, signature=(N, 18, 0, 37, 4, 0), closed=False)
    with pytest.raises(ValueError, match="another configuration"):
        check_restore_args(N, snapshot=stale, batch=batch)
    with pytest.raises(ValueError, match="closed"):
        check_restore_args(N, snapshot=types.SimpleNamespace(batch=batch, signature=sig, closed=True), batch=batch)


def test_index_walks_on_the_host_under_sanitizers(tmp_path):
    """tests/snapshot_walk_main.cpp: segment tables for N = 1, 37, 64 (SoA rows of 4- and 1-byte elements, AoS rows of 112 and 128
    bytes), save, identity restore and a gathered restore whose source list holds repeats, -1, N and INT_MIN, against a naive loop.
    A stand-alone program with its own main: nothing sanitised is loaded into this interpreter."""
    exe = str(tmp_path / "snapshot_walk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, os.path.join(ROOT, "tests", "snapshot_walk_main.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "snapshot walks: ok" in run.stdout
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
