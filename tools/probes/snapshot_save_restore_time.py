"""Time of a snapshot save, an identity restore and a gathered restore (HipBatch.snapshot / restore), by HIP events on the caller's
stream, beside one control step of the same batch (HipBatch.rollout's kernel_ms per step): median of 20 after warm-up, bytes moved,
effective copy rate (bytes read + bytes written over the time). DESIGN.md section 5 quotes its output.
    python tools/probes/snapshot_save_restore_time.py [n_envs]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loco_mujoco_amd import LocoEnv

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
REPEATS, WARMUP = 20, 5


def timed(fn, stream):
    ms = []
    for i in range(WARMUP + REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if i >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(min(ms)), float(max(ms))


for task in ("UnitreeA1.simple", "HumanoidTorque.run"):
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, n_envs=N)
    env.reset()
    env.enable_auto_reset(seed=0)
    env.step(np.zeros((N, len(env._action_indices))))
    b = env.backend
    b.rollout(50, action_mode=1)
    step_ms = b.rollout(200, action_mode=1)["kernel_ms"] / 200
    side = torch.cuda.Stream()
    s = side.cuda_stream
    src = torch.randperm(N, device="cuda").to(torch.int32).contiguous()
    torch.cuda.synchronize()
    print("%s, %d environments: control step %.4f ms" % (task, N, step_ms))
    for keep in ((True, False) if b.snapshot(keep_collider_cache=False).nbytes < b.snapshot().nbytes else (True,)):
        snap = b.snapshot(keep_collider_cache=keep)
        nbytes = snap.nbytes
        rows = (("save", lambda: snap.save(stream=s, sync=False)),
                ("restore (identity)", lambda: b.restore(snap, stream=s, sync=False)),
                ("restore (gather, a permutation)", lambda: b.restore(snap, src=src, stream=s, sync=False)))
        for name, fn in rows:
            med, lo, hi = timed(fn, side)
            print("  %-34s cache %-3s %10d B  median %.4f ms (min %.4f, max %.4f)  %.3f TB/s read+write  = %.2f %% of a control step"
                  % (name, "in" if keep else "out", nbytes, med, lo, hi, 2 * nbytes / (med * 1e-3) / 1e12, 100 * med / step_ms))
        snap.close()
    b.close()
