"""Writes tests/golden/a1_newton_hard_states.npz: quadruped states whose Newton iterations exercise every path of the Hessian pass
(lm_core.h hess_slot / accumulate), with what the lane emulator of a given source tree computes from them in one control step.

    python tools/probes/newton_hard_states.py --root <tree whose emulator records the expected values> --out tests/golden/a1_newton_hard_states.npz
                                              [--trace-lib libemu_trace.so] [--row 0] [--steps 40]

The states: a reset-table row stepped under zero action with the warm start carried (ls_points=4) until the robot has collapsed — the
standing state it starts from (foot contacts only), the control step with the most Newton iterations, steps whose Hessian passes mix
the quadratic and the cone zone —, the robot turned on its back (condim-3 contacts only) and states with self-contacts from
tests/golden/a1_self_contact_states.npz. --trace-lib: an emulator built with -DLM_HESS_TRACE -DEMU_LS_POINTS=4 (it prints dim and zone
of every slot visit); without it the states are picked by iteration count alone and their zones are not reported.
The expected values are recorded twice and must agree with themselves before the file is written."""
import argparse
import ctypes
import os
import re
import sys
import tempfile

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--out", required=True)
ap.add_argument("--trace-lib", default=None)
ap.add_argument("--row", type=int, default=0)
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()
root = os.path.abspath(args.root)
sys.path[:0] = [root, os.path.join(root, "tests")]

from loco_mujoco_amd import LocoEnv, lowering          # noqa: E402
from oracle.model_blob import pack_model               # noqa: E402
from oracle.pyoracle import Oracle                     # noqa: E402
from emu import pyemu                                  # noqa: E402

np.random.seed(0)
env = LocoEnv.make("UnitreeA1.simple", debug=True)
m = env._model
cmod, info = lowering.lower(m, env._device_task())
oracle = Oracle(pack_model(m))
nv, nu = m.nv, len(env._action_indices)
CONFIGS = (("ls4_rep1", dict(ls_points=4, rep=1)), ("ls4_rep4", dict(ls_points=4, rep=4)), ("ls1_rep1", dict(ls_points=1, rep=1)))


def step(q, v, w, a, **kw):
    qe, ve, we, cnt, _ = pyemu.run(cmod, q, v, a, nsub=10, warm=w, **kw)
    return qe[0], ve[0], we[0], cnt


def contact_dims(q, v, w, a):
    """condim of every contact the fp64 oracle finds in the state (a contact takes the larger condim of its two geoms)."""
    ctrl = np.zeros(m.nu)
    ctrl[env._action_indices] = env._preprocess_action(a)
    f = oracle.forward(q, v, ctrl, w)
    return sorted(int(max(m.geom_condim[c["geom1"]], m.geom_condim[c["geom2"]])) for c in f["contacts"]), \
        sum(1 for c in f["contacts"] if m.geom_type[c["geom1"]] != 0)


def trace(q, v, w, a):
    """(passes, visits by (dim, zone), passes that mix dims, passes that mix zones) of one control step, from the traced emulator."""
    if not args.trace_lib:
        return None
    real_build = pyemu.build
    pyemu.build = lambda *a_, **k_: os.path.abspath(args.trace_lib)
    sys.stdout.flush()
    with tempfile.TemporaryFile() as tmp:
        keep = os.dup(1)
        os.dup2(tmp.fileno(), 1)
        try:
            pyemu.run(cmod, q, v, a, nsub=10, warm=w, ls_points=4)
        finally:
            ctypes.CDLL(None).fflush(None)          # (the emulator prints through C stdio)
            os.dup2(keep, 1)
            os.close(keep)
            pyemu.build = real_build
        tmp.seek(0)
        text = tmp.read().decode()
    passes, visits, cur, last_it = [], {}, None, None
    for mt in re.finditer(r"hess it (\d+) lane (\d+) rep (\d+) slot (\d+) dim (\d+) zone (\d+)", text):
        it, lane, _, slot, dim, zone = (int(x) for x in mt.groups())
        # the four lane threads print concurrently: a pass = the run of lines with one iteration number (it restarts at 0 every substep)
        if cur is None or it != last_it:
            cur = []
            passes.append(cur)
            last_it = it
        cur.append((dim, zone))
        visits[(dim, zone)] = visits.get((dim, zone), 0) + 1
    mix_dim = sum(1 for p in passes if len({d for d, _ in p}) > 1)
    mix_zone = sum(1 for p in passes if len({z for _, z in p}) > 1)
    return dict(passes=len(passes), visits=visits, mix_dim=mix_dim, mix_zone=mix_zone)


# ---- the roll-out of one reset row under zero action
table = env._reset_table()
q, v, w = table[args.row, :nv].copy(), table[args.row, nv:2 * nv].copy(), np.zeros(nv)
zero = np.zeros(nu)
roll = []
for k in range(args.steps):
    qn, vn, wn, cnt = step(q, v, w, zero, ls_points=4)
    roll.append((q, v, w, cnt))
    print("step %2d: Newton iterations %3d, line-search rounds %3d, contacts %3d" % (k, cnt["solver_iters"], cnt["ls_evals"], cnt["ncon"]))
    q, v, w = qn, vn, wn
hard = sorted(range(len(roll)), key=lambda k: -roll[k][3]["solver_iters"])
standing = next(k for k in range(len(roll)) if (lambda dims: len(dims) >= 4 and min(dims) == 6)(contact_dims(roll[k][0], roll[k][1], roll[k][2], zero)[0]))
picks = [("reset_row", 0), ("standing", standing), ("collapsed", hard[0])]
traces = {k: trace(roll[k][0], roll[k][1], roll[k][2], zero) for k in hard[:6]} if args.trace_lib else {}
zone_mixed = sorted((k for k in traces if k != hard[0]), key=lambda k: -traces[k]["mix_zone"])
picks += [("zones_mixed_%d" % i, k) for i, k in enumerate((zone_mixed or hard[1:])[:2])]

names, Q, V, W, A = [], [], [], [], []
for name, k in picks:
    names.append("%s_step%d" % (name, k)); Q.append(roll[k][0]); V.append(roll[k][1]); W.append(roll[k][2]); A.append(zero)

# ---- the robot on its side or on its back: condim-3 contacts only. Turned directly (the trunk's first rotation), then left to fall and
# settle under zero action; the first states with two or more contacts, all of them condim 3, are taken
side = []
for ang in (np.pi / 2, -np.pi / 2, np.pi):
    q = table[args.row, :nv].copy(); v = np.zeros(nv); w = np.zeros(nv)
    q[3] += ang
    for k in range(60):
        dims, _ = contact_dims(q, v, w, zero)
        if len(dims) >= 2 and max(dims) == 3:
            side.append((ang, k, q.copy(), v.copy(), w.copy(), len(dims)))
            break
        q, v, w, cnt = step(q, v, w, zero, ls_points=4)
        assert np.isfinite(q).all()
side.sort(key=lambda s: -s[5])
assert side, "no laid-down state with condim-3 contacts only"
for ang, k, q, v, w, n in side[:2]:
    names.append("turned_%+.2f_step%d" % (ang, k)); Q.append(q); V.append(v); W.append(w); A.append(zero)

# ---- self-contacts: a state of the oracle roll-outs in which two legs touch
d = np.load(os.path.join(root, "tests", "golden", "a1_self_contact_states.npz"))
for i in (65, 143):
    names.append("self_contact_%d" % i); Q.append(d["q"][i]); V.append(d["v"][i]); W.append(d["w"][i]); A.append(d["a"][i])

# the device holds float32: the inputs are stored as what it will see
Q, V, W, A = (np.array(x, dtype=np.float32).astype(np.float64) for x in (Q, V, W, A))
out = dict(names=np.array(names), qpos=Q, qvel=V, warm=W, action=A)
for i, name in enumerate(names):
    dims, nself = contact_dims(Q[i], V[i], W[i], A[i])
    print("%-32s contact condims %s, self-contacts %d, trace %s" % (name, dims, nself, trace(Q[i], V[i], W[i], A[i])))
for tag, kw in CONFIGS:
    res = []
    for rep_ in range(2):          # twice: the recorder must reproduce itself
        rows = [step(Q[i], V[i], W[i], A[i], **kw) for i in range(len(names))]
        res.append(dict(q=np.array([r[0] for r in rows]), v=np.array([r[1] for r in rows]), w=np.array([r[2] for r in rows]),
                        solver_iters=np.array([r[3]["solver_iters"] for r in rows]), ls_evals=np.array([r[3]["ls_evals"] for r in rows]),
                        ncon=np.array([r[3]["ncon"] for r in rows])))
    for key in res[0]:
        assert np.array_equal(res[0][key], res[1][key]), (tag, key)
        out["%s_%s" % (tag, key)] = res[0][key]
    print(tag, "iterations", res[0]["solver_iters"], "line-search rounds", res[0]["ls_evals"], "contacts", res[0]["ncon"])
np.savez_compressed(args.out, **out)
print("wrote", args.out, os.path.getsize(args.out), "bytes")
