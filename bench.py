"""
bench.py — env-steps/s of the batched LocoEnv.step() hot path (BASELINE.json metric) on N GPUs of one node.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--envs-per-gpu 4096] [--task UnitreeA1.simple] [--full] [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up (W control steps), times exactly K control steps, writes the outputs of that block when
`--dump-outputs DIR` is given (dump_outputs: final qpos / qvel and the block's counters as DIR/<name>.npy; the inputs are
seeded, so two builds can be compared output for output) and prints the line: `value` = env-steps/s of the K-step block,
`ms_per_step` = milliseconds of one of its control steps. `--full` adds every other leg described below (the sustained
block, the fused rollout, the parity sample against the fp64 oracle, the CPU baseline, the python_surface leg and the other
BASELINE configs); each of them can also be asked for on its own by its option.

`--gpus N` with N > 1 and no launcher around it (WORLD_SIZE unset): bench.py starts the N ranks itself (one process per
GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set, rendezvous on 127.0.0.1) and fails loudly on a node with fewer GPUs.
Under a launcher, WORLD_SIZE must equal --gpus.

Workload of the headline (BASELINE.json configs[1]): UnitreeA1.simple, 4096 environments per GPU,
zero action, initial states = the 300 samples of the bundled mini dataset drawn with RandomState(0),
device-side auto-reset on _has_fallen or after 1000 control steps. A "step" = one control step of every
environment (= 10 physics substeps + observation + reward + termination + resets), one kernel launch.
Environments are independent: ranks shard them (weak scaling), the only collective is the metric
all-reduce at report time: ncclAllReduce on librccl.so through ctypes (loco_mujoco_amd/utils/collective.py).

With --full, the other BASELINE configs ride in the same line under "configs" (one rank, default task only): short legs of
HumanoidTorque.run (4096, random policy), Atlas.walk with back joints and per-episode joint-damping randomisation (2048 =
config 4's per-GPU share) and HumanoidMuscle.run (2048 = config 5's per-GPU share), each with its own kernel time, roofline,
parity sample against the fp64 oracle and the number of control steps the replay kernel ran. `--task` runs any of them as
the main leg instead (side measurements; the driver's default run is the A1 line).

The timed region holds inputs resident in HBM (state lives on the device); it is bracketed by a barrier +
device synchronisation on both sides, the maximum over ranks is taken. When the sustained block runs (--full, or
`--sustained`), `value` is the rate of the LONGER of the two per-step blocks (`--steps` and `--sustained`): a 20-step burst
reads several per cent faster than steady state, and the headline is the conservative one; the burst is reported beside it.
roofline: this path is not HBM-bound; `achieved` = algorithmic bytes per launch
(636 B per env-step incl. warm start x envs) / mean kernel duration measured with HIP events on the
library's own stream (lm_rollout returns it), against the 8 TB/s HBM peak — expect ~1e-4..1e-3. What binds is the
FP32 vector pipe at one wave per SIMD: `roofline.binding` carries the VALU issue fraction and the FP32 flop fraction
(counted flops per env-step from the committed profile's instruction counts and the kernel's static instruction mix).
cpu_baseline (--full): the fp64 C oracle restatement ("port") on every host core, on a bounded sample of the same workload
(rank 0, N=1 only).
"""

import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
FP32_VECTOR_PEAK_TFLOPS = 157.3          # MI355X_MICROARCH.md: 256 CUs x 128 FP32 FMA lanes x 2 flop x 2.4 GHz (packed FP32 counted)
SIMDS = 1024
CLOCK_GHZ = 2.4
PROFILE_ROUND = "r6"
TOL = dict(qpos=1e-4, qvel=1e-2)

# Tasks the bench can time but whose device-vs-oracle parity is not a gate: the robot's own golden rollouts are only partly reproducible
# (the line says `"supported": false` and carries the sample's verdict; exit code 0)
_H1 = ("UnitreeH1: 30 of the 58 rows of the reference's golden rollouts are not reproduced by ANY float64 restatement — 26 carry the flat cap of a "
       "hip-yaw cylinder on a mesh hull (MPR picks its support points among equals: ill-conditioned in float64, tests/test_oracle_golden.py), 4 depend "
       "on the engine's own hull graph; device and oracle inherit that class of states (DESIGN.md §2, §7)")
PARITY_REPORTED_NOT_GATING = {"UnitreeH1.walk": _H1, "UnitreeH1.run": _H1, "UnitreeH1.carry": _H1}

# BASELINE.json configs[2..4] as they run on ONE GPU (4 and 5 at their per-GPU share)
SIDE_CONFIGS = [
    dict(key="HumanoidTorque.run", task="HumanoidTorque.run", envs=4096, dr=False, baseline_config=3),
    dict(key="Atlas.walk.dr", task="Atlas.walk", envs=2048, dr=True, baseline_config=4),
    dict(key="HumanoidMuscle.run", task="HumanoidMuscle.run", envs=2048, dr=False, baseline_config=5),
]


def algorithmic_bytes_per_env_step(nq, nv, nu, nobs, na=0):
    # state in + state out + action + obs + reward + done, plus the solver warm start in/out and the muscle
    # activations in/out
    return 4 * (2 * nq + 2 * nv + nu + nobs + 2) + 8 * nv + 8 * na


def oracle_reaches(step_fn, q0, v0, qd, vd, probes=32, seed=0):
    """THE NEIGHBOUR RULE (round 6; the GPU suite's 4096-state test applies the same one): does the fp64 oracle ITSELF, for an input
    within one float32 ulp of the state (`probes` perturbations of 1.2e-7 relative), produce the DEVICE'S result (qd, vd) to within the
    tolerance? Then the device sits on the other branch of a switch the oracle takes too (a contact or a joint limit coming on within a
    hair of a substep boundary; MPR on a flat face, UnitreeH1's hip cylinders) and the state is set aside, not compared.
    Rounds 4-5 asked only that the oracle's own result move by more than the tolerance — which would have excused a device far off
    beside an oracle that merely moved. Returns (reached, nearest approach in units of the tolerance)."""
    rs = np.random.RandomState(seed)
    near = np.inf
    for _ in range(probes):
        q1 = q0 + 1.2e-7 * rs.uniform(-1, 1, q0.shape) * np.maximum(1.0, np.abs(q0))          # (as in _worker_oracle_steps of the GPU suite)
        v1 = v0 + 1.2e-7 * rs.uniform(-1, 1, v0.shape) * np.maximum(1.0, np.abs(v0))
        q2, v2 = step_fn(q1, v1)
        near = min(near, max(float(np.abs(q2 - qd).max()) / TOL["qpos"], float(np.abs(v2 - vd).max()) / TOL["qvel"]))
        if near <= 1.0:
            break
    return near <= 1.0, near


def parity_of_states(env, hm, q0, v0, act0, acts, what, dofprm=None):
    """Second half of the metric: qpos / qvel L-infinity of the device against the fp64 oracle port after ONE control step from the
    given states (float32 as the device holds them) under the given actions (checker only, outside every timed region).
    `dofprm`: per-environment joint damping / stiffness / frictionloss (domain randomisation): the device steps with them, the
    oracle is compiled from each state's own values."""
    from loco_mujoco_amd.backend import HipBatch
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    m = env._model
    nv, na, n = m.nv, getattr(m, "na", 0), len(q0)
    oracle = Oracle(pack_model(m))
    b = HipBatch(hm, n)
    b.set_state(q0, v0)
    if na:
        b.set_activation(act0)
    if dofprm is not None:
        b.set_dof_params(damping=dofprm["damping"], stiffness=dofprm["stiffness"], frictionloss=dofprm["frictionloss"])
    b.stats(reset=True)
    b.step(acts)
    q, v = b.get_state()
    st = b.stats()
    b.close()
    eq = ev = 0.0
    used = illc = nonfinite = 0
    for i in range(n):
        ctrl = np.zeros(m.nu)
        ctrl[env._action_indices] = env._preprocess_action(acts[i])
        qi, vi = q0[i].astype(np.float32).astype(np.float64), v0[i].astype(np.float32).astype(np.float64)
        ai = act0[i].astype(np.float32).astype(np.float64) if na else None
        if dofprm is not None:
            import copy
            mi = copy.copy(m)
            mi.dof_damping, mi.jnt_stiffness, mi.dof_frictionloss = (np.array(dofprm[k][i].astype(np.float32), float) for k in ("damping", "stiffness", "frictionloss"))
            oracle = Oracle(pack_model(mi))

        def step_fn(qa, va):
            if na:
                r = oracle.step_act(qa, va, ai, ctrl, 10)
                return r[0], r[1]
            r = oracle.step(qa, va, ctrl, 10)
            return r[0], r[1]
        if na:
            qo, vo, _, _, ost = oracle.step_act(qi, vi, ai, ctrl, 10)
        else:
            qo, vo, _, ost = oracle.step(qi, vi, ctrl, 10)
        if ost["unhandled_pairs"]:
            continue                                         # a collider-less geom within reach of the floor on either side
        if not (np.isfinite(qo).all() and np.isfinite(vo).all() and np.isfinite(q[i]).all() and np.isfinite(v[i]).all()):
            nonfinite += 1
            continue
        dq, dv = float(np.abs(q[i] - qo).max()), float(np.abs(v[i] - vo).max())
        if dq > TOL["qpos"] or dv > TOL["qvel"]:
            if oracle_reaches(step_fn, qi, vi, q[i].astype(np.float64), v[i].astype(np.float64), seed=i)[0]:
                illc += 1
                continue
        used += 1
        eq, ev = max(eq, dq), max(ev, dv)
    return dict(qpos_linf=eq, qvel_linf=ev, states=used, ill_conditioned=illc, non_finite=nonfinite, sample=what,
                replayed_env_steps=st.get("replayed_env_steps", 0.0), own_manifold_contacts=st.get("own_manifold_contacts", 0.0),
                against="fp64 oracle port (CPU), one control step = 10 substeps, same (qpos, qvel, act, ctrl); ill_conditioned = beyond the "
                        "tolerance AND the oracle itself produces the device's result within the tolerance for an input within one float32 ulp "
                        "(the neighbour rule, 32 probes; not compared)",
                tolerance=TOL, within_tolerance=bool(used > 0 and nonfinite == 0 and eq <= TOL["qpos"] and ev <= TOL["qvel"]))


def parity_sample(W, random_policy, n=64):
    """The parity sample of a leg: n states OF THE ROLLOUT THE LEG JUST TIMED (lm_get_state behind the timed block: walking, stumbling,
    folded and freshly restarted robots in the mixture the rate was measured on — rounds 1-5 took dataset states), one more control
    step from each on a fresh batch and in the oracle."""
    m = W.env._model
    q, v = W.b.get_state()
    act = W.b.get_activation() if getattr(m, "na", 0) else None
    rs = np.random.RandomState(5)
    pick = rs.choice(len(q), size=min(n, len(q)), replace=False)
    nu = len(W.env._action_indices)
    acts = rs.uniform(-1, 1, (len(pick), nu)) if random_policy else np.zeros((len(pick), nu))
    prm = None
    if W.dr:
        got = W.b.get_dof_params()
        prm = {k: got[k][pick] for k in ("damping", "stiffness", "frictionloss")}
    return parity_of_states(W.env, W.hm, q[pick], v[pick], None if act is None else act[pick], acts,
                            "%d states of the timed rollout (lm_get_state after the timed block)%s" % (len(pick), ", each with its own joint parameters" if W.dr else ""), prm)


def leg_rate(envs_per_gpu, world, steps, seconds):
    """env-steps/s of ONE timed block: every environment of every rank advances `steps` control steps in `seconds` (the maximum
    over the ranks). The only place a rate is computed — cumulative device counters never enter a rate (round 3 divided the
    cumulative count of all legs by the last leg's time)."""
    return dict(value=envs_per_gpu * world * steps / seconds, ms_per_step=1e3 * seconds / steps)


def baseline_metric():
    """The headline metric, spelled exactly as /root/repo/BASELINE.json spells it."""
    try:
        return json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    except Exception:
        return "env-steps/sec at 4096 envs/GPU; qpos L∞ vs CPU MuJoCo"


def host_cores():
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:                                     # a container's CPU quota, not the host's core count, is what can run at once
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, int(float(quota) / float(period) + 0.5)))
    except Exception:
        pass
    return cores


def cpu_baseline_all_cores(task, random_policy, dr, budget_s=8.0):
    """The same loop in one process per host core (fresh interpreters without torch / HIP), counts summed."""
    cores = host_cores()
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-worker", "--task", task, "--cpu-budget", str(budget_s)]
    if dr:
        cmd.append("--dr")
    if random_policy:
        cmd.append("--cpu-random-policy")
    t0 = time.perf_counter()
    procs = [subprocess.Popen(cmd + ["--cpu-seed", str(i)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL) for i in range(cores)]
    outs = [p.communicate()[0].decode().strip().splitlines() for p in procs]
    wall = time.perf_counter() - t0
    rates = [float(o[-1].split()[1]) for o in outs if o and o[-1].startswith("RATE")]
    if len(rates) < max(1, cores // 2):
        return None
    return dict(value=sum(rates), cores=len(rates), per_core=sum(rates) / len(rates), wall_s=wall, budget_s=budget_s)


def cpu_baseline(env, table, task, random_policy, budget_s=12.0, seed=0):
    """fp64 oracle restatement, one thread, same policy and initial-state distribution; bounded sample."""
    from oracle.model_blob import pack_model
    from oracle.pyoracle import Oracle
    m = env._model
    oracle = Oracle(pack_model(m))
    # timing: the same physics as the device simulates. The oracle's bookkeeping of geom pairs WITHOUT a collider (exact GJK
    # distances of convex hulls, test instrumentation that no simulator needs) stays out of the timed loop
    oracle.set_option("skip_pair_counter", 1)
    rs = np.random.RandomState(seed)
    nv, na = m.nv, getattr(m, "na", 0)
    qi = [m.jnt_id(n) for k, n, t in env.obs_helper.observation_spec[2:] if k.startswith("q_")]
    vi = [m.jnt_id(n) for k, n, t in env.obs_helper.observation_spec[2:] if k.startswith("dq_")]
    steps, t0, n_env = 0, time.perf_counter(), 0
    while time.perf_counter() - t0 < budget_s:
        row = table[rs.randint(0, len(table))]
        q, v, w, act = row[:nv].copy(), row[nv:2 * nv].copy(), np.zeros(nv), np.zeros(na)
        n_env += 1
        for _ in range(25):
            ctrl = np.zeros(m.nu)
            if random_policy:
                ctrl[env._action_indices] = env._preprocess_action(rs.uniform(-1, 1, len(env._action_indices)))
            if na:
                q, v, act, w, _ = oracle.step_act(q, v, act, ctrl, 10, w)
            else:
                q, v, w, _ = oracle.step(q, v, ctrl, 10, w)
            steps += 1
            if env._has_fallen(np.concatenate([q[qi], v[vi], row[2 * nv:]])):
                break
            if time.perf_counter() - t0 >= budget_s:
                break
    dt = time.perf_counter() - t0
    return dict(value=steps / dt, unit="env-steps/s", cores=1, kind="port",
                sample="%d control steps over %d episodes of %s (%s, until fallen or 25 steps), "
                       "fp64 C oracle restatement, 1 thread, %.1f s"
                       % (steps, n_env, task, "random action" if random_policy else "zero action", dt))


def make_env(task, dr):
    from loco_mujoco_amd import LocoEnv
    make_kw = {}
    if dr:
        assert task == "Atlas.walk", "--dr is BASELINE config 4 (Atlas.walk)"
        import loco_mujoco_amd
        make_kw = dict(disable_back_joint=False, domain_randomization_config=os.path.join(
            os.path.dirname(loco_mujoco_amd.__file__), "environments", "data", "atlas", "domain_randomization_atlas.yaml"))
    np.random.seed(0)
    return LocoEnv.make(task, debug=True, **make_kw)


class Workload:
    """One task on this rank's GPU: environment, model, batch with the bench's initial states and device-side restarts."""

    def __init__(self, task, n, dr, rank, world, device, no_pollers=False):
        from loco_mujoco_amd.backend import HipBatch, HipModel
        self.task, self.n, self.dr, self.world = task, n, dr, world
        self.default_task = task == "UnitreeA1.simple"
        self.action_mode = 0 if self.default_task else 1            # zero action (config 2) | device random policy (configs 3-5)
        self.env = env = make_env(task, dr)
        self.table = table = env._reset_table()
        self.hm = HipModel(env._chain_model(), device=device)
        self.b = b = HipBatch(self.hm, n)
        if no_pollers:
            b.set_replay(3)
        self.offset = offset = rank * n
        self.nv = nv = env._model.nv
        rs = np.random.RandomState(0)
        if self.default_task:
            traj, step = rs.randint(0, 3, n * world), rs.randint(0, 100, n * world)
            pick = traj * 100 + step
        else:
            pick = rs.randint(0, len(table), n * world)
        rows = table[pick[offset:offset + n]]
        b.set_reset_table(table, seed=0, global_env_offset=offset)
        b.set_auto_reset(True, horizon=env.info.horizon)
        b.set_state(rows[:, :nv], rows[:, nv:2 * nv])
        if rows.shape[1] > 2 * nv:
            b.set_goal(rows[:, 2 * nv:])
        if dr:
            d = env._domain_rand.sample(n)                       # first episode: host draw; restarts: device redraw
            b.set_dof_params(damping=d[0], stiffness=d[1], frictionloss=d[2])
            b.set_dof_randomization(env._domain_rand.spec)

    def label(self):
        return self.task + (" (back joints, joint-damping randomisation per episode)" if self.dr else "")

    def per_env_step_bytes(self):
        m = self.env._model
        return algorithmic_bytes_per_env_step(self.nv, self.nv, len(self.env._action_indices), self.b.nobs, getattr(m, "na", 0))

    def forwards_per_env_step(self):
        return 40 if self.env._model.integrator else 10             # RK4: four forward passes per substep

    def close(self):
        self.b.close()
        self.hm.close()


def timed_leg(W, coll, n_steps, seed, steps_per_launch=1):
    """One timed block: barrier + device sync, this rank's clock around exactly `n_steps` control steps + device sync, barrier.
    The clock stops BEFORE the closing barrier (a host-staged all-reduce): the maximum over the ranks of these per-rank times,
    taken at report time, is what a clock around both barriers would show less the collective's own latency. The device
    counters are reset first, so the returned statistics are this block's alone."""
    b = W.b

    def barrier():
        b.sync()                       # device synchronisation of this rank's stream ...
        coll.barrier()                 # ... then every rank has arrived (no-op for one rank)
        b.sync()
    b.stats(reset=True)
    barrier()
    t = time.perf_counter()
    stats = b.rollout(n_steps, action_mode=W.action_mode, seed=seed, steps_per_launch=steps_per_launch)
    b.sync()
    dt = time.perf_counter() - t
    barrier()
    return dt, stats


DUMP_LIMIT_BYTES = 64 * 10 ** 6
DUMP_STATS = ("env_steps", "episodes", "reward_sum", "nan_resets", "overflow_contacts", "unhandled_geoms", "self_contacts")


def dump_outputs(W, st, out_dir, rank, world):
    """`--dump-outputs DIR`: what a caller of the timed path (lm_rollout) holds after its last control step, as DIR/<name>.npy —
    qpos / qvel [envs, nq / nv] (float32 as the device keeps them), act [envs, na] (muscle tasks), flags [envs] (lm_get_flags of the
    last control step, as float32) and stats (float64: the block's counters in the order of DUMP_STATS; its kernel time is left
    out). Above 64 MB in all (over the ranks), a fixed sample of environments (RandomState(0), sorted ids in env_index.npy) is written instead.
    With more than one rank every rank writes its own share as <name>.rank<r>.npy."""
    b = W.b
    q, v = b.get_state()
    arrays = {"qpos": q, "qvel": v}
    if b.na:
        arrays["act"] = b.get_activation()
    arrays["flags"] = b.flags().astype(np.float32)
    per_env = sum(a.nbytes for a in arrays.values()) / W.n
    limit = DUMP_LIMIT_BYTES // world - 4096                   # every rank its share; 4 KB for the .npy headers and the stats
    if W.n * per_env > limit:
        keep = int(limit // (per_env + 8))
        idx = np.sort(np.random.RandomState(0).choice(W.n, keep, replace=False))
        arrays = {k: a[idx] for k, a in arrays.items()}
        arrays["env_index"] = (idx + W.offset).astype(np.float64)
    arrays["stats"] = np.array([st[k] for k in DUMP_STATS], dtype=np.float64)
    os.makedirs(out_dir, exist_ok=True)
    suffix = ".rank%d" % rank if world > 1 else ""
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + suffix + ".npy"), np.ascontiguousarray(a))


def lib_sha16():
    from loco_mujoco_amd import backend as _backend
    return hashlib.sha256(open(_backend.LIB_PATH, "rb").read()).hexdigest()[:16]


def profile_tag(W):
    return PROFILE_ROUND if (W.default_task and W.n == 4096) else "%s_%s%s%s" % (PROFILE_ROUND, W.task, ".dr" if W.dr else "", "" if W.n == 4096 else str(W.n))


def roofline_block(W, kernel_ms_per_launch, lib_sha):
    """`roofline` of one workload: algorithmic bytes per launch / mean kernel time (HIP events on the library's stream) against
    the HBM peak (the contract's figure), the committed profile's counter traffic when that profile was taken on THIS build, and
    `binding`: the resource that does bind — FP32 VALU issue at one wave per SIMD."""
    per_env_step = W.per_env_step_bytes()
    bytes_per_launch = per_env_step * W.n
    launch_s = kernel_ms_per_launch * 1e-3
    achieved = bytes_per_launch / launch_s / 1e9
    tag = profile_tag(W)
    prof = os.path.join(ROOT, "profiles", tag + "_pmc.json")
    prof_name = "profiles/%s_pmc.json" % tag
    note = "no committed profile for this workload"
    traffic = None
    binding = None
    # counters of the committed profile (tools/probes/prof_run.sh: the same command under rocprofv3, separate --pmc passes).
    # They are only quoted when the profile was taken on THIS build of the library (sha256 of liblocohip.so stamped into it):
    # after a kernel change they go stale, and stale numbers are dropped (null) rather than reported.
    if os.path.exists(prof):
        pj = json.load(open(prof))
        if pj.get("lib_sha16") != lib_sha:
            note = "%s was taken on another build of liblocohip.so (%s, this one is %s): counters not quoted" % (prof_name, pj.get("lib_sha16"), lib_sha)
        else:
            note = "%s, taken on this build (liblocohip.so sha256[:16] = %s)" % (prof_name, lib_sha)
            try:
                pmc = pj["pmc"]
                # separate --pmc passes; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950)
                traffic = pmc["FETCH_SIZE"]["bytes_per_dispatch_corrected_x2"] + pmc["WRITE_SIZE"]["bytes_per_dispatch"]
                # One wave64 VALU instruction holds a 16-lane SIMD for 4 cycles; SQ_WAVE_CYCLES counts in units of 4 cycles (it
                # reproduces the mean wave time measured with s_memtime). VALU issue fraction of the chip = VALU wave-instructions
                # x 4 cycles / (SIMDs x launch cycles), with the launch time of the profiled run itself.
                prof_ns = pj["duration_ns"]["avg"]
                valu = pmc["SQ_INSTS_VALU"]["per_dispatch"]
                issue = valu * 4.0 / (SIMDS * prof_ns * CLOCK_GHZ)
                binding = dict(resource="fp32-valu-issue", valu_issue_frac=issue,
                               valu_insts_per_wave=valu / pmc["SQ_WAVES"]["per_dispatch"],
                               valu_busy_frac_of_wave_time=valu / pmc["SQ_WAVE_CYCLES"]["per_dispatch"],
                               mean_wave_time_over_launch_time=4.0 * pmc["SQ_WAVE_CYCLES"]["per_dispatch"] / pmc["SQ_WAVES"]["per_dispatch"] / (prof_ns * CLOCK_GHZ),
                               note=prof_name + "; %.1f GHz assumed; issue fraction = SQ_INSTS_VALU x 4 cycles / (%d SIMDs x launch cycles)" % (CLOCK_GHZ, SIMDS))
                mix = pj.get("valu_mix")           # static instruction mix of the kernel (tools/valu_mix.py): flops per VALU lane-op
                if mix:
                    # counted flops: every VALU wave-instruction executes 64 lane-ops; the replicated layout runs each environment on
                    # 4 replica quads, so the USEFUL share is 1/replicas of what the pipe executes (both are reported)
                    executed = valu * 64.0 * mix["flops_per_valu_lane_op"]
                    reps = float(mix.get("replicas", 4))
                    binding.update(flops_per_env_step_executed=executed / W.n, flops_per_env_step_distinct=executed / reps / W.n,
                                   fp32_tflops_executed=executed / (prof_ns * 1e-9) / 1e12,
                                   fp32_frac_of_vector_peak=executed / (prof_ns * 1e-9) / 1e12 / FP32_VECTOR_PEAK_TFLOPS,
                                   fp32_peak_tflops=FP32_VECTOR_PEAK_TFLOPS,
                                   flops_note="flops = SQ_INSTS_VALU x 64 lanes x %.3f flops per VALU lane-op (static mix of the kernel's ISA: "
                                              "fma/mac/pk_fma 2 per lane and element, add/mul/trans 1, moves and integer 0; %s); "
                                              "distinct = executed / %d replicas" % (mix["flops_per_valu_lane_op"], mix.get("kernel", "?"), int(reps)))
            except Exception as e:      # noqa: BLE001 - a malformed profile must not take the bench line down
                note += " (unreadable: %s)" % e
    out = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
           "hbm_frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "algorithmic_bytes_per_launch": bytes_per_launch, "algorithmic_bytes_per_env_step": per_env_step,
           "kernel_ms_per_launch": kernel_ms_per_launch, "profile": note, "lib_sha16": lib_sha,
           "note": "the HBM figure is the contract's; it does NOT bind (SURVEY.md 8d: %d algorithmic B per env-step). What binds is "
                   "`binding`: FP32 VALU issue at one wave per SIMD. traffic = PMC bytes per launch from the committed profile (same "
                   "command, separate rocprofv3 --pmc passes), null when that profile is not of this build" % per_env_step}
    if binding is not None:
        # what binds is named as the bound, with ITS fraction as `frac` (round-5 review); the contract's HBM figure stays beside it
        # (`achieved` / `peak` / `unit` / `hbm_frac`: algorithmic bytes per launch over the kernel time against the 8 TB/s peak)
        out["binding"] = binding
        out["bound"] = "fp32-valu-issue"
        out["frac"] = binding["valu_issue_frac"]
    return out


def side_config(cfg, rank, device, steps, warmup, lib_sha, with_cpu):
    """A short leg of one of the other BASELINE configs on this GPU: `warmup` + `steps` per-step launches, kernel time by HIP
    events, roofline, parity sample, the replay kernel's share. Runs after (and outside) the headline's timed region."""
    from loco_mujoco_amd.utils.collective import Collective
    t_all = time.perf_counter()
    coll1 = Collective(backend="tcp", rank=0, world=1)
    W = Workload(cfg["task"], cfg["envs"], cfg["dr"], 0, 1, device)
    W.b.rollout(warmup, action_mode=W.action_mode, seed=11)
    dt, st = timed_leg(W, coll1, steps, 12)
    assert abs(st["env_steps"] - W.n * steps) < 0.5, (st["env_steps"], W.n, steps)
    rate = leg_rate(W.n, 1, steps, dt)
    out = {"baseline_config": cfg["baseline_config"],
           "workload": "%s, %d envs, random-policy rollout, device-side auto-reset (horizon 1000), 10 physics substeps per env-step" % (W.label(), W.n),
           "envs": W.n, "steps": steps, "warmup": warmup,
           "value": rate["value"], "unit": "env-steps/s", "ms_per_step": rate["ms_per_step"], "kernel_ms": st["kernel_ms"] / steps,
           "roofline": roofline_block(W, st["kernel_ms"] / steps, lib_sha),
           "stats": {"overflow_contacts": st["overflow_contacts"], "unhandled_geom_substeps": st["unhandled_geoms"],
                     "self_proximity": st["self_proximity"], "self_contacts": st["self_contacts"],
                     "own_manifold_contacts": st.get("own_manifold_contacts", 0.0),
                     "replayed_env_steps": st.get("replayed_env_steps", 0.0), "episodes": st["episodes"], "nan_resets": st["nan_resets"],
                     "newton_iters_per_forward_pass": st["solver_iters"] / max(st["env_steps"] * W.forwards_per_env_step(), 1)}}
    out["parity"] = parity_sample(W, True)
    # beside `value` (per-step launches: what a policy in the loop gets), never as it: the same rollout with 25 control steps per launch
    # (lm_rollout_fused, bitwise the same states: no device-wide join behind every control step, so a launch no longer ends with the
    # single hardest robot of EVERY step — the humanoids' per-step launches wait 2-3 x the mean wave's time for it)
    try:
        W.b.rollout(25, action_mode=W.action_mode, seed=13, steps_per_launch=25)
        nf = max(25, (steps // 25) * 25)
        dtf, stf = timed_leg(W, coll1, nf, 14, steps_per_launch=25)
        fr = leg_rate(W.n, 1, nf, dtf)
        out["rollout_fused"] = {"steps_per_launch": 25, "steps": nf, "value": fr["value"], "unit": "env-steps/s", "ms_per_step": fr["ms_per_step"],
                                "overflow_contacts": stf["overflow_contacts"], "replayed_env_steps": stf.get("replayed_env_steps", 0.0)}
    except Exception as e:      # noqa: BLE001 - reported in the line
        out["rollout_fused"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if with_cpu:
        one = cpu_baseline(W.env, W.table, W.task, True, budget_s=2.0)
        out["cpu_baseline"] = dict(value=one["value"], unit="env-steps/s", cores=1, kind="port", sample=one["sample"])
    W.close()
    out["wall_s"] = time.perf_counter() - t_all
    # the side legs ride at the END of a line whose head carries the same explanations once (`roofline.note`, `parity.against`): they keep
    # their numbers and drop the prose, so that the whole line stays within what a log tail of a few KB shows
    for blk, drop in (("roofline", ("note", "kernel")), ("parity", ("against", "tolerance", "sample"))):
        for k in drop:
            out[blk].pop(k, None)
    if out["roofline"].get("binding"):
        out["roofline"]["binding"].pop("note", None)
    if "cpu_baseline" in out:
        out["cpu_baseline"]["sample"] = out["cpu_baseline"]["sample"][:60]
    return out


def python_surface_leg(device, n, steps, warmup):
    """The surface the reference's users call (reference gymnasium.py:47-65 -> LocoEnv.step): `steps` calls of LocoEnv.step() at
    n_envs = n with numpy actions in and numpy observation / reward / absorbing out — H2D of the action, the launch, D2H of the results,
    dtype conversion — timed on the host clock. Reported beside `value` (which is the policy-free rollout with everything resident)."""
    from loco_mujoco_amd import LocoEnv
    np.random.seed(0)
    env = LocoEnv.make("UnitreeA1.simple", debug=True, n_envs=n, device=device)
    env.reset()
    env.enable_auto_reset(seed=0)
    act = np.zeros((n, 12))
    for _ in range(warmup):
        env.step(act)
    env.backend.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        obs, rew, absorbing, info = env.step(act)
    dt = time.perf_counter() - t0
    assert obs.shape == (n, 37) and obs.dtype == np.float64 and rew.shape == (n,) and absorbing.shape == (n,)
    k0 = env.backend.stats()["kernel_ms"] if hasattr(env.backend, "stats") else None
    out = dict(envs=n, steps=steps, warmup=warmup, ms_per_step=1e3 * dt / steps, value=n * steps / dt, unit="env-steps/s",
               obs_dtype=str(obs.dtype), action_dtype=str(act.dtype),
               note="LocoEnv.step(numpy float64 action) -> (obs float64, reward float64, absorbing bool, info) through lm_step_pinned: the action "
                    "is converted into a pinned staging buffer the step kernel reads itself, a conversion kernel writes float64 observation / "
                    "reward / done straight into a pinned result set (a ring of 4: the arrays returned are views, intact for the next three "
                    "calls; copy_outputs=True returns fresh arrays) — no copy queued on either side of the launch; UnitreeA1.simple, zero "
                    "action, device-side auto-reset")
    del k0
    return out


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks (one process per GPU) with the environment a launcher would
    set, rendezvous on 127.0.0.1. Rank 0 prints the line. Fails loudly where the node cannot give every rank a GPU of its own."""
    n = args.gpus
    if not (args.share_gpu or args.plumbing_only):
        from loco_mujoco_amd import backend as _be
        have = _be.load_library().lm_device_count()
        if have < n:
            print("bench: --gpus %d asked for, this node has %d GPU(s): cannot give every rank a GPU of its own "
                  "(--share-gpu runs the multi-rank control flow on GPU 0 for testing)" % (n, have), file=sys.stderr)
            sys.exit(2)
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env))
    rcs = [p.wait() for p in procs]
    sys.exit(max(abs(rc) for rc in rcs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--envs-per-gpu", type=int, default=4096)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--task", default="UnitreeA1.simple")
    ap.add_argument("--dr", action="store_true", help="Atlas.walk only: BASELINE config 4 — back joints kept, joint damping "
                    "redrawn per episode from the reference's domain_randomization_atlas.yaml")
    ap.add_argument("--cpu-worker", action="store_true", help=argparse.SUPPRESS)       # one process of the all-cores CPU baseline
    ap.add_argument("--cpu-budget", type=float, default=8.0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-seed", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cpu-random-policy", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--share-gpu", action="store_true", help="testing only: run all ranks on GPU 0 with the socket reduction "
                    "(checks the multi-rank control flow on a one-GPU box; the numbers mean nothing)")
    ap.add_argument("--plumbing-only", action="store_true", help=argparse.SUPPRESS)     # tests: ranks, rendezvous and the reduction only (no GPU work)
    ap.add_argument("--dump-states", default=None, help=argparse.SUPPRESS)              # tests: <prefix>.rank<r>.npz with the final states
    ap.add_argument("--require-rccl", action="store_true", help="exit non-zero instead of reducing the metrics over TCP sockets when the RCCL "
                    "communicator does not come up (N > 1). The DEFAULT whenever WORLD_SIZE > 1 and every rank has a GPU of its own")
    ap.add_argument("--allow-tcp-fallback", action="store_true", help="N > 1: let the metric reduction fall back to the rendezvous sockets "
                    "when the RCCL communicator does not come up (the bench line names the transport in config.collective)")
    ap.add_argument("--full", action="store_true", help="everything beside the headline as well: the sustained block, the fused-rollout "
                    "leg, the parity sample against the fp64 oracle (exit 3 beyond the tolerance), the CPU baseline, the python_surface "
                    "leg and the other BASELINE configs. Without it a run sets up, warms up, times the --steps block and prints the line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the --steps block, write what it computed (final "
                    "qpos / qvel, muscle activations, validity flags, the block's counters) as DIR/<name>.npy for output-for-output "
                    "comparisons of two builds")
    ap.add_argument("--sustained", type=int, default=None, help="control steps of the sustained leg (per-step launches, one "
                    "timed block of at least this many steps; 0 = skip; skipped when --steps already covers it). When it runs, "
                    "`value` is ITS rate (the conservative one) and the --steps block is reported as `burst`. Default: 200 with --full, else 0")
    ap.add_argument("--no-pollers", action="store_true", help="profiling runs (rocprofv3 runs one kernel at a time): the replay kernel only as the "
                    "pass behind the regular launch, no polling workgroups beside it (lm_batch_set_replay(3))")
    ap.add_argument("--fuse", type=int, default=None, help="control steps per launch of the extra fused-rollout leg (0/1 = skip). "
                    "Default: 25 with --full, else 0")
    ap.add_argument("--configs", default=None, choices=["auto", "on", "off"], help="short legs of the other BASELINE configs "
                    "(HumanoidTorque.run, Atlas.walk --dr 2048, HumanoidMuscle.run 2048) under the `configs` key; auto = one rank, default task. "
                    "Default: auto with --full, else off")
    ap.add_argument("--surface-steps", type=int, default=None, help="calls of LocoEnv.step() of the `python_surface` leg (0 = skip; one rank, "
                    "default task). Default: 200 with --full, else 0")
    ap.add_argument("--config-steps", type=int, default=60)
    ap.add_argument("--config-warmup", type=int, default=20)
    args = ap.parse_args()
    # the legs beside the headline: on with --full, off in a plain run; an explicit option wins either way
    for name, full_default, plain_default in (("sustained", 200, 0), ("fuse", 25, 0), ("configs", "auto", "off"), ("surface_steps", 200, 0)):
        if getattr(args, name) is None:
            setattr(args, name, full_default if args.full else plain_default)
    # the parity sample and the CPU baseline: --full only (--no-cpu-baseline drops them there too)
    checks = args.full and not args.no_cpu_baseline

    if args.cpu_worker:
        env = make_env(args.task, args.dr)
        r = cpu_baseline(env, env._reset_table(), args.task, args.cpu_random_policy, args.cpu_budget, seed=args.cpu_seed)
        print("RATE %.3f" % r["value"])
        return

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args, sys.argv[1:])                            # (does not return)

    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world != args.gpus:
        # under a launcher the number of ranks and --gpus must say the same thing: a line that reports n_gpus = 1 for a run that was
        # asked for 8 (or the reverse) is worse than no line
        print("bench: --gpus %d but WORLD_SIZE=%d: launch one rank per GPU (python -m torch.distributed.run --nproc-per-node %d ... "
              "bench.py --gpus %d) or run `python bench.py --gpus %d` without a launcher" % (args.gpus, world, args.gpus, args.gpus, args.gpus), file=sys.stderr)
        sys.exit(2)
    # the only collective of the path: the metric all-reduce at report time — ncclAllReduce on librccl.so through ctypes
    # (loco_mujoco_amd/utils/collective.py; no PyTorch anywhere in this file). --share-gpu: all ranks on GPU 0 and the
    # reduction over the rendezvous sockets (RCCL refuses two ranks on one device)
    from loco_mujoco_amd.utils.collective import Collective, MAX, SUM
    if args.share_gpu:
        local_rank = 0
    if args.plumbing_only:
        coll = Collective(backend="tcp", rank=rank, world=world, device=local_rank)
        seen = coll.all_reduce(np.array([1.0, float(rank)]), SUM)
        coll.barrier()
        coll.close()
        if rank == 0:
            print(json.dumps({"plumbing_only": True, "n_gpus": world, "ranks_counted": int(seen[0]), "rank_sum": seen[1], "collective": coll.backend}))
        return
    from loco_mujoco_amd import backend as _be
    # one rank per GPU on a node that has a GPU for every rank: the reduction IS RCCL or the run fails (no silent socket fallback)
    own_gpu = world > 1 and not args.share_gpu and _be.load_library().lm_device_count() >= world
    require_rccl = (args.require_rccl or (own_gpu and not args.allow_tcp_fallback)) and not args.share_gpu
    coll = Collective(backend="tcp" if args.share_gpu else "rccl", rank=rank, world=world, device=local_rank,
                      require_rccl=require_rccl)
    ranks_rccl = coll.comm_count()

    n = args.envs_per_gpu
    W = Workload(args.task, n, args.dr, rank, world, local_rank, no_pollers=args.no_pollers)
    b, env = W.b, W.env

    b.rollout(args.warmup, action_mode=W.action_mode, seed=11)
    elapsed, st = timed_leg(W, coll, args.steps, 12)
    if args.dump_outputs:                                     # what the --steps block computed, before any other leg moves the state
        dump_outputs(W, st, args.dump_outputs, rank, world)

    # extra leg, reported beside `value`, never as `value`: the same number of control steps with --fuse steps per launch
    # (lm_rollout_fused: no device-wide join between control steps; bitwise the same results). Continues from the state
    # the timed region left, so it runs the same mixture of walking and collapsing robots.
    fused = None
    if args.fuse > 1:
        b.rollout(args.fuse, action_mode=W.action_mode, seed=13, steps_per_launch=args.fuse)
        dtf, stf = timed_leg(W, coll, args.steps, 14, steps_per_launch=args.fuse)
        fused = [dtf, stf["kernel_ms"]]

    # the sustained block of per-step launches (thermal / clock steady state rather than a short burst); the timed region above
    # already is one when --steps >= --sustained
    sustained = None
    if args.sustained > args.steps:
        dts, sts = timed_leg(W, coll, args.sustained, 15)
        sustained = [dts, sts["env_steps"], sts["kernel_ms"], sts]

    vals = np.array([elapsed, st["env_steps"], st["episodes"], st["reward_sum"], st["nan_resets"],
                     st["overflow_contacts"], st["unhandled_geoms"], st["solver_iters"], st["kernel_ms"],
                     fused[0] if fused is not None else 0.0, st["self_proximity"], st["self_contacts"],
                     sustained[0] if sustained is not None else 0.0, sustained[1] if sustained is not None else 0.0,
                     st.get("replayed_env_steps", 0.0), sustained[2] if sustained is not None else 0.0,
                     st.get("own_manifold_contacts", 0.0)], dtype=np.float64)
    tmax = coll.all_reduce(vals, MAX)
    vals = coll.all_reduce(vals, SUM)
    elapsed, kernel_ms, fused_elapsed = float(tmax[0]), float(tmax[8]), float(tmax[9])
    if args.dump_states:                                      # tests: this rank's final states, to compare partitions
        q_fin, v_fin = b.get_state()
        np.savez(args.dump_states + ".rank%d.npz" % rank, qpos=q_fin, qvel=v_fin, offset=W.offset)
    coll.close()                                              # every collective happens before the non-zero ranks leave
    if rank != 0:
        return
    env_steps = vals[1]
    burst = leg_rate(n, world, args.steps, elapsed)
    # the device's own count of this block (counters reset right before it) must be the same number of env-steps
    assert abs(env_steps - n * world * args.steps) < 0.5, (env_steps, n, world, args.steps)
    # `value`: the longer per-step block. With the driver's --steps 20 that is the sustained block of 200 launches — the burst reads
    # several per cent faster (clocks) and is reported beside it
    if sustained is not None and tmax[12] > 0:
        assert abs(vals[13] - n * world * args.sustained) < 0.5, (vals[13], n, world, args.sustained)    # this block's own count
        main_leg = leg_rate(n, world, args.sustained, float(tmax[12]))
        main_steps, main_kernel_ms = args.sustained, float(tmax[15])
    else:
        main_leg, main_steps, main_kernel_ms = burst, args.steps, kernel_ms
    value = main_leg["value"]
    lib_sha = lib_sha16()
    roof = roofline_block(W, main_kernel_ms / main_steps, lib_sha)
    roof["kernel"] = "step_kernel<3 links,6 slots,Euler,elliptic,self-collisions,4 replicas>" if W.default_task else "step_kernel"
    out = {
        "metric": baseline_metric(),
        # `steps` = the launches `value` / `ms_per_step` were measured over (the driver's --steps block is `burst`, with its own `steps`)
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": main_steps, "warmup": args.warmup,
        "ms_per_step": main_leg["ms_per_step"], "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "timed_steps": main_steps,
        "config": {"workload": "%s, %d envs/GPU, %s rollout, device-side auto-reset "
                               "(horizon 1000), 10 physics substeps per env-step"
                               % (W.label(), n, "zero-action" if W.default_task else "random-policy"),
                   "envs_per_gpu": n, "global_envs": n * world, "parallelism": "env-sharded x%d" % world,
                   "collective": {"none": "none (one rank)", "rccl": "ncclAllReduce (RCCL) of 17 doubles at report time",
                                  "tcp": "socket reduction of 17 doubles at report time (RCCL not used)"}[coll.backend],
                   "ranks_seen_by_rccl": ranks_rccl,
                   "value_is": ("the sustained block: %d per-step launches after the --steps block (same policy, same state mixture); the --steps "
                                "block is `burst`" % args.sustained) if main_steps != args.steps else
                               "the --steps block" + (" (it covers --sustained)" if args.sustained else "")},
        "roofline": roof,
        "stats": {"episodes": vals[2], "mean_reward": vals[3] / max(env_steps, 1), "nan_resets": vals[4],
                  "overflow_contacts": vals[5], "unhandled_geom_substeps": vals[6],
                  # where the device left its validated collision model (all ranks): forward passes x geom pairs of the robot
                  # without a pair collider (box / cylinder) within the margin, and self-contacts it did simulate
                  "self_proximity": vals[10], "self_contacts": vals[11],
                  # of those: contacts of box-box / capsule-box pairs, whose manifold construction is the library's own (lm_core.h nat_*)
                  "own_manifold_contacts": vals[16],
                  # control steps that left the regular kernel's capacity (contact slots, pair lists) and were run by the replay kernel
                  "replayed_env_steps": vals[14],
                  "newton_iters_per_forward_pass": vals[7] / max(env_steps * W.forwards_per_env_step(), 1),
                  "physics_substeps_per_s": 10 * value,
                  "note": "counters of the --steps block"},
        "burst": {"steps": args.steps, "value": burst["value"], "unit": "env-steps/s", "ms_per_step": burst["ms_per_step"],
                  "kernel_ms_per_launch": kernel_ms / args.steps,
                  "note": "the --steps block (the first timed block after the warm-up)"},
    }
    if fused is not None:
        fl = leg_rate(n, world, args.steps, fused_elapsed)
        out["rollout_fused"] = {"steps_per_launch": args.fuse, "value": fl["value"], "unit": "env-steps/s",
                                "ms_per_step": fl["ms_per_step"],
                                "note": "policy-free rollout with %d control steps per launch (lm_rollout_fused): every "
                                        "environment advances on its own, results bitwise those of single-step launches; "
                                        "a policy in the loop gets `value`" % args.fuse}
    if args.sustained > 0:
        out["sustained"] = {"steps": main_steps, "value": value, "unit": "env-steps/s", "ms_per_step": main_leg["ms_per_step"],
                            "note": "= `value`"}
    if world == 1 and checks:
        out["parity"] = parity_sample(W, not W.default_task)
        one = cpu_baseline(env, W.table, args.task, not W.default_task, budget_s=6.0)
        allc = cpu_baseline_all_cores(args.task, not W.default_task, args.dr)
        # reported baseline = every host core running the fp64 port (falls back to the single-core sample)
        out["cpu_baseline"] = dict(one)
        out["cpu_baseline"]["single_core"] = one["value"]
        if allc is not None:
            out["cpu_baseline"].update(value=allc["value"], cores=allc["cores"],
                                       sample=one["sample"] + "; value = the same loop in %d processes (one per host core) for "
                                       "%.0f s each, counts summed (%.0f env-steps/s per process under full load; process count = CPU affinity "
                                       "capped by the cgroup quota)"
                                       % (allc["cores"], allc["budget_s"], allc["per_core"]))
        out["cpu_baseline"]["gpu_over_cpu"] = value / out["cpu_baseline"]["value"]
    # the other BASELINE configs, short legs (after the headline's timed legs and outside them)
    want_configs = args.configs == "on" or (args.configs == "auto" and world == 1 and W.default_task and n == 4096)
    want_surface = args.surface_steps > 0 and world == 1 and W.default_task and not args.no_cpu_baseline
    parity_ok = "parity" not in out or out["parity"]["within_tolerance"]
    if args.task in PARITY_REPORTED_NOT_GATING and "parity" in out:
        # a robot whose parity is NOT pinned: the sample is reported with its verdict, the run does not fail on it
        out["parity"]["gate"] = "reported, not gating: " + PARITY_REPORTED_NOT_GATING[args.task]
        out["supported"] = False
        parity_ok = True
    if want_surface:
        W.close()
        try:
            out["python_surface"] = python_surface_leg(local_rank, n, args.surface_steps, 20)
            out["python_surface"]["over_kernel_rate"] = out["python_surface"]["ms_per_step"] / (main_kernel_ms / main_steps)
        except Exception as e:      # noqa: BLE001 - reported in the line
            out["python_surface"] = {"error": "%s: %s" % (type(e).__name__, e)}
    if want_configs and world == 1:
        if not want_surface:
            W.close()
        out["configs"] = {}
        for cfg in SIDE_CONFIGS:
            try:
                res = side_config(cfg, rank, local_rank, args.config_steps, args.config_warmup, lib_sha, with_cpu=checks)
            except Exception as e:      # noqa: BLE001 - a failing side leg is reported in the line, and fails the run
                res = {"error": "%s: %s" % (type(e).__name__, e)}
                parity_ok = False
            out["configs"][cfg["key"]] = res
            if "parity" in res and not res["parity"]["within_tolerance"]:
                parity_ok = False
        # the last few hundred bytes of the line: every leg's rate again, so that a log TAIL shows them whatever the line's length
        out["summary"] = {"value": out["value"], "ms_per_step": out["ms_per_step"], "parity_within_tolerance": out.get("parity", {}).get("within_tolerance"),
                          "python_surface_over_kernel_rate": (out.get("python_surface") or {}).get("over_kernel_rate"),
                          "configs": {k: ({"error": v["error"]} if "error" in v else
                                          {"value": v["value"], "ms_per_step": v["ms_per_step"], "parity_within_tolerance": v["parity"]["within_tolerance"],
                                           "overflow_contacts": v["stats"]["overflow_contacts"], "roofline_frac": v["roofline"].get("frac"), "traffic": v["roofline"].get("traffic")})
                                      for k, v in out["configs"].items()}}
    print(json.dumps(out))
    if not parity_ok:
        # the second half of the metric failed somewhere: the line above says where ("within_tolerance": false), and so does the exit code
        print("bench: device vs fp64 oracle beyond the stated tolerance (qpos %.0e, qvel %.0e) in: %s"
              % (TOL["qpos"], TOL["qvel"],
                 ", ".join([args.task] * (not out.get("parity", {"within_tolerance": True})["within_tolerance"]) +
                           [k for k, v in out.get("configs", {}).items() if "error" in v or not v["parity"]["within_tolerance"]])), file=sys.stderr)
        sys.exit(3)


if __name__ == "__main__":
    main()
