"""Closed-loop rollouts under a 2 x 256 tanh MLP policy at 4096 environments: ms per control step of
  (a) rollout_policy, 25 control steps per launch (the policy inside the fused kernel),
  (b) rollout_policy, 1 control step per launch (policy_kernel + the ordinary step kernel),
  (c) the same torch module driving step_device in a loop on one stream (a handful of torch launches + one step launch per step),
  (d) as (a) with the input normaliser on (set_policy_obs_norm) at mean 0, inv_std 1 and a clip no input reaches: the subtraction, the
      multiplication and the selects run, the actions stay bitwise those of (a) — a normaliser with real moments changes the actions, the
      states the robots get into and with them the cost of the STEP, for every leg that shares the batch,
for UnitreeA1.simple and HumanoidTorque.run. Device-side restarts at the task's horizon, 50 warm-up steps, then `steps` control steps
per repeat timed by HIP events on the caller's stream, `repeats` repeats per leg, the legs alternating. Noise on (log_std = -1): (c)
draws its own normal numbers with torch. Usage: policy_rollout_time.py [steps] [repeats] [n_envs]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loco_mujoco_amd import LocoEnv  # noqa: E402
from loco_mujoco_amd.backend import MlpPolicy, ObsNorm  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
K = 25
dev = torch.device("cuda", 0)

for task in ("UnitreeA1.simple", "HumanoidTorque.run"):
    np.random.seed(0)
    env = LocoEnv.make(task, debug=True, n_envs=n)
    env.reset()
    env.enable_auto_reset(seed=0)
    b = env.backend
    torch.manual_seed(0)
    seq = torch.nn.Sequential(torch.nn.Linear(b.nobs, 256), torch.nn.Tanh(), torch.nn.Linear(256, 256), torch.nn.Tanh(), torch.nn.Linear(256, b.nu)).to(dev)
    log_std = torch.full((b.nu,), -1.0, device=dev)
    policy = MlpPolicy.from_torch(seq, log_std)
    acts = torch.empty((K, n, b.nu), device=dev)
    obs = torch.empty((K, n, b.nobs), device=dev)
    rew = torch.empty((K, n), device=dev)
    done = torch.empty((K, n), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    s = stream.cuda_stream
    b.step_device(obs=obs[K - 1], stream=s, sync=False)

    def leg_fused(count, spl):
        for i in range(0, count, K):
            b.rollout_policy(policy, K, obs0=obs[K - 1], actions=acts, obs=obs, reward=rew, done=done, steps_per_launch=spl,
                             noise_seed=i, stream=s, sync=False)

    def leg_loop(count):
        std = log_std.exp()
        o = obs[K - 1]
        with torch.no_grad():
            for i in range(count):
                mean = seq(o)
                a = torch.addcmul(mean, std, torch.randn_like(mean))
                b.step_device(a, obs[i % K], rew[i % K], done[i % K], stream=s, sync=False)
                o = obs[i % K]
        if (count % K) != 0:
            obs[K - 1].copy_(o)

    norm = ObsNorm(b.nobs, dev, clip=3.0e38)              # never updated: mean 0, inv_std 1

    def leg_normalised(count):
        leg_fused(count, K)

    legs = (("(a) rollout_policy, 25 steps per launch", lambda c: leg_fused(c, K)), ("(b) rollout_policy, 1 step per launch", lambda c: leg_fused(c, 1)),
            ("(c) torch module + step_device loop", leg_loop), ("(d) as (a), input normaliser on", leg_normalised))

    def prepare(leg):
        # the setting waits for the batch's launches on the host: outside the timed span
        if leg is leg_normalised:
            b.set_policy_obs_norm(norm.mean, norm.inv_std, norm.clip)
        else:
            b.set_policy_obs_norm(None, None)

    times = {name: [] for name, _ in legs}
    for name, leg in legs:
        prepare(leg)
        leg(50)
    torch.cuda.synchronize(dev)
    for _ in range(repeats):
        for name, leg in legs:
            prepare(leg)
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            leg(steps)
            e1.record(stream)
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / steps)
    b.set_policy_obs_norm(None, None)
    for name, _ in legs:
        t = sorted(times[name])
        print("%s n=%d %s: ms per control step %s, median %.4f, spread %.4f" % (task, n, name, ", ".join("%.4f" % v for v in times[name]),
                                                                               t[len(t) // 2], t[-1] - t[0]), flush=True)
    st = b.stats(reset=True)
    print("%s: %d env-steps, %d episodes, %d replayed env-steps in all legs" % (task, st["env_steps"], st["episodes"], st["replayed_env_steps"]), flush=True)
