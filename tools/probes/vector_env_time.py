"""What the vector environment's per-step bookkeeping costs: UnitreeA1.simple at 4096 environments under the README's
2 x 256 tanh torch module (noise on, log_std = -1), ms per control step of
  (a)  the bare step_device loop with pre-allocated tensors — the loop a user writes today — on a batch of its own, terminal
       observations off,
  (a') the same loop on the vector environment's batch, whose step kernel also stores terminal observations,
  (b)  LocoVectorEnv.step: the step kernel, lv_finish_step behind it, and one torch launch for the `_final_obs` mask,
  (c)  loop (a') plus the same bookkeeping written as torch ops: the done byte split, the final observation selected, returns and
       lengths accumulated, reported and restarted.
Device-side restarts at the task's horizon, 50 warm-up steps per leg, then `steps` control steps per repeat timed by HIP events on the
caller's stream, `repeats` repeats per leg, the legs alternating. (a) steps a batch of its own and (a'), (b), (c) share one: the robots
of the two batches are in different states at any time, which is why (a') is there. Usage: vector_env_time.py [steps] [repeats] [n_envs]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from loco_mujoco_amd import LocoEnv, LocoVectorEnv  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 500
repeats = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 5
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
task = "UnitreeA1.simple"
dev = torch.device("cuda", 0)

np.random.seed(0)
env = LocoEnv.make(task, debug=True, n_envs=n)
env.reset()
env.enable_auto_reset(seed=0)
np.random.seed(0)
venv = LocoVectorEnv(task, n, seed=0, debug=True)
first_obs, _ = venv.reset()
plain, shared = env.backend, venv.unwrapped.backend
nobs, nu = plain.nobs, plain.nu

torch.manual_seed(0)
pi = torch.nn.Sequential(torch.nn.Linear(nobs, 256), torch.nn.Tanh(), torch.nn.Linear(256, 256), torch.nn.Tanh(), torch.nn.Linear(256, nu)).to(dev)
std = torch.full((nu,), -1.0, device=dev).exp()
stream = torch.cuda.current_stream(dev)
s = stream.cuda_stream


def act(o):
    mean = pi(o)
    return torch.addcmul(mean, std, torch.randn_like(mean))


class Loop:
    """The pre-allocated tensors of a step_device loop on batch `b`: two observation slots, so that (obs, next_obs) stay apart."""

    def __init__(self, b):
        self.b = b
        self.obs = torch.zeros((2, n, nobs), device=dev)
        self.rew = torch.zeros(n, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.at = 0

    def start(self, o):
        self.obs[self.at].copy_(o)

    def step(self):
        a = act(self.obs[self.at])
        self.at ^= 1
        self.b.step_device(a, self.obs[self.at], self.rew, self.done, stream=s, sync=False)
        return self.obs[self.at]


bare, bare_shared = Loop(plain), Loop(shared)
plain.step_device(obs=bare.obs[0], stream=s, sync=False)
bare_shared.start(first_obs)
# the bookkeeping of (c), as tensors of the probe
term = venv._term
final_obs = torch.zeros((n, nobs), device=dev)
run_r, run_l = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
state = {"venv_obs": first_obs}


def leg_bare(count):
    with torch.no_grad():
        for _ in range(count):
            bare.step()


def leg_bare_shared(count):
    with torch.no_grad():
        for _ in range(count):
            bare_shared.step()


def leg_vector(count):
    o = state["venv_obs"]
    with torch.no_grad():
        for _ in range(count):
            o, r, terminated, truncated, info = venv.step(act(o))
    state["venv_obs"] = o


def leg_torch_bookkeeping(count):
    L = bare_shared
    with torch.no_grad():
        for _ in range(count):
            o = L.step()
            terminated = (L.done & 1).bool()
            restarted = (L.done & 2).bool()
            truncated = restarted & ~terminated
            ended = L.done != 0
            run_r.add_(L.rew)
            run_l.add_(1)
            ep_r = torch.where(ended, run_r, 0.0)
            ep_l = torch.where(ended, run_l, 0)
            run_r.masked_fill_(ended, 0.0)
            run_l.masked_fill_(ended, 0)
            last = torch.where(restarted[:, None], term, o)
            torch.where(ended[:, None], last, final_obs, out=final_obs)
    state["c"] = (terminated, truncated, ep_r, ep_l)


legs = (("(a) bare step_device loop, own batch", leg_bare), ("(a') bare step_device loop, the vector env's batch", leg_bare_shared),
        ("(b) LocoVectorEnv.step", leg_vector), ("(c) (a') + the bookkeeping as torch ops", leg_torch_bookkeeping))


def prepare(leg):
    # (a') and (c) leave the shared batch's newest observation in their own slot: (b) continues from it, and the other way round
    if leg is leg_vector:
        state["venv_obs"] = bare_shared.obs[bare_shared.at]
    elif leg is not leg_bare:
        bare_shared.start(state["venv_obs"])


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
med = {}
for name, _ in legs:
    t = sorted(times[name])
    med[name] = t[len(t) // 2]
    print("%s n=%d %s: ms per control step %s, median %.4f, spread %.4f" % (task, n, name, ", ".join("%.4f" % v for v in times[name]),
                                                                           med[name], t[-1] - t[0]), flush=True)
a, a2, b_, c = (med[name] for name, _ in legs)
print("(b) - (a) %.4f ms, (b) - (a') %.4f ms, (c) - (a') %.4f ms, (c) - (b) %.4f ms" % (b_ - a, b_ - a2, c - a2, c - b_), flush=True)
for label, batch in (("own batch", plain), ("the vector env's batch", shared)):
    st = batch.stats(reset=True)
    print("%s: %d env-steps, %d episodes" % (label, st["env_steps"], st["episodes"]), flush=True)
