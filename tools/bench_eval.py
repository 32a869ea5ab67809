"""Evaluation rate on the GPU box: python tools/bench_eval.py [--sizes 1,16,256] [--steps 2000] [--reps 3]
VectorEvaluator (prism_amd/evals.py) over a device-resident stub environment on configs[3], N environments in lockstep:
environment steps (timesteps) per second of whole evaluations of --steps steps, host clock around work that ends in the
evaluator's own device wait.  Beside it the same loop with the reference's bookkeeping on the host -- reward and done read
back with .cpu() on every step, the sums kept in Python (sync_agent_evaluator.py:42-59): the baseline of the comparison, not
a product path.  Then the cost of prism_eval_track alone at n = 16 and n = 1024: device events around --calls
back-to-back launches on one stream (launch and the Python call included: what a step of the loop pays).
--track-only [--track-sizes 16]   only that last part: the run to put under `rocprofv3 --kernel-trace --stats` for the
                                  kernel's own duration, one size per run (the kernel has one name).
--episodes-per-env E              the quota rule (prism_eval_track_quota) in place of the budget rule: whole evaluations
                                  of E episodes per environment, capped at --steps steps (no host twin: the reference has
                                  no such rule), and the cost of the quota kernel with every row live."""
import argparse, contextlib, io, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from prism_amd.config import baseline_config
from prism_amd.evals import EVAL_DRAW_BASE, EvalTracker, VectorEvaluator
from prism_amd.factory import agent_factory

DEV = "cuda:0"


class StubEnvs:
    """N environments whose observations, rewards and ends are rows of device tables: a step launches nothing and reads
    nothing back.  Episodes end with probability 1/200 per stream and step (stream 0 ends at step 5: no evaluation waits
    for its first episode)."""
    n_actions, obs_shape = 6, (10, 10, 4)

    def __init__(self, n, steps, seed=0):
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.n, self.k, self.period = n, 0, steps + 64
        self.obs = (torch.rand((8, n) + self.obs_shape, device=DEV, generator=g) < 0.1).float()
        self.reward = (torch.rand((self.period, n), device=DEV, generator=g) < 0.3).float()          # MinAtar's 0 / 1
        self.done = torch.rand((self.period, n), device=DEV, generator=g) < 1 / 200
        self.done[5, 0] = True
        self.trunc = torch.zeros((self.period, n), dtype=torch.bool, device=DEV)

    def reset(self):
        self.k = 0
        return self.obs[0]

    def step(self, action):
        k = self.k % self.period
        self.k += 1
        return self.obs[self.k & 7], self.reward[k], self.done[k], self.trunc[k]

    def observe(self):
        return self.obs[self.k & 7]


def host_bookkeeping_evaluation(agent, envs, horizon, draws):
    """The reference's loop for N streams with its bookkeeping where the reference has it: on the host."""
    obs = envs.reset()
    n = int(obs.shape[0])
    ep_rews, cur, collected = [], [0.0] * n, 0
    agent.eval()
    try:
        with agent.acting_stream(EVAL_DRAW_BASE + draws):
            while collected < horizon or len(ep_rews) == 0:
                action = agent.forward(obs)
                _, reward, done, trunc = envs.step(action)
                reward, done, trunc = reward.cpu().tolist(), done.cpu().tolist(), trunc.cpu().tolist()
                for i in range(n):
                    cur[i] += reward[i]
                    if done[i] or trunc[i]:
                        ep_rews.append(cur[i])
                        cur[i] = 0.0
                obs = envs.observe()
                collected += n
    finally:
        agent.train()
    return ep_rews, collected


def rates(n, steps, reps):
    cfg = baseline_config(3, device=DEV, log_to_wandb=False)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, StubEnvs.obs_shape, StubEnvs.n_actions)
    envs = StubEnvs(n, steps)
    ev = VectorEvaluator(agent, envs, 0, steps * n)
    out = {}
    for name in ("device", "host") * reps:          # alternating, one warm-up evaluation each (graph capture)
        for timed in ((False, True) if name not in out else (True,)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "device":
                returns = ev.evaluate_agent()
                ts = ev.last["timesteps"]
            else:
                returns, ts = host_bookkeeping_evaluation(agent, envs, steps * n, ev.eval_draws)
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if timed:
                out.setdefault(name, []).append(ts / dt)
                out[name + "_returns"] = [float(r) for r in returns]
    assert out["device_returns"] == out["host_returns"]          # 0 / 1 rewards: both precisions give the same sums
    dev, host = float(np.median(out["device"])), float(np.median(out["host"]))
    return dict(n=n, steps=steps, episodes=len(out["device_returns"]), device_steps_per_s=round(dev, 1),
                host_steps_per_s=round(host, 1), ratio=round(dev / host, 3),
                device_all=[round(x, 1) for x in out["device"]], host_all=[round(x, 1) for x in out["host"]])


def quota_rates(n, steps, reps, episodes_per_env):
    cfg = baseline_config(3, device=DEV, log_to_wandb=False)
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, StubEnvs.obs_shape, StubEnvs.n_actions)
    ev = VectorEvaluator(agent, StubEnvs(n, steps), 0, steps * n, episodes_per_env=episodes_per_env, max_steps_per_env=steps)
    out = []
    for k in range(reps + 1):          # one warm-up evaluation (graph capture)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev.evaluate_agent()
        dt = time.perf_counter() - t0
        if k:
            out.append(ev.last["timesteps"] / dt)
    last = ev.last
    return dict(n=n, steps=steps, episodes_per_env=episodes_per_env, episodes=last["episodes"], calls=last["calls"],
                incomplete_streams=last["incomplete_streams"], device_steps_per_s=round(float(np.median(out)), 1),
                device_all=[round(x, 1) for x in out])


def track_cost(n, calls, quota=0):
    """quota > 0: the quota kernel, with a quota no stream reaches (every row stays live: the full cost)."""
    tr = EvalTracker(n, 10 ** 15, 4096, DEV, episodes_per_stream=quota, max_calls=10 ** 15 if quota else 0)
    g = torch.Generator(device=DEV).manual_seed(n)
    reward = torch.rand(n, device=DEV, generator=g)
    done = torch.rand(n, device=DEV, generator=g) < 1 / 200
    trunc = torch.zeros(n, dtype=torch.bool, device=DEV)
    for _ in range(200):
        tr.track(reward, done, trunc)
    torch.cuda.synchronize()
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            tr.track(reward, done, trunc)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return dict(n=n, calls=calls, kernel="prism_eval_track_quota" if quota else "prism_eval_track", us_per_call=round(float(np.median(out)), 2), all=[round(x, 2) for x in out])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5000)
    ap.add_argument("--track-only", action="store_true")
    ap.add_argument("--track-sizes", default="16,1024")
    ap.add_argument("--episodes-per-env", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval needs the GPU"
    res = {"rates": [], "track": []}
    E = args.episodes_per_env
    for n in (() if args.track_only or not E else (int(x) for x in args.sizes.split(","))):
        r = quota_rates(n, args.steps, args.reps, E)
        res["rates"].append(r)
        print(f"N = {n:4d}: quota rule, {E} episodes per environment {r['device_steps_per_s']:10.1f} steps/s   "
              f"({r['episodes']} episodes in {r['calls']} calls, {r['incomplete_streams']} incomplete streams)", flush=True)
    for n in (() if args.track_only or E else (int(x) for x in args.sizes.split(","))):
        r = rates(n, args.steps, args.reps)
        res["rates"].append(r)
        print(f"N = {n:4d}: device bookkeeping {r['device_steps_per_s']:10.1f} steps/s   host bookkeeping "
              f"{r['host_steps_per_s']:10.1f} steps/s   ratio {r['ratio']:.3f}   ({r['episodes']} episodes)", flush=True)
    for n in (int(x) for x in args.track_sizes.split(",")):
        r = track_cost(n, args.calls, 2 ** 30 if E else 0)
        res["track"].append(r)
        print(f"{r['kernel']} n = {n:4d}: {r['us_per_call']:.2f} us per call, back to back on one stream", flush=True)
    print(json.dumps(res))
