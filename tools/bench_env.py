"""Environment and whole-loop rates on the GPU box:
python tools/bench_env.py [--game breakout|freeway|asterix|spaceinvaders|seaquest] [--sizes 64,512,4096] [--calls 4000] [--reps 3]
1. DeviceBreakout.step / DeviceFreeway.step / DeviceAsterix.step / DeviceSpaceInvaders.step / DeviceSeaquest.step alone (prism_amd/envs.py) for N environments: device events around --calls back-to-back steps on one
   stream with fixed device actions -- once as eager calls (launch and the Python call included: what a step of the loop
   pays), once as replays of a hipGraph of 64 captured steps (the kernel and its boundary).  Environment steps per second
   = N * steps / time.
2. The loop  Agent.forward -> envs.step -> extend_batch -> Learner.step  (one VectorCollector step
   and one learner step per iteration) at N = --loop-n on BASELINE's c3 (configs[2]): with the device environments, and with
   the NumPy host restatement of the same rules (tests/env_ref.py HostBreakout, tests/freeway_ref.py HostFreeway, tests/asterix_ref.py HostAsterix,
   tests/invaders_ref.py HostSpaceInvaders, tests/seaquest_ref.py HostSeaquest: the
   baseline of the comparison, not a product path) in the same loop.  Host clock around work that ends in a device synchronise, the two loops by turns, one warm-up
   run each, medians of --reps."""
import argparse, contextlib, io, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from prism_amd.collectors import VectorCollector
from prism_amd.config import baseline_config
from prism_amd.envs import DeviceAsterix, DeviceBreakout, DeviceFreeway, DeviceSeaquest, DeviceSpaceInvaders
from prism_amd.learner import Learner

DEV = "cuda:0"
GAMES = {"breakout": (DeviceBreakout, "MinAtar/Breakout-v0"), "freeway": (DeviceFreeway, "MinAtar/Freeway-v0"),
         "asterix": (DeviceAsterix, "MinAtar/Asterix-v0"), "spaceinvaders": (DeviceSpaceInvaders, "MinAtar/SpaceInvaders-v0"),
         "seaquest": (DeviceSeaquest, "MinAtar/Seaquest-v0")}
GRAPH_STEPS = 64          # even: the ping-pong buffers end where they began


def env_rate(game, n, calls, reps):
    env = GAMES[game][0](n, 7, DEV, sticky_action_prob=0.1, episode_timestep_limit=1000)
    acts = torch.randint(0, 6, (n,), device=DEV)
    env.reset()
    for _ in range(200):
        env.step(acts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side), torch.cuda.graph(g, stream=side):
        for _ in range(GRAPH_STEPS):
            env.step(acts)
    torch.cuda.synchronize()

    def timed(fn, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / steps          # us per step

    def eager():
        for _ in range(calls):
            env.step(acts)

    def replays():
        for _ in range(calls // GRAPH_STEPS):
            g.replay()

    replays()
    out = {"eager": [], "graph": []}
    for _ in range(reps):
        out["eager"].append(timed(eager, calls))
        out["graph"].append(timed(replays, calls // GRAPH_STEPS * GRAPH_STEPS))
    env.close()
    e, gr = float(np.median(out["eager"])), float(np.median(out["graph"]))
    return dict(game=game, n=n, calls=calls, eager_us_per_step=round(e, 2), graph_us_per_step=round(gr, 2),
                eager_env_steps_per_s=round(n / e * 1e6), graph_env_steps_per_s=round(n / gr * 1e6),
                eager_all=[round(x, 2) for x in out["eager"]], graph_all=[round(x, 2) for x in out["graph"]])


def make_loop(game, n, envs, ckpt_dir):
    cfg = baseline_config(2, device=DEV, log_to_wandb=False, env_name=GAMES[game][1], num_processes=n,
                          experience_replay_capacity=100_000, checkpoint_dir=ckpt_dir, seed=3)
    col, ln = VectorCollector(envs, cfg), Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
    rows = col.collect_timesteps(max(1024, 4 * n), ln.agent, ln.experience_buffer, random=True)
    ln.cumulative_timesteps += rows

    def run(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            col.collect_timesteps(n, ln.agent, ln.experience_buffer)
            ln.step(n)
        torch.cuda.synchronize()
        return iters / (time.perf_counter() - t0)
    return run


def loop_rates(game, n, iters, host_iters, reps):
    if game == "freeway":
        from tests.freeway_ref import HostFreeway as Host
    elif game == "asterix":
        from tests.asterix_ref import HostAsterix as Host
    elif game == "spaceinvaders":
        from tests.invaders_ref import HostSpaceInvaders as Host
    elif game == "seaquest":
        from tests.seaquest_ref import HostSeaquest as Host
    else:
        from tests.env_ref import HostBreakout as Host
    with tempfile.TemporaryDirectory() as tmp:
        kw = dict(sticky_action_prob=0.1, episode_timestep_limit=1000)
        loops = {"device": (make_loop(game, n, GAMES[game][0](n, 3, DEV, **kw), os.path.join(tmp, "d")), iters),
                 "host": (make_loop(game, n, Host(n, 3, **kw), os.path.join(tmp, "h")), host_iters)}
        out = {"device": [], "host": []}
        for name, (run, k) in loops.items():
            run(max(50, k // 10))                      # warm-up: graph captures, first launches
        for _ in range(reps):
            for name, (run, k) in loops.items():
                out[name].append(run(k))
    d, h = float(np.median(out["device"])), float(np.median(out["host"]))
    return dict(game=game, n=n, config="c3", device_iters_per_s=round(d, 1), host_iters_per_s=round(h, 1), ratio=round(d / h, 2),
                device_env_steps_per_s=round(d * n), host_env_steps_per_s=round(h * n),
                device_all=[round(x, 1) for x in out["device"]], host_all=[round(x, 1) for x in out["host"]])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=sorted(GAMES), default="breakout")
    ap.add_argument("--sizes", default="64,512,4096")
    ap.add_argument("--calls", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--host-iters", type=int, default=300)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_env needs the GPU"
    res = {"game": args.game, "env": [], "loop": None}
    for n in (int(x) for x in args.sizes.split(",") if x):
        r = env_rate(args.game, n, args.calls, args.reps)
        res["env"].append(r)
        print(f"{args.game} N = {n:5d}: eager {r['eager_us_per_step']:7.2f} us/step = {r['eager_env_steps_per_s']:12d} env steps/s   "
              f"graph {r['graph_us_per_step']:7.2f} us/step = {r['graph_env_steps_per_s']:12d} env steps/s", flush=True)
    if args.loop_n > 0:
        r = res["loop"] = loop_rates(args.game, args.loop_n, args.iters, args.host_iters, args.reps)
        print(f"loop at N = {r['n']} on c3: device environments {r['device_iters_per_s']:.1f} iterations/s, host restatement "
              f"{r['host_iters_per_s']:.1f} iterations/s, ratio {r['ratio']:.2f}", flush=True)
    print(json.dumps(res))
