"""Whole-loop rate on the GPU box, eager or as captured iterations:
python tools/bench_loop.py [--n 64] [--iters 3000] [--reps 1] [--captured] [--game breakout]
                           [--no-prefill] [--capacity 100000] [--fill-graph]
The loop of Learner._learn -- k x (Agent.forward -> envs.step -> extend_batch) and one Learner.step per iteration, with
timesteps_per_iteration = N (k = 1) -- on BASELINE's c3 (configs[2], B = 256, 100 000 slots) over the device environments.  The
ring is filled first (uniform random actions), so the eager loop replays its step graph and --captured (config.captured_loop)
replays whole iterations: the two differ in what a single replay saves, nothing else.  Host clock around work that ends in a
device synchronise; one warm-up run (graph captures, first launches), then --reps runs of --iters iterations.  Without
--captured nothing of the captured loop is touched: the same file measures an older tree.
--no-prefill starts the clock behind the random prologue (config.num_initial_random_timesteps rows) instead: the loop while the
ring fills, which is all a run sees whose ring (--capacity, e.g. the presets' 3 000 000) is larger than its timestep limit.
There the eager loop launches its step eagerly; --fill-graph (config.graph_while_filling) replays it, and with --captured the
whole iteration.  Without the three flags nothing they stand for is touched either.  captured_iterations and
fill_graph_replays in the result count the timed runs alone."""
import argparse, contextlib, io, json, os, sys, tempfile, time
sys.path.insert(0, os.getcwd() if os.path.isdir(os.path.join(os.getcwd(), "prism_amd")) else
                os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from prism_amd import envs as E
from prism_amd.collectors import VectorCollector
from prism_amd.config import baseline_config
from prism_amd.learner import Learner

DEV = "cuda:0"
GAMES = {"breakout": ("DeviceBreakout", "MinAtar/Breakout-v0"), "freeway": ("DeviceFreeway", "MinAtar/Freeway-v0"),
         "asterix": ("DeviceAsterix", "MinAtar/Asterix-v0"), "spaceinvaders": ("DeviceSpaceInvaders", "MinAtar/SpaceInvaders-v0"),
         "seaquest": ("DeviceSeaquest", "MinAtar/Seaquest-v0")}
CAPACITY = 100_000

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--game", choices=sorted(GAMES), default="breakout")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--captured", action="store_true")
    ap.add_argument("--no-prefill", action="store_true")
    ap.add_argument("--capacity", type=int, default=CAPACITY)
    ap.add_argument("--fill-graph", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_loop needs the GPU"
    n = args.n
    with tempfile.TemporaryDirectory() as tmp:
        cfg = baseline_config(2, device=DEV, log_to_wandb=False, env_name=GAMES[args.game][1], num_processes=n,
                              experience_replay_capacity=args.capacity, timesteps_per_iteration=n, checkpoint_dir=tmp, seed=3)
        cfg.captured_loop = args.captured
        if args.fill_graph:
            cfg.graph_while_filling = True
        envs = getattr(E, GAMES[args.game][0])(n, 3, DEV, sticky_action_prob=0.1, episode_timestep_limit=1000)
        col, ln = VectorCollector(envs, cfg), Learner()
        with contextlib.redirect_stdout(io.StringIO()):
            ln.configure(cfg, collector=col)
        agent, buf = ln.agent, ln.experience_buffer
        prologue = int(cfg.num_initial_random_timesteps) if args.no_prefill else args.capacity          # default: the ring is full
        ln.cumulative_timesteps += col.collect_timesteps(prologue, agent, buf, random=True)

        def run(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                if args.captured and ln._captured_iteration() is not None:
                    continue
                col.collect_timesteps(n, agent, buf)
                ln.step(n)
            torch.cuda.synchronize()
            return iters / (time.perf_counter() - t0)

        run(max(50, args.iters // 10))
        counts = lambda: (getattr(ln, "captured_iterations", 0), getattr(agent, "fill_graph_replays", 0))
        before = counts()
        rates = [run(args.iters) for _ in range(args.reps)]
        timed = [a - b for a, b in zip(counts(), before)]
        size = len(buf)
        envs.close()
    r = float(np.median(rates))
    print(json.dumps(dict(game=args.game, n=n, config="c3", captured=bool(args.captured), iters=args.iters,
                          iters_per_s=round(r, 1), us_per_iter=round(1e6 / r, 1), env_steps_per_s=round(r * n),
                          all=[round(x, 1) for x in rates], captured_iterations=timed[0], fill_graph_replays=timed[1],
                          fill_graph=bool(args.fill_graph), capacity=args.capacity, rows_at_end=size,
                          refusal=ln.captured_loop_refusal() if args.captured else None)))
