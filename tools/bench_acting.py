"""Latency of Agent.forward on the HIP acting path (GPU box): python tools/bench_acting.py
host -> actions on the host, per call, for the hipGraph form (default) and the eager launches (config.act_graph = False):
  numpy in      a host array in, .cpu() out (evaluators: sync_agent_evaluator.py:43)
  device in     the reference collector's pattern: one persistent device inference buffer in, .cpu().numpy() out
                (multiprocessing_experience_collection/experience_collector.py:77-78,127)
--rows ids      only the ten-head IDS configuration, deterministic and sampled (ids_use_random_samples), hipGraph form
--rows egreedy  the DQN configuration configs[1], hipGraph form: the greedy selector (use_e_greedy off) before and after the
                per-observation epsilon-greedy mode (e_greedy_per_env; epsilon pinned to 0 and to 1: every row greedy, every
                row a random action) -- the two greedy rows give the run-to-run spread of one visit
--rows eval     the ten-head IDS configuration in eval mode (agent.eval()), hipGraph form: the greedy evaluation selector,
                the MinRegret one (eval_action_selector = "min_regret"; skipped with --no-min-regret, for a tree without it)
                and greedy again -- the two greedy rows give the run-to-run spread of one visit
--rows risk     the IQN configuration configs[2], hipGraph form: the greedy selector on the quantile mean, neutral, under each
                risk policy (iqn_risk_policy_id: one prism_act_tau_distort in front of the forward) and neutral again -- the
                two neutral rows give the run-to-run spread of one visit; --neutral-only for a tree without the knob
--sizes 1,16    observation counts;  --reps 300   calls per median;  --tag NAME   prefix of every printed row (two trees
                measured alternately in one visit)"""
import argparse, contextlib, io, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from prism_amd.config import baseline_config
from prism_amd.learner import Learner


def measure(cfg_i, graph, reps=400, sizes=(1, 4, 16), eval_mode=False, **over):
    cfg = baseline_config(cfg_i, device="cuda:0", log_to_wandb=False, act_graph=graph, **over)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6)
    ag = ln.agent
    if eval_mode:
        ag.eval()
    rng = np.random.default_rng(0)
    out = {}
    for n in sizes:
        obs = (rng.random((n, 10, 10, 4)) < 0.1).astype(np.float32)
        dev_buf = torch.zeros((n, 10, 10, 4), device="cuda:0")
        host_t = torch.from_numpy(obs)
        for mode in ("numpy in", "device in"):
            def call():
                if mode == "numpy in":
                    return ag.forward(obs).cpu()
                dev_buf.copy_(host_t, non_blocking=True)
                return ag.forward(dev_buf).cpu().numpy()
            for _ in range(30):
                call()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            out[f"n={n} {mode}"] = round(float(np.median(ts)) * 1e6, 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="all", choices=["all", "ids", "egreedy", "eval", "risk"])
    ap.add_argument("--neutral-only", action="store_true")
    ap.add_argument("--no-min-regret", action="store_true")
    ap.add_argument("--sizes", default="1,4,16")
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    sizes = tuple(int(x) for x in args.sizes.split(","))
    sampled = dict(ids_use_random_samples=True)
    rows = [(2, "IQN (greedy on the quantile mean)", {}), (3, "IDS + IQN, ten heads", {}),
            (3, "IDS + IQN, ten heads, sampled", sampled)]
    if args.rows == "ids":
        rows = rows[1:]
    if args.rows == "egreedy":
        greedy = dict(use_e_greedy=False)
        per_env = dict(e_greedy_per_env=True, e_greedy_decay_timesteps=0)
        rows = [(1, "DQN, greedy", greedy),
                (1, "DQN, e-greedy per env, eps 0", dict(per_env, e_greedy_final_epsilon=0.0)),
                (1, "DQN, e-greedy per env, eps 1", dict(per_env, e_greedy_final_epsilon=1.0)),
                (1, "DQN, greedy (again)", greedy)]
    if args.rows == "eval":
        rows = [(3, "IDS + IQN, eval: greedy", {}), (3, "IDS + IQN, eval: min_regret", dict(eval_action_selector="min_regret")),
                (3, "IDS + IQN, eval: greedy (again)", {})]
        if args.no_min_regret:
            del rows[1]
    if args.rows == "risk":
        policies = [] if args.neutral_only else ["cvar:0.25", "wang:-0.75", "cpw:0.71", "pow:-2"]
        rows = [(2, "IQN, neutral", {})] + [(2, f"IQN, {p}", dict(iqn_risk_policy_id=p)) for p in policies] + \
               [(2, "IQN, neutral (again)", {})]
    res = {}
    for cfg_i, name, over in rows:
        for graph in ((True,) if args.rows != "all" else (True, False)):
            r = measure(cfg_i, graph, args.reps, sizes, eval_mode=args.rows == "eval", **over)
            what = f" {name}" if args.rows in ("egreedy", "eval", "risk") else " sampled" if over else ""
            res[f"{args.tag}configs[{cfg_i}]{what} {'graph' if graph else 'eager'}"] = r
            for k, v in r.items():
                print(f"{args.tag}{name:36s} {'hipGraph' if graph else 'eager   '} {k:18s}: {v:7.1f} us per Agent.forward (host -> actions on the host)",
                      flush=True)
    print(json.dumps(res))
