"""The bias of the budget rule over N lock-stepped streams, as a MODEL on the CPU (no device, no game):
    python tools/eval_bias.py [--horizon 100000] [--mean-length 500 2500] [--reps 20] [--streams 1 16 64 256] [--json]
Synthetic streams: episode lengths are drawn from the geometric distribution on 1, 2, ... with the given mean (every step
ends the episode with probability 1 / mean: the discrete exponential), independently per stream, reward 1 per step, so
return = length and the true mean return is the mean length.  The same streams are fed to the two restatements the device
is held to: ``EvalHost`` (tests/eval_ref.py, the budget rule: the reference's, `horizon` rows over all streams, open
episodes dropped) and ``EvalQuotaHost`` (tests/eval_quota_ref.py, the quota rule: every stream's first E episodes), with
E = ceil(horizon / (N x mean length)) so that both see about the same number of rows.  Reported: the mean over --reps
evaluations of (reported mean return / true mean - 1), per rule, with the standard error of that mean over the evaluations
(the sampling noise of the table itself: a cell within two of it of zero shows no bias)."""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.eval_quota_ref import EvalQuotaHost          # noqa: E402
from tests.eval_ref import EvalHost                     # noqa: E402


def one_evaluation(n, horizon, mean_length, quota, rng):
    """One evaluation of each rule over the same n streams: (budget rule's mean return, quota rule's)."""
    budget, by_quota = EvalHost(n, horizon, 0), EvalQuotaHost(n, quota, log_capacity=0)
    ones, none = [1.0] * n, [0] * n
    p = 1.0 / mean_length
    while not (budget.closed() and by_quota.closed()):
        ends = (rng.random(n) < p).tolist()
        budget.track(ones, ends, none)          # a closed evaluation takes nothing
        by_quota.track(ones, ends, none)
    return budget.stats[0] / budget.counts[0], by_quota.stats[0] / by_quota.counts[0]


def bias_rows(horizon, mean_length, streams, reps, seed=0):
    rows = []
    for n in streams:
        quota = max(1, math.ceil(horizon / (n * mean_length)))
        rng = np.random.default_rng([seed, n, int(mean_length)])
        got = np.array([one_evaluation(n, horizon, mean_length, quota, rng) for _ in range(reps)])
        rel = got / mean_length - 1.0
        (b, q), (b_se, q_se) = rel.mean(axis=0), rel.std(axis=0, ddof=1) / math.sqrt(reps) if reps > 1 else (0.0, 0.0)
        rows.append(dict(n=n, mean_length=mean_length, episodes_per_stream=quota, budget_bias=float(b), budget_se=float(b_se),
                         quota_bias=float(q), quota_se=float(q_se)))
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=100_000)
    ap.add_argument("--mean-length", type=float, nargs="+", default=[500.0, 2500.0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    rows = []
    for m in args.mean_length:
        rows += bias_rows(args.horizon, m, args.streams, args.reps, args.seed)
    if not args.json:
        print(f"model: geometric episode lengths, return = length, horizon {args.horizon}, {args.reps} evaluations per cell")
        print("|   N | mean length |   E | budget rule (s.e.) | quota rule (s.e.) |")
        print("|-----|-------------|-----|--------------------|-------------------|")
        for r in rows:
            print(f"| {r['n']:3d} | {r['mean_length']:11.0f} | {r['episodes_per_stream']:3d} | {100 * r['budget_bias']:+6.1f} % "
                  f"({100 * r['budget_se']:.1f}) | {100 * r['quota_bias']:+6.1f} % ({100 * r['quota_se']:.1f}) |")
    print(json.dumps(dict(horizon=args.horizon, reps=args.reps, rows=rows)))
