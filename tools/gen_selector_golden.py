#!/usr/bin/env python3
"""Generate tests/golden/selectors_ref.npz and tests/golden/ref_state_min_regret/ by RUNNING the reference's
MinRegretActionSelector and SimpleIDSActionSelector (imported from /root/reference; prism/agents/action_selectors.py:85-111,
:195-286).  Build-container only, like tools/gen_golden.py: nothing in tests/ or the product imports the reference, and the
fixture holds the reference's OUTPUTS only -- the inputs are redrawn from the seeded table tests/selector_cases.py.

    python tools/gen_selector_golden.py            # walks the seed steps (near ties, ill-conditioned values); prints SEED_STEP for tests/selector_cases.py when
                                                   # it differs from the table's, and writes the fixture when it does not

Recorded, flat over the table's cases in order (tests/selector_cases.py ``layout``), [2] = both lambdas / betas:
  mr_action [2][rows] mr_scores [2][values]   MinRegret: the action; regret^2, the argument of its torch.argmin (:104)
  mr_spread [values]                          its ``variance`` (q.std(-1)), the argument of its torch.sqrt (:99)
  si_action [2][rows] si_scaled [2][values]   SimpleIDS on the per-head list: the action; loggable "Scaled Q Values"
  si_mean, si_max_diff [values]               loggables "Q Estimate Ensemble Mean", "Q Estimate Max Difference"
The loggables "Action Uncertainty" (the same tensor as the max difference) and "Action Probs" (the one-hot of the action)
are compared to those on the spot and not stored.  The same under ``g/<name>/`` for the recorded ensemble outputs ``act/q``
of the update fixtures selector_cases.GOLDEN_CASES, with the unsquish function of the case's loss_squish_fn_id; those
inputs are what they are, and a row of theirs may lie near a tie (selector_cases.near_ties finds it from the scores)."""
import os
import pickle
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, ROOT)

from prism.agents import action_selectors as R          # noqa: E402
from prism.agents import squish_functions as RQ          # noqa: E402
from tests import helpers as H          # noqa: E402
from tests import selector_cases as T          # noqa: E402

UNSQUISH = {"none": None, "symlog": RQ.symexp, "obs_look_further": RQ.obs_look_further_squish_fn_inverse}


def unsquish(usq, exact):
    """The reference's unsquish function; ``exact``: evaluated in float64 and rounded to fp32 once."""
    f = UNSQUISH[usq]
    return (lambda x: f(x.double()).float()) if exact and f is not None else f


def run_min_regret(q, lmbda, usq, exact=False):
    """The reference class on ``q [n, A, heads]``; its regret^2 and its ``variance`` are taken from the arguments of the
    torch.argmin and torch.sqrt calls it makes (the class keeps neither)."""
    seen = {}
    keep = torch.argmin, torch.sqrt

    def argmin(x, *a, **k):
        seen["scores"] = x.clone()
        return keep[0](x, *a, **k)

    def sqrt(x, *a, **k):
        seen["spread"] = x.clone()
        return keep[1](x, *a, **k)

    sel = R.MinRegretActionSelector(lmbda, unsquish(usq, exact))
    torch.argmin, torch.sqrt = argmin, sqrt
    try:
        probs = sel.generate_action_probs(None, torch.from_numpy(q))
    finally:
        torch.argmin, torch.sqrt = keep
    return dict(action=sel.select_action(probs).numpy(), scores=seen["scores"].numpy(), spread=seen["spread"].numpy())


def run_simple_ids(q, beta, usq, exact=False):
    sel = R.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, beta, unsquish(usq, exact))
    t = torch.from_numpy(q)
    heads = [t[:, :, h].clone() for h in range(t.shape[2])]          # (the class writes into the list it is given)
    probs = sel.generate_action_probs(torch.zeros((1,) + tuple(t.shape[:2])), heads, for_log=True)
    lg = {k: v.numpy() for k, v in sel.loggables.items()}
    action = sel.select_action(probs).numpy()
    assert sorted(lg) == ["Action Probs", "Action Uncertainty", "Q Estimate Ensemble Mean", "Q Estimate Max Difference",
                          "Scaled Q Values"]
    np.testing.assert_array_equal(lg["Action Uncertainty"], lg["Q Estimate Max Difference"])
    np.testing.assert_array_equal(lg["Action Probs"], np.eye(t.shape[1], dtype=np.int64)[action])
    return dict(action=action, scores=lg["Scaled Q Values"], mean=lg["Q Estimate Ensemble Mean"],
                max_diff=lg["Q Estimate Max Difference"])


def run_case(q, usq):
    mr = [run_min_regret(q, lm, usq) for lm in T.LAMBDAS]
    si = [run_simple_ids(q, b, usq) for b in T.BETAS]
    np.testing.assert_array_equal(mr[0]["spread"], mr[1]["spread"])
    for k in ("mean", "max_diff"):
        np.testing.assert_array_equal(si[0][k], si[1][k])
    ties = np.zeros(q.shape[0], dtype=bool)
    for r in mr:
        ties |= T.near_ties(r["scores"], usq, largest=False)
    for r in si:
        ties |= T.near_ties(r["scores"], usq, largest=True)
    return mr, si, ties | ill_conditioned(q, usq, mr, si)


def ill_conditioned(q, usq, mr, si):
    """Rows with a recorded value that the reference's OWN fp32 rounding inside the unsquish function moves by more than
    half the value's tolerance: the same classes with that function evaluated in float64.  obs_look_further's inverse
    takes (sqrt(1 + ...) - 1), which turns one ulp of the root into 3e-6 relative; the centred means and scaled values of
    SimpleIDS are differences of such estimates and can lie anywhere near zero.  On such a value two correct fp32
    evaluations need not agree within the tolerance (torch's CPU sqrt and exp themselves differ by an ulp between CPUs)."""
    bad = np.zeros(q.shape[0], dtype=bool)
    if UNSQUISH[usq] is None:
        return bad
    rtol, atol = T.tol(usq)
    pairs = [(r, run_min_regret(q, lm, usq, exact=True), ("scores", "spread")) for r, lm in zip(mr, T.LAMBDAS)]
    pairs += [(r, run_simple_ids(q, b, usq, exact=True), ("scores", "mean", "max_diff")) for r, b in zip(si, T.BETAS)]
    for got, ref, keys in pairs:
        for k in keys:
            bad |= (np.abs(got[k] - ref[k]) > 0.5 * (rtol * np.abs(got[k]) + atol)).any(axis=-1)
    return bad


def pack(results):
    """[(mr, si)] per case -> the flat arrays."""
    flat = lambda key, which, i: np.concatenate([r[which][i][key].reshape(-1) for r in results])          # noqa: E731
    return {
        "mr_action": np.stack([flat("action", 0, i) for i in (0, 1)]).astype(np.int8),
        "mr_scores": np.stack([flat("scores", 0, i) for i in (0, 1)]).astype(np.float32),
        "mr_spread": flat("spread", 0, 0).astype(np.float32),
        "si_action": np.stack([flat("action", 1, i) for i in (0, 1)]).astype(np.int8),
        "si_scaled": np.stack([flat("scores", 1, i) for i in (0, 1)]).astype(np.float32),
        "si_mean": flat("mean", 1, 0).astype(np.float32),
        "si_max_diff": flat("max_diff", 1, 0).astype(np.float32),
    }


def write_state_pkl():
    """A ``state.pkl`` as the reference's Agent.save writes it (agent.py:194-203), holding both selectors."""
    state = {"action_selector": R.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, 0.8, None), "n_updates": 2,
             "eval_action_selector": R.MinRegretActionSelector(0.1, None), "max_grad_norm": 10.0, "use_cuda_graph": False}
    d = os.path.join(OUT, "ref_state_min_regret")
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "state.pkl"), "wb") as f:
        pickle.dump(state, f)


def main():
    steps, results = [], []
    for c in T.cases():
        step = 0
        while True:
            mr, si, ties = run_case(T.case_q(c, seed=1000 * c["index"] + step), c["unsquish"])
            if not ties.any():
                break
            step += 1
            assert step < 1000, c
        steps.append(step)
        results.append((mr, si))
    if tuple(steps) != tuple(T.SEED_STEP):
        print("tests/selector_cases.py: SEED_STEP = " + repr(tuple(steps)))
        print("(the table's seed steps leave rows near a tie: put the line above in and run again)")
        return 1
    out = pack(results)
    for name in T.GOLDEN_CASES:
        g = H.load_case(name)
        usq = str(H.case_overrides(g).get("loss_squish_fn_id", "none"))
        usq = usq if usq in UNSQUISH else "none"
        mr, si, ties = run_case(np.ascontiguousarray(g["act/q"], dtype=np.float32), usq)
        print(f"{name}: unsquish {usq}, q {g['act/q'].shape}, rows near a tie or ill-conditioned: {int(ties.sum())}")
        # (recorded inputs cannot be redrawn: the tests find these rows again from the recorded scores and hold their
        # values, not their actions)
        for k, v in pack([(mr, si)]).items():
            out[f"g/{name}/{k}"] = v
    path = os.path.join(OUT, "selectors_ref.npz")
    np.savez_compressed(path, **out)
    write_state_pkl()
    print(f"{path}: {os.path.getsize(path)} bytes, {out['mr_action'].shape[1]} rows, {out['mr_spread'].shape[0]} values")
    assert os.path.getsize(path) <= 100_000
    return 0


if __name__ == "__main__":
    sys.exit(main())
