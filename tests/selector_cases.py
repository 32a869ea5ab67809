"""The seeded input table of the MinRegret / SimpleIDS selector tests (tests/test_selectors_host.py,
tests/test_gpu_selectors.py) and of the fixture generator (tools/gen_selector_golden.py), which runs the live reference's
two classes on exactly these inputs and writes tests/golden/selectors_ref.npz -- outputs only; the inputs are redrawn here.

Every (A, heads, unsquish) combination is a case; n walks its four values so that every (n, A), (n, heads) and
(n, unsquish) pair occurs; every case runs at both lambdas (MinRegret) and both betas (SimpleIDS).  The whole cross
product with n as well would be four times the rows, and the recorded values alone would not fit the fixture's 100 KB.

``q = N(0, 1)[n, A, 1] + 0.5 N(0, 1)[n, A, heads]`` in fp32: a per-action level the heads agree on plus their disagreement.
A case's seed is ``1000 * index + SEED_STEP[index]``: the generator walked ``SEED_STEP`` up from 0 until no row of the case,
at either lambda or beta, was NEAR A TIE in the reference's own scores -- best and runner-up closer than
``margin(unsquish) * (1 + |best|)``, five times the value tolerance: on the rows kept a different action is a bug, not
rounding -- or ILL-CONDITIONED: a recorded value that the reference's own fp32 rounding inside the unsquish function moves by
more than half its tolerance (the same classes with that function evaluated in float64; tools/gen_selector_golden.py).
The walk looks at the reference alone."""
import numpy as np

NS = (1, 5, 17, 33)
AS = (1, 2, 6, 16)
HEADS = (2, 10, 16)
UNSQUISH = ("none", "obs_look_further", "symlog")          # PRISM_SQUISH_* 0, 1, 2
LAMBDAS = (0.1, 1.0)
BETAS = (0.8, 0.5)
GOLDEN_CASES = ("full_small", "full_c4", "full_olf")          # tests/golden/update_<name>.npz: their ``act/q``

# value tolerances (rtol, atol): tests/test_gpu_acting.py holds the IDS scores to the same
TOL = {False: (2e-4, 1e-7), True: (1e-3, 1e-6)}


def tol(unsquish):
    return TOL[unsquish != "none"]


def margin(unsquish):
    return 1e-3 if unsquish == "none" else 5e-3


SEED_STEP = (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 5, 0, 0, 0, 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1)


def cases():
    out = []
    for ia, A in enumerate(AS):
        for ih, heads in enumerate(HEADS):
            for iu, usq in enumerate(UNSQUISH):
                i = len(out)
                out.append(dict(index=i, n=NS[(ia + ih + iu) % 4], A=A, heads=heads, unsquish=usq,
                                seed=1000 * i + SEED_STEP[i]))
    return out


def case_q(case, seed=None):
    """``[n, A, heads]`` fp32."""
    rng = np.random.default_rng(case["seed"] if seed is None else seed)
    n, A, heads = case["n"], case["A"], case["heads"]
    level = rng.standard_normal((n, A, 1)).astype(np.float32)
    return level + np.float32(0.5) * rng.standard_normal((n, A, heads)).astype(np.float32)


def layout():
    """Where each case's rows and values lie in the fixture's flat arrays: ``[(row_lo, row_hi, value_lo, value_hi)]``."""
    out, r, v = [], 0, 0
    for c in cases():
        out.append((r, r + c["n"], v, v + c["n"] * c["A"]))
        r, v = out[-1][1], out[-1][3]
    return out


def near_ties(scores, unsquish, largest):
    """Rows of ``scores [n, A]`` whose best and runner-up are within the margin (``largest``: arg-max, else arg-min)."""
    s = np.sort(np.asarray(scores, dtype=np.float64), axis=-1)
    if s.shape[-1] < 2:
        return np.zeros(s.shape[0], dtype=bool)
    best, second = (s[:, -1], s[:, -2]) if largest else (s[:, 0], s[:, 1])
    return np.abs(best - second) < margin(unsquish) * (1 + np.abs(best))
