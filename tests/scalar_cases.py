"""What the tests away from the presets' scalars share: the fixtures' oracle trajectories (tests/test_scalar_case_inputs.py
shows on the CPU, by the oracle alone, that the inputs reach what they are meant to reach), the Theil-gradient differential
(tests/test_gpu_scalars.py) and the selector's random estimates (tests/test_gpu_acting.py)."""
import numpy as np
import torch

from tests import helpers as H

FIXTURES = H.SCALAR_CASES + ["dqn_rmsprop_scalars"]

# ---- the Theil gradient in isolation: the full_scalars inputs, step 0, at ids_ensemble_variation_coef = THEIL_C and at 0.
# The term's gradient on head h is c * q_w * mean(w) * (log r_h - theil) / (n_heads * mean norm) * theta / |theta_h|, r_h the
# head's norm over the mean norm: linear in the coefficient, exactly zero on tensors that are zero (the biases of the heads'
# LayerNorms at initialisation), and small on the head whose log r_h is close to the index itself (head 5 at head_scale
# (0.55, 0.1): 2.9 rounding terms at c = 8).  64 puts the difference of the two gradients >= 20 rounding terms above zero on
# every nonzero head tensor (23.5 on the weakest; asserted by tests/test_scalar_case_inputs.py).
THEIL_CASE, THEIL_C = "full_scalars", 64.0
FP32_EPS = 2.0 ** -23
HEAD_PREFIX = "q_function_model.q_heads."


def oracle_for(name, **extra):
    """(fixture, cpu config, spec, a fresh LearnerOracle with the optimizer the configuration asks for)."""
    from oracle.learner_ref import LearnerOracle
    from tests.test_optimizers import swap_optimizer
    g = H.load_case(name)
    cfg = H.case_config(g, **extra)
    C, A = int(g["C"]), int(g["A"])
    sd, tgt = H.build_init_state(cfg, int(g["seed"]), C=C, A=A, head_scale=H.case_head_scale(g))
    spec = H.spec_from_config(cfg, C=C, A=A)
    return g, cfg, spec, swap_optimizer(LearnerOracle(sd, spec, tgt), cfg)


_RUNS = {}


def oracle_run(name):
    """Per step of a fixture, from the oracle alone: quadratic-branch share (None without an IQN loss), gradient norm, Theil
    index (None without a Q ensemble), the batch's gammas and terminal count."""
    if name not in _RUNS:
        g, cfg, spec, orc = oracle_for(name)
        steps = []
        for step in range(int(g["steps"])):
            batch, w, taus = H.case_batch(g, step)
            orc.update(batch, w, taus)
            theil = orc.last.get("theil")
            steps.append(dict(quad_share=orc.last.get("quad_share"), grad_norm=float(orc.last["grad_norm"]),
                              theil=None if theil is None else float(theil.detach()),
                              gammas=np.unique(batch["gamma"].numpy()), terminals=int((~batch["nonterminal"].bool()).sum())))
            if cfg.use_target_network and step == 0:
                orc.sync_target()
        _RUNS[name] = (cfg, steps)
    return _RUNS[name]


def worst_kink(name, draws=12):
    """The oracle measured against itself at the inputs of a fixture, as tests/envelope_cases.py does for its seeds: over all
    steps and tensors, the larger of the fp32 / fp64 gradient gap and the largest move under helpers.jitter_grads, in units of
    the tensor's gradient tolerance.  <= 0.5: no ReLU unit sits within rounding distance of zero."""
    g, cfg, spec, orc = oracle_for(name)
    worst = 0.0
    for step in range(int(g["steps"])):
        batch, w, taus = H.case_batch(g, step)
        g64 = orc.grads_fp64(batch, w, taus)
        pre_sd = orc.state_dict()
        pre_tgt = None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()}
        orc.update(batch, w, taus)
        jit = H.jitter_grads(pre_sd, pre_tgt, spec, batch, w, taus, seed=99 + step, draws=draws)
        for k, go in orc.last["grads"].items():
            tol = 1e-4 * float(go.abs().max()) + 1e-7
            gap = float((go.double() - g64[k]).abs().max())
            move = max(float((j[k] - go).abs().max()) for j in jit)
            worst = max(worst, max(gap, move) / tol)
        if cfg.use_target_network and step == 0:
            orc.sync_target()
    return worst


_THEIL = {}


def theil_reference():
    """The oracle at THEIL_C and at 0 on step 0 of THEIL_CASE: dict(names, g = fp64 gradient at THEIL_C, delta = the
    difference of the two fp64 gradients, theil, total_c, total_0, q_w, w_mean, batch, w, taus, zero = the names of the
    tensors that are all zero before the step)."""
    if not _THEIL:
        out = {}
        for tag, c in (("c", THEIL_C), ("0", 0.0)):
            g, cfg, spec, orc = oracle_for(THEIL_CASE, ids_ensemble_variation_coef=c)
            batch, w, taus = H.case_batch(g, 0)
            out["g64_" + tag] = orc.grads_fp64(batch, w, taus)
            orc.update(batch, w, taus, apply=False)
            out["total_" + tag] = float(orc.last["total"])
            if c:
                out["theil"] = float(orc.last["theil"].detach())
        out.update(names=list(out["g64_c"]), g=out["g64_c"], q_w=cfg.q_loss_weight, w_mean=float(w.double().mean()),
                   delta={k: out["g64_c"][k] - out["g64_0"][k] for k in out["g64_c"]}, batch=batch, w=w, taus=taus,
                   zero={k for k, v in orc.p.items() if not bool(v.detach().any())})
        _THEIL.update(out)
    return _THEIL


def theil_rounding_term(ref, k):
    """fp32 roundings of forming g + kappa_h * theta twice and subtracting: four roundings at the size of the gradient."""
    return 4.0 * FP32_EPS * max(float(ref["g64_c"][k].abs().max()), float(ref["g64_0"][k].abs().max()))


# ---- prism_ids_select on random estimates (tests/test_gpu_acting.py): the scalars, the shapes, the estimates
IDS_SELECT_SCALARS = [(0.1, 1e-10, 0.25), (0.5, 1e-3, 0.05), (0.0, 1e-10, 1.0)]          # (lambda, epsilon, rho_min)
IDS_SELECT_SHAPES = ((1, 200, 6, 10), (7, 32, 3, 2), (33, 200, 16, 10), (4, 1, 6, 1))      # (n, T, A, heads)
IDS_SCORE_RTOL, IDS_SCORE_ATOL = 2e-4, 1e-7


def ids_select_estimates():
    """[(n, T, A, heads, dist (T,n,A), q (n,A,heads))]: the same draws for every scalar triple."""
    rng = np.random.default_rng(11)
    out = []
    for n, T, A, heads in IDS_SELECT_SHAPES:
        dist = torch.from_numpy(rng.standard_normal((T, n, A)).astype(np.float32) * 2.0 + 1.0)
        q = torch.from_numpy(rng.standard_normal((n, A, heads)).astype(np.float32))
        out.append((n, T, A, heads, dist, q))
    return out


def ids_ambiguous_rows(scores):
    """Rows whose two smallest oracle scores lie within the score tolerance of each other: either action is a correct
    argmin of scores that are only held to that tolerance.  scores: (n, A) array; returns a bool array (n,)."""
    s = np.sort(np.asarray(scores, np.float64), axis=-1)
    if s.shape[-1] < 2:
        return np.zeros(s.shape[0], bool)
    tol = lambda x: IDS_SCORE_RTOL * np.abs(x) + IDS_SCORE_ATOL
    return s[:, 1] - s[:, 0] <= tol(s[:, 0]) + tol(s[:, 1])
