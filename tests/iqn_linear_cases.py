"""The linear IQN head (iqn_quantile_model_layers = 0) as a case table, shared by tests/test_gpu_iqn_linear.py (the kernels
against the oracle) and tests/test_iqn_linear_host.py (envelope, offsets and inputs, on the CPU by the oracle alone).

The generated cases are the smallest shapes at which the linear-head kernels can go wrong, not the workload's: one sample
per 16-row tile (B = 1, T = 16), a sample spread over four tiles (T = 64), T != T', four samples in a tile (T = 4), odd
batches (3, 17); action counts 1, 2, 3, 16 (every remainder of n_params % 4 = A % 4, and the padded action columns of the
head product full and nearly empty); 1 and 10 observation channels; LayerNorm on and off; with and without a target network
and double Q.  Each axis value meets each LayerNorm setting; the table is not the full product.

Minibatch seeds are chosen as tests/envelope_cases.py chooses them: ``python -m tests.iqn_linear_cases`` walks seeds
1, 2, ... per case until the oracle's fp32 / fp64 gradients and six two-ulp parameter jitters agree within half the gradient
tolerance on every tensor of every step, and prints the ones that are not 1.  The kernels play no part in it."""
import numpy as np

from tests import envelope_cases as E
from tests import helpers as H

INIT_SEED = 11
FIXTURES = ["iqn_l0", "iqn_l0_noln_dq"]


def _case(B, T, Tn, ln, A, C, tdq, steps=2):
    over = dict(iqn_quantile_model_layers=0, use_layer_norm=ln, iqn_n_current_state_quantile_samples=T,
                iqn_n_next_state_quantile_samples=Tn)
    if tdq:
        over.update(E.TARGET_DQ)
    return dict(A=A, C=C, B=B, over=over, steps=steps, patterns=None)


def _name(B, T, Tn, ln, A, C, tdq):
    return f"b{B}t{T}{'' if Tn == T else f'n{Tn}'}_{'ln' if ln else 'noln'}_a{A}c{C}{'_tdq' if tdq else ''}"


UPDATE_CASES = {_name(*row): _case(*row) for row in (
    # B, T, T', LayerNorm, A, C, target + double Q
    (1, 16, 16, True, 1, 1, False), (1, 16, 16, False, 16, 10, True),
    (1, 64, 64, True, 2, 10, True), (1, 64, 64, False, 3, 1, False),
    (2, 8, 16, True, 3, 1, True), (2, 8, 16, False, 2, 10, False),
    (4, 4, 4, True, 16, 10, False), (4, 4, 4, False, 1, 1, True),
    (3, 16, 16, True, 2, 1, False), (3, 16, 16, False, 3, 10, True),
    (17, 16, 16, True, 3, 10, True), (17, 16, 16, False, 16, 1, False))}

# Minibatch-generator seeds that are not 1 (chosen as the module docstring says)
BATCH_SEEDS = {}


def case_config(name, device="cpu", **extra):
    return H.variant_config(device, dict(UPDATE_CASES[name]["over"], **extra))


_RUNS = {}


def oracle_run(name):
    """The oracle's trajectory of a case, evaluated once for both GEMM modes (as tests/envelope_cases.py oracle_run)."""
    if name not in _RUNS:
        from oracle.learner_ref import LearnerOracle
        case = UPDATE_CASES[name]
        A, C = case["A"], case["C"]
        cfg = case_config(name)
        sd, tgt = H.build_init_state(cfg, INIT_SEED, C=C, A=A)
        spec = H.spec_from_config(cfg, C=C, A=A)
        orc = LearnerOracle(sd, spec, tgt)
        rng = np.random.default_rng(BATCH_SEEDS.get(name, 1))
        steps = []
        for step in range(case["steps"]):
            batch, w, taus = E.batch_of(rng, case, cfg)
            rec = dict(batch=batch, w=w, taus=taus, pre_sd=orc.state_dict(), jitter=None,
                       pre_tgt=None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()})
            rec["g64"] = orc.grads_fp64(batch, w, taus)
            rec["td"] = orc.update(batch, w, taus)
            rec["total"], rec["grads"], rec["post"] = float(orc.last["total"]), orc.last["grads"], orc.state_dict()
            rec["grad_norm"] = float(orc.last["grad_norm"])
            steps.append(rec)
            if cfg.use_target_network and step == 0:
                orc.sync_target()
        _RUNS[name] = (cfg, spec, sd, steps)
    return _RUNS[name]


def forget(name):
    _RUNS.pop(name, None)


def kink_rows(spec, rec, step):
    """Per tensor of one recorded step: (name, the oracle's fp32 / fp64 gradient gap, the largest move under
    helpers.jitter_grads, the tensor's tolerance)."""
    jit = E.jitter_of(rec, spec, step)
    return [(k, float((g.double() - rec["g64"][k]).abs().max()), max(float((jg[k] - g).abs().max()) for jg in jit),
             E.grad_tolerance(g)) for k, g in rec["grads"].items()]


def kink_report(name):
    cfg, spec, sd, steps = oracle_run(name)
    return [(step,) + row for step, rec in enumerate(steps) for row in kink_rows(spec, rec, step)]


def fixture_run(name):
    """The same record for a fixture recorded from the live reference: (cpu_cfg, spec, initial state dict, steps)."""
    key = "fixture/" + name
    if key not in _RUNS:
        from oracle.learner_ref import LearnerOracle
        g = H.load_case(name)
        A, C = int(g["A"]), int(g["C"])
        cfg = H.case_config(g)
        sd, tgt = H.build_init_state(cfg, int(g["seed"]), C=C, A=A)
        spec = H.spec_from_config(cfg, C=C, A=A)
        orc = LearnerOracle(sd, spec, tgt)
        steps = []
        for step in range(int(g["steps"])):
            batch, w, taus = H.case_batch(g, step)
            rec = dict(batch=batch, w=w, taus=taus, pre_sd=orc.state_dict(), jitter=None,
                       pre_tgt=None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()})
            rec["g64"] = orc.grads_fp64(batch, w, taus)
            rec["td"] = orc.update(batch, w, taus)
            rec["total"], rec["grads"], rec["post"] = float(orc.last["total"]), orc.last["grads"], orc.state_dict()
            rec["grad_norm"] = float(orc.last["grad_norm"])
            steps.append(rec)
            if cfg.use_target_network and step == 0:
                orc.sync_target()
        _RUNS[key] = (cfg, spec, sd, steps)
    return _RUNS[key]


if __name__ == "__main__":
    import sys
    for name in sys.argv[1:] or list(UPDATE_CASES):
        for seed in range(1, 40):
            BATCH_SEEDS[name] = seed
            forget(name)
            worst = max(max(gap, move) / tol for _, _, gap, move, tol in kink_report(name))
            if worst <= 0.5:
                break
            print(f"# {name}: seed {seed} refused, worst ratio {worst:.2f}", flush=True)
        else:
            raise SystemExit(f"{name}: no kink-free seed below 40")
        print(f"{name!r}: {seed},   # worst ratio {worst:.3f}", flush=True)
        forget(name)
