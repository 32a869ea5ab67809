"""The supported (action count, channels, batch) envelope as a case table, shared by tests/test_gpu_envelope.py (the
kernels against the oracle) and tests/test_envelope_inputs.py (the envelope, the alignment facts and the inputs, checked
on the CPU by the oracle alone).

A case is everything that fixes its inputs: model configuration, A, C, B, the seed of the initial weights and the seed of
the minibatch generator.  The minibatch seeds are chosen on the CPU, by the oracle alone: ``python -m tests.envelope_cases``
walks seeds 1, 2, ... per case until no gradient tensor of any step moves by more than half its tolerance between the
oracle's fp32 and fp64 evaluations or under a two-ulp parameter jitter (``kink_report``), and prints the ones that are
not 1.  The kernels play no part in choosing their own inputs.  ``--independent`` runs the same search for the named cases
without `patterns` (row 8: why the B = 4096 cases do not use independent samples)."""
import numpy as np
import torch

from tests import helpers as H

INIT_SEED = 11


def _iqn(T, Tn=None, **kw):
    return dict(iqn_n_current_state_quantile_samples=T, iqn_n_next_state_quantile_samples=T if Tn is None else Tn, **kw)


FULL = dict(use_ids=True)                                                     # IQN + the ten-head Q ensemble
DQN1 = dict(use_iqn=False, use_dqn=True, dqn_n_model_layers=1)                # the single Linear(1024, A) head
TARGET_DQ = dict(use_target_network=True, use_double_q_learning=True)
RMSPROP, SGD = dict(use_adam=False, use_rmsprop=True), dict(use_adam=False, use_rmsprop=False)


def _case(A, C, B, over, steps=2, modes=("fp32", "bf16x3"), check_params=True, patterns=None, mixed_gamma=False):
    return dict(A=A, C=C, B=B, over=over, steps=steps, modes=modes, check_params=check_params, patterns=patterns,
                mixed_gamma=mixed_gamma)


UPDATE_CASES = {}
# 1: IQN, T = 8 (a 16-row tile holds two samples: the loss finishes inside the forward tiles)
for _A, _C in ((1, 4), (2, 2), (3, 1), (5, 4), (7, 3), (16, 10)):
    UPDATE_CASES[f"r1_iqn_t8_a{_A}c{_C}"] = _case(_A, _C, 32, {})
# 2: IQN, T = T' = 16 with a target network and double Q: the stand-alone loss kernel
for _A in (3, 16):
    UPDATE_CASES[f"r2_iqn_t16_target_dq_a{_A}"] = _case(_A, 4, 16, _iqn(16, **TARGET_DQ))
# 3: IQN + Q ensemble
for _A in (1, 3, 5, 16):
    for _C in (1, 4):
        UPDATE_CASES[f"r3_full_a{_A}c{_C}"] = _case(_A, _C, 32, dict(FULL))
UPDATE_CASES["r3_full_a3c4_target"] = _case(3, 4, 32, dict(FULL, use_target_network=True))
UPDATE_CASES["r3_full_a5c1_symlog"] = _case(5, 1, 32, dict(FULL, loss_squish_fn_id="symlog"))
# 4: one-layer DQN head
for _A in (1, 3, 16):
    for _ln in (True, False):
        UPDATE_CASES[f"r4_dqn1_{'ln' if _ln else 'noln'}_a{_A}"] = _case(_A, 4, 32, dict(DQN1, use_layer_norm=_ln))
# 5: width 256 (head code of fwd_tile_kernel<256>, iqn_bwd4_kernel, qh_bwd_kernel<256>)
UPDATE_CASES["r5_w256_iqn_t8_noln_a3"] = _case(3, 4, 32, dict(iqn_quantile_model_feature_dim=256, use_layer_norm=False))
UPDATE_CASES["r5_w256_full_a16"] = _case(16, 4, 32, dict(FULL, iqn_quantile_model_feature_dim=256, ids_q_head_feature_dim=256))
# 6: batch edges, IQN (B * T a multiple of 16 with B itself not)
for _B, _T in ((1, 16), (2, 8), (4, 4), (3, 16)):
    for _A in (6, 5):
        UPDATE_CASES[f"r6_iqn_b{_B}t{_T}_a{_A}"] = _case(_A, 4, _B, _iqn(_T))
# 7: batch edges, one-layer DQN (no B % 16 rule)
for _B in (1, 5, 17):
    for _ln in (True, False):
        UPDATE_CASES[f"r7_dqn1_{'ln' if _ln else 'noln'}_b{_B}"] = _case(6, 4, _B, dict(DQN1, use_layer_norm=_ln))
# 8: top of the batch range: one step, the fp32 GEMM chain, TD errors / loss / gradients.  The DQN case runs independent
#    random samples like every other row.  The IQN case cannot: its four million quantile-network ReLU units of independent
#    random inputs always hold a few within rounding distance of zero (the oracle's fp32 and fp64 gradients then differ by 3.5
#    to 122 tolerances over seeds 1..39: `python -m tests.envelope_cases --independent r8_iqn_t4_b4096`), so its minibatch
#    draws (observation, next observation, quantile samples) from 32 patterns, assigned to the 4096 positions at random,
#    while reward, action, end-of-episode flag and PER weight are drawn per sample: the pre-activations take the values of a
#    32-sample batch, every sample's loss and gradient differ, and a kernel that confuses two positions still fails (batch_of)
UPDATE_CASES["r8_iqn_t4_b4096"] = _case(6, 4, 4096, _iqn(4), steps=1, modes=("fp32",), check_params=False, patterns=32)
UPDATE_CASES["r8_dqn1_b4096"] = _case(6, 4, 4096, dict(DQN1, use_layer_norm=False), steps=1, modes=("fp32",), check_params=False)
# 9: centered RMSprop and SGD (prism_learner_clip_step: scalar tails of their own)
for _A in (3, 5):
    UPDATE_CASES[f"r9_rmsprop_a{_A}"] = _case(_A, 4, 32, dict(RMSPROP))
    UPDATE_CASES[f"r9_sgd_a{_A}"] = _case(_A, 4, 32, dict(SGD))
# 10: a discount per sample, drawn from {0.99, 0.99**2, 0.99**3} (every other row gives all samples 0.99**3)
UPDATE_CASES["r10_iqn_gammas_a5"] = _case(5, 4, 32, {}, mixed_gamma=True)

# Minibatch-generator seeds that are not 1 (chosen as the module docstring says)
BATCH_SEEDS = {}

# 1b: acting, one case per model kind and A
ACT_CASES = {f"{kind}_a{A}": dict(A=A, C=C, over=over)
             for kind, C, over in (("iqn", 4, {}), ("full", 3, dict(FULL)), ("dqn1", 4, dict(DQN1, use_layer_norm=True)))
             for A in (1, 3, 16)}

# 1c: the fused step forms at parameter counts that are 1 and 3 mod 4: (baseline configuration, A, C, overrides,
#     n_params % 4, first Q-head offset % 4 or None)
FUSED_CASES = {
    "iqn_a3": dict(base=2, A=3, C=4, over={}, rem=3, head_rem=None),
    "iqn_a5": dict(base=2, A=5, C=4, over={}, rem=1, head_rem=None),
    "full_a5": dict(base=3, A=5, C=4, over=dict(target_update_period=3), rem=3, head_rem=1),
    "dqn_a7": dict(base=0, A=7, C=4, over={}, rem=3, head_rem=0),
    "iqn_rmsprop_a3": dict(base=2, A=3, C=4, over=dict(RMSPROP), rem=3, head_rem=None),
}


def case_config(name, device="cpu", **extra):
    return H.variant_config(device, dict(UPDATE_CASES[name]["over"], **extra))


def layout(sd):
    """(n_params, {state_dict key: flat offset}) of the unpadded flat parameter buffer (parameters() order)."""
    off, table = 0, {}
    for k, v in sd.items():
        table[k] = off
        off += v.numel()
    return off, table


def first_head_offset(table):
    heads = [o for k, o in table.items() if k.startswith("q_function_model.q_heads.0.")]
    return min(heads) if heads else None


def batch_of(rng, case, cfg):
    """The minibatch, PER weights and quantile samples of one step of a case (helpers.random_batch; see row 8 for
    `patterns`)."""
    A, C, B, P = case["A"], case["C"], case["B"], case["patterns"]
    if P is None:
        return H.random_batch(rng, B, C, A, cfg, mixed_gamma=True) if case.get("mixed_gamma") else H.random_batch(rng, B, C, A, cfg)
    pat, _, ptaus = H.random_batch(rng, P, C, A, cfg)
    batch, w, _ = H.random_batch(rng, B, C, A, cfg)
    pid = torch.from_numpy(rng.integers(0, P, B))
    batch["obs"], batch["next_obs"] = pat["obs"][pid], pat["next_obs"][pid]
    # quantile samples are tau-major: row t * B + b
    taus = [t.view(-1, P)[:, pid].reshape(-1, 1).contiguous() for t in ptaus]
    return batch, w, taus


_RUNS = {}


def oracle_run(name):
    """The oracle's trajectory of a case, evaluated once for both GEMM modes: (cpu_cfg, spec, initial state dict, steps);
    a step records its inputs, the parameters before it and the oracle's TD errors, loss, gradients and parameters after."""
    if name not in _RUNS:
        from oracle.learner_ref import LearnerOracle
        from tests.test_optimizers import swap_optimizer
        case = UPDATE_CASES[name]
        A, C, B = case["A"], case["C"], case["B"]
        cfg = case_config(name)
        sd, tgt = H.build_init_state(cfg, INIT_SEED, C=C, A=A)
        spec = H.spec_from_config(cfg, C=C, A=A)
        orc = swap_optimizer(LearnerOracle(sd, spec, tgt), cfg)
        rng = np.random.default_rng(BATCH_SEEDS.get(name, 1))
        steps = []
        for step in range(case["steps"]):
            batch, w, taus = batch_of(rng, case, cfg)
            rec = dict(batch=batch, w=w, taus=taus, pre_sd=orc.state_dict(), jitter=None,
                       pre_tgt=None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()})
            rec["td"] = orc.update(batch, w, taus)
            rec["total"], rec["grads"], rec["post"] = float(orc.last["total"]), orc.last["grads"], orc.state_dict()
            steps.append(rec)
            if cfg.use_target_network and step == 0:
                orc.sync_target()
        _RUNS[name] = (cfg, spec, sd, steps)
    return _RUNS[name]


def forget(name):
    """Drop the cached trajectory of a case (it holds the minibatches: 4096 observations at the top of the range)."""
    _RUNS.pop(name, None)


def grad_tolerance(g):
    """The project's gradient tolerance of one tensor (tests/test_gpu_learner.py)."""
    return 1e-4 * float(g.abs().max()) + 1e-7


def jitter_of(rec, spec, step):
    if rec["jitter"] is None:
        rec["jitter"] = H.jitter_grads(rec["pre_sd"], rec["pre_tgt"], spec, rec["batch"], rec["w"], rec["taus"], seed=77 + step)
    return rec["jitter"]


def kink_report(name):
    """Per (step, tensor): (the oracle's fp32 / fp64 gradient gap, the largest move under helpers.jitter_grads, the tensor's
    tolerance) -- the oracle measured against itself at the inputs of a case."""
    from oracle.learner_ref import LearnerOracle
    cfg, spec, sd, steps = oracle_run(name)
    out = []
    for step, rec in enumerate(steps):
        probe = LearnerOracle(rec["pre_sd"], spec, rec["pre_tgt"])
        g64 = probe.grads_fp64(rec["batch"], rec["w"], rec["taus"])
        jit = jitter_of(rec, spec, step)
        for k, g in rec["grads"].items():
            gap = float((g.double() - g64[k]).abs().max())
            move = max(float((jg[k] - g).abs().max()) for jg in jit)
            out.append((step, k, gap, move, grad_tolerance(g)))
    return out


def worst_kink(name):
    """The largest of gap / tolerance and move / tolerance over a case: the inputs are kink-free when it is <= 0.5."""
    return max(max(gap, move) / tol for _, _, gap, move, tol in kink_report(name))


if __name__ == "__main__":
    # python -m tests.envelope_cases [--independent] [case ...]: the seed search.  --independent drops `patterns` from the
    # named cases (row 8 with independent random samples: the search then reports every seed it refuses and fails)
    import sys
    args = sys.argv[1:]
    independent = "--independent" in args
    names = [a for a in args if a != "--independent"] or list(UPDATE_CASES)
    for name in names:
        if independent:
            UPDATE_CASES[name]["patterns"] = None
        for seed in range(1, 40):
            BATCH_SEEDS[name] = seed
            forget(name)
            worst = worst_kink(name)
            if worst <= 0.5:
                break
            print(f"# {name}: seed {seed} refused, worst ratio {worst:.2f}", flush=True)
        else:
            raise SystemExit(f"{name}: no kink-free seed below 40")
        print(f"{name!r}: {seed},   # worst ratio {worst:.3f}", flush=True)
        forget(name)
