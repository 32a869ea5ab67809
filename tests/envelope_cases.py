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


def _case(A, C, B, over, steps=2, modes=("fp32", "bf16x3"), check_params=True, patterns=None, mixed_gamma=False, expect=None):
    """`expect`: the fields of prism_learner_plan_info (prism_amd/_native.py PLAN_FIELDS) the case exists for -- one dict for
    all its modes, or one per mode; tests/test_envelope_inputs.py holds the library's plan to it, so a case written for one
    launch form cannot silently turn into a case of another."""
    return dict(A=A, C=C, B=B, over=over, steps=steps, modes=modes, check_params=check_params, patterns=patterns,
                mixed_gamma=mixed_gamma, expect=expect)


def _x(bwd, conv=0, q_bwd="none", chunks=8, **more):
    return dict(bwd=bwd, conv_in_bwd=conv, q_bwd=q_bwd, n_chunks=chunks, **more)


BF16 = ("bf16x3",)
UPDATE_CASES = {}
# 1: IQN, T = 8 (a 16-row tile holds two samples: the loss finishes inside the forward tiles)
for _A, _C in ((1, 4), (2, 2), (3, 1), (5, 4), (7, 3), (16, 10)):
    UPDATE_CASES[f"r1_iqn_t8_a{_A}c{_C}"] = _case(_A, _C, 32, {}, expect=_x("fp32", int(_C in (2, 4)), local_loss=1))
# 2: IQN, T = T' = 16 with a target network and double Q: the stand-alone loss kernel
for _A in (3, 16):
    UPDATE_CASES[f"r2_iqn_t16_target_dq_a{_A}"] = _case(_A, 4, 16, _iqn(16, **TARGET_DQ),
                                                        expect=_x("fp32", 1, local_loss=0, merged_loss=0))
# 3: IQN + Q ensemble
for _A in (1, 3, 5, 16):
    for _C in (1, 4):
        UPDATE_CASES[f"r3_full_a{_A}c{_C}"] = _case(_A, _C, 32, dict(FULL), expect=_x("fp32", 0, "cols", local_loss=1, q_de_slots=10))
UPDATE_CASES["r3_full_a3c4_target"] = _case(3, 4, 32, dict(FULL, use_target_network=True),
                                            expect=_x("fp32", 0, "cols", local_loss=0, merged_loss=1))
UPDATE_CASES["r3_full_a5c1_symlog"] = _case(5, 1, 32, dict(FULL, loss_squish_fn_id="symlog"), expect=_x("fp32", 0, "cols"))
# 4: one-layer DQN head
for _A in (1, 3, 16):
    for _ln in (True, False):
        UPDATE_CASES[f"r4_dqn1_{'ln' if _ln else 'noln'}_a{_A}"] = _case(_A, 4, 32, dict(DQN1, use_layer_norm=_ln), expect=_x("none"))
# 5: width 256 (head code of fwd_tile_kernel<256>, iqn_bwd4_kernel, qh_bwd_kernel<256>)
UPDATE_CASES["r5_w256_iqn_t8_noln_a3"] = _case(3, 4, 32, dict(iqn_quantile_model_feature_dim=256, use_layer_norm=False),
                                               expect=dict(fp32=_x("fp32", 1, chunks=4), bf16x3=_x("bw4", 0, chunks=8)))
UPDATE_CASES["r5_w256_full_a16"] = _case(16, 4, 32, dict(FULL, iqn_quantile_model_feature_dim=256, ids_q_head_feature_dim=256),
                                         expect=dict(fp32=_x("fp32", 0, "cols", chunks=4), bf16x3=_x("bw4", 0, "cols", chunks=8)))
# 6: batch edges, IQN (B * T a multiple of 16 with B itself not)
for _B, _T in ((1, 16), (2, 8), (4, 4), (3, 16)):
    for _A in (6, 5):
        UPDATE_CASES[f"r6_iqn_b{_B}t{_T}_a{_A}"] = _case(_A, 4, _B, _iqn(_T), expect=_x("fp32", int(_T != 4), local_loss=int(_T <= 8)))
# 7: batch edges, one-layer DQN (no B % 16 rule)
for _B in (1, 5, 17):
    for _ln in (True, False):
        UPDATE_CASES[f"r7_dqn1_{'ln' if _ln else 'noln'}_b{_B}"] = _case(6, 4, _B, dict(DQN1, use_layer_norm=_ln), expect=_x("none"))
# 8: top of the batch range: one step, the fp32 GEMM chain, TD errors / loss / gradients.  The DQN case runs independent
#    random samples like every other row.  The IQN case cannot: its four million quantile-network ReLU units of independent
#    random inputs always hold a few within rounding distance of zero (the oracle's fp32 and fp64 gradients then differ by 3.5
#    to 122 tolerances over seeds 1..39: `python -m tests.envelope_cases --independent r8_iqn_t4_b4096`), so its minibatch
#    draws (observation, next observation, quantile samples) from 32 patterns, assigned to the 4096 positions at random,
#    while reward, action, end-of-episode flag and PER weight are drawn per sample: the pre-activations take the values of a
#    32-sample batch, every sample's loss and gradient differ, and a kernel that confuses two positions still fails (batch_of)
UPDATE_CASES["r8_iqn_t4_b4096"] = _case(6, 4, 4096, _iqn(4), steps=1, modes=("fp32",), check_params=False, patterns=32,
                                        expect=_x("fp32", 0))
UPDATE_CASES["r8_dqn1_b4096"] = _case(6, 4, 4096, dict(DQN1, use_layer_norm=False), steps=1, modes=("fp32",), check_params=False,
                                      expect=_x("none"))
# 9: centered RMSprop and SGD (prism_learner_clip_step: scalar tails of their own)
for _A in (3, 5):
    UPDATE_CASES[f"r9_rmsprop_a{_A}"] = _case(_A, 4, 32, dict(RMSPROP), expect=_x("fp32", 1))
    UPDATE_CASES[f"r9_sgd_a{_A}"] = _case(_A, 4, 32, dict(SGD), expect=_x("fp32", 1))
# 10: a discount per sample, drawn from {0.99, 0.99**2, 0.99**3} (every other row gives all samples 0.99**3)
UPDATE_CASES["r10_iqn_gammas_a5"] = _case(5, 4, 32, {}, mixed_gamma=True, expect=_x("fp32", 1))

# Rows 11-16: every backward form the plan can pick (prism_amd/csrc/plan.h make_plan), away from A = 6, C = 4.  Rows 1-10 run
# B <= 32 (or B = 4096 in fp32 mode), where both GEMM modes take iqn_bwd_kernel and qh_bwd_kernel by columns; the forms the
# default configuration and the benchmark run -- iqn_bwd3_kernel (B * T % 512 == 0, bf16x3), qh_bwd2_kernel (B % 128 == 0) --
# start above that.  A row runs the one mode that selects its form unless it says otherwise.
# 11: iqn_bwd3_kernel, T = 8.  B = 64: one 32-row block per row chunk; B = 128: two.  The conv backward is folded into the
#     launch for C = 2 (one channel per lane) and C = 4 (two), and stays with the post launch for every other C
UPDATE_CASES["r11_bw3_t8_a3c2"] = _case(3, 2, 64, {}, modes=BF16, expect=_x("bw3", 1, chunks=16, local_loss=1))
UPDATE_CASES["r11_bw3_t8_a16c7"] = _case(16, 7, 64, {}, modes=BF16, expect=_x("bw3", 0, chunks=16))
UPDATE_CASES["r11_bw3_t8_a1c4_b128"] = _case(1, 4, 128, {}, modes=BF16, expect=_x("bw3", 1, chunks=16))
UPDATE_CASES["r11_bw3_t8_noln_a5c10"] = _case(5, 10, 64, dict(use_layer_norm=False), modes=BF16, expect=_x("bw3", 0, chunks=16))
# 12: iqn_bwd3_kernel at the other T.  T >= 16: four lanes share a (sample, position), conv folded in for C = 4 (one channel per
#     lane) and C = 8 (two); T = 4: never folded in (bw3_conv_ok wants T >= 8).  a5c8 runs the fp32 mode too: there it is
#     iqn_bwd_kernel with the conv taps inside at two channels per lane, which no other case reaches at a C other than 2 or 4
UPDATE_CASES["r12_bw3_t16_a5c8"] = _case(5, 8, 32, _iqn(16), expect=dict(fp32=_x("fp32", 1), bf16x3=_x("bw3", 1, chunks=16, local_loss=0)))
UPDATE_CASES["r12_bw3_t16_a2c10"] = _case(2, 10, 32, _iqn(16), modes=BF16, expect=_x("bw3", 0, chunks=16))
UPDATE_CASES["r12_bw3_t32_a7c1"] = _case(7, 1, 16, _iqn(32), modes=BF16, expect=_x("bw3", 0, chunks=16))
UPDATE_CASES["r12_bw3_t64_target_dq_a16c4"] = _case(16, 4, 16, _iqn(64, **TARGET_DQ), modes=BF16,
                                                    expect=_x("bw3", 1, chunks=16, local_loss=0, merged_loss=0))
UPDATE_CASES["r12_bw3_t4_a5c3"] = _case(5, 3, 128, _iqn(4), modes=BF16, expect=_x("bw3", 0, chunks=16, local_loss=1))
# 13: the staging bound of the folded conv backward, bw3_samples * 10 * C <= 1024: at C = 8, T = 16 it holds up to B = 192
#     (12 samples per row chunk) and fails from B = 224 (14).  One step; `patterns` as in row 8 and for its reason (3072 and
#     3584 rows x 128 trunk units of independent inputs were not searched for a kink-free seed)
UPDATE_CASES["r13_bw3_t16_a3c8_b192"] = _case(3, 8, 192, _iqn(16), steps=1, modes=BF16, patterns=32, expect=_x("bw3", 1, chunks=16))
UPDATE_CASES["r13_bw3_t16_a3c8_b224"] = _case(3, 8, 224, _iqn(16), steps=1, modes=BF16, patterns=32, expect=_x("bw3", 0, chunks=16))
# 14: qh_bwd2_kernel (B % 128 == 0, >= 2 heads, bf16x3) beside iqn_bwd3_kernel: ten heads, the fewest (2) and the most (16) the
#     kernel takes, a target network (the merged loss launch); and at B = 64 qh_bwd_kernel by columns beside iqn_bwd3_kernel
for _A, _C in ((1, 10), (3, 1), (16, 4)):
    UPDATE_CASES[f"r14_qb2_a{_A}c{_C}"] = _case(_A, _C, 128, dict(FULL), modes=BF16, expect=_x("bw3", 0, "qb2", chunks=16, q_de_slots=2))
UPDATE_CASES["r14_qb2_heads2_a5c4"] = _case(5, 4, 128, dict(FULL, ids_n_q_heads=2), modes=BF16, expect=_x("bw3", 0, "qb2", chunks=16))
UPDATE_CASES["r14_qb2_heads16_a5c4"] = _case(5, 4, 128, dict(FULL, ids_n_q_heads=16), modes=BF16, expect=_x("bw3", 0, "qb2", chunks=16))
UPDATE_CASES["r14_qb2_target_a3c4"] = _case(3, 4, 128, dict(FULL, use_target_network=True), modes=BF16,
                                            expect=_x("bw3", 0, "qb2", chunks=16, local_loss=0, merged_loss=1))
UPDATE_CASES["r14_cols_b64_a5c1"] = _case(5, 1, 64, dict(FULL), modes=BF16, expect=_x("bw3", 0, "cols", chunks=16, q_de_slots=10))
UPDATE_CASES["r14_cols_b64_a2c7"] = _case(2, 7, 64, dict(FULL), modes=BF16, expect=_x("bw3", 0, "cols", chunks=16, q_de_slots=10))
# 15: qh_bwd_kernel by rows (B > 128 where qh_bwd2_kernel does not apply); B * T = 1152 leaves the trunk to iqn_bwd_kernel
UPDATE_CASES["r15_rows_b144_a3c4"] = _case(3, 4, 144, dict(FULL), expect=_x("fp32", 0, "rows", q_de_slots=10))
UPDATE_CASES["r15_rows_b144_a16c1"] = _case(16, 1, 144, dict(FULL), modes=BF16, expect=_x("fp32", 0, "rows", q_de_slots=10))
UPDATE_CASES["r15_rows_b144_a5c7"] = _case(5, 7, 144, dict(FULL), modes=BF16, expect=_x("fp32", 0, "rows", q_de_slots=10))
# 16: width 256 at small batches: iqn_bwd4_kernel with two row chunks and with one (bw4_chunks), and B * T = 16, which no
#     chunk count divides into 32-row blocks: iqn_bwd_kernel<256> in the bf16x3 mode
W256 = dict(iqn_quantile_model_feature_dim=256)
UPDATE_CASES["r16_w256_t4_b16_a5c3"] = _case(5, 3, 16, _iqn(4, **W256), modes=BF16, expect=_x("bw4", 0, chunks=2))
UPDATE_CASES["r16_w256_t4_b8_a16c10"] = _case(16, 10, 8, _iqn(4, **W256), modes=BF16, expect=_x("bw4", 0, chunks=1))
UPDATE_CASES["r16_w256_t8_b4_a3c4"] = _case(3, 4, 4, _iqn(8, **W256), modes=BF16, expect=_x("bw4", 0, chunks=1))
UPDATE_CASES["r16_w256_t4_b4_a5c4"] = _case(5, 4, 4, _iqn(4, **W256), modes=BF16, expect=_x("fp32", 0, chunks=4, split=1))

# Minibatch-generator seeds that are not 1 (chosen as the module docstring says)
BATCH_SEEDS = {
    "r11_bw3_t8_a3c2": 2,                   # worst ratio 0.054 (seed 1 refused)
    "r11_bw3_t8_a16c7": 3,                  # worst ratio 0.064
    "r11_bw3_t8_a1c4_b128": 2,              # worst ratio 0.050
    "r12_bw3_t64_target_dq_a16c4": 7,       # worst ratio 0.039
    "r14_qb2_a3c1": 4,                      # worst ratio 0.043
    "r14_qb2_a16c4": 5,                     # worst ratio 0.050
    "r14_cols_b64_a2c7": 3,                 # worst ratio 0.054 (seed 2: 695)
    "r15_rows_b144_a3c4": 7,                # worst ratio 0.039
    "r15_rows_b144_a16c1": 4,               # worst ratio 0.042
    "r15_rows_b144_a5c7": 5,                # worst ratio 0.041 (seed 4: 424)
    "r16_w256_t4_b8_a16c10": 2,             # worst ratio 0.082
}

# 1b: acting, one case per model kind and A
ACT_CASES = {f"{kind}_a{A}": dict(A=A, C=C, over=over)
             for kind, C, over in (("iqn", 4, {}), ("full", 3, dict(FULL)), ("dqn1", 4, dict(DQN1, use_layer_norm=True)))
             for A in (1, 3, 16)}

# 1c: the fused step forms at parameter counts that are 1 and 3 mod 4: (baseline configuration, A, C, overrides,
#     n_params % 4, first Q-head offset % 4 or None), at B = 32 unless the case gives a `B`.  At 32 the backward is
#     iqn_bwd_kernel's 8 row chunks; the `_b64` / `_b128` cases run the default GEMM mode's iqn_bwd3_kernel, whose 16 gradient
#     slabs the post launch sums (and, with heads, qh_bwd2_kernel's two embedding-gradient slots): `expect` as in UPDATE_CASES
FUSED_CASES = {
    "iqn_a3": dict(base=2, A=3, C=4, over={}, rem=3, head_rem=None, expect=_x("fp32", 1)),
    "iqn_a5": dict(base=2, A=5, C=4, over={}, rem=1, head_rem=None, expect=_x("fp32", 1)),
    "full_a5": dict(base=3, A=5, C=4, over=dict(target_update_period=3), rem=3, head_rem=1, expect=_x("fp32", 0, "cols", merged_loss=1)),
    "dqn_a7": dict(base=0, A=7, C=4, over={}, rem=3, head_rem=0, expect=_x("none")),
    "iqn_rmsprop_a3": dict(base=2, A=3, C=4, over=dict(RMSPROP), rem=3, head_rem=None, expect=_x("fp32", 1)),
    "iqn_a3_b64": dict(base=2, A=3, C=4, over={}, rem=3, head_rem=None, B=64, expect=_x("bw3", 1, chunks=16)),
    "iqn_a5_b64": dict(base=2, A=5, C=4, over={}, rem=1, head_rem=None, B=64, expect=_x("bw3", 1, chunks=16)),
    "full_a5_b128": dict(base=3, A=5, C=4, over=dict(target_update_period=3), rem=3, head_rem=1, B=128,
                         expect=_x("bw3", 0, "qb2", chunks=16, q_de_slots=2, merged_loss=1)),
}


def expect_of(case, mode):
    """The plan fields a case expects in one of its modes."""
    e = case["expect"]
    return e[mode] if set(e) <= {"fp32", "bf16x3"} else e


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
