"""No GPU needed: the fixtures recorded away from the presets' scalars (tools/gen_golden.py, helpers.SCALAR_CASES and
dqn_rmsprop_scalars) are shown fit for their purpose by the oracle alone -- a kappa that nothing clips, a clip threshold
above the gradient norm, one gamma per batch or a vanishing Theil index would leave the code they are meant to reach
unexercised while every parity test still passed.  These are conditions on the inputs: where one fails, the case changes
(kappa, p_short, the batch seed), never the bound."""
import numpy as np
import pytest

from tests import helpers as H
from tests import scalar_cases as S


def _preset(g):
    from prism_amd import config as C
    return {"minatar": C.MINATAR_CONFIG, "additive": C.ADDITIVE_ABLATION_BASE_CONFIG,
            "subtractive": C.SUBTRACTIVE_ABLATION_BASE_CONFIG}[str(g["base"])]


def test_the_fixtures_leave_the_presets():
    """Every loss, clip and optimizer scalar leaves its preset value in at least one fixture, and kappa does on both sides
    of 1."""
    seen = {}
    for name in S.FIXTURES:
        g = H.load_case(name)
        for k, v in H.case_overrides(g).items():
            if isinstance(v, float) or k == "ids_allow_distributional_gradients":
                assert v != getattr(_preset(g), k), (name, k)
                seen.setdefault(k, set()).add(v)
        assert int(g["steps"]) == 2 and int(g["A"]) == 6 and int(g["C"]) == 4
    for k in ("iqn_huber_loss_kappa", "distributional_loss_weight", "q_loss_weight", "ids_ensemble_variation_coef",
              "ids_allow_distributional_gradients", "max_grad_norm", "learning_rate", "adam_beta1", "adam_beta2",
              "adam_epsilon", "rmsprop_alpha", "rmsprop_epsilon"):
        assert k in seen, k
    assert min(seen["iqn_huber_loss_kappa"]) < 1.0 < max(seen["iqn_huber_loss_kappa"])
    assert H.case_head_scale(H.load_case("full_scalars")) == (0.55, 0.1)


@pytest.mark.parametrize("name", S.FIXTURES)
def test_optimizer_sensitivity_stays_at_or_below_the_presets(name):
    """The parameter tolerance 2e-6 + lr * allowance / eps is written for the presets' lr / eps; a larger ratio turns the
    1e-7 floor of the gradient tolerance into parameter differences above 2e-6 in a correct kernel."""
    g = H.load_case(name)
    cfg, base = H.case_config(g), _preset(g)
    if cfg.use_adam:
        assert cfg.learning_rate / cfg.adam_epsilon <= base.learning_rate / base.adam_epsilon * (1 + 1e-12)
    elif cfg.use_rmsprop:
        assert cfg.learning_rate / cfg.rmsprop_epsilon <= base.learning_rate / base.rmsprop_epsilon * (1 + 1e-12)


@pytest.mark.parametrize("name", S.FIXTURES)
def test_inputs_reach_what_the_case_is_for(name):
    g = H.load_case(name)
    cfg, steps = S.oracle_run(name)
    assert len(steps) == int(g["steps"])
    for step, rec in enumerate(steps):
        print(f"{name} step {step}: quadratic share {rec['quad_share']}, gradient norm {rec['grad_norm']:.3f} "
              f"(max_grad_norm {cfg.max_grad_norm}), theil {rec['theil']}, gammas {rec['gammas']}, terminals {rec['terminals']}")
        if cfg.use_iqn:
            # both Huber branches carry weight: |delta| <= kappa on 10 % .. 90 % of the (sample, j, t) pairs
            assert 0.10 <= rec["quad_share"] <= 0.90, (step, rec["quad_share"])
        if cfg.max_grad_norm < _preset(g).max_grad_norm:
            assert rec["grad_norm"] > cfg.max_grad_norm, (step, rec["grad_norm"])      # clip coefficient < 1
        assert len(rec["gammas"]) >= 3 and rec["terminals"] >= 2, (step, rec["gammas"], rec["terminals"])
        if name == "full_scalars":
            assert rec["theil"] > 1e-2, (step, rec["theil"])


@pytest.mark.parametrize("name", S.FIXTURES)
def test_inputs_are_kink_free_by_the_oracle_alone(name):
    """A ReLU unit within rounding distance of zero makes two correct evaluations of one gradient differ by the unit's whole
    contribution.  The batch seeds of these fixtures are chosen so that the oracle's own gradient does not
    move by more than half a tolerance between fp32 and fp64 or under a two-ulp parameter jitter: what the kernels are held
    to at these scalars is then the tolerance itself, not an allowance."""
    worst = S.worst_kink(name)
    print(f"{name}: worst (gap or move) / tolerance {worst:.3f}")
    assert worst <= 0.5


def test_theil_differential_stands_clear_of_rounding():
    """tests/test_gpu_scalars.py compares g_dev(c) - g_dev(0) with the oracle's; at c = THEIL_C the oracle's difference is
    >= 20 rounding terms on every head tensor that is not zero itself (the term is a multiple of the tensor: the LayerNorm
    biases, zero at initialisation, receive none), and exactly zero everywhere else."""
    ref = S.theil_reference()
    heads = [k for k in ref["names"] if k.startswith(S.HEAD_PREFIX) and k not in ref["zero"]]
    assert len(heads) == 60 and len([k for k in ref["zero"] if k.startswith(S.HEAD_PREFIX)]) == 20
    worst = min(float(ref["delta"][k].abs().max()) / S.theil_rounding_term(ref, k) for k in heads)
    print(f"c = {S.THEIL_C}: theil {ref['theil']:.4f}, smallest max|delta_ref| / rounding term over the head tensors {worst:.1f}")
    assert worst >= 20.0
    for k in ref["names"]:
        if k not in heads:
            assert float(ref["delta"][k].abs().max()) == 0.0, k
    assert ref["theil"] > 1e-2
    # the total loss moves by -q_w * c * theil * mean(w) (fp32 totals: the project's 1e-5 on each)
    move = -ref["q_w"] * S.THEIL_C * ref["theil"] * ref["w_mean"]
    assert abs((ref["total_c"] - ref["total_0"]) - move) < 2e-5


def test_ids_select_rows_are_rarely_ambiguous():
    """tests/test_gpu_acting.py skips the action comparison on rows whose two smallest oracle scores lie within the score
    tolerance of each other: at most 5 % of the rows of any scalar triple."""
    from oracle.learner_ref import ids_scores
    for lam, eps, rho in S.IDS_SELECT_SCALARS:
        rows = skipped = 0
        for n, T, A, heads, dist, q in S.ids_select_estimates():
            if T == 1 or heads == 1:
                continue
            amb = S.ids_ambiguous_rows(ids_scores(dist, q, lam, eps, rho)["scores"].numpy())
            rows, skipped = rows + n, skipped + int(amb.sum())
        print(f"(lambda, epsilon, rho_min) = {(lam, eps, rho)}: {skipped} of {rows} rows ambiguous")
        assert skipped <= 0.05 * rows
