"""GPU: the Theil-index gradient of the Q ensemble in isolation.

In the update fixtures the data gradient dominates max|g| of every head tensor, so the project's gradient rule
(1e-4 * max|g| + 1e-7) would let a wrong Theil term through on most of them even at ids_ensemble_variation_coef = 0.5 with
heads of unequal norm (it exceeds 10 tolerances on 7 of 80 head tensors).  Here the term is taken apart from the rest: one
update on the full_scalars inputs at coefficient c and one at 0, fresh agents from the same seed and head scaling, and

    delta_dev = g_dev(c) - g_dev(0)      against      delta_ref = the oracle's float64 gradients' difference,

per tensor within (1e-4 * max|delta_ref| + 1e-7) + 4 * 2**-23 * max|g_ref|: the project's gradient rule applied to the
difference, plus the fp32 roundings of forming g + kappa_h * theta twice and subtracting.  Tensors outside the heads, and
the heads' LayerNorm biases (zero at initialisation: the term is a multiple of the tensor), are held to the rounding
term alone.  c = scalar_cases.THEIL_C; tests/test_scalar_case_inputs.py shows on the CPU that max|delta_ref| is then at
least 20 rounding terms on every other head tensor, so a wrong sign, a wrong c_h or a missing mean(w) fails here."""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import scalar_cases as S
from tests.test_gpu_learner import LOSS_TOL, build_hip_agent, to_hip_batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _one_update(dev, gemm_mode, coef, ref):
    g = H.load_case(S.THEIL_CASE)
    cfg, agent = build_hip_agent(g, dev, gemm_mode=gemm_mode, ids_ensemble_variation_coef=coef)
    agent.update(to_hip_batch(ref["batch"], dev), per_weights=ref["w"].to(dev), taus=[t.to(dev) for t in ref["taus"]])
    torch.cuda.synchronize()
    return agent.grads.cpu().double(), float(agent.scalars[4]), float(agent._static_total_loss)


@pytest.mark.parametrize("gemm_mode", ["fp32", "bf16x3"])
def test_theil_gradient_matches_the_oracle(dev, gemm_mode):
    ref = S.theil_reference()
    g_c, theil_c, total_c = _one_update(dev, gemm_mode, S.THEIL_C, ref)
    g_0, theil_0, total_0 = _one_update(dev, gemm_mode, 0.0, ref)
    # the index itself, and what it does to the loss: total moves by -q_w * c * theil * mean(w)
    assert abs(theil_c - ref["theil"]) < 1e-6
    # (formed from the device's own index, held to the oracle's just above: at c = 64 the index's 1e-6 is 6e-5 of loss; each
    # total carries the project's 1e-5)
    move = -ref["q_w"] * S.THEIL_C * theil_c * ref["w_mean"]
    print(f"{gemm_mode}: theil {theil_c:.7f} (oracle {ref['theil']:.7f}), total {total_0:.6f} -> {total_c:.6f}, "
          f"move {total_c - total_0:.6f} (expected {move:.6f})")
    assert abs(total_0 - ref["total_0"]) < LOSS_TOL
    assert abs((total_c - total_0) - move) < 2 * LOSS_TOL
    off, worst_head, worst_rest = 0, 0.0, 0.0
    for k in ref["names"]:
        d_ref = ref["delta"][k].reshape(-1)
        n = d_ref.numel()
        d_dev = g_c[off:off + n] - g_0[off:off + n]
        off += n
        rounding = S.theil_rounding_term(ref, k)
        err = float((d_dev - d_ref).abs().max())
        if k.startswith(S.HEAD_PREFIX) and k not in ref["zero"]:
            tol = 1e-4 * float(d_ref.abs().max()) + 1e-7 + rounding
            worst_head = max(worst_head, err / tol)
        else:
            assert float(d_ref.abs().max()) == 0.0
            tol = rounding
            worst_rest = max(worst_rest, err / tol if tol else float(err > 0))
        assert err <= tol, f"{k}: |delta_dev - delta_ref| {err:.3e} > {tol:.3e} (max|delta_ref| {float(d_ref.abs().max()):.3e})"
    assert off <= g_c.numel()
    print(f"{gemm_mode}: worst error / tolerance, head tensors {worst_head:.3f}, the rest {worst_rest:.3f}")
