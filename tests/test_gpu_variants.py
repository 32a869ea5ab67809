"""GPU parity on shapes the golden reference runs do not cover: the HIP TD update vs the torch-CPU
oracle (itself pinned by tests/test_oracle_golden.py) on seeded random minibatches.

Each case exercises a different code path of the kernels: how many samples share a 16-row tile
(fused loss in tile_fwd for T = 4 / 16, stand-alone loss kernel when T' != T), how the conv backward
is produced (inside the backward kernel for C = 4, post-kernel role for C = 7), ragged row chunks.
Tolerances as in test_gpu_learner.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_learner import to_hip_batch

pytestmark = pytest.mark.gpu

CASES = {
    "tau4": dict(B=32, C=4, over=dict(iqn_n_current_state_quantile_samples=4, iqn_n_next_state_quantile_samples=4)),
    "tau16": dict(B=16, C=4, over=dict(iqn_n_current_state_quantile_samples=16, iqn_n_next_state_quantile_samples=16)),
    "tau8_next16": dict(B=16, C=4, over=dict(iqn_n_current_state_quantile_samples=8, iqn_n_next_state_quantile_samples=16)),
    "channels7": dict(B=32, C=7, over=dict()),
    "ragged48": dict(B=48, C=4, over=dict()),
    "tau16_target": dict(B=16, C=4, over=dict(iqn_n_current_state_quantile_samples=16,
                                              iqn_n_next_state_quantile_samples=16, use_target_network=True,
                                              use_double_q_learning=True)),
    # hidden width 256 (the ablation presets' width) away from their T = 32, B = 64: the bf16 forward tiles at H = 256 with
    # the loss inside the tile (T <= 8) or behind it, and every row-chunk count / sample-sum path of iqn_bwd4_kernel
    # (bwd4_kernels.h bw4_chunks: 8, 4; T = 4, 8, 16, 64)
    "w256_tau8": dict(B=64, C=4, over=dict(iqn_quantile_model_feature_dim=256)),
    "w256_tau4": dict(B=32, C=4, over=dict(iqn_quantile_model_feature_dim=256, iqn_n_current_state_quantile_samples=4,
                                           iqn_n_next_state_quantile_samples=4)),
    "w256_tau16_c7": dict(B=32, C=7, over=dict(iqn_quantile_model_feature_dim=256, iqn_n_current_state_quantile_samples=16,
                                               iqn_n_next_state_quantile_samples=16)),
    "w256_tau64_target": dict(B=16, C=4, over=dict(iqn_quantile_model_feature_dim=256, iqn_n_current_state_quantile_samples=64,
                                                   iqn_n_next_state_quantile_samples=64, use_target_network=True,
                                                   use_double_q_learning=True)),
    "w256_noln_ragged48": dict(B=48, C=4, over=dict(iqn_quantile_model_feature_dim=256, use_layer_norm=False)),
}


_config, _batch = H.variant_config, H.random_batch          # (shared with tests/test_gpu_envelope.py)


@pytest.mark.parametrize("name", sorted(CASES))
def test_variant_matches_oracle(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle.learner_ref import LearnerOracle
    from prism_amd.factory import agent_factory
    dev, A, seed = "cuda:0", 6, 11
    case = CASES[name]
    B, C = case["B"], case["C"]
    cfg = _config(dev, case["over"])
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A)
    cpu_cfg = _config("cpu", case["over"])
    sd, tgt = H.build_init_state(cpu_cfg, seed, C=C, A=A)
    for k, v in agent.model.state_dict().items():          # same seed, same construction order
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k].numpy(), err_msg=k)
    orc = LearnerOracle(sd, H.spec_from_config(cpu_cfg, C=C, A=A), tgt)
    # (seed chosen so that no trunk pre-activation sits within rounding distance of the ReLU kink:
    # there the HIP and the autograd gradients legitimately differ by a whole unit's contribution)
    rng = np.random.default_rng(1)
    wide = cfg.iqn_quantile_model_feature_dim >= 256
    for step in range(3):
        batch, w, taus = _batch(rng, B, C, A, cfg)
        pre_sd = orc.state_dict()
        pre_tgt = None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()}
        td_o = orc.update(batch, w, taus)
        td = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus])
        torch.cuda.synchronize()
        np.testing.assert_allclose(td.cpu().numpy(), td_o.numpy(), rtol=0, atol=1e-5)
        assert abs(float(agent._static_total_loss) - float(orc.last["total"])) < 1e-5
        off, gflat = 0, agent.grads.cpu()
        jitter, allowance = None, {}
        for k in sd:
            n = sd[k].numel()
            go = orc.last["grads"][k].reshape(-1)
            tol = 1e-4 * float(go.abs().max()) + 1e-7
            err = float((gflat[off:off + n] - go).abs().max())
            kink = 0.0
            if err > tol and wide:
                # width 256: a ReLU unit within rounding distance of zero -- bounded by what the oracle shows on itself
                # under a two-ulp parameter jitter (tests/test_gpu_learner.py)
                if jitter is None:
                    jitter = H.jitter_grads(pre_sd, pre_tgt, H.spec_from_config(cpu_cfg, C=C, A=A), batch, w, taus, seed=77 + step)
                kink = 2.0 * max(float((jg[k].reshape(-1) - go).abs().max()) for jg in jitter)
            allowance[k] = kink
            assert err <= tol + kink, f"{name} step {step} grad {k}: max err {err:.3e} > {tol:.3e} + {kink:.3e}"
            off += n
        post = agent.model.state_dict()
        for k, v in orc.state_dict().items():
            np.testing.assert_allclose(post[k].cpu().numpy(), v.numpy(), rtol=0,
                                       atol=2e-6 + cfg.learning_rate * allowance[k] / cfg.adam_epsilon, err_msg=k)
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()
            orc.sync_target()
