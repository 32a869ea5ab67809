"""GPU: the path bench.py times -- Learner.step() fused, replayed from the hipGraph -- held to the oracle AT THE SIZES THE
BENCH USES (B = 256 / 512, replay 100 000 -> 17 tree levels, and the 1.25 M-slot shard of configs[4] -> 21 levels).

At steps 1 (eager: the first full-buffer step), 10 and 100 (graph replays) of a run the test snapshots parameters, Adam
state and both priority trees before the step, lets the device run it, then replays that ONE step on the CPU:
  * masses are re-drawn on the host from the same Philox counters -> ReplayOracle.sample: indices and IS weights bit-exact;
  * n-step walk + collate of those slots through the oracle: every static-batch tensor bit-exact;
  * LearnerOracle.update on the device's minibatch and recorded quantile samples: td <= 1e-5, parameters after Adam <= 2e-6;
  * oracle update_priority(index, |td of the device|): EVERY node of both trees bit-exact (duplicates included), and the
    running maximum priority.
Reference: /root/reference/prism/learner.py:95-125 (one loop body)."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

CHECK_STEPS = (1, 10, 100)


def _learner(dev, base, B, cap, **over):
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from prism_amd.synthetic import fill_replay
    cfg = baseline_config(base, device=dev, batch_size=B, experience_replay_capacity=cap, **over)
    cfg.fused_step, cfg.hip_graph = True, True
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6)
    fill_replay(ln.experience_buffer, cap, seed=5)
    return ln, cfg


def _check_step(ln, cfg, orc_ring, step):
    from oracle.learner_ref import LearnerOracle
    buf, agent = ln.experience_buffer, ln.agent
    B = cfg.batch_size
    torch.cuda.synchronize()
    # ---- snapshot before the step
    sd0 = {k: v.detach().cpu().clone() for k, v in agent.model.state_dict().items()}
    tg0 = None if agent.target_model is None else {k: v.detach().cpu().clone() for k, v in agent.target_model.state_dict().items()}
    opt0 = agent.optimizer.state_dict()
    snap = H.replay_snapshot(buf, agent)
    td = ln.step(timesteps_this_iteration=1).clone()
    torch.cuda.synchronize()
    buf.check_status()
    if step > 2:
        assert any(isinstance(g, tuple) for g in agent._graphs.values()), "the step did not run from a hipGraph"

    # ---- sampling, n-step walk + collate (tests/helpers.py: the replay half, shared with tests/test_gpu_replay_geometry.py)
    idx, w_o, g = H.check_replay_front(buf, orc_ring, snap, B, step)
    # ---- the TD update on that minibatch
    batch = dict(obs=torch.from_numpy(g["obs"]).view(B, 10, 10, 4), next_obs=torch.from_numpy(g["next_obs"]).view(B, 10, 10, 4),
                 reward=torch.from_numpy(g["reward"]), nonterminal=torch.from_numpy(g["nonterminal"].astype(bool)),
                 gamma=torch.from_numpy(g["gamma"]), action=torch.from_numpy(g["action"]))
    taus = []
    if cfg.use_iqn:
        T, Tn = cfg.iqn_n_current_state_quantile_samples, cfg.iqn_n_next_state_quantile_samples
        taus.append(agent.tau_out[0, :T * B].cpu().reshape(-1, 1))
        if not cfg.use_target_network or cfg.use_double_q_learning:
            taus.append(agent.tau_out[1, :Tn * B].cpu().reshape(-1, 1))
        if cfg.use_target_network:
            taus.append(agent.tau_out[2, :Tn * B].cpu().reshape(-1, 1))
    orc = LearnerOracle(sd0, H.spec_from_config(cfg), tg0)
    orc.opt.load_state_dict(opt0)
    td_o = orc.update(batch, torch.from_numpy(w_o), taus)
    td_d = td.cpu()
    err = float((td_d - td_o).abs().max())
    assert err <= 1e-5, f"step {step}: td error {err}"
    # Parameters after Adam: 2e-6, plus lr / adam_eps times the ill-conditioning of the tensor's gradient.  At these sizes
    # (655 360 ReLU units in the ten Q heads of configs[3] per step, pre-activations ~ N(0, 1)) about one unit per step
    # sits within fp32 rounding distance of zero; two correct evaluations may put it on different sides, which moves a whole
    # row of that layer's weight gradient by the unit's contribution (here 3e-6), and d update / d g reaches lr / eps = 1.7
    # where |g| is small against Adam's epsilon.  The oracle measures it on itself: the same gradient in float64, and in
    # fp32 at parameters jittered by about two ulps (six draws) -- where those agree with the plain fp32 gradient the
    # tensor is well-conditioned and the bare 2e-6 applies (as in tests/test_gpu_learner.py).
    spec = H.spec_from_config(cfg)
    g32 = orc.last["grads"]
    probe = LearnerOracle(sd0, spec, tg0)
    g64 = probe.grads_fp64(batch, torch.from_numpy(w_o), taus)
    kink = {k: float((g32[k].double() - g64[k]).abs().max()) for k in g32}
    gen = torch.Generator().manual_seed(1234 + step)
    # (six draws at two units in the last place: the device's GEMMs differ from the oracle's by the summation order of a
    # K = 1024 product -- rms 1.3, at most 7 units in the last place of a pre-activation, profiles/r03_split_bf16_ubench.txt --
    # and the order changes with the launch form: eight or four K slices per tile, fwd_kernels.h.  Three draws at one unit
    # missed a unit the four-slice form flipped: 2.3e-6 on one row of one head's weight at step 10 of the configs[4] shard)
    for _ in range(6):
        jit = {k: v * (1.0 + 2.4e-7 * torch.randn(v.shape, generator=gen)) for k, v in sd0.items()}
        pj = LearnerOracle(jit, spec, tg0)
        pj.update(batch, torch.from_numpy(w_o), taus, apply=False)
        for k in g32:
            kink[k] = max(kink[k], float((pj.last["grads"][k] - g32[k]).abs().max()))
    post = agent.model.state_dict()
    perr, needed = 0.0, []
    for k, v in orc.state_dict().items():
        d = float((post[k].cpu() - v).abs().max())
        tol = 2e-6 + (cfg.learning_rate / cfg.adam_epsilon) * 2.0 * kink[k]
        assert d <= tol, f"step {step}: parameter error after Adam {d} in {k} (tolerance {tol}, gradient ill-conditioning {kink[k]})"
        if d > 2e-6:
            needed.append(k)
        perr = max(perr, d)
    assert len(needed) <= 4, f"step {step}: {needed} needed the ill-conditioning allowance"
    # ---- priority writeback with the device's own |td|: every node of both trees, duplicates included
    H.check_replay_writeback(buf, orc_ring.sampler, idx, td_d.abs().numpy(), step)
    return err, perr, B - len(np.unique(idx))


# (configs[0], [1], [2], [3] of BASELINE.json at full size; configs[3] again without the fused tail -- the launch form a
#  data-parallel step uses; the 1.25 M-slot shard of configs[4]: 21 tree levels)
CASES = {
    "c1_dqn_uniform": dict(base=0, B=32, cap=100_000),
    "c2_dqn_per": dict(base=1, B=256, cap=100_000),
    "c3_iqn_per": dict(base=2, B=256, cap=100_000),
    "c4_full": dict(base=3, B=512, cap=100_000, target_update_period=40),
    "c4_full_split_tail": dict(base=3, B=512, cap=100_000, target_update_period=40, fuse_tail=False),
    "c3_split_tail": dict(base=2, B=256, cap=100_000, fuse_tail=False),
    "c5_shard_1p25M": dict(base=4, B=512, cap=1_250_000, target_update_period=40),
    # the exact fp32 MFMA chain in the forward GEMMs (the default is the three-piece bf16 form, prism_hip.h gemm_mode)
    "c3_iqn_per_fp32": dict(base=2, B=256, cap=100_000, gemm_mode="fp32"),
    "c4_full_fp32": dict(base=3, B=512, cap=100_000, target_update_period=40, gemm_mode="fp32"),
    # the ablation presets' shape (width 256, T = 32, batch 64) through the fused graph step with PER + 3-step returns: the bf16
    # forward tiles at H = 256 and iqn_bwd4_kernel, 100 steps against the oracle; and the full model at that width
    "w256_t32_iqn_per": dict(base=2, B=64, cap=100_000, iqn_quantile_model_feature_dim=256,
                             iqn_n_current_state_quantile_samples=32, iqn_n_next_state_quantile_samples=32),
    "w256_t32_full": dict(base=3, B=64, cap=100_000, target_update_period=40, iqn_quantile_model_feature_dim=256,
                          ids_q_head_feature_dim=256, iqn_n_current_state_quantile_samples=32,
                          iqn_n_next_state_quantile_samples=32),
}


@pytest.mark.parametrize("name", list(CASES))
def test_graph_step_matches_oracle_at_bench_sizes(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    kw = dict(CASES[name])
    base, B, cap = kw.pop("base"), kw.pop("B"), kw.pop("cap")
    ln, cfg = _learner("cuda:0", base, B, cap, **kw)
    buf = ln.experience_buffer
    levels = int(np.log2(buf.tree_capacity))
    assert levels == (21 if cap > 1_000_000 else 17)
    ring = H.oracle_ring(buf, cfg)
    worst = [0.0, 0.0, 0]
    for step in range(1, max(CHECK_STEPS) + 1):
        if step in CHECK_STEPS:
            e, p, dup = _check_step(ln, cfg, ring, step)
            worst = [max(worst[0], e), max(worst[1], p), worst[2] + dup]
        else:
            ln.step(timesteps_this_iteration=1)
    torch.cuda.synchronize()
    assert int(ln.agent.optimizer.step_t.item()) == max(CHECK_STEPS)
    print(f"{name}: td err {worst[0]:.2e}, param err {worst[1]:.2e}, duplicate slots seen {worst[2]}")
