"""GPU parity across the envelope prism_learner_supported accepts: action counts 1..16, observation channels 1..10, batch
sizes at the edges of the divisibility rules and at 4096 (tests/envelope_cases.py holds the case table; the rest of the
suite runs A = 6, C >= 4 and batches that are multiples of 16).

The action count is not a passive dimension: the forward tiles stage W2[A][H] with clamped indices, every tail / loss /
selector kernel masks lanes with `lane < A`, and the unpadded flat parameter buffer makes A decide n_params % 4 (the
scalar tails of the optimizer kernels and of the all-reduce slices) and the alignment of every Q-head tensor.

  a. the unfused update against LearnerOracle, both GEMM modes, tolerances of tests/test_gpu_variants.py; rows 11-16 of the
     case table run every backward form the plan can pick (iqn_bwd3_kernel with and without the conv backward inside,
     qh_bwd2_kernel, qh_bwd_kernel by rows, iqn_bwd4_kernel with 1 and 2 row chunks) in the mode that selects it;
  b. acting (prism_act_forward, prism_ids_select, prism_greedy_select, the hipGraph form) over the same grid, with exact ties;
  c. the fused step forms bit-equal to the unfused one at n_params % 4 in {1, 3};
  d. the direct all-reduce at lengths 8k + 1 and 8k + 3.
The inputs of (a) are shown kink-free by the oracle alone in tests/test_envelope_inputs.py."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import envelope_cases as E
from tests import helpers as H
from tests.test_gpu_learner import to_hip_batch

pytestmark = pytest.mark.gpu
TD_TOL, LOSS_TOL, PARAM_TOL = 1e-5, 1e-5, 2e-6
MAX_ALLOWANCES = 4          # (tensor, step) pairs of a width-256 case that may take the kink allowance (test_gpu_fullsize_parity.py)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _build_agent(cfg, C, A, seed=E.INIT_SEED):
    from prism_amd.factory import agent_factory
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return agent_factory.build_agent(cfg, (10, 10, C), A)


# ------------------------------------------------------------------------------------------------------ a. update parity
@pytest.mark.parametrize("name,gemm_mode", [(n, m) for n, c in E.UPDATE_CASES.items() for m in c["modes"]])
def test_update_matches_oracle(dev, name, gemm_mode):
    case = E.UPDATE_CASES[name]
    A, C = case["A"], case["C"]
    cpu_cfg, spec, sd, steps = E.oracle_run(name)
    cfg = E.case_config(name, device=dev, gemm_mode=gemm_mode)
    agent = _build_agent(cfg, C, A)
    for k, v in agent.model.state_dict().items():          # same seed, same construction order
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k].numpy(), err_msg=k)
    wide = max(cfg.iqn_quantile_model_feature_dim if cfg.use_iqn else 0, cfg.ids_q_head_feature_dim if cfg.use_ids else 0) >= 256
    if cfg.use_adam:
        sens = cfg.learning_rate / cfg.adam_epsilon
    else:
        sens = cfg.learning_rate / cfg.rmsprop_epsilon if cfg.use_rmsprop else cfg.learning_rate
    taken = 0
    for step, rec in enumerate(steps):
        td = agent.update(to_hip_batch(rec["batch"], dev), per_weights=rec["w"].to(dev), taus=[t.to(dev) for t in rec["taus"]])
        torch.cuda.synchronize()
        np.testing.assert_allclose(td.cpu().numpy(), rec["td"].numpy(), rtol=0, atol=TD_TOL)
        assert abs(float(agent._static_total_loss) - rec["total"]) < LOSS_TOL
        off, gflat, allowance = 0, agent.grads.cpu(), {}
        for k in sd:
            n = sd[k].numel()
            go = rec["grads"][k].reshape(-1)
            tol = E.grad_tolerance(go)
            err = float((gflat[off:off + n] - go).abs().max())
            kink = 0.0
            if err > tol and wide:
                # width 256 only: a ReLU unit within rounding distance of zero, bounded by what the oracle shows on itself
                # under a two-ulp parameter jitter; width 128 gets no allowance at all
                kink = 2.0 * max(float((jg[k].reshape(-1) - go).abs().max()) for jg in E.jitter_of(rec, spec, step))
                taken += 1
            allowance[k] = kink
            assert err <= tol + kink, f"{name} {gemm_mode} step {step} grad {k}: max err {err:.3e} > {tol:.3e} + {kink:.3e}"
            off += n
        assert off == agent.flat.numel()
        if case["check_params"]:
            post = agent.model.state_dict()
            for k, v in rec["post"].items():
                np.testing.assert_allclose(post[k].cpu().numpy(), v.numpy(), rtol=0, atol=PARAM_TOL + sens * allowance[k],
                                           err_msg=f"{name} {gemm_mode} step {step} {k}")
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()
    assert int(agent.optimizer.step_t.item()) == case["steps"]
    assert taken <= (MAX_ALLOWANCES if wide else 0), f"{taken} (tensor, step) pairs took the kink allowance"


# ------------------------------------------------------------------------------------------------------ b. acting
def _acting_agent(name, dev):
    """An agent of ACT_CASES[name] on perturbed weights (LayerNorm gains away from 1, biases away from 0) and the same
    weights on the CPU."""
    case = E.ACT_CASES[name]
    A, C = case["A"], case["C"]
    cfg = H.variant_config(dev, case["over"])
    agent = _build_agent(cfg, C, A)
    gen = torch.Generator().manual_seed(5)
    sd = {k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen) for k, v in agent.model.state_dict().items()}
    agent.model.load_state_dict(sd)
    agent._params_replaced()
    return cfg, agent, sd, H.spec_from_config(H.variant_config("cpu", case["over"]), C=C, A=A)


def _select(agent, cfg, kind):
    """The selector kernel on the buffers the last act_estimates call left: (actions, scores or None), on the CPU."""
    from prism_amd import _native as N
    z, qb, n, n_pad, T = agent._act_raw
    A, dev = agent.dims.n_actions, agent.device
    action = torch.full((n,), -1, dtype=torch.int64, device=dev)
    scores = None
    if kind == "ids":
        scores = torch.empty((n, A), device=dev)
        N.check(N.lib().prism_ids_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, cfg.ids_n_q_heads, cfg.ids_lambda, cfg.ids_epsilon,
                                         cfg.ids_rho_lower_bound, 0, N.ptr(scores), None, N.ptr(action), None,
                                         N.current_stream_handle()), "prism_ids_select")
    else:
        N.check(N.lib().prism_greedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, agent.dims.n_heads, N.ptr(action), None, None,
                                            N.current_stream_handle()), "prism_greedy_select")
    torch.cuda.synchronize()
    return action.cpu(), None if scores is None else scores.cpu()


@pytest.mark.parametrize("name", list(E.ACT_CASES))
def test_acting_matches_oracle(dev, name):
    """prism_act_forward against act_forward for one observation, a count that is no multiple of a 16-row tile and more
    than the workspace holds at once; then the selector kernels on the device's own estimates against the reference
    selectors' arithmetic on the CPU (ids_scores / mean + argmax)."""
    from oracle.learner_ref import act_forward, ids_scores
    cfg, agent, sd, spec = _acting_agent(name, dev)
    A, C = agent.dims.n_actions, agent.dims.in_channels
    B = int(cfg.batch_size)
    T = cfg.iqn_quantile_samples_per_action if cfg.use_iqn else 0
    rng = np.random.default_rng(7)
    for n in (1, 17, B + 7):
        obs = torch.from_numpy((rng.random((n, 10, 10, C)) < 0.15).astype(np.float32))
        taus = torch.from_numpy(rng.random((T * n, 1)).astype(np.float32)) if cfg.use_iqn else None
        q, dist = agent.act_estimates(obs.to(dev), taus=None if taus is None else taus.to(dev))
        torch.cuda.synchronize()
        qo, do = act_forward(sd, spec, obs, taus)
        assert tuple(q.shape) == tuple(qo.shape)
        np.testing.assert_allclose(q.cpu().numpy(), qo.numpy(), rtol=0, atol=1e-5, err_msg=f"q, n = {n}")
        if cfg.use_iqn:
            assert tuple(dist.shape) == tuple(do.shape) == (T, n, A)
            np.testing.assert_allclose(dist.cpu().numpy(), do.numpy(), rtol=0, atol=1e-5, err_msg=f"dist, n = {n}")
        else:
            assert dist is None
        if n > B:
            continue          # served in pieces: no estimate buffers are left for the selector kernels (_act_raw is None)
        qc, dc = q.cpu(), None if dist is None else dist.cpu()
        act, _ = _select(agent, cfg, "greedy")
        np.testing.assert_array_equal(act.numpy(), torch.argmax(qc.mean(dim=-1), dim=-1).numpy())
        if cfg.use_ids:
            act, scores = _select(agent, cfg, "ids")
            r = ids_scores(dc, qc, cfg.ids_lambda, cfg.ids_epsilon, cfg.ids_rho_lower_bound)
            np.testing.assert_allclose(scores.numpy(), r["scores"].numpy(), rtol=2e-4, atol=1e-7)
            np.testing.assert_array_equal(act.numpy(), r["action"].numpy())


def _tie_rows(A):
    """Mean action values [rows][A] with exact ties: all equal; two equal maxima at the first and the last action; and,
    so that a kernel answering 0 everywhere fails, a single maximum at the last action and one in the middle."""
    rows = [np.full(A, 1.5), np.full(A, -0.25)]
    r = np.linspace(-1.0, 0.5, A).round(3)
    r[0] = r[-1] = 2.0
    rows.append(r)
    r = -np.arange(A, dtype=np.float64) * 0.125
    r[-1] = 3.0
    rows.append(r)
    r = np.zeros(A)
    r[A // 2] = 0.75
    rows.append(r)
    return np.stack(rows).astype(np.float32)


@pytest.mark.parametrize("A", [2, 7, 16])
def test_selectors_break_exact_ties_like_the_reference(dev, A):
    """Hand-built estimates with exact ties.  Greedy: what torch.argmax of the reference selector's means returns, through
    both estimate arrays (ensemble heads, quantile samples).  IDS: what the arg-min of ids_scores returns; the tied actions
    carry heads that agree exactly (zero spread) at the largest upper bound, so that their regret and with it their score
    is exactly zero in any correct evaluation, while every other action scores above zero."""
    from oracle.learner_ref import ids_scores
    from prism_amd import _native as N
    m = torch.from_numpy(_tie_rows(A))                           # [n][A]
    n, heads, T = m.shape[0], 4, 8
    n_pad = 16
    L = N.lib()

    def greedy(z, qb):
        act = torch.full((n,), -1, dtype=torch.int64, device=dev)
        N.check(L.prism_greedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, heads, N.ptr(act), None, None,
                                      N.current_stream_handle()), "prism_greedy_select")
        torch.cuda.synchronize()
        return act.cpu().numpy()

    # ensemble heads: head h = mean + d_h with offsets that cancel exactly (dyadic values: every sum is exact)
    d = torch.tensor([0.5, -0.5, 0.25, -0.25])
    q = m[:, :, None] + d[None, None, :]                         # [n][A][heads], the reference's layout
    qb = torch.zeros((heads, n_pad, A))
    qb[:, :n] = q.permute(2, 0, 1)
    want = torch.argmax(q.mean(dim=-1), dim=-1).numpy()
    assert want[2] == 0 and want[3] == A - 1                     # (first of two equal maxima; a single one at the end)
    np.testing.assert_array_equal(greedy(None, qb.to(dev)), want)
    # quantile samples only (models without Q heads: q_estimates = return_distribution.mean(dim=0))
    dt = torch.tensor([1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 0.25, -0.25])
    dist = m[None, :, :] + dt[:, None, None]                     # [T][n][A]
    z = torch.zeros((n_pad * T, A))
    z[:n * T] = dist.permute(1, 0, 2).reshape(n * T, A)
    want = torch.argmax(dist.mean(dim=0).unsqueeze(-1).mean(dim=-1), dim=-1).numpy()
    np.testing.assert_array_equal(greedy(z.to(dev), None), want)

    # IDS: rows of (tied actions, value)
    rng = np.random.default_rng(A)
    rows = [(list(range(A)), 1.0), ([0, A - 1], 2.0), ([A - 1], 2.0), ([A // 2, A - 1], 0.5)]
    nr = len(rows)
    q = torch.zeros((nr, A, heads))
    for i, (tied, val) in enumerate(rows):
        q[i] = val - 1.0 - torch.from_numpy(rng.random((A, 1)).astype(np.float32)) + 0.1 * d[None, :]      # below val by >= 0.5
        q[i, tied, :] = val
    dist = torch.from_numpy(rng.standard_normal((T, nr, A)).astype(np.float32))
    for i, (tied, _) in enumerate(rows):
        dist[:, i, tied] = dist[:, i, tied[:1]]                  # the tied actions share one return distribution
    r = ids_scores(dist, q, 0.1, 1e-10, 0.25)
    for i, (tied, _) in enumerate(rows):
        assert float(r["scores"][i, tied].abs().max()) == 0.0 and int(r["action"][i]) == tied[0]
        assert all(float(r["scores"][i, a]) > 0 for a in range(A) if a not in tied)
    qb = torch.zeros((heads, n_pad, A))
    qb[:, :nr] = q.permute(2, 0, 1)
    z = torch.zeros((n_pad * T, A))
    z[:nr * T] = dist.permute(1, 0, 2).reshape(nr * T, A)
    scores = torch.empty((nr, A), device=dev)
    act = torch.full((nr,), -1, dtype=torch.int64, device=dev)
    z_d, qb_d = z.to(dev), qb.to(dev)
    N.check(L.prism_ids_select(N.ptr(z_d), N.ptr(qb_d), nr, n_pad, T, A, heads, 0.1, 1e-10, 0.25, 0, N.ptr(scores),
                               None, N.ptr(act), None, N.current_stream_handle()), "prism_ids_select")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(act.cpu().numpy(), r["action"].numpy())
    np.testing.assert_allclose(scores.cpu().numpy(), r["scores"].numpy(), rtol=2e-4, atol=1e-7)


@pytest.mark.parametrize("name", ["iqn_a3", "iqn_a16", "full_a3", "full_a16", "dqn1_a3", "dqn1_a16"])
def test_forward_from_the_hipgraph_equals_the_eager_launches(dev, name):
    """Agent.forward replayed from its hipGraph against the eager launches on the same counters (the pattern of
    tests/test_gpu_acting.py), from host arrays and from one persistent device buffer."""
    cfg, agent, sd, spec = _acting_agent(name, dev)
    A, C = agent.dims.n_actions, agent.dims.in_channels
    rng = np.random.default_rng(3)
    n = 5
    assert agent.act_graph
    frames = [(rng.random((n, 10, 10, C)) < 0.15).astype(np.float32) for _ in range(6)]
    agent.act_graph = False
    agent._act_draws = 777
    want = [agent.forward(f).cpu().numpy().copy() for f in frames]
    end_draws = agent._act_draws
    assert all(w.min() >= 0 and w.max() < A for w in want)
    agent.act_graph = True
    agent._act_draws = 777
    for i, f in enumerate(frames):
        a = agent.forward(f)
        assert type(a).__name__ == "_Actions"
        np.testing.assert_array_equal(a.cpu().numpy(), want[i])
        np.testing.assert_array_equal(torch.Tensor.cpu(a.as_subclass(torch.Tensor)).numpy(), want[i])
    assert agent._act_draws == end_draws and int(agent.rng_counters[2].item()) == end_draws
    buf = torch.zeros((n, 10, 10, C), device=dev)
    agent._act_draws = 777
    for i, f in enumerate(frames):
        buf.copy_(torch.from_numpy(f))
        np.testing.assert_array_equal(agent.forward(buf).cpu().numpy(), want[i])
    assert any(st["g"] is not None for st in agent._act_graphs.values()), "no call was replayed from a graph"


# ------------------------------------------------------------------------------------------------------ c. fused forms
def _mk(dev, case, fused, graph, fuse_tail=True, B=32, cap=2048):
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from prism_amd.synthetic import fill_replay
    cfg = baseline_config(case["base"], device=dev, batch_size=B, experience_replay_capacity=cap, **case["over"])
    cfg.fused_step, cfg.hip_graph, cfg.fuse_tail = fused, graph, fuse_tail
    shape = (10, 10, case["C"])
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=shape, n_actions=case["A"])
    fill_replay(ln.experience_buffer, cap, obs_shape=shape, n_actions=case["A"], seed=3)
    return ln


@pytest.mark.parametrize("name", list(E.FUSED_CASES))
def test_fused_forms_equal_unfused_at_odd_parameter_counts(dev, name):
    """The pattern of tests/test_gpu_step.py::test_fused_and_graph_equal_unfused at parameter counts that leave a scalar
    tail of 1 and of 3 floats behind the float4 part of every flat-buffer kernel, and Q-head tensors at an odd float offset:
    unfused, fused eager, hipGraph and the five-launch form stay bit-identical for 6 steps.  With (a) holding the unfused
    form to the oracle, bit-equality carries parity to the others.  Cases with a `B` of 64 or 128 run the post launch's sum
    over iqn_bwd3_kernel's 16 gradient slabs (8 at B = 32) and over qh_bwd2_kernel's two embedding-gradient slots."""
    case = E.FUSED_CASES[name]
    B = case.get("B", 32)
    ref, fus, gra = _mk(dev, case, False, False, B=B), _mk(dev, case, True, False, B=B), _mk(dev, case, True, True, B=B)
    spl = _mk(dev, case, True, True, fuse_tail=False, B=B)
    from prism_amd import _native as N
    plan = N.plan_info(ref.agent.dims, B, str(getattr(ref.agent.config, "gemm_mode", "auto")))
    assert {k: plan[k] for k in case["expect"]} == case["expect"]          # (the launch forms the case is here for)
    n_params, table = E.layout(ref.agent.model.state_dict())
    assert n_params == ref.agent.flat.numel() and n_params % 4 == case["rem"] and case["rem"] in (1, 3)
    head = E.first_head_offset(table)
    assert (None if head is None else head % 4) == case["head_rem"]
    assert ref.agent.dims.n_actions == case["A"]
    for step in range(6):
        outs = []
        for ln in (ref, fus, gra, spl):
            td = ln.step(timesteps_this_iteration=1).clone()
            torch.cuda.synchronize()
            buf, ag = ln.experience_buffer, ln.agent
            tree = buf.sum_tree.cpu().numpy() if buf.use_per else np.zeros(1)
            outs.append((td.cpu().numpy(), buf._index.cpu().numpy(), buf._weight.cpu().numpy(), ag.flat.cpu().numpy(), tree,
                         float(ag.scalars[0])) + tuple(b.cpu().numpy() for b in ag.optimizer.buffers()))
        for i, other in enumerate(outs[1:]):
            for j, (x, y) in enumerate(zip(outs[0], other)):
                np.testing.assert_array_equal(x, y, err_msg=f"step {step}, form {i + 1}, item {j}")
        assert np.isfinite(outs[0][3]).all() and int(outs[0][0].shape[0]) == B
    for ln in (ref, fus, gra, spl):
        assert int(ln.agent.optimizer.step_t.item()) == 6
        ln.agent.check_status()
    assert any(isinstance(g, tuple) for g in gra.agent._graphs.values())      # a graph really was captured
    assert int(ref.experience_buffer.action.max().item()) == case["A"] - 1   # the replay really holds every action


# ------------------------------------------------------------------------------------------------------ d. direct all-reduce
@pytest.mark.timeout(600)
def test_direct_allreduce_at_lengths_not_divisible_by_four_times_world(dev):
    """tests/test_gpu_dp.py's "direct equals the collective" check (two ranks in fresh child processes on the one device,
    host-side barriers, bounded waits) at the IQN parameter counts of A = 1 (8k + 1) and A = 3, C = 1 (8k + 3)."""
    from tests.test_gpu_dp import _run_direct
    sizes = (200_785, 200_611)
    assert [s % 8 for s in sizes] == [1, 3]
    assert all(ok is True for _, ok in _run_direct(None, sizes=sizes))
