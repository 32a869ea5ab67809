"""GPU: the linear IQN head (iqn_quantile_model_layers = 0; prism_amd/csrc/iqn_lin_kernels.h) in both gemm_mode values.

  1. the two fixtures recorded from the live reference (tests/golden/update_iqn_l0*.npz), every step: recorded values and
     the oracle;
  2. generated edge cases against the oracle (tests/iqn_linear_cases.py);
  3. the launch forms over a ring of 64 slots filled by ``extend``: sample() -> update() == fused eager step == hipGraph
     replay, bit for bit;
  4. every quantile draw against the host's Philox restatement at the counters DESIGN 4.2 predicts: update, fused step, acting;
  5. acting: the fixtures' recorded estimates and actions, hipGraph == eager, epsilon-greedy's greedy branch;
  6. two agents of one seed stay bit-identical over 20 fused steps;
  7. save / load into a fresh agent continues bit-identically.

Tolerances are the project's (tests/test_gpu_learner.py): losses and TD errors 1e-5; gradients 1e-4 max|g| + 1e-7 against the
better of the oracle's fp32 and fp64 autograd, with NO kink allowance (tests/test_iqn_linear_host.py shows the inputs
kink-free by the oracle alone); global norm 1e-4 relative; parameters after the step 2e-6; post_l2 rtol 2e-6."""
import contextlib
import io
import weakref

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import iqn_linear_cases as L
from tests.test_gpu_acting import TOL, updated_agent
from tests.test_gpu_learner import build_hip_agent, to_hip_batch
from tests.test_gpu_rng_streams import assert_disjoint, assert_eager_call_draws_at, assert_tau_out, host_act_taus

pytestmark = pytest.mark.gpu
LOSS_TOL, PARAM_TOL = 1e-5, 2e-6
MODES = ["fp32", "bf16x3"]
L0 = dict(iqn_quantile_model_layers=0)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _check_step(agent, sd, rec, where, lr_eps=None):
    """TD errors, total loss, every gradient tensor, the global norm and the parameters after the step against the oracle's
    record of the same step."""
    torch.cuda.synchronize()
    np.testing.assert_allclose(agent.out_td.cpu().numpy(), rec["td"].numpy(), rtol=0, atol=LOSS_TOL, err_msg=where)
    assert abs(float(agent._static_total_loss) - rec["total"]) < LOSS_TOL, where
    off, gflat = 0, agent.grads.cpu()
    for k in sd:
        n = sd[k].numel()
        go, g64 = rec["grads"][k].reshape(-1), rec["g64"][k].reshape(-1)
        gh = gflat[off:off + n]
        tol = 1e-4 * float(go.abs().max()) + 1e-7
        err32, err64 = float((gh - go).abs().max()), float((gh.double() - g64).abs().max())
        print(f"{where} grad {k}: max err {err32:.3e} (vs fp64 {err64:.3e}), tolerance {tol:.3e}")
        assert min(err32, err64) <= tol, f"{where} grad {k}: max err {err32:.3e} (vs fp64: {err64:.3e}) > {tol:.3e}"
        off += n
    assert off == agent.flat.numel()
    assert abs(float(agent.scalars[3]) - rec["grad_norm"]) < 1e-4 * max(1.0, rec["grad_norm"]), where
    post = agent.model.state_dict()
    for k, v in rec["post"].items():
        np.testing.assert_allclose(post[k].cpu().numpy(), v.numpy(), rtol=0, atol=PARAM_TOL, err_msg=f"{where} {k}")


# ------------------------------------------------------------------------------------------------------ 1. fixtures
@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("name", L.FIXTURES)
def test_fixture_matches_reference_and_oracle(dev, name, gemm_mode):
    g = H.load_case(name)
    cfg, agent = build_hip_agent(g, dev, gemm_mode=gemm_mode)
    assert agent.dims.iqn_layers == 0 and agent.off.iqn_w1 == -1
    np.testing.assert_array_equal(np.array([float(v.double().sum()) for v in agent.model.state_dict().values()]), g["init_sum"])
    cpu_cfg, spec, sd, steps = L.fixture_run(name)
    for step, rec in enumerate(steps):
        td = agent.update(to_hip_batch(rec["batch"], dev), per_weights=rec["w"].to(dev), taus=[t.to(dev) for t in rec["taus"]])
        torch.cuda.synchronize()
        pre = f"s{step}/"
        np.testing.assert_allclose(td.cpu().numpy(), g[pre + "td"], rtol=0, atol=LOSS_TOL)
        np.testing.assert_allclose(agent._static_distribution_loss.cpu().numpy(), g[pre + "dl"], rtol=0, atol=LOSS_TOL)
        assert agent._static_q_loss is None
        assert abs(float(agent._static_total_loss) - float(g[pre + "total"])) < LOSS_TOL
        _check_step(agent, sd, rec, f"{name} {gemm_mode} step {step}")
        l2 = np.array([float(v.double().norm()) for v in agent.model.state_dict().values()])
        np.testing.assert_allclose(l2, g[pre + "post_l2"], rtol=2e-6, atol=1e-7)
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()
    assert int(agent.optimizer.step_t.item()) == int(g["steps"])
    agent.check_status()


# ------------------------------------------------------------------------------------------------------ 2. generated cases
def _build_agent(cfg, C, A, seed=L.INIT_SEED):
    from prism_amd.factory import agent_factory
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        return agent_factory.build_agent(cfg, (10, 10, C), A)


@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("name", list(L.UPDATE_CASES))
def test_generated_case_matches_oracle(dev, name, gemm_mode):
    case = L.UPDATE_CASES[name]
    A, C = case["A"], case["C"]
    cpu_cfg, spec, sd, steps = L.oracle_run(name)
    cfg = L.case_config(name, device=dev, gemm_mode=gemm_mode)
    agent = _build_agent(cfg, C, A)
    for k, v in agent.model.state_dict().items():          # same seed, same construction order
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k].numpy(), err_msg=k)
    assert agent.flat.numel() % 4 == A % 4
    for step, rec in enumerate(steps):
        agent.update(to_hip_batch(rec["batch"], dev), per_weights=rec["w"].to(dev), taus=[t.to(dev) for t in rec["taus"]])
        _check_step(agent, sd, rec, f"{name} {gemm_mode} step {step}")
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()
    assert int(agent.optimizer.step_t.item()) == case["steps"]
    agent.check_status()


@pytest.mark.parametrize("phi_bias,conv_bias", [(0.0, 0.0), (10.0, 2.0), (30.0, 5.0), (100.0, 10.0)])
@pytest.mark.parametrize("gemm_mode", MODES)
def test_layernorm_rows_with_large_mean(dev, phi_bias, conv_bias, gemm_mode):
    """tests/test_gpu_ln_stress.py for the linear head, whose LayerNorm(1024) feeds the estimates directly: rows whose mean
    is large against their spread (phi and conv biases raised).  Same bars: within 1e-5 of the fp32 oracle and parameters
    within 2e-6 up to the second setting; beyond it the loss error against float64 within twice torch's own fp32 error
    (+ 3e-6)."""
    from oracle.learner_ref import LearnerOracle, composite_losses
    g = H.load_case("iqn_l0")
    cfg, agent = build_hip_agent(g, dev, gemm_mode=gemm_mode)
    with torch.no_grad():
        sd = agent.model.state_dict()            # views of the flat parameter buffer: written in place
        sd["distribution_model.phi.0.bias"] += phi_bias
        sd["embedding_model.model.0.bias"] += conv_bias
    sd0 = {k: v.detach().cpu().clone() for k, v in agent.model.state_dict().items()}
    batch, w, taus = H.case_batch(g, 0)
    td = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus])
    torch.cuda.synchronize()
    spec = H.spec_from_config(cfg, C=int(g["C"]), A=int(g["A"]))
    orc = LearnerOracle(sd0, spec, None)
    orc.update(batch, w, taus)
    dl32 = orc.last["dl"]
    p64 = {k: v.double() for k, v in sd0.items()}
    b64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in batch.items()}
    dl64 = composite_losses(p64, None, spec, b64, [t.double() for t in taus])[0]
    dl = agent.out_dl.cpu()
    floor = float((dl32.double() - dl64).abs().max())            # what fp32 arithmetic costs torch itself here
    err64, err32 = float((dl.double() - dl64).abs().max()), float((dl - dl32).abs().max())
    print(f"{gemm_mode} phi_bias {phi_bias} conv_bias {conv_bias}: |dl - fp64| {err64:.2e} (torch fp32: {floor:.2e}), "
          f"|dl - fp32 oracle| {err32:.2e}")
    assert err64 <= 2.0 * floor + 3e-6, f"kernel loss error vs fp64 {err64} against torch's own fp32 error {floor}"
    if phi_bias <= 10.0:
        assert err32 <= 1e-5, f"loss error vs the fp32 oracle {err32}"
        post = agent.model.state_dict()
        perr = max(float((post[k].cpu() - v).abs().max()) for k, v in orc.state_dict().items())
        assert perr <= 2e-6, f"parameter error after Adam {perr}"
    assert np.isfinite(td.cpu().numpy()).all()


# ------------------------------------------------------------------------------------------------------ 3. launch forms
def _ring_learner(dev, fused, graph, over, B=16, cap=64, C=4, A=6, gemm_mode="auto"):
    """A learner on a depth-0 model whose 64-slot ring was filled by ``extend``: three interleaved streams, episode ends and
    truncations, written once round and a third of the way again."""
    from prism_amd.config import baseline_config
    from prism_amd.experience import Timestep
    from prism_amd.learner import Learner
    cfg = baseline_config(2, device=dev, batch_size=B, experience_replay_capacity=cap, gemm_mode=gemm_mode, **dict(L0, **over))
    cfg.fused_step, cfg.hip_graph, cfg.fuse_tail = fused, graph, True
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, C), n_actions=A)
    rng = np.random.default_rng(5)
    frame = lambda: torch.from_numpy((rng.random((10, 10, C)) < 0.1).astype(np.float32))
    n_streams, rows = 3, cap + cap // 3 + 5
    cur = [Timestep(id=e, obs=frame()) for e in range(n_streams)]
    keep = []
    for i in range(rows):
        e = i % n_streams
        t, u = cur[e], rng.random()
        t.reward, t.action = float(rng.standard_normal()), int(rng.integers(0, A))
        t.done, t.truncated = bool(u < 0.07), bool(0.07 <= u < 0.10)
        nxt = Timestep(id=n_streams + i, obs=frame())
        if t.truncated:
            t.next = Timestep(id=10_000 + i, obs=frame())
        elif not t.done:
            t.next = weakref.ref(nxt)
        keep.append(t)
        ln.experience_buffer.extend(t)
        cur[e] = nxt
        if i % 16 == 15:          # (a staging block holds at most `capacity` rows)
            ln.experience_buffer.flush()
    ln.experience_buffer.flush()
    ln._keep = keep + cur
    assert len(ln.experience_buffer) == cap
    return ln


def _form_state(ln):
    buf, ag = ln.experience_buffer, ln.agent
    torch.cuda.synchronize()
    trees = (buf.sum_tree.cpu().numpy(), buf.min_tree.cpu().numpy()) if buf.use_per else (np.zeros(1), np.zeros(1))
    return (ag.out_td.cpu().numpy(), buf._index.cpu().numpy(), buf._weight.cpu().numpy(), ag.flat.cpu().numpy(),
            ag.grads.cpu().numpy(), ag.tau_out.cpu().numpy(), float(ag.scalars[0]), float(ag.scalars[3])) + trees + \
        tuple(b.cpu().numpy() for b in ag.optimizer.buffers()) + \
        ((ag.flat_target.cpu().numpy(),) if ag.flat_target is not None else ())


FORM_CASES = {"per": dict(), "uniform": dict(use_per=False),
              "per_noln_target_dq": dict(use_layer_norm=False, use_target_network=True, use_double_q_learning=True,
                                         target_update_period=2)}


@pytest.mark.parametrize("name", list(FORM_CASES))
def test_launch_forms_are_bit_identical(dev, name):
    over = FORM_CASES[name]
    ref, fus, gra = (_ring_learner(dev, f, g, over) for f, g in ((False, False), (True, False), (True, True)))
    assert ref.agent.dims.iqn_layers == 0
    for step in range(4):
        outs = []
        for ln in (ref, fus, gra):
            ln.step(timesteps_this_iteration=1)
            outs.append(_form_state(ln))
        for i, other in enumerate(outs[1:]):
            for j, (x, y) in enumerate(zip(outs[0], other)):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} step {step}, form {i + 1}, item {j}")
        assert np.isfinite(outs[0][3]).all() and outs[0][5].any()
    for ln in (ref, fus, gra):
        assert int(ln.agent.optimizer.step_t.item()) == 4
        ln.agent.check_status()
        ln.experience_buffer.check_status()
    assert any(isinstance(g, tuple) for g in gra.agent._graphs.values())      # a graph really was captured
    if over.get("use_target_network"):          # ... and the target network was synchronised on the way (period 2)
        assert torch.equal(ref.agent.flat_target, gra.agent.flat_target) and bool((ref.agent.flat_target != 0).any())


# ------------------------------------------------------------------------------------------------------ 4. quantile draws
TAU_CASES = {"t8_b16": (16, dict()), "t8n16_b4": (4, dict(iqn_n_current_state_quantile_samples=8, iqn_n_next_state_quantile_samples=16)),
             "t16_b3_target_dq": (3, dict(iqn_n_current_state_quantile_samples=16, iqn_n_next_state_quantile_samples=16,
                                          use_target_network=True, use_double_q_learning=True)),
             "t64_b1_noln": (1, dict(iqn_n_current_state_quantile_samples=64, iqn_n_next_state_quantile_samples=64,
                                     use_layer_norm=False))}


@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("name", list(TAU_CASES))
def test_update_draws_equal_the_host_restatement(dev, name, gemm_mode):
    B, over = TAU_CASES[name]
    cfg = H.variant_config(dev, dict(L0, gemm_mode=gemm_mode, **over))
    agent = _build_agent(cfg, 4, 6)
    rng = np.random.default_rng(2)
    span, ranges = H.tau_span(cfg, B), []
    for step in range(3):
        batch, w, _ = H.random_batch(rng, B, 4, 6, cfg)
        assert agent._draw_offset + agent._fused_tau == step * span
        agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
        assert_tau_out(agent, cfg, B, step * span, f"{name} step {step}")
        ranges.append((step * span, step * span + span // 3))
        agent.tau_out.zero_()
    assert_disjoint(ranges)


@pytest.mark.parametrize("form", ["fused_eager", "graph"])
@pytest.mark.parametrize("name", ["per", "per_noln_target_dq"])
def test_fused_step_draws_equal_the_host_restatement(dev, name, form):
    ln = _ring_learner(dev, True, form == "graph", FORM_CASES[name])
    agent, cfg, B = ln.agent, ln.agent.config, 16
    span, ranges = H.tau_span(cfg, B), []
    for k in range(4):
        ln.step(timesteps_this_iteration=1)
        assert_tau_out(agent, cfg, B, k * span, f"{name} {form} step {k}")
        ranges.append((k * span, k * span + span // 3))
        assert agent._fused_tau == (k + 1) * span and int(agent.rng_counters[1].item()) == agent._fused_tau
        assert int(agent.rng_counters[0].item()) == (k + 1) * B
        agent.tau_out.zero_()
    assert_disjoint(ranges)


@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("name", L.FIXTURES)
def test_acting_draws_equal_the_host_restatement(dev, name, gemm_mode):
    """``act_estimates`` drawing on the device against the same call on the host's samples at the count it started from
    (bit-equal) and against the oracle (1e-5): one observation, a partial tile, one row into the next, more than the
    workspace takes at once."""
    g, cfg, agent = updated_agent(name, dev, gemm_mode=gemm_mode)
    rng = np.random.default_rng(6)
    assert agent._act_draws == 0
    for n in (1, 5, 17, int(g["B"]) + 7):
        obs = torch.from_numpy((rng.random((n, 10, 10, int(g["C"]))) < 0.1).astype(np.float32)).to(dev)
        assert_eager_call_draws_at(agent, obs, g, f"{name} n={n}")


# ------------------------------------------------------------------------------------------------------ 5. acting
@pytest.mark.parametrize("gemm_mode", MODES)
@pytest.mark.parametrize("name", L.FIXTURES)
def test_acting_matches_the_recorded_reference(dev, name, gemm_mode):
    g, cfg, agent, orc = updated_agent(name, dev, with_oracle=True, gemm_mode=gemm_mode)
    obs, taus, ref = H.case_act(g)
    # the acting forward on the oracle's parameters after the same updates (pinned to the reference's: tests/test_iqn_linear_host.py)
    agent.model.load_state_dict(orc.state_dict())
    agent._params_replaced()
    q, dist = agent.act_estimates(obs.to(dev), taus=taus.to(dev))
    torch.cuda.synchronize()
    assert tuple(dist.shape) == ref["dist"].shape == (cfg.iqn_quantile_samples_per_action, obs.shape[0], int(g["A"]))
    np.testing.assert_allclose(dist.cpu().numpy(), ref["dist"], rtol=0, atol=TOL)
    np.testing.assert_allclose(q.cpu().numpy(), ref["q"], rtol=0, atol=TOL)
    sel = agent.action_selector
    np.testing.assert_array_equal(sel.select_action(sel.generate_action_probs(dist, q)).cpu().numpy(), ref["action"])
    # prism_greedy_select on the buffers the forward left
    from prism_amd import _native as N
    z, qb, n, n_pad, T = agent._act_raw
    action = torch.full((n,), -1, dtype=torch.int64, device=dev)
    N.check(N.lib().prism_greedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, int(g["A"]), 0, N.ptr(action), None, None,
                                        N.current_stream_handle()), "prism_greedy_select")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(action.cpu().numpy(), ref["action"])


@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("name", L.FIXTURES)
def test_forward_from_the_hipgraph_equals_the_eager_launches(dev, name, n):
    """Agent.forward replayed from its hipGraph against the eager launches on the same counters: actions, the raw estimate
    rows the graph's forward left, the acting count and its device mirror."""
    g, cfg, agent = updated_agent(name, dev)
    A, C = int(g["A"]), int(g["C"])
    T = agent._act_T()
    if n > agent._B:          # (more observations than the fixture's workspace takes at once: make room, as a collector's agent has)
        agent._prepare(32)
    rng = np.random.default_rng(3)
    frames = [(rng.random((n, 10, 10, C)) < 0.15).astype(np.float32) for _ in range(5)]
    assert agent.act_graph
    agent.act_graph = False
    agent._act_draws = 777
    want, want_z = [], []
    for f in frames:
        want.append(agent.forward(f).cpu().numpy().copy())
        want_z.append(agent._act_raw[0][:n * T].clone())
    end_draws = agent._act_draws
    assert end_draws == 777 + len(frames) * T * n and all(w.min() >= 0 and w.max() < A for w in want)
    agent.act_graph = True
    agent._act_draws = 777
    for i, f in enumerate(frames):
        a = agent.forward(f)
        assert type(a).__name__ == "_Actions"
        np.testing.assert_array_equal(a.cpu().numpy(), want[i])
        torch.cuda.synchronize()
        assert torch.equal(agent._act_raw[0][:n * T], want_z[i]), f"frame {i}: estimates of the graph's forward"
    assert agent._act_draws == end_draws and int(agent.rng_counters[2].item()) == end_draws
    assert any(st["g"] is not None for st in agent._act_graphs.values()), "no call was replayed from a graph"


@pytest.mark.parametrize("name", L.FIXTURES)
def test_epsilon_greedy_takes_the_greedy_branch_natively(dev, name):
    """EGreedyActionSelector with epsilon 0: every call takes the greedy branch, i.e. prism_greedy_select on the linear
    head's estimates -- the action of the mean over the host-drawn quantile samples of the same counters; with epsilon 1 the
    forward's draws are consumed all the same."""
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    g, cfg, agent = updated_agent(name, dev)
    C, n = int(g["C"]), 5
    rng = np.random.default_rng(9)
    obs = torch.from_numpy((rng.random((n, 10, 10, C)) < 0.15).astype(np.float32)).to(dev)
    agent.action_selector = EGreedyActionSelector(0.0, 0.0, 0, seed=7)
    for graph in (False, True):
        agent.act_graph = graph
        draws = agent._act_draws
        taus, T = host_act_taus(agent, draws, n)
        act = agent.forward(obs).cpu().numpy()
        assert agent._act_draws == draws + T * n
        q, dist = agent.act_estimates(obs, taus=taus.to(dev))
        agent._act_draws = draws + T * n
        np.testing.assert_array_equal(act, torch.argmax(dist.mean(dim=0), dim=-1).cpu().numpy())
    agent.action_selector = EGreedyActionSelector(1.0, 1.0, 0, seed=7)
    draws = agent._act_draws
    act = agent.forward(obs)
    assert agent._act_draws == draws + agent._act_T() * n and tuple(act.shape) == (n,)


# ------------------------------------------------------------------------------------------------------ 6. determinism
@pytest.mark.parametrize("name", ["per", "per_noln_target_dq"])
def test_two_agents_of_one_seed_stay_bit_identical(dev, name):
    a, b = (_ring_learner(dev, True, True, FORM_CASES[name]) for _ in range(2))
    for step in range(20):
        a.step(timesteps_this_iteration=1)
        b.step(timesteps_this_iteration=1)
        if step in (0, 1, 2, 9, 19):
            for j, (x, y) in enumerate(zip(_form_state(a), _form_state(b))):
                np.testing.assert_array_equal(x, y, err_msg=f"{name} step {step}, item {j}")
    assert int(a.agent.optimizer.step_t.item()) == 20 and np.isfinite(a.agent.flat.cpu().numpy()).all()
    a.agent.check_status()
    b.agent.check_status()


# ------------------------------------------------------------------------------------------------------ 7. checkpoints
@pytest.mark.parametrize("name", L.FIXTURES)
def test_save_load_continues_bit_identically(dev, tmp_path, name):
    g = H.load_case(name)
    cfg, agent = build_hip_agent(g, dev)
    batch, w, taus = H.case_batch(g, 0)
    agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus])
    if cfg.use_target_network:
        agent.sync_target_model()
    agent.save(str(tmp_path))
    _, other = build_hip_agent(g, dev)                    # (at the initial weights, one update behind)
    assert not torch.equal(agent.flat.cpu(), other.flat.cpu())
    other.load(str(tmp_path))
    torch.cuda.synchronize()
    assert torch.equal(agent.flat.cpu(), other.flat.cpu())
    for x, y in zip(agent.optimizer.buffers(), other.optimizer.buffers()):
        assert torch.equal(x.cpu(), y.cpu())
    assert int(agent.optimizer.step_t.item()) == int(other.optimizer.step_t.item()) == 1
    sd = torch.load(str(tmp_path / "agent" / "model.pt"), map_location="cpu")
    assert list(sd.keys()) == [str(k) for k in g["param_names"]]
    batch, w, taus = H.case_batch(g, 1)
    td0 = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus]).clone()
    td1 = other.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus]).clone()
    torch.cuda.synchronize()
    assert torch.equal(td0.cpu(), td1.cpu()) and torch.equal(agent.flat.cpu(), other.flat.cpu())
    assert torch.equal(agent.grads.cpu(), other.grads.cpu())
