"""GPU: every quantile sample the kernels draw, held bit for bit to the host restatement ``tests/helpers.py::philox_taus``
(itself held to the published Philox vectors and to common.h compiled for the host: tests/test_philox_host.py).

The one formula every drawing site implements (step_kernels.h cos_basis_block with its three tile forms, both tile
prologues of fwd_kernels.h, the acting offsets of learner.hip prism_act_forward):

    tau[t * B + b] = float32(Philox(seed, offset + t * B + b, "TAU0" + sid)[0] >> 8) * 2**-24

and the counter accounting (hip_agent.py): one counter space for all updates of an agent -- step k, whichever path ran it,
draws at offset k * 3 * max(T, T') * B -- and a second one, stream 3, for acting, counted in observations * samples.

The learner records what it drew (``tau_out``) and is compared directly.  Acting records nothing: the call that draws on
the device is compared with the same entry point handed the host's samples, which runs the same arithmetic on the same
numbers (bit-equal), and with the CPU oracle on the host's samples at the acting tolerance."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_acting import TOL, updated_agent
from tests.test_gpu_learner import LOSS_TOL, to_hip_batch
from tests.test_gpu_step import _mk
from tests.test_gpu_variants import _batch, _config

pytestmark = pytest.mark.gpu
C, A = 4, 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _tt(T, Tn=None):
    return dict(iqn_n_current_state_quantile_samples=T, iqn_n_next_state_quantile_samples=T if Tn is None else Tn)


_TARGET_DQ = dict(use_target_network=True, use_double_q_learning=True)
_W256 = dict(iqn_quantile_model_feature_dim=256)

# Shapes of tests/test_gpu_variants.py / the golden update cases, by what they reach: how many samples share a 16-row tile
# (kind-2 tiles with current- and next-state rows side by side for T <= 8 without a target network: T = 4 two samples a
# tile, T = 8 one; kind-0 tiles otherwise), T' != T (the stride of tau_out is max(T, T')), a batch that is no multiple of
# 64, all three streams, both hidden widths, a model with Q heads beside the IQN rows.
UPDATE_CASES = {
    "c3": dict(B=256, over=dict()),
    "tau4": dict(B=32, over=_tt(4)),
    "tau16": dict(B=16, over=_tt(16)),
    "tau8_next16": dict(B=16, over=_tt(8, 16)),
    "tau16_next8": dict(B=16, over=_tt(16, 8)),
    "ragged48": dict(B=48, over=dict()),
    "target": dict(B=32, over=dict(use_target_network=True)),
    "target_dq": dict(B=32, over=dict(_TARGET_DQ)),
    "tau16_target_dq": dict(B=16, over=dict(_tt(16), **_TARGET_DQ)),
    "w256_tau8": dict(B=64, over=dict(_W256)),
    "w256_tau32": dict(B=64, over=dict(_W256, **_tt(32))),
    "w256_tau64_target_dq": dict(B=16, over=dict(_W256, **_tt(64), **_TARGET_DQ)),
    "ids_full_small": dict(B=16, over=dict(use_ids=True, use_target_network=True)),
}
# the launch forms are run on these
STEP_CASES = {
    "c3": dict(B=256, over=dict()),
    "tau4": dict(B=32, over=_tt(4)),
    "tau8_next16": dict(B=16, over=_tt(8, 16)),
    "target_dq": dict(B=32, over=dict(_TARGET_DQ)),
}


def _span(cfg, B):
    return H.tau_span(cfg, B)


def _build(dev, over, seed=11):
    from prism_amd.factory import agent_factory
    cfg = _config(dev, over)
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A)
    return cfg, agent


def host_update_taus(agent, cfg, B, offset):
    """The quantile samples of the update that starts at counter `offset`, as the oracle takes them."""
    T, Tn = cfg.iqn_n_current_state_quantile_samples, cfg.iqn_n_next_state_quantile_samples
    return [torch.from_numpy(H.philox_taus(agent.seed, offset, T if sid == H.TAU_CUR else Tn, B, sid)).reshape(-1, 1)
            for sid in H.tau_streams(cfg)]


def assert_tau_out(agent, cfg, B, offset, where=""):
    """``agent.tau_out`` after the update that started at counter `offset`: the streams the configuration draws equal the
    host's, bit for bit.  A stream it does not draw (fill_iqn_args: no next-state pass on the online network with a target
    network and no double-Q, no target pass without a target network), and the tail of a row past T_sid * B when
    T != T', are written by nobody: they stay at the zeros the buffer was allocated with -- asserted, so a draw that lands
    in the wrong row or past its stream's end shows here even where nothing reads it."""
    T, Tn = cfg.iqn_n_current_state_quantile_samples, cfg.iqn_n_next_state_quantile_samples
    torch.cuda.synchronize()
    out = agent.tau_out.cpu().numpy()
    assert out.dtype == np.float32 and out.shape == (3, max(T, Tn) * B)
    used = H.tau_streams(cfg)
    for sid in range(3):
        n = (T if sid == H.TAU_CUR else Tn) * B if sid in used else 0
        if sid in used:
            np.testing.assert_array_equal(out[sid, :n], H.philox_taus(agent.seed, offset, n // B, B, sid),
                                          err_msg=f"{where}: stream {sid} at counter {offset}")
        assert not out[sid, n:].any(), f"{where}: stream {sid} written past its {n} samples"


def assert_disjoint(ranges):
    """Counter ranges [lo, hi) drawn over a run: no counter twice."""
    spans = sorted(ranges)
    for (lo0, hi0), (lo1, hi1) in zip(spans, spans[1:]):
        assert lo0 < hi0 <= lo1 < hi1, f"counter ranges overlap: [{lo0}, {hi0}) and [{lo1}, {hi1})"


# ---------------------------------------------------------------------------------------------------------------------
# the learner's draws
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gemm_mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", sorted(UPDATE_CASES))
def test_update_draws_equal_the_host_restatement(dev, name, gemm_mode):
    """``agent.update`` without ``taus`` (host-issued offset).  fp32: the forward tiles draw in their own prologue
    (fwd_kernels.h, exact chain); bf16x3: the embed launch draws for them (step_kernels.h cos_basis_block)."""
    case = UPDATE_CASES[name]
    B = case["B"]
    cfg, agent = _build(dev, dict(case["over"], gemm_mode=gemm_mode))
    rng = np.random.default_rng(2)
    ranges = []
    for step in range(3):
        batch, w, _ = _batch(rng, B, C, A, cfg)
        off = step * _span(cfg, B)
        assert agent._draw_offset + agent._fused_tau == off
        agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
        assert_tau_out(agent, cfg, B, off, f"{name} step {step}")
        ranges.append((off, off + _span(cfg, B) // 3))
        agent.tau_out.zero_()          # (so that a step that wrote nothing cannot pass on the last step's record)
    assert_disjoint(ranges)


@pytest.mark.parametrize("name", ["c3", "target_dq"])
def test_update_on_host_drawn_taus_matches_the_oracle(dev, name):
    """The circle the parity tests leave open (they feed the oracle the device's own record): the oracle is given the
    HOST's samples and the device, drawing for itself, must land on its TD errors."""
    from oracle.learner_ref import LearnerOracle
    case = UPDATE_CASES[name]
    B, seed = case["B"], 11
    cfg, agent = _build(dev, case["over"], seed=seed)
    cpu_cfg = _config("cpu", case["over"])
    sd, tgt = H.build_init_state(cpu_cfg, seed, C=C, A=A)
    for k, v in agent.model.state_dict().items():
        np.testing.assert_array_equal(v.cpu().numpy(), sd[k].numpy(), err_msg=k)
    orc = LearnerOracle(sd, H.spec_from_config(cpu_cfg, C=C, A=A), tgt)
    rng = np.random.default_rng(1)
    for step in range(2):
        batch, w, _ = _batch(rng, B, C, A, cfg)
        taus = host_update_taus(agent, cfg, B, step * _span(cfg, B))
        td_o = orc.update(batch, w, taus)
        td = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
        torch.cuda.synchronize()
        err = float((td.cpu() - td_o).abs().max())
        print(f"{name} step {step}: max |td - oracle td| = {err:.3e}")
        np.testing.assert_allclose(td.cpu().numpy(), td_o.numpy(), rtol=0, atol=LOSS_TOL)


def _learner(dev, case, fused, graph, fuse_tail=True, **extra):
    return _mk(dev, fused, graph, B=case["B"], cap=4096, fuse_tail=fuse_tail, **dict(case["over"], **extra))


def _fused_step(ln, k, ranges, where, fused_before=None):
    """Step k (0-based, over ALL updates the agent has run) of a learner through ``Learner.step()``; checks its draws and
    the device counters' host mirrors."""
    agent, cfg = ln.agent, ln.agent.config
    B = cfg.batch_size
    ln.step(timesteps_this_iteration=1)
    off = k * _span(cfg, B)
    assert_tau_out(agent, cfg, B, off, f"{where} step {k}")
    ranges.append((off, off + _span(cfg, B) // 3))
    if ln.fused:
        n_fused = (k if fused_before is None else fused_before) + 1
        assert agent._fused_tau == n_fused * _span(cfg, B)
        assert int(agent.rng_counters[1].item()) == agent._fused_tau, f"{where} step {k}: device tau counter"
        assert int(agent.rng_counters[0].item()) == n_fused * B, f"{where} step {k}: device PER counter"
    agent.tau_out.zero_()


@pytest.mark.parametrize("gemm_mode", ["auto", "fp32"])
@pytest.mark.parametrize("form", ["unfused", "fused_eager", "graph", "graph_split_tail"])
@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_learner_step_draws_equal_the_host_restatement(dev, name, form, gemm_mode):
    """``Learner.step()`` in each of its launch forms: sample() -> update() (host-issued offset), the fused step launched
    eagerly (offset + device counter), and the hipGraph of it through warm-up, capture and four replays, with the fused
    tail and with the post + back launch pair.  Every step draws at k * 3 max(T, T') B, whatever ran it."""
    fused, graph = form != "unfused", form.startswith("graph")
    ln = _learner(dev, STEP_CASES[name], fused, graph, fuse_tail=form != "graph_split_tail", gemm_mode=gemm_mode)
    ranges = []
    for k in range(6 if graph else 3):
        _fused_step(ln, k, ranges, f"{name} {form}")
    if graph:
        assert any(isinstance(g, tuple) for g in ln.agent._graphs.values()), "no step was replayed from a hipGraph"
    assert_disjoint(ranges)


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_fused_steps_and_updates_share_one_counter_space(dev, name):
    """fused, fused (captured), fused (replayed), ``update()``, then fused again: the update moves the host-issued part of
    the offset, which the captured launches bake, so the graph is warmed and captured anew -- and the draws go on as one
    sequence."""
    case = STEP_CASES[name]
    ln = _learner(dev, case, True, True)
    agent, cfg, B = ln.agent, ln.agent.config, case["B"]
    ranges, k = [], 0
    for _ in range(3):
        _fused_step(ln, k, ranges, f"{name} mixed")
        k += 1
    graphs_before = [g for g in agent._graphs.values() if isinstance(g, tuple)]
    assert graphs_before
    batch, w, _ = _batch(np.random.default_rng(4), B, C, A, cfg)
    agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
    assert_tau_out(agent, cfg, B, k * _span(cfg, B), f"{name} mixed update()")
    ranges.append((k * _span(cfg, B), k * _span(cfg, B) + _span(cfg, B) // 3))
    assert agent._draw_offset == _span(cfg, B) and agent._fused_tau == 3 * _span(cfg, B)
    agent.tau_out.zero_()
    k += 1
    for i in range(4):
        _fused_step(ln, k, ranges, f"{name} mixed", fused_before=3 + i)
        k += 1
    graphs_after = [g for g in agent._graphs.values() if isinstance(g, tuple)]
    assert graphs_after and graphs_after[0] is not graphs_before[0]
    assert_disjoint(ranges)
    assert len(ranges) == 8


# ---------------------------------------------------------------------------------------------------------------------
# acting draws
# ---------------------------------------------------------------------------------------------------------------------
def _cap(agent):
    """Observations one ``prism_act_forward`` call takes (hip_agent.py act_estimates)."""
    dm = agent.dims
    return (agent._B // 16) * 16 if (dm.n_heads > 0 and dm.head_layers == 2) else agent._B


def host_act_taus(agent, draws, n):
    """The samples ``act_estimates`` draws for n observations starting at acting count `draws`, in the reference's order
    ([T * n, 1], tau-major over all n).  More observations than one call takes go in pieces; every piece is a call of its
    own: its own width in the counter (t * n_piece + b) and the count moved on by T * n_piece."""
    T = int(agent.model.distribution_model.n_quantile_samples_per_action)
    cap = _cap(agent)
    full = np.empty((T, n), dtype=np.float32)
    for i in range(0, n, cap):
        m = min(cap, n - i)
        full[:, i:i + m] = H.philox_taus(agent.seed, draws, T, m, H.TAU_ACT).reshape(T, m)
        draws += T * m
    return torch.from_numpy(full.reshape(-1, 1)), T


def oracle_act(agent, g, obs, taus, T, chunk=64):
    """``oracle.learner_ref.act_forward`` on the agent's parameters, a few observations at a time."""
    from oracle.learner_ref import act_forward
    sd = {k: v.cpu() for k, v in agent.model.state_dict().items()}
    spec = H.spec_from_config(H.case_config(g), C=int(g["C"]), A=int(g["A"]))
    n = obs.shape[0]
    qs, ds = [], []
    for i in range(0, n, chunk):
        j = min(n, i + chunk)
        q, d = act_forward(sd, spec, obs[i:j].cpu(), taus.view(T, n)[:, i:j].reshape(-1, 1))
        qs.append(q)
        ds.append(d)
    return torch.cat(qs, dim=0), torch.cat(ds, dim=1)


def _obs(rng, n, Cn, dev):
    return torch.from_numpy((rng.random((n, 10, 10, Cn)) < 0.1).astype(np.float32)).to(dev)


def assert_eager_call_draws_at(agent, obs, g=None, where=""):
    """One ``act_estimates(obs)`` drawing on the device against the same call on the host's samples at the count the call
    started from: the same kernels on the same numbers, so equal bit for bit; the count moves by T * n."""
    n = int(obs.shape[0])
    draws = agent._act_draws
    taus, T = host_act_taus(agent, draws, n)
    q, dist = agent.act_estimates(obs)
    q, dist = q.clone(), dist.clone()
    assert agent._act_draws == draws + T * n, f"{where}: acting count after the call"
    q_h, dist_h = agent.act_estimates(obs, taus=taus.to(obs.device))
    agent._act_draws = draws + T * n          # (the explicit call counted too: back to where the checked call left it)
    torch.cuda.synchronize()
    assert tuple(dist.shape) == (T, n, agent.dims.n_actions)
    assert torch.equal(dist, dist_h), f"{where}: device-drawn estimates differ from those on the host's samples at count {draws}" \
        f" (max |diff| {float((dist - dist_h).abs().max()):.3e})"
    assert torch.equal(q, q_h), f"{where}: q"
    if g is not None:
        q_o, dist_o = oracle_act(agent, g, obs, taus, T)
        np.testing.assert_allclose(dist.cpu().numpy(), dist_o.numpy(), rtol=0, atol=TOL, err_msg=where)
        np.testing.assert_allclose(q.cpu().numpy(), q_o.numpy(), rtol=0, atol=TOL, err_msg=where)


@pytest.mark.parametrize("gemm_mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", ["iqn_c3", "full_small", "abl_ids"])
def test_eager_acting_draws_equal_the_host_restatement(dev, name, gemm_mode):
    """``act_estimates`` for 1, 5, 16 and 17 observations (a partial tile, whole tiles, one row into the next; 17 is more
    than the full_small workspace takes at once), then B + 7 and 2 B + 5 in pieces, one call after the other on a running
    count.  fp32 / bf16x3: the two tile prologues of fwd_kernels.h."""
    g, cfg, agent = updated_agent(name, dev, gemm_mode=gemm_mode)
    B = int(g["B"])
    rng = np.random.default_rng(6)
    assert agent._act_draws == 0
    for n in (1, 5, 16, 17, B + 7, 2 * B + 5):
        assert_eager_call_draws_at(agent, _obs(rng, n, int(g["C"]), dev), g, f"{name} n={n}")
    # a count past 2**32: the high counter word is the call's too
    agent._act_draws = 2 ** 32 - 300
    assert_eager_call_draws_at(agent, _obs(rng, 5, int(g["C"]), dev), g, f"{name} across the 32-bit carry")


def _graph_call_checked(agent, frame_in, frame_dev, where):
    """One ``Agent.forward`` through the hipGraph path; its raw estimate buffers against the explicit-sample call at the
    count the call started from, and the device counter against its host mirror."""
    draws = agent._act_draws
    n = int(frame_dev.shape[0])
    taus, T = host_act_taus(agent, draws, n)
    act = agent.forward(frame_in)
    torch.cuda.synchronize()
    assert type(act).__name__ == "_Actions", f"{where}: the call did not take the graph path"
    assert agent._act_draws == draws + T * n
    assert int(agent.rng_counters[2].item()) == agent._act_draws, f"{where}: device acting counter vs its host mirror"
    z, qb, n_, n_pad, T_ = agent._act_raw
    assert (n_, T_) == (n, T)
    z, qb = z[:n * T].clone(), (None if qb is None else qb[:, :n].clone())
    agent.act_estimates(frame_dev, taus=taus.to(frame_dev.device))
    agent._act_draws = draws + T * n
    z_h, qb_h = agent._act_raw[0][:n * T], agent._act_raw[1]
    torch.cuda.synchronize()
    assert torch.equal(z, z_h), f"{where}: graph-drawn estimates differ from those on the host's samples at count {draws}" \
        f" (max |diff| {float((z - z_h).abs().max()):.3e})"
    if qb is not None:
        assert torch.equal(qb, qb_h[:, :n]), f"{where}: q"
    return act, (z, taus, T)


@pytest.mark.parametrize("name", ["iqn_c3", "full_small", "abl_ids"])
def test_graph_acting_draws_equal_the_host_restatement(dev, name):
    """``Agent.forward`` from its hipGraph: the first call of a shape (eager launches on the device counter), the capture
    call and the replays, for host arrays, one persistent device buffer and fresh device tensors.  (The explicit-sample
    call in between moves the host count on and back; the graph path re-seeds the device word only when the two differ.)"""
    g, cfg, agent = updated_agent(name, dev)
    Cn, n = int(g["C"]), 5
    rng = np.random.default_rng(3)
    frames = [(rng.random((n, 10, 10, Cn)) < 0.1).astype(np.float32) for _ in range(5)]
    assert agent.act_graph
    agent._act_draws = 4000
    first = None
    for i, f in enumerate(frames):                                     # host arrays in
        _, rec = _graph_call_checked(agent, f, torch.from_numpy(f).to(dev), f"{name} host call {i}")
        first = first or (f, rec)
    # the device-drawn estimates of one graph call against the oracle on the host's samples
    f, (z, taus, T) = first
    q_o, dist_o = oracle_act(agent, g, torch.from_numpy(f), taus, T)
    np.testing.assert_allclose(z.view(n, T, -1).permute(1, 0, 2).cpu().numpy(), dist_o.numpy(), rtol=0, atol=TOL)
    buf = torch.zeros((n, 10, 10, Cn), device=dev)
    for i, f in enumerate(frames):                                     # one persistent device buffer, read in place
        buf.copy_(torch.from_numpy(f))
        _graph_call_checked(agent, buf, buf, f"{name} buffer call {i}")
    keep = []
    for i, f in enumerate(frames):                                     # a fresh device tensor every call
        keep.append(torch.from_numpy(f).to(dev))
        _graph_call_checked(agent, keep[-1], keep[-1], f"{name} fresh call {i}")
    assert any(k[2] == "dev" for k in agent._act_graphs)
    assert sum(st["g"] is not None for st in agent._act_graphs.values()) >= 3, "not every input form was replayed from a graph"
    assert agent._act_draws == 4000 + 15 * n * int(agent.model.distribution_model.n_quantile_samples_per_action)


# ---------------------------------------------------------------------------------------------------------------------
# acting after fused learner steps: the descriptor the steps leave behind points at the device counters
# ---------------------------------------------------------------------------------------------------------------------
def _stepped_learner(dev, graph, steps):
    ln = _learner(dev, STEP_CASES["c3"], True, graph)
    for _ in range(steps):
        ln.step(timesteps_this_iteration=1)
    torch.cuda.synchronize()
    if graph:
        assert any(isinstance(g, tuple) for g in ln.agent._graphs.values())
    return ln


@pytest.mark.parametrize("graph", [False, True], ids=["fused_eager", "graph"])
def test_eager_acting_after_fused_steps_draws_at_the_host_count(dev, graph):
    """After ``Learner.step()`` the eager acting call still draws at the host's acting count (not at host count + device
    word), call after call, and leaves the learner's streams alone."""
    steps = 5 if graph else 3
    ln = _stepped_learner(dev, graph, steps)
    agent, cfg, B = ln.agent, ln.agent.config, STEP_CASES["c3"]["B"]
    rng = np.random.default_rng(8)
    word = int(agent.rng_counters[2].item())
    for i, n in enumerate((5, 5, 16, 3)):
        assert_eager_call_draws_at(agent, _obs(rng, n, C, dev), None, f"eager call {i} after {steps} fused steps")
    assert agent._act_draws == 29 * int(agent.model.distribution_model.n_quantile_samples_per_action)
    # the device word belongs to the graph path: eager calls count on the host alone
    assert int(agent.rng_counters[2].item()) == word
    assert int(agent.rng_counters[0].item()) == steps * B and int(agent.rng_counters[1].item()) == steps * _span(cfg, B)
    agent.tau_out.zero_()
    _fused_step(ln, steps, [], "the step after acting")


@pytest.mark.parametrize("graph", [False, True], ids=["fused_eager", "graph"])
def test_graph_and_eager_acting_interleaved_with_learner_steps(dev, graph):
    """graph forward, eager forward, graph forward, the explore branch of epsilon-greedy, graph forward, a learner step,
    eager forward, graph forward -- against a twin (same construction, same steps: identical parameters) that acts
    eagerly throughout from the same count: the same actions, the same estimates bit for bit and the same final acting count.  The device word
    ``rng_counters[2]`` belongs to the graph path: where a graph call has just run it equals the count; the twin, which
    never acts from a graph, must leave it where it was."""
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    steps = 5 if graph else 3
    mixed, twin = _stepped_learner(dev, graph, steps), _stepped_learner(dev, graph, steps)
    assert torch.equal(mixed.agent.flat, twin.agent.flat)
    cfg, B = mixed.agent.config, STEP_CASES["c3"]["B"]
    T = int(mixed.agent.model.distribution_model.n_quantile_samples_per_action)
    rng = np.random.default_rng(9)
    n = 5
    frames = [_obs(rng, n, C, dev) for _ in range(7)]
    twin_word = int(twin.agent.rng_counters[2].item())
    program = ["graph", "eager", "graph", "explore", "graph", "step", "eager", "graph"]

    def run(ln, all_eager):
        agent, acts, it = ln.agent, [], iter(frames)
        greedy = agent.action_selector
        agent._act_draws = 600
        for op in program:
            if op == "step":
                ln.step(timesteps_this_iteration=1)
                continue
            if op == "explore":
                agent.action_selector = EGreedyActionSelector(1.0, 1.0, 0, seed=7)
            agent.act_graph = op == "graph" and not all_eager
            a = agent.forward(next(it))
            if op == "graph" and not all_eager:
                assert type(a).__name__ == "_Actions"
                assert int(agent.rng_counters[2].item()) == agent._act_draws
            # (the explore branch runs no model; otherwise the raw estimates go into the comparison too: five greedy actions
            # may survive a wrong draw, the 200 estimates per observation and action do not)
            z = None if op == "explore" else agent._act_raw[0][:n * T].clone()
            acts.append((a.cpu().numpy().copy(), z))
            agent.action_selector = greedy
        torch.cuda.synchronize()
        return acts

    got, want = run(mixed, False), run(twin, True)
    for i, ((x, zx), (y, zy)) in enumerate(zip(got, want)):
        what = f"forward call {i} ({[p for p in program if p != 'step'][i]})"
        np.testing.assert_array_equal(x, y, err_msg=what)
        assert (zx is None and zy is None) or torch.equal(zx, zy), f"{what}: estimates differ from the all-eager twin's"
    assert mixed.agent._act_draws == twin.agent._act_draws == 600 + 7 * T * n
    assert int(mixed.agent.rng_counters[2].item()) == mixed.agent._act_draws
    assert int(twin.agent.rng_counters[2].item()) == twin_word
    assert torch.equal(mixed.agent.flat, twin.agent.flat)
    # the learner's own streams: what the step count alone predicts, and the next step draws where it should
    for ln in (mixed, twin):
        agent = ln.agent
        assert int(agent.rng_counters[0].item()) == (steps + 1) * B
        assert int(agent.rng_counters[1].item()) == (steps + 1) * _span(cfg, B) == agent._fused_tau
        agent.tau_out.zero_()
        _fused_step(ln, steps + 1, [], "the step after the acting sequence")
