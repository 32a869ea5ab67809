"""GPU: sampled information-directed action selection (``prism_ids_sample_select``; ``ids_use_random_samples``) held to
the host restatement of tests/select_ref.py, itself held to Philox, to the selector's torch code and to its own
frequencies in tests/test_ids_sampled_host.py.

Direct calls: scores and aux bit-equal to ``prism_ids_select``; the clamped probabilities within 1e-5 relative of the
torch-CPU clamped softmax of the device's own scores (the project's bar for acting outputs; fp32 expf and a sum of at
most 16 terms stay some 40x inside it); the action the float64 inverse CDF of the device's own probabilities, for given
uniforms and for the Philox draw at (seed, c0 + b, "IDSA"), bit for bit.  Agent level: ``Agent.forward`` returns the
restatement's actions at the counters the acting-draw accounting predicts, from the hipGraph and from the eager launches."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import envelope_cases as E
from tests import helpers as H
from tests import select_ref as S
from tests.test_gpu_learner import to_hip_batch
from tests.test_ids_sampled_host import N_DRAWS, SEED

pytestmark = pytest.mark.gpu
HEADS, LMBDA, EPS, RHO = 10, 0.1, 1e-10, 0.25
PROB_RTOL = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _estimates(rng, n, T, A, dev, heads=HEADS):
    """Synthetic z [n][T][A] and q [heads][n_pad][A] (rows past n: poison nobody may read into a result)."""
    n_pad = (n + 15) // 16 * 16
    z = torch.from_numpy((rng.standard_normal((n, T, A)) * 2.0 + 1.0).astype(np.float32)).to(dev)
    q = np.full((heads, n_pad, A), 1e30, dtype=np.float32)
    q[:, :n] = rng.standard_normal((heads, n, A)).astype(np.float32)
    return z, torch.from_numpy(q).to(dev), n_pad


def _sample(z, qb, n, n_pad, T, A, usq=0, u_in=None, seed=SEED, offset=0, rng_counters=None, heads=HEADS):
    """One ``prism_ids_sample_select``: dict of scores, aux, probs, action, host (the pinned copy), all on the CPU."""
    from prism_amd import _native as N
    dev = z.device
    scores, aux = torch.full((n, A), -7.0, device=dev), torch.full((n, 4, A), -7.0, device=dev)
    probs = torch.full((n, A), -7.0, device=dev)
    action = torch.full((n,), -1, dtype=torch.int64, device=dev)
    host = torch.full((n,), -1, dtype=torch.int64).pin_memory()
    u = None if u_in is None else torch.from_numpy(np.asarray(u_in, dtype=np.float64)).to(dev)
    N.check(N.lib().prism_ids_sample_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, heads, LMBDA, EPS, RHO, usq, N.ptr(u), seed, offset,
                                            N.ptr(rng_counters), N.ptr(scores), N.ptr(aux), N.ptr(probs), N.ptr(action),
                                            N.ptr(host), N.current_stream_handle()), "prism_ids_sample_select")
    torch.cuda.synchronize()
    return dict(scores=scores.cpu(), aux=aux.cpu(), probs=probs.cpu().numpy(), action=action.cpu().numpy(), host=host.numpy().copy())


def _deterministic(z, qb, n, n_pad, T, A, usq=0, heads=HEADS):
    from prism_amd import _native as N
    dev = z.device
    scores, aux = torch.empty((n, A), device=dev), torch.empty((n, 4, A), device=dev)
    action = torch.empty(n, dtype=torch.int64, device=dev)
    N.check(N.lib().prism_ids_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, heads, LMBDA, EPS, RHO, usq, N.ptr(scores), N.ptr(aux),
                                     N.ptr(action), None, N.current_stream_handle()), "prism_ids_select")
    torch.cuda.synchronize()
    return scores.cpu(), aux.cpu()


def _boundary_uniforms(probs, rng):
    """Per row a uniform whose t = u * S lands exactly on a cumulative boundary of the row's probabilities where float64
    allows it (the quotient, or a neighbour of it), else as near as it gets: the restatement runs the same arithmetic."""
    p = probs.astype(np.float64)
    out = np.empty(p.shape[0])
    for b in range(p.shape[0]):
        cum = np.add.accumulate(p[b])          # (sequential: index order)
        k = int(rng.integers(0, max(1, p.shape[1] - 1)))
        u = cum[k] / cum[-1]
        for cand in (u, np.nextafter(u, 0.0), np.nextafter(u, 1.0)):
            if cand < 1.0 and cand * cum[-1] == cum[k]:
                u = cand
                break
        out[b] = min(u, 1.0 - 2.0 ** -53)
    return out


DIRECT = [(n, A, T, 0) for n in (1, 3, 17) for A in (1, 2, 6, 16) for T in (8, 200)] + [(3, 6, 8, 1), (17, 16, 200, 2)]


@pytest.mark.parametrize("n,A,T,usq", DIRECT)
def test_direct_calls_equal_the_restatement(dev, n, A, T, usq):
    rng = np.random.default_rng(1000 * n + 10 * A + T + usq)
    z, qb, n_pad = _estimates(rng, n, T, A, dev)
    if usq:
        z, qb = z * 0.5, torch.where(qb > 1e29, qb, qb * 0.5)          # (symexp of the estimates stays of order one)
    ref_scores, ref_aux = _deterministic(z, qb, n, n_pad, T, A, usq)
    assert bool(torch.isfinite(ref_scores).all())
    # given uniforms: 0, the largest double below 1, exactly on a cumulative boundary, random
    first = _sample(z, qb, n, n_pad, T, A, usq, u_in=np.zeros(n))
    us = [np.zeros(n), np.full(n, 1.0 - 2.0 ** -53), _boundary_uniforms(first["probs"], rng), rng.random(n)]
    for i, u in enumerate(us):
        r = first if i == 0 else _sample(z, qb, n, n_pad, T, A, usq, u_in=u)
        assert torch.equal(r["scores"], ref_scores) and torch.equal(r["aux"], ref_aux), "scores / aux differ from prism_ids_select"
        want_p = S.clamped_probs(r["scores"].numpy(), EPS)
        rel = float(np.max(np.abs(r["probs"] - want_p) / want_p))
        print(f"n={n} A={A} T={T} usq={usq} u[{i}]: max rel err of the probabilities {rel:.3e}")
        np.testing.assert_allclose(r["probs"], want_p, rtol=PROB_RTOL, atol=0)
        np.testing.assert_array_equal(r["probs"], first["probs"])
        np.testing.assert_array_equal(r["action"], S.inverse_cdf(r["probs"], u), err_msg=f"u[{i}] = {u}")
        np.testing.assert_array_equal(r["host"], r["action"])
        if A == 1:
            assert not r["action"].any()
    assert not S.inverse_cdf(first["probs"], us[0]).any()          # (u = 0: always the first action)
    # Philox draws: immediate counts, one of them across the 32-bit carry of the low counter word
    for off in (0, 2 ** 32 - 5):
        r = _sample(z, qb, n, n_pad, T, A, usq, offset=off)
        assert torch.equal(r["scores"], ref_scores) and torch.equal(r["aux"], ref_aux)
        np.testing.assert_array_equal(r["probs"], first["probs"])
        np.testing.assert_array_equal(r["action"], S.sample_actions(r["probs"], SEED, off), err_msg=f"offset {off}")
        np.testing.assert_array_equal(r["host"], r["action"])
        assert int(r["action"].min()) >= 0 and int(r["action"].max()) < A
    # the device word: [2] is the count AFTER the forward of this call (n * T draws); read, not written
    words = torch.tensor([11, 22, 1000 + n * T], dtype=torch.int64, device=dev)
    r = _sample(z, qb, n, n_pad, T, A, usq, offset=7, rng_counters=words)
    np.testing.assert_array_equal(r["action"], S.sample_actions(r["probs"], SEED, 1007))
    assert words.cpu().tolist() == [11, 22, 1000 + n * T]


def test_frequencies_on_the_device(dev):
    """65 536 identical rows, A = 6, one action pushed to the clamp floor: draw for draw the restatement's actions at the
    seed of the CPU frequency test, and every count within 5 standard deviations of N p_a / S."""
    A, T = 6, 8
    rng = np.random.default_rng(6)
    z1, q1, _ = _estimates(rng, 1, T, A, dev)
    q1[:, :1, 0] -= 30.0          # a regret of 30: softmax(-score) underflows to the floor
    z = z1.expand(N_DRAWS, T, A).contiguous()
    qb = q1[:, :1].expand(HEADS, N_DRAWS, A).contiguous()
    r = _sample(z, qb, N_DRAWS, N_DRAWS, T, A, seed=SEED, offset=0)
    p = r["probs"]
    assert (p == p[0]).all() and p[0, 0] == np.float32(EPS) and float(p[0].max()) > 0.2
    np.testing.assert_array_equal(r["action"], S.sample_actions(p, SEED, 0))
    w = p[0].astype(np.float64) / p[0].astype(np.float64).sum()
    counts = np.bincount(r["action"], minlength=A)
    for a in range(A):
        mu, sd = N_DRAWS * w[a], np.sqrt(N_DRAWS * w[a] * (1.0 - w[a]))
        print(f"action {a}: p {p[0, a]:.6e} count {counts[a]}, expected {mu:.2f} +- {sd:.2f}")
        assert abs(counts[a] - mu) <= 5.0 * sd
    assert len(np.unique(r["action"])) >= 3


# ---------------------------------------------------------------------------------------------------------------------
# agent level
# ---------------------------------------------------------------------------------------------------------------------
BATCH = 32


def _agent(dev, A, **over):
    from prism_amd.factory import agent_factory
    case = E.ACT_CASES[f"full_a{A}"]
    cfg = H.variant_config(dev, dict(case["over"], ids_use_random_samples=True, batch_size=BATCH, **over))
    torch.manual_seed(E.INIT_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, case["C"]), A)
    gen = torch.Generator().manual_seed(5)
    agent.model.load_state_dict({k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen) for k, v in agent.model.state_dict().items()})
    agent._params_replaced()
    return cfg, agent, case["C"]


def _want_from_raw(agent, cfg, c0):
    """The restatement's actions of the acting call that left ``agent._act_raw``, its forward started at count c0."""
    z, qb, n, n_pad, T = agent._act_raw
    r = _sample(z, qb, n, n_pad, T, agent.dims.n_actions, 0, u_in=np.zeros(n), heads=cfg.ids_n_q_heads)
    return S.sample_actions(r["probs"], agent.seed, c0)


@pytest.mark.parametrize("A", [3, 16])
def test_agent_forward_returns_the_restatements_actions(dev, A):
    cfg, agent, C = _agent(dev, A)
    assert (cfg.ids_lambda, cfg.ids_epsilon, cfg.ids_rho_lower_bound) == (LMBDA, EPS, RHO) and cfg.ids_n_q_heads == HEADS
    sel = agent.action_selector
    assert sel.random_sample and agent.tau_rng == "philox" and agent.act_graph
    assert agent._selector_key(sel) == ("ids_sampled", LMBDA, EPS, RHO, 0)
    T = int(agent.model.distribution_model.n_quantile_samples_per_action)
    rng = np.random.default_rng(4)

    def obs(n):          # (host arrays: one graph per shape, whatever the address)
        return (rng.random((n, 10, 10, C)) < 0.15).astype(np.float32)

    def call(n, graph, where):
        agent.act_graph = graph
        c0 = agent._act_draws
        x = obs(n)
        a = agent.forward(x)
        torch.cuda.synchronize()
        assert (type(a).__name__ == "_Actions") == graph, f"{where}: graph path expected {graph}"
        assert agent._act_draws == c0 + n * T, f"{where}: the selector must not move the acting count"
        if graph:
            assert int(agent.rng_counters[2].item()) == agent._act_draws, f"{where}: device acting counter"
        got = a.cpu().numpy().copy()
        np.testing.assert_array_equal(got, _want_from_raw(agent, cfg, c0), err_msg=f"{where} at count {c0}")
        np.testing.assert_array_equal(torch.Tensor.cpu(a.as_subclass(torch.Tensor)).numpy(), got)
        agent.act_graph = True
        return got

    agent._act_draws = 300
    cap = None
    for n in (1, 17):
        # the agent's very first acting call rebuilds the packed weight copies (a graph key of its own: n = 1 here, not
        # n = 17); the first call of the steady form launches eagerly on the device counter, its second captures, later
        # ones replay
        for i in range(3):
            call(n, True, f"n={n} graph call {i}")
        st = [s for k, s in agent._act_graphs.items() if k[0] == n and k[1][0] == "ids_sampled" and s["g"] is not None]
        assert len(st) == 1 and st[0]["calls"] == (2 if n == 1 else 3), "the second call of the steady form captures the graph"
        graphs, before = list(st[0]["g"]), st[0]["calls"]
        call(n, True, f"n={n} replay")
        call(n, False, f"n={n} eager in between")
        call(n, True, f"n={n} replay after an eager call")
        assert all(x is y for x, y in zip(st[0]["g"], graphs)) and st[0]["calls"] == before + 2, "the capture is reused"
    # across an update: other parameters, the packed weight copies rebuilt, the counts go on
    batch, w, _ = H.random_batch(np.random.default_rng(2), BATCH, C, A, cfg)
    agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
    for n in (17, 1):
        call(n, True, f"n={n} after the update")
        call(n, False, f"n={n} eager after the update")
        call(n, True, f"n={n} graph after the update")
    # more observations than the workspace takes: pieces, every piece a call of its own with its own count
    cap = agent._act_cap
    assert cap == BATCH
    n = cap + 7
    x = obs(n)
    c0 = agent._act_draws
    a = agent.forward(x)
    torch.cuda.synchronize()
    assert tuple(a.shape) == (n,) and agent._act_draws == c0 + n * T
    got = a.cpu().numpy().copy()
    agent._act_draws = c0
    want = []
    for i in range(0, n, cap):
        c = agent._act_draws
        agent.act_estimates(x[i:i + cap])
        want.append(_want_from_raw(agent, cfg, c))
    assert agent._act_draws == c0 + n * T
    np.testing.assert_array_equal(got, np.concatenate(want))
    # same count, same actions; the next count, other uniforms
    agent._act_draws = c0
    np.testing.assert_array_equal(agent.forward(x).cpu().numpy(), got)


def test_parity_mode_keeps_the_torch_path(dev):
    """``tau_rng == "torch"``: the selector's torch code and ``torch.multinomial`` on torch's generator, as before; the
    default mode beside it selects natively."""
    cfg, agent, C = _agent(dev, 3, tau_rng="torch")
    _, native, _ = _agent(dev, 3)
    sel = agent.action_selector
    assert sel.random_sample and agent._selector_key(sel) is None
    assert native._selector_key(native.action_selector) == ("ids_sampled", LMBDA, EPS, RHO, 0)
    rng = np.random.default_rng(8)
    for n in (1, 17):
        x = torch.from_numpy((rng.random((n, 10, 10, C)) < 0.15).astype(np.float32)).to(dev)
        torch.manual_seed(77)
        a = agent.forward(x)
        assert type(a).__name__ != "_Actions"
        torch.manual_seed(77)
        q, dist = agent.act_estimates(x)
        want = sel.select_action(sel.generate_action_probs(dist, q))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(a.cpu().numpy(), want.cpu().numpy())
        a = native.forward(x)
        assert type(native.forward(x)).__name__ == "_Actions" and tuple(a.shape) == (n,)
