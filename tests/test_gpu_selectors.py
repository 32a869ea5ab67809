"""GPU: the MinRegret and SimpleIDS action selectors on the device (prism_amd/csrc/act_ensemble.hip:
``prism_min_regret_select``, ``prism_simple_ids_select``).

Direct calls on every case of the seeded table (tests/selector_cases.py) against the reference's recorded outputs
(tests/golden/selectors_ref.npz): actions exactly -- no row of the table is near a tie --, values within rtol 2e-4 / atol 1e-7
without an unsquish function and rtol 1e-3 / atol 1e-6 with one (what tests/test_gpu_acting.py holds the IDS scores to); the
pad rows of the estimates are NaN and must never be read.  MinRegret's mean and spread bit-equal to ``prism_ids_select``'s;
exact ties; ``Agent.forward`` with both selectors from the hipGraph, eagerly and in pieces; the vector evaluator with the
MinRegret evaluation selector; checkpoints, one of them with a ``state.pkl`` the reference wrote."""
import os
import shutil

import numpy as np
import pytest
import torch

from tests import eval_ref as ER
from tests import helpers as H
from tests import select_ens_ref as E
from tests import selector_cases as T
from tests.test_gpu_acting import updated_agent
from tests.test_selectors_host import close, table_items

pytestmark = pytest.mark.gpu
USQ_ID = {"none": 0, "obs_look_further": 1, "symlog": 2}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def to_qb(q, dev, pad_value=float("nan")):
    """``q [n, A, heads]`` -> the device layout ``[heads][n_pad][A]``, pad rows filled with ``pad_value``."""
    q = torch.as_tensor(q)
    n, A, heads = q.shape
    n_pad = (n + 15) // 16 * 16
    qb = torch.full((heads, n_pad, A), pad_value)
    qb[:, :n] = q.permute(2, 0, 1)
    return qb.to(dev), n_pad


def run(kind, qb, n, n_pad, A, heads, scalar, usq, dev):
    """One direct call: dict(action, host_action, scores [n, A], aux [n, 2 or 3, A]) on the CPU."""
    from prism_amd import _native as N
    rows = 2 if kind == "min_regret" else 3
    scores = torch.full((n, A), float("nan"), device=dev)
    aux = torch.full((n, rows, A), float("nan"), device=dev)
    action = torch.full((n,), -1, dtype=torch.int64, device=dev)
    host = torch.full((n,), -1, dtype=torch.int64).pin_memory()
    fn = getattr(N.lib(), f"prism_{kind}_select")
    N.check(fn(N.ptr(qb), n, n_pad, A, heads, scalar, USQ_ID[usq], N.ptr(scores), N.ptr(aux), N.ptr(action), N.ptr(host),
               N.current_stream_handle()), kind)
    torch.cuda.synchronize()
    return dict(action=action.cpu().numpy(), host_action=host.numpy().copy(), scores=scores.cpu().numpy(), aux=aux.cpu().numpy())


@pytest.mark.parametrize("unsquish", T.UNSQUISH)
def test_direct_calls_on_every_table_case(dev, unsquish):
    seen = 0
    for c, q, r in table_items():
        if c["unsquish"] != unsquish:
            continue
        n, A, heads = q.shape
        qb, n_pad = to_qb(q, dev)
        for i, lm in enumerate(T.LAMBDAS):
            got = run("min_regret", qb, n, n_pad, A, heads, lm, unsquish, dev)
            np.testing.assert_array_equal(got["action"], r["mr_action"][i], err_msg=str((c, lm)))
            np.testing.assert_array_equal(got["host_action"], got["action"])
            close(got["scores"], r["mr_scores"][i], unsquish, (c, lm, "regret^2"))
            close(got["aux"][:, 0], r["si_mean"], unsquish, (c, "mean"))          # (the reference's MinRegret keeps no mean)
            close(got["aux"][:, 1], r["mr_spread"], unsquish, (c, "spread"))
        for i, beta in enumerate(T.BETAS):
            got = run("simple_ids", qb, n, n_pad, A, heads, beta, unsquish, dev)
            np.testing.assert_array_equal(got["action"], r["si_action"][i], err_msg=str((c, beta)))
            np.testing.assert_array_equal(got["host_action"], got["action"])
            close(got["scores"], r["si_scaled"][i], unsquish, (c, beta, "scaled"))
            close(got["aux"][:, 0], r["si_mean"], unsquish, (c, "mean"))
            close(got["aux"][:, 1], r["si_max_diff"], unsquish, (c, "max_diff"))
            # the centred means are no loggable of the reference's: held to the host restatement, itself held to the fixture
            close(got["aux"][:, 2], E.simple_ids(q, beta, unsquish)["q_values"], unsquish, (c, "q_values"))
        seen += 1
    assert seen == 12


def test_min_regret_mean_and_spread_are_bit_equal_to_ids(dev):
    from prism_amd import _native as N
    rng = np.random.default_rng(2)
    T_ = 8
    seen = set()
    for c, q, r in table_items():
        n, A, heads = q.shape
        qb, n_pad = to_qb(q, dev)
        z = torch.from_numpy(rng.standard_normal((n_pad * T_, A)).astype(np.float32)).to(dev)
        scores = torch.empty((n, A), device=dev)
        aux = torch.empty((n, 4, A), device=dev)
        action = torch.empty(n, dtype=torch.int64, device=dev)
        N.check(N.lib().prism_ids_select(N.ptr(z), N.ptr(qb), n, n_pad, T_, A, heads, 0.1, 1e-10, 0.25, USQ_ID[c["unsquish"]],
                                         N.ptr(scores), N.ptr(aux), N.ptr(action), None, N.current_stream_handle()),
                "prism_ids_select")
        got = run("min_regret", qb, n, n_pad, A, heads, 0.1, c["unsquish"], dev)
        ids = aux.cpu().numpy()
        assert got["aux"][:, 0].tobytes() == ids[:, 0].tobytes(), (c, "mean")
        assert got["aux"][:, 1].tobytes() == ids[:, 1].tobytes(), (c, "spread")
        seen.add(c["unsquish"])
    assert seen == set(T.UNSQUISH)


D = torch.tensor([0.5, -0.5, 0.25, -0.25])          # head offsets that cancel exactly (dyadic: every sum is exact)


def _tie_cases(A):
    """(tied actions, value) per row, as tests/test_gpu_envelope.py builds its IDS ties; the rows with one winner at the
    end or in the middle fail a kernel that answers 0 everywhere."""
    return [(list(range(A)), 1.0), ([0, A - 1], 2.0), ([A - 1], 2.0), ([A // 2, A - 1], 0.5), ([A // 2], -1.0)]


@pytest.mark.parametrize("A", [2, 7, 16])
def test_exact_ties(dev, A):
    from prism_amd.agents import action_selectors as S
    rng = np.random.default_rng(A)
    rows, heads = _tie_cases(A), 4
    n = len(rows)
    # MinRegret: the tied actions' heads agree exactly (no spread) at the largest upper bound: regret, and the score, is
    # exactly zero for them in any correct evaluation and above zero for every other action; the first tied minimum wins
    q = torch.zeros((n, A, heads))
    for i, (tied, val) in enumerate(rows):
        q[i] = val - 1.0 - torch.from_numpy(rng.random((A, 1)).astype(np.float32)) + 0.1 * D[None, :]      # below val by >= 0.5
        q[i, tied, :] = val
    qb, n_pad = to_qb(q, dev)
    for lm in (0.0, 0.1, 1.0):
        got = run("min_regret", qb, n, n_pad, A, heads, lm, "none", dev)
        sel = S.MinRegretActionSelector(lm)
        want = sel.select_action(sel.generate_action_probs(None, q)).numpy()
        for i, (tied, _) in enumerate(rows):
            assert want[i] == tied[0] and float(np.abs(got["scores"][i, tied]).max()) == 0.0, (lm, i)
            assert all(got["scores"][i, a] > 0 for a in range(A) if a not in tied), (lm, i)
        np.testing.assert_array_equal(got["action"], want)
        np.testing.assert_array_equal(got["host_action"], want)
        close(got["scores"], sel.regret_squared(q).numpy(), "none", lm)
    # SimpleIDS: the tied actions carry the same heads -- the same mean and the same widest gap, so the same scaled value
    # bit for bit -- above every other action in both terms (mean higher by >= 0.5, gap 1 against 0.1): they win at every
    # beta, also where only one term counts (beta = 0: the gap alone, beta = 1: the mean alone); the first tied maximum wins
    q = torch.zeros((n, A, heads))
    for i, (tied, val) in enumerate(rows):
        q[i] = val - 1.0 - torch.from_numpy(rng.random((A, 1)).astype(np.float32)) + 0.1 * D[None, :]
        q[i, tied, :] = val + D
    qb, n_pad = to_qb(q, dev)
    for beta in (0.0, 1.0, 0.8, 0.5):
        got = run("simple_ids", qb, n, n_pad, A, heads, beta, "none", dev)
        sel = S.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, beta)
        want = sel.select_action(sel.generate_action_probs(None, q, for_log=True)).numpy()
        for i, (tied, _) in enumerate(rows):
            assert want[i] == tied[0], (beta, i)
            assert len(set(got["scores"][i, tied].tolist())) == 1, (beta, i)
            assert all(got["scores"][i, a] < got["scores"][i, tied[0]] for a in range(A) if a not in tied), (beta, i)
        np.testing.assert_array_equal(got["action"], want)
        np.testing.assert_array_equal(got["host_action"], want)
        close(got["scores"], sel.loggables["Scaled Q Values"].numpy(), "none", beta)
        if beta == 0.0:
            np.testing.assert_array_equal(got["scores"], got["aux"][:, 1])          # the widest gap alone
        if beta == 1.0:
            np.testing.assert_array_equal(got["scores"], got["aux"][:, 2])          # the centred mean alone


# ------------------------------------------------------------------------------------------------ the agent
KNOBS = dict(eval_action_selector="min_regret", ids_action_selector="simple_ids")


@pytest.fixture(scope="module")
def agent_full_small(dev):
    g, cfg, agent = updated_agent("full_small", dev, **KNOBS)
    return g, cfg, agent


def _modes(agent):
    """(name, enter, leave, key) of the two selectors under test."""
    return [("min_regret", agent.eval, agent.train, "min_regret"), ("simple_ids", lambda: None, lambda: None, "simple_ids")]


def test_forward_selects_natively_eagerly_and_in_pieces(dev, agent_full_small):
    """n = 2 B + 5 observations: served in pieces, every piece selected by its kernel from its own estimate buffers; the
    actions are the selector's torch code on ``act_estimates`` at the same Philox counters.  n = 5 the same, eagerly."""
    from prism_amd.agents import action_selectors as S
    g, cfg, agent = agent_full_small
    assert type(agent.eval_action_selector) is S.MinRegretActionSelector
    assert type(agent.action_selector) is S.SimpleIDSActionSelector and agent.action_selector.beta == cfg.ids_beta == 0.8
    C, A = int(g["C"]), int(g["A"])
    rng = np.random.default_rng(9)
    big = 2 * int(g["B"]) + 5
    obs = torch.from_numpy((rng.random((big, 10, 10, C)) < 0.1).astype(np.float32)).to(dev)
    keep_graph = agent.act_graph
    try:
        for name, enter, leave, key in _modes(agent):
            enter()
            sel = agent.eval_action_selector if name == "min_regret" else agent.action_selector
            skey = agent._selector_key(sel)
            assert skey is not None and skey[0] == key and skey[-1] == 0
            for n, graph in ((big, True), (5, False)):
                agent.act_graph = graph
                agent._act_draws = 5000
                act = agent.forward(obs[:n])
                agent._act_draws = 5000
                q, dist = agent.act_estimates(obs[:n])
                want = sel.select_action(sel.generate_action_probs(dist, q))
                torch.cuda.synchronize()
                assert act.dtype == torch.int64 and tuple(act.shape) == (n,)
                np.testing.assert_array_equal(act.cpu().numpy(), want.cpu().numpy(), err_msg=f"{name}, n = {n}")
            leave()
    finally:
        agent.act_graph = keep_graph
        agent.train()


def test_forward_from_the_hipgraph_equals_the_eager_launches(dev, agent_full_small):
    """Seven calls replayed from the acting hipGraph against the eager launches at the same counters, twice over."""
    g, cfg, agent = agent_full_small
    C = int(g["C"])
    rng = np.random.default_rng(3)
    n = 5
    assert agent.act_graph
    frames = [(rng.random((n, 10, 10, C)) < 0.1).astype(np.float32) for _ in range(7)]
    try:
        for name, enter, leave, key in _modes(agent):
            enter()
            agent.act_graph = False
            agent._act_draws = 777
            want = [agent.forward(f).cpu().numpy().copy() for f in frames]
            end_draws = agent._act_draws
            agent.act_graph = True
            for _ in range(2):
                agent._act_draws = 777
                for i, f in enumerate(frames):
                    a = agent.forward(f)
                    assert type(a).__name__ == "_Actions" and a.is_cuda and a.dtype == torch.int64
                    np.testing.assert_array_equal(a.cpu().numpy(), want[i], err_msg=f"{name}, call {i}")      # the pinned copy
                    np.testing.assert_array_equal(torch.Tensor.cpu(a.as_subclass(torch.Tensor)).numpy(), want[i])
                assert agent._act_draws == end_draws
            graphs = [st for k, st in agent._act_graphs.items() if k[1][0] == key]
            assert graphs and any(st["g"] is not None for st in graphs), f"{name}: no call was replayed from a graph"
            assert all(st["scores"] is not None and tuple(st["scores"].shape) == (n, agent.dims.n_actions) for st in graphs)
            leave()
    finally:
        agent.act_graph = True
        agent.train()


def _eval_agent(dev, act_graph):
    import contextlib
    import io
    from prism_amd.config import baseline_config
    from prism_amd.factory import agent_factory
    cfg = baseline_config(3, device=dev, batch_size=32, log_to_wandb=False, seed=31)
    cfg.act_graph, cfg.eval_action_selector = act_graph, "min_regret"
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, 4), 6)
    gen = torch.Generator().manual_seed(5)          # away from the initialisation, as tests/test_gpu_eval.py does
    agent.model.load_state_dict({k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen)
                                 for k, v in agent.model.state_dict().items()})
    agent._params_replaced()
    return agent


def test_vector_evaluator_with_the_min_regret_selector(dev):
    from prism_amd.agents import action_selectors as S
    from prism_amd.evals import VectorEvaluator
    n, steps, horizon = 5, 24, 53
    rng = np.random.default_rng(n)
    kind = np.where(rng.random((steps, n)) < 0.12, rng.integers(1, 4, (steps, n)), 0).astype(np.uint8)
    kind[-1] = 1          # (an episode ends before the script does)
    reward = rng.integers(-2, 4, (steps, n)).astype(np.float64)
    host = ER.EvalHost(n, horizon)
    used = ER.run_script(host, reward, kind)
    runs = []
    for act_graph in (True, False):
        agent = _eval_agent(dev, act_graph)
        assert type(agent.eval_action_selector) is S.MinRegretActionSelector and agent.act_graph == act_graph
        warm = agent.forward(ER.ScriptedEnvs(reward, kind)._frames[0])          # a training call first: its draws are counted
        draws = agent._act_draws
        assert draws == n * agent._act_T() > 0 and tuple(warm.shape) == (n,)
        envs = ER.ScriptedEnvs(reward, kind)
        ev = VectorEvaluator(agent, envs, 0, horizon)
        returns = ev.evaluate_agent()
        np.testing.assert_array_equal(ER.bits64(returns), ER.bits64(host.returns()))
        assert ev.last == host.result() and ev.last["timesteps"] == used * n
        # the evaluation left the training draw counters where they were and the agent in train mode
        assert agent._act_draws == draws and not agent._is_eval and ev.eval_draws == used * n * agent._act_T()
        runs.append((np.stack(envs.actions), returns, ev.last))
        # the actions are the selector's torch code on the estimates of the same observations
        sel = agent.eval_action_selector
        q, dist = agent.act_estimates(torch.from_numpy(envs._frames[0]).to(dev))
        np.testing.assert_array_equal(runs[-1][0][0], sel.select_action(sel.generate_action_probs(dist, q)).cpu().numpy())
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(ER.bits64(runs[0][1]), ER.bits64(runs[1][1]))
    assert runs[0][2] == runs[1][2] and len(np.unique(runs[0][0])) > 1


def test_checkpoints_keep_both_selectors(dev, agent_full_small, tmp_path):
    """``save`` -> ``load`` into an agent built WITHOUT the knobs: both selectors come along and act as before.  The same
    directory with the ``state.pkl`` the reference wrote (tests/golden/ref_state_min_regret) loads and acts too."""
    from prism_amd.agents import action_selectors as S
    from tests.test_gpu_learner import build_hip_agent
    g, cfg, agent = agent_full_small
    rng = np.random.default_rng(17)
    obs = (rng.random((5, 10, 10, int(g["C"]))) < 0.1).astype(np.float32)

    def acts(a):
        out = []
        a._act_draws = 100
        out.append(a.forward(obs).cpu().numpy().copy())
        a.eval()
        out.append(a.forward(obs).cpu().numpy().copy())
        a.train()
        return out

    want = acts(agent)
    agent.save(str(tmp_path / "ours"))
    raw = open(tmp_path / "ours" / "agent" / "state.pkl", "rb").read()
    assert b"prism_amd" not in raw
    for name in (b"MinRegretActionSelector", b"SimpleIDSActionSelector"):
        assert b"cprism.agents.action_selectors\n" + name + b"\n" in raw
    shutil.copytree(tmp_path / "ours", tmp_path / "theirs")
    shutil.copy(os.path.join(H.GOLDEN, "ref_state_min_regret", "state.pkl"), tmp_path / "theirs" / "agent" / "state.pkl")
    for which in ("ours", "theirs"):
        _, other = build_hip_agent(g, dev)
        assert type(other.action_selector) is S.IDSActionSelector and type(other.eval_action_selector) is S.GreedyActionSelector
        other.load(str(tmp_path / which))
        assert type(other.action_selector) is S.SimpleIDSActionSelector, which
        assert type(other.eval_action_selector) is S.MinRegretActionSelector, which
        # (the reference-written selectors carry the same constants: lambda 0.1, beta 0.8, no unsquish function)
        assert (other.action_selector.beta, other.eval_action_selector.lmbda) == (0.8, 0.1) == (cfg.ids_beta, cfg.ids_lambda)
        assert other._selector_key(other.eval_action_selector) == ("min_regret", 0.1, 0)
        assert other._selector_key(other.action_selector) == ("simple_ids", 0.8, 0)
        assert torch.equal(agent.flat.cpu(), other.flat.cpu())
        got = acts(other)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b, err_msg=which)
