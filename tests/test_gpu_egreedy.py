"""GPU: epsilon-greedy action selection per observation (``prism_egreedy_select``; ``config.e_greedy_per_env``) held to the
host restatement of tests/egreedy_ref.py, itself held to Philox, to the selector's ``LinearAnneal`` and to its own
frequencies in tests/test_egreedy_host.py.

Direct calls: the greedy action is ``prism_greedy_select``'s on the same buffers (exact ties included); coin, random action,
``out_explored`` and ``out_epsilon`` are the restatement's, bit for bit, for given coins and for the Philox draw at
(seed, s0 + row, "EGRD"); the device word advances by the rows of every call, also under hipGraph replay.  Agent level:
``Agent.forward`` in the mode returns the restatement's actions at the counter ``epsilon.current_step`` predicts, from the
hipGraph and from the eager launches, leaves the selector's host generator and the quantile-draw count alone, and resumes
exactly; ``Learner.learn()`` over a vector collector is reproducible."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import egreedy_ref as R
from tests import helpers as H
from tests.test_gpu_learner import to_hip_batch

pytestmark = pytest.mark.gpu
SEED = 123
MID = (1.0, 0.1, 1000, 400)          # (start, stop, anneal steps, rows seen before): mid-anneal
ANNEALS = [(0.0, 0.0, 0, 0), (1.0, 1.0, 0, 7), MID, (0.5, 0.5, 0, 2 ** 32 - 5)]      # eps 0 | 1 | mid | across the 32-bit carry


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _estimates(rng, n, T, A, heads, dev, ties=False):
    """Synthetic ``(z [n][T][A] or None, q [heads][n_pad][A] or None, n_pad)``: T = 0 -> the q path alone, heads = 0 -> the
    z path alone (rows of q past n: poison nobody may read into a result).  ``ties``: small whole numbers, so that sums
    are exact and several actions share the maximal mean."""
    n_pad = (n + 15) // 16 * 16

    def values(shape):
        if ties:
            return rng.integers(-1, 2, shape).astype(np.float32)
        return rng.standard_normal(shape).astype(np.float32)

    z = torch.from_numpy(values((n, T, A))).to(dev) if T else None
    q = None
    if heads:
        q = np.full((heads, n_pad, A), 1e30, dtype=np.float32)
        q[:, :n] = values((heads, n, A))
        q = torch.from_numpy(q).to(dev)
    return z, q, n_pad


def _greedy(z, qb, n, n_pad, T, A, heads):
    """``prism_greedy_select`` on the buffers: (actions, means) on the CPU."""
    from prism_amd import _native as N
    dev = (z if z is not None else qb).device
    action = torch.full((n,), -1, dtype=torch.int64, device=dev)
    mean = torch.full((n, A), -7.0, device=dev)
    N.check(N.lib().prism_greedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, heads, N.ptr(action), N.ptr(mean), None,
                                        N.current_stream_handle()), "prism_greedy_select")
    torch.cuda.synchronize()
    return action.cpu().numpy(), mean.cpu()


def _egreedy(z, qb, n, n_pad, T, A, heads, anneal, seed=SEED, row0=0, n_call=None, word=None, u_in=None, sync=True, out=None):
    """One ``prism_egreedy_select``: dict of action, host (the pinned copy), explored, eps, mean, all on the CPU (``out``:
    device outputs to reuse, ``sync`` off: the launch alone, e.g. under capture)."""
    from prism_amd import _native as N
    dev = (z if z is not None else qb).device
    start, stop, steps, steps0 = anneal
    if out is None:
        out = dict(action=torch.full((n,), -1, dtype=torch.int64, device=dev), mean=torch.full((n, A), -7.0, device=dev),
                   host=torch.full((n,), -1, dtype=torch.int64).pin_memory(), eps=torch.full((1,), -1.0, dtype=torch.float64, device=dev),
                   explored=torch.full((n,), 9, dtype=torch.uint8, device=dev))
    u = None if u_in is None else torch.from_numpy(np.asarray(u_in, dtype=np.float64)).to(dev)
    N.check(N.lib().prism_egreedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, A, heads, start, stop, steps, seed, steps0, row0,
                                         n if n_call is None else n_call, N.ptr(word), N.ptr(u), N.ptr(out["mean"]),
                                         N.ptr(out["eps"]), N.ptr(out["explored"]), N.ptr(out["action"]), N.ptr(out["host"]),
                                         N.current_stream_handle()), "prism_egreedy_select")
    if not sync:
        return out
    torch.cuda.synchronize()
    return _host(out)


def _host(out):
    return dict(action=out["action"].cpu().numpy(), host=out["host"].numpy().copy(), explored=out["explored"].cpu().numpy(),
                eps=float(out["eps"].cpu()[0]), mean=out["mean"].cpu())


def _check(r, greedy, mean, A, anneal, seed=SEED, row0=0, n_call=None, coins=None, where=""):
    start, stop, steps, steps0 = anneal
    n = len(greedy)
    want, explored, eps = R.select(greedy, seed, steps0, row0, n if n_call is None else n_call, A, start, stop, steps, coins)
    assert np.float64(r["eps"]).tobytes() == np.float64(eps).tobytes(), f"{where}: epsilon {r['eps']!r}, restated {eps!r}"
    np.testing.assert_array_equal(r["explored"], explored, err_msg=where)
    np.testing.assert_array_equal(r["action"], want, err_msg=where)
    np.testing.assert_array_equal(r["host"], want, err_msg=where)
    assert torch.equal(r["mean"], mean), f"{where}: the means differ from prism_greedy_select's"
    assert int(r["action"].min()) >= 0 and int(r["action"].max()) < A
    return explored


# (T, heads): the q path with 1 and 10 heads, the z path staged in LDS (T * A <= 12288 floats)
PATHS = [(0, 1), (0, 10), (8, 0), (200, 0)]


@pytest.mark.parametrize("n", [1, 3, 17, 64])
@pytest.mark.parametrize("A", [1, 3, 6, 16])
def test_direct_calls_equal_the_restatement(dev, n, A):
    rng = np.random.default_rng(100 * n + A)
    for T, heads in PATHS:
        z, qb, n_pad = _estimates(rng, n, T, A, heads, dev)
        assert n_pad == (n + 15) // 16 * 16
        greedy, mean = _greedy(z, qb, n, n_pad, T, A, heads)
        for anneal in ANNEALS:
            where = f"n={n} A={A} T={T} heads={heads} anneal={anneal}"
            explored = _check(_egreedy(z, qb, n, n_pad, T, A, heads, anneal), greedy, mean, A, anneal, where=where)
            if anneal[:3] in ((0.0, 0.0, 0), (1.0, 1.0, 0)):          # eps = 1 always explores, eps = 0 never
                assert explored.all() == (anneal[0] == 1.0) and explored.any() == (anneal[0] == 1.0)
            # given coins: 0, the largest double below 1, epsilon itself (strict "<": does not explore), random
            eps = R.anneal(anneal[0], anneal[1], anneal[2], anneal[3] + n)
            for coins in (np.zeros(n), np.full(n, 1.0 - 2.0 ** -53), np.full(n, eps), rng.random(n)):
                r = _egreedy(z, qb, n, n_pad, T, A, heads, anneal, u_in=coins)
                _check(r, greedy, mean, A, anneal, coins=coins, where=where + " given coins")
            # rows 3 .. 3 + n of a call of n + 5 rows: their own counters and coins, the epsilon of the WHOLE call
            n_call = n + 5
            _check(_egreedy(z, qb, n, n_pad, T, A, heads, anneal, row0=3, n_call=n_call), greedy, mean, A, anneal, row0=3,
                   n_call=n_call, where=where + " row0=3")
            coins = rng.random(n_call)
            _check(_egreedy(z, qb, n, n_pad, T, A, heads, anneal, row0=3, n_call=n_call, u_in=coins), greedy, mean, A, anneal,
                   row0=3, n_call=n_call, coins=coins, where=where + " row0=3, given coins")
    # mid-anneal, a random action is not the greedy one everywhere: both branches were seen across the shapes
    r = R.select(np.zeros(64, dtype=np.int64), SEED, MID[3], 0, 64, 6, *MID[:3])
    assert 0 < int(r[1].sum()) < 64


def test_unstaged_estimates_and_a_call_in_pieces(dev):
    """T * A = 16384 floats: beyond the LDS staging (read from global memory).  And rows k .. n of a call handed over as a
    piece of their own (row0 = k, the whole call's row count) equal the same rows of the call in one piece."""
    n, T, A = 17, 1024, 16
    rng = np.random.default_rng(5)
    z, _, n_pad = _estimates(rng, n, T, A, 0, dev)
    greedy, mean = _greedy(z, None, n, n_pad, T, A, 0)
    for anneal in ANNEALS:
        whole = _egreedy(z, None, n, n_pad, T, A, 0, anneal)
        _check(whole, greedy, mean, A, anneal, where=f"unstaged {anneal}")
        k = 6
        first = _egreedy(z[:k].contiguous(), None, k, 16, T, A, 0, anneal, row0=0, n_call=n)
        rest = _egreedy(z[k:].contiguous(), None, n - k, 16, T, A, 0, anneal, row0=k, n_call=n)
        for name in ("action", "explored"):
            np.testing.assert_array_equal(np.concatenate([first[name], rest[name]]), whole[name], err_msg=name)
        assert first["eps"] == rest["eps"] == whole["eps"]


@pytest.mark.parametrize("T,heads", [(0, 1), (0, 10), (8, 0), (200, 0)])
def test_greedy_equality_with_exact_ties(dev, T, heads):
    n, A = 64, 6
    rng = np.random.default_rng(T + heads)
    z, qb, n_pad = _estimates(rng, n, T, A, heads, dev, ties=True)
    greedy, mean = _greedy(z, qb, n, n_pad, T, A, heads)
    m = mean.numpy()
    tied = (m == m.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied.sum() >= 3, "the inputs must hold rows whose maximal mean is shared"
    np.testing.assert_array_equal(greedy, m.argmax(axis=1))                   # (numpy: the first maximum)
    never = _egreedy(z, qb, n, n_pad, T, A, heads, (0.0, 0.0, 0, 11))
    np.testing.assert_array_equal(never["action"], greedy)
    assert not never["explored"].any() and never["eps"] == 0.0 and torch.equal(never["mean"], mean)
    always = _egreedy(z, qb, n, n_pad, T, A, heads, (1.0, 1.0, 0, 11))
    assert always["explored"].all() and always["eps"] == 1.0
    np.testing.assert_array_equal(always["action"], R.draws(SEED, 11, 0, n, A)[1])
    assert (always["action"] != greedy).any()


def test_the_device_word_counts_the_rows(dev):
    from prism_amd.agents.hip_agent import graph_capture
    A, heads, T = 6, 10, 0
    start, stop, steps, base = 1.0, 0.1, 250, 1000
    rng = np.random.default_rng(9)
    word = torch.zeros(1, dtype=torch.int64, device=dev)
    seen = 0
    for n in (3, 17, 1, 64, 5, 64, 64, 64):          # (the last ones walk past the end of the anneal: base + word >= steps ...)
        z, qb, n_pad = _estimates(rng, n, T, A, heads, dev)
        greedy, mean = _greedy(z, qb, n, n_pad, T, A, heads)
        got = _egreedy(z, qb, n, n_pad, T, A, heads, (start, stop, steps + base, base), word=word)
        now = (start, stop, steps + base, base + seen)
        _check(got, greedy, mean, A, now, where=f"word at {seen}, n={n}")
        same = _egreedy(z, qb, n, n_pad, T, A, heads, now)          # the same call with the count handed over
        for name in ("action", "explored", "eps"):
            np.testing.assert_array_equal(got[name], same[name])
        seen += n
        assert int(word.item()) == seen, "the word after the call: the sum of the rows"
    assert got["eps"] == stop
    # captured once, replayed five times: every replay draws at the count the one before left
    n = 17
    z, qb, n_pad = _estimates(rng, n, T, A, heads, dev)
    greedy, mean = _greedy(z, qb, n, n_pad, T, A, heads)
    word.fill_(40)
    anneal = (start, stop, 200, 0)
    out = _egreedy(z, qb, n, n_pad, T, A, heads, anneal, word=word, sync=False)          # (warm-up: 40 -> 57)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        _egreedy(z, qb, n, n_pad, T, A, heads, anneal, word=word, sync=False, out=out)
    assert int(word.item()) == 57, "a capture only records"
    actions = []
    for i in range(5):
        g.replay()
        torch.cuda.synchronize()
        r = _host(out)
        _check(r, greedy, mean, A, (start, stop, 200, 57 + n * i), where=f"replay {i}")
        assert int(word.item()) == 57 + n * (i + 1)
        actions.append(r["action"])
    assert any((a != actions[0]).any() for a in actions[1:]), "replays draw fresh"


# ---------------------------------------------------------------------------------------------------------------------
# agent level
# ---------------------------------------------------------------------------------------------------------------------
BATCH, C, A6 = 32, 4, 6
EG = dict(use_e_greedy=True, e_greedy_decay_timesteps=150, e_greedy_final_epsilon=0.3)      # both coin sides happen
CONFIGS = {"dqn1": (0, {}), "iqn": (2, {})}          # the single-Linear DQN head | IQN, greedy on the quantile mean


def _agent(dev, kind, per_env=True, **over):
    from prism_amd.config import baseline_config
    from prism_amd.factory import agent_factory
    base, extra = CONFIGS[kind]
    cfg = baseline_config(base, device=dev, batch_size=BATCH, log_to_wandb=False, seed=SEED, **dict(EG, **extra, **over))
    if per_env is not None:
        cfg.e_greedy_per_env = per_env
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A6)
    return cfg, agent


def _obs(rng, n):
    return (rng.random((n, 10, 10, C)) < 0.15).astype(np.float32)


def _want(agent, x, s0, c0):
    """The restatement's actions of a call on observations ``x`` that started at ``s0`` rows seen and acting count ``c0``:
    the greedy actions are prism_greedy_select's on the estimates of the same forward, piece by piece as the agent runs it."""
    sel = agent.action_selector
    n, cap, keep = len(x), agent._act_cap, agent._act_draws
    if n <= cap:          # the estimates the call itself left behind
        z, qb, m, n_pad, T = agent._act_raw
        greedy = [_greedy(z, qb, m, n_pad, T, A6, agent.dims.n_heads)[0]]
    else:                 # (nobody keeps those of a call in pieces: the same forwards again, at the same counts)
        agent._act_draws = c0
        greedy = []
        for i in range(0, n, cap):
            agent.act_estimates(x[i:i + cap])
            z, qb, m, n_pad, T = agent._act_raw
            greedy.append(_greedy(z, qb, m, n_pad, T, A6, agent.dims.n_heads)[0])
        assert agent._act_draws == keep
    e = sel.epsilon
    return R.select(np.concatenate(greedy), agent.seed, s0, 0, n, A6, e.start, e.stop, e.max_steps)


@pytest.mark.parametrize("kind", ["dqn1", "iqn"])
def test_agent_forward_returns_the_restatements_actions(dev, kind):
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    cfg, agent = _agent(dev, kind)
    sel = agent.action_selector
    assert type(sel) is EGreedyActionSelector and agent.e_greedy_per_env and agent.act_graph and agent.tau_rng == "philox"
    assert agent._selector_key(sel) == ("egreedy", 1.0, 0.3, 150)
    assert agent._selector_key(agent.eval_action_selector) == ("greedy",)
    T = agent._act_T()
    assert T == (200 if kind == "iqn" else 0)
    rng = np.random.default_rng(4)
    host_rng = sel.rng.get_state()
    dev_buf = {n: torch.zeros((n, 10, 10, C), device=dev) for n in (1, 5)}          # (one inference buffer per shape)
    calls, explored_rows = [], 0

    def call(n, graph, on_device, where):
        nonlocal explored_rows
        agent.act_graph = graph
        s0, c0 = sel.epsilon.current_step, agent._act_draws
        x = _obs(rng, n)
        if on_device:
            dev_buf[n].copy_(torch.from_numpy(x))
        a = agent.forward(dev_buf[n] if on_device else x)
        torch.cuda.synchronize()
        agent.act_graph = True
        assert (type(a).__name__ == "_Actions") == graph, f"{where}: graph path expected {graph}"
        got = a.cpu().numpy().copy()
        assert sel.epsilon.current_step == s0 + n, f"{where}: epsilon.current_step counts the rows seen"
        assert agent._act_draws == c0 + n * T, f"{where}: the selector must not move the acting count"
        if graph:
            assert int(agent._eg_word.item()) == s0 + n, f"{where}: the device's count of rows"
        state = sel.rng.get_state()
        assert state[0] == host_rng[0] and np.array_equal(state[1], host_rng[1]) and state[2:] == host_rng[2:], where
        want, explored, _ = _want(agent, x, s0, c0)
        np.testing.assert_array_equal(got, want, err_msg=f"{where} at {s0} rows seen")
        explored_rows += int(explored.sum())
        calls.append((n, graph, on_device, agent._act_draws))
        return got

    for n in (1, 5):
        for on_device in (False, True):
            for i in range(3):          # first call of a shape: eager launches on the device word; second: capture; then replays
                call(n, True, on_device, f"n={n} dev={on_device} graph call {i}")
            call(n, False, on_device, f"n={n} dev={on_device} eager in between")
            call(n, True, on_device, f"n={n} dev={on_device} replay after an eager call")
    assert any(k[1][0] == "egreedy" and s["g"] is not None for k, s in agent._act_graphs.items()), "graphs were captured"
    # interleaved with learner steps: other parameters, the counts go on
    for step in range(2):
        batch, w, _ = H.random_batch(np.random.default_rng(step), BATCH, C, A6, cfg)
        agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
        for n in (5, 1):
            call(n, True, False, f"n={n} after update {step}")
            call(n, False, True, f"n={n} eager after update {step}")
    # more observations than the workspace takes: pieces of ONE call (one epsilon, one range of counters)
    cap = agent._act_cap
    assert cap == BATCH
    s0, c0 = sel.epsilon.current_step, agent._act_draws
    x = _obs(rng, cap + 7)
    got = agent.forward(x).cpu().numpy().copy()
    assert sel.epsilon.current_step == s0 + cap + 7 and agent._act_draws == c0 + (cap + 7) * T
    want, explored, eps = _want(agent, x, s0, c0)
    np.testing.assert_array_equal(got, want)
    assert eps == R.anneal(1.0, 0.3, 150, s0 + cap + 7)
    calls.append((cap + 7, True, False, agent._act_draws))
    call(5, True, False, "n=5 after the call in pieces")
    rows = sel.epsilon.current_step
    assert 0 < explored_rows + int(explored.sum()) < rows, "both sides of the coin were seen"
    # the acting quantile count: what the same calls give with a greedy selector
    _, twin = _agent(dev, kind, use_e_greedy=False)
    assert agent._selector_key(twin.action_selector) == ("greedy",)
    for n, graph, on_device, draws in calls:
        twin.act_graph = graph
        x = _obs(rng, n)
        twin.forward(torch.from_numpy(x).to(dev) if on_device else x)
        assert twin._act_draws == draws
    torch.cuda.synchronize()


def test_parity_mode_selects_on_the_eager_path(dev):
    """``tau_rng == "torch"``: the quantile samples are torch's, so no graph; the selector kernel runs all the same, at the
    count the host hands over, and the device word is not involved."""
    cfg, agent = _agent(dev, "iqn", tau_rng="torch")
    sel = agent.action_selector
    assert agent._selector_key(sel) == ("egreedy", 1.0, 0.3, 150)
    rng = np.random.default_rng(6)
    for n in (5, 1, 5, BATCH + 7):
        s0 = sel.epsilon.current_step
        x = _obs(rng, n)
        torch.manual_seed(1000 + s0)
        a = agent.forward(x)
        assert type(a).__name__ != "_Actions" and sel.epsilon.current_step == s0 + n and agent._eg_dev_steps is None
        got = a.cpu().numpy().copy()
        if n <= agent._act_cap:
            want = _want(agent, x, s0, None)[0]
        else:          # (the same torch samples again, piece by piece)
            torch.manual_seed(1000 + s0)
            greedy = []
            for i in range(0, n, agent._act_cap):
                agent.act_estimates(x[i:i + agent._act_cap])
                z, qb, m, n_pad, T = agent._act_raw
                greedy.append(_greedy(z, qb, m, n_pad, T, A6, 0)[0])
            want = R.select(np.concatenate(greedy), agent.seed, s0, 0, n, A6, 1.0, 0.3, 150)[0]
        np.testing.assert_array_equal(got, want, err_msg=f"n={n} at {s0} rows seen")


def _run(agent, rng, sizes, update_every=None, cfg=None):
    out = []
    for i, n in enumerate(sizes):
        out.append(agent.forward(_obs(rng, n)).cpu().numpy().copy())
        if update_every and (i + 1) % update_every == 0:
            batch, w, _ = H.random_batch(np.random.default_rng(i), BATCH, C, A6, cfg)
            agent.update(to_hip_batch(batch, agent.device), per_weights=w.to(agent.device))
    return out


SIZES = [5, 5, 1, 5, 5, 5, 1, 5]


@pytest.mark.parametrize("kind,how", [("iqn", "save_state"), ("dqn1", "save_state"), ("dqn1", "save")])
def test_resume_continues_with_identical_actions(dev, tmp_path, kind, how):
    """``save_state`` / ``load_state`` (every stream position) and, for the model without quantile draws, a plain
    ``save`` / ``load`` checkpoint: ``state.pkl`` carries ``epsilon.current_step``, the device's count follows it."""
    cfg, agent = _agent(dev, kind)
    rng = np.random.default_rng(21)
    _run(agent, rng, SIZES, update_every=3, cfg=cfg)
    getattr(agent, how)(str(tmp_path))
    rows = agent.action_selector.epsilon.current_step
    assert rows == sum(SIZES)
    rng_state = rng.bit_generator.state
    want = _run(agent, rng, SIZES)
    _, fresh = _agent(dev, kind)
    _run(fresh, np.random.default_rng(1), [5, 5, 1])          # (graphs captured, the device word somewhere else)
    (fresh.load_state if how == "save_state" else fresh.load)(str(tmp_path))
    assert fresh.action_selector.epsilon.current_step == rows and fresh._eg_dev_steps is None
    rng.bit_generator.state = rng_state
    got = _run(fresh, rng, SIZES)
    for i, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(g, w, err_msg=f"call {i} after the resume")
    assert fresh.action_selector.epsilon.current_step == rows + sum(SIZES) == int(fresh._eg_word.item())


def _learn(dev, ckpt_dir, iterations=40):
    """``Learner.learn()`` in the mode over four lock-stepped toy environments: (actions of every step, final parameters,
    rows the selector saw)."""
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from tests.test_gpu_episodes import ToyEnvs
    n_env, first = 4, 64
    cfg = baseline_config(0, device=dev, batch_size=BATCH, experience_replay_capacity=1024, num_initial_random_timesteps=first,
                          timesteps_per_iteration=n_env, timestep_limit=first + n_env * iterations, timesteps_per_report=10 ** 6,
                          timesteps_between_evaluations=10 ** 6, target_update_period=40, checkpoint_dir=str(ckpt_dir),
                          log_to_wandb=False, seed=SEED, **EG)
    cfg.e_greedy_per_env = True
    envs, actions = ToyEnvs(n=n_env), []
    step = envs.step

    def logged_step(a):
        actions.append(torch.as_tensor(a).cpu().numpy().copy() if torch.is_tensor(a) else np.array(a))
        return step(a)
    envs.step = logged_step
    torch.manual_seed(11)
    col, ln = VectorCollector(envs, cfg), Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
        ln.learn()
    torch.cuda.synchronize()
    return actions, ln.agent.flat.cpu().clone(), ln.agent.action_selector.epsilon.current_step, ln.agent


def test_learn_with_a_vector_collector_is_reproducible(dev, tmp_path):
    iterations = 40
    a1, p1, rows1, agent = _learn(dev, tmp_path / "one", iterations)
    a2, p2, rows2, _ = _learn(dev, tmp_path / "two", iterations)
    assert rows1 == rows2 == 4 * iterations, "every row acted on is a row of the stream (the random first steps are not)"
    assert len(a1) == len(a2) == 16 + iterations
    for i, (x, y) in enumerate(zip(a1, a2)):
        np.testing.assert_array_equal(x, y, err_msg=f"step {i}")
    assert torch.equal(p1.view(torch.int32), p2.view(torch.int32)), "final parameters, bit for bit"
    assert type(agent.action_selector).__name__ == "EGreedyActionSelector"
    # per environment: within one step the rows do not all do the same thing
    acted = np.stack(a1[16:])
    assert acted.shape == (iterations, 4) and (acted != acted[:, :1]).any()


def test_knob_off_never_reaches_the_entry_point(dev, monkeypatch):
    from prism_amd import _native as N
    L = N.lib()
    real, reached = L.prism_egreedy_select, []

    def counted(*a):
        reached.append(1)
        return real(*a)
    monkeypatch.setattr(L, "prism_egreedy_select", counted)
    rng = np.random.default_rng(2)
    for per_env in (None, False):
        _, agent = _agent(dev, "dqn1", per_env=per_env)
        assert not agent.e_greedy_per_env
        sel, before = agent.action_selector, agent.action_selector.rng.get_state()[1].copy()
        for graph in (True, True, True, False):
            agent.act_graph = graph
            for n in (1, 5, BATCH + 7):
                agent.forward(_obs(rng, n))
        torch.cuda.synchronize()
        assert sel.epsilon.current_step == 4 * (6 + BATCH + 7)
        assert not np.array_equal(sel.rng.get_state()[1], before), "the host coin is tossed as before"
    assert not reached
    _, agent = _agent(dev, "dqn1", per_env=True)
    agent.forward(_obs(rng, 5))
    torch.cuda.synchronize()
    assert len(reached) == 1
