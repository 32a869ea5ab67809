"""GPU: risk-sensitive acting (``config.iqn_risk_policy_id``) -- ``prism_act_tau_distort`` against the host restatement
(tests/risk_ref.py), its device word under hipGraph replay, the acting forward behind it against ``prism_act_forward`` on the
same samples and the CPU oracle, the actions of ``Agent.forward`` in its three forms, the draw accounting against a neutral
twin, and ``learn()`` over device environments: captured against eager, resume, and neutral against the default.

Shapes: the kernel at n in {1, 3, 16, 17, 65} x n_tau in {1, 8, 32, 200} (a single lane, a partial wave, 65 x 32 = 9 and
65 x 200 = 51 workgroups of 256 lanes); the agent at the smallest model of the envelope, A = 6, C = 4, width 128, batch 16,
32 samples per action; the loop at the shapes of tests/resume_helpers.py (capacity 96, batch 16, N = 5)."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import resume_helpers as RH
from tests import risk_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-5                      # the tolerance tests/test_gpu_acting.py holds the neutral acting forward to
SEED, T_ACT, BATCH, C, A = 123, 32, 16, 4, 6
# Initial weights (torch.manual_seed before the model is built) and observations (numpy generator) of the action tests:
# searched once on the CPU with the oracle (seeds 0 .. 7): under seed 4 cvar:0.1 changes the greedy action of 20 of the 40
# observations, and the two best action means of every observation lie at least 6e-3 apart under both policies, far above
# the forward's tolerance.
WEIGHT_SEED, OBS_SEED = 4, 4
DEFAULT = object()
ETAS = {R.CVAR: (0.1, 0.25, 1.0), R.CPW: (0.1, 0.25, 1.0), R.WANG: (-2.0, -0.75, 0.75), R.POW: (-2.0, -0.75, 0.75)}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def risk_config(dev, pid=DEFAULT, **over):
    from prism_amd.config import baseline_config
    cfg = baseline_config(2, device=dev, batch_size=BATCH, iqn_quantile_samples_per_action=T_ACT, seed=SEED, **over)
    if pid is not DEFAULT:
        cfg.iqn_risk_policy_id = pid
    return cfg


def make_agent(dev, pid=DEFAULT, attrs=None, **over):
    from prism_amd.factory import agent_factory
    cfg = risk_config(dev, pid, **over)
    for k, v in (attrs or {}).items():
        setattr(cfg, k, v)
    torch.manual_seed(WEIGHT_SEED)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A)
    return cfg, agent


def observations(n, seed=OBS_SEED):
    return (np.random.default_rng(seed).random((n, 10, 10, C)) < 0.15).astype(np.float32)


def piece_taus(seed, offset, T, n, cap):
    """The raw samples ``Agent.forward`` draws for n observations from draw count ``offset``, piece by piece (``cap``
    observations a piece, each tau-major over its own rows): [(first row, rows, float32[T * rows])]."""
    out = []
    for i in range(0, n, cap):
        m = min(cap, n - i)
        out.append((i, m, R.raw_taus(seed, offset + i * T, T, m)))
    return out


def greedy_actions(dist):
    """``prism_greedy_select`` on quantile values ``dist`` (T, n, A), restated: the float32 sum in sample order, divided by
    T, the first maximum."""
    d = np.asarray(dist, dtype=np.float32)
    s = np.zeros(d.shape[1:], dtype=np.float32)
    for t in range(d.shape[0]):
        s = s + d[t]
    return np.argmax(s / np.float32(d.shape[0]), axis=1)


def _distort(N, n, T, policy, eta, raw=None, seed=SEED, offset=0, word=None, want_raw=True):
    dev = "cuda:0"
    out = torch.full((n * T,), -1.0, device=dev)
    out_raw = torch.full((n * T,), -1.0, device=dev) if want_raw else None
    N.check(N.lib().prism_act_tau_distort(n, T, policy, eta, N.ptr(raw), seed, offset, N.ptr(word), N.ptr(out), N.ptr(out_raw),
                                          N.current_stream_handle()), "prism_act_tau_distort")
    return out, out_raw


# ---------------------------------------------------------------------------------------------- 1. kernel against restatement
@pytest.mark.parametrize("policy", [R.CVAR, R.WANG, R.CPW, R.POW])
def test_kernel_against_the_restatement(dev, policy):
    from prism_amd import _native as N
    worst = 0
    for n in (1, 3, 16, 17, 65):
        for T in (1, 8, 32, 200):
            offset = 1000 * n + T
            raw = R.raw_taus(SEED, offset, T, n)
            for eta in ETAS[policy]:
                out, out_raw = _distort(N, n, T, policy, eta, offset=offset)
                got, got_raw = out.cpu().numpy(), out_raw.cpu().numpy()
                np.testing.assert_array_equal(got_raw.view(np.uint32), raw.view(np.uint32))
                d = int(R.ulp_distance(got, R.beta(policy, eta, raw)).max())
                worst = max(worst, d)
                assert d <= (0 if policy == R.CVAR else 1), (n, T, eta, d)
                assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    print(f"policy {policy}: largest distance from the restatement {worst} float32 ulp")
    # explicit raw samples, the ends of the range among them: into [0, 1], 0 to 0; the word is left alone
    ends = np.float32([0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24])
    word = torch.tensor([0, 0, 77], dtype=torch.int64, device=dev)
    for eta in ETAS[policy]:
        out, out_raw = _distort(N, 4, 1, policy, eta, raw=torch.from_numpy(ends).to(dev), word=word)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(out_raw.cpu().numpy(), ends)
        assert got[0] == 0.0 and float(got.min()) >= 0.0 and float(got.max()) <= 1.0, (eta, got)
        assert int(R.ulp_distance(got, R.beta(policy, eta, ends)).max()) <= (0 if policy == R.CVAR else 1)
    assert word.cpu().tolist() == [0, 0, 77]
    # PRISM_RISK_NEUTRAL copies
    out, out_raw = _distort(N, 17, 8, R.NEUTRAL, 0.0, offset=5)
    assert torch.equal(out, out_raw) and np.array_equal(out.cpu().numpy(), R.raw_taus(SEED, 5, 8, 17))


# ---------------------------------------------------------------------------------------------- 2. the device word
@pytest.mark.parametrize("n,T", [(65, 32), (1, 8)])
def test_device_word_under_graph_replay(dev, n, T):
    """One launch with the word bound, captured and replayed 50 times: replay r draws the counters [r n T, (r + 1) n T) and
    leaves the plain count (r + 1) n T; a ``prism_act_forward`` that draws for itself goes on from there."""
    from prism_amd import _native as N
    from prism_amd.agents.hip_agent import graph_capture
    word = torch.zeros(3, dtype=torch.int64, device=dev)
    out = torch.empty(n * T, device=dev)
    out_raw = torch.empty(n * T, device=dev)

    def launch():
        N.check(N.lib().prism_act_tau_distort(n, T, R.WANG, -0.75, None, SEED, 0, N.ptr(word), N.ptr(out), N.ptr(out_raw),
                                              N.current_stream_handle()), "prism_act_tau_distort")
    launch()                                      # (eager once: the library is warm before the capture)
    torch.cuda.synchronize()
    assert word.cpu().tolist() == [0, 0, n * T]
    word.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        launch()
    for r in range(50):
        g.replay()
        raw = out_raw.cpu().numpy()
        want = R.raw_taus(SEED, r * n * T, T, n)
        assert np.array_equal(raw.view(np.uint32), want.view(np.uint32)), f"replay {r}"
        assert int(R.ulp_distance(out.cpu().numpy(), R.beta(R.WANG, -0.75, want)).max()) <= 1
        assert word.cpu().tolist() == [0, 0, (r + 1) * n * T], f"replay {r}"
    # an evaluation's count (2^62 + c): the word's two top bits belong to the count
    base = 2 ** 62 + 12345
    word[2] = base
    g.replay()
    assert np.array_equal(out_raw.cpu().numpy(), R.raw_taus(SEED, base, T, n))
    assert int(word[2].item()) == base + n * T
    # a neutral acting forward behind it on the same word draws at the count the launch left
    word[2] = 50 * n * T
    cfg, agent = make_agent(dev)
    agent._prepare(BATCH)
    obs = torch.from_numpy(observations(4)).to(dev)
    z, _, _, _ = agent._act_buffers(4)
    z2 = torch.empty_like(z)
    count = 51 * n * T
    with torch.cuda.device(agent.device):
        g.replay()
        agent._act_launch(obs, 4, T_ACT, None, 0, z, None, rng_counters=word.data_ptr(), act_flags=0)
        taus = torch.from_numpy(R.raw_taus(SEED, count, T_ACT, 4)).to(dev)
        agent._act_launch(obs, 4, T_ACT, taus, 0, z2, None, rng_counters=None, act_flags=0)
    torch.cuda.synchronize()
    assert torch.equal(z[:4 * T_ACT], z2[:4 * T_ACT])
    assert int(word[2].item()) == count + 4 * T_ACT


# ---------------------------------------------------------------------------------------------- 3. forward equivalence
@pytest.mark.parametrize("pid", ["cvar:0.25", "wang:-0.75", "cpw:0.71", "pow:-2"])
def test_forward_equals_act_forward_on_the_distorted_samples(dev, pid):
    from oracle.learner_ref import act_forward
    from prism_amd import _native as N
    from prism_amd.agents import risk_policies
    cfg, agent = make_agent(dev, pid)
    policy, eta = risk_policies.parse(pid)
    n, offset = BATCH, 4242
    obs = torch.from_numpy(observations(n)).to(dev)
    agent._act_draws = offset
    q, dist = agent.act_estimates(obs)
    assert agent._act_draws == offset + n * T_ACT
    # the buffer the kernel writes for this pass, and prism_act_forward on it
    buf, raw = _distort(N, n, T_ACT, policy, eta, offset=offset)
    assert np.array_equal(raw.cpu().numpy(), R.raw_taus(SEED, offset, T_ACT, n))
    z2 = torch.empty((n * T_ACT, A), device=dev)
    d = agent._desc
    keep = d.rng_counters, d.act_flags
    d.rng_counters, d.act_flags = None, 0
    try:
        N.check(N.lib().prism_act_forward(ctypes.byref(d), N.ptr(obs), n, T_ACT, N.ptr(buf), SEED, 0, N.ptr(z2), None,
                                          N.current_stream_handle()), "prism_act_forward")
    finally:
        d.rng_counters, d.act_flags = keep
    torch.cuda.synchronize()
    dist2 = z2.view(n, T_ACT, A).permute(1, 0, 2)
    assert torch.equal(dist, dist2)
    sd = {k: v.cpu() for k, v in agent.model.state_dict().items()}
    qo, do = act_forward(sd, H.spec_from_config(risk_config("cpu", pid), C=C, A=A), obs.cpu(), buf.cpu().view(-1, 1))
    err = float((dist.cpu() - do).abs().max())
    print(f"{pid}: largest distance of z from the oracle {err:.3g}")
    np.testing.assert_allclose(dist.cpu().numpy(), do.numpy(), rtol=0, atol=TOL)
    np.testing.assert_allclose(q.cpu().numpy(), qo.numpy(), rtol=0, atol=TOL)
    # explicit samples are the raw ones: Z at beta of them
    given = torch.from_numpy(R.raw_taus(SEED, offset, T_ACT, n)).view(-1, 1)
    draws = agent._act_draws
    q3, dist3 = agent.act_estimates(obs, taus=given.to(dev))
    assert torch.equal(dist3, dist) and agent._act_draws == draws + n * T_ACT


# ---------------------------------------------------------------------------------------------- 4. actions
def _forms(agent, obs, offset):
    """``Agent.forward`` on ``obs`` from draw count ``offset``, eagerly and (where one pass takes them) from the hipGraph --
    twice, so that the second call is a replay -- and the device's own estimates at the same counters."""
    n, out = obs.shape[0], {}
    agent.act_graph = False
    agent._act_draws = offset
    out["eager"] = agent.forward(obs).cpu().numpy()
    assert agent._act_draws == offset + n * T_ACT
    if n <= BATCH:
        agent.act_graph = True
        for call in ("graph, eager first call", "graph, capture and replay", "graph, replay"):
            agent._act_draws = offset
            out[call] = agent.forward(obs).cpu().numpy()
        assert any(st["g"] is not None for st in agent._act_graphs.values())
        assert int(agent.rng_counters[2].item()) == offset + n * T_ACT == agent._act_draws
    agent._act_draws = offset
    _, dist = agent.act_estimates(torch.from_numpy(obs).to(agent.device))
    return out, dist.cpu().numpy()


@pytest.mark.parametrize("pid", ["cvar:0.25", "wang:-0.75"])
def test_actions_are_the_argmax_of_the_device_estimates(dev, pid):
    cfg, agent = make_agent(dev, pid)
    obs = observations(40)
    for rows in (obs[:BATCH], obs[:5], obs):          # one pass (graph and eager), and 40 > 16 in pieces
        forms, dist = _forms(agent, rows, 900)
        want = greedy_actions(dist)
        for name, act in forms.items():
            np.testing.assert_array_equal(act, want, err_msg=f"{pid}, {len(rows)} observations, {name}")
    assert agent._selector_key(agent.action_selector) == ("greedy", ("risk",) + agent.risk)


def test_cvar_changes_actions_and_neutral_is_the_default(dev):
    obs = observations(40)
    acts = {}
    for pid in (DEFAULT, "neutral", None, "cvar:0.1"):
        cfg, agent = make_agent(dev, pid)
        forms, dist = _forms(agent, obs, 900)
        acts[pid] = forms["eager"]
        np.testing.assert_array_equal(acts[pid], greedy_actions(dist))
        forms16, _ = _forms(agent, obs[:BATCH], 900)
        for name, act in forms16.items():          # (the first piece of the 40 draws what the pass of 16 draws)
            np.testing.assert_array_equal(act, acts[pid][:BATCH], err_msg=name)
        if pid != "cvar:0.1":
            assert agent._selector_key(agent.action_selector) == ("greedy",) and not agent._risk_on
            assert "risk_policy" not in agent._compat_record()
            assert all(st["rtau"] is None for st in agent._act_graphs.values())
    np.testing.assert_array_equal(acts["neutral"], acts[DEFAULT])
    np.testing.assert_array_equal(acts[None], acts[DEFAULT])
    differ = int((acts["cvar:0.1"] != acts[DEFAULT]).sum())
    print(f"cvar:0.1 chooses another action than neutral for {differ} of 40 observations")
    assert differ >= 1


# ---------------------------------------------------------------------------------------------- 5. accounting
def test_accounting_equals_a_neutral_twin(dev):
    EG = dict(use_e_greedy=True, e_greedy_decay_timesteps=100, e_greedy_final_epsilon=0.3)
    agents = [make_agent(dev, pid, attrs=dict(e_greedy_per_env=True), **EG)[1] for pid in ("cvar:0.25", DEFAULT)]
    frames = [observations(5, seed=s) for s in range(10)]
    records = []
    for agent in agents:
        for f in frames:
            agent.forward(f)
        torch.cuda.synchronize()
        rec = [agent._act_draws, int(agent.rng_counters[2].item()), int(agent.action_selector.epsilon.current_step),
               int(agent._eg_word.item())]
        assert rec == [10 * 5 * T_ACT, 10 * 5 * T_ACT, 50, 50]
        # an evaluation inside acting_stream: the training count is where it was, the block's count is its own
        base = 2 ** 62 + 640
        agent.eval()
        with agent.acting_stream(base) as stream:
            for f in frames[:3]:
                agent.forward(f)
            assert int(agent.rng_counters[2].item()) == base + 3 * 5 * T_ACT
        agent.train()
        assert stream.count == base + 3 * 5 * T_ACT and agent._act_draws == rec[0]
        agent.forward(frames[0])
        rec += [agent._act_draws, int(agent.rng_counters[2].item()), int(agent.action_selector.epsilon.current_step)]
        assert rec[4:] == [11 * 5 * T_ACT, 11 * 5 * T_ACT, 55]
        records.append(rec)
    assert records[0] == records[1]
    # a count the word's form cannot hold is refused on the host, before a launch
    risk = agents[0]
    with risk.acting_stream(2 ** 50):
        with pytest.raises(ValueError, match="2\\^42"):
            risk.forward(frames[0])


# ---------------------------------------------------------------------------------------------- 6. the loop
RISK = dict(iqn_risk_policy_id="cvar:0.25")
NAME, TPI, PAST_FILL = "iqn_per_egreedy", 5, 30


def test_learn_captured_equals_eager(dev, tmp_path):
    from tests import test_gpu_captured_loop as L
    limit, total = L._limit(NAME, TPI, PAST_FILL)
    states = {}
    for knob in (True, False):
        ln, col = L._learner(dev, tmp_path / str(knob), NAME, TPI, knob, limit, **RISK)
        assert ln.agent.risk == (R.CVAR, 0.25)
        states[knob], eager = L._learn(ln, col)
        if knob:
            assert ln.captured_loop_refusal() is None and ln.captured_iterations == PAST_FILL - 1
            assert eager + ln.captured_iterations == total
        else:
            assert ln.captured_iterations == 0 and eager == total
    RH.assert_same(states[True], states[False], "cvar:0.25, the captured loop against the eager loop")


def test_learn_resumes_bit_identically_and_refuses_another_policy(dev, tmp_path):
    from tests import test_gpu_captured_loop as L
    (cut, _), (limit, _) = L._limit(NAME, TPI, 12), L._limit(NAME, TPI, PAST_FILL)
    whole, col = L._learner(dev, tmp_path / "whole", NAME, TPI, True, limit, **RISK)
    want, _ = L._learn(whole, col)
    first, col = L._learner(dev, tmp_path / "cut", NAME, TPI, True, cut, backup_checkpoints=True, **RISK)
    L._learn(first, col)
    snap = first.checkpointer.latest_backup()
    assert snap is not None
    from prism_amd.util import snapshot
    assert snapshot.read_manifest(snap)["compat"]["agent"]["risk_policy"] == "cvar:0.25"
    # a neutral agent and one under another policy refuse the snapshot before anything is touched
    for other in ({}, dict(iqn_risk_policy_id="cvar:0.5"), dict(iqn_risk_policy_id="wang:0.25")):
        ln, col = L._learner(dev, tmp_path / "other", NAME, TPI, True, cut, backup_checkpoints=True, **other)
        before = ln.agent.flat.clone()
        with pytest.raises(ValueError, match="risk_policy"):
            with contextlib.redirect_stdout(io.StringIO()):
                ln.load_state(snap)
        assert torch.equal(ln.agent.flat, before) and ln.cumulative_timesteps == 0
    ln, col = L._learner(dev, tmp_path / "cut", NAME, TPI, True, cut, backup_checkpoints=True, **RISK)
    with contextlib.redirect_stdout(io.StringIO()):
        ln.load_state(snap)
    ln.timestep_limit = limit
    got, _ = L._learn(ln, col)
    got, want = dict(got), dict(want)
    # (a fresh agent's PER and tau words start at 0 and the host offsets carry what came before: their sums are compared)
    got["rng_counters"], want["rng_counters"] = got["rng_counters"][2:], want["rng_counters"][2:]
    RH.assert_same(got, want, "cvar:0.25, resumed")


def test_learn_neutral_equals_the_default(dev, tmp_path):
    from tests import test_gpu_captured_loop as L
    from prism_amd.util import snapshot
    limit, total = L._limit(NAME, TPI, PAST_FILL)
    states, records = {}, {}
    for which, over in (("neutral", dict(iqn_risk_policy_id="neutral")), ("default", {})):
        ln, col = L._learner(dev, tmp_path / which, NAME, TPI, True, limit, backup_checkpoints=True, **over)
        states[which], _ = L._learn(ln, col)
        assert ln.captured_iterations == PAST_FILL - 1
        records[which] = snapshot.read_manifest(ln.checkpointer.latest_backup())["compat"]["agent"]
        assert "risk_policy" not in records[which]
    RH.assert_same(states["neutral"], states["default"], "iqn_risk_policy_id = 'neutral' against the attribute left alone")
    assert records["neutral"] == records["default"]
