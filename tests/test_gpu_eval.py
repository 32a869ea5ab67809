"""GPU: the evaluation path.  ``prism_eval_track`` against ``EvalHost`` (tests/eval_ref.py) bit for bit; ``EvalTracker``'s
input paths; ``VectorEvaluator`` over scripted environments against ``EvalHost``, the reference's fixture and a twin agent;
the isolation of the training draws; ``learn()`` with and without evaluations; ``CheckpointEvaluator``."""
import contextlib
import ctypes
import io
import os
import shutil

import numpy as np
import pytest
import torch

from tests import eval_ref as ER
from tests import helpers as H

pytestmark = pytest.mark.gpu

BIG = 10 ** 12          # a budget nothing here reaches
POOL = np.array([0.0, 1.0, -1.0, 0.5, -0.25, 3.0, -7.5, 0.1, -0.1, 1e-3, 1e6, -123456.0, 0.7, -2.59], np.float32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- 1, 2: the kernel
class Rig:
    """The arrays of one prism_eval_desc on the device, and the same evaluation in an EvalHost."""

    def __init__(self, dev, n_streams, budget, log_capacity=4096, tail=None):
        from prism_amd import _native as N
        self.N, self.lib, self.dev = N, N.lib(), dev
        self.host = ER.EvalHost(n_streams, budget, log_capacity)
        z = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=dev)
        self.t = dict(ep_return=z(n_streams, torch.float64), ep_length=z(n_streams, torch.int32),
                      log_return=z(log_capacity, torch.float64), log_length=z(log_capacity, torch.int32),
                      stats=z(4, torch.float64), counts=z(4, torch.int64))
        if tail is not None:                          # streams no call reaches: whatever they hold stays
            first, ret, length = tail
            self.t["ep_return"][first:], self.t["ep_length"][first:] = ret, length
            for i in range(first, n_streams):
                self.host.ep_return[i], self.host.ep_length[i] = ret, length
        self.host_counts = torch.zeros(2, dtype=torch.int64).pin_memory()
        d = N.EvalDesc(n_streams=n_streams, log_capacity=log_capacity, budget=budget)
        for k, v in self.t.items():
            setattr(d, k, v.data_ptr() if (log_capacity or not k.startswith("log_")) else None)
        d.host_counts = self.host_counts.data_ptr()
        self.d, self.log_capacity = d, log_capacity

    def call(self, reward, done, trunc):
        N = self.N
        r, dn, tr = (torch.as_tensor(np.ascontiguousarray(x, dt)).to(self.dev) for x, dt in
                     ((reward, np.float32), (done, np.uint8), (trunc, np.uint8)))
        N.check(self.lib.prism_eval_track(ctypes.byref(self.d), len(reward), N.ptr(r), N.ptr(dn), N.ptr(tr),
                                          N.current_stream_handle()), "prism_eval_track")
        self.host.track(reward, done, trunc)

    def device_arrays(self):
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in self.t.items()}
        for k in ("log_return", "log_length"):
            out[k] = out[k][:self.log_capacity]
        return out

    def check(self):
        got, want = self.device_arrays(), self.host.arrays()
        for k in want:
            bits = np.uint64 if want[k].dtype == np.float64 else want[k].dtype
            np.testing.assert_array_equal(got[k].view(bits), want[k].view(bits), err_msg=k)
        assert self.host_counts.tolist() == [self.host.counts[0], self.host.counts[2]]


def _ends(pattern, n, rng):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "last_lane":
        return i % 64 == 63
    if pattern == "second_pass_first_row":
        return i == 1024
    return rng.random(n) < 0.1


@pytest.mark.parametrize("pattern", ["none", "all", "last_lane", "second_pass_first_row", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 2049])
def test_kernel_equals_the_host_restatement(dev, n, pattern):
    """6 to 12 calls at n_streams = n; every array by its float64 / int64 bit pattern.  ("all" at 2049 rows ends more
    episodes than the log holds.)"""
    rng = np.random.default_rng([n, len(pattern)])
    rig = Rig(dev, n, BIG)
    calls = int(rng.integers(6, 13))
    for _ in range(calls):
        ends = _ends(pattern, n, rng)
        trunc = ends & (rng.random(n) < 0.4)
        done = ends & (~trunc | (rng.random(n) < 0.3))
        rig.call(POOL[rng.integers(0, len(POOL), n)], done, trunc)
    rig.check()
    assert rig.host.counts[2:] == [n * calls, calls]
    if pattern == "all":
        assert rig.host.counts[0] == n * calls
    if pattern == "none":
        assert rig.host.counts[0] == 0 and max(rig.host.ep_length) == calls


def test_fewer_rows_than_streams_leave_the_tail_untouched(dev):
    rng = np.random.default_rng(5)
    rig = Rig(dev, 100, BIG, tail=(37, 7.5, 3))
    for _ in range(8):
        ends = rng.random(37) < 0.2
        rig.call(POOL[rng.integers(0, len(POOL), 37)], ends, np.zeros(37, bool))
    rig.check()
    assert rig.host.ep_return[37:] == [7.5] * 63 and rig.host.ep_length[99] == 3 and rig.host.counts[0] > 5


@pytest.mark.parametrize("log_capacity", [0, 5])
def test_seven_episodes_and_a_short_log(dev, log_capacity):
    """log_capacity 0 (no log arrays at all) and 5: the sums, extremes and counts still cover all seven."""
    rig = Rig(dev, 3, BIG, log_capacity)
    rng = np.random.default_rng(11)
    ends = [[1, 0, 0], [0, 1, 1], [0, 0, 0], [1, 1, 0], [0, 0, 1], [0, 0, 0], [0, 1, 0]]
    for e in ends:
        rig.call(POOL[rng.integers(0, len(POOL), 3)], np.array(e, bool), np.zeros(3, bool))
    rig.check()
    assert rig.host.counts[0] == 7 and len(rig.host.returns()) == log_capacity


# (streams, budget, call index whose rows hold the first episode end, calls made): the call after which it is closed
BUDGETS = [
    ("on_a_call_boundary", 4, 12, 1, 3),
    ("inside_a_call", 4, 10, 0, 3),
    ("when_the_first_episode_ends", 4, 4, 5, 6),
    ("budget_zero", 4, 0, 2, 3),
]


@pytest.mark.parametrize("name,n,budget,first_end,closes_after", BUDGETS)
def test_budgets_and_the_closed_evaluation(dev, name, n, budget, first_end, closes_after):
    """Up to the closing call the device follows the restatement; after it, three further calls with non-zero rewards and
    ends leave every array bit-identical, and host_counts (zeroed by the host in between) reports the counts again."""
    rng = np.random.default_rng(len(name))
    rig = Rig(dev, n, budget)
    for k in range(closes_after):
        assert not rig.host.closed()
        ends = np.zeros(n, bool)
        ends[k % n] = k >= first_end
        rig.call(POOL[rng.integers(1, len(POOL), n)], ends, np.zeros(n, bool))
    assert rig.host.closed() and rig.host.counts[2] == n * closes_after >= budget
    rig.check()
    before = rig.device_arrays()
    for _ in range(3):
        rig.host_counts.zero_()
        rig.call(POOL[rng.integers(1, len(POOL), n)], np.ones(n, bool), np.ones(n, bool))
        after = rig.device_arrays()
        for k in before:
            np.testing.assert_array_equal(after[k].view(np.uint8), before[k].view(np.uint8), err_msg=k)
        assert rig.host_counts.tolist() == [int(before["counts"][0]), int(before["counts"][2])]
    rig.check()


# ---------------------------------------------------------------------------------------------------- 3: EvalTracker
def _tracker_state(tr):
    torch.cuda.synchronize()
    return [t.cpu().clone() for t in (tr._words, tr._ep_return.view(torch.int64), tr._ep_length)]


def _tracker_script(n, calls, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(calls):
        ends = rng.random(n) < 0.15
        trunc = ends & (rng.random(n) < 0.5)
        out.append((POOL[rng.integers(0, len(POOL), n)], ends & ~trunc, trunc))
    return out


def test_tracker_input_paths(dev):
    """n = 65.  NumPy arrays, host tensors and device tensors, float32 / float64 rewards, bool / uint8 flags: one state,
    the restatement's; thirty host-array calls without a synchronisation in between equal the same calls made one by one
    (the pinned rotation)."""
    from prism_amd.evals import EvalTracker
    n, script = 65, _tracker_script(65, 30, 3)
    host = ER.EvalHost(n, BIG, 64)
    for r, d, t in script:
        host.track(r, d, t)

    def run(convert, sync):
        tr = EvalTracker(n, BIG, 64, dev)
        tr.reset()
        for k, (r, d, t) in enumerate(script):
            tr.track(*convert(k, r, d, t))
            if sync:
                torch.cuda.synchronize()
        return tr, _tracker_state(tr)

    as_numpy = lambda k, r, d, t: (r, d, t)
    on_device = lambda k, r, d, t: tuple(torch.as_tensor(x).to(dev) for x in (r, d, t))
    wide = lambda k, r, d, t: (r.astype(np.float64), d.astype(np.uint8), torch.as_tensor(t))
    wide_dev = lambda k, r, d, t: (torch.as_tensor(r.astype(np.float64)).to(dev), torch.as_tensor(d.astype(np.uint8)).to(dev), t)
    mixed = lambda k, r, d, t: (r, torch.as_tensor(d).to(dev), t) if k % 2 else (torch.as_tensor(r), d, torch.as_tensor(t).to(dev))
    tr0, want = run(as_numpy, sync=True)
    for convert in (as_numpy, on_device, wide, wide_dev, mixed):
        _, got = run(convert, sync=False)
        for g, w in zip(got, want):
            assert torch.equal(g, w), convert
    res = tr0.result()
    assert res == host.result() and res["episodes"] > 64 == len(res["returns"])          # std from the two sums here
    assert tr0.closed() is False
    np.testing.assert_array_equal(want[0][:8].numpy(), np.concatenate([ER.bits64(host.stats).view(np.int64), host.counts]))
    short = EvalTracker(n, 65 * 3, 4096, dev)
    for r, d, t in script[:3]:
        short.track(r, d, t)
    assert short.closed() is True and short.result()["timesteps"] == 65 * 3
    assert short.result()["std"] == float(np.std(short.result()["returns"]))
    short.track(*script[3])
    assert short.result()["timesteps"] == 65 * 3
    short.reset()
    assert short.closed() is False and short.result()["episodes"] == 0 and short.result()["mean"] is None
    with pytest.raises(ValueError, match="rows"):
        short.track(np.zeros(66, np.float32), np.zeros(66, bool), np.zeros(66, bool))


# ---------------------------------------------------------------------------------------------------- agents
SEED, BATCH, C, A = 31, 32, 4, 6


def _agent(dev, base=2, **over):
    from prism_amd.config import baseline_config
    from prism_amd.factory import agent_factory
    knobs = {k: over.pop(k) for k in ("act_graph",) if k in over}
    cfg = baseline_config(base, device=dev, batch_size=BATCH, log_to_wandb=False, seed=SEED, **over)
    for k, v in knobs.items():
        setattr(cfg, k, v)
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A)
    gen = torch.Generator().manual_seed(5)          # away from the initialisation: actions that depend on the draws
    agent.model.load_state_dict({k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen)
                                 for k, v in agent.model.state_dict().items()})
    agent._params_replaced()
    return cfg, agent


def _script(n, steps, seed, p_end=0.12):
    rng = np.random.default_rng(seed)
    kind = np.where(rng.random((steps, n)) < p_end, rng.integers(1, 4, (steps, n)), 0).astype(np.uint8)
    return POOL[rng.integers(0, len(POOL), (steps, n))].astype(np.float64), kind


def _host_run(reward, kind, horizon, start=0):
    host = ER.EvalHost(reward.shape[1], horizon)
    return host, ER.run_script(host, reward[start:], kind[start:])


@pytest.mark.parametrize("n", [1, 5, 17])
def test_vector_evaluator_equals_the_restatement_and_a_twin_agent(dev, n):
    from prism_amd.evals import EVAL_DRAW_BASE, VectorEvaluator
    if n == 1:
        run = ER.fixture_runs()["done_and_truncated"]
        reward, kind, horizon = run["reward"][:, None], run["kind"][:, None], run["horizon"]
    else:
        (reward, kind), horizon = _script(n, 60, n), 103          # (not a multiple of either N)
    host, steps = _host_run(reward, kind, horizon)
    _, agent = _agent(dev)
    envs = ER.ScriptedEnvs(reward, kind, device=dev if n == 5 else None)
    ev = VectorEvaluator(agent, envs, 0, horizon)
    returns = ev.evaluate_agent()
    np.testing.assert_array_equal(ER.bits64(returns), ER.bits64(host.returns()))
    assert ev.last == host.result() and ev.last["timesteps"] == steps * n == envs.k * n and envs.resets == 1
    if n == 1:
        np.testing.assert_array_equal(ER.bits64(returns), run["ep_rews_bits"])
        assert ev.last["timesteps"] == run["timesteps"]
    T = agent._act_T()
    assert not agent._is_eval and agent.model.training and agent._act_draws == 0 and ev.eval_draws == steps * n * T > 0
    # the twin: same seed and parameters, eval() + forward on the same observations at the evaluation's draw counts
    _, twin = _agent(dev)
    twin.eval()
    with twin.acting_stream(EVAL_DRAW_BASE) as reached:
        want = [twin.forward(envs._frames[k % 16]).cpu().numpy().copy() for k in range(steps)]
    twin.train()
    assert reached.count == EVAL_DRAW_BASE + ev.eval_draws and twin._act_draws == 0
    np.testing.assert_array_equal(np.stack(envs.actions), np.stack(want))
    # an environment that raises: the agent is back in train mode and its own draw count is where it was
    bad = VectorEvaluator(agent, ER.ScriptedEnvs(reward, kind, fail_at=3), 0, horizon)
    with pytest.raises(RuntimeError, match="scripted failure"):
        bad.evaluate_agent()
    assert not agent._is_eval and agent.model.training and agent._act_draws == 0 and bad.eval_draws == 4 * n * T


# ---------------------------------------------------------------------------------------------------- 5: isolation
ISOLATION = {"iqn_graph": dict(base=2), "iqn_eager": dict(base=2, act_graph=False),
             "ids_sampled": dict(base=3, ids_use_random_samples=True)}


@pytest.mark.parametrize("case", sorted(ISOLATION))
def test_an_evaluation_does_not_move_the_training_draws(dev, case):
    """X: 5 forwards, an evaluation of 40 steps, 5 forwards.  Y: 10 forwards.  Same actions, same acting draw counts.  A
    second evaluation goes on at the first one's count."""
    from prism_amd.evals import EVAL_DRAW_BASE, VectorEvaluator
    over = dict(ISOLATION[case])
    base = over.pop("base")
    (_, x), (_, y) = _agent(dev, base, **over), _agent(dev, base, **over)
    rng = np.random.default_rng(9)
    obs = [(rng.random((4, 10, 10, C)) < 0.15).astype(np.float32) for _ in range(10)]
    n, steps = 3, 40
    reward = POOL[rng.integers(0, len(POOL), (steps + 5, n))].astype(np.float64)
    kind = np.zeros((steps + 5, n), np.uint8)
    kind[steps - 1, 1] = 1                                     # the first episode ends at step 40: horizon 40 * 3 or less
    envs = ER.ScriptedEnvs(reward, kind)
    ev = VectorEvaluator(x, envs, 0, 100)
    offsets, real = [], x.acting_stream
    x.acting_stream = lambda offset: (offsets.append(offset), real(offset))[1]
    got = [x.forward(o).cpu().numpy().copy() for o in obs[:5]]
    ev.evaluate_agent()
    first = [a.copy() for a in envs.actions]
    assert envs.k == steps and ev.last["episodes"] == 1 and ev.last["timesteps"] == steps * n
    got += [x.forward(o).cpu().numpy().copy() for o in obs[5:]]
    want = [y.forward(o).cpu().numpy().copy() for o in obs]
    np.testing.assert_array_equal(np.stack(got), np.stack(want))
    T = x._act_T()
    assert x._act_draws == y._act_draws == 10 * 4 * T and ev.eval_draws == steps * n * T
    if x.act_graph:
        torch.cuda.synchronize()
        assert int(x.rng_counters[2].item()) == int(y.rng_counters[2].item()) == x._act_draws
    ev.evaluate_agent()
    assert offsets == [EVAL_DRAW_BASE, EVAL_DRAW_BASE + steps * n * T] and ev.eval_draws == 2 * steps * n * T
    assert x._act_draws == y._act_draws and ev.evaluations == 2
    _, z = _agent(dev, base, **over)                            # the second evaluation's actions: those at the continued count
    z.eval()
    with z.acting_stream(offsets[1]):
        again = [z.forward(envs._frames[k % 16]).cpu().numpy().copy() for k in range(steps)]
    np.testing.assert_array_equal(np.stack(envs.actions), np.stack(again))
    assert len(first) == steps


# ---------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_come_before_any_launch(dev):
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    from prism_amd.evals import VectorEvaluator
    reward, kind = _script(2, 8, 1)
    envs = ER.ScriptedEnvs(reward, kind)
    _, agent = _agent(dev, tau_rng="torch")
    with pytest.raises(ValueError, match="tau_rng"):
        VectorEvaluator(agent, envs, 0, 4)
    _, agent = _agent(dev)
    ev = VectorEvaluator(agent, envs, 0, 4)
    agent.eval_action_selector = EGreedyActionSelector(1.0, 0.1, 100, 0)          # (what a loaded checkpoint may bring)
    with pytest.raises(ValueError, match="EGreedyActionSelector"):
        ev.evaluate_agent()
    with pytest.raises(ValueError, match="EGreedyActionSelector"):
        VectorEvaluator(agent, envs, 0, 4)
    assert envs.resets == 0 and agent._B is None and not agent._is_eval and ev.tracker is None


# ---------------------------------------------------------------------------------------------------- 7: learn()
EVAL_N, EVAL_HORIZON, FIRST, ITER = 5, 60, 256, 8


class _RunningEnvs(ER.ScriptedEnvs):
    """Evaluation environments that go on through their script from one evaluation to the next."""

    def reset(self):
        self.resets += 1
        self.actions = []
        return self._obs()


def _learn(dev, ckpt_dir, iterations, evaluate, resume_from=None, raise_to=None):
    """learn() over ToyEnvs (tests/test_gpu_episodes.py) with a VectorCollector: (learner, environments, evaluation
    environments, [(cumulative timesteps, Eval Reward, Eval Episodes)], the full state before the buffer is emptied)."""
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from tests import resume_helpers as R
    from tests.test_gpu_episodes import ToyEnvs
    cfg = baseline_config(2, device=dev, batch_size=32, experience_replay_capacity=512, num_initial_random_timesteps=FIRST,
                          timesteps_per_iteration=ITER, timestep_limit=FIRST + ITER * iterations, timesteps_per_report=80,
                          timesteps_between_evaluations=200, evaluation_timestep_horizon=EVAL_HORIZON,
                          target_update_period=40, checkpoint_dir=str(ckpt_dir), log_to_wandb=False,
                          reward_clipping_type="dopamine_clamp", backup_checkpoints=True, seed=SEED)
    envs = ToyEnvs()
    eval_envs = _RunningEnvs(*_script(EVAL_N, 400, 77, p_end=0.15)) if evaluate else None
    col, ln, evals, state = VectorCollector(envs, cfg), Learner(), [], []
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col, eval_envs=eval_envs) if evaluate else ln.configure(cfg, collector=col)
        real, seen = ln.logger.log_data, {}

        def log_data(data, group_name, var_name, *a, **kw):
            if var_name == "Eval Reward":
                seen["reward"] = data
            if var_name == "Eval Episodes":
                evals.append((ln.cumulative_timesteps, seen.pop("reward"), data))
            return real(data, group_name, var_name, *a, **kw)
        ln.logger.log_data = log_data
        if resume_from is not None:
            envs.k, envs.cur = resume_from[0].k, resume_from[0].cur.copy()         # the environments' own business
            eval_envs.k = resume_from[1].k
            ln.load_state(ln.checkpointer.latest_backup())
            ln.timestep_limit = raise_to
        buf = ln.experience_buffer
        empty = buf.empty

        def capture():
            st = R.full_state(ln)
            st["episodes"] = {k: v for k, v in buf.episode_stats().items()}
            state.append(st)
            return empty()
        buf.empty = capture
        ln.learn()
    torch.cuda.synchronize()
    return ln, envs, eval_envs, evals, state[0]


@pytest.fixture(scope="module")
def eval_run(dev, tmp_path_factory):
    return _learn(dev, tmp_path_factory.mktemp("eval_run"), 60, True)


def test_learn_with_evaluations_computes_what_learn_without_them_computes(dev, eval_run, tmp_path):
    from tests import resume_helpers as R
    ln, envs, eval_envs, evals, state = eval_run
    plain, _, _, none, plain_state = _learn(dev, tmp_path, 60, False)
    assert plain.evaluator is None and none == [] and ln.evaluator is not None
    R.assert_same(state, plain_state)                          # parameters, optimizer, ring, trees, counters, episodes
    assert state["episodes"]["episodes"] > 10 and state["act_draws"] > 0
    # three evaluations, at the first iteration and then every 200 timesteps, with the restatement's values
    assert [e[0] for e in evals] == [FIRST + ITER, FIRST + ITER * 26, FIRST + ITER * 51]
    start, want = 0, []
    for _ in range(3):
        host, steps = _host_run(eval_envs.reward, eval_envs.kind, EVAL_HORIZON, start)
        want.append((host.result()["mean"], host.result()["episodes"]))
        start += steps
    assert [(e[1], e[2]) for e in evals] == want and eval_envs.k == start and eval_envs.closed
    assert ln.evaluator.evaluations == 3 and ln.evaluator.last == host.result()
    assert ln.evaluator.eval_draws == start * EVAL_N * ln.agent._act_T()


def test_learn_cut_after_the_second_evaluation_resumes_bit_identically(dev, eval_run, tmp_path):
    from tests import resume_helpers as R
    ln, _, eval_envs, evals, state = eval_run
    first, envs1, ev1, evals1, _ = _learn(dev, tmp_path, 30, True)
    assert len(evals1) == 2 and first.checkpointer.latest_backup() is not None
    second, _, ev2, evals2, state2 = _learn(dev, tmp_path, 30, True, resume_from=(envs1, ev1), raise_to=FIRST + ITER * 60)
    assert second.agent is not first.agent and second.cumulative_timesteps == FIRST + ITER * 60
    assert evals1 + evals2 == evals and len(evals2) == 1
    R.assert_same(state2, state)
    assert second.evaluator.state_dict() == ln.evaluator.state_dict()
    np.testing.assert_array_equal(ER.bits64(second.evaluator.last["returns"]), ER.bits64(ln.evaluator.last["returns"]))


def test_a_snapshot_without_an_evaluator_loads_into_a_learner_with_one_and_back(dev, tmp_path):
    """The ``learner`` part has the key only when there is an evaluator; load_state tolerates its absence."""
    from prism_amd.util import snapshot
    plain, envs1, _, _, _ = _learn(dev, tmp_path / "plain", 3, False)
    parts, _ = snapshot.read_snapshot(plain.checkpointer.latest_backup(), ["learner"])
    assert "evaluator" not in parts["learner"]
    shutil.copytree(tmp_path / "plain", tmp_path / "with")
    ln, _, _, evals, _ = _learn(dev, tmp_path / "with", 3, True, resume_from=(envs1, ER.ScriptedEnvs(*_script(EVAL_N, 4, 1))),
                                raise_to=FIRST + ITER * 5)
    assert len(evals) == 1 and ln.evaluator.evaluations == 1          # (since = inf: the first iteration evaluates)
    parts, _ = snapshot.read_snapshot(ln.checkpointer.latest_backup(), ["learner"])
    assert parts["learner"]["evaluator"]["evaluations"] == 1


# ---------------------------------------------------------------------------------------------------- 8: checkpoints
class _Log:
    def __init__(self):
        self.rows = []

    def log_data(self, data, group_name, var_name):
        self.rows.append((group_name, var_name, data))


def test_checkpoint_evaluator(dev, tmp_path, capsys):
    from prism_amd.evals import CheckpointEvaluator
    cfg, agent = _agent(dev, evaluation_timestep_horizon=50)
    flats = {}
    for ts in (300, 7000):
        agent.flat.mul_(1.01)
        agent._params_replaced()
        flats[ts] = agent.flat.cpu().clone()
        agent.save(str(tmp_path / f"agent_checkpoint_{ts}"))
    os.makedirs(tmp_path / "agent_checkpoint_9000" / "agent")                  # incomplete: nothing in it yet
    reward, kind = _script(5, 40, 21)
    envs, log = ER.ScriptedEnvs(reward, kind), _Log()
    ce = CheckpointEvaluator(cfg, str(tmp_path), envs, logger=log)
    ce.run_evals()
    want = [str(tmp_path / f"agent_checkpoint_{ts}") for ts in (7000, 300)]
    assert ce.processed_checkpoints == want and ce.unprocessed_checkpoints == [] and envs.resets == 2
    host, steps = _host_run(reward, kind, 50)
    mean = host.result()["mean"]
    assert log.rows == [("Report/Rewards", "Eval Reward", mean), ("Report/Metrics", "Cumulative Timesteps", 7000),
                        ("Report/Rewards", "Eval Reward", mean), ("Report/Metrics", "Cumulative Timesteps", 300)]
    assert torch.equal(ce.agent.flat.cpu(), flats[300]) and ce.evaluator.last == host.result()
    out = capsys.readouterr().out
    assert out.count("Evaluating checkpoint") == 2 and out.count("MEAN REWARD: {}\nSTD REWARD: {}".format(
        mean, host.result()["std"])) == 2 and out.index(want[0]) < out.index(want[1])
    assert f"EVALUATION OF CHECKPOINT {want[1]} COMPLETE." in out
    ce.run_evals()                                                              # nothing new
    assert len(log.rows) == 4 and envs.resets == 2 and ce.processed_checkpoints == want


def test_checkpoint_evaluator_on_a_checkpoint_the_reference_wrote(dev, tmp_path):
    """tests/golden/ref_checkpoint (tools/gen_golden.py checkpoint), through the same path."""
    from prism_amd.config import MINATAR_CONFIG, derive
    from prism_amd.evals import CheckpointEvaluator
    shutil.copytree(os.path.join(H.GOLDEN, "ref_checkpoint"), tmp_path / "agent_checkpoint_5000")
    cfg = derive(MINATAR_CONFIG, device=dev, use_cuda_graph=False, use_ids=False, use_iqn=False, use_dqn=True,
                 use_layer_norm=False, use_e_greedy=True, use_target_network=True, seed=999, log_to_wandb=False,
                 evaluation_timestep_horizon=30)
    reward, kind = _script(4, 30, 8)
    envs, log = ER.ScriptedEnvs(reward, kind), _Log()
    with contextlib.redirect_stdout(io.StringIO()):
        ce = CheckpointEvaluator(cfg, str(tmp_path), envs, logger=log)
        ce.run_evals()
    host, steps = _host_run(reward, kind, 30)
    assert ce.processed_checkpoints == [str(tmp_path / "agent_checkpoint_5000")] and ce.evaluator.last == host.result()
    assert log.rows == [("Report/Rewards", "Eval Reward", host.result()["mean"]),
                        ("Report/Metrics", "Cumulative Timesteps", 5000)]
    assert envs.k == steps and all(0 <= a < 6 for acts in envs.actions for a in acts) and not ce.agent._is_eval
