"""``config.captured_loop`` on the GPU: ``Learner.learn()`` with whole iterations (k x (act -> environment step -> ingest) +
the fused step) replayed from one hipGraph, against the eager loop from the same seed -- bit for bit, in everything a run
leaves behind; the knob switched off mid-run, evaluations between replays, resume, and the conditions that keep the loop eager.

Shapes: those of tests/resume_helpers.py (capacity 96, B = 16, N = 5 unless a case says otherwise)."""
import contextlib
import io

import pytest
import torch

from tests import resume_helpers as RH

pytestmark = pytest.mark.gpu

RANDOM = 40                      # num_initial_random_timesteps (resume_helpers.make_config)
PER_ENV = dict(e_greedy_per_env=True)
CONFIGS = {
    # IQN + PER + epsilon-greedy with a coin per environment, a target network synchronised inside the run; Breakout, A = 6
    "iqn_per_egreedy": dict(case="a_iqn_per_egreedy_adam", game="Breakout", attrs=PER_ENV),
    # the IDS ensemble (IQN + Q heads + LayerNorm + target network), the action a Philox draw
    "ids_sampled": dict(case="b_ids_sampled_full", game="Breakout"),
    # uniform replay, one-layer DQN head, RMSprop, a target network whose period (35 timesteps) falls inside the run
    "uniform_target": dict(case="c_dqn1_uniform_rmsprop", game="Breakout", over=dict(use_target_network=True), attrs=PER_ENV),
    # Freeway (C = 7, A = 3): uint8 observations into a uint8 ring
    "freeway_u8": dict(case="a_iqn_per_egreedy_adam", game="Freeway", obs_dtype="uint8", storage="uint8", attrs=PER_ENV),
    # Seaquest (C = 10, the wide state record) at N = 3
    "seaquest_n3": dict(case="a_iqn_per_egreedy_adam", game="Seaquest", n_env=3, attrs=PER_ENV),
}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _shape(name, tpi):
    """(environments, environment steps per iteration, rows of the random prologue, iterations until the ring is full)."""
    n = CONFIGS[name].get("n_env", RH.N_ENV)
    k = -(-tpi // n)
    rows0 = -(-RANDOM // n) * n
    return n, k, rows0, -(-(RH.CAPACITY - rows0) // (k * n))


def _limit(name, tpi, past_fill):
    n, k, rows0, fill = _shape(name, tpi)
    return rows0 + (fill + past_fill) * k * n, fill + past_fill


def _learner(dev, ckpt_dir, name, tpi, knob, limit, eval_every=None, evaluate=True, **over):
    from prism_amd import envs as E
    from prism_amd.collectors import VectorCollector
    from prism_amd.learner import Learner
    spec = CONFIGS[name]
    kw = dict(timesteps_per_iteration=tpi, timestep_limit=limit, atari_sticky_actions_prob=0.1, episode_timestep_limit=25,
              timesteps_between_evaluations=eval_every or 10 ** 9, evaluation_timestep_horizon=30)
    kw.update(spec.get("over", {}))
    kw.update(over)
    cfg = RH.make_config(spec["case"], ckpt_dir, dev, **kw)
    for k, v in spec.get("attrs", {}).items():
        setattr(cfg, k, v)
    cfg.captured_loop = knob
    cfg.replay_obs_storage = spec.get("storage", "float32")
    cls = dict(Breakout=E.DeviceBreakout, Freeway=E.DeviceFreeway, Seaquest=E.DeviceSeaquest)[spec["game"]]
    mk = lambda seed: cls(spec.get("n_env", RH.N_ENV), seed, dev, sticky_action_prob=0.1, episode_timestep_limit=25,
                          minimal_actions=spec["game"] != "Breakout", obs_dtype=spec.get("obs_dtype", "float32"))
    col = VectorCollector(mk(cfg.seed), cfg)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col, eval_envs=mk(cfg.seed + 1) if eval_every and evaluate else None)
    return ln, col


def _full(ln, col):
    """Everything the run has become (resume_helpers.full_state) plus what the device loop keeps: the environments' state
    records and acting observation, the episode bookkeeping, the device counters and the selector's position."""
    agent, buf = ln.agent, ln.experience_buffer
    st = RH.full_state(ln, col if isinstance(col, RH.ScriptedVectorCollector) else None)
    st["rng_counters"], st["eg_word"] = agent.rng_counters.cpu().clone(), agent._eg_word.cpu().clone()
    eps = getattr(agent.action_selector, "epsilon", None)
    st["current_step"] = int(eps.current_step) if hasattr(eps, "current_step") else None          # (IDS: epsilon is a float)
    st["episodes"] = [t.cpu().clone() for t in (buf._ep_return, buf._ep_length, buf._ep_words)] if buf._ep is not None else None
    envs = getattr(col, "envs", None)
    if envs is not None:
        st["env_state"], st["acting_obs"] = envs._state.cpu().clone(), envs.observe().cpu().clone()
        st["env_status"], st["rows"] = envs._status.cpu().clone(), int(col.rows)
    return st


def _learn(ln, col, hook=None):
    """learn() with the state taken before the way out empties the buffer: (state, eager iterations)."""
    buf, state, eager = ln.experience_buffer, [], [0]
    empty, step = buf.empty, ln.step

    def capture():
        state.append(_full(ln, col))
        return empty()

    def counted(*a, **k):
        eager[0] += 1
        return step(*a, **k)
    buf.empty, ln.step = capture, counted
    if hook is not None:
        real = ln.checkpointer.checkpoint
        ln.checkpointer.checkpoint = lambda *a, **k: (hook(ln), real(*a, **k))[1]
    with contextlib.redirect_stdout(io.StringIO()):
        ln.learn()
    torch.cuda.synchronize()
    return state[0], eager[0]


_EAGER = {}


def _eager_run(dev, tmp_path_factory, name, tpi, past_fill=60, **kw):
    """The knob-off run of a case, computed once and shared by the tests that compare against it."""
    key = (name, tpi, past_fill, tuple(sorted(kw.items())))
    if key not in _EAGER:
        limit, total = _limit(name, tpi, past_fill)
        ln, col = _learner(dev, tmp_path_factory.mktemp("eager"), name, tpi, False, limit, **kw)
        state, eager = _learn(ln, col)
        assert eager == total == ln.cumulative_model_updates and ln.captured_iterations == 0
        assert ln.captured_loop_refusal() == "config.captured_loop is off"
        _EAGER[key] = state
    return _EAGER[key]


@pytest.mark.parametrize("tpi", [5, 7, 10])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_knob_on_equals_knob_off(dev, tmp_path, tmp_path_factory, name, tpi):
    want = _eager_run(dev, tmp_path_factory, name, tpi)
    limit, total = _limit(name, tpi, 60)
    ln, col = _learner(dev, tmp_path, name, tpi, True, limit)
    got, eager = _learn(ln, col)
    assert ln.captured_loop_refusal() is None
    n, k, rows0, fill = _shape(name, tpi)
    # everything past the fill but the iteration that warms the capture up (the target sync is eager BETWEEN replays)
    assert ln.captured_iterations == 59 and eager + ln.captured_iterations == total == ln.cumulative_model_updates
    assert got["rows"] == limit and got["episodes"] is not None
    if k & 1:
        assert sorted(ln._captured._graphs) == [0, 1]          # both starting parities were replayed or ready
    RH.assert_same(got, want, f"{name}, {tpi} timesteps per iteration")


def test_knob_switched_off_mid_run(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 5
    want = _eager_run(dev, tmp_path_factory, name, tpi)
    limit, total = _limit(name, tpi, 60)
    fill = _shape(name, tpi)[3]
    ln, col = _learner(dev, tmp_path, name, tpi, True, limit)

    def hook(ln):
        if ln.cumulative_model_updates == fill + 30:
            ln.captured_loop = False
    got, eager = _learn(ln, col, hook)
    assert ln.captured_iterations == 29 and eager == total - 29
    RH.assert_same(got, want, "on for 30 iterations, off for 30")          # every host mirror was advanced


def test_evaluations_between_replays(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 5
    limit, total = _limit(name, tpi, 60)
    ln, col = _learner(dev, tmp_path, name, tpi, True, limit, eval_every=150)
    got, eager = _learn(ln, col)
    assert ln.evaluator.evaluations == 3 and ln.captured_iterations == 59
    # (the same configuration without evaluation environments: the evaluation period also sets the agent checkpoints')
    plain, plain_col = _learner(dev, tmp_path / "plain", name, tpi, True, limit, eval_every=150, evaluate=False)
    want, _ = _learn(plain, plain_col)
    assert plain.evaluator is None and plain.captured_iterations == 59
    RH.assert_same(got, want, "captured, with and without evaluations")
    RH.assert_same(want, _eager_run(dev, tmp_path_factory, name, tpi, eval_every=150, evaluate=False), "and the eager loop")


def _parts(path):
    from prism_amd.util import snapshot
    parts, _ = snapshot.read_snapshot(path, ["replay", "agent_resume", "learner"])
    for k in ("collected_steps_per_second_ema", "overall_steps_per_second_ema"):          # wall-clock rates
        parts["learner"].pop(k)
    return parts


def test_resume_after_captured_iterations(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 7
    (cut, _), (limit, _) = _limit(name, tpi, 25), _limit(name, tpi, 60)
    runs = {}
    for knob in (True, False):
        ln, col = _learner(dev, tmp_path / f"first_{knob}", name, tpi, knob, cut, backup_checkpoints=True)
        _learn(ln, col)
        assert ln.captured_iterations == (24 if knob else 0)
        runs[knob] = ln.checkpointer.latest_backup()
        assert runs[knob] is not None
    RH.assert_same(_parts(runs[True]), _parts(runs[False]), "the snapshot after captured iterations")
    # fresh objects, the knob on: what follows is the uninterrupted run (which is the eager run)
    ln, col = _learner(dev, tmp_path / "first_True", name, tpi, True, cut, backup_checkpoints=True)
    with contextlib.redirect_stdout(io.StringIO()):
        ln.load_state(ln.checkpointer.latest_backup())
    ln.timestep_limit = limit
    got, eager = _learn(ln, col)
    assert ln.captured_iterations == 34 and eager == 1 and ln.captured_loop_refusal() is None
    want = dict(_eager_run(dev, tmp_path_factory, name, tpi))
    # the device's PER and tau words start at 0 in a fresh agent and the host offsets carry what came before: their sums
    # (per_draws, tau_draws) are compared, of the words themselves only the acting count, which is seeded from the host's
    got["rng_counters"], want["rng_counters"] = got["rng_counters"][2:], want["rng_counters"][2:]
    RH.assert_same(got, want, "resumed with the knob on")


REFUSALS = {
    "host_coin": (dict(name="iqn_per_egreedy", attrs={"e_greedy_per_env": False}), "host coin", 20),
    "hip_graph_off": (dict(name="iqn_per_egreedy", attrs={"hip_graph": False}), "hip_graph", 20),
    "ring_not_full": (dict(name="ids_sampled"), "not full", -3),
}


@pytest.mark.parametrize("which", sorted(REFUSALS))
def test_refusals_keep_the_eager_loop(dev, tmp_path, which, monkeypatch):
    spec, text, past_fill = REFUSALS[which]
    name, tpi = spec["name"], 5
    monkeypatch.setitem(CONFIGS, name, dict(CONFIGS[name], attrs=dict(CONFIGS[name].get("attrs", {}), **spec.get("attrs", {}))))
    limit, total = _limit(name, tpi, past_fill)
    states = {}
    for knob in (True, False):
        ln, col = _learner(dev, tmp_path / str(knob), name, tpi, knob, limit)
        states[knob], eager = _learn(ln, col)
        assert ln.captured_iterations == 0 and eager == total
        if knob:
            assert text in ln.captured_loop_refusal(), ln.captured_loop_refusal()
            assert len(ln.experience_buffer) == 0          # (emptied on the way out; the reason is the last iteration's)
    if which == "ring_not_full":
        assert states[True]["size"] < RH.CAPACITY
    RH.assert_same(states[True], states[False], which)


def test_a_host_collector_keeps_the_eager_loop(dev, tmp_path):
    states = {}
    for knob in (True, False):
        ln, col = RH.make_learner("b_ids_sampled_full", tmp_path / str(knob), dev, timestep_limit=RANDOM + 5 * 30)
        ln.captured_loop = knob
        states[knob], eager = _learn(ln, col)
        assert ln.captured_iterations == 0 and eager == 30 and col.closed
        if knob:
            assert "collector" in ln.captured_loop_refusal()
    RH.assert_same(states[True], states[False], "a scripted host collector")
