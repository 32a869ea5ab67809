"""GPU: MinAtar Seaquest on the device (``prism_env_seaquest_reset`` / ``prism_env_seaquest_step``, ``DeviceSeaquest``) against
``HostSeaquest`` (tests/seaquest_ref.py: five Python lists per environment), exactly: the case table with given coins and
spawns, the Philox path, the ping-pong observation buffers, a captured step, ``VectorCollector`` / ``learn()`` /
``VectorEvaluator`` over the device environments (C = 10, A = 6), resume, and the overflow bit.  Neither side is checked
against the ``minatar`` package."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import eval_ref as ER
from tests import resume_helpers as RH
from tests import seaquest_cases as SC
from tests.seaquest_ref import HostSeaquest, assert_same_state
from tests.test_seaquest_host import PHILOX_RUN, SEED, philox_actions

pytestmark = pytest.mark.gpu
WIDE_ON = ("Seaquest",)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _pair(dev, n, obs_dtype="float32", seed=SEED, **kw):
    from prism_amd.envs import DeviceSeaquest
    return DeviceSeaquest(n, seed, dev, obs_dtype=obs_dtype, **kw), HostSeaquest(n, seed, **kw)


def _np(x):
    return x.cpu().numpy()


def assert_step_equal(got, want, where):
    """(next_obs, reward, done, truncated) of the device against the host's, exactly."""
    next_obs, reward, done, trunc = got
    assert reward.dtype == torch.float32 and done.dtype == torch.uint8 and trunc.dtype == torch.uint8
    np.testing.assert_array_equal(_np(next_obs).astype(np.float32), want[0], err_msg=f"{where}: next_obs")
    np.testing.assert_array_equal(_np(reward).view(np.uint32), want[1].view(np.uint32), err_msg=f"{where}: reward")
    np.testing.assert_array_equal(_np(done), want[2], err_msg=f"{where}: done")
    np.testing.assert_array_equal(_np(trunc), want[3], err_msg=f"{where}: truncated")


def assert_env_equal(env, host, where):
    from prism_amd.envs import pack_seaquest_state
    assert_same_state(env.get_state(), host.get_state(), where)
    # every state word: the record is the codec's packing of the lists, an emptied slot zero
    np.testing.assert_array_equal(_np(env._state), pack_seaquest_state(host.get_state()), err_msg=f"{where}: state words")
    np.testing.assert_array_equal(_np(env.observe()).astype(np.float32), host.observe(), err_msg=f"{where}: acting observation")


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(SC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    """Every case of the group (offsets 0, n, 2n, ... lay all of them over the n environments), every state word, both
    images, reward, done and truncated after every step; the observation the step acted on is left alone.  The cases of
    the overflow group drop the same append on both sides and raise the status bit."""
    from prism_amd import _native as N
    n_cases = len(SC.group_cases(group))
    for offset in range(0, n_cases, n):
        env, host = _pair(dev, n, obs_dtype, **SC.GROUPS[group])
        assert env.n_actions == host.n_actions == 6 and tuple(env.obs_shape) == (10, 10, 10)
        state, actions, u, draws = SC.vector(group, n, offset)
        env.set_state(state)
        host.set_state(state)
        assert env.observe().dtype == getattr(torch, obs_dtype) and env.observe().shape == (n, 10, 10, 10)
        assert_env_equal(env, host, f"{group} + {offset}: installed")
        for k in range(actions.shape[0]):
            where = f"{group} + {offset}, step {k}"
            acted_on = env.observe()
            kept = acted_on.clone()
            got = env.step(torch.from_numpy(actions[k]).to(dev), u=u[k], draws=draws[k])
            assert_step_equal(got, host.step(actions[k], u=u[k], draws=draws[k]), where)
            assert_env_equal(env, host, where)
            assert env.observe().data_ptr() != acted_on.data_ptr() and torch.equal(acted_on, kept), where
        names = SC.vector_names(group, n, offset)
        bad = any(SC.CASES[name].get("bad_action") for name in names)
        over = any(SC.CASES[name].get("overflow") for name in names)
        assert host.bad_action == bad and host.overflow == over
        if bad:
            with pytest.raises(N.PrismError, match=rf"outside \[0, {env.n_actions}\)"):
                env.check_status()
        if over:
            with pytest.raises(N.PrismError, match="full entity list"):
                env.check_status()
        env.close()          # (the status word is clean, or was cleared by the check above)


def test_the_overflow_bit_is_sticky_and_check_status_clears_it(dev):
    from prism_amd import _native as N
    n = 3
    env, host = _pair(dev, n)
    state, actions, u, draws = SC.vector("overflow", n)
    env.set_state(state)
    host.set_state(state)
    env.step(actions[0], u=u[0], draws=draws[0])
    host.step(actions[0], u=u[0], draws=draws[0])
    assert int(env._status.item()) == N.ENV_STATUS_OVERFLOW and host.overflow
    for k in range(3):          # further steps overflow nothing; the bit stays
        env.step(np.zeros(n, np.int64), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
        host.step(np.zeros(n, np.int64), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
    assert int(env._status.item()) == N.ENV_STATUS_OVERFLOW
    assert_env_equal(env, host, "after the overflow")          # the append was dropped on both sides, nothing else
    with pytest.raises(N.PrismError, match="DeviceSeaquest: a step appended to a full entity list"):
        env.check_status()
    env.check_status()          # cleared
    env.step(np.full(n, 9), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
    with pytest.raises(N.PrismError, match=r"outside \[0, 6\)"):
        env.close()


def test_philox_path_300_steps_at_n_5(dev):
    """The device's own coins and spawn draws against the host drawing through philox4x32; host actions (the pinned
    rotation) and device actions by turns; one lifetime count about to carry into its high word."""
    n, steps = PHILOX_RUN["n"], PHILOX_RUN["steps"]
    env, host = _pair(dev, n, **PHILOX_RUN["kw"])
    np.testing.assert_array_equal(_np(env.reset()), host.reset())
    assert_env_equal(env, host, "reset")
    terminals = truncations = 0
    for k, acts in enumerate(philox_actions()):
        if k == steps // 2:          # from here on environment 1 draws beyond a 32-bit counter
            st = host.get_state()
            st["t"][1] = 2 ** 32 - 3
            env.set_state(st)
            host.set_state(st)
        got = env.step(acts if k % 2 else torch.from_numpy(acts).to(dev))
        want = host.step(acts)
        assert_step_equal(got, want, f"step {k}")
        assert_env_equal(env, host, f"step {k}")
        terminals, truncations = terminals + int(want[2].sum()), truncations + int(want[3].sum())
    br = host.branches
    assert terminals >= 1 and truncations >= 1 and br["spawn_fish"] >= 1 and br["spawn_sub"] >= 1 and br["spawn_diver"] >= 1
    assert br["sticky_repeat"] > 100 and br["fire"] >= 1 and not host.overflow
    assert int(env.get_state()["t"][1]) == 2 ** 32 - 3 + steps - steps // 2
    env.close()


def test_philox_path_at_the_hardest_ramp(dev):
    """Long lists: 200 steps from the hardest ramp (a spawn every step, enemies that move every third), the device's own draws."""
    n = 4
    env, host = _pair(dev, n, sticky_action_prob=0.1)
    host.reset()
    st = host.get_state()
    st["e_spawn_speed"][:], st["move_speed"][:], st["ramp_index"][:], st["e_spawn_timer"][:] = 1, 2, 19, 0
    st["sub_x"][:], st["sub_y"][:], st["surface"][:] = [1, 3, 6, 8], [2, 4, 6, 8], 0
    env.set_state(st)
    host.set_state(st)
    rng = np.random.default_rng(3)
    longest = 0
    for k in range(200):
        acts = rng.integers(0, 6, n)
        assert_step_equal(env.step(acts), host.step(acts), f"step {k}")
        assert_env_equal(env, host, f"step {k}")
        longest = max([longest] + [len(e["e_fish"]) + len(e["e_subs"]) for e in host.envs])
        if any(e["ep_steps"] == 0 for e in host.envs):          # an episode that ended begins at the hardest ramp again
            st = host.get_state()
            fresh = st["ep_steps"] == 0
            st["e_spawn_speed"][fresh], st["move_speed"][fresh], st["ramp_index"][fresh], st["e_spawn_timer"][fresh] = 1, 2, 19, 0
            env.set_state(st)
            host.set_state(st)
    assert longest >= 8 and host.branches["sub_fires"] >= 3 and not host.overflow
    env.close()


def test_given_draw_argument_checks(dev):
    env, host = _pair(dev, 3, "uint8", sticky_action_prob=0.5)
    np.testing.assert_array_equal(_np(env.reset()).astype(np.float32), host.reset())
    acts = torch.full((3,), 5, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="one value per environment"):
        env.step(acts, u=np.zeros(2))
    with pytest.raises(ValueError, match="5 values per environment"):
        env.step(acts, None, np.ones((3, 3), np.uint8))
    with pytest.raises(ValueError, match="draws must be"):
        env.step(acts, None, np.zeros((3, 5), np.uint8))
    assert_env_equal(env, host, "after the refusals")          # none of them stepped
    u = np.array([0.1, 0.5, 0.9])
    for k in range(4):
        assert_step_equal(env.step(acts, u=u), host.step(np.full(3, 5), u=u), f"step {k}")
    assert_env_equal(env, host, "given coins")
    assert list(env.get_state()["last_action"]) == [0, 5, 5]
    env.close()


def test_the_previous_acting_observation_survives_step(dev):
    env, host = _pair(dev, 7)
    first = env.reset()
    host.reset()
    seen = [first.data_ptr()]
    for k in range(6):
        acted_on, want = env.observe(), host.observe()
        env.step(torch.full((7,), 1 + 2 * (k % 3), dtype=torch.int64, device=dev))
        host.step(np.full(7, 1 + 2 * (k % 3)))
        np.testing.assert_array_equal(_np(acted_on), want)          # still what the step acted on
        np.testing.assert_array_equal(_np(env.observe()), host.observe())
        seen.append(env.observe().data_ptr())
    assert seen[0::2] == [seen[0]] * 4 and seen[1::2] == [seen[1]] * 3 and seen[0] != seen[1]          # two addresses, by turns
    with pytest.raises(RuntimeError, match="reset"):
        _pair(dev, 2)[0].step(np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="actions"):
        env.step(torch.zeros(6, dtype=torch.int64, device=dev))


def test_a_captured_step_replayed_50_times_equals_an_eager_twin(dev):
    """The launch takes no host value that changes between steps: one captured ``step`` replayed 50 times (the actions
    change in their buffer) is the eager twin's 50 steps, bit for bit."""
    n = 9
    kw = dict(sticky_action_prob=0.25, episode_timestep_limit=20)
    graphed, eager = _pair(dev, n, "uint8", **kw)[0], _pair(dev, n, "uint8", **kw)[0]
    rng = np.random.default_rng(8)
    acts = torch.from_numpy(rng.integers(0, 6, (51, n))).to(dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got, want = [], []
    with torch.cuda.stream(side):
        buf = acts[0].clone()
        graphed.reset()
        graphed.step(buf)                        # (eager once: the first launch of a kernel loads it)
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = graphed.step(buf)
        written = graphed.observe()              # the ping-pong buffer the captured launch writes
        for k in range(1, 51):
            buf.copy_(acts[k])
            g.replay()
            got.append([t.clone() for t in out] + [written.clone()])
        side.synchronize()
    eager.reset()
    eager.step(acts[0])
    for k in range(1, 51):
        out_e = eager.step(acts[k])
        want.append([t.clone() for t in out_e] + [eager.observe().clone()])
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(got, want)):
        for name, x, y in zip(("next_obs", "reward", "done", "truncated", "acting observation"), a, b):
            assert torch.equal(x, y), f"replay {k}: {name}"
    assert torch.equal(graphed._state, eager._state)
    assert int(eager.get_state()["t"].min()) == 51 and sum(int(w[2].sum() + w[3].sum()) for w in want) >= 5


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
ENV_NAME = "MinAtar/Seaquest-v1"
ENV_INFO = ((10, 10, 10), 6, 1)


def _learner(dev, ckpt_dir, envs=None, obs_storage="float32", **over):
    """A small learner (tests/resume_helpers.py case (a): IQN + PER + epsilon-greedy) over ``envs`` or, by default, over the
    configuration's own device environments (``build_collector`` with the wide-record knob on): C = 10, A = 6."""
    from prism_amd.collectors import VectorCollector
    from prism_amd.factory.collector_factory import build_collector
    from prism_amd.learner import Learner
    kw = dict(env_name=ENV_NAME, num_processes=RH.N_ENV, atari_sticky_actions_prob=0.1, episode_timestep_limit=25,
              experience_replay_capacity=512)
    kw.update(over)
    cfg = RH.make_config("a_iqn_per_egreedy_adam", ckpt_dir, dev, **kw)
    cfg.device_env_wide_games = WIDE_ON
    cfg.replay_obs_storage = obs_storage
    col = build_collector(cfg) if envs is None else VectorCollector(envs(cfg), cfg)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
    return ln, col


def _ring(buf):
    buf.flush()
    torch.cuda.synchronize()
    return {name: getattr(buf, name).cpu().clone() for name in ("obs", "succ_obs", "reward", "action", "flags", "link", "back")
            if getattr(buf, name) is not None}


@pytest.mark.parametrize("obs_storage", ["float32", "uint8"])
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path, obs_storage):
    from prism_amd.envs import DeviceSeaquest
    obs_dtype = obs_storage
    ln_d, col_d = _learner(dev, tmp_path / "d", obs_storage=obs_storage, envs=lambda cfg: DeviceSeaquest(
        RH.N_ENV, cfg.seed, dev, sticky_action_prob=cfg.atari_sticky_actions_prob, episode_timestep_limit=cfg.episode_timestep_limit,
        minimal_actions=True, obs_dtype=obs_dtype))
    ln_h, col_h = _learner(dev, tmp_path / "h", obs_storage=obs_storage, envs=lambda cfg: HostSeaquest(
        RH.N_ENV, cfg.seed, sticky_action_prob=cfg.atari_sticky_actions_prob, episode_timestep_limit=cfg.episode_timestep_limit,
        minimal_actions=True))
    assert col_d.envs.seed == col_h.envs.seed == ln_d.agent.config.seed
    assert col_d.get_env_info() == ENV_INFO
    for ln, col in ((ln_d, col_d), (ln_h, col_h)):
        assert col.collect_timesteps(40, ln.agent, ln.experience_buffer, random=True) == 40
        assert col.collect_timesteps(120, ln.agent, ln.experience_buffer) == 120
    ring_d, ring_h = _ring(ln_d.experience_buffer), _ring(ln_h.experience_buffer)
    assert col_d.envs.observe().dtype == ring_d["obs"].dtype == getattr(torch, obs_storage)
    RH.assert_same(ring_d, ring_h, "ring")
    ln_d.experience_buffer.check_status()
    set_elements = ring_d["obs"][:160].reshape(160, -1).float().sum(dim=1)
    assert set_elements.ge(2).all() and set_elements.max() >= 12          # the sub and its rear cell; a reset's image has 12
    assert ln_d.experience_buffer.episode_stats() == ln_h.experience_buffer.episode_stats()
    assert ln_d.experience_buffer.episode_stats()["episodes"] >= 5
    assert_env_equal(col_d.envs, col_h.envs, "after 160 rows")
    assert len(ring_d["action"][:160].unique()) > 2 and int(ring_d["action"][:160].max()) == 5
    col_d.close()


def test_build_collector_with_the_wide_knob_builds_device_seaquest(dev, tmp_path):
    from prism_amd.envs import DeviceSeaquest
    ln, col = _learner(dev, tmp_path / "k")
    assert isinstance(col.envs, DeviceSeaquest) and col.envs.minimal_actions and col.envs.n_envs == RH.N_ENV
    assert col.envs.n_actions == 6 and col.envs.seed == ln.agent.config.seed and col.get_env_info() == ENV_INFO
    assert tuple(col.envs._state.shape) == (RH.N_ENV, 112)
    col.close()


def _learn(dev, ckpt_dir):
    ln, col = _learner(dev, ckpt_dir, num_initial_random_timesteps=40, timestep_limit=40 + RH.N_ENV * 40,
                       timesteps_per_report=100, timesteps_between_evaluations=10 ** 6)
    buf = ln.experience_buffer
    with contextlib.redirect_stdout(io.StringIO()):
        real_empty, buf.empty = buf.empty, lambda: None          # learn() empties the buffer on exit: keep it for the checks
        ln.learn()
        buf.empty = real_empty
    return ln, col


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    a, col_a = _learn(dev, tmp_path / "a")
    b, col_b = _learn(dev, tmp_path / "b")
    assert a.cumulative_timesteps == b.cumulative_timesteps == 40 + RH.N_ENV * 40 and a.cumulative_model_updates == 40
    assert col_a.envs.closed and col_a.rows == 240 and col_a.get_env_info() == ENV_INFO
    RH.assert_same(RH.full_state(a), RH.full_state(b), "learn")
    RH.assert_same(_ring(a.experience_buffer), _ring(b.experience_buffer), "ring")
    assert_same_state(col_a.envs.get_state(), col_b.envs.get_state(), "environments")
    assert int(col_a.envs.get_state()["t"].min()) == 240 // RH.N_ENV
    assert a.experience_buffer.episode_stats() == b.experience_buffer.episode_stats()
    assert a.experience_buffer.episode_stats()["episodes"] >= 5


def _agent(dev):
    from prism_amd.config import baseline_config
    from prism_amd.factory import agent_factory
    cfg = baseline_config(2, device=dev, batch_size=16, log_to_wandb=False, seed=SEED & 0xFFFF)
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, 10), 6)
    gen = torch.Generator().manual_seed(5)          # away from the initialisation: actions that depend on the draws
    agent.model.load_state_dict({k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen)
                                 for k, v in agent.model.state_dict().items()})
    agent._params_replaced()
    return agent


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    from prism_amd.evals import EVAL_DRAW_BASE, VectorEvaluator
    n, horizon = 5, 203
    kw = dict(sticky_action_prob=0.1, episode_timestep_limit=30, minimal_actions=True)
    env, host = _pair(dev, n, **kw)
    agent = _agent(dev)
    ev = VectorEvaluator(agent, env, 0, horizon)
    returns = ev.evaluate_agent()
    twin = _agent(dev)
    want = ER.EvalHost(n, horizon)
    twin.eval()
    with twin.acting_stream(EVAL_DRAW_BASE):
        obs, steps = host.reset(), 0
        while True:
            _, reward, done, trunc = host.step(twin.forward(obs))
            want.track(reward, done, trunc)
            obs = host.observe()
            steps += 1
            if steps * n >= horizon and want.closed():
                break
    twin.train()
    np.testing.assert_array_equal(ER.bits64(returns), ER.bits64(want.returns()))
    assert ev.last == want.result() and ev.last["timesteps"] == steps * n and ev.last["episodes"] >= 3
    assert_env_equal(env, host, "after the evaluation")
    assert len(ev.evaluate_agent()) >= 3
    env.close()


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    from prism_amd.envs import DeviceSpaceInvaders
    from prism_amd.util import snapshot
    n = 6
    kw = dict(sticky_action_prob=0.25, episode_timestep_limit=40, minimal_actions=True)
    a, host = _pair(dev, n, "uint8", **kw)
    a.reset()
    host.reset()
    rng = np.random.default_rng(4)
    acts = rng.integers(0, 6, (70, n))
    for k in range(35):
        a.step(acts[k])
        host.step(acts[k])
    sd = a.state_dict()
    snapshot.check_plain(sd)
    assert sd["kind"] == "DeviceSeaquest" and sd["n_actions"] == 6 and tuple(sd["state"].shape) == (n, 112)
    assert sum(len(x) for name in ("e_fish", "e_subs", "divers") for x in a.get_state()[name]) >= 1          # lists travel with it
    b = _pair(dev, n, "uint8", **kw)[0]
    b.load_state_dict(sd)
    np.testing.assert_array_equal(_np(b.observe()), _np(a.observe()))
    assert torch.equal(b._state, a._state)          # get_state -> set_state reproduces the words exactly
    for k in range(35, 70):
        out_a, out_b = a.step(acts[k]), b.step(acts[k])
        want = host.step(acts[k])
        assert_step_equal(out_b, want, f"step {k}")
        for x, y in zip(out_a, out_b):
            assert torch.equal(x, y)
        assert torch.equal(a.observe(), b.observe())
    assert_env_equal(b, host, "continued")
    fresh = _pair(dev, n, "uint8", **kw)[0]
    fresh.load_state_dict(fresh.state_dict())          # never started: stays so
    with pytest.raises(RuntimeError, match="reset"):
        fresh.observe()
    with pytest.raises(ValueError, match="n_envs"):
        _pair(dev, n + 1, "uint8", **kw)[0].load_state_dict(sd)
    with pytest.raises(ValueError, match="seed"):
        _pair(dev, n, "uint8", seed=1, **kw)[0].load_state_dict(sd)
    # another game's snapshot is refused, either way round
    other = DeviceSpaceInvaders(n, SEED, dev, obs_dtype="uint8", sticky_action_prob=0.25, episode_timestep_limit=40)
    with pytest.raises(ValueError, match="kind"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        b.load_state_dict(other.state_dict())


def _iterate(ln, col):
    col.collect_timesteps(RH.N_ENV, ln.agent, ln.experience_buffer)
    ln.cumulative_timesteps += RH.N_ENV
    td = ln.step(RH.N_ENV)
    return td.cpu().clone(), col.envs.get_state()


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    ln, col = _learner(dev, tmp_path / "a")
    col.collect_timesteps(40, ln.agent, ln.experience_buffer, random=True)
    ln.cumulative_timesteps += 40
    for _ in range(6):
        _iterate(ln, col)
    ln.save_state(tmp_path / "snap")
    assert ln._state_part()["collector"]["envs"]["kind"] == "DeviceSeaquest"
    want = [_iterate(ln, col) for _ in range(8)]
    ln2, col2 = _learner(dev, tmp_path / "b")
    ln2.load_state(tmp_path / "snap")
    got = [_iterate(ln2, col2) for _ in range(8)]
    for k, ((td_a, st_a), (td_b, st_b)) in enumerate(zip(want, got)):
        assert torch.equal(td_a.view(torch.int32), td_b.view(torch.int32)), f"iteration {k}: TD errors"
        assert_same_state(st_b, st_a, f"iteration {k}")
    RH.assert_same(RH.full_state(ln2), RH.full_state(ln), "resumed")
    RH.assert_same(_ring(ln2.experience_buffer), _ring(ln.experience_buffer), "ring")
    assert int(col2.envs.get_state()["t"].min()) == (40 + 14 * RH.N_ENV) // RH.N_ENV
