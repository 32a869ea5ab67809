"""What the five device games' suites share, once: tests/test_gpu_<game>.py and tests/test_<game>_host.py call these routines
with their game's row of ``tests/env_frame_cases.py GAMES`` and keep their game's own assertions.  The upper half needs a GPU
(torch is imported there only); the lower half is the host side of the device environment and needs none."""
import contextlib
import ctypes
import importlib
import io
import os
import re

import numpy as np
import pytest

from tests import eval_ref as ER
from tests import helpers as H
from tests import resume_helpers as RH
from tests.env_frame_cases import GAMES


def ref(game):
    return importlib.import_module(game.ref)


def cases(game):
    return importlib.import_module(game.cases)


def host_class(game):
    return getattr(ref(game), game.host)


def device_class(game):
    from prism_amd import envs
    return getattr(envs, game.device)


def env_info(game):
    """``get_env_info()`` of the game's learner: the suite learns on the minimal set, Breakout's on the full one."""
    return (game.obs_shape, game.minimal if game.learn_minimal else game.full, 1)


def philox_actions(game, host=None):
    """The actions of the game's Philox-path run, step by step: one held action, ``RandomState(s).randint(0, high, n)`` per
    step, or Breakout's paddle that follows the ball of ``host`` six times in ten (read when the step is asked for)."""
    run = game.philox
    kind, *args = run["actions"]
    rng = np.random.default_rng(args[0]) if kind == "track" else np.random.RandomState(args[0])
    for _ in range(run["steps"]):
        if kind == "hold":
            yield np.full(run["n"], args[0], dtype=np.int64)
        elif kind == "randint":
            yield rng.randint(0, args[1], size=run["n"]).astype(np.int64)
        else:
            hs = host.get_state()
            track = np.where(hs["ball_x"] < hs["pos"], 1, np.where(hs["ball_x"] > hs["pos"], 3, 0))
            yield np.where(rng.random(run["n"]) < 0.6, track, rng.integers(0, 6, run["n"])).astype(np.int64)


def philox_host_run(game):
    """The Philox-path run on the host restatement alone -> (host, [rewards, terminals, truncations])."""
    host = host_class(game)(game.philox["n"], game.seed, **game.philox["kw"])
    host.reset()
    tally = [0, 0, 0]
    for acts in philox_actions(game, host):
        tally = [a + int(b.sum()) for a, b in zip(tally, host.step(acts)[1:])]
    return host, tally


# ---------------------------------------------------------------------------------------------------- GPU: device against host
def _np(x):
    return x.cpu().numpy()


def pair(game, dev, n, obs_dtype="float32", seed=None, **kw):
    seed = game.seed if seed is None else seed
    return device_class(game)(n, seed, dev, obs_dtype=obs_dtype, **kw), host_class(game)(n, seed, **kw)


def assert_step_equal(got, want, where):
    """(next_obs, reward, done, truncated) of the device against the host's, exactly."""
    import torch
    next_obs, reward, done, trunc = got
    assert reward.dtype == torch.float32 and done.dtype == torch.uint8 and trunc.dtype == torch.uint8
    np.testing.assert_array_equal(_np(next_obs).astype(np.float32), want[0], err_msg=f"{where}: next_obs")
    np.testing.assert_array_equal(_np(reward).view(np.uint32), want[1].view(np.uint32), err_msg=f"{where}: reward")
    np.testing.assert_array_equal(_np(done), want[2], err_msg=f"{where}: done")
    np.testing.assert_array_equal(_np(trunc), want[3], err_msg=f"{where}: truncated")


def assert_env_equal(game, env, host, where):
    """Every state field, the acting image and, for a game whose record the suite holds to the codec, every state word."""
    ref(game).assert_same_state(env.get_state(), host.get_state(), where)
    if game.words_packed:          # the record is the codec's packing of the host's fields, an emptied slot zero
        np.testing.assert_array_equal(_np(env._state), type(env)._pack(host.get_state()), err_msg=f"{where}: state words")
    np.testing.assert_array_equal(_np(env.observe()).astype(np.float32), host.observe(), err_msg=f"{where}: acting observation")


def case_table_run(game, dev, group, n, obs_dtype):
    """Every case of the group (offsets 0, n, 2n, ... lay all of them over the n environments), every state field, both
    images, reward, done and truncated after every step; the observation the step acted on is left alone; the status word
    holds what the cases say (an action out of range, an append to a full list) and nothing else."""
    import torch
    from prism_amd import _native as N
    C = cases(game)
    for offset in range(0, len(C.group_cases(group)), n):
        env, host = pair(game, dev, n, obs_dtype, **C.GROUPS[group])
        actions_of = game.minimal if C.GROUPS[group].get("minimal_actions") else game.full
        assert env.n_actions == host.n_actions == actions_of and tuple(env.obs_shape) == game.obs_shape
        state, actions, u, *draws = C.vector(group, n, offset)
        assert len(draws) == (game.step_draw is not None)
        env.set_state(state)
        host.set_state(state)
        assert env.observe().dtype == getattr(torch, obs_dtype) and env.observe().shape == (n,) + game.obs_shape
        assert_env_equal(game, env, host, f"{group} + {offset}: installed")
        for k in range(actions.shape[0]):
            where = f"{group} + {offset}, step {k}"
            given = {game.step_draw: draws[0][k]} if draws else {}
            acted_on = env.observe()
            kept = acted_on.clone()
            got = env.step(torch.from_numpy(actions[k]).to(dev), u=u[k], **given)
            assert_step_equal(got, host.step(actions[k], u=u[k], **given), where)
            assert_env_equal(game, env, host, where)
            assert env.observe().data_ptr() != acted_on.data_ptr() and torch.equal(acted_on, kept), where
        names = C.vector_names(group, n, offset)
        bad = any(C.CASES[name].get("bad_action") for name in names)
        over = any(C.CASES[name].get("overflow") for name in names)
        assert host.bad_action == bad and getattr(host, "overflow", False) == over
        if bad:
            with pytest.raises(N.PrismError, match=rf"outside \[0, {env.n_actions}\)"):
                env.check_status()
        if over:
            with pytest.raises(N.PrismError, match="full entity list"):
                env.check_status()
        env.close()          # (the status word is clean, or was cleared by the checks above)


def philox_run(game, dev):
    """The device's own draws against the host drawing through philox4x32, over the game's Philox-path run; host actions and
    device actions by turns; from step ``carry_at`` on environment 1 draws beyond a 32-bit counter.
    -> (host, [rewards, terminals, truncations])"""
    import torch
    run = game.philox
    env, host = pair(game, dev, run["n"], **run["kw"])
    np.testing.assert_array_equal(_np(env.reset()), host.reset())
    assert_env_equal(game, env, host, "reset")
    tally = [0, 0, 0]
    for k, acts in enumerate(philox_actions(game, host)):
        if k == run["carry_at"]:
            st = host.get_state()
            st["t"][1] = 2 ** 32 - 3
            env.set_state(st)
            host.set_state(st)
        got = env.step(acts if k % 2 else torch.from_numpy(acts).to(dev))
        want = host.step(acts)
        assert_step_equal(got, want, f"step {k}")
        assert_env_equal(game, env, host, f"step {k}")
        tally = [a + int(b.sum()) for a, b in zip(tally, want[1:])]
    assert int(env.get_state()["t"][1]) == 2 ** 32 - 3 + run["steps"] - run["carry_at"]
    env.close()
    return host, tally


def ping_pong_check(game, dev, action):
    """Six steps of ``action(k)`` at n = 7: the observation a step acted on survives it, at two addresses by turns."""
    import torch
    env, host = pair(game, dev, 7)
    first = env.reset()
    host.reset()
    seen = [first.data_ptr()]
    for k in range(6):
        acted_on, want = env.observe(), host.observe()
        env.step(torch.full((7,), action(k), dtype=torch.int64, device=dev))
        host.step(np.full(7, action(k)))
        np.testing.assert_array_equal(_np(acted_on), want)          # still what the step acted on
        np.testing.assert_array_equal(_np(env.observe()), host.observe())
        seen.append(env.observe().data_ptr())
    assert seen[0::2] == [seen[0]] * 4 and seen[1::2] == [seen[1]] * 3 and seen[0] != seen[1]          # two addresses, by turns
    with pytest.raises(RuntimeError, match="reset"):
        pair(game, dev, 2)[0].step(np.zeros(2, np.int64))
    with pytest.raises(ValueError, match="actions"):
        env.step(torch.zeros(6, dtype=torch.int64, device=dev))


def captured_step_run(game, dev, obs_dtype="uint8", acts=None):
    """The launch takes no host value that changes between steps: one captured ``step`` replayed 50 times (the actions
    change in their buffer) is the eager twin's 50 steps, bit for bit.  ``acts``: int64 [51, 9], by default uniform in
    [0, 6) from ``default_rng(8)``.  -> (the eager twin, its 50 [next_obs, reward, done, truncated, acting observation])"""
    import torch
    n = 9
    kw = dict(sticky_action_prob=0.25, episode_timestep_limit=20)
    graphed, eager = pair(game, dev, n, obs_dtype, **kw)[0], pair(game, dev, n, obs_dtype, **kw)[0]
    acts = torch.from_numpy(np.random.default_rng(8).integers(0, 6, (51, n)) if acts is None else acts).to(dev)
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
    ref(game).assert_same_state(graphed.get_state(), eager.get_state(), "after 50 replays")
    assert torch.equal(graphed._state, eager._state)
    assert int(eager.get_state()["t"].min()) == 51 and sum(int(w[2].sum() + w[3].sum()) for w in want) >= 5
    return eager, want


# ---------------------------------------------------------------------------------------------------- GPU: collector, learn, evaluator
def learner(game, dev, ckpt_dir, envs=None, obs_storage="float32", **over):
    """A small learner (tests/resume_helpers.py case (a): IQN + PER + epsilon-greedy) over ``envs(cfg)`` or, by default, over
    the configuration's own device environments: ``build_collector`` with the game's knob on."""
    from prism_amd.collectors import VectorCollector
    from prism_amd.factory.collector_factory import build_collector
    from prism_amd.learner import Learner
    kw = dict(env_name=f"MinAtar/{game.name}-v{int(game.learn_minimal)}", num_processes=RH.N_ENV, atari_sticky_actions_prob=0.1,
              episode_timestep_limit=25, experience_replay_capacity=512)
    kw.update(over)
    cfg = RH.make_config("a_iqn_per_egreedy_adam", ckpt_dir, dev, **kw)
    for knob, value in game.knob.items():
        setattr(cfg, knob, value)
    cfg.replay_obs_storage = obs_storage
    col = build_collector(cfg) if envs is None else VectorCollector(envs(cfg), cfg)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
    return ln, col


def ring(buf):
    import torch
    buf.flush()
    torch.cuda.synchronize()
    return {name: getattr(buf, name).cpu().clone() for name in ("obs", "succ_obs", "reward", "action", "flags", "link", "back")
            if getattr(buf, name) is not None}


def collector_twin_run(game, dev, tmp_path, obs_storage=None):
    """40 random and 120 acted rows through a ``VectorCollector`` over the device environments and through a twin fed by
    the host restatement: the same ring, episodes and environments.  The device side observes in ``obs_storage``; with
    None it is the configuration's own (``build_collector``) and the ring is fp32.
    -> (ring_d, ring_h, col_d, col_h); the caller closes ``col_d``."""
    import torch
    storage = obs_storage or "float32"
    kw = lambda cfg: dict(sticky_action_prob=cfg.atari_sticky_actions_prob, episode_timestep_limit=cfg.episode_timestep_limit,
                          minimal_actions=game.learn_minimal)
    ln_d, col_d = learner(game, dev, tmp_path / "d", obs_storage=storage, envs=None if obs_storage is None else (
        lambda cfg: device_class(game)(RH.N_ENV, cfg.seed, dev, obs_dtype=obs_storage, **kw(cfg))))
    ln_h, col_h = learner(game, dev, tmp_path / "h", obs_storage=storage, envs=lambda cfg: host_class(game)(RH.N_ENV, cfg.seed, **kw(cfg)))
    assert isinstance(col_d.envs, device_class(game)) and col_d.envs.seed == col_h.envs.seed == ln_d.agent.config.seed
    assert col_d.get_env_info() == env_info(game)
    for ln, col in ((ln_d, col_d), (ln_h, col_h)):
        assert col.collect_timesteps(40, ln.agent, ln.experience_buffer, random=True) == 40
        assert col.collect_timesteps(120, ln.agent, ln.experience_buffer) == 120
    ring_d, ring_h = ring(ln_d.experience_buffer), ring(ln_h.experience_buffer)
    assert col_d.envs.observe().dtype == ring_d["obs"].dtype == getattr(torch, storage)
    RH.assert_same(ring_d, ring_h, "ring")
    ln_d.experience_buffer.check_status()
    assert ln_d.experience_buffer.episode_stats() == ln_h.experience_buffer.episode_stats()
    assert ln_d.experience_buffer.episode_stats()["episodes"] >= 5
    assert_env_equal(game, col_d.envs, col_h.envs, "after 160 rows")
    assert len(ring_d["action"][:160].unique()) > 1
    return ring_d, ring_h, col_d, col_h


def knob_collector_check(game, dev, tmp_path):
    """``build_collector`` with the game's knob on builds its device class on the minimal set.  -> the collector (open)"""
    ln, col = learner(game, dev, tmp_path / "k")
    assert isinstance(col.envs, device_class(game)) and col.envs.minimal_actions and col.envs.n_envs == RH.N_ENV
    assert col.envs.n_actions == game.minimal and col.envs.seed == ln.agent.config.seed and col.get_env_info() == env_info(game)
    return col


def learn(game, dev, ckpt_dir, updates):
    ln, col = learner(game, dev, ckpt_dir, num_initial_random_timesteps=40, timestep_limit=40 + RH.N_ENV * updates,
                      timesteps_per_report=100, timesteps_between_evaluations=10 ** 6)
    buf = ln.experience_buffer
    with contextlib.redirect_stdout(io.StringIO()):
        real_empty, buf.empty = buf.empty, lambda: None          # learn() empties the buffer on exit: keep it for the checks
        ln.learn()
        buf.empty = real_empty
    return ln, col


def learn_twice_check(game, dev, tmp_path, updates=40):
    """``learn()`` twice from one seed: learner, ring and environments bit-identical."""
    a, col_a = learn(game, dev, tmp_path / "a", updates)
    b, col_b = learn(game, dev, tmp_path / "b", updates)
    rows = 40 + RH.N_ENV * updates
    assert a.cumulative_timesteps == b.cumulative_timesteps == rows and a.cumulative_model_updates == updates
    assert col_a.envs.closed and col_a.rows == rows and col_a.get_env_info() == env_info(game)
    RH.assert_same(RH.full_state(a), RH.full_state(b), "learn")
    RH.assert_same(ring(a.experience_buffer), ring(b.experience_buffer), "ring")
    ref(game).assert_same_state(col_a.envs.get_state(), col_b.envs.get_state(), "environments")
    assert int(col_a.envs.get_state()["t"].min()) == rows // RH.N_ENV
    assert a.experience_buffer.episode_stats() == b.experience_buffer.episode_stats()
    assert a.experience_buffer.episode_stats()["episodes"] >= 5


def agent(game, dev):
    import torch
    from prism_amd.config import baseline_config
    from prism_amd.factory import agent_factory
    cfg = baseline_config(2, device=dev, batch_size=16, log_to_wandb=False, seed=game.seed & 0xFFFF)
    torch.manual_seed(11)
    with contextlib.redirect_stdout(io.StringIO()):
        made = agent_factory.build_agent(cfg, game.obs_shape, game.minimal)
    gen = torch.Generator().manual_seed(5)          # away from the initialisation: actions that depend on the draws
    made.model.load_state_dict({k: v.cpu() + 0.05 * torch.randn(v.shape, generator=gen) for k, v in made.model.state_dict().items()})
    made._params_replaced()
    return made


def evaluator_run(game, dev, make_agent=None, **kw):
    """``VectorEvaluator`` over the device environments against ``EvalHost`` over the host restatement, each with an agent
    of ``make_agent()`` (by default ``agent(game, dev)``, on the minimal action set)."""
    from prism_amd.evals import EVAL_DRAW_BASE, VectorEvaluator
    make_agent = make_agent or (lambda: agent(game, dev))
    n, horizon = 5, 203
    env, host = pair(game, dev, n, sticky_action_prob=0.1, episode_timestep_limit=30, **kw)
    ev = VectorEvaluator(make_agent(), env, 0, horizon)
    returns = ev.evaluate_agent()
    twin = make_agent()
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
    assert_env_equal(game, env, host, "after the evaluation")
    # a second evaluation starts the environments afresh: same episodes unless the agent's draws differ
    assert len(ev.evaluate_agent()) >= 3
    env.close()


# ---------------------------------------------------------------------------------------------------- GPU: resume
def state_dict_run(game, dev, acts, other, limit=20, at_snapshot=None):
    """Half of ``acts`` (int [steps, 6], minimal set), ``state_dict`` into a fresh object, the other half on both and on the
    host; what ``load_state_dict`` refuses: other ``n_envs``, another seed, the snapshot of game ``other`` either way round.
    ``at_snapshot(a, sd)`` runs when the snapshot is taken."""
    import torch
    from prism_amd.util import snapshot
    n, half = 6, len(acts) // 2
    kw = dict(sticky_action_prob=0.25, episode_timestep_limit=limit, minimal_actions=True)
    a, host = pair(game, dev, n, "uint8", **kw)
    a.reset()
    host.reset()
    for k in range(half):
        a.step(acts[k])
        host.step(acts[k])
    sd = a.state_dict()
    snapshot.check_plain(sd)
    assert sd["kind"] == game.device and sd["n_actions"] == game.minimal
    if at_snapshot is not None:
        at_snapshot(a, sd)
    b = pair(game, dev, n, "uint8", **kw)[0]
    b.load_state_dict(sd)
    np.testing.assert_array_equal(_np(b.observe()), _np(a.observe()))
    assert torch.equal(b._state, a._state)          # get_state -> set_state reproduces the words exactly
    for k in range(half, len(acts)):
        out_a, out_b = a.step(acts[k]), b.step(acts[k])
        want = host.step(acts[k])
        assert_step_equal(out_b, want, f"step {k}")
        for x, y in zip(out_a, out_b):
            assert torch.equal(x, y)
        assert torch.equal(a.observe(), b.observe())
    assert_env_equal(game, b, host, "continued")
    fresh = pair(game, dev, n, "uint8", **kw)[0]
    fresh.load_state_dict(fresh.state_dict())          # never started: stays so
    with pytest.raises(RuntimeError, match="reset"):
        fresh.observe()
    with pytest.raises(ValueError, match="n_envs"):
        pair(game, dev, n + 1, "uint8", **kw)[0].load_state_dict(sd)
    with pytest.raises(ValueError, match="seed"):
        pair(game, dev, n, "uint8", seed=1, **kw)[0].load_state_dict(sd)
    # another game's snapshot is refused, either way round
    other = device_class(GAMES[other])(n, game.seed, dev, obs_dtype="uint8", **kw)
    with pytest.raises(ValueError, match="kind"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="kind"):
        b.load_state_dict(other.state_dict())


def iterate(ln, col):
    col.collect_timesteps(RH.N_ENV, ln.agent, ln.experience_buffer)
    ln.cumulative_timesteps += RH.N_ENV
    td = ln.step(RH.N_ENV)
    return td.cpu().clone(), col.envs.get_state()


def save_state_check(game, dev, tmp_path):
    """``Learner.save_state`` carries the environments through the collector's key: 8 iterations after ``load_state`` into a
    fresh learner equal the first learner's 8, TD errors, environments, learner and ring."""
    import torch
    ln, col = learner(game, dev, tmp_path / "a")
    col.collect_timesteps(40, ln.agent, ln.experience_buffer, random=True)
    ln.cumulative_timesteps += 40
    for _ in range(6):
        iterate(ln, col)
    ln.save_state(tmp_path / "snap")
    assert ln._state_part()["collector"]["envs"]["kind"] == game.device
    want = [iterate(ln, col) for _ in range(8)]
    ln2, col2 = learner(game, dev, tmp_path / "b")
    ln2.load_state(tmp_path / "snap")
    got = [iterate(ln2, col2) for _ in range(8)]
    for k, ((td_a, st_a), (td_b, st_b)) in enumerate(zip(want, got)):
        assert torch.equal(td_a.view(torch.int32), td_b.view(torch.int32)), f"iteration {k}: TD errors"
        ref(game).assert_same_state(st_b, st_a, f"iteration {k}")
    RH.assert_same(RH.full_state(ln2), RH.full_state(ln), "resumed")
    RH.assert_same(ring(ln2.experience_buffer), ring(ln.experience_buffer), "ring")
    assert int(col2.envs.get_state()["t"].min()) == (40 + 14 * RH.N_ENV) // RH.N_ENV


# ---------------------------------------------------------------------- no GPU: the host side of the device environment
def native_lib():
    """The body of every host file's ``lib`` fixture."""
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def fake_desc():
    """A descriptor every check accepts, over buffers that do not exist: each case breaks ONE condition, so the call is
    refused before anything touches a device."""
    from prism_amd import _native as N
    d = N.EnvDesc()
    d.n_envs, d.n_actions, d.step_limit, d.obs_kind, d.sticky_p, d.seed = 5, 6, 0, N.OBS_F32, 0.25, 7
    addr = 0x10000000
    for f in ("state", "status", "next_obs", "reward", "done", "truncated"):
        setattr(d, f, addr)
        addr += 0x100000
    d.obs[0], d.obs[1] = addr, addr + 0x100000
    return d


def edit(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _obs(i, v):
    def f(d):
        d.obs[i] = v
    return f


# Breakout's table
ENV_REFUSALS = [
    (None, b"null descriptor"),
    (edit(n_envs=0), b"n_envs must be in [1, 65536]"),
    (edit(n_envs=65537), b"n_envs must be in [1, 65536]"),
    (edit(n_actions=4), b"n_actions must be 3 or 6"),
    (edit(n_actions=0), b"n_actions must be 3 or 6"),
    (edit(step_limit=-1), b"step_limit is negative"),
    (edit(sticky_p=-0.01), b"sticky_p outside [0, 1]"),
    (edit(sticky_p=1.5), b"sticky_p outside [0, 1]"),
    (edit(sticky_p=float("nan")), b"sticky_p outside [0, 1]"),
    (edit(obs_kind=2), b"obs_kind must be"),
    (edit(state=None), b"null state block / status word"),
    (edit(status=None), b"null state block / status word"),
    (_obs(0, None), b"null or shared ping-pong observation buffers"),
    (_obs(1, None), b"null or shared ping-pong observation buffers"),
    (lambda d: _obs(1, d.obs[0])(d), b"null or shared ping-pong observation buffers"),
    (edit(next_obs=None), b"null step outputs"),
    (edit(reward=None), b"null step outputs"),
    (edit(done=None), b"null step outputs"),
    (edit(truncated=None), b"null step outputs"),
    (lambda d: setattr(d, "state", d.state + 4), b"16-byte aligned"),
    (lambda d: _obs(1, d.obs[1] + 8)(d), b"16-byte aligned"),
]


def refusals(game):
    """Breakout's table with the game's action counts: its own text, and the counts ``game.refused`` for Breakout's two."""
    text = b"n_actions must be " + (b"6" if game.minimal == game.full else b"%d or 6" % game.minimal)
    return [(e, t) for e, t in ENV_REFUSALS if b"n_actions" not in t] + [(edit(n_actions=k), text) for k in game.refused]


def env_call(lib, game, entry, p, actions=0x40000000, parity=0):
    """``prism_env_<stem>_reset(p, [first draws,] stream)`` or ``_step(p, actions, u, [draws,] parity, stream)``: no draws given."""
    if entry == "reset":
        return getattr(lib, f"prism_env_{game.stem}_reset")(p, *[None] * game.reset_ptrs, None)
    return getattr(lib, f"prism_env_{game.stem}_step")(p, actions, None, *[None] * game.step_ptrs, parity, None)


def refusal_check(lib, game, entry, case):
    """One refusal of the game's table, with Breakout's text but for the action counts, through the game's entry point."""
    change, text = refusals(game)[case]
    d = fake_desc()
    if change is not None:
        change(d)
    rc = env_call(lib, game, entry, None if change is None else ctypes.byref(d))
    assert rc == -1, (rc, lib.prism_last_error())
    assert b"check_env: " in lib.prism_last_error() and text in lib.prism_last_error(), lib.prism_last_error()


def null_actions_and_parity_check(lib, game):
    d = fake_desc()
    assert env_call(lib, game, "step", ctypes.byref(d), actions=None) == -1
    assert b"prism_env_%s_step: actions is null" % game.stem.encode() in lib.prism_last_error()
    for parity in (2, -1):
        assert env_call(lib, game, "step", ctypes.byref(d), parity=parity) == -1
        assert b"parity must be 0 or 1" in lib.prism_last_error()
    d.n_actions = game.minimal          # the minimal set is accepted as far as the next check
    assert env_call(lib, game, "step", ctypes.byref(d), actions=None) == -1 and b"actions is null" in lib.prism_last_error()


def kernel_segments(game, tmp_path):
    """Compile ``env_<stem>.hip`` for gfx950 as the library's Makefile does and read the code object's metadata: the file
    holds one reset and one step kernel.  -> {kernel: (private segment bytes, group segment bytes)}"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / f"env_{game.stem}.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, f"env_{game.stem}.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S))
    names = [k for k in kernels if f"env_{game.stem}_" in k]
    assert len(names) == 2 and all(sum(f"env_{game.stem}_{e}_kernel" in k for k in names) == 1 for e in ("reset", "step"))
    return {k: tuple(int(re.search(rf"\.amdhsa_{seg}_segment_fixed_size (\d+)", kernels[k]).group(1)) for seg in ("private", "group"))
            for k in names}


def symbols_check(lib, game):
    """Both entry points exported, declared in the header over the shared descriptor and mirrored with the table's draw
    pointers; the 8-word record; the source in the Makefile.  -> (the header's text, ``_native.SIGNATURES``)"""
    from prism_amd import _native as N
    src = open(N.HEADER_PATH).read()
    raw = ctypes.CDLL(N.LIB_PATH)
    for entry, args in (("reset", 2 + game.reset_ptrs), ("step", 5 + game.step_ptrs)):
        name = f"prism_env_{game.stem}_{entry}"
        assert hasattr(raw, name) and re.search(r"\bint " + name + r"\(const prism_env_desc \*d,", src)
        assert N.SIGNATURES[name][1][0] == ctypes.POINTER(N.EnvDesc) and len(N.SIGNATURES[name][1]) == args
    assert f"#define PRISM_ENV_STATE_WORDS {N.ENV_STATE_WORDS}" in src and N.ENV_STATE_WORDS == 8
    makefile = open(os.path.join(H.ROOT, "prism_amd", "csrc", "Makefile")).read()
    assert f"env_{game.stem}.hip" in re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    return src, N.SIGNATURES


def sticky_coin_check(game, steps, free_steps):
    """Over ``steps`` steps of 8 environments at p = 0.25 the repeats are the coins below p, t running on through the episode
    ends; the coin is the 53-bit uniform of words 0, 1 under the game's coin key; at p = 0 no action ever repeats."""
    R = ref(game)
    seed, n = 99, 8
    host = host_class(game)(n, seed=seed, sticky_action_prob=0.25)
    host.reset()
    for _ in range(steps):
        host.step(np.zeros(n, np.int64))
    coins = np.array([R.coin(seed, e, t) for e in range(n) for t in range(steps)])
    assert 0.0 <= coins.min() and coins.max() < 1.0
    r = H.philox4x32(seed, np.array([17], np.uint64), (3 << 32) | R.KEY_COIN)[0]
    assert R.coin(seed, 3, 17) == R.unit_double(r[0], r[1])
    assert host.branches["sticky_repeat"] == int((coins < 0.25).sum())
    host = host_class(game)(n, seed=seed, sticky_action_prob=0.0)
    host.reset()
    rng = np.random.default_rng(0)
    for _ in range(free_steps):
        acts = rng.integers(0, 6, n)
        host.step(acts)
        assert [e["last_action"] for e in host.envs] == list(acts)
    assert host.branches["sticky_repeat"] == 0


def fake_device_classes(monkeypatch, game, kinds):
    """Put a class that only records its construction in place of ``envs.Device<kind>`` for every kind (each with the game's
    observation shape and minimal action count).  -> the list of (kind, args, kwargs) they append to"""
    from prism_amd import envs
    made = []

    def fake(kind):
        class Fake:
            obs_shape, n_actions = game.obs_shape, game.minimal

            def __init__(self, *a, **kw):
                made.append((kind, a, kw))
        return Fake

    for kind in kinds:
        monkeypatch.setattr(envs, "Device" + kind, fake(kind))
    return made


def bare(cls, n_actions=6):
    """A device environment with everything a device would need taken away: ``load_state_dict`` checks first."""
    env = cls.__new__(cls)
    env.__dict__.update(dict(_name=cls.__name__, n_envs=4, n_actions=n_actions, seed=9, _started=False))
    return env


def snap(kind, n_actions=6, words=8):
    import torch
    return dict(kind=kind, n_envs=4, n_actions=n_actions, seed=9, started=False, state=torch.zeros((4, words), dtype=torch.int32))
