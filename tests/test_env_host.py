"""No GPU needed: the Breakout rules on ``HostBreakout`` (tests/env_ref.py) alone -- the case table reaches every branch,
invariants hold over seeded random play, the draws sit where DESIGN.md 7.3 puts them -- and the host side of the device
environment: argument checks of the two entry points through the C ABI, the descriptor mirror, the state codec, the
factories."""
import ctypes
import os

import numpy as np
import pytest

from tests import env_cases as EC
from tests import game_suite as GS
from tests import helpers as H
from tests.env_frame_cases import GAMES
from tests.env_ref import BRANCHES, ENV_KEY, FIRST_COUNTER, HostBreakout, draw, unit_double

GAME = GAMES["breakout"]


def run_case(name):
    c = EC.CASES[name]
    host = HostBreakout(1, seed=1, **EC.GROUPS[c["group"]])
    host.set_state({k: [v] for k, v in c["state"].items()})
    out = []
    for a, u, side in c["script"]:
        out.append(host.step([a], u=[u], side=[side]))
    return host, out


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_case_reaches_its_branches(name):
    host, _ = run_case(name)
    for b in EC.CASES[name]["reach"]:
        assert host.branches[b] > 0, (name, b, host.branches)
    assert host.bad_action == bool(EC.CASES[name].get("bad_action", False))


def test_case_table_covers_every_branch():
    total = {b: 0 for b in BRANCHES}
    for name in EC.CASES:
        host, _ = run_case(name)
        for b, k in host.branches.items():
            total[b] += k
    assert all(total[b] > 0 for b in EC.REQUIRED), total
    assert all(total[b] > 0 for b in BRANCHES), total          # (and the bookkeeping ones: moves, bad action)
    for g in EC.GROUPS:
        assert len(EC.group_cases(g)) >= 2


def test_cases_in_detail():
    """What the crafted cases are for, step by step."""
    host, out = run_case("pass_through")
    rewards = [float(o[1][0]) for o in out]
    assert rewards == [1.0, 0.0, 0.0, 0.0]                     # the second brick is passed, not taken
    assert host.envs[0]["bricks"].sum() == 1 and host.envs[0]["bricks"][3, 4] == 1
    host, out = run_case("refill")
    assert host.envs[0]["bricks"][1:4].all() and sum(float(o[1][0]) for o in out) == 1.0
    assert host.envs[0]["ball_y"] < 9 and not any(o[2][0] for o in out)
    host, out = run_case("limit_on_a_miss")
    assert [(int(o[2][0]), int(o[3][0])) for o in out[:2]] == [(0, 0), (1, 0)]          # done on the limit's step: not truncated
    host, out = run_case("truncation")
    assert [int(o[3][0]) for o in out] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0]
    assert [int(o[2][0]) for o in out] == [0] * 12
    # the image a step returns is the one BEFORE the reset; the next acting image is the fresh episode's
    assert out[4][0][0, 8, 5, 1] == 1 and host.envs[0]["ep_steps"] == 2
    host, out = run_case("sticky")
    # (l, u = 0.1: repeats r) (l, u = 0.25: not below p) (n, u = 0.2499: repeats l) (r, u = 0: repeats l) (r)
    assert host.branches["sticky_repeat"] == 3 and host.envs[0]["pos"] == 4 + 1 - 1 - 1 - 1 + 1
    host, out = run_case("miss_then_side_1")
    e = host.envs[0]
    assert e["t"] == 123456789012 + 11 and e["ep_steps"] == 9          # t carries over the reset, ep_steps does not
    host, out = run_case("minimal_out_of_range")
    assert host.envs[0]["pos"] == 6                                    # r, (3: no-op), r


def _play(seed, n=17, steps=300, **kw):
    rng = np.random.default_rng(seed)
    host = HostBreakout(n, seed=seed, **kw)
    host.reset()
    for k in range(steps):
        st = host.get_state()
        track = np.where(st["ball_x"] < st["pos"], 1, np.where(st["ball_x"] > st["pos"], 3, 0))
        acts = np.where(rng.random(n) < 0.5, track, rng.integers(0, 6, n))
        yield host, st, acts, host.step(acts)


def test_invariants_over_seeded_random_play():
    ends = 0
    for host, before, acts, (next_obs, reward, done, trunc) in _play(11, sticky_action_prob=0.1, episode_timestep_limit=25):
        after_img = next_obs
        assert set(np.unique(reward)) <= {0.0, 1.0}
        assert set(np.unique(next_obs)) <= {0.0, 1.0}
        # one paddle cell in row 9, one ball cell, one last-ball cell, bricks in rows 1..3 only
        assert (after_img[..., 0].sum(axis=(1, 2)) == 1).all() and (after_img[:, :9, :, 0] == 0).all()
        assert (after_img[..., 1].sum(axis=(1, 2)) == 1).all() and (after_img[..., 2].sum(axis=(1, 2)) == 1).all()
        assert (after_img[:, 0, :, 3] == 0).all() and (after_img[:, 4:, :, 3] == 0).all()
        # reward equals bricks removed (a refill, which only happens on an empty board, aside)
        b0, b1 = before["bricks"].sum(axis=(1, 2)), after_img[..., 3].sum(axis=(1, 2))
        refilled = (b1 == 30) & (b0 <= 1)
        np.testing.assert_array_equal(np.where(refilled, reward, b0 - b1), reward)
        st = host.get_state()
        for f in ("ball_x", "ball_y", "last_x", "last_y", "pos"):
            assert st[f].min() >= 0 and st[f].max() <= 9
        assert not (done & trunc).any()
        ends += int(done.sum() + trunc.sum())
    assert ends > 20
    assert all(host.branches[b] > 0 for b in ("wall", "strike", "paddle_under", "miss", "truncation", "sticky_repeat"))


def test_draws_stream_key_and_counters():
    """The coin and side of environment e at lifetime step t are Philox(seed)(t, (e << 32) | "ENVB"); the first side is
    word 3 of the draw at counter 2^64 - 1."""
    assert ENV_KEY == int.from_bytes(b"ENVB", "big")
    seed = 0x1234567890ABCDEF
    host = HostBreakout(6, seed=seed, sticky_action_prob=1.0)
    host.reset()
    for i, e in enumerate(host.envs):
        side = int(H.philox4x32(seed, np.array([FIRST_COUNTER], np.uint64), (i << 32) | ENV_KEY)[0, 3]) & 1
        assert (e["ball_x"], e["ball_dir"]) == ((0, 2) if side == 0 else (9, 3))
        assert e["t"] == 0 and e["last_action"] == 0
    # environments draw apart from each other and from step to step
    words = {tuple(draw(seed, e, t)) for e in range(6) for t in range(5)}
    assert len(words) == 30
    # sticky_p = 1: every coin is below it, the first action (no-op) repeats for ever
    for _ in range(20):
        host.step(np.full(6, 1))
    assert all(e["last_action"] == 0 and e["pos"] == 4 for e in host.envs)
    # the side of the episode a miss begins is word 2 of the draw AT the step that ended it
    host = HostBreakout(4, seed=seed)
    host.reset()
    seen = 0
    for _ in range(40):
        t0 = [e["t"] for e in host.envs]
        _, _, done, _ = host.step(np.zeros(4, np.int64))
        for i in np.nonzero(done)[0]:
            side = int(draw(seed, i, t0[i])[2]) & 1
            assert host.envs[i]["ball_x"] == (0 if side == 0 else 9) and host.envs[i]["ep_steps"] == 0
            seen += 1
    assert seen >= 4


def test_sticky_coin_frequency_and_zero_never_repeats():
    seed, n, steps = 99, 8, 500
    coins = np.array([unit_double(*draw(seed, e, t)[:2]) for e in range(n) for t in range(steps)])
    assert 0.0 <= coins.min() and coins.max() < 1.0
    p = 0.25
    # 4000 Bernoulli(0.25) draws: standard deviation 0.0068; five of them
    assert abs((coins < p).mean() - p) < 5 * np.sqrt(p * (1 - p) / coins.size)
    host = HostBreakout(n, seed=seed, sticky_action_prob=p)
    host.reset()
    for _ in range(steps):
        host.step(np.zeros(n, np.int64))
    assert host.branches["sticky_repeat"] == int((coins < p).sum())
    host = HostBreakout(n, seed=seed, sticky_action_prob=0.0)
    host.reset()
    rng = np.random.default_rng(0)
    for _ in range(200):
        acts = rng.integers(0, 6, n)
        host.step(acts)
        assert [e["last_action"] for e in host.envs] == list(acts)
    assert host.branches["sticky_repeat"] == 0


# ---------------------------------------------------------------------- the host side of the device environment
@pytest.fixture(scope="module")
def lib():
    return GS.native_lib()


@pytest.mark.parametrize("entry", ["reset", "step"])
@pytest.mark.parametrize("case", range(len(GS.refusals(GAME))))
def test_env_refusals_without_device(lib, entry, case):
    """Every refusal of the table (tests/game_suite.py ENV_REFUSALS: the other games derive theirs from it)."""
    GS.refusal_check(lib, GAME, entry, case)


def test_step_refuses_null_actions_and_bad_parity(lib):
    GS.null_actions_and_parity_check(lib, GAME)


def test_descriptor_mirror_layout():
    from prism_amd import _native as N
    D = N.EnvDesc
    assert ctypes.sizeof(D) == 4 * 4 + 8 + 8 + 2 * 8 + 2 * 8 + 8 + 8 + 2 * 8
    want = dict(n_envs=0, n_actions=4, step_limit=8, obs_kind=12, sticky_p=16, seed=24, state=32, status=40, obs=48, next_obs=64,
                reward=72, done=80, truncated=88)
    assert {f: getattr(D, f).offset for f, _ in D._fields_} == want
    src = open(os.path.join(H.ROOT, "include", "prism_hip.h")).read()
    assert f"#define PRISM_ENV_STATE_WORDS {N.ENV_STATE_WORDS}" in src and f"#define PRISM_ENV_MAX {N.ENV_MAX}" in src
    assert f"#define PRISM_ENV_STATUS_BAD_ACTION {N.ENV_STATUS_BAD_ACTION}u" in src


def test_state_codec_round_trips():
    from prism_amd.envs import pack_state, render, unpack_state
    for group in EC.GROUPS:
        state, _, _, _ = EC.vector(group, 11)
        words = pack_state(state)
        assert words.shape == (11, 8) and words.dtype == np.int32
        back = unpack_state(words)
        for k in state:
            np.testing.assert_array_equal(np.asarray(back[k]).astype(np.uint64), np.asarray(state[k]).astype(np.uint64), err_msg=k)
        host = HostBreakout(11)
        host.set_state(state)
        np.testing.assert_array_equal(render(state).astype(np.float32), host.observe())
    bad = EC.vector("plain", 2)[0]
    bad["pos"] = np.array([4, 10])
    with pytest.raises(ValueError, match="pos"):
        pack_state(bad)
    bad = EC.vector("plain", 2)[0]
    bad["bricks"][1, 5, 0] = 1
    with pytest.raises(ValueError, match="rows 1..3"):
        pack_state(bad)


def test_factories_names_accepted_and_refused(monkeypatch):
    from prism_amd import envs
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.factory import collector_factory, env_factory
    made = []

    class Fake:
        obs_shape, n_actions = (10, 10, 4), 6

        def __init__(self, *a, **kw):
            made.append((a, kw))

    monkeypatch.setattr(envs, "DeviceBreakout", Fake)
    cfg = baseline_config(2, device="cuda:0", env_name="MinAtar/Breakout-v1", atari_sticky_actions_prob=0.1, num_processes=9,
                          seed=31, episode_timestep_limit=777)
    assert isinstance(env_factory.build_environment(cfg, 5), Fake)
    (a, kw), = made
    assert a == (5, 31, "cuda:0") and kw == dict(sticky_action_prob=0.1, episode_timestep_limit=777, minimal_actions=True)
    cfg.env_name = "MinAtar/Breakout-v0"
    env_factory.build_environment(cfg, 3, seed=8)
    assert made[-1][0] == (3, 8, "cuda:0") and made[-1][1]["minimal_actions"] is False
    col = collector_factory.build_collector(cfg)
    assert isinstance(col, VectorCollector) and isinstance(col.envs, Fake) and made[-1][0][0] == 9
    for game in ("Asterix", "Freeway", "Seaquest", "SpaceInvaders"):
        cfg.env_name = f"MinAtar/{game}-v1"
        with pytest.raises(NotImplementedError, match=game):
            env_factory.build_environment(cfg, 4)
    for name in ("ALE/Defender-v5", "LunarLander-v2", "MinAtar/Pong-v1", "Breakout-v1"):
        cfg.env_name = name
        with pytest.raises(ValueError):
            env_factory.build_environment(cfg, 4)


def test_collector_snapshot_gains_envs_key_only_with_a_state_dict():
    from prism_amd.collectors import VectorCollector

    class Plain:
        obs_shape, n_actions = (10, 10, 4), 6

    class Stateful(Plain):
        def __init__(self):
            self.loaded = None

        def state_dict(self):
            return {"k": 5}

        def load_state_dict(self, st):
            self.loaded = st

    cfg = type("C", (), dict(seed=3, training_reward_ema=0.9))()
    plain = VectorCollector(Plain(), cfg).state_dict()
    assert sorted(plain) == ["rng", "rows", "started"]
    col = VectorCollector(Stateful(), cfg)
    st = col.state_dict()
    assert sorted(st) == ["envs", "rng", "rows", "started"] and st["envs"] == {"k": 5}
    assert {k: st[k] for k in plain} == plain
    col2 = VectorCollector(Stateful(), cfg)
    col2.load_state_dict(st)
    assert col2.envs.loaded == {"k": 5}
    VectorCollector(Plain(), cfg).load_state_dict(st)          # environments that cannot restore: the key is ignored
    col3 = VectorCollector(Stateful(), cfg)
    col3.load_state_dict(plain)                                # an older snapshot: nothing to restore
    assert col3.envs.loaded is None
