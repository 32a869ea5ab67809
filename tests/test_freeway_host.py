"""No GPU needed: the Freeway rules on ``HostFreeway`` (tests/freeway_ref.py) alone -- the case table reaches every branch,
invariants hold over seeded play, the draws sit where DESIGN.md 7.4 puts them -- and the host side of the device
environment: the two entry points through the C ABI, their kernels' private segment, the state codec, the factory knob, the
snapshot kinds."""
import os
import re

import numpy as np
import pytest

from tests import freeway_cases as FC
from tests import game_suite as GS
from tests import helpers as H
from tests.env_frame_cases import GAMES
from tests.freeway_ref import BRANCHES, FIRST_COUNTER, KEY_COIN, KEYS_RESET, KEYS_WIN, HostFreeway, draw, draw_speeds, speed_of_word

GAME = GAMES["freeway"]          # its seed and Philox-path run are tests/test_gpu_freeway.py's: kept where no GPU is needed


def run_case(name):
    c = FC.CASES[name]
    host = HostFreeway(1, seed=1, **FC.GROUPS[c["group"]])
    host.set_state({k: [v] for k, v in c["state"].items()})
    out, states = [], []
    for a, u, speeds in c["script"]:
        out.append(host.step([a], u=[u], speeds=[speeds]))
        states.append({k: v[0].copy() for k, v in host.get_state().items()})
    return host, out, states


@pytest.mark.parametrize("name", sorted(FC.CASES))
def test_case_reaches_its_branches(name):
    host, _, _ = run_case(name)
    for b in FC.CASES[name]["reach"]:
        assert host.branches[b] > 0, (name, b, host.branches)
    assert host.bad_action == bool(FC.CASES[name].get("bad_action", False))


def test_case_table_covers_every_branch_speed_and_channel():
    total = {b: 0 for b in BRANCHES}
    speeds_seen, channels, trail_columns = set(), np.zeros(7, np.int64), set()
    for name in FC.CASES:
        host, out, states = run_case(name)
        for b, k in host.branches.items():
            total[b] += k
        for (next_obs, _, _, _), st in zip(out, states):
            channels += next_obs[0].sum(axis=(0, 1)).astype(np.int64)
            trail_columns |= {(int(x), int(np.sign(v))) for x, v in zip(st["car_x"], st["car_speed"])}
        speeds_seen |= {int(v) for st in states for v in st["car_speed"]}
    assert set(FC.REQUIRED) == set(BRANCHES) and all(total[b] > 0 for b in BRANCHES), total
    assert speeds_seen == {s * m for s in (1, -1) for m in range(1, 6)}          # every |speed| in both directions
    assert (channels > 0).all(), channels
    assert (0, 1) in trail_columns and (9, -1) in trail_columns                  # the trail cell wraps at x = 0 and at x = 9
    for g in FC.GROUPS:
        assert len(FC.group_cases(g)) >= 2
    assert any(int(c["state"]["t"]) < 2 ** 32 <= int(c["state"]["t"]) + len(c["script"]) for c in FC.CASES.values())


def test_cases_in_detail():
    """What the crafted cases are for, step by step."""
    host, out, states = run_case("move_gating")
    assert [int(s["pos"]) for s in states] == [5, 5, 5, 4, 4, 4, 5]          # refused at 3, 2, 1, accepted at 0; d the same
    assert [int(s["move_timer"]) for s in states] == [2, 1, 0, 2, 1, 0, 2]
    assert host.branches["move_refused"] == 5
    host, out, states = run_case("clamp_bottom")
    assert (int(states[0]["pos"]), int(states[0]["move_timer"])) == (9, 2)   # the clamped move still starts the timer
    for name, x_after in (("hit_before_move", 5), ("hit_after_move_right", 4), ("hit_after_move_left", 4), ("hit_waiting_car", 4)):
        host, out, states = run_case(name)
        row = int(FC.CASES[name]["state"]["pos"])
        assert int(states[0]["pos"]) == 9 and int(states[0]["car_x"][row - 1]) == x_after, name
        assert float(out[0][1][0]) == 0.0 and not out[0][2][0]
    host, out, states = run_case("walk_into_a_car")
    assert int(states[0]["pos"]) == 9 and host.branches["hit_waiting_car"] == 1
    host, out, states = run_case("wraps")
    assert list(states[0]["car_x"]) == [0, 9] * 4                            # 9 -> 0 and 0 -> 9
    img = out[0][0][0]
    assert img[1, 9, 2] == 1 and img[2, 0, 2] == 1                           # their trail cells: 0 - 1 -> 9, 9 + 1 -> 0
    assert int(states[-1]["t"]) == 2 ** 32 + 2
    host, out, states = run_case("win")
    assert [float(o[1][0]) for o in out] == [1.0, 0.0, 0.0, 0.0] and not any(o[2][0] or o[3][0] for o in out)
    assert list(states[0]["car_speed"]) == FC.FAST and int(states[0]["pos"]) == 9
    assert list(states[0]["car_x"]) == [1, 2, 3, 5, 6, 7, 8, 9]              # x kept (timer = |speed| >= 3: nobody moved yet)
    assert list(states[0]["car_timer"]) == [abs(v) - 1 for v in FC.FAST]     # timer = |speed|, then the cars' own step
    host, out, states = run_case("win_on_the_last_step")
    next_obs, reward, done, trunc = out[0]
    assert (float(reward[0]), int(done[0]), int(trunc[0])) == (1.0, 1, 0)
    want = np.zeros((10, 10, 7), np.float32)                                 # the returned image: the win's speeds, x kept
    want[9, 4, 0] = 1
    for i, v in enumerate(FC.SLOW):
        want[i + 1, 6, 1] = 1
        want[i + 1, 6 - int(np.sign(v)), 1 + abs(v)] = 1
    np.testing.assert_array_equal(next_obs[0], want)
    assert int(states[0]["ep_steps"]) == 0 and int(states[0]["t"]) == 123456789013 and list(states[0]["car_x"]) == [0] * 8
    assert int(states[0]["terminate_timer"]) == 2500 and int(states[0]["move_timer"]) == 3
    host, out, states = run_case("terminal_from_0")
    assert [int(o[2][0]) for o in out] == [1, 0, 0, 0, 0] and list(states[0]["car_speed"]) == FC.FAST
    host, out, states = run_case("terminal_from_1")
    assert [int(o[2][0]) for o in out] == [0, 1, 0, 0, 0] and int(states[0]["terminate_timer"]) == 0
    host, out, states = run_case("limit_on_a_terminal")
    assert [(int(o[2][0]), int(o[3][0])) for o in out[:2]] == [(0, 0), (1, 0)]          # done on the limit's step: not truncated
    host, out, states = run_case("truncation")
    assert [int(o[3][0]) for o in out] == [0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0] and [int(o[2][0]) for o in out] == [0] * 12
    assert list(states[4]["car_speed"]) == FC.FAST and list(states[9]["car_speed"]) == FC.SLOW and int(states[-1]["ep_steps"]) == 2
    host, out, states = run_case("sticky")
    # (u, 0.1: repeats d) (u, 0.25: not below p, refused) (n, 0.2499: repeats u, refused) (d, 0: repeats u) (d: refused)
    assert host.branches["sticky_repeat"] == 3 and [int(s["pos"]) for s in states] == [6, 6, 6, 5, 5]
    host, out, states = run_case("minimal_moves")
    assert [int(s["pos"]) for s in states] == [4, 4, 4, 5] and [int(s["last_action"]) for s in states] == [2, 0, 0, 4]
    host, out, states = run_case("minimal_out_of_range")
    assert [int(s["pos"]) for s in states] == [6, 6, 6, 7] and host.branches["bad_action"] == 2
    host, out, states = run_case("unused_actions")
    assert [int(s["pos"]) for s in states] == [5, 5, 5, 4] and host.branches["unused_action"] == 3


def test_an_untouched_episode_lasts_2501_steps():
    host = HostFreeway(1, seed=5)
    host.reset()
    done_at = [k for k in range(2600) if host.step([0])[2][0]]
    assert done_at == [2500] and host.envs[0]["ep_steps"] == 99 and host.envs[0]["t"] == 2600


def check_image(img, st, where):
    """One chicken, eight cars, eight trails, each trail in the channel of its car's speed and behind it."""
    assert set(np.unique(img)) <= {0.0, 1.0}, where
    assert img[..., 0].sum() == 1 and img[int(st["pos"]), 4, 0] == 1, where
    assert img[..., 1].sum() == 8 and img[..., 2:].sum() == 8, where
    assert img[0].sum() == (st["pos"] == 0) and img[9].sum() == (st["pos"] == 9), where          # no car on rows 0 and 9
    for i in range(8):
        x, v = int(st["car_x"][i]), int(st["car_speed"][i])
        assert img[i + 1, x, 1] == 1 and img[i + 1, (x - np.sign(v)) % 10, 1 + abs(v)] == 1, (where, i)
        assert 0 <= x <= 9 and 1 <= abs(v) <= 5 and 0 <= int(st["car_timer"][i]) <= abs(v), (where, i)


def test_invariants_over_seeded_play():
    n, steps = 6, 700
    rng = np.random.default_rng(11)
    host = HostFreeway(n, seed=11, sticky_action_prob=0.1, episode_timestep_limit=150)
    host.reset()
    ends = wins = 0
    for k in range(steps):
        acts = np.where(rng.random(n) < 0.8, 2, rng.integers(0, 6, n))
        next_obs, reward, done, trunc = host.step(acts)
        assert set(np.unique(reward)) <= {0.0, 1.0} and not (done & trunc).any()
        st = host.get_state()
        acting = host.observe()
        for i in range(n):
            one = {f: st[f][i] for f in st}
            check_image(acting[i], one, f"step {k}, env {i}")
            assert 0 <= one["pos"] <= 9 and 0 <= one["move_timer"] <= 3 and 0 <= one["terminate_timer"] <= 2500
            if not (done[i] or trunc[i]):
                np.testing.assert_array_equal(next_obs[i], acting[i])
            else:
                assert next_obs[i][..., 0].sum() == 1 and next_obs[i][..., 1].sum() == 8 and next_obs[i][..., 2:].sum() == 8
        ends += int(done.sum() + trunc.sum())
        wins += int(reward.sum())
    assert n * steps >= 4000 and ends >= 20 and wins >= 10
    for b in ("move_up", "move_refused", "win", "truncation", "sticky_repeat", "reset", "wrap_right", "wrap_left"):
        assert host.branches[b] > 0, b
    assert sum(host.branches[b] for b in BRANCHES if b.startswith("hit_")) > 0


def test_draws_stream_keys_and_counters():
    """The coin of environment e at lifetime step t is words 0, 1 of Philox(seed)(t, (e << 32) | "FWYC"); the win set is the
    draws under "FWW0", "FWW1" and the reset set those under "FWR0", "FWR1" at the same counter; the first episode's speeds
    are the reset set at counter 2^64 - 1."""
    keys = dict(FWYC=KEY_COIN, FWW0=KEYS_WIN[0], FWW1=KEYS_WIN[1], FWR0=KEYS_RESET[0], FWR1=KEYS_RESET[1])
    for text, key in keys.items():
        assert key == int.from_bytes(text.encode(), "big")
    # no two streams share a key: the four-character keys of csrc/, and TAU0 + sid for every stream id below 2^16
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            found += [int(m, 16) for m in re.findall(r"0x([0-9A-Fa-f]{8})ull", open(os.path.join(csrc, name)).read())]
    ours = sorted(keys.values())
    assert all(found.count(k) == 1 for k in ours), "a Freeway key appears twice in csrc/"
    tau0 = int.from_bytes(b"TAU0", "big")
    assert tau0 in found and all(not tau0 <= k < tau0 + 2 ** 16 for k in ours)
    for k in (b"PERM", b"UNIF", b"IDSA", b"EGRD", b"ENVB"):
        assert int.from_bytes(k, "big") in set(found) - set(ours)
    seed = 0x1234567890ABCDEF
    host = HostFreeway(6, seed=seed, sticky_action_prob=1.0)
    host.reset()
    for i, e in enumerate(host.envs):
        words = [w for key in KEYS_RESET for w in H.philox4x32(seed, np.array([FIRST_COUNTER], np.uint64), (i << 32) | key)[0]]
        assert e["car_speed"] == [speed_of_word(w) for w in words] == draw_speeds(seed, i, FIRST_COUNTER, KEYS_RESET)
        assert e["car_timer"] == [abs(v) for v in e["car_speed"]] and e["car_x"] == [0] * 8
        assert (e["t"], e["last_action"], e["pos"], e["move_timer"], e["terminate_timer"]) == (0, 0, 9, 3, 2500)
    words = {tuple(draw(seed, e, t, key)) for e in range(6) for t in range(5) for key in keys.values()}
    assert len(words) == 6 * 5 * 5                                             # apart by environment, step and purpose
    # sticky_p = 1: every coin is below it, the first action (no-op) repeats for ever
    for _ in range(20):
        host.step(np.full(6, 2))
    assert all(e["last_action"] == 0 and e["pos"] == 9 for e in host.envs)
    # a win installs the win set of the draw AT that step; a truncation the reset set of the draw at its step
    host = HostFreeway(4, seed=seed, episode_timestep_limit=60)
    host.reset()
    wins = ends = 0
    for _ in range(130):
        t0 = [e["t"] for e in host.envs]
        before = [list(e["car_speed"]) for e in host.envs]
        _, reward, done, trunc = host.step(np.full(4, 2))
        for i in range(4):
            if trunc[i]:
                assert host.envs[i]["car_speed"] == draw_speeds(seed, i, t0[i], KEYS_RESET) and host.envs[i]["ep_steps"] == 0
                ends += 1
            elif reward[i]:
                assert host.envs[i]["car_speed"] == draw_speeds(seed, i, t0[i], KEYS_WIN)
                wins += 1
            else:
                assert host.envs[i]["car_speed"] == before[i]
    assert wins >= 2 and ends == 8


def test_speed_map_frequencies_and_edges():
    """|speed| = 1 + floor(5 (w >> 1) / 2^31) with direction w & 1: the edges of the map, and over 40 000 car words each of
    the ten (speed, direction) outcomes within 6 binomial sigma of a tenth (the map's own bias, (2^31 mod 5) / 2^31 ~ 1e-9,
    is far below that)."""
    assert [speed_of_word(w) for w in (0, 1, 2 ** 32 - 1, 2 ** 32 - 2)] == [-1, 1, 5, -5]
    edges = [-(-k * 2 ** 31 // 5) for k in range(1, 5)]                        # the first w >> 1 of |speed| = k + 1
    for k, e in enumerate(edges, 1):
        assert speed_of_word((e << 1) | 1) == k + 1 and speed_of_word(((e - 1) << 1) | 1) == k
    seed = 77
    speeds = np.array([v for e in range(50) for t in range(100) for v in draw_speeds(seed, e, t, KEYS_WIN)])
    assert speeds.size == 40000
    sigma = np.sqrt(0.1 * 0.9 / speeds.size)
    for s in (1, -1):
        for m in range(1, 6):
            assert abs((speeds == s * m).mean() - 0.1) < 6 * sigma, (s * m, (speeds == s * m).mean())


def test_sticky_coin_counts_and_zero_never_repeats():
    GS.sticky_coin_check(GAME, steps=300, free_steps=100)


def test_the_philox_script_of_the_gpu_test_shows_a_win():
    """tests/test_gpu_freeway.py's Philox-path run (its seed, hold u, 200 steps at N = 5, sticky_p = 0.25) has a win on
    ``HostFreeway`` alone."""
    host, (wins, _, _) = GS.philox_host_run(GAME)
    assert wins >= 1 and host.branches["sticky_repeat"] > 100 and host.branches["truncation"] >= 5


# ---------------------------------------------------------------------- the host side of the device environment
@pytest.fixture(scope="module")
def lib():
    return GS.native_lib()


def test_symbols_exported_declared_and_mirrored(lib):
    src, signatures = GS.symbols_check(lib, GAME)
    assert signatures["prism_env_freeway_reset"] == signatures["prism_env_breakout_reset"]
    assert signatures["prism_env_freeway_step"] == signatures["prism_env_breakout_step"]
    assert "const int8_t *first_speeds_in" in src and "const int8_t *speeds_in" in src


@pytest.mark.parametrize("entry", ["reset", "step"])
@pytest.mark.parametrize("case", range(len(GS.refusals(GAME))))
def test_env_refusals_without_device(lib, entry, case):
    """Every refusal of Breakout's table, with the same text, through Freeway's entry points."""
    GS.refusal_check(lib, GAME, entry, case)


def test_step_refuses_null_actions_and_bad_parity(lib):
    GS.null_actions_and_parity_check(lib, GAME)


def test_the_kernels_have_no_private_segment(tmp_path):
    """Read from the code object's metadata of env_freeway.hip (the cars are looked up by a lane's row: an array would land
    in the private segment); no group segment either."""
    assert set(GS.kernel_segments(GAME, tmp_path).values()) == {(0, 0)}


def test_state_codec_round_trips_and_refuses():
    from prism_amd.envs import pack_freeway_state, render_freeway, unpack_freeway_state
    for group in FC.GROUPS:
        state, _, _, _ = FC.vector(group, 15)
        words = pack_freeway_state(state)
        assert words.shape == (15, 8) and words.dtype == np.int32 and not words[:, 7].any()
        back = unpack_freeway_state(words)
        assert sorted(back) == sorted(state)
        for k in state:
            np.testing.assert_array_equal(np.asarray(back[k]).astype(np.int64), np.asarray(state[k]).astype(np.int64), err_msg=k)
        host = HostFreeway(15)
        host.set_state(state)
        np.testing.assert_array_equal(render_freeway(state).astype(np.float32), host.observe())
    # ep_steps and t sit where Breakout keeps them
    state = FC.vector("plain", 3)[0]
    state["ep_steps"], state["t"] = np.array([1, 2, 3]), np.array([2 ** 40 + 5, 6, 2 ** 64 - 1], dtype=np.uint64)
    w = pack_freeway_state(state).view(np.uint32)
    assert list(w[:, 2]) == [1, 2, 3] and list(w[:, 4]) == [5, 6, 2 ** 32 - 1] and list(w[:, 5]) == [256, 0, 2 ** 32 - 1]
    for field, value, text in (("pos", 10, "pos"), ("move_timer", 4, "move_timer"), ("terminate_timer", 2501, "terminate_timer"),
                               ("last_action", 6, "last_action"), ("pos", -1, "pos")):
        bad = FC.vector("plain", 2)[0]
        bad[field] = np.array([0, value])
        with pytest.raises(ValueError, match=text):
            pack_freeway_state(bad)
    for field, value, text in (("car_x", 10, "car_x"), ("car_timer", 6, "car_timer"), ("car_speed", 0, "car_speed"),
                               ("car_speed", 6, "car_speed"), ("car_speed", -6, "car_speed"), ("car_x", -1, "car_x")):
        bad = FC.vector("plain", 2)[0]
        bad[field][1, 7] = value
        with pytest.raises(ValueError, match=text):
            pack_freeway_state(bad)


def test_breakout_names_of_the_module_mean_what_they_meant():
    from prism_amd import envs
    assert envs.OBS_SHAPE == (10, 10, 4) and envs.FREEWAY_OBS_SHAPE == (10, 10, 7)
    assert envs.DeviceBreakout.OBS_SHAPE == (10, 10, 4) and envs.DeviceFreeway.OBS_SHAPE == (10, 10, 7)
    assert issubclass(envs.DeviceBreakout, envs._DeviceEnv) and issubclass(envs.DeviceFreeway, envs._DeviceEnv)
    for shared in ("observe", "close", "check_status", "get_state", "set_state", "state_dict", "load_state_dict", "_stage_actions"):
        assert getattr(envs.DeviceBreakout, shared) is getattr(envs.DeviceFreeway, shared) is getattr(envs._DeviceEnv, shared)
    assert envs.DeviceBreakout._pack is envs.pack_state and envs.DeviceFreeway._pack is envs.pack_freeway_state
    assert envs.DeviceBreakout._render is envs.render and envs.DeviceFreeway._render is envs.render_freeway
    with pytest.raises(ValueError, match="speeds must be"):
        envs.DeviceFreeway._speeds(np.zeros((2, 8), np.int8))


def test_factory_knob_off_on_and_bad(monkeypatch):
    from prism_amd import envs
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.factory import collector_factory, env_factory
    made = GS.fake_device_classes(monkeypatch, GAME, ("Freeway", "Breakout"))
    cfg = baseline_config(2, device="cuda:0", env_name="MinAtar/Freeway-v1", atari_sticky_actions_prob=0.1, num_processes=9,
                          seed=31, episode_timestep_limit=777)
    # the knob off: refused as before, and the text says how to enable the game
    with pytest.raises(NotImplementedError, match="Freeway.*device_env_games"):
        env_factory.build_environment(cfg, 5)
    with pytest.raises(NotImplementedError, match="Freeway"):
        collector_factory.build_collector(cfg)
    cfg.device_env_games = ("Breakout",)
    with pytest.raises(NotImplementedError, match="Freeway"):
        env_factory.build_environment(cfg, 5)
    assert made == []
    # the knob on
    cfg.device_env_games = ("Breakout", "Freeway")
    assert isinstance(env_factory.build_environment(cfg, 5), envs.DeviceFreeway)
    assert made == [("Freeway", (5, 31, "cuda:0"), dict(sticky_action_prob=0.1, episode_timestep_limit=777, minimal_actions=True))]
    cfg.env_name = "MinAtar/Freeway-v0"
    env_factory.build_environment(cfg, 3, seed=8)
    assert made[-1][:2] == ("Freeway", (3, 8, "cuda:0")) and made[-1][2]["minimal_actions"] is False
    col = collector_factory.build_collector(cfg)
    assert isinstance(col, VectorCollector) and isinstance(col.envs, envs.DeviceFreeway) and made[-1][1][0] == 9
    cfg.env_name = "MinAtar/Breakout-v1"
    env_factory.build_environment(cfg, 4)
    assert made[-1][0] == "Breakout"
    for game in ("Asterix", "Seaquest", "SpaceInvaders"):
        cfg.env_name = f"MinAtar/{game}-v1"
        with pytest.raises(NotImplementedError, match=game):
            env_factory.build_environment(cfg, 4)
    cfg.device_env_games = ["Freeway"]                                         # any sequence; Breakout is then off
    cfg.env_name = "MinAtar/Freeway-v1"
    env_factory.build_environment(cfg, 2)
    assert made[-1][0] == "Freeway"
    cfg.env_name = "MinAtar/Breakout-v1"
    with pytest.raises(NotImplementedError, match="Breakout"):
        env_factory.build_environment(cfg, 2)
    # a bad knob value
    for bad in (("Breakout", "Seaquest"), ("freeway",), "Pong"):
        cfg.device_env_games = bad
        cfg.env_name = "MinAtar/Breakout-v1"
        with pytest.raises(ValueError, match="device_env_games"):
            env_factory.build_environment(cfg, 2)
    n = len(made)
    cfg.device_env_games = ("Breakout", "Freeway")
    for name in ("ALE/Defender-v5", "MinAtar/Pong-v1", "Freeway-v1"):
        cfg.env_name = name
        with pytest.raises(ValueError):
            env_factory.build_environment(cfg, 4)
    assert len(made) == n


def test_snapshot_kind_mismatch_is_refused():
    from prism_amd.envs import DeviceBreakout, DeviceFreeway
    snap, freeway, breakout = GS.snap, GS.bare(DeviceFreeway), GS.bare(DeviceBreakout)
    with pytest.raises(ValueError, match="kind = 'DeviceBreakout' in the snapshot, 'DeviceFreeway' here"):
        freeway.load_state_dict(snap("DeviceBreakout"))
    with pytest.raises(ValueError, match="kind = 'DeviceFreeway' in the snapshot, 'DeviceBreakout' here"):
        breakout.load_state_dict(snap("DeviceFreeway"))
    freeway.load_state_dict(snap("DeviceFreeway"))                             # its own kind, never started: accepted
    breakout.load_state_dict(snap("DeviceBreakout"))
    with pytest.raises(ValueError, match="n_actions"):
        freeway.load_state_dict(dict(snap("DeviceFreeway"), n_actions=3))
