"""No GPU needed: the Seaquest rules on ``HostSeaquest`` (tests/seaquest_ref.py, the LIST form) alone -- the case table reaches
every branch, invariants hold over seeded play under three policies (the condition: no state the codec refuses and no
overflow), the draws sit where DESIGN.md 7.7 puts them -- and the host side of the device environment: the two entry points
through the C ABI, their kernels' private segment, the state codec, the two factory knobs, the snapshot kinds.  Neither the
restatement nor the kernel is checked against the ``minatar`` package."""
import os
import re

import numpy as np
import pytest

from tests import game_suite as GS
from tests import helpers as H
from tests import seaquest_cases as SC
from tests.env_frame_cases import GAMES
from tests.seaquest_ref import (BRANCHES, CAPACITY, KEY_COIN, KEY_DIVER, KEY_ENEMY, LISTS, HostSeaquest, assert_same_state, coin,
                                diver_map, draw, enemy_map, unit_double)

GAME = GAMES["seaquest"]          # its seed and Philox-path run are tests/test_gpu_seaquest.py's: kept where no GPU is needed


def run_case(name):
    c = SC.CASES[name]
    host = HostSeaquest(1, seed=1, **SC.GROUPS[c["group"]])
    host.set_state({k: [v] for k, v in c["state"].items()})
    out, states = [], []
    for a, u, draws in c["script"]:
        out.append(host.step([a], u=[u], draws=[draws]))
        states.append({k: v[0] for k, v in host.get_state().items()})
    return host, out, states


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_case_reaches_its_branches(name):
    host, _, _ = run_case(name)
    for b in SC.CASES[name]["reach"]:
        assert host.branches[b] > 0, (name, b, host.branches)
    assert host.bad_action == bool(SC.CASES[name].get("bad_action", False))
    assert host.overflow == bool(SC.CASES[name].get("overflow", False))          # only the crafted cases overflow


def test_case_table_covers_every_branch_and_channel():
    total = {b: 0 for b in BRANCHES}
    channels = np.zeros(10, np.int64)
    for name in SC.CASES:
        host, out, _ = run_case(name)
        for b, k in host.branches.items():
            total[b] += k
        for next_obs, _, _, _ in out:
            channels += next_obs[0].sum(axis=(0, 1)).astype(np.int64)
    assert all(total[b] > 0 for b in BRANCHES), {b: k for b, k in total.items() if k == 0}
    assert (channels > 0).all(), channels
    for g in SC.GROUPS:
        assert len(SC.group_cases(g)) >= 2
    assert any(int(c["state"]["t"]) < 2 ** 32 <= int(c["state"]["t"]) + len(c["script"]) for c in SC.CASES.values())
    assert sum(bool(c.get("overflow")) for c in SC.CASES.values()) == len(SC.group_cases("overflow")) == 3


def _fields(states, *names):
    return [tuple(int(s[f]) for f in names) for s in states]


def test_cases_in_detail():
    """What the crafted cases are for, step by step."""
    host, out, states = run_case("spawn_fish_from_the_left_and_a_diver")
    assert states[0]["e_fish"] == [(0, 3, 1, 4)] and states[0]["divers"] == [(0, 8, 1, 4)] and states[0]["e_subs"] == []          # (they wait on their first step)
    assert _fields(states, "e_spawn_timer", "d_spawn_timer", "t") == [(19, 29, 2 ** 32), (18, 28, 2 ** 32 + 1)]
    assert states[1]["e_fish"] == [(0, 3, 1, 3)] and out[0][0][0][3, 0, 5] == 1 and out[0][0][0][..., 3].sum() == 0          # the trail is off the board
    host, out, states = run_case("spawn_sub_from_the_right_and_a_diver")
    assert states[0]["e_subs"] == [(9, 8, -1, 2, 9)] and states[0]["divers"] == [(9, 1, -1, 4)] and out[0][0][0][8, 9, 6] == 1
    host, out, states = run_case("spawn_blocked_by_a_fish")
    assert states[0]["e_fish"] == [(4, 3, -1, 1)] and int(states[0]["e_spawn_timer"]) == 19
    host, out, states = run_case("spawn_blocked_by_a_sub")
    assert states[0]["e_subs"] == [(4, 3, 1, 1, 6)] and states[0]["e_fish"] == [] and int(states[0]["e_spawn_timer"]) == 6
    host, out, states = run_case("spawn_beside_the_same_direction")
    assert states[0]["e_fish"] == [(8, 3, 1, 0), (0, 3, 1, 4)]
    host, out, states = run_case("the_sub_moves")
    assert _fields(states, "sub_x", "sub_y", "sub_or", "oxygen") == [(0, 1, 0, 199), (0, 1, 0, 198), (1, 1, 1, 197), (5, 0, 0, 200), (5, 1, 0, 199),
                                                                     (5, 2, 0, 198)]
    assert [int(o[2][0]) for o in out] == [0, 0, 0, 1, 0, 0]          # surfacing without a diver ends the episode; t goes on
    host, out, states = run_case("fire_and_cool_down")
    assert _fields(states, "shot_timer") == [(4,), (3,), (2,), (1,), (0,), (4,), (3,)]
    assert [s["f_bullets"] for s in states] == [[(7, 2, 1)], [(8, 2, 1)], [(9, 2, 1)], [], [], [(7, 2, 1)], [(8, 2, 1)]]
    assert out[0][0][0][2, 7, 2] == 1 and out[0][0][0][2, 6, 0] == 1 and out[0][0][0][2, 5, 1] == 1
    host, out, states = run_case("bullets_leave_at_both_edges")
    assert states[0]["f_bullets"] == [] and states[0]["e_bullets"] == [] and float(out[0][1][0]) == 0.0
    host, out, states = run_case("three_fish_on_one_cell")
    assert states[0]["e_fish"] == [(6, 4, -1, 0), (6, 4, -1, 1)] and states[0]["f_bullets"] == [] and float(out[0][1][0]) == 1.0
    host, out, states = run_case("three_subs_on_one_cell")
    assert states[0]["e_subs"] == [(6, 4, 1, 0, 7), (6, 4, 1, 1, 6)] and float(out[0][1][0]) == 1.0
    host, out, states = run_case("a_fish_and_a_sub_on_one_cell")
    assert states[0]["e_fish"] == [(1, 7, 1, 3)] and states[0]["e_subs"] == [(6, 4, -1, 2, 4)] and float(out[0][1][0]) == 1.0
    host, out, states = run_case("two_bullets_one_step")
    assert states[0]["e_fish"] == [] and states[0]["e_subs"] == [] and states[0]["f_bullets"] == [] and float(out[0][1][0]) == 2.0
    host, out, states = run_case("subs_walk_onto_a_bullet")
    assert states[0]["e_subs"] == [(6, 4, -1, 5, 4)] and states[0]["f_bullets"] == [] and float(out[0][1][0]) == 1.0
    host, out, states = run_case("two_subs_two_bullets")
    assert states[0]["e_subs"] == [(1, 1, 1, 1, 3)] and states[0]["f_bullets"] == [(6, 6, 1)] and float(out[0][1][0]) == 2.0
    host, out, states = run_case("a_fish_walks_onto_a_bullet")
    assert states[0]["e_fish"] == [(1, 4, 1, 2)] and states[0]["f_bullets"] == [] and float(out[0][1][0]) == 1.0
    host, out, states = run_case("a_sub_fires_on_the_step_it_moves")
    assert states[0]["e_subs"] == [(6, 4, -1, 4, 10)] and states[0]["e_bullets"] == [(5, 4, -1)]          # fired from (6, 4), moved on the same step
    assert states[2]["e_subs"] == [(6, 4, -1, 2, 8)] and states[2]["e_bullets"] == [(3, 4, -1)]
    host, out, states = run_case("two_enemy_bullets_in_one_row")
    assert states[0]["e_bullets"] == [(3, 4, -1), (6, 4, -1)] and out[0][0][0][4, :, 4].sum() == 2
    host, out, states = run_case("enemies_leave")
    assert states[0]["e_subs"] == [] and states[0]["e_fish"] == [(3, 7, -1, 0)] and states[0]["e_bullets"] == []          # a sub that left does not fire
    host, out, states = run_case("diver_picked_up_before_its_move")
    assert states[0]["divers"] == [] and int(states[0]["diver_count"]) == 1 and out[0][0][0][9, 8, 8] == 1 and out[0][0][0][9, :, 8].sum() == 1
    host, out, states = run_case("diver_picked_up_after_its_move")
    assert states[0]["divers"] == [(6, 5, -1, 5), (0, 7, -1, 1)] and int(states[0]["diver_count"]) == 1
    host, out, states = run_case("a_refused_seventh_diver")
    assert states[0]["divers"] == [(2, 2, 1, 2)] and int(states[0]["diver_count"]) == 6 and out[0][0][0][9, 3:9, 8].all()
    host, out, states = run_case("a_refused_diver_moves_on")
    assert states[0]["divers"] == [(3, 2, 1, 5), (2, 2, 1, 5)] and int(states[0]["diver_count"]) == 6
    host, out, states = run_case("surfacing_without_divers")
    assert int(out[0][2][0]) == 1 and float(out[0][1][0]) == 0.0 and out[0][0][0][0, 2, 0] == 1
    assert _fields(states[:1], "sub_x", "sub_y", "surface", "ep_steps", "t") == [(5, 0, 1, 0, 1)]          # a reset's
    host, out, states = run_case("surfacing_with_three")
    assert _fields(states, "diver_count", "oxygen", "surface", "e_spawn_speed", "move_speed", "ramp_index") == \
        [(2, 200, 1, 19, 5, 1), (2, 200, 1, 19, 5, 1), (2, 199, 0, 19, 5, 1), (1, 200, 1, 18, 4, 2)]
    assert [float(o[1][0]) for o in out] == [0.0] * 4
    host, out, states = run_case("surfacing_with_six")
    assert _fields(states[:1], "diver_count", "oxygen", "e_spawn_speed", "move_speed", "ramp_index") == [(0, 200, 19, 4, 2)]
    assert float(out[0][1][0]) == 7.0 and out[0][0][0][9, :, 7].all() and out[0][0][0][9, :, 8].sum() == 0
    host, out, states = run_case("surfacing_at_the_slowest_move_speed")
    assert _fields(states[:1], "diver_count", "e_spawn_speed", "move_speed", "ramp_index") == [(1, 4, 2, 16)]
    host, out, states = run_case("surfacing_at_the_ramps_last_step")
    assert _fields(states[:2], "diver_count", "e_spawn_speed", "move_speed", "ramp_index") == [(0, 1, 2, 19)] * 2 and int(out[2][2][0]) == 1
    host, out, states = run_case("surfacing_after_the_ramps_end")
    assert _fields(states[:1], "diver_count", "e_spawn_speed", "move_speed", "ramp_index") == [(0, 1, 2, 19)] and float(out[0][1][0]) == 9.0
    host, out, states = run_case("oxygen_runs_out")
    assert [int(o[2][0]) for o in out] == [0, 1, 0] and int(states[0]["oxygen"]) == -1 and out[0][0][0][9, :, 7].sum() == 0
    host, out, states = run_case("surfacing_with_six_and_no_oxygen")
    assert int(out[0][2][0]) == 1 and float(out[0][1][0]) == -1.0
    for name in ("a_sub_on_the_sub_before_its_move", "a_sub_onto_the_sub", "a_fish_on_the_sub_before_its_move", "a_fish_onto_the_sub",
                 "an_enemy_bullet_on_the_sub", "an_enemy_bullet_onto_the_sub"):
        host, out, states = run_case(name)
        assert [int(o[2][0]) for o in out] == [1, 0] and host.branches["terminal"] == 1, name
    host, out, states = run_case("a_fish_on_the_sub_before_its_move")
    assert out[0][0][0][2, 1, 5] == 1 and out[0][0][0][2, 2, 3] == 1          # a terminal step still runs the later rules
    host, out, states = run_case("a_full_fish_array")
    assert len(states[0]["e_fish"]) == 32 and states[0]["e_fish"][31] == (0, 5, 1, 4) and states[1]["e_fish"][0] == (0, 1, 1, 3)
    host, out, states = run_case("overflow_of_the_fish")
    assert len(states[0]["e_fish"]) == 32 and states[0]["e_fish"][31] == (1, 8, 1, 4) and host.branches["overflow"] == 1
    host, out, states = run_case("overflow_of_the_enemy_bullets")
    assert len(states[0]["e_bullets"]) == 32 and states[0]["e_subs"] == [(4, 3, 1, 1, 10)] and host.branches["overflow"] == 1
    host, out, states = run_case("overflow_of_the_friendly_bullets_and_divers")
    assert len(states[0]["f_bullets"]) == 4 and len(states[0]["divers"]) == 4 and host.branches["overflow"] == 2 and int(states[0]["shot_timer"]) == 4
    host, out, states = run_case("truncation")
    assert [int(o[3][0]) for o in out] == [0, 0, 0, 0, 1, 0, 0] and [int(o[2][0]) for o in out] == [0] * 7
    assert int(states[-1]["ep_steps"]) == 2 and int(states[-1]["t"]) == 7 and int(states[4]["e_spawn_timer"]) == 20
    host, out, states = run_case("limit_on_a_terminal")
    assert (int(out[0][2][0]), int(out[0][3][0])) == (1, 0)          # done on the limit's step: not truncated
    host, out, states = run_case("sticky_fire")
    assert host.branches["sticky_repeat"] == 3 and _fields(states, "sub_x", "last_action", "shot_timer") == \
        [(5, 5, 4), (5, 5, 3), (4, 1, 2), (3, 1, 1), (4, 3, 0)]
    host, out, states = run_case("sticky_out_of_range")
    assert host.branches["bad_action"] == 4 and _fields(states, "sub_x", "last_action") == [(6, 3), (6, 0), (6, 0), (6, 0), (6, 5)]


def check_state(one, where):
    """What the device's record can hold: the condition is "no state the codec refuses"."""
    from prism_amd.envs import pack_seaquest_state, unpack_seaquest_state
    state = {k: [v] for k, v in one.items()}
    assert_same_state(unpack_seaquest_state(pack_seaquest_state(state)), state, where)
    assert one["ramp_index"] == 20 - one["e_spawn_speed"] and one["move_speed"] == max(2, 5 - one["ramp_index"] // 2), where


def _policy(name, env, rng):
    if name == "fire":
        return 5 if env["shot_timer"] == 0 else 4 if env["sub_y"] < 3 else int(rng.integers(0, 5))
    if name == "dive_and_surface":          # down while the oxygen lasts, up to deliver
        if env["diver_count"] > 0 and env["oxygen"] < 40 or env["diver_count"] == 6:
            return 2
        return int(rng.choice([1, 3, 4, 5, 5]))
    return int(rng.integers(0, 6))


MAXIMA = {}


@pytest.mark.parametrize("policy", ["random", "fire", "dive_and_surface"])
def test_invariants_over_seeded_play(policy):
    """The codec accepts every state play reaches and gives it back; nothing overflows; the ramp's three fields move
    together.  Half of the steps start from the hardest ramp, installed by ``set_state``."""
    n = 4
    rng = np.random.default_rng(11)
    ends = kills = 0
    maxima = {name: 0 for name in LISTS + ("enemies",)}
    for hardest, steps in ((False, 400), (True, 600)):          # 4 x 600 = 2400 steps from the hardest ramp
        host = HostSeaquest(n, seed=11 + hardest, sticky_action_prob=0.1, episode_timestep_limit=450)
        host.reset()
        for k in range(steps):
            if hardest:          # an episode that ended begins at the hardest ramp again
                st = host.get_state()
                fresh = st["ep_steps"] == 0
                st["e_spawn_speed"][fresh], st["move_speed"][fresh], st["ramp_index"][fresh] = 1, 2, 19
                st["e_spawn_timer"][fresh] = 1
                host.set_state(st)
            next_obs, reward, done, trunc = host.step([_policy(policy, e, rng) for e in host.envs])
            assert not (done & trunc).any() and reward.min() >= 0.0
            st = host.get_state()
            acting = host.observe()
            assert set(np.unique(acting)) <= {0.0, 1.0}
            for i in range(n):
                check_state({f: st[f][i] for f in st}, f"{policy}, hardest {hardest}, step {k}, env {i}")
                if not (done[i] or trunc[i]):
                    np.testing.assert_array_equal(next_obs[i], acting[i])
                else:
                    assert acting[i].sum() == 12 and acting[i][0, 5, 0] == 1 and acting[i][0, 6, 1] == 1 and acting[i][9, :, 7].all()
                for name in LISTS:
                    maxima[name] = max(maxima[name], len(st[name][i]))
                maxima["enemies"] = max(maxima["enemies"], len(st["e_fish"][i]) + len(st["e_subs"][i]))
            ends += int(done.sum() + trunc.sum())
            kills += int(reward.sum())
        assert not host.overflow and not host.bad_action
    print(f"{policy}: list maxima {maxima}, episode ends {ends}, reward {kills}")
    assert ends >= 8 and all(maxima[name] <= CAPACITY[name] for name in LISTS) and maxima["enemies"] <= 31
    assert maxima["e_fish"] >= 4 and maxima["e_subs"] >= 2 and maxima["e_bullets"] >= 1
    for b in ("spawn_fish", "spawn_sub", "spawn_diver", "sub_fires", "fish_moves", "sub_moves", "terminal", "sticky_repeat", "reset", "under_water"):
        assert host.branches[b] > 0, b


def test_draw_stream_keys_and_counter():
    """Coin, enemy spawn and diver spawn of environment e at lifetime step t are Philox(seed)(t, (e << 32) | key) under three
    keys of their own; a reset draws nothing."""
    keys = (KEY_COIN, KEY_ENEMY, KEY_DIVER)
    assert keys == tuple(int.from_bytes(k, "big") for k in (b"SQXC", b"SQXE", b"SQXD")) == (0x53515843, 0x53515845, 0x53515844)
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            found += [int(m, 16) for m in re.findall(r"0x([0-9A-Fa-f]{8})ull", open(os.path.join(csrc, name)).read())]
    for k in keys:
        assert found.count(k) == 1, "each Seaquest key must appear once in csrc/"
    tau0 = int.from_bytes(b"TAU0", "big")
    assert tau0 in found and not any(tau0 <= k < tau0 + 2 ** 16 for k in keys)
    others = (b"PERM", b"UNIF", b"IDSA", b"EGRD", b"ENVB", b"FWYC", b"FWW0", b"FWW1", b"FWR0", b"FWR1", b"ASXC", b"ASXS", b"SPIC")
    for k in others:
        assert int.from_bytes(k, "big") in set(found) - set(keys)
    seed = 0x1234567890ABCDEF
    words = {tuple(draw(seed, e, t, key)) for e in range(6) for t in range(5) for key in keys}
    assert len(words) == 6 * 5 * 3                                            # apart by environment, step and purpose
    a, b = HostSeaquest(3, seed=1), HostSeaquest(3, seed=2)
    np.testing.assert_array_equal(a.reset(), b.reset())
    assert_same_state(a.get_state(), b.get_state(), "reset")
    first = a.get_state()
    assert a.reset().sum() == 3 * 12 and all(first[name] == [[], [], []] for name in LISTS)
    assert all(tuple(int(first[f][i]) for f in ("sub_x", "sub_y", "sub_or", "oxygen", "diver_count", "surface", "shot_timer", "e_spawn_speed",
                                                 "e_spawn_timer", "d_spawn_timer", "move_speed", "ramp_index")) ==
               (5, 0, 0, 200, 0, 1, 0, 20, 20, 30, 5, 0) for i in range(3))
    # the spawn draws are those of the step that spawns: the first enemy enters on step 20 (t = 20), the first diver on t = 30
    host = HostSeaquest(2, seed=seed)
    host.reset()
    for _ in range(31):
        host.step(np.zeros(2, np.int64))
    for i, e in enumerate(host.envs):
        side, is_sub, row = enemy_map(draw(seed, i, 20, KEY_ENEMY))
        entry = (e["e_subs"] if is_sub else e["e_fish"])[0]
        assert entry[1] == row and entry[2] == (1 if side else -1)
        side, row = diver_map(draw(seed, i, 30, KEY_DIVER))
        assert e["divers"][0][1] == row and e["divers"][0][2] == (1 if side else -1)


def test_draw_map_edges_and_frequencies():
    top = 2 ** 32 - 1
    assert enemy_map((0, 0, 0, 0)) == (0, 1, 1) and enemy_map((top, top, top, 0)) == (1, 0, 8)
    assert enemy_map((1, 1431655765, 2 ** 29 - 1, 0)) == (1, 1, 1) and enemy_map((2, 1431655766, 2 ** 29, 0)) == (0, 0, 2)          # is_sub below 2^32 / 3
    assert diver_map((0, 0, 0, 0)) == (0, 1) and diver_map((top, top, 0, 0)) == (1, 8) and diver_map((0, 7 * 2 ** 29 - 1, 0, 0)) == (0, 7)
    # the row is the top three bits: all eight rows exactly equally likely; is_sub has 1431655766 of 2^32 words
    w = H.philox4x32(77, np.arange(24000, dtype=np.uint64), KEY_ENEMY)
    maps = [enemy_map(r) for r in w]
    rows = np.bincount([m[2] for m in maps], minlength=9)
    assert rows[0] == 0 and rows[1:].min() > 2700 and rows[1:].max() < 3300
    assert 7600 < sum(m[1] for m in maps) < 8400 and 11600 < sum(m[0] for m in maps) < 12400
    c = coin(5, 3, 17)
    r = H.philox4x32(5, np.array([17], np.uint64), (3 << 32) | KEY_COIN)[0]
    assert c == unit_double(r[0], r[1]) and 0.0 <= c < 1.0


def test_sticky_coin_counts_and_zero_never_repeats():
    GS.sticky_coin_check(GAME, steps=120, free_steps=60)


def test_the_philox_run_of_the_gpu_test_shows_spawns_a_terminal_and_a_truncation():
    host, (_, terminals, truncations) = GS.philox_host_run(GAME)
    br = host.branches
    print(f"terminals {terminals}, truncations {truncations}, fish {br['spawn_fish']}, subs {br['spawn_sub']}, divers {br['spawn_diver']}, "
          f"blocked {br['spawn_blocked']}, fired {br['fire']}")
    assert terminals >= 1 and truncations >= 1 and br["spawn_fish"] >= 1 and br["spawn_sub"] >= 1 and br["spawn_diver"] >= 1 and br["fire"] >= 1
    assert terminals == br["terminal"] and truncations == br["truncation"] and not host.overflow


# ---------------------------------------------------------------------- the host side of the device environment
@pytest.fixture(scope="module")
def lib():
    return GS.native_lib()


def test_symbols_exported_declared_and_mirrored(lib):
    from prism_amd import _native as N
    src, signatures = GS.symbols_check(lib, GAME)
    assert signatures["prism_env_seaquest_step"] == signatures["prism_env_asterix_step"]          # one draw array
    assert signatures["prism_env_seaquest_reset"] == signatures["prism_env_asterix_reset"]        # a reset draws nothing
    assert "int prism_env_seaquest_reset(const prism_env_desc *d, prism_stream_t stream);" in src
    assert re.search(r"int prism_env_seaquest_step\(const prism_env_desc \*d, const int64_t \*actions, const double \*u_in, "
                     r"const uint8_t \*draws_in,\s+int32_t parity, prism_stream_t stream\);", src)
    # a record width and a status bit of its own; the 8-word record and the descriptor are what they were
    assert f"#define PRISM_ENV_SEAQUEST_STATE_WORDS {N.ENV_SEAQUEST_STATE_WORDS}" in src and N.ENV_SEAQUEST_STATE_WORDS == 112
    assert f"#define PRISM_ENV_STATUS_OVERFLOW {N.ENV_STATUS_OVERFLOW}u" in src and N.ENV_STATUS_OVERFLOW == 2 != N.ENV_STATUS_BAD_ACTION
    assert 8 + sum(CAPACITY.values()) == N.ENV_SEAQUEST_STATE_WORDS


@pytest.mark.parametrize("entry", ["reset", "step"])
@pytest.mark.parametrize("case", range(len(GS.refusals(GAME))))
def test_env_refusals_without_device(lib, entry, case):
    """Every refusal of Breakout's table, with the same text but for the action count (6 only), through this game's entry points."""
    GS.refusal_check(lib, GAME, entry, case)


def test_step_refuses_null_actions_and_bad_parity(lib):
    GS.null_actions_and_parity_check(lib, GAME)


def test_the_kernels_have_no_private_segment(tmp_path):
    """Read from the code object's metadata of env_seaquest.hip: lane i holds entry i of every list, so no per-lane array is
    indexed by a run-time value.  The group segment is the four waves' boards of 104 words."""
    assert set(GS.kernel_segments(GAME, tmp_path).values()) == {(0, 4 * 104 * 4)}


def test_named_constants_stand_once_on_each_side():
    from tests import seaquest_ref as R
    src = open(os.path.join(H.ROOT, "prism_amd", "csrc", "env_seaquest.hip")).read()
    want = dict(SQ_MAX_OXYGEN=R.MAX_OXYGEN, SQ_MAX_DIVERS=R.MAX_DIVERS, SQ_SHOT_COOL_DOWN=R.SHOT_COOL_DOWN,
                SQ_ENEMY_SHOT_INTERVAL=R.ENEMY_SHOT_INTERVAL, SQ_ENEMY_SPAWN_SPEED=R.ENEMY_SPAWN_SPEED, SQ_DIVER_SPAWN_SPEED=R.DIVER_SPAWN_SPEED,
                SQ_ENEMY_MOVE_SPEED=R.ENEMY_MOVE_SPEED, SQ_DIVER_MOVE_INTERVAL=R.DIVER_MOVE_INTERVAL, SQ_MOVE_SPEED_MIN=R.MOVE_SPEED_MIN,
                SQ_FISH=CAPACITY["e_fish"], SQ_SUBS=CAPACITY["e_subs"], SQ_EBULLETS=CAPACITY["e_bullets"], SQ_FBULLETS=CAPACITY["f_bullets"],
                SQ_DIVERS=CAPACITY["divers"])
    for name, value in want.items():
        found = re.findall(r"\b" + name + r" = (\d+)\b", src)
        assert found == [str(value)], (name, found)
    assert (R.MAX_OXYGEN, R.MAX_DIVERS, R.SHOT_COOL_DOWN, R.ENEMY_SHOT_INTERVAL, R.ENEMY_SPAWN_SPEED, R.DIVER_SPAWN_SPEED, R.ENEMY_MOVE_SPEED,
            R.DIVER_MOVE_INTERVAL, R.MOVE_SPEED_MIN) == (200, 6, 5, 10, 20, 30, 5, 5, 2)


def test_state_codec_round_trips_and_refuses():
    from prism_amd.envs import SEAQUEST_LISTS, pack_seaquest_state, render_seaquest, unpack_seaquest_state
    assert {k: v[1] for k, v in SEAQUEST_LISTS.items()} == CAPACITY
    for group in SC.GROUPS:
        state = SC.vector(group, 31)[0]
        words = pack_seaquest_state(state)
        assert words.shape == (31, 112) and words.dtype == np.int32
        back = unpack_seaquest_state(words)
        assert sorted(back) == sorted(state)
        assert_same_state(back, state, group)
        np.testing.assert_array_equal(pack_seaquest_state(back), words)          # the words exactly
        host = HostSeaquest(31)
        host.set_state(state)
        assert_same_state(host.get_state(), state, group)
        np.testing.assert_array_equal(render_seaquest(state).astype(np.float32), host.observe())
    # where include/prism_hip.h puts the fields
    state = SC.vector("plain", 2)[0]
    state["ep_steps"], state["t"] = np.array([1, 2]), np.array([2 ** 40 + 5, 2 ** 64 - 1], dtype=np.uint64)
    for f, v in dict(sub_x=(9, 0), sub_y=(8, 0), sub_or=(1, 0), surface=(1, 0), shot_timer=(5, 0), diver_count=(6, 0), last_action=(5, 0),
                     move_speed=(5, 2), ramp_index=(19, 0), oxygen=(200, -1), e_spawn_speed=(20, 1), e_spawn_timer=(20, 0),
                     d_spawn_timer=(30, 0)).items():
        state[f] = np.array(v)
    state["e_fish"], state["e_subs"] = [[(9, 8, 1, 5)], []], [[(0, 1, -1, 0, 10), (3, 4, 1, 2, 7)], []]
    state["e_bullets"], state["f_bullets"], state["divers"] = [[(1, 2, -1)], []], [[(4, 0, 1)], []], [[(5, 6, -1, 3)], []]
    w = pack_seaquest_state(state).view(np.uint32)
    assert list(w[:, 2]) == [1, 2] and list(w[:, 4]) == [5, 2 ** 32 - 1] and list(w[:, 5]) == [256, 2 ** 32 - 1]
    assert w[0, 0] == 9 | 8 << 4 | 1 << 8 | 1 << 9 | 5 << 10 | 6 << 13 | 5 << 16 | 5 << 19 | 19 << 22 and w[1, 0] == 2 << 19
    assert w[0, 1] == 201 | 20 << 8 | 20 << 13 | 30 << 18 and w[1, 1] == 1 << 8
    assert not w[:, [3, 6, 7]].any() and not w[1, 8:].any()                   # an empty slot reads back as zeros
    assert w[0, 8] == 9 | 8 << 4 | 1 << 8 | 5 << 9 | 1 << 16 and w[0, 40] == 1 << 4 | 10 << 12 | 1 << 16
    assert w[0, 41] == 3 | 4 << 4 | 1 << 8 | 2 << 9 | 7 << 12 | 1 << 16 and w[0, 72] == 1 | 2 << 4 | 1 << 16
    assert w[0, 104] == 4 | 1 << 8 | 1 << 16 and w[0, 108] == 5 | 6 << 4 | 3 << 9 | 1 << 16 and not w[0, [9, 42, 73, 105, 109]].any()
    assert_same_state(unpack_seaquest_state(w), state, "edited")
    for field, value in (("sub_x", 10), ("sub_x", -1), ("sub_y", 9), ("sub_or", 2), ("surface", 2), ("shot_timer", 6), ("diver_count", 7),
                         ("last_action", 6), ("move_speed", 1), ("move_speed", 6), ("ramp_index", 20), ("oxygen", -2), ("oxygen", 201),
                         ("e_spawn_speed", 0), ("e_spawn_speed", 21), ("e_spawn_timer", 21), ("d_spawn_timer", 31), ("d_spawn_timer", -1)):
        bad = SC.vector("plain", 2)[0]
        bad[field] = np.array([bad[field][0], value])
        with pytest.raises(ValueError, match=f"DeviceSeaquest.set_state: {field} outside"):
            pack_seaquest_state(bad)
    for x, facing in ((0, 1), (9, 0)):                                        # the cell behind the sub off the board
        bad = SC.vector("plain", 2)[0]
        bad["sub_x"][1], bad["sub_or"][1] = x, facing
        with pytest.raises(ValueError, match="DeviceSeaquest.set_state: the cell behind the sub"):
            pack_seaquest_state(bad)
        bad["sub_or"][1] = 1 - facing
        pack_seaquest_state(bad)
    for name, capacity in CAPACITY.items():                                   # a list longer than its capacity
        entry = {3: (4, 4, 1), 4: (4, 4, 1, 0), 5: (4, 4, 1, 0, 0)}[SEAQUEST_LISTS[name][3]]
        bad = SC.vector("plain", 2)[0]
        bad[name][1] = [entry] * capacity
        pack_seaquest_state(bad)
        bad[name][1] = [entry] * (capacity + 1)
        with pytest.raises(ValueError, match=f"DeviceSeaquest.set_state: {name} holds {capacity + 1} entries"):
            pack_seaquest_state(bad)
    for name, entry in (("e_fish", (4, 0, 1, 0)), ("e_fish", (4, 9, 1, 0)), ("e_subs", (4, 0, 1, 0, 0)), ("e_subs", (4, 9, -1, 0, 0)),
                        ("e_bullets", (4, 0, 1)), ("divers", (4, 9, 1, 0)), ("f_bullets", (4, 9, 1)), ("e_fish", (10, 4, 1, 0)),
                        ("f_bullets", (-1, 4, 1)), ("e_fish", (4, 4, 0, 0)), ("e_fish", (4, 4, 1, 6)), ("e_subs", (4, 4, 1, 0, 11)),
                        ("divers", (4, 4, 2, 0)), ("e_fish", (4, 4, 1)), ("e_bullets", (4, 4, 1, 0))):
        bad = SC.vector("plain", 2)[0]
        bad[name][1] = [entry]
        with pytest.raises(ValueError, match=f"DeviceSeaquest.set_state: .*{name}"):
            pack_seaquest_state(bad)


def test_the_base_class_gained_only_the_record_width():
    from prism_amd import _native as N
    from prism_amd import envs
    SQ = envs.DeviceSeaquest
    assert SQ.OBS_SHAPE == envs.SEAQUEST_OBS_SHAPE == (10, 10, 10) and issubclass(SQ, envs._DeviceEnv)
    assert SQ._MINIMAL_ACTIONS == 6 and SQ._STEP_DRAWS and not SQ._RESET_DRAWS and SQ._DRAW_WIDTH == 5
    others = (envs.DeviceBreakout, envs.DeviceFreeway, envs.DeviceAsterix, envs.DeviceSpaceInvaders)
    assert [c._STATE_WORDS for c in others] == [N.ENV_STATE_WORDS] * 4 and SQ._STATE_WORDS == N.ENV_SEAQUEST_STATE_WORDS
    for shared in ("observe", "close", "check_status", "get_state", "set_state", "state_dict", "load_state_dict", "_stage_actions",
                   "_reset", "_step"):
        assert getattr(SQ, shared) is getattr(envs._DeviceEnv, shared)
    assert SQ._pack is envs.pack_seaquest_state and SQ._unpack is envs.unpack_seaquest_state and SQ._render is envs.render_seaquest
    import inspect
    assert list(inspect.signature(SQ.step).parameters) == ["self", "actions", "u", "draws"] and list(inspect.signature(SQ.reset).parameters) == ["self"]
    for bad in ([[2, 0, 1, 0, 1]], [[0, 2, 1, 0, 1]], [[0, 0, 0, 0, 1]], [[0, 0, 9, 0, 1]], [[0, 0, 1, 2, 1]], [[0, 0, 1, 0, 0]], [[0, 0, 1, 0, 9]]):
        with pytest.raises(ValueError, match="DeviceSeaquest: draws must be"):
            SQ._draws(np.array(bad))
    assert SQ._draws(None) is None and SQ._draws(np.array([[1, 1, 8, 1, 8], [0, 0, 1, 0, 1]])) is not None


def test_both_factory_knobs(monkeypatch):
    from prism_amd import envs
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.factory import collector_factory, env_factory
    made = GS.fake_device_classes(monkeypatch, GAME, ("Seaquest", "SpaceInvaders", "Asterix", "Freeway", "Breakout"))
    assert env_factory.WIDE_DEVICE_GAMES == {"Seaquest": "DeviceSeaquest"} and env_factory.DEFAULT_WIDE_DEVICE_GAMES == ()
    assert "Seaquest" not in env_factory.DEVICE_GAMES and env_factory.DEFAULT_DEVICE_GAMES == ("Breakout",)
    assert sorted(set(env_factory.MINATAR_GAMES) - set(env_factory.DEVICE_GAMES) - set(env_factory.WIDE_DEVICE_GAMES)) == []
    cfg = baseline_config(2, device="cuda:0", env_name="MinAtar/Seaquest-v1", atari_sticky_actions_prob=0.1, num_processes=9,
                          seed=31, episode_timestep_limit=777)
    # both knobs at their defaults, and every 8-word game on: refused as before, and the text names the new knob
    with pytest.raises(NotImplementedError, match="MinAtar Seaquest is not implemented on the device.*device_env_wide_games"):
        env_factory.build_environment(cfg, 5)
    with pytest.raises(NotImplementedError, match="Seaquest"):
        collector_factory.build_collector(cfg)
    cfg.device_env_games = ("Breakout", "Freeway", "Asterix", "SpaceInvaders")
    with pytest.raises(NotImplementedError, match="MinAtar Seaquest is not implemented on the device"):
        env_factory.build_environment(cfg, 5)
    cfg.device_env_wide_games = ()
    with pytest.raises(NotImplementedError, match="Seaquest"):
        env_factory.build_environment(cfg, 5)
    assert made == []
    # the 8-word knob does not take the game
    cfg.device_env_games = ("Breakout", "Seaquest")
    with pytest.raises(ValueError, match="device_env_games"):
        env_factory.build_environment(cfg, 5)
    cfg.device_env_games = ("Breakout",)
    # the wide knob on
    for knob in (("Seaquest",), "Seaquest", ["Seaquest"]):
        cfg.device_env_wide_games = knob
        cfg.env_name = "MinAtar/Seaquest-v1"
        assert isinstance(env_factory.build_environment(cfg, 5), envs.DeviceSeaquest)
        assert made[-1] == ("Seaquest", (5, 31, "cuda:0"), dict(sticky_action_prob=0.1, episode_timestep_limit=777, minimal_actions=True))
    cfg.env_name = "MinAtar/Seaquest-v0"
    env_factory.build_environment(cfg, 3, seed=8)
    assert made[-1][:2] == ("Seaquest", (3, 8, "cuda:0")) and made[-1][2]["minimal_actions"] is False
    col = collector_factory.build_collector(cfg)
    assert isinstance(col, VectorCollector) and isinstance(col.envs, envs.DeviceSeaquest) and made[-1][1][0] == 9
    # the other knob's paths are what they were
    cfg.env_name = "MinAtar/Breakout-v1"
    env_factory.build_environment(cfg, 4)
    assert made[-1][0] == "Breakout"
    cfg.env_name = "MinAtar/Freeway-v1"
    with pytest.raises(NotImplementedError, match="Freeway.*device_env_games"):
        env_factory.build_environment(cfg, 4)
    # a bad value of the wide knob, whatever the game asked for
    for bad in (("Seaquest", "Breakout"), ("seaquest",), "Sea quest", ("Pong",)):
        cfg.device_env_wide_games = bad
        for name in ("MinAtar/Seaquest-v1", "MinAtar/Breakout-v1"):
            cfg.env_name = name
            with pytest.raises(ValueError, match="device_env_wide_games"):
                env_factory.build_environment(cfg, 2)
    n = len(made)
    cfg.device_env_wide_games = ("Seaquest",)
    for name in ("ALE/Seaquest-v5", "MinAtar/Pong-v1", "Seaquest-v1"):
        cfg.env_name = name
        with pytest.raises(ValueError):
            env_factory.build_environment(cfg, 4)
    assert len(made) == n


def test_the_real_class_checks_before_it_needs_a_device():
    from prism_amd import _native as N
    from prism_amd.envs import DeviceSeaquest
    with pytest.raises(N.NativeLibraryError, match="DeviceSeaquest needs a GPU device"):
        DeviceSeaquest(2, 1, "cpu", minimal_actions=True)
    with pytest.raises(ValueError, match="DeviceSeaquest: n_envs"):
        DeviceSeaquest(0, 1, "cuda:0")
    with pytest.raises(ValueError, match="DeviceSeaquest: obs_dtype"):
        DeviceSeaquest(2, 1, "cuda:0", obs_dtype="float16")


def test_snapshot_kind_mismatch_is_refused():
    from prism_amd.envs import DeviceAsterix, DeviceSeaquest
    bare, snap = GS.bare, lambda kind, words=8: GS.snap(kind, words=words)
    with pytest.raises(ValueError, match="kind = 'DeviceSpaceInvaders' in the snapshot, 'DeviceSeaquest' here"):
        bare(DeviceSeaquest).load_state_dict(snap("DeviceSpaceInvaders"))
    with pytest.raises(ValueError, match="kind = 'DeviceAsterix' in the snapshot, 'DeviceSeaquest' here"):
        bare(DeviceSeaquest).load_state_dict(snap("DeviceAsterix"))
    with pytest.raises(ValueError, match="kind = 'DeviceSeaquest' in the snapshot, 'DeviceAsterix' here"):
        bare(DeviceAsterix).load_state_dict(snap("DeviceSeaquest", 112))
    bare(DeviceSeaquest).load_state_dict(snap("DeviceSeaquest", 112))          # its own kind, never started: accepted
