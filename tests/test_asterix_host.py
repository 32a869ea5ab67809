"""No GPU needed: the Asterix rules on ``HostAsterix`` (tests/asterix_ref.py) alone -- the case table reaches every branch,
invariants hold over seeded play, the draws sit where DESIGN.md 7.5 puts them -- and the host side of the device
environment: the two entry points through the C ABI, their kernels' private segment, the state codec, the factory knob, the
snapshot kinds.  Neither the restatement nor the kernel is checked against the ``minatar`` package."""
import os
import re

import numpy as np
import pytest

from tests import asterix_cases as AC
from tests import game_suite as GS
from tests import helpers as H
from tests.asterix_ref import BRANCHES, KEY_COIN, KEY_SPAWN, HostAsterix, assert_same_state, draw, draw_spawn, spawn_of_words
from tests.env_frame_cases import GAMES

GAME = GAMES["asterix"]          # its seed and Philox-path run are tests/test_gpu_asterix.py's: kept where no GPU is needed


def run_case(name):
    c = AC.CASES[name]
    host = HostAsterix(1, seed=1, **AC.GROUPS[c["group"]])
    host.set_state({k: [v] for k, v in c["state"].items()})
    out, states = [], []
    for a, u, spawn in c["script"]:
        out.append(host.step([a], u=[u], spawn=[spawn]))
        states.append({k: v[0].copy() for k, v in host.get_state().items()})
    return host, out, states


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_case_reaches_its_branches(name):
    host, _, _ = run_case(name)
    for b in AC.CASES[name]["reach"]:
        assert host.branches[b] > 0, (name, b, host.branches)
    assert host.bad_action == bool(AC.CASES[name].get("bad_action", False))


def test_case_table_covers_every_branch_and_channel():
    total = {b: 0 for b in BRANCHES}
    channels = np.zeros(4, np.int64)
    for name in AC.CASES:
        host, out, _ = run_case(name)
        for b, k in host.branches.items():
            total[b] += k
        for next_obs, _, _, _ in out:
            channels += next_obs[0].sum(axis=(0, 1)).astype(np.int64)
    assert set(AC.REQUIRED) == set(BRANCHES) and all(total[b] > 0 for b in BRANCHES), total
    assert (channels > 0).all(), channels
    for g in AC.GROUPS:
        assert len(AC.group_cases(g)) >= 2
    assert any(int(c["state"]["t"]) < 2 ** 32 <= int(c["state"]["t"]) + len(c["script"]) for c in AC.CASES.values())
    # the spawns of the table: the 0th, a middle and the last of k = 8, 3 and 1 empty slots
    want = {(8, 0), (8, 3), (8, 7), (3, 0), (3, 1), (3, 2), (1, 0)}
    seen = {(8 - sum(c["state"]["ent_active"]), c["script"][0][2][2]) for c in AC.CASES.values() if c["state"]["spawn_timer"] == 0}
    assert want <= seen, seen


def _slot(st, i):
    return tuple(int(st[f][i]) for f in ("ent_active", "ent_x", "ent_dir", "ent_gold"))


def test_cases_in_detail():
    """What the crafted cases are for, step by step."""
    host, out, states = run_case("moves_left_up")
    assert [(int(s["px"]), int(s["py"])) for s in states] == [(0, 2), (0, 2), (0, 1), (0, 1)]
    host, out, states = run_case("moves_right_down")
    assert [(int(s["px"]), int(s["py"])) for s in states] == [(9, 7), (9, 7), (9, 8), (9, 8), (9, 8)]
    assert int(states[-1]["last_action"]) == 5
    for name, slot, want in (("spawn_k8_first", 0, (1, 0, 1, 1)), ("spawn_k8_middle", 3, (1, 9, -1, 0)), ("spawn_k8_last", 7, (1, 0, 1, 0)),
                             ("spawn_k3_first", 1, (1, 9, -1, 1)), ("spawn_k3_middle", 3, (1, 0, 1, 1)), ("spawn_k3_last", 7, (1, 9, -1, 0)),
                             ("spawn_k1", 2, (1, 0, 1, 1)), ("rank_clamped", 6, (1, 0, 1, 0))):
        host, out, states = run_case(name)
        before = AC.CASES[name]["state"]["ent_active"]
        assert _slot(states[0], slot) == want and before[slot] == 0, name
        assert sum(states[0]["ent_active"]) == sum(before) + 1 and int(states[0]["spawn_timer"]) == 9, name
        assert out[0][0][0][slot + 1, want[1], 3 if want[3] else 1] == 1, name
    host, out, states = run_case("spawn_full")
    assert list(states[0]["ent_active"]) == [1] * 8 and [int(s["spawn_timer"]) for s in states] == [0, 0]
    assert host.branches["spawn_full"] == 2 and list(states[1]["ent_gold"]) == [0] * 8
    host, out, states = run_case("spawn_gold_on_the_player")
    assert float(out[0][1][0]) == 1.0 and not out[0][2][0] and _slot(states[0], 2) == (0, 0, 0, 0)          # collected on that step
    assert out[0][0][0].sum() == 1
    host, out, states = run_case("spawn_enemy_on_the_player")
    assert float(out[0][1][0]) == 0.0 and out[0][2][0] == 1
    assert out[0][0][0][6, 9, 0] == 1 and out[0][0][0][6, 9, 1] == 1 and out[0][0][0][..., 2].sum() == 0          # its trail is off the board
    assert (int(states[0]["px"]), int(states[0]["py"]), int(states[0]["t"]), int(states[0]["ep_steps"])) == (5, 5, 1, 0)
    host, out, states = run_case("walk_into_gold")
    assert float(out[0][1][0]) == 1.0 and _slot(states[0], 3) == (0, 0, 0, 0) and int(states[0]["px"]) == 6
    host, out, states = run_case("walk_into_enemy")
    assert out[0][2][0] == 1 and out[0][0][0][6, 4, 1] == 1 and out[0][0][0][6, 5, 2] == 1          # it waited
    host, out, states = run_case("terminal_shows_the_move")
    img = out[0][0][0]
    assert out[0][2][0] == 1 and img[6, 4, 0] == 1 and img[6, 3, 1] == 1 and img[6, 4, 2] == 1          # the enemy moved on
    assert img[2, 4, 3] == 1 and img[2, 3, 2] == 1 and img.sum() == 5
    for name, reward, done in (("gold_from_the_left", 1.0, 0), ("gold_from_the_right", 1.0, 0), ("enemy_from_the_left", 0.0, 1),
                               ("enemy_from_the_right", 0.0, 1)):
        host, out, states = run_case(name)
        assert (float(out[0][1][0]), int(out[0][2][0])) == (reward, done), name
        assert out[0][0][0][5, 5].sum() == (1 if reward else 2), name          # the gold is gone; the enemy shares the player's cell
    host, out, states = run_case("exits_and_trails")
    assert list(states[0]["ent_active"]) == [1, 1, 1, 1, 0, 0, 1, 0] and list(states[1]["ent_active"]) == [0, 0, 1, 1, 0, 0, 1, 0]
    assert _slot(states[1], 0) == _slot(states[1], 1) == (0, 0, 0, 0)
    first, second = out[0][0][0], out[1][0][0]
    assert first[3, :, 2].sum() == 0 and first[4, :, 2].sum() == 0 and first[1, 1, 2] == 1 and first[2, 8, 2] == 1 and first[7, 3, 2] == 1
    assert second[3, 0, 2] == 1 and second[3, 1, 1] == 1 and second[4, 9, 2] == 1 and second[4, 8, 3] == 1 and second[7, 4, 2] == 1
    assert int(states[-1]["t"]) == 2 ** 32 + 2
    host, out, states = run_case("ramp_even")
    assert [(int(s["ramp_timer"]), int(s["ramp_index"]), int(s["spawn_speed"]), int(s["move_speed"])) for s in states] == \
        [(-1, 0, 10, 5), (100, 1, 9, 5), (99, 1, 9, 5)]
    host, out, states = run_case("ramp_odd")
    assert [(int(s["ramp_timer"]), int(s["ramp_index"]), int(s["spawn_speed"]), int(s["move_speed"])) for s in states] == \
        [(100, 4, 6, 3), (99, 4, 6, 3)]
    host, out, states = run_case("ramp_move_speed_at_1")
    assert (int(states[0]["ramp_index"]), int(states[0]["spawn_speed"]), int(states[0]["move_speed"])) == (10, 2, 1)
    host, out, states = run_case("ramp_last")
    assert [(int(s["ramp_timer"]), int(s["ramp_index"]), int(s["spawn_speed"]), int(s["move_speed"])) for s in states] == \
        [(100, 9, 1, 1)] * 3 and host.branches["ramp_frozen"] == 2          # the timer freezes
    host, out, states = run_case("ramp_index_15")
    assert (int(states[0]["ramp_index"]), int(states[0]["spawn_speed"]), int(states[0]["move_speed"])) == (16, 4, 2)
    host, out, states = run_case("truncation")
    assert [int(o[3][0]) for o in out] == [0, 0, 0, 0, 1, 0, 0] and [int(o[2][0]) for o in out] == [0] * 7
    assert int(states[-1]["ep_steps"]) == 2 and int(states[-1]["t"]) == 7 and int(states[4]["spawn_timer"]) == 10
    host, out, states = run_case("limit_on_a_terminal")
    assert (int(out[0][2][0]), int(out[0][3][0])) == (1, 0)          # done on the limit's step: not truncated
    host, out, states = run_case("minimal_moves")
    assert [(int(s["px"]), int(s["py"])) for s in states] == [(4, 5), (4, 4), (5, 4), (5, 5)]
    host, out, states = run_case("minimal_out_of_range")
    assert [(int(s["px"]), int(s["py"]), int(s["last_action"])) for s in states] == [(5, 5, 0), (5, 5, 0), (5, 6, 4)]
    host, out, states = run_case("sticky")
    # (l, 0.1: repeats r) (l, 0.25: not below p) (n, 0.2499: repeats l) (u, 0: repeats l) (u)
    assert host.branches["sticky_repeat"] == 3 and [(int(s["px"]), int(s["py"])) for s in states] == [(6, 5), (5, 5), (4, 5), (3, 5), (3, 4)]


def check_state(one, where):
    """Fields within their ranges, one entity per row, an empty slot all zeros."""
    assert 0 <= one["px"] <= 9 and 1 <= one["py"] <= 8, where
    assert 1 <= one["spawn_speed"] <= 10 and 0 <= one["spawn_timer"] <= 10, where
    assert 1 <= one["move_speed"] <= 5 and 0 <= one["move_timer"] <= 5, where
    assert -1 <= one["ramp_timer"] <= 100 and 0 <= one["ramp_index"] <= 9 and 0 <= one["last_action"] <= 5, where
    for i in range(8):
        act, x, d, g = _slot(one, i)
        assert (act, abs(d)) in ((0, 0), (1, 1)) and 0 <= x <= 9 and g in (0, 1), (where, i)
        if not act:
            assert (x, d, g) == (0, 0, 0), (where, i)


def check_image(img, one, where):
    assert set(np.unique(img)) <= {0.0, 1.0} and img.sum() <= 17, where
    assert img[..., 0].sum() == 1 and img[int(one["py"]), int(one["px"]), 0] == 1, where
    assert img[0, :, 1:].sum() == 0 and img[9, :, 1:].sum() == 0, where          # no entity on rows 0 and 9
    for i in range(8):
        act, x, d, g = _slot(one, i)
        row = img[i + 1]
        assert row[:, 1].sum() + row[:, 3].sum() == act and row[:, 2].sum() <= act, (where, i)          # one entity per row
        if act:
            assert row[x, 3 if g else 1] == 1, (where, i)
            assert row[:, 2].sum() == (0 <= x - d <= 9) and (not 0 <= x - d <= 9 or row[x - d, 2] == 1), (where, i)


def test_invariants_over_seeded_play():
    n, steps = 6, 700
    rng = np.random.default_rng(11)
    host = HostAsterix(n, seed=11, sticky_action_prob=0.1, episode_timestep_limit=450)
    host.reset()
    ends = golds = 0
    for k in range(steps):
        next_obs, reward, done, trunc = host.step(rng.integers(0, 6, n))
        assert set(np.unique(reward)) <= {0.0, 1.0} and not (done & trunc).any()
        st = host.get_state()
        acting = host.observe()
        for i in range(n):
            one = {f: st[f][i] for f in st}
            check_state(one, f"step {k}, env {i}")
            check_image(acting[i], one, f"step {k}, env {i}")
            if not (done[i] or trunc[i]):
                np.testing.assert_array_equal(next_obs[i], acting[i])
            else:
                assert acting[i].sum() == 1 and acting[i][5, 5, 0] == 1 and next_obs[i][..., 0].sum() == 1
        ends += int(done.sum() + trunc.sum())
        golds += int(reward.sum())
    assert ends >= 20 and golds >= 10
    for b in ("move_left", "move_up", "clamp_top", "spawn_left", "spawn_right", "spawn_gold", "spawn_enemy", "entities_wait",
              "entities_move", "terminal", "sticky_repeat", "reset", "exit_left", "exit_right", "ramp_even", "ramp_timer_below_zero"):
        assert host.branches[b] > 0, b


def test_draws_stream_keys_and_counters():
    """The coin of environment e at lifetime step t is words 0, 1 of Philox(seed)(t, (e << 32) | "ASXC"); a spawn on that step
    takes the words under "ASXS" at the same counter; a reset draws nothing."""
    keys = dict(ASXC=KEY_COIN, ASXS=KEY_SPAWN)
    for text, key in keys.items():
        assert key == int.from_bytes(text.encode(), "big")
    # no two streams share a key: the four-character keys of csrc/, and TAU0 + sid for every stream id below 2^16
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            found += [int(m, 16) for m in re.findall(r"0x([0-9A-Fa-f]{8})ull", open(os.path.join(csrc, name)).read())]
    ours = sorted(keys.values())
    assert all(found.count(k) == 1 for k in ours), "an Asterix key appears twice in csrc/"
    tau0 = int.from_bytes(b"TAU0", "big")
    assert tau0 in found and all(not tau0 <= k < tau0 + 2 ** 16 for k in ours)
    for k in (b"PERM", b"UNIF", b"IDSA", b"EGRD", b"ENVB", b"FWYC", b"FWW0", b"FWW1", b"FWR0", b"FWR1"):
        assert int.from_bytes(k, "big") in set(found) - set(ours)
    seed = 0x1234567890ABCDEF
    words = {tuple(draw(seed, e, t, key)) for e in range(6) for t in range(5) for key in keys.values()}
    assert len(words) == 6 * 5 * 2                                             # apart by environment, step and purpose
    # a reset draws nothing: two seeds, one first state
    a, b = HostAsterix(3, seed=1), HostAsterix(3, seed=2)
    np.testing.assert_array_equal(a.reset(), b.reset())
    assert_same_state(a.get_state(), b.get_state(), "reset")
    assert a.reset().sum() == 3 and all((e["px"], e["py"], e["spawn_timer"], e["move_timer"], e["ramp_timer"]) == (5, 5, 10, 5, 100)
                                        for e in a.envs)
    # sticky_p = 1: every coin is below it, the first action (no-op) repeats for ever
    host = HostAsterix(6, seed=seed, sticky_action_prob=1.0)
    host.reset()
    for _ in range(9):
        host.step(np.full(6, 1))
    assert all(e["last_action"] == 0 and e["px"] == 5 for e in host.envs)
    # a spawn is the draw AT its step, with k the empty slots before it
    host = HostAsterix(4, seed=seed, episode_timestep_limit=60)
    host.reset()
    spawns = 0
    for _ in range(130):
        t0 = [e["t"] for e in host.envs]
        before = [[s is None for s in e["slots"]] for e in host.envs]
        due = [e["spawn_timer"] == 0 for e in host.envs]
        host.step(np.zeros(4, np.int64))
        for i in range(4):
            if not due[i]:
                continue
            empty = [j for j in range(8) if before[i][j]]
            side, gold, rank = draw_spawn(seed, i, t0[i], len(empty))
            assert spawn_of_words(H.philox4x32(seed, np.array([t0[i]], np.uint64), (i << 32) | KEY_SPAWN)[0], len(empty)) == (side, gold, rank)
            ent = host.envs[i]["slots"][empty[rank]]
            if host.envs[i]["ep_steps"] and ent is not None:          # (not reset on that step, not gone on that step)
                assert (ent["dir"], ent["gold"]) == (1 if side else -1, gold)
                spawns += 1
    assert spawns >= 30


def test_spawn_map_edges_and_frequencies():
    """side = w0 & 1; gold = floor(3 w1 / 2^32) == 0, i.e. w1 < ceil(2^32 / 3); rank = floor(k w2 / 2^32) < k for every k.  Over
    40 000 draws every outcome within 6 binomial sigma of its share (the maps' own bias -- (2^32 mod 3) / 2^32 and at most
    (k - 1) / 2^32 -- is far below that)."""
    third = -(-2 ** 32 // 3)
    assert spawn_of_words([0, 0, 0, 0], 8) == (0, 1, 0) and spawn_of_words([1, third - 1, 2 ** 32 - 1, 0], 8) == (1, 1, 7)
    assert spawn_of_words([2 ** 32 - 1, third, 0, 0], 8)[:2] == (1, 0) and spawn_of_words([2, 2 ** 32 - 1, 0, 0], 8)[:2] == (0, 0)
    for k in range(1, 9):
        assert spawn_of_words([0, 0, 2 ** 32 - 1, 0], k)[2] == k - 1 and spawn_of_words([0, 0, 0, 0], k)[2] == 0
        for r in range(1, k):
            edge = -(-r * 2 ** 32 // k)                                      # the first w2 of rank r
            assert spawn_of_words([0, 0, edge, 0], k)[2] == r and spawn_of_words([0, 0, edge - 1, 0], k)[2] == r - 1
    assert spawn_of_words([0, 0, 2 ** 32 - 1, 0], 0)[2] == 0                 # k = 0: nothing is placed, the rank is not used
    seed, count = 77, 40000
    words = np.array([draw(seed, e, t, KEY_SPAWN) for e in range(50) for t in range(800)], dtype=np.uint64)
    assert words.shape == (count, 4)
    side, gold = words[:, 0] & np.uint64(1), ((words[:, 1] * np.uint64(3)) >> np.uint64(32)) == 0
    assert abs(side.mean() - 0.5) < 6 * np.sqrt(0.25 / count) and abs(gold.mean() - 1 / 3) < 6 * np.sqrt(2 / 9 / count)
    for k in (1, 3, 5, 8):
        rank = (words[:, 2] * np.uint64(k)) >> np.uint64(32)
        assert rank.max() < k
        for r in range(k):
            assert abs((rank == r).mean() - 1 / k) <= 6 * np.sqrt((1 / k) * (1 - 1 / k) / count), (k, r)


def test_sticky_coin_counts_and_zero_never_repeats():
    GS.sticky_coin_check(GAME, steps=200, free_steps=100)


def test_the_philox_run_of_the_gpu_test_shows_a_gold_a_terminal_a_truncation_and_an_exit():
    """tests/test_gpu_asterix.py's Philox-path run (n = 5, 300 steps, limit 60, sticky_p = 0.25, actions of RandomState(7)) on
    ``HostAsterix`` alone.  This restatement gives 9 golds, 15 terminals, 11 truncations and 11 exits."""
    host, (golds, terminals, truncations) = GS.philox_host_run(GAME)
    exits = host.branches["exit_left"] + host.branches["exit_right"]
    print(f"golds {golds}, terminals {terminals}, truncations {truncations}, exits {exits}")
    assert golds >= 1 and terminals >= 1 and truncations >= 1 and exits >= 1
    assert terminals == host.branches["terminal"] and truncations == host.branches["truncation"]


# ---------------------------------------------------------------------- the host side of the device environment
@pytest.fixture(scope="module")
def lib():
    return GS.native_lib()


def test_symbols_exported_declared_and_mirrored(lib):
    src, signatures = GS.symbols_check(lib, GAME)
    assert signatures["prism_env_asterix_step"] == signatures["prism_env_breakout_step"]
    assert len(signatures["prism_env_asterix_reset"][1]) == 2          # a reset draws nothing: no draw pointer
    assert "int prism_env_asterix_reset(const prism_env_desc *d, prism_stream_t stream);" in src and "const uint8_t *spawn_in" in src


@pytest.mark.parametrize("entry", ["reset", "step"])
@pytest.mark.parametrize("case", range(len(GS.refusals(GAME))))
def test_env_refusals_without_device(lib, entry, case):
    """Every refusal of Breakout's table, with the same text but for the action counts (5 or 6), through Asterix's entry points."""
    GS.refusal_check(lib, GAME, entry, case)


def test_step_refuses_null_actions_and_bad_parity(lib):
    GS.null_actions_and_parity_check(lib, GAME)


def test_the_kernels_have_no_private_and_no_group_segment(tmp_path):
    """Read from the code object's metadata of env_asterix.hip (the slots are looked up by constant shifts: an array indexed
    by the chosen slot would land in the private segment)."""
    assert set(GS.kernel_segments(GAME, tmp_path).values()) == {(0, 0)}


def test_state_codec_round_trips_and_refuses():
    from prism_amd.envs import pack_asterix_state, render_asterix, unpack_asterix_state
    for group in AC.GROUPS:
        state, _, _, _ = AC.vector(group, 31)
        words = pack_asterix_state(state)
        assert words.shape == (31, 8) and words.dtype == np.int32 and not words[:, 7].any()
        back = unpack_asterix_state(words)
        assert sorted(back) == sorted(state)
        assert_same_state(back, state, group)
        host = HostAsterix(31)
        host.set_state(state)
        assert_same_state(host.get_state(), state, group)
        np.testing.assert_array_equal(render_asterix(state).astype(np.float32), host.observe())
    # ep_steps and t sit where the other games keep them; ramp_timer -1 is word 6 = 0
    state = AC.vector("plain", 3)[0]
    state["ep_steps"], state["t"] = np.array([1, 2, 3]), np.array([2 ** 40 + 5, 6, 2 ** 64 - 1], dtype=np.uint64)
    state["ramp_timer"] = np.array([-1, 0, 100])
    w = pack_asterix_state(state).view(np.uint32)
    assert list(w[:, 2]) == [1, 2, 3] and list(w[:, 4]) == [5, 6, 2 ** 32 - 1] and list(w[:, 5]) == [256, 0, 2 ** 32 - 1]
    assert list(w[:, 6]) == [0, 1, 101] and list(unpack_asterix_state(w)["ramp_timer"]) == [-1, 0, 100]
    for field, value in (("px", 10), ("px", -1), ("py", 0), ("py", 9), ("spawn_speed", 0), ("spawn_speed", 11), ("spawn_timer", 11),
                         ("spawn_timer", -1), ("move_speed", 0), ("move_speed", 6), ("move_timer", 6), ("ramp_timer", -2),
                         ("ramp_timer", 101), ("ramp_index", 16), ("ramp_index", -1), ("last_action", 6)):
        bad = AC.vector("plain", 2)[0]
        bad[field] = np.array([bad[field][0], value])
        with pytest.raises(ValueError, match=f"DeviceAsterix.set_state: {field} outside"):
            pack_asterix_state(bad)
    full = AC.vector("plain", 10)[0]          # environment 9 is "spawn_full": every slot holds an entity
    assert full["ent_active"][9].all()
    for field, value in (("ent_active", 2), ("ent_x", 10), ("ent_x", -1), ("ent_gold", 2), ("ent_dir", 0), ("ent_dir", 2)):
        bad = {k: v.copy() for k, v in full.items()}
        bad[field][9, 7] = value
        with pytest.raises(ValueError, match=field):
            pack_asterix_state(bad)
    for field in ("ent_x", "ent_gold", "ent_dir"):          # an empty slot holds zeros
        bad = {k: v.copy() for k, v in full.items()}
        bad[field][0, 7] = 1
        with pytest.raises(ValueError, match=field):
            pack_asterix_state(bad)


def test_the_base_class_gained_only_what_asterix_needs():
    from prism_amd import envs
    assert envs.DeviceAsterix.OBS_SHAPE == envs.OBS_SHAPE == (10, 10, 4) and issubclass(envs.DeviceAsterix, envs._DeviceEnv)
    assert (envs.DeviceBreakout._MINIMAL_ACTIONS, envs.DeviceFreeway._MINIMAL_ACTIONS, envs.DeviceAsterix._MINIMAL_ACTIONS) == (3, 3, 5)
    assert envs.DeviceBreakout._RESET_DRAWS and envs.DeviceFreeway._RESET_DRAWS and not envs.DeviceAsterix._RESET_DRAWS
    assert envs.DeviceAsterix._DRAW_WIDTH == 3
    for shared in ("observe", "close", "check_status", "get_state", "set_state", "state_dict", "load_state_dict", "_stage_actions",
                   "_reset", "_step"):
        assert getattr(envs.DeviceAsterix, shared) is getattr(envs._DeviceEnv, shared)
    assert envs.DeviceAsterix._pack is envs.pack_asterix_state and envs.DeviceAsterix._render is envs.render_asterix
    for bad in ([[2, 0, 0]], [[0, 2, 0]], [[0, 0, 8]], [[0, 0, 0], [1, 1, -1]]):
        with pytest.raises(ValueError, match="spawn must be"):
            envs.DeviceAsterix._spawn(np.array(bad))
    ok = np.array([[1, 1, 7], [0, 0, 0]], np.uint8)
    assert envs.DeviceAsterix._spawn(ok) is ok and envs.DeviceAsterix._spawn(None) is None


def test_factory_knob_off_on_and_bad(monkeypatch):
    from prism_amd import envs
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.factory import collector_factory, env_factory
    made = GS.fake_device_classes(monkeypatch, GAME, ("Asterix", "Freeway", "Breakout"))
    assert env_factory.DEVICE_GAMES["Asterix"] == "DeviceAsterix" and env_factory.DEFAULT_DEVICE_GAMES == ("Breakout",)
    cfg = baseline_config(2, device="cuda:0", env_name="MinAtar/Asterix-v1", atari_sticky_actions_prob=0.1, num_processes=9,
                          seed=31, episode_timestep_limit=777)
    # the knob off: refused as before, and the text says how to enable the game
    with pytest.raises(NotImplementedError, match="Asterix.*device_env_games"):
        env_factory.build_environment(cfg, 5)
    with pytest.raises(NotImplementedError, match="Asterix"):
        collector_factory.build_collector(cfg)
    cfg.device_env_games = ("Breakout", "Freeway")
    with pytest.raises(NotImplementedError, match="Asterix"):
        env_factory.build_environment(cfg, 5)
    assert made == []
    # the knob on
    cfg.device_env_games = ("Breakout", "Freeway", "Asterix")
    assert isinstance(env_factory.build_environment(cfg, 5), envs.DeviceAsterix)
    assert made == [("Asterix", (5, 31, "cuda:0"), dict(sticky_action_prob=0.1, episode_timestep_limit=777, minimal_actions=True))]
    cfg.env_name = "MinAtar/Asterix-v0"
    env_factory.build_environment(cfg, 3, seed=8)
    assert made[-1][:2] == ("Asterix", (3, 8, "cuda:0")) and made[-1][2]["minimal_actions"] is False
    col = collector_factory.build_collector(cfg)
    assert isinstance(col, VectorCollector) and isinstance(col.envs, envs.DeviceAsterix) and made[-1][1][0] == 9
    for game, kind in (("Breakout", "Breakout"), ("Freeway", "Freeway")):
        cfg.env_name = f"MinAtar/{game}-v1"
        env_factory.build_environment(cfg, 4)
        assert made[-1][0] == kind
    for game in ("Seaquest", "SpaceInvaders"):
        cfg.env_name = f"MinAtar/{game}-v1"
        with pytest.raises(NotImplementedError, match=game):
            env_factory.build_environment(cfg, 4)
    cfg.device_env_games = ["Asterix"]                                         # any sequence; the others are then off
    cfg.env_name = "MinAtar/Asterix-v1"
    env_factory.build_environment(cfg, 2)
    assert made[-1][0] == "Asterix"
    cfg.env_name = "MinAtar/Breakout-v1"
    with pytest.raises(NotImplementedError, match="Breakout"):
        env_factory.build_environment(cfg, 2)
    # a bad knob value
    for bad in (("Asterix", "Seaquest"), ("asterix",), "Pong"):
        cfg.device_env_games = bad
        cfg.env_name = "MinAtar/Asterix-v1"
        with pytest.raises(ValueError, match="device_env_games"):
            env_factory.build_environment(cfg, 2)
    n = len(made)
    cfg.device_env_games = ("Asterix",)
    for name in ("ALE/Defender-v5", "MinAtar/Pong-v1", "Asterix-v1"):
        cfg.env_name = name
        with pytest.raises(ValueError):
            env_factory.build_environment(cfg, 4)
    assert len(made) == n


def test_the_real_class_counts_five_minimal_actions_before_it_needs_a_device():
    """``DeviceAsterix.__init__`` sets nothing before its checks; the action count is the class's."""
    from prism_amd import _native as N
    from prism_amd.envs import DeviceAsterix
    with pytest.raises(N.NativeLibraryError, match="DeviceAsterix needs a GPU device"):
        DeviceAsterix(2, 1, "cpu", minimal_actions=True)
    with pytest.raises(ValueError, match="DeviceAsterix: n_envs"):
        DeviceAsterix(0, 1, "cuda:0")


def test_snapshot_kind_mismatch_is_refused():
    from prism_amd.envs import DeviceAsterix, DeviceFreeway
    bare, snap = GS.bare, GS.snap
    with pytest.raises(ValueError, match="kind = 'DeviceBreakout' in the snapshot, 'DeviceAsterix' here"):
        bare(DeviceAsterix).load_state_dict(snap("DeviceBreakout"))
    with pytest.raises(ValueError, match="kind = 'DeviceFreeway' in the snapshot, 'DeviceAsterix' here"):
        bare(DeviceAsterix).load_state_dict(snap("DeviceFreeway"))
    with pytest.raises(ValueError, match="kind = 'DeviceAsterix' in the snapshot, 'DeviceFreeway' here"):
        bare(DeviceFreeway).load_state_dict(snap("DeviceAsterix"))
    bare(DeviceAsterix).load_state_dict(snap("DeviceAsterix"))                 # its own kind, never started: accepted
    bare(DeviceAsterix, 5).load_state_dict(snap("DeviceAsterix", 5))
    with pytest.raises(ValueError, match="n_actions"):
        bare(DeviceAsterix).load_state_dict(snap("DeviceAsterix", 5))
