"""No GPU needed: the Space Invaders rules on ``HostSpaceInvaders`` (tests/invaders_ref.py, the MAP form) alone -- the case
table reaches every branch, invariants hold over seeded play under three policies, the one draw sits where DESIGN.md 7.6 puts
it -- and the host side of the device environment: the two entry points through the C ABI, their kernels' private and group
segments, the compact state codec, the factory knob, the snapshot kinds.  Neither the restatement nor the kernel is checked
against the ``minatar`` package."""
import os
import re

import numpy as np
import pytest

from tests import game_suite as GS
from tests import helpers as H
from tests import invaders_cases as IC
from tests.env_frame_cases import GAMES
from tests.invaders_ref import BRANCHES, KEY_COIN, HostSpaceInvaders, assert_same_state, draw

GAME = GAMES["invaders"]          # its seed and Philox-path run are tests/test_gpu_invaders.py's: kept where no GPU is needed


def run_case(name):
    c = IC.CASES[name]
    host = HostSpaceInvaders(1, seed=1, **IC.GROUPS[c["group"]])
    host.set_state({k: [v] for k, v in c["state"].items()})
    out, states = [], []
    for a, u in c["script"]:
        out.append(host.step([a], u=[u]))
        states.append({k: v[0].copy() for k, v in host.get_state().items()})
    return host, out, states


@pytest.mark.parametrize("name", sorted(IC.CASES))
def test_case_reaches_its_branches(name):
    host, _, _ = run_case(name)
    for b in IC.CASES[name]["reach"]:
        assert host.branches[b] > 0, (name, b, host.branches)
    assert host.bad_action == bool(IC.CASES[name].get("bad_action", False))


def test_case_table_covers_every_branch_and_channel():
    total = {b: 0 for b in BRANCHES}
    channels = np.zeros(6, np.int64)
    for name in IC.CASES:
        host, out, _ = run_case(name)
        for b, k in host.branches.items():
            total[b] += k
        for next_obs, _, _, _ in out:
            channels += next_obs[0].sum(axis=(0, 1)).astype(np.int64)
    assert set(IC.REQUIRED) == set(BRANCHES) and all(total[b] > 0 for b in BRANCHES), total
    assert (channels > 0).all(), channels
    for g in IC.GROUPS:
        assert len(IC.group_cases(g)) >= 2
    assert any(int(c["state"]["t"]) < 2 ** 32 <= int(c["state"]["t"]) + len(c["script"]) for c in IC.CASES.values())
    # both extremes of the origin, with the outer block columns dead
    assert {-5, 9} <= {c["state"]["alien_x"] for c in IC.CASES.values()}


def _fields(states, *names):
    return [tuple(int(s[f]) for f in names) for s in states]


def test_cases_in_detail():
    """What the crafted cases are for, step by step."""
    host, out, states = run_case("cannon_left")
    assert _fields(states, "pos", "last_action") == [(0, 1), (0, 1), (0, 2), (0, 4)]
    host, out, states = run_case("cannon_right")
    assert _fields(states, "pos") == [(9,), (9,)]
    host, out, states = run_case("fire_and_cool_down")
    assert _fields(states, "shot_timer") == [(4,), (3,), (2,), (1,), (0,), (0,), (4,)]
    assert [list(np.nonzero(s["f_bullet_x"] >= 0)[0]) for s in states] == [[8], [7], [6], [5], [4], [], [8]]          # row 8 after the shot
    assert [float(o[1][0]) for o in out] == [0, 0, 0, 0, 0, 1, 0] and states[5]["alien_block"][3, 3] == 0 and states[5]["alien_block"].sum() == 23
    host, out, states = run_case("friendly_bullet_leaves")
    assert list(states[0]["f_bullet_x"]) == [-1, -1, -1, -1, 9, -1, -1, -1, -1, -1] and host.branches["f_bullet_leaves"] == 1
    host, out, states = run_case("enemy_bullet_leaves")
    assert list(states[0]["e_bullet_x"]) == [-1, -1, -1, -1, -1, 9, -1, -1, -1, -1] and not out[0][2][0]
    host, out, states = run_case("hit_by_a_bullet")
    assert out[0][2][0] == 1 and out[0][0][0][9, 5, 5] == 1 and out[0][0][0][9, 5, 0] == 1
    assert _fields(states[:1], "ep_steps", "t", "alien_move_timer", "alien_shot_timer") == [(0, 1, 12, 10)]          # a reset's
    host, out, states = run_case("aliens_left")
    assert _fields(states, "alien_x", "alien_y", "alien_dir", "alien_move_timer") == [(1, 0, -1, 11), (1, 0, -1, 10)]
    assert int(states[-1]["t"]) == 2 ** 32 + 1 and out[0][0][0][..., 2].sum() == 24 and out[0][0][0][..., 3].sum() == 0
    host, out, states = run_case("aliens_right")
    assert _fields(states, "alien_x", "alien_dir", "alien_move_timer") == [(3, 1, 8), (3, 1, 7)]          # min(24, 9) - 1
    assert out[0][0][0][..., 3].sum() == 24 and out[0][0][0][..., 2].sum() == 0
    for name, x, d in (("turn_at_column_0", 0, 1), ("turn_at_column_9", 4, -1), ("turn_at_column_0_outer_columns_dead", -5, 1),
                       ("turn_at_column_9_outer_columns_dead", 9, -1)):
        host, out, states = run_case(name)
        assert _fields(states[:1], "alien_x", "alien_y", "alien_dir") == [(x, 1, d)], name
    host, out, states = run_case("turn_at_column_0_outer_columns_dead")
    assert _fields(states, "alien_x", "alien_y", "alien_move_timer") == [(-5, 1, 1), (-5, 1, 0), (-4, 1, 1)]          # min(2, 12) - 1
    assert out[0][0][0][1, 0, 1] == out[0][0][0][2, 0, 1] == 1 and out[0][0][0][..., 1].sum() == 2
    host, out, states = run_case("one_alien_moves_every_step")
    assert _fields(states, "alien_x", "alien_move_timer") == [(1, 0), (0, 0), (-1, 0), (-2, 0)]
    assert out[3][0][0][3, 0, 1] == 1          # the alien of block column 2 is on board column 0
    host, out, states = run_case("alien_on_the_cannon_before_the_move")
    assert out[0][2][0] == 1 and out[0][0][0][9, 5, :2].sum() == 2 and host.branches["alien_on_cannon_after_move"] == 0
    host, out, states = run_case("alien_on_the_cannon_after_the_move")
    assert out[0][2][0] == 1 and out[0][0][0][9, 5, :2].sum() == 2 and host.branches["alien_on_cannon_before_move"] == 0
    host, out, states = run_case("terminal_descent_wraps_and_fires")
    img = out[0][0][0]
    assert out[0][2][0] == 1 and img[0, 0, 1] == 1 and img[9, 0, 1] == 1 and img[7, 3, 1] == 1 and img[..., 1].sum() == 3
    assert img[..., 3].sum() == 3 and img[9, 0, 5] == 1 and img[..., 5].sum() == 1          # turned; the shot from board row 9, not 0
    host, out, states = run_case("shot_from_the_cannons_column")
    assert list(states[0]["e_bullet_x"]) == [-1, -1, -1, 5] + [-1] * 6 and int(states[0]["alien_shot_timer"]) == 9
    host, out, states = run_case("shot_tie_takes_the_lower_column")
    assert list(states[0]["e_bullet_x"]) == [3] + [-1] * 9
    host, out, states = run_case("shot_from_nine_columns_away")
    assert list(states[0]["e_bullet_x"]) == [-1, -1, 9] + [-1] * 7
    host, out, states = run_case("shot_onto_a_bullet")
    assert list(states[0]["e_bullet_x"]) == [-1, -1, -1, 5] + [-1] * 6 and out[0][0][0][..., 5].sum() == 1
    host, out, states = run_case("single_kill")
    assert float(out[0][1][0]) == 1.0 and states[0]["alien_block"].sum() == 23 and (states[0]["f_bullet_x"] == -1).all()
    host, out, states = run_case("two_kills")
    assert float(out[0][1][0]) == 2.0 and states[0]["alien_block"][3, 3] == states[0]["alien_block"][2, 2] == 0
    assert states[0]["alien_block"].sum() == 22 and (states[0]["f_bullet_x"] == -1).all()
    host, out, states = run_case("pass_through")
    assert float(out[0][1][0]) == 0.0 and states[0]["alien_block"].sum() == 2 and list(states[0]["f_bullet_x"][:5]) == [-1, -1, -1, 3, -1]
    assert out[0][0][0][4, 3, 1] == 1 and out[0][0][0][3, 3, 4] == 1
    host, out, states = run_case("last_alien_ramps")
    assert _fields(states[:1], "enemy_move_interval", "ramp_index", "alien_x", "alien_y", "alien_dir", "alien_move_timer") == [(11, 1, 2, 0, -1, 6)]
    assert states[0]["alien_block"].all() and float(out[0][1][0]) == 1.0
    host, out, states = run_case("last_alien_at_the_fastest")
    assert _fields(states[:1], "enemy_move_interval", "ramp_index", "alien_dir", "alien_move_timer") == [(6, 6, 1, 2)] and states[0]["alien_block"].all()
    host, out, states = run_case("truncation")
    assert [int(o[3][0]) for o in out] == [0, 0, 0, 0, 1, 0, 0] and [int(o[2][0]) for o in out] == [0] * 7
    assert int(states[-1]["ep_steps"]) == 2 and int(states[-1]["t"]) == 7 and int(states[4]["alien_move_timer"]) == 12
    host, out, states = run_case("limit_on_a_terminal")
    assert (int(out[0][2][0]), int(out[0][3][0])) == (1, 0)          # done on the limit's step: not truncated
    host, out, states = run_case("minimal_mapping")
    assert _fields(states, "pos", "last_action", "shot_timer") == [(4, 1, 0), (5, 3, 0), (6, 3, 0), (6, 5, 4)] and int(states[3]["f_bullet_x"][8]) == 6
    host, out, states = run_case("minimal_out_of_range")
    assert _fields(states, "pos", "last_action", "shot_timer") == [(5, 0, 0), (5, 0, 0), (5, 0, 0), (5, 5, 4)] and host.branches["bad_action"] == 3
    host, out, states = run_case("sticky_fire")
    assert host.branches["sticky_repeat"] == 3 and _fields(states, "pos", "last_action", "shot_timer") == \
        [(5, 5, 4), (5, 5, 3), (4, 1, 2), (3, 1, 1), (4, 3, 0)]


def check_state(one, where):
    """What the device's record can hold: the condition is "no state the codec refuses"."""
    from prism_amd.envs import pack_invaders_state, unpack_invaders_state
    words = pack_invaders_state({k: np.asarray(v)[None] for k, v in one.items()})
    assert_same_state(unpack_invaders_state(words), {k: np.asarray(v)[None] for k, v in one.items()}, where)
    assert 0 <= one["alien_move_timer"] <= 12 and 0 <= one["alien_shot_timer"] <= 10 and 0 <= one["shot_timer"] <= 5, where
    assert 6 <= one["enemy_move_interval"] <= 12 and one["ramp_index"] == 12 - one["enemy_move_interval"], where
    assert (one["f_bullet_x"] >= 0).sum() <= 2 and (one["e_bullet_x"] >= 0).sum() <= 1, where          # what play was seen to reach


def _policy(name, env, rng):
    if name == "fire" and env["shot_timer"] == 0:
        return 5
    if name == "track":
        cols = np.nonzero(env["alien_map"].any(axis=0))[0]
        target = int(cols[np.argmin(np.abs(cols - env["pos"]))])
        return 5 if target == env["pos"] and env["shot_timer"] == 0 else 1 if target < env["pos"] else 3 if target > env["pos"] else 0
    return int(rng.integers(0, 6))


@pytest.mark.parametrize("policy", ["random", "fire", "track"])
def test_invariants_over_seeded_play(policy):
    """``get_state`` itself asserts one bullet per row and map and the live aliens inside the block's window; the codec
    accepts every state and gives it back; the timers stay in range."""
    n, steps = 4, 500
    rng = np.random.default_rng(11)
    host = HostSpaceInvaders(n, seed=11, sticky_action_prob=0.1, episode_timestep_limit=450)
    host.reset()
    ends = kills = 0
    for k in range(steps):
        next_obs, reward, done, trunc = host.step([_policy(policy, e, rng) for e in host.envs])
        assert set(np.unique(reward)) <= {0.0, 1.0, 2.0} and not (done & trunc).any()
        st = host.get_state()
        acting = host.observe()
        assert set(np.unique(acting)) <= {0.0, 1.0} and acting.reshape(n, -1).sum(axis=1).max() <= 2 * 24 + 1 + 3
        for i in range(n):
            check_state({f: st[f][i] for f in st}, f"{policy}, step {k}, env {i}")
            if not (done[i] or trunc[i]):
                np.testing.assert_array_equal(next_obs[i], acting[i])
            else:
                assert acting[i].sum() == 49 and acting[i][9, 5, 0] == 1 and acting[i][0:4, 2:8, 1:3].all()
        ends += int(done.sum() + trunc.sum())
        kills += int(reward.sum())
    assert ends >= 8 and kills >= 40
    # (the tracking cannon stays under the block and is shot before the block reaches column 0)
    for b in ("fire", "aliens_left", "alien_shot", "kill", "hit_by_bullet", "terminal", "sticky_repeat", "reset", "timer_from_interval",
              "aliens_wait") + (() if policy == "track" else ("turn_at_column_0", "aliens_right")):
        assert host.branches[b] > 0, b


def test_draw_stream_key_and_counter():
    """The coin of environment e at lifetime step t is words 0, 1 of Philox(seed)(t, (e << 32) | "SPIC"); nothing else is
    drawn, a reset draws nothing."""
    assert KEY_COIN == int.from_bytes(b"SPIC", "big") == 0x53504943
    # no two streams share a key: the four-character keys of csrc/, and TAU0 + sid for every stream id below 2^16
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    found = []
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")):
            found += [int(m, 16) for m in re.findall(r"0x([0-9A-Fa-f]{8})ull", open(os.path.join(csrc, name)).read())]
    assert found.count(KEY_COIN) == 1, "the Space Invaders key must appear once in csrc/"
    tau0 = int.from_bytes(b"TAU0", "big")
    assert tau0 in found and not tau0 <= KEY_COIN < tau0 + 2 ** 16
    for k in (b"PERM", b"UNIF", b"IDSA", b"EGRD", b"ENVB", b"FWYC", b"FWW0", b"FWW1", b"FWR0", b"FWR1", b"ASXC", b"ASXS"):
        assert int.from_bytes(k, "big") in set(found) - {KEY_COIN}
    seed = 0x1234567890ABCDEF
    words = {tuple(draw(seed, e, t)) for e in range(6) for t in range(5)}
    assert len(words) == 6 * 5                                                 # apart by environment and step
    # a reset draws nothing: two seeds, one first state
    a, b = HostSpaceInvaders(3, seed=1), HostSpaceInvaders(3, seed=2)
    np.testing.assert_array_equal(a.reset(), b.reset())
    assert_same_state(a.get_state(), b.get_state(), "reset")
    first = a.get_state()
    assert a.reset().sum() == 3 * 49 and first["alien_block"].all() and (first["f_bullet_x"] == -1).all() and (first["e_bullet_x"] == -1).all()
    assert all(tuple(int(first[f][i]) for f in ("pos", "alien_x", "alien_y", "alien_dir", "alien_move_timer", "alien_shot_timer",
                                                 "enemy_move_interval", "ramp_index", "shot_timer")) == (5, 2, 0, -1, 12, 10, 12, 0, 0)
               for i in range(3))
    # sticky_p = 1: every coin is below it, the first action (no-op) repeats for ever
    host = HostSpaceInvaders(6, seed=seed, sticky_action_prob=1.0)
    host.reset()
    for _ in range(9):
        host.step(np.full(6, 1))
    assert all(e["last_action"] == 0 and e["pos"] == 5 for e in host.envs)


def test_sticky_coin_counts_and_zero_never_repeats():
    GS.sticky_coin_check(GAME, steps=200, free_steps=100)


def test_the_philox_run_of_the_gpu_test_shows_a_kill_a_terminal_a_truncation_and_a_turn():
    """tests/test_gpu_invaders.py's Philox-path run (n = 5, 300 steps, limit 60, sticky_p = 0.25, actions of RandomState(7)) on
    ``HostSpaceInvaders`` alone."""
    host, (kills, terminals, truncations) = GS.philox_host_run(GAME)
    turns = host.branches["turn_at_column_0"] + host.branches["turn_at_column_9"]
    print(f"kills {kills}, terminals {terminals}, truncations {truncations}, turns {turns}")
    assert kills >= 1 and terminals >= 1 and truncations >= 1 and turns >= 1 and host.branches["alien_shot"] >= 1
    assert terminals == host.branches["terminal"] and truncations == host.branches["truncation"]


# ---------------------------------------------------------------------- the host side of the device environment
@pytest.fixture(scope="module")
def lib():
    return GS.native_lib()


def test_symbols_exported_declared_and_mirrored(lib):
    src, signatures = GS.symbols_check(lib, GAME)
    # no draw pointer at either entry point: the step is Breakout's signature without its draw array
    breakout = signatures["prism_env_breakout_step"]
    assert signatures["prism_env_invaders_step"] == (breakout[0], breakout[1][:3] + breakout[1][4:])
    assert signatures["prism_env_invaders_reset"] == signatures["prism_env_asterix_reset"] and len(signatures["prism_env_invaders_reset"][1]) == 2
    assert "int prism_env_invaders_reset(const prism_env_desc *d, prism_stream_t stream);" in src
    assert re.search(r"int prism_env_invaders_step\(const prism_env_desc \*d, const int64_t \*actions, const double \*u_in, int32_t parity,\s+"
                     r"prism_stream_t stream\);", src)


assert len(GS.refusals(GAME)) == len(GS.ENV_REFUSALS) + 2          # 4 or 6 (4 is among the counts Breakout's table refuses)


@pytest.mark.parametrize("entry", ["reset", "step"])
@pytest.mark.parametrize("case", range(len(GS.refusals(GAME))))
def test_env_refusals_without_device(lib, entry, case):
    """Every refusal of Breakout's table, with the same text but for the action counts, through this game's entry points."""
    GS.refusal_check(lib, GAME, entry, case)


def test_step_refuses_null_actions_and_bad_parity(lib):
    GS.null_actions_and_parity_check(lib, GAME)


def test_the_kernels_have_no_private_and_no_group_segment(tmp_path):
    """Read from the code object's metadata of env_invaders.hip (block and bullet rows are reached by shifts of scalar words:
    an array indexed by a row or a column would land in the private segment)."""
    assert set(GS.kernel_segments(GAME, tmp_path).values()) == {(0, 0)}


def test_named_constants_stand_once_on_each_side():
    """The block size, its first place and the three intervals are named constants, once in the kernel and once in the host
    restatement, and the two agree."""
    from tests import invaders_ref as R
    src = open(os.path.join(H.ROOT, "prism_amd", "csrc", "env_invaders.hip")).read()
    want = dict(SI_ROWS=R.BLOCK_ROWS, SI_COLS=R.BLOCK_COLS, SI_FIRST_X=R.FIRST_X, SI_FIRST_Y=R.FIRST_Y, SI_SHOT_COOL_DOWN=R.SHOT_COOL_DOWN,
                SI_ENEMY_SHOT_INTERVAL=R.ENEMY_SHOT_INTERVAL, SI_ENEMY_MOVE_INTERVAL=R.ENEMY_MOVE_INTERVAL, SI_MOVE_INTERVAL_MIN=R.MOVE_INTERVAL_MIN)
    for name, value in want.items():
        found = re.findall(r"\b" + name + r" = (\d+)\b", src)
        assert found == [str(value)], (name, found)
    assert (R.BLOCK_ROWS, R.BLOCK_COLS, R.FIRST_X, R.FIRST_Y) == (4, 6, 2, 0)
    assert (R.SHOT_COOL_DOWN, R.ENEMY_SHOT_INTERVAL, R.ENEMY_MOVE_INTERVAL, R.MOVE_INTERVAL_MIN) == (5, 10, 12, 6)


def test_state_codec_round_trips_and_refuses():
    from prism_amd.envs import pack_invaders_state, render_invaders, unpack_invaders_state
    for group in IC.GROUPS:
        state, _, _ = IC.vector(group, 31)
        words = pack_invaders_state(state)
        assert words.shape == (31, 8) and words.dtype == np.int32
        back = unpack_invaders_state(words)
        assert sorted(back) == sorted(state)
        assert_same_state(back, state, group)
        np.testing.assert_array_equal(pack_invaders_state(back), words)          # the words exactly
        host = HostSpaceInvaders(31)
        host.set_state(state)
        assert_same_state(host.get_state(), state, group)
        np.testing.assert_array_equal(render_invaders(state).astype(np.float32), host.observe())
    # ep_steps and t sit where the other games keep them; the fields of words 0, 6 and 7 where include/prism_hip.h puts them
    state = IC.vector("plain", 3)[0]
    state["ep_steps"], state["t"] = np.array([1, 2, 3]), np.array([2 ** 40 + 5, 6, 2 ** 64 - 1], dtype=np.uint64)
    state["alien_x"], state["alien_y"], state["alien_dir"] = np.array([0, 2, 4]), np.array([9, 0, 5]), np.array([1, -1, 1])
    state["f_bullet_x"][0], state["e_bullet_x"][0] = np.arange(10) - 1, 8 - np.arange(10)
    state["pos"], state["shot_timer"], state["last_action"] = np.array([9, 0, 3]), np.array([5, 0, 2]), np.array([5, 0, 4])
    state["alien_move_timer"], state["alien_shot_timer"] = np.array([12, 0, 7]), np.array([10, 0, 3])
    state["enemy_move_interval"], state["ramp_index"] = np.array([6, 12, 9]), np.array([6, 0, 3])
    w = pack_invaders_state(state).view(np.uint32)
    assert list(w[:, 2]) == [1, 2, 3] and list(w[:, 4]) == [5, 6, 2 ** 32 - 1] and list(w[:, 5]) == [256, 0, 2 ** 32 - 1]
    assert list(w[:, 0] >> 24) == [5 | 9 << 4, 7, 9 | 5 << 4] and list(w[:, 0] & 0xFFFFFF) == [0xFFFFFF] * 3
    assert w[0, 1] == 0x76543210 and w[0, 3] == 0x23456789 and w[0, 6] & 0xFFFF == 0x0198
    assert list(w[:, 6] >> 16) == [9 | 5 << 4 | 1 << 7 | 5 << 8, 0, 3 | 2 << 4 | 1 << 7 | 4 << 8]
    assert list(w[:, 7]) == [12 | 10 << 4 | 6 << 8 | 6 << 12, 12 << 8, 7 | 3 << 4 | 9 << 8 | 3 << 12]
    assert_same_state(unpack_invaders_state(w), state, "edited")
    for field, value in (("pos", 10), ("pos", -1), ("alien_x", -6), ("alien_x", 10), ("alien_y", 10), ("alien_y", -1), ("alien_dir", 0),
                         ("alien_dir", 2), ("alien_move_timer", 13), ("alien_move_timer", -1), ("alien_shot_timer", 11),
                         ("enemy_move_interval", 5), ("enemy_move_interval", 13), ("ramp_index", 7), ("ramp_index", -1),
                         ("shot_timer", 6), ("shot_timer", -1), ("last_action", 6)):
        bad = IC.vector("plain", 2)[0]
        bad[field] = np.array([bad[field][0], value])
        with pytest.raises(ValueError, match=f"DeviceSpaceInvaders.set_state: {field}"):
            pack_invaders_state(bad)
    for field, at, value in (("alien_block", (1, 2, 3), 2), ("alien_block", (1, 0, 0), -1), ("f_bullet_x", (1, 4), 10), ("f_bullet_x", (1, 0), -2),
                             ("e_bullet_x", (1, 9), 10), ("e_bullet_x", (1, 9), -2)):
        bad = IC.vector("plain", 2)[0]
        bad[field][at] = value
        with pytest.raises(ValueError, match=f"DeviceSpaceInvaders.set_state: {field}"):
            pack_invaders_state(bad)
    bad = IC.vector("plain", 2)[0]
    bad["alien_block"][1] = 0                                                  # an empty block
    with pytest.raises(ValueError, match="DeviceSpaceInvaders.set_state: alien_block is empty"):
        pack_invaders_state(bad)
    for x, column in ((-1, 0), (5, 5), (-5, 4), (9, 1)):                       # a live alien off the board, at either side
        bad = IC.vector("plain", 2)[0]
        bad["alien_block"][1] = 0
        bad["alien_block"][1, 2, column] = 1
        bad["alien_x"][1] = x
        with pytest.raises(ValueError, match="DeviceSpaceInvaders.set_state: alien_x puts a live alien"):
            pack_invaders_state(bad)
        bad["alien_x"][1] = x + (1 if x < 0 else -1)                           # one column further in: accepted
        pack_invaders_state(bad)


def test_the_base_class_gained_only_the_step_without_draws():
    from prism_amd import envs
    SI = envs.DeviceSpaceInvaders
    assert SI.OBS_SHAPE == envs.SPACEINVADERS_OBS_SHAPE == (10, 10, 6) and issubclass(SI, envs._DeviceEnv)
    assert [c._MINIMAL_ACTIONS for c in (envs.DeviceBreakout, envs.DeviceFreeway, envs.DeviceAsterix, SI)] == [3, 3, 5, 4]
    assert [c._STEP_DRAWS for c in (envs.DeviceBreakout, envs.DeviceFreeway, envs.DeviceAsterix, SI)] == [True, True, True, False]
    assert [c._RESET_DRAWS for c in (envs.DeviceBreakout, envs.DeviceFreeway, envs.DeviceAsterix, SI)] == [True, True, False, False]
    for shared in ("observe", "close", "check_status", "get_state", "set_state", "state_dict", "load_state_dict", "_stage_actions",
                   "_reset", "_step"):
        assert getattr(SI, shared) is getattr(envs._DeviceEnv, shared)
    assert SI._pack is envs.pack_invaders_state and SI._unpack is envs.unpack_invaders_state and SI._render is envs.render_invaders
    import inspect
    assert list(inspect.signature(SI.step).parameters) == ["self", "actions", "u"] and list(inspect.signature(SI.reset).parameters) == ["self"]


def test_factory_knob_off_on_and_bad(monkeypatch):
    from prism_amd import envs
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.factory import collector_factory, env_factory
    made = GS.fake_device_classes(monkeypatch, GAME, ("SpaceInvaders", "Asterix", "Freeway", "Breakout"))
    assert env_factory.DEVICE_GAMES["SpaceInvaders"] == "DeviceSpaceInvaders" and env_factory.DEFAULT_DEVICE_GAMES == ("Breakout",)
    assert sorted(set(env_factory.MINATAR_GAMES) - set(env_factory.DEVICE_GAMES)) == ["Seaquest"]
    cfg = baseline_config(2, device="cuda:0", env_name="MinAtar/SpaceInvaders-v1", atari_sticky_actions_prob=0.1, num_processes=9,
                          seed=31, episode_timestep_limit=777)
    # the knob off: refused as before, and the text says how to enable the game
    with pytest.raises(NotImplementedError, match="SpaceInvaders.*device_env_games"):
        env_factory.build_environment(cfg, 5)
    with pytest.raises(NotImplementedError, match="SpaceInvaders"):
        collector_factory.build_collector(cfg)
    cfg.device_env_games = ("Breakout", "Freeway", "Asterix")
    with pytest.raises(NotImplementedError, match="SpaceInvaders"):
        env_factory.build_environment(cfg, 5)
    assert made == []
    # the knob on
    cfg.device_env_games = ("Breakout", "Freeway", "Asterix", "SpaceInvaders")
    assert isinstance(env_factory.build_environment(cfg, 5), envs.DeviceSpaceInvaders)
    assert made == [("SpaceInvaders", (5, 31, "cuda:0"), dict(sticky_action_prob=0.1, episode_timestep_limit=777, minimal_actions=True))]
    cfg.env_name = "MinAtar/SpaceInvaders-v0"
    env_factory.build_environment(cfg, 3, seed=8)
    assert made[-1][:2] == ("SpaceInvaders", (3, 8, "cuda:0")) and made[-1][2]["minimal_actions"] is False
    col = collector_factory.build_collector(cfg)
    assert isinstance(col, VectorCollector) and isinstance(col.envs, envs.DeviceSpaceInvaders) and made[-1][1][0] == 9
    for game in ("Breakout", "Freeway", "Asterix"):
        cfg.env_name = f"MinAtar/{game}-v1"
        env_factory.build_environment(cfg, 4)
        assert made[-1][0] == game
    cfg.env_name = "MinAtar/Seaquest-v1"                                       # still not on the device
    with pytest.raises(NotImplementedError, match="Seaquest is not implemented"):
        env_factory.build_environment(cfg, 4)
    cfg.device_env_games = "SpaceInvaders"                                     # one name; the others are then off
    cfg.env_name = "MinAtar/SpaceInvaders-v1"
    env_factory.build_environment(cfg, 2)
    assert made[-1][0] == "SpaceInvaders"
    cfg.env_name = "MinAtar/Breakout-v1"
    with pytest.raises(NotImplementedError, match="Breakout"):
        env_factory.build_environment(cfg, 2)
    # a bad knob value
    for bad in (("SpaceInvaders", "Seaquest"), ("spaceinvaders",), "Space Invaders"):
        cfg.device_env_games = bad
        cfg.env_name = "MinAtar/SpaceInvaders-v1"
        with pytest.raises(ValueError, match="device_env_games"):
            env_factory.build_environment(cfg, 2)
    n = len(made)
    cfg.device_env_games = ("SpaceInvaders",)
    for name in ("ALE/SpaceInvaders-v5", "MinAtar/Pong-v1", "SpaceInvaders-v1"):
        cfg.env_name = name
        with pytest.raises(ValueError):
            env_factory.build_environment(cfg, 4)
    assert len(made) == n


def test_the_real_class_counts_four_minimal_actions_before_it_needs_a_device():
    """``DeviceSpaceInvaders.__init__`` sets nothing before its checks; the action count is the class's."""
    from prism_amd import _native as N
    from prism_amd.envs import DeviceSpaceInvaders
    with pytest.raises(N.NativeLibraryError, match="DeviceSpaceInvaders needs a GPU device"):
        DeviceSpaceInvaders(2, 1, "cpu", minimal_actions=True)
    with pytest.raises(ValueError, match="DeviceSpaceInvaders: n_envs"):
        DeviceSpaceInvaders(0, 1, "cuda:0")
    with pytest.raises(ValueError, match="DeviceSpaceInvaders: obs_dtype"):
        DeviceSpaceInvaders(2, 1, "cuda:0", obs_dtype="float16")


def test_snapshot_kind_mismatch_is_refused():
    from prism_amd.envs import DeviceAsterix, DeviceSpaceInvaders
    bare, snap = GS.bare, GS.snap
    with pytest.raises(ValueError, match="kind = 'DeviceBreakout' in the snapshot, 'DeviceSpaceInvaders' here"):
        bare(DeviceSpaceInvaders).load_state_dict(snap("DeviceBreakout"))
    with pytest.raises(ValueError, match="kind = 'DeviceAsterix' in the snapshot, 'DeviceSpaceInvaders' here"):
        bare(DeviceSpaceInvaders).load_state_dict(snap("DeviceAsterix"))
    with pytest.raises(ValueError, match="kind = 'DeviceSpaceInvaders' in the snapshot, 'DeviceAsterix' here"):
        bare(DeviceAsterix).load_state_dict(snap("DeviceSpaceInvaders"))
    bare(DeviceSpaceInvaders).load_state_dict(snap("DeviceSpaceInvaders"))     # its own kind, never started: accepted
    bare(DeviceSpaceInvaders, 4).load_state_dict(snap("DeviceSpaceInvaders", 4))
    with pytest.raises(ValueError, match="n_actions"):
        bare(DeviceSpaceInvaders).load_state_dict(snap("DeviceSpaceInvaders", 4))
