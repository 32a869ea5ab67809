"""The case table of the Asterix rules: crafted start states and action scripts that reach every branch of the
step -- play from reset never fills all eight slots and never gets past ramp_index 7; a spawn onto the player's cell, the
clamped rank, both exits, the clipped trails and the last ramp need a prepared board.

A case: a start state (``start(...)``: the player on (5, 5), an empty board, the timers of a reset, fields replaced; ``ents``
are (slot, x, dir, gold) tuples), a script of (action, coin u, (side, gold, rank) of a spawn on this step) per step, and the
branches (tests/asterix_ref.py BRANCHES) it must reach.  Cases that share (n_actions, step_limit, sticky_p) form a GROUP: they
run side by side as the environments of one vector."""
import numpy as np

NOOP, LEFT, UP, RIGHT, DOWN, FIRE = 0, 1, 2, 3, 4, 5          # the six actions n, l, u, r, d, f
NONE = (0, 0, 0)


def start(ents=(), **over):
    s = dict(px=5, py=5, spawn_speed=10, spawn_timer=10, move_speed=5, move_timer=5, ramp_timer=100, ramp_index=0, last_action=0,
             ep_steps=0, t=0, ent_active=[0] * 8, ent_x=[0] * 8, ent_dir=[0] * 8, ent_gold=[0] * 8)
    for slot, x, d, gold in ents:
        s["ent_active"][slot], s["ent_x"][slot], s["ent_dir"][slot], s["ent_gold"][slot] = 1, x, d, gold
    s.update(over)
    return s


def board(empty, **over):
    """Every slot but those of ``empty`` holds a waiting enemy on column 2 (the player is on (5, 5): nobody touches)."""
    return start(ents=[(i, 2, 1 if i % 2 else -1, 0) for i in range(8) if i not in empty], spawn_timer=0, **over)


def acts(*actions, u=0.9, spawn=NONE):
    return [(a, u, spawn) for a in actions]


def noops(k, u=0.9, spawn=NONE):
    return acts(*([NOOP] * k), u=u, spawn=spawn)


CASES = {
    # ---- group (6 actions, no step limit, no sticky actions)
    "moves_left_up": dict(group="plain", state=start(px=1, py=2), script=acts(LEFT, LEFT, UP, UP),
                          reach=["move_left", "clamp_left", "move_up", "clamp_top", "entities_wait"]),
    "moves_right_down": dict(group="plain", state=start(px=8, py=7), script=acts(RIGHT, RIGHT, DOWN, DOWN, FIRE),
                             reach=["move_right", "clamp_right", "move_down", "clamp_bottom", "fire_noop"]),
    # spawns into the 0th, a middle and the last of k = 8, 3 and 1 empty slots; both sides, both kinds
    "spawn_k8_first": dict(group="plain", state=start(spawn_timer=0), script=noops(1, spawn=(1, 1, 0)) + noops(1),
                           reach=["spawn_first", "spawn_left", "spawn_gold"]),
    "spawn_k8_middle": dict(group="plain", state=start(spawn_timer=0), script=noops(1, spawn=(0, 0, 3)) + noops(1),
                            reach=["spawn_middle", "spawn_right", "spawn_enemy"]),
    "spawn_k8_last": dict(group="plain", state=start(spawn_timer=0), script=noops(1, spawn=(1, 0, 7)) + noops(1),
                          reach=["spawn_last", "spawn_left", "spawn_enemy"]),
    "spawn_k3_first": dict(group="plain", state=board({1, 4, 6}), script=noops(1, spawn=(0, 1, 0)) + noops(1),
                           reach=["spawn_first", "spawn_right", "spawn_gold"]),
    "spawn_k3_middle": dict(group="plain", state=board({1, 3, 6}), script=noops(1, spawn=(1, 1, 1)) + noops(1), reach=["spawn_middle"]),
    "spawn_k3_last": dict(group="plain", state=board({0, 3, 7}), script=noops(1, spawn=(0, 0, 2)) + noops(1), reach=["spawn_last"]),
    "spawn_k1": dict(group="plain", state=board({2}), script=noops(1, spawn=(1, 1, 0)) + noops(1), reach=["spawn_first", "spawn_last"]),
    # no empty slot: only the timer reloads (spawn_speed 1: it spawns on every step, the second step too)
    "spawn_full": dict(group="plain", state=board(set(), spawn_speed=1), script=noops(2, spawn=(1, 1, 0)), reach=["spawn_full"]),
    "rank_clamped": dict(group="plain", state=board({1, 4, 6}), script=noops(1, spawn=(1, 0, 7)) + noops(1),
                         reach=["rank_clamped", "spawn_last"]),
    # a spawn at x = 0 / x = 9 onto the player's cell: a gold is collected, an enemy ends the episode, on that step
    "spawn_gold_on_the_player": dict(group="plain", state=start(px=0, py=3, spawn_timer=0), script=noops(1, spawn=(1, 1, 2)) + noops(1),
                                     reach=["spawn_on_player_gold"]),
    "spawn_enemy_on_the_player": dict(group="plain", state=start(px=9, py=6, spawn_timer=0), script=noops(1, spawn=(0, 0, 5)) + noops(1),
                                      reach=["spawn_on_player_enemy", "terminal", "reset"]),
    # the player walks into an entity that waits
    "walk_into_gold": dict(group="plain", state=start(ents=[(3, 6, 1, 1)], py=4, move_timer=3), script=acts(RIGHT, NOOP),
                           reach=["walk_into_gold", "move_right", "entities_wait"]),
    "walk_into_enemy": dict(group="plain", state=start(ents=[(5, 4, -1, 0)], px=4, move_timer=3), script=acts(DOWN, NOOP),
                            reach=["walk_into_enemy", "terminal", "reset"]),
    # a terminal step still moves the entities, and next_obs shows them moved
    "terminal_shows_the_move": dict(group="plain", state=start(ents=[(5, 4, -1, 0), (1, 3, 1, 1)], px=4, move_timer=0),
                                    script=acts(DOWN, NOOP), reach=["walk_into_enemy", "entities_move", "terminal"]),
    # an entity walks into the player
    "gold_from_the_left": dict(group="plain", state=start(ents=[(4, 4, 1, 1)], move_timer=0), script=noops(2),
                               reach=["gold_arrives_from_left", "entities_move"]),
    "gold_from_the_right": dict(group="plain", state=start(ents=[(4, 6, -1, 1)], move_timer=0), script=noops(2),
                                reach=["gold_arrives_from_right"]),
    "enemy_from_the_left": dict(group="plain", state=start(ents=[(4, 4, 1, 0)], move_timer=0), script=noops(2),
                                reach=["enemy_arrives_from_left", "terminal", "reset"]),
    "enemy_from_the_right": dict(group="plain", state=start(ents=[(4, 6, -1, 0)], move_timer=0), script=noops(2),
                                 reach=["enemy_arrives_from_right", "terminal", "reset"]),
    # a step of waiting, then the move: both exits; trails clipped at columns 0 and 9 and present elsewhere; t carries
    "exits_and_trails": dict(group="plain", state=start(ents=[(0, 0, -1, 0), (1, 9, 1, 1), (2, 0, 1, 0), (3, 9, -1, 1), (6, 4, 1, 1)],
                                                        move_timer=1, t=2 ** 32 - 1), script=noops(3),
                             reach=["entities_wait", "entities_move", "exit_left", "exit_right", "trail_clipped_left",
                                    "trail_clipped_right", "trail_drawn"]),
    # the ramp: timer 0 -> -1 -> ramp on consecutive steps, at an even index (spawn_speed only)
    "ramp_even": dict(group="plain", state=start(ramp_timer=0), script=noops(3), reach=["ramp_timer_below_zero", "ramp_even"]),
    "ramp_odd": dict(group="plain", state=start(ramp_timer=-1, ramp_index=3, spawn_speed=7, move_speed=4, spawn_timer=7, move_timer=4),
                     script=noops(2), reach=["ramp_odd"]),
    "ramp_move_speed_at_1": dict(group="plain", state=start(ramp_timer=-1, ramp_index=9, spawn_speed=3, move_speed=1, spawn_timer=2,
                                                            move_timer=0), script=noops(2), reach=["ramp_odd", "ramp_move_speed_at_1"]),
    "ramp_last": dict(group="plain", state=start(ramp_timer=-1, ramp_index=8, spawn_speed=2, move_speed=1, spawn_timer=1, move_timer=0),
                      script=noops(3), reach=["ramp_even", "ramp_last", "ramp_frozen"]),
    # the widest index the codec takes, ramped once more
    "ramp_index_15": dict(group="plain", state=start(ramp_timer=-1, ramp_index=15, spawn_speed=5, move_speed=3, spawn_timer=4,
                                                     move_timer=2), script=noops(2), reach=["ramp_odd"]),
    # ---- group (5 actions: n, l, u, r, d; step limit 5)
    "truncation": dict(group="minimal", state=start(), script=noops(7), reach=["truncation", "reset"]),
    # the limit and the terminal on the same step: done, not truncated
    "limit_on_a_terminal": dict(group="minimal", state=start(ents=[(4, 4, 1, 0)], move_timer=0, ep_steps=4), script=noops(2),
                                reach=["terminal", "terminal_on_the_limit", "reset"]),
    "minimal_moves": dict(group="minimal", state=start(), script=acts(1, 2, 3, 4),
                          reach=["move_left", "move_up", "move_right", "move_down"]),
    # 5 is `f` of the six actions and outside the five: it acts as no-op, as -1 does
    "minimal_out_of_range": dict(group="minimal", state=start(), script=acts(-1, 5, 4), reach=["bad_action", "move_down"], bad_action=True),
    # ---- group (6 actions, sticky_p = 0.25)
    "sticky": dict(group="sticky", state=start(last_action=RIGHT),
                   script=[(LEFT, 0.1, NONE), (LEFT, 0.25, NONE), (NOOP, 0.2499, NONE), (UP, 0.0, NONE), (UP, 0.7, NONE)],
                   reach=["sticky_repeat", "move_right", "move_left", "move_up"]),
    "sticky_out_of_range": dict(group="sticky", state=start(last_action=DOWN),
                                script=[(6, 0.1, NONE), (-1, 0.9, NONE), (6, 0.9, NONE), (2 ** 40 + 1, 0.9, NONE), (FIRE, 0.9, NONE)],
                                reach=["bad_action", "sticky_repeat", "move_down", "fire_noop"], bad_action=True),
}

GROUPS = {"plain": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.0),
          "minimal": dict(minimal_actions=True, episode_timestep_limit=5, sticky_action_prob=0.0),
          "sticky": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.25)}

REQUIRED = ("move_left", "move_right", "move_up", "move_down", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom",
            "fire_noop", "spawn_left", "spawn_right", "spawn_gold", "spawn_enemy", "spawn_first", "spawn_middle", "spawn_last",
            "spawn_full", "rank_clamped", "spawn_on_player_gold", "spawn_on_player_enemy", "walk_into_gold", "walk_into_enemy",
            "gold_arrives_from_left", "gold_arrives_from_right", "enemy_arrives_from_left", "enemy_arrives_from_right",
            "entities_wait", "entities_move", "exit_left", "exit_right", "trail_clipped_left", "trail_clipped_right", "trail_drawn",
            "ramp_even", "ramp_odd", "ramp_move_speed_at_1", "ramp_last", "ramp_frozen", "ramp_timer_below_zero", "terminal",
            "truncation", "terminal_on_the_limit", "sticky_repeat", "reset", "bad_action")
SCALARS = ("px", "py", "spawn_speed", "spawn_timer", "move_speed", "move_timer", "ramp_timer", "ramp_index", "last_action",
           "ep_steps", "t")
PER_SLOT = ("ent_active", "ent_x", "ent_dir", "ent_gold")


def group_cases(group):
    return [n for n, c in CASES.items() if c["group"] == group]


def vector_names(group, n_envs, offset=0):
    names = group_cases(group)
    return [names[(offset + i) % len(names)] for i in range(n_envs)]


def vector(group, n_envs, offset=0):
    """The group's cases laid over ``n_envs`` environments (environment i runs case offset + i modulo the number of cases;
    scripts are padded with no-ops): (state dict of arrays, actions [steps][n] int64, u [steps][n] float64, spawn
    [steps][n][3] uint8).  Offsets 0, n_envs, 2 n_envs, ... below the number of cases cover the whole group."""
    pick = [CASES[name] for name in vector_names(group, n_envs, offset)]
    steps = max(len(c["script"]) for c in pick)
    state = {k: np.array([c["state"][k] for c in pick], dtype=np.uint64 if k == "t" else np.int64) for k in SCALARS}
    for k in PER_SLOT:
        state[k] = np.array([c["state"][k] for c in pick], dtype=np.int64)
    script = [[(c["script"][s] if s < len(c["script"]) else (NOOP, 0.9, NONE)) for c in pick] for s in range(steps)]
    actions = np.array([[x[0] for x in row] for row in script], dtype=np.int64)
    u = np.array([[x[1] for x in row] for row in script], dtype=np.float64)
    spawn = np.array([[x[2] for x in row] for row in script], dtype=np.uint8)
    return state, actions, u, spawn
