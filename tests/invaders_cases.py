"""The case table of the Space Invaders rules: crafted start states and action scripts that reach every branch
of the step -- play from reset reaches little (an episode ends within about 50-100 steps): a block whose outer columns are
dead, the wrapped row of a terminal descent, a shot from nine columns away, two kills in one step, a pass-through and the
last ramp need a prepared board.

A case: a start state (``start(...)``: the state of a reset, fields replaced; ``aliens`` are the live (r, c) block cells, ``f``
and ``e`` the (row, column) of friendly and enemy bullets), a script of (action, coin u) per step, and the branches
(tests/invaders_ref.py BRANCHES) it must reach.  Cases that share (n_actions, step_limit, sticky_p) form a GROUP: they run
side by side as the environments of one vector."""
import numpy as np

NOOP, LEFT, UP, RIGHT, DOWN, FIRE = 0, 1, 2, 3, 4, 5          # the six actions n, l, u, r, d, f


def start(aliens=None, f=(), e=(), **over):
    s = dict(pos=5, alien_x=2, alien_y=0, alien_dir=-1, alien_move_timer=12, alien_shot_timer=10, enemy_move_interval=12,
             ramp_index=0, shot_timer=0, last_action=0, ep_steps=0, t=0,
             alien_block=[[1 if aliens is None else 0] * 6 for _ in range(4)], f_bullet_x=[-1] * 10, e_bullet_x=[-1] * 10)
    for r, c in aliens or ():
        s["alien_block"][r][c] = 1
    for key, bullets in (("f_bullet_x", f), ("e_bullet_x", e)):
        for y, x in bullets:
            s[key][y] = x
    s.update(over)
    return s


def acts(*actions, u=0.9):
    return [(a, u) for a in actions]


def noops(k, u=0.9):
    return acts(*([NOOP] * k), u=u)


CASES = {
    # ---- group (6 actions, no step limit, no sticky actions)
    "cannon_left": dict(group="plain", state=start(pos=1), script=acts(LEFT, LEFT, UP, DOWN),
                        reach=["move_left", "clamp_left", "up_down_noop", "aliens_wait"]),
    "cannon_right": dict(group="plain", state=start(pos=8), script=acts(RIGHT, RIGHT), reach=["move_right", "clamp_right"]),
    # a shot, a refused shot, the cool-down runs out, the next shot; the first bullet reaches (3, 5) on the sixth step
    "fire_and_cool_down": dict(group="plain", state=start(), script=acts(FIRE, FIRE, NOOP, NOOP, NOOP, NOOP, FIRE),
                               reach=["fire", "fire_cooling", "kill"]),
    "friendly_bullet_leaves": dict(group="plain", state=start(f=[(0, 0), (5, 9)]), script=noops(2), reach=["f_bullet_leaves"]),
    "enemy_bullet_leaves": dict(group="plain", state=start(e=[(9, 0), (4, 9)]), script=noops(2), reach=["e_bullet_leaves"]),
    "hit_by_a_bullet": dict(group="plain", state=start(e=[(8, 5)]), script=noops(2), reach=["hit_by_bullet", "terminal", "reset"]),
    # the block moves: 24 aliens, the timer is the interval; t carries into its high word
    "aliens_left": dict(group="plain", state=start(alien_move_timer=0, t=2 ** 32 - 1), script=noops(2),
                        reach=["aliens_left", "timer_from_interval"]),
    "aliens_right": dict(group="plain", state=start(alien_move_timer=0, alien_dir=1, enemy_move_interval=9), script=noops(2),
                         reach=["aliens_right", "timer_from_interval"]),
    "turn_at_column_0": dict(group="plain", state=start(alien_x=0, alien_move_timer=0), script=noops(2), reach=["turn_at_column_0"]),
    "turn_at_column_9": dict(group="plain", state=start(alien_x=4, alien_dir=1, alien_move_timer=0), script=noops(2),
                             reach=["turn_at_column_9"]),
    # only the block's last / first column lives: the origin is as far off the board as it goes
    "turn_at_column_0_outer_columns_dead": dict(group="plain", state=start(aliens=[(0, 5), (1, 5)], alien_x=-5, alien_move_timer=0),
                                                script=noops(3), reach=["turn_at_column_0", "turn_with_dead_outer_column", "timer_from_count"]),
    "turn_at_column_9_outer_columns_dead": dict(group="plain", state=start(aliens=[(2, 0), (3, 0)], alien_x=9, alien_dir=1, alien_move_timer=0),
                                                script=noops(3), reach=["turn_at_column_9", "turn_with_dead_outer_column", "timer_from_count"]),
    # one alien: the timer is 1, it moves on every step
    "one_alien_moves_every_step": dict(group="plain", state=start(aliens=[(3, 2)], alien_move_timer=0), script=noops(4),
                                       reach=["timer_from_count", "aliens_left"]),
    "alien_on_the_cannon_before_the_move": dict(group="plain", state=start(aliens=[(3, 3), (0, 0)], alien_y=6, alien_move_timer=5),
                                                script=noops(2), reach=["alien_on_cannon_before_move", "terminal", "reset"]),
    "alien_on_the_cannon_after_the_move": dict(group="plain", state=start(aliens=[(3, 4), (1, 1)], alien_y=6, alien_move_timer=0),
                                               script=noops(2), reach=["alien_on_cannon_after_move", "aliens_left", "terminal"]),
    # the descent with an alien on row 9: terminal, that alien drawn on row 0; the same step fires from column 0, whose
    # aliens stand on board rows 0 (block row 3, wrapped) and 9 (block row 2): the largest BOARD row takes the bullet
    "terminal_descent_wraps_and_fires": dict(group="plain", state=start(aliens=[(3, 0), (2, 0), (0, 3)], alien_x=0, alien_y=6, pos=1,
                                                                        alien_move_timer=0, alien_shot_timer=0), script=noops(2),
                                             reach=["turn_at_column_0", "descent_onto_row_9", "wrapped_row_drawn", "shot_on_terminal_descent",
                                                    "alien_shot", "terminal", "reset"]),
    # the nearest column: the cannon's own, a tie (columns 3 and 7 around 5: the lower), nine columns away
    "shot_from_the_cannons_column": dict(group="plain", state=start(alien_shot_timer=0), script=noops(2), reach=["alien_shot", "shot_distance_0"]),
    "shot_tie_takes_the_lower_column": dict(group="plain", state=start(aliens=[(0, 1), (1, 5)], alien_shot_timer=0), script=noops(2),
                                            reach=["alien_shot", "shot_tie_lower_column"]),
    "shot_from_nine_columns_away": dict(group="plain", state=start(aliens=[(2, 5)], alien_x=4, alien_dir=1, pos=0, alien_shot_timer=0),
                                        script=noops(2), reach=["alien_shot", "shot_distance_9"]),
    "shot_onto_a_bullet": dict(group="plain", state=start(e=[(2, 5)], alien_shot_timer=0), script=noops(2), reach=["shot_onto_a_bullet"]),
    "single_kill": dict(group="plain", state=start(f=[(4, 5)]), script=noops(2), reach=["kill"]),
    "two_kills": dict(group="plain", state=start(f=[(4, 5), (3, 4)]), script=noops(2), reach=["kill", "two_kills"]),
    # the bullet comes up onto (3, 3) as the only alien of that column goes down to (4, 3): they swap rows, neither is lost
    "pass_through": dict(group="plain", state=start(aliens=[(3, 3), (0, 0)], alien_x=0, alien_move_timer=0, f=[(4, 3)]), script=noops(2),
                         reach=["pass_through", "turn_at_column_0"]),
    "last_alien_ramps": dict(group="plain", state=start(aliens=[(3, 3)], f=[(4, 5)], alien_move_timer=7), script=noops(2),
                             reach=["kill", "board_cleared", "ramp"]),
    "last_alien_at_the_fastest": dict(group="plain", state=start(aliens=[(3, 3)], f=[(4, 5)], enemy_move_interval=6, ramp_index=6,
                                                                 alien_move_timer=3, alien_dir=1), script=noops(2),
                                      reach=["kill", "board_cleared", "ramp_at_fastest"]),
    # ---- group (4 actions: n, l, r, f; step limit 5)
    "truncation": dict(group="minimal", state=start(), script=noops(7), reach=["truncation", "reset"]),
    # the limit and the terminal on the same step: done, not truncated
    "limit_on_a_terminal": dict(group="minimal", state=start(e=[(8, 5)], ep_steps=4), script=noops(2),
                                reach=["terminal", "terminal_on_the_limit", "hit_by_bullet", "reset"]),
    "minimal_mapping": dict(group="minimal", state=start(), script=acts(1, 2, 2, 3), reach=["move_left", "move_right", "fire"]),
    # 4 and 5 are d and f of the six actions and outside the four: they act as no-op, as -1 does
    "minimal_out_of_range": dict(group="minimal", state=start(), script=acts(-1, 4, 5, 3), reach=["bad_action", "fire"], bad_action=True),
    # ---- group (6 actions, sticky_p = 0.25)
    # (n, 0.1: repeats f) (n, 0.2499: repeats f, cooling) (l, 0.25: not below p) (r, 0: repeats l) (r)
    "sticky_fire": dict(group="sticky", state=start(last_action=FIRE),
                        script=[(NOOP, 0.1), (NOOP, 0.2499), (LEFT, 0.25), (RIGHT, 0.0), (RIGHT, 0.7)],
                        reach=["sticky_repeat", "fire", "fire_cooling", "move_left", "move_right"]),
    "sticky_out_of_range": dict(group="sticky", state=start(last_action=RIGHT),
                                script=[(6, 0.1), (-1, 0.9), (6, 0.9), (2 ** 40 + 1, 0.9), (FIRE, 0.9)],
                                reach=["bad_action", "sticky_repeat", "move_right", "fire"], bad_action=True),
}

GROUPS = {"plain": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.0),
          "minimal": dict(minimal_actions=True, episode_timestep_limit=5, sticky_action_prob=0.0),
          "sticky": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.25)}

REQUIRED = ("move_left", "move_right", "clamp_left", "clamp_right", "fire", "fire_cooling", "up_down_noop",
            "f_bullet_leaves", "e_bullet_leaves", "hit_by_bullet",
            "aliens_wait", "aliens_left", "aliens_right", "turn_at_column_0", "turn_at_column_9", "turn_with_dead_outer_column",
            "timer_from_count", "timer_from_interval", "alien_on_cannon_before_move", "alien_on_cannon_after_move",
            "descent_onto_row_9", "wrapped_row_drawn",
            "alien_shot", "shot_distance_0", "shot_tie_lower_column", "shot_distance_9", "shot_onto_a_bullet", "shot_on_terminal_descent",
            "kill", "two_kills", "pass_through", "board_cleared", "ramp", "ramp_at_fastest",
            "terminal", "truncation", "terminal_on_the_limit", "sticky_repeat", "reset", "bad_action")
SCALARS = ("pos", "alien_x", "alien_y", "alien_dir", "alien_move_timer", "alien_shot_timer", "enemy_move_interval", "ramp_index",
           "shot_timer", "last_action", "ep_steps", "t")
ARRAYS = ("alien_block", "f_bullet_x", "e_bullet_x")


def group_cases(group):
    return [n for n, c in CASES.items() if c["group"] == group]


def vector_names(group, n_envs, offset=0):
    names = group_cases(group)
    return [names[(offset + i) % len(names)] for i in range(n_envs)]


def vector(group, n_envs, offset=0):
    """The group's cases laid over ``n_envs`` environments (environment i runs case offset + i modulo the number of cases;
    scripts are padded with no-ops): (state dict of arrays, actions [steps][n] int64, u [steps][n] float64).  Offsets 0,
    n_envs, 2 n_envs, ... below the number of cases cover the whole group."""
    pick = [CASES[name] for name in vector_names(group, n_envs, offset)]
    steps = max(len(c["script"]) for c in pick)
    state = {k: np.array([c["state"][k] for c in pick], dtype=np.uint64 if k == "t" else np.int64) for k in SCALARS}
    for k in ARRAYS:
        state[k] = np.array([c["state"][k] for c in pick], dtype=np.int64)
    script = [[(c["script"][s] if s < len(c["script"]) else (NOOP, 0.9)) for c in pick] for s in range(steps)]
    actions = np.array([[x[0] for x in row] for row in script], dtype=np.int64)
    u = np.array([[x[1] for x in row] for row in script], dtype=np.float64)
    return state, actions, u
