"""The case table of the Seaquest rules: crafted start states and scripts that between them reach every branch
of the step.  Play from reset reaches little of it (three enemies on one cell, a refused seventh diver, the end of the ramp
and a full array need a prepared state).

A case: a start state (``start(...)``: the state of a reset, fields replaced; the sub usually under water), a script of
(action, coin u, draws) per step -- draws = (enemy side, is_sub, row, diver side, row), used only on a step that spawns --
and the branches (tests/seaquest_ref.py BRANCHES) it must reach.  Cases that share (step_limit, sticky_p) form a GROUP: they
run side by side as the environments of one vector.  Entries are (x, y, dir) for bullets, (x, y, dir, move_timer) for fish
and divers, (x, y, dir, move_timer, shot_timer) for enemy subs; dir is +1 / -1."""
import numpy as np

NOOP, LEFT, UP, RIGHT, DOWN, FIRE = 0, 1, 2, 3, 4, 5          # the six actions n, l, u, r, d, f
DRAWS = (1, 0, 1, 1, 1)                                       # what a script gives where the step's draws do not matter
SCALARS = ("sub_x", "sub_y", "sub_or", "oxygen", "diver_count", "surface", "shot_timer", "e_spawn_speed", "e_spawn_timer",
           "d_spawn_timer", "move_speed", "ramp_index", "last_action", "ep_steps", "t")
LISTS = ("f_bullets", "e_bullets", "e_fish", "e_subs", "divers")


def start(**over):
    s = dict(sub_x=5, sub_y=0, sub_or=0, oxygen=200, diver_count=0, surface=1, shot_timer=0, e_spawn_speed=20, e_spawn_timer=20,
             d_spawn_timer=30, move_speed=5, ramp_index=0, last_action=0, ep_steps=0, t=0,
             f_bullets=[], e_bullets=[], e_fish=[], e_subs=[], divers=[])
    s.update(over)
    return s


def deep(**over):
    """The sub under water at (2, 2), facing -x, away from the rows the cases use."""
    return start(**{**dict(sub_x=2, sub_y=2, surface=0), **over})


def acts(*actions, u=0.9, draws=DRAWS):
    return [(a, u, draws) for a in actions]


def noops(k, u=0.9, draws=DRAWS):
    return acts(*([NOOP] * k), u=u, draws=draws)


# 32 fish that all move to +x, four per row, their timers at 5: nothing moves during a short script
FISH_32 = [(k % 10, 1 + k % 8, 1, 5) for k in range(32)]
BULLETS_32 = [(2 + k % 6, 1 + k % 8, 1 if k % 2 else -1) for k in range(32)]          # enemy bullets on columns 2..7

CASES = {
    # ---- group (no step limit, no sticky actions)
    "spawn_fish_from_the_left_and_a_diver": dict(group="plain", state=deep(e_spawn_timer=0, d_spawn_timer=0, t=2 ** 32 - 1),
                                                 script=noops(2, draws=(1, 0, 3, 1, 8)),
                                                 reach=["spawn_fish", "spawn_from_left", "spawn_diver"]),
    "spawn_sub_from_the_right_and_a_diver": dict(group="plain", state=deep(e_spawn_timer=0, d_spawn_timer=0, move_speed=3),
                                                 script=noops(2, draws=(0, 1, 8, 0, 1)),
                                                 reach=["spawn_sub", "spawn_from_right", "spawn_diver"]),
    "spawn_blocked_by_a_fish": dict(group="plain", state=deep(e_spawn_timer=0, e_fish=[(4, 3, -1, 2)]), script=noops(2, draws=(1, 0, 3, 1, 1)),
                                    reach=["spawn_blocked"]),
    "spawn_blocked_by_a_sub": dict(group="plain", state=deep(e_spawn_timer=0, e_spawn_speed=7, e_subs=[(4, 3, 1, 2, 7)]),
                                   script=noops(2, draws=(0, 1, 3, 1, 1)), reach=["spawn_blocked"]),
    "spawn_beside_the_same_direction": dict(group="plain", state=deep(e_spawn_timer=0, e_subs=[(4, 3, 1, 2, 7)], e_fish=[(8, 3, 1, 1)]),
                                            script=noops(2, draws=(1, 0, 3, 1, 1)), reach=["spawn_beside_same_direction", "spawn_fish"]),
    "the_sub_moves": dict(group="plain", state=deep(sub_x=1, sub_y=1), script=acts(LEFT, LEFT, RIGHT, UP, DOWN, DOWN),
                          reach=["move_left", "clamp_left", "move_right", "move_up", "move_down", "under_water"]),
    "the_sub_at_the_far_corner": dict(group="plain", state=deep(sub_x=8, sub_y=7, sub_or=1), script=acts(RIGHT, RIGHT, DOWN, DOWN, NOOP),
                                      reach=["move_right", "clamp_right", "move_down", "clamp_down", "noop"]),
    "at_the_surface": dict(group="plain", state=start(), script=acts(UP, NOOP), reach=["clamp_up", "at_surface_already"]),
    "fire_and_cool_down": dict(group="plain", state=deep(sub_x=6, sub_or=1), script=acts(FIRE, FIRE, NOOP, NOOP, NOOP, FIRE, NOOP),
                               reach=["fire", "fire_cooling", "f_bullet_flies", "f_bullet_leaves_right"]),
    "bullets_leave_at_both_edges": dict(group="plain", state=deep(f_bullets=[(9, 3, 1), (0, 5, -1)], e_bullets=[(0, 6, -1), (9, 7, 1)]),
                                        script=noops(2), reach=["f_bullet_leaves_left", "f_bullet_leaves_right", "e_bullet_leaves_left",
                                                                "e_bullet_leaves_right"]),
    # three fish on (6, 4): the first in list order dies, the timers of the two that stay show which
    "three_fish_on_one_cell": dict(group="plain", state=deep(f_bullets=[(5, 4, 1)], e_fish=[(6, 4, -1, 3), (6, 4, -1, 1), (6, 4, -1, 2)]),
                                   script=noops(2), reach=["f_bullet_hits_fish", "f_bullet_picks_first_of_stack"]),
    "three_subs_on_one_cell": dict(group="plain", state=deep(f_bullets=[(7, 4, -1)], e_subs=[(6, 4, 1, 3, 9), (6, 4, 1, 1, 8), (6, 4, 1, 2, 7)]),
                                   script=noops(2), reach=["f_bullet_hits_sub", "f_bullet_picks_first_of_stack"]),
    "a_fish_and_a_sub_on_one_cell": dict(group="plain", state=deep(f_bullets=[(5, 4, 1)], e_subs=[(6, 4, -1, 3, 5)], e_fish=[(1, 7, 1, 4), (6, 4, -1, 3)]),
                                         script=noops(2), reach=["f_bullet_hits_fish", "f_bullet_prefers_fish"]),
    # two bullets, last to first: the second one kills the fish, the first one then finds the sub behind it
    "two_bullets_one_step": dict(group="plain", state=deep(f_bullets=[(5, 4, 1), (5, 4, 1)], e_subs=[(6, 4, -1, 3, 5)], e_fish=[(6, 4, -1, 3)]),
                                 script=noops(2), reach=["f_bullet_hits_fish", "f_bullet_hits_sub"]),
    # rule 7: of two subs that walk onto one bullet the LAST in list order (shot_timer 3) dies; the first goes on
    "subs_walk_onto_a_bullet": dict(group="plain", state=deep(f_bullets=[(5, 4, 1)], e_subs=[(7, 4, -1, 0, 5), (7, 4, -1, 0, 3)]),
                                    script=noops(2), reach=["sub_walks_onto_bullet", "sub_moves"]),
    # two bullets on one cell, two subs: each sub takes one, the first bullet in list order goes to the last sub
    "two_subs_two_bullets": dict(group="plain", state=deep(f_bullets=[(7, 4, -1), (5, 4, 1), (5, 6, 1)], e_subs=[(7, 4, -1, 0, 5), (1, 1, 1, 2, 4), (7, 4, -1, 0, 3)]),
                                 script=noops(2), reach=["sub_walks_onto_bullet"]),
    "a_fish_walks_onto_a_bullet": dict(group="plain", state=deep(f_bullets=[(7, 4, -1)], e_fish=[(5, 4, 1, 0), (0, 4, 1, 0)], move_speed=2),
                                       script=noops(2), reach=["fish_walks_onto_bullet", "fish_moves"]),
    "a_sub_fires_on_the_step_it_moves": dict(group="plain", state=deep(e_subs=[(7, 4, -1, 0, 0)], move_speed=4), script=noops(3),
                                             reach=["sub_fires", "sub_fires_on_its_move", "sub_moves", "sub_counts_down", "e_bullet_flies"]),
    # two subs of one row fire on one step: the LAST in list order fires first, so its bullet stands first
    "two_enemy_bullets_in_one_row": dict(group="plain", state=deep(e_subs=[(7, 4, -1, 2, 0), (4, 4, -1, 2, 0)]), script=noops(2),
                                         reach=["sub_fires", "sub_waits", "two_e_bullets_in_a_row"]),
    "enemies_leave": dict(group="plain", state=deep(e_subs=[(0, 4, -1, 0, 0), (9, 5, 1, 0, 3)], e_fish=[(9, 6, 1, 0), (0, 7, -1, 0), (3, 7, -1, 1)]),
                          script=noops(2), reach=["sub_leaves", "fish_leaves", "fish_waits"]),
    "diver_picked_up_before_its_move": dict(group="plain", state=deep(divers=[(2, 2, 1, 3)]), script=noops(2), reach=["diver_picked_before_move"]),
    "diver_picked_up_after_its_move": dict(group="plain", state=deep(divers=[(1, 2, 1, 0), (7, 5, -1, 0), (9, 6, 1, 0), (0, 7, -1, 2)]),
                                           script=noops(2), reach=["diver_picked_after_move", "diver_moves", "diver_leaves", "diver_waits"]),
    # five aboard, two divers on the sub's cell: the last in list order is the sixth, the first is refused and stays
    "a_refused_seventh_diver": dict(group="plain", state=deep(diver_count=5, divers=[(2, 2, 1, 3), (2, 2, -1, 2)]), script=noops(2),
                                    reach=["diver_picked_before_move", "diver_refused", "diver_waits"]),
    "a_refused_diver_moves_on": dict(group="plain", state=deep(diver_count=6, divers=[(2, 2, 1, 0), (1, 2, 1, 0)]), script=noops(2),
                                     reach=["diver_refused", "diver_moves"]),
    "surfacing_without_divers": dict(group="plain", state=deep(sub_y=1), script=acts(UP, NOOP), reach=["surface_without_divers", "terminal", "reset"]),
    "surfacing_with_three": dict(group="plain", state=deep(sub_y=1, diver_count=3, oxygen=90), script=acts(UP, NOOP, DOWN, UP),
                                 reach=["surface_with_some", "ramp_spawn_speed_only", "ramp_move_speed", "at_surface_already"]),
    "surfacing_with_six": dict(group="plain", state=deep(sub_y=1, diver_count=6, oxygen=150, ramp_index=1), script=acts(UP, NOOP),
                               reach=["surface_with_six", "ramp_move_speed"]),
    "surfacing_at_the_slowest_move_speed": dict(group="plain", state=deep(sub_y=1, diver_count=2, move_speed=2, e_spawn_speed=5, ramp_index=15),
                                                script=acts(UP, NOOP), reach=["surface_with_some", "ramp_spawn_speed_only"]),
    "surfacing_at_the_ramps_last_step": dict(group="plain", state=deep(sub_y=1, diver_count=1, move_speed=2, e_spawn_speed=2, ramp_index=18),
                                             script=acts(UP, DOWN, UP), reach=["surface_with_some", "ramp_spawn_speed_only", "surface_without_divers"]),
    "surfacing_after_the_ramps_end": dict(group="plain", state=deep(sub_y=1, diver_count=6, oxygen=199, move_speed=2, e_spawn_speed=1, ramp_index=19),
                                          script=acts(UP, NOOP), reach=["surface_with_six", "ramp_over"]),
    "oxygen_runs_out": dict(group="plain", state=deep(oxygen=0), script=noops(3), reach=["oxygen_out", "terminal", "reset"]),
    # the floor of -1 * 10 / 200 is -1: the reward of a terminal step
    "surfacing_with_six_and_no_oxygen": dict(group="plain", state=deep(sub_y=1, diver_count=6, oxygen=-1), script=acts(UP, NOOP),
                                             reach=["oxygen_out", "surface_with_six", "terminal"]),
    "a_sub_on_the_sub_before_its_move": dict(group="plain", state=deep(e_subs=[(2, 2, 1, 3, 5)]), script=noops(2),
                                             reach=["sub_contact_before_move", "terminal", "reset"]),
    "a_sub_onto_the_sub": dict(group="plain", state=deep(e_subs=[(1, 2, 1, 0, 0)]), script=noops(2), reach=["sub_contact_after_move", "sub_fires", "terminal"]),
    "a_fish_on_the_sub_before_its_move": dict(group="plain", state=deep(e_fish=[(2, 2, -1, 0)]), script=noops(2),
                                              reach=["fish_contact_before_move", "terminal"]),
    "a_fish_onto_the_sub": dict(group="plain", state=deep(e_fish=[(3, 2, -1, 0)]), script=noops(2), reach=["fish_contact_after_move", "terminal"]),
    "an_enemy_bullet_on_the_sub": dict(group="plain", state=deep(e_bullets=[(2, 2, 1)]), script=noops(2), reach=["e_bullet_contact_before_move", "terminal"]),
    "an_enemy_bullet_onto_the_sub": dict(group="plain", state=deep(e_bullets=[(6, 5, 1), (3, 2, -1)]), script=noops(2),
                                         reach=["e_bullet_contact_after_move", "terminal"]),
    # 31 fish and a spawn: the array is full afterwards and nothing is lost
    "a_full_fish_array": dict(group="plain", state=start(e_fish=FISH_32[:31], e_spawn_timer=0), script=noops(2, draws=(1, 0, 5, 1, 1)),
                              reach=["spawn_fish", "spawn_beside_same_direction", "fish_waits"]),
    # ---- group (no step limit, no sticky actions): appends to a full array are dropped, on both sides, and reported
    "overflow_of_the_fish": dict(group="overflow", state=start(e_fish=FISH_32, e_spawn_timer=0), script=noops(2, draws=(1, 0, 5, 1, 1)),
                                 reach=["overflow", "spawn_fish"], overflow=True),
    # the transient inside a step: the sub fires (rule 7) before the bullets that leave are removed (rule 8)
    "overflow_of_the_enemy_bullets": dict(group="overflow", state=start(e_bullets=BULLETS_32, e_subs=[(4, 3, 1, 2, 0)]), script=noops(2),
                                          reach=["overflow", "sub_fires"], overflow=True),
    "overflow_of_the_friendly_bullets_and_divers": dict(group="overflow", state=start(f_bullets=[(4, 1, 1), (5, 1, 1), (4, 2, -1), (5, 2, -1)],
                                                                                      divers=[(3, 5, 1, 4), (4, 5, 1, 4), (5, 5, 1, 4), (6, 5, 1, 4)],
                                                                                      d_spawn_timer=0),
                                                        script=acts(FIRE, NOOP), reach=["overflow", "fire", "spawn_diver"], overflow=True),
    # ---- group (step limit 5)
    "truncation": dict(group="limited", state=start(), script=noops(7), reach=["truncation", "reset"]),
    # the limit and the terminal on the same step: done, not truncated
    "limit_on_a_terminal": dict(group="limited", state=deep(e_bullets=[(3, 2, -1)], ep_steps=4), script=noops(2),
                                reach=["terminal", "terminal_on_the_limit", "e_bullet_contact_after_move", "reset"]),
    # ---- group (sticky_p = 0.25)
    # (n, 0.1: repeats f) (n, 0.2499: repeats f, cooling) (l, 0.25: not below p) (r, 0: repeats l) (r)
    "sticky_fire": dict(group="sticky", state=deep(sub_x=5, last_action=FIRE),
                        script=[(NOOP, 0.1, DRAWS), (NOOP, 0.2499, DRAWS), (LEFT, 0.25, DRAWS), (RIGHT, 0.0, DRAWS), (RIGHT, 0.7, DRAWS)],
                        reach=["sticky_repeat", "fire", "fire_cooling", "move_left", "move_right"]),
    "sticky_out_of_range": dict(group="sticky", state=deep(sub_x=5, last_action=RIGHT),
                                script=[(6, 0.1, DRAWS), (-1, 0.9, DRAWS), (6, 0.9, DRAWS), (2 ** 40 + 1, 0.9, DRAWS), (FIRE, 0.9, DRAWS)],
                                reach=["bad_action", "sticky_repeat", "move_right", "fire"], bad_action=True),
}

GROUPS = {"plain": dict(episode_timestep_limit=0, sticky_action_prob=0.0),
          "overflow": dict(episode_timestep_limit=0, sticky_action_prob=0.0),
          "limited": dict(episode_timestep_limit=5, sticky_action_prob=0.0),
          "sticky": dict(episode_timestep_limit=0, sticky_action_prob=0.25)}


def group_cases(group):
    return [n for n, c in CASES.items() if c["group"] == group]


def vector_names(group, n_envs, offset=0):
    names = group_cases(group)
    return [names[(offset + i) % len(names)] for i in range(n_envs)]


def vector(group, n_envs, offset=0):
    """The group's cases laid over ``n_envs`` environments (environment i runs case offset + i modulo the number of cases;
    scripts are padded with no-ops): (state dict, actions [steps][n] int64, u [steps][n] float64, draws [steps][n][5] uint8).
    Offsets 0, n_envs, 2 n_envs, ... below the number of cases cover the whole group."""
    pick = [CASES[name] for name in vector_names(group, n_envs, offset)]
    steps = max(len(c["script"]) for c in pick)
    state = {k: np.array([c["state"][k] for c in pick], dtype=np.uint64 if k == "t" else np.int64) for k in SCALARS}
    for k in LISTS:
        state[k] = [[tuple(x) for x in c["state"][k]] for c in pick]
    script = [[(c["script"][s] if s < len(c["script"]) else (NOOP, 0.9, DRAWS)) for c in pick] for s in range(steps)]
    actions = np.array([[x[0] for x in row] for row in script], dtype=np.int64)
    u = np.array([[x[1] for x in row] for row in script], dtype=np.float64)
    draws = np.array([[x[2] for x in row] for row in script], dtype=np.uint8)
    return state, actions, u, draws
