"""The case table of the Freeway rules: crafted start states and action scripts that reach every branch of
the step -- play from reset needs some forty steps for a win and 2501 for a terminal; collisions before and after a car's
move, the wraps, the clamp and a win on the last step need a prepared road.

A case: a start state (``start(...)``: chicken on row 9 free to move, the cars of ``SPEEDS`` on column 0, fields replaced), a
script of (action, coin u, speeds that a win or a reset on this step installs) per step, and the branches
(tests/freeway_ref.py BRANCHES) it must reach.  Cases that share (n_actions, step_limit, sticky_p) form a GROUP: they run
side by side as the environments of one vector."""
import numpy as np

NOOP, LEFT, UP, RIGHT, DOWN, FIRE = 0, 1, 2, 3, 4, 5          # the six actions n, l, u, r, d, f
SPEEDS = [1, -2, 3, -4, 5, -1, 2, -3]
SLOW = [1, -1, 2, -2, 3, -3, 4, -4]
FAST = [5, -5, 4, -4, 3, -3, 5, -5]
PARKED = dict(car_x=[7] * 8, car_timer=[5] * 8, car_speed=[5, -5] * 4)          # nobody reaches column 4 within ten steps


def start(**over):
    s = dict(pos=9, move_timer=0, terminate_timer=2500, last_action=0, ep_steps=0, t=0, car_x=[0] * 8,
             car_timer=[abs(v) for v in SPEEDS], car_speed=list(SPEEDS))
    s.update(over)
    if "car_speed" in over and "car_timer" not in over:
        s["car_timer"] = [abs(v) for v in s["car_speed"]]
    return s


def one_car(row, x, timer, speed, **over):
    """The parked road with the car of ``row`` replaced."""
    cars = {k: list(v) for k, v in PARKED.items()}
    cars["car_x"][row - 1], cars["car_timer"][row - 1], cars["car_speed"][row - 1] = x, timer, speed
    return start(**cars, **over)


def acts(*actions, u=0.9, speeds=SPEEDS):
    return [(a, u, speeds) for a in actions]


def noops(k, u=0.9, speeds=SPEEDS):
    return acts(*([NOOP] * k), u=u, speeds=speeds)


CASES = {
    # ---- group (6 actions, no step limit, no sticky actions)
    # u refused at move_timer 3, 2, 1 and accepted at 0; then d refused at 2, 1 and accepted at 0
    "move_gating": dict(group="plain", state=start(pos=5, move_timer=3, **PARKED), script=acts(UP, UP, UP, UP, DOWN, DOWN, DOWN),
                        reach=["move_refused", "move_up", "move_down"]),
    "clamp_bottom": dict(group="plain", state=start(**PARKED), script=acts(DOWN, NOOP), reach=["clamp_bottom", "move_down"]),
    "hit_before_move": dict(group="plain", state=one_car(3, 4, 0, 1, pos=3), script=noops(2), reach=["hit_before_move"]),
    "hit_after_move_right": dict(group="plain", state=one_car(3, 3, 0, 2, pos=3), script=noops(2), reach=["hit_after_move_right"]),
    "hit_after_move_left": dict(group="plain", state=one_car(8, 5, 0, -2, pos=8), script=noops(2), reach=["hit_after_move_left"]),
    "hit_waiting_car": dict(group="plain", state=one_car(1, 4, 2, -3, pos=1), script=noops(2), reach=["hit_waiting_car"]),
    # the chicken steps up INTO the row of a car on column 4: the move comes first, the car's check after it
    "walk_into_a_car": dict(group="plain", state=one_car(5, 4, 3, 4, pos=6), script=acts(UP, NOOP), reach=["move_up", "hit_waiting_car"]),
    # + cars on column 9 and - cars on column 0, all about to move: both wraps, then both trail cells wrap
    "wraps": dict(group="plain", state=start(car_x=[9, 0] * 4, car_timer=[0] * 8, car_speed=SLOW, t=2 ** 32 - 1), script=noops(3),
                  reach=["wrap_right", "wrap_left"]),
    "fast_cars": dict(group="plain", state=start(car_x=[9, 0, 3, 5, 9, 0, 8, 1], car_timer=[0] * 8, car_speed=FAST), script=noops(7),
                      reach=["wrap_right", "wrap_left"]),
    # a win: new speeds, every x kept, the chicken back on row 9
    "win": dict(group="plain", state=start(pos=1, car_x=[1, 2, 3, 5, 6, 7, 8, 9], car_timer=[3] * 8),
                script=acts(UP, speeds=FAST) + noops(3), reach=["move_up", "win"]),
    # a win on the step the episode's timer runs out: reward 1 and done, the returned image shows the win's speeds
    "win_on_the_last_step": dict(group="plain", state=start(pos=1, terminate_timer=0, ep_steps=2500, t=123456789012, car_x=[6] * 8),
                                 script=acts(UP, speeds=SLOW) + noops(3), reach=["win", "terminal", "reset"]),
    "terminal_from_0": dict(group="plain", state=start(terminate_timer=0, car_x=[3] * 8), script=noops(1, speeds=FAST) + noops(4),
                            reach=["terminal", "reset"]),
    "terminal_from_1": dict(group="plain", state=start(terminate_timer=1, car_x=[5] * 8), script=noops(2, speeds=SLOW) + noops(3),
                            reach=["terminal", "reset"]),
    "unused_actions": dict(group="plain", state=start(pos=5, **PARKED), script=acts(LEFT, RIGHT, FIRE, UP),
                           reach=["unused_action", "move_up"]),
    # ---- group (3 actions: n, u, d; step limit 5)
    "truncation": dict(group="minimal", state=start(), script=noops(5, speeds=FAST) + noops(5, speeds=SLOW) + noops(2),
                       reach=["truncation", "reset"]),
    # the limit and the terminal on the same step: done, not truncated
    "limit_on_a_terminal": dict(group="minimal", state=start(ep_steps=3, terminate_timer=1), script=noops(3), reach=["terminal", "reset"]),
    "minimal_moves": dict(group="minimal", state=start(pos=5, **PARKED), script=acts(1, 0, 0, 2), reach=["move_up", "move_down"]),
    # 3 is `r` of the six actions and outside the three: it acts as no-op
    "minimal_out_of_range": dict(group="minimal", state=start(pos=5, **PARKED), script=acts(2, 3, 3, 2),
                                 reach=["bad_action", "move_down"], bad_action=True),
    # ---- group (6 actions, sticky_p = 0.25)
    "sticky": dict(group="sticky", state=start(pos=5, last_action=DOWN, **PARKED),
                   script=[(UP, 0.1, SPEEDS), (UP, 0.25, SPEEDS), (NOOP, 0.2499, SPEEDS), (DOWN, 0.0, SPEEDS), (DOWN, 0.7, SPEEDS)],
                   reach=["sticky_repeat", "move_up", "move_down", "move_refused"]),
    "sticky_out_of_range": dict(group="sticky", state=start(pos=5, last_action=UP, **PARKED),
                                script=[(7, 0.1, SPEEDS), (-1, 0.9, SPEEDS), (6, 0.1, SPEEDS), (2 ** 40 + 1, 0.9, SPEEDS)],
                                reach=["bad_action", "sticky_repeat", "move_up"], bad_action=True),
}

GROUPS = {"plain": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.0),
          "minimal": dict(minimal_actions=True, episode_timestep_limit=5, sticky_action_prob=0.0),
          "sticky": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.25)}

REQUIRED = ("move_up", "move_down", "move_refused", "clamp_bottom", "hit_before_move", "hit_after_move_right",
            "hit_after_move_left", "hit_waiting_car", "wrap_right", "wrap_left", "win", "terminal", "truncation", "sticky_repeat",
            "reset", "bad_action", "unused_action")
SCALARS = ("pos", "move_timer", "terminate_timer", "last_action", "ep_steps", "t")
PER_CAR = ("car_x", "car_timer", "car_speed")


def group_cases(group):
    return [n for n, c in CASES.items() if c["group"] == group]


def vector_names(group, n_envs, offset=0):
    names = group_cases(group)
    return [names[(offset + i) % len(names)] for i in range(n_envs)]


def vector(group, n_envs, offset=0):
    """The group's cases laid over ``n_envs`` environments (environment i runs case offset + i modulo the number of cases;
    scripts are padded with no-ops): (state dict of arrays, actions [steps][n] int64, u [steps][n] float64, speeds
    [steps][n][8] int8).  Offsets 0, n_envs, 2 n_envs, ... below the number of cases cover the whole group."""
    pick = [CASES[name] for name in vector_names(group, n_envs, offset)]
    steps = max(len(c["script"]) for c in pick)
    state = {k: np.array([c["state"][k] for c in pick], dtype=np.uint64 if k == "t" else np.int64) for k in SCALARS}
    for k in PER_CAR:
        state[k] = np.array([c["state"][k] for c in pick], dtype=np.int64)
    script = [[(c["script"][s] if s < len(c["script"]) else (NOOP, 0.9, SPEEDS)) for c in pick] for s in range(steps)]
    actions = np.array([[x[0] for x in row] for row in script], dtype=np.int64)
    u = np.array([[x[1] for x in row] for row in script], dtype=np.float64)
    speeds = np.array([[x[2] for x in row] for row in script], dtype=np.int8)
    return state, actions, u, speeds
