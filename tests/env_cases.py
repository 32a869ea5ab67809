"""The case table of the Breakout rules: crafted start states and action scripts that reach every branch of
the step -- play from reset reaches only wall, strike, paddle-under and miss within a few hundred steps; ceiling,
pass-through, the diagonal paddle bounce and the refill need a prepared board.

A case: a start state (``start(...)``: the reset state of side 0 with fields replaced), a script of (action, coin u, side of
the episode that would begin) per step, and the branches (tests/env_ref.py BRANCHES) it must reach.  Cases that share
(n_actions, step_limit, sticky_p) form a GROUP: they run side by side as the environments of one vector."""
import numpy as np

NOOP, LEFT, RIGHT = 0, 1, 3          # of the six actions n, l, u, r, d, f


def board(*cells, full=False):
    """bricks[10][10] with the given (y, x) cells set (``full``: rows 1..3 set and the given cells CLEARED)."""
    b = np.zeros((10, 10), np.uint8)
    if full:
        b[1:4, :] = 1
    for y, x in cells:
        b[y, x] = 0 if full else 1
    return b


def start(**over):
    s = dict(pos=4, ball_x=0, ball_y=3, ball_dir=2, last_x=0, last_y=3, strike=0, last_action=0, ep_steps=0, t=0,
             bricks=board(full=True))
    s.update(over)
    if "last_x" not in over:
        s["last_x"], s["last_y"] = s["ball_x"], s["ball_y"]
    return s


def noops(k, u=0.9, side=0):
    return [(NOOP, u, side)] * k


CASES = {
    # ---- group (6 actions, no step limit, no sticky actions)
    "wall_left": dict(group="plain", state=start(ball_x=0, ball_y=5, ball_dir=3), script=noops(3), reach=["wall"]),
    "wall_right": dict(group="plain", state=start(ball_x=9, ball_y=5, ball_dir=1, t=2 ** 32 - 1), script=noops(2),
                       reach=["wall", "strike"]),
    # the ball's diagonal (5,3) (6,2) (7,1) opened: up through the bricks to the ceiling, off the right wall, into a brick
    "ceiling": dict(group="plain", state=start(ball_x=4, ball_y=4, ball_dir=1, bricks=board((3, 5), (2, 6), (1, 7), full=True)),
                    script=noops(8), reach=["ceiling", "wall", "strike"]),
    # two stacked bricks on the ball's diagonal: strike (3,1) from row 2, then through (4,3) with `strike` set
    "pass_through": dict(group="plain", state=start(ball_x=2, ball_y=2, ball_dir=1, bricks=board((1, 3), (3, 4))),
                         script=noops(4), reach=["strike", "pass_through"]),
    # a one-brick board: the last brick goes, the ball comes down onto the paddle two to the right, the board refills
    "refill": dict(group="plain", state=start(ball_x=0, ball_y=5, ball_dir=1, bricks=board((3, 2))),
                   script=[(RIGHT, 0.9, 0), (RIGHT, 0.9, 0)] + noops(7), reach=["strike", "refill", "paddle_under", "move_right"]),
    "paddle_diagonal": dict(group="plain", state=start(ball_x=2, ball_y=7, ball_dir=2), script=noops(4), reach=["paddle_diagonal"]),
    "miss_then_side_1": dict(group="plain", state=start(ball_x=0, ball_y=7, ball_dir=2, pos=9, ep_steps=40, t=123456789012),
                             script=noops(2, side=1) + noops(9), reach=["miss", "reset_side_1", "paddle_under"]),
    "miss_then_side_0": dict(group="plain", state=start(ball_x=9, ball_y=7, ball_dir=3, pos=0), script=noops(2) + noops(9, side=1),
                             reach=["miss", "reset_side_0"]),
    "paddle_clamps": dict(group="plain", state=start(pos=1, ball_y=0, ball_dir=2, bricks=board()),
                          script=[(LEFT, 0.9, 0)] * 3 + [(RIGHT, 0.9, 0)] * 11, reach=["move_left", "move_right", "miss"]),
    "unused_actions": dict(group="plain", state=start(), script=[(2, 0.9, 0), (4, 0.9, 0), (5, 0.9, 0), (LEFT, 0.9, 0)],
                           reach=["move_left"]),
    # ---- group (3 actions: n, l, r; step limit 5)
    "truncation": dict(group="minimal", state=start(), script=noops(5, side=1) + noops(5, side=0) + noops(2),
                       reach=["truncation", "reset_side_1", "reset_side_0"]),
    # the limit and a miss on the same step: done, not truncated
    "limit_on_a_miss": dict(group="minimal", state=start(ball_x=0, ball_y=7, ball_dir=2, pos=9, ep_steps=3), script=noops(3),
                            reach=["miss"]),
    "minimal_moves": dict(group="minimal", state=start(), script=[(1, 0.9, 0), (1, 0.9, 0), (2, 0.9, 0), (0, 0.9, 0)],
                          reach=["move_left", "move_right"]),
    # 3 is `r` of the six actions and outside the three: it acts as no-op
    "minimal_out_of_range": dict(group="minimal", state=start(), script=[(2, 0.9, 0), (3, 0.9, 0), (2, 0.9, 0)],
                                 reach=["bad_action", "move_right"], bad_action=True),
    # ---- group (6 actions, sticky_p = 0.25)
    "sticky": dict(group="sticky", state=start(last_action=RIGHT),
                   script=[(LEFT, 0.1, 0), (LEFT, 0.25, 0), (NOOP, 0.2499, 0), (RIGHT, 0.0, 0), (RIGHT, 0.7, 0)],
                   reach=["sticky_repeat", "move_left", "move_right"]),
    "sticky_out_of_range": dict(group="sticky", state=start(last_action=LEFT), script=[(7, 0.1, 0), (-1, 0.9, 0), (6, 0.1, 0), (2 ** 40 + 1, 0.9, 0)],
                                reach=["bad_action", "sticky_repeat"], bad_action=True),
}

GROUPS = {"plain": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.0),
          "minimal": dict(minimal_actions=True, episode_timestep_limit=5, sticky_action_prob=0.0),
          "sticky": dict(minimal_actions=False, episode_timestep_limit=0, sticky_action_prob=0.25)}

REQUIRED = ("wall", "ceiling", "strike", "pass_through", "refill", "paddle_under", "paddle_diagonal", "miss", "truncation",
            "sticky_repeat", "reset_side_0", "reset_side_1")


def group_cases(group):
    return [n for n, c in CASES.items() if c["group"] == group]


def vector_names(group, n_envs, offset=0):
    names = group_cases(group)
    return [names[(offset + i) % len(names)] for i in range(n_envs)]


def vector(group, n_envs, offset=0):
    """The group's cases laid over ``n_envs`` environments (environment i runs case offset + i modulo the number of cases;
    scripts are padded with no-ops): (state dict of arrays, actions [steps][n] int64, u [steps][n] float64, side [steps][n]
    uint8).  Offsets 0, n_envs, 2 n_envs, ... below the number of cases cover the whole group."""
    pick = [CASES[name] for name in vector_names(group, n_envs, offset)]
    steps = max(len(c["script"]) for c in pick)
    state = {k: np.array([c["state"][k] for c in pick], dtype=np.uint64 if k == "t" else np.int64) for k in pick[0]["state"]
             if k != "bricks"}
    state["bricks"] = np.stack([c["state"]["bricks"] for c in pick])
    script = [[(c["script"][s] if s < len(c["script"]) else (NOOP, 0.9, 0)) for c in pick] for s in range(steps)]
    actions = np.array([[x[0] for x in row] for row in script], dtype=np.int64)
    u = np.array([[x[1] for x in row] for row in script], dtype=np.float64)
    side = np.array([[x[2] for x in row] for row in script], dtype=np.uint8)
    return state, actions, u, side
