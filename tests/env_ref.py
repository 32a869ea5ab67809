"""``HostBreakout``: the Breakout rules of DESIGN.md 7.3 restated in plain Python, one environment at a time -- the checker of
``prism_env_breakout_step`` (include/prism_hip.h).  Written from the rule table, not from the kernel: tables where the table
has tables, one ``if`` per rule.  The rules are MinAtar v1 as this project restates them; they are NOT checked against the
``minatar`` package.  No part of ``prism_amd/`` uses this file.

The coins and sides are given (``step(actions, u=..., side=...)``, ``reset(first_side=...)``) or drawn through
``tests/helpers.py philox4x32`` exactly as the device draws them.  ``branches`` counts which rule every step took."""
import numpy as np

from tests.helpers import philox4x32

ENV_KEY = 0x454E5642          # "ENVB"
FIRST_COUNTER = 2 ** 64 - 1
MOVES = [(-1, -1), (1, -1), (1, 1), (-1, 1)]          # dir 0..3 -> (dx, dy)
WALL, FLIP, DIAG = [1, 0, 3, 2], [3, 2, 1, 0], [2, 3, 0, 1]
FIELDS = ("pos", "ball_x", "ball_y", "ball_dir", "last_x", "last_y", "strike", "last_action", "ep_steps", "t")
BRANCHES = ("wall", "ceiling", "strike", "pass_through", "refill", "paddle_under", "paddle_diagonal", "miss", "truncation",
            "sticky_repeat", "reset_side_0", "reset_side_1", "move_left", "move_right", "bad_action")


def unit_double(hi, lo):
    """common.h u64_to_unit_double: 27 + 26 bits."""
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


def draw(seed, env, counter):
    """The four words of one environment's draw at ``counter``."""
    return philox4x32(seed, np.array([counter], dtype=np.uint64), (int(env) << 32) | ENV_KEY)[0]


class HostBreakout:
    def __init__(self, n_envs, seed=0, sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False):
        self.n_envs, self.seed = int(n_envs), int(seed)
        self.sticky_p, self.step_limit = float(sticky_action_prob), int(episode_timestep_limit)
        self.n_actions = 3 if minimal_actions else 6
        self.obs_shape = (10, 10, 4)
        self.envs = [dict(pos=0, ball_x=0, ball_y=0, ball_dir=0, last_x=0, last_y=0, strike=0, last_action=0, ep_steps=0, t=0,
                          bricks=np.zeros((10, 10), np.uint8)) for _ in range(self.n_envs)]
        self.branches = {b: 0 for b in BRANCHES}
        self.bad_action = False

    # ---- the rules
    def _reset_one(self, e, side):
        e["ball_y"] = 3
        e["ball_x"], e["ball_dir"] = (0, 2) if side == 0 else (9, 3)
        e["pos"] = 4
        e["bricks"] = np.zeros((10, 10), np.uint8)
        e["bricks"][1:4, :] = 1
        e["strike"] = 0
        e["last_x"], e["last_y"] = e["ball_x"], e["ball_y"]
        e["ep_steps"] = 0
        self.branches["reset_side_%d" % side] += 1

    def _step_one(self, e, action, u):
        """-> (reward, terminal, truncated); the state is the post-step state, before any reset."""
        br = self.branches
        a = int(action)
        if not 0 <= a < self.n_actions:
            a = 0
            self.bad_action = True
            br["bad_action"] += 1
        if self.n_actions == 3:
            a = [0, 1, 3][a]
        # 1. sticky
        if u < self.sticky_p:
            a = e["last_action"]
            br["sticky_repeat"] += 1
        e["last_action"] = a
        # 2. paddle
        if a == 1:
            e["pos"] = max(0, e["pos"] - 1)
            br["move_left"] += 1
        elif a == 3:
            e["pos"] = min(9, e["pos"] + 1)
            br["move_right"] += 1
        # 3. ball
        ball_x = e["ball_x"]
        e["last_x"], e["last_y"] = e["ball_x"], e["ball_y"]
        d = e["ball_dir"]
        new_x, new_y = e["ball_x"] + MOVES[d][0], e["ball_y"] + MOVES[d][1]
        # 4. side walls
        if new_x < 0 or new_x > 9:
            new_x = min(9, max(0, new_x))
            d = WALL[d]
            br["wall"] += 1
        # 5. the first case that applies
        reward, terminal, strike_toggle = 0.0, False, False
        if new_y < 0:
            new_y = 0
            d = FLIP[d]
            br["ceiling"] += 1
        elif e["bricks"][new_y, new_x]:
            strike_toggle = True
            if not e["strike"]:
                reward += 1.0
                e["strike"] = 1
                e["bricks"][new_y, new_x] = 0
                new_y = e["last_y"]
                d = FLIP[d]
                br["strike"] += 1
            else:
                br["pass_through"] += 1
        elif new_y == 9:
            if not e["bricks"].any():
                e["bricks"][1:4, :] = 1
                br["refill"] += 1
            if ball_x == e["pos"]:
                d = FLIP[d]
                new_y = e["last_y"]
                br["paddle_under"] += 1
            elif new_x == e["pos"]:
                d = DIAG[d]
                new_y = e["last_y"]
                br["paddle_diagonal"] += 1
            else:
                terminal = True
                br["miss"] += 1
        # 6.
        if not strike_toggle:
            e["strike"] = 0
        e["ball_x"], e["ball_y"], e["ball_dir"] = new_x, new_y, d
        # 7.
        e["ep_steps"] += 1
        e["t"] += 1
        truncated = self.step_limit > 0 and e["ep_steps"] >= self.step_limit and not terminal
        if truncated:
            br["truncation"] += 1
        return reward, terminal, truncated

    @staticmethod
    def image(e):
        img = np.zeros((10, 10, 4), np.uint8)
        img[9, e["pos"], 0] = 1
        img[e["ball_y"], e["ball_x"], 1] = 1
        img[e["last_y"], e["last_x"], 2] = 1
        img[:, :, 3] = e["bricks"]
        return img

    # ---- the VectorCollector protocol (float32 observations)
    def reset(self, first_side=None):
        for i, e in enumerate(self.envs):
            side = int(first_side[i]) & 1 if first_side is not None else int(draw(self.seed, i, FIRST_COUNTER)[3]) & 1
            e["last_action"], e["t"] = 0, 0
            self._reset_one(e, side)
        return self.observe()

    def observe(self):
        return np.stack([self.image(e) for e in self.envs]).astype(np.float32)

    def step(self, actions, u=None, side=None):
        actions = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions).reshape(-1)
        assert actions.shape[0] == self.n_envs
        n = self.n_envs
        next_obs = np.zeros((n, 10, 10, 4), np.float32)
        reward, done, trunc = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i, e in enumerate(self.envs):
            coin, new_side = 1.0, 0
            if u is None or side is None:
                r = draw(self.seed, i, e["t"])
                coin, new_side = unit_double(r[0], r[1]), int(r[2]) & 1
            if u is not None:
                coin = float(u[i])
            if side is not None:
                new_side = int(side[i]) & 1
            reward[i], done[i], trunc[i] = self._step_one(e, actions[i], coin)
            next_obs[i] = self.image(e)
            if done[i] or trunc[i]:          # 8. the acting image then comes from a reset
                self._reset_one(e, new_side)
        return next_obs, reward, done, trunc

    # ---- state
    def get_state(self):
        out = {f: np.array([e[f] for e in self.envs], dtype=np.uint64 if f == "t" else np.int64) for f in FIELDS}
        out["bricks"] = np.stack([e["bricks"] for e in self.envs]).astype(np.uint8)
        return out

    def set_state(self, state):
        for i, e in enumerate(self.envs):
            for f in FIELDS:
                e[f] = int(state[f][i])
            e["bricks"] = np.array(state["bricks"][i], dtype=np.uint8).reshape(10, 10).copy()


def assert_same_state(got, want, where=""):
    """Every state field of two ``get_state()`` dicts, exactly."""
    for f in FIELDS + ("bricks",):
        g, w = np.asarray(got[f]).astype(np.uint64 if f == "t" else np.int64), np.asarray(want[f]).astype(np.uint64 if f == "t" else np.int64)
        np.testing.assert_array_equal(g, w, err_msg=f"{where}: state field {f}")
