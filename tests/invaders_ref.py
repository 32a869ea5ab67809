"""``HostSpaceInvaders``: the Space Invaders rules of DESIGN.md 7.6 restated in plain NumPy, one environment at a time -- the
checker of ``prism_env_invaders_step`` (include/prism_hip.h).  Written from the rule table, not from the kernel, and in the MAP
form: three full 10 x 10 maps (aliens, friendly bullets, enemy bullets) moved with ``np.roll`` as MinAtar moves them, one
``if`` per rule, nothing packed -- so the kernel's compact record (a 4 x 6 block with an origin, one 4-bit field per bullet
row) is checked against the maps and not against itself.  The only bookkeeping beside the maps is the block's origin
``(alien_x, alien_y)``, which moves with every roll: ``get_state`` reads the block out of the alien map through it and
asserts that nothing stands outside the window and that no row of a bullet map holds two bullets.  The rules are MinAtar v1
as this project restates them; they are NOT checked against the ``minatar`` package.  No part of ``prism_amd/`` uses this
file.

The coins are given (``step(actions, u=...)``) or drawn through ``tests/helpers.py philox4x32`` exactly as the device draws
them; the game draws nothing else.  ``branches`` counts which rule every step took."""
import numpy as np

from tests.helpers import philox4x32

KEY_COIN = 0x53504943                        # "SPIC"
# the block: 4 rows x 6 columns, first placed at rows 0..3, columns 2..7; the three intervals
BLOCK_ROWS, BLOCK_COLS, FIRST_X, FIRST_Y = 4, 6, 2, 0
SHOT_COOL_DOWN, ENEMY_SHOT_INTERVAL, ENEMY_MOVE_INTERVAL, MOVE_INTERVAL_MIN = 5, 10, 12, 6
SCALARS = ("pos", "alien_x", "alien_y", "alien_dir", "alien_move_timer", "alien_shot_timer", "enemy_move_interval", "ramp_index",
           "shot_timer", "last_action", "ep_steps", "t")
ARRAYS = ("alien_block", "f_bullet_x", "e_bullet_x")
BRANCHES = ("move_left", "move_right", "clamp_left", "clamp_right", "fire", "fire_cooling", "up_down_noop",
            "f_bullet_leaves", "e_bullet_leaves", "hit_by_bullet",
            "aliens_wait", "aliens_left", "aliens_right", "turn_at_column_0", "turn_at_column_9", "turn_with_dead_outer_column",
            "timer_from_count", "timer_from_interval", "alien_on_cannon_before_move", "alien_on_cannon_after_move",
            "descent_onto_row_9", "wrapped_row_drawn",
            "alien_shot", "shot_distance_0", "shot_tie_lower_column", "shot_distance_9", "shot_onto_a_bullet", "shot_on_terminal_descent",
            "kill", "two_kills", "pass_through", "board_cleared", "ramp", "ramp_at_fastest",
            "terminal", "truncation", "terminal_on_the_limit", "sticky_repeat", "reset", "bad_action")


def unit_double(hi, lo):
    """common.h u64_to_unit_double: 27 + 26 bits."""
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


def draw(seed, env, counter, key=KEY_COIN):
    """The four words of one environment's draw at ``counter`` under stream key ``key``."""
    return philox4x32(seed, np.array([counter], dtype=np.uint64), (int(env) << 32) | key)[0]


def coin(seed, env, counter):
    r = draw(seed, env, counter)
    return unit_double(r[0], r[1])


class HostSpaceInvaders:
    def __init__(self, n_envs, seed=0, sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False):
        self.n_envs, self.seed = int(n_envs), int(seed)
        self.sticky_p, self.step_limit = float(sticky_action_prob), int(episode_timestep_limit)
        self.n_actions = 4 if minimal_actions else 6
        self.obs_shape = (10, 10, 6)
        self.envs = [dict(last_action=0, t=0) for _ in range(self.n_envs)]
        self.branches = {b: 0 for b in BRANCHES}
        for e in self.envs:
            self._reset_one(e)
        self.branches["reset"] = 0
        self.bad_action = False

    # ---- the rules
    @staticmethod
    def _full_board(e):
        e["alien_map"] = np.zeros((10, 10), np.uint8)
        e["alien_map"][FIRST_Y:FIRST_Y + BLOCK_ROWS, FIRST_X:FIRST_X + BLOCK_COLS] = 1
        e["alien_x"], e["alien_y"] = FIRST_X, FIRST_Y

    def _reset_one(self, e):
        e["pos"] = 5
        e["f_bullet_map"], e["e_bullet_map"] = np.zeros((10, 10), np.uint8), np.zeros((10, 10), np.uint8)
        self._full_board(e)
        e["alien_dir"] = -1
        e["enemy_move_interval"] = e["alien_move_timer"] = ENEMY_MOVE_INTERVAL
        e["alien_shot_timer"] = ENEMY_SHOT_INTERVAL
        e["ramp_index"], e["shot_timer"], e["ep_steps"] = 0, 0, 0
        self.branches["reset"] += 1

    def _step_one(self, e, action, u):
        """-> (reward, terminal, truncated); the state is the post-step state, before any reset."""
        br = self.branches
        a = int(action)
        if not 0 <= a < self.n_actions:
            a = 0
            self.bad_action = True
            br["bad_action"] += 1
        if self.n_actions == 4:
            a = (0, 1, 3, 5)[a]
        # 1. sticky
        if u < self.sticky_p:
            a = e["last_action"]
            br["sticky_repeat"] += 1
        e["last_action"] = a
        terminal = False
        # 2. the cannon
        if a == 5:
            if e["shot_timer"] == 0:
                e["f_bullet_map"][9, e["pos"]] = 1
                e["shot_timer"] = SHOT_COOL_DOWN
                br["fire"] += 1
            else:
                br["fire_cooling"] += 1
        elif a == 1:
            br["clamp_left" if e["pos"] == 0 else "move_left"] += 1
            e["pos"] = max(0, e["pos"] - 1)
        elif a == 3:
            br["clamp_right" if e["pos"] == 9 else "move_right"] += 1
            e["pos"] = min(9, e["pos"] + 1)
        elif a in (2, 4):
            br["up_down_noop"] += 1
        # 3. friendly bullets one row up
        br["f_bullet_leaves"] += int(e["f_bullet_map"][0].sum())
        e["f_bullet_map"] = np.roll(e["f_bullet_map"], -1, axis=0)
        e["f_bullet_map"][9, :] = 0
        # 4. enemy bullets one row down
        br["e_bullet_leaves"] += int(e["e_bullet_map"][9].sum())
        e["e_bullet_map"] = np.roll(e["e_bullet_map"], 1, axis=0)
        e["e_bullet_map"][0, :] = 0
        if e["e_bullet_map"][9, e["pos"]]:
            terminal = True
            br["hit_by_bullet"] += 1
        # 5. the aliens
        descended_onto_9 = False
        if e["alien_map"][9, e["pos"]]:
            terminal = True
            br["alien_on_cannon_before_move"] += 1
        if e["alien_move_timer"] == 0:
            count = int(np.count_nonzero(e["alien_map"]))
            e["alien_move_timer"] = min(count, e["enemy_move_interval"])
            br["timer_from_count" if count < e["enemy_move_interval"] else "timer_from_interval"] += 1
            at_0, at_9 = e["alien_map"][:, 0].sum() > 0 and e["alien_dir"] < 0, e["alien_map"][:, 9].sum() > 0 and e["alien_dir"] > 0
            if at_0 or at_9:
                br["turn_at_column_0" if at_0 else "turn_at_column_9"] += 1
                if e["alien_x"] in (-(BLOCK_COLS - 1), 9):
                    br["turn_with_dead_outer_column"] += 1
                e["alien_dir"] = -e["alien_dir"]
                if e["alien_map"][9, :].sum() > 0:
                    terminal = descended_onto_9 = True
                    br["descent_onto_row_9"] += 1
                if (e["f_bullet_map"] & e["alien_map"]).any():          # the bullet came up onto an alien that now goes down:
                    br["pass_through"] += 1                             # they swap rows and neither is lost
                e["alien_map"] = np.roll(e["alien_map"], 1, axis=0)
                e["alien_y"] = (e["alien_y"] + 1) % 10
            else:
                e["alien_map"] = np.roll(e["alien_map"], e["alien_dir"], axis=1)
                e["alien_x"] += e["alien_dir"]
                br["aliens_left" if e["alien_dir"] < 0 else "aliens_right"] += 1
            if e["alien_map"][9, e["pos"]]:
                terminal = True
                br["alien_on_cannon_after_move"] += 1
        else:
            br["aliens_wait"] += 1
        # 6. the aliens' shot
        if e["alien_shot_timer"] == 0:
            e["alien_shot_timer"] = ENEMY_SHOT_INTERVAL
            order = sorted(range(10), key=lambda x: (abs(x - e["pos"]), x))
            for x in order:
                rows = np.nonzero(e["alien_map"][:, x])[0]
                if len(rows):
                    y = int(rows.max())
                    br["alien_shot"] += 1
                    d = abs(x - e["pos"])
                    if d == 0:
                        br["shot_distance_0"] += 1
                    if d == 9:
                        br["shot_distance_9"] += 1
                    if d > 0 and x < e["pos"] and 0 <= e["pos"] + d <= 9 and e["alien_map"][:, e["pos"] + d].any():
                        br["shot_tie_lower_column"] += 1
                    if e["e_bullet_map"][y, x]:
                        br["shot_onto_a_bullet"] += 1
                    if descended_onto_9:
                        br["shot_on_terminal_descent"] += 1
                    e["e_bullet_map"][y, x] = 1
                    break
        # 7. kills
        kills =(e["alien_map"] == 1) & (e["f_bullet_map"] == 1)
        reward = float(kills.sum())
        if kills.sum():
            br["kill"] += 1
        if kills.sum() >= 2:
            br["two_kills"] += 1
        e["alien_map"][kills] = 0
        e["f_bullet_map"][kills] = 0
        # 8. timers
        e["shot_timer"] -= 1 if e["shot_timer"] > 0 else 0
        e["alien_move_timer"] -= 1
        e["alien_shot_timer"] -= 1
        # 9. a cleared board
        if np.count_nonzero(e["alien_map"]) == 0:
            br["board_cleared"] += 1
            if e["enemy_move_interval"] > MOVE_INTERVAL_MIN:
                e["enemy_move_interval"] -= 1
                e["ramp_index"] += 1
                br["ramp"] += 1
            else:
                br["ramp_at_fastest"] += 1
            self._full_board(e)
        # 10. counters and flags
        e["ep_steps"] += 1
        e["t"] += 1
        at_limit = self.step_limit > 0 and e["ep_steps"] >= self.step_limit
        truncated = at_limit and not terminal
        if terminal:
            br["terminal"] += 1
            if at_limit:
                br["terminal_on_the_limit"] += 1
            if descended_onto_9 and e["alien_map"][0].any():
                br["wrapped_row_drawn"] += 1
        if truncated:
            br["truncation"] += 1
        return reward, terminal, truncated

    @staticmethod
    def image(e):
        img = np.zeros((10, 10, 6), np.uint8)
        img[9, e["pos"], 0] = 1
        img[..., 1] = e["alien_map"]
        img[..., 2 if e["alien_dir"] < 0 else 3] = e["alien_map"]
        img[..., 4] = e["f_bullet_map"]
        img[..., 5] = e["e_bullet_map"]
        return img

    # ---- the VectorCollector protocol (float32 observations)
    def reset(self):
        for e in self.envs:
            e["last_action"], e["t"] = 0, 0
            self._reset_one(e)
        return self.observe()

    def observe(self):
        return np.stack([self.image(e) for e in self.envs]).astype(np.float32)

    def step(self, actions, u=None):
        actions = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions).reshape(-1)
        assert actions.shape[0] == self.n_envs
        n = self.n_envs
        next_obs = np.zeros((n, 10, 10, 6), np.float32)
        reward, done, trunc = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i, e in enumerate(self.envs):
            c = float(u[i]) if u is not None else coin(self.seed, i, e["t"])
            reward[i], done[i], trunc[i] = self._step_one(e, actions[i], c)
            next_obs[i] = self.image(e)
            if done[i] or trunc[i]:          # the acting image then comes from a reset
                self._reset_one(e)
        return next_obs, reward, done, trunc

    # ---- state, in the device's field names
    @staticmethod
    def _bullet_rows(m, what):
        assert (m.sum(axis=1) <= 1).all(), f"two {what} bullets in one row: no state of the device's record"
        return np.where(m.any(axis=1), m.argmax(axis=1), -1).astype(np.int64)

    def _one_state(self, e):
        out = {f: e[f] for f in SCALARS}
        block = np.zeros((BLOCK_ROWS, BLOCK_COLS), np.int64)
        seen = np.zeros((10, 10), np.uint8)
        for r in range(BLOCK_ROWS):
            for c in range(BLOCK_COLS):
                y, x = (e["alien_y"] + r) % 10, e["alien_x"] + c
                if 0 <= x <= 9:
                    block[r, c] = e["alien_map"][y, x]
                    seen[y, x] = 1
        assert not (e["alien_map"] & (1 - seen)).any(), "an alien outside the block's window: no state of the device's record"
        out["alien_block"] = block
        out["f_bullet_x"] = self._bullet_rows(e["f_bullet_map"], "friendly")
        out["e_bullet_x"] = self._bullet_rows(e["e_bullet_map"], "enemy")
        return out

    def get_state(self):
        rows = [self._one_state(e) for e in self.envs]
        out = {f: np.array([r[f] for r in rows], dtype=np.uint64 if f == "t" else np.int64) for f in SCALARS}
        for f in ARRAYS:
            out[f] = np.stack([r[f] for r in rows]).astype(np.int64)
        return out

    def set_state(self, state):
        for i, e in enumerate(self.envs):
            for f in SCALARS:
                e[f] = int(state[f][i])
            block = np.asarray(state["alien_block"][i]).reshape(BLOCK_ROWS, BLOCK_COLS)
            e["alien_map"] = np.zeros((10, 10), np.uint8)
            for r in range(BLOCK_ROWS):
                for c in range(BLOCK_COLS):
                    if block[r, c]:
                        e["alien_map"][(e["alien_y"] + r) % 10, e["alien_x"] + c] = 1
            for name, key in (("f_bullet_map", "f_bullet_x"), ("e_bullet_map", "e_bullet_x")):
                e[name] = np.zeros((10, 10), np.uint8)
                for y, x in enumerate(np.asarray(state[key][i]).reshape(10)):
                    if x >= 0:
                        e[name][y, int(x)] = 1


def assert_same_state(got, want, where=""):
    """Every state field of two ``get_state()`` dicts, exactly."""
    for f in SCALARS + ARRAYS:
        kind = np.uint64 if f == "t" else np.int64
        np.testing.assert_array_equal(np.asarray(got[f]).astype(kind), np.asarray(want[f]).astype(kind), err_msg=f"{where}: state field {f}")
