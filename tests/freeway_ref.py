"""``HostFreeway``: the Freeway rules of DESIGN.md 7.4 restated in plain Python, one environment at a time -- the checker of
``prism_env_freeway_step`` (include/prism_hip.h).  Written from the rule table, not from the kernel: cars are lists, one
``if`` per rule, nothing packed.  The rules are MinAtar v1 as this project restates them; they are NOT checked against the
``minatar`` package.  No part of ``prism_amd/`` uses this file.

The coins and speeds are given (``step(actions, u=..., speeds=...)``, ``reset(first_speeds=...)``) or drawn through
``tests/helpers.py philox4x32`` exactly as the device draws them.  ``branches`` counts which rule every step took."""
import numpy as np

from tests.helpers import philox4x32

KEY_COIN = 0x46575943                        # "FWYC"
KEYS_WIN = (0x46575730, 0x46575731)          # "FWW0", "FWW1": cars 0-3, 4-7
KEYS_RESET = (0x46575230, 0x46575231)        # "FWR0", "FWR1"
FIRST_COUNTER = 2 ** 64 - 1
N_CARS, MOVE_TIME, EPISODE_TIME = 8, 3, 2500
SCALARS = ("pos", "move_timer", "terminate_timer", "last_action", "ep_steps", "t")
PER_CAR = ("car_x", "car_timer", "car_speed")
BRANCHES = ("move_up", "move_down", "move_refused", "clamp_bottom", "hit_before_move", "hit_after_move_right",
            "hit_after_move_left", "hit_waiting_car", "wrap_right", "wrap_left", "win", "terminal", "truncation",
            "sticky_repeat", "reset", "bad_action", "unused_action")


def unit_double(hi, lo):
    """common.h u64_to_unit_double: 27 + 26 bits."""
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


def draw(seed, env, counter, key):
    """The four words of one environment's draw at ``counter`` under stream key ``key``."""
    return philox4x32(seed, np.array([counter], dtype=np.uint64), (int(env) << 32) | key)[0]


def speed_of_word(w):
    """|speed| = 1 + floor(5 (w >> 1) / 2^31), direction + if w & 1."""
    w = int(w)
    mag = 1 + (((w >> 1) * 5) >> 31)
    return mag if w & 1 else -mag


def draw_speeds(seed, env, counter, keys):
    """A set of eight speeds: two draws at ``counter``, one word per car."""
    return [speed_of_word(w) for key in keys for w in draw(seed, env, counter, key)]


def coin(seed, env, counter):
    r = draw(seed, env, counter, KEY_COIN)
    return unit_double(r[0], r[1])


class HostFreeway:
    def __init__(self, n_envs, seed=0, sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False):
        self.n_envs, self.seed = int(n_envs), int(seed)
        self.sticky_p, self.step_limit = float(sticky_action_prob), int(episode_timestep_limit)
        self.n_actions = 3 if minimal_actions else 6
        self.obs_shape = (10, 10, 7)
        self.envs = [dict(pos=9, move_timer=0, terminate_timer=0, last_action=0, ep_steps=0, t=0, car_x=[0] * N_CARS,
                          car_timer=[0] * N_CARS, car_speed=[1] * N_CARS) for _ in range(self.n_envs)]
        self.branches = {b: 0 for b in BRANCHES}
        self.bad_action = False

    # ---- the rules
    def _reset_one(self, e, speeds):
        for i in range(N_CARS):
            e["car_x"][i], e["car_speed"][i], e["car_timer"][i] = 0, int(speeds[i]), abs(int(speeds[i]))
        e["pos"], e["move_timer"], e["terminate_timer"], e["ep_steps"] = 9, MOVE_TIME, EPISODE_TIME, 0
        self.branches["reset"] += 1

    def _step_one(self, e, action, u, win_speeds):
        """-> (reward, terminal, truncated); the state is the post-step state, before any reset.  ``win_speeds`` is a
        callable: the draw happens only on a step that wins."""
        br = self.branches
        a = int(action)
        if not 0 <= a < self.n_actions:
            a = 0
            self.bad_action = True
            br["bad_action"] += 1
        if self.n_actions == 3:
            a = [0, 2, 4][a]
        # 1. sticky
        if u < self.sticky_p:
            a = e["last_action"]
            br["sticky_repeat"] += 1
        e["last_action"] = a
        # 2. the chicken
        if a in (1, 3, 5):
            br["unused_action"] += 1
        if a in (2, 4) and e["move_timer"] != 0:
            br["move_refused"] += 1
        if a == 2 and e["move_timer"] == 0:
            e["move_timer"] = MOVE_TIME
            e["pos"] = max(0, e["pos"] - 1)
            br["move_up"] += 1
        elif a == 4 and e["move_timer"] == 0:
            e["move_timer"] = MOVE_TIME
            if e["pos"] == 9:
                br["clamp_bottom"] += 1
            e["pos"] = min(9, e["pos"] + 1)
            br["move_down"] += 1
        # 3. a win
        reward = 0.0
        if e["pos"] == 0:
            reward = 1.0
            speeds = win_speeds()
            for i in range(N_CARS):
                e["car_speed"][i], e["car_timer"][i] = int(speeds[i]), abs(int(speeds[i]))
            e["pos"] = 9
            br["win"] += 1
        # 4. the cars, in order
        for i in range(N_CARS):
            y = i + 1
            if (e["car_x"][i], y) == (4, e["pos"]):
                e["pos"] = 9
                br["hit_before_move" if e["car_timer"][i] == 0 else "hit_waiting_car"] += 1
            if e["car_timer"][i] == 0:
                e["car_timer"][i] = abs(e["car_speed"][i])
                e["car_x"][i] += 1 if e["car_speed"][i] > 0 else -1
                if e["car_x"][i] < 0:
                    e["car_x"][i] = 9
                    br["wrap_left"] += 1
                elif e["car_x"][i] > 9:
                    e["car_x"][i] = 0
                    br["wrap_right"] += 1
                if (e["car_x"][i], y) == (4, e["pos"]):
                    e["pos"] = 9
                    br["hit_after_move_right" if e["car_speed"][i] > 0 else "hit_after_move_left"] += 1
            else:
                e["car_timer"][i] -= 1
        # 5. the timers
        e["move_timer"] -= 1 if e["move_timer"] > 0 else 0
        e["terminate_timer"] -= 1
        terminal = e["terminate_timer"] < 0
        if terminal:
            e["terminate_timer"] = 0
            br["terminal"] += 1
        # 6.
        e["ep_steps"] += 1
        e["t"] += 1
        truncated = self.step_limit > 0 and e["ep_steps"] >= self.step_limit and not terminal
        if truncated:
            br["truncation"] += 1
        return reward, terminal, truncated

    @staticmethod
    def image(e):
        img = np.zeros((10, 10, 7), np.uint8)
        img[e["pos"], 4, 0] = 1
        for i in range(N_CARS):
            x, speed = e["car_x"][i], e["car_speed"][i]
            img[i + 1, x, 1] = 1
            back = x - 1 if speed > 0 else x + 1
            if back < 0:
                back = 9
            elif back > 9:
                back = 0
            img[i + 1, back, 1 + abs(speed)] = 1
        return img

    # ---- the VectorCollector protocol (float32 observations)
    def reset(self, first_speeds=None):
        for i, e in enumerate(self.envs):
            speeds = first_speeds[i] if first_speeds is not None else draw_speeds(self.seed, i, FIRST_COUNTER, KEYS_RESET)
            e["last_action"], e["t"] = 0, 0
            self._reset_one(e, speeds)
        return self.observe()

    def observe(self):
        return np.stack([self.image(e) for e in self.envs]).astype(np.float32)

    def step(self, actions, u=None, speeds=None):
        actions = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions).reshape(-1)
        assert actions.shape[0] == self.n_envs
        n = self.n_envs
        next_obs = np.zeros((n, 10, 10, 7), np.float32)
        reward, done, trunc = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i, e in enumerate(self.envs):
            t0 = e["t"]
            c = float(u[i]) if u is not None else coin(self.seed, i, t0)
            if speeds is not None:
                win = reset = lambda i=i: [int(v) for v in np.asarray(speeds[i]).reshape(-1)]
            else:
                win = lambda i=i, t0=t0: draw_speeds(self.seed, i, t0, KEYS_WIN)
                reset = lambda i=i, t0=t0: draw_speeds(self.seed, i, t0, KEYS_RESET)
            reward[i], done[i], trunc[i] = self._step_one(e, actions[i], c, win)
            next_obs[i] = self.image(e)
            if done[i] or trunc[i]:          # 7. the acting image then comes from a reset
                self._reset_one(e, reset())
        return next_obs, reward, done, trunc

    # ---- state
    def get_state(self):
        out = {f: np.array([e[f] for e in self.envs], dtype=np.uint64 if f == "t" else np.int64) for f in SCALARS}
        for f in PER_CAR:
            out[f] = np.array([e[f] for e in self.envs], dtype=np.int64).reshape(self.n_envs, N_CARS)
        return out

    def set_state(self, state):
        for i, e in enumerate(self.envs):
            for f in SCALARS:
                e[f] = int(state[f][i])
            for f in PER_CAR:
                e[f] = [int(v) for v in np.asarray(state[f][i]).reshape(-1)]


def assert_same_state(got, want, where=""):
    """Every state field of two ``get_state()`` dicts, exactly."""
    for f in SCALARS + PER_CAR:
        kind = np.uint64 if f == "t" else np.int64
        np.testing.assert_array_equal(np.asarray(got[f]).astype(kind), np.asarray(want[f]).astype(kind), err_msg=f"{where}: state field {f}")
