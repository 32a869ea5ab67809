"""``HostAsterix``: the Asterix rules of DESIGN.md 7.5 restated in plain Python, one environment at a time -- the checker of
``prism_env_asterix_step`` (include/prism_hip.h).  Written from the rule table, not from the kernel: the slots are a list, one
``if`` per rule, nothing packed.  The rules are MinAtar v1 as this project restates them; they are NOT checked against the
``minatar`` package.  No part of ``prism_amd/`` uses this file.

The coins and spawns are given (``step(actions, u=..., spawn=...)``) or drawn through ``tests/helpers.py philox4x32`` exactly
as the device draws them.  ``branches`` counts which rule every step took."""
import numpy as np

from tests.helpers import philox4x32

KEY_COIN = 0x41535843                        # "ASXC"
KEY_SPAWN = 0x41535853                       # "ASXS"
N_SLOTS, SPAWN_SPEED, MOVE_SPEED, RAMP_INTERVAL = 8, 10, 5, 100
SCALARS = ("px", "py", "spawn_speed", "spawn_timer", "move_speed", "move_timer", "ramp_timer", "ramp_index", "last_action",
           "ep_steps", "t")
PER_SLOT = ("ent_active", "ent_x", "ent_dir", "ent_gold")
BRANCHES = ("move_left", "move_right", "move_up", "move_down", "clamp_left", "clamp_right", "clamp_top", "clamp_bottom",
            "fire_noop", "spawn_left", "spawn_right", "spawn_gold", "spawn_enemy", "spawn_first", "spawn_middle", "spawn_last",
            "spawn_full", "rank_clamped", "spawn_on_player_gold", "spawn_on_player_enemy", "walk_into_gold", "walk_into_enemy",
            "gold_arrives_from_left", "gold_arrives_from_right", "enemy_arrives_from_left", "enemy_arrives_from_right",
            "entities_wait", "entities_move", "exit_left", "exit_right", "trail_clipped_left", "trail_clipped_right", "trail_drawn",
            "ramp_even", "ramp_odd", "ramp_move_speed_at_1", "ramp_last", "ramp_frozen", "ramp_timer_below_zero", "terminal",
            "truncation", "terminal_on_the_limit", "sticky_repeat", "reset", "bad_action")


def unit_double(hi, lo):
    """common.h u64_to_unit_double: 27 + 26 bits."""
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


def draw(seed, env, counter, key):
    """The four words of one environment's draw at ``counter`` under stream key ``key``."""
    return philox4x32(seed, np.array([counter], dtype=np.uint64), (int(env) << 32) | key)[0]


def coin(seed, env, counter):
    r = draw(seed, env, counter, KEY_COIN)
    return unit_double(r[0], r[1])


def spawn_of_words(w, k):
    """(side, gold, rank) of the words of a spawn draw with ``k`` empty slots: side = w0 & 1, gold = floor(3 w1 / 2^32) == 0,
    rank = floor(k w2 / 2^32)."""
    return int(w[0]) & 1, int(((int(w[1]) * 3) >> 32) == 0), (int(w[2]) * int(k)) >> 32


def draw_spawn(seed, env, counter, k):
    return spawn_of_words(draw(seed, env, counter, KEY_SPAWN), k)


class HostAsterix:
    def __init__(self, n_envs, seed=0, sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False):
        self.n_envs, self.seed = int(n_envs), int(seed)
        self.sticky_p, self.step_limit = float(sticky_action_prob), int(episode_timestep_limit)
        self.n_actions = 5 if minimal_actions else 6
        self.obs_shape = (10, 10, 4)
        self.envs = [dict(px=5, py=5, spawn_speed=SPAWN_SPEED, spawn_timer=SPAWN_SPEED, move_speed=MOVE_SPEED, move_timer=MOVE_SPEED,
                          ramp_timer=RAMP_INTERVAL, ramp_index=0, last_action=0, ep_steps=0, t=0, slots=[None] * N_SLOTS)
                     for _ in range(self.n_envs)]
        self.branches = {b: 0 for b in BRANCHES}
        self.bad_action = False

    # ---- the rules
    def _reset_one(self, e):
        e["px"], e["py"], e["slots"] = 5, 5, [None] * N_SLOTS
        e["spawn_speed"], e["spawn_timer"] = SPAWN_SPEED, SPAWN_SPEED
        e["move_speed"], e["move_timer"] = MOVE_SPEED, MOVE_SPEED
        e["ramp_timer"], e["ramp_index"], e["ep_steps"] = RAMP_INTERVAL, 0, 0
        self.branches["reset"] += 1

    def _contact(self, e, i, how):
        """Rule 4 for slot i, known to hold an entity on the player's cell -> (reward, terminal)."""
        br = self.branches
        ent = e["slots"][i]
        kind = "gold" if ent["gold"] else "enemy"
        if how == "arrives":
            br[f"{kind}_arrives_from_{'left' if ent['dir'] > 0 else 'right'}"] += 1
        else:
            br[f"{how}_{kind}"] += 1
        if ent["gold"]:
            e["slots"][i] = None
            return 1.0, False
        return 0.0, True

    def _step_one(self, e, action, u, spawn):
        """-> (reward, terminal, truncated); the state is the post-step state, before any reset.  ``spawn`` is a callable of
        the number of empty slots: the draw happens only on a step that spawns."""
        br = self.branches
        a = int(action)
        if not 0 <= a < self.n_actions:
            a = 0
            self.bad_action = True
            br["bad_action"] += 1
        # 1. sticky
        if u < self.sticky_p:
            a = e["last_action"]
            br["sticky_repeat"] += 1
        e["last_action"] = a
        # 2. spawn
        spawned = None
        if e["spawn_timer"] == 0:
            empty = [i for i in range(N_SLOTS) if e["slots"][i] is None]
            k = len(empty)
            side, gold, rank = spawn(k)
            if k > 0:
                if rank >= k:          # a guard of the given path; the drawn rank is below k
                    rank = k - 1
                    br["rank_clamped"] += 1
                spawned = empty[rank]
                e["slots"][spawned] = dict(x=0, dir=1, gold=int(gold)) if side else dict(x=9, dir=-1, gold=int(gold))
                br["spawn_left" if side else "spawn_right"] += 1
                br["spawn_gold" if gold else "spawn_enemy"] += 1
                if rank == 0:
                    br["spawn_first"] += 1
                if rank == k - 1:
                    br["spawn_last"] += 1
                if 0 < rank < k - 1:
                    br["spawn_middle"] += 1
            else:
                br["spawn_full"] += 1
            e["spawn_timer"] = e["spawn_speed"]
        # 3. the player
        if a == 1:
            br["clamp_left" if e["px"] == 0 else "move_left"] += 1
            e["px"] = max(0, e["px"] - 1)
        elif a == 3:
            br["clamp_right" if e["px"] == 9 else "move_right"] += 1
            e["px"] = min(9, e["px"] + 1)
        elif a == 2:
            br["clamp_top" if e["py"] == 1 else "move_up"] += 1
            e["py"] = max(1, e["py"] - 1)
        elif a == 4:
            br["clamp_bottom" if e["py"] == 8 else "move_down"] += 1
            e["py"] = min(8, e["py"] + 1)
        elif a == 5:
            br["fire_noop"] += 1
        # 4. contact before the move
        reward, terminal = 0.0, False
        for i in range(N_SLOTS):
            ent = e["slots"][i]
            if ent is not None and (ent["x"], i + 1) == (e["px"], e["py"]):
                r, dead = self._contact(e, i, "spawn_on_player" if i == spawned else "walk_into")
                reward += r
                terminal = terminal or dead
        # 5. the entities
        if e["move_timer"] == 0:
            e["move_timer"] = e["move_speed"]
            br["entities_move"] += 1
            for i in range(N_SLOTS):
                ent = e["slots"][i]
                if ent is None:
                    continue
                ent["x"] += ent["dir"]
                if ent["x"] < 0:
                    e["slots"][i] = None
                    br["exit_left"] += 1
                elif ent["x"] > 9:
                    e["slots"][i] = None
                    br["exit_right"] += 1
                elif (ent["x"], i + 1) == (e["px"], e["py"]):
                    r, dead = self._contact(e, i, "arrives")
                    reward += r
                    terminal = terminal or dead
        else:
            br["entities_wait"] += 1
        # 6. the timers
        e["spawn_timer"] -= 1
        e["move_timer"] -= 1
        # 7. the ramp
        if e["spawn_speed"] > 1 or e["move_speed"] > 1:
            if e["ramp_timer"] >= 0:
                e["ramp_timer"] -= 1
                if e["ramp_timer"] < 0:
                    br["ramp_timer_below_zero"] += 1
            else:
                br["ramp_odd" if e["ramp_index"] % 2 else "ramp_even"] += 1
                if e["move_speed"] > 1 and e["ramp_index"] % 2 == 1:
                    e["move_speed"] -= 1
                elif e["move_speed"] == 1:
                    br["ramp_move_speed_at_1"] += 1
                if e["spawn_speed"] > 1:
                    e["spawn_speed"] -= 1
                e["ramp_index"] += 1
                e["ramp_timer"] = RAMP_INTERVAL
                if e["spawn_speed"] == 1 and e["move_speed"] == 1:
                    br["ramp_last"] += 1
        else:
            br["ramp_frozen"] += 1
        # 8. counters and flags
        e["ep_steps"] += 1
        e["t"] += 1
        at_limit = self.step_limit > 0 and e["ep_steps"] >= self.step_limit
        truncated = at_limit and not terminal
        if terminal:
            br["terminal"] += 1
            if at_limit:
                br["terminal_on_the_limit"] += 1
        if truncated:
            br["truncation"] += 1
        return reward, terminal, truncated

    def image(self, e, count=False):
        img = np.zeros((10, 10, 4), np.uint8)
        img[e["py"], e["px"], 0] = 1
        for i in range(N_SLOTS):
            ent = e["slots"][i]
            if ent is None:
                continue
            img[i + 1, ent["x"], 3 if ent["gold"] else 1] = 1
            back = ent["x"] - ent["dir"]
            if 0 <= back <= 9:
                img[i + 1, back, 2] = 1
            if count:
                self.branches["trail_drawn" if 0 <= back <= 9 else ("trail_clipped_left" if back < 0 else "trail_clipped_right")] += 1
        return img

    # ---- the VectorCollector protocol (float32 observations)
    def reset(self):
        for e in self.envs:
            e["last_action"], e["t"] = 0, 0
            self._reset_one(e)
        return self.observe()

    def observe(self):
        return np.stack([self.image(e) for e in self.envs]).astype(np.float32)

    def step(self, actions, u=None, spawn=None):
        actions = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions).reshape(-1)
        assert actions.shape[0] == self.n_envs
        n = self.n_envs
        next_obs = np.zeros((n, 10, 10, 4), np.float32)
        reward, done, trunc = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i, e in enumerate(self.envs):
            t0 = e["t"]
            c = float(u[i]) if u is not None else coin(self.seed, i, t0)
            if spawn is not None:
                draw_of = lambda k, i=i: tuple(int(v) for v in np.asarray(spawn[i]).reshape(-1))
            else:
                draw_of = lambda k, i=i, t0=t0: draw_spawn(self.seed, i, t0, k)
            reward[i], done[i], trunc[i] = self._step_one(e, actions[i], c, draw_of)
            next_obs[i] = self.image(e, count=True)
            if done[i] or trunc[i]:          # 9. the acting image then comes from a reset
                self._reset_one(e)
        return next_obs, reward, done, trunc

    # ---- state
    def get_state(self):
        out = {f: np.array([e[f] for e in self.envs], dtype=np.uint64 if f == "t" else np.int64) for f in SCALARS}
        for f, key in zip(PER_SLOT, (None, "x", "dir", "gold")):
            out[f] = np.array([[(0 if s is None else 1 if key is None else s[key]) for s in e["slots"]] for e in self.envs],
                              dtype=np.int64).reshape(self.n_envs, N_SLOTS)
        return out

    def set_state(self, state):
        for i, e in enumerate(self.envs):
            for f in SCALARS:
                e[f] = int(state[f][i])
            act, x, d, g = ([int(v) for v in np.asarray(state[f][i]).reshape(-1)] for f in PER_SLOT)
            e["slots"] = [dict(x=x[j], dir=d[j], gold=g[j]) if act[j] else None for j in range(N_SLOTS)]


def assert_same_state(got, want, where=""):
    """Every state field of two ``get_state()`` dicts, exactly: an emptied slot compares as zeros."""
    for f in SCALARS + PER_SLOT:
        kind = np.uint64 if f == "t" else np.int64
        np.testing.assert_array_equal(np.asarray(got[f]).astype(kind), np.asarray(want[f]).astype(kind), err_msg=f"{where}: state field {f}")
