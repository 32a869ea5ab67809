"""``HostSeaquest``: the Seaquest rules of DESIGN.md 7.7 restated in plain Python, one environment at a time -- the checker of
``prism_env_seaquest_step`` (include/prism_hip.h).  Written from the rule table, not from the kernel, and in the LIST form: five
Python lists per environment (friendly bullets, enemy bullets, fish, enemy subs, divers) that grow with ``append`` and shrink
with ``del``, walked ``reversed`` as MinAtar walks them, one ``if`` per rule -- so the kernel's bounded arrays, its ballots and
its compaction are checked against lists and not against themselves.  The lists have no bound of their own; the record's
capacities (``CAPACITY``) enter at one place only, ``_append``: an append to a list that already holds its capacity is
dropped and counted (``overflow``), which is what the device does and reports through its status word.  The rules are
MinAtar v1 as this project restates them; they are NOT checked against the ``minatar`` package.  No part of ``prism_amd/``
uses this file.

The coins and spawns are given (``step(actions, u=..., draws=...)``) or drawn through ``tests/helpers.py philox4x32`` exactly
as the device draws them.  ``branches`` counts which rule every step took."""
import numpy as np

from tests.helpers import philox4x32

KEY_COIN, KEY_ENEMY, KEY_DIVER = 0x53515843, 0x53515845, 0x53515844          # "SQXC", "SQXE", "SQXD"
MAX_OXYGEN, MAX_DIVERS, SHOT_COOL_DOWN, ENEMY_SHOT_INTERVAL = 200, 6, 5, 10
ENEMY_SPAWN_SPEED, DIVER_SPAWN_SPEED, ENEMY_MOVE_SPEED, DIVER_MOVE_INTERVAL, MOVE_SPEED_MIN = 20, 30, 5, 5, 2
CAPACITY = dict(e_fish=32, e_subs=32, e_bullets=32, f_bullets=4, divers=4)
SCALARS = ("sub_x", "sub_y", "sub_or", "oxygen", "diver_count", "surface", "shot_timer", "e_spawn_speed", "e_spawn_timer",
           "d_spawn_timer", "move_speed", "ramp_index", "last_action", "ep_steps", "t")
LISTS = ("f_bullets", "e_bullets", "e_fish", "e_subs", "divers")
BRANCHES = ("sticky_repeat", "bad_action", "reset",
            "spawn_fish", "spawn_sub", "spawn_from_left", "spawn_from_right", "spawn_blocked", "spawn_beside_same_direction",
            "spawn_diver",
            "fire", "fire_cooling", "move_left", "move_right", "move_up", "move_down", "clamp_left", "clamp_right", "clamp_up",
            "clamp_down", "noop",
            "f_bullet_leaves_left", "f_bullet_leaves_right", "f_bullet_hits_fish", "f_bullet_hits_sub", "f_bullet_picks_first_of_stack",
            "f_bullet_prefers_fish", "f_bullet_flies",
            "diver_picked_before_move", "diver_picked_after_move", "diver_refused", "diver_moves", "diver_waits", "diver_leaves",
            "sub_contact_before_move", "sub_contact_after_move", "sub_moves", "sub_waits", "sub_leaves", "sub_walks_onto_bullet",
            "sub_fires", "sub_fires_on_its_move", "sub_counts_down",
            "e_bullet_contact_before_move", "e_bullet_contact_after_move", "e_bullet_leaves_left", "e_bullet_leaves_right",
            "e_bullet_flies", "two_e_bullets_in_a_row",
            "fish_contact_before_move", "fish_contact_after_move", "fish_moves", "fish_waits", "fish_leaves", "fish_walks_onto_bullet",
            "oxygen_out", "under_water", "at_surface_already", "surface_without_divers", "surface_with_some", "surface_with_six",
            "ramp_move_speed", "ramp_spawn_speed_only", "ramp_over",
            "overflow", "terminal", "truncation", "terminal_on_the_limit")


def unit_double(hi, lo):
    """common.h u64_to_unit_double: 27 + 26 bits."""
    return (float(int(hi) >> 5) * 67108864.0 + float(int(lo) >> 6)) / 9007199254740992.0


def draw(seed, env, counter, key):
    """The four words of one environment's draw at ``counter`` under stream key ``key``."""
    return philox4x32(seed, np.array([counter], dtype=np.uint64), (int(env) << 32) | key)[0]


def coin(seed, env, counter):
    r = draw(seed, env, counter, KEY_COIN)
    return unit_double(r[0], r[1])


def enemy_map(w):
    """(side, is_sub, row) of the words of an enemy-spawn draw."""
    return int(w[0]) & 1, int((int(w[1]) * 3) >> 32 == 0), 1 + (int(w[2]) >> 29)


def diver_map(w):
    """(side, row) of the words of a diver-spawn draw."""
    return int(w[0]) & 1, 1 + (int(w[1]) >> 29)


class HostSeaquest:
    def __init__(self, n_envs, seed=0, sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False):
        self.n_envs, self.seed = int(n_envs), int(seed)
        self.sticky_p, self.step_limit = float(sticky_action_prob), int(episode_timestep_limit)
        self.n_actions = 6                                   # the minimal set is all six
        self.obs_shape = (10, 10, 10)
        self.envs = [dict(last_action=0, t=0) for _ in range(self.n_envs)]
        self.branches = {b: 0 for b in BRANCHES}
        for e in self.envs:
            self._reset_one(e)
        self.branches["reset"] = 0
        self.bad_action = False
        self.overflow = False

    # ---- the rules
    def _reset_one(self, e):
        e["sub_x"], e["sub_y"], e["sub_or"] = 5, 0, 0
        e["oxygen"], e["diver_count"], e["surface"], e["shot_timer"] = MAX_OXYGEN, 0, 1, 0
        e["e_spawn_speed"] = e["e_spawn_timer"] = ENEMY_SPAWN_SPEED
        e["d_spawn_timer"], e["move_speed"], e["ramp_index"], e["ep_steps"] = DIVER_SPAWN_SPEED, ENEMY_MOVE_SPEED, 0, 0
        for name in LISTS:
            e[name] = []
        self.branches["reset"] += 1

    def _append(self, e, name, entry):
        if len(e[name]) >= CAPACITY[name]:                  # the record is full: the device drops the append and says so
            self.overflow = True
            self.branches["overflow"] += 1
            return
        e[name].append(list(entry))

    def _enemies(self, e, name, with_shot):
        """Rules 7 and 9: one list of enemies, last to first -> (reward, terminal)."""
        br, reward, terminal = self.branches, 0.0, False
        kind = "sub" if with_shot else "fish"
        sub = [e["sub_x"], e["sub_y"]]
        for ent in list(reversed(e[name])):
            present = True
            if ent[0:2] == sub:
                terminal = True
                br[kind + "_contact_before_move"] += 1
            moved = ent[3] == 0
            if moved:
                ent[3] = e["move_speed"]
                ent[0] += ent[2]
                if not 0 <= ent[0] <= 9:
                    e[name] = [x for x in e[name] if x is not ent]
                    present = False
                    br[kind + "_leaves"] += 1
                elif ent[0:2] == sub:
                    terminal = True
                    br[kind + "_contact_after_move"] += 1
                else:
                    br[kind + "_moves"] += 1
                    for b in e["f_bullets"]:
                        if b[0:2] == ent[0:2]:
                            e["f_bullets"] = [x for x in e["f_bullets"] if x is not b]
                            e[name] = [x for x in e[name] if x is not ent]
                            present = False
                            reward += 1.0
                            br[kind + "_walks_onto_bullet"] += 1
                            break
            else:
                ent[3] -= 1
                br[kind + "_waits"] += 1
            if with_shot and present:
                if ent[4] == 0:
                    ent[4] = ENEMY_SHOT_INTERVAL
                    self._append(e, "e_bullets", ent[0:3])
                    br["sub_fires"] += 1
                    if moved:
                        br["sub_fires_on_its_move"] += 1
                else:
                    ent[4] -= 1
                    br["sub_counts_down"] += 1
        return reward, terminal

    def _step_one(self, e, action, u, enemy_draw, diver_draw):
        """-> (reward, terminal, truncated); the state is the post-step state, before any reset."""
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
        reward, terminal = 0.0, False
        # 2. an enemy enters
        if e["e_spawn_timer"] == 0:
            side, is_sub, row = enemy_draw()
            direction = 1 if side else -1
            others = [x for x in e["e_fish"] + e["e_subs"] if x[1] == row]
            if any(x[2] != direction for x in others):
                br["spawn_blocked"] += 1
            else:
                if others:
                    br["spawn_beside_same_direction"] += 1
                br["spawn_from_left" if side else "spawn_from_right"] += 1
                x0 = 0 if side else 9
                if is_sub:
                    self._append(e, "e_subs", [x0, row, direction, e["move_speed"], ENEMY_SHOT_INTERVAL])
                    br["spawn_sub"] += 1
                else:
                    self._append(e, "e_fish", [x0, row, direction, e["move_speed"]])
                    br["spawn_fish"] += 1
            e["e_spawn_timer"] = e["e_spawn_speed"]
        # 3. a diver enters
        if e["d_spawn_timer"] == 0:
            side, row = diver_draw()
            self._append(e, "divers", [0 if side else 9, row, 1 if side else -1, DIVER_MOVE_INTERVAL])
            br["spawn_diver"] += 1
            e["d_spawn_timer"] = DIVER_SPAWN_SPEED
        # 4. the player
        if a == 5:
            if e["shot_timer"] == 0:
                self._append(e, "f_bullets", [e["sub_x"], e["sub_y"], 1 if e["sub_or"] else -1])
                e["shot_timer"] = SHOT_COOL_DOWN
                br["fire"] += 1
            else:
                br["fire_cooling"] += 1
        elif a == 1:
            br["clamp_left" if e["sub_x"] == 0 else "move_left"] += 1
            e["sub_x"], e["sub_or"] = max(0, e["sub_x"] - 1), 0
        elif a == 3:
            br["clamp_right" if e["sub_x"] == 9 else "move_right"] += 1
            e["sub_x"], e["sub_or"] = min(9, e["sub_x"] + 1), 1
        elif a == 2:
            br["clamp_up" if e["sub_y"] == 0 else "move_up"] += 1
            e["sub_y"] = max(0, e["sub_y"] - 1)
        elif a == 4:
            br["clamp_down" if e["sub_y"] == 8 else "move_down"] += 1
            e["sub_y"] = min(8, e["sub_y"] + 1)
        else:
            br["noop"] += 1
        # 5. friendly bullets, last to first
        for b in list(reversed(e["f_bullets"])):
            b[0] += b[2]
            if not 0 <= b[0] <= 9:
                e["f_bullets"] = [x for x in e["f_bullets"] if x is not b]
                br["f_bullet_leaves_left" if b[0] < 0 else "f_bullet_leaves_right"] += 1
                continue
            fish = [x for x in e["e_fish"] if x[0:2] == b[0:2]]
            subs = [x for x in e["e_subs"] if x[0:2] == b[0:2]]
            if fish or subs:
                if len(fish) + len(subs) >= 3:
                    br["f_bullet_picks_first_of_stack"] += 1
                if fish and subs:
                    br["f_bullet_prefers_fish"] += 1
                name, victim = ("e_fish", fish[0]) if fish else ("e_subs", subs[0])          # the first in list order
                e[name] = [x for x in e[name] if x is not victim]
                e["f_bullets"] = [x for x in e["f_bullets"] if x is not b]
                reward += 1.0
                br["f_bullet_hits_fish" if fish else "f_bullet_hits_sub"] += 1
            else:
                br["f_bullet_flies"] += 1
        # 6. divers, last to first
        for d in list(reversed(e["divers"])):
            if d[0:2] == [e["sub_x"], e["sub_y"]] and e["diver_count"] < MAX_DIVERS:
                e["divers"] = [x for x in e["divers"] if x is not d]
                e["diver_count"] += 1
                br["diver_picked_before_move"] += 1
            elif d[3] == 0:
                d[3] = DIVER_MOVE_INTERVAL
                d[0] += d[2]
                if d[0:2] == [e["sub_x"], e["sub_y"]] and e["diver_count"] >= MAX_DIVERS:
                    br["diver_refused"] += 1
                if not 0 <= d[0] <= 9:
                    e["divers"] = [x for x in e["divers"] if x is not d]
                    br["diver_leaves"] += 1
                elif d[0:2] == [e["sub_x"], e["sub_y"]] and e["diver_count"] < MAX_DIVERS:
                    e["divers"] = [x for x in e["divers"] if x is not d]
                    e["diver_count"] += 1
                    br["diver_picked_after_move"] += 1
                else:
                    br["diver_moves"] += 1
            else:
                if d[0:2] == [e["sub_x"], e["sub_y"]]:
                    br["diver_refused"] += 1
                d[3] -= 1
                br["diver_waits"] += 1
        # 7. enemy subs, last to first
        r, term = self._enemies(e, "e_subs", True)
        reward, terminal = reward + r, terminal or term
        # 8. enemy bullets, last to first
        for b in list(reversed(e["e_bullets"])):
            if b[0:2] == [e["sub_x"], e["sub_y"]]:
                terminal = True
                br["e_bullet_contact_before_move"] += 1
            b[0] += b[2]
            if not 0 <= b[0] <= 9:
                e["e_bullets"] = [x for x in e["e_bullets"] if x is not b]
                br["e_bullet_leaves_left" if b[0] < 0 else "e_bullet_leaves_right"] += 1
            else:
                br["e_bullet_flies"] += 1
                if b[0:2] == [e["sub_x"], e["sub_y"]]:
                    terminal = True
                    br["e_bullet_contact_after_move"] += 1
        rows = [b[1] for b in e["e_bullets"]]
        if len(rows) != len(set(rows)):
            br["two_e_bullets_in_a_row"] += 1
        # 9. enemy fish, last to first
        r, term = self._enemies(e, "e_fish", False)
        reward, terminal = reward + r, terminal or term
        # 10. timers
        for timer in ("e_spawn_timer", "d_spawn_timer", "shot_timer"):
            if e[timer] > 0:
                e[timer] -= 1
        # 11. oxygen, surfacing and the ramp
        if e["oxygen"] < 0:
            terminal = True
            br["oxygen_out"] += 1
        if e["sub_y"] > 0:
            e["oxygen"] -= 1
            e["surface"] = 0
            br["under_water"] += 1
        elif e["surface"]:
            br["at_surface_already"] += 1
        elif e["diver_count"] == 0:
            terminal = True
            br["surface_without_divers"] += 1
        else:
            e["surface"] = 1
            if e["diver_count"] == MAX_DIVERS:
                reward += float(e["oxygen"] * 10 // MAX_OXYGEN)          # (Python's floor)
                e["diver_count"] = 0
                br["surface_with_six"] += 1
            else:
                e["diver_count"] -= 1
                br["surface_with_some"] += 1
            e["oxygen"] = MAX_OXYGEN
            if e["e_spawn_speed"] > 1 or e["move_speed"] > MOVE_SPEED_MIN:
                if e["move_speed"] > MOVE_SPEED_MIN and e["ramp_index"] % 2 == 1:
                    e["move_speed"] -= 1
                    br["ramp_move_speed"] += 1
                else:
                    br["ramp_spawn_speed_only"] += 1
                if e["e_spawn_speed"] > 1:
                    e["e_spawn_speed"] -= 1
                e["ramp_index"] += 1
            else:
                br["ramp_over"] += 1
        # 12. counters and flags
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

    @staticmethod
    def image(e):
        img = np.zeros((10, 10, 10), np.uint8)
        img[e["sub_y"], e["sub_x"], 0] = 1
        back = e["sub_x"] - 1 if e["sub_or"] else e["sub_x"] + 1
        assert 0 <= back <= 9, "the cell behind the sub is off the board: no state of the device's record"
        img[e["sub_y"], back, 1] = 1
        for b in e["f_bullets"]:
            img[b[1], b[0], 2] = 1
        for b in e["e_bullets"]:
            img[b[1], b[0], 4] = 1
        for name, ch in (("e_fish", 5), ("e_subs", 6), ("divers", 9)):
            for x in e[name]:
                img[x[1], x[0], ch] = 1
                if 0 <= x[0] - x[2] <= 9:
                    img[x[1], x[0] - x[2], 3] = 1
        img[9, 0:max(0, e["oxygen"] * 10 // MAX_OXYGEN), 7] = 1
        img[9, 9 - e["diver_count"]:9, 8] = 1
        return img

    # ---- the VectorCollector protocol (float32 observations)
    def reset(self):
        for e in self.envs:
            e["last_action"], e["t"] = 0, 0
            self._reset_one(e)
        return self.observe()

    def observe(self):
        return np.stack([self.image(e) for e in self.envs]).astype(np.float32)

    def step(self, actions, u=None, draws=None):
        actions = np.asarray(actions.cpu() if hasattr(actions, "cpu") else actions).reshape(-1)
        assert actions.shape[0] == self.n_envs
        n = self.n_envs
        given = None if draws is None else np.asarray(draws).reshape(n, 5)
        next_obs = np.zeros((n, 10, 10, 10), np.float32)
        reward, done, trunc = np.zeros(n, np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        for i, e in enumerate(self.envs):
            t0 = e["t"]
            c = float(u[i]) if u is not None else coin(self.seed, i, t0)
            if given is not None:
                enemy_draw = lambda i=i: tuple(int(v) for v in given[i, 0:3])
                diver_draw = lambda i=i: tuple(int(v) for v in given[i, 3:5])
            else:
                enemy_draw = lambda i=i, t0=t0: enemy_map(draw(self.seed, i, t0, KEY_ENEMY))
                diver_draw = lambda i=i, t0=t0: diver_map(draw(self.seed, i, t0, KEY_DIVER))
            reward[i], done[i], trunc[i] = self._step_one(e, actions[i], c, enemy_draw, diver_draw)
            next_obs[i] = self.image(e)
            if done[i] or trunc[i]:          # the acting image then comes from a reset
                self._reset_one(e)
        return next_obs, reward, done, trunc

    # ---- state, in the device's field names
    def get_state(self):
        out = {f: np.array([e[f] for e in self.envs], dtype=np.uint64 if f == "t" else np.int64) for f in SCALARS}
        for f in LISTS:
            out[f] = [[tuple(x) for x in e[f]] for e in self.envs]
        return out

    def set_state(self, state):
        for i, e in enumerate(self.envs):
            for f in SCALARS:
                e[f] = int(state[f][i])
            for f in LISTS:
                e[f] = [[int(v) for v in x] for x in state[f][i]]


def assert_same_state(got, want, where=""):
    """Every state field of two ``get_state()`` dicts, exactly."""
    for f in SCALARS:
        kind = np.uint64 if f == "t" else np.int64
        np.testing.assert_array_equal(np.asarray(got[f]).astype(kind), np.asarray(want[f]).astype(kind), err_msg=f"{where}: state field {f}")
    for f in LISTS:
        a = [[tuple(int(v) for v in x) for x in env] for env in got[f]]
        b = [[tuple(int(v) for v in x) for x in env] for env in want[f]]
        assert a == b, f"{where}: list {f}: {a} != {b}"
