// MinAtar Asterix (10 x 10 x 4 observations, 6 or 5 actions) on the games' shared frame (env_frame.h).  The rules are the table
// of DESIGN.md 7.5 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own:
// learner.hip's code object stays what it was.
//
// The 32-byte state record comes in through one broadcast load, lane 0 writes the new one.  The eight entity slots stay PACKED
// in two words (x; occupied, direction and gold bits) and every access is a constant shift of an unrolled loop -- an array
// indexed by a slot number would go to the private segment; picking the rank-th empty slot is such a loop with a wave-uniform
// counter.  A board cell is four channels = one chunk: lane l owns cells l and l + 64 (< 100), and the at most 17 set elements
// are placed from the state's side (scalar cell arithmetic, one compare per lane and element); a step whose episode goes on
// builds one image and stores it twice.  No LDS, no private segment.
#include "env_frame.h"

namespace prism {

// stream keys, apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD", "ENVB", Freeway's five and from each other
constexpr uint64_t AX_KEY_COIN = 0x41535843ull;           // "ASXC": the sticky coin
constexpr uint64_t AX_KEY_SPAWN = 0x41535853ull;          // "ASXS": side, gold and slot of a spawn
constexpr int AX_SLOTS = 8, AX_CELLS = 100;
constexpr int AX_SPAWN_SPEED = 10, AX_MOVE_SPEED = 5, AX_RAMP_INTERVAL = 100;
constexpr uint32_t AX_SLOT_BITS = 0x010101u;              // occupied | direction | gold of slot 0
static_assert(AX_CELLS <= 2 * WAVE, "lane l takes cells l and l + 64");

// The state record: PRISM_ENV_STATE_WORDS uint32 (include/prism_hip.h has the field map)
//   [0] x of slot i in bits 4i..4i+3   [1] occupied bit i, direction (1: +x) bit 8 + i, gold bit 16 + i
//   [2] ep_steps   [3] packed small fields   [4] t low   [5] t high   [6] ramp_timer + 1   [7] 0
// An empty slot holds zeros in all of its fields.
struct AxState {
    uint32_t xs, flags;
    int px, py, spawn_speed, spawn_timer, move_speed, move_timer, last_action, ramp_index, ramp_timer;
    uint32_t ep_steps;
    uint64_t t;
};
__host__ __device__ inline uint32_t ax_pack(const AxState &s) {
    return (uint32_t)s.px | ((uint32_t)s.py << 4) | ((uint32_t)s.spawn_speed << 8) | ((uint32_t)s.spawn_timer << 12) |
           ((uint32_t)s.move_speed << 16) | ((uint32_t)s.move_timer << 19) | ((uint32_t)s.last_action << 22) |
           ((uint32_t)s.ramp_index << 25);
}
__host__ __device__ inline void ax_unpack(uint32_t w, AxState &s) {
    s.px = w & 15, s.py = (w >> 4) & 15, s.spawn_speed = (w >> 8) & 15, s.spawn_timer = (w >> 12) & 15;
    s.move_speed = (w >> 16) & 7, s.move_timer = (w >> 19) & 7, s.last_action = (w >> 22) & 7, s.ramp_index = (w >> 25) & 31;
}
// "Reset": last_action and t carry over; no draw
__host__ __device__ inline void ax_reset(AxState &s) {
    s.xs = s.flags = 0u;
    s.px = s.py = 5;
    s.spawn_speed = s.spawn_timer = AX_SPAWN_SPEED;
    s.move_speed = s.move_timer = AX_MOVE_SPEED;
    s.ramp_timer = AX_RAMP_INTERVAL;
    s.ramp_index = 0;
    s.ep_steps = 0;
}
__host__ __device__ inline void ax_empty(AxState &s, int i) {
    s.xs &= ~(15u << (4 * i));
    s.flags &= ~(AX_SLOT_BITS << i);
}

// An image as a lane holds it: the four channels of cell lane in bits 0..3, of cell lane + 64 in bits 4..7.
// OR `bits` into cell `cell` = 10 y + x.  cell and bits are wave-uniform: which nibble and which lane is scalar work, a lane
// pays one compare and one select-OR.
__device__ __forceinline__ void ax_set(uint32_t &img, int lane, int cell, uint32_t bits) {
    img |= lane == (cell & 63) ? bits << (4 * (cell >> 6)) : 0u;
}
// Channel 0 at (py, px); per entity of row y = i + 1, channel 3 (gold) or 1 (enemy) at (y, x) and channel 2 at (y, x - dir)
// where that column is on the board.  The slots come out of the packed words by constant shifts (the loop is unrolled).
__device__ __forceinline__ uint32_t ax_image(const AxState &s, int lane) {
    uint32_t img = 0u;
    ax_set(img, lane, 10 * s.py + s.px, 1u);
#pragma unroll
    for (int i = 0; i < AX_SLOTS; ++i) {
        const bool there = (s.flags >> i) & 1u, plus = (s.flags >> (8 + i)) & 1u, gold = (s.flags >> (16 + i)) & 1u;
        const int x = (int)((s.xs >> (4 * i)) & 15u), back = plus ? x - 1 : x + 1;
        ax_set(img, lane, 10 * (i + 1) + x, there ? (gold ? 8u : 2u) : 0u);
        ax_set(img, lane, 10 * (i + 1) + (back & 15), there && back >= 0 && back <= 9 ? 4u : 0u);
    }
    return img;
}
__device__ __forceinline__ void ax_store_state(uint32_t *rec, const AxState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.xs, s.flags, s.ep_steps, ax_pack(s));
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), (uint32_t)(s.ramp_timer + 1), 0u);
}

__global__ __launch_bounds__(ENV_THREADS) void env_asterix_reset_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    AxState s;
    s.last_action = 0;
    s.t = 0;
    ax_reset(s);
    env_store_image<AX_CELLS>(k.obs_next, k.obs_kind, env, lane, ax_image(s, lane));
    if (lane == 0) ax_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(ENV_THREADS) void env_asterix_step_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 w1 = reinterpret_cast<const uint4 *>(rec)[1];
    AxState s;
    s.xs = uni(w0.x), s.flags = uni(w0.y), s.ep_steps = uni(w0.z);
    ax_unpack(uni(w0.w), s);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);
    s.ramp_timer = (int)(uni(w1.z) & 127u) - 1;
    const uint64_t t0 = s.t;          // the counter of this step's draws

    // (the action's load is in flight while the coin is drawn)
    int a = env_action(k.actions, env, k.n_actions, k.status, lane);
    const double u = env_coin(k.u_in, k.seed, t0, env, AX_KEY_COIN);
    // the 5-action set is n, l, u, r, d as they are
    a = env_sticky(a, u, k.sticky_p, s.last_action);

    // a spawn (drawn on such a step only; the branch is wave-uniform): the rank-th of the k empty slots, in ascending order
    if (s.spawn_timer == 0) {
        const int empty = AX_SLOTS - __builtin_popcount(s.flags & 255u);
        uint32_t side, gold, rank;
        if (k.draws_in) {
            const uint8_t *g = static_cast<const uint8_t *>(k.draws_in) + (size_t)env * 3;
            side = uni(g[0]) & 1u, gold = uni(g[1]) & 1u, rank = uni(g[2]);
            if ((int)rank >= empty) rank = (uint32_t)(empty - 1);          // a guard: the drawn rank is below k
        } else {
            uint32_t r[4];
            Philox(k.seed)(t0, ((uint64_t)env << 32) | AX_KEY_SPAWN, r);
            side = uni(r[0]) & 1u;
            gold = (uint32_t)(((uint64_t)uni(r[1]) * 3ull) >> 32) == 0u ? 1u : 0u;
            rank = (uint32_t)(((uint64_t)uni(r[2]) * (uint64_t)empty) >> 32);
        }
        int seen = 0;
#pragma unroll
        for (int i = 0; i < AX_SLOTS; ++i) {
            const bool free_slot = !((s.flags >> i) & 1u);
            if (free_slot && empty > 0 && seen == (int)rank) {
                s.xs |= (side ? 0u : 9u) << (4 * i);
                s.flags |= (1u | (side << 8) | (gold << 16)) << i;
            }
            seen += free_slot;
        }
        s.spawn_timer = s.spawn_speed;
    }
    // the player
    if (a == 1) s.px = max(0, s.px - 1);
    else if (a == 3) s.px = min(9, s.px + 1);
    else if (a == 2) s.py = max(1, s.py - 1);
    else if (a == 4) s.py = min(8, s.py + 1);
    // contact before the move: a gold is collected, an enemy ends the episode
    float reward = 0.f;
    bool terminal = false;
#pragma unroll
    for (int i = 0; i < AX_SLOTS; ++i) {
        if (((s.flags >> i) & 1u) && s.py == i + 1 && (int)((s.xs >> (4 * i)) & 15u) == s.px) {
            if ((s.flags >> (16 + i)) & 1u) {
                ax_empty(s, i);
                reward += 1.f;
            } else {
                terminal = true;
            }
        }
    }
    // the entities, in order: off the board a slot empties, on the player's cell the contact rule again
    if (s.move_timer == 0) {
        s.move_timer = s.move_speed;
#pragma unroll
        for (int i = 0; i < AX_SLOTS; ++i) {
            if ((s.flags >> i) & 1u) {
                const int x = (int)((s.xs >> (4 * i)) & 15u) + (((s.flags >> (8 + i)) & 1u) ? 1 : -1);
                if (x < 0 || x > 9) {
                    ax_empty(s, i);
                } else {
                    s.xs = (s.xs & ~(15u << (4 * i))) | ((uint32_t)x << (4 * i));
                    if (s.py == i + 1 && x == s.px) {
                        if ((s.flags >> (16 + i)) & 1u) {
                            ax_empty(s, i);
                            reward += 1.f;
                        } else {
                            terminal = true;
                        }
                    }
                }
            }
        }
    }
    // the timers and the ramp
    s.spawn_timer -= 1;
    s.move_timer -= 1;
    if (s.spawn_speed > 1 || s.move_speed > 1) {
        if (s.ramp_timer >= 0) {
            s.ramp_timer -= 1;
        } else {
            if (s.move_speed > 1 && (s.ramp_index & 1)) s.move_speed -= 1;
            if (s.spawn_speed > 1) s.spawn_speed -= 1;
            s.ramp_index += 1;
            s.ramp_timer = AX_RAMP_INTERVAL;
        }
    }
    const bool truncated = env_count_step(s.ep_steps, s.t, k.step_limit, terminal);

    uint32_t img = ax_image(s, lane);
    env_store_image<AX_CELLS>(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                                // (wave-uniform) only then is the acting image another one
        ax_reset(s);
        img = ax_image(s, lane);
    }
    env_store_image<AX_CELLS>(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    if (lane == 0) ax_store_state(rec, s);
    env_store_outcome(k, env, lane, reward, terminal, truncated);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_asterix_reset(const prism_env_desc *d, prism_stream_t stream_) {
    const int rc = check_env(d, 5, "n_actions must be 5 or 6");
    if (rc != PRISM_OK) return rc;
    return env_launch(env_asterix_reset_kernel, env_args(d, 0), stream_);
}

extern "C" int prism_env_asterix_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *spawn_in,
                                      int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d, 5, "n_actions must be 5 or 6");
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    return env_launch(env_asterix_step_kernel, env_args(d, parity ^ 1, actions, u_in, spawn_in), stream_);
}
