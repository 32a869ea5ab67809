// MinAtar Asterix (10 x 10 x 4 observations, 6 or 5 actions) for N lock-stepped environments: one launch per step, no host
// value that changes between steps (the counters live in the state records), nothing read back.  The rules are the table of
// DESIGN.md 7.5 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own, as
// env_breakout.hip and env_freeway.hip are: their code objects and learner.hip's stay what they were.
//
// One wave per environment, four environments per workgroup.  The game is wave-uniform: every lane computes it from the
// environment's 32-byte state record (one broadcast load, scalar registers after readfirstlane), lane 0 writes the new
// record.  The eight entity slots stay PACKED in two words (x; occupied, direction and gold bits) and every access is a
// constant shift of an unrolled loop -- an array indexed by a slot number would go to the private segment; picking the
// rank-th empty slot is such a loop with a wave-uniform counter.  A board cell is four channels = one store unit (one 16-byte
// store in fp32, one 32-bit word in bytes): lane l owns cells l and l + 64 (< 100), and the at most 17 set elements are
// placed from the state's side (scalar cell arithmetic, one compare per lane and element); a step whose episode goes on
// builds one image and stores it twice.  No LDS, no private segment.
#include "common.h"

namespace prism {

// stream keys, apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD", "ENVB", Freeway's five and from each other
constexpr uint64_t AX_KEY_COIN = 0x41535843ull;           // "ASXC": the sticky coin
constexpr uint64_t AX_KEY_SPAWN = 0x41535853ull;          // "ASXS": side, gold and slot of a spawn
constexpr int AX_THREADS = 256, AX_PER_WG = AX_THREADS / WAVE, AX_SLOTS = 8, AX_CELLS = 100;
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

struct AxArgs {
    int n_envs, n_actions, step_limit, obs_kind;
    double sticky_p;
    uint64_t seed;
    uint32_t *state, *status;
    void *obs_next;          // the ping-pong buffer this launch writes the acting image into
    void *next_obs;          // step only
    float *reward;
    uint8_t *done, *truncated;
    const int64_t *actions;
    const double *u_in;
    const uint8_t *spawn_in;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// An image as a lane holds it: the four channels of cell lane in bits 0..3 of c0, of cell lane + 64 in c1.
struct AxImage {
    uint32_t c0, c1;
};
// OR `bits` into cell `cell` = 10 y + x.  cell and bits are wave-uniform: which of the two words and which lane is scalar
// work, a lane pays one compare and two select-ORs.
__device__ __forceinline__ void ax_set(AxImage &img, int lane, int cell, uint32_t bits) {
    const bool mine = lane == (cell & 63);
    const bool high = cell >= 64;
    img.c0 |= mine ? (high ? 0u : bits) : 0u;
    img.c1 |= mine ? (high ? bits : 0u) : 0u;
}
// Channel 0 at (py, px); per entity of row y = i + 1, channel 3 (gold) or 1 (enemy) at (y, x) and channel 2 at (y, x - dir)
// where that column is on the board.  The slots come out of the packed words by constant shifts (the loop is unrolled).
__device__ __forceinline__ AxImage ax_image(const AxState &s, int lane) {
    AxImage img{0u, 0u};
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
__device__ __forceinline__ void ax_store_cell(void *base, int obs_kind, size_t at, uint32_t b) {
    if (obs_kind == PRISM_OBS_U8) {
        const uint32_t w = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);      // channel j in byte j
        __builtin_nontemporal_store(w, reinterpret_cast<uint32_t *>(base) + at);
    } else {
        stream_store4(reinterpret_cast<float4 *>(base) + at,
                      make_float4((float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)(b >> 3)));
    }
}
// One image of environment `env`: lane l writes cells l and l + 64 (< 100).  Streaming stores: the next launch reads them.
__device__ __forceinline__ void ax_store_image(void *base, int obs_kind, int env, int lane, const AxImage &img) {
    const size_t at = (size_t)env * AX_CELLS + lane;
    ax_store_cell(base, obs_kind, at, img.c0);
    if (lane + 64 < AX_CELLS) ax_store_cell(base, obs_kind, at + 64, img.c1);
}
__device__ __forceinline__ void ax_store_state(uint32_t *rec, const AxState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.xs, s.flags, s.ep_steps, ax_pack(s));
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), (uint32_t)(s.ramp_timer + 1), 0u);
}

__global__ __launch_bounds__(AX_THREADS) void env_asterix_reset_kernel(AxArgs k) {
    const int env = (int)uni(blockIdx.x * AX_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    AxState s;
    s.last_action = 0;
    s.t = 0;
    ax_reset(s);
    ax_store_image(k.obs_next, k.obs_kind, env, lane, ax_image(s, lane));
    if (lane == 0) ax_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(AX_THREADS) void env_asterix_step_kernel(AxArgs k) {
    const int env = (int)uni(blockIdx.x * AX_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 w1 = reinterpret_cast<const uint4 *>(rec)[1];
    AxState s;
    s.xs = uni(w0.x), s.flags = uni(w0.y), s.ep_steps = uni(w0.z);
    ax_unpack(uni(w0.w), s);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);
    s.ramp_timer = (int)(uni(w1.z) & 127u) - 1;
    const uint64_t t0 = s.t;          // the counter of this step's draws
    const int64_t raw = k.actions[env];
    const uint32_t raw_lo = uni((uint32_t)raw), raw_hi = uni((uint32_t)((uint64_t)raw >> 32));

    // the sticky coin
    double u;
    if (k.u_in) {
        const uint64_t ub = __builtin_bit_cast(uint64_t, k.u_in[env]);
        u = __builtin_bit_cast(double, (uint64_t)uni((uint32_t)ub) | ((uint64_t)uni((uint32_t)(ub >> 32)) << 32));
    } else {
        uint32_t r[4];
        Philox(k.seed)(t0, ((uint64_t)env << 32) | AX_KEY_COIN, r);
        u = u64_to_unit_double(uni(r[0]), uni(r[1]));
    }

    // the action: out of range acts as no-op and raises the sticky status bit; the 5-action set is n, l, u, r, d as they are
    const bool valid = raw_hi == 0u && raw_lo < (uint32_t)k.n_actions;
    int a = valid ? (int)raw_lo : 0;
    if (!valid && lane == 0) atomicOr(k.status, (uint32_t)PRISM_ENV_STATUS_BAD_ACTION);
    if (u < k.sticky_p) a = s.last_action;
    s.last_action = a;

    // a spawn (drawn on such a step only; the branch is wave-uniform): the rank-th of the k empty slots, in ascending order
    if (s.spawn_timer == 0) {
        const int empty = AX_SLOTS - __builtin_popcount(s.flags & 255u);
        uint32_t side, gold, rank;
        if (k.spawn_in) {
            const uint8_t *g = k.spawn_in + (size_t)env * 3;
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
    s.ep_steps += 1u;
    s.t += 1ull;
    const bool truncated = k.step_limit > 0 && s.ep_steps >= (uint32_t)k.step_limit && !terminal;

    AxImage img = ax_image(s, lane);
    ax_store_image(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                     // (wave-uniform) only then is the acting image another one
        ax_reset(s);
        img = ax_image(s, lane);
    }
    ax_store_image(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    if (lane == 0) {
        ax_store_state(rec, s);
        k.reward[env] = reward;
        k.done[env] = terminal ? 1 : 0;
        k.truncated[env] = truncated ? 1 : 0;
    }
}

// the checks and texts of env_breakout.hip's check_env but for the action counts: one descriptor, one contract
static int check_env(const prism_env_desc *d) {
    PRISM_CHECK_ARG(d, "null descriptor");
    PRISM_CHECK_ARG(d->n_envs >= 1 && d->n_envs <= PRISM_ENV_MAX, "n_envs must be in [1, 65536]");
    PRISM_CHECK_ARG(d->n_actions == 5 || d->n_actions == 6, "n_actions must be 5 or 6");
    PRISM_CHECK_ARG(d->step_limit >= 0, "step_limit is negative");
    // (written so that a NaN fails it)
    PRISM_CHECK_ARG(d->sticky_p >= 0.0 && d->sticky_p <= 1.0, "sticky_p outside [0, 1]");
    PRISM_CHECK_ARG(d->obs_kind == PRISM_OBS_F32 || d->obs_kind == PRISM_OBS_U8, "obs_kind must be PRISM_OBS_F32 or PRISM_OBS_U8");
    PRISM_CHECK_ARG(d->state && d->status, "null state block / status word");
    PRISM_CHECK_ARG(d->obs[0] && d->obs[1] && d->obs[0] != d->obs[1], "null or shared ping-pong observation buffers");
    PRISM_CHECK_ARG(d->next_obs && d->reward && d->done && d->truncated, "null step outputs");
    PRISM_CHECK_ARG(((uintptr_t)d->state | (uintptr_t)d->obs[0] | (uintptr_t)d->obs[1] | (uintptr_t)d->next_obs) % 16 == 0,
                    "state block and observation buffers must be 16-byte aligned");
    return PRISM_OK;
}

static AxArgs ax_args(const prism_env_desc *d, int parity) {
    return AxArgs{d->n_envs, d->n_actions, d->step_limit, d->obs_kind, d->sticky_p, d->seed, d->state, d->status,
                  d->obs[parity], d->next_obs, d->reward, d->done, d->truncated, nullptr, nullptr, nullptr};
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_asterix_reset(const prism_env_desc *d, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    AxArgs k = ax_args(d, 0);
    hipLaunchKernelGGL(env_asterix_reset_kernel, dim3((d->n_envs + AX_PER_WG - 1) / AX_PER_WG), dim3(AX_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_env_asterix_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *spawn_in,
                                      int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    AxArgs k = ax_args(d, parity ^ 1);
    k.actions = actions, k.u_in = u_in, k.spawn_in = spawn_in;
    hipLaunchKernelGGL(env_asterix_step_kernel, dim3((d->n_envs + AX_PER_WG - 1) / AX_PER_WG), dim3(AX_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
