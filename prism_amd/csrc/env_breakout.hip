// MinAtar Breakout (10 x 10 x 4 observations, 6 or 3 actions) for N lock-stepped environments: one launch per step, no host
// value that changes between steps (the counters live in the state records), nothing read back.  The rules are the table of
// DESIGN.md 7.3 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own:
// learner.hip's code object stays what it was.
//
// One wave per environment, four environments per workgroup.  The game is wave-uniform: every lane computes it from the
// environment's 32-byte state record (read through one broadcast load, held in scalar registers after readfirstlane), lane 0
// writes the new record, and the 64 lanes write the planes: board cell (y, x) is four channels = one 16-byte store in fp32,
// one 32-bit word in bytes; a wave's stores are contiguous HWC rows (1 KB, then 576 B).  No LDS, no private segment.
#include "common.h"

namespace prism {

constexpr uint64_t ENV_KEY = 0x454E5642ull;          // "ENVB": apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD"
constexpr int ENV_THREADS = 256, ENV_PER_WG = ENV_THREADS / WAVE, ENV_CELLS = 100;
constexpr uint32_t ENV_FULL_BRICKS = (1u << 30) - 1;          // rows 1..3: bit 10 (y - 1) + x

// The state record: PRISM_ENV_STATE_WORDS uint32 (include/prism_hip.h has the field map of word 1)
//   [0] bricks   [1] packed small fields   [2] ep_steps   [3] 0   [4] t low   [5] t high   [6] 0   [7] 0
struct EnvState {
    uint32_t bricks;
    int pos, ball_x, ball_y, dir, last_x, last_y, strike, last_action;
    uint32_t ep_steps;
    uint64_t t;
};
__host__ __device__ inline uint32_t env_pack(const EnvState &s) {
    return (uint32_t)s.pos | ((uint32_t)s.ball_x << 4) | ((uint32_t)s.ball_y << 8) | ((uint32_t)s.dir << 12) |
           ((uint32_t)s.last_x << 16) | ((uint32_t)s.last_y << 20) | ((uint32_t)s.strike << 24) | ((uint32_t)s.last_action << 25);
}
__host__ __device__ inline void env_unpack(uint32_t w, EnvState &s) {
    s.pos = w & 15, s.ball_x = (w >> 4) & 15, s.ball_y = (w >> 8) & 15, s.dir = (w >> 12) & 3;
    s.last_x = (w >> 16) & 15, s.last_y = (w >> 20) & 15, s.strike = (w >> 24) & 1, s.last_action = (w >> 25) & 7;
}
// "Reset with side s": last_action and t carry over
__host__ __device__ inline void env_reset(EnvState &s, int side) {
    s.ball_y = 3;
    s.ball_x = side ? 9 : 0;
    s.dir = side ? 3 : 2;
    s.pos = 4;
    s.bricks = ENV_FULL_BRICKS;
    s.strike = 0;
    s.last_x = s.ball_x, s.last_y = s.ball_y;
    s.ep_steps = 0;
}
__host__ __device__ inline bool env_brick(uint32_t bricks, int y, int x) {
    return y >= 1 && y <= 3 && ((bricks >> (10 * (y - 1) + x)) & 1u);
}

struct EnvArgs {
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
    const uint8_t *side_in;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the four channels of board cell c = 10 y + x as bits 0..3
__device__ __forceinline__ uint32_t env_cell(const EnvState &s, int c) {
    const int y = c / 10, x = c - 10 * y;
    return (uint32_t)(y == 9 && x == s.pos) | ((uint32_t)(y == s.ball_y && x == s.ball_x) << 1) |
           ((uint32_t)(y == s.last_y && x == s.last_x) << 2) | ((uint32_t)env_brick(s.bricks, y, x) << 3);
}
// One image of environment `env`: lane l writes cells l and l + 64 (< 100).  Streaming stores: the next launch reads them.
__device__ __forceinline__ void env_store_image(void *base, int obs_kind, int env, int lane, const EnvState &s) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int c = lane + 64 * k;
        if (c >= ENV_CELLS) break;
        const uint32_t b = env_cell(s, c);
        const size_t at = (size_t)env * ENV_CELLS + c;
        if (obs_kind == PRISM_OBS_U8) {
            const uint32_t w = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);      // channel j in byte j
            __builtin_nontemporal_store(w, reinterpret_cast<uint32_t *>(base) + at);
        } else {
            stream_store4(reinterpret_cast<float4 *>(base) + at,
                          make_float4((float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)(b >> 3)));
        }
    }
}
__device__ __forceinline__ void env_store_state(uint32_t *rec, const EnvState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.bricks, env_pack(s), s.ep_steps, 0u);
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), 0u, 0u);
}

__global__ __launch_bounds__(ENV_THREADS) void env_breakout_reset_kernel(EnvArgs k) {
    const int env = (int)uni(blockIdx.x * ENV_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    int side;
    if (k.side_in) {
        side = (int)uni(k.side_in[env]) & 1;
    } else {
        uint32_t r[4];
        Philox(k.seed)(~0ull, ((uint64_t)env << 32) | ENV_KEY, r);
        side = (int)uni(r[3] & 1u);
    }
    EnvState s;
    s.last_action = 0;
    s.t = 0;
    env_reset(s, side);
    env_store_image(k.obs_next, k.obs_kind, env, lane, s);
    if (lane == 0) env_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(ENV_THREADS) void env_breakout_step_kernel(EnvArgs k) {
    const int env = (int)uni(blockIdx.x * ENV_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint2 w1 = reinterpret_cast<const uint2 *>(rec)[2];
    EnvState s;
    s.bricks = uni(w0.x);
    env_unpack(uni(w0.y), s);
    s.ep_steps = uni(w0.z);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);
    const int64_t raw = k.actions[env];
    const uint32_t raw_lo = uni((uint32_t)raw), raw_hi = uni((uint32_t)((uint64_t)raw >> 32));

    // the draws of this step: the sticky coin and the side of the episode that begins if this step ends one
    double u = 1.0;
    int side = 0;
    if (!(k.u_in && k.side_in)) {
        uint32_t r[4];
        Philox(k.seed)(s.t, ((uint64_t)env << 32) | ENV_KEY, r);
        u = u64_to_unit_double(uni(r[0]), uni(r[1]));
        side = (int)uni(r[2] & 1u);
    }
    if (k.u_in) {
        const uint64_t ub = __builtin_bit_cast(uint64_t, k.u_in[env]);
        u = __builtin_bit_cast(double, (uint64_t)uni((uint32_t)ub) | ((uint64_t)uni((uint32_t)(ub >> 32)) << 32));
    }
    if (k.side_in) side = (int)uni(k.side_in[env]) & 1;

    // the action: out of range acts as no-op and raises the sticky status bit; the 3-action set is n, l, r
    const bool valid = raw_hi == 0u && raw_lo < (uint32_t)k.n_actions;
    int a = valid ? (int)raw_lo : 0;
    if (k.n_actions == 3) a = a == 2 ? 3 : a;
    if (!valid && lane == 0) atomicOr(k.status, (uint32_t)PRISM_ENV_STATUS_BAD_ACTION);
    if (u < k.sticky_p) a = s.last_action;
    s.last_action = a;

    if (a == 1) s.pos = max(0, s.pos - 1);
    else if (a == 3) s.pos = min(9, s.pos + 1);
    const int bx = s.ball_x;
    s.last_x = s.ball_x, s.last_y = s.ball_y;
    int nx = s.ball_x + ((s.dir == 1 || s.dir == 2) ? 1 : -1);
    int ny = s.ball_y + (s.dir >= 2 ? 1 : -1);
    if (nx < 0 || nx > 9) {
        nx = nx < 0 ? 0 : 9;
        s.dir ^= 1;          // [1, 0, 3, 2]
    }
    bool toggle = false, terminal = false;
    float reward = 0.f;
    if (ny < 0) {
        ny = 0;
        s.dir ^= 3;          // [3, 2, 1, 0]
    } else if (env_brick(s.bricks, ny, nx)) {
        toggle = true;
        if (!s.strike) {
            reward = 1.f;
            s.strike = 1;
            s.bricks &= ~(1u << (10 * (ny - 1) + nx));
            ny = s.last_y;
            s.dir ^= 3;
        }
    } else if (ny == 9) {
        if (s.bricks == 0u) s.bricks = ENV_FULL_BRICKS;
        if (bx == s.pos) {
            s.dir ^= 3;
            ny = s.last_y;
        } else if (nx == s.pos) {
            s.dir ^= 2;      // [2, 3, 0, 1]
            ny = s.last_y;
        } else {
            terminal = true;
        }
    }
    if (!toggle) s.strike = 0;
    s.ball_x = nx, s.ball_y = ny;
    s.ep_steps += 1u;
    s.t += 1ull;
    const bool truncated = k.step_limit > 0 && s.ep_steps >= (uint32_t)k.step_limit && !terminal;

    env_store_image(k.next_obs, k.obs_kind, env, lane, s);          // what the step returned, before any reset
    if (terminal || truncated) env_reset(s, side);
    env_store_image(k.obs_next, k.obs_kind, env, lane, s);          // what to act on next
    if (lane == 0) {
        env_store_state(rec, s);
        k.reward[env] = reward;
        k.done[env] = terminal ? 1 : 0;
        k.truncated[env] = truncated ? 1 : 0;
    }
}

static int check_env(const prism_env_desc *d) {
    PRISM_CHECK_ARG(d, "null descriptor");
    PRISM_CHECK_ARG(d->n_envs >= 1 && d->n_envs <= PRISM_ENV_MAX, "n_envs must be in [1, 65536]");
    PRISM_CHECK_ARG(d->n_actions == 3 || d->n_actions == 6, "n_actions must be 3 or 6");
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

static EnvArgs env_args(const prism_env_desc *d, int parity) {
    return EnvArgs{d->n_envs, d->n_actions, d->step_limit, d->obs_kind, d->sticky_p, d->seed, d->state, d->status,
                   d->obs[parity], d->next_obs, d->reward, d->done, d->truncated, nullptr, nullptr, nullptr};
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_breakout_reset(const prism_env_desc *d, const uint8_t *first_side_in, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    EnvArgs k = env_args(d, 0);
    k.side_in = first_side_in;
    hipLaunchKernelGGL(env_breakout_reset_kernel, dim3((d->n_envs + ENV_PER_WG - 1) / ENV_PER_WG), dim3(ENV_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_env_breakout_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *side_in,
                                       int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    EnvArgs k = env_args(d, parity ^ 1);
    k.actions = actions, k.u_in = u_in, k.side_in = side_in;
    hipLaunchKernelGGL(env_breakout_step_kernel, dim3((d->n_envs + ENV_PER_WG - 1) / ENV_PER_WG), dim3(ENV_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
