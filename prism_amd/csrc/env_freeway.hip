// MinAtar Freeway (10 x 10 x 7 observations, 6 or 3 actions) for N lock-stepped environments: one launch per step, no host
// value that changes between steps (the counters live in the state records), nothing read back.  The rules are the table of
// DESIGN.md 7.4 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own, as
// env_breakout.hip is: learner.hip's code object stays what it was.
//
// One wave per environment, four environments per workgroup.  The game is wave-uniform: every lane computes it from the
// environment's 32-byte state record (one broadcast load, scalar registers after readfirstlane), lane 0 writes the new
// record.  The eight cars stay PACKED in three words (x, timer + direction, |speed|) and every access is a constant shift of
// an unrolled loop -- an array indexed by a lane's row would go to the private segment.  A cell is 7 values, which is no
// store unit in either kind, so the image is written as 175 flat chunks of four consecutive HWC elements: one 16-byte store
// in fp32, one 32-bit word in bytes (an environment's byte image is 700 bytes: 4-byte aligned only).  The 17 set elements
// are placed from the state's side (scalar index arithmetic, one compare per lane and element); a step whose episode goes
// on builds one image and stores it twice.  No LDS, no private segment.
#include "common.h"

namespace prism {

// stream keys, apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD", "ENVB" and from each other
constexpr uint64_t FW_KEY_COIN = 0x46575943ull;                                   // "FWYC": the sticky coin
constexpr uint64_t FW_KEY_WIN0 = 0x46575730ull, FW_KEY_WIN1 = 0x46575731ull;      // "FWW0", "FWW1": win speeds of cars 0-3, 4-7
constexpr uint64_t FW_KEY_RST0 = 0x46575230ull, FW_KEY_RST1 = 0x46575231ull;      // "FWR0", "FWR1": reset speeds
constexpr int FW_THREADS = 256, FW_PER_WG = FW_THREADS / WAVE, FW_CARS = 8, FW_CHANNELS = 7;
constexpr int FW_ELEMS = 100 * FW_CHANNELS, FW_CHUNKS = FW_ELEMS / 4;             // 700 elements = 175 chunks of four
constexpr int FW_MOVE_TIME = 3, FW_EPISODE_TIME = 2500;
static_assert(FW_ELEMS % 4 == 0 && FW_CHUNKS <= 3 * WAVE, "lane l takes chunks l, l + 64, l + 128");

// The state record: PRISM_ENV_STATE_WORDS uint32 (include/prism_hip.h has the field map)
//   [0] x of car i in bits 4i..4i+3   [1] timer of car i in bits 3i..3i+2, direction of car i (1: +x) in bit 24 + i
//   [2] ep_steps   [3] |speed| of car i in bits 3i..3i+2   [4] t low   [5] t high   [6] packed small fields   [7] 0
struct FwState {
    uint32_t xs, timers, mags;          // timers holds the direction bits too
    int pos, move_timer, terminate_timer, last_action;
    uint32_t ep_steps;
    uint64_t t;
};
__host__ __device__ inline uint32_t fw_pack(const FwState &s) {
    return (uint32_t)s.pos | ((uint32_t)s.move_timer << 4) | ((uint32_t)s.terminate_timer << 6) | ((uint32_t)s.last_action << 18);
}
__host__ __device__ inline void fw_unpack(uint32_t w, FwState &s) {
    s.pos = w & 15, s.move_timer = (w >> 4) & 3, s.terminate_timer = (w >> 6) & 4095, s.last_action = (w >> 18) & 7;
}
// A set of eight speeds as (|speed| in 3-bit fields, direction bits 24..31): what words [3] and [1] hold of them
struct FwSpeeds {
    uint32_t mags, dirs;
};
// every car takes the set's speed and timer = |speed|; x stays
__host__ __device__ inline void fw_install_speeds(FwState &s, const FwSpeeds &v) {
    s.mags = v.mags;
    s.timers = v.mags | v.dirs;
}
// "Reset with speeds": last_action and t carry over
__host__ __device__ inline void fw_reset(FwState &s, const FwSpeeds &v) {
    s.xs = 0u;
    fw_install_speeds(s, v);
    s.pos = 9;
    s.move_timer = FW_MOVE_TIME;
    s.terminate_timer = FW_EPISODE_TIME;
    s.ep_steps = 0;
}

struct FwArgs {
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
    const int8_t *speeds_in;
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// word w -> one car: |speed| = 1 + floor(5 (w >> 1) / 2^31) in 1..5, direction + if w & 1
__device__ __forceinline__ void fw_add_car(FwSpeeds &v, int i, uint32_t mag, uint32_t plus) {
    v.mags |= mag << (3 * i);
    v.dirs |= plus << (24 + i);
}
// the eight speeds of one set: two Philox calls at `counter`, one word per car
__device__ __forceinline__ FwSpeeds fw_draw_speeds(uint64_t seed, uint64_t counter, int env, uint64_t key0, uint64_t key1) {
    FwSpeeds v{0u, 0u};
    const Philox ph(seed);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        uint32_t r[4];
        ph(counter, ((uint64_t)env << 32) | (h ? key1 : key0), r);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = uni(r[j]);
            fw_add_car(v, 4 * h + j, 1u + (uint32_t)(((uint64_t)(w >> 1) * 5ull) >> 31), w & 1u);
        }
    }
    return v;
}
// the parity path: eight signed bytes, +-1 .. +-5
__device__ __forceinline__ FwSpeeds fw_given_speeds(const int8_t *speeds_in, int env) {
    FwSpeeds v{0u, 0u};
#pragma unroll
    for (int i = 0; i < FW_CARS; ++i) {
        const int sp = (int)uni((uint32_t)(int)speeds_in[(size_t)env * FW_CARS + i]);
        fw_add_car(v, i, (uint32_t)(sp < 0 ? -sp : sp) & 7u, sp > 0 ? 1u : 0u);
    }
    return v;
}

// An image as a lane holds it: chunk lane + 64 k in w[k] (named, never indexed by a run-time value), in the byte kind's form --
// element 4 j + q of the HWC image is byte q of chunk j, 0 or 1.
struct FwImage {
    uint32_t w0, w1, w2;
};
// Set element e = 7 (10 y + x) + channel.  e is wave-uniform: its chunk, the word that chunk lives in and the byte are
// scalar work; a lane pays one compare and three select-ORs.  An image has 17 set elements and 683 clear ones, so it is built
// from the state's side (17 of these) and not decoded per element (700 divisions by 7 and by 10).
__device__ __forceinline__ void fw_set(FwImage &img, int lane, int e) {
    const int chunk = e >> 2, k = chunk >> 6;
    const uint32_t bit = 1u << (8 * (e & 3));
    const bool mine = lane == (chunk & 63);
    img.w0 |= mine ? (k == 0 ? bit : 0u) : 0u;
    img.w1 |= mine ? (k == 1 ? bit : 0u) : 0u;
    img.w2 |= mine ? (k == 2 ? bit : 0u) : 0u;
}
// Channel 0 at (pos, 4); per car of row y = i + 1, channel 1 at (y, x) and channel 1 + |speed| at its trail cell.  The cars
// come out of the packed words by constant shifts (the loop is unrolled).
__device__ __forceinline__ FwImage fw_image(const FwState &s, int lane) {
    FwImage img{0u, 0u, 0u};
    fw_set(img, lane, FW_CHANNELS * (10 * s.pos + 4));
#pragma unroll
    for (int i = 0; i < FW_CARS; ++i) {
        const int cx = (int)((s.xs >> (4 * i)) & 15u), mag = (int)((s.mags >> (3 * i)) & 7u);
        const bool plus = (s.timers >> (24 + i)) & 1u;
        const int back = plus ? (cx == 0 ? 9 : cx - 1) : (cx == 9 ? 0 : cx + 1);
        fw_set(img, lane, FW_CHANNELS * (10 * (i + 1) + cx) + 1);
        fw_set(img, lane, FW_CHANNELS * (10 * (i + 1) + back) + 1 + mag);
    }
    return img;
}
__device__ __forceinline__ void fw_store_chunk(void *base, int obs_kind, size_t at, uint32_t w) {
    if (obs_kind == PRISM_OBS_U8) {
        __builtin_nontemporal_store(w, reinterpret_cast<uint32_t *>(base) + at);
    } else {
        stream_store4(reinterpret_cast<float4 *>(base) + at,
                      make_float4((float)(w & 1u), (float)((w >> 8) & 1u), (float)((w >> 16) & 1u), (float)(w >> 24)));
    }
}
// One image of environment `env`: lane l writes chunks l, l + 64, l + 128 (< 175) of four consecutive elements.  Streaming
// stores: the next launch reads them.
__device__ __forceinline__ void fw_store_image(void *base, int obs_kind, int env, int lane, const FwImage &img) {
    const size_t at = (size_t)env * FW_CHUNKS + lane;
    fw_store_chunk(base, obs_kind, at, img.w0);
    fw_store_chunk(base, obs_kind, at + 64, img.w1);
    if (lane + 128 < FW_CHUNKS) fw_store_chunk(base, obs_kind, at + 128, img.w2);
}
__device__ __forceinline__ void fw_store_state(uint32_t *rec, const FwState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.xs, s.timers, s.ep_steps, s.mags);
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), fw_pack(s), 0u);
}

__global__ __launch_bounds__(FW_THREADS) void env_freeway_reset_kernel(FwArgs k) {
    const int env = (int)uni(blockIdx.x * FW_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    const FwSpeeds first = k.speeds_in ? fw_given_speeds(k.speeds_in, env) : fw_draw_speeds(k.seed, ~0ull, env, FW_KEY_RST0, FW_KEY_RST1);
    FwState s;
    s.last_action = 0;
    s.t = 0;
    fw_reset(s, first);
    fw_store_image(k.obs_next, k.obs_kind, env, lane, fw_image(s, lane));
    if (lane == 0) fw_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(FW_THREADS) void env_freeway_step_kernel(FwArgs k) {
    const int env = (int)uni(blockIdx.x * FW_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (env >= k.n_envs) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 w1 = reinterpret_cast<const uint4 *>(rec)[1];
    FwState s;
    s.xs = uni(w0.x), s.timers = uni(w0.y), s.ep_steps = uni(w0.z), s.mags = uni(w0.w);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);
    fw_unpack(uni(w1.z), s);
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
        Philox(k.seed)(t0, ((uint64_t)env << 32) | FW_KEY_COIN, r);
        u = u64_to_unit_double(uni(r[0]), uni(r[1]));
    }

    // the action: out of range acts as no-op and raises the sticky status bit; the 3-action set is n, u, d
    const bool valid = raw_hi == 0u && raw_lo < (uint32_t)k.n_actions;
    int a = valid ? (int)raw_lo : 0;
    if (k.n_actions == 3) a *= 2;
    if (!valid && lane == 0) atomicOr(k.status, (uint32_t)PRISM_ENV_STATUS_BAD_ACTION);
    if (u < k.sticky_p) a = s.last_action;
    s.last_action = a;

    // the chicken
    if (a == 2 && s.move_timer == 0) {
        s.move_timer = FW_MOVE_TIME;
        s.pos = max(0, s.pos - 1);
    } else if (a == 4 && s.move_timer == 0) {
        s.move_timer = FW_MOVE_TIME;
        s.pos = min(9, s.pos + 1);
    }
    // a win: new speeds for every car (drawn on such a step only; the branch is wave-uniform)
    float reward = 0.f;
    if (s.pos == 0) {
        reward = 1.f;
        fw_install_speeds(s, k.speeds_in ? fw_given_speeds(k.speeds_in, env) : fw_draw_speeds(k.seed, t0, env, FW_KEY_WIN0, FW_KEY_WIN1));
        s.pos = 9;
    }
    // the cars, in order; car i is on row i + 1
#pragma unroll
    for (int i = 0; i < FW_CARS; ++i) {
        int cx = (int)((s.xs >> (4 * i)) & 15u);
        const int timer = (int)((s.timers >> (3 * i)) & 7u), mag = (int)((s.mags >> (3 * i)) & 7u);
        const bool plus = (s.timers >> (24 + i)) & 1u;
        if (cx == 4 && s.pos == i + 1) s.pos = 9;
        int new_timer;
        if (timer == 0) {
            new_timer = mag;
            cx = plus ? (cx == 9 ? 0 : cx + 1) : (cx == 0 ? 9 : cx - 1);
            if (cx == 4 && s.pos == i + 1) s.pos = 9;
        } else {
            new_timer = timer - 1;
        }
        s.xs = (s.xs & ~(15u << (4 * i))) | ((uint32_t)cx << (4 * i));
        s.timers = (s.timers & ~(7u << (3 * i))) | ((uint32_t)new_timer << (3 * i));
    }
    // the timers
    s.move_timer -= s.move_timer > 0;
    s.terminate_timer -= 1;
    const bool terminal = s.terminate_timer < 0;
    if (terminal) s.terminate_timer = 0;
    s.ep_steps += 1u;
    s.t += 1ull;
    const bool truncated = k.step_limit > 0 && s.ep_steps >= (uint32_t)k.step_limit && !terminal;

    FwImage img = fw_image(s, lane);
    fw_store_image(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                     // (wave-uniform) only then is the acting image another one
        fw_reset(s, k.speeds_in ? fw_given_speeds(k.speeds_in, env) : fw_draw_speeds(k.seed, t0, env, FW_KEY_RST0, FW_KEY_RST1));
        img = fw_image(s, lane);
    }
    fw_store_image(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    if (lane == 0) {
        fw_store_state(rec, s);
        k.reward[env] = reward;
        k.done[env] = terminal ? 1 : 0;
        k.truncated[env] = truncated ? 1 : 0;
    }
}

// the checks and texts of env_breakout.hip's check_env: one descriptor, one contract
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

static FwArgs fw_args(const prism_env_desc *d, int parity) {
    return FwArgs{d->n_envs, d->n_actions, d->step_limit, d->obs_kind, d->sticky_p, d->seed, d->state, d->status,
                  d->obs[parity], d->next_obs, d->reward, d->done, d->truncated, nullptr, nullptr, nullptr};
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_freeway_reset(const prism_env_desc *d, const int8_t *first_speeds_in, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    FwArgs k = fw_args(d, 0);
    k.speeds_in = first_speeds_in;
    hipLaunchKernelGGL(env_freeway_reset_kernel, dim3((d->n_envs + FW_PER_WG - 1) / FW_PER_WG), dim3(FW_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_env_freeway_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const int8_t *speeds_in,
                                      int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d);
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    FwArgs k = fw_args(d, parity ^ 1);
    k.actions = actions, k.u_in = u_in, k.speeds_in = speeds_in;
    hipLaunchKernelGGL(env_freeway_step_kernel, dim3((d->n_envs + FW_PER_WG - 1) / FW_PER_WG), dim3(FW_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
