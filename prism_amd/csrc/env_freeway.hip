// MinAtar Freeway (10 x 10 x 7 observations, 6 or 3 actions) on the games' shared frame (env_frame.h).  The rules are the table
// of DESIGN.md 7.4 -- a restatement of MinAtar v1, NOT checked against the `minatar` package.  A translation unit of its own:
// learner.hip's code object stays what it was.
//
// The 32-byte state record comes in through one broadcast load, lane 0 writes the new one.  The eight cars stay PACKED in three
// words (x, timer + direction, |speed|) and every access is a constant shift of an unrolled loop -- an array indexed by a
// lane's row would go to the private segment.  A cell is 7 values, which is no store unit in either kind, so the image is 175
// flat chunks (an environment's byte image is 700 bytes: 4-byte aligned only).  The 17 set elements are placed from the
// state's side (scalar index arithmetic, one compare per lane and element); a step whose episode goes on builds one image and
// stores it twice.  No LDS, no private segment.
#include "env_frame.h"

namespace prism {

// stream keys, apart from "TAU0" + sid, "PERM", "UNIF", "IDSA", "EGRD", "ENVB" and from each other
constexpr uint64_t FW_KEY_COIN = 0x46575943ull;                                   // "FWYC": the sticky coin
constexpr uint64_t FW_KEY_WIN0 = 0x46575730ull, FW_KEY_WIN1 = 0x46575731ull;      // "FWW0", "FWW1": win speeds of cars 0-3, 4-7
constexpr uint64_t FW_KEY_RST0 = 0x46575230ull, FW_KEY_RST1 = 0x46575231ull;      // "FWR0", "FWR1": reset speeds
constexpr int FW_CARS = 8, FW_CHANNELS = 7;
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

// An image as a lane holds it: the four elements of chunk lane + 64 j in bits 4j .. 4j+3 (element 4 c + q of the HWC image is
// bit q of chunk c).
// Set element e = 7 (10 y + x) + channel.  e is wave-uniform: its chunk, that chunk's lane and the bit are scalar work; a lane
// pays one compare and one select-OR.  An image has 17 set elements and 683 clear ones, so it is built from the state's side
// (17 of these) and not decoded per element (700 divisions by 7 and by 10).
__device__ __forceinline__ void fw_set(uint32_t &img, int lane, int e) {
    const int chunk = e >> 2;
    img |= lane == (chunk & 63) ? 1u << (4 * (chunk >> 6) + (e & 3)) : 0u;
}
// Channel 0 at (pos, 4); per car of row y = i + 1, channel 1 at (y, x) and channel 1 + |speed| at its trail cell.  The cars
// come out of the packed words by constant shifts (the loop is unrolled).
__device__ __forceinline__ uint32_t fw_image(const FwState &s, int lane) {
    uint32_t img = 0u;
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
__device__ __forceinline__ void fw_store_state(uint32_t *rec, const FwState &s) {
    uint4 *p = reinterpret_cast<uint4 *>(rec);
    p[0] = make_uint4(s.xs, s.timers, s.ep_steps, s.mags);
    p[1] = make_uint4((uint32_t)s.t, (uint32_t)(s.t >> 32), fw_pack(s), 0u);
}

// this launch's set of speeds under `key0`, `key1`: the given one on the parity path
__device__ __forceinline__ FwSpeeds fw_speeds(const EnvArgs &k, uint64_t counter, int env, uint64_t key0, uint64_t key1) {
    const int8_t *speeds_in = static_cast<const int8_t *>(k.draws_in);
    return speeds_in ? fw_given_speeds(speeds_in, env) : fw_draw_speeds(k.seed, counter, env, key0, key1);
}

__global__ __launch_bounds__(ENV_THREADS) void env_freeway_reset_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    FwState s;
    s.last_action = 0;
    s.t = 0;
    fw_reset(s, fw_speeds(k, ~0ull, env, FW_KEY_RST0, FW_KEY_RST1));
    env_store_image<FW_CHUNKS>(k.obs_next, k.obs_kind, env, lane, fw_image(s, lane));
    if (lane == 0) fw_store_state(k.state + (size_t)env * PRISM_ENV_STATE_WORDS, s);
}

__global__ __launch_bounds__(ENV_THREADS) void env_freeway_step_kernel(EnvArgs k) {
    int env, lane;
    if (!env_of_wave(k, env, lane)) return;
    uint32_t *rec = k.state + (size_t)env * PRISM_ENV_STATE_WORDS;
    const uint4 w0 = reinterpret_cast<const uint4 *>(rec)[0];
    const uint4 w1 = reinterpret_cast<const uint4 *>(rec)[1];
    FwState s;
    s.xs = uni(w0.x), s.timers = uni(w0.y), s.ep_steps = uni(w0.z), s.mags = uni(w0.w);
    s.t = (uint64_t)uni(w1.x) | ((uint64_t)uni(w1.y) << 32);
    fw_unpack(uni(w1.z), s);
    const uint64_t t0 = s.t;          // the counter of this step's draws

    // (the action's load is in flight while the coin is drawn)
    int a = env_action(k.actions, env, k.n_actions, k.status, lane);
    const double u = env_coin(k.u_in, k.seed, t0, env, FW_KEY_COIN);
    // the 3-action set is n, u, d
    if (k.n_actions == 3) a *= 2;
    a = env_sticky(a, u, k.sticky_p, s.last_action);

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
        fw_install_speeds(s, fw_speeds(k, t0, env, FW_KEY_WIN0, FW_KEY_WIN1));
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
    const bool truncated = env_count_step(s.ep_steps, s.t, k.step_limit, terminal);

    uint32_t img = fw_image(s, lane);
    env_store_image<FW_CHUNKS>(k.next_obs, k.obs_kind, env, lane, img);          // what the step returned, before any reset
    if (terminal || truncated) {                                                 // (wave-uniform) only then is the acting image another one
        fw_reset(s, fw_speeds(k, t0, env, FW_KEY_RST0, FW_KEY_RST1));
        img = fw_image(s, lane);
    }
    env_store_image<FW_CHUNKS>(k.obs_next, k.obs_kind, env, lane, img);          // what to act on next
    if (lane == 0) fw_store_state(rec, s);
    env_store_outcome(k, env, lane, reward, terminal, truncated);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_env_freeway_reset(const prism_env_desc *d, const int8_t *first_speeds_in, prism_stream_t stream_) {
    const int rc = check_env(d, 3, "n_actions must be 3 or 6");
    if (rc != PRISM_OK) return rc;
    return env_launch(env_freeway_reset_kernel, env_args(d, 0, nullptr, nullptr, first_speeds_in), stream_);
}

extern "C" int prism_env_freeway_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const int8_t *speeds_in,
                                      int32_t parity, prism_stream_t stream_) {
    const int rc = check_env(d, 3, "n_actions must be 3 or 6");
    if (rc != PRISM_OK) return rc;
    PRISM_CHECK_ARG(actions, "actions is null");
    PRISM_CHECK_ARG(parity == 0 || parity == 1, "parity must be 0 or 1");
    return env_launch(env_freeway_step_kernel, env_args(d, parity ^ 1, actions, u_in, speeds_in), stream_);
}
