// What the on-device games share: the launch arguments, the wave-to-environment map, the sticky coin, the
// action check, the image store, the step's counters and outcome store, and on the host the descriptor check, the argument
// builder and the launch.  Helpers, not a framework: every game keeps its own two kernels (env_<game>_reset_kernel,
// env_<game>_step_kernel), whose bodies read: load the record, prologue from here, the game's rules, epilogue from here.
//
// One wave per environment, ENV_PER_WG environments per workgroup, one launch per step, no host value that changes between
// steps (the counters live in the state records), nothing read back.  The game is wave-uniform: what every lane computes
// from the record goes through uni() and lives in scalar registers.  An observation is written as chunks of four consecutive
// HWC elements, one 16-byte store in fp32 and one 32-bit word in bytes: lane l owns chunks l, l + 64, ... and holds them as one
// nibble each.  Streaming stores: the next launch reads them.
//
// Stream keys stay in the game files (each literal once in csrc/); the frame takes the key as an argument.  Device builtins
// stand inside __device__ functions only: tools/invaders_host_check.hip compiles a game file's host-and-device code for the CPU.
#pragma once
#include "common.h"

namespace prism {

constexpr int ENV_THREADS = 256, ENV_PER_WG = ENV_THREADS / WAVE;

struct EnvArgs {
    int n_envs, n_actions, step_limit, obs_kind;
    double sticky_p;
    uint64_t seed;
    uint32_t *state, *status;
    void *obs_next;               // the ping-pong buffer this launch writes the acting image into
    void *next_obs;               // step only
    float *reward;
    uint8_t *done, *truncated;
    const int64_t *actions;
    const double *u_in;           // parity path: the sticky coins, or null
    const void *draws_in;         // parity path: the game's other draws in the game's own layout, or null
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }

// The wave's environment and the lane's place in the wave; false where the last workgroup has no environment for this wave.
__device__ __forceinline__ bool env_of_wave(const EnvArgs &k, int &env, int &lane) {
    env = (int)uni(blockIdx.x * ENV_PER_WG + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    return env < k.n_envs;
}

// a coin the parity path gives
__device__ __forceinline__ double env_given_coin(const double *u_in, int env) {
    return __builtin_bit_cast(double, uni64(__builtin_bit_cast(uint64_t, u_in[env])));
}
// The sticky coin of step t: the given one, or words 0, 1 of Philox(seed)(t, env << 32 | key) as a double in [0, 1).
__device__ __forceinline__ double env_coin(const double *u_in, uint64_t seed, uint64_t t, int env, uint64_t key) {
    if (u_in) return env_given_coin(u_in, env);
    uint32_t r[4];
    const Philox ph(seed);
    ph(t, ((uint64_t)env << 32) | key, r);
    return u64_to_unit_double(uni(r[0]), uni(r[1]));
}

// The agent's action: one out of [0, n_actions) acts as no-op and raises the sticky status bit.  (The minimal set's map to the
// game's actions is the game's.)
__device__ __forceinline__ int env_action(const int64_t *actions, int env, int n_actions, uint32_t *status, int lane) {
    const uint64_t raw = uni64((uint64_t)actions[env]);
    const bool valid = raw < (uint64_t)(uint32_t)n_actions;
    if (!valid && lane == 0) atomicOr(status, (uint32_t)PRISM_ENV_STATUS_BAD_ACTION);
    return valid ? (int)raw : 0;
}
// the sticky select: under the coin the last action again; what is taken is the next step's last action
__device__ __forceinline__ int env_sticky(int a, double u, double sticky_p, int &last_action) {
    return last_action = u < sticky_p ? last_action : a;
}

// four consecutive elements, element j in bit j of b (b < 16)
__device__ __forceinline__ void env_store_chunk(void *base, int obs_kind, size_t at, uint32_t b) {
    if (obs_kind == PRISM_OBS_U8) {
        const uint32_t w = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);      // element j in byte j
        __builtin_nontemporal_store(w, reinterpret_cast<uint32_t *>(base) + at);
    } else {
        stream_store4(reinterpret_cast<float4 *>(base) + at,
                      make_float4((float)(b & 1u), (float)((b >> 1) & 1u), (float)((b >> 2) & 1u), (float)(b >> 3)));
    }
}
// One image of CHUNKS chunks for environment `env`: chunk lane + 64 j is bits 4j .. 4j+3 of img.  Only the last stride is guarded.
template <int CHUNKS>
__device__ __forceinline__ void env_store_image(void *base, int obs_kind, int env, int lane, uint32_t img) {
    static_assert(CHUNKS <= 8 * WAVE, "a nibble per stride of 64 chunks");
    const size_t at = (size_t)env * CHUNKS + lane;
#pragma unroll
    for (int j = 0; 64 * j < CHUNKS; ++j)
        if (64 * (j + 1) <= CHUNKS || lane + 64 * j < CHUNKS) env_store_chunk(base, obs_kind, at + 64 * j, (img >> (4 * j)) & 15u);
}

// The counters of a step that was taken; whether the step limit ends the episode here (a terminal step is not truncated).
__device__ __forceinline__ bool env_count_step(uint32_t &ep_steps, uint64_t &t, int step_limit, bool terminal) {
    ep_steps += 1u;
    t += 1ull;
    return step_limit > 0 && ep_steps >= (uint32_t)step_limit && !terminal;
}
__device__ __forceinline__ void env_store_outcome(const EnvArgs &k, int env, int lane, float reward, bool terminal, bool truncated) {
    if (lane == 0) {
        k.reward[env] = reward;
        k.done[env] = terminal ? 1 : 0;
        k.truncated[env] = truncated ? 1 : 0;
    }
}

// ---- host side ----
// One descriptor, one contract; a game accepts its minimal action count or 6 and says so in `actions_text`.
static int check_env(const prism_env_desc *d, int minimal_actions, const char *actions_text) {
    PRISM_CHECK_ARG(d, "null descriptor");
    PRISM_CHECK_ARG(d->n_envs >= 1 && d->n_envs <= PRISM_ENV_MAX, "n_envs must be in [1, 65536]");
    PRISM_CHECK_ARG(d->n_actions == minimal_actions || d->n_actions == 6, actions_text);
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

// `parity`: which of the two ping-pong buffers takes the acting image
static EnvArgs env_args(const prism_env_desc *d, int parity, const int64_t *actions = nullptr, const double *u_in = nullptr,
                        const void *draws_in = nullptr) {
    return EnvArgs{d->n_envs, d->n_actions, d->step_limit, d->obs_kind, d->sticky_p, d->seed, d->state, d->status,
                   d->obs[parity], d->next_obs, d->reward, d->done, d->truncated, actions, u_in, draws_in};
}

static int env_launch(void (*kernel)(EnvArgs), const EnvArgs &k, prism_stream_t stream) {
    hipLaunchKernelGGL(kernel, dim3((k.n_envs + ENV_PER_WG - 1) / ENV_PER_WG), dim3(ENV_THREADS), 0, (hipStream_t)stream, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

}  // namespace prism
