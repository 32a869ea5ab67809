// The two action selectors that read the ensemble estimates alone: MinRegretActionSelector
// (prism/agents/action_selectors.py:85-111) and SimpleIDSActionSelector (:195-286, its per-head reading: q_estimates a
// sequence over heads of [n, A] estimates).  Both read Q [heads][n_pad][A] as the forward tiles leave it (fwd_kernels.h,
// kind 1) and nothing else: no LDS, one wave per observation, lane = action, ACT_THREADS / 64 observations a workgroup, one round of loads.
// The ensemble mean and spread are ids_score_wave's (act_kernels.h), restated operation for operation: the same bits.  A
// translation unit of its own: learner.hip's code object stays what it was.
#define PRISM_ACT_NO_KERNELS
#include "act_kernels.h"

namespace prism {

constexpr int ENS_ROWS = ACT_THREADS / 64;       // observations per workgroup: one per wave
constexpr int ENS_MAX_HEADS = 16;

struct EnsembleArgs {
    const float *q;          // [heads][n_pad][A]; rows n .. n_pad - 1 are never read
    int n, n_pad, A, heads;
    float c0, c1;            // MinRegret: lmbda, -; SimpleIDS: (float)(1 - beta) formed in double, (float)beta
    int unsquish;            // PRISM_SQUISH_*: applied to every estimate as it is read
    float *scores;           // optional [n][A]
    float *aux;              // optional [n][2][A] (MinRegret) / [n][3][A] (SimpleIDS)
    int64_t *action;         // [n]
    int64_t *action2;        // optional second copy of the actions (pinned host memory)
};

// The heads' estimates of action `lane` of observation b, unsquished, into registers: ONE round of loads, issued together
// (ids_score_wave walks the heads twice and unsquishes inside the walk; the values and what is done with them are the same).
__device__ __forceinline__ void ens_load(const EnsembleArgs &k, int b, int lane, float (&x)[ENS_MAX_HEADS]) {
#pragma unroll
    for (int h = 0; h < ENS_MAX_HEADS; ++h) x[h] = h < k.heads ? k.q[((int64_t)h * k.n_pad + b) * k.A + lane] : 0.f;
#pragma unroll
    for (int h = 0; h < ENS_MAX_HEADS; ++h)
        if (h < k.heads) x[h] = unsquish_value(k.unsquish, x[h]);
}

__device__ __forceinline__ float lane_value(float v, int a) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), a));
}

__device__ __forceinline__ void ens_store_action(const EnsembleArgs &k, int b, int lane, int best) {
    if (lane == 0) {
        k.action[b] = best;
        if (k.action2) k.action2[b] = best;
    }
}

// regret^2 of every action, first minimum wins (torch.argmin)
__global__ __launch_bounds__(ACT_THREADS) void min_regret_select_kernel(EnsembleArgs k) {
    const int b = blockIdx.x * ENS_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= k.n) return;          // (a whole wave)
    const int A = k.A, Hd = k.heads;
    float mean = 0.f, spread = 0.f;
    if (lane < A) {
        float x[ENS_MAX_HEADS];
        ens_load(k, b, lane, x);
        float s = 0.f;
#pragma unroll
        for (int h = 0; h < ENS_MAX_HEADS; ++h)
            if (h < Hd) s += x[h];
        mean = s / (float)Hd;
        float v = 0.f;
#pragma unroll
        for (int h = 0; h < ENS_MAX_HEADS; ++h)
            if (h < Hd) {
                const float d = x[h] - mean;
                v += d * d;
            }
        spread = sqrtf(v / (float)(Hd - 1));                        // q_estimates.std(dim=-1): called "variance" there
    }
    const float sd = sqrtf(spread);                                 // torch.sqrt(variance)
    const float hi = lane < A ? mean + k.c0 * sd : -INFINITY;
    const float upper = wave_max(hi);
    const float regret = upper - (mean - k.c0 * sd);
    const float regret_sq = regret * regret;
    if (lane < A) {
        if (k.scores) k.scores[(int64_t)b * A + lane] = regret_sq;
        if (k.aux) {
            float *o = k.aux + (int64_t)b * 2 * A;
            o[lane] = mean;
            o[A + lane] = spread;
        }
    }
    int best = 0;
    float bv = lane_value(regret_sq, 0);
    for (int a = 1; a < A; ++a) {
        const float v = lane_value(regret_sq, a);
        if (v < bv) {
            bv = v;
            best = a;
        }
    }
    ens_store_action(k, b, lane, best);
}

// (1 - beta) max_diff + beta (mean - mean over the actions), first maximum wins (torch.argmax)
__global__ __launch_bounds__(ACT_THREADS) void simple_ids_select_kernel(EnsembleArgs k) {
    const int b = blockIdx.x * ENS_ROWS + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= k.n) return;          // (a whole wave)
    const int A = k.A, Hd = k.heads;
    float mean = 0.f, max_diff = 0.f;
    if (lane < A) {
        float x[ENS_MAX_HEADS];
        ens_load(k, b, lane, x);
        float s = 0.f, lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int h = 0; h < ENS_MAX_HEADS; ++h)
            if (h < Hd) {
                s += x[h];                                          // mean += q_estimates[i], in head order
                lo = fminf(lo, x[h]);
                hi = fmaxf(hi, x[h]);
            }
        mean = s / (float)Hd;
        max_diff = hi - lo;                                         // max over pairs of |q_i - q_j|: rounding is monotone
    }
    float total = 0.f;                                              // mean.mean(dim=-1), in action order
    for (int a = 0; a < A; ++a) total += lane_value(mean, a);
    const float q_value = mean - total / (float)A;
    const float scaled = k.c0 * max_diff + q_value * k.c1;
    if (lane < A) {
        if (k.scores) k.scores[(int64_t)b * A + lane] = scaled;
        if (k.aux) {
            float *o = k.aux + (int64_t)b * 3 * A;
            o[lane] = mean;
            o[A + lane] = max_diff;
            o[2 * A + lane] = q_value;
        }
    }
    int best = 0;
    float bv = lane_value(scaled, 0);
    for (int a = 1; a < A; ++a) {
        const float v = lane_value(scaled, a);
        if (v > bv) {
            bv = v;
            best = a;
        }
    }
    ens_store_action(k, b, lane, best);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_min_regret_select(const float *q, int32_t n, int32_t n_pad, int32_t n_actions, int32_t n_heads,
                                       float lmbda, int32_t unsquish_fn, float *out_scores, float *out_aux,
                                       int64_t *out_action, int64_t *out_action_host, prism_stream_t stream_) {
    PRISM_CHECK_ARG(q && out_action, "null buffers");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_actions >= 1 && n_actions <= 16, "bad sizes");
    PRISM_CHECK_ARG(n_heads >= 2 && n_heads <= ENS_MAX_HEADS, "n_heads must be in [2, 16] (one head has no spread)");
    PRISM_CHECK_ARG(unsquish_fn >= PRISM_SQUISH_NONE && unsquish_fn <= PRISM_SQUISH_SYMLOG, "unknown unsquish function");
    PRISM_CHECK_ARG(lmbda == lmbda, "lmbda is NaN");
    EnsembleArgs k{q, n, n_pad, n_actions, n_heads, lmbda, 0.f, unsquish_fn, out_scores, out_aux, out_action, out_action_host};
    hipLaunchKernelGGL(min_regret_select_kernel, dim3((n + ENS_ROWS - 1) / ENS_ROWS), dim3(ACT_THREADS), 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_simple_ids_select(const float *q, int32_t n, int32_t n_pad, int32_t n_actions, int32_t n_heads,
                                       double beta, int32_t unsquish_fn, float *out_scores, float *out_aux,
                                       int64_t *out_action, int64_t *out_action_host, prism_stream_t stream_) {
    PRISM_CHECK_ARG(q && out_action, "null buffers");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_actions >= 1 && n_actions <= 16, "bad sizes");
    PRISM_CHECK_ARG(n_heads >= 1 && n_heads <= ENS_MAX_HEADS, "n_heads must be in [1, 16]");
    PRISM_CHECK_ARG(unsquish_fn >= PRISM_SQUISH_NONE && unsquish_fn <= PRISM_SQUISH_SYMLOG, "unknown unsquish function");
    PRISM_CHECK_ARG(beta == beta, "beta is NaN");
    EnsembleArgs k{q, n, n_pad, n_actions, n_heads, (float)(1.0 - beta), (float)beta, unsquish_fn, out_scores, out_aux,
                   out_action, out_action_host};
    hipLaunchKernelGGL(simple_ids_select_kernel, dim3((n + ENS_ROWS - 1) / ENS_ROWS), dim3(ACT_THREADS), 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
