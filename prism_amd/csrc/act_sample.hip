// Sampled information-directed action selection (IDSActionSelector with random_sample set,
// prism/agents/action_selectors.py:125-176): probs = softmax(-scores).clamp(epsilon, 1), action ~ multinomial(probs).
// The scores are ids_score_wave's (act_kernels.h), the routine ids_score_kernel runs; the draw is a Philox draw of the
// agent's seed.  A translation unit of its own: learner.hip's code object stays what it was.
#define PRISM_ACT_NO_KERNELS
#include "act_kernels.h"

namespace prism {

constexpr uint64_t IDS_SAMPLE_KEY = 0x49445341ull;      // "IDSA": apart from "TAU0" + sid, "PERM", "UNIF"

struct IdsSampleArgs {
    IdsArgs ids;             // (action / action2: the sampled actions)
    const double *u_in;      // optional [n]: the uniforms, in place of the Philox draws (parity)
    uint64_t seed, offset;
    const uint64_t *rng;     // optional device counters: word [2] is the acting count AFTER this call's forward
    float *probs;            // optional [n][A] clamped, not renormalised
};

// One wave per observation, lane = action.  Counter of observation b: c0 + b with c0 = offset (+ rng[2] - n * T: the count
// the forward of this call started from; the word is read, never written).
__global__ __launch_bounds__(ACT_THREADS) void ids_sample_kernel(IdsSampleArgs s) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int A = s.ids.A;
    const float *zb = act_stage(s.ids.z, b, s.ids.T, A, s_act, s.ids.stage != 0);
    if (lane >= 64) return;
    const float score = ids_score_wave(s.ids, zb, b, lane);
    // softmax(-scores) over the A lanes, then clamp(min = epsilon, max = 1)
    const float x = lane < A ? -score : -INFINITY;
    const float m = wave_max(x);
    const float e = lane < A ? expf(x - m) : 0.f;
    const float p = fminf(fmaxf(e / wave_sum(e), s.ids.eps), 1.0f);
    if (lane < A && s.probs) s.probs[(int64_t)b * A + lane] = p;
    // the uniform: 53 bits (the clamp floor lies far below 2^-24)
    double u;
    if (s.u_in) {
        u = s.u_in[b];
    } else {
        uint64_t c0 = s.offset;
        if (s.rng) c0 += s.rng[2] - (uint64_t)s.ids.n * (uint64_t)s.ids.T;
        uint32_t r[4];
        Philox(s.seed)(c0 + (uint64_t)b, IDS_SAMPLE_KEY, r);
        u = u64_to_unit_double(r[0], r[1]);
    }
    // inverse CDF in float64, index order, on wave-uniform values: the weights are not renormalised (torch.multinomial
    // samples proportionally), t = u * S, first a with t < p_0 + ... + p_a; A - 1 when rounding brought t up to S
    double total = 0.0;
    for (int a = 0; a < A; ++a) total += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), a));
    const double t = u * total;
    int pick = A - 1;
    bool open = true;
    double cum = 0.0;
    for (int a = 0; a < A; ++a) {
        cum += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(p), a));
        if (open && t < cum) {
            pick = a;
            open = false;
        }
    }
    if (lane == 0) {
        s.ids.action[b] = pick;
        if (s.ids.action2) s.ids.action2[b] = pick;
    }
}

}  // namespace prism

using namespace prism;

extern "C" int prism_ids_sample_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                                       int32_t n_heads, float lmbda, float epsilon, float rho_lower_bound, int32_t unsquish_fn,
                                       const double *u_in, uint64_t seed, uint64_t offset, const uint64_t *rng_counters,
                                       float *out_scores, float *out_aux, float *out_probs, int64_t *out_action,
                                       int64_t *out_action_host, prism_stream_t stream_) {
    PRISM_CHECK_ARG(z && q && out_scores && out_action, "null buffers");
    PRISM_CHECK_ARG(unsquish_fn >= PRISM_SQUISH_NONE && unsquish_fn <= PRISM_SQUISH_SYMLOG, "unknown unsquish function");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_tau >= 1 && n_actions >= 1 && n_actions <= 16 && n_heads >= 1, "bad sizes");
    const int stage = n_tau * n_actions <= ACT_STAGE_MAX_FLOATS;
    IdsSampleArgs k{{z, q, n, n_pad, n_tau, n_actions, n_heads, lmbda, epsilon, rho_lower_bound, out_scores, out_aux, out_action,
                     out_action_host, stage, unsquish_fn},
                    u_in, seed, offset, rng_counters, out_probs};
    hipLaunchKernelGGL(ids_sample_kernel, dim3(n), dim3(ACT_THREADS), stage ? (size_t)n_tau * n_actions * 4 : 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
