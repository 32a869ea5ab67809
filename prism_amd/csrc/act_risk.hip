// Risk-sensitive acting (config.iqn_risk_policy_id): the quantile samples of one acting forward, passed through a distortion
// beta (Dabney et al. 2018, "Risk-sensitive reinforcement learning") before prism_act_forward embeds them as its tau_in.  The
// reference leaves the policies unimplemented (model_factory.py:10-13 returns None for every id) behind the hook of
// iqn_model.py:73-78.  The raw sample is the acting forward's own draw (fwd_kernels.h, stream id 3); beta runs in float64
// and is narrowed once.  A translation unit of its own: learner.hip's code object stays what it was.
#include "common.h"

namespace prism {

constexpr uint64_t TAU_ACT_KEY = 0x54415530ull + 3ull;      // "TAU0" + stream id 3: prism_act_forward's draws
constexpr int RISK_THREADS = 256;

// rng_counters[2] while a launch runs: the count in bits 0 .. 41 and 62 .. 63 (evaluations count from 2^62), one ticket per
// workgroup in the 20 bits between.  Between launches the ticket bits are zero: the word IS the count.
constexpr int RISK_TICKET_SHIFT = 42;
constexpr uint64_t RISK_TICKET_ONE = 1ull << RISK_TICKET_SHIFT;
constexpr uint64_t RISK_TICKET_MASK = ((1ull << 20) - 1) << RISK_TICKET_SHIFT;
constexpr int64_t RISK_MAX_SAMPLES = (int64_t)RISK_THREADS << 20;

struct RiskArgs {
    int64_t total;                  // n * n_tau
    int policy;
    double eta;
    const float *raw_in;            // optional [total]: the raw samples, in place of the Philox draws
    uint64_t seed, offset;
    unsigned long long *word;       // optional device count of acting draws: added to offset, advanced by total
    float *out, *out_raw;
};

// beta(u) in float64; u in [0, 1].  Every branch maps 0 to 0: Wang through normcdfinv(0) = -inf, normcdf(-inf) = 0.
__device__ __forceinline__ double risk_beta(int policy, double eta, double u) {
    switch (policy) {
    case PRISM_RISK_CVAR:
        return eta * u;
    case PRISM_RISK_WANG:
        return normcdf(normcdfinv(u) + eta);
    case PRISM_RISK_CPW: {
        const double a = pow(u, eta), b = pow(1.0 - u, eta);
        return a / pow(a + b, 1.0 / eta);
    }
    case PRISM_RISK_POW: {
        const double e = 1.0 / (1.0 + fabs(eta));
        return eta >= 0.0 ? pow(u, e) : 1.0 - pow(1.0 - u, e);
    }
    default:
        return u;
    }
}

// One lane per sample.  With the device word: ONE atomic add per workgroup is both its read of the count and its ticket, so
// nobody can read the word after the holder of the last ticket has advanced it, and the word after the call is count + total
// whatever the order of the workgroups (the form of egreedy_select_kernel, act_egreedy.hip).
__global__ __launch_bounds__(RISK_THREADS) void tau_distort_kernel(RiskArgs k) {
    __shared__ unsigned long long s_count;
    uint64_t c0 = k.offset;
    if (k.word) {
        if (threadIdx.x == 0) {
            const uint64_t old = atomicAdd(k.word, (unsigned long long)RISK_TICKET_ONE);
            s_count = old & ~RISK_TICKET_MASK;
            if ((old & RISK_TICKET_MASK) >> RISK_TICKET_SHIFT == (uint64_t)gridDim.x - 1)      // the last ticket: tickets off, total on
                atomicAdd(k.word, (unsigned long long)((uint64_t)k.total - ((uint64_t)gridDim.x << RISK_TICKET_SHIFT)));
        }
        __syncthreads();
        c0 += s_count;
    }
    const int64_t i = (int64_t)blockIdx.x * RISK_THREADS + threadIdx.x;
    if (i >= k.total) return;
    float u;
    if (k.raw_in) {
        u = k.raw_in[i];
    } else {
        uint32_t r[4];
        Philox(k.seed)(c0 + (uint64_t)i, TAU_ACT_KEY, r);
        u = u32_to_unit_float(r[0]);
    }
    k.out[i] = (float)risk_beta(k.policy, k.eta, (double)u);
    if (k.out_raw) k.out_raw[i] = u;
}

}  // namespace prism

using namespace prism;

extern "C" int prism_act_tau_distort(int32_t n, int32_t n_tau, int32_t policy, double eta, const float *tau_raw_in, uint64_t seed,
                                     uint64_t offset, uint64_t *rng_counters, float *out_tau, float *out_tau_raw,
                                     prism_stream_t stream_) {
    PRISM_CHECK_ARG(out_tau, "out_tau is null");
    PRISM_CHECK_ARG(n >= 1 && n_tau >= 1, "bad sizes");
    const int64_t total = (int64_t)n * (int64_t)n_tau;
    PRISM_CHECK_ARG(total < RISK_MAX_SAMPLES, "takes fewer than 2^28 samples a call");
    PRISM_CHECK_ARG(policy >= PRISM_RISK_NEUTRAL && policy <= PRISM_RISK_POW, "unknown policy");
    // (written so that a NaN fails them)
    PRISM_CHECK_ARG(eta - eta == 0.0, "eta is not finite");
    PRISM_CHECK_ARG((policy != PRISM_RISK_CVAR && policy != PRISM_RISK_CPW) || (eta > 0.0 && eta <= 1.0), "eta outside (0, 1]");
    RiskArgs k{total, policy, eta, tau_raw_in, seed, offset,
               tau_raw_in ? nullptr : reinterpret_cast<unsigned long long *>(rng_counters ? rng_counters + 2 : nullptr), out_tau,
               out_tau_raw};
    hipLaunchKernelGGL(tau_distort_kernel, dim3((unsigned)((total + RISK_THREADS - 1) / RISK_THREADS)), dim3(RISK_THREADS), 0,
                       (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
