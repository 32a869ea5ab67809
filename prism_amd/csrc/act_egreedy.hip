// Per-observation epsilon-greedy action selection: EGreedyActionSelector (prism/agents/action_selectors.py:24-45) with one
// coin and one random action PER ROW, where the reference tosses one coin for the whole call.  The greedy action is
// greedy_argmax_wave's (act_kernels.h), the routine greedy_select_kernel runs; coin and random action are one Philox draw
// of the agent's seed; epsilon is the reference's LinearAnneal (prism/util/annealing_strategies.py:22-33) in float64.  A
// translation unit of its own: learner.hip's code object stays what it was.
#define PRISM_ACT_NO_KERNELS
#include "act_kernels.h"

namespace prism {

constexpr uint64_t EGREEDY_KEY = 0x45475244ull;      // "EGRD": apart from "TAU0" + sid, "PERM", "UNIF", "IDSA"

// The device word that counts the rows seen: the count in its low 44 bits (17e12 rows), the tickets of the call in flight
// in the 20 above them.  Between calls the ticket bits are zero: the word IS the count.
constexpr int EG_TICKET_SHIFT = 44;
constexpr uint64_t EG_TICKET_ONE = 1ull << EG_TICKET_SHIFT, EG_COUNT_MASK = EG_TICKET_ONE - 1;
constexpr int EG_MAX_TICKETS = 1 << 20;

struct EGreedyArgs {
    GreedyArgs g;            // (action / action2: the selected actions)
    double eps_start, eps_stop;
    int64_t anneal_steps;
    uint64_t seed, steps0;
    int row0, n_call;
    unsigned long long *word;       // optional device count of rows seen: added to steps0, advanced by n_call
    const double *u_in;      // optional [n_call]: the coins, in place of the Philox draws (parity)
    double *epsilon;         // optional [1]
    uint8_t *explored;       // optional [n]
};

// LinearAnneal.get_value() at step s, operation for operation (-ffp-contract=off: no fused multiply-add forms here)
__host__ __device__ inline double linear_anneal(double start, double stop, int64_t max_steps, uint64_t s) {
    if (max_steps == 0 || s >= (uint64_t)max_steps) return stop;
    const double f = fmin(1.0, (double)s / (double)max_steps);
    return start * (1.0 - f) + stop * f;
}

// One workgroup per observation, wave 0 decides, lane = action; lane 0 alone tosses the coin.  With the device word: ONE
// atomic add per workgroup is both its read of the count and its ticket, so nobody can read the word after the holder of
// the last ticket has advanced it, and the word after the call is count + n_call whatever the order of the workgroups.
__global__ __launch_bounds__(ACT_THREADS) void egreedy_select_kernel(EGreedyArgs k) {
    extern __shared__ __attribute__((aligned(16))) float s_act[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float *zb = k.g.q ? nullptr : act_stage(k.g.z, b, k.g.T, k.g.A, s_act, k.g.stage != 0);
    if (lane >= 64) return;
    const int best = greedy_argmax_wave(k.g, zb, b, lane);
    if (lane != 0) return;
    uint64_t s0 = k.steps0;
    if (k.word) {
        const uint64_t old = atomicAdd(k.word, (unsigned long long)EG_TICKET_ONE);
        s0 += old & EG_COUNT_MASK;
        if ((int)(old >> EG_TICKET_SHIFT) == k.g.n - 1)          // the last ticket: tickets off, n_call rows on
            atomicAdd(k.word, (unsigned long long)((uint64_t)k.n_call - ((uint64_t)k.g.n << EG_TICKET_SHIFT)));
    }
    const double eps = linear_anneal(k.eps_start, k.eps_stop, k.anneal_steps, s0 + (uint64_t)k.n_call);
    const int row = k.row0 + b;
    uint32_t r[4];
    Philox(k.seed)(s0 + (uint64_t)row, EGREEDY_KEY, r);
    const double u = k.u_in ? k.u_in[row] : u64_to_unit_double(r[0], r[1]);
    const bool explore = u < eps;
    const int pick = explore ? (int)(uint32_t)(((uint64_t)r[2] * (uint32_t)k.g.A) >> 32) : best;
    k.g.action[b] = pick;
    if (k.g.action2) k.g.action2[b] = pick;
    if (k.explored) k.explored[b] = explore ? 1 : 0;
    if (k.epsilon && b == 0) k.epsilon[0] = eps;
}

}  // namespace prism

using namespace prism;

extern "C" int prism_egreedy_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                                    int32_t n_heads, double eps_start, double eps_stop, int64_t anneal_steps, uint64_t seed,
                                    uint64_t steps0, int32_t row0, int32_t n_call, uint64_t *steps_word, const double *u_in,
                                    float *out_mean, double *out_epsilon, uint8_t *out_explored, int64_t *out_action,
                                    int64_t *out_action_host, prism_stream_t stream_) {
    PRISM_CHECK_ARG(out_action, "out_action is null");
    PRISM_CHECK_ARG(z || q, "z and q are both null");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_actions >= 1 && n_actions <= 16, "bad sizes");
    PRISM_CHECK_ARG(q ? n_heads >= 1 : n_tau >= 1, "bad sizes");
    PRISM_CHECK_ARG(anneal_steps >= 0, "anneal_steps is negative");
    // (written so that a NaN fails them)
    PRISM_CHECK_ARG(eps_start >= 0.0 && eps_start <= 1.0 && eps_stop >= 0.0 && eps_stop <= 1.0, "epsilon outside [0, 1]");
    PRISM_CHECK_ARG(row0 >= 0 && (int64_t)row0 + n <= (int64_t)n_call, "rows outside the call");
    PRISM_CHECK_ARG(!steps_word || (row0 == 0 && n_call == n), "steps_word needs the whole call (row0 == 0, n_call == n)");
    PRISM_CHECK_ARG(!steps_word || n < EG_MAX_TICKETS, "steps_word takes fewer than 2^20 rows a call");
    const int stage = !q && n_tau * n_actions <= ACT_STAGE_MAX_FLOATS;
    EGreedyArgs k{{z, q, n, n_pad, n_tau, n_actions, n_heads, out_action, out_mean, out_action_host, stage},
                  eps_start, eps_stop, anneal_steps, seed, steps0, row0, n_call,
                  reinterpret_cast<unsigned long long *>(steps_word), u_in, out_epsilon, out_explored};
    hipLaunchKernelGGL(egreedy_select_kernel, dim3(n), dim3(ACT_THREADS), stage ? (size_t)n_tau * n_actions * 4 : 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
