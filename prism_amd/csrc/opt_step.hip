// The clip + optimizer step for the optimizers other than Adam (agent_factory.py:48-58: centered RMSprop, SGD): the two
// launches of learner.hip (clip_adam_kernel, step_back_kernel) instantiated for another per-element update.
// Reference: torch/optim/rmsprop.py (_single_tensor_rmsprop), torch/optim/sgd.py (_single_tensor_sgd), prism/agents/agent.py:73-74.
#include "opt_kernels.h"

namespace prism {

template <int KIND>
__global__ __launch_bounds__(256) void clip_opt_kernel(AdamArgs a) { clip_adam_block<256, KIND>(a, blockIdx.x, gridDim.x); }

// back: block 0 = priority writeback (+ RNG counters); blocks [1, gridDim) = clip + optimizer step.
template <int KIND>
__global__ __launch_bounds__(256) void step_back_opt_kernel(AdamArgs a, prism_replay_desc rp, BackArgs k) {
    kernarg_prefetch<sizeof(AdamArgs) + sizeof(prism_replay_desc) + sizeof(BackArgs)>();
    if (blockIdx.x == 0) {
        __shared__ __attribute__((aligned(16))) char s_pool[PER_UPDATE_LDS_BYTES];
        if (k.plan) per_update_finish(rp, k.plan, k.n, s_pool, k.sib, k.n, k.sib_state);
        else if (k.use_per) per_update_block(rp, k.index, k.priority, k.n, k.alpha, k.eps, k.take_abs, s_pool);
        if (k.rng && threadIdx.x == 0) {
            k.rng[0] += k.inc_per;
            k.rng[1] += k.inc_tau;
        }
        return;
    }
    clip_adam_block<256, KIND>(a, blockIdx.x - 1, gridDim.x - 1);
}

int launch_clip_opt(int kind, int blocks, hipStream_t stream, const AdamArgs &a) {
    if (kind == OPT_RMSPROP) hipLaunchKernelGGL(clip_opt_kernel<OPT_RMSPROP>, dim3(blocks), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(clip_opt_kernel<OPT_SGD>, dim3(blocks), dim3(256), 0, stream, a);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

int launch_step_back_opt(int kind, int blocks, hipStream_t stream, const AdamArgs &a, const prism_replay_desc &rp, const BackArgs &k) {
    if (kind == OPT_RMSPROP) hipLaunchKernelGGL(step_back_opt_kernel<OPT_RMSPROP>, dim3(1 + blocks), dim3(256), 0, stream, a, rp, k);
    else hipLaunchKernelGGL(step_back_opt_kernel<OPT_SGD>, dim3(1 + blocks), dim3(256), 0, stream, a, rp, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

}  // namespace prism
