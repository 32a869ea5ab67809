// Global-norm clip + optimizer step over the flat buffers (Adam, centered RMSprop, SGD) and the arguments of the back
// launch that carries it.  A header of its own: learner.hip holds Adam's two kernels, opt_step.hip the instantiations for
// the other kinds -- in another translation unit, so that the code object with every kernel of the Adam step is the one
// it was before the optimizer kind became a template parameter (same kernels at the same offsets).
#pragma once
#include "replay_kernels.h"

namespace prism {

// ---- global-norm clip + optimizer step over the flat buffers -------------------------------------
// The optimizer behind the clip (agent_factory.py:40-58): torch.optim.Adam, torch.optim.RMSprop(centered=True) or
// torch.optim.SGD, each without momentum / weight decay (the reference constructs no other form).  The numbers are
// PRISM_OPT_* of include/prism_hip.h.
constexpr int OPT_ADAM = 0, OPT_RMSPROP = 1, OPT_SGD = 2;

struct AdamArgs {
    float *p;
    const float *g;
    float *m, *v;                  // Adam: exp_avg, exp_avg_sq.  RMSprop: grad_avg, square_avg.  SGD: never dereferenced
    int64_t n;
    int64_t *step;
    const float *normpart;
    int n_slots;
    double lr, b1, b2, eps;        // RMSprop: b2 = alpha (the decay of square_avg), b1 unused.  SGD: lr only
    float max_norm, grad_scale;
    float *out_scalars;
    unsigned int *ticket;
    const unsigned int *poison;    // data parallel: the workspace status word (PRISM_WS_STATUS_COLLECTIVE_TIMEOUT), else NULL
};

// One NT-thread block of the clip + optimizer update (block `blk` of `nblk`), one instantiation per optimizer KIND: the
// clip, the poison check and the step counter are shared, the per-element update and the buffers it streams differ.
// The operands of the block's first float4 per thread are requested BEFORE the norm is folded: the fold's own loads and
// two barriers then ride on the same memory round trip.  The fold itself is always the 256-lane form (strided partial
// sums, LDS tree), whatever NT: every launch shape arrives at the same bits for the norm.
template <int NT, int KIND = OPT_ADAM>
__device__ __forceinline__ void clip_adam_block(const AdamArgs &a, int blk, int nblk) {
    constexpr bool STATE = KIND != OPT_SGD;      // SGD streams the gradient and the parameters only
    __shared__ float s_red[256];
    __shared__ float s_c[4];     // clip coef, -step_size, sqrt(bias_correction2)
    const int tid = threadIdx.x;
    // the all-reduce in front of this launch gave up on a peer (direct.hip): the gradient is not a sum over all ranks --
    // apply NOTHING (uniform over the grid: every block reads the same sticky word; the host raises at its next poll)
    if (a.poison && (__hip_atomic_load(a.poison, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & PRISM_WS_STATUS_COLLECTIVE_TIMEOUT)) return;
    const int64_t nvec = a.n >> 2;
    const int64_t i0 = (int64_t)blk * NT + tid;
    float4 g0 = make_float4(0.f, 0.f, 0.f, 0.f), p0 = g0, m0 = g0, v0 = g0;
    if (i0 < nvec) {
        g0 = reinterpret_cast<const float4 *>(a.g)[i0];
        p0 = reinterpret_cast<const float4 *>(a.p)[i0];
        if constexpr (STATE) {
            m0 = reinterpret_cast<const float4 *>(a.m)[i0];
            v0 = reinterpret_cast<const float4 *>(a.v)[i0];
        }
    }
    // every block folds the same partials in the same order -> identical norm everywhere
    if (tid < 256) {
        float s = 0.f;
#pragma unroll 4
        for (int i = tid; i < a.n_slots; i += 256) s += a.normpart[i];
        s_red[tid] = s;
    }
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float total = sqrtf(s_red[0]);
        float coef = a.max_norm / (total + 1e-6f);   // torch.nn.utils.clip_grad_norm_
        coef = fminf(coef, 1.0f);
        if constexpr (KIND == OPT_ADAM) {
            // torch.optim.Adam (_single_tensor_adam): bias corrections in float64 from the step count
            const double t = (double)(a.step[0] + 1);
            const double bc1 = 1.0 - pow(a.b1, t), bc2 = 1.0 - pow(a.b2, t);
            s_c[0] = coef;
            s_c[1] = (float)(-(a.lr / bc1));
            s_c[2] = (float)sqrt(bc2);
        } else {
            s_c[0] = coef;
        }
        if (blk == 0) {
            a.out_scalars[3] = total;
            a.out_scalars[5] = coef;
        }
    }
    __syncthreads();
    const float coef = s_c[0], neg_step = KIND == OPT_ADAM ? s_c[1] : (float)(-a.lr), bc2s = KIND == OPT_ADAM ? s_c[2] : 1.0f;
    const float w1 = (float)(1.0 - a.b1), b2f = (float)a.b2, w2 = (float)(1.0 - a.b2), epsf = (float)a.eps;
    const float gs = a.grad_scale;
    auto upd = [&](float g_, float &p, float &m, float &v) {
        const float g = (g_ * gs) * coef;
        if constexpr (KIND == OPT_ADAM) {
            m = fmaf(w1, g - m, m);                 // exp_avg.lerp_(grad, 1 - beta1)
            v = v * b2f + (w2 * g) * g;             // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1-beta2)
            const float denom = sqrtf(v) / bc2s + epsf;
            p = p + (neg_step * m) / denom;         // param.addcdiv_(exp_avg, denom, value=-step_size)
        } else if constexpr (KIND == OPT_RMSPROP) {
            // torch.optim.RMSprop (_single_tensor_rmsprop, centered, no momentum), operation by operation.  The three
            // fused multiply-adds are torch's own: its addcmul evaluates self + (value * t1) * t2 with the last product
            // folded into the sum, its lerp weight * (end - self) + self likewise (restated in float32 on the host and
            // compared bit for bit over several steps).  m = grad_avg, v = square_avg, b2f = alpha.
            v = fmaf(w2 * g, g, v * b2f);           // square_avg.mul_(alpha).addcmul_(grad, grad, value=1-alpha)
            m = fmaf(w2, g - m, m);                 // grad_avg.lerp_(grad, 1 - alpha)
            // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_().add_(eps): NOT clamped -- where rounding leaves the
            // difference below zero the reference's parameter becomes NaN, and so does this one
            const float avg = sqrtf(fmaf(-m, m, v)) + epsf;
            p = p + (neg_step * g) / avg;           // param.addcdiv_(grad, avg, value=-lr)
        } else {
            p = fmaf(neg_step, g, p);               // param.add_(grad, alpha=-lr): torch's add folds alpha * grad into the sum
        }
    };
    auto upd4 = [&](int64_t i, const float4 &g, float4 p, float4 m, float4 v) {
        upd(g.x, p.x, m.x, v.x);
        upd(g.y, p.y, m.y, v.y);
        upd(g.z, p.z, m.z, v.z);
        upd(g.w, p.w, m.w, v.w);
        stream_store4(reinterpret_cast<float4 *>(a.p) + i, p);
        if constexpr (STATE) {
            stream_store4(reinterpret_cast<float4 *>(a.m) + i, m);
            stream_store4(reinterpret_cast<float4 *>(a.v) + i, v);
        }
    };
    if (i0 < nvec) upd4(i0, g0, p0, m0, v0);
    for (int64_t i = i0 + (int64_t)nblk * NT; i < nvec; i += (int64_t)nblk * NT) {
        if constexpr (STATE)
            upd4(i, reinterpret_cast<const float4 *>(a.g)[i], reinterpret_cast<float4 *>(a.p)[i],
                 reinterpret_cast<float4 *>(a.m)[i], reinterpret_cast<float4 *>(a.v)[i]);
        else upd4(i, reinterpret_cast<const float4 *>(a.g)[i], reinterpret_cast<float4 *>(a.p)[i], g0, g0);
    }
    if (blk == 0 && tid < (int)(a.n & 3)) {
        const int64_t i = (nvec << 2) + tid;
        float p = a.p[i], m = 0.f, v = 0.f;
        if constexpr (STATE) {
            m = a.m[i];
            v = a.v[i];
        }
        upd(a.g[i], p, m, v);
        a.p[i] = p;
        if constexpr (STATE) {
            a.m[i] = m;
            a.v[i] = v;
        }
    }
    // the block that finishes last advances the step counter (every block has read it by then)
    __syncthreads();
    if (tid == 0) {
        const unsigned int done = atomicAdd(a.ticket, 1u);
        if (done == (unsigned)(nblk - 1)) {
            a.step[0] = a.step[0] + 1;
            *a.ticket = 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------
// back: block 0 = priority writeback (+ RNG counters); blocks [1, 1 + n_adam) = clip + Adam.
// ------------------------------------------------------------------------------------------
struct BackArgs {
    const int64_t *index;
    const float *priority;
    int n;
    float alpha, eps;
    int take_abs, use_per;
    const int4 *plan;          // non-NULL: the post kernel prepared this writeback; finish it here
    const float2 *sib;
    unsigned int *sib_state;
    uint64_t *rng;
    uint64_t inc_per, inc_tau;
};

// opt_step.hip: clip_adam_block<256, KIND> for KIND = OPT_RMSPROP / OPT_SGD as a launch of its own (`blocks` workgroups)
// and behind the writeback workgroup of the back launch (1 + `blocks`).  PRISM_OK, or PRISM_ERR_HIP with the error set.
int launch_clip_opt(int kind, int blocks, hipStream_t stream, const AdamArgs &a);
int launch_step_back_opt(int kind, int blocks, hipStream_t stream, const AdamArgs &a, const prism_replay_desc &rp, const BackArgs &k);

}  // namespace prism
