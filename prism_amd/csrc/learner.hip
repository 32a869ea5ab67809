// TD update entry points: get_losses + backward (prism_learner_fwd_bwd), clip_grad_norm_ + optimizer step
// (prism_learner_clip_adam; prism_learner_clip_step for RMSprop / SGD), and the fused step front/back (prism_step_front /
// prism_step_back, prism_step_back_opt).
// Reference: /root/reference/prism/agents/models/composite_model.py:94-144,
// prism/agents/agent.py:53-79, prism/learner.py:95-125.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <set>
#include <type_traits>
#include <utility>

#include "step_kernels.h"
#include "fwd_kernels.h"
#include "act_kernels.h"
#include "qbwd2_kernels.h"
#include "bwd3_kernels.h"
#include "bwd4_kernels.h"
#include "plan.h"

namespace prism {

// sum of squares of the (scaled) gradient, one partial per block — data-parallel path, where the
// partials written by the backward kernels predate the all-reduce
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ g, int64_t n, float scale,
                                                        float *__restrict__ normpart) {
    __shared__ float s_red[256];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float x = g[i] * scale;
        s += x * x;
    }
    s_red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) s_red[threadIdx.x] += s_red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) normpart[blockIdx.x] = s_red[0];
}

__global__ __launch_bounds__(256) void clip_adam_kernel(AdamArgs a) { clip_adam_block<256>(a, blockIdx.x, gridDim.x); }

// back: block 0 = priority writeback (+ RNG counters); blocks [1, gridDim) = clip + Adam.
__global__ __launch_bounds__(256) void step_back_kernel(AdamArgs a, prism_replay_desc rp, BackArgs k) {
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
    clip_adam_block<256>(a, blockIdx.x - 1, gridDim.x - 1);
}

// Models with both parts (IDS: IQN + Q ensemble): the two per-sample losses in ONE launch -- blocks [0, B) the quantile
// loss, [B, 2 B) the ensemble loss (both 512-thread routines; neither reads what the other writes: td = dl / 2 + ql / 2 is
// combined by the post launch).  Two latency-bound launches and a boundary become one.
template <int H, bool LN>
__global__ __launch_bounds__(512) void loss_both_kernel(IqnArgs a) {
    if ((int)blockIdx.x < a.B) iqn_loss_body<H, LN, LOSS_WAVES>(a, blockIdx.x);
    else qh_loss_body<H, LN>(a, (int)blockIdx.x - a.B);
}

}  // namespace prism

using namespace prism;

extern "C" int prism_learner_supported(const prism_model_dims *dims, int32_t batch) {
    if (!dims) return PRISM_ERR_INVALID;
    return iqn_supported(dims, batch);
}

extern "C" size_t prism_learner_workspace_bytes(const prism_model_dims *dims, int32_t batch) {
    if (!dims || iqn_supported(dims, batch) != PRISM_OK) return 0;
    return make_plan(*dims, batch).ws_bytes;
}

// What make_plan() decides for (dims, batch, gemm_mode), read-only and without a device call: out[0 .. PRISM_PLAN_N) in
// the order of the PRISM_PLAN_* indices (include/prism_hip.h).  A test asks it which launch forms its case really takes.
extern "C" int prism_learner_plan_info(const prism_model_dims *dims, int32_t batch, int32_t gemm_mode, int32_t *out, int32_t n_out) {
    static_assert(BWD_NONE == PRISM_BWD_NONE && BWD_FP32 == PRISM_BWD_FP32 && BWD_BW3 == PRISM_BWD_BW3 && BWD_BW4 == PRISM_BWD_BW4 &&
                      BWD_LIN == PRISM_BWD_LIN && QB_NONE == PRISM_QB_NONE && QB_ROWS == PRISM_QB_ROWS && QB_COLS == PRISM_QB_COLS &&
                      QB_QB2 == PRISM_QB_QB2, "plan.h's forms are the header's");
    if (!dims || !out || n_out < PRISM_PLAN_N) return PRISM_ERR_INVALID;
    if (iqn_supported(dims, batch) != PRISM_OK) return PRISM_ERR_UNSUPPORTED;
    const LearnerPlan p = make_plan(*dims, batch, gemm_mode);
    out[PRISM_PLAN_BWD] = p.bwd;
    out[PRISM_PLAN_Q_BWD] = p.q_bwd;
    out[PRISM_PLAN_CONV_IN_BWD] = p.conv_in_bwd;
    out[PRISM_PLAN_N_CHUNKS] = p.n_chunks;
    out[PRISM_PLAN_LOCAL_LOSS] = p.local_loss;
    out[PRISM_PLAN_MERGED_LOSS] = p.merged_loss;
    out[PRISM_PLAN_SPLIT] = p.split;
    out[PRISM_PLAN_Q_DE_SLOTS] = p.q_de_slots;
    out[PRISM_PLAN_POST_BLOCKS] = p.post_blocks;
    return PRISM_OK;
}

// The ONE envelope check, plan and carve of a call: every entry point starts here and hands `pl` on.
// `need_batch`: the minibatch arrays and outputs of an update must be bound (not for the acting forward, which may well
// run before the first update)
static int check_learner(const prism_learner_desc *ld, LearnerPlan &pl, bool need_batch = true) {
    PRISM_CHECK_ARG(ld != nullptr, "null descriptor");
    if (iqn_supported(&ld->dims, ld->batch) != PRISM_OK) {
        set_error("prism_learner: model dims / batch not covered by the HIP kernels "
                  "(need E=1024; IQN: K=64, T in {4,8,16,32,64}, B*T %% 16 == 0, and either one trunk layer with H in {128,256} "
                  "or no trunk layer and no Q heads beside it -- the linear head next to a Q ensemble needs the merged loss "
                  "launch and the heads' embedding-gradient sum, which are not built for it; "
                  "Q heads: one layer, or two layers of width 128/256 with B %% 16 == 0)");
        return PRISM_ERR_UNSUPPORTED;
    }
    pl = make_plan(ld->dims, ld->batch, ld->gemm_mode, ld->workspace, ld->fused_replay, ld->fused_index, ld->fuse_tail,
                   ld->hyper.grad_scale);
    PRISM_CHECK_ARG(ld->params && ld->grads && ld->adam_m && ld->adam_v && ld->adam_step, "null parameter buffers");
    PRISM_CHECK_ARG(!ld->dims.has_target || ld->target_params, "has_target without target_params");
    PRISM_CHECK_ARG(ld->workspace && ld->workspace_bytes >= pl.ws_bytes, "workspace too small");
    PRISM_CHECK_ARG(((uintptr_t)ld->workspace & 15) == 0, "workspace must be 16-byte aligned");
    PRISM_CHECK_ARG((((uintptr_t)ld->params | (uintptr_t)ld->grads | (uintptr_t)ld->adam_m | (uintptr_t)ld->adam_v) & 15) == 0,
                    "parameter / gradient / Adam buffers must be 16-byte aligned");
    PRISM_CHECK_ARG(ld->off.n_params > 0 && (!ld->dims.use_iqn || (ld->off.phi_w & 3) == 0),
                    "n_params / phi_w offset alignment");
    PRISM_CHECK_ARG(ld->dims.n_heads == 0 || (ld->off.head_base >= 0 && ld->off.h_w1 >= 0 && ld->off.h_b1 >= 0),
                    "Q-head parameter offsets missing");
    PRISM_CHECK_ARG(ld->dims.n_heads == 0 || ld->dims.head_layers == 1 ||
                        (ld->off.h_w2 >= 0 && (!ld->dims.use_layer_norm || (ld->off.h_ln1_g >= 0 && ld->off.h_ln2_g >= 0))),
                    "two-layer Q-head parameter offsets missing");
    PRISM_CHECK_ARG(!ld->dims.use_iqn || pl.lin ||
                        (ld->off.iqn_w1 >= 0 && ld->off.iqn_w2 >= 0 &&
                         (!ld->dims.use_layer_norm || (ld->off.iqn_ln1_g >= 0 && ld->off.iqn_ln2_g >= 0))),
                    "IQN parameter offsets missing (one trunk layer: iqn_w1, iqn_w2 and, with LayerNorm, iqn_ln1_g, iqn_ln2_g)");
    if (pl.lin) {
        // no trunk: phi | [the final LayerNorm, in iqn_ln2_*] | head, contiguous in model.parameters() order -- the
        // backward's slabs are laid out like that and summed straight into the flat gradient
        const prism_param_offsets &o = ld->off;
        const int64_t after_phi = o.phi_w + (int64_t)E_DIM * K_BASIS + E_DIM;
        PRISM_CHECK_ARG(o.phi_w >= 0 && o.phi_b == o.phi_w + (int64_t)E_DIM * K_BASIS && o.iqn_w2 >= 0 && o.iqn_b2 >= 0,
                        "linear IQN head: parameter offsets missing (phi_w, phi_b, iqn_w2, iqn_b2)");
        PRISM_CHECK_ARG(ld->dims.use_layer_norm
                            ? (o.iqn_ln2_g == after_phi && o.iqn_ln2_b == after_phi + E_DIM && o.iqn_w2 == after_phi + 2 * E_DIM)
                            : o.iqn_w2 == after_phi,
                        "linear IQN head: phi, [LayerNorm in iqn_ln2_g / iqn_ln2_b] and iqn_w2 must follow each other");
        PRISM_CHECK_ARG(o.iqn_b2 == o.iqn_w2 + (int64_t)ld->dims.n_actions * E_DIM, "linear IQN head: iqn_b2 must follow iqn_w2");
    }
    if (!need_batch) return PRISM_OK;
    PRISM_CHECK_ARG(ld->obs && ld->next_obs && ld->reward && ld->nonterminal && ld->gamma && ld->action,
                    "null batch arrays");
    PRISM_CHECK_ARG(ld->out_td && ld->out_scalars, "null outputs");
    return PRISM_OK;
}

// One forward pass over `n_tiles` 16-row tiles.  kind 0: IQN quantile rows, 1: Q-head rows, 2: mixed tiles of whole samples
// (T current-state + T next-state rows; e2 / tau2 / z2 are the next-state half).  `set`: 0 online, 1 target weights (and
// their packed copies / u|v tables).  The tau draws are tied to `sid` (IqnPass.stream_id) in the reference's draw order
// (iqn_model.py:104,112-126).  Needs a.params / target_params / ws / Hi / Hq / n_heads.
static IqnPass make_pass(const IqnArgs &a, int kind, int set, const float *e, const float *tau, float *z, int T, int n_tiles,
                         int save, int sid, const float *e2 = nullptr, const float *tau2 = nullptr, float *z2 = nullptr) {
    IqnPass p;
    memset(&p, 0, sizeof(p));
    p.params = set ? a.target_params : a.params;
    p.wpk = kind == 1 ? a.ws.q_wpk[set] : a.ws.wpk[set];
    p.uv = kind == 1 ? a.ws.q_uv + (size_t)set * a.n_heads * UV_ROWS * a.Hq : a.ws.uv + (size_t)set * UV_ROWS * a.Hi;
    p.e = e;
    p.e2 = e2;
    p.tau_in = tau;
    p.tau_in2 = tau2;
    p.z_out = z;
    p.z_out2 = z2;
    p.T = T;
    p.n_tiles = n_tiles;
    p.save = save;
    p.stream_id = sid;
    p.kind = kind;
    return p;
}

// The arguments the embed / front launch sees.  Its parameter-only roles (front_extra_blocks: u / v tables, stream-packed
// weight copies, cos tiles) exist for an IQN TRUNK; the linear head has none, and says so the one way those kernels read
// it: no IQN part.  (The sampling and convolution workgroups do not look at the field.)
static IqnArgs front_args(const IqnArgs &a) {
    IqnArgs f = a;
    if (iqn_linear(a.use_iqn, a.Hi)) f.use_iqn = 0;
    return f;
}

// the kernel arguments of an update: the plan's decisions, the descriptor's pointers, the learner's pass list
static void fill_iqn_args(const prism_learner_desc *ld, const LearnerPlan &pl, IqnArgs &a) {
    const prism_model_dims &d = ld->dims;
    const int B = ld->batch;
    memset(&a, 0, sizeof(a));
    a.ws = pl.ws;
    a.B = B;
    a.Bt = B;
    a.A = d.n_actions;
    a.C = d.in_channels;
    a.T = d.n_tau;
    a.Tn = d.n_tau_next;
    a.Hi = pl.Hi;
    a.Hq = pl.Hq;
    a.ln = d.use_layer_norm;
    a.slab = pl.slab;
    a.q_slab = pl.q_slab;
    a.n_chunks = pl.n_chunks;
    a.has_target = d.has_target;
    a.double_q = d.double_q;
    a.propagate_grad = d.propagate_grad;
    a.squish = d.squish_fn;
    a.split = pl.split;
    a.q_de_slots = pl.q_de_slots;
    a.conv_in_bwd = pl.conv_in_bwd;
    a.conv_rows = pl.conv_rows;
    a.bg = bwd_geometry(a.Hi, a.B, a.C, a.T, a.n_chunks, a.conv_in_bwd != 0);
    a.huber_k = d.huber_k;
    a.dist_w = d.dist_loss_weight;
    a.use_iqn = d.use_iqn;
    a.n_heads = d.n_heads;
    a.head_layers = d.head_layers;
    a.q_w = d.q_loss_weight;
    a.theil_coef = d.n_heads > 1 ? d.theil_coef : 0.f;
    { const char *e = getenv("PRISM_DBG"); a.dbg = e ? atoi(e) : 0; }
    a.stamps = (unsigned long long *)ld->dbg_stamps;
    if (!a.stamps) a.dbg &= ~(8 | 16 | 32);
    a.off = ld->off;
    a.params = ld->params;
    a.target_params = ld->target_params;
    a.obs = ld->obs;
    a.next_obs = ld->next_obs;
    a.reward = ld->reward;
    a.gamma = ld->gamma;
    a.per_weights = ld->per_weights;
    a.nonterminal = ld->nonterminal;
    a.action = ld->action;
    a.seed = ld->seed;
    a.offset = ld->offset;
    a.rng = ld->rng_counters;
    a.tau_out = ld->tau_out ? ld->tau_out : pl.tau_buf;
    a.maxT = pl.maxT;
    a.out_dl = ld->out_dist_loss ? ld->out_dist_loss : pl.dl_buf;
    a.out_ql = ld->out_q_loss ? ld->out_q_loss : pl.dl_buf + B;
    a.out_td = ld->out_td;
    a.out_scalars = ld->out_scalars;
    a.grads = ld->grads;
    a.local_loss = pl.local_loss;
    // passes: current state | next state on the online weights (no target network, or double Q) | next state on the target's
    int np = 0;
    const bool online_next = !d.has_target || d.double_q;
    if (pl.local_loss) {
        a.pass[np++] = make_pass(a, 2, 0, a.ws.e_cur, ld->tau_cur, a.ws.zcur, d.n_tau, B * 2 * d.n_tau / 16, 1, 0, a.ws.e_next,
                                 ld->tau_next_online, a.ws.zon);
    } else if (d.use_iqn) {
        const int nt = B * d.n_tau_next / 16;
        a.pass[np++] = make_pass(a, 0, 0, a.ws.e_cur, ld->tau_cur, a.ws.zcur, d.n_tau, B * d.n_tau / 16, 1, 0);
        if (online_next) a.pass[np++] = make_pass(a, 0, 0, a.ws.e_next, ld->tau_next_online, a.ws.zon, d.n_tau_next, nt, 0, 1);
        if (d.has_target) a.pass[np++] = make_pass(a, 0, 1, a.ws.e_next, ld->tau_next_target, a.ws.ztg, d.n_tau_next, nt, 0, 2);
    }
    if (d.use_iqn) {
        if (!d.has_target) a.ws.ztg = a.ws.zon;            // bootstrap from self
        else if (!d.double_q) a.ws.zon = a.ws.ztg;         // DQN-style: target picks the action too
    }
    if (d.n_heads > 0 && d.head_layers == 2) {
        // Q-head tiles: (B/16) x heads per pass; same online/target selection (q_ensemble.py:62-68)
        const int nt = (B / 16) * d.n_heads;
        a.pass[np++] = make_pass(a, 1, 0, a.ws.e_cur, nullptr, a.ws.zq_cur, 1, nt, 1, 0);
        if (online_next) a.pass[np++] = make_pass(a, 1, 0, a.ws.e_next, nullptr, a.ws.zq_on, 1, nt, 0, 1);
        if (d.has_target) a.pass[np++] = make_pass(a, 1, 1, a.ws.e_next, nullptr, a.ws.zq_tg, 1, nt, 0, 2);
        if (!d.has_target) a.ws.zq_tg = a.ws.zq_on;
        else if (!d.double_q) a.ws.zq_on = a.ws.zq_tg;
    }
    a.n_pass = np;
    // the IQN tiles' quantile samples + cos basis come prepared from the embed / front launch (bf16 mode: the prologue they
    // replace is the split forward's)
    if (a.split)
        for (int i = 0; i < np; ++i)
            if (a.pass[i].kind != 1) {
                a.pass[i].cospk = a.ws.cospk + (size_t)a.cos_tiles * CP_TILE;
                a.cos_tiles += a.pass[i].n_tiles;
            }
}

static void fill_adam_args(const prism_learner_desc *ld, const IqnWs &ws, AdamArgs &a) {
    a.p = ld->params;
    a.g = ld->grads;
    a.m = ld->adam_m;
    a.v = ld->adam_v;
    a.n = ld->off.n_params;
    a.step = ld->adam_step;
    a.normpart = ws.normpart;
    a.lr = ld->hyper.lr;
    a.b1 = ld->hyper.beta1;
    a.b2 = ld->hyper.beta2;
    a.eps = ld->hyper.eps;
    a.max_norm = ld->hyper.max_grad_norm;
    a.grad_scale = ld->hyper.grad_scale;
    a.out_scalars = ld->out_scalars;
    a.ticket = ws.ticket;
    // data parallel (the gradient is scaled by 1 / world): a collective that gave up on a peer poisons the step
    a.poison = ld->hyper.grad_scale != 1.0f ? ws.ticket + PRISM_WS_STATUS_WORD : nullptr;
}

// The optimizer of the new entry points (prism_learner_clip_step / prism_step_back_opt).  Refusals that need no device
// come first: tests run them on machines without one.
static int check_opt(const prism_learner_desc *ld, const prism_opt_hyper *opt) {
    PRISM_CHECK_ARG(ld != nullptr, "null descriptor");
    PRISM_CHECK_ARG(opt != nullptr, "null optimizer hyper-parameters");
    PRISM_CHECK_ARG(opt->kind == PRISM_OPT_ADAM || opt->kind == PRISM_OPT_RMSPROP || opt->kind == PRISM_OPT_SGD,
                    "optimizer kind must be PRISM_OPT_ADAM, PRISM_OPT_RMSPROP or PRISM_OPT_SGD");
    if (opt->kind != PRISM_OPT_ADAM && ld->fuse_tail != 0) {
        set_error("%s: the fused tail (fuse_tail != 0) is built for Adam only; pass fuse_tail = 0 with RMSprop / SGD", __func__);
        return PRISM_ERR_UNSUPPORTED;
    }
    return PRISM_OK;
}
// (Adam keeps reading ld->hyper: the old and the new entry points then cannot disagree)
static void apply_opt(const prism_opt_hyper *opt, AdamArgs &a) {
    if (opt->kind == PRISM_OPT_ADAM) return;
    a.lr = opt->lr;
    a.b1 = 0.0;
    a.b2 = opt->alpha;
    a.eps = opt->eps;
}

// (one workgroup per CU -- every workgroup folds the norm partials itself before its first update, a fixed cost per workgroup:
// measured on c4's 1.5 M parameters, clip + Adam + writeback: 2048 workgroups 25.5 us, 512: 15.5, 256: 13.4, 128: 15.4;
// subtractive preset, 3.0 M: 33.8 / 20.7 / 18.8 / 23.8)
#ifndef ADAM_MAX_BLOCKS
#define ADAM_MAX_BLOCKS 256
#endif
static int adam_blocks(int64_t n) {
    int blocks = (int)(((n >> 2) + 255) / 256);
    if (blocks > ADAM_MAX_BLOCKS) blocks = ADAM_MAX_BLOCKS;
    return blocks < 1 ? 1 : blocks;
}

// template dispatch over the hidden width and LayerNorm on/off
template <typename F>
static void dispatch_hl(int H, int ln, F &&f) {
    if (H == 128) {
        if (ln) f(std::integral_constant<int, 128>{}, std::true_type{});
        else f(std::integral_constant<int, 128>{}, std::false_type{});
    } else {
        if (ln) f(std::integral_constant<int, 256>{}, std::true_type{});
        else f(std::integral_constant<int, 256>{}, std::false_type{});
    }
}

// dynamic-LDS opt-in of the kernels that need more than 64 KB: once per device and instantiation
static hipError_t set_max_lds(const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({fn, dev})) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) done.insert({fn, dev});
    return e;
}

// launch of a kernel with `lds` bytes of dynamic LDS, after the opt-in to `opt_in` bytes (0: `lds`); the caller checks the launch
static int launch_lds(void (*kernel)(IqnArgs), const char *name, dim3 grid, dim3 block, size_t lds, hipStream_t stream,
                      IqnArgs a, size_t opt_in = 0) {
    const hipError_t e = set_max_lds((const void *)kernel, opt_in ? opt_in : lds);
    if (e != hipSuccess) {
        set_error("hipFuncSetAttribute(%s): %s", name, hipGetErrorString(e));
        return PRISM_ERR_HIP;
    }
    void *args[] = {&a};
    (void)hipLaunchKernel((const void *)kernel, grid, block, args, lds, stream);
    return PRISM_OK;
}

static int device_cus() {
    static std::mutex mu;
    static std::map<int, int> cache;
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(dev);
    if (it != cache.end()) return it->second;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cache[dev] = cus;
}

// Forward tiles on four waves (fwd_kernels.h, WAVES = 4: two 256-thread workgroups per CU, the latency-bound phases of one tile
// beside the weight stream of another): where the launch has at least two tiles per CU and no mixed tile (their loss tail
// needs all sixteen rows in registers at once).
static bool fwd_four_waves(const IqnArgs &aa, int tiles) {
    if (!aa.split) return false;
    for (int i = 0; i < aa.n_pass; ++i)
        if (aa.pass[i].kind == 2) return false;
    return tiles >= 2 * device_cus();
}

// the forward tiles of every pass: one launch when every tile kind has the same hidden width, else one per kind
static int launch_fwd_tiles(const IqnArgs &a, hipStream_t stream) {
    if (iqn_linear(a.use_iqn, a.Hi)) {
        // the linear head: every pass is IQN rows (no Q heads beside it), one tile form for both gemm modes
        int tiles = 0;
        for (int i = 0; i < a.n_pass; ++i) tiles += a.pass[i].n_tiles;
        if (tiles > 0)
            hipLaunchKernelGGL(a.ln ? lin_fwd_tile_kernel<true> : lin_fwd_tile_kernel<false>, dim3(tiles), dim3(256), 0, stream, a);
        return PRISM_OK;
    }
    auto launch = [&](const IqnArgs &aa, int H, int tiles) {
        int rc = PRISM_OK;
        dispatch_hl(H, aa.ln, [&](auto h, auto l) {
            constexpr int HH = decltype(h)::value;
            constexpr bool LL = decltype(l)::value;
            const size_t lds = fw_lds_floats<HH>() * sizeof(float);
            if constexpr (HH == 128) {
                if (fwd_four_waves(aa, tiles)) {
                    rc = launch_lds(fwd_tile_kernel<HH, LL, true, 4>, "fwd_tile", dim3(tiles), dim3(256),
                                    fw_lds_floats<HH, 4>() * sizeof(float), stream, aa);
                    return;
                }
            }
            if (aa.split) rc = launch_lds(fwd_tile_kernel<HH, LL, true>, "fwd_tile", dim3(tiles), dim3(fw_threads(HH)), lds, stream, aa);
            else rc = launch_lds(fwd_tile_kernel<HH, LL>, "fwd_tile", dim3(tiles), dim3(fw_threads(HH)), lds, stream, aa);
        });
        return rc;
    };
    int n_iqn = 0, n_q = 0;
    for (int i = 0; i < a.n_pass; ++i) (a.pass[i].kind == 1 ? n_q : n_iqn) += a.pass[i].n_tiles;
    if (n_iqn && n_q && a.Hi != a.Hq) {
        IqnArgs a1 = a, a2 = a;
        a1.n_pass = a2.n_pass = 0;
        for (int i = 0; i < a.n_pass; ++i) {
            if (a.pass[i].kind == 1) a2.pass[a2.n_pass++] = a.pass[i];
            else a1.pass[a1.n_pass++] = a.pass[i];
        }
        const int rc = launch(a1, a.Hi, n_iqn);
        return rc ? rc : launch(a2, a.Hq, n_q);
    }
    return n_iqn + n_q > 0 ? launch(a, n_iqn ? a.Hi : a.Hq, n_iqn + n_q) : PRISM_OK;
}

// ---- the post launch: gradient slabs / small tensors / conv fold (+ priority writeback block); with `tail` also the
// clip + Adam update behind a grid barrier (single GPU) ------------------------------------------------------------
// its instantiation: the fused tail (always the full writer) with the dense tree top or without | preparing a writeback
// the back launch finishes (`planned`) | the full writer, dense or not (also: no writeback at all)
using PostKernel = void (*)(IqnArgs, PostWriteback, TailArgs);
static PostKernel post_kernel(bool tail, bool planned, bool dense, bool lin = false) {
    if (lin) {          // (the linear IQN head: its own instantiations, never the fused tail)
        if (planned) return iqn_post_kernel<false, false, false, true>;
        return dense ? iqn_post_kernel<true, false, true, true> : iqn_post_kernel<true, false, false, true>;
    }
    if (tail) return dense ? iqn_post_kernel<true, true, true> : iqn_post_kernel<true, true, false>;
    if (planned) return iqn_post_kernel<false, false, false>;
    return dense ? iqn_post_kernel<true, false, true> : iqn_post_kernel<true, false, false>;
}

// workgroups of the fused-tail instantiation `dense` that fit the CURRENT device at once (per device: processes that
// drive several GPUs, and per instantiation: the two forms differ in registers)
static int post_max_resident(bool dense) {
    static std::mutex mu;
    static std::map<std::pair<int, bool>, int> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({dev, dense});
    if (it != cache.end()) return it->second;
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, post_kernel(true, false, dense), 1024, 0) != hipSuccess) return 0;
    return cache[{dev, dense}] = cus * per;
}

// The fused tail needs every workgroup of the launch resident at once (it has a grid barrier; the device must not be
// shared with other processes' kernels -- the barrier gives up after GRID_WAIT_TICKS and flags it, step_kernels.h): the
// plan says whether it is wanted, the device whether it fits.
static bool tail_fused(const LearnerPlan &pl) { return pl.tail_wanted && pl.post_blocks + 1 <= post_max_resident(pl.post_dense); }

// (`ld`: the writeback's pointers and exponents; every decision is the plan's)
static int launch_post(const prism_learner_desc *ld, const LearnerPlan &pl, const IqnArgs &a, const TailArgs *tail, hipStream_t stream) {
    ProfileScope ps_(tail ? K_TAIL : K_POST, stream);
    int nb = pl.post_blocks;
    PostWriteback wb;
    memset(&wb, 0, sizeof(wb));
    if (pl.writeback_rides) {
        // TD errors are final: the priority writeback rides along as one more block of this launch
        wb.enabled = 1;
        wb.rp = *ld->fused_replay;
        wb.index = ld->fused_index;
        wb.sib = reinterpret_cast<const float2 *>(a.ws.sib);
        wb.sib_state = a.ws.ticket + 3;
        wb.plan = (!tail && pl.split_writeback) ? reinterpret_cast<int4 *>(a.ws.wb_plan) : nullptr;
        wb.alpha = ld->fused_alpha;
        wb.eps = ld->fused_eps;
        wb.block = nb;
        nb += 1;
    }
    TailArgs none;
    memset(&none, 0, sizeof(none));
    hipLaunchKernelGGL(post_kernel(tail != nullptr, wb.plan != nullptr, pl.post_dense, pl.lin), dim3(nb), dim3(1024), 0, stream, a, wb,
                       tail ? *tail : none);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// get_losses + backward as its launch sequence: embed, forward tiles, loss, Q loss, backward, Q backward, post -- each in
// the form the plan names.  Losses first (TD errors final), then the backward kernels.
extern "C" int prism_learner_fwd_bwd(const prism_learner_desc *ld, prism_stream_t stream_) {
    LearnerPlan pl;
    int rc = check_learner(ld, pl);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = ld->batch, heads = ld->dims.n_heads;
    IqnArgs a;
    fill_iqn_args(ld, pl, a);

    if (!ld->embed_done) {
        ProfileScope ps_(K_EMBED, stream);
        const IqnArgs af = front_args(a);
        hipLaunchKernelGGL(iqn_embed_kernel, dim3(2 * B + front_extra_blocks(extra_dims(af))), dim3(256), 0, stream, af);
        PRISM_CHECK_LAUNCH();
    }
    {
        ProfileScope ps_(K_TILE_FWD, stream);
        rc = launch_fwd_tiles(a, stream);
        if (rc) return rc;
        PRISM_CHECK_LAUNCH();
    }
    if (pl.merged_loss) {
        ProfileScope ps_(K_LOSS, stream);
        dispatch_hl(a.Hi, a.ln, [&](auto h, auto l) {
            hipLaunchKernelGGL((loss_both_kernel<decltype(h)::value, decltype(l)::value>), dim3(2 * B), dim3(512), 0, stream, a);
        });
        PRISM_CHECK_LAUNCH();
    } else if (pl.lin) {
        ProfileScope ps_(K_LOSS, stream);
        hipLaunchKernelGGL(a.ln ? lin_loss_kernel<true> : lin_loss_kernel<false>, dim3(B), dim3(256), 0, stream, a);
        PRISM_CHECK_LAUNCH();
    } else if (ld->dims.use_iqn && !pl.local_loss) {
        ProfileScope ps_(K_LOSS, stream);
        dispatch_hl(a.Hi, a.ln, [&](auto h, auto l) {
            if (pl.loss_waves == 16)
                hipLaunchKernelGGL((iqn_loss_kernel<decltype(h)::value, decltype(l)::value, 16>), dim3(B), dim3(64 * 16), 0, stream, a);
            else
                hipLaunchKernelGGL((iqn_loss_kernel<decltype(h)::value, decltype(l)::value, LOSS_WAVES>), dim3(B),
                                   dim3(64 * LOSS_WAVES), 0, stream, a);
        });
        PRISM_CHECK_LAUNCH();
    }
    if (heads > 0 && !pl.merged_loss) {
        ProfileScope ps_(K_Q_FWD, stream);
        if (ld->dims.head_layers == 1) {
            hipLaunchKernelGGL(dqn_loss_kernel, dim3(B), dim3(256), 0, stream, a);
        } else {
            dispatch_hl(a.Hq, a.ln, [&](auto h, auto l) {
                hipLaunchKernelGGL((qh_loss_kernel<decltype(h)::value, decltype(l)::value>), dim3(B), dim3(512), 0, stream, a);
            });
        }
        PRISM_CHECK_LAUNCH();
    }
    if (pl.bwd != BWD_NONE) {
        const bool conv = a.conv_in_bwd != 0;
        if (pl.bwd == BWD_FP32 && !bwd_lds_layout_ok(a.Hi, B, a.C, a.T, a.n_chunks, conv)) {
            set_error("prism_learner_fwd_bwd: internal: LDS layout of the backward kernel overlaps for this shape");
            return PRISM_ERR_INVALID;
        }
        ProfileScope ps_(K_BWD, stream);
        switch (pl.bwd) {
        case BWD_BW3:
            rc = launch_lds(a.ln ? iqn_bwd3_kernel<true> : iqn_bwd3_kernel<false>, "iqn_bwd3", dim3((E_DIM / 64) * BW3_RC), dim3(512),
                            (size_t)bw3_lds_bytes(B, a.T, a.C, conv), stream, a, 160 * 1024);
            break;
        case BWD_BW4:
            rc = launch_lds(a.ln ? iqn_bwd4_kernel<true> : iqn_bwd4_kernel<false>, "iqn_bwd4", dim3((E_DIM / 32) * a.n_chunks), dim3(512),
                            BW4_LDS_BYTES, stream, a);
            break;
        case BWD_LIN:
            hipLaunchKernelGGL(a.ln ? lin_bwd_kernel<true> : lin_bwd_kernel<false>, dim3((E_DIM / 16) * a.n_chunks), dim3(256), 0,
                               stream, a);
            break;
        default:
            dispatch_hl(a.Hi, a.ln, [&](auto h, auto l) {
                rc = launch_lds(iqn_bwd_kernel<decltype(h)::value, decltype(l)::value>, "iqn_bwd", dim3((E_DIM / 16) * a.n_chunks),
                                dim3(256), (size_t)bwd_lds_floats(a.Hi, B, a.C, a.T, a.n_chunks, conv) * sizeof(float), stream, a);
            });
        }
        if (rc) return rc;
        PRISM_CHECK_LAUNCH();
    }
    if (pl.q_bwd != QB_NONE) {
        ProfileScope ps_(K_Q_BWD, stream);
        const size_t lds = qb_lds_floats(a.Hq) * sizeof(float);
        switch (pl.q_bwd) {
        case QB_QB2:
            rc = launch_lds(a.ln ? qh_bwd2_kernel<true> : qh_bwd2_kernel<false>, "qh_bwd2", dim3(qb2_blocks(heads, B)), dim3(256),
                            QB2_LDS_BYTES, stream, a);
            break;
        default:
            dispatch_hl(a.Hq, a.ln, [&](auto h, auto l) {
                constexpr int HH = decltype(h)::value;
                constexpr bool LL = decltype(l)::value;
                if (pl.q_bwd == QB_COLS)      // (qhead_kernels.h, COLS)
                    rc = launch_lds(qh_bwd_kernel<HH, LL, true>, "qh_bwd", dim3((E_DIM / 64) * heads), dim3(256), lds, stream, a);
                else
                    rc = launch_lds(qh_bwd_kernel<HH, LL>, "qh_bwd", dim3((E_DIM / 16) * heads), dim3(256), lds, stream, a);
            });
        }
        if (rc) return rc;
        PRISM_CHECK_LAUNCH();
    }
    if (!tail_fused(pl)) {
        rc = launch_post(ld, pl, a, nullptr, stream);
        if (rc) return rc;
    }
    if (ld->dbg_z) {
        const size_t R = (size_t)B * ld->dims.n_tau, Rn = (size_t)B * ld->dims.n_tau_next, A = ld->dims.n_actions;
        (void)hipMemcpyAsync(ld->dbg_z, a.ws.zcur, R * A * 4, hipMemcpyDeviceToDevice, stream);
        (void)hipMemcpyAsync(ld->dbg_z + R * A, a.ws.ztg, Rn * A * 4, hipMemcpyDeviceToDevice, stream);
    }
    return PRISM_OK;
}

// Acting forward (agent.py:31-41 -> composite_model.py:51-70, iqn_model.py:61-87 with for_action=True): embeds `n`
// observations, runs n_tau quantile rows per observation through the IQN tiles and the observations through every
// Q head -- the same forward tiles as the update, on the learner's workspace (the stream-packed weights are rebuilt
// first: the last Adam step left them stale).
extern "C" int prism_act_forward(const prism_learner_desc *ld, const float *obs, int32_t n, int32_t n_tau,
                                 const float *tau_in, uint64_t seed, uint64_t offset, float *out_z, float *out_q,
                                 prism_stream_t stream_) {
    LearnerPlan pl;
    int rc = check_learner(ld, pl, false);
    if (rc) return rc;
    const int heads = ld->dims.n_heads;
    const bool heads2 = heads > 0 && ld->dims.head_layers == 2;
    PRISM_CHECK_ARG(obs != nullptr && n >= 1 && n <= ld->batch, "n must be in [1, batch]");
    const int n_pad = (n + 15) / 16 * 16;
    PRISM_CHECK_ARG(n_pad <= ld->batch || !heads2, "Q-head tiles need the workspace of a batch >= 16-padded n");
    PRISM_CHECK_ARG(!ld->dims.use_iqn || (n_tau >= 1 && out_z), "quantile samples per action / output buffer");
    PRISM_CHECK_ARG(!heads2 || out_q, "Q output buffer");
    hipStream_t stream = (hipStream_t)stream_;
    // the learner's arguments with the acting call's overrides, each stated once: here for the embed launch (+ the
    // parameter-only roles), where the n observations stand in for both batch halves ...
    IqnArgs a;
    fill_iqn_args(ld, pl, a);
    a.cos_tiles = 0;          // (acting tiles draw and evaluate their basis themselves: no learner passes here)
    a.B = n;
    a.obs = a.next_obs = obs;
    // quantile draws counted on the device (ld->rng_counters[2], added to `offset`): the call can be captured into a hipGraph
    // and replayed -- the embed launch advances the counter by this call's n * n_tau draws, the tiles of the next launch
    // start from counter - n * n_tau
    const uint64_t act_inc = ld->dims.use_iqn ? (uint64_t)n * (uint64_t)n_tau : 0ull;
    a.act_rng = (ld->rng_counters && !tau_in && act_inc) ? ld->rng_counters + 2 : nullptr;
    a.act_inc = act_inc;
    // PRISM_ACT_WEIGHTS_CURRENT: the stream-packed weight copies / LayerNorm helpers in the workspace were built from the
    // parameters as they are now (by an earlier acting call since the last update): the launch is the n embeddings alone
    const IqnArgs af = front_args(a);
    const int extra = (ld->act_flags & PRISM_ACT_WEIGHTS_CURRENT) ? 0 : front_extra_blocks(extra_dims(af));
    hipLaunchKernelGGL(iqn_embed_kernel, dim3((extra ? 2 * n : n) + extra), dim3(256), 0, stream, af);
    PRISM_CHECK_LAUNCH();
    if (heads > 0 && ld->dims.head_layers == 1) {
        // single-Linear DQN head: one workgroup per observation on the embeddings just written
        PRISM_CHECK_ARG(out_q != nullptr, "Q output buffer");
        hipLaunchKernelGGL(dqn1_act_kernel, dim3(n), dim3(256), 0, stream, a, out_q);
        PRISM_CHECK_LAUNCH();
        return PRISM_OK;
    }
    // ... and here for the tiles: rows padded to whole tiles, the caller's Philox position, no loss
    a.B = n_pad;
    a.Bt = n;
    a.seed = seed;
    a.offset = a.act_rng ? offset - act_inc : offset;
    a.rng = a.act_rng ? ld->rng_counters + 1 : nullptr;      // (the tiles read word [1] of what they are given)
    a.act_rng = nullptr;
    a.tau_out = nullptr;
    a.local_loss = 0;
    a.n_pass = 0;
    // (stream_id 3: a Philox stream of its own -- acting draws never repeat an update's)
    if (ld->dims.use_iqn) a.pass[a.n_pass++] = make_pass(a, 0, 0, a.ws.e_cur, tau_in, out_z, n_tau, (n * n_tau + 15) / 16, 0, 3);
    if (heads2) a.pass[a.n_pass++] = make_pass(a, 1, 0, a.ws.e_cur, nullptr, out_q, 1, (n_pad / 16) * heads, 0, 0);
    PRISM_CHECK_ARG(a.n_pass > 0, "nothing to run");
    rc = launch_fwd_tiles(a, stream);
    if (rc) return rc;
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// IDSActionSelector.generate_action_probs + select_action without random sampling (action_selectors.py:125-176).
extern "C" int prism_ids_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                                int32_t n_heads, float lmbda, float epsilon, float rho_lower_bound, int32_t unsquish_fn,
                                float *out_scores, float *out_aux, int64_t *out_action, int64_t *out_action_host,
                                prism_stream_t stream_) {
    PRISM_CHECK_ARG(z && q && out_scores && out_action, "null buffers");
    PRISM_CHECK_ARG(unsquish_fn >= PRISM_SQUISH_NONE && unsquish_fn <= PRISM_SQUISH_SYMLOG, "unknown unsquish function");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_tau >= 1 && n_actions >= 1 && n_actions <= 16 && n_heads >= 1, "bad sizes");
    const int stage = n_tau * n_actions <= ACT_STAGE_MAX_FLOATS;
    IdsArgs k{z, q, n, n_pad, n_tau, n_actions, n_heads, lmbda, epsilon, rho_lower_bound, out_scores, out_aux, out_action,
              out_action_host, stage, unsquish_fn};
    hipLaunchKernelGGL(ids_score_kernel, dim3(n), dim3(ACT_THREADS), stage ? (size_t)n_tau * n_actions * 4 : 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// GreedyActionSelector (action_selectors.py:70-83) on the buffers prism_act_forward filled.
extern "C" int prism_greedy_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                                   int32_t n_heads, int64_t *out_action, float *out_mean, int64_t *out_action_host,
                                   prism_stream_t stream_) {
    PRISM_CHECK_ARG((z || q) && out_action, "null buffers");
    PRISM_CHECK_ARG(n >= 1 && n_pad >= n && n_actions >= 1 && n_actions <= 16, "bad sizes");
    PRISM_CHECK_ARG(q ? n_heads >= 1 : n_tau >= 1, "bad sizes");
    const int stage = !q && n_tau * n_actions <= ACT_STAGE_MAX_FLOATS;
    GreedyArgs k{z, q, n, n_pad, n_tau, n_actions, n_heads, out_action, out_mean, out_action_host, stage};
    hipLaunchKernelGGL(greedy_select_kernel, dim3(n), dim3(ACT_THREADS), stage ? (size_t)n_tau * n_actions * 4 : 0, (hipStream_t)stream_, k);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// grid-norm partial slots valid for the Adam kernels: either what post left, or a fresh pass
static int prepare_norm(const LearnerPlan &pl, AdamArgs &a, hipStream_t stream) {
    if (a.grad_scale == 1.0f) {
        a.n_slots = pl.post_blocks;
    } else {
        // data parallel: the gradient was all-reduced after the backward; recompute the partials
        const int nb = 256;
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(nb), dim3(256), 0, stream, a.g, a.n, a.grad_scale, pl.ws.normpart);
        PRISM_CHECK_LAUNCH();
        a.n_slots = nb;
    }
    return PRISM_OK;
}

static int clip_step(const prism_learner_desc *ld, const prism_opt_hyper *opt, prism_stream_t stream_) {
    LearnerPlan pl;
    int rc = check_learner(ld, pl);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    AdamArgs a;
    fill_adam_args(ld, pl.ws, a);
    const int kind = opt ? opt->kind : PRISM_OPT_ADAM;
    if (opt) apply_opt(opt, a);
    rc = prepare_norm(pl, a, stream);
    if (rc) return rc;
    {
        ProfileScope ps_(K_CLIP_ADAM, stream);
        if (kind != PRISM_OPT_ADAM) return launch_clip_opt(kind, adam_blocks(a.n), stream, a);          // (opt_step.hip)
        hipLaunchKernelGGL(clip_adam_kernel, dim3(adam_blocks(a.n)), dim3(256), 0, stream, a);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_learner_clip_adam(const prism_learner_desc *ld, prism_stream_t stream_) {
    return clip_step(ld, nullptr, stream_);
}

extern "C" int prism_learner_clip_step(const prism_learner_desc *ld, const prism_opt_hyper *opt, prism_stream_t stream_) {
    int rc = check_opt(ld, opt);
    if (rc) return rc;
    return clip_step(ld, opt, stream_);
}

static int check_replay_for_step(const prism_learner_desc *ld, const prism_replay_desc *rp) {
    PRISM_CHECK_ARG(rp != nullptr, "null replay descriptor");
    PRISM_CHECK_ARG(rp->obs_elems == 100 * ld->dims.in_channels && (rp->obs_elems & 3) == 0,
                    "replay obs_elems must equal 10*10*C");
    PRISM_CHECK_ARG(rp->n_step >= 1 && rp->n_step <= PRISM_MAX_NSTEP, "n_step out of range");
    return PRISM_OK;
}

// the launch of prism_step_front / prism_step_front_ring and, with `cursor` set, of prism_step_front_cursor (`size` unused:
// the kernel reads it)
static int step_front(const prism_learner_desc *ld, const prism_replay_desc *rp, int32_t ring_kind, int64_t size,
                      const float *mass, uint64_t seed, uint64_t offset, float beta, int64_t *out_index, float *out_weight,
                      prism_stream_t stream_, const int64_t *cursor = nullptr, int32_t slot = 0) {
    LearnerPlan pl;
    int rc = check_learner(ld, pl);
    if (rc) return rc;
    rc = check_replay_for_step(ld, rp);
    if (rc) return rc;
    PRISM_CHECK_ARG(cursor || (size > 0 && size <= rp->capacity), "size must be in (0, capacity] (empty storage)");
    PRISM_CHECK_ARG(out_index && (rp->tree == nullptr || out_weight), "null outputs");
    hipStream_t stream = (hipStream_t)stream_;
    IqnArgs a;
    fill_iqn_args(ld, pl, a);
    FrontArgs f;
    f.size = cursor ? 1 : size;
    f.mass = mass;
    f.seed = seed;
    f.offset = offset;
    f.rng = ld->rng_counters;
    f.beta = beta;
    f.use_per = rp->tree != nullptr;
    f.out_index = out_index;
    f.out_weight = out_weight;
    f.obs = const_cast<float *>(ld->obs);
    f.next_obs = const_cast<float *>(ld->next_obs);
    f.reward = const_cast<float *>(ld->reward);
    f.gamma = const_cast<float *>(ld->gamma);
    f.nonterminal = const_cast<uint8_t *>(ld->nonterminal);
    f.action = const_cast<int64_t *>(ld->action);
    {
        ProfileScope ps_(K_FRONT, stream);
        const IqnArgs af = front_args(a);
        const int extra = front_extra_blocks(extra_dims(af));
        if (cursor)
            launch_front_cursor(ring_kind, ld->batch + extra, stream, af, *rp, f, cursor, slot);          // (front_cursor.hip)
        else if (ring_kind == PRISM_RING_U8)
            hipLaunchKernelGGL(step_front_byte_ring_kernel, dim3(ld->batch + extra), dim3(256), 0, stream, af, *rp, f);
        else
            hipLaunchKernelGGL(step_front_kernel, dim3(ld->batch + extra), dim3(256), 0, stream, af, *rp, f);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_step_front(const prism_learner_desc *ld, const prism_replay_desc *rp, int64_t size,
                                const float *mass, uint64_t seed, uint64_t offset, float beta, int64_t *out_index,
                                float *out_weight, prism_stream_t stream_) {
    return step_front(ld, rp, PRISM_RING_F32, size, mass, seed, offset, beta, out_index, out_weight, stream_);
}

extern "C" int prism_step_front_ring(const prism_learner_desc *ld, const prism_replay_desc *rp, int32_t ring_kind, int64_t size,
                                     const float *mass, uint64_t seed, uint64_t offset, float beta, int64_t *out_index,
                                     float *out_weight, prism_stream_t stream_) {
    PRISM_CHECK_ARG(ring_kind == PRISM_RING_F32 || ring_kind == PRISM_RING_U8,
                    "ring_kind must be PRISM_RING_F32 or PRISM_RING_U8");
    PRISM_CHECK_ARG(ring_kind != PRISM_RING_U8 || rp == nullptr ||
                        ((reinterpret_cast<uintptr_t>(rp->obs) | reinterpret_cast<uintptr_t>(rp->succ_obs)) & 3) == 0,
                    "a byte ring's obs / succ_obs must be 4-byte aligned");
    return step_front(ld, rp, ring_kind, size, mass, seed, offset, beta, out_index, out_weight, stream_);
}

// prism_step_front_ring with the ring's size read on the device (front_cursor.hip): size =
// min(cursor[slot], capacity).  `slot` is by value: a captured graph bakes it.
extern "C" int prism_step_front_cursor(const prism_learner_desc *ld, const prism_replay_desc *rp, int32_t ring_kind,
                                       const int64_t *cursor, int32_t slot, const float *mass, uint64_t seed,
                                       uint64_t offset, float beta, int64_t *out_index, float *out_weight,
                                       prism_stream_t stream_) {
    PRISM_CHECK_ARG(ring_kind == PRISM_RING_F32 || ring_kind == PRISM_RING_U8,
                    "ring_kind must be PRISM_RING_F32 or PRISM_RING_U8");
    PRISM_CHECK_ARG(ring_kind != PRISM_RING_U8 || rp == nullptr ||
                        ((reinterpret_cast<uintptr_t>(rp->obs) | reinterpret_cast<uintptr_t>(rp->succ_obs)) & 3) == 0,
                    "a byte ring's obs / succ_obs must be 4-byte aligned");
    PRISM_CHECK_ARG(cursor != nullptr, "null cursor");
    PRISM_CHECK_ARG(slot == 0 || slot == 1, "slot must be 0 or 1");
    PRISM_CHECK_ARG(rp == nullptr || (out_index && (rp->tree == nullptr || out_weight)), "null outputs");
    return step_front(ld, rp, ring_kind, 0, mass, seed, offset, beta, out_index, out_weight, stream_, cursor, slot);
}

static int step_back(const prism_learner_desc *ld, const prism_opt_hyper *opt, const prism_replay_desc *rp, const int64_t *index,
                     float alpha, float eps, prism_stream_t stream_) {
    LearnerPlan pl;
    int rc = check_learner(ld, pl);
    if (rc) return rc;
    rc = check_replay_for_step(ld, rp);
    if (rc) return rc;
    PRISM_CHECK_ARG(index != nullptr, "null index");
    hipStream_t stream = (hipStream_t)stream_;
    AdamArgs a;
    fill_adam_args(ld, pl.ws, a);
    const int kind = opt ? opt->kind : PRISM_OPT_ADAM;
    if (opt) apply_opt(opt, a);
    rc = prepare_norm(pl, a, stream);
    if (rc) return rc;
    BackArgs k;
    k.index = index;
    k.priority = ld->out_td;
    k.n = ld->batch;
    k.alpha = alpha;
    k.eps = eps;
    k.take_abs = 1;
    // fused_replay set: the writeback belongs to the learner's launches (post, finished below where it is split).  That holds
    // for fused_replay with a NULL fused_index too, where nothing rides along: then nobody writes priorities back.
    k.use_per = rp->tree != nullptr && !ld->fused_replay;
    k.plan = nullptr;
    k.sib = nullptr;
    k.sib_state = nullptr;
    if (pl.writeback_rides && pl.split_writeback) {
        k.plan = reinterpret_cast<const int4 *>(pl.ws.wb_plan);
        k.sib = reinterpret_cast<const float2 *>(pl.ws.sib);
        k.sib_state = pl.ws.ticket + 3;
    }
    k.rng = ld->rng_counters;
    k.inc_per = (uint64_t)ld->batch;
    k.inc_tau = (uint64_t)3 * pl.maxT * ld->batch;
    if (kind == PRISM_OPT_ADAM && tail_fused(pl)) {          // (check_opt refused fuse_tail with the other kinds)
        // single GPU: gradient reduction + clip + Adam + writeback in one launch
        IqnArgs ia;
        fill_iqn_args(ld, pl, ia);
        TailArgs t;
        t.adam = a;
        t.barrier = reinterpret_cast<unsigned long long *>(pl.ws.ticket + 4);
        t.status = pl.ws.ticket + PRISM_WS_STATUS_WORD;
        t.host_status = ld->host_status;
        t.rng = k.rng;
        t.inc_per = k.inc_per;
        t.inc_tau = k.inc_tau;
        rc = launch_post(ld, pl, ia, &t, stream);
        if (rc) return rc;
        if (k.use_per) {          // prioritised replay that is not riding in the learner's launches: its own update
            launch_per_update(*rp, index, ld->out_td, ld->batch, alpha, eps, 1, stream);
            PRISM_CHECK_LAUNCH();
        }
        return PRISM_OK;
    }
    {
        ProfileScope ps_(K_BACK, stream);
        if (kind != PRISM_OPT_ADAM) return launch_step_back_opt(kind, adam_blocks(a.n), stream, a, *rp, k);          // (opt_step.hip)
        hipLaunchKernelGGL(step_back_kernel, dim3(1 + adam_blocks(a.n)), dim3(256), 0, stream, a, *rp, k);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_step_back(const prism_learner_desc *ld, const prism_replay_desc *rp, const int64_t *index,
                               float alpha, float eps, prism_stream_t stream_) {
    return step_back(ld, nullptr, rp, index, alpha, eps, stream_);
}

extern "C" int prism_step_back_opt(const prism_learner_desc *ld, const prism_opt_hyper *opt, const prism_replay_desc *rp,
                                   const int64_t *index, float alpha, float eps, prism_stream_t stream_) {
    int rc = check_opt(ld, opt);
    if (rc) return rc;
    return step_back(ld, opt, rp, index, alpha, eps, stream_);
}
