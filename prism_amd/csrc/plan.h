// The learner's plan: everything an entry point of learner.hip decides from the descriptor before it launches -- the
// envelope, the form of every launch of the step, its grid sizes and the layout of the workspace.  One make_plan() per call:
// Python changes the descriptor in place between calls (fuse_tail, fused_replay, hyper-parameters), so no plan outlives
// its call.  Host code only; learner.hip includes it after the kernel headers, whose predicates (bw3_ok, qb2_ok,
// post_blocks, ...) it asks in ONE place each.
#pragma once
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace prism {

// ---- workspace carving -----------------------------------------------------------------------
struct Carver {
    char *base;
    size_t off;
    explicit Carver(void *b) : base((char *)b), off(0) {}
    float *f(size_t n) {
        float *p = base ? (float *)(base + off) : nullptr;
        off += ((n + 3) / 4) * 16;   // n floats rounded up to 16 bytes
        return p;
    }
};

// backward decomposition (iqn_bwd_kernel) into row chunks x 64 column slices: width 128, two workgroups per CU share
// each SIMD (8 row chunks); width 256, one workgroup per CU (4 row chunks)
static constexpr int MAX_CHUNKS = 16;
static int bwd_chunks(int H) { return H == 128 ? 8 : 4; }      // workgroups per CU x 4

static bool width_ok(int h) { return h == 128 || h == 256; }

// Forward GEMMs: 1 = exact fp32 chain (v_mfma_f32_16x16x4_f32), 2 = three-piece bf16 operands on v_mfma_f32_16x16x32_bf16
// (fp32 accuracy, common.h).  prism_learner_desc.gemm_mode picks one, 0 = the library default (PRISM_GEMM=fp32|bf16x3
// overrides it; read once per process).
static int default_gemm_mode() {
    static const int mode = [] {
        const char *e = getenv("PRISM_GEMM");
        if (e && !strcmp(e, "fp32")) return 1;
        if (e && !strcmp(e, "bf16x3")) return 2;
        return PRISM_GEMM_DEFAULT;
    }();
    return mode;
}

static int iqn_supported(const prism_model_dims *d, int32_t B) {
    auto pow2_ok = [](int t) { return t == 4 || t == 8 || t == 16 || t == 32 || t == 64; };
    if (!d->use_iqn && d->n_heads == 0) return PRISM_ERR_UNSUPPORTED;
    if (d->embed_dim != E_DIM) return PRISM_ERR_UNSUPPORTED;
    if (d->squish_fn < PRISM_SQUISH_NONE || d->squish_fn > PRISM_SQUISH_SYMLOG) return PRISM_ERR_UNSUPPORTED;
    if (d->use_iqn) {
        if (d->n_basis != K_BASIS) return PRISM_ERR_UNSUPPORTED;
        if (d->iqn_layers == 0) {
            // the linear head (iqn_lin_kernels.h): no trunk, so iqn_width is ignored as the reference ignores it; no Q heads
            // beside it (the two-layer ensemble would need the merged loss launch and the de_q sum: not built)
            if (d->n_heads != 0) return PRISM_ERR_UNSUPPORTED;
        } else if (d->iqn_layers != 1 || !width_ok(d->iqn_width)) {
            return PRISM_ERR_UNSUPPORTED;
        }
        if (!pow2_ok(d->n_tau) || !pow2_ok(d->n_tau_next)) return PRISM_ERR_UNSUPPORTED;
        if ((B * d->n_tau) % 16 || (B * d->n_tau_next) % 16) return PRISM_ERR_UNSUPPORTED;
    }
    if (d->n_heads != 0) {
        // ensemble / DQN heads of the form [LN] -> Linear(1024,H) -> ReLU -> [LN] -> Linear(H,A)
        if (d->head_layers == 1) {
            // single Linear(1024 -> A) DQN head, with or without LayerNorm, no IQN beside it
            if (d->n_heads != 1 || d->use_iqn) return PRISM_ERR_UNSUPPORTED;
        } else {
            if (d->n_heads < 0 || d->n_heads > Q_MAX_HEADS || d->head_layers != 2 || !width_ok(d->head_width))
                return PRISM_ERR_UNSUPPORTED;
            if (B % 16) return PRISM_ERR_UNSUPPORTED;
        }
    }
    if (B < 1 || B > SMALL_MAX_B) return PRISM_ERR_UNSUPPORTED;
    if (d->n_actions < 1 || d->n_actions > 16 || d->in_channels < 1 || d->in_channels > 10) return PRISM_ERR_UNSUPPORTED;
    return PRISM_OK;
}

// the IQN trunk's backward: none (no IQN) | iqn_bwd_kernel | the 64-column bf16 form of width 128 (bwd3_kernels.h; the forward
// then saves ReLU(phi)) | its width-256 form (bwd4_kernels.h: pairs of waves share 16 columns, one hidden half each)
// | lin_bwd_kernel of the linear head (no trunk)
enum BwdForm { BWD_NONE, BWD_FP32, BWD_BW3, BWD_BW4, BWD_LIN };
// the two-layer Q heads' input-side backward: none | qh_bwd_kernel by rows | by columns (B <= 128: a wave per column slice
// over all rows) | two shared-operand GEMMs on the bf16 pipe (qbwd2_kernels.h)
enum QBwdForm { QB_NONE, QB_ROWS, QB_COLS, QB_QB2 };

struct LearnerPlan {
    int Hi, Hq;                // hidden width of the IQN trunk / of the Q heads (128 where the part is absent; Hi == 0: an IQN
                               // without a trunk, the linear head)
    bool lin;                  // ... that one: lin_fwd_tile / lin_loss / lin_bwd launches, post + back behind them
    int split;                 // forward GEMMs on the bf16 matrix pipe
    BwdForm bwd;
    int n_chunks, conv_in_bwd, conv_rows;
    int local_loss;            // the IQN loss finishes inside the forward tiles (kind 2): no loss launch
    int merged_loss;           // IQN and ensemble loss in one launch (loss_both_kernel)
    int loss_waves;            // waves of iqn_loss_kernel's workgroup
    QBwdForm q_bwd;
    int q_de_slots;            // slots of ws.de_q the post launch sums: one per head, or the two K halves of qh_bwd2_kernel
    int slab, q_slab, maxT;
    int post_blocks;           // workgroups of the post launch (without the writeback's) = grid-norm partials it leaves
    bool writeback_rides;      // the priority writeback is one more block of the post launch
    bool split_writeback;      // ... in two halves: preparation there, level walk beside clip + Adam (back launch,
                               // 256-thread workgroups: one leaf per thread)
    bool post_dense;           // ... recomputing the top of the tree whole (tree_dense_finish)
    bool tail_wanted;          // the fused tail is asked for and worth it (learner.hip tail_fused adds: and fits this device)
    IqnWs ws;
    float *tau_buf, *dl_buf;   // stand-ins for tau_out / out_dist_loss | out_q_loss when the caller binds none
    size_t ws_bytes;
};

// the workspace layout: every buffer of `p.ws` at its offset from `base` (NULL: sizes alone)
static void carve(const prism_model_dims &d, int B, void *base, LearnerPlan &p) {
    Carver c(base);
    const size_t R = (size_t)B * d.n_tau, Rn = (size_t)B * d.n_tau_next, A = d.n_actions;
    const size_t Hi = p.Hi, Hq = p.Hq;
    const int ln = d.use_layer_norm;
    IqnWs &w = p.ws;
    w.ticket = (unsigned int *)c.f(8);     // first 32 bytes: the self-resetting tickets (zeroed once by the caller)
    w.e_cur = c.f((size_t)B * E_DIM);
    w.e_next = c.f((size_t)B * E_DIM);
    w.uv = c.f(2 * UV_ROWS * Hi);
    w.wpk[0] = c.f(iqn_pack_split_floats((int)Hi));      // (the larger of the two layouts: fp32 stream order / bf16 pieces)
    w.wpk[1] = c.f(iqn_pack_split_floats((int)Hi));
    w.cosb = c.f(R * K_BASIS);
    w.cospk = (unsigned int *)c.f((size_t)((R + 2 * Rn + 15) / 16 + 3) * CP_TILE);
    w.phis = c.f(p.lin ? 0 : ((R + 15) / 16) * 16 * (size_t)E_DIM);
    w.mu1 = c.f(R);
    w.rstd1 = c.f(R);
    w.pre1 = c.f(R * Hi);
    w.xhat2 = c.f(R * Hi);
    w.rstd2 = c.f(R);
    w.zcur = c.f(R * A);
    w.zon = c.f(Rn * A);
    w.ztg = c.f(Rn * A);
    w.dq = c.f(R);
    w.c1 = c.f(R);
    w.c2 = c.f(R);
    w.dpre1 = c.f(p.lin ? R * LIN_AP : R * Hi);      // (linear head: dz[R][LIN_AP])
    w.Sb = c.f((size_t)B * Hi);
    w.Pb = c.f((size_t)B * Hi);
    w.Db = c.f(B);
    w.lossw = c.f(B);
    w.de_iqn = c.f((size_t)B * E_DIM);
    w.slabs = c.f((size_t)MAX_CHUNKS * p.slab);
    {
        const size_t post_rows = (size_t)((B + 3) / 4) * CONV_ROW;      // (post_conv_blocks(B, C) <= this)
        const size_t bwd_rows = (size_t)(E_DIM / 16) * MAX_CHUNKS * BWD_CONV_ROW;
        const size_t dqn_rows = d.head_layers == 1 && d.n_heads ? (size_t)B * CONV_ROW : 0;   // one row per sample
        w.convpart = c.f(std::max({post_rows, bwd_rows, dqn_rows}));
    }
    w.normpart = c.f(NORM_SLOTS);
    w.sib = c.f((size_t)TREE_MAX_LEVELS * B * 2);
    w.wb_plan = c.f((size_t)B * 4);
    {
        const size_t Hd = d.n_heads, RQ = Hd * (size_t)B;
        w.q_mu1 = c.f(RQ);
        w.q_rstd1 = c.f(RQ);
        w.q_pre1 = c.f(RQ * Hq);
        w.q_xhat2 = c.f(RQ * Hq);
        w.q_rstd2 = c.f(RQ);
        w.zq_cur = c.f(RQ * A);
        w.zq_on = c.f(RQ * A);
        w.zq_tg = c.f(RQ * A);
        w.q_dq = c.f(RQ);
        w.q_c1 = c.f(RQ);
        w.q_c2 = c.f(RQ);
        w.q_dpre1 = c.f(RQ * Hq);
        w.q_pp = (unsigned short *)c.f(RQ * Hq * 3 / 2);
        w.q_xp = (unsigned short *)c.f((size_t)B * E_DIM * 3 / 2);
        w.q_lossw = c.f(B);
        w.q_uv = c.f(2 * Hd * UV_ROWS * Hq);
        w.q_kappa = c.f(Q_MAX_HEADS * Q_NORM_PARTS);
        w.q_wpk[0] = c.f(Hd * (size_t)q_pack_split_floats((int)Hq));
        w.q_wpk[1] = c.f(d.has_target ? Hd * (size_t)q_pack_split_floats((int)Hq) : 0);
        w.de_q = c.f(Hd * (size_t)B * E_DIM);      // (one slot for the single-Linear DQN head)
        w.q_slabs = c.f(Hd * (size_t)q_slab_floats((int)Hq, ln));
    }
    p.tau_buf = c.f(3 * (size_t)p.maxT * B);
    p.dl_buf = c.f(2 * (size_t)B);       // per-sample dl | ql (the post launch reads both)
    p.ws_bytes = c.off;
}

// `d`, `B`: inside the envelope (iqn_supported).  `fused_replay` / `fused_index` / `fuse_tail` / `grad_scale` as in the
// descriptor; a caller that only sizes the workspace passes none of them.
static LearnerPlan make_plan(const prism_model_dims &d, int B, int gemm_mode = 0, void *workspace = nullptr,
                             const prism_replay_desc *fused_replay = nullptr, const int64_t *fused_index = nullptr,
                             int fuse_tail = 0, float grad_scale = 1.0f) {
    LearnerPlan p;
    memset(&p, 0, sizeof(p));
    const bool heads2 = d.n_heads && d.head_layers == 2;
    p.lin = d.use_iqn && d.iqn_layers == 0;
    p.Hi = p.lin ? 0 : d.use_iqn ? d.iqn_width : 128;
    p.Hq = heads2 ? d.head_width : 128;
    const int mode = gemm_mode == PRISM_GEMM_FP32 || gemm_mode == PRISM_GEMM_BF16X3 ? gemm_mode : default_gemm_mode();
    // (the linear head's products run the fp32 chain in both modes: iqn_lin_kernels.h)
    p.split = mode == PRISM_GEMM_BF16X3 && ((d.use_iqn && !p.lin) || heads2);
    p.slab = p.lin ? lin_slab_floats(d.n_actions, d.use_layer_norm) : iqn_slab_floats(p.Hi, d.use_layer_norm);
    p.q_slab = q_slab_floats(p.Hq, d.use_layer_norm);
    p.maxT = std::max(d.n_tau, d.n_tau_next);
    // the IQN backward and what depends on it: row chunks (gradient slabs), who folds the conv backward, in how many rows
    p.conv_rows = 4;
    if (p.lin) {
        p.bwd = BWD_LIN;
        p.n_chunks = lin_chunks(B, d.n_tau);
        p.conv_in_bwd = 0;          // (d e is final per (sample, column) there: the post launch's conv role takes it)
    } else if (d.use_iqn && p.split && bw3_ok(p.Hi, B, d.n_tau, true)) {
        p.bwd = BWD_BW3;
        p.n_chunks = BW3_RC;
        p.conv_in_bwd = bw3_conv_ok(d.use_iqn, d.n_heads, d.propagate_grad, d.n_tau, d.in_channels, B);
        p.conv_rows = 1;
    } else if (d.use_iqn && p.split && bw4_ok(p.Hi, B, d.n_tau)) {
        p.bwd = BWD_BW4;
        p.n_chunks = bw4_chunks(B, d.n_tau);
        p.conv_in_bwd = 0;
    } else {
        p.bwd = d.use_iqn ? BWD_FP32 : BWD_NONE;
        p.n_chunks = bwd_chunks(p.Hi);
        p.conv_in_bwd = bwd_conv_ok(d.use_iqn, d.n_heads, d.propagate_grad, d.n_tau, d.in_channels, B, p.n_chunks, p.Hi);
    }
    // the IQN loss finishes inside the forward tiles when current- and next-state rows of a sample run through the SAME
    // weights (no target network) and a 16-row tile holds whole samples (2 T <= 16)
    p.local_loss = d.use_iqn && !p.lin && !d.has_target && d.n_tau_next == d.n_tau && d.n_tau <= 8;
    p.loss_waves = loss_waves(d.n_tau);
    p.merged_loss = d.use_iqn && !p.local_loss && heads2 && p.Hi == p.Hq && p.loss_waves == LOSS_WAVES;
    p.q_bwd = !heads2 ? QB_NONE : p.split && qb2_ok(p.Hq, B, d.n_heads, d.head_layers) ? QB_QB2 : B <= 128 ? QB_COLS : QB_ROWS;
    p.q_de_slots = p.q_bwd == QB_QB2 ? 2 : d.n_heads;
    p.post_blocks = d.head_layers == 1 && d.n_heads
                        ? post_blocks_dqn1(d.in_channels)
                    : p.lin      // conv role | slab sums | lin_small_block
                        ? post_conv_blocks(B, d.in_channels) + post_slab_blocks(p.slab, p.n_chunks) + 1
                        : post_blocks(B, d.in_channels, d.use_iqn, d.n_heads, p.conv_in_bwd != 0, p.slab, p.q_slab, p.Hi, p.Hq, p.n_chunks);
    p.writeback_rides = fused_replay && fused_replay->tree && fused_index;
    p.split_writeback = B <= 256;
    // the full writer's live threads: 2 x the batch rounded up to waves (iqn_post_kernel)
    const int wb_live = B <= UPD_MAX ? std::min(1024, 2 * ((B + 63) & ~63)) : 1024;
    p.post_dense = p.writeback_rides && tree_dense_ok(fused_replay->tree_capacity, B, wb_live);
    // The fused tail wants nothing between the gradient and the optimizer step (no all-reduce: grad_scale 1) and something
    // to hide behind its grid barrier: a priority writeback riding along (measured without, uniform replay + one-layer DQN
    // head: 32.7 us fused vs 30.1 us as two launches) or an IQN's gradient slabs (additive ablation base, uniform replay,
    // width 256: 95.5 vs 97.3 us per step).
    // (The linear head takes the post + back pair: the fused tail has not been measured for it.)
    p.tail_wanted = fuse_tail && grad_scale == 1.0f && (p.writeback_rides || d.use_iqn) && !p.lin;
    carve(d, B, workspace, p);
    return p;
}

}  // namespace prism
