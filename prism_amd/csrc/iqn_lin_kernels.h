// The linear IQN head for gfx950 (iqn_quantile_model_layers = 0): no trunk between the quantile embedding and the head,
//   z = W2 . [LayerNorm(1024)]( ReLU(Wphi cos(pi k tau) + bphi) * e ) + b2
// (/root/reference/prism/agents/models/iqn_model.py:32-46 with self.model = None, :48-93).  Loss, target, double Q, target
// network and squish are those of the one-layer trunk (iqn_model.py:95-201).  IqnArgs.Hi == 0 IS "no trunk" to every
// kernel and role dispatcher (iqn_linear()).  The final LayerNorm's affine lives in off.iqn_ln2_*.
//
//   lin_fwd_tile   16 (sample, tau) rows per 256-thread workgroup, rows on chip: cos basis -> phi product (K = 64) -> bias,
//                  ReLU, * e -> LayerNorm(1024), two-pass moments -> head product (K = 1024, N = A padded to 16)
//   lin_loss       one workgroup per sample: the quantile-Huber loss of iqn_loss_body, leaving dz[R][16] and, with
//                  LayerNorm, the two row sums of its backward (c1 = dz . W2 g, c2 = dz . (z - b2 - W2 beta))
//   lin_bwd        workgroup = 16 embed columns x a row chunk: recomputes its columns of phi / xhat from the saved cos
//                  basis and row statistics, accumulates dWphi, dbphi, dW2, dg, dbeta with rows as the MFMA K dimension
//                  into the chunk's slab (flat-parameter order: the post launch's slab role sums the chunks), and owns
//                  d e[b][its columns] outright
//   lin_small      role of the post launch: db2 and the total loss
// Every product runs on v_mfma_f32_16x16x4_f32 (exact fp32 chain) for both gemm_mode values: K = 64 and N = 16 leave the
// bf16 pipe's three-piece form nothing to win that the operand splitting would not cost again.  No floating-point
// atomics: every sum has one owner and a fixed order.
#pragma once
#include "iqn_kernels.h"

namespace prism {

__host__ __device__ inline bool iqn_linear(int use_iqn, int Hi) { return use_iqn && Hi == 0; }
constexpr int LIN_AP = 16;          // action columns of dz / of the head product, padded
// gradient slab of one row chunk, in flat-parameter order: phi_w | phi_b | [ln_g | ln_b] | w2  (b2: lin_small_block)
__host__ __device__ inline int lin_slab_floats(int A, int ln) { return E_DIM * K_BASIS + E_DIM + (ln ? 2 * E_DIM : 0) + A * E_DIM; }
// a unit = the 16-row tiles one wave of the backward walks in a row: whole samples (T > 16: T / 16 tiles)
__host__ __device__ inline int lin_unit(int T) { return T > 16 ? T / 16 : 1; }
__host__ __device__ inline int lin_units(int B, int T) { return (B * T / 16) / lin_unit(T); }
// row chunks of the backward (four waves each): as many as give every wave a unit, eight at the most
__host__ __device__ inline int lin_chunks(int B, int T) {
    const int c = lin_units(B, T) / 4;
    return c < 1 ? 1 : (c > 8 ? 8 : c);
}

// ------------------------------------------------------------------------------------------
// forward tile.  MFMA 16x16x4 fp32: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15], D[i = 4(l>>4)+r][j = l&15].
//   Y^T[n][m] = Wphi[n][:] . cos[m][:]     A = Wphi rows (16 bytes of a row per lane and k group), B = cos tile (registers)
//   z^T[a][m] = W2[a][:] . y[m][:]         A = W2 rows, B = y: the D registers of the first product as they stand
// Wave w owns embed columns [256 w, 256 w + 256) and keeps its 16 x 256 inputs in registers between the two products
// (the row statistics need the whole row first).  LayerNorm moments in two passes over those registers: the mean from
// sums shifted by each lane's first element, then the squared deviations from that mean -- the shifted-moment form of
// fwd_kernels.h with the shift every row wants, affordable because nothing streams past: no E[x^2] - mean^2, and no
// (shift - mean)^2 terms either, which lose digits when a lane's first element is an outlier of a sparse row
// (tests/test_gpu_ln_stress.py; tests/test_gpu_iqn_linear.py).
// The four K slices of z fold through LDS in wave order.
// ------------------------------------------------------------------------------------------
struct LinFwLds {
    static constexpr unsigned PRO = 1u, STREAM = 2u, ROWS = 4u;
    static constexpr LdsRegion COST{0, 16 * CS, PRO};                               // [16][CS] cos basis of the tile's rows
    static constexpr LdsRegion TAU{COST.off + COST.size, 16, PRO};                  // quantile samples
    static constexpr LdsRegion STAT{TAU.off + TAU.size, 3 * 16 * 16, STREAM | ROWS};   // [shift | sum (x - shift) | sum (x - mean)^2][16 parts][16 rows]
    static constexpr LdsRegion ZP{STAT.off + STAT.size, 4 * 16 * 17, ROWS};         // [4 waves][16 actions][17]
    static constexpr int TOTAL = ZP.off + ZP.size;
    static constexpr LdsRegion ALL[] = {COST, TAU, STAT, ZP};
    static_assert(lds_layout_ok(ALL, TOTAL), "linear-head forward tile: LDS regions overlap");
    static_assert(COST.off % 4 == 0 && CS % 4 == 0, "16-byte accessed region");
};

template <bool LN>
__global__ __launch_bounds__(256) void lin_fwd_tile_kernel(IqnArgs a_by_value) {
    kernarg_prefetch<sizeof(IqnArgs)>();
    __shared__ __attribute__((aligned(16))) float smem[LinFwLds::TOTAL];
    typedef LinFwLds LD;
    float *cost = smem + LD::COST.off, *s_tau = smem + LD::TAU.off, *stat = smem + LD::STAT.off;
    float *zp = smem + LD::ZP.off;
    // the pass descriptor is read from the kernel-argument segment itself (fwd_kernels.h: a run-time index into the
    // by-value argument would move it to scratch)
    typedef const float __attribute__((address_space(1))) *gcf;
    typedef const f32x4 __attribute__((address_space(1))) *gcf4;
    typedef float __attribute__((address_space(1))) *gf;
    (void)a_by_value;
    const auto *kargs = (const __attribute__((address_space(4))) IqnArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const __attribute__((address_space(4))) IqnArgs &a = *kargs;
    int tile = blockIdx.x, pi = 0;
    const int n_pass = a.n_pass;
    int nt[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) nt[i] = a.pass[i].n_tiles;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const bool adv = (pi == i) & (i + 1 < n_pass) & (tile >= nt[i]);
        tile -= adv ? nt[i] : 0;
        pi += adv ? 1 : 0;
    }
    const __attribute__((address_space(4))) IqnPass *pp = &kargs->pass[pi];
    const gcf P = (gcf)pp->params, ps_e = (gcf)pp->e, ps_tau_in = (gcf)pp->tau_in;
    const gf ps_z_out = (gf)pp->z_out;
    const int T = pp->T, ps_save = pp->save, sid = pp->stream_id;
    const int A = a.A, Bt = a.Bt;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int64_t rows = (int64_t)Bt * T;        // rows that exist: the last tile of an acting pass may run past them
    const bool t_pow2 = (T & (T - 1)) == 0;
    const int tsh = 31 - __clz(T);
    // (rows past the end compute on the last sample's data and are not stored)
    auto sample_of = [&](int row) __attribute__((always_inline)) { return min(t_pow2 ? row >> tsh : row / T, Bt - 1); };

    unsigned long long rng_tau = 0ull;
    if (a.rng) rng_tau = ((const unsigned long long __attribute__((address_space(1))) *)a.rng)[1];
    // quantile samples of the 16 rows (same draw, same bits as cos_basis_block / fwd_tile_kernel), then their cos basis
    if (tid < 16) {
        const int row = tile * 16 + tid, b = sample_of(row), t = row - b * T;
        float tau;
        if (ps_tau_in) {
            tau = ps_tau_in[min((int64_t)t, (int64_t)T - 1) * Bt + b];
        } else {
            uint32_t rr[4];
            Philox ph(a.seed);
            ph(a.offset + rng_tau + (uint64_t)((int64_t)t * Bt + b), 0x54415530ull + (uint64_t)sid, rr);
            tau = u32_to_unit_float(rr[0]);
        }
        if (a.tau_out && t < T) a.tau_out[(int64_t)sid * a.maxT * Bt + (int64_t)t * Bt + b] = tau;
        s_tau[tid] = tau;
    }
    __syncthreads();
    for (int idx = tid; idx < 16 * K_BASIS; idx += 256) {
        const int m = idx >> 6, k = idx & 63;
        const float c = cosf((s_tau[m] * (float)(k + 1)) * PI_F);      // two fp32 multiplies as torch does (iqn_model.py:90-92)
        cost[m * CS + k] = c;
        if (ps_save) __builtin_nontemporal_store(c, &a.ws.cosb[((int64_t)tile * 16 + m) * K_BASIS + k]);   // the backward reads it
    }
    __syncthreads();
    f32x4 cosB[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cosB[q] = *reinterpret_cast<const f32x4 *>(&cost[li * CS + 16 * q + 4 * g]);

    // ---- phi product + epilogue: x[s][r] = input element (row li, column 256 w + 16 s + 4 g + r)
    const int myrow = tile * 16 + li, myb = sample_of(myrow);
    const gcf wphi = P + a.off.phi_w + (int64_t)(256 * w + li) * K_BASIS + 4 * g;
    const gcf erow = ps_e + (int64_t)myb * E_DIM + 256 * w + 4 * g;
    const gcf brow = P + a.off.phi_b + 256 * w + 4 * g;
    f32x4 x[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        f32x4 wq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wq[q] = *reinterpret_cast<gcf4>(wphi + (int64_t)s * 16 * K_BASIS + 16 * q);
        const f32x4 b4 = *reinterpret_cast<gcf4>(brow + 16 * s), e4 = *reinterpret_cast<gcf4>(erow + 16 * s);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = mfma16(wq[q][j], cosB[q][j], acc);
        // (the bias is added once, to the finished sum)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[s][r] = fmaxf(acc[r] + b4[r], 0.f) * e4[r];
    }

    float mean = 0.f, rstd = 1.f;
    if (LN) {
        // the whole row is on chip, so the moments take two passes: the mean from sums shifted by each lane's first element
        // (16 parts x 64 elements, parts added in part order by every lane alike), then the squares of the deviations FROM
        // THAT MEAN -- the shifted-moment form with the one shift that leaves nothing to cancel
        const float c = x[0][0];
        float s1 = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) s1 += x[s][r] - c;
        const int part = 4 * w + g;
        stat[(0 * 16 + part) * 16 + li] = c;
        stat[(1 * 16 + part) * 16 + li] = s1;
        __syncthreads();
        float sc = 0.f, ss = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) {
            sc += stat[(0 * 16 + p) * 16 + li];
            ss += stat[(1 * 16 + p) * 16 + li];
        }
        mean = sc * (1.0f / 16.0f) + ss * (1.0f / E_DIM);
        float s2 = 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float d = x[s][r] - mean;
                s2 += d * d;
            }
        stat[(2 * 16 + part) * 16 + li] = s2;
        __syncthreads();
        float m2 = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) m2 += stat[(2 * 16 + p) * 16 + li];
        rstd = 1.0f / sqrtf(m2 * (1.0f / E_DIM) + LN_EPS);
        if (ps_save && tid < 16) {          // (w = 0, g = 0: li = tid)
            a.ws.mu1[(int64_t)tile * 16 + tid] = mean;
            a.ws.rstd1[(int64_t)tile * 16 + tid] = rstd;
        }
    }

    // ---- head product over this wave's 256 columns
    const int la = min(li, A - 1);
    const float amask = li < A ? 1.f : 0.f;
    const gcf w2row = P + a.off.iqn_w2 + (int64_t)la * E_DIM + 256 * w + 4 * g;
    const gcf grow = P + (LN ? a.off.iqn_ln2_g : 0) + 256 * w + 4 * g, berow = P + (LN ? a.off.iqn_ln2_b : 0) + 256 * w + 4 * g;
    f32x4 accz = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        f32x4 w2v = *reinterpret_cast<gcf4>(w2row + 16 * s);
        f32x4 y = x[s];
        if (LN) {
            const f32x4 g4 = *reinterpret_cast<gcf4>(grow + 16 * s), be4 = *reinterpret_cast<gcf4>(berow + 16 * s);
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = ((x[s][r] - mean) * rstd) * g4[r] + be4[r];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) accz = mfma16(w2v[j] * amask, y[j], accz);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) zp[(w * 16 + 4 * g + r) * 17 + li] = accz[r];
    __syncthreads();
    {
        const int aa = tid >> 4, m = tid & 15;
        const int64_t row = (int64_t)tile * 16 + m;
        if (aa < A && row < rows) {
            const float z = ((zp[(0 * 16 + aa) * 17 + m] + zp[(1 * 16 + aa) * 17 + m]) + zp[(2 * 16 + aa) * 17 + m]) +
                            zp[(3 * 16 + aa) * 17 + m] + P[a.off.iqn_b2 + aa];
            ps_z_out[row * A + aa] = z;
        }
    }
}

// ------------------------------------------------------------------------------------------
// loss (iqn_model.py:95-201): one 256-thread workgroup per sample.  Wave 0 runs the argmax / n-step target / pairwise
// quantile-Huber tile exactly as iqn_loss_body does; the head's backward is one row of W2, so what is left per
// quantile row is dz (dq in the action's column), dq and -- with LayerNorm -- the row sums
//   c1 = sum_n dyhat = dq (W2 g)[act],    c2 = sum_n dyhat xhat = dq (z[act] - b2[act] - (W2 beta)[act])
// that let the column-sliced backward apply LayerNorm's backward without seeing the whole row.
// ------------------------------------------------------------------------------------------
template <bool LN>
__global__ __launch_bounds__(256) void lin_loss_kernel(IqnArgs a) {
    kernarg_prefetch<sizeof(IqnArgs)>();
    __shared__ float s_zc[64 * 16], s_zo[64 * 16], s_zt[64 * 16];
    __shared__ float s_y[64], s_q[64], s_tau[64], s_dq[64], s_uv[2][4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int b = blockIdx.x, B = a.B, A = a.A, T = a.T, Tn = a.Tn;
    const float kap = a.huber_k;
    const int act = (int)a.action[b];
    const float *P = a.params;
    if (LN) {
        const float4 w2 = *reinterpret_cast<const float4 *>(P + a.off.iqn_w2 + (int64_t)act * E_DIM + 4 * tid);
        const float4 gg = *reinterpret_cast<const float4 *>(P + a.off.iqn_ln2_g + 4 * tid);
        const float4 bb = *reinterpret_cast<const float4 *>(P + a.off.iqn_ln2_b + 4 * tid);
        const float u = wave_sum((w2.x * gg.x + w2.y * gg.y) + (w2.z * gg.z + w2.w * gg.w));
        const float v = wave_sum((w2.x * bb.x + w2.y * bb.y) + (w2.z * bb.z + w2.w * bb.w));
        if (lane == 0) {
            s_uv[0][w] = u;
            s_uv[1][w] = v;
        }
    }
    for (int i = tid; i < T * A; i += 256) s_zc[i] = a.ws.zcur[(int64_t)b * T * A + i];
    for (int i = tid; i < Tn * A; i += 256) {
        s_zo[i] = a.ws.zon[(int64_t)b * Tn * A + i];
        s_zt[i] = a.ws.ztg[(int64_t)b * Tn * A + i];
    }
    if (tid < T) s_tau[tid] = a.tau_out[(int64_t)tid * B + b];      // (slot 0: the current-state pass)
    __syncthreads();
    if (w == 0) {
        // a* = argmax_a mean_j Zon[j][a], first maximum wins (iqn_model.py:129-133)
        float mean = 0.f;
        {
            const int la = lane < A ? lane : 0;
            float sacc = 0.f;
            for (int j = 0; j < Tn; ++j) sacc += s_zo[j * A + la];
            mean = sacc / (float)Tn;
        }
        int astar = 0;
        float bestv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mean), 0));
#pragma unroll
        for (int aa = 1; aa < 16; ++aa) {
            const float m = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mean), aa));
            if (aa < A && m > bestv) {
                bestv = m;
                astar = aa;
            }
        }
        const float R = a.reward[b];
        const float dg = a.gamma[b] * (a.nonterminal[b] ? 1.0f : 0.0f);
        if (lane < Tn) s_y[lane] = td_target(a.squish, R, s_zt[lane * A + astar], dg);
        if (lane < T) s_q[lane] = s_zc[lane * A + act];
        __builtin_amdgcn_wave_barrier();
        // pairwise quantile-Huber tile: pair p = j*T + t; a lane keeps a fixed t because T | 64
        float lsum = 0.f, gq = 0.f;
        const int tsh = 31 - __clz(T);
        const int t_l = lane & (T - 1);
        const float q_l = s_q[t_l], tau_l = s_tau[t_l];
        for (int p = lane; p < T * Tn; p += 64) {
            const int j = p >> tsh;
            const float d = s_y[j] - q_l;
            const float ad = fabsf(d);
            const float hub = (ad <= kap) ? 0.5f * (d * d) : kap * (ad - 0.5f * kap);
            const float wgt = fabsf(tau_l - (d < 0.f ? 1.0f : 0.0f));
            lsum += (wgt * hub) / kap;
            const float cl = fminf(fmaxf(d, -kap), kap);
            gq += (wgt * cl) / kap;
        }
        lsum = wave_sum(lsum);
        for (int o = 32; o >= T; o >>= 1) gq += __shfl_xor(gq, o, 64);
        const float dl = (lsum / (float)Tn) * a.dist_w;
        const float wb = a.per_weights ? a.per_weights[b] : 1.0f;
        const float scale = -(wb / (float)B) * a.dist_w / (float)Tn;
        if (lane < T) s_dq[lane] = gq * scale;
        if (lane == 0) {
            a.out_dl[b] = dl;
            if (a.out_td) a.out_td[b] = dl;      // IQN only: td_errors = distribution_loss (composite_model.py:138-139)
            a.ws.lossw[b] = dl * wb;
        }
    }
    __syncthreads();
    float *dz = a.ws.dpre1;                      // [R][LIN_AP]
    for (int i = tid; i < T * LIN_AP; i += 256) {
        const int t = i >> 4, col = i & 15;
        __builtin_nontemporal_store(col == act ? s_dq[t] : 0.f, &dz[((int64_t)b * T + t) * LIN_AP + col]);
    }
    if (tid < T) {
        const int64_t r = (int64_t)b * T + tid;
        const float dq = s_dq[tid];
        a.ws.dq[r] = dq;
        if (LN) {
            const float u = (s_uv[0][0] + s_uv[0][1]) + (s_uv[0][2] + s_uv[0][3]);
            const float v = (s_uv[1][0] + s_uv[1][1]) + (s_uv[1][2] + s_uv[1][3]);
            a.ws.c1[r] = dq * u;
            a.ws.c2[r] = dq * ((s_zc[tid * A + act] - P[a.off.iqn_b2 + act]) - v);
        }
    }
}

// ------------------------------------------------------------------------------------------
// bwd: grid = 64 column slices x n_chunks row chunks, 256 threads = 4 waves; wave w of chunk rc walks the units
// rc * 4 + w, + 4 n_chunks, ...  Per 16-row tile, with D[i = m = 4 g + r][j = n = li] the layout of everything elementwise:
//   Y[m][n]      = cos[m][:] . Wphi[n][:]        A = cos rows (16-byte pieces), B = Wphi slice (registers)
//   dy[m][n]     = dz[m][:] . W2[:][n]           A = dz rows, B = W2 slice (registers)
//   dyhat = dy g;  dx = rstd (dyhat - c1 / 1024 - xhat c2 / 1024);  dY = dx e [Y + bphi > 0]       (LayerNorm off: dx = dy)
//   dWphi[n][k] += dY[m][n] cos[m][k]            A = dY: the D registers as they stand, B = cos (row on the k index)
//   dW2[a][n]   += dz[m][a] yin[m][n]            A = dz (row on the k index), B = the head's input: D registers again
//   dbphi, dg, dbeta: per-lane column sums;  d e[b][n] = sum_t dx phi: a unit holds whole samples, so the wave owns it
// The four waves' accumulators fold through LDS in wave order into the chunk's slab.
// ------------------------------------------------------------------------------------------
constexpr int LIN_BW_ACC = 16 + 4 + 3;       // dWphi (4 x 4) | dW2 (4) | dbphi, dg, dbeta
struct LinBwLds {
    static constexpr LdsRegion RED{0, 4 * LIN_BW_ACC * 64, LDS_ALWAYS};      // [4 waves][LIN_BW_ACC][64 lanes]
    static constexpr int TOTAL = RED.off + RED.size;
    static constexpr LdsRegion ALL[] = {RED};
    static_assert(lds_layout_ok(ALL, TOTAL), "linear-head backward: LDS regions overlap");
};

template <bool LN>
__global__ __launch_bounds__(256) void lin_bwd_kernel(IqnArgs a) {
    kernarg_prefetch<sizeof(IqnArgs)>();
    __shared__ __attribute__((aligned(16))) float s_red[LinBwLds::TOTAL];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int cs = blockIdx.x & (E_DIM / 16 - 1), rc = blockIdx.x / (E_DIM / 16), n0 = 16 * cs;
    const int B = a.B, A = a.A, T = a.T, tsh = 31 - __clz(T);
    const int unit = lin_unit(T), units_total = lin_units(B, T);
    const float *P = a.params;
    // the workgroup's weight slices, in operand order
    f32x4 wphi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) wphi[q] = *reinterpret_cast<const f32x4 *>(P + a.off.phi_w + (int64_t)(n0 + li) * K_BASIS + 16 * q + 4 * g);
    float w2s[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int aa = 4 * g + j;
        const float v = P[a.off.iqn_w2 + (int64_t)min(aa, A - 1) * E_DIM + n0 + li];
        w2s[j] = aa < A ? v : 0.f;
    }
    const float bph = P[a.off.phi_b + n0 + li];
    const float gn = LN ? P[a.off.iqn_ln2_g + n0 + li] : 1.f, ben = LN ? P[a.off.iqn_ln2_b + n0 + li] : 0.f;

    f32x4 accW[4], accW2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) accW[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbp = 0.f, dgs = 0.f, dbs = 0.f;

    for (int u = rc * 4 + w; u < units_total; u += 4 * a.n_chunks) {
        float de_acc = 0.f;
        const int bs = (u * unit * 16 + 4 * g) >> tsh;           // sample of this lane's four rows (T >= 4: one sample)
        const float ev = a.ws.e_cur[(int64_t)bs * E_DIM + n0 + li];
        for (int tt = 0; tt < unit; ++tt) {
            const int64_t row0 = ((int64_t)u * unit + tt) * 16;
            f32x4 cosA[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) cosA[q] = *reinterpret_cast<const f32x4 *>(a.ws.cosb + (row0 + li) * K_BASIS + 16 * q + 4 * g);
            const f32x4 dzA = *reinterpret_cast<const f32x4 *>(a.ws.dpre1 + (row0 + li) * LIN_AP + 4 * g);
            float cosK[4][4], dzK[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int q = 0; q < 4; ++q) cosK[q][r] = a.ws.cosb[(row0 + 4 * g + r) * K_BASIS + 16 * q + li];
                dzK[r] = a.ws.dpre1[(row0 + 4 * g + r) * LIN_AP + li];
            }
            f32x4 mu4 = {0.f, 0.f, 0.f, 0.f}, rs4 = {1.f, 1.f, 1.f, 1.f}, c14 = mu4, c24 = mu4;
            if (LN) {
                mu4 = *reinterpret_cast<const f32x4 *>(a.ws.mu1 + row0 + 4 * g);
                rs4 = *reinterpret_cast<const f32x4 *>(a.ws.rstd1 + row0 + 4 * g);
                c14 = *reinterpret_cast<const f32x4 *>(a.ws.c1 + row0 + 4 * g);
                c24 = *reinterpret_cast<const f32x4 *>(a.ws.c2 + row0 + 4 * g);
            }
            f32x4 Y = {0.f, 0.f, 0.f, 0.f}, DY = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) Y = mfma16(cosA[q][j], wphi[q][j], Y);
#pragma unroll
            for (int j = 0; j < 4; ++j) DY = mfma16(dzA[j], w2s[j], DY);
            float dYp[4], yin[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pre = Y[r] + bph, phi = fmaxf(pre, 0.f), xv = phi * ev;
                float dx;
                if (LN) {
                    const float xh = (xv - mu4[r]) * rs4[r];
                    const float dyh = DY[r] * gn;
                    dx = rs4[r] * ((dyh - c14[r] * (1.0f / E_DIM)) - xh * (c24[r] * (1.0f / E_DIM)));
                    yin[r] = xh * gn + ben;
                    dgs += DY[r] * xh;
                    dbs += DY[r];
                } else {
                    dx = DY[r];
                    yin[r] = xv;
                }
                dYp[r] = pre > 0.f ? dx * ev : 0.f;
                dbp += dYp[r];
                de_acc += dx * phi;
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) accW[q] = mfma16(dYp[r], cosK[q][r], accW[q]);
#pragma unroll
            for (int r = 0; r < 4; ++r) accW2 = mfma16(dzK[r], yin[r], accW2);
        }
        if (a.propagate_grad) {
            // rows of one sample: 4 (one lane group), 8 (two), 16 and more (all four, over the unit's tiles)
            if (T >= 8) de_acc += __shfl_xor(de_acc, 16, 64);
            if (T >= 16) de_acc += __shfl_xor(de_acc, 32, 64);
            const bool owner = T == 4 || (T == 8 ? (g & 1) == 0 : g == 0);
            if (owner) __builtin_nontemporal_store(de_acc, &a.ws.de_iqn[(int64_t)bs * E_DIM + n0 + li]);
        }
    }

    // ---- fold the four waves in wave order; slab of this chunk in flat-parameter order
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[(w * LIN_BW_ACC + 4 * q + r) * 64 + lane] = accW[q][r];
#pragma unroll
    for (int r = 0; r < 4; ++r) s_red[(w * LIN_BW_ACC + 16 + r) * 64 + lane] = accW2[r];
    s_red[(w * LIN_BW_ACC + 20) * 64 + lane] = dbp;
    s_red[(w * LIN_BW_ACC + 21) * 64 + lane] = dgs;
    s_red[(w * LIN_BW_ACC + 22) * 64 + lane] = dbs;
    __syncthreads();
    auto fold = [&](int slot, int ln_) __attribute__((always_inline)) {
        return ((s_red[(0 * LIN_BW_ACC + slot) * 64 + ln_] + s_red[(1 * LIN_BW_ACC + slot) * 64 + ln_]) +
                s_red[(2 * LIN_BW_ACC + slot) * 64 + ln_]) + s_red[(3 * LIN_BW_ACC + slot) * 64 + ln_];
    };
    float *slab = a.ws.slabs + (int64_t)rc * a.slab;
    // d phi_w[n0 + nl][k]: accumulator q = k >> 4 of lane ((nl >> 2), k & 15), element nl & 3
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int o = tid + 256 * i, nl = o >> 6, k = o & 63;
        __builtin_nontemporal_store(fold(4 * (k >> 4) + (nl & 3), (nl >> 2) * 16 + (k & 15)), &slab[(int64_t)(n0 + nl) * K_BASIS + k]);
    }
    const int o_pb = E_DIM * K_BASIS, o_w2 = o_pb + E_DIM + (LN ? 2 * E_DIM : 0);
    {
        const int aa = tid >> 4, nl = tid & 15;
        if (aa < A) __builtin_nontemporal_store(fold(16 + (aa & 3), (aa >> 2) * 16 + nl), &slab[o_w2 + (int64_t)aa * E_DIM + n0 + nl]);
    }
    if (tid < (LN ? 48 : 16)) {
        const int which = tid >> 4, nl = tid & 15;
        const float t = ((fold(20 + which, nl) + fold(20 + which, 16 + nl)) + fold(20 + which, 32 + nl)) + fold(20 + which, 48 + nl);
        __builtin_nontemporal_store(t, &slab[o_pb + which * E_DIM + n0 + nl]);
    }
}

// ------------------------------------------------------------------------------------------
// post role (one 1024-thread workgroup): d b2[a] = sum_rows dz[row][a] (64 row parts folded in part order) and the total
// loss mean_b(dl_b w_b) (agent.py:58-64).  `pool`: 1024 + 16 floats of LDS.
// ------------------------------------------------------------------------------------------
constexpr int LIN_SMALL_POOL_FLOATS = 1024 + 16;
__device__ __forceinline__ void lin_small_block(const IqnArgs &a, float &sq, float *pool) {
    const int tid = threadIdx.x, col = tid & 15, part = tid >> 4;
    const int64_t R = (int64_t)a.B * a.T;
    float s = 0.f;
    for (int64_t r = part; r < R; r += 64) s += a.ws.dpre1[r * LIN_AP + col];
    float lw = 0.f;
    for (int b = tid; b < a.B; b += 1024) lw += a.ws.lossw[b];
    lw = wave_sum(lw);
    pool[tid] = s;
    if ((tid & 63) == 0) pool[1024 + (tid >> 6)] = lw;
    __syncthreads();
    if (tid < a.A) {
        float t = 0.f;
#pragma unroll 16
        for (int p = 0; p < 64; ++p) t += pool[p * 16 + tid];
        far_store(&a.grads[a.off.iqn_b2 + tid], t);
        sq += t * t;
    }
    if (tid == 0) {
        float l = 0.f;
#pragma unroll
        for (int p = 0; p < 16; ++p) l += pool[1024 + p];
        l = l / (float)a.B;
        a.out_scalars[1] = l;
        a.out_scalars[0] = l;
        a.out_scalars[2] = 0.f;
    }
}

}  // namespace prism
