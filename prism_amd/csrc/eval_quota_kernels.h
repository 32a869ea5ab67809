// Device code of the quota rule of the evaluation tracker (prism_eval_track_quota, include/prism_hip.h): every stream
// contributes exactly its first `quota` finished episodes, a stream that has met the quota is masked out, and the
// evaluation closes when every stream has met it (or after max_calls taken calls).  The shape is eval_track_kernel's
// (eval_kernels.h): ONE workgroup, passes of EP_PASS rows, the ends of a pass compacted in row order by pass_compact
// (ingest_kernels.h) and folded by ONE lane with the same float64 recurrences.  What is new is per-stream state beyond
// the open episode (ep_done) and two counts a pass adds to: the live rows and the streams that met the quota.  Both are
// integer sums, so the order of the per-wave additions does not show.  The build's -ffp-contract=off keeps the square
// and its sum separate roundings; they must not be written with fma.
//
// Who reads what whom writes: the closing words (qcounts[0], counts[3]) are read by every thread in front of the first
// barrier and written by lane 0 behind the last one; ep_done[i], ep_return[i] and ep_length[i] are read and written by
// row i's own thread only; everything else in global memory is lane 0's.
#pragma once
#include "ingest_kernels.h"

namespace prism {

static __global__ __launch_bounds__(EP_PASS) void eval_track_quota_kernel(prism_eval_desc ev, prism_eval_quota q, int32_t n,
                                                                          const float *reward, const uint8_t *done,
                                                                          const uint8_t *truncated) {
    __shared__ double s_ret[EP_PASS];
    __shared__ int32_t s_len[EP_PASS];
    __shared__ int s_wcnt[EP_PASS / 64];
    __shared__ int s_live, s_met;
    const int tid = threadIdx.x, bd = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = bd >> 6;
    // the closing rule, read by every thread before the first barrier (lane 0 writes the words behind the last one)
    const int64_t met0 = q.qcounts[0], calls0 = ev.counts[3];
    if (met0 >= ev.n_streams || calls0 >= q.max_calls) {             // closed: nothing is taken
        if (tid == 0) {
            if (ev.host_counts) {
                ev.host_counts[0] = ev.counts[0];
                ev.host_counts[1] = ev.counts[2];
            }
            if (q.host_closed) q.host_closed[0] = 1;
        }
        return;
    }
    // lane 0 of wave 0 carries the finished-episode words through the passes
    int64_t c_eps = 0, c_len = 0;
    double st_sum = 0.0, st_sq = 0.0, st_min = 0.0, st_max = 0.0;
    if (tid == 0) {
        c_eps = ev.counts[0];
        c_len = ev.counts[1];
        st_sum = ev.stats[0];
        st_sq = ev.stats[1];
        st_min = ev.stats[2];
        st_max = ev.stats[3];
        s_live = 0;                                                  // first added to behind pass_compact's barrier
        s_met = 0;
    }
    const int64_t log_cap = ev.log_capacity;
    const int32_t quota = q.quota;
    for (int base = 0; base < n; base += bd) {
        const int i = base + tid;
        bool live = false, end = false, met = false;
        double ret = 0.0;
        int32_t len = 0;
        if (i < n) {                                                 // row i is stream i
            const int32_t had = q.ep_done[i];
            live = had < quota;                                      // a row that is not live is not touched, nor read
            if (live) {
                len = ev.ep_length[i] + 1;
                ret = (double)reward[i] + ev.ep_return[i];           // the first reward of an episode counts
                end = (done[i] | truncated[i]) != 0;
                ev.ep_return[i] = end ? 0.0 : ret;
                ev.ep_length[i] = end ? 0 : len;
                if (end) {
                    q.ep_done[i] = had + 1;
                    met = had + 1 == quota;
                }
            }
        }
        const unsigned long long lives = __ballot(live), mets = __ballot(met);
        int total;
        const int pos = pass_compact(__ballot(end), s_wcnt, lane, wave, n_waves, total);
        if (lane == 0) {
            if (lives) atomicAdd(&s_live, __popcll(lives));
            if (mets) atomicAdd(&s_met, __popcll(mets));
        }
        if (end) {
            s_ret[pos] = ret;
            s_len[pos] = len;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < total; ++k) {
                const double r = s_ret[k];
                const int32_t l = s_len[k];
                if (c_eps < log_cap) {
                    ev.log_return[c_eps] = r;
                    ev.log_length[c_eps] = l;
                }
                const double sq = r * r;
                st_sum += r;
                st_sq += sq;
                if (c_eps == 0) {
                    st_min = r;
                    st_max = r;
                } else {
                    if (r < st_min) st_min = r;
                    if (r > st_max) st_max = r;
                }
                c_eps += 1;
                c_len += l;
            }
        }
        __syncthreads();                                             // the lists and counts are free for the next pass
    }
    if (tid == 0) {                                                  // behind the last barrier: every wave's sums are in
        const int64_t rows = ev.counts[2] + s_live, met_now = met0 + s_met;
        ev.counts[0] = c_eps;
        ev.counts[1] = c_len;
        ev.counts[2] = rows;
        ev.counts[3] = calls0 + 1;
        ev.stats[0] = st_sum;
        ev.stats[1] = st_sq;
        ev.stats[2] = st_min;
        ev.stats[3] = st_max;
        q.qcounts[0] = met_now;
        if (ev.host_counts) {
            ev.host_counts[0] = c_eps;
            ev.host_counts[1] = rows;
        }
        if (q.host_closed) q.host_closed[0] = (met_now >= ev.n_streams || calls0 + 1 >= q.max_calls) ? 1 : 0;
    }
}

}  // namespace prism
