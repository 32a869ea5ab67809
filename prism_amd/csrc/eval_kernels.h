// Device code of the evaluation tracker (prism_eval_track, include/prism_hip.h): the bookkeeping of the reference's
// SyncAgentEvaluator.evaluate_agent (/root/reference/prism/evals/sync_agent_evaluator.py:37-59) for N environment
// streams stepped in lockstep, without a host read.  ONE workgroup, passes of EP_PASS rows: per row in parallel the
// stream's running return and length; the ends of a pass are compacted in row order by the routine the collector's
// episode role uses (pass_compact, ingest_kernels.h) and ONE lane folds them in that order: the log is a list in
// (call, row) order and the two sums are float64 recurrences whose rounding order is the host's.  The build's
// -ffp-contract=off keeps the square and its sum separate roundings; they must not be written with fma.
#pragma once
#include "ingest_kernels.h"

namespace prism {

static __global__ __launch_bounds__(EP_PASS) void eval_track_kernel(prism_eval_desc ev, int32_t n, const float *reward,
                                                                    const uint8_t *done, const uint8_t *truncated) {
    __shared__ double s_ret[EP_PASS];
    __shared__ int32_t s_len[EP_PASS];
    __shared__ int s_wcnt[EP_PASS / 64];
    const int tid = threadIdx.x, bd = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, n_waves = bd >> 6;
    // the closing rule, read by every thread before the first barrier (lane 0 writes the words behind the last one):
    // the reference's loop condition `collected_ts < n_ts or len(ep_rews) == 0`, before the step
    const int64_t eps0 = ev.counts[0], rows0 = ev.counts[2];
    if (rows0 >= ev.budget && eps0 >= 1) {                           // closed: nothing is taken
        if (tid == 0 && ev.host_counts) {
            ev.host_counts[0] = eps0;
            ev.host_counts[1] = rows0;
        }
        return;
    }
    // lane 0 of wave 0 carries the finished-episode words through the passes
    int64_t c_eps = eps0, c_len = 0;
    double st_sum = 0.0, st_sq = 0.0, st_min = 0.0, st_max = 0.0;
    if (tid == 0) {
        c_len = ev.counts[1];
        st_sum = ev.stats[0];
        st_sq = ev.stats[1];
        st_min = ev.stats[2];
        st_max = ev.stats[3];
    }
    const int64_t log_cap = ev.log_capacity;
    for (int base = 0; base < n; base += bd) {
        const int i = base + tid;
        bool end = false;
        double ret = 0.0;
        int32_t len = 0;
        if (i < n) {                                                 // row i is stream i
            len = ev.ep_length[i] + 1;
            ret = (double)reward[i] + ev.ep_return[i];               // the first reward of an episode counts
            end = (done[i] | truncated[i]) != 0;
            ev.ep_return[i] = end ? 0.0 : ret;
            ev.ep_length[i] = end ? 0 : len;
        }
        int total;
        const int pos = pass_compact(__ballot(end), s_wcnt, lane, wave, n_waves, total);
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
    if (tid == 0) {
        ev.counts[0] = c_eps;
        ev.counts[1] = c_len;
        ev.counts[2] = rows0 + n;
        ev.counts[3] += 1;
        ev.stats[0] = st_sum;
        ev.stats[1] = st_sq;
        ev.stats[2] = st_min;
        ev.stats[3] = st_max;
        if (ev.host_counts) {
            ev.host_counts[0] = c_eps;
            ev.host_counts[1] = rows0 + n;
        }
    }
}

}  // namespace prism
