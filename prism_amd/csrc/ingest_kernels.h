// Device code of the vectorised producer seam: one step of N environment streams -> ring rows, links and default
// priorities in ONE launch (prism_replay_ingest, include/prism_hip.h).  Row semantics as the reference's collector
// derives them (/root/reference/multiprocessing_experience_collection/collector_process_interface.py:154-169) and as
// HipReplayBuffer.extend() restates them row by row; the block routines come from replay_kernels.h.
//
// Roles by workgroup, no data shared between them (so no cross-workgroup wait):
//   workgroup 0        plan (predecessor of every row from the stream table) + link + default priority
//   workgroups 1 ..    row store: copy / widen the observations, reward (clipped, tracked launch), action, flags
//   last workgroup     (tracked launch only, prism_replay_ingest_tracked) episode returns + the training-reward EMA
// The stream table holds, per stream, the WRITE SERIAL of the stream's open row (or -1).  A ring slot is reused exactly
// every `capacity` writes, so "the open row is still in the ring" is `serial0 + i - w < capacity` and its slot is
// `w % capacity`: no per-slot owner array, no host dict.
#pragma once
#include "replay_kernels.h"

namespace prism {

constexpr int INGEST_MAX_STREAMS = 65536;
constexpr int INGEST_ROW_THREADS = 128;             // threads that share one row in the row-store role
constexpr int INGEST_MAX_ROW_WGS = 2048;
// LDS of the plan workgroup: two bitmaps over the stream ids (seen in this call / seen twice), dead before the tree
// writer takes the pool over (a workgroup barrier separates the two).
constexpr unsigned IG_PLAN = 8u;
constexpr LdsRegion IG_SEEN{0, INGEST_MAX_STREAMS / 8, IG_PLAN};
constexpr LdsRegion IG_DUP{INGEST_MAX_STREAMS / 8, INGEST_MAX_STREAMS / 8, IG_PLAN};
constexpr LdsRegion IG_REGIONS[] = {TW_SORTED, TW_VAL, TW_PART, TW_KEYS, TW_REC, TW_DENSE, IG_SEEN, IG_DUP};
static_assert(lds_layout_ok(IG_REGIONS, TREE_WRITE_LDS_BYTES), "ingest: the bitmaps do not fit the tree writer's pool");

struct IngestArgs {
    int32_t n, n_streams, obs_kind, vec;            // vec: 16-byte (fp32) / 4-byte (uint8) row accesses are aligned, both sides
    int64_t first_slot, serial0;
    const void *obs, *next_obs;                     // [n][obs_elems] fp32 (obs_kind 0) or uint8 (obs_kind 1)
    const float *reward;
    const int32_t *action;
    const uint8_t *done, *truncated;
    const int32_t *stream_ids;                      // NULL: row i belongs to stream i
    int64_t *stream_tab;                            // [n_streams]
    float alpha, eps;
};

// The two bitmaps of one call's stream ids, by the whole workgroup (zeroed here; a barrier must follow before they are
// read).  True for a thread that met an id outside the table or one already seen.
// (tid, bd and the grid's shape are read by the two kernels and handed down to these routines: read in a kernel they are
// plain words of the dispatch, read in a function the compiler also emits the partial-last-workgroup form of blockDim.)
static __device__ __forceinline__ bool ingest_mark_streams(const int32_t *ids, int n, int n_streams, uint32_t *s_seen,
                                                           uint32_t *s_dup, int tid, int bd) {
    for (int w = tid; w < (n_streams + 31) >> 5; w += bd) {
        s_seen[w] = 0u;
        s_dup[w] = 0u;
    }
    __syncthreads();
    bool flag = false;
    for (int i = tid; i < n; i += bd) {
        const int32_t sid = ids[i];
        if ((uint32_t)sid >= (uint32_t)n_streams) {                  // outside the table: stored unlinked, table untouched
            flag = true;
            continue;
        }
        const uint32_t bit = 1u << (sid & 31);
        if (atomicOr(&s_seen[sid >> 5], bit) & bit) {
            atomicOr(&s_dup[sid >> 5], bit);
            flag = true;
        }
    }
    return flag;
}

// The row-order compaction of one pass, shared with the evaluation tracker (eval_kernels.h): `flagged` = __ballot(flag)
// of the caller's wave.  Every thread of the workgroup calls it; it holds ONE workgroup barrier (what lane 0 of a wave
// wrote in front of the call is visible behind it).  Returns the position of a flagged row among the pass's flagged
// rows in row order (only meaningful where flag is set) and their number in `total`.  s_wcnt: n_waves ints, free again
// after the caller's next barrier.
static __device__ __forceinline__ int pass_compact(unsigned long long flagged, int *s_wcnt, int lane, int wave,
                                                   int n_waves, int &total) {
    if (lane == 0) s_wcnt[wave] = __popcll(flagged);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int w = 0; w < n_waves; ++w) {
        const int c = s_wcnt[w];
        before += w < wave ? c : 0;
        total += c;
    }
    return before + __popcll(flagged & ((1ull << lane) - 1ull));
}

// ---- episode role: one workgroup, the last of the tracked launch.  It reads the call's arguments and its own four
// arrays only -- nothing the other roles write -- and rebuilds the id bitmaps for itself, so it waits on nobody.
// Passes of blockDim.x rows.  Per row in parallel (the ids of a call are distinct): the stream's running return and
// length; a row with done | truncated is an episode end.  The ends of a pass are compacted in ROW ORDER (ballot +
// per-wave counts) and ONE lane folds them in that order: the EMA is a sequential recurrence in float64 whose rounding
// order is the host's (the reference folds timesteps as they reach the buffer).  The build's -ffp-contract=off keeps its
// two products and the sum separate roundings; it must not be written with fma.
constexpr int EP_PASS = 1024;
static __device__ __forceinline__ void ingest_episode_role(const IngestArgs &a, const prism_episode_desc &ep, char *s_pool,
                                                           int tid, int bd) {
    __shared__ double s_ret[EP_PASS];
    __shared__ int32_t s_len[EP_PASS];
    __shared__ int s_wcnt[EP_PASS / 64];
    __shared__ int s_tracked;
    if (!ep.ep_return) return;                                       // clip without tracking
    const int lane = tid & 63, wave = tid >> 6, n_waves = bd >> 6;
    const int n = a.n, n_streams = a.n_streams;
    const int32_t *ids = a.stream_ids;
    uint32_t *s_seen = reinterpret_cast<uint32_t *>(s_pool + IG_SEEN.off);
    uint32_t *s_dup = reinterpret_cast<uint32_t *>(s_pool + IG_DUP.off);
    if (tid == 0) s_tracked = 0;
    if (ids) ingest_mark_streams(ids, n, n_streams, s_seen, s_dup, tid, bd);      // (workgroup 0 owns the status bit)
    __syncthreads();
    const bool count_first = ep.count_first_step != 0;
    const double ema = ep.ema;
    // lane 0 of wave 0 carries the finished-episode words through the passes
    int64_t c_eps = 0, c_len = 0;
    double st_ema = 0.0, st_sum = 0.0, st_last = 0.0;
    if (tid == 0) {
        c_eps = ep.counts[0];
        c_len = ep.counts[1];
        st_ema = ep.stats[0];
        st_sum = ep.stats[1];
        st_last = ep.stats[2];
    }
    for (int base = 0; base < n; base += bd) {
        const int i = base + tid;
        bool end = false, tracked = false;
        double ret = 0.0;
        int32_t len = 0;
        if (i < n) {
            int32_t s = i;
            bool closed = false;                                     // a repeated stream: in the table, not tracked
            if (ids) {
                const int32_t sid = ids[i];
                if ((uint32_t)sid >= (uint32_t)n_streams) {
                    s = -1;
                } else if ((s_dup[sid >> 5] >> (sid & 31)) & 1u) {
                    s = sid;
                    closed = true;
                } else {
                    s = sid;
                }
            }
            if (s >= 0 && closed) {                                  // (every row of it writes the same zeros)
                ep.ep_return[s] = 0.0;
                ep.ep_length[s] = 0;
            } else if (s >= 0) {
                tracked = true;
                const int32_t had = ep.ep_length[s];
                len = had + 1;
                ret = (had == 0 && !count_first) ? 0.0 : (double)a.reward[i] + ep.ep_return[s];
                end = (a.done[i] | a.truncated[i]) != 0;
                ep.ep_return[s] = end ? 0.0 : ret;
                ep.ep_length[s] = end ? 0 : len;
            }
        }
        const unsigned long long ends = __ballot(end), trk = __ballot(tracked);
        if (lane == 0 && trk) atomicAdd(&s_tracked, __popcll(trk));
        int total;
        const int pos = pass_compact(ends, s_wcnt, lane, wave, n_waves, total);
        if (end) {
            s_ret[pos] = ret;
            s_len[pos] = len;
        }
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < total; ++k) {
                const double r = s_ret[k];
                st_ema = c_eps == 0 ? r : ema * st_ema + (1.0 - ema) * r;
                st_sum += r;
                st_last = r;
                c_eps += 1;
                c_len += s_len[k];
            }
        }
        __syncthreads();                                             // the lists and counts are free for the next pass
    }
    if (tid == 0) {
        ep.counts[0] = c_eps;
        ep.counts[1] = c_len;
        ep.counts[2] += s_tracked;
        ep.stats[0] = st_ema;
        ep.stats[1] = st_sum;
        ep.stats[2] = st_last;
    }
}

// TRACKED: the launch of prism_replay_ingest_tracked -- one more workgroup behind the row stores, a reward clip in them.
// RING: the storage kind of rp.obs / rp.succ_obs (prism_replay_ingest_ring); only the row-store role knows it.
template <bool TRACKED, int RING = PRISM_RING_F32>
static __device__ __forceinline__ void replay_ingest_body(const prism_replay_desc &rp, const IngestArgs &a,
                                                          const prism_episode_desc &ep, const int tid, const int bd,
                                                          const unsigned wg, const unsigned n_wgs) {
    __shared__ __attribute__((aligned(16))) char s_pool[TREE_WRITE_LDS_BYTES];
    __shared__ int s_serial;
    const int n = a.n;
    const int64_t cap = rp.capacity, first = a.first_slot;
    const unsigned row_wgs = n_wgs - (TRACKED ? 2u : 1u);

    if constexpr (TRACKED) {
        if (wg == n_wgs - 1) {
            ingest_episode_role(a, ep, s_pool, tid, bd);
            return;
        }
    }
    if (wg != 0) {
        // ---- row store: INGEST_ROW_THREADS threads per row, blockDim / INGEST_ROW_THREADS rows per workgroup and trip
        const int O = rp.obs_elems;
        const int per_wg = bd / INGEST_ROW_THREADS, lane = tid % INGEST_ROW_THREADS;
        const int64_t stride = (int64_t)(row_wgs)*per_wg;
        [[maybe_unused]] bool inexact = false;                       // (byte ring: a float that was not byte-exact)
        for (int64_t i = (int64_t)(wg - 1) * per_wg + tid / INGEST_ROW_THREADS; i < n; i += stride) {
            const int64_t s = (first + i) % cap;
            const bool done = a.done[i] != 0, trunc = a.truncated[i] != 0;
            const bool has_next = trunc || !done;
            if constexpr (RING == PRISM_RING_F32) {
                float *d0 = rp.obs + s * O, *d1 = rp.succ_obs + s * O;
                if (a.obs_kind == 0) {
                    const float *s0 = static_cast<const float *>(a.obs) + i * O;
                    const float *s1 = static_cast<const float *>(a.next_obs) + i * O;
                    if (a.vec) {
                        for (int k = lane; k < O / 4; k += INGEST_ROW_THREADS) {
                            const float4 v0 = reinterpret_cast<const float4 *>(s0)[k];
                            float4 v1 = make_float4(0.f, 0.f, 0.f, 0.f);
                            if (has_next) v1 = reinterpret_cast<const float4 *>(s1)[k];
                            reinterpret_cast<float4 *>(d0)[k] = v0;
                            reinterpret_cast<float4 *>(d1)[k] = v1;
                        }
                    } else {
                        for (int k = lane; k < O; k += INGEST_ROW_THREADS) {
                            d0[k] = s0[k];
                            d1[k] = has_next ? s1[k] : 0.f;
                        }
                    }
                } else {
                    const uint8_t *s0 = static_cast<const uint8_t *>(a.obs) + i * O;
                    const uint8_t *s1 = static_cast<const uint8_t *>(a.next_obs) + i * O;
                    if (a.vec) {
                        for (int k = lane; k < O / 4; k += INGEST_ROW_THREADS) {
                            const uint32_t w0 = reinterpret_cast<const uint32_t *>(s0)[k];
                            uint32_t w1 = 0u;
                            if (has_next) w1 = reinterpret_cast<const uint32_t *>(s1)[k];
                            reinterpret_cast<float4 *>(d0)[k] = make_float4((float)(w0 & 255u), (float)((w0 >> 8) & 255u),
                                                                            (float)((w0 >> 16) & 255u), (float)(w0 >> 24));
                            reinterpret_cast<float4 *>(d1)[k] = make_float4((float)(w1 & 255u), (float)((w1 >> 8) & 255u),
                                                                            (float)((w1 >> 16) & 255u), (float)(w1 >> 24));
                        }
                    } else {
                        for (int k = lane; k < O; k += INGEST_ROW_THREADS) {
                            d0[k] = (float)s0[k];
                            d1[k] = has_next ? (float)s1[k] : 0.f;
                        }
                    }
                }
            } else if (a.obs_kind == 0) {
                // fp32 rows into a byte ring: narrowed (obs_narrow; a float that is not byte-exact is stored as 0)
                uint8_t *d0 = reinterpret_cast<uint8_t *>(rp.obs) + s * O, *d1 = reinterpret_cast<uint8_t *>(rp.succ_obs) + s * O;
                const float *s0 = static_cast<const float *>(a.obs) + i * O;
                const float *s1 = static_cast<const float *>(a.next_obs) + i * O;
                if (a.vec) {
                    for (int k = lane; k < O / 4; k += INGEST_ROW_THREADS) {
                        const float4 v0 = reinterpret_cast<const float4 *>(s0)[k];
                        float4 v1 = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (has_next) v1 = reinterpret_cast<const float4 *>(s1)[k];
                        reinterpret_cast<uint32_t *>(d0)[k] = obs_narrow4(v0, inexact);
                        reinterpret_cast<uint32_t *>(d1)[k] = obs_narrow4(v1, inexact);
                    }
                } else {
                    for (int k = lane; k < O; k += INGEST_ROW_THREADS) {
                        d0[k] = (uint8_t)obs_narrow(s0[k], inexact);
                        d1[k] = (uint8_t)obs_narrow(has_next ? s1[k] : 0.f, inexact);
                    }
                }
            } else {
                // uint8 / bool rows into a byte ring: copied, a 32-bit word per thread where the rows start on words
                uint8_t *d0 = reinterpret_cast<uint8_t *>(rp.obs) + s * O, *d1 = reinterpret_cast<uint8_t *>(rp.succ_obs) + s * O;
                const uint8_t *s0 = static_cast<const uint8_t *>(a.obs) + i * O;
                const uint8_t *s1 = static_cast<const uint8_t *>(a.next_obs) + i * O;
                if (a.vec) {
                    for (int k = lane; k < O / 4; k += INGEST_ROW_THREADS) {
                        const uint32_t w0 = reinterpret_cast<const uint32_t *>(s0)[k];
                        uint32_t w1 = 0u;
                        if (has_next) w1 = reinterpret_cast<const uint32_t *>(s1)[k];
                        reinterpret_cast<uint32_t *>(d0)[k] = w0;
                        reinterpret_cast<uint32_t *>(d1)[k] = w1;
                    }
                } else {
                    for (int k = lane; k < O; k += INGEST_ROW_THREADS) {
                        d0[k] = s0[k];
                        d1[k] = has_next ? s1[k] : (uint8_t)0;
                    }
                }
            }
            if (lane == 0) {
                float r = a.reward[i];
                if constexpr (TRACKED) {                             // NaN and -0.0 fail both compares: stored as they are
                    if (ep.reward_clip == PRISM_CLIP_CLAMP) r = r < -1.f ? -1.f : (r > 1.f ? 1.f : r);
                }
                rp.reward[s] = r;
                rp.action[s] = a.action[i];
                rp.flags[s] = (uint8_t)((done ? PRISM_FLAG_DONE : 0u) | (trunc ? PRISM_FLAG_TRUNC : 0u) |
                                        (has_next ? PRISM_FLAG_HAS_NEXT : 0u));
            }
        }
        if constexpr (RING == PRISM_RING_U8) {
            if (inexact) atomicOr(rp.status, PRISM_STATUS_OBS_INEXACT);
        }
        return;
    }

    // ---- plan + link + default priority: one workgroup ----------------------------------------------------------------
    uint32_t *s_seen = reinterpret_cast<uint32_t *>(s_pool + IG_SEEN.off);
    uint32_t *s_dup = reinterpret_cast<uint32_t *>(s_pool + IG_DUP.off);
    const int32_t *ids = a.stream_ids;
    const int n_streams = a.n_streams;
    const int64_t serial0 = a.serial0;
    int64_t *tab = a.stream_tab;
    if (tid == 0) s_serial = 0;
    if (ids) {                                                       // (identity ids cannot repeat: no bitmap pass)
        if (ingest_mark_streams(ids, n, n_streams, s_seen, s_dup, tid, bd))
            atomicOr(rp.status, PRISM_STATUS_INGEST_DUP_STREAM);
    }
    __syncthreads();
    // stream of row i, or -1 when the row is stored unlinked (id outside the table / id repeated in this call)
    auto stream_of = [&](int i) __attribute__((always_inline)) -> int32_t {
        if (!ids) return i;
        const int32_t sid = ids[i];
        if ((uint32_t)sid >= (uint32_t)n_streams) return -1;
        return (s_dup[sid >> 5] >> (sid & 31)) & 1u ? -1 : sid;
    };
    // slot of the row's predecessor as the table has it on entry, or -1
    auto pred_of = [&](int i) __attribute__((always_inline)) -> int32_t {
        const int32_t sid = stream_of(i);
        if (sid < 0) return -1;
        const int64_t w = tab[sid];
        if (w < 0 || w >= serial0 + i) return -1;
        if (serial0 + i - w >= cap) return -1;                       // its slot has been written again since
        return (int32_t)(w % cap);
    };
    {
        bool bad = false;
        for (int i = tid; i < n; i += bd) {
            const int32_t p = pred_of(i);
            if (p >= 0) {
                const int64_t pos = ((int64_t)p - first + cap) % cap;
                // predecessor overwritten later in this call.  (pos < i cannot happen: a live predecessor has
                // serial0 + i - w < cap, so the row of this call that reuses its slot, w + cap - serial0, comes after row i.)
                if (pos < n && pos >= i) bad = true;
            }
        }
        if (bad) s_serial = 1;
    }
    __syncthreads();
    if (s_serial) {
        if (tid == 0) {
            for (int i = 0; i < n; ++i) {                            // the sequential loop itself (replay_link_kernel)
                const int32_t s = (int32_t)((first + i) % cap);
                const int32_t b = rp.back[s];
                if (b >= 0 && rp.link[b] == s) rp.link[b] = -1;
                const int32_t q = rp.link[s];
                if (q >= 0 && rp.back[q] == s) rp.back[q] = -1;
                rp.link[s] = -1;
                rp.back[s] = -1;
                const int32_t p = pred_of(i);
                if (p >= 0) {
                    rp.link[p] = s;
                    rp.back[s] = p;
                }
            }
        }
    } else {
        for (int i = tid; i < n; i += bd) {                          // A  detach the overwritten rows' old neighbours
            const int32_t s = (int32_t)((first + i) % cap);
            const int32_t b = rp.back[s], q = rp.link[s];
            if (b >= 0 && rp.link[b] == s) rp.link[b] = -1;
            if (q >= 0 && rp.back[q] == s) rp.back[q] = -1;
        }
        __syncthreads();
        for (int i = tid; i < n; i += bd) {                          // B  reset the slots' own link / back
            const int32_t s = (int32_t)((first + i) % cap);
            rp.link[s] = -1;
            rp.back[s] = -1;
        }
        __syncthreads();
        for (int i = tid; i < n; i += bd) {                          // C  attach each row to its predecessor
            const int32_t p = pred_of(i);
            if (p >= 0) {
                const int32_t s = (int32_t)((first + i) % cap);
                rp.link[p] = s;
                rp.back[s] = p;
            }
        }
    }
    __syncthreads();                                                 // every reader of the table's old state is through
    for (int i = tid; i < n; i += bd) {                              // D  the stream's open row is this one, or none
        const int32_t raw = ids ? ids[i] : i;
        if ((uint32_t)raw >= (uint32_t)n_streams) continue;
        const bool open = stream_of(i) >= 0 && a.done[i] == 0 && a.truncated[i] == 0;
        tab[raw] = open ? serial0 + i : -1;                          // (a repeated id: every row of it writes -1)
    }
    if (!rp.tree) return;
    const float prio = pow_alpha(rp.per_state[0] + a.eps, a.alpha);
    const int pass = min(UPD_MAX, bd);
    for (int base = 0; base < n; base += pass) {
        const int cnt = min(pass, n - base);
        __syncthreads();                                             // bitmaps / previous pass: LDS free
        const int32_t me = tid < cnt ? (int32_t)((first + base + tid) % cap) : 0;
        block_tree_write(rp, me, prio, cnt, s_pool);
    }
}

static __global__ __launch_bounds__(1024) void replay_ingest_kernel(prism_replay_desc rp, IngestArgs a) {
    replay_ingest_body<false>(rp, a, prism_episode_desc{}, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

static __global__ __launch_bounds__(1024) void replay_ingest_tracked_kernel(prism_replay_desc rp, IngestArgs a,
                                                                            prism_episode_desc ep) {
    replay_ingest_body<true>(rp, a, ep, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

// The two launches for a byte ring (prism_replay_ingest_ring with PRISM_RING_U8): the same roles, the row stores byte-wide.
static __global__ __launch_bounds__(1024) void byte_ring_ingest_kernel(prism_replay_desc rp, IngestArgs a) {
    replay_ingest_body<false, PRISM_RING_U8>(rp, a, prism_episode_desc{}, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

static __global__ __launch_bounds__(1024) void byte_ring_ingest_tracked_kernel(prism_replay_desc rp, IngestArgs a,
                                                                               prism_episode_desc ep) {
    replay_ingest_body<true, PRISM_RING_U8>(rp, a, ep, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

// ---- the cursor form (prism_replay_ingest_cursor): the ring cursor is read from device memory, so a captured launch
// writes other slots on every replay.  cursor[2] is a pair of words in ping-pong: this launch READS cursor[slot] -- the
// write serial of its first row -- and one lane WRITES cursor[slot ^ 1] = serial0 + n, an ordinary store.  No thread reads
// the word the launch writes and none writes the word it reads, so every workgroup sees the same serial0 whenever it
// runs; the next launch is handed the other `slot` and sees the advanced word across the kernel boundary.  A negative
// serial0 (nothing on the host could refuse it): the ring is left alone, the word is passed on, the sticky bit is raised.
struct IngestCursor {
    int64_t *cursor;                                // device, [2]
    int32_t slot;                                   // 0 | 1: the word this launch reads
};

// The four words that differ from the by-value launch are handed to the body in a copy of the argument struct made of
// scalars (never indexed, never addressed past inlining: it stays in registers like the kernel arguments themselves).
template <bool TRACKED, int RING>
static __device__ __forceinline__ void cursor_ingest_body(const prism_replay_desc &rp, const IngestArgs &a,
                                                                 const prism_episode_desc &ep, const IngestCursor &c,
                                                                 const int tid, const int bd, const unsigned wg,
                                                                 const unsigned n_wgs) {
    const int64_t serial0 = c.cursor[c.slot];
    if (serial0 < 0) {
        if (wg == 0 && tid == 0) {
            c.cursor[c.slot ^ 1] = serial0;
            atomicOr(rp.status, PRISM_STATUS_INGEST_BAD_CURSOR);
        }
        return;
    }
    if (wg == 0 && tid == 0) c.cursor[c.slot ^ 1] = serial0 + a.n;
    IngestArgs b = a;
    b.serial0 = serial0;
    b.first_slot = serial0 % rp.capacity;
    replay_ingest_body<TRACKED, RING>(rp, b, ep, tid, bd, wg, n_wgs);
}

static __global__ __launch_bounds__(1024) void cursor_ingest_kernel(prism_replay_desc rp, IngestArgs a,
                                                                           IngestCursor c) {
    cursor_ingest_body<false, PRISM_RING_F32>(rp, a, prism_episode_desc{}, c, threadIdx.x, blockDim.x, blockIdx.x,
                                                     gridDim.x);
}

static __global__ __launch_bounds__(1024) void cursor_ingest_tracked_kernel(prism_replay_desc rp, IngestArgs a,
                                                                                   prism_episode_desc ep, IngestCursor c) {
    cursor_ingest_body<true, PRISM_RING_F32>(rp, a, ep, c, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

static __global__ __launch_bounds__(1024) void byte_ring_cursor_ingest_kernel(prism_replay_desc rp, IngestArgs a,
                                                                              IngestCursor c) {
    cursor_ingest_body<false, PRISM_RING_U8>(rp, a, prism_episode_desc{}, c, threadIdx.x, blockDim.x, blockIdx.x,
                                                    gridDim.x);
}

static __global__ __launch_bounds__(1024) void byte_ring_cursor_ingest_tracked_kernel(prism_replay_desc rp, IngestArgs a,
                                                                                      prism_episode_desc ep,
                                                                                      IngestCursor c) {
    cursor_ingest_body<true, PRISM_RING_U8>(rp, a, ep, c, threadIdx.x, blockDim.x, blockIdx.x, gridDim.x);
}

}  // namespace prism
