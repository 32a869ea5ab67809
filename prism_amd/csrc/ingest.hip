// Host entry points of the vectorised producer seam (C ABI in include/prism_hip.h).
#include <cmath>

#include "ingest_kernels.h"

using namespace prism;

// The checks both entry points run (a macro: the message names the entry point that was called).  In two halves around
// the cursor's own: the cursor form (prism_replay_ingest_cursor) reads the cursor on the device and runs the halves alone.
#define INGEST_CHECK_SHAPE()                                                                                            \
    do {                                                                                                                \
        int rc = check_ring(rp, false);                                                                                 \
        if (rc) return rc;                                                                                              \
        PRISM_CHECK_ARG(!rp->tree || rp->tree_capacity <= (1ll << TREE_MAX_LEVELS),                                     \
                        "prioritized capacity above 2^24 - 1 rows");                                                    \
        PRISM_CHECK_ARG(n >= 1 && n <= rp->capacity, "n must be in [1, capacity]");                                     \
        PRISM_CHECK_ARG(n_streams >= 1 && n_streams <= INGEST_MAX_STREAMS, "n_streams must be in [1, 65536]");          \
        PRISM_CHECK_ARG(obs_kind == PRISM_OBS_F32 || obs_kind == PRISM_OBS_U8,                                          \
                        "obs_kind must be PRISM_OBS_F32 or PRISM_OBS_U8");                                              \
    } while (0)

#define INGEST_CHECK_ARRAYS()                                                                                           \
    do {                                                                                                                \
        PRISM_CHECK_ARG(obs && next_obs && reward && action && done && truncated, "null transition array");             \
        PRISM_CHECK_ARG(stream_tab != nullptr, "null stream_tab");                                                      \
        PRISM_CHECK_ARG(stream_ids != nullptr || n <= n_streams,                                                        \
                        "stream_ids NULL (row i is stream i) needs n <= n_streams");                                    \
    } while (0)

#define INGEST_CHECK_ARGS()                                                                                             \
    do {                                                                                                                \
        INGEST_CHECK_SHAPE();                                                                                           \
        PRISM_CHECK_ARG(first_slot >= 0 && first_slot < rp->capacity, "first_slot must be in [0, capacity)");           \
        PRISM_CHECK_ARG(serial0 >= 0 && serial0 % rp->capacity == first_slot,                                           \
                        "serial0 must be >= 0 and serial0 % capacity == first_slot");                                   \
        INGEST_CHECK_ARRAYS();                                                                                          \
    } while (0)

// ... and what the tracked launch adds on its episode descriptor
#define INGEST_CHECK_EPISODES()                                                                                         \
    do {                                                                                                                \
        PRISM_CHECK_ARG(ep->reward_clip == PRISM_CLIP_NONE || ep->reward_clip == PRISM_CLIP_CLAMP,                      \
                        "reward_clip must be PRISM_CLIP_NONE or PRISM_CLIP_CLAMP");                                     \
        PRISM_CHECK_ARG(std::isfinite(ep->ema) && ep->ema >= 0.0 && ep->ema <= 1.0, "ema must be finite and in [0, 1]"); \
        const int set = (ep->ep_return != nullptr) + (ep->ep_length != nullptr) + (ep->stats != nullptr) +              \
                        (ep->counts != nullptr);                                                                        \
        PRISM_CHECK_ARG(set == 0 || set == 4, "ep_return, ep_length, stats and counts must be all set or all NULL");    \
        PRISM_CHECK_ARG(ep->count_first_step == 0 || ep->count_first_step == 1, "count_first_step must be 0 or 1");     \
    } while (0)

namespace {

struct IngestLaunch {
    IngestArgs a;
    int threads, row_wgs;
};

IngestLaunch ingest_plan(const prism_replay_desc *rp, int32_t n, int64_t first_slot, int64_t serial0, const void *obs,
                         const void *next_obs, int32_t obs_kind, const float *reward, const int32_t *action,
                         const uint8_t *done, const uint8_t *truncated, const int32_t *stream_ids, int64_t *stream_tab,
                         int32_t n_streams, float alpha, float eps, int32_t ring_kind = PRISM_RING_F32) {
    IngestLaunch L;
    IngestArgs &a = L.a;
    a.n = n;
    a.n_streams = n_streams;
    a.obs_kind = obs_kind;
    const uintptr_t src = reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(next_obs);
    const uintptr_t dst = reinterpret_cast<uintptr_t>(rp->obs) | reinterpret_cast<uintptr_t>(rp->succ_obs);
    a.vec = (rp->obs_elems & 3) == 0 && (dst & (ring_kind == PRISM_RING_F32 ? 15 : 3)) == 0 &&
            (src & (obs_kind == PRISM_OBS_F32 ? 15 : 3)) == 0;
    a.first_slot = first_slot;
    a.serial0 = serial0;
    a.obs = obs;
    a.next_obs = next_obs;
    a.reward = reward;
    a.action = action;
    a.done = done;
    a.truncated = truncated;
    a.stream_ids = stream_ids;
    a.stream_tab = stream_tab;
    a.alpha = alpha;
    a.eps = eps;
    L.threads = n >= 1024 ? 1024 : ((n + 127) / 128) * 128;
    const int per_wg = L.threads / INGEST_ROW_THREADS;
    L.row_wgs = (n + per_wg - 1) / per_wg;
    if (L.row_wgs > INGEST_MAX_ROW_WGS) L.row_wgs = INGEST_MAX_ROW_WGS;
    return L;
}

}  // namespace

extern "C" int prism_replay_ingest(const prism_replay_desc *rp, int32_t n, int64_t first_slot, int64_t serial0,
                                   const void *obs, const void *next_obs, int32_t obs_kind, const float *reward,
                                   const int32_t *action, const uint8_t *done, const uint8_t *truncated,
                                   const int32_t *stream_ids, int64_t *stream_tab, int32_t n_streams, float alpha,
                                   float eps, prism_stream_t stream) {
    INGEST_CHECK_ARGS();
    const IngestLaunch L = ingest_plan(rp, n, first_slot, serial0, obs, next_obs, obs_kind, reward, action, done, truncated,
                                       stream_ids, stream_tab, n_streams, alpha, eps);
    hipLaunchKernelGGL(replay_ingest_kernel, dim3(1 + L.row_wgs), dim3(L.threads), 0, (hipStream_t)stream, *rp, L.a);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_replay_ingest_tracked(const prism_replay_desc *rp, int32_t n, int64_t first_slot, int64_t serial0,
                                           const void *obs, const void *next_obs, int32_t obs_kind, const float *reward,
                                           const int32_t *action, const uint8_t *done, const uint8_t *truncated,
                                           const int32_t *stream_ids, int64_t *stream_tab, int32_t n_streams, float alpha,
                                           float eps, const prism_episode_desc *ep, prism_stream_t stream) {
    INGEST_CHECK_ARGS();
    PRISM_CHECK_ARG(ep != nullptr, "null episode descriptor");
    INGEST_CHECK_EPISODES();
    const IngestLaunch L = ingest_plan(rp, n, first_slot, serial0, obs, next_obs, obs_kind, reward, action, done, truncated,
                                       stream_ids, stream_tab, n_streams, alpha, eps);
    // workgroup 0 and the row stores keep their indices; the episode role is the last workgroup
    hipLaunchKernelGGL(replay_ingest_tracked_kernel, dim3(2 + L.row_wgs), dim3(L.threads), 0, (hipStream_t)stream, *rp, L.a,
                       *ep);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// Either storage kind, plain (ep == NULL) or tracked: the fp32 kind launches the kernels of the two entry points above.
extern "C" int prism_replay_ingest_ring(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, int64_t first_slot,
                                        int64_t serial0, const void *obs, const void *next_obs, int32_t obs_kind,
                                        const float *reward, const int32_t *action, const uint8_t *done,
                                        const uint8_t *truncated, const int32_t *stream_ids, int64_t *stream_tab,
                                        int32_t n_streams, float alpha, float eps, const prism_episode_desc *ep,
                                        prism_stream_t stream) {
    INGEST_CHECK_ARGS();
    PRISM_CHECK_RING_KIND(rp, ring_kind);
    if (ep) INGEST_CHECK_EPISODES();
    const IngestLaunch L = ingest_plan(rp, n, first_slot, serial0, obs, next_obs, obs_kind, reward, action, done, truncated,
                                       stream_ids, stream_tab, n_streams, alpha, eps, ring_kind);
    const dim3 grid((ep ? 2 : 1) + L.row_wgs), block(L.threads);
    hipStream_t st = (hipStream_t)stream;
    if (ring_kind == PRISM_RING_U8) {
        if (ep) hipLaunchKernelGGL(byte_ring_ingest_tracked_kernel, grid, block, 0, st, *rp, L.a, *ep);
        else hipLaunchKernelGGL(byte_ring_ingest_kernel, grid, block, 0, st, *rp, L.a);
    } else {
        if (ep) hipLaunchKernelGGL(replay_ingest_tracked_kernel, grid, block, 0, st, *rp, L.a, *ep);
        else hipLaunchKernelGGL(replay_ingest_kernel, grid, block, 0, st, *rp, L.a);
    }
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// prism_replay_ingest_ring with the ring cursor read on the device (ingest_kernels.h, "the cursor form"): the launch takes
// serial0 = cursor[slot], first_slot = serial0 % capacity, and leaves serial0 + n in cursor[slot ^ 1].  `slot` is by value:
// a captured graph bakes it, successive launches alternate it.
extern "C" int prism_replay_ingest_cursor(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, int64_t *cursor,
                                          int32_t slot, const void *obs, const void *next_obs, int32_t obs_kind,
                                          const float *reward, const int32_t *action, const uint8_t *done,
                                          const uint8_t *truncated, const int32_t *stream_ids, int64_t *stream_tab,
                                          int32_t n_streams, float alpha, float eps, const prism_episode_desc *ep,
                                          prism_stream_t stream) {
    INGEST_CHECK_SHAPE();
    PRISM_CHECK_ARG(cursor != nullptr, "null cursor");
    PRISM_CHECK_ARG(slot == 0 || slot == 1, "slot must be 0 or 1");
    INGEST_CHECK_ARRAYS();
    PRISM_CHECK_RING_KIND(rp, ring_kind);
    if (ep) INGEST_CHECK_EPISODES();
    // (first_slot / serial0 of the plan are placeholders: the kernel overwrites them with what it reads)
    const IngestLaunch L = ingest_plan(rp, n, 0, 0, obs, next_obs, obs_kind, reward, action, done, truncated, stream_ids,
                                       stream_tab, n_streams, alpha, eps, ring_kind);
    const IngestCursor c{cursor, slot};
    const dim3 grid((ep ? 2 : 1) + L.row_wgs), block(L.threads);
    hipStream_t st = (hipStream_t)stream;
    if (ring_kind == PRISM_RING_U8) {
        if (ep) hipLaunchKernelGGL(byte_ring_cursor_ingest_tracked_kernel, grid, block, 0, st, *rp, L.a, *ep, c);
        else hipLaunchKernelGGL(byte_ring_cursor_ingest_kernel, grid, block, 0, st, *rp, L.a, c);
    } else {
        if (ep) hipLaunchKernelGGL(cursor_ingest_tracked_kernel, grid, block, 0, st, *rp, L.a, *ep, c);
        else hipLaunchKernelGGL(cursor_ingest_kernel, grid, block, 0, st, *rp, L.a, c);
    }
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
