// Host entry points of the replay ring + PER trees (C ABI in include/prism_hip.h).
#include "replay_kernels.h"

using namespace prism;

extern "C" int prism_replay_init(const prism_replay_desc *rp, prism_stream_t stream) {
    int rc = check_ring(rp, false);
    if (rc) return rc;
    hipLaunchKernelGGL(replay_init_kernel, dim3(1024), dim3(256), 0, (hipStream_t)stream, *rp);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

// the launches of prism_replay_insert / prism_replay_insert_ring, arguments checked by the caller
static int replay_insert(const prism_replay_desc *rp, int32_t ring_kind, int32_t obs_kind, int32_t n, const int32_t *slots,
                         const void *obs, const void *succ_obs, const float *reward, const int32_t *action,
                         const uint8_t *flags, const int32_t *prev_slot, float alpha, float eps, prism_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int grid = n < 2048 ? n : 2048;
    if (ring_kind == PRISM_RING_F32) {
        hipLaunchKernelGGL(replay_store_rows_kernel, dim3(grid), dim3(128), 0, stream, *rp, n, slots,
                           static_cast<const float *>(obs), static_cast<const float *>(succ_obs), reward, action, flags);
    } else {
        const uintptr_t src = reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(succ_obs);
        const uintptr_t dst = reinterpret_cast<uintptr_t>(rp->obs) | reinterpret_cast<uintptr_t>(rp->succ_obs);
        const int vec = (rp->obs_elems & 3) == 0 && (src & (obs_kind == PRISM_OBS_F32 ? 15 : 3)) == 0 && (dst & 3) == 0;
        if (obs_kind == PRISM_OBS_U8)
            hipLaunchKernelGGL(replay_store_rows_byte_ring_kernel<PRISM_OBS_U8>, dim3(grid), dim3(128), 0, stream, *rp, n, vec,
                               slots, obs, succ_obs, reward, action, flags);
        else
            hipLaunchKernelGGL(replay_store_rows_byte_ring_kernel<PRISM_OBS_F32>, dim3(grid), dim3(128), 0, stream, *rp, n, vec,
                               slots, obs, succ_obs, reward, action, flags);
    }
    PRISM_CHECK_LAUNCH();
    const int threads = n >= 1024 ? 1024 : ((n + 127) / 128) * 128;
    hipLaunchKernelGGL(replay_link_kernel, dim3(1), dim3(threads), 0, stream, *rp, n, slots, prev_slot, alpha, eps);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_replay_insert(const prism_replay_desc *rp, int32_t n, const int32_t *slots, const float *obs,
                                   const float *succ_obs, const float *reward, const int32_t *action,
                                   const uint8_t *flags, const int32_t *prev_slot, float alpha, float eps,
                                   prism_stream_t stream) {
    int rc = check_ring(rp, false);
    if (rc) return rc;
    if (n == 0) return PRISM_OK;
    PRISM_CHECK_ARG(n > 0 && n <= rp->capacity, "n must be in (0, capacity]");
    PRISM_CHECK_ARG(slots && obs && succ_obs && reward && action && flags && prev_slot, "null staging array");
    return replay_insert(rp, PRISM_RING_F32, PRISM_OBS_F32, n, slots, obs, succ_obs, reward, action, flags, prev_slot, alpha, eps,
                         stream);
}

extern "C" int prism_replay_insert_ring(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, const int32_t *slots,
                                        const void *obs, const void *succ_obs, int32_t obs_kind, const float *reward,
                                        const int32_t *action, const uint8_t *flags, const int32_t *prev_slot, float alpha,
                                        float eps, prism_stream_t stream) {
    int rc = check_ring(rp, false);
    if (rc) return rc;
    PRISM_CHECK_RING_KIND(rp, ring_kind);
    PRISM_CHECK_ARG(obs_kind == PRISM_OBS_F32 || obs_kind == PRISM_OBS_U8, "obs_kind must be PRISM_OBS_F32 or PRISM_OBS_U8");
    PRISM_CHECK_ARG(ring_kind == PRISM_RING_U8 || obs_kind == PRISM_OBS_F32, "an fp32 ring takes fp32 staging rows");
    if (n == 0) return PRISM_OK;
    PRISM_CHECK_ARG(n > 0 && n <= rp->capacity, "n must be in (0, capacity]");
    PRISM_CHECK_ARG(slots && obs && succ_obs && reward && action && flags && prev_slot, "null staging array");
    return replay_insert(rp, ring_kind, obs_kind, n, slots, obs, succ_obs, reward, action, flags, prev_slot, alpha, eps, stream);
}

extern "C" int prism_per_rebuild(const prism_replay_desc *rp, prism_stream_t stream) {
    int rc = check_ring(rp, true);
    if (rc) return rc;
    for (int64_t first = rp->tree_capacity >> 1; first >= 1; first >>= 1) {
        const int64_t count = first;
        int grid = (int)((count + 255) / 256);
        if (grid > 2048) grid = 2048;
        hipLaunchKernelGGL(per_rebuild_level_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, *rp, first, count);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_per_sample(const prism_replay_desc *rp, int64_t size, int32_t batch, const float *mass,
                                uint64_t seed, uint64_t offset, float beta, int64_t *out_index, float *out_weight,
                                prism_stream_t stream) {
    int rc = check_ring(rp, true);
    if (rc) return rc;
    PRISM_CHECK_ARG(size > 0 && size <= rp->capacity, "size must be in (0, capacity] (empty storage)");
    PRISM_CHECK_ARG(batch > 0 && out_index && out_weight, "batch/out");
    {
        ProfileScope ps_(K_PER_SAMPLE, (hipStream_t)stream);
        hipLaunchKernelGGL(per_sample_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, *rp, size,
                           batch, mass, seed, offset, beta, out_index, out_weight);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_uniform_sample(int64_t size, int32_t batch, uint64_t seed, uint64_t offset, int64_t *out_index,
                                    prism_stream_t stream) {
    PRISM_CHECK_ARG(size > 0 && batch > 0 && out_index, "size/batch/out");
    hipLaunchKernelGGL(uniform_sample_kernel, dim3((batch + 255) / 256), dim3(256), 0, (hipStream_t)stream, size,
                       batch, seed, offset, out_index);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}

extern "C" int prism_replay_gather(const prism_replay_desc *rp, const int64_t *index, int32_t batch, float *out_obs,
                                   float *out_next_obs, float *out_reward, uint8_t *out_nonterminal, float *out_gamma,
                                   int64_t *out_action, prism_stream_t stream) {
    int rc = check_ring(rp, false);
    if (rc) return rc;
    PRISM_CHECK_ARG(batch > 0 && index && out_obs && out_next_obs && out_reward && out_nonterminal && out_gamma &&
                        out_action,
                    "batch/out");
    {
        ProfileScope ps_(K_GATHER, (hipStream_t)stream);
        hipLaunchKernelGGL(replay_gather_kernel<PRISM_RING_F32>, dim3(batch), dim3(128), 0, (hipStream_t)stream, *rp, index,
                           batch, out_obs, out_next_obs, out_reward, out_nonterminal, out_gamma, out_action);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_replay_gather_ring(const prism_replay_desc *rp, int32_t ring_kind, const int64_t *index, int32_t batch,
                                        float *out_obs, float *out_next_obs, float *out_reward, uint8_t *out_nonterminal,
                                        float *out_gamma, int64_t *out_action, prism_stream_t stream) {
    int rc = check_ring(rp, false);
    if (rc) return rc;
    PRISM_CHECK_RING_KIND(rp, ring_kind);
    PRISM_CHECK_ARG(batch > 0 && index && out_obs && out_next_obs && out_reward && out_nonterminal && out_gamma &&
                        out_action,
                    "batch/out");
    {
        ProfileScope ps_(K_GATHER, (hipStream_t)stream);
        if (ring_kind == PRISM_RING_U8)
            hipLaunchKernelGGL(replay_gather_kernel<PRISM_RING_U8>, dim3(batch), dim3(128), 0, (hipStream_t)stream, *rp, index,
                               batch, out_obs, out_next_obs, out_reward, out_nonterminal, out_gamma, out_action);
        else
            hipLaunchKernelGGL(replay_gather_kernel<PRISM_RING_F32>, dim3(batch), dim3(128), 0, (hipStream_t)stream, *rp, index,
                               batch, out_obs, out_next_obs, out_reward, out_nonterminal, out_gamma, out_action);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_per_update(const prism_replay_desc *rp, const int64_t *index, const float *priority,
                                int32_t batch, float alpha, float eps, int32_t take_abs, prism_stream_t stream) {
    int rc = check_ring(rp, true);
    if (rc) return rc;
    PRISM_CHECK_ARG(batch > 0 && index && priority, "batch/index/priority");
    {
        ProfileScope ps_(K_PER_UPDATE, (hipStream_t)stream);
        launch_per_update(*rp, index, priority, batch, alpha, eps, take_abs, (hipStream_t)stream);
        PRISM_CHECK_LAUNCH();
    }
    return PRISM_OK;
}

extern "C" int prism_per_query(const prism_replay_desc *rp, int64_t size, float *out2, prism_stream_t stream) {
    int rc = check_ring(rp, true);
    if (rc) return rc;
    PRISM_CHECK_ARG(size > 0 && size <= rp->capacity && out2, "size/out");
    hipLaunchKernelGGL(per_query_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, *rp, size, out2);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
