// Host entry point of the evaluation tracker's quota rule (C ABI in include/prism_hip.h).
#include "eval_quota_kernels.h"

using namespace prism;

extern "C" int prism_eval_track_quota(const prism_eval_desc *ev, const prism_eval_quota *q, int32_t n, const float *reward,
                                      const uint8_t *done, const uint8_t *truncated, prism_stream_t stream) {
    PRISM_CHECK_ARG(ev != nullptr, "null descriptor");
    PRISM_CHECK_ARG(q != nullptr, "null quota descriptor");
    PRISM_CHECK_ARG(ev->n_streams >= 1 && ev->n_streams <= INGEST_MAX_STREAMS, "n_streams must be in [1, 65536]");
    PRISM_CHECK_ARG(n == ev->n_streams, "n must equal n_streams: the quota rule speaks about every stream");
    PRISM_CHECK_ARG(q->quota >= 1, "quota must be >= 1");
    PRISM_CHECK_ARG(q->max_calls >= 1, "max_calls must be >= 1");
    PRISM_CHECK_ARG(ev->log_capacity >= 0, "log_capacity must be >= 0");
    PRISM_CHECK_ARG(ev->ep_return && ev->ep_length && ev->stats && ev->counts, "null evaluation array");
    PRISM_CHECK_ARG(q->ep_done && q->qcounts, "null quota array");
    PRISM_CHECK_ARG(ev->log_capacity == 0 || (ev->log_return && ev->log_length),
                    "log_return and log_length may be NULL only with log_capacity == 0");
    PRISM_CHECK_ARG(reward && done && truncated, "null step array");
    hipLaunchKernelGGL(eval_track_quota_kernel, dim3(1), dim3(EP_PASS), 0, (hipStream_t)stream, *ev, *q, n, reward, done,
                       truncated);
    PRISM_CHECK_LAUNCH();
    return PRISM_OK;
}
