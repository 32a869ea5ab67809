/*
 * prism_hip.h — C ABI of libprism_hip.so (gfx950 / MI355X).
 *
 * The reference (AechPro/Prism) has no FFI layer: its hot path is Python calling torch + the
 * third-party torchrl segment trees.  These entry points are what a binding for that path would
 * call; each one names the reference interface it replaces (paths under /root/reference).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller unless
 *     the parameter says "host";
 *   - every call enqueues work on `stream` (a hipStream_t passed as void*) and returns without
 *     synchronising; no hidden allocation, no hidden sync — safe to capture into a hipGraph;
 *   - return value: PRISM_OK or a negative PRISM_ERR_* code; prism_last_error() returns a
 *     thread-local message; nothing throws across the boundary;
 *   - single-threaded caller per stream, as the reference's learner loop
 *     (prism/learner.py:75-143).
 */
#ifndef PRISM_HIP_H
#define PRISM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PRISM_ABI_VERSION 3

#define PRISM_OK 0
#define PRISM_ERR_INVALID (-1)     /* bad argument / shape the kernels do not cover          */
#define PRISM_ERR_HIP (-2)         /* a HIP runtime call failed                             */
#define PRISM_ERR_UNSUPPORTED (-3) /* valid reference configuration not implemented here    */

#define PRISM_MAX_NSTEP 15

#define PRISM_GEMM_FP32 1
#define PRISM_GEMM_BF16X3 2
#define PRISM_GEMM_DEFAULT PRISM_GEMM_BF16X3

#define PRISM_ACT_WEIGHTS_CURRENT 1

/* per-slot flag bits of the replay ring */
#define PRISM_FLAG_DONE 1u      /* Timestep.done                                            */
#define PRISM_FLAG_TRUNC 2u     /* Timestep.truncated                                       */
#define PRISM_FLAG_HAS_NEXT 4u  /* Timestep.next is not None                                */

/* device status word bits (prism_replay_desc.status) */
#define PRISM_WS_STATUS_WORD 7             /* index of the sticky status word in prism_learner_desc.workspace (uint32) */
#define PRISM_WS_STATUS_BARRIER_TIMEOUT 1u
#define PRISM_WS_STATUS_COLLECTIVE_TIMEOUT 2u /* a direct all-reduce wait gave up (prism_direct_desc.poison): clip + Adam are skipped */
#define PRISM_STATUS_NONPOSITIVE_PSUM 1
#define PRISM_STATUS_NONPOSITIVE_PMIN 2
#define PRISM_STATUS_INGEST_DUP_STREAM 4   /* prism_replay_ingest: a stream id repeated in one call or outside the table */
#define PRISM_STATUS_OBS_INEXACT 8         /* byte ring: a float that is not byte-exact was narrowed (stored as 0) */
#define PRISM_STATUS_INGEST_BAD_CURSOR 16  /* prism_replay_ingest_cursor: the device cursor word was negative; nothing was written */
#define PRISM_STATUS_FRONT_BAD_SIZE 32     /* prism_step_front_cursor: the device cursor word was <= 0; the launch sampled as from one row */

/* prism_replay_ingest obs_kind */
#define PRISM_OBS_F32 0
#define PRISM_OBS_U8 1     /* uint8 / bool observations, widened to fp32 on the device */

/* Storage kind of the ring's two observation arrays (prism_replay_desc.obs / succ_obs), the `ring_kind` argument of the
 * prism_*_ring entry points.  The descriptor is the same for both kinds: a byte ring holds its two uint8
 * [capacity][obs_elems] arrays in `obs` / `succ_obs`.  The entry points without the argument are the fp32 kind.
 *   byte-exact   a float whose bit pattern is that of (float)b for a b in 0..255: +0.0, 1.0 .. 255.0 (not -0.0, NaN,
 *                +-inf, fractions, negatives, values above 255)
 *   narrowing    a byte-exact float is stored as b; every other float is stored as 0 and the sticky bit
 *                PRISM_STATUS_OBS_INEXACT is set in rp->status (the call never reads device memory on the host)
 *   widening     (float)b, exact: a byte ring fed byte-exact rows yields bit for bit what the fp32 ring yields
 * Entry points that never touch observation rows (prism_per_*, prism_step_back*, prism_replay_init) take a byte ring's
 * descriptor as it is.  An unknown ring_kind is PRISM_ERR_INVALID, the message names the entry point. */
#define PRISM_RING_F32 0
#define PRISM_RING_U8 1

typedef void *prism_stream_t;

const char *prism_last_error(void);
int prism_abi_version(void);
/* host out-params; multiprocessor count and gcnArch name ("gfx950") of `device`. */
int prism_device_info(int device, int *cu_count, char *arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------
 * Replay ring + prioritized sum/min trees, resident in HBM.
 *
 * Replaces torchrl PrioritizedReplayBuffer(ListStorage) + prism TimestepBuffer
 * (prism/factory/exp_buffer_factory.py:22-33, prism/experience/timestep_buffer.py:10-238).
 * Layout: structure-of-arrays ring of `capacity` slots; trees are binary segment trees with
 * `tree_capacity` = smallest power of two STRICTLY greater than `capacity`, 2*tree_capacity fp32
 * nodes each, leaf i at node (i | tree_capacity), root at node 1.
 * ------------------------------------------------------------------------------------------ */
typedef struct prism_replay_desc {
    int64_t capacity;
    int64_t tree_capacity;
    int32_t obs_elems;   /* floats per observation (10*10*C for MinAtar)                      */
    int32_t n_step;      /* n-step return length, 1..PRISM_MAX_NSTEP                          */
    float *obs;          /* [capacity][obs_elems]                                             */
    float *succ_obs;     /* [capacity][obs_elems] observation of the slot's immediate successor */
    float *reward;       /* [capacity]                                                        */
    int32_t *action;     /* [capacity]                                                        */
    uint8_t *flags;      /* [capacity] PRISM_FLAG_*                                           */
    int32_t *link;       /* [capacity] ring slot of the stored successor, -1 if none yet      */
    int32_t *back;       /* [capacity] ring slot of the predecessor that links here, or -1    */
    float *tree;         /* [2*tree_capacity][2] {sum, min} of every node interleaved (both children
                            of a node are one aligned 16-byte load); NULL for uniform replay   */
    float *per_state;    /* [4] {running max raw priority, last p_sum, last p_min, unused}    */
    int32_t *status;     /* [1] sticky PRISM_STATUS_* bits                                    */
    double gammas[PRISM_MAX_NSTEP + 1]; /* gamma**k as Python float64 (timestep_buffer.py:17)  */
} prism_replay_desc;

/* trees := identity (0 / FLT_MAX), per_state := {1,0,0,0}, status := 0, link/back := -1.
 * torchrl PrioritizedSampler._init. */
int prism_replay_init(const prism_replay_desc *rp, prism_stream_t stream);

/* TimestepBuffer.extend (timestep_buffer.py:32-33) for n completed timesteps, applied in order
 * i = 0..n-1: overwrite ring slot slots[i] (detaching any predecessor that linked to the old row),
 * store the row, link prev_slot[i] -> slots[i] when prev_slot[i] >= 0, and give the slot the
 * sampler's default priority (max_priority + eps) ** alpha in both trees
 * (torchrl PrioritizedSampler.extend).  All array arguments are device staging buffers. */
int prism_replay_insert(const prism_replay_desc *rp, int32_t n, const int32_t *slots,
                        const float *obs, const float *succ_obs, const float *reward,
                        const int32_t *action, const uint8_t *flags, const int32_t *prev_slot,
                        float alpha, float eps, prism_stream_t stream);

/* prism_replay_insert for a ring of either storage kind.  A byte ring takes uint8 staging rows (obs_kind PRISM_OBS_U8,
 * copied) or fp32 ones (PRISM_OBS_F32, narrowed); an fp32 ring takes fp32 rows only, and is prism_replay_insert. */
int prism_replay_insert_ring(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, const int32_t *slots,
                             const void *obs, const void *succ_obs, int32_t obs_kind, const float *reward,
                             const int32_t *action, const uint8_t *flags, const int32_t *prev_slot,
                             float alpha, float eps, prism_stream_t stream);

/* One step of a vectorised collector: n transitions of n DISTINCT environment streams, applied in
 * order i = 0..n-1 with exactly the result of n one-row prism_replay_insert calls -- in one launch and
 * without the host resolving any predecessor (the per-row bookkeeping of
 * multiprocessing_experience_collection/collector_process_interface.py:154-169 + TimestepBuffer.extend).
 *   slot of row i      (first_slot + i) % capacity; `serial0` = rows ever written to this ring since
 *                      init / empty / bulk load, serial0 % capacity == first_slot, 1 <= n <= capacity.
 *   obs, next_obs      [n][obs_elems], fp32 (obs_kind PRISM_OBS_F32) or uint8 (PRISM_OBS_U8).
 *   flags              DONE if done[i], TRUNC if truncated[i], HAS_NEXT if truncated[i] or not done[i];
 *                      the successor row is next_obs[i] when HAS_NEXT, zeros otherwise.
 *   stream_ids         stream of row i, in [0, n_streams); NULL: row i is stream i (needs n <= n_streams).
 *   stream_tab         [n_streams] int64, device, owned by the caller, -1 = no open row: the write serial
 *                      w of the stream's open row.  Row i links back to slot w % capacity iff
 *                      0 < serial0 + i - w < capacity (a slot is reused exactly every `capacity` writes);
 *                      afterwards the entry is serial0 + i if not done[i] and not truncated[i], else -1.
 *                      1 <= n_streams <= 65536.
 * Overwritten slots detach their old neighbours and every written slot gets the default priority, as
 * prism_replay_insert.  A stream id that repeats within the call (or lies outside the table) cannot be
 * refused by a call that never reads device memory on the host: its rows are stored UNLINKED, the
 * stream is closed and the sticky bit PRISM_STATUS_INGEST_DUP_STREAM is set in rp->status. */
int prism_replay_ingest(const prism_replay_desc *rp, int32_t n, int64_t first_slot, int64_t serial0,
                        const void *obs, const void *next_obs, int32_t obs_kind, const float *reward,
                        const int32_t *action, const uint8_t *done, const uint8_t *truncated,
                        const int32_t *stream_ids, int64_t *stream_tab, int32_t n_streams,
                        float alpha, float eps, prism_stream_t stream);

/* prism_replay_ingest with the rest of what the reference's collector does per timestep
 * (collector_process_interface.py:129-139, experience_collector.py:113-118): the reward clip and, per stream,
 * the episodic return with the training-reward EMA -- same launch, one more workgroup, still no host read. */
#define PRISM_CLIP_NONE  0
#define PRISM_CLIP_CLAMP 1  /* r < -1 ? -1 : (r > 1 ? 1 : r): NaN and -0.0 pass through unchanged ("dopamine_clamp") */
typedef struct prism_episode_desc {
    int32_t reward_clip;       /* PRISM_CLIP_*: applied to the reward STORED in the ring only               */
    int32_t count_first_step;  /* 0: the reference's rule (an episode's first reward is not counted); 1: it is */
    double ema;                /* training_reward_ema, in [0, 1]                                            */
    double *ep_return;         /* [n_streams] running return of each stream's open episode; NULL: no tracking */
    int32_t *ep_length;        /* [n_streams] steps of the open episode so far (0 = none open)              */
    double *stats;             /* [4] training reward (EMA) | sum of finished returns | last finished return | unused */
    int64_t *counts;           /* [4] episodes finished | sum of their lengths | rows tracked | unused      */
} prism_episode_desc;

/* The ring, flags, links, stream table, default priorities and status word come out bit for bit as from
 * prism_replay_ingest fed rewards the host clipped beforehand.  Per row of stream s, in float64 on the RAW reward:
 * len = ep_length[s] + 1; ret = 0 if the episode had no step yet and count_first_step == 0, else reward + ep_return[s];
 * done | truncated: an episode end (ret, len), both accumulators of s return to 0; else they are stored back.  Ends are
 * folded in row order: counts[0] += 1, counts[1] += len, stats[1] += ret, stats[2] = ret and
 * stats[0] = first ever ? ret : ema * stats[0] + (1 - ema) * ret (two products, one sum, each rounded).  counts[2] grows
 * by the rows tracked.  Rows stored unlinked (id outside the table / repeated in the call) are not tracked; a repeated
 * stream's accumulators are zeroed.  ep_return .. counts are all set or all NULL (clip only). */
int prism_replay_ingest_tracked(const prism_replay_desc *rp, int32_t n, int64_t first_slot, int64_t serial0,
                                const void *obs, const void *next_obs, int32_t obs_kind, const float *reward,
                                const int32_t *action, const uint8_t *done, const uint8_t *truncated,
                                const int32_t *stream_ids, int64_t *stream_tab, int32_t n_streams,
                                float alpha, float eps, const prism_episode_desc *ep, prism_stream_t stream);

/* prism_replay_ingest (ep == NULL) / prism_replay_ingest_tracked (ep != NULL) for a ring of either storage kind.  Into a
 * byte ring uint8 / bool rows are copied and fp32 rows narrowed (a row without successor stores zeros, as ever). */
int prism_replay_ingest_ring(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, int64_t first_slot,
                             int64_t serial0, const void *obs, const void *next_obs, int32_t obs_kind,
                             const float *reward, const int32_t *action, const uint8_t *done,
                             const uint8_t *truncated, const int32_t *stream_ids, int64_t *stream_tab,
                             int32_t n_streams, float alpha, float eps, const prism_episode_desc *ep,
                             prism_stream_t stream);

/* prism_replay_ingest_ring with the ring cursor in device memory, for a launch that is captured once and replayed: a
 * by-value cursor would send every replay to the same slots.  `cursor` is a pair of device words in ping-pong and `slot`
 * (0 | 1, by value: a captured graph bakes it, successive launches alternate it) names the one this launch reads:
 *   serial0 = cursor[slot], first_slot = serial0 % capacity
 *   everything the launch writes is, bit for bit, what prism_replay_ingest_ring writes when handed those two values
 *   before the launch ends one lane stores cursor[slot ^ 1] = serial0 + n (an ordinary store)
 * No thread reads cursor[slot ^ 1] and none writes cursor[slot]: the word a launch reads is never written while it runs,
 * and the next launch, handed the other slot, sees the advanced word across the kernel boundary.  A negative serial0
 * cannot be refused on the host (the call never reads device memory there): the launch writes nothing to the ring, copies
 * the value unchanged to cursor[slot ^ 1] and raises the sticky bit PRISM_STATUS_INGEST_BAD_CURSOR in rp->status.
 * Refused on the host: what prism_replay_ingest_ring refuses (its two cursor checks aside), a NULL cursor, any other slot. */
int prism_replay_ingest_cursor(const prism_replay_desc *rp, int32_t ring_kind, int32_t n, int64_t *cursor /* device, [2] */,
                               int32_t slot /* 0 | 1 */, const void *obs, const void *next_obs, int32_t obs_kind,
                               const float *reward, const int32_t *action, const uint8_t *done, const uint8_t *truncated,
                               const int32_t *stream_ids, int64_t *stream_tab, int32_t n_streams, float alpha, float eps,
                               const prism_episode_desc *ep, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation bookkeeping -- SyncAgentEvaluator.evaluate_agent (prism/evals/sync_agent_evaluator.py:37-59) for n_streams
 * environments stepped in lockstep: episode returns, the list of finished episodes and the loop's own stopping rule, on
 * the device in one launch per environment step, without a host read.
 * ------------------------------------------------------------------------------------------ */
typedef struct prism_eval_desc {
    int32_t n_streams;      /* 1 .. 65536 */
    int32_t log_capacity;   /* >= 0: finished episodes kept one by one */
    int64_t budget;         /* evaluation_timestep_horizon, >= 0 */
    double  *ep_return;     /* [n_streams] return of the open episode */
    int32_t *ep_length;     /* [n_streams] its steps so far */
    double  *log_return;    /* [log_capacity] finished returns, in (call, row) order */
    int32_t *log_length;    /* [log_capacity] */
    double  *stats;         /* [4] sum | sum of squares | min | max of finished returns */
    int64_t *counts;        /* [4] episodes | sum of their lengths | rows taken | calls taken */
    int64_t *host_counts;   /* optional, pinned host [2]: counts[0], counts[2] after this call */
} prism_eval_desc;

/* One environment step of an evaluation: row i is stream i, 1 <= n <= n_streams; reward [n] fp32, done / truncated [n].
 * The call first reads closed = counts[2] >= budget && counts[0] >= 1 -- the reference's loop condition
 * `collected_ts < n_ts or len(ep_rews) == 0` (sync_agent_evaluator.py:42), evaluated before the step.  A closed
 * evaluation takes nothing: every array stays bit for bit as it was and only host_counts is rewritten, so a host that
 * runs ahead of the device cannot spoil the result.  Otherwise, per row, in float64 on the widened reward:
 * len = ep_length[i] + 1; ret = reward[i] + ep_return[i] (an episode's first reward counts: the evaluator's rule, not
 * the collector's); done | truncated: an episode end (ret, len), both accumulators of i return to 0; else they are
 * stored back.  Ends are folded in row order: if counts[0] < log_capacity the pair goes to log slot counts[0];
 * stats[0] += ret; stats[1] += ret * ret (the product and the sum each rounded); stats[2] / stats[3] = min / max by
 * plain < / > compares, the first episode setting both; counts[0] += 1; counts[1] += len.  After the rows
 * counts[2] += n and counts[3] += 1.  The whole call is taken or none of it: the rule is not read again between rows.
 * host_counts, when given, receives counts[0] and counts[2] as the call leaves them (plain stores, visible to the host
 * once the launch has ended).  log_return / log_length may be NULL only with log_capacity == 0. */
int prism_eval_track(const prism_eval_desc *ev, int32_t n, const float *reward, const uint8_t *done,
                     const uint8_t *truncated, prism_stream_t stream);

/* The quota rule: the project's own stopping rule for n_streams > 1, not the reference's.  Under the budget rule above
 * every stream gets budget / n_streams steps and the n_streams episodes open at the cut are dropped; an episode open at a
 * fixed cut is length-biased long, so the mean is biased low where long episodes are the good ones.  Here every stream
 * contributes exactly its first `quota` finished episodes, whatever their lengths: the counted set is fixed in advance.
 * prism_eval_desc is used as it is (budget is not read); this struct carries what is new. */
typedef struct prism_eval_quota {
    int32_t quota;          /* E >= 1: finished episodes taken from every stream */
    int64_t max_calls;      /* >= 1: the evaluation also closes after this many taken calls (safety cap) */
    int32_t *ep_done;       /* device [n_streams]: finished episodes of stream i so far */
    int64_t *qcounts;       /* device [2]: streams that have met the quota | unused (0) */
    int64_t *host_closed;   /* optional, pinned host [1]: 1 once closed as this call leaves it, else 0 */
} prism_eval_quota;

/* One environment step of an evaluation under the quota rule: row i is stream i and n must equal n_streams (the rule
 * speaks about every stream); reward [n] fp32, done / truncated [n].  The call first reads
 * closed = qcounts[0] >= n_streams || counts[3] >= max_calls.  A closed evaluation takes nothing: every array stays bit
 * for bit as it was and only host_counts and host_closed are rewritten, so a host that runs ahead of the device cannot
 * spoil the result.  Otherwise, per row i, with live = ep_done[i] < quota read before the row: a row that is not live is
 * not touched and its reward and flags are never read (they may be NaN or set); a live row does prism_eval_track's
 * arithmetic, in float64 on the widened reward: len = ep_length[i] + 1; ret = reward[i] + ep_return[i] (an episode's
 * first reward counts); done | truncated: an episode end (ret, len), both accumulators of i return to 0 and
 * ep_done[i] += 1; else they are stored back.  Ends are folded in row order by the recurrences of prism_eval_track: log
 * slot counts[0] while counts[0] < log_capacity; stats[0] += ret; stats[1] += ret * ret (the product and the sum each
 * rounded); stats[2] / stats[3] = min / max by plain < / > compares, the first episode setting both; counts[0] += 1;
 * counts[1] += len.  Each stream whose ep_done reaches quota in this call adds 1 to qcounts[0].  After the rows
 * counts[2] += the number of live rows of this call and counts[3] += 1.  The whole call is taken or none of it: the rule
 * is not read again between rows.  host_counts, when given, receives counts[0] and counts[2] and host_closed, when
 * given, the closing predicate, both as the call leaves them (plain stores, visible to the host once the launch has
 * ended).  Nothing the launch takes by value changes from step to step: a captured launch replays as it is. */
int prism_eval_track_quota(const prism_eval_desc *ev, const prism_eval_quota *q, int32_t n, const float *reward,
                           const uint8_t *done, const uint8_t *truncated, prism_stream_t stream);

/* PrioritizedSampler.sample (called at timestep_buffer.py:37): p_sum/p_min = query(0,size);
 * index[i] = min(scan_lower_bound(mass[i]), size-1); weight[i] = (leaf/p_min) ** -beta.
 * mass == NULL: masses are drawn on the device, U(0,p_sum) in float64 narrowed to fp32, from
 * Philox4x32-10 keyed by (seed, offset); else `mass` holds `batch` fp32 values (parity mode: the
 * reference draws them with NumPy's global RNG, which cannot be reproduced on the device).
 * `size` = number of stored items (len(storage)).  Indices are int64 as in torchrl. */
int prism_per_sample(const prism_replay_desc *rp, int64_t size, int32_t batch, const float *mass,
                     uint64_t seed, uint64_t offset, float beta, int64_t *out_index,
                     float *out_weight, prism_stream_t stream);

/* torchrl RandomSampler (uniform replay, exp_buffer_factory.py:30-33): index ~ U{0..size-1}. */
int prism_uniform_sample(int64_t size, int32_t batch, uint64_t seed, uint64_t offset,
                         int64_t *out_index, prism_stream_t stream);

/* _compute_n_step + _timesteps_to_batch (timestep_buffer.py:79-238) for the sampled slots:
 * walks <= n_step links per sample (fp64 accumulate, fp32 store) and gathers rows.
 * out_nonterminal is torch.bool storage (1 byte), out_action int64. */
int prism_replay_gather(const prism_replay_desc *rp, const int64_t *index, int32_t batch,
                        float *out_obs, float *out_next_obs, float *out_reward,
                        uint8_t *out_nonterminal, float *out_gamma, int64_t *out_action,
                        prism_stream_t stream);

/* prism_replay_gather from a ring of either storage kind (the outputs are fp32 either way: bytes are widened). */
int prism_replay_gather_ring(const prism_replay_desc *rp, int32_t ring_kind, const int64_t *index, int32_t batch,
                             float *out_obs, float *out_next_obs, float *out_reward,
                             uint8_t *out_nonterminal, float *out_gamma, int64_t *out_action,
                             prism_stream_t stream);

/* PrioritizedSampler.update_priority (timestep_buffer.py:53-54 <- learner.py:120):
 * max_priority = max(max_priority, max(priority)); leaf = (priority + eps) ** alpha in both
 * trees; duplicate indices resolve as the sequential loop would (last occurrence wins); every
 * ancestor is recomputed as op(left, right).  take_abs != 0 applies |.| first (learner.py:120
 * passes new_per_weights.abs()). */
int prism_per_update(const prism_replay_desc *rp, const int64_t *index, const float *priority,
                     int32_t batch, float alpha, float eps, int32_t take_abs,
                     prism_stream_t stream);

/* Recompute every internal node from the leaves (after the caller wrote leaves in bulk: restoring a
 * saved sampler, torchrl PrioritizedSampler.loads, or a synthetic pre-fill). */
int prism_per_rebuild(const prism_replay_desc *rp, prism_stream_t stream);

/* out[0] = sum.query(0,size), out[1] = min.query(0,size) (device floats). */
int prism_per_query(const prism_replay_desc *rp, int64_t size, float *out2, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * TD update: CompositeModel.get_losses + Agent._update_without_cuda_graph
 * (prism/agents/models/composite_model.py:94-144, iqn_model.py:48-201, q_ensemble.py:44-92,
 *  prism/agents/agent.py:53-79), fp32 throughout.
 * ------------------------------------------------------------------------------------------ */
/* prism_model_dims.squish_fn (/root/reference/prism/agents/squish_functions.py:4-18) */
#define PRISM_SQUISH_NONE 0
#define PRISM_SQUISH_OBS_LOOK_FURTHER 1   /* sign(x) (sqrt(|x| + 1) - 1) + 0.01 x  and its inverse   */
#define PRISM_SQUISH_SYMLOG 2             /* sign(x) log(|x| + 1)  /  sign(x) (exp(|x|) - 1)          */

typedef struct prism_model_dims {
    int32_t in_channels;   /* C; observations are (10,10,C) NHWC                              */
    int32_t n_actions;     /* A <= 16                                                         */
    int32_t embed_dim;     /* 1024 = 16*8*8 (minatar_cnn_model.py:14)                         */
    int32_t use_iqn;
    int32_t n_basis;       /* 64                                                              */
    int32_t iqn_layers;    /* iqn_quantile_model_layers: 1, or 0 = no trunk (the linear head)   */
    int32_t iqn_width;     /* iqn_quantile_model_feature_dim (128 | 256); ignored at depth 0  */
    int32_t n_tau;         /* current-state quantile samples T                                */
    int32_t n_tau_next;    /* next-state quantile samples T'                                  */
    int32_t use_layer_norm;
    int32_t n_heads;       /* 0 none, 1 DQN, >1 IDS ensemble                                  */
    int32_t head_layers;   /* linear layers per head (1 or 2)                                 */
    int32_t head_width;    /* hidden width of a 2-layer head (128)                            */
    int32_t has_target;    /* target network present                                          */
    int32_t double_q;
    int32_t propagate_grad; /* IQN gradients reach the embedding (model_factory.py:87)        */
    float huber_k;
    float dist_loss_weight;
    float q_loss_weight;
    float theil_coef;      /* ids_ensemble_variation_coef                                     */
    int32_t squish_fn;     /* PRISM_SQUISH_*: loss_squish_fn_id (model_factory.py:16-23): the TD target is
                            * squish(r + gamma' * unsquish(z_next)) (iqn_model.py:141-148, q_ensemble.py:77-82) */
} prism_model_dims;

/* Offsets (in floats) of each tensor inside the flat parameter buffer, which is laid out in
 * model.parameters() order.  -1 = tensor absent. */
typedef struct prism_param_offsets {
    int64_t n_params;
    int64_t conv_w, conv_b;
    int64_t phi_w, phi_b;
    int64_t iqn_ln1_g, iqn_ln1_b, iqn_w1, iqn_b1;   /* the trunk: all -1 at iqn_layers 0                 */
    int64_t iqn_ln2_g, iqn_ln2_b, iqn_w2, iqn_b2;   /* [LayerNorm] -> Linear(., A) in front of the estimates */
    int64_t head_base;    /* first float of head 0                                           */
    int64_t head_stride;  /* floats per head                                                 */
    int64_t h_ln1_g, h_ln1_b, h_w1, h_b1; /* relative to the head's base                     */
    int64_t h_ln2_g, h_ln2_b, h_w2, h_b2; /* (1-layer head: only h_ln1_* (if LN) and h_w1/h_b1) */
} prism_param_offsets;

typedef struct prism_adam_hyper {
    double lr, beta1, beta2, eps; /* doubles: torch evaluates the bias corrections in Python floats */
    float max_grad_norm;
    float grad_scale;      /* multiplied into the gradient before the norm (1/world_size)    */
} prism_adam_hyper;

typedef struct prism_learner_desc {
    prism_model_dims dims;
    prism_param_offsets off;
    int32_t batch;            /* B                                                           */
    int32_t embed_done;       /* != 0: prism_step_front already produced the embeddings for this batch */
    /* parameters and optimizer state, flat fp32 [n_params] */
    float *params;
    const float *target_params; /* NULL when !has_target                                     */
    float *grads;             /* out: dL/dparams (unclipped, unscaled)                        */
    float *adam_m;            /* Adam exp_avg    | RMSprop grad_avg   | SGD: unused, still a valid pointer (prism_opt_hyper) */
    float *adam_v;            /* Adam exp_avg_sq | RMSprop square_avg | SGD: unused, still a valid pointer               */
    int64_t *adam_step;       /* [1] device step counter, incremented by every optimizer step    */
    /* minibatch (the static batch of timestep_buffer.py:84-104) */
    const float *obs;         /* [B][10][10][C]                                               */
    const float *next_obs;
    const float *reward;      /* [B] n-step return                                            */
    const uint8_t *nonterminal; /* [B] torch.bool                                            */
    const float *gamma;       /* [B] gamma ** m                                               */
    const int64_t *action;    /* [B]                                                          */
    const float *per_weights; /* [B] or NULL (== 1, learner.py:109)                           */
    /* quantile samples, tau-major rows (row = t*B + b, iqn_model.py:70).  NULL => drawn in-kernel
     * from Philox(seed, offset) and written to tau_out. */
    const float *tau_cur;     /* [T*B]                                                        */
    const float *tau_next_online; /* [T'*B] used when !has_target or double_q                 */
    const float *tau_next_target; /* [T'*B] used when has_target                              */
    float *tau_out;           /* [3][max(T,T')*B] or NULL                                     */
    uint64_t seed, offset;
    uint64_t *rng_counters;   /* optional device [3] {PER draws, tau draws, acting draws} added to the immediate
                                 offsets; [0], [1] are advanced by prism_step_back, [2] by prism_act_forward (lets a
                                 captured hipGraph draw fresh numbers on every replay); NULL = immediate offsets only */
    /* Optional: when fused_replay is set, prism_per_update(fused_index, |out_td|) rides along in the
     * learner's launches instead of being a workgroup of its own in prism_step_back: one more workgroup
     * of prism_learner_fwd_bwd's last launch prepares it (|TD|^alpha, ranking, duplicate resolution --
     * the TD errors are final by then) and, for batches up to 256, prism_step_back walks the tree levels
     * using the sibling values prism_step_front recorded (larger batches: all of it in fwd_bwd).
     * With fused_replay set, prism_learner_fwd_bwd MUST be followed by prism_step_back on the same
     * stream before the tree is read again.  Results are identical to the stand-alone update. */
    const struct prism_replay_desc *fused_replay;   /* host pointer or NULL */
    const int64_t *fused_index;                     /* [B] sampled slots */
    float fused_alpha, fused_eps;
    /* != 0 (fused hot path, single GPU only): prism_learner_fwd_bwd leaves the gradient partials unreduced and
     * prism_step_back reduces them, clips and applies Adam in ONE launch (a grid barrier stands where the launch
     * boundary was).  ld->grads is complete only after prism_step_back then, so nothing may sit between the two
     * calls -- leave it 0 when an all-reduce does (hyper.grad_scale != 1 ignores it).  The library falls back to the
     * separate launches by itself when the launch would not be resident at once or no priority writeback rides along
     * (fused_replay unset: nothing to hide behind the barrier).  Results are bit-identical.
     * The residency proof (occupancy of the launched instantiation x CUs of the current device) assumes the process has the
     * GPU to itself: with other processes' kernels on the device leave it 0.  A barrier that is not through after 100 ms
     * is abandoned: the workgroup sets PRISM_WS_STATUS_BARRIER_TIMEOUT in the workspace's status word and skips its
     * update instead of spinning for ever. */
    int32_t fuse_tail;
    /* prism_act_forward only.  PRISM_ACT_WEIGHTS_CURRENT: the stream-packed weight copies and LayerNorm helper vectors in
     * the workspace were built from `params` as they are now (an earlier prism_act_forward without this flag ran since the
     * parameters last changed): the call skips rebuilding them.  0 is always correct. */
    int32_t act_flags;
    /* How the forward GEMMs (quantile embedding, trunk, Q-head first layers) are multiplied: PRISM_GEMM_FP32 = the exact
     * fp32 MFMA chain; PRISM_GEMM_BF16X3 = every fp32 operand as the sum of three bf16 pieces, the six leading piece
     * products on the bf16 matrix pipe with fp32 accumulation (what is dropped is of the size of one fp32 rounding; same rms
     * error against float64 as the fp32 chain, profiles/r03_split_bf16_ubench.txt); 0 = library default (environment
     * PRISM_GEMM=fp32|bf16x3 overrides the default).  Both forms cover hidden widths 128 and 256. */
    int32_t gemm_mode;
    /* outputs */
    float *out_dist_loss;     /* [B] or NULL  (Agent._static_distribution_loss)               */
    float *out_q_loss;        /* [B] or NULL  (Agent._static_q_loss)                          */
    float *out_td;            /* [B]          (td_errors, composite_model.py:135-142)         */
    float *out_scalars;       /* [8] {total loss, mean dl*w, mean ql*w, grad norm, theil, clip coef, -, -} */
    float *dbg_z;             /* optional [ (T+T')*B*A ] quantile estimates (tests) or NULL    */
    void *dbg_stamps;         /* diagnostics only (PRISM_DBG & 8): [4096][64] uint64 shader-clock stamps, else NULL */
    void *workspace;          /* >= prism_learner_workspace_bytes(), zero-filled once.  32-bit word 2 of it is the
                                 "target set packed" flag: whoever writes target_params (prism_sync_target's caller,
                                 a checkpoint load) stores 0 there, on the stream; the library sets it.  32-bit word 7
                                 is a sticky status word: bit 0 = a workgroup of the fused tail abandoned its grid
                                 barrier (PRISM_WS_STATUS_BARRIER_TIMEOUT): the step that set it is incomplete     */
    size_t workspace_bytes;
    prism_adam_hyper hyper;
    /* Optional: uint32[4] in pinned, device-mapped HOST memory (hipHostMalloc; NULL = none), zeroed by the caller.  When
     * the library raises sticky bit k of the workspace's status word it also stores 1 into word k here (a plain
     * system-scope store: no PCIe atomics needed), so the host can poll for an abandoned barrier / collective on every
     * step WITHOUT synchronising with the device (the workspace word itself costs a device-to-host copy to read). */
    uint32_t *host_status;
} prism_learner_desc;

/* host: bytes of scratch prism_learner_fwd_bwd needs for (dims, batch). 0 on unsupported dims. */
size_t prism_learner_workspace_bytes(const prism_model_dims *dims, int32_t batch);

/* host: PRISM_OK if the kernels cover this (dims, batch) combination.  The envelope: embed_dim 1024, A 1..16, C 1..10,
 * B 1..4096, squish_fn one of PRISM_SQUISH_*; and
 *   IQN (use_iqn): n_basis 64; T, T' in {4, 8, 16, 32, 64}; B*T and B*T' multiples of 16; and either
 *     iqn_layers 1 with iqn_width 128 or 256 (one trunk layer), or
 *     iqn_layers 0 (iqn_model.py:32-46 with self.model = None: Hadamard product -> [LayerNorm(1024)] -> Linear(1024, A)),
 *     iqn_width ignored as the reference ignores it, and n_heads 0.  Its parameter offsets: iqn_w1 / iqn_b1 / iqn_ln1_* = -1,
 *     the final LayerNorm in iqn_ln2_*, and phi | [LayerNorm] | head contiguous in model.parameters() order;
 *   Q heads: one single-Linear head (head_layers 1) without IQN, or up to 16 two-layer heads of width 128 or 256 with
 *     B % 16 == 0, beside a one-layer IQN trunk or alone.
 * Refused (PRISM_ERR_UNSUPPORTED): iqn_layers >= 2, other widths, Q heads beside a depth-0 IQN (the two-layer ensemble
 * there would need the merged loss launch and the heads' embedding-gradient sum: not built). */
int prism_learner_supported(const prism_model_dims *dims, int32_t batch);

/* host: which launch forms an update of (dims, batch) takes in `gemm_mode` (PRISM_GEMM_*; 0 = the library default), as the
 * learner entry points decide them before they launch.  Read-only, no device call.  Fills out[0 .. PRISM_PLAN_N):
 *   PRISM_PLAN_BWD          the IQN trunk's backward: PRISM_BWD_NONE (no IQN) | PRISM_BWD_FP32 (iqn_bwd_kernel) |
 *                           PRISM_BWD_BW3 (iqn_bwd3_kernel: bf16x3, width 128) | PRISM_BWD_BW4 (iqn_bwd4_kernel: bf16x3,
 *                           width 256) | PRISM_BWD_LIN (the linear head's lin_bwd_kernel)
 *   PRISM_PLAN_Q_BWD        the two-layer Q heads' input-side backward: PRISM_QB_NONE | PRISM_QB_ROWS | PRISM_QB_COLS
 *                           (qh_bwd_kernel by rows / by columns) | PRISM_QB_QB2 (qh_bwd2_kernel)
 *   PRISM_PLAN_CONV_IN_BWD  1: the conv backward's taps are folded into the IQN backward launch; 0: the post launch's
 *   PRISM_PLAN_N_CHUNKS     row chunks of the IQN backward = gradient slabs the post launch sums
 *   PRISM_PLAN_LOCAL_LOSS   1: the IQN loss finishes inside the forward tiles (no loss launch)
 *   PRISM_PLAN_MERGED_LOSS  1: IQN and ensemble loss in one launch
 *   PRISM_PLAN_SPLIT        1: forward GEMMs on the bf16 matrix pipe (three-piece operands)
 *   PRISM_PLAN_Q_DE_SLOTS   embedding-gradient slots of the Q heads the post launch sums
 *   PRISM_PLAN_POST_BLOCKS  workgroups of the post launch (without the priority writeback's)
 * PRISM_ERR_INVALID: dims or out NULL, n_out < PRISM_PLAN_N.  PRISM_ERR_UNSUPPORTED: outside prism_learner_supported's
 * envelope.  Neither sets prism_last_error(), as prism_learner_supported sets none. */
#define PRISM_PLAN_BWD 0
#define PRISM_PLAN_Q_BWD 1
#define PRISM_PLAN_CONV_IN_BWD 2
#define PRISM_PLAN_N_CHUNKS 3
#define PRISM_PLAN_LOCAL_LOSS 4
#define PRISM_PLAN_MERGED_LOSS 5
#define PRISM_PLAN_SPLIT 6
#define PRISM_PLAN_Q_DE_SLOTS 7
#define PRISM_PLAN_POST_BLOCKS 8
#define PRISM_PLAN_N 9
#define PRISM_BWD_NONE 0
#define PRISM_BWD_FP32 1
#define PRISM_BWD_BW3 2
#define PRISM_BWD_BW4 3
#define PRISM_BWD_LIN 4
#define PRISM_QB_NONE 0
#define PRISM_QB_ROWS 1
#define PRISM_QB_COLS 2
#define PRISM_QB_QB2 3
int prism_learner_plan_info(const prism_model_dims *dims, int32_t batch, int32_t gemm_mode, int32_t *out, int32_t n_out);

/* get_losses + backward: fills out_*, grads (complete dL/dparams of
 * mean(dl*w) + mean(ql*w), agent.py:58-64,71-72) — the RCCL all-reduce of `grads` sits between
 * this call and prism_learner_clip_adam in data-parallel runs. */
int prism_learner_fwd_bwd(const prism_learner_desc *ld, prism_stream_t stream);

/* clip_grad_norm_(max_grad_norm) + Adam step (agent.py:73-74; torch.optim.Adam defaults,
 * agent_factory.py:44-47) over the flat buffers; adam_step += 1. */
int prism_learner_clip_adam(const prism_learner_desc *ld, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused hot path — one Learner iteration (prism/learner.py:95-125) in four launches on one GPU (IQN; one or
 * two more with Q heads), five when an all-reduce sits in the middle:
 *   prism_step_front                        PER sample + n-step gather + conv embed (+ LayerNorm helpers)
 *   prism_learner_fwd_bwd (embed_done = 1)  quantile forward tiles with the loss in their tail, column-sliced
 *                                           backward [, post: gradient reduction + first half of the writeback]
 *   [RCCL all-reduce of ld->grads when data-parallel]
 *   prism_step_back                         [fuse_tail: gradient reduction, then behind a grid barrier] clip + Adam,
 *                                           priority writeback with |td|, RNG counters
 * Results are identical to per_sample -> replay_gather -> fwd_bwd -> clip_adam -> per_update.
 * ------------------------------------------------------------------------------------------ */
/* TimestepBuffer.sample (timestep_buffer.py:35-51) fused with the embedding of both observations.
 * Writes the minibatch into ld->obs/next_obs/reward/nonterminal/gamma/action (the static batch),
 * out_index [B] int64 and out_weight [B] (set ld->per_weights = out_weight to use them).
 * rp->tree == NULL selects uniform replay. */
int prism_step_front(const prism_learner_desc *ld, const prism_replay_desc *rp, int64_t size,
                     const float *mass, uint64_t seed, uint64_t offset, float beta,
                     int64_t *out_index, float *out_weight, prism_stream_t stream);

/* prism_step_front sampling from a ring of either storage kind: the three observation-row reads of the launch take
 * one 32-bit word per thread from a byte ring and widen it; the static batch it writes stays fp32, so nothing behind
 * this launch (prism_learner_fwd_bwd, prism_step_back*) knows the kind. */
int prism_step_front_ring(const prism_learner_desc *ld, const prism_replay_desc *rp, int32_t ring_kind, int64_t size,
                          const float *mass, uint64_t seed, uint64_t offset, float beta,
                          int64_t *out_index, float *out_weight, prism_stream_t stream);

/* prism_step_front_ring with the number of stored rows read on the device, for a launch a hipGraph replays while the
 * ring fills: size = min(cursor[slot], rp->capacity), `cursor` the pair of words prism_replay_ingest_cursor keeps (the
 * write serial, which is the ring's size until the ring wraps).  `slot` is by value: it names the word the last ingest
 * launch in front of this one wrote.  The launch only reads the pair.  The kernel clamps the size into [1, capacity]; a
 * word <= 0 raises the sticky bit PRISM_STATUS_FRONT_BAD_SIZE in rp->status and the launch samples as from one row.
 * Everything else, results included, is prism_step_front_ring's at that size. */
int prism_step_front_cursor(const prism_learner_desc *ld, const prism_replay_desc *rp, int32_t ring_kind,
                            const int64_t *cursor, int32_t slot,
                            const float *mass, uint64_t seed, uint64_t offset, float beta,
                            int64_t *out_index, float *out_weight, prism_stream_t stream);

/* prism_learner_clip_adam + prism_per_update(index, |ld->out_td|) in one launch. */
int prism_step_back(const prism_learner_desc *ld, const prism_replay_desc *rp, const int64_t *index,
                    float alpha, float eps, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * The reference's other optimizers (prism/factory/agent_factory.py:40-58): torch.optim.RMSprop(lr, alpha, eps,
 * centered=True) when use_adam is off and use_rmsprop on, torch.optim.SGD(lr) when both are off -- no momentum and no
 * weight decay in either.  prism_adam_hyper and prism_learner_desc keep their layout: the optimizer kind and its own
 * hyper-parameters arrive through the two calls below.  The clip (hyper.max_grad_norm) and hyper.grad_scale still come
 * from ld->hyper.
 *   PRISM_OPT_ADAM     exactly prism_learner_clip_adam / prism_step_back: every Adam hyper-parameter is read from
 *                      ld->hyper, lr / alpha / eps of prism_opt_hyper are ignored; results are bit-identical
 *   PRISM_OPT_RMSPROP  ld->adam_m holds grad_avg, ld->adam_v holds square_avg (torch's state names), float32 [n_params];
 *                      torch/optim/rmsprop.py, _single_tensor_rmsprop, operation by operation in float32.  The radicand
 *                      square_avg - grad_avg^2 is NOT clamped: where rounding leaves it negative the parameter becomes
 *                      NaN, as in the reference
 *   PRISM_OPT_SGD      params -= lr * grad; ld->adam_m / ld->adam_v are neither read nor written, but must still be
 *                      valid 16-byte aligned pointers (the descriptor check is shared)
 * Every kind advances ld->adam_step by one.  The fused tail is built for Adam only: with another kind ld->fuse_tail
 * must be 0 (PRISM_ERR_UNSUPPORTED otherwise -- never a silent Adam step), in these calls AND in the
 * prism_learner_fwd_bwd in front of them, which then reduces the gradient itself.
 * ------------------------------------------------------------------------------------------ */
#define PRISM_OPT_ADAM 0
#define PRISM_OPT_RMSPROP 1
#define PRISM_OPT_SGD 2

typedef struct prism_opt_hyper {
    int32_t kind;          /* PRISM_OPT_*                                                     */
    double lr;             /* config.learning_rate                                            */
    double alpha;          /* RMSprop: config.rmsprop_alpha (decay of both running averages)  */
    double eps;            /* RMSprop: config.rmsprop_epsilon, added to the root              */
} prism_opt_hyper;

/* clip_grad_norm_(max_grad_norm) + optimizer.step() (agent.py:73-74) for the optimizer agent_factory.py:40-58 built:
 * prism_learner_clip_adam with the per-element update of opt->kind; adam_step += 1. */
int prism_learner_clip_step(const prism_learner_desc *ld, const prism_opt_hyper *opt, prism_stream_t stream);

/* prism_learner_clip_step + prism_per_update(index, |ld->out_td|) in one launch: prism_step_back for the optimizer
 * agent_factory.py:40-58 built (the tail of one Learner iteration, prism/learner.py:95-125). */
int prism_step_back_opt(const prism_learner_desc *ld, const prism_opt_hyper *opt, const prism_replay_desc *rp,
                        const int64_t *index, float alpha, float eps, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Acting forward -- Agent.forward (prism/agents/agent.py:31-41): CompositeModel.forward(for_action=True)
 * (composite_model.py:51-70; iqn_model.py:61-87 with n_quantile_samples_per_action rows per observation;
 * q_ensemble.py:44-48) on the learner's parameters and workspace, with the same forward tiles as the update.
 *   obs      [n][10][10][C], 1 <= n <= ld->batch (Q heads: the 16-padded n as well); device memory, or pinned
 *            device-mapped host memory read in place (no host-to-device copy in front of a small batch)
 *   tau_in   [n_tau*n] tau-major (row = t*n + b, iqn_model.py:66-70) or NULL -> Philox(seed, offset)
 *   out_z    [ceil16(n*n_tau)][A]  quantile estimates, SAMPLE-major (row = b*n_tau + t); reference layout =
 *            view(n, n_tau, A).permute(1, 0, 2)
 *   out_q    [heads][ceil16(n)][A] ensemble estimates; reference layout = [:, :n].permute(1, 2, 0)
 *            (the single-Linear DQN head, dqn_n_model_layers = 1: heads = 1, one workgroup per observation)
 * Either output may be NULL when the model has no such part.
 * Quantile draws: Philox(seed, offset [+ ld->rng_counters[2] when ld->rng_counters is set and tau_in is NULL; the call then
 * advances that device word by n * n_tau: capture the call into a hipGraph and every replay draws fresh samples]). */
int prism_act_forward(const prism_learner_desc *ld, const float *obs, int32_t n, int32_t n_tau,
                      const float *tau_in, uint64_t seed, uint64_t offset, float *out_z, float *out_q,
                      prism_stream_t stream);

/* Risk-sensitive acting (config.iqn_risk_policy_id; Dabney et al. 2018, "Risk-sensitive reinforcement learning"): the
 * quantile samples of one acting forward, passed through a distortion beta, for prism_act_forward's tau_in.
 *   out_tau[t*n + b] = float32(beta(u)), u = tau_raw_in ? tau_raw_in[t*n + b]
 *     : float32(Philox4x32-10(seed, c0 + t*n + b, "TAU0" + 3)[0] >> 8) * 2^-24        (the acting forward's own draw)
 *   beta is evaluated in float64 from the float32 u and narrowed once:
 *     PRISM_RISK_NEUTRAL  u
 *     PRISM_RISK_CVAR     eta * u                                                 0 < eta <= 1
 *     PRISM_RISK_WANG     Phi(Phi^-1(u) + eta)                                    eta finite (< 0: risk-averse)
 *     PRISM_RISK_CPW      u^eta / (u^eta + (1 - u)^eta)^(1 / eta)                 0 < eta <= 1
 *     PRISM_RISK_POW      eta >= 0: u^(1 / (1 + |eta|)); eta < 0: 1 - (1 - u)^(1 / (1 + |eta|))     eta finite
 *   every one maps 0 to 0 (Wang through Phi^-1(0) = -inf) and [0, 1] into [0, 1].
 *   c0 = offset, plus rng_counters[2] when rng_counters is set and tau_raw_in is NULL; the launch then leaves that word
 *   advanced by n * n_tau, exactly as prism_act_forward with tau_in == NULL does: the prism_act_forward behind it takes
 *   out_tau as tau_in with ld->rng_counters unset.  With tau_raw_in the word is neither read nor written.
 * The word while the launch runs: one lane per sample, ceil(n * n_tau / 256) workgroups, and every workgroup has to read the
 * count before any advances it.  One atomic add per workgroup is both its read and its ticket; the tickets stand in bits
 * 42 .. 61 (fewer than 2^20 workgroups: n * n_tau < 2^28), the count in bits 0 .. 41 and 62 .. 63 -- a count is
 * k * 2^62 + c with c + n * n_tau < 2^42, which covers the training counts and those of evaluations (2^62 + c).  The holder
 * of the last ticket takes the tickets off and adds n * n_tau: between launches the word is the plain count, and its value
 * does not depend on the order of the workgroups.  Calls on one word must follow each other on the device.
 * out_tau_raw (optional) [n_tau*n]: the raw samples u. */
#define PRISM_RISK_NEUTRAL 0
#define PRISM_RISK_CVAR 1
#define PRISM_RISK_WANG 2
#define PRISM_RISK_CPW 3
#define PRISM_RISK_POW 4
int prism_act_tau_distort(int32_t n, int32_t n_tau, int32_t policy, double eta, const float *tau_raw_in, uint64_t seed,
                          uint64_t offset, uint64_t *rng_counters, float *out_tau, float *out_tau_raw, prism_stream_t stream);

/* IDSActionSelector.generate_action_probs + select_action for ids_use_random_samples = False
 * (prism/agents/action_selectors.py:125-176): scores [n][A] = regret^2 / information gain, action [n] = argmin.
 * z / q: the buffers prism_act_forward filled.  out_aux (optional) [n][4][A]: ensemble mean, ensemble spread
 * (torch.std), return-distribution variance, information gain -- what the selector logs.  out_action_host (optional): a
 * second destination of the actions -- pinned, device-mapped host memory, so that the caller needs no device-to-host copy.
 * unsquish_fn (PRISM_SQUISH_*): the selector's unsquish function, applied to both estimate arrays first (:128-130). */
int prism_ids_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                     int32_t n_heads, float lmbda, float epsilon, float rho_lower_bound, int32_t unsquish_fn,
                     float *out_scores, float *out_aux, int64_t *out_action, int64_t *out_action_host, prism_stream_t stream);

/* IDSActionSelector.generate_action_probs + select_action for ids_use_random_samples = True
 * (prism/agents/action_selectors.py:125-176; :150-152 the probabilities, :175 the draw).  Scores and out_aux: those of
 * prism_ids_select, bit for bit (one device routine).  Per observation b, fp32 unless stated:
 *   p_a = min(max(softmax_a(-scores), epsilon), 1)           (max subtracted first; NOT renormalised after the clamp:
 *                                                             torch.multinomial samples proportionally to its weights)
 *   u   = u_in[b] (float64, parity input) when u_in is given, else the 53-bit uniform of the first two words of
 *         Philox4x32-10(seed, c0 + b, "IDSA" = 0x49445341): a stream key apart from "TAU0" + sid, "PERM" and "UNIF"
 *   c0  = offset when rng_counters is NULL (the caller's acting-draw count at the start of this call's forward), else
 *         offset + rng_counters[2] - n * n_tau: prism_act_forward, earlier on the same stream or in the same hipGraph,
 *         has advanced that word by its n * n_tau draws; the word is read, never written.  A forward consumes
 *         n * n_tau >= n counts, so the ranges [c0, c0 + n) of successive calls cannot overlap.
 *   action = first a with u * S < p_0 + ... + p_a in float64, index order, S = p_0 + ... + p_(A-1); A - 1 if none.
 * out_probs (optional) [n][A]: the clamped probabilities; out_action [n]; out_action_host as for prism_ids_select. */
int prism_ids_sample_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                            int32_t n_heads, float lmbda, float epsilon, float rho_lower_bound, int32_t unsquish_fn,
                            const double *u_in, uint64_t seed, uint64_t offset, const uint64_t *rng_counters,
                            float *out_scores, float *out_aux, float *out_probs, int64_t *out_action,
                            int64_t *out_action_host, prism_stream_t stream);

/* GreedyActionSelector.generate_action_probs + select_action (prism/agents/action_selectors.py:70-83; also the greedy
 * branch of EGreedyActionSelector, :24-45): action [n] = argmax_a mean(q_estimates[:, a, :]).  q != NULL: mean over the
 * n_heads ensemble estimates prism_act_forward left in out_q; q == NULL: mean over the n_tau quantile estimates in z
 * (composite_model.py:66-68, models without Q heads).  out_mean (optional) [n][A]; out_action_host as for prism_ids_select. */
int prism_greedy_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                        int32_t n_heads, int64_t *out_action, float *out_mean, int64_t *out_action_host,
                        prism_stream_t stream);

/* MinRegretActionSelector.generate_action_probs + select_action (prism/agents/action_selectors.py:85-111): act on the
 * ensemble's pessimistic bound.  q: the [n_heads][n_pad][A] ensemble estimates prism_act_forward left in out_q, the only
 * input; rows n .. n_pad - 1 are never read.  Per observation and action, fp32, sums in head order, unsquish_fn
 * (PRISM_SQUISH_*, :93-94) applied to every estimate first:
 *   mean   = (q_0 + ... + q_(H-1)) / H                        spread = sqrt(sum_h (q_h - mean)^2 / (H - 1))   (:96-97,
 *            torch.std, unbiased; "variance" there)           sd     = sqrt(spread)                            (:99)
 *   regret = max_a(mean + lmbda * sd) - (mean - lmbda * sd)   score  = regret^2                               (:101-103)
 *   action = first arg-min of the scores                                                                      (:104)
 * mean and spread are prism_ids_select's, bit for bit.  n_heads 2..16: one head has no spread (NaN in the reference).
 * out_scores (optional) [n][A]: regret^2; out_aux (optional) [n][2][A]: mean | spread; out_action [n]; out_action_host as
 * for prism_ids_select. */
int prism_min_regret_select(const float *q, int32_t n, int32_t n_pad, int32_t n_actions, int32_t n_heads, float lmbda,
                            int32_t unsquish_fn, float *out_scores, float *out_aux, int64_t *out_action,
                            int64_t *out_action_host, prism_stream_t stream);

/* SimpleIDSActionSelector.generate_action_probs + select_action for random_sample = False
 * (prism/agents/action_selectors.py:195-286), q_estimates read as the class is written: a sequence over heads of [n, A]
 * estimates.  q as for prism_min_regret_select.  Per observation and action, fp32, unsquish_fn applied to every estimate
 * first (:215-216):
 *   mean     = (q_0 + ... + q_(H-1)) / H, summed in head order                                                (:213-218)
 *   max_diff = max_h q_h - min_h q_h: the reference's max over pairs i < j of |q_i - q_j| (:226-230) exactly, fp32
 *              rounding being monotone; 0 with one head
 *   q_values = mean - (mean_0 + ... + mean_(A-1)) / A, summed in action order                                 (:247)
 *   scaled   = (float)(1 - beta) * max_diff + q_values * (float)beta, 1 - beta formed in double               (:250)
 *   action   = first arg-max of the scaled values                                                             (:252)
 * The quantile_difference of :244-245 is computed there and never used: not here.  n_heads 1..16.
 * out_scores (optional) [n][A]: scaled; out_aux (optional) [n][3][A]: mean | max_diff | q_values; out_action [n];
 * out_action_host as for prism_ids_select. */
int prism_simple_ids_select(const float *q, int32_t n, int32_t n_pad, int32_t n_actions, int32_t n_heads, double beta,
                            int32_t unsquish_fn, float *out_scores, float *out_aux, int64_t *out_action,
                            int64_t *out_action_host, prism_stream_t stream);

/* EGreedyActionSelector (prism/agents/action_selectors.py:24-45) with the coin tossed PER OBSERVATION: the reference (and
 * the agent's default) tosses one coin for the whole call, which makes N lock-stepped environments explore together or not
 * at all.  Row b of this launch is row row0 + b of a call of n_call rows (row0 = 0, n_call = n: the whole call in one
 * launch; a call in pieces hands every piece its row0 and the whole call's n_call, and equals the call in one piece).
 *   greedy = prism_greedy_select's action on the same buffers, bit for bit (one device routine); out_mean as there
 *   s0     = steps0 when steps_word is NULL, else steps0 + *steps_word: the rows seen before this call, the selector's
 *            epsilon.current_step
 *   eps    = ONE value per call, LinearAnneal.get_value() after epsilon.update(n_call), i.e. at s = s0 + n_call
 *            (prism/util/annealing_strategies.py:22-33), float64 in the reference's operation order: eps_stop if
 *            anneal_steps == 0 || s >= anneal_steps, else f = min(1, s / anneal_steps), eps_start * (1 - f) + eps_stop * f
 *   r      = Philox4x32-10(seed, s0 + row0 + b, "EGRD" = 0x45475244): a stream key apart from "TAU0" + sid, "PERM", "UNIF"
 *            and "IDSA".  Every row seen has a counter of its own: the ranges [s0, s0 + n_call) of successive calls touch
 *            and never overlap.
 *   u      = u_in[row0 + b] (float64, parity input) when u_in is given, else the 53-bit uniform of r[0], r[1]
 *   action = (uint32)(((uint64)r[2] * n_actions) >> 32) if u < eps (eps = 1 always explores, eps = 0 never), else greedy
 * steps_word (optional, device): a uint64 count of rows seen that the call ADVANCES by n_call, so that a call captured into a
 * hipGraph draws fresh at every replay.  Needs the whole call in one launch (row0 == 0, n_call == n < 2^20) and counts
 * below 2^44: while the launch runs, bits 44 and up hold one ticket per workgroup -- a workgroup's one atomic add is both its
 * read of the count and its ticket, and the holder of the last ticket takes the tickets off and adds n_call.  No workgroup
 * reads the word after it has advanced, and its value after the call does not depend on their order.  Calls on one word
 * must follow each other on the device (one stream, or one hipGraph after another).
 * out_epsilon (optional) [1] float64; out_explored (optional) [n] 1 / 0; out_action [n]; out_action_host as for
 * prism_ids_select. */
int prism_egreedy_select(const float *z, const float *q, int32_t n, int32_t n_pad, int32_t n_tau, int32_t n_actions,
                         int32_t n_heads, double eps_start, double eps_stop, int64_t anneal_steps, uint64_t seed,
                         uint64_t steps0, int32_t row0, int32_t n_call, uint64_t *steps_word, const double *u_in,
                         float *out_mean, double *out_epsilon, uint8_t *out_explored, int64_t *out_action,
                         int64_t *out_action_host, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MinAtar Breakout on the device: n_envs environments stepped in lockstep, one launch per step (DESIGN.md 7.3 has the
 * rules: a restatement of MinAtar v1, not checked against the `minatar` package).  Observations are [n_envs][10][10][4],
 * values 0 / 1, fp32 (PRISM_OBS_F32) or uint8 (PRISM_OBS_U8); channel 0 paddle, 1 ball, 2 the ball's last cell, 3 bricks.
 *
 * State block: PRISM_ENV_STATE_WORDS uint32 per environment,
 *   [0] bricks, bit 10 (y - 1) + x for rows y = 1..3 (no other row ever holds one)
 *   [1] pos (bits 0-3) | ball_x (4-7) | ball_y (8-11) | ball_dir (12-13) | last_x (16-19) | last_y (20-23) | strike (24) |
 *       last_action (25-27; the game's action 0..5 after the 3-action map)
 *   [2] ep_steps   [4], [5] t, the environment's lifetime step count (low, high)   [3], [6], [7] zero
 * obs[2] are the two ping-pong buffers of the observation to act on: a reset writes obs[0]; a step with `parity` p -- the
 * buffer that holds the current acting observation -- writes obs[p ^ 1] and does not touch obs[p], which the caller may
 * still hand to the replay ingestion.  A step also writes next_obs (the image after the step, BEFORE any reset; obs[p ^ 1]
 * is the same image unless the episode ended, then that of the fresh episode), reward (0 or 1), done, truncated.
 * Draws: r = Philox4x32-10(seed, t, (env << 32) | "ENVB" = 0x454E5642) with t the count BEFORE the step; the sticky coin is
 * the 53-bit uniform of r[0], r[1], r[2] & 1 the side of the episode that begins if this step ends one; the first episode's
 * side is r[3] & 1 of the draw at counter 2^64 - 1.  u_in / side_in / first_side_in (optional, device, [n_envs]) replace
 * them: the parity path.
 * actions: [n_envs] int64 on the device, read in place.  n_actions 6: n, l, u, r, d, f (only l = 1 and r = 3 act);
 * n_actions 3: 0 -> n, 1 -> l, 2 -> r.  An action outside [0, n_actions) acts as no-op and ORs
 * PRISM_ENV_STATUS_BAD_ACTION into *status (sticky; the host reads it when it likes, never per step).
 * Neither launch takes a host value that changes from step to step except `parity`: a captured step replays as is and
 * writes the buffer it wrote at capture.  Calls on one descriptor must follow each other on the device.
 * ------------------------------------------------------------------------------------------ */
#define PRISM_ENV_STATE_WORDS 8
#define PRISM_ENV_MAX 65536
#define PRISM_ENV_STATUS_BAD_ACTION 1u
typedef struct prism_env_desc {
    int32_t n_envs, n_actions;      /* n_envs in [1, PRISM_ENV_MAX]; n_actions 6 or the game's minimal set: 3 in Breakout
                                       and Freeway, 5 in Asterix, 4 in Space Invaders */
    int32_t step_limit;             /* > 0: truncate an episode after that many steps; 0: never */
    int32_t obs_kind;               /* PRISM_OBS_F32 | PRISM_OBS_U8 */
    double sticky_p;                /* in [0, 1]: probability that a step repeats the action before it */
    uint64_t seed;
    uint32_t *state;                /* [n_envs][PRISM_ENV_STATE_WORDS], 16-byte aligned */
    uint32_t *status;               /* [1] */
    void *obs[2];                   /* 16-byte aligned */
    void *next_obs;                 /* 16-byte aligned */
    float *reward;                  /* [n_envs] */
    uint8_t *done, *truncated;      /* [n_envs] 1 / 0 */
} prism_env_desc;
/* every environment: a fresh first episode, t = 0, last_action = 0, the acting observation in obs[0] */
int prism_env_breakout_reset(const prism_env_desc *d, const uint8_t *first_side_in, prism_stream_t stream);
int prism_env_breakout_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *side_in,
                            int32_t parity, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MinAtar Freeway on the device, behind the same descriptor, checks, ping-pong contract, action checks and status word as
 * Breakout above (DESIGN.md 7.4 has the rules: a restatement of MinAtar v1, not checked against the `minatar` package).
 * Observations are [n_envs][10][10][7], values 0 / 1, fp32 or uint8; channel 0 the chicken at (pos, 4), 1 the cars at
 * (y, x), 1 + |speed| (2..6) the trail cell of a car at (y, x - 1) for speed > 0, else (y, x + 1), wrapped to 0..9.
 * An environment's image is 2800 bytes in fp32 and 700 bytes in uint8: the buffers are 16-byte aligned at their base, a
 * byte image inside them at 4 bytes only.
 *
 * State block: PRISM_ENV_STATE_WORDS uint32 per environment; car i = 0..7 is on row y = i + 1,
 *   [0] x of car i (0..9) in bits 4i .. 4i+3
 *   [1] timer of car i (0..5) in bits 3i .. 3i+2 | direction of car i in bit 24 + i (1: speed > 0, moves to +x)
 *   [2] ep_steps
 *   [3] |speed| of car i (1..5) in bits 3i .. 3i+2
 *   [4], [5] t, the environment's lifetime step count (low, high)
 *   [6] pos (bits 0-3) | move_timer (4-5) | terminate_timer (6-17, 0..2500) | last_action (18-20; the game's action 0..5
 *       after the 3-action map)
 *   [7] zero
 * Draws, with t the count BEFORE the step and one stream key per purpose: the sticky coin is the 53-bit uniform of words
 * 0, 1 of Philox4x32-10(seed, t, (env << 32) | "FWYC" = 0x46575943).  A set of eight speeds is the four words of the draw
 * under a first key (cars 0-3) and the four under a second (cars 4-7), |speed| = 1 + (((uint64_t)(w >> 1) * 5) >> 31),
 * direction + if w & 1: the win set under "FWW0", "FWW1" = 0x46575730, 0x46575731 at counter t, drawn only on a step
 * that wins; the reset set under "FWR0", "FWR1" = 0x46575230, 0x46575231 at counter t, drawn only on a step that ends an
 * episode; the first episode's speeds are the reset set at counter 2^64 - 1.  u_in ([n_envs] double) replaces the coin;
 * speeds_in ([n_envs][8] int8, each +-1 .. +-5) replaces BOTH sets of that step, first_speeds_in the reset's: the parity
 * path.
 * actions: [n_envs] int64 on the device, read in place.  n_actions 6: n, l, u, r, d, f (only u = 2 and d = 4 act);
 * n_actions 3: 0 -> n, 1 -> u, 2 -> d.  Out of range: as Breakout.
 * ------------------------------------------------------------------------------------------ */
int prism_env_freeway_reset(const prism_env_desc *d, const int8_t *first_speeds_in, prism_stream_t stream);
int prism_env_freeway_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const int8_t *speeds_in,
                           int32_t parity, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MinAtar Asterix on the device, behind the same descriptor, checks (but n_actions must be 5 or 6), ping-pong contract,
 * action checks and status word as Breakout above (DESIGN.md 7.5 has the rules: a restatement of MinAtar v1, not checked
 * against the `minatar` package).  Observations are [n_envs][10][10][4], values 0 / 1, fp32 or uint8; channel 0 the player
 * at (py, px), 1 an enemy at (y, x), 3 a gold at (y, x), 2 the trail cell of either at (y, x - dir) where that column is
 * in 0..9 (no wrap).
 *
 * State block: PRISM_ENV_STATE_WORDS uint32 per environment; entity slot i = 0..7 is row y = i + 1 and is empty or holds
 * one entity; every field of an empty slot is zero,
 *   [0] x of slot i (0..9) in bits 4i .. 4i+3
 *   [1] slot i occupied in bit i | its direction in bit 8 + i (1: dir = +1, moves to +x) | gold in bit 16 + i
 *   [2] ep_steps
 *   [3] px (bits 0-3) | py (4-7, 1..8) | spawn_speed (8-11, 1..10) | spawn_timer (12-15, 0..10) | move_speed (16-18, 1..5) |
 *       move_timer (19-21, 0..5) | last_action (22-24, 0..5) | ramp_index (25-29)
 *   [4], [5] t, the environment's lifetime step count (low, high)
 *   [6] ramp_timer + 1 (bits 0-6: ramp_timer is -1..100)
 *   [7] zero
 * Draws, with t the count BEFORE the step and one stream key per purpose: the sticky coin is the 53-bit uniform of words
 * 0, 1 of Philox4x32-10(seed, t, (env << 32) | "ASXC" = 0x41535843).  A spawn takes the words w of the draw under
 * "ASXS" = 0x41535853 at counter t, drawn only on a step that spawns: side = w[0] & 1 (1: x = 0 moving to +x, 0: x = 9
 * moving to -x), gold = (((uint64_t)w[1] * 3) >> 32) == 0, and among the k empty slots in ascending order the one of
 * rank ((uint64_t)w[2] * k) >> 32.  A reset draws nothing.  u_in ([n_envs] double) replaces the coin; spawn_in
 * ([n_envs][3] uint8: side 0 / 1, gold 0 / 1, rank 0..7, a rank >= k taken as k - 1) replaces the spawn draw of that step:
 * the parity path.
 * actions: [n_envs] int64 on the device, read in place.  n_actions 6: n, l, u, r, d, f (f does nothing); n_actions 5:
 * n, l, u, r, d.  Out of range: as Breakout.
 * ------------------------------------------------------------------------------------------ */
int prism_env_asterix_reset(const prism_env_desc *d, prism_stream_t stream);
int prism_env_asterix_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *spawn_in,
                           int32_t parity, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MinAtar Space Invaders on the device, behind the same descriptor, checks (but n_actions must be 4 or 6), ping-pong
 * contract, action checks and status word as Breakout above (DESIGN.md 7.6 has the rules: a restatement of MinAtar v1, not
 * checked against the `minatar` package).  Observations are [n_envs][10][10][6], values 0 / 1, fp32 or uint8; channel 0 the
 * cannon at (9, pos), 1 the aliens, 2 the aliens again while they move to -x, 3 the aliens again while they move to +x,
 * 4 the friendly bullets, 5 the enemy bullets.  An environment's image is 2400 bytes in fp32 and 600 bytes in uint8: the
 * buffers are 16-byte aligned at their base, a byte image inside them at 4 bytes only.
 *
 * State block: PRISM_ENV_STATE_WORDS uint32 per environment.  The aliens are a rigid block of 4 rows x 6 columns: the alien
 * of block cell (r, c) stands on board cell ((alien_y + r) mod 10, alien_x + c); a live alien's column is on the board.  A
 * bullet map holds at most one bullet per board row: the field of row y is x + 1, 0 for none (play never puts a second
 * bullet into a row; placing one replaces the row's field),
 *   [0] block cell (r, c) alive in bit 6r + c (bits 0-23, never all zero) | alien_x + 5 (bits 24-27, alien_x is -5..9) |
 *       alien_y (28-31, 0..9)
 *   [1] friendly bullet field of row y = 0..7 in bits 4y .. 4y+3
 *   [2] ep_steps
 *   [3] enemy bullet field of row y = 0..7 in bits 4y .. 4y+3
 *   [4], [5] t, the environment's lifetime step count (low, high)
 *   [6] friendly bullet fields of rows 8, 9 (bits 0-3, 4-7) | enemy bullet fields of rows 8, 9 (8-11, 12-15) | pos (16-19) |
 *       shot_timer (20-22, 0..5) | direction (23; 1: alien_dir = +1) | last_action (24-26; the game's action 0..5 after the
 *       4-action map)
 *   [7] alien_move_timer (bits 0-3, 0..12) | alien_shot_timer (4-7, 0..10) | enemy_move_interval (8-11, 6..12) |
 *       ramp_index (12-14, 0..6)
 * Draws: only the sticky coin, the 53-bit uniform of words 0, 1 of Philox4x32-10(seed, t, (env << 32) | "SPIC" =
 * 0x53504943) with t the count BEFORE the step; a reset draws nothing.  u_in ([n_envs] double) replaces the coin: the
 * parity path.  There is no other draw, so neither entry point takes a draw array.
 * actions: [n_envs] int64 on the device, read in place.  n_actions 6: n, l, u, r, d, f (only l = 1, r = 3 and f = 5 act);
 * n_actions 4: 0 -> n, 1 -> l, 2 -> r, 3 -> f.  Out of range: as Breakout.
 * ------------------------------------------------------------------------------------------ */
int prism_env_invaders_reset(const prism_env_desc *d, prism_stream_t stream);
int prism_env_invaders_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, int32_t parity,
                            prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * MinAtar Seaquest on the device, behind the same descriptor, checks (but n_actions must be 6: the minimal set is all six),
 * ping-pong contract, action checks and status word as Breakout above (DESIGN.md 7.7 has the rules: a restatement of MinAtar
 * v1, not checked against the `minatar` package).  Observations are [n_envs][10][10][10], values 0 / 1, fp32 or uint8;
 * channel 0 the sub at (sub_y, sub_x), 1 the cell behind it, 2 friendly bullets, 3 the trail cell behind every fish, enemy
 * sub and diver (only on the board), 4 enemy bullets, 5 fish, 6 enemy subs, 7 the oxygen gauge (row 9, columns
 * 0 .. oxygen * 10 / 200 - 1), 8 the diver gauge (row 9, columns 9 - diver_count .. 8), 9 divers.
 *
 * State block: d->state is [n_envs][PRISM_ENV_SEAQUEST_STATE_WORDS] uint32 -- the row width belongs to the game, the
 * descriptor is unchanged.  The game's five ordered lists are fixed-capacity arrays in list order; removal compacts them
 * stably, an empty slot is all zeros,
 *   [0] sub_x (bits 0-3) | sub_y (4-7, 0..8) | sub_or (8; 1: faces +x) | surface (9) | shot_timer (10-12, 0..5) |
 *       diver_count (13-15, 0..6) | last_action (16-18) | move_speed (19-21, 2..5) | ramp_index (22-26, 0..19)
 *   [1] oxygen + 1 (bits 0-7; oxygen is -1..200) | e_spawn_speed (8-12, 1..20) | e_spawn_timer (13-17, 0..20) |
 *       d_spawn_timer (18-22, 0..30)
 *   [2] ep_steps   [4], [5] t, the environment's lifetime step count (low, high)   [3], [6], [7] zero
 *   [8 .. 39] fish   [40 .. 71] enemy subs   [72 .. 103] enemy bullets   [104 .. 107] friendly bullets   [108 .. 111] divers
 * An entry: x (bits 0-3) | y (4-7) | direction (8; 1: moves to +x) | move_timer (9-11, 0..5; 0 in a bullet) | shot_timer
 * (12-15, 0..10; enemy subs only) | present (16).
 * An append to a full array is dropped and ORs PRISM_ENV_STATUS_OVERFLOW into *status (sticky, as the bad-action bit).
 * Draws, with t the count BEFORE the step and one stream key per purpose: the sticky coin is the 53-bit uniform of words
 * 0, 1 of Philox4x32-10(seed, t, (env << 32) | "SQXC" = 0x53515843).  An enemy spawn takes the words w of the draw under
 * "SQXE" = 0x53515845 at counter t, drawn only on a step whose e_spawn_timer is 0: side = w[0] & 1 (1: x = 0 moving to +x,
 * 0: x = 9 moving to -x), is_sub = (((uint64_t)w[1] * 3) >> 32) == 0, row = 1 + (w[2] >> 29).  A diver spawn takes the draw
 * under "SQXD" = 0x53515844, only on a step whose d_spawn_timer is 0: side = w[0] & 1, row = 1 + (w[1] >> 29).  A reset
 * draws nothing.  u_in ([n_envs] double) replaces the coin; draws_in ([n_envs][5] uint8: enemy side, is_sub, row 1..8; diver
 * side, row 1..8) replaces both spawn draws of that step: the parity path.
 * actions: [n_envs] int64 on the device, read in place: n, l, u, r, d, f.  Out of range: as Breakout.
 * ------------------------------------------------------------------------------------------ */
#define PRISM_ENV_SEAQUEST_STATE_WORDS 112
#define PRISM_ENV_STATUS_OVERFLOW 2u
int prism_env_seaquest_reset(const prism_env_desc *d, prism_stream_t stream);
int prism_env_seaquest_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *draws_in,
                            int32_t parity, prism_stream_t stream);

/* Agent.sync_target_model (agent.py:149-152): target := online (device-to-device copy). */
int prism_sync_target(float *target_params, const float *params, int64_t n_params,
                      prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Direct all-reduce (sum) of the flat gradient over peer-mapped buffers -- the data-parallel step's one exchange
 * (the reference has no collective: prism/learner.py:95-125 is a single process).  An
 * alternative to the RCCL all-reduce between prism_learner_fwd_bwd and prism_step_back for the 0.8 - 6 MB messages of
 * this path on a fully connected xGMI node: two shots, every GPU pulling 1/world of the buffer from all peers at once.
 *   bufs[s]   rank s's gradient buffer as mapped into THIS process (own buffer at [rank]); the host maps the peers
 *             (hipIpcGetMemHandle / hipIpcOpenMemHandle, or the sharing of its tensor library)
 *   flags[s]  rank s's flag array, PRISM_MAX_PEERS + 2 uint32 zeroed once, mapped likewise (use_flags only)
 * prism_direct_reduce_scatter: slice `rank` of the own buffer := sum over s = 0..world-1 (in that order) of slice `rank`
 * of bufs[s];  prism_direct_all_gather: every other slice := its owner's.  Afterwards all ranks hold bit-identical sums.
 * Synchronisation: all ranks must have finished writing before the reduce-scatter, finished the reduce-scatter before
 * the all-gather, and finished the all-gather before anyone overwrites its buffer.  use_flags = 0: the CALLER provides
 * these three barriers (the only legal form when ranks share a device); use_flags = 1 (one device per rank): one-workgroup
 * kernels signal and poll the flag arrays on the stream (phase numbers come from a counter in the flag array itself, so the
 * calls may be captured into a hipGraph and replayed).
 *
 * Memory types (every word another DEVICE reads or writes while a kernel runs):
 *   flags[s]  MUST be fine-grained / uncached device memory -- prism_direct_flags_alloc() -- not an ordinary hipMalloc
 *             (coarse-grained) allocation: a store from a peer into coarse-grained memory is only guaranteed visible at
 *             kernel boundaries, a kernel polling it may spin on a stale L2 line.  (RCCL keeps its flags the same way.)
 *   bufs[s]   ordinary (coarse-grained) device memory: written by kernels that END before the flag announcing them is
 *             stored (the end of a kernel writes its L2 back at system scope), read by kernels that START after the wait
 *             kernel has ended (the start of a kernel invalidates).  No kernel ever reads a peer's gradient word that is
 *             written while it runs.
 * Failure: a wait that is not through after `wait_seconds` (0 = 30 s; RCCL would wait for ever, a rank that saves a
 * checkpoint or captures a graph can stall for seconds) gives up: it sets flags[rank][PRISM_MAX_PEERS] (sticky; bit 0),
 * stores the mark 2 into flags[s][PRISM_MAX_PEERS] of EVERY peer s (a plain system-scope store, made in the launch that
 * gave up, i.e. before this rank's next announcement), ORs PRISM_WS_STATUS_COLLECTIVE_TIMEOUT into *poison and into
 * *host_status when given, and every later kernel of the collective returns at once, as do prism_step_back /
 * prism_learner_clip_adam of a learner whose workspace status word is `poison`.  The rank goes on announcing its phases, so
 * its peers do not wait out their own bound on it; but every wait, once through, reads the own sticky slot, and a peer
 * that finds it set -- by its own wait or by a mark -- poisons ITS step in the same way before the launch behind the wait
 * starts.  So: the step of the rank that timed out applies NO update (never a partial sum); neither does the step of any
 * peer whose next wait ends after the mark has landed, which is every peer when the give-up was in phase 1 or 2 (a peer
 * cannot pass phase 3 without this rank's phase-3 announcement, and that is stored after the mark).  A rank that gives
 * up in phase 3 has gathered everything, and a peer may be through its last wait already: that peer applies the step's
 * (complete) update and is stopped at the first wait of the next step.  The state is terminal on every rank: the sticky
 * slots are never cleared, every wait kernel re-raises the poison bit while its slot is set, and the host sees the bit at
 * its next poll; the way out is a new set of flag arrays on all ranks together.
 * ------------------------------------------------------------------------------------------ */
#define PRISM_MAX_PEERS 8
#define PRISM_DIRECT_FLAG_WORDS (PRISM_MAX_PEERS + 2)
#define PRISM_IPC_HANDLE_BYTES 64
typedef struct prism_direct_desc {
    int32_t world, rank;
    float *bufs[PRISM_MAX_PEERS];
    uint32_t *flags[PRISM_MAX_PEERS];
    int64_t n;             /* floats */
    uint32_t *poison;      /* optional device word (the learner workspace's status word): see Failure above */
    uint32_t *host_status; /* optional pinned, device-mapped host words [4]: see prism_learner_desc.host_status */
    double wait_seconds;   /* bound of one flag wait; 0 = 30 s */
} prism_direct_desc;
int prism_direct_reduce_scatter(const prism_direct_desc *d, int32_t use_flags, prism_stream_t stream);
int prism_direct_all_gather(const prism_direct_desc *d, int32_t use_flags, prism_stream_t stream);
/* One synchronisation point of the protocol as its own launch: phase 1 (gradients written), 2 (slices reduced) or 3
 * (slices gathered; its wait advances the all-reduce count), what = 1 announce to the peers, 2 wait for them, 3 both
 * (what use_flags = 1 enqueues).  For callers that pace the phases from the host -- announce, host barrier, wait, the
 * use_flags = 0 kernel -- e.g. ranks that SHARE a device, where a kernel that spins would keep the peer it waits for
 * off the device: the flag addressing and the phase arithmetic run exactly as on the step's path. */
int prism_direct_phase(const prism_direct_desc *d, int32_t phase, int32_t what, prism_stream_t stream);

/* host, synchronous (set-up time, never on the step's path).  The flag array of one rank: PRISM_DIRECT_FLAG_WORDS uint32
 * of UNCACHED (fine-grained) device memory on the current device, zeroed, plus its inter-process handle
 * (hipIpcGetMemHandle; PRISM_IPC_HANDLE_BYTES bytes the host ships to the peers however it likes). */
int prism_direct_flags_alloc(uint32_t **flags_out, void *ipc_handle_out);
int prism_direct_flags_free(uint32_t *flags);
/* map a peer's flag array into this process (hipIpcOpenMemHandle) / unmap it */
int prism_direct_flags_open(const void *ipc_handle, uint32_t **flags_out);
int prism_direct_flags_close(uint32_t *flags);
/* hipDeviceEnablePeerAccess(peer_device) from the current device, explicitly (idempotent; PRISM_ERR_HIP when the two
 * devices have no peer path) -- a mapped peer buffer is only dereferenceable after this. */
int prism_direct_enable_peer(int32_t peer_device);
/* copy the PRISM_DIRECT_FLAG_WORDS words of the own flag array to the host (synchronises with `stream`) */
int prism_direct_flags_read(const uint32_t *flags, uint32_t *host_out, prism_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optional per-kernel timing with HIP events on the launch stream (used by bench.py for the
 * roofline figure; off by default, adds two event records per instrumented launch).
 * Kernel ids: 0 embed, 1 fwd_tile, 2 loss, 3 bwd, 4 post, 5 front, 6 clip_adam, 7 per_sample,
 * 8 gather, 9 per_update, 10 back, 11 q_loss, 12 q_bwd, 13 tail (post + clip + Adam in one launch).
 * ------------------------------------------------------------------------------------------ */
#define PRISM_N_KERNEL_IDS 16
/* on != 0: instrument every launch issued by the calling thread until switched off */
int prism_profile_enable(int on);
/* host: synchronises the recorded events, ADDS elapsed milliseconds and launch counts per kernel id
 * into ms_sum[PRISM_N_KERNEL_IDS] / count[PRISM_N_KERNEL_IDS], and recycles the events. */
int prism_profile_collect(double *ms_sum, int64_t *count);
const char *prism_profile_kernel_name(int id);

#ifdef __cplusplus
}
#endif
#endif /* PRISM_HIP_H */
