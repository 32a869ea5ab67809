// prism_step_front_cursor's device code: the fused step's front launch (step_kernels.h step_front_body) with the number of
// stored rows read from device memory.  A translation unit of its own, so a code object of its own: the learner's
// (learner.hip) holds what it held before these two kernels came, every kernel where it was.  The headers are included for
// their device functions alone -- their non-template kernels are learner.hip's.
#define PRISM_STEP_NO_KERNELS
#include "step_kernels.h"

namespace prism {

// ---- the cursor form (prism_step_front_cursor): the number of stored rows is read from device memory, so a captured
// launch samples from the ring as it has grown by the time of each replay.  The word is cursor[slot] of the ingest's
// ping-pong pair (ingest_kernels.h): the write serial behind the last ingest launch, which is the ring's size until the
// ring wraps and at least the capacity ever after -> size = min(word, capacity).  The launch only READS the pair, so
// every workgroup sees the same size whenever it is scheduled.
struct FrontCursor {
    const int64_t *cursor;                          // device, [2]
    int32_t slot;                                   // 0 | 1: the word this launch reads
};

// Only the sampling wave uses the size, so only that wave asks for the word, and before anything else: a vector load on
// its own counter, which leaves the conv-weight staging of waves 1-3 (and the helper workgroups, which never look) where
// they were.  A word the host never saw cannot be trusted: the size is clamped into [1, capacity] and a word <= 0 raises
// the sticky bit -- no early return, the launch does everything the by-value one does.  The size goes to the body in a
// copy of the argument struct made of scalars (never indexed, never addressed past inlining: it stays in registers).
template <int RING>
__device__ __forceinline__ void step_front_cursor_body(const IqnArgs &a, const prism_replay_desc &rp, const FrontArgs &f,
                                                       const FrontCursor &c, const int tid, const int b) {
    int64_t size = 1;
    if (b < a.B && tid < 64) {
        const int64_t word = __atomic_load_n(c.cursor + c.slot, __ATOMIC_RELAXED);
        size = word < rp.capacity ? word : rp.capacity;
        if (size < 1) {
            size = 1;
            if (b == 0 && tid == 0) atomicOr(rp.status, PRISM_STATUS_FRONT_BAD_SIZE);
        }
    }
    FrontArgs g = f;
    g.size = size;
    step_front_body<RING>(a, rp, g, tid, b);
}

// (IqnArgs and prism_replay_desc first, in this order: the body reads `gammas` from the argument segment by offset)
static __global__ __launch_bounds__(256) void step_front_cursor_kernel(IqnArgs a, prism_replay_desc rp, FrontArgs f,
                                                                       FrontCursor c) {
    step_front_cursor_body<PRISM_RING_F32>(a, rp, f, c, threadIdx.x, blockIdx.x);
}

static __global__ __launch_bounds__(256) void step_front_byte_ring_cursor_kernel(IqnArgs a, prism_replay_desc rp, FrontArgs f,
                                                                                 FrontCursor c) {
    step_front_cursor_body<PRISM_RING_U8>(a, rp, f, c, threadIdx.x, blockIdx.x);
}

// the launch alone: learner.hip's step_front has checked and filled everything, and looks at the launch's error itself
void launch_front_cursor(int32_t ring_kind, unsigned blocks, hipStream_t stream, const IqnArgs &a, const prism_replay_desc &rp,
                         const FrontArgs &f, const int64_t *cursor, int32_t slot) {
    const FrontCursor c{cursor, slot};
    if (ring_kind == PRISM_RING_U8)
        hipLaunchKernelGGL(step_front_byte_ring_cursor_kernel, dim3(blocks), dim3(256), 0, stream, a, rp, f, c);
    else
        hipLaunchKernelGGL(step_front_cursor_kernel, dim3(blocks), dim3(256), 0, stream, a, rp, f, c);
}

}  // namespace prism
