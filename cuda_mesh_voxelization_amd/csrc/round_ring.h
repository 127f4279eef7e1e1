// round_ring.h -- the NAIVE fixed-point driver of fill.hip, geodesic.hip and watershed.hip: whole-grid rounds repeat until one changes nothing,
// without a host synchronisation per round.
// Round r has its own flag word in a ring of 2 * batch words.  A kernel of round r that changes something stores 1 into the round's flag (a
// plain store: the value is idempotent and the kernel boundary makes it visible); every kernel of round r + 1 reads flag r first and returns
// at once if it is 0.  The host enqueues `batch` rounds, reads their flags back once, and stops at the first round that changed nothing.  The
// last flag of a batch lives in the other half of the ring, so the next batch's first round can still read it.  No persistent kernel, grid
// barrier or hand-off between workgroups: kernel boundaries are the only synchronisation.
// Who zeroes what: the driver zeroes a half of the ring right before that half's batch is enqueued, the first batch of a run included, and
// nobody else touches the ring.  That one rule is correct for every user: a run may start on a ring that an earlier run (the previous call,
// the previous level of a watershed) left full of ones; the first round of a run reads no flag, so the other half can wait until the second
// batch zeroes it; and the half that is zeroed never holds the flag that the batch's first round reads (tests/cpp/round_ring_check.cpp).
#pragma once

#include <cstdint>
#ifdef __HIPCC__
#include "vp_internal.h"
#endif

namespace vp {

// 2 * batch device words and the pinned host words (batch, or batch + 1 with an extra word) a batch comes back through.  Rounds count from 0
// at the start of a run.  Pure index arithmetic, no HIP call.
struct RoundRing {
    uint32_t* dev;
    uint32_t batch;
    volatile uint32_t* host;
    uint32_t* slot(uint32_t r) const { return dev + r % (2u * batch); }                  // where round r's flag lives
    const uint32_t* prev(uint32_t r) const { return r ? slot(r - 1u) : nullptr; }        // what round r reads first: nothing in round 0
};

#ifdef __HIPCC__

namespace {

// true when the previous round changed nothing: the kernel returns at once
__device__ __forceinline__ bool round_skip(const uint32_t* prev) { return prev && *prev == 0u; }

// the round's flag: one plain store per wave that changed something
__device__ __forceinline__ void round_mark(bool changed, uint32_t* cur) { if (__any(changed) && (threadIdx.x & 63) == 0) *cur = 1u; }

// Runs rounds until one changes nothing; *rounds = their number, that last round included.  enqueue(r, prev, cur) launches the kernels of
// round r (under the caller's own ProfScopes).  Per batch: one memset, the launches, one read-back, one synchronisation; d_extra, if given, is
// one more device word that comes back with the flags, in ring.host[ring.batch].
template <typename Enqueue>
int run_rounds(hipStream_t st, const RoundRing& ring, uint32_t* rounds, const uint32_t* d_extra, Enqueue enqueue)
{
    for (uint32_t r0 = 0;; r0 += ring.batch) {
        VP_HIP(hipMemsetAsync(ring.slot(r0), 0, ring.batch * sizeof(uint32_t), st));
        for (uint32_t r = r0; r < r0 + ring.batch; ++r) enqueue(r, ring.prev(r), ring.slot(r));
        VP_HIP(hipGetLastError());
        VP_HIP(hipMemcpyAsync((void*)ring.host, ring.slot(r0), ring.batch * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (d_extra) VP_HIP(hipMemcpyAsync((void*)(ring.host + ring.batch), d_extra, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VP_HIP(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < ring.batch; ++i)
            if (!ring.host[i]) {
                if (rounds) *rounds = r0 + i + 1u;
                return 0;
            }
    }
}

}  // namespace

#endif  // __HIPCC__

}  // namespace vp
