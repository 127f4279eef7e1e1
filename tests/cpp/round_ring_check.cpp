// round_ring_check.cpp -- the index arithmetic of the flag ring (csrc/round_ring.h) on the host, no HIP: for batch sizes 1, 4 and 8 and the
// rounds of five batches, where a round's flag lives, which flag a round reads first, and that the half of the ring that is zeroed before a
// batch is enqueued never holds the flag that the batch's first round reads.  Prints "ok" and returns 0, or says what failed.
#include <cstdio>
#include <initializer_list>

#include "round_ring.h"

int main()
{
    int failures = 0;
    auto fail = [&](const char* what, unsigned batch, unsigned r) {
        std::printf("batch %u round %u: %s\n", batch, r, what);
        ++failures;
    };
    for (uint32_t batch : {1u, 4u, 8u}) {
        uint32_t words[16] = {};
        const vp::RoundRing ring{words, batch, nullptr};
        if (ring.prev(0) != nullptr) fail("the first round of a run reads a flag", batch, 0);
        for (uint32_t r = 0; r <= 5u * batch; ++r) {
            const uint32_t* s = ring.slot(r);
            if (s < words || s >= words + 2u * batch) fail("the slot lies outside the ring", batch, r);
            if (r > 0 && ring.prev(r) != ring.slot(r - 1u)) fail("the round does not read the previous round's flag", batch, r);
            if (r > 0 && ring.slot(r) == ring.slot(r - 1u)) fail("two consecutive rounds share a flag", batch, r);
        }
        for (uint32_t r0 = 0; r0 < 5u * batch; r0 += batch) {        // a batch: rounds r0 .. r0 + batch - 1, zeroed from slot(r0) on
            if (ring.slot(r0) != words && ring.slot(r0) != words + batch) fail("the batch does not start a half of the ring", batch, r0);
            for (uint32_t r = r0; r < r0 + batch; ++r) {
                if (ring.slot(r) != ring.slot(r0) + (r - r0)) fail("the flags of a batch are not the consecutive words that are zeroed", batch, r);
                if (ring.slot(r) == ring.prev(r0)) fail("zeroing the batch wipes the flag its first round reads", batch, r);
            }
        }
    }
    if (failures == 0) std::printf("ok\n");
    return failures ? 1 : 0;
}
