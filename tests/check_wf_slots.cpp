// check_wf_slots.cpp — csrc/wf_slots.h, the path-slot arithmetic of the wavefront pipeline, held to its statement on the host: for every
// n_samples in 1 .. 130 and the block counts below, slot -> (b, j, k) -> slot is the identity, (b, j, k) stays in range, every slot below
// n_blocks * 64 * n_samples is hit exactly once by the triples, a wave-group (64 consecutive slots) lies in one block and wf_slot_at /
// wf_group_of / wf_group_split agree with wf_slot_split; wf_div, the division by reciprocal they all use, gives the machine's quotient
// and remainder up to the ends of the 32-bit range.  Compiled once per order (-DRT_WF_BLOCK_MAJOR=0, 1, 2) with
// -fsanitize=address,undefined by tests/test_gpu_pixel_major_slots.py.  Prints "<cases> cases, <failures> failures"; the exit status is
// 1 with any failure.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wf_slots.h"

using namespace rt;

static long long g_cases = 0, g_failures = 0;

#define EXPECT(cond, ...)                        \
    do {                                         \
        if (!(cond)) {                           \
            if (g_failures++ < 20) {             \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);        \
                std::printf("\n");               \
            }                                    \
        }                                        \
    } while (0)

// wf_div: the quotient and remainder of the reciprocal multiplication against the machine's, at the ends of the 32-bit range and around
// every multiple of n near them
static void check_div(uint32_t nn) {
    const WfSamples n = wf_samples(nn);
    EXPECT(n.n == nn, "wf_samples(%u).n = %u", nn, n.n);
    const uint32_t xs[] = {0u, 1u, nn - 1u, nn, nn + 1u, 64u * nn - 1u, 64u * nn, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu - nn, 0xFFFFFFFEu, 0xFFFFFFFFu};
    for (uint32_t x0 : xs)
        for (uint32_t d = 0; d < 3u; d++) {
            const uint32_t x = x0 - x0 % nn + (d == 0 ? 0u : d == 1 ? nn - 1u : nn / 2u); // a multiple of n, one below the next, in between
            for (uint32_t y : {x0, x}) {
                uint32_t r = 0;
                const uint32_t q = wf_div(y, n, r);
                EXPECT(q == y / nn && r == y % nn, "%u / %u = %u rem %u, not %u rem %u", y, nn, q, r, y / nn, y % nn);
            }
        }
}

static void check(uint32_t nn, uint32_t nb) {
    g_cases++;
    const WfSamples n = wf_samples(nn);
    const uint32_t slots = nb * 64u * nn;
    std::vector<uint8_t> hit(slots, 0);
    // slot -> triple -> slot
    for (uint32_t p = 0; p < slots; p++) {
        const WfSlot s = wf_slot_split(p, n, nb);
        EXPECT(s.b < nb && s.j < 64u && s.k < nn, "n %u nb %u: slot %u -> (%u, %u, %u)", nn, nb, p, s.b, s.j, s.k);
        EXPECT(wf_slot_of(s.b, s.j, s.k, n, nb) == p, "n %u nb %u: slot %u -> (%u, %u, %u) -> %u", nn, nb, p, s.b, s.j, s.k, wf_slot_of(s.b, s.j, s.k, n, nb));
        const WfSlot a = wf_slot_at(p / 64u, p % 64u, n, nb);
        EXPECT(a.b == s.b && a.j == s.j && a.k == s.k, "n %u nb %u: slot %u, wf_slot_at (%u, %u, %u) != (%u, %u, %u)", nn, nb, p, a.b, a.j, a.k, s.b, s.j, s.k);
        // the slot's wave-group belongs to the slot's block
        uint32_t gb, g;
        wf_group_split(p / 64u, n, nb, gb, g);
        EXPECT(gb == s.b && g < nn && wf_group_of(gb, g, n, nb) == p / 64u, "n %u nb %u: slot %u in group %u -> block %u group %u, slot's block %u", nn, nb, p, p / 64u, gb, g, s.b);
    }
    // triple -> slot: every slot exactly once
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t j = 0; j < 64u; j++)
            for (uint32_t k = 0; k < nn; k++) {
                const uint32_t p = wf_slot_of(b, j, k, n, nb);
                EXPECT(p < slots, "n %u nb %u: (%u, %u, %u) -> %u", nn, nb, b, j, k, p);
                if (p < slots) hit[p]++;
            }
    uint32_t wrong = 0;
    for (uint32_t p = 0; p < slots; p++) wrong += hit[p] != 1;
    EXPECT(wrong == 0, "n %u nb %u: %u slots not hit exactly once", nn, nb, wrong);
#if RT_WF_BLOCK_MAJOR == 2
    // pixel-major: a pixel's samples are consecutive slots, in sample order, and a block's pixels follow each other
    for (uint32_t b = 0; b < nb; b++)
        for (uint32_t j = 0; j < 64u; j++)
            EXPECT(wf_slot_of(b, j, 0, n, nb) == (b * 64u + j) * nn && wf_slot_of(b, j, nn - 1u, n, nb) == (b * 64u + j) * nn + nn - 1u, "n %u nb %u: pixel (%u, %u)", nn, nb, b, j);
#endif
}

int main() {
    for (uint32_t n = 1; n <= 130; n++) {
        check_div(n);
        for (uint32_t nb : {1u, 2u, 3u, 7u, 24u, 61u}) check(n, nb);
    }
    for (uint32_t n : {255u, 256u, 257u, 4096u, 65535u, 65536u, 65537u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu}) check_div(n);
    std::printf("%lld cases, %lld failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
