// check_query_plan.cpp — csrc/query_plan.h, the range and chunk arithmetic of the batch calls (rt_query.cpp, run_batch), held to its
// statement on the host: for every device count, chunk size and batch size below, the devices' ranges are contiguous and cover [0, n)
// exactly; the chunks of a range cover it exactly once, in order, each of 1 .. chunk records (so a chunk's count fits the kernels'
// uint32_t); and the chunks are as many as the event pairs the runner asks for.  Built with -fsanitize=address,undefined by
// tests/test_query_plan.py.  Prints "<cases> cases, <failures> failures"; the exit status is 1 with any failure.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "query_plan.h"
#include "rt_hip.h"

using namespace rti;

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

// The chunks of `r` at `chunk` records each, as run_batch walks them.
static void check_chunks(PlanRange r, size_t chunk) {
    const size_t chunks = chunk_count(r.count, chunk);
    size_t next = r.first;
    for (size_t c = 0; c < chunks; c++) {
        const PlanChunk pc = chunk_of(r, chunk, c);
        EXPECT(pc.off == next, "first %zu count %zu chunk %zu: chunk %zu starts at %zu, not %zu", r.first, r.count, chunk, c, pc.off, next);
        EXPECT(pc.m >= 1 && pc.m <= chunk && pc.m <= UINT32_MAX, "first %zu count %zu chunk %zu: chunk %zu has %zu records", r.first, r.count, chunk, c, pc.m);
        EXPECT(c + 1 == chunks || pc.m == chunk, "first %zu count %zu chunk %zu: chunk %zu is short and not the last", r.first, r.count, chunk, c);
        next = pc.off + pc.m;
    }
    EXPECT(next == r.first + r.count, "first %zu count %zu chunk %zu: the chunks end at %zu", r.first, r.count, chunk, next);
    EXPECT(event_pairs(r.count, chunk, false) == chunks, "count %zu chunk %zu: %zu pairs for %zu chunks", r.count, chunk, event_pairs(r.count, chunk, false), chunks);
    EXPECT(event_pairs(r.count, chunk, true) == (r.count ? 1u : 0u), "count %zu chunk %zu: %zu pairs around all chunks", r.count, chunk, event_pairs(r.count, chunk, true));
}

static void check(size_t n, size_t nd, size_t chunk) {
    g_cases++;
    size_t next = 0; // a host batch: one range per device
    for (size_t j = 0; j < nd; j++) {
        const PlanRange r = device_range(n, nd, j);
        EXPECT(r.first == next, "n %zu nd %zu: device %zu starts at %zu, not %zu", n, nd, j, r.first, next);
        EXPECT(r.count <= n / nd + 1 && r.count + 1 >= n / nd, "n %zu nd %zu: device %zu takes %zu", n, nd, j, r.count);
        check_chunks(r, chunk);
        next = r.first + r.count;
    }
    EXPECT(next == n, "n %zu nd %zu: the ranges end at %zu", n, nd, next);
    check_chunks(PlanRange{0, n}, chunk); // a device batch: whole on its device
}

int main() {
    const size_t chunks[] = {1, 1024, RT_QUERY_CHUNK / 4096, RT_QUERY_CHUNK, (size_t)1 << 24};
    for (size_t nd = 1; nd <= 8; nd++)
        for (size_t chunk : chunks) {
            for (size_t n : {(size_t)0, (size_t)1, nd - 1, nd, chunk - 1, chunk, chunk + 1, 2 * chunk + 5}) check(n, nd, chunk);
            if (chunk == (size_t)1 << 24) check((size_t)1 << 40, nd, chunk);
        }
    std::printf("%lld cases, %lld failures\n", g_cases, g_failures);
    return g_failures ? 1 : 0;
}
