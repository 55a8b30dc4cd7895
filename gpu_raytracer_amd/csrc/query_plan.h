// query_plan.h — the arithmetic of a batch call (rt_query.cpp, run_batch): which records each device takes, how a device's range is
// cut into chunks, and how many event pairs time them.  Pure functions of sizes: nothing of HIP, so tests/check_query_plan.cpp holds
// them to their statement on the host.
#ifndef RT_QUERY_PLAN_H
#define RT_QUERY_PLAN_H

#include <cstddef>

namespace rti __attribute__((visibility("hidden"))) {

struct PlanRange {
    size_t first, count; // records [first, first + count) of the caller's arrays
};
struct PlanChunk {
    size_t off, m; // records [off, off + m) of the caller's arrays
};

// Device j's share of a host batch of n records on nd devices: contiguous ranges in device order that cover [0, n); count may be 0.
inline PlanRange device_range(size_t n, size_t nd, size_t j) {
    const size_t first = n * j / nd;
    return {first, n * (j + 1) / nd - first};
}

// The chunks of `count` records at `chunk` (>= 1) records each: all full but the last.
inline size_t chunk_count(size_t count, size_t chunk) { return (count + chunk - 1) / chunk; }

// Chunk c (< chunk_count(r.count, chunk)) of range r: 1 <= m <= chunk.
inline PlanChunk chunk_of(PlanRange r, size_t chunk, size_t c) {
    const size_t off = r.first + c * chunk, left = r.first + r.count - off;
    return {off, left < chunk ? left : chunk};
}

// The event pairs around the launches of `count` records: one per chunk, or with one_pair a single pair around all of them.
inline size_t event_pairs(size_t count, size_t chunk, bool one_pair) { return one_pair && count > 0 ? 1 : chunk_count(count, chunk); }

} // namespace rti
#endif
