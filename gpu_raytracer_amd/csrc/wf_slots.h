// wf_slots.h — the path slots of a wavefront batch (wavefront.hip), stated once.  Pure integer arithmetic, nothing of HIP, so
// tests/check_wf_slots.cpp holds it to its statement on the host.
//
// A batch of n_samples samples over n_blocks 8x8 pixel blocks has P = n_blocks * 64 * n_samples path slots.  A slot is a triple
//   b  pixel block,  j  pixel lane inside it (0 .. 63, block_pixel_at's lane),  k  sample of the batch (0 .. n_samples - 1)
// and a WAVE-GROUP is 64 consecutive slots [64 sb, 64 sb + 64): the lanes of one wave of every depth-0 stage, and (each wave reserves its
// queue entries in one piece) 64 neighbours of the depth-0 queue.  A block owns n_samples whole wave-groups in every order, so a wave-group
// never spans two blocks.  RT_WF_BLOCK_MAJOR picks what else the lanes of a wave-group share:
//   2  pixel-major   p = (b * 64 + j) * n_samples + k   a block's 64 n_samples slots are consecutive, index i = j * n_samples + k inside it: a
//                                                       wave-group is 64 / n_samples pixels x all their samples (n_samples need not divide 64:
//                                                       a pixel's samples may end inside a wave-group; above 64 they span several)
//   1  block-major   p = (b * n_samples + k) * 64 + j   a wave-group is the block's 64 pixels for one sample; a block's groups are neighbours
//   0  sample-major  p = (k * n_blocks + b) * 64 + j    the same wave-groups, all blocks of a sample adjacent
// Measurements: DESIGN.md section 4 and profiles/ab_r08.json.
#ifndef RT_WF_SLOTS_H
#define RT_WF_SLOTS_H

#include <cstdint>

#ifndef RT_WF_BLOCK_MAJOR
#define RT_WF_BLOCK_MAJOR 2
#endif
#if RT_WF_BLOCK_MAJOR < 0 || RT_WF_BLOCK_MAJOR > 2
#error "RT_WF_BLOCK_MAJOR is 0 (sample-major), 1 (block-major) or 2 (pixel-major)"
#endif

#if defined(__HIPCC__)
#define RT_WF_SLOT_FN __host__ __device__ inline
#else
#define RT_WF_SLOT_FN inline
#endif

namespace rt {

// The batch's sample count with the reciprocal its divisions use.  The host makes it (wf_samples) and the kernels take it as an argument:
// pixel-major, a lane divides by n_samples to find its pixel and sample, and a division by a number the compiler does not know is 25
// instructions and a register held across the loop, against a multiplication, a product and one correction here.
struct WfSamples {
    uint32_t n;   // samples per pixel in the batch, >= 1
    uint32_t inv; // min(floor(2^32 / n), 2^32 - 1)
};
RT_WF_SLOT_FN WfSamples wf_samples(uint32_t n_samples) {
    WfSamples s;
    s.n = n_samples > 0u ? n_samples : 1u;
    s.inv = s.n > 1u ? (uint32_t)(0x100000000ull / s.n) : 0xFFFFFFFFu;
    return s;
}
// x / n and the remainder, exact for every 32-bit x: x inv / 2^32 lies in (x / n - 1, x / n], so its floor is the quotient or one below
RT_WF_SLOT_FN uint32_t wf_div(uint32_t x, WfSamples s, uint32_t& rem) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t q = __umulhi(x, s.inv);
#else
    uint32_t q = (uint32_t)(((uint64_t)x * s.inv) >> 32);
#endif
    uint32_t r = x - q * s.n;
    const bool low = r >= s.n;
    q = low ? q + 1u : q;
    rem = low ? r - s.n : r;
    return q;
}

struct WfSlot {
    uint32_t b, j, k; // pixel block, pixel lane in the block, sample of the batch
};

// wave-group g (0 .. n_samples - 1) of block b -> its index sb among the batch's n_blocks * n_samples wave-groups, and back
RT_WF_SLOT_FN uint32_t wf_group_of(uint32_t b, uint32_t g, WfSamples s, uint32_t n_blocks) { return RT_WF_BLOCK_MAJOR ? b * s.n + g : g * n_blocks + b; }
RT_WF_SLOT_FN void wf_group_split(uint32_t sb, WfSamples s, uint32_t n_blocks, uint32_t& b, uint32_t& g) {
#if RT_WF_BLOCK_MAJOR
    (void)n_blocks;
    b = wf_div(sb, s, g);
#else
    g = sb / n_blocks, b = sb - g * n_blocks;
#endif
}

// (b, j, k) -> slot
RT_WF_SLOT_FN uint32_t wf_slot_of(uint32_t b, uint32_t j, uint32_t k, WfSamples s, uint32_t n_blocks) {
#if RT_WF_BLOCK_MAJOR == 2
    (void)n_blocks;
    return (b * 64u + j) * s.n + k;
#else
    return wf_group_of(b, k, s, n_blocks) * 64u + j;
#endif
}
// slot -> (b, j, k)
RT_WF_SLOT_FN WfSlot wf_slot_split(uint32_t p, WfSamples s, uint32_t n_blocks) {
    WfSlot t;
#if RT_WF_BLOCK_MAJOR == 2
    (void)n_blocks;
    const uint32_t pixel = wf_div(p, s, t.k); // b * 64 + j: the one division per lane
    t.b = pixel / 64u, t.j = pixel & 63u;
#else
    wf_group_split(p / 64u, s, n_blocks, t.b, t.k);
    t.j = p & 63u;
#endif
    return t;
}
// lane `lane` (0 .. 63) of wave-group sb, i.e. slot sb * 64 + lane -> (b, j, k); b is the same for the 64 lanes
RT_WF_SLOT_FN WfSlot wf_slot_at(uint32_t sb, uint32_t lane, WfSamples s, uint32_t n_blocks) { return wf_slot_split(sb * 64u + lane, s, n_blocks); }

} // namespace rt
#endif
