"""Host-only check of the bound on compacted path ids (wf_state_slots, gpu_raytracer_amd/csrc/wavefront.hip).

From depth 1 on a path's id is its position in the extension queue k_wf_finish writes, window padding included, so the arrays indexed
by id must hold every position such a launch can reach.  This simulates the reservation protocol (the library's own window rule,
rt_debug_pick_window) through generate -> finish -> finish ... chains with adversarial request patterns and asserts that no position
reaches rt_debug_state_slots.  No GPU, no kernels."""
import ctypes as C
import random

import pytest


@pytest.fixture(scope="module")
def lib(rt_api):
    l = rt_api.load()
    l.rt_debug_state_slots.restype = C.c_ulonglong
    l.rt_debug_state_slots.argtypes = [C.c_ulonglong, C.c_ulonglong]
    l.rt_debug_queue_slots.restype = C.c_ulonglong
    l.rt_debug_queue_slots.argtypes = [C.c_ulonglong, C.c_uint32, C.c_ulonglong]
    l.rt_debug_pick_window.restype = C.c_uint32
    l.rt_debug_pick_window.argtypes = [C.c_uint32, C.c_uint32]
    return l


def _launch(lib, consumed_len, waves, budget, pattern, rnd):
    """One producing launch (per_lane 1) over a consumed queue of consumed_len positions; at most `budget` entries continue.
    Returns (queue length incl. padding, real entries)."""
    stride = waves * 64
    iters = (consumed_len + stride - 1) // stride
    window = lib.rt_debug_pick_window(iters, 1)
    counter = real = 0
    for w in range(waves):
        nxt = end = 0
        for it in range(iters):
            if it * stride + w * 64 >= consumed_len:
                break
            total = min(64, budget - real) if pattern == "full" else min(rnd.choice((0, 1, 63, 64)), budget - real)
            if total <= 0:
                continue
            if nxt + total > end:
                nxt, end = counter, counter + window
                counter += window
            nxt += total
            real += total
        # the wave's last window stays reserved, padded with sentinels
    return counter, real


@pytest.mark.parametrize("paths,waves", [(64, 16384), (3840, 16384), (1 << 20, 1024), (1 << 22, 64), (5 << 16, 4096)])
@pytest.mark.parametrize("pattern", ["full", "ragged"])
def test_positions_stay_below_the_bound(lib, paths, waves, pattern):
    rnd = random.Random(paths ^ waves)
    bound = lib.rt_debug_state_slots(paths, waves)
    assert paths <= bound <= lib.rt_debug_queue_slots(paths, 1, waves)
    length, _ = _launch(lib, paths, waves, paths, pattern, rnd)  # k_wf_generate: entries are path slots, not ids
    for depth in range(8):
        length, real = _launch(lib, length, waves, paths, pattern, rnd)
        assert length <= bound, (depth, length, bound)
        if real == 0:
            break


def test_headline_batch_fits_27_bit_ids(lib):
    """A 1080p frame at 32 samples per batch (the two-lane headline batch) on 256 CUs x 16 blocks x 4 waves: its ids fit the 27 bits
    they share with a light index."""
    paths = 240 * 135 * 64 * 32
    assert lib.rt_debug_state_slots(paths, 256 * 16 * 4) <= 1 << 27
