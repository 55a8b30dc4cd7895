"""The queue pipeline past its every-8th-bounce poll (rt_frame.cpp: wf_step_bounce reads back the live paths after bounce iterations
7, 15, 23, ...; a batch that reads 0 goes to its resolve at whatever bounce parity it has reached, any other goes on).

The frames are those of long_path_cases.py; test_long_paths_oracle.py says, from the CPU statement alone, which of them stop early at
a poll, which go on once, twice, three times and more, and that with one sample per batch both happen within one frame.  Here every
frame is held bit for bit to that statement and to the two megakernels (which keep a path in registers and poll nothing), every way of
splitting the work - batches, lanes, a device listed twice, flags, accumulating calls, tile shares - to the same bits and segment
totals, frames that follow one another in one context to the frames fresh contexts give, and an adaptive sequence at 17 bounces to the
closed frames of its pixels' own counts."""
import numpy as np
import pytest

import long_path_cases as lp
from test_gpu_adaptive import MIN, SEQ, _check_identity, _owned, _threshold, np_active
from test_gpu_path_compaction import MEGAKERNELS

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = lp.W, lp.HT, lp.SPP, lp.FRAME_SEED
FRAMES = [(name, b) for name in lp.SCENES for b in lp.BOUNCES[name]]
SPLIT_FRAMES = [(name, b) for name in lp.SCENES for b in lp.SPLIT_BOUNCES[name]]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _segments(st):
    return st["primary_rays"], st["continuation_rays"], st["shadow_rays"]


def _want(oracle_mod, name, bounces):
    ref = lp.statement(oracle_mod, name, bounces)
    seg = ref["segments"]
    return ref["rgb"], (seg["camera"], seg["continuation"], seg["shadow"])


def _render(rt_api, name, bounces, devices=(0,), **kw):
    """One closed frame in a fresh context (the batch size and the lanes are chosen per allocation): image and segment totals."""
    sc = lp.scene(name)
    with rt_api.Context(devices) as ctx:
        ctx.upload_scene(sc)
        st = ctx.render(W, H, sc.camera, mode=2, spp=SPP, max_bounces=bounces, frame_seed=SEED, **kw)
        return ctx.read_rgb32f(), _segments(st)


def _assert_frame(got, want, label):
    assert got[1] == want[1], f"{label}: segments (camera, continuation, shadow) {got[1]}, the statement has {want[1]}"
    np.testing.assert_array_equal(_u32(got[0]), _u32(want[0]), err_msg=label)


# 1 + 2 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bounces", FRAMES, ids=[f"{n}-{b}b" for n, b in FRAMES])
def test_frames_past_the_poll_equal_the_statement_and_the_megakernels(rt_api, oracle_mod, monkeypatch, name, bounces):
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    want = _want(oracle_mod, name, bounces)
    print(f"{name} at {bounces} bounces: the statement's poll outcome (went on, stopped early) {lp.MEASURED_POLLS[name][bounces]}")
    _assert_frame(_render(rt_api, name, bounces), want, "pipeline")
    for kernel, kw in MEGAKERNELS.items():
        _assert_frame(_render(rt_api, name, bounces, **kw), want, kernel)


# 3 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", ["1", "2"])
@pytest.mark.parametrize("batch", ["1", "3"])
@pytest.mark.parametrize("name,bounces", SPLIT_FRAMES, ids=[f"{n}-{b}b" for n, b in SPLIT_FRAMES])
def test_batches_and_lanes(rt_api, oracle_mod, monkeypatch, name, bounces, batch, lanes):
    """6 batches of one sample or 2 of three, on one lane or alternating between two: every batch starts on the first state set and
    the first queue again whatever parity the one before it on its lane ended on, and a poll reads the counters of the lane that ran
    the batch.  closed_bright at 255 bounces with one sample per batch has polls at which one sample index stops while another goes
    on (long_path_cases.MEASURED_MIXED)."""
    monkeypatch.setenv("RT_WF_LANES", lanes)
    monkeypatch.setenv("RT_WF_BATCH", batch)
    _assert_frame(_render(rt_api, name, bounces), _want(oracle_mod, name, bounces), f"RT_WF_BATCH={batch} RT_WF_LANES={lanes}")


@pytest.mark.parametrize("name,bounces", SPLIT_FRAMES, ids=[f"{n}-{b}b" for n, b in SPLIT_FRAMES])
def test_every_split_of_the_work_gives_the_same_bits_and_totals(rt_api, oracle_mod, monkeypatch, name, bounces):
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    want = _want(oracle_mod, name, bounces)
    # one device listed twice: 3 x 2 tiles of 16 x 16, every second tile on the context's second share of the same device
    _assert_frame(_render(rt_api, name, bounces, devices=(0, 0), tile_size=16), want, "one device listed twice")
    for flag in ("no_shadow_grid", "no_beams", "counters"):
        _assert_frame(_render(rt_api, name, bounces, **{flag: True}), want, flag)
    sc = lp.scene(name)
    # accumulating calls of 2 + 3 + 1 samples against the closed 6-spp frame
    with rt_api.Context() as ctx:
        ctx.upload_scene(sc)
        total = np.zeros(3, np.int64)
        for n in (2, 3, 1):
            total += _segments(ctx.render(W, H, sc.camera, mode=2, spp=n, max_bounces=bounces, frame_seed=SEED, accumulate=True))
        assert ctx.accumulated_samples() == SPP == 2 + 3 + 1
        _assert_frame((ctx.read_rgb32f(), tuple(total.tolist())), want, "accumulating calls 2 + 3 + 1")
    # tile shares: 3 x 2 tiles of 16 x 16 (the last column and row ragged), every second tile per rank, united
    tile, world = 16, 2
    rgb, total = np.zeros((H, W, 3), np.float32), np.zeros(3, np.int64)
    for rank in range(world):
        share, seg = _render(rt_api, name, bounces, tile_size=tile, tile_world=world, tile_rank=rank)
        m = _owned(W, H, tile, world, rank)
        assert m.any()
        rgb[m] = share[m]
        total += seg
    _assert_frame((rgb, tuple(total.tolist())), want, "tile shares of 2 united")


# 4 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [None, "1"])
def test_frames_that_follow_one_another_in_one_context(rt_api, oracle_mod, monkeypatch, batch):
    """255 bounces (every batch ends at a poll), then 17, 8 and 255 again in one context: no parity, queue or counter state of a batch
    that ended at a poll reaches the next frame."""
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    if batch is None:
        monkeypatch.delenv("RT_WF_BATCH", raising=False)
    else:
        monkeypatch.setenv("RT_WF_BATCH", batch)
    name = "closed_bright"
    sc = lp.scene(name)
    fresh = {b: _render(rt_api, name, b) for b in (255, 17, 8)}
    with rt_api.Context() as ctx:
        ctx.upload_scene(sc)
        for i, b in enumerate((255, 17, 8, 255)):
            st = ctx.render(W, H, sc.camera, mode=2, spp=SPP, max_bounces=b, frame_seed=SEED)
            got = (ctx.read_rgb32f(), _segments(st))
            _assert_frame(got, fresh[b], f"frame {i} ({b} bounces) against a fresh context")
            _assert_frame(got, _want(oracle_mod, name, b), f"frame {i} ({b} bounces) against the statement")


# 5 ------------------------------------------------------------------------------------------------------------------------------
def test_adaptive_sequence_at_17_bounces(rt_api, monkeypatch):
    """The standard adaptive call sequence on closed_bright at 17 bounces (past the second poll; the live blocks shrink from call to
    call): the rule's active set per call, and every pixel holds the bits of the closed frame of its own count."""
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    sc, bounces = lp.scene("closed_bright"), 17
    kw = dict(w=W, h=H, frame_seed=SEED)
    t = _threshold(rt_api, sc, bounces=bounces, **kw)
    with rt_api.Context() as ctx:
        ctx.upload_scene(sc)
        prev = None
        for i, n in enumerate(SEQ):
            st = ctx.render_adaptive(W, H, sc.camera, n, t, min_samples=MIN, max_bounces=bounces, restart=i == 0, frame_seed=SEED)
            rec = ctx.read_adaptive()
            grew = rec[..., 3] > (prev[..., 3] if prev is not None else 0)
            if prev is not None:
                np.testing.assert_array_equal(grew, np_active(prev, t, MIN), err_msg=f"call {i}: active set")
            assert st["primary_rays"] == int(grew.sum()) * n and st["pixels"] == int(grew.sum())
            prev = rec
        images = (ctx.read_rgb32f(), ctx.read_rgba8_combined())
    counts = _check_identity(rt_api, sc, rec, images, bounces=bounces, **kw)  # (asserts at least three distinct counts)
    assert counts.min() == MIN  # some pixels stopped as early as allowed
