"""The camera beams' one property - a block's list is a superset of the triangles Moeller-Trumbore can accept for any sample of the
block, in an order whose early-out loses nothing (csrc/wavefront.hip, "Camera beams") - tested where it can break, on the cases of
beam_edge_cases.py: lists at 127, 128 and 129 entries, blocks without a list at the first, the last, alternate and all places of the
walk queue with sample counts on both sides of the 8-sample chunk, lists whose order by box distance is not the order of the hits,
slivers within a fraction of a pixel of block, tile and image borders, and pyramids from 0.003 to 170 degrees.

Per case, with kernel_pipeline=True: the frame with beams carries the bits of the frame with no_beams=True (whole byte strings, equal
segment counts) and the bits of the brute-force oracle; debug_beams reports exactly the list lengths the case states (cap, fallback),
a list for every block (order), or is printed (pyramids).  Two cases run once more through every caller of the lists: batches, lanes,
rt_render_adaptive, progressive accumulation and two devices.  test_beam_edge_cases.py checks the cases themselves on the CPU.

Found with these cases: before k_wf_beams rejected pyramids whose widening drowns in the rounding of a corner direction, the frames at
0.3, 0.1 and 0.02 degrees lost 2, 13 and 17 pixels' hits on the fringe triangles against the tree walk."""
import numpy as np
import pytest

import beam_edge_cases as ec

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
KEYS = ("primary_rays", "continuation_rays", "shadow_rays")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same_bits(case, got, want, what):
    diff = np.argwhere((_bits(got) != _bits(want)).reshape(got.shape[0], got.shape[1], -1).any(-1))
    if len(diff):
        y, x = (int(v) for v in diff[0])
        b = ec.block_of_pixel(case, x, y)
        raise AssertionError(f"{case.name}: {len(diff)} pixels differ between beams and {what}, first at (x, y) = ({x}, {y}) in block {b} "
                             f"at {tuple(ec.case_blocks(case)[b][:2]) if b >= 0 else None}: {got[y, x]} != {want[y, x]}")
    assert got.tobytes() == want.tobytes()


def _lists(ctx):
    return ctx.debug_beams(1 << 20)


def _both(ctx, case, spp=None):
    """The frame with beams and with no_beams -> (image, stats, debug_beams after the frame with beams)."""
    kw = case.render_kw(spp)
    a = ctx.render(case.w, case.h, case.camera, **kw)
    img, lists = ctx.read_rgb32f().copy(), _lists(ctx)
    b = ctx.render(case.w, case.h, case.camera, no_beams=True, **kw)
    ref = ctx.read_rgb32f()
    assert tuple(a[k] for k in KEYS) == tuple(b[k] for k in KEYS), case.name
    assert a["primary_rays"] == int(ec.owned_mask(case.w, case.h, case.tile, case.rank, case.world).sum()) * kw["spp"]
    _assert_same_bits(case, img, ref, "the tree walk")
    return img, a, lists


def _assert_oracle(oracle_mod, case, scene, img, spp=None):
    x0, y0, rw, rh = case.region or (0, 0, case.w, case.h)
    kw = case.render_kw(spp)
    ref = oracle_mod.render_extended(oracle_mod.PackedScene(scene, use_bvh=False), case.w, case.h, kw["spp"], 0, camera=case.camera,
                                     frame_seed=case.frame_seed, region=(x0, y0, rw, rh))["rgb"]
    got = img[y0:y0 + rh, x0:x0 + rw].copy()
    owned = ec.owned_mask(case.w, case.h, case.tile, case.rank, case.world)[y0:y0 + rh, x0:x0 + rw]
    ref = ref.copy()
    ref[~owned] = got[~owned]  # (pixels of another share: not this context's)
    diff = np.argwhere((_bits(got) != _bits(ref)).any(-1))
    if len(diff):
        y, x = (int(v) for v in diff[0])
        raise AssertionError(f"{case.name}: {len(diff)} pixels differ between beams and the brute-force oracle, first at (x, y) = ({x + x0}, {y + y0}) "
                             f"in block {ec.block_of_pixel(case, x + x0, y + y0)}: {got[y, x]} != {ref[y, x]}")
    return ref


def _want_lists(case):
    return np.array([NONE if n is ec.NO_LIST else n for n in ec.expected_lists(case)], np.uint32)


def _assert_lists(case, lists):
    want = _want_lists(case)
    assert len(lists) == len(want) and (lists == want).all(), f"{case.name}: debug_beams {lists.tolist()}, stated {want.tolist()}"


# cap ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ec.CAP_NS)
def test_cap(gpu_ctx, oracle_mod, n):
    case = ec.cap(n)
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    img, st, lists = _both(gpu_ctx, case)
    _assert_lists(case, lists)  # (a target block that is not at n + 2: the case did not aim)
    assert lists[case.info["target"]] == (n + 2 if n + 2 <= ec.CAP else NONE)
    _assert_oracle(oracle_mod, case, scene, img)
    img, _, lists = _both(gpu_ctx, case, spp=9)  # jittered, two chunks
    _assert_lists(case, lists)
    _assert_oracle(oracle_mod, case, scene, img, spp=9)


# fallback -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ec.FALLBACK_PATTERNS)
@pytest.mark.parametrize("frame", list(ec.FALLBACK_FRAMES))
def test_fallback(gpu_ctx, oracle_mod, frame, pattern):
    case = ec.fallback(frame, pattern)
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    for spp in ec.FALLBACK_SPP:
        img, st, lists = _both(gpu_ctx, case, spp=spp)
        _assert_lists(case, lists)
        assert int((lists == NONE).sum()) == len(case.info["over"])
        _assert_oracle(oracle_mod, case, scene, img, spp=spp)


# order --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.ORDER))
def test_order(gpu_ctx, oracle_mod, name):
    case = ec.ORDER[name]()
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    img, st, lists = _both(gpu_ctx, case)
    assert len(lists) == len(ec.case_blocks(case)) and (lists != NONE).all(), lists.tolist()  # every block has a list
    print(case.name, "lists", sorted(set(lists.tolist())))
    _assert_oracle(oracle_mod, case, scene, img)


# edges --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp", [64, 1])
def test_edges(gpu_ctx, oracle_mod, spp):
    case = ec.edges(spp)
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    img, st, lists = _both(gpu_ctx, case)
    assert (lists != NONE).all() and lists.min() >= 2
    print(case.name, "lists", lists.tolist())
    _assert_oracle(oracle_mod, case, scene, img)


# pyramids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ec.PYRAMIDS))
def test_pyramids(gpu_ctx, oracle_mod, name):
    case = ec.pyramid(name)
    scene = case.scene()
    gpu_ctx.upload_scene(scene)
    img, st, lists = _both(gpu_ctx, case)
    print(f"{case.name}: {len(lists)} blocks, {int((lists == NONE).sum())} without a list, longest list {int(lists[lists != NONE].max()) if (lists != NONE).any() else 0}")  # recorded, not asserted
    ref = _assert_oracle(oracle_mod, case, scene, img)
    sky = (ref == np.array([0.1, 0.2, 0.3], np.float32)).all(-1)[8:8 + ec.CARPET_PX, 8:8 + ec.CARPET_PX]
    assert 1.0 - sky.mean() >= ec.MIN_COVERAGE  # the oracle sees the carpet the case says it built


# every caller of the lists ----------------------------------------------------------------------------------------------------------
CALLER_CASES = {"cap 126": lambda: ec.cap(126), "fallback alternate": lambda: ec.fallback("20x12 tile 12", "alternate")}


@pytest.mark.parametrize("batch,lanes", [(None, None), ("1", None), (None, "1"), (None, "2"), ("1", "2")])
@pytest.mark.parametrize("which", list(CALLER_CASES))
def test_batches_and_lanes(rt_api, oracle_mod, monkeypatch, which, batch, lanes):
    for key, v in (("RT_WF_BATCH", batch), ("RT_WF_LANES", lanes)):
        if v is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, v)
    case = CALLER_CASES[which]()
    scene = case.scene()
    with rt_api.Context() as ctx:
        ctx.upload_scene(scene)
        for spp in (9, 1):
            img, st, lists = _both(ctx, case, spp=spp)
            _assert_lists(case, lists)
            _assert_oracle(oracle_mod, case, scene, img, spp=spp)


def _adaptive_kw(case):
    kw = case.render_kw()
    del kw["spp"], kw["mode"]
    return kw


@pytest.mark.parametrize("which", list(CALLER_CASES))
def test_adaptive_calls(rt_api, monkeypatch, which):
    """k_wf_beams<true>: the live blocks are renumbered through ad_blocks.  A tiny threshold retires the pixels whose samples are all
    equal (the backdrop away from its diagonal, the sparse blocks) after the first call and keeps the piles running."""
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    case = CALLER_CASES[which]()
    scene = case.scene()
    n_blocks = len(ec.case_blocks(case))
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        live = []
        for i, spp in enumerate((4, 4, 9)):
            a = ctx.render_adaptive(case.w, case.h, case.camera, spp, 1e-6, min_samples=4, restart=i == 0, **_adaptive_kw(case))
            lists = _lists(ctx)
            b = ref.render_adaptive(case.w, case.h, case.camera, spp, 1e-6, min_samples=4, restart=i == 0, no_beams=True, **_adaptive_kw(case))
            assert tuple(a[k] for k in KEYS) == tuple(b[k] for k in KEYS) and a["pixels"] == b["pixels"]
            _assert_same_bits(case, ctx.read_rgb32f(), ref.read_rgb32f(), f"the tree walk (adaptive call {i})")
            assert ctx.read_adaptive().tobytes() == ref.read_adaptive().tobytes()
            live.append((a["pixels"], len(lists), int((lists == NONE).sum())))
        print(which, "adaptive calls (pixels, live blocks, of them without a list):", live)
        with_pixels = int((ec.case_blocks(case)[:, 2] > 0).sum())
        assert live[0][1] == with_pixels <= n_blocks and 0 < live[2][1] < with_pixels and 0 < live[2][0] <= live[1][0] < live[0][0]  # blocks retired, blocks live
        if which == "cap 126":
            assert 128 in lists.tolist()


@pytest.mark.parametrize("which", list(CALLER_CASES))
def test_progressive_accumulation(rt_api, monkeypatch, which):
    """Three accumulating calls of one sample: sample_base > 0, jitter at spp 1."""
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    case = CALLER_CASES[which]()
    scene = case.scene()
    kw = case.render_kw(spp=1)
    with rt_api.Context() as ctx, rt_api.Context() as ref:
        ctx.upload_scene(scene)
        ref.upload_scene(scene)
        for i in range(3):
            a = ctx.render(case.w, case.h, case.camera, accumulate=True, restart=i == 0, **kw)
            _assert_lists(case, _lists(ctx))
            b = ref.render(case.w, case.h, case.camera, accumulate=True, restart=i == 0, no_beams=True, **kw)
            assert tuple(a[k] for k in KEYS) == tuple(b[k] for k in KEYS) and ctx.accumulated_samples() == ref.accumulated_samples() == i + 1
            _assert_same_bits(case, ctx.read_rgb32f(), ref.read_rgb32f(), f"the tree walk (accumulating call {i})")


@pytest.mark.parametrize("which", list(CALLER_CASES))
def test_two_devices(rt_api, oracle_mod, monkeypatch, which):
    torch = pytest.importorskip("torch")
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    monkeypatch.delenv("RT_WF_BATCH", raising=False)
    monkeypatch.delenv("RT_WF_LANES", raising=False)
    case = CALLER_CASES[which]()
    if which == "cap 126":
        case = ec.dataclasses.replace(case, tile=8)  # nine tiles of one block: both devices get some (the lists' statement does not depend on the tiles here)
    scene = case.scene()
    with rt_api.Context((0, 1)) as ctx:
        ctx.upload_scene(scene)
        img, st, lists = _both(ctx, case, spp=9)
        _assert_oracle(oracle_mod, case, scene, img, spp=9)
