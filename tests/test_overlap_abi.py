"""Overlap queries (rt_overlap_box) without a GPU: the symbol, the constants and the struct against the header; the statement, the list
and the whole walk on the host - csrc/overlap_rules.h, the statements the kernel calls - held to a brute force over all primitives
under AddressSanitizer + UBSan (tests/check_overlap.cpp); the numpy float32 statement the GPU tests compare bytes with
(tests/overlap_cases.py) against the same statement in float64 and on hand-worked cases; and what Context.overlap_box validates before
the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import overlap_cases as oc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
INF, NAN = np.inf, np.nan
MISS = cc.PRIM_MISS


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_overlap_box" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_overlap_box")
    assert re.search(r"int rt_overlap_box\(rt_ctx\* ctx, const rt_box\* boxes, size_t n, uint32_t max_prims,\s*uint32_t\* prims,\s*uint32_t\* counts,\s*"
                     r"uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_signed_distance, rt_overlap_box,", _header(), re.S), "listed among the calls a running image survives"
    flat = re.sub(r"\s*\n \*\s+", " ", _header())
    assert "The list gives no spatial bound" in flat and "list mode and RT_QUERY_COUNT_ALL both visit every node the box reaches" in flat
    assert _header().index("Sphere sweeps:") < _header().index("Overlap queries:") < _header().index("Geometry updates:")


def test_defines_agree_with_the_python_constants(rt_api):
    def value(name):
        return int(re.search(r"^#define %s (\d+)u" % name, _header(), re.M).group(1))
    assert value("RT_OVERLAP_MAX") == rt_api.OVERLAP_MAX == oc.OVERLAP_MAX == 32
    assert value("RT_OVERLAP_ANY") == rt_api.OVERLAP_ANY == 4
    assert value("RT_QUERY_COUNT_ALL") == rt_api.QUERY_COUNT_ALL and value("RT_QUERY_COUNTERS") == rt_api.QUERY_COUNTERS
    assert len({value("RT_QUERY_COUNTERS"), value("RT_QUERY_COUNT_ALL"), value("RT_OVERLAP_ANY")}) == 3, "the call's three flags are distinct bits"


def test_struct_layout_agrees_with_the_dtype(tmp_path):
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_box), offsetof(rt_box, center),'
           ' offsetof(rt_box, _pad0), offsetof(rt_box, half_extent), offsetof(rt_box, _pad1));return 0;}\n')
    exe = str(tmp_path / "rt_box_probe")
    subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    vals = list(map(int, subprocess.check_output([exe]).split()))
    assert vals == [T.BOX.itemsize] + [T.BOX.fields[f][1] for f in ("center", "_pad0", "half_extent", "_pad1")] == [32, 0, 12, 16, 28]
    assert T.EXPECTED_SIZES["BOX"] == 32
    b = oc.make_boxes([[1, 2, 3]], [[4, 5, 6]]).view(T.BOX)
    assert b["center"].tolist() == [[[1, 2, 3]]] and b["half_extent"].tolist() == [[[4, 5, 6]]] and not b["_pad0"].any() and not b["_pad1"].any()


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    boxes, prims, counts = (C.c_float * 8)(), (C.c_uint32 * 4)(), (C.c_uint32 * 1)()
    assert lib.rt_overlap_box(C.c_void_p(0), boxes, C.c_size_t(1), C.c_uint32(4), prims, counts, C.c_uint32(0)) == -1
    assert lib.rt_overlap_box(C.c_void_p(0), None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_uint32(0)) == -1
    assert not any(bytes(prims)) and not any(bytes(counts))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ovl") / "check_overlap"
    cc_run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_overlap.cpp"),
                             os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc_run.returncode == 0, cc_run.stderr[-3000:]
    return str(exe)


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every id and count of the walk - statement, list, node test, order and stack as the kernel runs them - is the brute force's at
    K = 1, 4 and 32, with and without COUNT_ALL, and in ANY mode; the stack and the list stay inside the words the kernel's launch
    provides (the program checks every index).  On ordinary input at n = 20000 the small boxes make fewer than n / 10 triangle tests."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        per_k = re.findall(r"^K +(\d+)( COUNT_ALL)? *: 0 failed, ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)
        assert sorted((k, bool(a)) for k, a, _, _ in per_k) == sorted((k, a) for k in ("1", "4", "32") for a in (False, True)), run.stdout[-1500:]
        assert re.search(r"^ANY +: 0 failed", run.stdout, re.M), run.stdout[-1500:]
        small = re.search(r"^small boxes +: ([0-9.]+) node visits and ([0-9.]+) triangle tests per box over (\d+) boxes", run.stdout, re.M)
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            print(f"kind {kind} method {method}: the small boxes make {small.group(2)} triangle tests per box (brute force 20000)")
            assert int(small.group(3)) > 100 and float(small.group(2)) < 20000 / 10, run.stdout[-1500:]


# -- the float32 statement against the float64 one ----------------------------------------------------------------------------
def test_f32_statement_agrees_with_f64_away_from_zero_margin():
    """random_soup(3000, n_spheres=3) with soup_boxes(2048, 11): every pair whose float64 margin is further than 1e-5 from zero agrees;
    the pairs left out are at most 1e-4 of all pairs and the boxes with a pair left out at most 5 %.  Measured on the CPU: 17 of
    6,150,144 pairs left out (2.8e-6), 16 of 2048 boxes (0.8 %), and no disagreement even among the pairs left out."""
    soup = scenes.random_soup(3000, n_spheres=3)
    boxes = oc.soup_boxes(soup, 2048, 11)
    f32 = oc.touching(soup, boxes)
    margin = oc.margins(soup, boxes)
    left_out = np.abs(margin) <= 1e-5
    print(f"{left_out.sum()} of {left_out.size} pairs left out ({left_out.mean():.1e}), {left_out.any(1).sum()} of {len(boxes)} boxes "
          f"({left_out.any(1).mean():.1%}); {((margin >= 0) != f32).sum()} disagreements in all")
    assert f32.shape == margin.shape == (2048, 3003) and f32.any() and not f32.all()
    assert ((margin >= 0) == f32)[~left_out].all()
    assert left_out.mean() <= 1e-4 and left_out.any(1).mean() <= 0.05


# -- the numpy statement on hand-worked cases ---------------------------------------------------------------------------------
def _families(corners, centre, half):
    v0, e1, e2, _ = cc.records(ca.triangles_scene([corners]))
    fam = oc.triangle_families(v0, e1, e2, np.array([centre], F32), np.array([half], F32))
    return tuple(bool(f[0, 0]) for f in fam)


def _touch(scene, centre, half, k=4):
    ids, listed, total = oc.overlap_all(scene, oc.make_boxes([centre], [half]), k)
    return ids[0].tolist(), int(listed[0]), int(total[0])


def test_each_axis_family_separates_alone():
    """(finite, box axes, normal, cross axes): exactly one family separates."""
    assert _families([[3, 0, 0], [0, 3, 0], [0, 0, 3]], (0, 0, 0), (0.9, 0.9, 0.9)) == (True, True, False, True), "the plane x + y + z = 3 misses the corner"
    assert _families([[3, 0, 0], [0, 3, 0], [0, 0, 3]], (0, 0, 0), (1, 1, 1)) == (True, True, True, True), "... and touches it at (1, 1, 1)"
    assert _families([[2.5, 0, 0], [0, 2.5, 0], [2.5, 2.5, 0]], (0, 0, 0), (1, 1, 1)) == (True, True, True, False), "cross(z, the hypotenuse)"
    # in the plane z = 0 a wedge points at the face x = 1 from (1.5, 0); the lines of all three edges cut the square
    assert _families([[1.5, 0, 0], [5, 1, 0], [7, -1, 0]], (0, 0, 0), (1, 1, 1)) == (True, False, True, True), "x >= 1.5"
    assert _families([[0.5, 0, 0], [4, 1, 0], [6, -1, 0]], (0, 0, 0), (1, 1, 1)) == (True, True, True, True), "the same wedge moved in"


def test_the_box_is_closed_and_one_ulp_outside_is_outside():
    one_up = float(np.nextafter(F32(1), F32(2)))
    on = ca.triangles_scene([[[1, 0, 0], [2, 0.5, 0], [2, 0, 0.5]]])
    off = ca.triangles_scene([[[one_up, 0, 0], [2, 0.5, 0], [2, 0, 0.5]]])
    assert _touch(on, (0, 0, 0), (1, 1, 1)) == ([0, MISS, MISS, MISS], 1, 1)
    assert _touch(off, (0, 0, 0), (1, 1, 1)) == ([MISS] * 4, 0, 0)
    corner = ca.triangles_scene([[[1, 1, 1], [2, 1, 1], [1, 2, 3]]])  # meets the box in its corner only
    assert _touch(corner, (0, 0, 0), (1, 1, 1))[2] == 1 and _touch(corner, (0, 0, 0), (1, 1, 0.99))[2] == 0


def test_a_point_a_segment_and_a_slab():
    tri = ca.triangles_scene([ca.UNIT])
    assert _touch(tri, (0.25, 0.25, 0), (0, 0, 0))[2] == 1, "half_extent = 0 on a point of the interior"
    assert _touch(tri, (0.25, 0.25, 1e-3), (0, 0, 0))[2] == 0
    assert _touch(tri, (0.25, 0.25, 0.5), (0, 0, 0.5))[2] == 1 and _touch(tri, (0.75, 0.75, 0), (0, 0, 1))[2] == 0, "a segment along z"
    assert _touch(tri, (5, 5, 0), (10, 10, 0))[2] == 1 and _touch(tri, (5, 5, 0.1), (10, 10, 0))[2] == 0, "a slab"
    assert _touch(ca.tripled_triangle(), (0.25, 0.25, 0), (0, 0, 0), 2) == ([0, 1], 2, 3), "the K lowest keys, and the total"


def test_spheres_are_surfaces_and_come_first():
    scene = ca.triangles_scene([[[1.9, -1, -1], [1.9, 1, -1], [1.9, 0, 1]]], spheres=[((0, 0, 0), 2.0, 0), ((0, 0, 0), 2.0, 0)])
    assert _touch(scene, (0, 0, 0), (0.5, 0.5, 0.5))[2] == 0, "wholly inside the ball"
    assert _touch(scene, (0, 0, 0), (1.2, 1.2, 1.2))[2] == 2, "its corners reach the surface (1.2 * sqrt 3 > 2)"
    assert _touch(scene, (2, 0, 0), (0.5, 0.5, 0.5)) == ([cc.SPHERE_FLAG, cc.SPHERE_FLAG | 1, 0, MISS], 3, 3), "straddles the surface; spheres before triangles"
    assert _touch(scene, (5, 0, 0), (0.5, 0.5, 0.5))[2] == 0
    assert _touch(scene, (2, 0, 0), (0, 0, 0))[2] == 2 and _touch(scene, (0, 0, 0), (50, 50, 50))[2] == 3


def test_degenerate_queries_and_nan_vertices_give_nothing():
    tri = ca.triangles_scene([ca.UNIT], spheres=[((0, 0, 0), 1.0, 0)])
    for centre, half in (((NAN, 0, 0), (1, 1, 1)), ((0, INF, 0), (1, 1, 1)), ((0, 0, 0), (1, NAN, 1)), ((0, 0, 0), (1, 1, INF)), ((0, 0, 0), (1, -1, 1)),
                         ((0, 0, 0), (-0.5, 1, 1))):
        assert _touch(tri, centre, half) == ([MISS] * 4, 0, 0)
    assert _touch(tri, (0, 0, 0), (1, 1, 1))[2] == 2
    for bad in (NAN, INF, -INF):
        for corner in range(3):
            corners = np.array(ca.UNIT, F32)
            corners[corner, 0] = bad
            assert _touch(ca.triangles_scene([corners]), (0, 0, 0), (1, 1, 1))[2] == 0, (bad, corner)
            assert _touch(ca.triangles_scene([corners]), (0, 0, 0), (3e38, 3e38, 3e38))[2] == 0, (bad, corner)


def test_smaller_k_is_a_prefix_and_the_lists_ascend():
    soup = scenes.random_soup(300, n_spheres=3)
    boxes = oc.soup_boxes(soup, 128, 7)
    ids, listed, total = oc.overlap_all(soup, boxes)
    for k in (1, 4):
        want = oc.overlap_all(soup, boxes, k)
        got = oc.first_k(ids, total, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and total.tobytes() == want[2].tobytes()
    key = ids ^ np.uint32(cc.SPHERE_FLAG)
    listed_mask = np.arange(oc.OVERLAP_MAX)[None] < listed[:, None]
    assert (np.diff(key.astype(np.int64), axis=1)[listed_mask[:, 1:]] > 0).all() and ((ids != MISS) == listed_mask).all()
    assert (total > 0).any() and (total == 0).any()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.overlap_box
    good = np.zeros((4, 8), F32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="boxes: shape"):
        call(nc, np.zeros((4, 6), F32), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), F32)[::2], 4)
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8], 4)
    for bad in (-1, 33, 2.0, True, None):
        with pytest.raises(ValueError, match="max_prims"):
            call(nc, good, bad)
    with pytest.raises(ValueError, match="count_all"):
        call(nc, good, 0)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 4, any_hit=True)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 0, any_hit=True, count_all=True)
    with pytest.raises(TypeError):
        call(nc, good, 2, np.zeros((4, 2), np.uint32))  # out is keyword-only
    with pytest.raises(ValueError, match="rows for 4 boxes"):
        call(nc, good, 2, out=np.zeros((3, 2), np.uint32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 3), np.uint32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 2, 1), np.uint32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, out=np.zeros((4, 2), np.int32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="counts: 3 rows"):
        call(nc, good, 2, counts=np.zeros(3, np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_overlap_box(self, h, boxes, n, max_prims, prims, counts, flags):
        self.calls.append((boxes.value, n.value, max_prims.value, prims.value, counts.value, flags.value))
        return 0


def test_overlap_box_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    boxes = rt_api.make_boxes(np.arange(18, dtype=F32).reshape(6, 3), (0.5, 0.25, 1.0))
    assert boxes.shape == (6, 8) and boxes.dtype == np.float32 and boxes.tobytes() == oc.make_boxes(np.arange(18).reshape(6, 3), (0.5, 0.25, 1.0)).tobytes()
    assert rt_api.make_boxes(np.zeros((2, 3)), 0.5)[:, 4:].tolist() == [[0.5, 0.5, 0.5, 0]] * 2
    out, counts = ctx.overlap_box(boxes, 3)
    assert out.shape == (6, 3) and out.dtype == np.uint32 and counts.shape == (6,) and counts.dtype == np.uint32
    own, own_counts = np.zeros((6, 32), np.uint32), np.zeros(6, np.uint32)
    got = ctx.overlap_box(boxes, np.int64(32), out=own, counts=own_counts, count_all=True, counters=True)
    assert got[0] is own and got[1] is own_counts
    none, only_counts = ctx.overlap_box(boxes, 0, out=own, count_all=True)
    assert none is None and only_counts.shape == (6,)
    none, any_counts = ctx.overlap_box(boxes, 0, any_hit=True, counters=True)
    assert none is None and any_counts.shape == (6,)
    assert ctx.lib.calls == [(boxes.ctypes.data, 6, 3, out.ctypes.data, counts.ctypes.data, 0),
                             (boxes.ctypes.data, 6, 32, own.ctypes.data, own_counts.ctypes.data, rt_api.QUERY_COUNTERS | rt_api.QUERY_COUNT_ALL),
                             (boxes.ctypes.data, 6, 0, None, only_counts.ctypes.data, rt_api.QUERY_COUNT_ALL),
                             (boxes.ctypes.data, 6, 0, None, any_counts.ctypes.data, rt_api.OVERLAP_ANY | rt_api.QUERY_COUNTERS)]
