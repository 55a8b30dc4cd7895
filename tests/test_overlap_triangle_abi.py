"""Triangle queries (rt_overlap_triangle) without a GPU: the symbol, the prototype and the record's layout against the header's static
asserts, a ctypes mirror and the numpy dtype; the whole walk on the host - csrc/overlap_triangle_rules.h, the statements the kernel
calls - held to a brute force under AddressSanitizer + UBSan (tests/check_overlap_triangle.cpp, a stand-alone program); the numpy
float32 statement the GPU tests compare bytes with (tests/overlap_triangle_cases.py) held to the same statement in float64, that one
to an independent edge-piercing predicate, and both to hand-worked cases; and what Context.overlap_triangle validates before the
library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import overlap_cases as oc
import overlap_triangle_cases as tc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
INF, NAN = np.inf, np.nan
MISS = cc.PRIM_MISS


class RtQueryTriangle(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("_pad0", C.c_uint32), ("v1", C.c_float * 3), ("_pad1", C.c_uint32), ("v2", C.c_float * 3), ("_pad2", C.c_uint32)]


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and the record ---------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_overlap_triangle" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_overlap_triangle")
    assert re.search(r"int rt_overlap_triangle\(rt_ctx\* ctx, const rt_query_triangle\* triangles, size_t n, uint32_t max_prims,\s*uint32_t\* prims,\s*"
                     r"uint32_t\* counts,\s*uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_overlap_obb, rt_sweep_obb, rt_overlap_triangle,", _header(), re.S), "listed among the calls a running image survives"
    assert _header().index("Oriented boxes:") < _header().index("Triangle queries:") < _header().index("Geometry updates:")
    for define in ("RT_OVERLAP_ANY", "RT_QUERY_COUNT_ALL"):
        assert "rt_overlap_triangle" in re.search(r"^#define %s \d+u +/\*(.*?)\*/" % define, _header(), re.M).group(1), define


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layout_matches_the_mirror_and_the_dtype(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static assert of rt_hip.h holds, and the size and offsets are the ctypes mirror's and the dtype's."""
    fields = [f for f, _ in RtQueryTriangle._fields_]
    args = ", ".join(["sizeof(rt_query_triangle)"] + [f"offsetof(rt_query_triangle, {f})" for f in fields])
    src = '#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", %s);return 0;}\n' % (" ".join(["%zu"] * (1 + len(fields))), args)
    exe = str(tmp_path / "triangle_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got == [48, 0, 12, 16, 28, 32, 44]
    assert got == [C.sizeof(RtQueryTriangle)] + [getattr(RtQueryTriangle, f).offset for f in fields]
    assert got == [T.TRIANGLE_QUERY.itemsize] + [T.TRIANGLE_QUERY.fields[f][1] for f in fields]
    assert T.EXPECTED_SIZES["TRIANGLE_QUERY"] == 48
    assert "RT_STATIC_ASSERT(sizeof(rt_query_triangle) == 48" in _header() and "offsetof(rt_query_triangle, _pad2) == 44" in _header()
    t = tc.make_triangles([[1, 2, 3]], [[4, 5, 6]], [[7, 8, 9]]).view(T.TRIANGLE_QUERY)
    assert t["v0"].tolist() == [[[1, 2, 3]]] and t["v1"].tolist() == [[[4, 5, 6]]] and t["v2"].tolist() == [[[7, 8, 9]]]
    assert not t["_pad0"].any() and not t["_pad1"].any() and not t["_pad2"].any()


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    tris, prims, counts = (RtQueryTriangle * 1)(), (C.c_uint32 * 4)(), (C.c_uint32 * 1)()
    assert lib.rt_overlap_triangle(C.c_void_p(0), tris, C.c_size_t(1), C.c_uint32(4), prims, counts, C.c_uint32(0)) == -1
    assert lib.rt_overlap_triangle(C.c_void_p(0), None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_uint32(0)) == -1
    assert not any(bytes(prims)) and not any(bytes(counts))


def test_the_overlap_body_stays_written_once():
    """The entry is a host unit of its own that calls rt_query.cpp's checks and batch; nothing new includes query_plan.h."""
    for name in ("overlap_triangle_rules.h", "overlap_triangle.hip", "overlap_triangle.h", "rt_mesh_query.cpp"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name
    unit = open(os.path.join(CSRC, "rt_mesh_query.cpp")).read()
    assert unit.count("overlap_query(ctx, ") == 1 and "run_batch" not in unit and "RT_OVERLAP_ANY" not in unit
    assert re.search(r"^int overlap_query\(", open(os.path.join(CSRC, "rt_internal.h")).read(), re.M)


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_overlap_triangle.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("ovt") / "check_overlap_triangle")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every id and count of the walk - statement, list, node test, order and stack as the kernel runs them - is the brute force's at
    K = 1, 4 and 32, with and without COUNT_ALL, and in ANY mode; the stack and the list stay inside the words the kernel's launch
    provides (the program checks every index); every query made on a corner of a record's bounds touches.  On ordinary input at
    n = 20000 the small triangles make fewer than n / 10 triangle tests."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        per_k = re.findall(r"^K +(\d+)( COUNT_ALL)? *: 0 failed, ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)
        assert sorted((k, bool(a)) for k, a, _, _ in per_k) == sorted((k, a) for k in ("1", "4", "32") for a in (False, True)), run.stdout[-1500:]
        assert re.search(r"^ANY +: 0 failed", run.stdout, re.M), run.stdout[-1500:]
        made, touch = map(int, re.search(r"^corner queries: (\d+) made, (\d+) of them touch", run.stdout, re.M).groups())
        assert made == touch and (made > 0 or (n == 1 and kind == 5)), run.stdout[-1500:]
        small = re.search(r"^small queries +: ([0-9.]+) node visits and ([0-9.]+) triangle tests per triangle over (\d+) triangles", run.stdout, re.M)
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            print(f"kind {kind} method {method}: the small triangles make {small.group(2)} triangle tests per query (brute force 20000)")
            assert int(small.group(3)) > 100 and float(small.group(2)) < 20000 / 10, run.stdout[-1500:]


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the node test's margin negative the queries that touch a record only at a corner of its bounds lose it wherever a child
    box's plane is exact, and the check must report wrong answers."""
    exe = _build_checker(tmp_path / "check_overlap_triangle_flipped", "-DRT_CP_SLACK=-1.0e-5f")
    for n in (300, 20000):
        run = subprocess.run([exe, str(n), "1", "0", "0"], capture_output=True, text=True)
        failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
        print(run.stdout.strip().splitlines()[-1])
        assert run.returncode == 1 and failures > 0


# -- the float32 statement against the float64 one, and that one against an independent predicate -----------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000, n_spheres=3), "cornell12": scenes.cornell12}
GRID = sorted(m * 10.0 ** e for e in range(-12, 1) for m in (1, 1.5, 2, 3, 5, 7))


def _smallest_k(worst):
    return 0.0 if worst <= 0 else next(k for k in GRID if k >= worst)


@pytest.fixture(scope="module")
def soup_case():
    soup = SCENES["soup"]()
    tris = tc.soup_triangles(soup, 2048, 11)
    return soup, tris, tc.touching(soup, tris), tc.gaps(soup, tris)


def test_the_soup_batch_fills_and_overflows_its_lists(soup_case):
    """On the CPU: 28.5 % / 22.0 % at K = 4, 44.9 % / 7.8 % at K = 16, 1.9 % above 32, 46.5 % empty, at most 61; the spheres are
    touched by 34, 47 and 4 queries."""
    _, _, f32, _ = soup_case
    total = f32.sum(1)
    for k in (4, 16):
        short, over = ((total > 0) & (total < k)).mean(), (total > k).mean()
        print(f"K = {k}: {short:.1%} of the queries with 1 .. {k - 1} primitives, {over:.1%} with more than {k}")
        assert short > 0.05 and over > 0.05
    print(f"{(total == 0).mean():.1%} empty, {(total > 32).mean():.1%} above 32, at most {total.max()}; spheres touched by {f32[:, :3].sum(0).tolist()} queries")
    assert (total > 32).any() and f32[:, :3].any()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_f32_statement_agrees_with_f64_within_k_diagonals(name, soup_case):
    """For every pair: "touches in f32" implies gap64 <= k x diagonal and "does not" implies gap64 >= -k x diagonal, with k twice
    K_MEASURED.  Measured on the CPU: no pair of either batch disagrees in sign (soup: 6,150,144 pairs, 8,187 touching; cornell12:
    the same generator), so K_MEASURED is 0 for both and the assertion is that none does."""
    if name == "soup":
        scene, tris, f32, (f64, gap, _) = soup_case
    else:
        scene = SCENES[name]()
        tris = tc.soup_triangles(scene, 2048, 11)
        f32, (f64, gap, _) = tc.touching(scene, tris), tc.gaps(scene, tris)
    diag = cc.diagonal(scene)
    worst = np.where(f32, gap, -gap).max() / diag
    k = _smallest_k(worst)
    print(f"{name}: {f32.size} pairs, {f32.sum()} touch in f32, {(f32 != f64).sum()} differ from f64; worst signed gap {worst:.3g} diagonals -> k = {k:g} "
          f"(recorded {tc.K_MEASURED[name]:g})")
    assert f32.any() and not f32.all()
    assert ((gap <= 0) == f64).all(), "the gap's sign is the float64 statement"
    assert (np.where(f32, gap, -gap) <= 2 * tc.K_MEASURED[name] * diag).all()


def test_f64_statement_is_the_edge_piercing_predicate(soup_case):
    """Some edge of one triangle pierces the other (closed Moeller-Trumbore, both ways) exactly where the float64 statement holds, on
    every soup pair whose |gap64| exceeds 2 x K_MEASURED diagonals - all of them while that is 0 - and whose bounds are not clearly
    apart (the others are not evaluated: nothing pierces across disjoint bounds).  On the CPU: 86,440 pairs, 8,102 touch."""
    soup, tris, _, (f64, gap, evaluated) = soup_case
    ns = len(soup.spheres)
    rows, cols = np.nonzero(evaluated[:, ns:])
    pierce = tc.pierces(soup, tris, rows, cols)
    clear = np.abs(gap[:, ns:][rows, cols]) > 2 * tc.K_MEASURED["soup"] * cc.diagonal(soup)
    print(f"{len(rows)} pairs evaluated, {clear.sum()} of them clear, {pierce.sum()} pierce, {f64[:, ns:].sum()} touch")
    assert pierce.sum() > 1000 and clear.mean() > 0.99
    assert (pierce == f64[:, ns:][rows, cols])[clear].all()
    assert not f64[:, ns:][~evaluated[:, ns:]].any()


def test_scene_triangles_and_their_edges_list_themselves(soup_case):
    """Offered as the query (v0, v0 + e1, v0 + e2), a_k equals the query's own relative vertices bit for bit, so every span holds its
    own ends: each record lists itself, and so does each of its edges as a segment query."""
    soup = soup_case[0]
    v0, e1, e2, _ = cc.records(soup)
    s = (v0, v0 + e1, v0 + e2)
    ns, idx = len(soup.spheres), np.arange(len(v0))
    assert tc.touching(soup, tc.make_triangles(*s))[idx, ns + idx].all()
    for i, j in ((0, 1), (1, 2), (2, 0)):
        assert tc.touching(soup, tc.make_triangles(s[i], s[j], s[j]))[idx, ns + idx].all(), (i, j)
        assert tc.touching(soup, tc.make_triangles(s[i], s[i], s[j]))[idx, ns + idx].all(), (i, j)


def test_lattice_triangles_and_points_on_coplanar_walls():
    """Exact arithmetic: f32 equals f64 on every pair, every total from 0 to 8 occurs, and a point query on a lattice point gives
    overlap_cases' answer for the zero-extent box there."""
    walls, tris = ca.coplanar_walls(), tc.lattice_triangles()
    f32 = tc.touching(walls, tris)
    total = f32.sum(1)
    v = tc.vertices(tris)
    repeated = (v[0] == v[1]).all(1) | (v[1] == v[2]).all(1) | (v[0] == v[2]).all(1)
    print(f"totals {np.bincount(total).tolist()}, {repeated.sum()} queries with a repeated vertex")
    assert all((total == t).any() for t in range(9)) and total.max() == 8
    assert (tc.gaps(walls, tris, near=np.inf)[0] == f32).all()
    points, boxes = tc.lattice_points()
    on_points = tc.touching(walls, points)
    assert (on_points == oc.touching(walls, boxes)).all() and on_points.any() and not on_points.all(1).any()


# -- the numpy statement on hand-worked cases ---------------------------------------------------------------------------------
def _touch(scene, v0, v1, v2, k=4):
    ids, listed, total = tc.overlap_all(scene, tc.make_triangles([v0], [v1], [v2]), k)
    return ids[0].tolist(), int(listed[0]), int(total[0])


def test_the_triangle_is_closed_and_one_ulp_outside_is_outside():
    tri = ca.triangles_scene([ca.UNIT])  # (0, 0, 0), (1, 0, 0), (0, 1, 0)
    one_up = float(np.nextafter(F32(1), F32(2)))
    assert _touch(tri, (1, 0, 0), (2, 0, 1), (2, 1, -1)) == ([0, MISS, MISS, MISS], 1, 1), "a shared vertex"
    assert _touch(tri, (one_up, 0, 0), (2, 0, 1), (2, 1, -1))[2] == 0
    assert _touch(tri, (0.25, 0.25, -1), (0.25, 0.25, 1), (0.25, 0.25, 1))[2] == 1, "a segment through the interior"
    assert _touch(tri, (0.25, 0.25, 0), (0.25, 0.25, 1), (3, 3, 1))[2] == 1, "... that ends on it"
    assert _touch(tri, (0.25, 0.25, 1e-3), (0.25, 0.25, 1), (3, 3, 1))[2] == 0
    assert _touch(tri, (0.75, 0.75, -1), (0.75, 0.75, 1), (0.75, 0.75, 1))[2] == 0, "past the hypotenuse"
    assert _touch(tri, (0.25, 0.25, 0), (0.25, 0.25, 0), (0.25, 0.25, 0))[2] == 1, "a point of the interior"
    assert _touch(ca.tripled_triangle(), (0.25, 0.25, -1), (0.25, 0.25, 1), (0.3, 0.25, 1), 2) == ([0, 1], 2, 3), "the K lowest keys, and the total"


def test_coplanar_pairs_and_segments_need_the_in_plane_axes():
    """Turned out of the coordinate planes, so that no coordinate axis helps: a coplanar triangle beside the scene's triangle, and a
    coplanar segment beside it, are separated only by the in-plane axes (the last twelve)."""
    c, s = np.cos(0.7), np.sin(0.6)
    rot = np.array([[c, -np.sin(0.7), 0], [np.sin(0.7), c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.6), -s], [0, s, np.cos(0.6)]])
    turn = lambda p: (rot @ np.array(p, float)).tolist()
    scene = ca.triangles_scene([[turn(p) for p in ca.UNIT]])
    assert _touch(scene, turn((0.2, 0.2, 0)), turn((2, 0.1, 0)), turn((0.1, 2, 0)))[2] == 1, "coplanar, overlapping"
    assert _touch(scene, turn((0.6, 0.6, 0)), turn((2, 0.7, 0)), turn((0.7, 2, 0)))[2] == 0, "coplanar, beyond the hypotenuse"
    assert _touch(scene, turn((0.1, 0.1, 0)), turn((0.2, 0.3, 0)), turn((0.2, 0.3, 0)))[2] == 1, "a coplanar segment inside"
    assert _touch(scene, turn((0.9, 0.4, 0)), turn((0.4, 0.9, 0)), turn((0.4, 0.9, 0)))[2] == 0, "a coplanar segment along the hypotenuse, outside"
    # a coplanar segment past the corner (1, 0): it overlaps the triangle's extent along each of the triangle's edge normals, and only its
    # own in-plane normal (0.6, 0.3) separates the two (0.63 against at most 0.6)
    beside = tc.make_triangles([turn((1.2, -0.3, 0))], [turn((0.9, 0.3, 0))], [turn((0.9, 0.3, 0))])
    assert tc.touching(scene, beside).sum() == 0
    # without the last six axes (cross(nS, u_i), cross(nQ, f_j)) that segment would be listed: in float64, none of the first 17 separates
    # it by more than rounding noise (the cross(u_i, f_j) are multiples of the normal, along which both extents are the plane's), and
    # one of the last six does by 0.03 / |(0.6, 0.3)|
    v0, e1, e2, _ = cc.records(scene, np.float64)
    q0, q1, q2 = (v.astype(np.float64) for v in tc.vertices(beside))
    a = [v0 - q0, (v0 + e1) - q0, (v0 + e2) - q0]
    sep = []
    for L in tc.axes(q1 - q0, q2 - q0, e1, e2):
        lo_s, hi_s, lo_q, hi_q, _ = tc._project(L, a, q1 - q0, q2 - q0)
        length = float(np.sqrt((L * L).sum()))
        sep.append(float(np.maximum(lo_s - hi_q, lo_q - hi_s)[0]) / length if length > 0 else -np.inf)
    assert len(sep) == 23 and max(sep[:17]) < 1e-6 and max(sep[17:]) > 0.04


def test_spheres_are_surfaces_and_come_first():
    scene = ca.triangles_scene([[[1.9, -1, -1], [1.9, 1, -1], [1.9, 0, 1]]], spheres=[((0, 0, 0), 2.0, 0), ((0, 0, 0), 2.0, 0)])
    assert _touch(scene, (0, 0, 0), (0.5, 0, 0), (0, 0.5, 0))[2] == 0, "wholly inside the ball"
    assert _touch(scene, (0, 0, 0), (1.5, 0, 0), (0, 3, 0))[2] == 2, "one vertex outside: the surface passes through"
    assert _touch(scene, (1.5, 0, 0), (2.5, 0.1, 0), (2.5, -0.1, 0.1)) == ([cc.SPHERE_FLAG, cc.SPHERE_FLAG | 1, 0, MISS], 3, 3), "spheres before triangles"
    assert _touch(scene, (5, 0, 0), (6, 0, 0), (5, 1, 0))[2] == 0
    assert _touch(scene, (2, 0, 0), (2, 0, 0), (2, 0, 0))[2] == 2, "a point on the surface"
    assert _touch(scene, (-9, -9, 0.5), (9, -9, 0.5), (0, 9, 0.5))[2] == 3, "a large triangle cuts the ball with all its vertices outside"


def test_non_finite_queries_and_vertices_give_nothing():
    tri = ca.triangles_scene([ca.UNIT], spheres=[((0, 0, 0), 1.0, 0)])
    good = [(0.25, 0.25, -1), (0.25, 0.25, 1), (3, 3, 1)]
    assert _touch(tri, *good)[2] == 2
    for bad in (NAN, INF, -INF):
        for vertex in range(3):
            for axis in range(3):
                q = [list(p) for p in good]
                q[vertex][axis] = bad
                assert _touch(tri, *q) == ([MISS] * 4, 0, 0), (bad, vertex, axis)
        for corner in range(3):
            corners = np.array(ca.UNIT, F32)
            corners[corner, 0] = bad
            assert _touch(ca.triangles_scene([corners]), *good)[2] == 0, (bad, corner)
            assert _touch(ca.triangles_scene([corners]), (-3e38, -3e38, 0), (3e38, -3e38, 0), (0, 3e38, 0))[2] == 0, (bad, corner)


def test_smaller_k_is_a_prefix_and_the_lists_ascend(soup_case):
    soup, tris, f32, _ = soup_case
    tris, f32 = tris[:256], f32[:256]
    ids, listed, total = tc.overlap_all(soup, tris, touch=f32)
    for k in (1, 4):
        want = tc.overlap_all(soup, tris, k, touch=f32)
        got = tc.first_k(ids, total, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and total.tobytes() == want[2].tobytes()
    key = ids ^ np.uint32(cc.SPHERE_FLAG)
    listed_mask = np.arange(tc.OVERLAP_MAX)[None] < listed[:, None]
    assert (np.diff(key.astype(np.int64), axis=1)[listed_mask[:, 1:]] > 0).all() and ((ids != MISS) == listed_mask).all()
    assert (total > 0).any() and (total == 0).any()


def test_deck_slivers_have_their_boxes_bounds():
    for kind in ("corner", "covered", "mixed"):
        t, b = tc.deck_triangles(kind), oc.deck_boxes(kind)
        lo, hi = tc.bounds(t)
        assert (lo == b[:, 0:3] - b[:, 4:7]).all() and (hi == b[:, 0:3] + b[:, 4:7]).all() and tc.valid(t).all()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.overlap_triangle
    good = np.zeros((4, 12), F32)
    with pytest.raises(TypeError, match="triangles: dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="triangles: shape"):
        call(nc, np.zeros((4, 9), F32), 4)
    with pytest.raises(ValueError, match="triangles: not C-contiguous"):
        call(nc, np.zeros((8, 12), F32)[::2], 4)
    with pytest.raises(TypeError, match="triangles"):
        call(nc, [[0.0] * 12], 4)
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
    with pytest.raises(ValueError, match="rows for 4 triangles"):
        call(nc, good, 2, out=np.zeros((3, 2), np.uint32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 3), np.uint32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, out=np.zeros((4, 2), np.int32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="counts: 3 rows for 4 triangles"):
        call(nc, good, 2, counts=np.zeros(3, np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_overlap_triangle(self, h, triangles, n, max_prims, prims, counts, flags):
        self.calls.append((triangles.value, n.value, max_prims.value, prims.value, counts.value, flags.value))
        return 0


def test_overlap_triangle_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    v = np.arange(54, dtype=F32).reshape(3, 6, 3)
    tris = rt_api.make_triangles(v[0], v[1], v[2])
    assert tris.shape == (6, 12) and tris.dtype == np.float32 and tris.tobytes() == tc.make_triangles(v[0], v[1], v[2]).tobytes()
    out, counts = ctx.overlap_triangle(tris, 3)
    assert out.shape == (6, 3) and out.dtype == np.uint32 and counts.shape == (6,) and counts.dtype == np.uint32
    own, own_counts = np.zeros((6, 32), np.uint32), np.zeros(6, np.uint32)
    got = ctx.overlap_triangle(tris, np.int64(32), out=own, counts=own_counts, count_all=True, counters=True)
    assert got[0] is own and got[1] is own_counts
    none, only_counts = ctx.overlap_triangle(tris, 0, out=own, count_all=True)
    assert none is None and only_counts.shape == (6,)
    none, any_counts = ctx.overlap_triangle(tris, 0, any_hit=True, counters=True)
    assert none is None and any_counts.shape == (6,)
    assert ctx.lib.calls == [(tris.ctypes.data, 6, 3, out.ctypes.data, counts.ctypes.data, 0),
                             (tris.ctypes.data, 6, 32, own.ctypes.data, own_counts.ctypes.data, rt_api.QUERY_COUNTERS | rt_api.QUERY_COUNT_ALL),
                             (tris.ctypes.data, 6, 0, None, only_counts.ctypes.data, rt_api.QUERY_COUNT_ALL),
                             (tris.ctypes.data, 6, 0, None, any_counts.ctypes.data, rt_api.OVERLAP_ANY | rt_api.QUERY_COUNTERS)]
