"""Triangle sweeps (rt_sweep_triangle) without a GPU: the symbol, the prototype and the records' layouts against the header's static
asserts, ctypes mirrors and the numpy dtypes; the whole walk on the host - csrc/sweep_triangle_rules.h, the statements the kernel
calls - held to a brute force under AddressSanitizer + UBSan (tests/check_sweep_triangle.cpp, a stand-alone program); the numpy
float32 statement the GPU tests compare bytes with (tests/sweep_triangle_cases.py) held to the same statement in float64, that one to
the static test along the path and to an independent feature-pair computation, and both to hand-worked cases; the start in contact
held to the overlap statement bit for bit; and what Context.sweep_triangle validates before the library."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import overlap_triangle_cases as tc
import sweep_triangle_cases as st
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32, F64 = np.float32, np.float64
INF = np.inf
NONE = st.AXIS_NONE


class RtTriangleSweep(C.Structure):
    _fields_ = [("v0", C.c_float * 3), ("_pad0", C.c_uint32), ("v1", C.c_float * 3), ("_pad1", C.c_uint32), ("v2", C.c_float * 3), ("_pad2", C.c_uint32),
                ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtTriangleSweepHit(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("t", C.c_float), ("axis", C.c_uint32), ("_reserved", C.c_uint32), ("prim_id", C.c_uint32), ("material_id", C.c_uint32)]


MIRRORS = {"rt_triangle_sweep": (RtTriangleSweep, T.TRIANGLE_SWEEP), "rt_triangle_sweep_hit": (RtTriangleSweepHit, T.TRIANGLE_SWEEP_HIT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_sweep_triangle" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_sweep_triangle")
    assert re.search(r"int rt_sweep_triangle\(rt_ctx\* ctx, const rt_triangle_sweep\* sweeps, size_t n, rt_triangle_sweep_hit\* out, uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_overlap_triangle, rt_sweep_triangle,", _header(), re.S), "listed among the calls a running image survives"
    assert re.search(r"#define RT_SWEEP_TRIANGLE_AXIS_SPHERE 26u\n", code)
    assert rt_api.SWEEP_TRIANGLE_AXIS_SPHERE == st.AXIS_SPHERE == 26 and rt_api.SWEEP_AXIS_NONE == NONE
    assert _header().index("Triangle queries:") < _header().index("Triangle sweeps:") < _header().index("Geometry updates:")
    unit = open(os.path.join(CSRC, "rt_mesh_query.cpp")).read()
    assert unit.count("record_query(ctx, ") == 1 and "run_batch" not in unit
    assert re.search(r"^int record_query\(", open(os.path.join(CSRC, "rt_internal.h")).read(), re.M)
    for name in ("sweep_triangle_rules.h", "sweep_triangle.hip", "sweep_triangle.h"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "swt_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [64, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtTriangleSweep, f).offset for f, _ in RtTriangleSweep._fields_] == [0, 12, 16, 28, 32, 44, 48, 60]
    assert [getattr(RtTriangleSweepHit, f).offset for f, _ in RtTriangleSweepHit._fields_] == [0, 12, 16, 20, 24, 28]
    assert T.EXPECTED_SIZES["TRIANGLE_SWEEP"] == 64 and T.EXPECTED_SIZES["TRIANGLE_SWEEP_HIT"] == 32
    assert all(T.TRIANGLE_SWEEP.fields[f][1] == T.TRIANGLE_QUERY.fields[f][1] for f in T.TRIANGLE_QUERY.names), "an rt_query_triangle first"
    assert [T.TRIANGLE_SWEEP.fields[f][1] - 48 for f in ("direction", "tmax")] == [T.SWEEP.fields[f][1] - 16 for f in ("direction", "tmax")], "then half an rt_sweep"
    assert T.TRIANGLE_SWEEP_HIT == T.BOX_SWEEP_HIT
    header = _header()  # the header asserts them itself
    assert "RT_STATIC_ASSERT(sizeof(rt_triangle_sweep) == 64" in header and "RT_STATIC_ASSERT(sizeof(rt_triangle_sweep_hit) == 32" in header
    for text in ("offsetof(rt_triangle_sweep, direction) == 48", "offsetof(rt_triangle_sweep, tmax) == 60", "offsetof(rt_triangle_sweep_hit, t) == 12",
                 "offsetof(rt_triangle_sweep_hit, axis) == 16", "offsetof(rt_triangle_sweep_hit, prim_id) == 24", "offsetof(rt_triangle_sweep_hit, material_id) == 28"):
        assert text in header, text


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    sweeps, out = (RtTriangleSweep * 1)(), (RtTriangleSweepHit * 1)()
    assert lib.rt_sweep_triangle(C.c_void_p(0), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_triangle(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_sweep_triangle.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("swt") / "check_sweep_triangle")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every answer of the walk - bound, order, stack, leaf test and its early returns as the kernel runs them - has the bytes of the
    brute force, which knows no limit, and the stack stays inside the entries the kernel's launch provides (the program checks every
    index).  On ordinary input at n = 20000 a small sweep makes fewer than n / 10 triangle tests."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        small = re.search(r"^small sweeps: ([0-9.]+) node visits and ([0-9.]+) triangle tests per sweep over (\d+) sweeps", run.stdout, re.M)
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            print(f"kind {kind} method {method}: {small.group(1)} node visits and {small.group(2)} triangle tests per small sweep (brute force 20000)")
            assert int(small.group(3)) > 100 and float(small.group(2)) < 20000 / 10, run.stdout[-500:]
        if n == 300 and kind in (0, 1):  # every group of axes closes some contact last (on the plane the in-plane ones too), and the spheres and the starts in contact are there
            counts = list(map(int, re.search(r"axes 0\.\.25, sphere, none:((?: \d+){28})", run.stdout).group(1).split()))
            groups = [sum(counts[0:3]), sum(counts[3:5]), sum(counts[5:14]), counts[26], counts[27]] + ([sum(counts[14:20]), sum(counts[20:26])] if kind == 1 else [])
            assert all(c > 0 for c in groups), counts


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the margin's sign flipped (-1e-5 for 1e-5, nothing else) the child boxes are narrower than the query's bounds ask and the
    entry times later: the corner sweeps and the flat-on-flat ones lose their records, and the check must report wrong answers."""
    exe = _build_checker(tmp_path / "check_sweep_triangle_flipped", "-DRT_SWB_SLACK=-1.0e-5f")
    for n in (300, 20000):
        run = subprocess.run([exe, str(n), "1", "0", "0"], capture_output=True, text=True)
        failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
        print(run.stdout.strip().splitlines()[-1])
        assert run.returncode == 1 and failures > 0


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000, n_spheres=3), "cornell12": scenes.cornell12, "plane": st.plane_scene}


@pytest.fixture(scope="module")
def cases():
    """name -> (scene, all its fixture sweeps, the float32 statement's records, the float64 statement's times), computed once."""
    out = {}
    for name, make in SCENES.items():
        scene = make()
        sweeps = np.concatenate(list(st.fixtures(name, scene).values()))
        out[name] = (scene, sweeps, st.brute_force(scene, sweeps), st.times(scene, sweeps, F64))
    return out


def test_fixtures_close_on_every_group_of_axes(cases):
    """A condition on the inputs of the GPU tests, by the numpy statement: over all fixtures each group of contact_kinds has at least
    20 members (the misses 100).  In general position only axes 3 .. 13 close last; the aimed sets are what fills the others."""
    total = np.zeros(8, int)
    for name, (_, _, rec, _) in cases.items():
        kinds = [int(m.sum()) for m in st.contact_kinds(rec)]
        print(name, dict(zip(("0-2", "3-4", "5-13", "14-19", "20-25", "sphere", "at start", "miss"), kinds)))
        total += kinds
    assert (total[:7] >= 20).all() and total[7] >= 100, total
    general = st.contact_kinds(st.brute_force(cases["soup"][0], st.fixtures("soup", cases["soup"][0])["five_kinds"]))
    assert general[0].sum() + general[3].sum() + general[4].sum() == 0, "the soup in general position closes on none of them"


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_lies_between_the_float64_ones_of_wider_and_narrower_spans(name, cases):
    """t64(+eps) <= t32 <= t64(-eps) with a relative 1e-6 on finite times, for every sweep of the scene's fixtures, none left out:
    eps = 2 x K_MEASURED x the scene's diagonal, K_MEASURED at most the box sweep's cap."""
    scene, sweeps, rec, _ = cases[name]
    assert st.K_MEASURED[name] <= 1e-4
    eps = 2 * st.K_MEASURED[name] * cc.diagonal(scene)
    t32 = st.times(scene, sweeps, F32).astype(F64)
    hit = rec[:, 6].view(np.uint32) != st.PRIM_MISS
    assert (t32[hit] == rec[hit, 3]).all() and np.isinf(t32[~hit]).all(), "times() is the brute force's t"
    early, late = st.times(scene, sweeps, F64, eps), st.times(scene, sweeps, F64, -eps)
    below, above = early * (1 - 1e-6) <= t32, t32 <= np.where(np.isfinite(late), late * (1 + 1e-6), late)
    print(f"{name}: {len(sweeps)} sweeps, {hit.sum()} hit, eps {eps:.3g}: {(~below).sum()} before t64(+eps), {(~above).sum()} after t64(-eps)")
    assert below.all() and above.all()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float64_statement_touches_at_its_time_and_not_before(name, cases):
    """Against the static 26-axis test in float64: at the statement's time the clearance is within 1e-9 diagonals of 0, at 25, 50, 75,
    95 and 99.9 % of it the triangle is clear, and a miss stays clear along ten diagonals."""
    scene, sweeps, _, t64 = cases[name]
    diag = cc.diagonal(scene)
    q0, q1, q2, d = st._parts(sweeps, F64)
    at = lambda rows, t: [q[rows] + d[rows] * np.asarray(t)[:, None] for q in (q0, q1, q2)]
    moving = np.flatnonzero(np.isfinite(t64) & (t64 > 0))
    touch = st.clearance(scene, *at(moving, t64[moving]))
    print(f"{name}: {len(moving)} contacts with t > 0: clearance at t within {np.abs(touch).max() / diag:.3g} diagonals")
    assert len(moving) >= 100 and (np.abs(touch) <= 1e-9 * diag).all()
    for part in (0.25, 0.5, 0.75, 0.95, 0.999):
        clear = st.clearance(scene, *at(moving, t64[moving] * part))
        assert (clear > 0).all(), (part, int((clear <= 0).sum()))
    start = np.flatnonzero(t64 == 0)
    assert (st.clearance(scene, q0[start], q1[start], q2[start]) <= 0).all()
    miss = np.flatnonzero(np.isinf(t64))  # all of them: every kind and every aimed set
    speed = np.linalg.norm(d[miss], axis=1)
    for part in np.linspace(0.0, 1.0, 41):
        clear = st.clearance(scene, *at(miss, part * 10 * diag / speed))
        assert (clear > 0).all(), (part, int((clear <= 0).sum()))


def _pairs_with_winners(scene, sweeps, seed):
    """(sweep, triangle) pairs: each sweep with the triangle the float64 statement meets first (where it meets one) and with a drawn
    one -> rows, cols, the float64 statement's time of each pair."""
    t = st.triangle_times_all(scene, sweeps, F64)
    first = np.where(np.isnan(t), INF, t).argmin(1)
    drawn = np.random.default_rng(seed).integers(0, t.shape[1], len(sweeps))
    rows = np.concatenate([np.arange(len(sweeps))] * 2)
    cols = np.concatenate([first, drawn])
    return rows, cols, t[rows, cols]


def test_float64_statement_is_the_feature_pair_computation(cases):
    """Three query-vertex rays, three scene-vertex rays and nine edge pairs, in float64, give the statement's time to 1e-9 relative on
    the soup's sweeps in general position that do not start in contact; pairs with a 3 x 3 system singular to 1e-12 are left out, at
    most 1 % of them.  Point queries agree with a Moeller-Trumbore ray."""
    scene = cases["soup"][0]
    sweeps = st.fixtures("soup", scene)["five_kinds"]
    kind = np.repeat(np.arange(5), 600)
    sweeps = sweeps[(kind == 0) | (kind == 1) | (kind == 4)]  # toward surfaces, scattered, from far outside: triangles of the four sizes
    rows, cols, t = _pairs_with_winners(scene, sweeps, 5)
    keep = t != 0
    rows, cols, t = rows[keep], cols[keep], t[keep]
    v0, e1, e2, _ = cc.records(scene, F64)
    q0, q1, q2, d = st._parts(sweeps, F64)
    ft, singular = st.feature_times(v0[cols], e1[cols], e2[cols], q0[rows], q1[rows], q2[rows], d[rows])
    both = np.isfinite(t) & np.isfinite(ft)
    with np.errstate(invalid="ignore"):
        agree = (np.isinf(t) & np.isinf(ft)) | (both & (np.abs(t - ft) <= 1e-9 * np.maximum(t, ft)))
    print(f"{len(t)} pairs, {np.isfinite(t).sum()} meet, {singular.sum()} left out as singular, {(~agree & ~singular).sum()} disagree")
    assert np.isfinite(t).sum() >= 1000 and singular.mean() <= 0.01
    assert agree[~singular].all()
    points = st.segments_and_points(scene, 600, 21)[2::3]
    assert (points[:, 0:3] == points[:, 4:7]).all() and (points[:, 0:3] == points[:, 8:11]).all()
    rows, cols, t = _pairs_with_winners(scene, points, 6)
    p, _, _, d = st._parts(points, F64)
    ray = st.point_ray_times(v0[cols], e1[cols], e2[cols], p[rows], d[rows])
    both = np.isfinite(t) & np.isfinite(ray)
    print(f"{len(t)} point pairs, {both.sum()} meet")
    assert both.sum() >= 50 and (np.isfinite(t) == np.isfinite(ray)).all() and (np.abs(t[both] - ray[both]) <= 1e-9 * ray[both]).all()


def test_prefiltered_brute_force_is_the_brute_force(cases):
    scene, sweeps, rec, _ = cases["soup"]
    pick = np.arange(0, len(sweeps), 8)
    np.testing.assert_array_equal(st.brute_force(scene, sweeps[pick], prefilter=True).view(np.uint32), rec[pick].view(np.uint32))


def test_contact_at_the_start_is_the_overlap_statement(cases):
    """Bit for bit, on the soup without its spheres: t == 0 exactly where overlap_triangle_cases lists something for the triangle at
    its start, and then prim_id is that statement's lowest key; the axis is NONE and the normal 0."""
    soup, sweeps, _, _ = cases["soup"]
    scene = dataclasses.replace(soup, spheres=soup.spheres[:0])
    rec = st.brute_force(scene, sweeps).view(T.TRIANGLE_SWEEP_HIT).reshape(-1)
    touches = tc.touching(scene, np.ascontiguousarray(sweeps[:, 0:12]))
    at_start = (rec["prim_id"] != st.PRIM_MISS) & (rec["t"] == 0)
    print(f"{len(sweeps)} sweeps, {at_start.sum()} start in contact")
    assert len(sweeps) >= 2000 and at_start.sum() >= 500 and (~at_start).sum() >= 500
    np.testing.assert_array_equal(at_start, touches.any(1))
    np.testing.assert_array_equal(rec["prim_id"][at_start], touches.argmax(1)[at_start])
    assert (rec["axis"][at_start] == NONE).all() and not rec["normal"][at_start].any()
    assert (rec["axis"][~at_start & (rec["prim_id"] != st.PRIM_MISS)] < 26).all()


# -- hand-worked cases --------------------------------------------------------------------------------------------------------
def _one(scene, v0, v1, v2, d, tmax=INF):
    r = st.brute_force(scene, st.make_sweeps([v0], [v1], [v2], [d], tmax)).view(T.TRIANGLE_SWEEP_HIT)[0, 0]
    return float(r["t"]), int(r["axis"]), int(r["prim_id"]), r["normal"].tolist()


def test_statement_on_hand_worked_cases():
    s3, s2 = 1 / np.sqrt(3), 1 / np.sqrt(2)
    # a vertex onto a face: the scene's triangle in the plane z = x + y, nS = (-1, -1, 1); the query's lowest vertex (0.25, 0.25, 1.5)
    # falls onto the plane's point at z = 0.5: dot(nS, a_k) = -1 for every k, hi = -1 - 0, w = dot(nS, d) = -1, enter = 1.  The z axis
    # enters at (1 - 1.5) / -1 = 0.5 only.
    tilted = ca.triangles_scene([[[0, 0, 0], [1, 0, 1], [0, 1, 1]]])
    t, axis, prim, normal = _one(tilted, (0.25, 0.25, 1.5), (0.5, 0.25, 3), (0.25, 0.5, 3), (0, 0, -1))
    assert (t, axis, prim) == (1.0, 3, 0) and np.allclose(normal, [-s3, -s3, s3], atol=1e-7)
    # an edge onto an edge: the query's edge along y at x = 0, z = 1 falls onto the scene's edge (-1, 0, -0.5) .. (1, 0, 0.5) and meets it
    # at the origin at t = 1; L = cross(u1, f1) = (0, 2, 0) x (2, 0, 1) = (2, 0, -4) is axis 5
    crossing = ca.triangles_scene([[[-1, 0, -0.5], [1, 0, 0.5], [0, -2, -2]]])
    t, axis, prim, normal = _one(crossing, (0, -1, 1), (0, 1, 1), (1, 0, 4), (0, 0, -1))
    assert (t, axis, prim) == (1.0, 5, 0) and np.allclose(normal, np.array([-2, 0, 4]) / np.sqrt(20), atol=1e-7)
    # a tie resolved by the axis' number: onto the unit triangle in z = 0 the z axis (2), nS (3) enter together at t = 1
    unit = ca.triangles_scene([ca.UNIT])
    t, axis, prim, normal = _one(unit, (0.25, 0.25, 1), (0.5, 0.25, 2), (0.25, 0.5, 2), (0, 0, -1))
    assert (t, axis, prim, normal) == (1.0, 2, 0, [0.0, 0.0, 1.0])
    assert _one(unit, (0.25, 0.25, 1), (0.5, 0.25, 2), (0.25, 0.5, 2), (0, 0, -1), tmax=1.0)[2] == st.PRIM_MISS, "t < tmax, strictly"
    assert _one(unit, (0.25, 0.25, 1), (0.5, 0.25, 2), (0.25, 0.5, 2), (0, 0, 1))[2] == st.PRIM_MISS, "moving away"
    # a start in contact: the query stands across the unit triangle
    assert _one(unit, (0.25, 0.25, -1), (0.25, 0.25, 1), (3, 3, 1), (1, 2, 3)) == (0.0, NONE, 0, [0.0, 0.0, 0.0])
    # a coplanar slide in z = 0: the query's vertex (2, 2) moves by (-1, -1) onto the edge x + y = 2.5 of the plane scene's first
    # triangle, alone, and meets it at t = 0.75.  cross(nS, f3) = (-5.625, -5.625, 0) is axis 19: lo = 8.4375, w = 11.25; cross(nQ, f3)
    # (25) = (-1.3125, -1.3125, 0) ties at 1.96875 / 2.625; nS, nQ and the nine edge pairs have w == 0, and no edge of the query is
    # parallel to that edge, so none of 14 - 16 enters as late.
    plane = ca.triangles_scene([[[0, 0, 0], [2, 0.5, 0], [0.5, 2, 0]]])
    t, axis, prim, normal = _one(plane, (2, 2, 0), (3, 2.25, 0), (2.5, 3, 0), (-1, -1, 0))
    assert (t, axis, prim) == (0.75, 19, 0) and np.allclose(normal, [s2, s2, 0], atol=1e-7)
    # a segment past a corner: the segment (-2, 0.5) .. (1, -1.5) on 2 x + 3 y = -2.5 moves by (1, 1) and its middle meets the corner
    # (0, 0) at t = 2.5 / 5.  nQ is zero, so are 14 - 16 and 23 - 25; cross(nS, u2) = (7.5, 11.25, 0) is axis 21 (22 is the same vector):
    # lo = 9.375, w = 18.75.  No edge of the triangle is parallel to the segment, so none of 17 - 19 enters as late.
    t, axis, prim, normal = _one(plane, (-2, 0.5, 0), (-2, 0.5, 0), (1, -1.5, 0), (1, 1, 0))
    assert (t, axis, prim) == (0.5, 21, 0) and np.allclose(normal, np.array([-2, -3, 0]) / np.sqrt(13), atol=1e-7)
    # a sphere from outside (a vertex reaches it at t = 2), from inside (the vertex (0.5, 0, 0) reaches the surface at x = 2 at
    # t = 1.5) and touching at the start
    ball = ca.triangles_scene([[[50, 50, 50], [51, 50, 50], [50, 51, 50]]], spheres=[((0, 0, 0), 1.0, 4)])
    assert _one(ball, (0, 0, 3), (0.5, 0, 4), (0, 0.5, 4), (0, 0, -1)) == (2.0, st.AXIS_SPHERE, st.SPHERE_FLAG, [0.0, 0.0, 1.0])
    wide = ca.triangles_scene([[[50, 50, 50], [51, 50, 50], [50, 51, 50]]], spheres=[((0, 0, 0), 2.0, 4)])
    assert _one(wide, (0, 0, 0), (0.5, 0, 0), (0, 0.5, 0), (1, 0, 0)) == (1.5, st.AXIS_SPHERE, st.SPHERE_FLAG, [-1.0, 0.0, 0.0])
    assert _one(wide, (0, 0, 0), (3, 0, 0), (0, 3, 0), (1, 0, 0)) == (0.0, NONE, st.SPHERE_FLAG, [0.0, 0.0, 0.0])
    # invalid queries are misses that carry tmax as given
    for v0, d, tmax in (((np.nan, 0, 1), (0, 0, -1), 3.0), ((0.25, 0.25, 1), (0, 0, 0), 3.0), ((0.25, 0.25, 1), (0, np.inf, -1), 3.0), ((0.25, 0.25, 1), (0, 0, -1), -1.0)):
        assert _one(unit, v0, (0.5, 0.25, 2), (0.25, 0.5, 2), d, tmax) == (tmax, NONE, st.PRIM_MISS, [0.0, 0.0, 0.0])


def test_which_form_of_a_segment_meets_a_sphere():
    """The fourth limit of rt_hip.h "Triangle sweeps": the segment (-1, 0, 3) .. (1, 0, 3) falls onto the unit ball and its middle
    meets it at t = 2.  Given as v2 == v1 or as v2 == v0 it does; given as v1 == v0 the closest-point statement divides 0 by 0, near2
    is a NaN and the sphere is not met.  Over drawn segments and centres only that form ever has a NaN near2."""
    ball = ca.triangles_scene([[[50, 50, 50], [51, 50, 50], [50, 51, 50]]], spheres=[((0, 0, 0), 1.0, 4)])
    a, b, d = (-1, 0, 3), (1, 0, 3), (0, 0, -1)
    hit = (2.0, st.AXIS_SPHERE, st.SPHERE_FLAG, [0.0, 0.0, 1.0])
    assert _one(ball, a, b, b, d) == hit and _one(ball, a, b, a, d) == hit
    assert _one(ball, a, a, b, d)[2] == st.PRIM_MISS
    t, axis, prim, _ = _one(ball, a, a, a, (1, 0, -3))  # a point moving at the centre: the closest point is q0 itself
    assert abs(t - (1 - 1 / np.sqrt(10))) < 1e-6 and (axis, prim) == (st.AXIS_SPHERE, st.SPHERE_FLAG)
    rng = np.random.default_rng(1)
    p, q, o = (rng.normal(size=(4000, 3)).astype(F32) * s for s in (1, 1, 2))
    nans = {name: int(np.isnan(st._closest_elementwise(q0, q1 - q0, q2 - q0, o)[0]).sum())
            for name, (q0, q1, q2) in {"v1 == v0": (p, p, q), "v2 == v1": (p, q, q), "v2 == v0": (p, q, p), "point": (p, p, p)}.items()}
    print(nans)
    assert nans["v1 == v0"] > 1000 and nans["v2 == v1"] == nans["v2 == v0"] == nans["point"] == 0


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_triangle_sweeps_and_split_triangle_sweep_hits(rt_api):
    v = np.arange(18, dtype=np.float64).reshape(3, 2, 3)
    sw = rt_api.make_triangle_sweeps(v[0], v[1], v[2], np.array([[0, 0, 1], [0, 1, 0]], np.float64))
    assert sw.dtype == np.float32 and sw.shape == (2, 16) and sw.flags.c_contiguous
    assert sw.tobytes() == st.make_sweeps(v[0], v[1], v[2], [[0, 0, 1], [0, 1, 0]]).tobytes()
    np.testing.assert_array_equal(sw[:, 0:12], rt_api.make_triangles(v[0], v[1], v[2]))
    rec = rt_api.make_triangle_sweeps(v[0], v[1], v[2], np.ones((2, 3)), tmax=np.array([1.0, 3.0])).view(T.TRIANGLE_SWEEP).reshape(-1)
    assert rec["v1"].tolist() == v[1].tolist() and rec["tmax"].tolist() == [1.0, 3.0] and rec["direction"].tolist() == [[1, 1, 1]] * 2
    rec = np.zeros(2, T.TRIANGLE_SWEEP_HIT)
    rec["normal"], rec["t"], rec["axis"] = [[0, 0, 1], [0, 0, 0]], [0.5, 7], [21, NONE]
    rec["prim_id"], rec["material_id"] = [0x80000001, 0xFFFFFFFF], [3, 0]
    normal, t, axis, prim, mat = rt_api.split_triangle_sweep_hits(rec.view(np.float32).reshape(2, 8))
    assert prim.dtype == np.uint32 and prim.tolist() == [0x80000001, 0xFFFFFFFF] and mat.tolist() == [3, 0] and axis.tolist() == [21, NONE]
    np.testing.assert_array_equal(normal, rec["normal"])
    assert t.tolist() == [0.5, 7]


def test_make_triangle_sweeps_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    sw = rt_api.make_triangle_sweeps(torch.tensor([[1.0, 2, 3]]), [[4, 5, 6]], torch.tensor([[7.0, 8, 9]]), torch.tensor([[0.0, 0, -1]]), tmax=2.0)
    assert sw.dtype == torch.float32 and sw.tolist() == [[1, 2, 3, 0, 4, 5, 6, 0, 7, 8, 9, 0, 0, 0, -1, 2]]
    rec = np.zeros(1, T.TRIANGLE_SWEEP_HIT)
    rec["axis"], rec["prim_id"], rec["material_id"] = NONE, 0xFFFFFFFF, 7
    axis, prim, mat = rt_api.split_triangle_sweep_hits(torch.from_numpy(rec.view(np.float32).reshape(1, 8).copy()))[2:]
    assert prim.dtype == torch.int64 and prim.tolist() == [0xFFFFFFFF] and mat.tolist() == [7] and axis.tolist() == [NONE]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.sweep_triangle
    good = np.zeros((4, 16), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="sweeps: shape"):
        call(nc, np.zeros((4, 12), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 16), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 16])
    with pytest.raises(ValueError, match="rows for 4 sweeps"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 16), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 8), np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_sweep_triangle(self, h, sweeps, n, out, flags):
        self.calls.append((sweeps.value, n.value, out.value, flags.value))
        return 0


def test_sweep_triangle_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    sweeps = rt_api.make_triangle_sweeps(np.zeros((6, 3), np.float32), np.ones((6, 3), np.float32), np.ones((6, 3), np.float32), np.ones((6, 3), np.float32))
    got = ctx.sweep_triangle(sweeps)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.sweep_triangle(sweeps, out=own, counters=True) is own
    assert ctx.lib.calls == [(sweeps.ctypes.data, 6, got.ctypes.data, 0), (sweeps.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS)]
