"""Triangle contacts (rt_contact_triangle) without a GPU: the symbol and the structs against the header; the statement, the list and
the whole walk on the host - csrc/contact_triangle_rules.h, the statements the kernel calls - held to a brute-force sort under
AddressSanitizer + UBSan (tests/check_contact_triangle.cpp); the numpy float32 statement the GPU tests compare bytes with
(tests/contact_triangle_cases.py) against the C++ one bit for bit, against the same statement in float64, and the float64 statement
against hand-worked cases, six segment - triangle distances and the capsule statement; and what Context.contact_triangle validates
before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import contact_capsule_cases as kc
import contact_triangle_cases as kt
import overlap_triangle_cases as otc
import stack_cases as sk
import sweep_capsule_cases as scs
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
F64 = np.float64
INF, NAN = np.inf, np.nan
MISS = cc.PRIM_MISS


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_contact_triangle" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_contact_triangle")
    assert re.search(r"int rt_contact_triangle\(rt_ctx\* ctx, const rt_triangle_contact_query\* triangles, size_t n, uint32_t max_contacts,\s*"
                     r"rt_triangle_contact\* out,\s*uint32_t\* counts,\s*uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_overlap_triangle, rt_sweep_triangle, rt_contact_triangle,[^.]*\.\s+A call rejected for its arguments "
                     r"changes nothing", _header(), re.S), "listed among the calls a running image survives"
    assert _header().index("Triangle sweeps:") < _header().index("Triangle contacts:") < _header().index("Geometry updates:")
    assert re.search(r"#define RT_QUERY_COUNT_ALL 2u[^\n]*rt_contact_triangle", _header()) and re.search(r"#define RT_CONTACT_ANY 4u[^\n]*rt_contact_triangle", _header())
    flat = re.sub(r"\s*\n \*\s+", " ", _header())
    assert "the penetration depth of an intersecting pair is out of scope here" in flat and "depth = margin - distance" in flat
    assert rt_api.CONTACT_MAX == kt.CONTACT_MAX == 16


def test_struct_layouts_agree_with_the_dtypes(tmp_path):
    q_fields, r_fields = ("v0", "margin", "v1", "_pad1", "v2", "_pad2"), ("position", "distance", "qu", "qv", "prim_id", "material_id")
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%zu", sizeof(rt_triangle_contact_query));'
           + "".join(f'printf(" %zu", offsetof(rt_triangle_contact_query, {f}));' for f in q_fields)
           + 'printf("\\n%zu", sizeof(rt_triangle_contact));' + "".join(f'printf(" %zu", offsetof(rt_triangle_contact, {f}));' for f in r_fields)
           + 'printf("\\n");return 0;}\n')
    for lang, compiler in (("c", "gcc"), ("c++", "g++")):
        exe = str(tmp_path / ("probe_" + compiler))
        subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
        query, rec = (list(map(int, line.split())) for line in subprocess.check_output([exe]).decode().splitlines())
        assert query == [T.TRIANGLE_CONTACT_QUERY.itemsize] + [T.TRIANGLE_CONTACT_QUERY.fields[f][1] for f in q_fields] == [48, 0, 12, 16, 28, 32, 44]
        assert rec == [T.TRIANGLE_CONTACT.itemsize] + [T.TRIANGLE_CONTACT.fields[f][1] for f in r_fields] == [32, 0, 12, 16, 20, 24, 28]
    assert [T.TRIANGLE_CONTACT_QUERY.fields[f][1] for f in ("v0", "v1", "v2")] == [T.TRIANGLE_QUERY.fields[f][1] for f in ("v0", "v1", "v2")]
    assert T.TRIANGLE_CONTACT_QUERY.fields["margin"][1] == T.POINT_QUERY.fields["radius"][1] == T.CAPSULE.fields["radius"][1]
    assert [T.TRIANGLE_CONTACT.fields[f][1] for f in ("position", "distance", "qu", "qv", "prim_id", "material_id")] == \
           [T.NEAREST.fields[f][1] for f in ("position", "distance", "u", "v", "prim_id", "material_id")]
    assert T.EXPECTED_SIZES["TRIANGLE_CONTACT_QUERY"] == 48 and T.EXPECTED_SIZES["TRIANGLE_CONTACT"] == 32


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    tris, out, counts = (C.c_float * 12)(), (C.c_float * 32)(), (C.c_uint32 * 1)()
    assert lib.rt_contact_triangle(C.c_void_p(0), tris, C.c_size_t(1), C.c_uint32(4), out, counts, C.c_uint32(0)) == -1
    assert lib.rt_contact_triangle(C.c_void_p(0), None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_uint32(0)) == -1
    assert not any(bytes(out)) and not any(bytes(counts))


def test_both_entries_are_one_call_of_contact_query():
    """The argument checks and the batch are written once, in rt_query.cpp; each entry names contact_query once."""
    host, unit = open(os.path.join(CSRC, "rt_query.cpp")).read(), open(os.path.join(CSRC, "rt_mesh_query.cpp")).read()
    assert host.count("int contact_query(rt_ctx* ctx, ") == 1 and host.count("contact_query(ctx, ") == 1 and unit.count("contact_query(ctx, ") == 1
    assert re.search(r'int rt_contact_capsule\([^)]*\) \{\s*return contact_query\(ctx, "rt_contact_capsule", "capsules", [^;]*;\s*\}', host)
    assert re.search(r'int rt_contact_triangle\([^)]*\) \{\s*return contact_query\(ctx, "rt_contact_triangle", "triangles", [^;]*;\s*\}', unit)
    assert "contact_triangle.hip" in open(os.path.join(ROOT, "gpu_raytracer_amd", "build.py")).read()


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *extra):
    run = subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread", *extra,
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_contact_triangle.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("ct") / "check_contact_triangle")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every record and count of the walk - statement, list, node bound, order and stack as the kernel runs them - is the brute-force
    sort's at K = 1, 4 and 16, with and without COUNT_ALL, and in ANY mode; a point gives cp_walk_all's records, counts and work; the
    corner queries (a vertex bit-equal to a record's, the rest pointing away, margin 1e-18) each list the record they were built on at
    distance 0; the stack and the list stay inside the words the kernel's launch provides (the program checks every index).  As in
    check_contact_capsule.cpp, COUNT_ALL and ANY run with finite margins only and skip every second query that is neither small nor a
    corner query; the list mode runs them all.  On ordinary input at n = 20000 the small triangles make fewer than n / 10 triangle
    tests."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        per_k = re.findall(r"^K +(\d+)( COUNT_ALL)? *: 0 failed, ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)
        assert sorted((k, bool(a)) for k, a, _, _ in per_k) == sorted((k, a) for k in ("1", "4", "16") for a in (False, True)), run.stdout[-1500:]
        assert re.search(r"^ANY +: 0 failed", run.stdout, re.M), run.stdout[-1500:]
        point = re.search(r"^points +: 0 failed over (\d+) queries", run.stdout, re.M)
        assert point and int(point.group(1)) >= 20, run.stdout[-1500:]
        corner = re.search(r"^corner queries: (\d+) of (\d+) list their record at distance 0", run.stdout, re.M)
        assert corner and int(corner.group(1)) == int(corner.group(2)) and (int(corner.group(2)) >= 24 or n < 300), run.stdout[-1500:]  # n < 300: NaN vertices can leave no record
        small = re.search(r"^small triangles: ([0-9.]+) node visits and ([0-9.]+) triangle tests per query over (\d+) queries", run.stdout, re.M)
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            print(f"kind {kind} method {method}: the small triangles make {small.group(2)} triangle tests per query (brute force 20000)")
            assert int(small.group(3)) >= 24 and float(small.group(2)) < 20000 / 10, run.stdout[-1500:]


def test_the_check_can_fail(tmp_path):
    """The same program with a negative margin on the node bound reports wrong answers: boxes that hold a listed primitive are culled."""
    exe = _build_checker(tmp_path / "check_negative_slack", "-DRT_CP_SLACK=-1.0e-5f")
    run = subprocess.run([exe, "300", "1", "0", "0"], capture_output=True, text=True)
    assert run.returncode == 1 and re.search(r" [1-9]\d* failures$", run.stdout.strip()), run.stdout[-1500:]
    corner = re.search(r"^corner queries: (\d+) of (\d+) list", run.stdout, re.M)
    assert corner and int(corner.group(1)) == int(corner.group(2)), "the brute force still holds every corner's record: it is the walk that loses them"
    assert re.search(r"^FAIL: query \d+ [^\n]*margin 1\.0+\d*e-18\)", run.stdout, re.M), "and corner queries are among the walk's wrong answers"


def test_numpy_and_the_header_agree_bit_for_bit(checker, tmp_path):
    """The statement alone, through the checker's `eval` mode: soup pairs in range and at random, the queries as they are, as segments
    (v2 == v1, v1 == v0) and as points; the three spheres with queries around, across and inside them."""
    scene = kt.soup()
    tris, d2, _, _ = kt.soup_reference()
    rng = np.random.default_rng(0)
    v0, e1, e2, _ = kt.records(scene)
    n = 20000
    near = np.argwhere(kt.in_range(tris, d2)[:, len(scene.spheres):])
    near = near[rng.integers(0, len(near), n)]
    qi, ti = np.concatenate([rng.integers(0, len(tris), n), near[:, 0]]), np.concatenate([rng.integers(0, len(v0), n), near[:, 1]])
    q = np.array(tris[qi])
    m = np.arange(len(q)) % 5
    q[m == 1, 8:11] = q[m == 1, 4:7]
    q[m == 2, 4:7] = q[m == 2, 8:11] = q[m == 2, 0:3]
    q[m == 3, 4:7] = q[m == 3, 0:3]
    rec = np.concatenate([v0[ti], e1[ti], e2[ti], q[:, 0:3], q[:, 4:7], q[:, 8:11]], 1).astype(F32)
    centre, radius = kt._spheres(scene, F32)
    ns = 9000
    si, qs = rng.integers(0, len(centre), ns), np.array(tris[rng.integers(0, len(tris), ns)])
    ms = np.arange(ns) % 4
    qs[ms == 1, 8:11] = qs[ms == 1, 4:7]
    qs[ms == 2, 4:7] = qs[ms == 2, 8:11] = qs[ms == 2, 0:3]
    qs[ms == 3, 4:7] = qs[ms == 3, 0:3]
    shift = ((centre[si] + rng.normal(size=(ns, 3)) * radius[si, None] * 0.8) - qs[:, 0:3]).astype(F32)
    for c in (0, 4, 8):
        qs[:, c:c + 3] += shift
    srec = np.concatenate([centre[si], radius[si, None], np.full((ns, 2), NAN, F32), np.zeros((ns, 3), F32), qs[:, 0:3], qs[:, 4:7], qs[:, 8:11]], 1).astype(F32)
    np.concatenate([rec, srec]).tofile(str(tmp_path / "in.bin"))
    subprocess.run([checker, "eval", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    got = np.fromfile(str(tmp_path / "out.bin"), F32).reshape(-1, 5)
    want = np.stack(kt.tri_tri(*(rec[:, c:c + 3] for c in range(0, 18, 3))), 1)
    assert (want[:, 0] == 0).sum() > 500 and (want[:, 0] > 0).sum() > 10000
    np.testing.assert_array_equal(got[:len(rec)].view(np.uint32), want.view(np.uint32))
    swant = np.stack(kt.sphere_candidates(srec[:, 0:3], srec[:, 3], srec[:, 9:12], srec[:, 12:15], srec[:, 15:18]), 1)
    assert (swant[:, 0] == 0).sum() > 500 and not np.isnan(swant).any()
    np.testing.assert_array_equal(got[len(rec):, :3].view(np.uint32), swant.view(np.uint32))


# -- the float64 statement on hand-worked cases -------------------------------------------------------------------------------
S = [np.array(x, F64) for x in ([0, 0, 0], [4, 0, 0], [0, 4, 0])]  # the scene triangle (0, 0, 0), (4, 0, 0), (0, 4, 0) as v0, e1, e2


def _pair(q0, q1, q2, dtype=F64):
    return [float(x) for x in kt.tri_tri(*(np.array(a, dtype) for a in (*S, q0, q1, q2)))]


def test_hand_worked_triangle_pairs():
    assert _pair((1, 1, .5), (2, 1, .5), (1, 2, .5)) == [0.25, 0, 0, 0.25, 0.25], "parallel at height 0.5: the first vertex, ties never replace"
    assert _pair((1, 1, .25), (2, 1, 1), (1, 2, 1)) == [0.0625, 0, 0, 0.25, 0.25], "a vertex over the face"
    assert _pair((2, 1, 1), (1, 1, .25), (1, 2, 1)) == [0.0625, 1, 0, 0.25, 0.25], "... the second vertex"
    assert _pair((2, -1, -1), (2, -1, 1), (2, -3, 0)) == [1, 0.5, 0, 0.5, 0], "two skew edges: the middle of each"
    assert _pair((1, 1, -1), (1, 1, 1), (5, 5, 1)) == [0, 0.5, 0, 0.25, 0.25], "an edge of the query pierces the scene triangle"
    assert _pair((-10, -10, -1), (20, -10, -1), (-10, 20, 2))[0] == 0, "an edge of the scene triangle pierces the query"
    assert _pair((1, -1, 0), (1, 4, 0), (1.5, 4, 0)) == [0, 0.2, 0, 0.25, 0], "coplanar, no vertex contained: the first pair of crossing edges"
    assert _pair((1, 1, 0), (2, 1, 0), (1, 2, 0)) == [0, 0, 0, 0.25, 0.25], "coplanar, the query nested in the scene triangle"
    d2, qu, qv, v, w = _pair((-10, -10, 0), (20, -10, 0), (-10, 20, 0))
    assert (d2, v, w) == (0, 0, 0) and abs(qu - 1 / 3) < 1e-15 and abs(qv - 1 / 3) < 1e-15, "coplanar, the scene triangle nested in the query"
    assert _pair((5, 0, 0), (6, 0, 0), (5, 1, 0)) == [1, 0, 0, 1, 0], "coplanar apart"
    assert _pair((1, 1, .5), (1, 1, .5), (1, 1, .5)) == [0.25, 0, 0, 0.25, 0.25], "a point"
    assert _pair((2, -1, -1), (2, -1, 1), (2, -1, 1)) == [1, 0.5, 0, 0.5, 0], "a segment given as v2 == v1"
    assert _pair((1, 1, .5), (2, 1, .5), (1, 2, .5), F32) == [0.25, 0, 0, 0.25, 0.25]
    nan_scene = kt.tri_tri(np.array([NAN, 0, 0]), S[1], S[2], *(np.array(a, F64) for a in ((1, 1, .5), (2, 1, .5), (1, 2, .5))))[0]
    assert np.isnan(nan_scene), "a degenerate scene triangle is never listed"


def _ball(q0, q1, q2, r=2.0, dtype=F64):
    q = [np.array(a, dtype) for a in (q0, q1, q2)]
    d2, qu, qv = kt.sphere_candidates(np.zeros(3, dtype), dtype(r), *q)
    pos = kt.sphere_position(np.zeros(3, dtype), dtype(r), *q, qu, qv)
    return float(d2), float(qu), float(qv), pos


def test_hand_worked_sphere_cases():
    d2, qu, qv, pos = _ball((3, -1, -1), (3, 1, -1), (3, 0, 1))
    assert (d2, qu, qv) == (1, 0.25, 0.5) and pos.tolist() == [2, 0, 0], "outside: the query's point nearest the centre"
    d2, qu, qv, pos = _ball((.5, 0, 0), (1, 0, 0), (.5, .5, 0))
    assert (d2, qu, qv) == (1, 1, 0) and pos.tolist() == [2, 0, 0], "wholly inside: the farthest vertex"
    d2, qu, qv, pos = _ball((.5, 0, 0), (-.5, 0, 0), (0, .25, 0))
    assert (d2, qu, qv) == (2.25, 0, 0), "... the lowest vertex on a tie"
    d2, qu, qv, pos = _ball((1, 0, 0), (4, 0, 0), (1, 1, 0))
    assert d2 == 0 and abs(qu - 1 / 3) < 1e-15 and qv == 0 and np.abs(pos - [2, 0, 0]).max() < 1e-15, "crossing: between the nearest point and the farthest vertex"
    d2, qu, qv, pos = _ball((0, 2, 0), (0, 2, 0), (0, 2, 0))
    assert (d2, qu, qv) == (0, 0, 0) and pos.tolist() == [0, 2, 0], "a point on the surface"
    assert np.isnan(_ball((3, -1, -1), (3, 1, -1), (3, 0, 1), NAN)[0])
    # a segment, however it is given (v2 == v1, v1 == v0, v2 == v0): the centre's foot is its middle, 1 from the centre
    forms = (((-3, 1, 0), (3, 1, 0), (3, 1, 0)), ((-3, 1, 0), (-3, 1, 0), (3, 1, 0)), ((-3, 1, 0), (3, 1, 0), (-3, 1, 0)))
    for r, want in ((0.5, 0.25), (1.0, 0.0)):  # outside; touching, which is the crossing case at its nearest point
        given = [_ball(*q, r=r) for q in forms]
        assert [g[0] for g in given] == [want] * 3 and [g[1:3] for g in given] == [(0.5, 0), (0, 0.5), (0.5, 0)], (r, given)
        assert all(np.abs(g[3] - [0, r, 0]).max() < 1e-15 for g in given)
    given = [_ball(*q, r=5.0) for q in forms]  # wholly inside: both ends sqrt(10) from the centre, the lowest vertex on the tie
    assert all(abs(g[0] - (5 - np.sqrt(10)) ** 2) < 1e-14 and g[1:3] == (0, 0) for g in given), given
    given = [_ball(*q, r=1.5) for q in forms]  # crossing: the segment leaves the ball on its way from the middle to the first end
    assert all(g[0] == 0 and abs(np.linalg.norm(g[3]) - 1.5) < 1e-15 and abs(g[3][1] - 1) < 1e-15 and g[3][0] < 0 for g in given), given
    assert _ball((3, -1, -1), (3, 1, -1), (3, 0, 1), dtype=F32)[:3] == (1, 0.25, 0.5)


def test_records_and_the_push_out_on_a_small_scene():
    scene = ca.triangles_scene([[[0, 0, 0], [4, 0, 0], [0, 4, 0]]], spheres=[((0, 0, -5), 2.0, 3)])
    q = kt.make_contact_triangles([(1, 1, .5)], [(2, 1, .75)], [(1, 2, .75)], 1.0)
    recs, listed, total = kt.contacts_all(scene, q, 4)
    r = recs[0].view(T.TRIANGLE_CONTACT).reshape(-1)
    assert (int(listed[0]), int(total[0])) == (1, 1) and r["prim_id"].tolist() == [0, MISS, MISS, MISS]
    assert r["distance"][0] == F32(0.5) and r["qu"][0] == 0 and r["qv"][0] == 0 and r["position"][0].tolist() == [1, 1, 0]
    assert r["distance"][1:].tolist() == [1.0] * 3 and not r["position"][1:].any() and not r["material_id"][1:].any(), "unused slots: cp_answer_miss(margin)"
    v0, v1, v2 = (q[0, c:c + 3] for c in (0, 4, 8))
    normal = ((v0 + (v1 - v0) * r["qu"][0] + (v2 - v0) * r["qv"][0]) - r["position"][0]) / r["distance"][0]
    assert normal.tolist() == [0, 0, 1] and q[0, 3] - r["distance"][0] == 0.5, "the push-out of the header"
    assert kt.contacts_all(scene, kt.with_margin(q, 0.5), 4)[2][0] == 0, "dist2 < margin * margin, strictly"
    assert kt.contacts_all(scene, kt.with_margin(q, np.nextafter(F32(0.5), F32(1))), 4)[2][0] == 1
    wide = kt.contacts_all(scene, kt.with_margin(q, INF), 4)
    assert wide[2][0] == 2 and np.ascontiguousarray(wide[0][0, :2, 6]).view(np.uint32).tolist() == [0, cc.SPHERE_FLAG] and wide[0][0, 1, 7].view(np.uint32) == 3
    for bad in (kt.with_margin(q, NAN), kt.with_margin(q, 0), kt.with_margin(q, -1), kt.make_contact_triangles([(NAN, 1, .5)], [(2, 1, .75)], [(1, 2, .75)], 1.0),
                kt.make_contact_triangles([(1, 1, .5)], [(2, INF, .75)], [(1, 2, .75)], 1.0)):
        recs, listed, total = kt.contacts_all(scene, bad, 2)
        assert not kt.valid(bad).any() and (int(listed[0]), int(total[0])) == (0, 0) and (np.ascontiguousarray(recs[..., 6]).view(np.uint32) == MISS).all()
        assert recs[0, :, 3].tobytes() == np.full(2, bad[0, 3], F32).tobytes(), "the margin as given"


def test_a_point_is_the_nearest_k_statement():
    soup = scenes.random_soup(300, n_spheres=3)
    points = cc.four_kinds(soup, 128, 5)
    radius = np.where(np.arange(128) % 2 == 0, 0.4, INF).astype(F32)
    want, want_listed, want_total = ca.nearest_all(soup, np.concatenate([points, radius[:, None]], 1), 8)
    got, listed, total = kt.contacts_all(soup, kt.make_contact_triangles(points, points, points, radius), 8)
    assert got[..., [0, 1, 2, 3, 6, 7]].tobytes() == want[..., [0, 1, 2, 3, 6, 7]].tobytes() and not got[..., 4:6].any()
    assert listed.tobytes() == want_listed.tobytes() and total.tobytes() == want_total.tobytes() and (total > 8).any()


# -- the float64 statement against independent ones ---------------------------------------------------------------------------
SCENES = {"soup": kt.soup, "cornell12": scenes.cornell12}


@pytest.fixture(scope="module")
def both():
    cache = {}

    def get(name):
        if name not in cache:
            scene = SCENES[name]()
            tris = kt.soup_reference()[0] if name == "soup" else kt.soup_triangles_with_margins(scene, 2048, 11)
            d32 = kt.soup_reference()[1] if name == "soup" else kt.pair_dist2(scene, tris)
            cache[name] = (scene, tris, d32, kt.pair_dist2(scene, tris, F64))
        return cache[name]
    return get


def test_f64_is_the_least_of_six_segment_triangle_distances(both):
    """Independently of rules a - d: two triangles are as far apart as the nearest of the query's three edges from the scene triangle
    and the scene triangle's three edges from the query, each by the capsule statement's float64 cap_triangle.  On every soup pair
    whose boxes are within the margin, to 1e-12 of the diagonal."""
    scene, tris, _, d64 = both("soup")
    v0, e1, e2, _ = kt.records(scene, F64)
    n_sph = len(scene.spheres)
    q = [a for a in kt._vertices(tris, F64)]
    qlo, qhi = np.minimum(np.minimum(q[0], q[1]), q[2]), np.maximum(np.maximum(q[0], q[1]), q[2])
    s = [v0, v0 + e1, v0 + e2]
    slo, shi = np.minimum(np.minimum(s[0], s[1]), s[2]), np.maximum(np.maximum(s[0], s[1]), s[2])
    gap = np.maximum(np.maximum(slo[None] - qhi[:, None], qlo[:, None] - shi[None]), 0)
    rows, cols = np.nonzero((gap * gap).sum(2) < (tris[:, 3].astype(F64) ** 2)[:, None])
    assert len(rows) > 20000
    least = np.full(len(rows), INF)
    u1, u2 = q[1][rows] - q[0][rows], q[2][rows] - q[0][rows]
    for P, ax in ((q[0][rows], u1), (q[0][rows], u2), (q[1][rows], u2 - u1)):
        least = np.minimum(least, scs.cap_triangle(v0[cols], e1[cols], e2[cols], P, ax)[0])
    for P, ax in ((s[0][cols], e1[cols]), (s[0][cols], e2[cols]), (s[1][cols], e2[cols] - e1[cols])):
        least = np.minimum(least, scs.cap_triangle(q[0][rows], u1, u2, P, ax)[0])
    diff = np.abs(np.sqrt(d64[rows, n_sph + cols]) - np.sqrt(least))
    print(f"{len(rows)} pairs, {(least == 0).sum()} intersecting; the largest difference is {diff.max():.3g} ({diff.max() / kt.diagonal(scene):.3g} diagonals)")
    assert (least == 0).sum() > 1000 and diff.max() <= 1e-12 * kt.diagonal(scene)


def test_f64_segments_are_the_capsule_statement(both):
    """The soup queries as segments v0 .. v1 (given as v2 == v1): the float64 distances are the capsule statement's for the axis
    v1 - v0, triangles and spheres, to 1e-12 of the diagonal."""
    scene, tris, _, _ = both("soup")
    seg = np.array(tris[:256])
    seg[:, 8:11] = seg[:, 4:7]
    d64 = kt.pair_dist2(scene, seg, F64)
    v0, e1, e2, _ = kt.records(scene, F64)
    centre, radius = kt._spheres(scene, F64)
    A, B, _ = kt._vertices(seg, F64)
    want = np.concatenate([kc.sphere_candidates(centre[None], radius[None], A[:, None], (B - A)[:, None])[0],
                           scs.cap_triangle(v0[None], e1[None], e2[None], A[:, None], (B - A)[:, None])[0]], 1)
    diff = np.abs(np.sqrt(d64) - np.sqrt(want))
    print(f"segments: the largest difference is {diff.max():.3g}; {(want == 0).sum()} pairs at distance 0")
    assert (want == 0).sum() > 10 and diff.max() <= 1e-12 * kt.diagonal(scene)


# -- the float32 statement against the float64 one ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_f32_distances_lie_within_k_diagonals_of_f64(both, name):
    """Every listed distance (K = CONTACT_MAX) of soup_triangles_with_margins(scene, 2048, 11) lies within K_MEASURED x the scene's
    diagonal of the float64 statement's distance for the same primitive, and K_MEASURED is the smallest k of the grid that holds: the
    next smaller one is violated.  Measured: soup 2.17e-7 at most (2.74e-8 diagonals), cornell12 2.17e-7 (6.27e-8 diagonals)."""
    scene, tris, d32, d64 = both(name)
    recs, _, total = kt.contacts_all(scene, tris, kt.CONTACT_MAX, d32)
    col = kt.columns(scene, recs)
    listed = col >= 0
    assert listed.sum() > 1000 and (listed.sum(1) == np.minimum(total, kt.CONTACT_MAX)).all()
    want = np.sqrt(d64[np.arange(len(tris))[:, None], np.where(listed, col, 0)])
    diff = np.abs(recs[..., 3].astype(F64) - want)[listed] / kt.diagonal(scene)
    k = kt.K_MEASURED[name]
    grid = sorted(m * 10.0 ** e for m in (1, 1.5, 2, 3, 5, 7) for e in range(-12, -3))
    below = max(g for g in grid if g < k * (1 - 1e-9))
    print(f"{name}: the largest |distance32 - distance64| is {diff.max():.3g} diagonals over {listed.sum()} listed contacts; K_MEASURED {k:g}")
    assert below < diff.max() <= k, "K_MEASURED is the smallest k of the grid that holds"


def test_f32_membership_agrees_with_f64_away_from_zero_margin(both):
    """The soup batch: every pair whose float64 |distance - margin| exceeds 1e-5 agrees; the pairs left out are at most 1e-4 of all
    pairs and the queries with a pair left out at most 5 %.  Measured on the CPU: 1 of 6,150,144 pairs left out (1.6e-7), 1 of 2048
    queries (0.05 %), and no disagreement even among the pairs left out."""
    scene, tris, d32, d64 = both("soup")
    with np.errstate(all="ignore"):
        margin = np.sqrt(d64) - tris[:, 3].astype(F64)[:, None]
    f32, f64 = kt.in_range(tris, d32), margin < 0
    left_out = np.abs(margin) <= 1e-5
    print(f"{left_out.sum()} of {left_out.size} pairs left out ({left_out.mean():.1e}), {left_out.any(1).sum()} of {len(tris)} queries "
          f"({left_out.any(1).mean():.2%}); {(f64 != f32).sum()} disagreements in all")
    assert f32.shape == margin.shape == (2048, 3003) and f32.any() and not f32.all() and kt.valid(tris).all()
    assert (f64 == f32)[~left_out].all()
    assert left_out.mean() <= 1e-4 and left_out.any(1).mean() <= 0.05


def test_what_the_overlap_statement_lists_is_at_distance_k_touch(both):
    """Every pair rt_overlap_triangle's f32 statement lists on the soup batch has an f32 distance here of at most K_TOUCH x the
    diagonal - measured: 0 for all 8187 of them - so that with any margin above that, contact ANY >= overlap ANY."""
    scene, tris, d32, _ = both("soup")
    touch = otc.touching(scene, tris)
    d = np.sqrt(d32[touch])
    print(f"{touch.sum()} touching pairs; the largest f32 distance is {d.max():.3g}")
    assert touch.sum() > 5000 and not np.isnan(d).any() and d.max() <= kt.K_TOUCH["soup"] * kt.diagonal(scene) < 0.05


def test_the_batches_are_what_they_are_for():
    total = kt.soup_reference()[3]
    for k in (4, 16):
        short, over, none = kt.batch_condition(total, k)
        print(f"K {k}: {short:.1%} of the queries hold some but fewer than K contacts, {over:.1%} more than K, {none:.1%} none")
        assert short > 0.05 and over > 0.05 and none > 0
    walls, tris = ca.coplanar_walls(), kt.lattice_triangles()
    q0, q1, q2 = kt._vertices(tris, F32)
    recs, _, total = kt.contacts_all(walls, tris)
    d, listed = recs[..., 3], np.ascontiguousarray(recs[..., 6]).view(np.uint32) != MISS
    v0, e1, e2, _ = kt.records(walls, F64)
    normal = np.cross(e1, e2)
    h = np.stack([((q.astype(F64)[:, None] - v0[None]) * normal[None]).sum(2) for q in (q0, q1, q2)])  # (vertex, query, wall triangle)
    zero = kt.pair_dist2(walls, tris, F64)[:, len(walls.spheres):] == 0
    in_plane, pierces = zero & (h == 0).all(0), zero & (h.min(0) < 0) & (h.max(0) > 0)
    above = ~zero & (h[0] == h[1]) & (h[1] == h[2]) & (h[0] != 0)
    print(f"lattice: {in_plane.any(1).sum()} queries lie in a wall triangle's plane at distance 0, {pierces.any(1).sum()} pass through one, {above.any(1).sum()} are parallel to one")
    assert in_plane.any(1).sum() > 20 and pierces.any(1).sum() > 20 and above.any(1).sum() > 20, "in the planes without piercing, piercing, and parallel above"
    assert ((q0 == q1).all(1) & (q1 == q2).all(1)).any() and ((q1 == q2).all(1) & ~(q0 == q1).all(1)).any(), "points and segments among them"
    assert (total == 0).any() and (listed[:, 1] & (d[:, 0] == d[:, 1])).mean() > 0.5 and (listed[:, 0] & (d[:, 0] == 0)).any() and (listed[:, 0] & (d[:, 0] > 0)).any()
    deck = sk.deck_scene()
    n_cards = deck.meta["cards"]
    assert (kt.contacts_all(deck, kt.deck_triangles("corner"), 1)[2] == 0).all()
    assert (kt.contacts_all(deck, kt.deck_triangles("covered"), 1)[2] == n_cards).all()
    assert set(kt.contacts_all(deck, kt.deck_triangles("mixed"), 1)[2].tolist()) == {0, n_cards}


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.contact_triangle
    good = np.zeros((4, 12), F32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="tris: shape"):
        call(nc, np.zeros((4, 8), F32), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 12), F32)[::2], 4)
    for bad in (-1, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="max_contacts"):
            call(nc, good, bad)
    with pytest.raises(ValueError, match="count_all"):
        call(nc, good, 0)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 4, any_hit=True)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 0, any_hit=True, count_all=True)
    with pytest.raises(ValueError, match="rows for 4 tris"):
        call(nc, good, 2, out=np.zeros((3, 2, 8), F32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 3, 8), F32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="counts: 3 rows"):
        call(nc, good, 2, counts=np.zeros(3, np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_contact_triangle(self, h, tris, n, max_contacts, out, counts, flags):
        self.calls.append((tris.value, n.value, max_contacts.value, out.value, counts.value, flags.value))
        return 0


def test_contact_triangle_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    v = np.arange(54, dtype=F32).reshape(3, 6, 3)
    tris = rt_api.make_contact_triangles(v[0], v[1], v[2], 0.5)
    assert tris.shape == (6, 12) and tris.dtype == np.float32 and tris.tobytes() == kt.make_contact_triangles(v[0], v[1], v[2], 0.5).tobytes()
    per = rt_api.make_contact_triangles(v[0], v[1], v[2], np.arange(1, 7)).view(T.TRIANGLE_CONTACT_QUERY)
    assert per["margin"].ravel().tolist() == [1, 2, 3, 4, 5, 6] and per["v2"].reshape(6, 3).tolist() == v[2].tolist() and not per["_pad1"].any() and not per["_pad2"].any()
    out, counts = ctx.contact_triangle(tris, 3)
    assert out.shape == (6, 3, 8) and out.dtype == np.float32 and counts.shape == (6,) and counts.dtype == np.uint32
    own, own_counts = np.zeros((6, 16, 8), F32), np.zeros(6, np.uint32)
    got = ctx.contact_triangle(tris, np.int64(16), out=own, counts=own_counts, count_all=True, counters=True)
    assert got[0] is own and got[1] is own_counts
    none, only_counts = ctx.contact_triangle(tris, 0, out=own, count_all=True)
    assert none is None and only_counts.shape == (6,)
    none, any_counts = ctx.contact_triangle(tris, 0, any_hit=True, counters=True)
    assert none is None and any_counts.shape == (6,)
    assert ctx.lib.calls == [(tris.ctypes.data, 6, 3, out.ctypes.data, counts.ctypes.data, 0),
                             (tris.ctypes.data, 6, 16, own.ctypes.data, own_counts.ctypes.data, rt_api.QUERY_COUNTERS | rt_api.QUERY_COUNT_ALL),
                             (tris.ctypes.data, 6, 0, None, only_counts.ctypes.data, rt_api.QUERY_COUNT_ALL),
                             (tris.ctypes.data, 6, 0, None, any_counts.ctypes.data, rt_api.CONTACT_ANY | rt_api.QUERY_COUNTERS)]
    recs = np.zeros((2, 8), F32)
    recs[0] = [1, 2, 3, 0.25, 0.5, 0.125, 0, 0]
    recs.view(np.uint32)[:, 6:8] = [[7, 2], [MISS, 0]]
    pos, dist, qu, qv, prim, mat = rt_api.split_triangle_contacts(recs)
    assert pos[0].tolist() == [1, 2, 3] and dist[0] == 0.25 and qu[0] == 0.5 and qv[0] == 0.125 and prim.tolist() == [7, MISS] and mat.tolist() == [2, 0]
