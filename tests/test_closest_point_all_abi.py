"""Nearest-K queries (rt_closest_point_all) without a GPU: the symbol against the header; the list, its bound and the whole walk on the
host - csrc/closest_point_all_rules.h, the statements the kernel calls - held to a brute-force sort under AddressSanitizer + UBSan
(tests/check_closest_point_all.cpp); the numpy float32 statement the GPU tests compare bytes with (tests/closest_point_all_cases.py)
on hand-worked cases; and what Context.closest_point_all validates before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
INF = np.inf


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports --------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_closest_point_all" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_closest_point_all")
    assert re.search(r"int rt_closest_point_all\(rt_ctx\* ctx, const rt_point_query\* points, size_t n, uint32_t max_nearest,\s*rt_nearest\* out,\s*"
                     r"uint32_t\* counts,\s*uint32_t flags\);", code)
    assert re.search(r"^#define RT_NEAREST_MAX (\d+)u", _header(), re.M).group(1) == str(rt_api.NEAREST_MAX) == str(ca.NEAREST_MAX) == "16"
    assert re.search(r"It survives rt_prepare,[^.]*rt_closest_point, rt_closest_point_all,", _header(), re.S), "listed among the calls a running image survives"
    assert re.search(r"It survives rt_prepare,[^.]*rt_closest_point", _header(), re.S), "the sentence rt_closest_point's test reads still matches"
    assert "RT_QUERY_COUNT_ALL with radius = +inf tests every primitive" in re.sub(r"\s*\n \* ", " ", _header())


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    points, out, counts = (C.c_float * 4)(), (C.c_float * 32)(), (C.c_uint32 * 1)()
    assert lib.rt_closest_point_all(C.c_void_p(0), points, C.c_size_t(1), C.c_uint32(4), out, counts, C.c_uint32(0)) == -1
    assert lib.rt_closest_point_all(C.c_void_p(0), None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_uint32(0)) == -1
    assert not any(bytes(out)) and not any(bytes(counts))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cpa") / "check_closest_point_all"
    cc_run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_closest_point_all.cpp"),
                             os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc_run.returncode == 0, cc_run.stderr[-3000:]
    return str(exe)


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force_sort(checker, method, kind):
    """Every record and count of the walk - list, bound, order, stack and leaf test as the kernel runs them - has the brute-force
    sort's bytes at K = 1, 4 and 16, with and without COUNT_ALL; K = 1 has cp_walk's records, node visits and triangle tests; the stack
    and the list stay inside the words the kernel's launch provides (the program checks every index)."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        per_k = {k: (float(v), float(t)) for k, v, t in re.findall(r"^K +(\d+)  +: 0 failed, ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)}
        assert sorted(per_k) == ["1", "16", "4"], run.stdout[-1500:]
        one = re.search(r"^rt_closest_point: ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)
        assert per_k["1"] == (float(one.group(1)), float(one.group(2)))
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls at K = 16 too (degenerate input need not)
            print(f"kind {kind} method {method}: K = 16 makes {per_k['16'][1]} triangle tests per query (brute force 20000)")
            assert per_k["16"][1] < 20000 / 10, run.stdout[-1500:]


# -- the numpy statement on hand-worked cases ---------------------------------------------------------------------------------
def test_one_triangle_stored_three_times():
    q = np.array([[0.25, 0.25, 2, INF]], F32)
    rec, listed, total = ca.nearest_all(ca.tripled_triangle(), q, 2)
    r = rec.view(T.NEAREST).reshape(1, 2)
    assert r["prim_id"].tolist() == [[0, 1]] and listed.tolist() == [2] and total.tolist() == [3]
    assert r["distance"].tolist() == [[2, 2]] and r["position"].tolist() == [[[0.25, 0.25, 0]] * 2] and r["u"].tolist() == [[0.25, 0.25]]
    rec, listed, total = ca.nearest_all(ca.tripled_triangle(), q, 4)
    assert rec.view(T.NEAREST).reshape(4)["prim_id"].tolist() == [0, 1, 2, cc.PRIM_MISS] and listed.tolist() == [3] and total.tolist() == [3]
    assert rec[0, 3].tobytes() == cc.brute_force(scenes.empty_scene(), q).tobytes(), "padding is the miss record"


def test_a_sphere_and_a_triangle_at_equal_dist2():
    q = np.array([[0, 0, 0, INF]], F32)
    for k, prims in ((1, [cc.SPHERE_FLAG]), (2, [cc.SPHERE_FLAG, 0]), (3, [cc.SPHERE_FLAG, 0, cc.PRIM_MISS])):
        rec, listed, total = ca.nearest_all(ca.sphere_and_triangle_tie(), q, k)
        r = rec.view(T.NEAREST).reshape(k)
        assert r["prim_id"].tolist() == prims and total.tolist() == [2] and listed.tolist() == [min(k, 2)]
        assert r["distance"][:2].tolist() == [1.0, 1.0][:k]
    assert r["position"][:2].tolist() == [[0, 0, 1], [0, 0, -1]]
    np.testing.assert_array_equal(rec[:, 0], cc.brute_force(ca.sphere_and_triangle_tie(), q))


def test_the_radius_is_strict_and_degenerate_queries_list_nothing():
    nan = np.nan
    q = np.array([[0.25, 0.25, 2, 2.0], [0.25, 0.25, 2, 2.0000002], [nan, 0, 0, INF], [0, INF, 0, INF], [0, 0, 1, nan], [0, 0, 1, 0.0], [0, 0, 1, -1.0]], F32)
    rec, listed, total = ca.nearest_all(ca.tripled_triangle(), q, 4)
    assert listed.tolist() == [0, 3, 0, 0, 0, 0, 0] and total.tolist() == listed.tolist(), "r * r == dist2 is not in range"
    r = rec.view(T.NEAREST).reshape(len(q), 4)
    assert r["prim_id"][1].tolist() == [0, 1, 2, cc.PRIM_MISS]
    miss = np.delete(r, 1, 0)
    assert (miss["prim_id"] == cc.PRIM_MISS).all() and not miss["position"].any() and not miss["material_id"].any()
    assert miss["distance"].tobytes() == np.repeat(np.delete(q[:, 3], 1), 4).tobytes(), "the radius as given, bit for bit"


def test_the_statement_at_one_is_the_closest_point_statement_and_smaller_k_is_a_prefix():
    scene = scenes.random_soup(300, n_spheres=3)
    points = np.concatenate([cc.four_kinds(scene, 128, 7), np.tile(np.array([0.3, INF], F32), 64)[:, None]], 1)
    rec, listed, total = ca.nearest_all(scene, points)
    np.testing.assert_array_equal(rec[:, 0].view(np.uint32), cc.brute_force(scene, points).view(np.uint32))
    for k in (1, 4):
        want = ca.nearest_all(scene, points, k)
        got = ca.first_k(rec, total, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and total.tobytes() == want[2].tobytes()
    d = rec[:, :, 3]
    prim = rec[:, :, 6].copy().view(np.uint32)
    listed_mask = np.arange(16)[None] < listed[:, None]
    assert (np.diff(d, axis=1)[listed_mask[:, 1:]] >= 0).all() and ((prim != cc.PRIM_MISS) == listed_mask).all()
    assert (total > 16).any() and ((total > 0) & (total < 16)).any() and (total == 0).any()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.closest_point_all
    good = np.zeros((4, 4), F32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="points: shape"):
        call(nc, np.zeros((4, 3), F32), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 4), F32)[::2], 4)
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 4], 4)
    for bad in (-1, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="max_nearest"):
            call(nc, good, bad)
    with pytest.raises(ValueError, match="count_all"):
        call(nc, good, 0)
    with pytest.raises(ValueError, match="rows for 4 points"):
        call(nc, good, 2, out=np.zeros((3, 2, 8), F32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 8), F32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 3, 8), F32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, out=np.zeros((4, 2, 8), np.uint32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="counts: 3 rows"):
        call(nc, good, 2, counts=np.zeros(3, np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_closest_point_all(self, h, points, n, max_nearest, out, counts, flags):
        self.calls.append((points.value, n.value, max_nearest.value, out.value, counts.value, flags.value))
        return 0


def test_closest_point_all_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    points = rt_api.make_points(np.zeros((6, 3), F32))
    out, counts = ctx.closest_point_all(points, 3)
    assert out.shape == (6, 3, 8) and out.dtype == np.float32 and counts.shape == (6,) and counts.dtype == np.uint32
    own, own_counts = np.zeros((6, 16, 8), F32), np.zeros(6, np.uint32)
    got = ctx.closest_point_all(points, np.int64(16), out=own, counts=own_counts, count_all=True, counters=True)
    assert got[0] is own and got[1] is own_counts
    none, only_counts = ctx.closest_point_all(points, 0, out=own, count_all=True)
    assert none is None and only_counts.shape == (6,)
    assert ctx.lib.calls == [(points.ctypes.data, 6, 3, out.ctypes.data, counts.ctypes.data, 0),
                             (points.ctypes.data, 6, 16, own.ctypes.data, own_counts.ctypes.data, rt_api.QUERY_COUNTERS | rt_api.QUERY_COUNT_ALL),
                             (points.ctypes.data, 6, 0, None, only_counts.ctypes.data, rt_api.QUERY_COUNT_ALL)]
