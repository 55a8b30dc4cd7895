"""Closest-point queries (rt_closest_point) without a GPU: the symbol and the record layouts against the header's static asserts and
the numpy dtypes; the whole walk on the host - csrc/closest_point_rules.h, the statements the kernel calls - held to a brute force
under AddressSanitizer + UBSan (tests/check_closest_point.cpp); the numpy float32 statement the GPU tests compare bytes with
(tests/closest_point_cases.py) held to the same statement in float64; and what Context.closest_point validates before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_cases as cc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")


class RtPointQuery(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("radius", C.c_float)]


class RtNearest(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("distance", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_id", C.c_uint32),
                ("material_id", C.c_uint32)]


MIRRORS = {"rt_point_query": (RtPointQuery, T.POINT_QUERY), "rt_nearest": (RtNearest, T.NEAREST)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_closest_point" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_closest_point")
    assert re.search(r"int rt_closest_point\(rt_ctx\* ctx, const rt_point_query\* points, size_t n, rt_nearest\* out, uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_closest_point", _header(), re.S), "listed among the calls a running image survives"


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "cp_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [16, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtPointQuery, f).offset for f in ("position", "radius")] == [0, 12]
    assert [getattr(RtNearest, f).offset for f in ("position", "distance", "u", "v", "prim_id", "material_id")] == [0, 12, 16, 20, 24, 28]
    assert T.EXPECTED_SIZES["POINT_QUERY"] == 16 and T.EXPECTED_SIZES["NEAREST"] == 32
    header = _header()  # the header asserts them itself
    assert "RT_STATIC_ASSERT(sizeof(rt_point_query) == 16" in header and "RT_STATIC_ASSERT(sizeof(rt_nearest) == 32" in header
    assert "offsetof(rt_nearest, prim_id) == 24" in header and "offsetof(rt_point_query, radius) == 12" in header


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    points, out = (RtPointQuery * 1)(), (RtNearest * 1)()
    assert lib.rt_closest_point(C.c_void_p(0), points, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_closest_point(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cp") / "check_closest_point"
    cc_run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_closest_point.cpp"),
                             os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc_run.returncode == 0, cc_run.stderr[-3000:]
    return str(exe)


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every answer of the walk - bound, order, stack and leaf test as the kernel runs them - has the brute force's bytes, and the
    stack stays inside the entries the kernel's launch provides (the program checks every index)."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            tests = float(re.search(r"and ([0-9.]+) triangle tests per query", run.stdout).group(1))
            assert tests < 20000 / 10, run.stdout[-500:]


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000), "cornell12": scenes.cornell12}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_is_the_float64_one_to_a_millionth_of_the_diagonal(name):
    """|d32 - d64| <= 1e-6 x the scene's diagonal over points near surfaces (sigma 0.05), scattered over three times the box, on
    vertices and on surfaces.  Measured with these inputs (1024 points, seed 11): 9.6e-8 of the diagonal on the soup, 6.1e-8 on
    cornell12; the bound is about ten times that, to allow for other seeds.  Prim ids are not compared: exact ties (shared edges)
    may resolve differently in the two precisions."""
    scene = SCENES[name]()
    p = cc.four_kinds(scene, 1024, 11)
    d32, d64 = cc.distances(scene, p, np.float32), cc.distances(scene, p, np.float64)
    err = float(np.abs(d32.astype(np.float64) - d64).max()) / cc.diagonal(scene)
    print(f"{name}: max |d32 - d64| = {err:.3g} of the diagonal")
    assert np.isfinite(d64).all() and err <= 1e-6
    # brute_force's distances are those of the float32 statement
    rec = cc.brute_force(scene, np.concatenate([p, np.full((len(p), 1), np.inf, np.float32)], 1))
    np.testing.assert_array_equal(rec[:, 3], d32)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_prefiltered_brute_force_is_the_brute_force(name):
    scene = scenes.random_soup(3000, n_spheres=3) if name == "soup" else SCENES[name]()
    p = cc.four_kinds(scene, 512, 5)
    radius = np.where(np.arange(len(p)) % 3 == 0, np.float32(0.1), np.float32(np.inf)).astype(np.float32)
    points = np.concatenate([p, radius[:, None]], 1)
    plain, filtered = cc.brute_force(scene, points), cc.brute_force(scene, points, prefilter=True)
    assert plain.tobytes() == filtered.tobytes()
    prim = plain[:, 6].copy().view(np.uint32)
    assert (prim == cc.PRIM_MISS).any() and (prim != cc.PRIM_MISS).any()


def test_statement_on_hand_worked_cases():
    """One triangle (0,0,0) (1,0,0) (0,1,0): each of Ericson's seven regions, the strict radius, degenerate queries; one sphere from
    outside, inside and its centre."""
    import dataclasses
    base = scenes.single_triangle()
    v = base.vertices.copy()
    v["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    tri = dataclasses.replace(base, vertices=v)
    inf = np.inf
    q = np.array([[-1, -1, 0, inf], [2, -1, 0, inf], [0.5, -1, 0, inf], [-1, 2, 0, inf], [-1, 0.5, 0, inf], [1, 1, 0, inf], [0.25, 0.25, 2, inf],
                  [0.25, 0.25, 2, 2.0], [0.25, 0.25, 2, 2.0000002], [np.nan, 0, 0, inf], [0, inf, 0, inf], [0, 0, 1, np.nan], [0, 0, 1, 0.0], [0, 0, 1, -1.0]],
                 np.float32)
    rec = cc.brute_force(tri, q).view(T.NEAREST).reshape(-1)
    np.testing.assert_array_equal(rec["position"][:7], [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]])
    np.testing.assert_array_equal(np.stack([rec["u"][:7], rec["v"][:7]], 1), [[0, 0], [1, 0], [0.5, 0], [0, 1], [0, 0.5], [0.5, 0.5], [0.25, 0.25]])
    np.testing.assert_array_equal(rec["distance"][:7], np.sqrt(np.array([2, 2, 1, 2, 1, 0.5, 4], np.float32)))
    assert (rec["prim_id"][:7] == 0).all() and rec["prim_id"][8] == 0
    miss = rec[[7, 9, 10, 11, 12, 13]]  # r * r == dist2 is not accepted; degenerate queries
    assert (miss["prim_id"] == cc.PRIM_MISS).all() and not miss["position"].any() and not miss["material_id"].any()
    assert miss["distance"].tobytes() == q[[7, 9, 10, 11, 12, 13], 3].tobytes(), "the radius as given, bit for bit"
    sph = dataclasses.replace(base, vertices=base.vertices[:0], triangles=base.triangles[:0],
                              spheres=np.array([((1, 2, 3), 0.5, 4)], T.SPHERE))
    rec = cc.brute_force(sph, np.array([[3, 2, 3, inf], [1.25, 2, 3, inf], [1, 2, 3, inf]], np.float32)).view(T.NEAREST).reshape(-1)
    np.testing.assert_array_equal(rec["position"], [[1.5, 2, 3], [1.5, 2, 3], [1.5, 2, 3]])
    np.testing.assert_array_equal(rec["distance"], np.array([1.5, 0.25, 0.5], np.float32))
    assert (rec["prim_id"] == cc.SPHERE_FLAG).all() and (rec["material_id"] == 4).all() and not rec["u"].any() and not rec["v"].any()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_points_and_split_nearest(rt_api):
    pts = rt_api.make_points([[1, 2, 3], [4, 5, 6]])
    assert pts.dtype == np.float32 and pts.shape == (2, 4) and pts.flags.c_contiguous
    np.testing.assert_array_equal(pts, [[1, 2, 3, np.inf], [4, 5, 6, np.inf]])
    np.testing.assert_array_equal(rt_api.make_points(np.zeros((2, 3)), radius=np.array([0.5, 2.0]))[:, 3], [0.5, 2.0])
    assert pts.view(T.POINT_QUERY).reshape(-1)["radius"].tolist() == [np.inf, np.inf]
    rec = np.zeros(2, T.NEAREST)
    rec["position"], rec["distance"], rec["u"], rec["v"] = [[1, 2, 3], [0, 0, 0]], [0.5, 7], [0.25, 0], [0.5, 0]
    rec["prim_id"], rec["material_id"] = [0x80000001, 0xFFFFFFFF], [3, 0]
    pos, dist, u, v, prim, mat = rt_api.split_nearest(rec.view(np.float32).reshape(2, 8))
    assert prim.dtype == np.uint32 and prim.tolist() == [0x80000001, 0xFFFFFFFF] and mat.tolist() == [3, 0]
    np.testing.assert_array_equal(pos, rec["position"])
    assert (dist.tolist(), u.tolist(), v.tolist()) == ([0.5, 7], [0.25, 0], [0.5, 0])


def test_make_points_and_split_nearest_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    pts = rt_api.make_points(torch.tensor([[1.0, 2, 3]]), radius=2.0)
    assert pts.dtype == torch.float32 and pts.tolist() == [[1, 2, 3, 2]]
    rec = np.zeros(1, T.NEAREST)
    rec["prim_id"], rec["material_id"] = 0xFFFFFFFF, 7
    prim, mat = rt_api.split_nearest(torch.from_numpy(rec.view(np.float32).reshape(1, 8).copy()))[4:]
    assert prim.dtype == torch.int64 and prim.tolist() == [0xFFFFFFFF] and mat.tolist() == [7]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.closest_point
    good = np.zeros((4, 4), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="points: shape"):
        call(nc, np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 4), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 4])
    with pytest.raises(ValueError, match="rows for 4 points"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 8), np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_closest_point(self, h, points, n, out, flags):
        self.calls.append((points.value, n.value, out.value, flags.value))
        return 0


def test_closest_point_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    points = rt_api.make_points(np.zeros((6, 3), np.float32))
    got = ctx.closest_point(points)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.closest_point(points, out=own, counters=True) is own
    assert ctx.lib.calls == [(points.ctypes.data, 6, got.ctypes.data, 0), (points.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS)]
