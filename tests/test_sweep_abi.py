"""Sphere sweeps (rt_sweep_sphere) without a GPU: the symbol and the record layouts against the header's static asserts and the numpy
dtypes; the whole walk on the host - csrc/sweep_rules.h, the statements the kernel calls - held to a brute force under
AddressSanitizer + UBSan (tests/check_sweep.cpp); the numpy float32 statement the GPU tests compare bytes with (tests/sweep_cases.py)
held to the same statement in float64 and to hand-worked cases; and what Context.sweep_sphere validates before the library."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_cases as sc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
INF = np.inf


class RtSweep(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("radius", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtSweepHit(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_id", C.c_uint32),
                ("material_id", C.c_uint32)]


MIRRORS = {"rt_sweep": (RtSweep, T.SWEEP), "rt_sweep_hit": (RtSweepHit, T.SWEEP_HIT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_sweep_sphere" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_sweep_sphere")
    assert re.search(r"int rt_sweep_sphere\(rt_ctx\* ctx, const rt_sweep\* sweeps, size_t n, rt_sweep_hit\* out, uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_sweep_sphere", _header(), re.S), "listed among the calls a running image survives"
    assert "the LOWEST KEY wins, not the nearest" in _header()


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "sw_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [32, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtSweep, f).offset for f in ("origin", "radius", "direction", "tmax")] == [0, 12, 16, 28]
    assert [getattr(RtSweepHit, f).offset for f in ("position", "t", "u", "v", "prim_id", "material_id")] == [0, 12, 16, 20, 24, 28]
    assert T.EXPECTED_SIZES["SWEEP"] == 32 and T.EXPECTED_SIZES["SWEEP_HIT"] == 32
    header = _header()  # the header asserts them itself
    assert "RT_STATIC_ASSERT(sizeof(rt_sweep) == 32" in header and "RT_STATIC_ASSERT(sizeof(rt_sweep_hit) == 32" in header
    for text in ("offsetof(rt_sweep, radius) == 12", "offsetof(rt_sweep, direction) == 16", "offsetof(rt_sweep, tmax) == 28",
                 "offsetof(rt_sweep_hit, t) == 12", "offsetof(rt_sweep_hit, u) == 16", "offsetof(rt_sweep_hit, v) == 20",
                 "offsetof(rt_sweep_hit, prim_id) == 24", "offsetof(rt_sweep_hit, material_id) == 28"):
        assert text in header, text


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    sweeps, out = (RtSweep * 1)(), (RtSweepHit * 1)()
    assert lib.rt_sweep_sphere(C.c_void_p(0), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_sphere(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_sweep.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("sw") / "check_sweep")


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
            tests = float(re.search(r"and ([0-9.]+) triangle tests per sweep", run.stdout).group(1))
            assert tests < 20000 / 10, run.stdout[-500:]


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the margin's sign flipped (-1e-5 for 1e-5, nothing else) the boxes are narrower than the radius asks by as much as they
    were wider, and the check must report wrong answers: 48 of 581 (145 at -1e-4, 213 at -2e-3)."""
    exe = _build_checker(tmp_path / "check_sweep_flipped", "-DRT_SW_SLACK=-1.0e-5f")
    run = subprocess.run([exe, "20000", "1", "0", "0"], capture_output=True, text=True)
    failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
    print(run.stdout.strip().splitlines()[-1])
    assert run.returncode == 1 and failures > 0


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000), "cornell12": scenes.cornell12}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_lies_between_the_float64_ones_of_a_larger_and_a_smaller_radius(name):
    """For every sweep t64(r + eps) <= t32 <= t64(r - eps), a miss counting as +inf, with a relative slack of 1e-6 on finite t and
    eps = k x the scene's diagonal: the float32 time of contact is the exact one of a sphere whose radius is off by at most eps.  No
    sweep is left out.  Measured over these 4096 sweeps (seed 11; toward surfaces, scattered, grazing at r -+ 0.1 %, starting in
    contact, from 20 to 100 diagonals away), the smallest k of the grid 1, 1.5, 2, 3, 5, 7 x 10^n without a violation: 1e-6 on the soup
    and 2e-8 on cornell12 (sweep_cases.K_MEASURED).  On the soup that is one sweep's doing - from 31 diagonals away, t32 = 69.65820
    against 69.65811, 1.4e-6 of t where the relative slack allows 1e-6; without it 2e-9 would do, as it does for 2048 sweeps.  The
    test asserts at twice the measured k, and that this is at most 1e-4: coarser would be wrong, not rounded."""
    scene = SCENES[name]()
    sweeps = sc.five_kinds(scene, 4096, 11)
    k = 2 * sc.K_MEASURED[name]
    assert k <= 1e-4
    eps = k * sc.diagonal(scene)
    t32 = sc.times(scene, sweeps, np.float32).astype(np.float64)
    lower, upper = sc.times(scene, sweeps, np.float64, eps), sc.times(scene, sweeps, np.float64, -eps)
    bad = (lower * (1 - 1e-6) > t32) | (t32 > upper * (1 + 1e-6))
    hit = np.isfinite(t32)
    print(f"{name}: {int(bad.sum())} of {len(sweeps)} outside the sandwich at k = {k:.1e}; {hit.mean():.0%} hit, {(t32 == 0).mean():.0%} in contact at the start")
    assert hit.sum() > 2500 and (~hit).sum() > 150 and (t32 == 0).sum() > 600
    assert not bad.any(), (sweeps[bad][:4], t32[bad][:4], lower[bad][:4], upper[bad][:4])
    # brute_force's times are those of the float32 statement
    rec = sc.brute_force(scene, sweeps[::8])
    np.testing.assert_array_equal(rec[:, 3], t32[::8].astype(F32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float64_statement_touches_at_the_radius_and_not_before(name):
    """The decomposition itself, in float64 where rounding does not blur it: at the time the statement gives, the centre is at distance
    r from the surface (the closest-point statement in float64), and at 25, 50, 75, 95 and 99.9 % of that time it is no nearer than r;
    a sweep the statement calls a miss stays clear of r at samples along ten diagonals of its path.  To 1e-9 of the diagonal: a
    thousand times below the float32 statement's error, and far above float64's (measured: 2.8e-13 on the soup, 6e-14 on cornell12)."""
    import closest_point_cases as cc
    scene = SCENES[name]()
    sweeps = sc.five_kinds(scene, 1024, 11).astype(np.float64)
    v0, e1, e2, _ = sc.records(scene, np.float64)
    o, r, d = sweeps[:, 0:3], sweeps[:, 3], sweeps[:, 4:7]
    t = sc.times(scene, sweeps, np.float64)
    tol = 1e-9 * sc.diagonal(scene)

    def distance(at):
        out = np.empty(len(at))
        for lo in range(0, len(at), 64):
            d2 = cc.triangle_candidates(v0, e1, e2, at[lo:lo + 64])[0]
            out[lo:lo + 64] = np.sqrt(np.where(np.isfinite(d2), d2, np.inf).min(1))
        return out

    hit, moving = np.isfinite(t), np.isfinite(t) & (t > 0)
    assert moving.sum() > 400 and (~hit).sum() > 30 and (hit & ~moving).sum() > 100
    worst = np.abs(distance(o[moving] + d[moving] * t[moving, None]) - r[moving]).max()
    print(f"{name}: the touching centre is at r to {worst:.3g}")
    assert worst <= tol
    for part in (0.25, 0.5, 0.75, 0.95, 0.999):
        assert (distance(o[moving] + d[moving] * (t[moving, None] * part)) >= r[moving] - tol).all(), part
    assert (distance(o[hit & ~moving]) <= r[hit & ~moving] + tol).all(), "t = 0: in contact at the start"
    length = 10 * sc.diagonal(scene) / np.linalg.norm(d[~hit], axis=1)
    for part in np.linspace(0.0, 1.0, 41):
        assert (distance(o[~hit] + d[~hit] * (length * part)[:, None]) > r[~hit] - tol).all(), part


@pytest.mark.parametrize("name", sorted(SCENES))
def test_prefiltered_brute_force_is_the_brute_force(name):
    scene = scenes.random_soup(3000, n_spheres=3) if name == "soup" else SCENES[name]()
    sweeps = sc.five_kinds(scene, 640, 5)
    sweeps[::3, 7] = 0.5  # a third end early: more misses
    plain, filtered = sc.brute_force(scene, sweeps), sc.brute_force(scene, sweeps, prefilter=True)
    assert plain.tobytes() == filtered.tobytes()
    face, edge, vertex, sphere, at_start, miss = sc.contact_kinds(plain)
    assert face.any() and edge.any() and vertex.any() and at_start.any() and miss.any() and (name != "soup" or sphere.any())


def _one_triangle():
    base = scenes.single_triangle()
    v = base.vertices.copy()
    v["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    return dataclasses.replace(base, vertices=v)


def test_statement_on_hand_worked_cases():
    """One triangle (0,0,0) (1,0,0) (0,1,0) in z = 0, a sphere of radius 0.5 dropped along -z from z = 2 onto its interior (t = 1.5),
    onto the edge y = 0 from 0.3 beside it and onto the vertex at the origin from 0.3 beside it (t = 2 - sqrt(0.25 - 0.09) = 1.6); a
    pass by that vertex at a distance of r (1 -+ 1e-5); overlap at the start; tmax on both sides of 1.5; degenerate queries; one sphere
    primitive from outside, from inside, and in contact at the start."""
    tri = _one_triangle()
    nan = np.nan
    x_in, x_out = F32(-0.5 * (1 - 1e-5)), F32(-0.5 * (1 + 1e-5))
    q = np.array([[0.25, 0.25, 2, 0.5, 0, 0, -1, INF], [0.5, -0.3, 2, 0.5, 0, 0, -1, INF], [-0.18, -0.24, 2, 0.5, 0, 0, -1, INF],
                  [0.25, 0.25, 2, 0.5, 0, 0, -2, INF], [0.25, 0.25, -2, 0.5, 0, 0, 1, INF],
                  [x_in, -2, 0, 0.5, 0, 1, 0, INF], [x_out, -2, 0, 0.5, 0, 1, 0, INF],
                  [0.25, 0.25, 0.3, 0.5, 0, 0, 1, INF], [0.25, 0.25, 0.3, 0.5, 0, 0, 1, 1e-38],
                  [0.25, 0.25, 2, 0.5, 0, 0, -1, np.nextafter(F32(1.5), F32(2))], [0.25, 0.25, 2, 0.5, 0, 0, -1, 1.5],
                  [0.25, 0.25, 2, 0.5, 0, 0, 1, INF],
                  [nan, 0, 2, 0.5, 0, 0, -1, INF], [0, 0, 2, 0.5, 0, INF, -1, INF], [0, 0, 2, 0.5, 0, 0, 0, INF], [0, 0, 2, 0.5, 0, -0.0, 0, INF],
                  [0, 0, 2, nan, 0, 0, -1, INF], [0, 0, 2, 0, 0, 0, -1, INF], [0, 0, 2, -1, 0, 0, -1, INF], [0, 0, 2, INF, 0, 0, -1, INF],
                  [0, 0, 2, 0.5, 0, 0, -1, nan], [0, 0, 2, 0.5, 0, 0, -1, 0], [0, 0, 2, 0.5, 0, 0, -1, -1]], F32)
    rec = sc.brute_force(tri, q).view(T.SWEEP_HIT).reshape(-1)
    hits = [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert (rec["prim_id"][hits] == 0).all() and (rec["material_id"][hits] == tri.triangles["material_id"][0]).all()
    np.testing.assert_array_equal(rec["t"][[0, 3, 4, 7, 8, 9]], np.array([1.5, 0.75, 1.5, 0, 0, 1.5], F32))
    np.testing.assert_array_equal(rec["position"][[0, 3, 4, 7, 8, 9]], [[0.25, 0.25, 0]] * 6)
    np.testing.assert_array_equal(np.stack([rec["u"], rec["v"]], 1)[[0, 3, 4, 7, 8, 9]], [[0.25, 0.25]] * 6)
    np.testing.assert_allclose(rec["t"][[1, 2]], [1.6, 1.6], rtol=1e-6)
    np.testing.assert_array_equal(rec["position"][[1, 2]], [[0.5, 0, 0], [0, 0, 0]])
    np.testing.assert_array_equal(np.stack([rec["u"], rec["v"]], 1)[[1, 2]], [[0.5, 0], [0, 0]])
    # past the vertex: inside of touching it the ball at the vertex is hit, outside nothing is
    np.testing.assert_allclose(rec["t"][5], 2 - np.sqrt(0.25 - float(x_in) ** 2), atol=1e-4)
    np.testing.assert_array_equal(rec["position"][5], [0, 0, 0])
    miss = rec[[6, 10, 11] + list(range(12, len(q)))]
    assert (miss["prim_id"] == sc.PRIM_MISS).all() and not miss["position"].any() and not miss["material_id"].any() and not miss["u"].any()
    assert miss["t"].tobytes() == q[[6, 10, 11] + list(range(12, len(q))), 7].tobytes(), "tmax as given, bit for bit"
    # the point reported at t = 0 is the closest-point statement's from the origin
    import closest_point_cases as cc
    near = cc.brute_force(tri, np.array([[0.25, 0.25, 0.3, INF]], F32)).view(T.NEAREST).reshape(-1)
    np.testing.assert_array_equal(rec["position"][7], near["position"][0])

    sph = dataclasses.replace(tri, vertices=tri.vertices[:0], triangles=tri.triangles[:0], spheres=np.array([((1, 2, 3), 0.5, 4)], T.SPHERE))
    q = np.array([[4, 2, 3, 0.25, -1, 0, 0, INF], [1, 2, 3, 0.25, 0, 2, 0, INF], [1.5, 2, 3.1, 0.25, 0, 0, 1, INF], [1.25, 2, 3, 0.25, 1, 0, 0, INF],
                  [4, 2, 3, 0.25, 1, 0, 0, INF], [4, 2, 3, 0.25, -1, 0, 0, 2.25]], F32)
    rec = sc.brute_force(sph, q).view(T.SWEEP_HIT).reshape(-1)
    np.testing.assert_array_equal(rec["t"], np.array([2.25, 0.125, 0, 0, INF, 2.25], F32))
    np.testing.assert_array_equal(rec["position"][[0, 1, 3]], [[1.5, 2, 3], [1, 2.5, 3], [1.5, 2, 3]])
    assert (rec["prim_id"][:4] == sc.SPHERE_FLAG).all() and (rec["material_id"][:4] == 4).all() and not rec["u"].any() and not rec["v"].any()
    assert (rec["prim_id"][4:] == sc.PRIM_MISS).all() and not rec["position"][4:].any()
    near = cc.brute_force(sph, np.array([[1.5, 2, 3.1, INF]], F32)).view(T.NEAREST).reshape(-1)
    np.testing.assert_array_equal(rec["position"][2], near["position"][0])


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_sweeps_and_split_sweep_hits(rt_api):
    sw = rt_api.make_sweeps([[1, 2, 3], [4, 5, 6]], np.array([[0, 0, 1], [0, 1, 0]], np.float64), 0.5)
    assert sw.dtype == np.float32 and sw.shape == (2, 8) and sw.flags.c_contiguous
    np.testing.assert_array_equal(sw, [[1, 2, 3, 0.5, 0, 0, 1, INF], [4, 5, 6, 0.5, 0, 1, 0, INF]])
    sw = rt_api.make_sweeps(np.zeros((2, 3)), np.ones((2, 3)), np.array([0.5, 2.0]), tmax=np.array([1.0, 3.0]))
    rec = sw.view(T.SWEEP).reshape(-1)
    assert rec["radius"].tolist() == [0.5, 2.0] and rec["tmax"].tolist() == [1.0, 3.0] and rec["direction"].tolist() == [[1, 1, 1]] * 2
    rec = np.zeros(2, T.SWEEP_HIT)
    rec["position"], rec["t"], rec["u"], rec["v"] = [[1, 2, 3], [0, 0, 0]], [0.5, 7], [0.25, 0], [0.5, 0]
    rec["prim_id"], rec["material_id"] = [0x80000001, 0xFFFFFFFF], [3, 0]
    pos, t, u, v, prim, mat = rt_api.split_sweep_hits(rec.view(np.float32).reshape(2, 8))
    assert prim.dtype == np.uint32 and prim.tolist() == [0x80000001, 0xFFFFFFFF] and mat.tolist() == [3, 0]
    np.testing.assert_array_equal(pos, rec["position"])
    assert (t.tolist(), u.tolist(), v.tolist()) == ([0.5, 7], [0.25, 0], [0.5, 0])


def test_make_sweeps_and_split_sweep_hits_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    sw = rt_api.make_sweeps(torch.tensor([[1.0, 2, 3]]), torch.tensor([[0.0, 0, -1]]), 0.25, tmax=2.0)
    assert sw.dtype == torch.float32 and sw.tolist() == [[1, 2, 3, 0.25, 0, 0, -1, 2]]
    rec = np.zeros(1, T.SWEEP_HIT)
    rec["prim_id"], rec["material_id"] = 0xFFFFFFFF, 7
    prim, mat = rt_api.split_sweep_hits(torch.from_numpy(rec.view(np.float32).reshape(1, 8).copy()))[4:]
    assert prim.dtype == torch.int64 and prim.tolist() == [0xFFFFFFFF] and mat.tolist() == [7]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.sweep_sphere
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="sweeps: shape"):
        call(nc, np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8])
    with pytest.raises(ValueError, match="rows for 4 sweeps"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 8), np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_sweep_sphere(self, h, sweeps, n, out, flags):
        self.calls.append((sweeps.value, n.value, out.value, flags.value))
        return 0


def test_sweep_sphere_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    sweeps = rt_api.make_sweeps(np.zeros((6, 3), np.float32), np.ones((6, 3), np.float32), 0.1)
    got = ctx.sweep_sphere(sweeps)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.sweep_sphere(sweeps, out=own, counters=True) is own
    assert ctx.lib.calls == [(sweeps.ctypes.data, 6, got.ctypes.data, 0), (sweeps.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS)]
