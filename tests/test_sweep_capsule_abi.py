"""Capsule sweeps (rt_sweep_capsule) without a GPU: the symbol and the record layouts against the header's static asserts and the numpy
dtypes; the whole walk on the host - csrc/sweep_capsule_rules.h, the statements the kernel calls - held to a brute force under
AddressSanitizer + UBSan (tests/check_sweep_capsule.cpp, a stand-alone program); the numpy float32 statement the GPU tests compare
bytes with (tests/sweep_capsule_cases.py) held to the same statement in float64, to a sampled closest pair, to the sphere sweep's
bytes for a zero axis and to hand-worked cases; and what Context.sweep_capsule validates before the library."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_capsule_cases as cap
import sweep_cases as sc
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
F64 = np.float64
INF = np.inf


class RtCapsuleSweep(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("radius", C.c_float), ("axis", C.c_float * 3), ("_pad", C.c_uint32), ("direction", C.c_float * 3),
                ("tmax", C.c_float)]


class RtCapsuleSweepHit(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("t", C.c_float), ("s", C.c_float), ("_reserved", C.c_uint32), ("prim_id", C.c_uint32),
                ("material_id", C.c_uint32)]


MIRRORS = {"rt_capsule_sweep": (RtCapsuleSweep, T.CAPSULE_SWEEP), "rt_capsule_sweep_hit": (RtCapsuleSweepHit, T.CAPSULE_SWEEP_HIT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_sweep_capsule" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_sweep_capsule")
    assert re.search(r"int rt_sweep_capsule\(rt_ctx\* ctx, const rt_capsule_sweep\* sweeps, size_t n, rt_capsule_sweep_hit\* out, uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_sweep_sphere, rt_sweep_box, rt_sweep_capsule,[^.]*\.\s+A call rejected for its arguments changes nothing",
                     _header(), re.S), "listed among the calls a running image survives"
    h = _header()
    assert h.index("Sphere sweeps:") < h.index("Box sweeps:") < h.index("Capsule sweeps:") < h.index("Overlap queries:")


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "swc_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [48, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtCapsuleSweep, f).offset for f in ("origin", "radius", "axis", "_pad", "direction", "tmax")] == [0, 12, 16, 28, 32, 44]
    assert [getattr(RtCapsuleSweepHit, f).offset for f in ("position", "t", "s", "_reserved", "prim_id", "material_id")] == [0, 12, 16, 20, 24, 28]
    assert T.EXPECTED_SIZES["CAPSULE_SWEEP"] == 48 and T.EXPECTED_SIZES["CAPSULE_SWEEP_HIT"] == 32
    # an rt_sweep with 16 bytes inserted at 16; rt_box_sweep_hit's layout with s where axis is
    assert [T.CAPSULE_SWEEP.fields[f][1] for f in ("origin", "radius")] == [T.SWEEP.fields[f][1] for f in ("origin", "radius")]
    assert [T.CAPSULE_SWEEP.fields[f][1] - 16 for f in ("direction", "tmax")] == [T.SWEEP.fields[f][1] for f in ("direction", "tmax")]
    assert [T.CAPSULE_SWEEP_HIT.fields[f][1] for f in ("t", "s", "_reserved", "prim_id", "material_id")] == \
           [T.BOX_SWEEP_HIT.fields[f][1] for f in ("t", "axis", "_reserved", "prim_id", "material_id")]
    header = _header()  # the header asserts them itself
    assert "RT_STATIC_ASSERT(sizeof(rt_capsule_sweep) == 48" in header and "RT_STATIC_ASSERT(sizeof(rt_capsule_sweep_hit) == 32" in header
    for text in ("offsetof(rt_capsule_sweep, radius) == 12", "offsetof(rt_capsule_sweep, axis) == 16", "offsetof(rt_capsule_sweep, direction) == 32",
                 "offsetof(rt_capsule_sweep, tmax) == 44", "offsetof(rt_capsule_sweep_hit, t) == 12", "offsetof(rt_capsule_sweep_hit, s) == 16",
                 "offsetof(rt_capsule_sweep_hit, prim_id) == 24", "offsetof(rt_capsule_sweep_hit, material_id) == 28"):
        assert text in header, text


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    sweeps, out = (RtCapsuleSweep * 1)(), (RtCapsuleSweepHit * 1)()
    assert lib.rt_sweep_capsule(C.c_void_p(0), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_capsule(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out))


def test_query_plan_has_no_new_user():
    """The rules, the kernel and its launcher go through group_walk and record_query; the split over devices stays where it was."""
    for name in ("sweep_capsule_rules.h", "sweep_capsule.hip", "sweep_capsule.h"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_sweep_capsule.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("swc") / "check_sweep_capsule")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every answer of the walk - bound, order, stack and leaf test as the kernel runs them - has the bytes of the brute force, and
    the stack stays inside the entries the kernel's launch provides (the program checks every index).  4 sizes x 6 kinds x 2 methods:
    48 runs."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            tests = float(re.search(r"and ([0-9.]+) triangle tests per sweep", run.stdout).group(1))
            assert tests < 20000 / 10, run.stdout[-500:]
        if n == 20000 and kind == 0:  # every piece group and the start rule decide some contact, and the spheres are there
            counts = list(map(int, re.search(r"start, sphere:((?: \d+){6})", run.stdout).group(1).split()))
            assert all(c > 0 for c in counts), counts


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the margin's sign flipped (-1e-5 for 1e-5, nothing else) the boxes are narrower than the capsule's box asks by as much as
    they were wider and the entry times later, and the check must report wrong answers: 53 of 586 on this input."""
    exe = _build_checker(tmp_path / "check_sweep_capsule_flipped", "-DRT_SWC_SLACK=-1.0e-5f")
    run = subprocess.run([exe, "20000", "1", "0", "0"], capture_output=True, text=True)
    failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
    print(run.stdout.strip().splitlines()[-1])
    assert run.returncode == 1 and failures > 0


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000), "cornell12": scenes.cornell12}


def _near_pairs(scene, sweeps, rng, n):
    """n (sweep, record) pairs that lie near each other, at the sweeps' start poses."""
    v0, e1, e2, _ = cap.records(scene, F64)
    s = sweeps.astype(F64)
    centroid, reach = sc._reach(v0, e1, e2)
    i, j = cap._pairs(centroid, reach, s[:, 0:3], s[:, 4:7], s[:, 8:11], s[:, 3], 0.05 * cap.diagonal(scene))
    pick = rng.choice(len(i), min(n, len(i)), replace=False)
    return i[pick], j[pick]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_cap_triangle_is_the_closest_pair_of_axis_and_triangle(name):
    """cap_triangle in float64 against a sampled brute force, the axis at 257 points x cp_triangle: its distance is never above the
    sampled minimum and below it by no more than the sample spacing; the point it reports lies at that distance; an axis built to
    pierce a triangle's interior gives exactly 0 with s where it crosses."""
    scene = SCENES[name]()
    rng = np.random.default_rng(3)
    sweeps = cap.five_kinds(scene, 640, 11)
    i, j = _near_pairs(scene, sweeps, rng, 6000)
    v0, e1, e2, _ = (a[j] if a.ndim == 2 else a for a in cap.records(scene, F64))
    P, ax = sweeps[i, 0:3].astype(F64), sweeps[i, 4:7].astype(F64)
    d2, s, v, w = cap.cap_triangle(v0, e1, e2, P, ax)
    u = np.linspace(0.0, 1.0, 257)[:, None, None]
    sampled = cap._cp_tri(e1[None], e2[None], (P[None] + ax[None] * u) - v0[None])[0].min(0)
    dist, samp, spacing = np.sqrt(d2), np.sqrt(sampled), np.linalg.norm(ax, axis=1) / 256
    tol = 1e-12 * cap.diagonal(scene)
    print(f"{name}: {len(i)} pairs, {int((d2 == 0).sum())} pierced, {int(((s > 0) & (s < 1)).sum())} with 0 < s < 1; "
          f"cap - sampled in [{(dist - samp).min():.3g}, {(dist - samp).max():.3g}]")
    assert (dist <= samp + tol).all() and (dist >= samp - spacing - tol).all()
    assert ((s >= 0) & (s <= 1) & (v >= -1e-12) & (w >= -1e-12) & (v + w <= 1 + 1e-12)).all()
    gap = (P + ax * s[:, None]) - (v0 + e1 * v[:, None] + e2 * w[:, None])
    np.testing.assert_allclose(np.linalg.norm(gap, axis=1), dist, atol=1e-9 * cap.diagonal(scene))
    assert ((s > 0) & (s < 1)).sum() > 200 and (s == 0).sum() > 500 and (s == 1).sum() > 200
    # piercing, both ends farther than any radius in use
    a, b = rng.uniform(0.1, 0.4, (len(j), 1)), rng.uniform(0.1, 0.4, (len(j), 1))
    through = v0 + e1 * a + e2 * b
    n = np.cross(e1, e2)
    lean = n / np.linalg.norm(n, axis=1, keepdims=True) + 0.5 * sc._unit(rng, len(j))
    where = rng.uniform(0.2, 0.8, (len(j), 1))
    d2, s, v, w = cap.cap_triangle(v0, e1, e2, through - lean * where, lean)
    assert (d2 == 0).all()
    np.testing.assert_allclose(s, where[:, 0], atol=1e-9)
    np.testing.assert_allclose(np.stack([v, w], 1), np.concatenate([a, b], 1), atol=1e-9)
    # and in float32 on the stored edges: the same rule, 0 exactly
    r32 = [x.astype(F32) for x in (v0, e1, e2, through - lean * where, lean)]
    ends = np.minimum(cap._cp_tri(r32[1], r32[2], r32[3] - r32[0])[0], cap._cp_tri(r32[1], r32[2], (r32[3] + r32[4]) - r32[0])[0])
    d32 = cap.cap_triangle(*r32)[0]
    assert d32.dtype == F32 and (d32 == 0).mean() > 0.99 and (ends > 0.01 * (e1 * e1).sum(1).min()).any()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float64_statement_touches_at_its_time_and_not_before(name):
    """The twenty pieces and the start rule, in float64 where rounding does not blur them, against the closest pair of the axis and
    the surface (sweep_capsule_cases.clearance): at the time the statement gives that distance is within 1e-9 of the diagonal of r,
    at 25, 50, 75, 95 and 99.9 % of that time it is above r, a start in contact is within r, and a sweep the statement calls a miss
    stays clear at samples along ten diagonals of its path."""
    scene = SCENES[name]()
    sweeps = cap.five_kinds(scene, 640, 11)
    r = sweeps[:, 3].astype(F64)
    t = cap.times(scene, sweeps, F64)
    tol = 1e-9 * cap.diagonal(scene)
    hit, moving = np.isfinite(t), np.isfinite(t) & (t > 0)
    assert moving.sum() > 200 and (~hit).sum() > 20 and (hit & ~moving).sum() > 100
    at = cap.clearance(scene, sweeps[moving], t[moving]) - r[moving]
    print(f"{name}: at the time of contact the distance is within {np.abs(at).max():.3g} of r")
    assert (np.abs(at) <= tol).all()
    for part in (0.25, 0.5, 0.75, 0.95, 0.999):
        assert (cap.clearance(scene, sweeps[moving], t[moving] * part) >= r[moving] - tol).all(), part
    assert (cap.clearance(scene, sweeps[hit & ~moving], t[hit & ~moving]) <= r[hit & ~moving] + tol).all(), "t = 0: in contact at the start"
    length = 10 * cap.diagonal(scene) / np.linalg.norm(sweeps[~hit, 8:11].astype(F64), axis=1)
    for part in np.linspace(0.0, 1.0, 21):
        assert (cap.clearance(scene, sweeps[~hit], length * part) > r[~hit] - tol).all(), part
    # the piercing starts of in_contact: both ends farther than r, and t = 0
    pierce = sweeps[3 * 128:4 * 128][3::4]
    P, ax = pierce[:, 0:3].astype(F64), pierce[:, 4:7].astype(F64)
    v0, e1, e2, _ = cap.records(scene, F64)
    ends = np.minimum(np.sqrt(cap._cp_tri(e1[None], e2[None], P[:, None] - v0[None])[0]).min(1),
                      np.sqrt(cap._cp_tri(e1[None], e2[None], (P + ax)[:, None] - v0[None])[0]).min(1))
    far = ends > pierce[:, 3]
    assert far.sum() >= 8 and (t[3 * 128:4 * 128][3::4][far] == 0).all()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_lies_between_the_float64_ones_of_a_fatter_and_a_thinner_capsule(name):
    """For every sweep t64(r + eps) <= t32 <= t64(r - eps), a miss counting as +inf, with a relative slack of 1e-6 on finite t and
    eps = k x the scene's diagonal: the float32 time of contact is the exact one of a capsule whose radius is off by at most eps.
    All 4096 sweeps of five_kinds(scene, 4096, 11), none left out.  Measured over them against the float64 statement, the smallest k of
    the grid 1, 1.5, 2, 3, 5, 7 x 10^n without a violation is 3e-9 on the soup (2 of 4096 violate at 2e-9, 17 at 1e-11) and 3e-8 on
    cornell12 (2 at 2e-8, 11 at 1e-11) (sweep_capsule_cases.K_MEASURED).  The test asserts at twice the measured k, and that this is
    at most 1e-4: coarser would be wrong, not rounded."""
    scene = SCENES[name]()
    sweeps = cap.five_kinds(scene, 4096, 11)
    assert len(sweeps) == 4096
    k = 2 * cap.K_MEASURED[name]
    assert k <= 1e-4
    eps = k * cap.diagonal(scene)
    assert eps < sweeps[:, 3].min()
    t32 = cap.times(scene, sweeps, F32).astype(F64)
    lower, upper = cap.times(scene, sweeps, F64, eps), cap.times(scene, sweeps, F64, -eps)
    bad = (lower * (1 - 1e-6) > t32) | (t32 > upper * (1 + 1e-6))
    hit = np.isfinite(t32)
    print(f"{name}: {int(bad.sum())} of {len(sweeps)} outside the sandwich at k = {k:.1e}; {hit.mean():.0%} hit, {(t32 == 0).mean():.0%} in contact at the start")
    assert hit.sum() > 2000 and (~hit).sum() > 150 and (t32 == 0).sum() > 600
    assert not bad.any(), (sweeps[bad][:4], t32[bad][:4], lower[bad][:4], upper[bad][:4])
    # brute_force's times are those of the float32 statement
    rec = cap.brute_force(scene, sweeps[::8])
    np.testing.assert_array_equal(rec[:, 3], t32[::8].astype(F32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_prefiltered_statements_are_the_statements(name):
    """times() evaluates only the pairs that can touch, brute_force(prefilter=True) only the records that can: both give what the
    full evaluation gives, bit for bit."""
    scene = scenes.random_soup(3000, n_spheres=3) if name == "soup" else SCENES[name]()
    sweeps = cap.five_kinds(scene, 320, 5)
    for dtype in (F32, F64):
        for off in (0.0, 1e-5):
            np.testing.assert_array_equal(cap.times(scene, sweeps, dtype, off), cap.times(scene, sweeps, dtype, off, prefilter=False))
    sweeps[::3, 11] = 0.5  # a third end early: more misses
    plain, filtered = cap.brute_force(scene, sweeps), cap.brute_force(scene, sweeps, prefilter=True)
    assert plain.tobytes() == filtered.tobytes()
    rec = plain.view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    hit = rec["prim_id"] != cap.PRIM_MISS
    assert hit.any() and (~hit).any() and (rec["t"][hit] == 0).any() and ((rec["s"] > 0) & (rec["s"] < 1)).any() and (rec["s"] == 1).any()


def test_a_zero_axis_gives_the_sphere_sweeps_bytes():
    """axis == 0 exactly: t, position, prim_id and material_id are sweep_cases.py's, bit for bit, and s = 0: 1024 sweeps of the
    sphere sweep's five kinds on the soup with its spheres."""
    scene = scenes.random_soup(3000, n_spheres=3)
    s8 = sc.five_kinds(scene, 1024, 11)
    want = sc.brute_force(scene, s8).view(T.SWEEP_HIT).reshape(-1)
    got = cap.brute_force(scene, cap.zero_axis(s8)).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    for f in ("t", "position", "prim_id", "material_id"):
        np.testing.assert_array_equal(got[f].view(np.uint32), want[f].view(np.uint32), err_msg=f)
    assert not got["s"].view(np.uint32).any() and not got["_reserved"].any()
    hit = want["prim_id"] != cap.PRIM_MISS
    assert hit.sum() > 700 and (want["prim_id"][hit] >= cap.SPHERE_FLAG).sum() >= 5 and (want["t"][hit] == 0).sum() > 100


def _one_triangle():
    base = scenes.single_triangle()
    v = base.vertices.copy()
    v["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    return dataclasses.replace(base, vertices=v)


def _q(A, r, axis, d, tmax=INF):
    return [*A, r, *axis, 0, *d, tmax]


def _decider(tri, q):
    """Per sweep: the piece group whose time is the smallest, first among equals (0 end A, 1 end B, 2 wall x vertex, 3 wall x edge),
    or 4 for the start rule."""
    v0, e1, e2, _ = cap.records(tri)
    q = np.asarray(q, F32)
    start, g = cap.triangle_groups(v0, e1, e2, *(np.ascontiguousarray(q[:, k:k + 3]) for k in (0, 4, 8)), q[:, 3])
    return np.where(start[:, 0], 4, g[:, :, 0].argmin(0)), g[:, :, 0]


def test_statement_on_hand_worked_cases():
    """One triangle (0,0,0) (1,0,0) (0,1,0) in z = 0, r = 0.25 unless said.
    0  Upright, A = (0.25, 0.25, 2), axis (0, 0, 1), dropped by (0, 0, -1): the lower end is A, t = (2 - 0.25) / 1 = 1.75, s = 0,
       position (0.25, 0.25, 0); end A's face decides (group 0).
    1  The same with twice the speed: t = (height - r) / |d| = 0.875.
    2  The same body given from its upper end, A = (0.25, 0.25, 3), axis (0, 0, -1): t = 1.75, s = 1; end B's face (group 1).
    3  Horizontal, A = (0.125, 0.25, 2), axis (0.5, 0, 0), landing flat: both ends' faces and the whole axis touch at t = 1.75, a tie
       along the axis.  cap_triangle takes the first candidate with the strictly smallest distance: end A, s = 0, position
       (0.125, 0.25, 0); group 0 is the first to give the time.
    4  The cylinder wall against a vertex: A = (3, -0.5, 0), axis (0, 1, 0), in the triangle's plane moving by (-1, 0, 0) toward the
       vertex (1, 0, 0): t = 3 - 1 - 0.25 = 1.75, s = 0.5, position (1, 0, 0); group 2, and no other group gives a time that early.
    5  The cylinder wall against an edge: A = (0.5, -2, -0.5), axis (0, 0, 1), an upright capsule across the plane moving by (0, 1, 0)
       toward the edge y = 0: t = 2 - 0.25 = 1.75, s = 0.5, position (0.5, 0, 0); group 3.
    6  The piercing start: A = (0.25, 0.25, -1), axis (0, 0, 2), r = 0.1: both ends are 1 away, the axis crosses the face: t = 0,
       s = 0.5, position (0.25, 0.25, 0); with the smallest tmax too (7).
    8, 9  Case 0 with tmax = nextafter(1.75) and with tmax = 1.75: the same contact, and the miss that carries 1.75.
    10  Away from the triangle: a miss.
    Then every degenerate query; an axis parallel to the direction, which equals the sphere sweep of the leading end; and one sphere
    primitive."""
    tri = _one_triangle()
    nan = np.nan
    down = [0, 0, -1]
    q = np.array([_q([0.25, 0.25, 2], 0.25, [0, 0, 1], down), _q([0.25, 0.25, 2], 0.25, [0, 0, 1], [0, 0, -2]),
                  _q([0.25, 0.25, 3], 0.25, [0, 0, -1], down), _q([0.125, 0.25, 2], 0.25, [0.5, 0, 0], down),
                  _q([3, -0.5, 0], 0.25, [0, 1, 0], [-1, 0, 0]), _q([0.5, -2, -0.5], 0.25, [0, 0, 1], [0, 1, 0]),
                  _q([0.25, 0.25, -1], 0.1, [0, 0, 2], [1, 0, 0]), _q([0.25, 0.25, -1], 0.1, [0, 0, 2], [1, 0, 0], 1e-38),
                  _q([0.25, 0.25, 2], 0.25, [0, 0, 1], down, np.nextafter(F32(1.75), F32(2))), _q([0.25, 0.25, 2], 0.25, [0, 0, 1], down, 1.75),
                  _q([0.25, 0.25, 2], 0.25, [0, 0, 1], [0, 0, 1]),
                  # degenerate
                  _q([nan, 0, 2], 0.25, [0, 0, 1], down), _q([0, INF, 2], 0.25, [0, 0, 1], down), _q([0, 0, 2], 0.25, [0, nan, 1], down),
                  _q([0, 0, 2], 0.25, [INF, 0, 1], down), _q([0, 0, 2], 0.25, [0, 0, 1], [0, nan, -1]), _q([0, 0, 2], 0.25, [0, 0, 1], [0, INF, -1]),
                  _q([0, 0, 2], 0.25, [0, 0, 1], [0, 0, 0]), _q([0, 0, 2], 0.25, [0, 0, 1], [0, -0.0, 0]), _q([0, 0, 2], nan, [0, 0, 1], down),
                  _q([0, 0, 2], 0.0, [0, 0, 1], down), _q([0, 0, 2], -0.25, [0, 0, 1], down), _q([0, 0, 2], INF, [0, 0, 1], down),
                  _q([0, 0, 2], 0.25, [0, 0, 1], down, nan), _q([0, 0, 2], 0.25, [0, 0, 1], down, 0), _q([0, 0, 2], 0.25, [0, 0, 1], down, -0.0),
                  _q([0, 0, 2], 0.25, [0, 0, 1], down, -1)], F32)
    rec = cap.brute_force(tri, q).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    hits = list(range(9))
    assert (rec["prim_id"][hits] == 0).all() and (rec["material_id"][hits] == tri.triangles["material_id"][0]).all() and not rec["_reserved"].any()
    np.testing.assert_array_equal(rec["t"][[0, 1, 2, 3, 6, 7, 8]], np.array([1.75, 0.875, 1.75, 1.75, 0, 0, 1.75], F32))
    np.testing.assert_allclose(rec["t"][[4, 5]], [1.75, 1.75], rtol=1e-6)
    np.testing.assert_array_equal(rec["s"][[0, 1, 2, 3, 6, 7, 8]], np.array([0, 0, 1, 0, 0.5, 0.5, 0], F32))
    np.testing.assert_allclose(rec["s"][[4, 5]], [0.5, 0.5], rtol=1e-6)
    np.testing.assert_allclose(rec["position"][hits], [[0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0], [0.125, 0.25, 0], [1, 0, 0], [0.5, 0, 0],
                                                        [0.25, 0.25, 0], [0.25, 0.25, 0], [0.25, 0.25, 0]], atol=1e-6)
    who, g = _decider(tri, q[:9])
    assert who.tolist() == [0, 0, 1, 0, 2, 3, 4, 4, 0]
    assert g[0, 3] == g[1, 3] == F32(1.75), "landing flat: both ends' faces at the same time"
    for k, group in ((4, 2), (5, 3)):  # the wall's piece alone is that early
        assert (np.delete(g[:, k], group) > g[group, k] * 1.01).all(), (k, g[:, k])
    misses = [9, 10] + list(range(11, len(q)))
    miss = rec[misses]
    assert (miss["prim_id"] == cap.PRIM_MISS).all() and not miss["position"].any() and not miss["s"].any() and not miss["material_id"].any()
    assert miss["t"].tobytes() == q[misses, 11].tobytes(), "tmax as given, bit for bit"
    assert cap.valid(q).tolist() == [True] * 11 + [False] * 16

    # an axis parallel to the direction (axis = -+ d / 4, exact in f32): the trailing end and the wall never come first.  Leading end
    # A: the time is the sphere sweep's from A bit for bit (its seven pieces are group 0).  Leading end B: the sphere sweep's from B
    # up to the rounding of ap + axis against (A + axis) - v0.
    rng = np.random.default_rng(5)
    target = np.array([[0.3, 0.3, 0], [0.5, 0, 0], [1, 0, 0], [0, 0, 0], [0.5, 0.5, 0], [0, 1, 0]] * 8, F64) + 0.0
    origin = target + rng.normal(size=target.shape) * 2 + [0, 0, 0.5]
    d = ((target - origin) * rng.uniform(0.3, 1.0, (len(target), 1))).astype(F32)
    r = rng.uniform(0.05, 0.3, len(d)).astype(F32)
    origin = origin.astype(F32)
    lead_a = cap._pack(origin, -d / 4, d, r)
    sphere_a = sc.brute_force(tri, sc._pack(origin, d, r)).view(T.SWEEP_HIT).reshape(-1)
    got = cap.brute_force(tri, lead_a).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    moving = sphere_a["t"] > 0
    assert moving.sum() > 30 and (sphere_a["prim_id"] == 0).all()
    np.testing.assert_array_equal(got["t"], sphere_a["t"])
    np.testing.assert_array_equal(got["position"][moving], sphere_a["position"][moving])
    assert not got["s"][moving].any()
    lead_b = cap._pack(origin - d / 4, d / 4, d, r)
    got = cap.brute_force(tri, lead_b).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    np.testing.assert_allclose(got["t"][moving], sphere_a["t"][moving], rtol=2e-5)  # B starts where the sphere does
    np.testing.assert_allclose(got["position"][moving], sphere_a["position"][moving], atol=2e-5)
    assert (got["s"][moving] == 1).all()

    # one sphere primitive, centre (1, 2, 3), R = 0.5; the capsule r = 0.25 with axis (0, 1, 0)
    # 0  from (4, 1.5, 3) by (-1, 0, 0): C's foot is the middle of the axis, the wall: t = 3 - (R + r) = 2.25, s = 0.5, position (1.5, 2, 3)
    # 1  from (4, 2.3, 3): end A, 0.3 above C: (3 - t)^2 + 0.09 = 0.5625, t = 3 - sqrt 0.4725, s = 0
    # 2  from (4, 0.7, 3): end B, 0.3 below C: the same t, s = 1
    # 3  inside, R = 0.5, r = 0.125, axis (0, 0.25, 0) from (1, 2, 3) by (0, 1, 0): end B leads and leaves at 0.25 + t = R - r, t = 0.125, s = 1,
    #    position (1, 2.5, 3)
    # 4  the axis through the sphere's centre, both ends 2 away: t = 0; dmin = 0 is not > R, so s is the farther end, A on the tie: s = 0.
    # 5  moving away: a miss.   6  case 0 with tmax = 2.25: a miss.
    sph = dataclasses.replace(tri, vertices=tri.vertices[:0], triangles=tri.triangles[:0], spheres=np.array([((1, 2, 3), 0.5, 4)], T.SPHERE))
    up = [0, 1, 0]
    q = np.array([_q([4, 1.5, 3], 0.25, up, [-1, 0, 0]), _q([4, 2.3, 3], 0.25, up, [-1, 0, 0]), _q([4, 0.7, 3], 0.25, up, [-1, 0, 0]),
                  _q([1, 2, 3], 0.125, [0, 0.25, 0], up), _q([1, 0, 3], 0.25, [0, 4, 0], [1, 0, 0]), _q([4, 1.5, 3], 0.25, up, [1, 0, 0]),
                  _q([4, 1.5, 3], 0.25, up, [-1, 0, 0], 2.25)], F32)
    rec = cap.brute_force(sph, q).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    assert rec["t"][4] == 0 and rec["t"][5] == INF and rec["t"][6] == 2.25
    np.testing.assert_allclose(rec["t"][:4], [2.25, 3 - np.sqrt(0.4725), 3 - np.sqrt(0.4725), 0.125], rtol=2e-6)
    np.testing.assert_allclose(rec["s"][:5], [0.5, 0, 1, 1, 0], atol=1e-6)
    np.testing.assert_allclose(rec["position"][[0, 3]], [[1.5, 2, 3], [1, 2.5, 3]], atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(rec["position"][:5] - [1, 2, 3], axis=1), 0.5, rtol=1e-6)
    assert (rec["prim_id"][:5] == cap.SPHERE_FLAG).all() and (rec["material_id"][:5] == 4).all()
    assert (rec["prim_id"][5:] == cap.PRIM_MISS).all() and not rec["material_id"][5:].any() and not rec["s"][5:].any()


def test_cube_sweeps_tie_between_neighbouring_triangles():
    """cornell12's cube_sweeps: different triangles reach the same t bit for bit, moving and at the start, and the lower index wins."""
    scene = scenes.cornell12()
    sweeps = cap.cube_sweeps(9)
    assert len(sweeps) == 1024
    v0, e1, e2, _ = cap.records(scene)
    t = cap.triangle_times(v0, e1, e2, *(np.ascontiguousarray(sweeps[:, k:k + 3]) for k in (0, 4, 8)), sweeps[:, 3])
    best = t.min(1, keepdims=True)
    tied = (t == best) & np.isfinite(best)
    several, moving = tied.sum(1) >= 2, best[:, 0] > 0
    print("cornell12:", dict(ties_moving=int((several & moving).sum()), ties_at_start=int((several & ~moving).sum())))
    assert (several & moving).sum() >= 100 and (several & ~moving).sum() >= 50
    rec = cap.brute_force(scene, sweeps).view(T.CAPSULE_SWEEP_HIT).reshape(-1)
    hit = rec["prim_id"] != cap.PRIM_MISS
    np.testing.assert_array_equal(rec["prim_id"][hit], tied.argmax(1)[hit])


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_capsule_sweeps_and_split_capsule_sweep_hits(rt_api):
    sw = rt_api.make_capsule_sweeps([[1, 2, 3], [4, 5, 6]], (0, 0.5, 0), np.array([[0, 0, 1], [0, 1, 0]], np.float64), 0.25)
    assert sw.dtype == np.float32 and sw.shape == (2, 12) and sw.flags.c_contiguous
    np.testing.assert_array_equal(sw, [[1, 2, 3, 0.25, 0, 0.5, 0, 0, 0, 0, 1, INF], [4, 5, 6, 0.25, 0, 0.5, 0, 0, 0, 1, 0, INF]])
    sw = rt_api.make_capsule_sweeps(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0]]), np.ones((2, 3)), np.array([0.1, 0.2]), tmax=np.array([1.0, 3.0]))
    rec = sw.view(T.CAPSULE_SWEEP).reshape(-1)
    assert rec["axis"].tolist() == [[1, 2, 3], [0, 0, 0]] and rec["tmax"].tolist() == [1.0, 3.0] and rec["direction"].tolist() == [[1, 1, 1]] * 2
    assert rec["radius"].tolist() == [F32(0.1), F32(0.2)] and not rec["_pad"].any()
    np.testing.assert_array_equal(sw, cap._pack(np.zeros((2, 3)), [[1, 2, 3], [0, 0, 0]], np.ones((2, 3)), [0.1, 0.2], [1.0, 3.0]))
    rec = np.zeros(2, T.CAPSULE_SWEEP_HIT)
    rec["position"], rec["t"], rec["s"] = [[0, 0, 1], [0, 0, 0]], [0.5, 7], [0.25, 0]
    rec["prim_id"], rec["material_id"] = [0x80000001, 0xFFFFFFFF], [3, 0]
    pos, t, s, prim, mat = rt_api.split_capsule_sweep_hits(rec.view(np.float32).reshape(2, 8))
    assert prim.dtype == np.uint32 and prim.tolist() == [0x80000001, 0xFFFFFFFF] and mat.tolist() == [3, 0] and s.tolist() == [0.25, 0]
    np.testing.assert_array_equal(pos, rec["position"])
    assert t.tolist() == [0.5, 7]


def test_make_capsule_sweeps_and_split_capsule_sweep_hits_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    sw = rt_api.make_capsule_sweeps(torch.tensor([[1.0, 2, 3]]), (0.5, 0.25, 0.0), torch.tensor([[0.0, 0, -1]]), 0.125, tmax=2.0)
    assert sw.dtype == torch.float32 and sw.tolist() == [[1, 2, 3, 0.125, 0.5, 0.25, 0, 0, 0, 0, -1, 2]]
    sw = rt_api.make_capsule_sweeps(torch.zeros((2, 3)), torch.tensor([[0.0, 1, 0], [0, 0, 0]]), torch.ones((2, 3)), torch.tensor([0.5, 0.25]))
    assert sw[:, 3].tolist() == [0.5, 0.25] and sw[:, 4:7].tolist() == [[0, 1, 0], [0, 0, 0]] and sw[:, 11].tolist() == [INF, INF]
    rec = np.zeros(1, T.CAPSULE_SWEEP_HIT)
    rec["s"], rec["prim_id"], rec["material_id"] = 0.5, 0xFFFFFFFF, 7
    s, prim, mat = rt_api.split_capsule_sweep_hits(torch.from_numpy(rec.view(np.float32).reshape(1, 8).copy()))[2:]
    assert prim.dtype == torch.int64 and prim.tolist() == [0xFFFFFFFF] and mat.tolist() == [7] and s.tolist() == [0.5]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.sweep_capsule
    good = np.zeros((4, 12), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="sweeps: shape"):
        call(nc, np.zeros((4, 8), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 12), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 12])
    with pytest.raises(ValueError, match="rows for 4 sweeps"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 12), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 8), np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_sweep_capsule(self, h, sweeps, n, out, flags):
        self.calls.append((sweeps.value, n.value, out.value, flags.value))
        return 0


def test_sweep_capsule_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    sweeps = rt_api.make_capsule_sweeps(np.zeros((6, 3), np.float32), (0, 0.2, 0), np.ones((6, 3), np.float32), 0.1)
    got = ctx.sweep_capsule(sweeps)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.sweep_capsule(sweeps, out=own, counters=True) is own
    assert ctx.lib.calls == [(sweeps.ctypes.data, 6, got.ctypes.data, 0), (sweeps.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS)]
