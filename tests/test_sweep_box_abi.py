"""Box sweeps (rt_sweep_box) without a GPU: the symbol and the record layouts against the header's static asserts and the numpy dtypes;
the whole walk on the host - csrc/sweep_box_rules.h, the statements the kernel calls - held to a brute force under AddressSanitizer +
UBSan (tests/check_sweep_box.cpp, a stand-alone program); the numpy float32 statement the GPU tests compare bytes with
(tests/sweep_box_cases.py) held to the same statement in float64, to the static test along the path and to hand-worked cases; and what
Context.sweep_box validates before the library."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import sweep_box_cases as sb
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
INF = np.inf
NONE = sb.AXIS_NONE


class RtBoxSweep(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("_pad0", C.c_uint32), ("half_extent", C.c_float * 3), ("_pad1", C.c_uint32),
                ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtBoxSweepHit(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("t", C.c_float), ("axis", C.c_uint32), ("_reserved", C.c_uint32), ("prim_id", C.c_uint32),
                ("material_id", C.c_uint32)]


MIRRORS = {"rt_box_sweep": (RtBoxSweep, T.BOX_SWEEP), "rt_box_sweep_hit": (RtBoxSweepHit, T.BOX_SWEEP_HIT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_sweep_box" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_sweep_box")
    assert re.search(r"int rt_sweep_box\(rt_ctx\* ctx, const rt_box_sweep\* sweeps, size_t n, rt_box_sweep_hit\* out, uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_sweep_sphere, rt_sweep_box,", _header(), re.S), "listed among the calls a running image survives"
    assert re.search(r"#define RT_SWEEP_AXIS_SPHERE 13u\n#define RT_SWEEP_AXIS_NONE 0xFFFFFFFFu\n", code)
    assert rt_api.SWEEP_AXIS_SPHERE == sb.AXIS_SPHERE == 13 and rt_api.SWEEP_AXIS_NONE == NONE == 0xFFFFFFFF
    assert _header().index("Sphere sweeps:") < _header().index("Box sweeps:") < _header().index("Overlap queries:")


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "swb_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [48, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtBoxSweep, f).offset for f in ("center", "half_extent", "direction", "tmax")] == [0, 16, 32, 44]
    assert [getattr(RtBoxSweepHit, f).offset for f in ("normal", "t", "axis", "_reserved", "prim_id", "material_id")] == [0, 12, 16, 20, 24, 28]
    assert T.EXPECTED_SIZES["BOX_SWEEP"] == 48 and T.EXPECTED_SIZES["BOX_SWEEP_HIT"] == 32
    assert [T.BOX_SWEEP.fields[f][1] for f in ("center", "half_extent")] == [T.BOX.fields[f][1] for f in ("center", "half_extent")], "an rt_box first"
    header = _header()  # the header asserts them itself
    assert "RT_STATIC_ASSERT(sizeof(rt_box_sweep) == 48" in header and "RT_STATIC_ASSERT(sizeof(rt_box_sweep_hit) == 32" in header
    for text in ("offsetof(rt_box_sweep, half_extent) == 16", "offsetof(rt_box_sweep, direction) == 32", "offsetof(rt_box_sweep, tmax) == 44",
                 "offsetof(rt_box_sweep_hit, t) == 12", "offsetof(rt_box_sweep_hit, axis) == 16", "offsetof(rt_box_sweep_hit, prim_id) == 24",
                 "offsetof(rt_box_sweep_hit, material_id) == 28"):
        assert text in header, text


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    sweeps, out = (RtBoxSweep * 1)(), (RtBoxSweepHit * 1)()
    assert lib.rt_sweep_box(C.c_void_p(0), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_box(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out))


def test_query_plan_has_no_new_user():
    """The rules, the kernel and its launcher go through group_walk and record_query; the split over devices stays where it was."""
    for name in ("sweep_box_rules.h", "sweep_box.hip", "sweep_box.h"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_sweep_box.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("swb") / "check_sweep_box")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every answer of the walk - bound, order, stack, leaf test and its early returns as the kernel runs them - has the bytes of the
    brute force, which knows no limit, and the stack stays inside the entries the kernel's launch provides (the program checks every
    index)."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            tests = float(re.search(r"and ([0-9.]+) triangle tests per sweep", run.stdout).group(1))
            assert tests < 20000 / 10, run.stdout[-500:]
        if n == 20000 and kind == 0:  # every axis closes some contact last, and the spheres and the starts in contact are there
            counts = list(map(int, re.search(r"axes 0\.\.12, sphere, none:((?: \d+){15})", run.stdout).group(1).split()))
            assert all(c > 0 for c in counts), counts


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the margin's sign flipped (-1e-5 for 1e-5, nothing else) the boxes are narrower than the half extents ask by as much as
    they were wider and the entry times later, and the check must report wrong answers: 68 of 584 on this input."""
    exe = _build_checker(tmp_path / "check_sweep_box_flipped", "-DRT_SWB_SLACK=-1.0e-5f")
    run = subprocess.run([exe, "20000", "1", "0", "0"], capture_output=True, text=True)
    failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
    print(run.stdout.strip().splitlines()[-1])
    assert run.returncode == 1 and failures > 0


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000), "cornell12": scenes.cornell12}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_lies_between_the_float64_ones_of_a_larger_and_a_smaller_box(name):
    """For every sweep t64(h + eps) <= t32 <= t64(h - eps), a miss counting as +inf, with a relative slack of 1e-6 on finite t and
    eps = k x the scene's diagonal on every axis: the float32 time of contact is the exact one of a box whose half extents are off by
    at most eps.  The sweeps are those of five_kinds(scene, 4096, 11) whose extents are all >= 1e-3 x the diagonal, so that h - eps
    stays positive (every eighth of each kind has a zero extent: 3586 remain), and none of these is left out.  Measured over them, the smallest k
    of the grid 1, 1.5, 2, 3, 5, 7 x 10^n without a violation is 5e-7 on the soup - one sweep's doing from k = 1.5e-9 on, six of 3586 at 1e-10 - and on cornell12,
    where every contact closes on a box axis, no value is violated down to eps = 0 (sweep_box_cases.K_MEASURED).  The test asserts at
    twice the measured k, and that this is at most 1e-4: coarser would be wrong, not rounded."""
    scene = SCENES[name]()
    sweeps = sb.five_kinds(scene, 4096, 11)
    sweeps = sweeps[sb.full_extents(scene, sweeps)]
    assert len(sweeps) == 3586
    k = 2 * sb.K_MEASURED[name]
    assert k <= 1e-4
    eps = k * sb.diagonal(scene)
    t32 = sb.times(scene, sweeps, np.float32).astype(np.float64)
    lower, upper = sb.times(scene, sweeps, np.float64, eps), sb.times(scene, sweeps, np.float64, -eps)
    bad = (lower * (1 - 1e-6) > t32) | (t32 > upper * (1 + 1e-6))
    hit = np.isfinite(t32)
    print(f"{name}: {int(bad.sum())} of {len(sweeps)} outside the sandwich at k = {k:.1e}; {hit.mean():.0%} hit, {(t32 == 0).mean():.0%} in contact at the start")
    assert hit.sum() > 2000 and (~hit).sum() > 150 and (t32 == 0).sum() > 600
    assert not bad.any(), (sweeps[bad][:4], t32[bad][:4], lower[bad][:4], upper[bad][:4])
    # brute_force's times are those of the float32 statement
    rec = sb.brute_force(scene, sweeps[::8])
    np.testing.assert_array_equal(rec[:, 3], t32[::8].astype(F32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float64_statement_touches_at_its_time_and_not_before(name):
    """The thirteen intervals themselves, in float64 where rounding does not blur them, against the static thirteen-axis test
    (sweep_box_cases.clearance: the largest gap over the axes, as a distance; <= 0 iff the box touches): at the time the statement
    gives the box touches to within 1e-9 of the diagonal, at 25, 50, 75, 95 and 99.9 % of that time it is clear, a start in contact
    touches, and a sweep the statement calls a miss stays clear at samples along ten diagonals of its path."""
    scene = SCENES[name]()
    sweeps = sb.five_kinds(scene, 640, 11).astype(np.float64)
    c, h, d = sweeps[:, 0:3], sweeps[:, 4:7], sweeps[:, 8:11]
    t = sb.times(scene, sweeps, np.float64)
    tol = 1e-9 * sb.diagonal(scene)
    hit, moving = np.isfinite(t), np.isfinite(t) & (t > 0)
    assert moving.sum() > 200 and (~hit).sum() > 20 and (hit & ~moving).sum() > 100
    at = sb.clearance(scene, c[moving] + d[moving] * t[moving, None], h[moving])
    print(f"{name}: at the time of contact the gap is within {np.abs(at).max():.3g}")
    assert (np.abs(at) <= tol).all()
    for part in (0.25, 0.5, 0.75, 0.95, 0.999):
        assert (sb.clearance(scene, c[moving] + d[moving] * (t[moving, None] * part), h[moving]) >= -tol).all(), part
    assert (sb.clearance(scene, c[hit & ~moving], h[hit & ~moving]) <= tol).all(), "t = 0: in contact at the start"
    length = 10 * sb.diagonal(scene) / np.linalg.norm(d[~hit], axis=1)
    for part in np.linspace(0.0, 1.0, 21):
        assert (sb.clearance(scene, c[~hit] + d[~hit] * (length * part)[:, None], h[~hit]) > -tol).all(), part


@pytest.mark.parametrize("name", sorted(SCENES))
def test_prefiltered_brute_force_is_the_brute_force(name):
    scene = scenes.random_soup(3000, n_spheres=3) if name == "soup" else SCENES[name]()
    sweeps = sb.five_kinds(scene, 640, 5)
    sweeps[::3, 11] = 0.5  # a third end early: more misses
    plain, filtered = sb.brute_force(scene, sweeps), sb.brute_force(scene, sweeps, prefilter=True)
    assert plain.tobytes() == filtered.tobytes()
    box_face, tri_face, edge_edge, sphere, at_start, miss = sb.contact_kinds(plain)
    assert box_face.any() and at_start.any() and miss.any() and (name != "soup" or (tri_face.any() and edge_edge.any()))


def _one_triangle():
    base = scenes.single_triangle()
    v = base.vertices.copy()
    v["position"] = [[0, 0, 0], [1, 0, 0], [0, 1, 0]]
    return dataclasses.replace(base, vertices=v)


def _q(c, h, d, tmax=INF):
    h = [h] * 3 if np.isscalar(h) else h
    return [*c, 0, *h, 0, *d, tmax]


def test_statement_on_hand_worked_cases():
    """One triangle (0,0,0) (1,0,0) (0,1,0) in z = 0; a_k = vertex - centre, lo = pmin - r, hi = pmax + r.
    0  A cube of half extent 0.5 dropped along -z from (0.25, 0.25, 2): on axis z every a_k.z = -2, r = 0.5, w = -1, so enter =
       hi / w = (-2 + 0.5) / -1 = 1.5 and exit = lo / w = 2.5; x and y have w = 0 and overlap; the normal (axis 3) gives the same 1.5,
       which is not strictly larger, and the edge axes have w = 0 or enter below: t = 1.5, axis 2, normal (0, 0, 1).
    1  The same with twice the speed: t = 0.75.   2  From below, +z: t = 1.5, axis 2, normal (0, 0, -1).
    3  A drop past the hypotenuse x + y = 1 from (1.1, 1.1, 2): the box's nearest corner (0.6, 0.6) has x + y = 1.2.  The box axes
       x and y overlap ([0.6, 1.6] against [0, 1]) and z closes at 1.5, but on axis 9 = cross(unit_z, e2 - e1), L = (-1, -1, 0), the
       vertices project to 2.2, 1.2, 1.2 against r = 1 and w = 0: separated for good, a miss that only this edge-edge axis sees.
    4  The same box in the triangle's plane moving by (-1, -1, 0) from (1.1, 1.1, 0): on axis 9 w = f.x d.y - f.y d.x = 2, lo = 1.2 - 1,
       enter = 0.1, while x and y enter at (-0.1 + 0.5) / -1 < 0: t = 0.1, axis 9, normal -L / |L| = (1, 1, 0) / sqrt 2: the box's
       vertical edge meets the hypotenuse.
    5, 6  A pass along +y from y = -2 with the box's +x face at x = -+ 0.5e-5 (centre x = -0.5 (1 -+ 1e-5)): axis x has w = 0 and
       pmin = 0.5 (1 -+ 1e-5) against r = 0.5, so the first passes and meets the vertex (0, 0, 0) when the +y face reaches y = 0, at
       enter = (2 - 0.5) / 1 = 1.5, axis 1, normal (0, -1, 0); the second clears the vertex and is a miss.
    7, 8  Starting across the triangle: t = 0, NONE, normal 0, with tmax = inf and with the smallest tmax.
    9, 10  Case 0 with tmax = nextafter(1.5) and with tmax = 1.5: the same contact, and the miss that carries 1.5.
    11  Away from the triangle: a miss.
    12  A point (h = 0) dropped from z = 2: a ray, t = 2, axis 2.   13  A flat box, h = (0.5, 0.5, 0): t = 2.
    Then every degenerate query; and one sphere primitive, centre (1, 2, 3), R = 0.5, against a cube of half extent 0.25, g = centre -
    c, P(t) = g - d t:
    0  from (4, 2, 3) by (-1, 0, 0): the face piece, t = (g_x + (h + R)) / d_x = (-3 + 0.75) / -1 = 2.25, normal (1, 0, 0)
    1  from (4, 2.55, 3): |P_y| = 0.55 > h, so no face; the edge along z at (-h, -h): (2.75 - t)^2 + 0.3^2 = 0.25, t = 2.35, normal
       (0.4, 0.3, 0) / 0.5
    2  from (4, 2.55, 3.55): the corner: (2.75 - t)^2 = 0.25 - 0.18, t = 2.75 - sqrt 0.07, normal (sqrt 0.07, 0.3, 0.3) / 0.5
    3  from the sphere's centre by (0, 2, 0), inside: the far corner (.., +h, ..) leaves when 2 (0.0625) + (2 t + 0.25)^2 = 0.25, t =
       (sqrt 0.125 - 0.25) / 2, normal (0.25, -sqrt 0.125, 0.25) / 0.5
    4  across the surface at the start: t = 0, NONE, normal 0.   5  moving away: a miss.   6  case 0 with tmax = 2.25: a miss."""
    tri = _one_triangle()
    nan = np.nan
    x_in, x_out = F32(-0.5 * (1 - 1e-5)), F32(-0.5 * (1 + 1e-5))
    down = [0, 0, -1]
    q = np.array([_q([0.25, 0.25, 2], 0.5, down), _q([0.25, 0.25, 2], 0.5, [0, 0, -2]), _q([0.25, 0.25, -2], 0.5, [0, 0, 1]),
                  _q([1.1, 1.1, 2], 0.5, down), _q([1.1, 1.1, 0], 0.5, [-1, -1, 0]),
                  _q([x_in, -2, 0], 0.5, [0, 1, 0]), _q([x_out, -2, 0], 0.5, [0, 1, 0]),
                  _q([0.25, 0.25, 0.3], 0.5, [0, 0, 1]), _q([0.25, 0.25, 0.3], 0.5, [0, 0, 1], 1e-38),
                  _q([0.25, 0.25, 2], 0.5, down, np.nextafter(F32(1.5), F32(2))), _q([0.25, 0.25, 2], 0.5, down, 1.5),
                  _q([0.25, 0.25, 2], 0.5, [0, 0, 1]),
                  _q([0.25, 0.25, 2], 0.0, down), _q([0.25, 0.25, 2], [0.5, 0.5, 0], down),
                  # degenerate
                  _q([nan, 0, 2], 0.5, down), _q([0, INF, 2], 0.5, down), _q([0, 0, 2], [0.5, nan, 0.5], down), _q([0, 0, 2], [0.5, 0.5, INF], down),
                  _q([0, 0, 2], [0.5, -1e-9, 0.5], down), _q([0, 0, 2], 0.5, [0, nan, -1]), _q([0, 0, 2], 0.5, [0, INF, -1]),
                  _q([0, 0, 2], 0.5, [0, 0, 0]), _q([0, 0, 2], 0.5, [0, -0.0, 0]),
                  _q([0, 0, 2], 0.5, down, nan), _q([0, 0, 2], 0.5, down, 0), _q([0, 0, 2], 0.5, down, -0.0), _q([0, 0, 2], 0.5, down, -1)], F32)
    rec = sb.brute_force(tri, q).view(T.BOX_SWEEP_HIT).reshape(-1)
    hits = [0, 1, 2, 4, 5, 7, 8, 9, 12, 13]
    assert (rec["prim_id"][hits] == 0).all() and (rec["material_id"][hits] == tri.triangles["material_id"][0]).all() and not rec["_reserved"].any()
    np.testing.assert_array_equal(rec["t"][[0, 1, 2, 5, 7, 8, 9, 12, 13]], np.array([1.5, 0.75, 1.5, 1.5, 0, 0, 1.5, 2, 2], F32))
    assert rec["axis"][[0, 1, 2, 5, 7, 8, 9, 12, 13]].tolist() == [2, 2, 2, 1, NONE, NONE, 2, 2, 2]
    np.testing.assert_array_equal(rec["normal"][[0, 1, 2, 5, 7, 8, 9, 12, 13]],
                                  [[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, -1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 1], [0, 0, 1]])
    assert not np.signbit(rec["normal"]).any() or (rec["normal"][np.signbit(rec["normal"])] != 0).all(), "no -0 in a normal"
    np.testing.assert_allclose(rec["t"][4], 0.1, rtol=1e-6)
    assert rec["axis"][4] == 9
    np.testing.assert_allclose(rec["normal"][4], [np.sqrt(0.5), np.sqrt(0.5), 0], rtol=1e-6)
    misses = [3, 6, 10, 11] + list(range(14, len(q)))
    miss = rec[misses]
    assert (miss["prim_id"] == sb.PRIM_MISS).all() and (miss["axis"] == NONE).all() and not miss["normal"].any() and not miss["material_id"].any()
    assert miss["t"].tobytes() == q[misses, 11].tobytes(), "tmax as given, bit for bit"
    assert sb.valid(q).tolist() == [True] * 14 + [False] * 13
    # the drop past the hypotenuse: every axis but 9 lets it through
    t_flat = sb.brute_force(tri, np.array([_q([0.6, 0.6, 2], 0.5, down)], F32)).view(T.BOX_SWEEP_HIT)["t"]
    assert t_flat[0] == 1.5, "the same drop with the corner at (0.1, 0.1) lands"

    sph = dataclasses.replace(tri, vertices=tri.vertices[:0], triangles=tri.triangles[:0], spheres=np.array([((1, 2, 3), 0.5, 4)], T.SPHERE))
    q = np.array([_q([4, 2, 3], 0.25, [-1, 0, 0]), _q([4, 2.55, 3], 0.25, [-1, 0, 0]), _q([4, 2.55, 3.55], 0.25, [-1, 0, 0]),
                  _q([1, 2, 3], 0.25, [0, 2, 0]), _q([1.5, 2, 3.1], 0.25, [0, 0, 1]), _q([4, 2, 3], 0.25, [1, 0, 0]),
                  _q([4, 2, 3], 0.25, [-1, 0, 0], 2.25)], F32)
    rec = sb.brute_force(sph, q).view(T.BOX_SWEEP_HIT).reshape(-1)
    assert rec["t"][0] == 2.25 and rec["t"][4] == 0 and rec["t"][5] == INF and rec["t"][6] == 2.25
    np.testing.assert_allclose(rec["t"][1:4], [2.35, 2.75 - np.sqrt(0.07), (np.sqrt(0.125) - 0.25) / 2], rtol=2e-6)
    np.testing.assert_array_equal(rec["normal"][[0, 4, 5, 6]], [[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    np.testing.assert_allclose(rec["normal"][1:4], [[0.8, 0.6, 0], [np.sqrt(0.07) / 0.5, 0.6, 0.6], [0.5, -np.sqrt(0.125) / 0.5, 0.5]], rtol=1e-5, atol=1e-7)
    assert rec["axis"].tolist() == [13, 13, 13, 13, NONE, NONE, NONE]
    assert (rec["prim_id"][:5] == sb.SPHERE_FLAG).all() and (rec["material_id"][:5] == 4).all()
    assert (rec["prim_id"][5:] == sb.PRIM_MISS).all() and not rec["material_id"][5:].any()


def test_contact_at_the_start_is_the_overlap_statement():
    """t = 0 with RT_SWEEP_AXIS_NONE exactly where rt_overlap_box's float32 statement says the box touches the primitive, pair by pair."""
    import overlap_cases as oc
    scene = scenes.random_soup(3000, n_spheres=3)
    sweeps = sb.five_kinds(scene, 640, 7)
    touch = oc.touching(scene, np.ascontiguousarray(sweeps[:, 0:8]))
    t_tri = sb.triangle_times_all(scene, sweeps)
    c, h, d = (np.ascontiguousarray(sweeps[:, k:k + 3]) for k in (0, 4, 8))
    t_sph = sb.sphere_times(np.ascontiguousarray(scene.spheres["center"], F32), scene.spheres["radius"].astype(F32), c, h, d)
    n_s = len(scene.spheres)
    assert touch[:, n_s:].sum() > 500
    np.testing.assert_array_equal(t_tri == 0, touch[:, n_s:])
    assert (t_sph[touch[:, :n_s]] == 0).all()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_box_sweeps_and_split_box_sweep_hits(rt_api):
    sw = rt_api.make_box_sweeps([[1, 2, 3], [4, 5, 6]], 0.5, np.array([[0, 0, 1], [0, 1, 0]], np.float64))
    assert sw.dtype == np.float32 and sw.shape == (2, 12) and sw.flags.c_contiguous
    np.testing.assert_array_equal(sw, [[1, 2, 3, 0, 0.5, 0.5, 0.5, 0, 0, 0, 1, INF], [4, 5, 6, 0, 0.5, 0.5, 0.5, 0, 0, 1, 0, INF]])
    sw = rt_api.make_box_sweeps(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0.5]]), np.ones((2, 3)), tmax=np.array([1.0, 3.0]))
    rec = sw.view(T.BOX_SWEEP).reshape(-1)
    assert rec["half_extent"].tolist() == [[1, 2, 3], [0, 0, 0.5]] and rec["tmax"].tolist() == [1.0, 3.0] and rec["direction"].tolist() == [[1, 1, 1]] * 2
    np.testing.assert_array_equal(sw[:, 0:8], rt_api.make_boxes(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0.5]])))
    rec = np.zeros(2, T.BOX_SWEEP_HIT)
    rec["normal"], rec["t"], rec["axis"] = [[0, 0, 1], [0, 0, 0]], [0.5, 7], [2, NONE]
    rec["prim_id"], rec["material_id"] = [0x80000001, 0xFFFFFFFF], [3, 0]
    normal, t, axis, prim, mat = rt_api.split_box_sweep_hits(rec.view(np.float32).reshape(2, 8))
    assert prim.dtype == np.uint32 and prim.tolist() == [0x80000001, 0xFFFFFFFF] and mat.tolist() == [3, 0] and axis.tolist() == [2, NONE]
    np.testing.assert_array_equal(normal, rec["normal"])
    assert t.tolist() == [0.5, 7]


def test_make_box_sweeps_and_split_box_sweep_hits_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    sw = rt_api.make_box_sweeps(torch.tensor([[1.0, 2, 3]]), (0.5, 0.25, 0.0), torch.tensor([[0.0, 0, -1]]), tmax=2.0)
    assert sw.dtype == torch.float32 and sw.tolist() == [[1, 2, 3, 0, 0.5, 0.25, 0, 0, 0, 0, -1, 2]]
    rec = np.zeros(1, T.BOX_SWEEP_HIT)
    rec["axis"], rec["prim_id"], rec["material_id"] = NONE, 0xFFFFFFFF, 7
    axis, prim, mat = rt_api.split_box_sweep_hits(torch.from_numpy(rec.view(np.float32).reshape(1, 8).copy()))[2:]
    assert prim.dtype == torch.int64 and prim.tolist() == [0xFFFFFFFF] and mat.tolist() == [7] and axis.tolist() == [NONE]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.sweep_box
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

    def rt_sweep_box(self, h, sweeps, n, out, flags):
        self.calls.append((sweeps.value, n.value, out.value, flags.value))
        return 0


def test_sweep_box_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    sweeps = rt_api.make_box_sweeps(np.zeros((6, 3), np.float32), 0.1, np.ones((6, 3), np.float32))
    got = ctx.sweep_box(sweeps)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.sweep_box(sweeps, out=own, counters=True) is own
    assert ctx.lib.calls == [(sweeps.ctypes.data, 6, got.ctypes.data, 0), (sweeps.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS)]
