"""Oriented boxes (rt_overlap_obb, rt_sweep_obb) without a GPU: the symbols and the record layouts against the header's static asserts
and the numpy dtypes; both walks on the host - csrc/obb_rules.h, the statements the kernels call - held to a brute force under
AddressSanitizer + UBSan (tests/check_obb.cpp, a stand-alone program); the numpy float32 statements the GPU tests compare bytes with
(tests/obb_cases.py) held to the axis-aligned statements at the identity, to the same statement in float64, and to the axis-aligned
answer of the turned extents at a quarter turn; and what Context.overlap_obb / sweep_obb validate before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import obb_cases as ob
import overlap_cases as oc
import sweep_box_cases as sb
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32 = np.float32
F64 = np.float64
INF = np.inf


class RtObb(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("_pad0", C.c_uint32), ("half_extent", C.c_float * 3), ("_pad1", C.c_uint32), ("rotation", C.c_float * 4)]


class RtObbSweep(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("_pad0", C.c_uint32), ("half_extent", C.c_float * 3), ("_pad1", C.c_uint32), ("rotation", C.c_float * 4),
                ("direction", C.c_float * 3), ("tmax", C.c_float)]


MIRRORS = {"rt_obb": (RtObb, T.OBB), "rt_obb_sweep": (RtObbSweep, T.OBB_SWEEP)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("rt_overlap_obb", "rt_sweep_obb"):
        assert name in rt_api.ABI_SYMBOLS and hasattr(lib, name)
    assert re.search(r"int rt_sweep_obb\(rt_ctx\* ctx, const rt_obb_sweep\* sweeps, size_t n, rt_box_sweep_hit\* out, uint32_t flags\);", code)
    assert re.search(r"int rt_overlap_obb\(rt_ctx\* ctx, const rt_obb\* boxes, size_t n, uint32_t max_prims,\s*uint32_t\* prims,\s*uint32_t\* counts,\s*"
                     r"uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_contact_capsule, rt_overlap_obb, rt_sweep_obb,", _header(), re.S), "listed among the calls a running image survives"
    assert _header().index("Contact queries:") < _header().index("Oriented boxes:") < _header().index("Geometry updates:")


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "obb_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [48, 64]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtObb, f).offset for f in ("center", "_pad0", "half_extent", "_pad1", "rotation")] == [0, 12, 16, 28, 32]
    assert [getattr(RtObbSweep, f).offset for f in ("center", "half_extent", "rotation", "direction", "tmax")] == [0, 16, 32, 48, 60]
    assert T.EXPECTED_SIZES["OBB"] == 48 and T.EXPECTED_SIZES["OBB_SWEEP"] == 64
    assert [T.OBB.fields[f][1] for f in ("center", "half_extent")] == [T.BOX.fields[f][1] for f in ("center", "half_extent")], "an rt_box first"
    assert [T.OBB_SWEEP.fields[f][1] for f in T.OBB.names] == [T.OBB.fields[f][1] for f in T.OBB.names], "an rt_obb first"
    header = _header()  # the header asserts them itself
    for text in ("RT_STATIC_ASSERT(sizeof(rt_obb) == 48", "RT_STATIC_ASSERT(sizeof(rt_obb_sweep) == 64", "offsetof(rt_obb, rotation) == 32",
                 "offsetof(rt_obb_sweep, rotation) == 32", "offsetof(rt_obb_sweep, direction) == 48", "offsetof(rt_obb_sweep, tmax) == 60"):
        assert text in header, text


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    sweeps, out, boxes, ids = (RtObbSweep * 1)(), (C.c_uint32 * 8)(), (RtObb * 1)(), (C.c_uint32 * 4)()
    assert lib.rt_sweep_obb(C.c_void_p(0), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_obb(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert lib.rt_overlap_obb(C.c_void_p(0), boxes, C.c_size_t(1), C.c_uint32(4), ids, None, C.c_uint32(0)) == -1
    assert not any(bytes(out)) and not any(bytes(ids))


def test_query_plan_has_no_new_user_and_the_overlap_body_is_written_once():
    for name in ("obb_rules.h", "overlap_obb.hip", "overlap_obb.h", "sweep_obb.hip", "sweep_obb.h"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name
    host = open(os.path.join(CSRC, "rt_query.cpp")).read()
    assert host.count("RT_OVERLAP_ANY needs max_prims 0") == 1 and host.count("overlap_query(ctx, ") == 2


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
def _build_checker(exe, *defines):
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          *defines, "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_obb.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build_checker(tmp_path_factory.mktemp("obb") / "check_obb")


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walks_equal_the_brute_force(checker, method, kind):
    """Every answer of both walks - the world bound, order, stack, the frame's leaf tests and their early returns as the kernels run
    them - has the bytes of the brute force; the sweep's (t = 0, NONE) is the overlap's statement pair by pair; the exact identity gives
    the axis-aligned statements' bytes; and the stacks stay inside the entries the launches provide (the program checks every index)."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        assert re.search(r"start in contact: 0 pairs differ; identity: 0 of [1-9]\d* differ", run.stdout), run.stdout[-500:]
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walks cull (degenerate input need not)
            tests = float(re.search(r"and ([0-9.]+) triangle tests per sweep", run.stdout).group(1))
            boxes = float(re.search(r"and ([0-9.]+) triangle tests per box", run.stdout).group(1))
            assert tests < 20000 / 10 and boxes < 20000 / 10, run.stdout[-500:]
        if n == 20000 and kind == 0:  # every axis closes some contact last, and the spheres and the starts in contact are there
            counts = list(map(int, re.search(r"axes 0\.\.12, sphere, none:((?: \d+){15})", run.stdout).group(1).split()))
            assert all(c > 0 for c in counts), counts


def test_host_check_sees_a_margin_that_is_too_tight(tmp_path):
    """With the margins' signs flipped (the world half extents and the node bounds narrower by as much as they were wider, nothing
    else) the check must report wrong answers."""
    exe = _build_checker(tmp_path / "check_obb_flipped", "-DRT_SWB_SLACK=-1.0e-5f", "-DRT_CP_SLACK=-1.0e-5f", "-DRT_OBB_SLACK=-1.0e-5f")
    run = subprocess.run([exe, "20000", "1", "0", "0"], capture_output=True, text=True)
    failures = int(re.search(r", (\d+) failures$", run.stdout.strip()).group(1))
    print(run.stdout.strip().splitlines()[-1])
    assert run.returncode == 1 and failures > 0


# -- the numpy statements -----------------------------------------------------------------------------------------------------
SCENES = {"soup": lambda: scenes.random_soup(3000), "cornell12": scenes.cornell12}


def test_the_frame_of_the_header():
    """R on hand-worked quaternions: the identity for (0, 0, 0, w), bit for bit with every zero +0; a quarter turn about z takes the
    box's x axis to the world's y; a quaternion of any length gives the same rotation; validity."""
    q = np.array([[0, 0, 0, 1], [0, 0, 0, -3], [0, 0, 0, 1e-10], [0, 0, np.sqrt(0.5), np.sqrt(0.5)], [0, 0, 3, 3], [0, 0, 1e-10, 1e-10],
                  [np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, 0, 0], [0, 0, 2e19, 2e19], [1e-30, 0, 0, 1e-30], [0, 0, 0, -np.inf]], F32)
    R, ok = ob.frame(q)
    assert ok.tolist() == [True] * 6 + [False] * 6
    for k in range(3):
        assert R[k].tobytes() == np.eye(3, dtype=F32).tobytes(), "no -0 either"
    R0 = ob.frame(np.array([[-0.0, 0, -0.0, 2], [0, -0.0, 0, -1]], F32))[0]
    assert (R0 == np.eye(3, dtype=F32)).all() and np.signbit(R0).any(), "the identity in value, with some -0 off the diagonal"
    for k in (3, 4, 5):
        np.testing.assert_allclose(R[k], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=2e-7)
    u = np.array([[1, 2, 3]], F32)
    np.testing.assert_allclose(ob.back(R[3:4], u), [[-2, 1, 3]], atol=1e-6)   # the box's (1, 2, 3) in the world
    np.testing.assert_allclose(ob.into(R[3:4], u), [[2, -1, 3]], atol=1e-6)   # the world's (1, 2, 3) in the box
    np.testing.assert_allclose(ob.world_half(R[3:4], u), [[2, 1, 3]], atol=1e-6)
    rot = ob.rotations(4096, 1)
    R, ok = ob.frame(rot, F64)
    assert ok.all() and (rot[0::16] == F32(ob.IDENTITY)).all() and (rot[1::16] == F32(ob.IDENTITY)).all()
    assert not (rot[2::16] == F32(ob.IDENTITY)).all(1).all() and not (rot[3::16] == F32(ob.IDENTITY)).all(1).all()
    np.testing.assert_allclose(R @ R.transpose(0, 2, 1), np.broadcast_to(np.eye(3), R.shape), atol=1e-12)
    sine = np.linalg.norm(rot[:, 0:3].astype(F64), axis=1) / np.linalg.norm(rot.astype(F64), axis=1)  # of the half angle
    angle = 2 * np.arcsin(np.clip(sine, 0, 1))
    assert (angle[2::16] <= 1e-3).all() and (angle[3::16] <= 1e-3).all() and (angle[2::16] > 0).any() and np.median(angle[4::16]) > 1.0


@pytest.mark.parametrize("name", sorted(SCENES))
@pytest.mark.parametrize("rotation", [(0, 0, 0, 1), (0, 0, 0, -3), (-0.0, 0, -0.0, 2), (0, -0.0, 0, -1)], ids=["w1", "w-3", "x-0_z-0_w2", "y-0_w-1"])
def test_identity_rotation_gives_the_axis_aligned_statements_bytes(name, rotation):
    """Consequence (a) of the header between the two numpy statements, before any GPU run: with R exactly the identity the oriented
    statement's records, lists and counts are the axis-aligned ones', byte for byte - signs of zeros included; with a -0 among x, y,
    z some off-diagonal entries of R are -0, which moves no output bit either."""
    scene = scenes.random_soup(3000, n_spheres=3) if name == "soup" else SCENES[name]()
    box = sb.five_kinds(scene, 640, 7)
    if name == "cornell12":
        box = np.concatenate([box, sb.cube_sweeps(3)])  # -0 direction components, faces in the walls' planes
    box[::3, 11] = 0.5
    sweeps = ob.with_rotation(box, rotation)
    got, want = ob.brute_force(scene, sweeps), sb.brute_force(scene, box)
    assert got.tobytes() == want.tobytes()
    kinds = sb.contact_kinds(want)
    assert kinds[0].any() and kinds[4].any() and kinds[5].any() and (name != "soup" or all(k.any() for k in kinds))
    boxes = np.ascontiguousarray(box[:, 0:8])
    touch = oc.touching(scene, boxes)
    assert touch.sum() > 500
    np.testing.assert_array_equal(ob.touching(scene, np.ascontiguousarray(sweeps[:, 0:12])), touch)
    for got_part, want_part in zip(ob.overlap_all(scene, np.ascontiguousarray(sweeps[:, 0:12]), 4), oc.overlap_all(scene, boxes, 4)):
        assert got_part.tobytes() == want_part.tobytes()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_float32_statement_lies_between_the_float64_ones_of_a_larger_and_a_smaller_box(name):
    """sweep_box_cases' sandwich for the turned box: t64(h + eps) <= t32 <= t64(h - eps), a miss counting as +inf, relative slack 1e-6 on
    finite t, eps = k x the scene's diagonal, k = twice obb_cases.K_MEASURED, over every one of five_kinds(scene, 4096, 11) whose
    extents are all >= 1e-3 x the diagonal.  The float64 statement computes R in float64 from the same f32 quaternion."""
    scene = SCENES[name]()
    sweeps = ob.five_kinds(scene, 4096, 11)
    sweeps = sweeps[ob.full_extents(scene, sweeps)]
    assert len(sweeps) == 3586
    k = 2 * ob.K_MEASURED[name]
    assert k <= 1e-4
    eps = k * ob.diagonal(scene)
    t32 = ob.times(scene, sweeps, F32).astype(F64)
    lower, upper = ob.times(scene, sweeps, F64, eps), ob.times(scene, sweeps, F64, -eps)
    bad = (lower * (1 - 1e-6) > t32) | (t32 > upper * (1 + 1e-6))
    hit = np.isfinite(t32)
    print(f"{name}: {int(bad.sum())} of {len(sweeps)} outside the sandwich at k = {k:.1e}; {hit.mean():.0%} hit, {(t32 == 0).mean():.0%} in contact at the start")
    assert hit.sum() > 2000 and (~hit).sum() > 150 and (t32 == 0).sum() > 600
    assert not bad.any(), (sweeps[bad][:4], t32[bad][:4], lower[bad][:4], upper[bad][:4])
    rec = ob.brute_force(scene, sweeps[::8])  # brute_force's times are those of the float32 statement
    np.testing.assert_array_equal(rec[:, 3], t32[::8].astype(F32))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_quarter_turn_about_z_is_the_axis_aligned_box_with_x_and_y_exchanged(name):
    """rotation = (0, 0, sqrt 1/2, sqrt 1/2) of a box with h = (a, b, c) gives, within K, the axis-aligned answer with h = (b, a, c),
    over every one of five_kinds(scene, 4096, 11) with all extents >= 1e-3 x the diagonal (3586, all five kinds, none left out):
      1  t64_aligned(h' + eps) <= t32_oriented <= t64_aligned(h' - eps), eps = twice K_MEASURED x the diagonal, relative slack 1e-6;
      2  for EVERY hit the oriented winner is one of the axis-aligned candidates whose float64 time is within thr = 2 K_MEASURED diag /
         |d| of the first; where the margin between the first and the second candidate exceeds thr (a CLEAR hit) that is the issue's
         "the same primitive wins", asserted as such; where it does not, the winner is one of the tied candidates;
      3  the hits that are not clear are exact ties and nothing else: their margin is 0.0 in float64 - a start pose that touches two or
         more triangles (both at t = 0), or the two coplanar triangles of a cornell12 wall met at the same time - so of the hits whose
         first two candidates do not tie exactly at least 90 % must be clear (measured: all of them, on both scenes).
    Where this departs from the issue: it asks that at least 90 % of ALL hits keep a clear margin.  On these sweeps 75.0 % do on the soup
    (2365 of 3152; the other 787 start in contact with two or more triangles) and 61.4 % on cornell12 (1874 of 3053; 339 such starts
    and 840 moving contacts with both triangles of a wall): an exact tie has no margin whatever K is, so that share measures the
    input, not the statement.  Both shares are printed; rule 2 checks the tied hits instead of dropping them."""
    scene = SCENES[name]()
    box = sb.five_kinds(scene, 4096, 11)
    box = box[sb.full_extents(scene, box)]
    assert len(box) == 3586
    turned = ob.with_rotation(box, F32(ob.QUARTER_Z))
    exchanged = box.copy()
    exchanged[:, 4], exchanged[:, 5] = box[:, 5], box[:, 4]
    k = 2 * ob.K_MEASURED[name]
    eps = k * ob.diagonal(scene)
    rec = ob.brute_force(scene, turned).view(T.BOX_SWEEP_HIT).reshape(-1)
    t32 = np.where(rec["prim_id"] == ob.PRIM_MISS, np.inf, rec["t"].astype(F64))
    lower, upper = sb.times(scene, exchanged, F64, eps), sb.times(scene, exchanged, F64, -eps)
    bad = (lower * (1 - 1e-6) > t32) | (t32 > upper * (1 + 1e-6))
    assert not bad.any(), (int(bad.sum()), turned[bad][:4], t32[bad][:4], lower[bad][:4], upper[bad][:4])
    aligned = sb.brute_force(scene, exchanged).view(T.BOX_SWEEP_HIT).reshape(-1)
    with np.errstate(invalid="ignore"):  # inf - inf where fewer than two triangles are ever touched
        t_all = sb.triangle_times_all(scene, exchanged, F64)
        first_two = np.sort(t_all, 1)[:, :2]
        hit = np.isfinite(first_two[:, 0])
        thr = k * ob.diagonal(scene) / np.linalg.norm(exchanged[:, 8:11].astype(F64), axis=1)
        margin = first_two[:, 1] - first_two[:, 0]
        clear, tie = hit & (margin > thr), hit & (margin == 0)
    print(f"{name}: {int(hit.sum())} hits, {int(clear.sum())} ({clear.sum() / hit.sum():.1%}) clear, {int(tie.sum())} exact ties "
          f"({int((tie & (first_two[:, 0] == 0)).sum())} of them at the start), {int((hit & ~clear & ~tie).sum())} neither")
    assert hit.sum() > 2500 and clear.sum() > 1500 and tie.sum() > 500
    rows = np.flatnonzero(hit)
    winner = rec["prim_id"][rows]
    assert (winner != ob.PRIM_MISS).all() and (winner < ob.SPHERE_FLAG).all()
    assert (t_all[rows, winner] <= first_two[rows, 0] + thr[rows]).all(), "the winner is one of the candidates within thr of the first"
    np.testing.assert_array_equal(rec["prim_id"][clear], aligned["prim_id"][clear])
    assert clear.sum() >= 0.9 * (hit & ~tie).sum()


def test_prefiltered_brute_forces_are_the_brute_forces():
    scene = scenes.random_soup(3000, n_spheres=3)
    sweeps = np.concatenate([ob.five_kinds(scene, 640, 5), ob.sphere_directed(scene, 64, 6)])
    sweeps[::3, 15] = 0.5  # a third end early: more misses
    plain, filtered = ob.brute_force(scene, sweeps), ob.brute_force(scene, sweeps, prefilter=True)
    assert plain.tobytes() == filtered.tobytes()
    assert all(kind.any() for kind in sb.contact_kinds(plain))
    boxes = np.ascontiguousarray(sweeps[:, 0:12])
    touch = ob.touching(scene, boxes)
    assert touch[:, :3].any() and touch[:, 3:].sum() > 500
    np.testing.assert_array_equal(ob.touching(scene, boxes, prefilter=True), touch)


def test_contact_at_the_start_is_the_overlap_statement():
    """Consequence (b): t = 0 with RT_SWEEP_AXIS_NONE exactly where rt_overlap_obb's float32 statement says the turned box touches the
    triangle, pair by pair; a touched sphere gives t = 0."""
    scene = scenes.random_soup(3000, n_spheres=3)
    sweeps = np.concatenate([ob.five_kinds(scene, 640, 7), ob.sphere_directed(scene, 64, 8)])
    touch = ob.touching(scene, np.ascontiguousarray(sweeps[:, 0:12]))
    t_tri = ob.triangle_times_all(scene, sweeps)
    assert touch[:, 3:].sum() > 500 and touch[:, :3].sum() > 10
    np.testing.assert_array_equal(t_tri == 0, touch[:, 3:])
    rec = ob.brute_force(scene, sweeps).view(T.BOX_SWEEP_HIT).reshape(-1)
    assert (rec["t"][touch.any(1)] == 0).all() and (rec["axis"][touch.any(1)] == ob.AXIS_NONE).all()


def test_degenerate_queries_of_the_statement():
    scene = scenes.single_triangle()
    good = ob.make_obb_sweeps([[0.1, 0.1, 2]], 0.5, (0.1, 0.2, 0.3, 0.9), [[0, 0, -1]])
    assert ob.valid(good).all() and ob.valid_boxes(good[:, :12]).all()
    for col, value in ((0, np.nan), (1, np.inf), (4, -1e-30), (5, np.nan), (8, np.nan), (9, np.inf), (11, -np.inf), (12, np.nan), (15, 0.0), (15, np.nan)):
        q = good.copy()
        q[0, col] = value
        assert not ob.valid(q).any(), (col, value)
        assert ob.valid_boxes(q[:, :12]).all() == (col >= 12), (col, value)
        rec = ob.brute_force(scene, q).view(T.BOX_SWEEP_HIT)[0]
        assert rec["prim_id"] == ob.PRIM_MISS and rec["axis"] == ob.AXIS_NONE and not rec["normal"].any() and rec["t"].tobytes() == q[0, 15].tobytes()
        assert col >= 12 or not ob.touching(scene, np.ascontiguousarray(q[:, :12])).any()
    for rot in ((0, 0, 0, 0), (0, 0, 2e19, 2e19), (1e-30, 0, 0, 1e-30)):
        q = ob.make_obb_sweeps([[0.1, 0.1, 2]], 0.5, rot, [[0, 0, -1]])
        assert not ob.valid(q).any() and not ob.valid_boxes(q[:, :12]).any()
    tiny = ob.make_obb_sweeps([[0.1, 0.1, 2]], 0.5, (0, 0, 1e-10, 1e-10), [[0, 0, -1]])
    assert ob.valid(tiny).all() and ob.valid_boxes(tiny[:, :12]).all()


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_make_obbs_and_make_obb_sweeps(rt_api):
    boxes = rt_api.make_obbs([[1, 2, 3], [4, 5, 6]], 0.5, (0, 0, 0, 1))
    assert boxes.dtype == np.float32 and boxes.shape == (2, 12) and boxes.flags.c_contiguous
    np.testing.assert_array_equal(boxes, [[1, 2, 3, 0, 0.5, 0.5, 0.5, 0, 0, 0, 0, 1], [4, 5, 6, 0, 0.5, 0.5, 0.5, 0, 0, 0, 0, 1]])
    np.testing.assert_array_equal(boxes, ob.make_obbs([[1, 2, 3], [4, 5, 6]], 0.5, (0, 0, 0, 1)))
    rot = np.array([[0, 0, 1, 1], [1, 0, 0, 0]], np.float64)
    sw = rt_api.make_obb_sweeps(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0.5]]), rot, np.ones((2, 3)), tmax=np.array([1.0, 3.0]))
    assert sw.dtype == np.float32 and sw.shape == (2, 16)
    rec = sw.view(T.OBB_SWEEP).reshape(-1)
    assert rec["half_extent"].tolist() == [[1, 2, 3], [0, 0, 0.5]] and rec["tmax"].tolist() == [1.0, 3.0] and rec["direction"].tolist() == [[1, 1, 1]] * 2
    assert rec["rotation"].tolist() == rot.tolist()
    np.testing.assert_array_equal(sw[:, 0:12], rt_api.make_obbs(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0.5]]), rot))
    np.testing.assert_array_equal(sw, ob.make_obb_sweeps(np.zeros((2, 3)), np.array([[1, 2, 3], [0, 0, 0.5]]), rot, np.ones((2, 3)), np.array([1.0, 3.0])))
    assert rt_api.make_obb_sweeps(np.zeros((1, 3)), 1.0, (0, 0, 0, 1), [[0, 0, 1]])[0, 15] == INF


def test_make_obbs_and_make_obb_sweeps_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    sw = rt_api.make_obb_sweeps(torch.tensor([[1.0, 2, 3]]), (0.5, 0.25, 0.0), (0.0, 0.5, 0.0, 0.5), torch.tensor([[0.0, 0, -1]]), tmax=2.0)
    assert sw.dtype == torch.float32 and sw.tolist() == [[1, 2, 3, 0, 0.5, 0.25, 0, 0, 0, 0.5, 0, 0.5, 0, 0, -1, 2]]
    boxes = rt_api.make_obbs(torch.tensor([[1.0, 2, 3]]), 0.5, torch.tensor([[0.0, 0, 0, 1]]))
    assert boxes.dtype == torch.float32 and boxes.tolist() == [[1, 2, 3, 0, 0.5, 0.5, 0.5, 0, 0, 0, 0, 1]]


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.sweep_obb
    good = np.zeros((4, 16), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="sweeps: shape"):
        call(nc, np.zeros((4, 12), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 16), np.float32)[::2])
    with pytest.raises(ValueError, match="rows for 4 sweeps"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    call = rt_api.Context.overlap_obb
    boxes = np.zeros((4, 12), np.float32)
    with pytest.raises(ValueError, match="boxes: shape"):
        call(nc, np.zeros((4, 8), np.float32), 4)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, boxes.astype(np.float64), 4)
    with pytest.raises(ValueError, match="max_prims"):
        call(nc, boxes, 33)
    with pytest.raises(ValueError, match="max_prims"):
        call(nc, boxes, 0)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, boxes, 4, any_hit=True)


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_sweep_obb(self, h, sweeps, n, out, flags):
        self.calls.append(("sweep", sweeps.value, n.value, out.value, flags.value))
        return 0

    def rt_overlap_obb(self, h, boxes, n, max_prims, prims, counts, flags):
        self.calls.append(("overlap", boxes.value, n.value, max_prims.value, prims.value, counts.value, flags.value))
        return 0


def test_the_calls_pass_their_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    sweeps = rt_api.make_obb_sweeps(np.zeros((6, 3), np.float32), 0.1, (0, 0, 0, 1), np.ones((6, 3), np.float32))
    got = ctx.sweep_obb(sweeps)
    assert got.shape == (6, 8) and got.dtype == np.float32
    own = np.zeros((6, 8), np.float32)
    assert ctx.sweep_obb(sweeps, out=own, counters=True) is own
    boxes = np.ascontiguousarray(sweeps[:, :12])
    ids, counts = ctx.overlap_obb(boxes, 4, count_all=True)
    assert ids.shape == (6, 4) and ids.dtype == np.uint32 and counts.shape == (6,) and counts.dtype == np.uint32
    none, occupied = ctx.overlap_obb(boxes, 0, any_hit=True, counters=True)
    assert none is None
    assert ctx.lib.calls == [("sweep", sweeps.ctypes.data, 6, got.ctypes.data, 0), ("sweep", sweeps.ctypes.data, 6, own.ctypes.data, rt_api.QUERY_COUNTERS),
                             ("overlap", boxes.ctypes.data, 6, 4, ids.ctypes.data, counts.ctypes.data, rt_api.QUERY_COUNT_ALL),
                             ("overlap", boxes.ctypes.data, 6, 0, None, occupied.ctypes.data, rt_api.OVERLAP_ANY | rt_api.QUERY_COUNTERS)]
