"""Posed meshes (rt_overlap_mesh, rt_sweep_mesh) without a GPU: the symbols, the prototypes and the records' layouts against the
header's static asserts, ctypes mirrors and the numpy dtypes; the posing statement in numpy (api.pose_triangles) held to float64, to
hand-worked poses bit for bit and to obb_cases' frame; the reduction in numpy (tests/posed_mesh_cases.py) on hand-worked ties; and the
walk of a group of lanes with its shared word on the host - csrc/mesh_pose_rules.h, the statements the kernels call - held to a brute
force under AddressSanitizer + UBSan (tests/check_posed_mesh.cpp, a stand-alone program)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import obb_cases as ob
import posed_mesh_cases as pm
from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
F32, F64 = np.float32, np.float64
INF, NAN = np.inf, np.nan
MISS = 0xFFFFFFFF


class RtPose(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("_pad0", C.c_uint32), ("rotation", C.c_float * 4)]


class RtPoseSweep(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("_pad0", C.c_uint32), ("rotation", C.c_float * 4), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtMeshSweepHit(C.Structure):
    _fields_ = [("normal", C.c_float * 3), ("t", C.c_float), ("axis", C.c_uint32), ("triangle", C.c_uint32), ("prim_id", C.c_uint32), ("material_id", C.c_uint32)]


MIRRORS = {"rt_pose": (RtPose, T.POSE), "rt_pose_sweep": (RtPoseSweep, T.POSE_SWEEP), "rt_mesh_sweep_hit": (RtMeshSweepHit, T.MESH_SWEEP_HIT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports and structs ------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    header = _header()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    for name in ("rt_overlap_mesh", "rt_sweep_mesh"):
        assert name in rt_api.ABI_SYMBOLS and hasattr(lib, name), name
    assert ("int rt_overlap_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose* poses, size_t n, uint32_t* pairs, uint32_t* first, "
            "uint32_t flags);") in code
    assert ("int rt_sweep_mesh(rt_ctx* ctx, const rt_query_triangle* mesh, size_t m, const rt_pose_sweep* sweeps, size_t n, rt_mesh_sweep_hit* out, "
            "uint32_t flags);") in code
    assert re.search(r"It survives rt_prepare,[^.]*rt_sweep_triangle, rt_contact_triangle, rt_overlap_mesh, rt_sweep_mesh, rt_camera_rays,", header, re.S)
    assert "#define RT_POSED_MESH_MAX 65536u" in header and rt_api.POSED_MESH_MAX == 65536
    assert header.index("Triangle contacts:") < header.index("Posed meshes:") < header.index("Geometry updates:")
    # the entries are a unit of their own; the checks and the batch stay in rt_query.cpp, which alone plans batches
    unit = open(os.path.join(CSRC, "rt_posed_query.cpp")).read()
    assert unit.count("pose_query(ctx, ") == 2 and "run_batch" not in unit and "query_plan.h" not in unit
    host = open(os.path.join(CSRC, "rt_query.cpp")).read()
    assert host.count("int pose_query(rt_ctx* ctx, ") == 1 and "rt_overlap_mesh" not in open(os.path.join(CSRC, "rt_mesh_query.cpp")).read()
    assert re.search(r"^int pose_query\(", open(os.path.join(CSRC, "rt_internal.h")).read(), re.M)
    build = open(os.path.join(ROOT, "gpu_raytracer_amd", "build.py")).read()
    assert '"posed_mesh.hip"' in build and '"rt_posed_query.cpp"' in build
    for name in ("mesh_pose_rules.h", "posed_mesh.hip", "posed_mesh.h"):
        assert "query_plan.h" not in open(os.path.join(CSRC, name)).read(), name


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "pm_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:3] == [32, 48, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtPose, f).offset for f, _ in RtPose._fields_] == [0, 12, 16]
    assert [getattr(RtPoseSweep, f).offset for f, _ in RtPoseSweep._fields_] == [0, 12, 16, 32, 44]
    assert [getattr(RtMeshSweepHit, f).offset for f, _ in RtMeshSweepHit._fields_] == [0, 12, 16, 20, 24, 28]
    assert [T.EXPECTED_SIZES[k] for k in ("POSE", "POSE_SWEEP", "MESH_SWEEP_HIT")] == [32, 48, 32]
    assert T.POSE.fields["rotation"][1] == T.OBB.fields["rotation"][1] - 16, "rt_obb's rotation after dropping the half extent"
    assert all(T.POSE_SWEEP.fields[f][1] == T.POSE.fields[f][1] for f in T.POSE.names), "an rt_pose first"
    assert [T.POSE_SWEEP.fields[f][1] - 32 for f in ("direction", "tmax")] == [T.SWEEP.fields[f][1] - 16 for f in ("direction", "tmax")], "then half an rt_sweep"
    renamed = [("triangle" if n == "_reserved" else n, T.TRIANGLE_SWEEP_HIT.fields[n][0], T.TRIANGLE_SWEEP_HIT.fields[n][1]) for n in T.TRIANGLE_SWEEP_HIT.names]
    assert [(n, T.MESH_SWEEP_HIT.fields[n][0], T.MESH_SWEEP_HIT.fields[n][1]) for n in T.MESH_SWEEP_HIT.names] == renamed and renamed[3][0] == "triangle"
    header = _header()
    for text in ("RT_STATIC_ASSERT(sizeof(rt_pose) == 32", "RT_STATIC_ASSERT(sizeof(rt_pose_sweep) == 48", "RT_STATIC_ASSERT(sizeof(rt_mesh_sweep_hit) == 32",
                 "offsetof(rt_pose, rotation) == 16", "offsetof(rt_pose_sweep, direction) == 32", "offsetof(rt_pose_sweep, tmax) == 44",
                 "offsetof(rt_mesh_sweep_hit, triangle) == 20", "offsetof(rt_mesh_sweep_hit, prim_id) == 24"):
        assert text in header, text


def test_null_context_returns_bad_arg_and_writes_nothing(rt_api):
    lib = rt_api.load()
    mesh, poses, sweeps, out = (C.c_float * 12)(), (RtPose * 1)(), (RtPoseSweep * 1)(), (RtMeshSweepHit * 1)()
    pairs, first = (C.c_uint32 * 1)(7), (C.c_uint32 * 1)(7)
    assert lib.rt_overlap_mesh(C.c_void_p(0), mesh, C.c_size_t(1), poses, C.c_size_t(1), pairs, first, C.c_uint32(0)) == -1
    assert lib.rt_sweep_mesh(C.c_void_p(0), mesh, C.c_size_t(1), sweeps, C.c_size_t(1), out, C.c_uint32(0)) == -1
    assert lib.rt_sweep_mesh(C.c_void_p(0), None, C.c_size_t(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert not any(bytes(out)) and pairs[0] == 7 and first[0] == 7


# -- the posing statement ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _word(x):
    return int(np.float32(x).view(np.uint32))


def test_posing_statement_is_the_float64_one_within_4_ulp(rt_api):
    """w_a = ((R_a0 v_0 + R_a1 v_1) + R_a2 v_2) + p_a on the frame's float32 R (held to obb_cases.frame bit for bit below, and that
    to float64 by test_obb_abi.py) is six roundings, each at most half an ulp of a product, a partial sum, p_a or the result: 3 ulp of
    the largest of those magnitudes.  Held to the float64 evaluation of the same formula within 4."""
    rng = np.random.default_rng(3)
    n = 4000
    mesh = pm.random_mesh(16, 5, edge=1.0, spread=3.0)
    q = (rng.normal(size=(n, 4)) * rng.uniform(0.01, 100, (n, 1))).astype(F32)
    p = (rng.normal(size=(n, 3)) * rng.choice([0, 0.1, 10, 1000], (n, 1))).astype(F32)
    poses = rt_api.make_poses(p, q)
    got = rt_api.pose_triangles(mesh, poses)
    assert got.shape == (n, 16, 12) and got.dtype == F32 and not got[:, :, 3::4].any()
    R, valid = rt_api.pose_frames(poses)
    assert valid.all()
    R, worst = R.astype(F64), 0.0
    for k in range(3):
        v = mesh[None, :, 4 * k:4 * k + 3].astype(F64)
        for a in range(3):
            t = [R[:, a, j, None] * v[:, :, j] for j in range(3)]
            s1 = t[0] + t[1]
            s2 = s1 + t[2]
            w = s2 + p[:, a, None].astype(F64)
            big = np.maximum.reduce([np.abs(x) for x in t + [s1, s2, w, np.broadcast_to(p[:, a, None].astype(F64), w.shape)]])
            worst = max(worst, float((np.abs(got[:, :, 4 * k + a] - w) / np.spacing(big.astype(F32)).astype(F64)).max()))
    print(f"worst error: {worst:.3f} ulp of the largest operand")
    assert worst <= 4.0


def test_posing_statement_on_hand_worked_poses(rt_api):
    """Bit for bit: the identity, (0, 0, 0, -3), a quarter turn about z given as the unnormalised (0, 0, 2, 2), and a position alone."""
    v = np.array([[[1.5, -2.25, 0.75], [-0.5, 4.0, 8.0], [3.0, 0.125, -6.5]]], F32)
    mesh = rt_api.make_triangles(v[:, 0], v[:, 1], v[:, 2])
    poses = rt_api.make_poses(np.array([[0, 0, 0], [0, 0, 0], [0, 0, 0], [10.5, -20.25, 0.0625]], F32),
                              np.array([[0, 0, 0, 1], [0, 0, 0, -3], [0, 0, 2, 2], [0, 0, 0, 1]], F32))
    got = rt_api.pose_triangles(mesh, poses)[:, 0].reshape(4, 3, 4)[:, :, :3]
    turned = np.stack([-v[0, :, 1], v[0, :, 0], v[0, :, 2]], -1)  # a quarter turn about z: (x, y, z) -> (-y, x, z)
    want = np.stack([v[0], v[0], turned, v[0] + np.array([10.5, -20.25, 0.0625], F32)])
    assert (_bits(got) == _bits(want)).all(), (got, want)
    R, valid = rt_api.pose_frames(poses)
    assert valid.all() and (R[0] == np.eye(3)).all() and (R[1] == np.eye(3)).all() and (R[2] == np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])).all()
    # a -0 component comes out +0, nothing else moves (mesh_pose_rules.h, rule 1)
    neg = rt_api.make_triangles(np.array([[-0.0, 1, 2]], F32), np.array([[3, -0.0, 4]], F32), np.array([[5, 6, 7]], F32))
    out = rt_api.pose_triangles(neg, poses[:2])
    assert (out == neg[None]).all() and not np.signbit(out).any()
    # the 48-byte record is read the same
    sweeps = rt_api.make_pose_sweeps(poses[:, 0:3], poses[:, 4:8], np.ones((4, 3), F32), 5.0)
    assert sweeps.shape == (4, 12) and (sweeps[:, :8] == poses).all() and (sweeps[:, 8:11] == 1).all() and (sweeps[:, 11] == 5).all()
    assert (_bits(rt_api.pose_triangles(mesh, sweeps)) == _bits(rt_api.pose_triangles(mesh, poses))).all()
    with pytest.raises(ValueError):
        rt_api.pose_triangles(mesh[:, :11], poses)
    with pytest.raises(ValueError):
        rt_api.pose_triangles(mesh, poses[:, :7])


def test_frame_is_the_oriented_boxes_frame_bit_for_bit(rt_api):
    q = np.concatenate([ob.rotations(512, 11), (np.random.default_rng(4).normal(size=(512, 4)) * 50).astype(F32)])
    R, valid = rt_api.pose_frames(rt_api.make_poses(np.zeros((len(q), 3), F32), q))
    R_ob, valid_ob = ob.frame(q)
    assert (_bits(R) == _bits(R_ob)).all() and (valid == valid_ob).all() and valid.all()


INVALID_POSES = pm.INVALID_POSES


def test_invalid_poses(rt_api):
    """An invalid pose is answered without a look at its triangles: the reducers give 0 pairs, no first, and the miss record with tmax
    as given, whatever the posed triangles hold - with a norm that overflows they are the mesh itself, finite and touching."""
    names = sorted(INVALID_POSES)
    poses = rt_api.make_poses(np.array([INVALID_POSES[k][0] for k in names], F32), np.array([INVALID_POSES[k][1] for k in names], F32))
    _, valid = rt_api.pose_frames(poses)
    assert not valid.any(), dict(zip(names, valid))
    assert rt_api.pose_frames(rt_api.make_poses(np.zeros((1, 3), F32), np.array([[0, 0, 1e-10, 1e-10]], F32)))[1].all(), "n = 2e-20 is valid"
    scene = scenes.cornell12()
    mesh = pm.box_hull(0.9, (0.2, 0.0, 0.0))  # its y and z faces cross the right wall
    assert (rt_api.pose_triangles(mesh, poses)[names.index("norm_overflows")] == mesh).all()
    pairs, first = pm.overlap_want(scene, mesh, poses)
    assert not pairs.any() and (first == MISS).all()
    sweeps = rt_api.make_pose_sweeps(poses[:, 0:3], poses[:, 4:8], np.array([0, -1, 0], F32), 2.5)
    rec = pm.sweep_want(scene, mesh, sweeps).view(np.uint32)
    assert (rec == np.array([0, 0, 0, _word(2.5), MISS, MISS, MISS, 0], np.uint32)).all()
    ok = rt_api.make_poses(np.zeros((1, 3), F32), np.array([[0, 0, 0, 1]], F32))
    assert pm.overlap_want(scene, mesh, ok)[0][0] > 0


# -- the reduction ------------------------------------------------------------------------------------------------------------------
def test_reducers_break_ties_as_the_contract_orders_them():
    """(bits of t, prim_id ^ 0x80000000, j): the earlier time; at equal time a sphere before a triangle, a lower scene index before a
    higher, a lower mesh triangle before a higher; misses never win; word 5 is j."""
    def rec(t, prim, axis=3, mat=9):
        return np.array([0, 1, 0, t, 0, 0, 0, 0], F32).view(np.uint32) | np.array([0, 0, 0, 0, axis, 0, prim, mat], np.uint32)
    miss = np.array([0, 0, 0, _word(INF), MISS, 0, MISS, 0], np.uint32)
    sphere2, tri5, tri7 = 0x80000002, 5, 7
    rows = np.stack([
        np.stack([rec(2.0, tri5), rec(1.0, tri7), miss, rec(1.5, sphere2)]),        # the earlier time, whatever the key
        np.stack([rec(1.0, tri5), miss, rec(1.0, sphere2), rec(1.0, sphere2)]),     # equal t: the sphere, the lower j of the two
        np.stack([miss, rec(1.0, tri7), rec(1.0, tri5), rec(1.0, tri5)]),           # equal t: the lower scene index, then the lower j
        np.stack([miss, miss, miss, miss]),
        np.stack([rec(0.0, tri5), rec(0.0, tri5), rec(0.0, tri5), rec(0.0, tri5)]),  # an invalid pose
    ]).view(F32)
    tmax = np.array([INF, INF, INF, 4.0, INF], F32)
    out = pm.reduce_sweep(rows, tmax, np.array([True, True, True, True, False])).view(np.uint32)
    assert out[:, 5].tolist() == [1, 2, 2, MISS, MISS] and out[:, 6].tolist() == [tri7, sphere2, tri5, MISS, MISS]
    assert out[3].tolist() == [0, 0, 0, _word(4.0), MISS, MISS, MISS, 0] and out[4, 3] == _word(INF)
    assert (out[0, [0, 1, 2, 3, 4, 7]] == rows.view(np.uint32)[0, 1][[0, 1, 2, 3, 4, 7]]).all()
    pairs, first = pm.reduce_overlap(np.array([[0, 3, 0, 2], [0, 0, 0, 0], [0xFFFFFFFF, 0xFFFFFFFF, 0, 1], [4, 4, 4, 4]], np.uint32),
                                     np.array([True, True, True, False]))
    assert pairs.tolist() == [5, 0, 0xFFFFFFFF, 0] and first.tolist() == [1, MISS, 0, MISS]


def test_box_hull_dropped_on_the_cornell_floor(rt_api):
    """Hand-worked: the bottom of the hull reaches the floor's two triangles at t = 0.75 exactly, and so do the bottom edges of the
    side triangles.  The record carries the lowest scene key and among equals the lowest mesh triangle."""
    scene = scenes.cornell12()
    mesh, sweeps, t, prim, triangle = pm.cornell_drop()
    per_triangle = pm.st.brute_force(scene, pm.posed_sweeps(mesh, sweeps)).view(np.uint32)
    at_t = (per_triangle[:, 3] == _word(t)) & (per_triangle[:, 6] != MISS)
    assert at_t.sum() >= 6 and at_t[[0, 1]].all() and set(per_triangle[at_t, 6].tolist()) == {0, 1}, "several triangles, both floor triangles"
    rec = pm.sweep_want(scene, mesh, sweeps)
    assert rec.view(np.uint32)[0].tolist() == [0, _word(1.0), 0, _word(t), 1, triangle, prim, int(scene.triangles["material_id"][prim])]
    # turned upside down about x (0 1 0 0 is a half turn about y; 1 0 0 0 about x): the top is the bottom now
    flipped = sweeps.copy()
    flipped[:, 4:8] = (1, 0, 0, 0)
    rec = pm.sweep_want(scene, mesh, flipped).view(np.uint32)[0]
    assert rec[3] == _word(t) and rec[5] == 2 and rec[6] == 0


def test_a_duplicated_mesh_triangle_resolves_to_the_lower_index(rt_api):
    scene = scenes.cornell12()
    mesh, sweeps, triangle = pm.duplicated_triangle(scene)
    assert (mesh[1] == mesh[2]).all()
    rec = pm.sweep_want(scene, mesh, sweeps).view(np.uint32)[0]
    assert rec[5] == triangle == 1 and rec[3] == _word(0.5) and rec[6] in (0, 1)
    pairs, first = pm.overlap_want(scene, mesh, rt_api.make_poses(np.array([[0, -1, 0]], F32), np.array([[0, 0, 0, 1]], F32)))
    assert first[0] == 1 and pairs[0] == 4, "both copies lie in the floor's plane and touch both of its triangles; the small one hangs above"


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pm") / "check_posed_mesh"
    run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                          "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_posed_mesh.cpp"),
                          os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    return str(exe)


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_lanes_equal_the_brute_force_in_every_order(checker, method, kind):
    """Meshes of 1, 2, 12 and 65 triangles: the lanes of a pose in forward, reverse and shuffled order, two at a time with their walks
    interleaved node by node and the shared word carried along, and the lanes without the word, all give the bytes of the brute
    force over every (mesh triangle, primitive) pair; the word never costs a node visit; the stacks stay inside their entries (the
    program checks every index); the overlap sums and first triangles are the brute force's."""
    for n in (1, 5, 300, 3000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        visits = re.search(r"^node visits: (\d+) with the shared word, (\d+) without", run.stdout, re.M)
        assert int(visits.group(1)) <= int(visits.group(2))
        last = re.search(r"(\d+) poses \((\d+) hit, (\d+) of them at the start, (\d+) with a tie", run.stdout)
        if n == 3000 and kind in (0, 1, 5):
            print(f"kind {kind} method {method}: {visits.group(1)} node visits with the word, {visits.group(2)} without; {last.group(0)}")
            assert int(last.group(2)) >= 40 and int(last.group(4)) >= 10 and int(visits.group(1)) < int(visits.group(2))
