"""Inside tests and signed distance (rt_inside, rt_signed_distance) without a GPU: the symbols against the header; the direction
table in its three places; the numpy float32 statement the GPU tests compare bytes with (tests/signed_distance_cases.py) held to the
analytic truth of two closed shapes for every direction, and to hand-worked cases; and what Context.inside / Context.signed_distance
validate before the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import closest_point_cases as cc
import signed_distance_cases as sd
import test_gpu_ray_queries as rq
from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
INF = np.inf
NAN = np.nan


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


# -- exports --------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in ("rt_inside", "rt_signed_distance"):
        assert name in rt_api.ABI_SYMBOLS and hasattr(lib, name)
    assert re.search(r"int rt_inside\(rt_ctx\* ctx, const rt_point_query\* points, size_t n, const rt_inside_params\* params,\s*uint8_t\* inside,\s*"
                     r"uint8_t\* votes\);", code)
    assert re.search(r"int rt_signed_distance\(rt_ctx\* ctx, const rt_point_query\* points, size_t n, const rt_inside_params\* params,\s*rt_nearest\* out,\s*"
                     r"uint8_t\* votes\);", code)
    assert re.search(r"^#define RT_INSIDE_MAX_RAYS (\d+)u", _header(), re.M).group(1) == str(rt_api.INSIDE_MAX_RAYS) == str(sd.MAX_RAYS) == "7"


def test_struct_sizes_match():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"typedef struct rt_inside_params \{\s*uint32_t rays;\s*uint32_t flags;\s*uint32_t _pad\[2\];\s*\} rt_inside_params;", code)
    assert "RT_STATIC_ASSERT(sizeof(rt_inside_params) == 16" in code
    assert T.INSIDE_PARAMS.itemsize == 16 and T.INSIDE_PARAMS.names == ("rays", "flags", "_pad")
    assert T.INSIDE_PARAMS.fields["flags"][1] == 4 and T.POINT_QUERY.itemsize == 16 and T.NEAREST.itemsize == 32


def test_the_direction_table_is_one_table(rt_api):
    block = re.search(r"^#define RT_INSIDE_DIRECTIONS \\\n((?:.*\\\n)*.*)\n", _header(), re.M).group(1)
    table = np.array([float(x) for x in re.findall(r"(-?\d+\.\d+)f", block)], F32).reshape(-1, 3)
    assert table.shape == (7, 3)
    assert rt_api.INSIDE_DIRECTIONS.dtype == np.float32 and rt_api.INSIDE_DIRECTIONS.shape == (7, 3)
    assert table.tobytes() == rt_api.INSIDE_DIRECTIONS.tobytes() == sd.DIRECTIONS.tobytes()
    assert (table != 0).all(), "no zero component"
    length = np.linalg.norm(table.astype(np.float64), axis=1)
    assert (np.abs(length - 1.0) < 1e-3).all(), "roughly unit length"


def test_the_survives_sentence_names_both_calls():
    h = _header()
    assert re.search(r"It survives rt_prepare,[^.]*rt_closest_point_all, rt_inside, rt_signed_distance,", h, re.S)
    # what the older tests read in that sentence
    assert re.search(r"It survives rt_prepare,[^.]*rt_closest_point, rt_closest_point_all,", h, re.S)
    for name in ("rt_closest_point", "rt_sweep_sphere", "rt_radiance", "rt_radiance_sh", "rt_irradiance"):
        assert re.search(r"It survives rt_prepare,[^.]*" + name, h, re.S), name


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    points, params = (C.c_float * 4)(), (C.c_uint32 * 4)(3, 0, 0, 0)
    inside, votes, out = (C.c_uint8 * 1)(), (C.c_uint8 * 1)(), (C.c_float * 8)()
    assert lib.rt_inside(C.c_void_p(0), points, C.c_size_t(1), params, inside, votes) == -1
    assert lib.rt_signed_distance(C.c_void_p(0), points, C.c_size_t(1), params, out, votes) == -1
    assert lib.rt_inside(C.c_void_p(0), None, C.c_size_t(0), None, None, None) == -1
    assert not any(bytes(inside)) and not any(bytes(votes)) and not any(bytes(out))


# -- the statement --------------------------------------------------------------------------------------------------------------
def test_the_restated_triangle_test_is_the_ray_queries(rt_api):
    rng = np.random.default_rng(21)
    v0, e1, e2 = (rng.normal(0, 1, (1, 257, 3)).astype(F32) for _ in range(3))
    e2[0, :8] = e1[0, :8]  # degenerate: a = 0
    o, d = rng.normal(0, 2, (129, 1, 3)).astype(F32), rng.normal(0, 1, (129, 1, 3)).astype(F32)
    mine, theirs = sd.moller_trumbore(v0, e1, e2, o, d), rq._moller_trumbore(v0, e1, e2, o, d)
    assert mine[0].any() and not mine[0].all()
    for a, b in zip(mine, theirs):
        assert a.shape == b.shape == (129, 257) and a.tobytes() == b.tobytes()
    mine, theirs = sd.moller_trumbore(v0, e1, e2, o, sd.DIRECTIONS[2][None, None, :]), rq._moller_trumbore(v0, e1, e2, o, np.broadcast_to(sd.DIRECTIONS[2], (129, 1, 3)))
    for a, b in zip(mine, theirs):
        assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def shape_points():
    return sd.closed_shape_points(5)


def test_every_direction_gives_the_boxes_analytic_answer(shape_points):
    """6126 points farther than 1e-3 from the box's surface, 1342 of them inside: no wrong vote in any direction."""
    p = shape_points[0]
    truth = sd.box_inside(p)
    assert (len(p), int(truth.sum())) == (6126, 1342)
    counts = sd.crossings(sd.make_scene("box", [sd.box_mesh()]), p)
    for k in range(7):
        assert ((counts[:, k] & 1) != 0).tolist() == truth.tolist(), f"direction {k}"
    assert counts.max() == 2 and (counts[truth] == 1).all(), "a convex solid: one crossing from inside, none or two from outside"


def test_every_direction_gives_the_torus_analytic_answer(shape_points):
    """3871 points farther than 0.02 from the smooth torus, 935 of them inside: no wrong vote in any direction."""
    p = shape_points[1]
    truth = sd.torus_inside(p)
    assert (len(p), int(truth.sum())) == (3871, 935)
    scene = sd.make_scene("torus", [sd.torus_mesh()])
    assert len(scene.triangles) == 2304 and len(scene.vertices) == 48 * 24
    counts = sd.crossings(scene, p)
    for k in range(7):
        assert ((counts[:, k] & 1) != 0).tolist() == truth.tolist(), f"direction {k}"
    assert counts.max() == 4 and (counts == 3).any(), "rays that pass through the tube twice"
    for rays in sd.RAYS:
        for with_votes in (False, True):
            inside, votes, traced = sd.statement(scene, cc_points(p), rays, with_votes, counts=counts)
            assert inside.tolist() == truth.tolist() and votes.tolist() == (truth * rays).tolist()
            assert traced.tolist() == [rays if with_votes else rays // 2 + 1] * len(p), "unanimous votes stop at the majority"


def cc_points(positions, radius=INF):
    out = np.empty((len(positions), 4), F32)
    out[:, :3], out[:, 3] = positions, radius
    return out


def test_the_box_has_188_triangles_as_scenes_box_builds_it():
    v, t = sd.box_mesh()
    assert len(t) == 188 and len(v) == 2 * (5 * 6 + 5 * 4 + 6 * 4), "per-face vertices"
    assert len(sd.box_mesh(open_top=True)[1]) == 188 - 40
    top = v[np.setdiff1d(t.ravel(), sd.box_mesh(open_top=True)[1].ravel())]
    assert (top[:, 1] == sd.BOX_HI[1]).all(), "the face left out is y = hi"


def test_a_tetrahedron():
    scene = sd.make_scene("tetrahedron", [sd.tetrahedron_mesh()])
    p = np.array([[0.1, 0.1, 0.1], [0.2, 0.3, 0.25], [0.05, 0.05, 0.8], [0.5, 0.5, 0.5], [-0.1, 0.2, 0.2], [2, 2, 2], [0.3, -0.2, 0.3], [-1, -1, -1]], F32)
    truth = [True, True, True, False, False, False, False, False]
    counts = sd.crossings(scene, p)
    assert ((counts & 1) != 0).tolist() == [[t] * 7 for t in truth]
    for rays in sd.RAYS:
        inside, votes, traced = sd.statement(scene, cc_points(p), rays, True)
        assert inside.tolist() == truth and votes.tolist() == [rays * t for t in truth] and traced.tolist() == [rays] * len(p)


def test_a_box_without_its_top_splits_the_votes():
    """From inside a convex box a ray crosses exactly the face it leaves through, so with the top removed vote k is odd iff direction k
    leaves through another face: (0, 0.45, 0) loses its first two votes and is outside after two rays, (0, 0.45, 0.45) votes 0 1 1."""
    scene = sd.make_scene("open box", [sd.box_mesh(open_top=True)])
    p = np.array([[0, 0.45, 0], [0, 0.45, 0.45], [1.2, -0.4, 0], [0.1, 0.0, -0.1]], F32)
    want = np.zeros((len(p), 7), bool)
    for k in range(7):
        axis, side = sd.box_exit_face(p, sd.DIRECTIONS[k])
        want[:, k] = ~((axis == 1) & (side == 1))
    counts = sd.crossings(scene, p)
    assert ((counts & 1) != 0).tolist() == want.tolist() and counts.max() == 1
    assert want[0, :3].tolist() == [False, False, True] and want[1, :3].tolist() == [False, True, True] and want[2, :2].tolist() == [True, True]
    inside, votes, traced = sd.statement(scene, cc_points(p), 3, False)
    assert inside[:3].tolist() == [False, True, True] and traced[:3].tolist() == [2, 3, 2]
    inside, votes, traced = sd.statement(scene, cc_points(p), 3, True)
    assert inside[:3].tolist() == [False, True, True] and votes[:3].tolist() == [1, 2, int(want[2, :3].sum())] and traced.tolist() == [3] * 4
    assert 0 < votes[0] < 3 and 0 < votes[1] < 3, "how a caller sees that the surface is not closed"
    inside1, _, _ = sd.statement(scene, cc_points(p), 1, True)
    assert inside1[:2].tolist() == [False, False], "one ray says what direction 0 says"


def test_the_stop_rule_counts_rays():
    parity = np.array([[0, 0, 1, 1, 1, 1, 1], [0, 1, 0, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0, 0]], np.uint32)
    yes, no = np.ones(4, bool), np.zeros(4, bool)
    inside, votes, traced = sd.vote(parity, 3, yes, no, False)
    assert traced.tolist() == [2, 3, 2, 3] and inside.tolist() == [False, False, True, True] and votes.tolist() == [1, 1, 2, 2]
    inside_v, votes_v, traced_v = sd.vote(parity, 3, yes, no, True)
    assert traced_v.tolist() == [3] * 4 and inside_v.tolist() == inside.tolist() and votes_v.tolist() == votes.tolist()
    assert sd.vote(parity, 1, yes, no, False)[2].tolist() == [1] * 4
    # four of seven and three of five are reached at the sixth and the fifth ray by these rows; a unanimous row stops at 4 and 3
    assert sd.vote(parity, 7, yes, no, False)[2].tolist() == [6, 6, 6, 6] and sd.vote(parity, 7, yes, no, False)[0].tolist() == [True, True, False, False]
    assert sd.vote(parity, 5, yes, no, False)[2].tolist() == [5, 5, 5, 5] and sd.vote(parity, 5, yes, no, False)[0].tolist() == [True, True, False, False]
    same = np.array([[1] * 7, [0] * 7, [1, 1, 1, 0, 1, 0, 0]], np.uint32)
    assert [sd.vote(same, r, yes[:3], no[:3], False)[2].tolist() for r in (1, 3, 5, 7)] == [[1, 1, 1], [2, 2, 2], [3, 3, 3], [4, 4, 5]]
    # inside a sphere: nothing traced without votes, everything with
    assert sd.vote(parity, 3, yes, yes, False)[2].tolist() == [0] * 4 and sd.vote(parity, 3, yes, yes, False)[0].all()
    assert sd.vote(parity, 3, yes, yes, True)[2].tolist() == [3] * 4 and sd.vote(parity, 3, yes, yes, True)[1].tolist() == [1, 1, 2, 2]
    # an invalid point: outside, no votes, nothing traced, sphere or not
    for with_votes in (False, True):
        assert [a.tolist() for a in sd.vote(parity, 3, no, yes, with_votes)] == [[False] * 4, [0] * 4, [0] * 4]


def test_spheres_are_a_union_with_the_triangles():
    scene = sd.make_scene("box and sphere", [sd.box_mesh()], [((3.0, 0.0, 0.0), 0.5), ((1.25, 0.0, 0.0), 0.4)])
    p = cc_points(np.array([[3.1, 0, 0], [3.0, 0, 0], [3.5, 0, 0], [3.6, 0, 0], [1.4, 0, 0], [1.0, 0, 0], [0, 0, 0], [0, 2, 0]], F32))
    assert sd.sphere_inside(scene, p[:, :3]).tolist() == [True, True, False, False, True, True, False, False], "strictly inside: not on the surface"
    inside, votes, traced = sd.statement(scene, p, 3, False)
    assert inside.tolist() == [True, True, False, False, True, True, True, False]
    assert traced.tolist() == [0, 0, 2, 2, 0, 0, 2, 2]
    inside, votes, traced = sd.statement(scene, p, 3, True)
    assert inside.tolist() == [True, True, False, False, True, True, True, False]
    assert votes.tolist() == [0, 0, 0, 0, 0, 3, 3, 0] and traced.tolist() == [3] * 8, "spheres cast no vote"


def test_degenerate_queries_and_the_truncated_field():
    scene = sd.make_scene("box", [sd.box_mesh()])
    centre = [0.125, 0.0, -0.125]
    q = np.array([[NAN, 0, 0, 1], [0, INF, 0, 1], [0, 0, -INF, INF], centre + [NAN], centre + [0.0], centre + [-1.0],
                  centre + [0.1], [5, 5, 5, 0.1], centre + [INF], [0.125, 0.3, -0.125, 0.25]], F32)
    inside, votes, traced = sd.statement(scene, q, 3, True)  # rt_inside: the radius is ignored
    assert inside.tolist() == [False] * 3 + [True] * 4 + [False, True, True] and votes.tolist() == [0] * 3 + [3] * 4 + [0, 3, 3]
    assert traced.tolist() == [0] * 3 + [3] * 7
    rec, votes, traced = sd.signed_records(scene, q, 3, True)
    r = rec.view(T.NEAREST).reshape(-1)
    assert votes.tolist() == [0] * 6 + [3, 0, 3, 3] and traced.tolist() == [0] * 6 + [3] * 4
    assert rec[:6].tobytes() == cc.brute_force(scene, q[:6]).tobytes(), "degenerate by rt_closest_point's rules: its unsigned miss record"
    assert r["prim_id"][:8].tolist() == [cc.PRIM_MISS] * 8
    assert r["distance"][6:8].tolist() == [F32(-0.1), F32(0.1)], "a miss within a finite radius: -radius inside, +radius outside"
    assert abs(r["distance"][8] + 0.5) < 1e-6 and abs(r["distance"][9] + 0.2) < 1e-6 and r["prim_id"][9] != cc.PRIM_MISS, "the nearest face, negative"
    unsigned = cc.brute_force(scene, q)
    assert (rec.view(np.uint32) ^ unsigned.view(np.uint32))[:, [0, 1, 2, 4, 5, 6, 7]].max() == 0, "only the distance's sign differs"
    assert sd.sign(unsigned[8:9], np.array([False])).tobytes() == unsigned[8:9].tobytes()


def test_inside_rays_are_the_statements_rays():
    p = np.array([[1, 2, 3], [-1, 0, 0.5]], F32)
    r = sd.inside_rays(p)
    assert r.shape == (7, 2, 8) and r.dtype == np.float32
    assert (r[:, :, 3] == sd.MIN_T).all() and np.isposinf(r[:, :, 7]).all()
    assert r[3, 1, :3].tolist() == p[1].tolist() and r[3, 1, 4:7].tobytes() == sd.DIRECTIONS[3].tobytes()


# -- Context.inside / Context.signed_distance -------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


@pytest.mark.parametrize("method", ["inside", "signed_distance"])
def test_rays_and_batches_are_validated_in_python(rt_api, method):
    nc = _no_context(rt_api)
    call = getattr(rt_api.Context, method)
    good = np.zeros((4, 4), F32)
    for rays in (0, 2, 4, 8, True, 3.0, -1, 9, None, "3"):
        with pytest.raises(ValueError, match="rays"):
            call(nc, good, rays=rays)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="points: shape"):
        call(nc, np.zeros((4, 3), F32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 4), F32)[::2])
    with pytest.raises(TypeError, match="votes"):
        call(nc, good, votes=np.zeros(4, np.uint32))
    with pytest.raises(ValueError, match="votes: 5 rows"):
        call(nc, good, votes=np.zeros(5, np.uint8))
    with pytest.raises((TypeError, ValueError), match="out"):
        call(nc, good, out=np.zeros((4, 8) if method == "inside" else (4,), F32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def _record(self, name, h, points, n, params, out, votes):
        p = np.frombuffer(C.string_at(params.value, 16), np.uint32)
        self.calls.append((name, points.value, n.value, p.tolist(), out.value, votes.value))
        return 0

    def rt_inside(self, *a):
        return self._record("rt_inside", *a)

    def rt_signed_distance(self, *a):
        return self._record("rt_signed_distance", *a)


def test_the_calls_pass_their_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    points = rt_api.make_points(np.zeros((6, 3), F32))
    inside = ctx.inside(points)
    assert inside.shape == (6,) and inside.dtype == np.bool_
    own, own_votes = np.zeros(6, bool), np.zeros(6, np.uint8)
    got = ctx.inside(points, rays=np.int64(7), out=own, votes=own_votes, counters=True)
    assert got[0] is own and got[1] is own_votes
    rec, votes = ctx.signed_distance(points, rays=5, votes=True)
    assert rec.shape == (6, 8) and rec.dtype == np.float32 and votes.shape == (6,) and votes.dtype == np.uint8
    rec1 = ctx.signed_distance(points, rays=1)
    P = points.ctypes.data
    assert ctx.lib.calls == [("rt_inside", P, 6, [3, 0, 0, 0], inside.ctypes.data, None),
                             ("rt_inside", P, 6, [7, rt_api.QUERY_COUNTERS, 0, 0], own.ctypes.data, own_votes.ctypes.data),
                             ("rt_signed_distance", P, 6, [5, 0, 0, 0], rec.ctypes.data, votes.ctypes.data),
                             ("rt_signed_distance", P, 6, [1, 0, 0, 0], rec1.ctypes.data, None)]
