"""Contact queries (rt_contact_capsule) without a GPU: the symbol, the constants and the structs against the header; the statement, the
list and the whole walk on the host - csrc/contact_capsule_rules.h, the statements the kernel calls - held to a brute-force sort under
AddressSanitizer + UBSan (tests/check_contact_capsule.cpp); the numpy float32 statement the GPU tests compare bytes with
(tests/contact_capsule_cases.py) against the same statement in float64 and on hand-worked cases; and what Context.contact_capsule
validates before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import closest_point_all_cases as ca
import closest_point_cases as cc
import contact_capsule_cases as kc
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
    assert "rt_contact_capsule" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_contact_capsule")
    assert re.search(r"int rt_contact_capsule\(rt_ctx\* ctx, const rt_capsule\* capsules, size_t n, uint32_t max_contacts,\s*rt_contact\* out,\s*"
                     r"uint32_t\* counts,\s*uint32_t flags\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_sweep_capsule, rt_contact_capsule,[^.]*\.\s+A call rejected for its arguments changes nothing",
                     _header(), re.S), "listed among the calls a running image survives"
    assert _header().index("Overlap queries:") < _header().index("Contact queries:") < _header().index("Geometry updates:")
    flat = re.sub(r"\s*\n \*\s+", " ", _header())
    assert "the converse fails only at dist2 == radius * radius" in flat and "the bound is loose for a long diagonal capsule" in flat


def test_defines_agree_with_the_python_constants(rt_api):
    def value(name):
        return int(re.search(r"^#define %s (\d+)u" % name, _header(), re.M).group(1))
    assert value("RT_CONTACT_MAX") == rt_api.CONTACT_MAX == kc.CONTACT_MAX == 16
    assert value("RT_CONTACT_ANY") == rt_api.CONTACT_ANY == 4
    assert len({value("RT_QUERY_COUNTERS"), value("RT_QUERY_COUNT_ALL"), value("RT_CONTACT_ANY")}) == 3, "the call's three flags are distinct bits"


def test_struct_layouts_agree_with_the_dtypes(tmp_path):
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(rt_capsule), offsetof(rt_capsule, origin),'
           ' offsetof(rt_capsule, radius), offsetof(rt_capsule, axis), offsetof(rt_capsule, _pad));'
           'printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_contact), offsetof(rt_contact, position), offsetof(rt_contact, distance), offsetof(rt_contact, s),'
           ' offsetof(rt_contact, _reserved), offsetof(rt_contact, prim_id), offsetof(rt_contact, material_id));'
           'printf("%zu %zu %zu\\n", offsetof(rt_capsule_sweep, origin), offsetof(rt_capsule_sweep, radius), offsetof(rt_capsule_sweep, axis));return 0;}\n')
    exe = str(tmp_path / "rt_capsule_probe")
    subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    cap, con, sweep = (list(map(int, line.split())) for line in subprocess.check_output([exe]).decode().splitlines())
    assert cap == [T.CAPSULE.itemsize] + [T.CAPSULE.fields[f][1] for f in ("origin", "radius", "axis", "_pad")] == [32, 0, 12, 16, 28]
    assert con == [T.CONTACT.itemsize] + [T.CONTACT.fields[f][1] for f in ("position", "distance", "s", "_reserved", "prim_id", "material_id")] == [32, 0, 12, 16, 20, 24, 28]
    assert sweep == cap[1:4], "an rt_capsule is the first 32 bytes of an rt_capsule_sweep"
    assert [T.CONTACT.fields[f][1] for f in ("position", "s", "prim_id", "material_id")] == [T.CAPSULE_SWEEP_HIT.fields[f][1] for f in ("position", "s", "prim_id", "material_id")]
    assert T.CONTACT.fields["distance"][1] == T.CAPSULE_SWEEP_HIT.fields["t"][1]
    assert T.EXPECTED_SIZES["CAPSULE"] == T.EXPECTED_SIZES["CONTACT"] == 32


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    caps, out, counts = (C.c_float * 8)(), (C.c_float * 32)(), (C.c_uint32 * 1)()
    assert lib.rt_contact_capsule(C.c_void_p(0), caps, C.c_size_t(1), C.c_uint32(4), out, counts, C.c_uint32(0)) == -1
    assert lib.rt_contact_capsule(C.c_void_p(0), None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_uint32(0)) == -1
    assert not any(bytes(out)) and not any(bytes(counts))


# -- the host check under sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cc") / "check_contact_capsule"
    cc_run = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-pthread",
                             "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, os.path.join(HERE, "check_contact_capsule.cpp"),
                             os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert cc_run.returncode == 0, cc_run.stderr[-3000:]
    return str(exe)


KINDS = {0: "soup", 1: "coplanar", 2: "coincident points", 3: "collinear chain", 4: "huge + tiny", 5: "NaN / inf vertices"}


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
@pytest.mark.parametrize("kind", sorted(KINDS), ids=[KINDS[k].replace(" ", "_") for k in sorted(KINDS)])
def test_host_walk_equals_the_brute_force(checker, method, kind):
    """Every record and count of the walk - statement, list, node bound, order and stack as the kernel runs them - is the brute-force
    sort's at K = 1, 4 and 16, with and without COUNT_ALL, and in ANY mode; a zero axis gives cp_walk_all's records, counts and work;
    the stack and the list stay inside the words the kernel's launch provides (the program checks every index).  On ordinary input at
    n = 20000 the small capsules make fewer than n / 10 triangle tests."""
    for n in (1, 5, 300, 20000):
        run = subprocess.run([checker, str(n), "1", str(kind), str(method)], capture_output=True, text=True)
        assert run.returncode == 0, (n, run.stdout[-2000:], run.stderr[-3000:])
        assert re.search(r" 0 failures$", run.stdout.strip()), run.stdout[-500:]
        per_k = re.findall(r"^K +(\d+)( COUNT_ALL)? *: 0 failed, ([0-9.]+) node visits and ([0-9.]+) triangle tests", run.stdout, re.M)
        assert sorted((k, bool(a)) for k, a, _, _ in per_k) == sorted((k, a) for k in ("1", "4", "16") for a in (False, True)), run.stdout[-1500:]
        assert re.search(r"^ANY +: 0 failed", run.stdout, re.M), run.stdout[-1500:]
        zero = re.search(r"^zero axis +: 0 failed over (\d+) capsules", run.stdout, re.M)
        assert zero and int(zero.group(1)) > 30, run.stdout[-1500:]  # 91 with a tree; 40 when every triangle is left out (NaN vertices, n = 1)
        small = re.search(r"^small capsules: ([0-9.]+) node visits and ([0-9.]+) triangle tests per capsule over (\d+) capsules", run.stdout, re.M)
        if n == 20000 and kind in (0, 1, 5):  # ordinary input: the walk culls (degenerate input need not)
            print(f"kind {kind} method {method}: the small capsules make {small.group(2)} triangle tests per capsule (brute force 20000)")
            assert int(small.group(3)) >= 64 and float(small.group(2)) < 20000 / 10, run.stdout[-1500:]


# -- the float32 statement against the float64 one ----------------------------------------------------------------------------
SCENES = {"soup": kc.soup, "cornell12": scenes.cornell12}


@pytest.fixture(scope="module")
def both(request):
    cache = {}

    def get(name):
        if name not in cache:
            scene = SCENES[name]()
            caps = kc.soup_reference()[0] if name == "soup" else kc.soup_capsules(scene, 2048, 11)
            d32 = kc.soup_reference()[1] if name == "soup" else kc.pair_dist2(scene, caps)
            cache[name] = (scene, caps, d32, kc.pair_dist2(scene, caps, F64))
        return cache[name]
    return get


@pytest.mark.parametrize("name", sorted(SCENES))
def test_f32_distances_lie_within_k_diagonals_of_f64(both, name):
    """Every listed distance (K = CONTACT_MAX) of soup_capsules(scene, 2048, 11) lies within 2 x K_MEASURED x the scene's diagonal of
    the float64 statement's distance for the same primitive, and K_MEASURED is the smallest k of the grid that holds: the next
    smaller one is violated.  Measured: soup 2.07e-7 at most (2.6e-8 diagonals), cornell12 4.29e-7 (1.24e-7 diagonals)."""
    scene, caps, d32, d64 = both(name)
    recs, _, total = kc.contacts_all(scene, caps, kc.CONTACT_MAX, d32)
    col = kc.columns(scene, recs)
    listed = col >= 0
    assert listed.sum() > 1000 and (listed.sum(1) == np.minimum(total, kc.CONTACT_MAX)).all()
    want = np.sqrt(d64[np.arange(len(caps))[:, None], np.where(listed, col, 0)])
    diff = np.abs(recs[..., 3].astype(F64) - want)[listed] / kc.diagonal(scene)
    k = kc.K_MEASURED[name]
    grid = sorted(m * 10.0 ** e for m in (1, 1.5, 2, 3, 5, 7) for e in range(-12, -3))
    below = max(g for g in grid if g < k * (1 - 1e-9))
    print(f"{name}: the largest |distance32 - distance64| is {diff.max():.3g} diagonals over {listed.sum()} listed contacts; K_MEASURED {k:g}")
    assert diff.max() <= 2 * k
    assert below < diff.max() <= k, "K_MEASURED is the smallest k of the grid that holds"


def test_f32_membership_agrees_with_f64_away_from_zero_margin(both):
    """random_soup(3000, n_spheres=3) with soup_capsules(2048, 11): every pair whose float64 margin |distance - radius| exceeds 1e-5
    agrees; the pairs left out are at most 1e-4 of all pairs and the capsules with a pair left out at most 5 %.  Measured on the CPU:
    2 of 6,150,144 pairs left out (3.3e-7), 2 of 2048 capsules (0.1 %), and no disagreement even among the pairs left out."""
    scene, caps, d32, d64 = both("soup")
    with np.errstate(all="ignore"):
        margin = np.sqrt(d64) - caps[:, 3].astype(F64)[:, None]
    f32, f64 = kc.in_range(caps, d32), margin < 0
    left_out = np.abs(margin) <= 1e-5
    print(f"{left_out.sum()} of {left_out.size} pairs left out ({left_out.mean():.1e}), {left_out.any(1).sum()} of {len(caps)} capsules "
          f"({left_out.any(1).mean():.1%}); {(f64 != f32).sum()} disagreements in all")
    assert f32.shape == margin.shape == (2048, 3003) and f32.any() and not f32.all() and kc.valid(caps).all()
    assert (f64 == f32)[~left_out].all()
    assert left_out.mean() <= 1e-4 and left_out.any(1).mean() <= 0.05


def test_the_batch_fills_and_overflows_its_lists():
    """What the GPU test's first case needs, from the numpy statement alone."""
    total = kc.soup_reference()[3]
    for k in (4, 16):
        some, more = ((total > 0) & (total < k)).mean(), (total > k).mean()
        print(f"K {k}: {some:.1%} of the capsules hold some but fewer than K contacts, {more:.1%} more than K")
        assert some > 0.05 and more > 0.05


# -- the numpy statement on hand-worked cases ---------------------------------------------------------------------------------
def _contacts(scene, origin, radius, axis, k=4):
    recs, listed, total = kc.contacts_all(scene, kc.make_capsules([origin], radius, [axis]), k)
    r = recs[0].view(T.CONTACT).reshape(-1)
    return r, int(listed[0]), int(total[0])


BIG = [[-4, -4, 0], [8, -4, 0], [-4, 8, 0]]  # a triangle in z = 0 whose interior holds the unit square


def test_a_capsule_lying_flat_above_a_triangle():
    """Both ends and the whole axis are at the same height: the first candidate with the strictly smallest dist2 is end A."""
    r, listed, total = _contacts(ca.triangles_scene([BIG]), (0, 0, 0.5), 1.0, (1, 0.5, 0))
    assert (listed, total) == (1, 1) and r["prim_id"].tolist() == [0, MISS, MISS, MISS]
    assert r["distance"][0] == F32(0.5) and r["s"][0] == 0 and r["position"][0].tolist() == [0, 0, 0] and r["_reserved"][0] == 0
    assert r["distance"][1:].tolist() == [1.0] * 3 and not r["position"][1:].any() and not r["material_id"][1:].any(), "unused slots: cp_answer_miss(radius)"
    r, _, _ = _contacts(ca.triangles_scene([BIG]), (0, 0, 0.75), 1.0, (1, 0, -0.5))
    assert r["distance"][0] == F32(0.25) and r["s"][0] == 1 and r["position"][0].tolist() == [1, 0, 0], "end B is the nearer"
    # normal and depth: the push-out of the issue
    normal = ((np.array([0, 0, 0.75]) + np.array([1, 0, -0.5]) * r["s"][0]) - r["position"][0]) / r["distance"][0]
    assert normal.tolist() == [0, 0, 1] and 1.0 - r["distance"][0] == 0.75


def test_an_axis_that_pierces_is_at_distance_zero():
    r, listed, total = _contacts(ca.triangles_scene([BIG]), (0.5, 0.25, 0.5), 0.125, (0, 0, -2))
    assert (listed, total) == (1, 1) and r["distance"][0] == 0 and r["s"][0] == F32(0.25) and r["position"][0].tolist() == [0.5, 0.25, 0]
    r, _, total = _contacts(ca.triangles_scene([BIG]), (0.5, 0.25, 0.5), 0.125, (0, 0, -0.25))
    assert total == 0, "both ends above the plane and farther than the radius"
    r, _, total = _contacts(ca.triangles_scene([BIG]), (0.5, 0.25, 0.0), 0.125, (0, 0, 1))
    assert total == 1 and r["distance"][0] == 0 and r["s"][0] == 0, "an end in the plane: end A's candidate, not the piercing one"


def test_one_ulp_outside_the_radius_and_equality_are_not_listed():
    """dist2 < radius * radius, strictly: at dist2 == radius^2 the capsule sweep is in contact (<=) and this query lists nothing."""
    tri = ca.triangles_scene([BIG])
    up, down = float(np.nextafter(F32(0.5), F32(1))), float(np.nextafter(F32(0.5), F32(0)))
    assert _contacts(tri, (0, 0, 0.5), 0.5, (1, 0, 0))[2] == 0, "dist2 == radius^2"
    assert _contacts(tri, (0, 0, 0.5), up, (1, 0, 0))[2] == 1
    assert _contacts(tri, (0, 0, up), 0.5, (1, 0, 0))[2] == 0, "one ulp outside"
    assert _contacts(tri, (0, 0, down), 0.5, (1, 0, 0))[2] == 1
    import sweep_capsule_cases as scs
    sweep = scs._pack(np.array([[0, 0, 0.5]]), np.array([[1, 0, 0]]), np.array([[0, 0, -1]]), 0.5)
    hit = scs.brute_force(tri, sweep).view(T.CAPSULE_SWEEP_HIT)[0]
    assert hit["t"] == 0 and hit["prim_id"] == 0, "... where rt_sweep_capsule starts in contact"
    assert _contacts(tri, (0, 0, 0.5), INF, (1, 0, 0))[2] == 1 and _contacts(tri, (0, 0, 1e30), INF, (1, 0, 0))[2] == 0, "inf radius; an infinite dist2 is never in range"


def test_a_sphere_outside_crossed_and_containing_the_capsule():
    ball = ca.triangles_scene([[[50, 50, 50], [51, 50, 50], [50, 51, 50]]], spheres=[((0, 0, 0), 2.0, 3)])
    # outside: the foot of the centre on the axis (s = 0.5), the surface 1 away
    r, listed, total = _contacts(ball, (3, -1, 0), 1.5, (0, 2, 0))
    assert (listed, total) == (1, 1) and r["prim_id"][0] == cc.SPHERE_FLAG and r["material_id"][0] == 3
    assert r["distance"][0] == 1 and r["s"][0] == F32(0.5) and r["position"][0].tolist() == [2, 0, 0]
    assert _contacts(ball, (3, -1, 0), 1.0, (0, 2, 0))[2] == 0
    # wholly inside: the end farther from the centre (B), the surface 0.5 away; A on a tie
    r, _, total = _contacts(ball, (0.5, 0, 0), 1.0, (1, 0, 0))
    assert total == 1 and r["distance"][0] == F32(0.5) and r["s"][0] == 1 and r["position"][0].tolist() == [2, 0, 0]
    r, _, _ = _contacts(ball, (-1, 0, 0), 1.5, (2, 0, 0))
    assert r["distance"][0] == 1 and r["s"][0] == 0 and r["position"][0].tolist() == [-2, 0, 0], "a tie: end A"
    assert _contacts(ball, (0.5, 0, 0), 0.5, (1, 0, 0))[2] == 0
    # crossed from inside: the upper root, s = (2 - 1) / 4
    r, _, total = _contacts(ball, (1, 0, 0), 0.25, (4, 0, 0))
    assert total == 1 and r["distance"][0] == 0 and r["s"][0] == F32(0.25) and r["position"][0].tolist() == [2, 0, 0]
    # crossed from outside, both ends outside: the lower root, s = (4 - 2) / 8
    r, _, total = _contacts(ball, (-4, 0, 0), 0.25, (8, 0, 0))
    assert total == 1 and r["distance"][0] == 0 and r["s"][0] == F32(0.25) and r["position"][0].tolist() == [-2, 0, 0]
    # a zero axis on the surface, and one inside: the closest-point statement
    r, _, total = _contacts(ball, (0, 2, 0), 0.25, (0, 0, 0))
    assert total == 1 and r["distance"][0] == 0 and r["s"][0] == 0 and r["position"][0].tolist() == [0, 2, 0]


def test_nan_vertices_and_degenerate_queries_list_nothing():
    scene = ca.triangles_scene([BIG], spheres=[((0, 0, 0), 1.0, 0)])
    assert _contacts(scene, (0, 0, 0.5), 2.0, (0.5, 0, 0))[2] == 2
    for origin, radius, axis in (((NAN, 0, 0.5), 2.0, (0.5, 0, 0)), ((0, INF, 0.5), 2.0, (0.5, 0, 0)), ((0, 0, 0.5), 2.0, (NAN, 0, 0)),
                                 ((0, 0, 0.5), 2.0, (0, -INF, 0)), ((0, 0, 0.5), NAN, (0.5, 0, 0)), ((0, 0, 0.5), 0.0, (0.5, 0, 0)),
                                 ((0, 0, 0.5), -1.0, (0.5, 0, 0))):
        r, listed, total = _contacts(scene, origin, radius, axis)
        assert (listed, total) == (0, 0) and (r["prim_id"] == MISS).all() and not r["position"].any() and not r["s"].any()
        assert r["distance"].tobytes() == np.full(4, radius, F32).tobytes(), "the radius as given"
    for bad in (NAN, INF, -INF):
        for corner in range(3):
            corners = np.array(BIG, F32)
            corners[corner, 0] = bad
            assert _contacts(ca.triangles_scene([corners]), (0, 0, 0.5), 3e38, (0.5, 0, 0))[2] == 0, (bad, corner)
        assert _contacts(ca.triangles_scene([BIG], spheres=[((bad, 0, 0), 1.0, 0)]), (0, 0, 0.5), 1.0, (0.5, 0, 0))[2] == 1, bad
    assert _contacts(ca.triangles_scene([BIG], spheres=[((0, 0, 0), NAN, 0)]), (0, 0, 0.5), 1.0, (0.5, 0, 0))[2] == 1


def test_a_zero_axis_is_the_nearest_k_statement():
    soup = scenes.random_soup(300, n_spheres=3)
    points = ca.cc.four_kinds(soup, 128, 5)
    radius = np.where(np.arange(128) % 2 == 0, 0.4, INF).astype(F32)
    want, want_listed, want_total = ca.nearest_all(soup, np.concatenate([points, radius[:, None]], 1), 8)
    got, listed, total = kc.contacts_all(soup, kc.make_capsules(points, radius, (0, 0, 0)), 8)
    assert got[..., [0, 1, 2, 3, 6, 7]].tobytes() == want[..., [0, 1, 2, 3, 6, 7]].tobytes() and not got[..., 4:6].any()
    assert listed.tobytes() == want_listed.tobytes() and total.tobytes() == want_total.tobytes() and (total > 8).any()


def test_smaller_k_is_a_prefix_and_the_lists_ascend():
    soup = scenes.random_soup(300, n_spheres=3)
    caps = kc.soup_capsules(soup, 128, 7, radii=(0.05, 1.0))
    recs, listed, total = kc.contacts_all(soup, caps)
    for k in (1, 4):
        want = kc.contacts_all(soup, caps, k)
        got = kc.first_k(recs, total, k)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and total.tobytes() == want[2].tobytes()
    listed_mask = np.arange(kc.CONTACT_MAX)[None] < listed[:, None]
    prim = np.ascontiguousarray(recs[..., 6]).view(np.uint32)
    assert ((prim != MISS) == listed_mask).all() and (np.diff(recs[..., 3], axis=1)[listed_mask[:, 1:]] >= 0).all()
    assert (recs[..., 3][listed_mask] < np.broadcast_to(caps[:, 3, None], listed_mask.shape)[listed_mask]).all()
    assert (total > kc.CONTACT_MAX).any() and (total == 0).any() and ((total > 0) & (total < 4)).any()


def test_the_lattice_and_the_deck_are_what_they_are_for():
    walls = ca.coplanar_walls()
    caps = kc.lattice_capsules()
    d2 = kc.pair_dist2(walls, caps)
    listed = kc.in_range(caps, d2)
    ties = np.array([len(np.unique(row[m])) < m.sum() for row, m in zip(d2, listed)])
    print(f"lattice: {len(caps)} capsules, {ties.sum()} with an exact tie among their contacts, {(d2 == 0)[listed].sum()} contacts at distance 0")
    assert ties.mean() > 0.5 and (d2 == 0)[listed].sum() > 100
    deck = kc.sk.deck_scene()
    n_cards = deck.meta["cards"]
    _, _, total = kc.contacts_all(deck, kc.deck_capsules("corner"), 1)
    assert (total == 0).all()
    _, _, total = kc.contacts_all(deck, kc.deck_capsules("covered"), 1)
    assert (total == n_cards).all(), "pierces every card; the wall stands behind the far end"
    _, _, total = kc.contacts_all(deck, kc.deck_capsules("mixed"), 1)
    assert set(total.tolist()) == {0, n_cards}


# -- the Python layer ---------------------------------------------------------------------------------------------------------
def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.contact_capsule
    good = np.zeros((4, 8), F32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="capsules: shape"):
        call(nc, np.zeros((4, 12), F32), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), F32)[::2], 4)
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8], 4)
    for bad in (-1, 17, 2.0, True, None):
        with pytest.raises(ValueError, match="max_contacts"):
            call(nc, good, bad)
    with pytest.raises(ValueError, match="count_all"):
        call(nc, good, 0)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 4, any_hit=True)
    with pytest.raises(ValueError, match="any_hit"):
        call(nc, good, 0, any_hit=True, count_all=True)
    with pytest.raises(TypeError):
        call(nc, good, 2, np.zeros((4, 2, 8), F32))  # out is keyword-only
    with pytest.raises(ValueError, match="rows for 4 capsules"):
        call(nc, good, 2, out=np.zeros((3, 2, 8), F32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 3, 8), F32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 2, out=np.zeros((4, 16), F32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, out=np.zeros((4, 2, 8), np.float64))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 2, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="counts: 3 rows"):
        call(nc, good, 2, counts=np.zeros(3, np.uint32))


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def rt_contact_capsule(self, h, capsules, n, max_contacts, out, counts, flags):
        self.calls.append((capsules.value, n.value, max_contacts.value, out.value, counts.value, flags.value))
        return 0


def test_contact_capsule_passes_its_arguments(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    origin = np.arange(18, dtype=F32).reshape(6, 3)
    caps = rt_api.make_capsules(origin, 0.5, (0, 1, 0))
    assert caps.shape == (6, 8) and caps.dtype == np.float32 and caps.tobytes() == kc.make_capsules(origin, 0.5, (0, 1, 0)).tobytes()
    per = rt_api.make_capsules(origin, np.arange(1, 7), origin[::-1]).view(T.CAPSULE)
    assert per["radius"].ravel().tolist() == [1, 2, 3, 4, 5, 6] and per["axis"].reshape(6, 3).tolist() == origin[::-1].tolist() and not per["_pad"].any()
    sweeps = rt_api.make_capsule_sweeps(origin, origin[::-1], np.ones((6, 3), F32), np.arange(1, 7))
    assert sweeps[:, :8].tobytes() == per.view(F32).reshape(6, 8).tobytes(), "the first 32 bytes of the sweep's record"
    out, counts = ctx.contact_capsule(caps, 3)
    assert out.shape == (6, 3, 8) and out.dtype == np.float32 and counts.shape == (6,) and counts.dtype == np.uint32
    own, own_counts = np.zeros((6, 16, 8), F32), np.zeros(6, np.uint32)
    got = ctx.contact_capsule(caps, np.int64(16), out=own, counts=own_counts, count_all=True, counters=True)
    assert got[0] is own and got[1] is own_counts
    none, only_counts = ctx.contact_capsule(caps, 0, out=own, count_all=True)
    assert none is None and only_counts.shape == (6,)
    none, any_counts = ctx.contact_capsule(caps, 0, any_hit=True, counters=True)
    assert none is None and any_counts.shape == (6,)
    assert ctx.lib.calls == [(caps.ctypes.data, 6, 3, out.ctypes.data, counts.ctypes.data, 0),
                             (caps.ctypes.data, 6, 16, own.ctypes.data, own_counts.ctypes.data, rt_api.QUERY_COUNTERS | rt_api.QUERY_COUNT_ALL),
                             (caps.ctypes.data, 6, 0, None, only_counts.ctypes.data, rt_api.QUERY_COUNT_ALL),
                             (caps.ctypes.data, 6, 0, None, any_counts.ctypes.data, rt_api.CONTACT_ANY | rt_api.QUERY_COUNTERS)]
    recs = np.zeros((2, 8), F32)
    recs[0] = [1, 2, 3, 0.25, 0.5, 0, 0, 0]
    recs.view(np.uint32)[:, 6:8] = [[7, 2], [MISS, 0]]
    pos, dist, s, prim, mat = rt_api.split_contacts(recs)
    assert pos[0].tolist() == [1, 2, 3] and dist[0] == 0.25 and s[0] == 0.5 and prim.tolist() == [7, MISS] and mat.tolist() == [2, 0]
