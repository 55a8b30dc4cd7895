"""The deck (tests/stack_cases.py) without a GPU: a model of the traversal stacks' step rules replayed on the host builders' trees under
AddressSanitizer + UBSan (tests/check_stack_marks.cpp), and the deck's closed forms held against the float64 statement.

Why the deck exists: the pipeline's closest-hit kernel keeps RT_WF8_LDS_STACK entries per lane in LDS and everything deeper in an HBM
overflow area, and the scenes the pipeline tests use never get there - the model prints it for a 3000-triangle random_soup below.  On the
deck the model's "mixed" waves do, with both host builders; tests/test_gpu_stack_marks.py reads the same mark from the counting kernel."""
import os
import re
import subprocess

import numpy as np
import pytest

import reference_cases as rc
import stack_cases as sc
from gpu_raytracer_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "gpu_raytracer_amd", "csrc")
SETS = ("through", "corner", "mixed")


def lds_stack_entries():
    """RT_WF8_LDS_STACK as csrc/wavefront.h defines it."""
    with open(os.path.join(CSRC, "wavefront.h")) as f:
        m = re.search(r"^#define\s+RT_WF8_LDS_STACK\s+(\d+)", f.read(), re.M)
    assert m, "RT_WF8_LDS_STACK not found in wavefront.h"
    return int(m.group(1))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stack") / "check_stack_marks"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-pthread",
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                         os.path.join(HERE, "check_stack_marks.cpp"), os.path.join(CSRC, "bvh_builder.cpp"), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return str(exe)


@pytest.fixture(scope="module")
def deck():
    scene = sc.deck_scene()
    rays = {k: sc.ray_set(k) for k in SETS}
    for r in rays.values():
        r.setflags(write=False)
    return scene, rays


def _corners(scene):
    p = scene.vertices["position"].astype(np.float32)
    tr = scene.triangles
    return np.stack([p[tr["v0_index"]], p[tr["v1_index"]], p[tr["v2_index"]]], 1)


def _run(checker, folder, scene, method, ray_sets):
    """-> (tree dict, {set name: dict of the marks}) as check_stack_marks prints them."""
    tris = os.path.join(folder, f"{scene.name}_tris.bin")
    _corners(scene).astype(np.float32).tofile(tris)
    files = []
    for name, rays in ray_sets.items():
        files.append(os.path.join(folder, f"{name}.bin"))
        np.ascontiguousarray(rays, np.float32).tofile(files[-1])
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    run = subprocess.run([checker, tris, str(method), str(lds_stack_entries())] + files, capture_output=True, text=True, env=env, timeout=300)
    assert run.returncode == 0, f"{run.stdout[-2000:]}\n{run.stderr[-3000:]}"
    print(run.stdout)
    m = re.search(r"tree method (\d+) tris (\d+) nodes (\d+) leaves (\d+) depth (\d+) real_depth (\d+) failures (\d+)", run.stdout)
    assert m, run.stdout[-500:]
    tree = dict(zip(("method", "tris", "nodes", "leaves", "depth", "real_depth", "failures"), map(int, m.groups())))
    marks = {}
    for r in re.finditer(r"rays (\w+)\.bin n (\d+) waves (\d+) mark_a (\d+) mark_b (\d+) mark_b_any (\d+) hits (\d+) via_overflow (\d+)", run.stdout):
        marks[r.group(1)] = dict(zip(("n", "waves", "mark_a", "mark_b", "mark_b_any", "hits", "via_overflow"), map(int, r.groups()[1:])))
    assert set(marks) == set(ray_sets), run.stdout[-1000:]
    return tree, marks


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
def test_model_marks_on_the_deck(checker, tmp_path, deck, method):
    """Replay on the deck (8192 cards; the model, not the kernel): "mixed" waves under k_wf_trace's rule hold 10 entries on the
    binned-SAH tree (depth 7) and 12 on the PLOC tree (depth 8); a coherent 8 x 8 camera block in the empty corner holds 5 and 6:
    coherent waves drain their leaf groups at once, so only bounced and shadow segments reach the overflow on the device.
    How many rays find their closest hit THROUGH an overflow entry (so that a lost or misaddressed entry would change their answer):
    recorded, not asserted - none of "through", "corner" and "mixed", whose deep lanes hit no card, and of the 256 "crossing" rays,
    which enter through the empty corner and find a card in mid-deck, 1 on the binned-SAH tree and 0 on the PLOC tree: the walk is
    nearest first, so the card is found before the groups parked deepest are looked at.  The deck shows that the overflow path runs,
    stays in bounds and ends; it does not show that every overflow entry comes back as it was written."""
    scene, rays = deck
    sets = dict(rays, block=sc.camera_block_rays(5, 1), crossing=sc.ray_set("crossing"))
    tree, marks = _run(checker, str(tmp_path), scene, method, sets)
    lds = lds_stack_entries()
    assert tree["failures"] == 0 and tree["tris"] == scene.n_triangles and tree["real_depth"] <= tree["depth"]
    assert lds < marks["mixed"]["mark_b"], "the deck's mixed waves must overflow the LDS part of the stack"
    for name, m in marks.items():
        assert max(m["mark_b"], m["mark_b_any"]) <= 2 * tree["real_depth"] + 2, name
        assert m["mark_a"] <= tree["real_depth"] - 1, name  # group_walk.h
    print("closest hits found through an overflow entry:", {name: m["via_overflow"] for name, m in marks.items()})
    n = len(rays["through"])
    assert marks["through"]["hits"] == n and marks["corner"]["hits"] == n  # card 0; the wall


@pytest.mark.parametrize("method", [0, 1], ids=["binned_sah", "ploc"])
def test_model_marks_on_a_soup_are_recorded(checker, tmp_path, method, capsys):
    """The reason this file exists, printed and not asserted: under k_wf_trace's rule a 3000-triangle random_soup stays at or below
    RT_WF8_LDS_STACK (measured: 6 for the incoherent rays and 5 for the camera rays on the binned-SAH tree, 5 for both on the PLOC
    tree) - the overflow area is never touched."""
    scene = scenes.random_soup(3000, n_spheres=3)
    rng = np.random.default_rng(5)
    p = scene.vertices["position"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (256, 3))
    d = rng.standard_normal((256, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    eye, cam = rc.camera_rays(scene.camera, *sc.FRAME)
    cam = cam[16:32, 24:40].reshape(-1, 3)
    sets = {"incoherent": sc._batch(o, d), "camera": sc._batch(np.broadcast_to(eye, cam.shape), cam)}
    tree, marks = _run(checker, str(tmp_path), scene, method, sets)
    with capsys.disabled():
        print(f"\nsoup3000 method {method}: depth {tree['real_depth']}, marks under k_wf_trace's rule "
              f"{ {k: max(v['mark_b'], v['mark_b_any']) for k, v in marks.items()} } (LDS part: {lds_stack_entries()})")
    assert tree["failures"] == 0


def test_closed_forms_of_the_ray_sets(deck):
    """Against the float64 statement: "through" rays hit card 0's plane at the analytic t and cross all n cards, "corner" rays cross
    none and end on the wall; in "mixed" the covered rays cross all n cards and the others none."""
    scene, rays = deck
    n = scene.meta["cards"]
    cards = sc.card_corners(n)
    for name in SETS:
        r = rays[name].astype(np.float64)
        hit = rc.closest_hit(scene, r[:, 0:3], r[:, 4:7], tmin=r[:, 3], tmax=r[:, 7], chunk=32, dtype=np.float64)
        crossed = sc.crossings(cards, rays[name])
        assert not hit["unsure"].any(), name
        if name == "through":
            np.testing.assert_array_equal(hit["prim"], 0)
            np.testing.assert_allclose(hit["t"], (r[:, 2] - sc.Z_FRONT) / -r[:, 6], rtol=1e-12)
            np.testing.assert_array_equal(crossed, n)
        elif name == "corner":
            assert np.isin(hit["prim"], (n, n + 1)).all()
            np.testing.assert_allclose(hit["t"], (r[:, 2] - sc.Z_WALL) / -r[:, 6], rtol=1e-12)
            np.testing.assert_array_equal(crossed, 0)
        else:
            covered = sc.mixed_covered(len(r))
            assert covered.sum() * 2 == len(r), "half of the set through each region"
            from_back = r[:, 6] > 0
            assert from_back[covered].any() and from_back[~covered].any() and (~from_back)[covered].any() and (~from_back)[~covered].any()
            np.testing.assert_array_equal(crossed, np.where(covered, n, 0))
            np.testing.assert_array_equal(hit["prim"][covered], np.where(from_back[covered], n - 1, 0))
            assert np.isin(hit["prim"][~covered & ~from_back], (n, n + 1)).all() and (hit["prim"][~covered & from_back] == rc.PRIM_MISS).all()


def test_closed_forms_of_the_camera(deck):
    """At the GPU tests' frame size at least a quarter of the pixels look through the empty half - inside every card's box from the
    first card to the last, crossing none - and at least a quarter through the cards."""
    scene, _ = deck
    n = scene.meta["cards"]
    w, h = sc.FRAME
    o, d = rc.camera_rays(scene.camera, w, h)
    d = d.reshape(-1, 3)
    rays = sc._batch(np.broadcast_to(o, d.shape), d)
    crossed = sc.crossings(sc.card_corners(n), rays)
    front = o[None, :2] + d[:, :2] * ((o[2] - sc.Z_FRONT) / -d[:, 2])[:, None]
    back = o[None, :2] + d[:, :2] * ((o[2] - (sc.Z_FRONT - sc.Z_LENGTH)) / -d[:, 2])[:, None]
    inside = (np.abs(front) <= 1.0 - sc.JITTER).all(1) & (np.abs(back) <= 1.0 - sc.JITTER).all(1)
    empty = inside & (front.sum(1) > 0) & (crossed == 0)
    through = crossed == n
    print(f"{w}x{h}: {empty.mean():.3f} of the pixels through the empty half, {through.mean():.3f} through all {n} cards")
    assert empty.mean() >= 0.25 and through.mean() >= 0.25
    some = np.arange(5, len(d), 12)  # every twelfth pixel: the statement's closest hit agrees with the count
    hit = rc.closest_hit(scene, np.broadcast_to(o, (len(some), 3)), d[some], chunk=32, dtype=np.float64)
    assert through[some].sum() > 50 and empty[some].sum() > 50
    assert (hit["prim"][through[some]] == 0).all() and np.isin(hit["prim"][empty[some]], (n, n + 1)).all()


def test_points_and_the_sheared_copy(deck):
    scene, _ = deck
    n = scene.meta["cards"]
    p = sc.points()
    assert p.shape == (sc.RECORDS, 3) and p.dtype == np.float32
    in_deck = (np.abs(p[:, :2]) <= 1.0).all(1) & (p[:, 2] <= sc.Z_FRONT) & (p[:, 2] >= sc.Z_FRONT - sc.Z_LENGTH)
    assert in_deck[0::4].all() and in_deck[1::4].all() and in_deck[2::4].all() and not in_deck[3::4].any()
    assert (p[0::4, :2].sum(1) < 0).all() and (p[2::4, :2].sum(1) > 0).all()
    moved = sc.sheared(scene)
    a, b = scene.vertices["position"].reshape(-1, 3, 3), moved.vertices["position"].reshape(-1, 3, 3)
    np.testing.assert_array_equal(a[..., 1:], b[..., 1:])
    np.testing.assert_allclose(b[:n, :, 0] - a[:n, :, 0], np.broadcast_to((sc.SHEAR * np.arange(n) / n)[:, None], (n, 3)), atol=1e-6)
    np.testing.assert_array_equal(a[n:], b[n:])
    assert moved.triangles.tobytes() == scene.triangles.tobytes()
