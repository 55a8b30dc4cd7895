"""Modes 0 and 1 of the CPU oracle against the independent float64 statement of reference_cases.py.

Every other test of the reference-semantics path compares two restatements made by one reading of the reference (the oracle and
the HIP kernels) with each other.  Here the oracle meets a second reading, written in numpy from the reference's source text alone:
ray generation, the sphere quadratic, Moeller-Trumbore, the three light types and their select, the BRDF switch, the transmission
mix with its dispersion table, emission, ambient, the channel filter, the unorm8 store and the combine.  test_gpu_reference.py runs
the same assertions on the HIP kernels.  Run with -s to see each case's unsure share, its largest errors against the tolerances
and the share of the frame on which each named wrong alternative is rejected.
"""
import numpy as np
import pytest

import reference_cases as rc
from gpu_raytracer_amd import hostpack as H

CASE_IDS = [c.name for c in rc.CASES]
_FRAMES = {}


def oracle_frame(oracle_mod, case, mode, use_bvh, scene=None):
    key = (case.name, mode, use_bvh, scene is not None)
    if key not in _FRAMES:
        packed = oracle_mod.PackedScene(scene if scene is not None else case.scene, use_bvh=use_bvh)
        _FRAMES[key] = oracle_mod.render_frame(packed, case.w, case.h, camera=case.camera, mode=mode, threads=4)
    return _FRAMES[key]


@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_case_conditions(case):
    """At most 2 % of a case's pixels are left out and every primitive class it is about covers at least 10 % of the frame: the
    statement alone, no renderer.  (That modes 0 and 1 agree on hits and what a miss looks like in each is asserted of the rendered
    frames in test_oracle_frame_matches_the_statement.)"""
    rc.check_case_conditions(case)


@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_oracle_frame_matches_the_statement(oracle_mod, case):
    """render_frame in both modes, brute force and through the reference-format BVH: primitive, t, float RGB, the three channel
    textures and the combined image (reference_cases.check_frame); a twin upload (other range / cone angles / roughness) gives
    the same bits; the named wrong alternatives are rejected."""
    for mode in (0, 1):
        for use_bvh in (False, True):
            frame = oracle_frame(oracle_mod, case, mode, use_bvh)
            rc.check_frame(case, mode, frame, "bvh" if use_bvh else "brute force", canonical_duplicates=use_bvh)
        if case.twin is not None:
            a, b = oracle_frame(oracle_mod, case, mode, False), oracle_frame(oracle_mod, case, mode, False, scene=case.twin)
            for k in ("prim", "red", "green", "blue", "combined"):
                np.testing.assert_array_equal(a[k], b[k])
            np.testing.assert_array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32))
        rc.check_alternatives(case, mode)
    a, b = oracle_frame(oracle_mod, case, 0, False), oracle_frame(oracle_mod, case, 1, False)
    np.testing.assert_array_equal(a["prim"], b["prim"])       # modes 0 and 1 agree on hits
    miss = ~rc.statement(case, 0)["unsure"] & (rc.statement(case, 0)["prim"] == rc.PRIM_MISS)
    if miss.any():                                            # a miss is black in mode 0 and the sky in mode 1
        assert not a["rgb"][miss].any()
        np.testing.assert_array_equal(b["rgb"][miss], np.broadcast_to(np.array([0.1, 0.2, 0.3], np.float32), b["rgb"][miss].shape))


@pytest.mark.parametrize("case", rc.CASES, ids=CASE_IDS)
def test_oracle_dispatch_per_tile_and_channel(oracle_mod, case):
    """Every case again as a sequence of main_cs dispatches, one per tile and channel (130 x 70 spans a tile edge)."""
    packed = oracle_mod.PackedScene(case.scene, use_bvh=True)
    for mode in (0, 1):
        imgs = [np.zeros((case.h, case.w, 4), np.uint8) for _ in range(3)]
        tx, ty = H.tile_count(case.w, case.h)
        for tile in range(tx * ty):
            ox, oy = (tile % tx) * 128, (tile // tx) * 128
            for ch in range(3):
                oracle_mod.dispatch(packed, packed.push_constants(case.w, case.h, channel=ch, mode=mode, tile_offset=(ox, oy)), imgs[ch])
        whole = oracle_frame(oracle_mod, case, mode, True)
        comb = np.zeros_like(imgs[0])
        comb[..., 0], comb[..., 1], comb[..., 2], comb[..., 3] = imgs[0][..., 0], imgs[1][..., 1], imgs[2][..., 2], 255
        frame = dict(whole, red=imgs[0], green=imgs[1], blue=imgs[2], combined=comb)
        rc.check_frame(case, mode, frame, "dispatch per tile and channel")


LIBM_SLACK = 0.05   # another libm's tanf / sqrt may move a measured figure's last digits: the guard's allowance, never the tolerance's


def _matches(measured, recorded):
    return measured <= (1.0 + LIBM_SLACK) * recorded and recorded <= (1.0 + LIBM_SLACK) * measured


def test_measured_constants_are_what_the_oracle_measures(oracle_mod):
    """The provenance of MEASURED_RGB_REL / MEASURED_T_REL: the largest error of the oracle against the statement per group and
    class (sphere pixels, flat pixels), over every case, mode and both traversals.  The recorded figures are the measurement,
    within 5 % either way; the bounds are exactly 4 x the recorded figures."""
    rgb = {g: {"flat": 0.0, "sphere": 0.0} for g in rc.GROUPS}
    t = {g: {"flat": 0.0, "sphere": 0.0} for g in rc.GROUPS}
    for case in rc.CASES:
        for mode in (0, 1):
            for use_bvh in (False, True):
                frame = oracle_frame(oracle_mod, case, mode, use_bvh)
                prim = frame["prim"].copy()
                if case.duplicates:
                    prim[np.isin(prim, case.duplicates)] = min(case.duplicates)
                m = rc.measure_frame(case, mode, dict(frame, prim=prim))
                for k in ("flat", "sphere"):
                    rgb[case.group][k], t[case.group][k] = max(rgb[case.group][k], m["rgb"][k]), max(t[case.group][k], m["t"][k])
    fmt = lambda d: {g: {k: float(f"{v:.3e}") for k, v in c.items()} for g, c in d.items()}  # noqa: E731
    print("MEASURED_RGB_REL =", fmt(rgb))
    print("MEASURED_T_REL =", fmt(t))
    for g in rc.GROUPS:
        for k in ("flat", "sphere"):
            assert _matches(rgb[g][k], rc.MEASURED_RGB_REL[g][k]), (g, k, rgb[g][k], rc.MEASURED_RGB_REL[g][k])
            assert _matches(t[g][k], rc.MEASURED_T_REL[g][k]), (g, k, t[g][k], rc.MEASURED_T_REL[g][k])
            assert rc.RGB_REL_BOUND[g][k] == 4.0 * rc.MEASURED_RGB_REL[g][k] and rc.T_REL_BOUND[g][k] == 4.0 * rc.MEASURED_T_REL[g][k]


def test_ray_query_batch_conditions_and_f32_measurement():
    """The ray-query batch of test_gpu_reference.py, with the statement alone: at most 2 % of the rays are unsure, at least 10 % hit
    a triangle, a sphere and nothing.  The oracle exports no barycentrics and takes no rays, so what f32 costs there is measured
    by evaluating the statement's own formulas in float32 (one rounding per operation) against float64, in units of each ray's
    conditioning (reference_cases.MEASURED_QUERY_T / _UV)."""
    scene, rays, hit = rc.query_statement()
    prim = hit["prim"]
    shares = {"unsure": hit["unsure"].mean(), "triangle": ((prim & rc.PRIM_SPHERE) == 0).mean(),
              "sphere": ((prim != rc.PRIM_MISS) & ((prim & rc.PRIM_SPHERE) != 0)).mean(), "miss": (prim == rc.PRIM_MISS).mean()}
    print(f"ray-query batch: {len(rays)} rays,", {k: f"{v:.4f}" for k, v in shares.items()})
    assert len(rays) == rc.QUERY_RAYS + 50 * 38
    assert shares["unsure"] <= rc.EDGE_SHARE_CAP and min(shares["triangle"], shares["sphere"], shares["miss"]) >= rc.CLASS_SHARE_MIN
    f32 = rc.closest_hit(scene, rays[:, 0:3], rays[:, 4:7], rays[:, 3], np.inf, dtype=np.float32)
    ok = ~hit["unsure"] & (f32["prim"] == prim)
    assert ok.mean() >= 1.0 - rc.EDGE_SHARE_CAP
    t_err, uv_err = rc.query_errors(hit, f32["t"], f32["u"], f32["v"])
    h = ok & (prim != rc.PRIM_MISS)
    tri = h & ((prim & rc.PRIM_SPHERE) == 0)
    t_m, uv_m = t_err[h].max(), uv_err[tri].max()
    print(f"f32 evaluation of the statement: MEASURED_QUERY_T = {t_m:.3e} (recorded {rc.MEASURED_QUERY_T:.3e}), MEASURED_QUERY_UV = {uv_m:.3e} "
          f"(recorded {rc.MEASURED_QUERY_UV:.3e}); conditioning of t: median {np.median(hit['cond_t'][h]):.1f}, largest {hit['cond_t'][h].max():.1f}; "
          f"of u, v: median {np.median(hit['cond_uv'][tri]):.1f}, largest {hit['cond_uv'][tri].max():.1f}")
    assert _matches(t_m, rc.MEASURED_QUERY_T) and _matches(uv_m, rc.MEASURED_QUERY_UV)
    assert rc.QUERY_T_BOUND == 4.0 * rc.MEASURED_QUERY_T and rc.QUERY_UV_BOUND == 4.0 * rc.MEASURED_QUERY_UV
    # what the bound means for the bulk of the rays, and the alternatives it rejects there
    tol_uv = rc.QUERY_UV_BOUND * hit["cond_uv"][tri]
    print(f"  u / v tolerance: median {np.median(tol_uv):.2e}, below 1e-4 on {(tol_uv < 1e-4).mean():.3f} of the triangle hits")
    assert (tol_uv < 1e-4).mean() > 0.9
    for name, alt_u in (("u and v swapped", hit["v"]), ("u off by 1e-3", hit["u"] + 1e-3)):
        share = (np.abs(alt_u - hit["u"])[tri] > 2.0 * tol_uv).mean()
        print(f"  alternative {name}: differs by more than twice the tolerance on {share:.3f} of the triangle hits")
        assert share > 0.5
    # the occlusion batch: rays that end just before / just beyond their closest hit
    orays, expected, unsure = rc.occlusion_batch()
    print(f"occlusion batch: {len(orays)} rays, occluded {expected.mean():.3f}, unsure {unsure.mean():.4f}")
    assert unsure.mean() <= rc.EDGE_SHARE_CAP and 0.2 < expected.mean() < 0.8
    n = len(rays)
    was_hit = prim != rc.PRIM_MISS
    sure = ~unsure[:n] & ~unsure[n:2 * n] & ~hit["unsure"]
    assert not expected[:n][was_hit & sure].any()        # the range ends just before the closest hit: nothing in it
    assert expected[n:2 * n][was_hit & sure].all()       # ... just beyond: the hit is in it


def test_f16_decode_of_the_threshold_words():
    """0x3800 is exactly 0.5 (not metallic: the test is `> 0.5`), 0x3801 the next f16 above; the low half of the packed word is the
    metallic, the high half the roughness (material.rs:27, 32)."""
    assert rc.f16_decode(0x3800) == 0.5 and rc.f16_decode(0x3801) == 0.5 + 2.0 ** -11
    m = H.material_new((1, 1, 1), 0.25, 0.75, (0, 0, 0), 1.5, 0.125)
    assert rc.f16_decode(m["metallic_roughness_f16"]) == 0.25 and rc.f16_decode(int(m["metallic_roughness_f16"]) >> 16) == 0.75
    assert rc.f16_decode(m["ior_transmission_f16"]) == 1.5 and rc.f16_decode(int(m["ior_transmission_f16"]) >> 16) == 0.125
