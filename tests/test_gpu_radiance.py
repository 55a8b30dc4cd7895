"""Path queries on the MI355X (rt_radiance), held to calls that already exist.

Against the frames: over the pixel-centre camera rays of a frame, with the frame's seed, the radiance is that pixel of the closed
extended-mode frame with one sample, bit for bit, for every bounce limit, with and without shadows, and the segments add up to the
frame's; composed per sample over rt_sample_rays it is the frame of several samples.  Against the queries: with no bounce it is
rt_direct_light at rt_surface's hit.  Against the closed forms of estimator_cases.py: the furnace, and rays aimed at the three
channels' critical angles, at the landing points of their refracted segments and at fixed incidences on the rough metal.  Against itself: the tree, the
device count, the kind of memory and the chunking change no byte."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import estimator_cases as ec
from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import hostpack as HP
from gpu_raytracer_amd import types as T
from test_gpu_direct_light import _geometric_facing

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
MISS = 0xFFFFFFFF
W, H = 64, 48
SEED = 7
SKY = np.array([0.1, 0.2, 0.3], F32)
MAGENTA = np.array([1.0, 0.0, 1.0], F32)
DIFFUSE, METAL, HALF_GLASS, GLASS, EMISSIVE = range(5)
PAST_TABLE = 9


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _soup(opaque=False):
    """A triangle soup with spheres, a directional, a point and a spot light, a diffuse, a metallic (roughness 0.8), a half and a fully
    transmissive and an emissive material, and every 97th triangle with a material id past the table.  opaque: no transmission."""
    base = scenes.random_soup(2000, n_spheres=3, n_lights=3)
    t_half, t_full = (0.0, 0.0) if opaque else (0.5, 1.0)
    materials = np.array([HP.material_new((0.8, 0.5, 0.3), 0.0, 0.5, (0, 0, 0), 1.5, 0.0), HP.material_new((0.9, 0.8, 0.6), 1.0, 0.8, (0, 0, 0), 1.5, 0.0),
                          HP.material_new((0.7, 0.9, 0.8), 0.0, 0.1, (0, 0, 0), 1.5, t_half), HP.material_new((0.95, 0.9, 0.85), 0.0, 0.0, (0, 0, 0), 1.45, t_full),
                          HP.material_new((0.4, 0.4, 0.6), 0.0, 0.9, (0.5, 0.4, 0.2), 1.5, 0.0)], dtype=T.MATERIAL)
    triangles = base.triangles.copy()
    triangles["material_id"][::97] = PAST_TABLE
    return dataclasses.replace(base, name="path soup", materials=materials, triangles=triangles)


@pytest.fixture(scope="module")
def scene_of():
    made = {}
    makers = {"cornell12": scenes.cornell12, "soup": _soup, "opaque": lambda: _soup(opaque=True)}

    def get(name):
        if name not in made:
            made[name] = makers[name]()
        return made[name]
    return get


def _incoherent_rays(scene, n, seed):
    """Rays from around the scene in random directions with ranges of their own, every 64th degenerate in one of four ways."""
    rng = np.random.default_rng(seed)
    p = scene.vertices["position"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    o = rng.uniform(lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), (n, 3)).astype(F32)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmin = rng.choice(np.array([0.0, 1e-5, 0.5, 2.0], F32), n)
    tmax = rng.choice(np.array([np.inf, 3.0, 6.0], F32), n)
    for k in range(8, n, 16 if len(scene.spheres) else n):  # every 16th ray starts a quarter unit off a sphere and points at its centre
        sp = scene.spheres[(k // 16) % len(scene.spheres)]
        o[k] = (sp["center"].astype(np.float64) - d[k] * (float(sp["radius"]) + 0.25)).astype(F32)
    rays = api.make_rays(o, d.astype(F32), tmin, tmax)
    rays[0::256, 1] = np.nan          # a NaN origin
    rays[64::256, 4:7] = 0            # a zero direction
    rays[128::256, 7] = rays[128::256, 3]  # an empty range
    rays[192::256, 5] = np.inf        # an infinite direction
    degenerate = np.zeros(n, bool)
    degenerate[0::64] = True
    return np.ascontiguousarray(rays), degenerate


# 1. the frames, 1 spp -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell12", "soup"])
def test_equals_the_closed_frame_of_one_sample_bit_for_bit(gpu_ctx, scene_of, name):
    scene = scene_of(name)
    gpu_ctx.upload_scene(scene)
    rays = gpu_ctx.camera_rays(W, H, scene.camera, mode=1)
    continuations = {}
    for bounces in (0, 1, 3, 9):
        for shadows in (True, False):
            st_f = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=1, max_bounces=bounces, frame_seed=SEED, no_shadows=not shadows)
            frame = gpu_ctx.read_rgb32f().reshape(-1, 3)
            got = gpu_ctx.radiance(rays, max_bounces=bounces, seed=SEED, shadows=shadows)
            st = gpu_ctx.stats()
            radiance, segments = api.split_radiance(got)
            np.testing.assert_array_equal(_bits(radiance), _bits(frame), err_msg=f"{name} max_bounces={bounces} shadows={shadows}")
            counts = [(st[k], st_f[k]) for k in ("rays", "primary_rays", "continuation_rays", "shadow_rays")]
            print(f"{name} max_bounces={bounces} shadows={shadows}: (query, frame) rays, primary, continuation, shadow {counts}")
            assert int(segments.astype(np.uint64).sum()) == st["rays"] == st_f["rays"]
            assert all(q == f for q, f in counts) and st["primary_rays"] == W * H and st["pixels"] == 0 and st["kernel_ms"] > 0
            assert st["node_visits"] == 0 and st["tri_tests"] == 0
            assert (st["shadow_rays"] > 0) == (shadows and len(scene.lights) > 0)
            if not shadows:
                continuations[bounces] = segments.astype(np.int64) - 1  # without shadow segments: the first and the continuations
    if name != "soup":
        return
    # what the soup covers, read from the first hits (rt_surface) and from the number of continuation segments
    _, prim, _, mid = api.split_surface(gpu_ctx.surface(rays))
    hit = prim != MISS
    shaded = hit & (mid < len(scene.materials))
    first = np.where(shaded, mid, 0).astype(np.int64)
    sky0 = gpu_ctx.radiance(rays, max_bounces=9, seed=SEED)
    assert (~hit).sum() > 50 and np.all(sky0[~hit, 0:3] == SKY) and np.all(_bits(sky0[~hit, 3]) == 1), "paths that end at a miss"
    assert (hit & ~shaded).sum() > 5 and np.all(sky0[hit & ~shaded, 0:3] == MAGENTA) and np.all(_bits(sky0[hit & ~shaded, 3]) == 1), "... at magenta"
    assert shaded.sum() > 1000 and np.all(continuations[0] == 0), "... at the terminal vertex (no bounce: every vertex is terminal)"
    absorbed = shaded & (continuations[1] == 0)  # a shaded vertex that is not terminal and has no continuation
    assert absorbed.any() and np.all(first[absorbed] == METAL), "... by absorption (a lobe direction below the surface)"
    glass = shaded & (first == GLASS)
    assert glass.sum() > 50 and np.all(continuations[1][glass] == 1), "paths that transmit (T = 1 always does)"
    assert (shaded & (first == HALF_GLASS)).sum() > 50
    for bounces in (3, 9):  # a path with three continuations scattered at its third vertex, where the roulette ran
        assert (continuations[bounces] >= 3).sum() > 50, f"the roulette runs at max_bounces={bounces}"
    assert continuations[9].max() > 3 and (continuations[9] < 9).sum() > 50 and continuations[3].max() == 3


# 2. the frames, 4 spp -----------------------------------------------------------------------------------------------------------
def test_composes_the_frame_of_four_samples_and_reduces_in_sample_order(gpu_ctx, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    spp, bounces = 4, 2
    st_f = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=spp, max_bounces=bounces, frame_seed=SEED)
    frame = gpu_ctx.read_rgb32f().reshape(-1, 3)
    total = np.zeros((W * H, 3), F32)
    segments = 0
    for s in range(spp):
        rays = gpu_ctx.sample_rays(W, H, scene.camera, s, spp=spp, frame_seed=SEED)
        x, seg = api.split_radiance(gpu_ctx.radiance(rays, max_bounces=bounces, seed=SEED, first_sample=s, camera_draws=True))
        total = total + x
        segments += int(seg.astype(np.uint64).sum())
    np.testing.assert_array_equal(_bits(total / F32(spp)), _bits(frame))
    assert segments == st_f["rays"]
    # the ordered reduction: one call of S samples is the f32 sum of S calls of one, from zero, in sample order, and one division
    rays = gpu_ctx.sample_rays(W, H, scene.camera, 0, spp=spp, frame_seed=SEED)
    for samples, first_sample in ((4, 0), (3, 5)):  # 3: the runs of a ray's samples cross the waves
        total, seg_total = np.zeros((W * H, 3), F32), np.zeros(W * H, np.uint32)
        for k in range(samples):
            x, seg = api.split_radiance(gpu_ctx.radiance(rays, max_bounces=bounces, seed=SEED, first_sample=first_sample + k, camera_draws=True))
            total, seg_total = total + x, seg_total + seg
        got, seg = api.split_radiance(gpu_ctx.radiance(rays, samples=samples, max_bounces=bounces, seed=SEED, first_sample=first_sample, camera_draws=True))
        st = gpu_ctx.stats()
        np.testing.assert_array_equal(_bits(got), _bits(total / F32(samples)), err_msg=f"samples={samples}")
        np.testing.assert_array_equal(seg, seg_total)
        assert st["rays"] == int(seg_total.astype(np.uint64).sum()) and st["primary_rays"] == W * H * samples
        assert len(np.unique(_bits(got), axis=0)) > 100  # (the samples differ: the sum is not one sample's)


# 3. composition on rays that are no camera rays -----------------------------------------------------------------------------------
def test_without_bounces_it_is_direct_light_at_the_surface_hit(gpu_ctx, scene_of):
    scene = scene_of("opaque")
    assert np.all(((scene.materials["ior_transmission_f16"] >> U32(16)) & U32(0xFFFF)).astype(np.uint16).view(np.float16) <= 0)
    gpu_ctx.upload_scene(scene)
    rays, degenerate = _incoherent_rays(scene, 2048, seed=33)
    pts = gpu_ctx.surface(rays)
    position, prim, _, mid = api.split_surface(pts)
    hit = prim != MISS
    assert not hit[degenerate].any() and hit.sum() > 500 and (~hit & ~degenerate).sum() > 100
    assert (hit & (rays[:, 3] > 0.1)).any() and (~hit & ~degenerate & np.isfinite(rays[:, 7])).any(), "ranges of their own, on both sides"
    # float64 facing of the unflipped geometric normal, from the scene's own arrays: a term within 1e-4 of zero may round either way
    cosang = np.zeros(len(rays))
    cosang[hit] = _geometric_facing(scene, rays[hit], prim[hit], position[hit])
    use = hit & (np.abs(cosang) >= 1e-4)
    left_out = 1.0 - use.sum() / hit.sum()
    print(f"{hit.sum()} hits, {left_out:.4f} left out, {(cosang[use] > 0).sum()} back faces, {(mid[use] >= len(scene.materials)).sum()} past the table")
    assert left_out <= 0.02 and (cosang[use] > 0).any() and (prim[use] >= 0x80000000).any()
    geo = pts.copy()
    geo[cosang > 0, 4:7] = -geo[cosang > 0, 4:7]  # rt_surface's face-forwarded normal turned back into the geometric one
    for shadows in (True, False):
        light, _ = api.split_lighting(gpu_ctx.direct_light(geo, bias=1e-3, ambient=True, shadows=shadows))
        got, segments = api.split_radiance(gpu_ctx.radiance(rays, max_bounces=0, seed=SEED, shadows=shadows))
        np.testing.assert_array_equal(_bits(got[use]), _bits((F32(0) + light[use]) / F32(1)), err_msg=f"shadows={shadows}")
        miss = ~hit & ~degenerate
        assert np.all(got[miss] == SKY) and np.all(segments[miss] == 1), "a miss within the range is the sky"
        assert not _bits(got[degenerate]).any() and not segments[degenerate].any(), "a degenerate ray is no path"
        assert np.all(segments[hit] >= 1) and (segments[hit] > 1).any() == shadows
        assert gpu_ctx.stats()["primary_rays"] == int((~degenerate).sum())


# 4. the closed form -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 1, 2])
def test_furnace_closed_form_from_interior_rays(gpu_ctx, bounces):
    """Every path in the furnace box IS sum_{k<B} E rho^k + rho^B (E + 0.1 rho), wherever it starts: within furnace_f32_rel_bound of it
    for one sample.  A path has B + 1 segments and any of them may escape (estimator_cases.py, ESCAPE_CAP: a vertex within 1e-5 of a
    second wall, a shared edge), the first one included - these rays are not a camera's - so at most ESCAPE_CAP of n (B + 1) rays are off."""
    case = ec.furnace(bounces)
    gpu_ctx.upload_scene(case.scene)
    n = 4096
    rng = np.random.default_rng(91)
    o = rng.uniform(0.05, 0.95, (n, 3)).astype(F32)
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    got, segments = api.split_radiance(gpu_ctx.radiance(api.make_rays(o, d.astype(F32)), max_bounces=bounces, seed=SEED))
    rel = np.abs(got.astype(np.float64) / ec.furnace_expected(bounces) - 1.0).max(-1)
    bound, allowed = ec.furnace_f32_rel_bound(bounces, 1), ec.escapes_allowed(n * (bounces + 1))
    off = int((rel > bound).sum())
    print(f"furnace B={bounces}: largest relative error {np.sort(rel)[-1 - off]:.3e} outside {off} rays, bound {bound:.3e}, allowed off {allowed}")
    assert off <= allowed
    assert int((segments != bounces + 1).sum()) <= off, "no lights: a path that does not escape has exactly B + 1 segments"


# 4b. step 4's geometry on aimed rays ----------------------------------------------------------------------------------------------
def _cone_rays(origin, cos_theta, phi):
    """f32 rays from `origin` whose y component is cos_theta (negative: downward) at azimuth phi about the y axis."""
    cos_theta, phi = np.broadcast_arrays(np.asarray(cos_theta, np.float64), np.asarray(phi, np.float64))
    s = np.sqrt(1.0 - cos_theta ** 2)
    d = np.stack([s * np.cos(phi), cos_theta, s * np.sin(phi)], -1)
    return api.make_rays(np.broadcast_to(np.asarray(origin, F32), d.shape), d.astype(F32))


def test_total_reflection_at_aimed_incidences(gpu_ctx):
    """The tir_back scene from below, samples = 1, max_bounces = 1: for each channel c, 4096 rays whose incidence puts
    x_c = ior_c^2 sin^2(theta) evenly across 1 +- 2e-3 - which no frame's pixel grid can aim at.  x_c is taken in float64 from the
    f32 direction that is passed; outside |x_c - 1| < 1e-5 (0.5 % of the rays aimed at that channel) the value names the hero channel
    and the branch (estimator_cases.check_hero_candidates), and every path has its two segments."""
    case = ec.tir_back()
    gpu_ctx.upload_scene(case.scene)
    n = 4096
    rng = np.random.default_rng(17)
    delta = (np.arange(n) + 0.5) / n * 4e-3 - 2e-3
    rays = np.concatenate([_cone_rays((0.0, 0.5, 0.0), np.sqrt(1.0 - (1.0 + delta) / ec.IOR_C[c] ** 2), rng.uniform(0, 2 * np.pi, n)) for c in range(3)])
    d = rays[:, 4:7].astype(np.float64)
    values, unsure, x = ec.tir_back_values(d)
    for c in range(3):
        aimed = x[c * n:(c + 1) * n, c] - 1.0
        assert abs(aimed.min() + 2e-3) < 1e-5 and abs(aimed.max() - 2e-3) < 1e-5 and 0.4 < (aimed > 0).mean() < 0.6
    got, segments = api.split_radiance(gpu_ctx.radiance(np.ascontiguousarray(rays), samples=1, max_bounces=1, seed=SEED))
    res = ec.check_hero_candidates("tir_back, aimed rays", got, values, unsure, {v: ec.tir_back_values(d, v)[0] for v in ec.TIR_VARIANTS})
    assert res["left_out"] <= 0.006
    assert np.all(segments == 2)
    heroes = (got != 0).sum(0)
    print(f"hero counts {heroes}")
    assert heroes.min() > 3000   # every channel is some paths' hero: all three critical angles are exercised


def test_refraction_at_aimed_landing_points(gpu_ctx):
    """The refract_front scene from above at 20, 55 and 75 degrees of incidence: for each incidence and channel c, 1024 rays whose
    channel-c segment lands evenly across X0 +- 2e-2; classified from the f32 rays that are passed, outside 1e-4 of X0."""
    case = ec.refract_front()
    gpu_ctx.upload_scene(case.scene)
    n = 1024
    rng = np.random.default_rng(18)
    u = (np.arange(n) + 0.5) / n * 4e-2 - 2e-2
    batches = []
    for theta in (20.0, 55.0, 75.0):
        th = np.radians(theta)
        d = np.array([np.sin(th), -np.cos(th), 0.0])
        for c in range(3):
            t, _, _ = ec.snell(d, np.array([0.0, 1.0, 0.0]), 1.0 / ec.IOR_C[c])
            glass_x = ec.REFRACT_X0 + u - (ec.GLASS_Y - ec.ORIGIN_EPS) * t[0] / -t[1]
            o = np.stack([glass_x - np.tan(th), np.full(n, ec.GLASS_Y + 1.0), rng.uniform(-0.05, 0.05, n)], -1)
            batches.append(api.make_rays(o.astype(F32), np.broadcast_to(d.astype(F32), o.shape)))
    rays = np.ascontiguousarray(np.concatenate(batches))
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
    values, unsure, land = ec.refract_front_values(o, d)
    for k in range(9):
        aimed = land[k * n:(k + 1) * n, k % 3] - ec.REFRACT_X0
        assert abs(aimed.min() + 2e-2) < 1e-4 and abs(aimed.max() - 2e-2) < 1e-4
    got, segments = api.split_radiance(gpu_ctx.radiance(rays, samples=1, max_bounces=1, seed=SEED))
    ec.check_hero_candidates("refract_front, aimed rays", got, values, unsure, {v: ec.refract_front_values(o, d, v)[0] for v in ec.REFRACT_VARIANTS})
    assert np.all(segments == 2)


@pytest.mark.parametrize("roughness,layout", [(1.0, "front"), (0.5, "backface")])
def test_rough_lobe_cap_at_fixed_incidences(gpu_ctx, roughness, layout):
    """The rough_metal scene: 256 rays at each of c = r . Nf = 0.1, 0.3, 0.5, 0.7, 0.9, 256 samples each.  Every ray is a sky k / 256
    with k the samples that were not absorbed, it traced 256 + k segments, and the mean of k / 256 over an incidence's 65,536 samples
    is 1 - max(0, (1 - c / roughness) / 2) within Hoeffding's band (0.0128 at p = 1e-9); where the cap is empty k = 256."""
    case = ec.rough_metal(roughness, layout)
    gpu_ctx.upload_scene(case.scene)
    n, samples = 256, 256
    rng = np.random.default_rng(19)
    cs = (0.1, 0.3, 0.5, 0.7, 0.9)
    rays = np.ascontiguousarray(np.concatenate([_cone_rays((0.5, 2.0, 0.0), np.full(n, -c), rng.uniform(-0.3, 0.3, n)) for c in cs]))
    got, segments = api.split_radiance(gpu_ctx.radiance(rays, samples=samples, max_bounces=1, seed=SEED))
    full = ec.MIRROR_A * ec.SKY
    k = np.rint(got[:, 0].astype(np.float64) * samples / full[0])
    err = np.abs(got.astype(np.float64) - (k / samples)[:, None] * full)
    tol = ec.mirror_f32_rel_bound(samples) * full
    print(f"largest |value - a sky k / {samples}| {err.max(0)}, tolerance {tol}")
    assert (err <= tol).all()
    np.testing.assert_array_equal(segments.astype(np.int64), samples + k.astype(np.int64))
    band = float(ec.hoeffding_eps(1.0, n * samples))
    for i, c in enumerate(cs):
        c32 = -rays[i * n:(i + 1) * n, 5].astype(np.float64)
        want = float((1.0 - ec.rough_cap(c32, roughness)).mean())
        share = k[i * n:(i + 1) * n].mean() / samples
        print(f"c = {c}: continuing share {share:.4f}, expected {want:.4f}, band {band:.4f}, nothing absorbed 1.0")
        assert abs(share - want) <= band
        if c < roughness - 0.05:
            assert 1.0 - want >= 2 * band   # the band rejects 'nothing absorbed'
        if c > roughness + 0.05:
            assert np.all(k[i * n:(i + 1) * n] == samples)


# 5. independence ----------------------------------------------------------------------------------------------------------------
def test_memory_kinds_devices_tree_and_updates(gpu_ctx, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    rays = np.ascontiguousarray(np.concatenate([gpu_ctx.camera_rays(W, H, scene.camera, mode=1), _incoherent_rays(scene, 1000, seed=5)[0]]))
    kw = dict(samples=2, max_bounces=3, seed=SEED, first_sample=3)
    want = gpu_ctx.radiance(rays, **kw)
    st_one = gpu_ctx.stats()
    own = np.full((len(rays), 4), 7, F32)
    assert gpu_ctx.radiance(rays, out=own, **kw) is own and own.tobytes() == want.tobytes()
    if torch is not None:
        dev = torch.from_numpy(rays).to("cuda:0") * 1.0  # produced by a kernel on torch's stream
        got = gpu_ctx.radiance(dev, **kw)
        assert got.device == dev.device and got.dtype == torch.float32 and tuple(got.shape) == (len(rays), 4)
        assert got.cpu().numpy().tobytes() == want.tobytes()
        assert gpu_ctx.radiance(torch.from_numpy(rays.copy()), **kw).numpy().tobytes() == want.tobytes()
        np.testing.assert_array_equal(api.split_radiance(got)[1].cpu().numpy(), api.split_radiance(want)[1].astype(np.int64))
    with api.Context((0, 0)) as two:  # each device gets a contiguous range of the rays; the seed's index stays the caller's
        two.upload_scene(scene)
        assert two.radiance(rays, **kw).tobytes() == want.tobytes()
        st_two = two.stats()
        assert all(st_two[k] == st_one[k] for k in ("rays", "primary_rays", "continuation_rays", "shadow_rays"))
    gpu_ctx.prepare(api.PREPARE_QUALITY_TREE)
    assert gpu_ctx.stats()["tree_build"] == 0
    assert gpu_ctx.radiance(rays, **kw).tobytes() == want.tobytes()
    gpu_ctx.prepare()  # light grids on the device: never looked at
    assert gpu_ctx.radiance(rays, **kw).tobytes() == want.tobytes()
    # after a vertex update the call walks the refitted tree: the result of a fresh upload of the moved scene
    pos = scene.vertices["position"].astype(F32)
    moved_pos = np.ascontiguousarray(pos + F32(0.2) * np.sin(pos[:, ::-1] * F32(3.0)), dtype=F32)
    v = scene.vertices.copy()
    v["position"] = moved_pos
    assert gpu_ctx.update_geometry(vertices=moved_pos)["flags"] & (api.STAT_REFIT | api.STAT_REBUILT)
    after = gpu_ctx.radiance(rays, **kw)
    with api.Context() as fresh:
        fresh.upload_scene(dataclasses.replace(scene, vertices=v))
        assert fresh.radiance(rays, **kw).tobytes() == after.tobytes()
    assert after.tobytes() != want.tobytes()


def test_host_batch_across_a_chunk_boundary(gpu_ctx, scene_of):
    """With 4096 samples a chunk is RT_QUERY_CHUNK / 4096 = 1024 rays: 1100 rays are two chunks, and the second one's rays keep the
    seeds of their places in the caller's array."""
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    samples = api.PATH_MAX_SAMPLES
    chunk = api.QUERY_CHUNK // samples
    rays = np.ascontiguousarray(gpu_ctx.camera_rays(W, H, scene.camera, mode=1)[1000:1000 + chunk + 76])
    kw = dict(samples=samples, max_bounces=1, first_sample=2)
    whole = gpu_ctx.radiance(rays, seed=SEED, **kw)
    st = gpu_ctx.stats()
    assert st["primary_rays"] == len(rays) * samples and st["rays"] == int(api.split_radiance(whole)[1].astype(np.uint64).sum())
    head = gpu_ctx.radiance(np.ascontiguousarray(rays[:chunk]), seed=SEED, **kw)
    tail = gpu_ctx.radiance(np.ascontiguousarray(rays[chunk:]), seed=SEED + chunk, **kw)
    assert whole[:chunk].tobytes() == head.tobytes() and whole[chunk:].tobytes() == tail.tobytes()
    assert gpu_ctx.radiance(np.ascontiguousarray(rays[chunk:]), seed=SEED, **kw).tobytes() != tail.tobytes()
    if torch is not None:
        dev = gpu_ctx.radiance(torch.from_numpy(rays).to("cuda:0"), seed=SEED, **kw)
        assert dev.cpu().numpy().tobytes() == whole.tobytes()
    with api.Context((0, 0)) as two:
        two.upload_scene(scene)
        assert two.radiance(rays, seed=SEED, **kw).tobytes() == whole.tobytes()


def test_device_batch_across_a_chunk_boundary(gpu_ctx, scene_of):
    """A device batch of two chunks (1024 rays and 5) is timed by one event pair around both launches, where the host batch has a pair
    per chunk: the bytes are the host batch's, and the pair has measured something."""
    if torch is None:
        pytest.skip("torch is not installed")
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    samples = api.PATH_MAX_SAMPLES
    n = api.QUERY_CHUNK // samples + 5
    assert n == 1029
    rays = np.ascontiguousarray(gpu_ctx.camera_rays(W, H, scene.camera, mode=1)[1000:1000 + n])
    kw = dict(samples=samples, max_bounces=1, seed=SEED, first_sample=2)
    whole = gpu_ctx.radiance(rays, **kw)
    host = gpu_ctx.stats()
    dev = gpu_ctx.radiance(torch.from_numpy(rays).to("cuda:0"), **kw)
    st = gpu_ctx.stats()
    assert dev.cpu().numpy().tobytes() == whole.tobytes()
    assert st["kernel_ms"] > 0
    assert st["primary_rays"] == n * samples and all(st[k] == host[k] for k in ("rays", "continuation_rays", "shadow_rays"))


# 6. edges -----------------------------------------------------------------------------------------------------------------------
def test_edges(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    gpu_ctx.upload_scene(scene)
    rays = gpu_ctx.camera_rays(W, H, scene.camera, mode=1)
    assert gpu_ctx.radiance(np.zeros((0, 8), F32)).shape == (0, 4)
    whole = gpu_ctx.radiance(rays[:130], samples=3, seed=SEED)
    for n in (1, 21, 22, 63, 64, 65):  # 3 n around the wave's 64 lanes
        assert gpu_ctx.radiance(np.ascontiguousarray(rays[:n]), samples=3, seed=SEED).tobytes() == whole[:n].tobytes()
    # counters change no byte
    plain = gpu_ctx.radiance(rays, max_bounces=3, seed=SEED)
    assert gpu_ctx.stats()["node_visits"] == 0
    counted = gpu_ctx.radiance(rays, max_bounces=3, seed=SEED, counters=True)
    st = gpu_ctx.stats()
    assert st["node_visits"] > 0 and st["tri_tests"] > 0 and counted.tobytes() == plain.tobytes()
    # no lights: the frame still, and no shadow segment
    gpu_ctx.upload_scene(dataclasses.replace(scene, lights=np.zeros(0, T.LIGHT)))
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=1, max_bounces=2, frame_seed=SEED)
    frame = gpu_ctx.read_rgb32f().reshape(-1, 3)
    got = gpu_ctx.radiance(rays, max_bounces=2, seed=SEED)
    assert gpu_ctx.stats()["shadow_rays"] == 0 and gpu_ctx.stats()["continuation_rays"] > 0
    np.testing.assert_array_equal(_bits(got[:, 0:3]), _bits(frame))
    # 33 lights: more than the pipeline takes - the frame falls back to the megakernel - and no limit here
    gpu_ctx.upload_scene(dataclasses.replace(scene, lights=np.repeat(scene.lights, 33)))
    st_f = gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=1, max_bounces=2, frame_seed=SEED)
    assert st_f["flags"] & api.STAT_MEGAKERNEL_FALLBACK
    frame = gpu_ctx.read_rgb32f().reshape(-1, 3)
    got = gpu_ctx.radiance(rays, max_bounces=2, seed=SEED)
    st = gpu_ctx.stats()
    np.testing.assert_array_equal(_bits(got[:, 0:3]), _bits(frame))
    assert st["rays"] == st_f["rays"] and st["shadow_rays"] == st_f["shadow_rays"] > 0
    # an empty scene: all sky, one segment per sample
    gpu_ctx.upload_scene(scenes.empty_scene())
    radiance, segments = api.split_radiance(gpu_ctx.radiance(rays, samples=5, seed=SEED))
    total = np.zeros(3, F32)
    for _ in range(5):
        total = total + SKY
    assert np.all(radiance == total / F32(5)) and np.all(segments == 5)
    assert np.all(api.split_radiance(gpu_ctx.radiance(rays, seed=SEED))[0] == SKY)


def test_the_frame_and_a_running_accumulation_are_left_alone(gpu_ctx, scene_of):
    scene = scene_of("soup")
    gpu_ctx.upload_scene(scene)
    rays = gpu_ctx.camera_rays(W, H, scene.camera, mode=1)
    gpu_ctx.render(W, H, scene.camera, mode=1)
    rgb, comb, hits = gpu_ctx.read_rgb32f(), gpu_ctx.read_rgba8_combined(), gpu_ctx.read_hits()
    gpu_ctx.radiance(rays, samples=2)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.read_rgba8_combined().tobytes() == comb.tobytes()
    again = gpu_ctx.read_hits()
    assert again[0].tobytes() == hits[0].tobytes() and again[1].tobytes() == hits[1].tobytes()
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    rgb, samples = gpu_ctx.read_rgb32f(), gpu_ctx.accumulated_samples()
    assert samples == 2
    gpu_ctx.radiance(rays, samples=2, counters=True)
    assert gpu_ctx.read_rgb32f().tobytes() == rgb.tobytes() and gpu_ctx.accumulated_samples() == samples
    gpu_ctx.render(W, H, scene.camera, mode=api.MODE_EXTENDED, spp=2, accumulate=True)
    assert gpu_ctx.accumulated_samples() == 4


def test_the_librarys_own_checks(gpu_ctx, scene_of):
    scene = scene_of("cornell12")
    rays, out = np.zeros((64, 8), F32), np.full((64, 4), 7, F32)
    rays[:, 2], rays[:, 3], rays[:, 6], rays[:, 7] = 3.0, 1e-5, -1.0, np.inf
    pp = np.zeros((), T.PATH_PARAMS)
    pp["samples"], pp["max_bounces"] = 1, 2
    lib, h = gpu_ctx.lib, gpu_ctx._h
    call = lambda r, n, a, o: lib.rt_radiance(h, C.c_void_p(r), C.c_size_t(n), C.c_void_p(a), C.c_void_p(o))
    assert call(rays.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == -4  # before any upload
    assert call(0, 0, 0, 0) == 0  # n == 0 (even then)
    gpu_ctx.upload_scene(scene)
    gpu_ctx.render(W, H, scene.camera, mode=1)
    before = gpu_ctx.stats()
    assert call(0, 0, 0, 0) == 0
    assert call(0, 64, pp.ctypes.data, out.ctypes.data) == -1 and "rays" in lib.rt_last_error(h).decode()
    assert call(rays.ctypes.data, 64, 0, out.ctypes.data) == -1 and "params" in lib.rt_last_error(h).decode()
    assert call(rays.ctypes.data, 64, pp.ctypes.data, 0) == -1 and "out" in lib.rt_last_error(h).decode()
    bad = [("samples", 0), ("samples", api.PATH_MAX_SAMPLES + 1), ("max_bounces", api.MAX_BOUNCES + 1), ("first_sample", 0xFFFFFFFF), ("flags", 2), ("flags", 4),
           ("flags", 16), ("flags", 128), ("flags", 1 << 31)]
    for field, value in bad:
        p = pp.copy()
        p[field] = value
        if field == "first_sample":
            p["samples"] = 2  # 2^32 - 1 + 2
        assert call(rays.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == -1, (field, value)
        assert field in lib.rt_last_error(h).decode() or field == "flags"
    assert np.all(out == 7) and gpu_ctx.stats() == before, "a rejected call changes nothing"
    p = pp.copy()
    p["first_sample"], p["samples"] = (1 << 32) - 2, 2  # the last two samples there are
    assert call(rays.ctypes.data, 64, p.ctypes.data, out.ctypes.data) == 0
    assert gpu_ctx.stats()["primary_rays"] == 128 and np.all(_bits(out[:, 3]) >= 2)
    if torch is not None:
        dev = torch.from_numpy(rays).to("cuda:0")
        skew = torch.zeros(64 * 8 + 4, device="cuda:0")[1:1 + 64 * 8].view(-1, 8)
        with pytest.raises(api.RtError) as e:
            gpu_ctx.radiance(skew)
        assert e.value.code == -1 and "aligned" in str(e.value)
        host = np.full((64, 4), 7, F32)
        assert call(dev.data_ptr(), 64, pp.ctypes.data, host.ctypes.data) == -1 and np.all(host == 7)  # device rays, host out
        assert call(rays.ctypes.data, 64, pp.ctypes.data, out.ctypes.data) == 0
        assert gpu_ctx.radiance(dev, max_bounces=2).cpu().numpy().tobytes() == out.tobytes()
