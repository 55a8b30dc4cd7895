"""What the ten batch calls share (rt_query.cpp, run_batch), asked of each of them in turn on the 12-triangle Cornell scene with 65
records, one wavefront plus one: a host batch and a device batch give the same bytes; a host input with a device output is rejected
with -1; a device input 4 bytes off its alignment is rejected with "aligned"; and rt_stats is the call's own after it."""
import ctypes as C

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

F32 = np.float32
N = 65
SAMPLES = 3


def _ptr(a):
    return C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


# the parameter records of the library calls, as the wrapper calls below fill them (kept alive here: the calls take their addresses)
AO, PATH, LIGHT = np.zeros((), T.AO_PARAMS), np.zeros((), T.PATH_PARAMS), np.zeros((), T.DIRECT_LIGHT_PARAMS)
AO["samples"], AO["seed"], AO["max_distance"], AO["bias"] = SAMPLES, 5, 1.0, 1e-3
PATH["samples"], PATH["max_bounces"], PATH["seed"] = SAMPLES, 2, 5
LIGHT["bias"] = 1e-3


# name -> (the records it takes, the wrapper call -> a tuple of outputs, the library call on (input, two output pointers), rt_stats.rays)
n_, zero = C.c_size_t(N), C.c_uint32(0)
CALLS = {
    "intersect": ("rays", lambda c, x: (c.intersect(x),), lambda c, i, o, o2: c.lib.rt_intersect(c._h, i, n_, o, zero), N),
    "occluded": ("rays", lambda c, x: (c.occluded(x),), lambda c, i, o, o2: c.lib.rt_occluded(c._h, i, n_, o, zero), N),
    "intersect_all": ("rays", lambda c, x: c.intersect_all(x, 2), lambda c, i, o, o2: c.lib.rt_intersect_all(c._h, i, n_, C.c_uint32(2), o, o2, zero), N),
    "surface": ("rays", lambda c, x: (c.surface(x),), lambda c, i, o, o2: c.lib.rt_surface(c._h, i, n_, o, zero), N),
    "ambient_occlusion": ("surface", lambda c, x: c.ambient_occlusion(x, SAMPLES, seed=5, max_distance=1.0),
                          lambda c, i, o, o2: c.lib.rt_ambient_occlusion(c._h, i, n_, _ptr(AO), o, o2), N * SAMPLES),
    "direct_light": ("surface", lambda c, x: (c.direct_light(x),), lambda c, i, o, o2: c.lib.rt_direct_light(c._h, i, n_, _ptr(LIGHT), o), None),
    "radiance": ("rays", lambda c, x: (c.radiance(x, samples=SAMPLES, max_bounces=2, seed=5),),
                 lambda c, i, o, o2: c.lib.rt_radiance(c._h, i, n_, _ptr(PATH), o), None),
    "radiance_sh": ("probes", lambda c, x: (c.radiance_sh(x, SAMPLES, max_bounces=2, seed=5),),
                    lambda c, i, o, o2: c.lib.rt_radiance_sh(c._h, i, n_, _ptr(PATH), o), None),
    "closest_point": ("points", lambda c, x: (c.closest_point(x),), lambda c, i, o, o2: c.lib.rt_closest_point(c._h, i, n_, o, zero), N),
    "sweep_sphere": ("sweeps", lambda c, x: (c.sweep_sphere(x),), lambda c, i, o, o2: c.lib.rt_sweep_sphere(c._h, i, n_, o, zero), N),
}


def _records(ctx, scene, kind):
    rays = np.ascontiguousarray(ctx.camera_rays(64, 48, scene.camera, mode=1)[1000:1000 + N])
    if kind == "rays":
        return rays
    points = ctx.surface(rays)
    assert (np.ascontiguousarray(points[:, 3]).view(np.uint32) != api.PRIM_MISS).sum() > N // 2
    if kind == "surface":
        return points
    inside = points[:, 0:3] + points[:, 4:7] * F32(0.25)  # off the walls
    if kind == "sweeps":
        return api.make_sweeps(inside, rays[:, 4:7], 0.05)
    return api.make_probes(inside) if kind == "probes" else api.make_points(inside)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_host_and_device_batches_checks_and_stats(gpu_ctx, name):
    if torch is None:
        pytest.skip("torch is not installed")
    kind, call, raw, want_rays = CALLS[name]
    scene = scenes.cornell12()
    gpu_ctx.upload_scene(scene)
    host_in = _records(gpu_ctx, scene, kind)
    assert host_in.shape[0] == N and host_in.dtype == F32
    gpu_ctx.render(64, 48, scene.camera, mode=1)  # another call's stats, for the batch call to replace
    # (a), (d): the same bytes from host memory and device memory, and the call's own rt_stats after either
    host_out = call(gpu_ctx, host_in)
    host_st = gpu_ctx.stats()
    dev_out = call(gpu_ctx, torch.from_numpy(host_in).to("cuda:0"))
    dev_st = gpu_ctx.stats()
    assert len(host_out) == len(dev_out)
    for h, d in zip(host_out, dev_out):
        assert d.device.type == "cuda" and d.cpu().numpy().tobytes() == h.tobytes()
    for st in (host_st, dev_st):
        assert st["pixels"] == 0 and st["kernel_ms"] > 0 and st["wall_ms"] > 0 and st["node_visits"] == 0 and st["tri_tests"] == 0
        if want_rays is not None:
            assert st["rays"] == want_rays and st["primary_rays"] == st["continuation_rays"] == st["shadow_rays"] == 0
        elif name == "direct_light":
            assert st["rays"] == st["shadow_rays"] > 0 and st["primary_rays"] == st["continuation_rays"] == 0
        else:
            assert st["primary_rays"] == N * SAMPLES and st["rays"] == st["primary_rays"] + st["continuation_rays"] + st["shadow_rays"]
    assert all(host_st[k] == dev_st[k] for k in ("rays", "primary_rays", "continuation_rays", "shadow_rays"))
    # (b): host records with device outputs
    out = torch.full((N * 28,), 7.0, device="cuda:0")
    out2 = torch.full((N,), 7, dtype=torch.int32, device="cuda:0")
    assert raw(gpu_ctx, _ptr(host_in), _ptr(out), _ptr(out2)) == -1
    assert name in gpu_ctx.lib.rt_last_error(gpu_ctx._h).decode()
    assert bool((out == 7).all()) and bool((out2 == 7).all()) and gpu_ctx.stats() == dev_st, "a rejected call changes nothing"
    # (c): device records 4 bytes past a 16-byte boundary
    cols = host_in.shape[1]
    skew = torch.zeros(N * cols + 4, device="cuda:0")[1:1 + N * cols].view(-1, cols)
    assert skew.data_ptr() % 16 == 4
    with pytest.raises(api.RtError) as e:
        call(gpu_ctx, skew)
    assert e.value.code == -1 and "aligned" in str(e.value)
    # ... and the context keeps working
    again = call(gpu_ctx, host_in)
    assert all(a.tobytes() == h.tobytes() for a, h in zip(again, host_out))
