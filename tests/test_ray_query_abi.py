"""Ray queries (rt_intersect / rt_occluded / rt_camera_rays) at the C-ABI and Python boundary, without a GPU: the symbols,
the record layouts against the header's static asserts, argument checks that need no device, and the batch helpers of api.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RtRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_id", C.c_uint32)]


def test_query_symbols_are_exported_and_listed(rt_api):
    lib = rt_api.load()
    for name in ("rt_intersect", "rt_occluded", "rt_camera_rays"):
        assert name in rt_api.ABI_SYMBOLS
        assert hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "#define RT_QUERY_COUNTERS 1u" in header and rt_api.QUERY_COUNTERS == 1
    assert "#define RT_QUERY_CHUNK 4194304u" in header and rt_api.QUERY_CHUNK == 4194304


def test_record_layout_from_ctypes():
    assert C.sizeof(RtRay) == 32 and C.sizeof(RtHit) == 16
    assert [RtRay.origin.offset, RtRay.tmin.offset, RtRay.direction.offset, RtRay.tmax.offset] == [0, 12, 16, 28]
    assert [RtHit.t.offset, RtHit.u.offset, RtHit.v.offset, RtHit.prim_id.offset] == [0, 4, 8, 12]


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layout_from_the_header(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirror's."""
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(rt_ray), '
           'offsetof(rt_ray, tmin), offsetof(rt_ray, direction), offsetof(rt_ray, tmax), sizeof(rt_hit), offsetof(rt_hit, u), '
           'offsetof(rt_hit, v), offsetof(rt_hit, prim_id));return 0;}\n')
    exe = str(tmp_path / "rq_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    assert list(map(int, subprocess.check_output([exe]).split())) == [32, 12, 16, 28, 16, 4, 8, 12]


def test_null_context_queries_return_bad_arg(rt_api):
    lib = rt_api.load()
    null = C.c_void_p(0)
    rays = (RtRay * 1)()
    hits = (RtHit * 1)()
    occ = (C.c_uint8 * 1)()
    assert lib.rt_intersect(null, rays, C.c_size_t(1), hits, C.c_uint32(0)) == -1
    assert lib.rt_occluded(null, rays, C.c_size_t(1), occ, C.c_uint32(0)) == -1
    cam = np.zeros((), dtype=T.CAMERA)
    assert lib.rt_camera_rays(null, C.c_void_p(cam.ctypes.data), C.c_uint32(4), C.c_uint32(4), C.c_uint32(0), rays) == -1


def test_make_rays_and_split_hits_round_trip_numpy(rt_api):
    rng = np.random.default_rng(3)
    o = rng.standard_normal((37, 3)).astype(np.float32)
    d = rng.standard_normal((37, 3)).astype(np.float32)
    tmax = rng.random(37).astype(np.float32) + 1
    r = rt_api.make_rays(o, d, tmin=0.5, tmax=tmax)
    assert r.dtype == np.float32 and r.shape == (37, 8) and r.flags.c_contiguous
    assert np.array_equal(r[:, 0:3], o) and np.array_equal(r[:, 4:7], d)
    assert np.all(r[:, 3] == np.float32(0.5)) and np.array_equal(r[:, 7], tmax)
    assert np.all(np.isinf(rt_api.make_rays(o, d)[:, 7])) and np.all(rt_api.make_rays(o, d)[:, 3] == np.float32(1e-5))
    prim = np.array([0, 7, 0x80000002, 0xFFFFFFFF], np.uint32)
    hits = np.zeros((4, 4), np.float32)
    hits[:, 0], hits[:, 1], hits[:, 2] = [1, 2, 3, 4], [0.25] * 4, [0.5] * 4
    hits[:, 3] = prim.view(np.float32)
    t, u, v, p = rt_api.split_hits(hits)
    assert p.dtype == np.uint32 and np.array_equal(p, prim)
    assert np.array_equal(t, [1, 2, 3, 4]) and np.all(u == 0.25) and np.all(v == 0.5)


def test_make_rays_and_split_hits_round_trip_torch(rt_api):
    torch = pytest.importorskip("torch")
    o = torch.randn(9, 3)
    d = torch.randn(9, 3)
    r = rt_api.make_rays(o, d, tmin=0.25, tmax=torch.full((9,), 3.0))
    assert isinstance(r, torch.Tensor) and r.dtype == torch.float32 and tuple(r.shape) == (9, 8) and r.is_contiguous()
    assert torch.equal(r[:, 0:3], o) and torch.equal(r[:, 4:7], d) and bool((r[:, 3] == 0.25).all()) and bool((r[:, 7] == 3).all())
    prim = np.array([0, 5, 0x80000000, 0xFFFFFFFF], np.uint32)
    hits = torch.zeros(4, 4)
    hits[:, 3] = torch.from_numpy(prim.view(np.float32).copy())
    _, _, _, p = rt_api.split_hits(hits)
    assert p.dtype == torch.int64 and p.tolist() == [0, 5, 0x80000000, 4294967295]


def _no_context(api):
    """A Context that holds no library and no rt_ctx: validation happens before the library is called."""
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


@pytest.mark.parametrize("method", ["intersect", "occluded"])
def test_batches_are_validated_in_python(rt_api, method):
    call = getattr(rt_api.Context, method)
    nc = _no_context(rt_api)
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros(32, np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2])
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.asfortranarray(np.zeros((4, 8), np.float32)))
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8])
    bad_out = np.zeros((3, 4), np.float32) if method == "intersect" else np.zeros(3, bool)
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, out=bad_out)
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="dtype"):
        call(nc, torch.zeros(4, 8, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        call(nc, torch.zeros(4, 9))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, torch.zeros(8, 4).t())
    with pytest.raises(TypeError, match="same kind"):
        call(nc, torch.zeros(4, 8), out=np.zeros((4, 4), np.float32))
