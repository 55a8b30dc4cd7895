"""Surface and ambient-occlusion queries (rt_surface, rt_ambient_occlusion) at the C-ABI and Python boundary, without a GPU: the
symbols, the record layouts against the header's static asserts, the ctypes mirrors and the numpy dtypes, the header's constants
against api.py's, the argument check that needs no device, and the validation Context.surface / Context.ambient_occlusion do before
the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_surface", "rt_ambient_occlusion")


class RtRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtSurfacePoint(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("prim_id", C.c_uint32), ("normal", C.c_float * 3), ("material_id", C.c_uint32)]


class RtAoParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("max_distance", C.c_float), ("bias", C.c_float), ("flags", C.c_uint32),
                ("_pad", C.c_uint32 * 3)]


MIRRORS = {"rt_surface_point": (RtSurfacePoint, T.SURFACE_POINT), "rt_ao_params": (RtAoParams, T.AO_PARAMS)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert name in rt_api.ABI_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert re.search(r"int rt_surface\(rt_ctx\* ctx, const rt_ray\* rays, size_t n, rt_surface_point\* out, uint32_t flags\);", code)
    assert re.search(r"int rt_ambient_occlusion\(rt_ctx\* ctx, const rt_surface_point\* points, size_t n, const rt_ao_params\* params,\s*"
                     r"float\* visibility,\s*uint32_t\* unoccluded\);", code)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "sq_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [32, 32]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtSurfacePoint, f).offset for f in ("position", "prim_id", "normal", "material_id")] == [0, 12, 16, 28]
    assert [getattr(RtAoParams, f).offset for f in ("samples", "seed", "max_distance", "bias", "flags", "_pad")] == [0, 4, 8, 12, 16, 20]


def test_header_constants_equal_the_python_ones(rt_api):
    header = _header()
    most = re.search(r"^#define RT_AO_MAX_SAMPLES (\d+)u", header, re.M)
    chunk = re.search(r"^#define RT_QUERY_CHUNK (\d+)u", header, re.M)
    counters = re.search(r"^#define RT_QUERY_COUNTERS (\d+)u", header, re.M)
    assert most and int(most.group(1)) == rt_api.AO_MAX_SAMPLES == 4096
    assert chunk and int(chunk.group(1)) == rt_api.QUERY_CHUNK
    assert counters and int(counters.group(1)) == rt_api.QUERY_COUNTERS
    assert rt_api.QUERY_CHUNK % rt_api.AO_MAX_SAMPLES == 0  # a chunk of the largest sample count is a whole number of points


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    rays, pts, vis, cnt = (RtRay * 1)(), (RtSurfacePoint * 1)(), (C.c_float * 1)(), (C.c_uint32 * 1)()
    ap = RtAoParams(samples=4, seed=0, max_distance=float("inf"), bias=1e-3, flags=0)
    assert lib.rt_surface(C.c_void_p(0), rays, C.c_size_t(1), pts, C.c_uint32(0)) == -1
    assert lib.rt_surface(C.c_void_p(0), None, C.c_size_t(0), None, C.c_uint32(0)) == -1
    assert lib.rt_ambient_occlusion(C.c_void_p(0), pts, C.c_size_t(1), C.byref(ap), vis, cnt) == -1
    assert lib.rt_ambient_occlusion(C.c_void_p(0), None, C.c_size_t(0), None, None, None) == -1
    assert vis[0] == 0 and cnt[0] == 0 and not any(bytes(pts))


def _no_context(api):
    """A Context that holds no library and no rt_ctx: validation happens before the library is called."""
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_surface_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.surface
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8])
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, out=np.zeros((3, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 8), np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, out=np.zeros((8, 8), np.float32)[::2])


def test_ao_batches_are_validated_in_python_numpy(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.ambient_occlusion
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64), 4)
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros((4, 7), np.float32), 4)
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros(32, np.float32), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2], 4)
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8], 4)
    for bad in (0, 4097, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="samples"):
            call(nc, good, bad)
    for bad in (0.0, -1.0, float("nan"), -float("inf"), None):
        with pytest.raises(ValueError, match="max_distance"):
            call(nc, good, 4, max_distance=bad)
    for bad in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bias"):
            call(nc, good, 4, bias=bad)
    for bad in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="seed"):
            call(nc, good, 4, seed=bad)
    # out: (N,) float32, C-contiguous
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, out=np.zeros(3, np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 4, out=np.zeros((4, 1), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, out=np.zeros(4, np.float64))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, 4, out=np.zeros(8, np.float32)[::2])
    # counts: (N,) uint32, C-contiguous
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, counts=np.zeros(5, np.uint32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 4, counts=np.zeros((4, 1), np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, 4, counts=np.zeros(8, np.uint32)[::2])


def test_ao_batches_are_validated_in_python_torch(rt_api):
    torch = pytest.importorskip("torch")
    nc = _no_context(rt_api)
    call = rt_api.Context.ambient_occlusion
    good = torch.zeros(4, 8)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, torch.zeros(4, 8, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="shape"):
        call(nc, torch.zeros(4, 9), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, torch.zeros(8, 4).t(), 4)
    with pytest.raises(ValueError, match="samples"):
        call(nc, good, 4097)
    with pytest.raises(ValueError, match="max_distance"):
        call(nc, good, 4, max_distance=0.0)
    with pytest.raises(ValueError, match="bias"):
        call(nc, good, 4, bias=-1.0)
    with pytest.raises(TypeError, match="same kind"):
        call(nc, good, 4, out=np.zeros(4, np.float32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, good, 4, counts=np.zeros(4, np.uint32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, np.zeros((4, 8), np.float32), 4, out=torch.zeros(4))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, np.zeros((4, 8), np.float32), 4, counts=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, out=torch.zeros(5))
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, counts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, out=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(TypeError, match="same kind"):
        rt_api.Context.surface(nc, good, out=np.zeros((4, 8), np.float32))


class _RecordingLib:
    """Stands in for librt_hip.so: records the parameters of every rt_ambient_occlusion."""

    def __init__(self):
        self.calls = []

    def rt_ambient_occlusion(self, h, points, n, params, visibility, unoccluded):
        raw = (C.c_char * T.AO_PARAMS.itemsize).from_address(params.value)
        self.calls.append((n.value, np.frombuffer(raw, dtype=T.AO_PARAMS)[0].copy(), points.value, visibility.value, unoccluded.value))
        return 0


def test_ambient_occlusion_passes_its_parameters(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    pts = np.zeros((6, 8), np.float32)
    vis, cnt = ctx.ambient_occlusion(pts, 16)
    assert vis.shape == (6,) and vis.dtype == np.float32 and cnt.shape == (6,) and cnt.dtype == np.uint32
    own_v, own_c = np.zeros(6, np.float32), np.zeros(6, np.uint32)
    got = ctx.ambient_occlusion(pts, 4096, seed=0xFFFFFFFF, max_distance=2.5, bias=0.0, out=own_v, counts=own_c, counters=True)
    assert got[0] is own_v and got[1] is own_c
    (n0, p0, _, _, _), (n1, p1, a_pts, a_vis, a_cnt) = ctx.lib.calls
    assert n0 == n1 == 6
    assert (p0["samples"], p0["seed"], p0["max_distance"], p0["bias"], p0["flags"]) == (16, 0, np.inf, np.float32(1e-3), 0)
    assert (p1["samples"], p1["seed"], p1["max_distance"], p1["bias"], p1["flags"]) == (4096, 0xFFFFFFFF, 2.5, 0.0, rt_api.QUERY_COUNTERS)
    assert not p0["_pad"].any() and not p1["_pad"].any()
    assert (a_pts, a_vis, a_cnt) == (pts.ctypes.data, own_v.ctypes.data, own_c.ctypes.data)


def test_split_surface(rt_api):
    rec = np.zeros(3, T.SURFACE_POINT)
    rec["position"] = [[1, 2, 3], [4, 5, 6], [0, 0, 0]]
    rec["normal"] = [[0, 0, 1], [0, 1, 0], [0, 0, 0]]
    rec["prim_id"] = [7, 0x80000001, 0xFFFFFFFF]
    rec["material_id"] = [2, 3, 0]
    pts = rec.view(np.float32).reshape(3, 8)
    position, prim, normal, material = rt_api.split_surface(pts)
    assert prim.dtype == np.uint32 and material.dtype == np.uint32
    np.testing.assert_array_equal(position, rec["position"])
    np.testing.assert_array_equal(normal, rec["normal"])
    np.testing.assert_array_equal(prim, rec["prim_id"])
    np.testing.assert_array_equal(material, rec["material_id"])
    torch = pytest.importorskip("torch")
    _, tprim, tnormal, tmat = rt_api.split_surface(torch.from_numpy(pts.copy()))
    assert tprim.dtype == torch.int64 and tprim.tolist() == [7, 0x80000001, rt_api.PRIM_MISS] and tmat.tolist() == [2, 3, 0]
    assert tnormal.tolist() == rec["normal"].tolist()
