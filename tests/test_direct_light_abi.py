"""Direct-light queries (rt_direct_light) at the C-ABI and Python boundary, without a GPU: the symbol, the record layouts against the
header's static asserts, the ctypes mirrors and the numpy dtypes, the header's constants against api.py's, the argument check that
needs no device, and what Context.direct_light validates and passes on before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RtSurfacePoint(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("prim_id", C.c_uint32), ("normal", C.c_float * 3), ("material_id", C.c_uint32)]


class RtLighting(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("lit_mask", C.c_uint32)]


class RtDirectLightParams(C.Structure):
    _fields_ = [("bias", C.c_float), ("flags", C.c_uint32), ("_pad", C.c_uint32 * 2)]


MIRRORS = {"rt_lighting": (RtLighting, T.LIGHTING), "rt_direct_light_params": (RtDirectLightParams, T.DIRECT_LIGHT_PARAMS)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_direct_light" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_direct_light")
    assert re.search(r"int rt_direct_light\(rt_ctx\* ctx, const rt_surface_point\* points, size_t n, const rt_direct_light_params\* params, "
                     r"rt_lighting\* out\);", code)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "dl_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [16, 16]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtLighting, f).offset for f in ("radiance", "lit_mask")] == [0, 12]
    assert [getattr(RtDirectLightParams, f).offset for f in ("bias", "flags", "_pad")] == [0, 4, 8]
    # the header asserts them itself
    header = _header()
    assert "RT_STATIC_ASSERT(sizeof(rt_lighting) == 16" in header and "RT_STATIC_ASSERT(sizeof(rt_direct_light_params) == 16" in header


def test_header_constants_equal_the_python_ones_and_are_distinct_flags(rt_api):
    header = _header()
    value = lambda name: int(re.search(r"^#define %s (\d+)u" % name, header, re.M).group(1))
    assert value("RT_DIRECT_AMBIENT") == rt_api.DIRECT_AMBIENT == 4
    assert value("RT_DIRECT_NO_SHADOWS") == rt_api.DIRECT_NO_SHADOWS == 8
    assert value("RT_DIRECT_NO_SHADOW_GRID") == rt_api.DIRECT_NO_SHADOW_GRID == 16
    assert value("RT_DIRECT_MAX_LIGHTS") == rt_api.DIRECT_MAX_LIGHTS == 32
    flags = [value(n) for n in ("RT_QUERY_COUNTERS", "RT_QUERY_COUNT_ALL", "RT_DIRECT_AMBIENT", "RT_DIRECT_NO_SHADOWS", "RT_DIRECT_NO_SHADOW_GRID")]
    assert all(f and f & (f - 1) == 0 for f in flags) and len(set(flags)) == len(flags), "single, distinct bits"
    assert value("RT_QUERY_COUNTERS") == rt_api.QUERY_COUNTERS and value("RT_QUERY_COUNT_ALL") == rt_api.QUERY_COUNT_ALL


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    pts, out = (RtSurfacePoint * 1)(), (RtLighting * 1)()
    dp = RtDirectLightParams(bias=1e-3, flags=0)
    assert lib.rt_direct_light(C.c_void_p(0), pts, C.c_size_t(1), C.byref(dp), out) == -1
    assert lib.rt_direct_light(C.c_void_p(0), None, C.c_size_t(0), None, None) == -1
    assert not any(bytes(out))


def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.direct_light
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8])
    for bad in (-1e-3, float("nan"), float("inf"), None, "x"):
        with pytest.raises(ValueError, match="bias"):
            call(nc, good, bias=bad)
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, out=np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 4), np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, out=np.zeros((8, 4), np.float32)[::2])
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="same kind"):
        call(nc, torch.zeros(4, 8), out=np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, good, out=torch.zeros(4, 4))


class _RecordingLib:
    """Stands in for librt_hip.so: records the parameters of every rt_direct_light."""

    def __init__(self):
        self.calls = []

    def rt_direct_light(self, h, points, n, params, out):
        raw = (C.c_char * T.DIRECT_LIGHT_PARAMS.itemsize).from_address(params.value)
        self.calls.append((n.value, np.frombuffer(raw, dtype=T.DIRECT_LIGHT_PARAMS)[0].copy(), points.value, out.value))
        return 0


def test_direct_light_passes_its_parameters(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    pts = np.zeros((6, 8), np.float32)
    got = ctx.direct_light(pts)
    assert got.shape == (6, 4) and got.dtype == np.float32
    own = np.zeros((6, 4), np.float32)
    assert ctx.direct_light(pts, bias=0.0, ambient=True, shadows=False, use_grids=False, out=own, counters=True) is own
    (n0, p0, _, _), (n1, p1, a_pts, a_out) = ctx.lib.calls
    assert n0 == n1 == 6
    assert (p0["bias"], p0["flags"]) == (np.float32(1e-3), 0)
    assert p0["bias"].tobytes() == np.float32(1e-3).tobytes(), "the default bias is the one the light grids were derived for"
    assert (p1["bias"], p1["flags"]) == (0.0, rt_api.DIRECT_AMBIENT | rt_api.DIRECT_NO_SHADOWS | rt_api.DIRECT_NO_SHADOW_GRID | rt_api.QUERY_COUNTERS)
    assert not p0["_pad"].any() and not p1["_pad"].any()
    assert (a_pts, a_out) == (pts.ctypes.data, own.ctypes.data)


def test_split_lighting(rt_api):
    rec = np.zeros(3, T.LIGHTING)
    rec["radiance"] = [[1, 2, 3], [0.5, 0.25, 0], [1, 0, 1]]
    rec["lit_mask"] = [5, 0x80000001, 0]
    lighting = rec.view(np.float32).reshape(3, 4)
    radiance, mask = rt_api.split_lighting(lighting)
    assert mask.dtype == np.uint32
    np.testing.assert_array_equal(radiance, rec["radiance"])
    np.testing.assert_array_equal(mask, rec["lit_mask"])
    torch = pytest.importorskip("torch")
    tr, tm = rt_api.split_lighting(torch.from_numpy(lighting.copy()))
    assert tm.dtype == torch.int64 and tm.tolist() == [5, 0x80000001, 0] and tr.tolist() == rec["radiance"].tolist()
