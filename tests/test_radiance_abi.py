"""Path queries (rt_radiance) at the C-ABI and Python boundary, without a GPU: the symbol, the record layouts against the header's
static asserts, the ctypes mirrors and the numpy dtypes, the header's constants against api.py's, the argument check that needs no
device, and what Context.radiance validates and passes on before the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RtRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtPathParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("max_bounces", C.c_uint32), ("seed", C.c_uint32), ("first_sample", C.c_uint32), ("flags", C.c_uint32),
                ("_pad", C.c_uint32 * 3)]


class RtPathResult(C.Structure):
    _fields_ = [("radiance", C.c_float * 3), ("segments", C.c_uint32)]


MIRRORS = {"rt_path_params": (RtPathParams, T.PATH_PARAMS), "rt_path_result": (RtPathResult, T.PATH_RESULT)}


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_symbol_is_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert "rt_radiance" in rt_api.ABI_SYMBOLS and hasattr(lib, "rt_radiance")
    assert re.search(r"int rt_radiance\(rt_ctx\* ctx, const rt_ray\* rays, size_t n, const rt_path_params\* params, rt_path_result\* out\);", code)
    assert re.search(r"It survives rt_prepare,[^.]*rt_radiance", _header(), re.S), "listed among the calls a running image survives"


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_mirrors(tmp_path, compiler, lang):
    """Compiled as C and as C++: the static asserts of rt_hip.h hold, and the sizes / offsets are the ctypes mirrors' and the dtypes'."""
    fields = [(s, f) for s, (mirror, _) in MIRRORS.items() for f, _ in mirror._fields_]
    args = ", ".join([f"sizeof({s})" for s in MIRRORS] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (len(MIRRORS) + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "pq_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    assert got[:2] == [32, 16]
    assert got == [C.sizeof(m) for m, _ in MIRRORS.values()] + [getattr(MIRRORS[s][0], f).offset for s, f in fields]
    assert got == [d.itemsize for _, d in MIRRORS.values()] + [MIRRORS[s][1].fields[f][1] for s, f in fields]
    assert [getattr(RtPathParams, f).offset for f in ("samples", "max_bounces", "seed", "first_sample", "flags", "_pad")] == [0, 4, 8, 12, 16, 20]
    assert [getattr(RtPathResult, f).offset for f in ("radiance", "segments")] == [0, 12]
    assert T.EXPECTED_SIZES["PATH_PARAMS"] == 32 and T.EXPECTED_SIZES["PATH_RESULT"] == 16
    # the header asserts them itself
    header = _header()
    assert "RT_STATIC_ASSERT(sizeof(rt_path_params) == 32" in header and "RT_STATIC_ASSERT(sizeof(rt_path_result) == 16" in header
    assert "offsetof(rt_path_params, first_sample) == 12" in header and "offsetof(rt_path_result, segments) == 12" in header


def test_header_constants_equal_the_python_ones_and_are_distinct_flags(rt_api):
    header = _header()
    value = lambda name: int(re.search(r"^#define %s (\d+)u" % name, header, re.M).group(1))
    assert value("RT_PATH_NO_SHADOWS") == rt_api.PATH_NO_SHADOWS == 32
    assert value("RT_PATH_CAMERA_DRAWS") == rt_api.PATH_CAMERA_DRAWS == 64
    assert value("RT_PATH_MAX_SAMPLES") == rt_api.PATH_MAX_SAMPLES == 4096
    assert value("RT_MAX_BOUNCES") == rt_api.MAX_BOUNCES == T.MAX_BOUNCES
    flags = [value(n) for n in ("RT_QUERY_COUNTERS", "RT_QUERY_COUNT_ALL", "RT_DIRECT_AMBIENT", "RT_DIRECT_NO_SHADOWS", "RT_DIRECT_NO_SHADOW_GRID",
                                "RT_PATH_NO_SHADOWS", "RT_PATH_CAMERA_DRAWS")]
    assert all(f and f & (f - 1) == 0 for f in flags) and len(set(flags)) == len(flags), "single, distinct bits"
    assert value("RT_QUERY_CHUNK") == rt_api.QUERY_CHUNK


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    rays, out = (RtRay * 1)(), (RtPathResult * 1)()
    pp = RtPathParams(samples=1, max_bounces=4)
    assert lib.rt_radiance(C.c_void_p(0), rays, C.c_size_t(1), C.byref(pp), out) == -1
    assert lib.rt_radiance(C.c_void_p(0), None, C.c_size_t(0), None, None) == -1
    assert not any(bytes(out))


def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.radiance
    good = np.zeros((4, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good.astype(np.float64))
    with pytest.raises(ValueError, match="shape"):
        call(nc, np.zeros((4, 7), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, np.zeros((8, 8), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, [[0.0] * 8])
    for bad in (0, -1, rt_api.PATH_MAX_SAMPLES + 1, 2.0, True, None, "x"):
        with pytest.raises(ValueError, match="samples"):
            call(nc, good, samples=bad)
    for bad in (-1, rt_api.MAX_BOUNCES + 1, 1.5, None):
        with pytest.raises(ValueError, match="max_bounces"):
            call(nc, good, max_bounces=bad)
    for bad in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="seed"):
            call(nc, good, seed=bad)
    for bad in (-1, 1 << 32, None):
        with pytest.raises(ValueError, match="first_sample"):
            call(nc, good, first_sample=bad)
    with pytest.raises(ValueError, match="first_sample"):
        call(nc, good, first_sample=(1 << 32) - 1, samples=2)
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, out=np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, out=np.zeros((4, 3), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, out=np.zeros((4, 4), np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, out=np.zeros((8, 4), np.float32)[::2])


def test_kind_mismatch_is_validated_in_python(rt_api):
    torch = pytest.importorskip("torch")
    nc = _no_context(rt_api)
    call = rt_api.Context.radiance
    with pytest.raises(TypeError, match="same kind"):
        call(nc, torch.zeros(4, 8), out=np.zeros((4, 4), np.float32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, np.zeros((4, 8), np.float32), out=torch.zeros(4, 4))


class _RecordingLib:
    """Stands in for librt_hip.so: records the parameters of every rt_radiance."""

    def __init__(self):
        self.calls = []

    def rt_radiance(self, h, rays, n, params, out):
        raw = (C.c_char * T.PATH_PARAMS.itemsize).from_address(params.value)
        self.calls.append((n.value, np.frombuffer(raw, dtype=T.PATH_PARAMS)[0].copy(), rays.value, out.value))
        return 0


def test_radiance_passes_its_parameters(rt_api):
    ctx = rt_api.Context.__new__(rt_api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    rays = np.zeros((6, 8), np.float32)
    got = ctx.radiance(rays)
    assert got.shape == (6, 4) and got.dtype == np.float32
    own = np.zeros((6, 4), np.float32)
    assert ctx.radiance(rays, samples=4096, max_bounces=255, seed=0xFFFFFFFF, first_sample=(1 << 32) - 4096, shadows=False, camera_draws=True, out=own,
                        counters=True) is own
    (n0, p0, _, _), (n1, p1, a_rays, a_out) = ctx.lib.calls
    assert n0 == n1 == 6
    assert (p0["samples"], p0["max_bounces"], p0["seed"], p0["first_sample"], p0["flags"]) == (1, 4, 0, 0, 0)
    assert (p1["samples"], p1["max_bounces"], p1["seed"], p1["first_sample"]) == (4096, 255, 0xFFFFFFFF, (1 << 32) - 4096)
    assert p1["flags"] == rt_api.PATH_NO_SHADOWS | rt_api.PATH_CAMERA_DRAWS | rt_api.QUERY_COUNTERS
    assert not p0["_pad"].any() and not p1["_pad"].any()
    assert (a_rays, a_out) == (rays.ctypes.data, own.ctypes.data)


def test_split_radiance(rt_api):
    rec = np.zeros(3, T.PATH_RESULT)
    rec["radiance"] = [[1, 2, 3], [0.5, 0.25, 0], [1, 0, 1]]
    rec["segments"] = [5, 0x80000001, 0]
    results = rec.view(np.float32).reshape(3, 4)
    radiance, segments = rt_api.split_radiance(results)
    assert segments.dtype == np.uint32
    np.testing.assert_array_equal(radiance, rec["radiance"])
    np.testing.assert_array_equal(segments, rec["segments"])


def test_split_radiance_on_torch(rt_api):
    torch = pytest.importorskip("torch")
    rec = np.zeros(3, T.PATH_RESULT)
    rec["radiance"] = [[1, 2, 3], [0.5, 0.25, 0], [1, 0, 1]]
    rec["segments"] = [5, 0x80000001, 0]
    tr, ts = rt_api.split_radiance(torch.from_numpy(rec.view(np.float32).reshape(3, 4).copy()))
    assert ts.dtype == torch.int64 and ts.tolist() == [5, 0x80000001, 0] and tr.tolist() == rec["radiance"].tolist()
