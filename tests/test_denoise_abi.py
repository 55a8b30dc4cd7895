"""Feature buffers and the denoiser (rt_aovs / rt_sample_rays / rt_denoise) at the C-ABI and Python boundary, without a GPU: the
symbols, the record layouts against the header's static asserts, the header constants against the Python ones, and the null-context
and Python-side argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_aovs", "rt_sample_rays", "rt_denoise")


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert name in rt_api.ABI_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_numpy_dtypes(tmp_path, compiler, lang):
    fields = [("rt_aov", "albedo"), ("rt_aov", "depth"), ("rt_aov", "normal"), ("rt_aov", "coverage"),
              ("rt_denoise_params", "width"), ("rt_denoise_params", "height"), ("rt_denoise_params", "iterations"),
              ("rt_denoise_params", "flags"), ("rt_denoise_params", "sigma_color"), ("rt_denoise_params", "sigma_normal"),
              ("rt_denoise_params", "sigma_depth"), ("rt_denoise_params", "sigma_albedo")]
    args = ", ".join(["sizeof(rt_aov)", "sizeof(rt_denoise_params)"] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (2 + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "dn_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    dtypes = {"rt_aov": T.AOV, "rt_denoise_params": T.DENOISE_PARAMS}
    assert got == [T.AOV.itemsize, T.DENOISE_PARAMS.itemsize] + [dtypes[s].fields[f][1] for s, f in fields]
    assert got[:2] == [32, 32]


def _define(name):
    m = re.search(r"#define\s+%s\s+([0-9.]+)[uf]?\b" % name, _header())
    assert m, name
    return float(m.group(1))


def test_header_constants_equal_the_python_constants(rt_api):
    assert _define("RT_AOV_SAMPLES_PER_LAUNCH") == T.AOV_SAMPLES_PER_LAUNCH == rt_api.AOV_SAMPLES_PER_LAUNCH
    assert _define("RT_DENOISE_DEMODULATE") == T.DENOISE_DEMODULATE == rt_api.DENOISE_DEMODULATE
    assert _define("RT_DENOISE_MAX_ITERATIONS") == T.DENOISE_MAX_ITERATIONS == rt_api.DENOISE_MAX_ITERATIONS
    for key in ("iterations", "sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
        v = _define("RT_DENOISE_DEFAULT_" + key.upper())
        assert np.float32(v) == np.float32(getattr(T, "DENOISE_DEFAULT_" + key.upper())) == np.float32(rt_api.DENOISE_DEFAULTS[key]), key
    assert 1 <= rt_api.DENOISE_DEFAULTS["iterations"] <= rt_api.DENOISE_MAX_ITERATIONS


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    null = C.c_void_p(0)
    p = np.zeros((), T.RENDER_PARAMS)
    p["width"], p["height"], p["mode"], p["spp"] = 4, 4, 2, 1
    aov = np.zeros((4, 4, 8), np.float32)
    rays = np.zeros((16, 8), np.float32)
    dp = np.zeros((), T.DENOISE_PARAMS)
    dp["width"], dp["height"], dp["iterations"] = 4, 4, 1
    dp["sigma_color"] = dp["sigma_normal"] = dp["sigma_depth"] = dp["sigma_albedo"] = 1.0
    rgb = np.zeros((4, 4, 3), np.float32)
    addr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    assert lib.rt_aovs(null, addr(p), addr(aov)) == -1
    assert lib.rt_sample_rays(null, addr(p), C.c_uint32(0), addr(rays)) == -1
    assert lib.rt_denoise(null, addr(dp), addr(rgb), addr(aov), addr(rgb)) == -1


def _no_context(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_denoise_arrays_are_validated_in_python(rt_api):
    nc = _no_context(rt_api)
    rgb, aov = np.zeros((5, 7, 3), np.float32), np.zeros((5, 7, 8), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        nc.denoise(rgb.astype(np.float64), aov)
    with pytest.raises(ValueError, match="shape"):
        nc.denoise(rgb, np.zeros((5, 6, 8), np.float32))
    with pytest.raises(ValueError, match="shape"):
        nc.denoise(rgb, aov, out=np.zeros((5, 7, 4), np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        nc.denoise(np.zeros((5, 14, 3), np.float32)[:, ::2], aov)
    with pytest.raises(TypeError):
        nc.denoise(rgb.tolist(), aov)
    with pytest.raises(ValueError, match="shape"):
        nc.aovs(7, 5, np.zeros((), T.CAMERA), out=np.zeros((7, 5, 8), np.float32))
    with pytest.raises(ValueError, match="rows"):
        nc.sample_rays(7, 5, np.zeros((), T.CAMERA), 0, out=np.zeros((34, 8), np.float32))
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="same kind"):
        nc.denoise(torch.zeros(5, 7, 3), aov)


def test_split_aovs_views():
    from gpu_raytracer_amd import api
    a = np.arange(2 * 3 * 8, dtype=np.float32).reshape(2, 3, 8)
    s = api.split_aovs(a)
    assert np.array_equal(s["albedo"], a[..., 0:3]) and np.array_equal(s["depth"], a[..., 3])
    assert np.array_equal(s["normal"], a[..., 4:7]) and np.array_equal(s["coverage"], a[..., 7])
    rec = a.view(T.AOV)[..., 0]
    assert np.array_equal(rec["depth"], s["depth"]) and np.array_equal(rec["normal"], s["normal"])
