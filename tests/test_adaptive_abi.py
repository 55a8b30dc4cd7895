"""Adaptive sampling (rt_render_adaptive, rt_read_adaptive) at the C-ABI and Python boundary, without a GPU: the symbols, the record
layouts against the header's static asserts and the numpy dtypes, the null-context errors, and the parameters api.Context.render_adaptive
passes to the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rt_render_adaptive", "rt_read_adaptive")


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_symbols_are_exported_declared_and_listed(rt_api):
    lib = rt_api.load()
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert name in rt_api.ABI_SYMBOLS
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert hasattr(lib, name), name
    assert re.search(r"int rt_render_adaptive\(rt_ctx\* ctx, const rt_render_params\* p, const rt_adaptive_params\* ap\);", code)
    assert re.search(r"int rt_read_adaptive\(rt_ctx\* ctx, rt_adaptive_pixel\* out, size_t n_pixels\);", code)


@pytest.mark.parametrize("compiler,lang", [("gcc", "c"), ("g++", "c++")])
def test_record_layouts_match_the_numpy_dtypes(tmp_path, compiler, lang):
    fields = [("rt_adaptive_params", "threshold"), ("rt_adaptive_params", "min_samples"), ("rt_adaptive_params", "flags"),
              ("rt_adaptive_params", "_pad"), ("rt_adaptive_pixel", "sum"), ("rt_adaptive_pixel", "samples"), ("rt_adaptive_pixel", "odd"),
              ("rt_adaptive_pixel", "error")]
    args = ", ".join(["sizeof(rt_adaptive_params)", "sizeof(rt_adaptive_pixel)"] + [f"offsetof({s}, {f})" for s, f in fields])
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%s\\n", ' % " ".join(["%zu"] * (2 + len(fields))) + args +
           ');return 0;}\n')
    exe = str(tmp_path / "ad_layout")
    subprocess.run([compiler, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = list(map(int, subprocess.check_output([exe]).split()))
    dtypes = {"rt_adaptive_params": T.ADAPTIVE_PARAMS, "rt_adaptive_pixel": T.ADAPTIVE_PIXEL}
    assert got == [T.ADAPTIVE_PARAMS.itemsize, T.ADAPTIVE_PIXEL.itemsize] + [dtypes[s].fields[f][1] for s, f in fields]
    assert got[:2] == [16, 32]


def test_no_new_flag_bits(rt_api):
    """Adaptive sampling is its own entry point: rt_render's flag set is unchanged."""
    flags = {m.group(1) for m in re.finditer(r"#define (RT_FLAG_\w+) (\d+)u", _header())}
    assert len(flags) == 10, sorted(flags)


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    p = np.zeros((), T.RENDER_PARAMS)
    p["mode"], p["spp"], p["width"], p["height"], p["flags"] = 2, 2, 8, 8, rt_api.FLAG_ACCUMULATE
    ap = np.zeros((), T.ADAPTIVE_PARAMS)
    ap["threshold"], ap["min_samples"] = 0.01, 4
    assert lib.rt_render_adaptive(C.c_void_p(0), C.c_void_p(p.ctypes.data), C.c_void_p(ap.ctypes.data)) == -1
    assert lib.rt_render_adaptive(C.c_void_p(0), C.c_void_p(0), C.c_void_p(0)) == -1
    out = np.zeros((8, 8, 8), np.float32)
    assert lib.rt_read_adaptive(C.c_void_p(0), C.c_void_p(out.ctypes.data), C.c_size_t(64)) == -1
    assert lib.rt_read_adaptive(C.c_void_p(0), C.c_void_p(0), C.c_size_t(0)) == -1
    assert not out.any()


class _RecordingLib:
    """Stands in for librt_hip.so: records the parameters of every rt_render_adaptive, answers rt_read_adaptive with a ramp."""

    def __init__(self):
        self.calls = []

    def rt_render_adaptive(self, h, params, aparams):
        raw = (C.c_char * T.RENDER_PARAMS.itemsize).from_address(params.value)
        araw = (C.c_char * T.ADAPTIVE_PARAMS.itemsize).from_address(aparams.value)
        self.calls.append((np.frombuffer(raw, dtype=T.RENDER_PARAMS)[0].copy(), np.frombuffer(araw, dtype=T.ADAPTIVE_PARAMS)[0].copy()))
        return 0

    def rt_read_adaptive(self, h, out, n):
        a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(n.value * 8,))
        a[:] = np.arange(n.value * 8, dtype=np.float32)
        return 0

    def rt_get_stats(self, *args):
        return 0

    def rt_last_error(self, *args):
        return b""


def _ctx(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    ctx.width = ctx.height = 0
    return ctx


def test_render_adaptive_passes_its_parameters(rt_api):
    ctx = _ctx(rt_api)
    cam = scenes.default_scene().camera
    acc, restart = rt_api.FLAG_ACCUMULATE, rt_api.FLAG_ACCUMULATE_RESTART
    ctx.render_adaptive(16, 8, cam, 2, 0.05)
    ctx.render_adaptive(16, 8, cam, 3, 0.0, min_samples=6, restart=True, kernel_sm=True, max_bounces=2, frame_seed=9)
    (p0, a0), (p1, a1) = ctx.lib.calls
    assert (p0["mode"], p0["spp"], p0["width"], p0["height"], p0["flags"]) == (2, 2, 16, 8, acc)
    assert (p1["mode"], p1["spp"], p1["max_bounces"], p1["frame_seed"], p1["flags"]) == (2, 3, 2, 9, acc | restart | rt_api.FLAG_KERNEL_SM)
    assert (np.float32(a0["threshold"]), a0["min_samples"], a0["flags"], a0["_pad"]) == (np.float32(0.05), 4, 0, 0)
    assert (a1["threshold"], a1["min_samples"], a1["flags"]) == (0.0, 6, 0)
    assert (ctx.width, ctx.height) == (16, 8)


def test_read_adaptive_shape_and_split(rt_api):
    ctx = _ctx(rt_api)
    ctx.width, ctx.height = 5, 3
    rec = ctx.read_adaptive()
    assert rec.shape == (3, 5, 8) and rec.dtype == np.float32
    assert rec[2, 4, 7] == 3 * 5 * 8 - 1
    parts = rt_api.split_adaptive(rec)
    assert parts["sum"].shape == (3, 5, 3) and parts["odd"].shape == (3, 5, 3)
    assert parts["samples"][0, 1] == 11 and parts["error"][0, 1] == 15
    assert np.array_equal(rec.view(T.ADAPTIVE_PIXEL)[..., 0]["odd"], parts["odd"])
