"""Progressive accumulation (RT_FLAG_ACCUMULATE, rt_accumulated_samples) at the C-ABI and Python boundary, without a GPU: the symbol,
the header's constants against api.py's, the null-context errors, and the flag bits api.Context.render passes to the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpu_raytracer_amd import scenes
from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def _define(name):
    m = re.search(r"#define %s (\d+)u" % name, _header())
    assert m, name
    return int(m.group(1))


def test_accumulated_samples_symbol_is_exported_and_listed(rt_api):
    assert "rt_accumulated_samples" in rt_api.ABI_SYMBOLS
    assert hasattr(rt_api.load(), "rt_accumulated_samples")
    assert re.search(r"int rt_accumulated_samples\(rt_ctx\* ctx, uint32_t\* samples\);", _header())


@pytest.mark.parametrize("name,attr", [("RT_FLAG_ACCUMULATE", "FLAG_ACCUMULATE"), ("RT_FLAG_ACCUMULATE_RESTART", "FLAG_ACCUMULATE_RESTART"),
                                       ("RT_ACCUMULATE_MAX_SAMPLES", "ACCUMULATE_MAX_SAMPLES")])
def test_header_constants_equal_the_python_ones(rt_api, name, attr):
    assert _define(name) == getattr(rt_api, attr)


def test_accumulation_flags_are_new_distinct_bits(rt_api):
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (RT_FLAG_\w+) (\d+)u", _header())}
    acc, restart = flags.pop("RT_FLAG_ACCUMULATE"), flags.pop("RT_FLAG_ACCUMULATE_RESTART")
    assert len(flags) == 8, sorted(flags)  # COUNTERS ... STAGE_TIMES
    others = 0
    for v in flags.values():
        assert v & (v - 1) == 0 and not (others & v)
        others |= v
    for v in (acc, restart):
        assert v & (v - 1) == 0 and not (others & v)
    assert acc != restart
    assert rt_api.ACCUMULATE_MAX_SAMPLES == 1 << 24


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    n = C.c_uint32(7)
    assert lib.rt_accumulated_samples(C.c_void_p(0), C.byref(n)) == -1
    assert lib.rt_accumulated_samples(C.c_void_p(0), C.c_void_p(0)) == -1
    assert n.value == 7
    p = np.zeros((), T.RENDER_PARAMS)
    p["mode"], p["spp"], p["width"], p["height"], p["flags"] = 2, 1, 8, 8, rt_api.FLAG_ACCUMULATE
    assert lib.rt_render(C.c_void_p(0), C.c_void_p(p.ctypes.data)) == -1


class _RecordingLib:
    """Stands in for librt_hip.so: records the flags of every rt_render and answers rt_accumulated_samples."""

    def __init__(self):
        self.flags = []
        self.samples = 0

    def rt_render(self, h, params):
        raw = (C.c_char * T.RENDER_PARAMS.itemsize).from_address(params.value)
        self.flags.append(int(np.frombuffer(raw, dtype=T.RENDER_PARAMS)[0]["flags"]))
        return 0

    def rt_accumulated_samples(self, h, out):
        C.cast(out, C.POINTER(C.c_uint32))[0] = self.samples
        return 0

    def rt_get_stats(self, *args):
        return 0

    def rt_last_error(self, *args):
        return b""


def _ctx(api):
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    return ctx


def test_render_passes_the_accumulation_bits(rt_api):
    ctx = _ctx(rt_api)
    cam = scenes.default_scene().camera
    acc, restart = rt_api.FLAG_ACCUMULATE, rt_api.FLAG_ACCUMULATE_RESTART
    ctx.render(8, 8, cam, mode=2, spp=2)
    ctx.render(8, 8, cam, mode=2, spp=2, accumulate=True)
    ctx.render(8, 8, cam, mode=2, spp=2, accumulate=True, restart=True)
    ctx.render(8, 8, cam, mode=2, spp=2, accumulate=True, kernel_sm=True, no_shadows=True)
    assert ctx.lib.flags == [0, acc, acc | restart, acc | rt_api.FLAG_KERNEL_SM | rt_api.FLAG_NO_SHADOWS]
    with pytest.raises(ValueError, match="accumulate"):
        ctx.render(8, 8, cam, mode=2, spp=2, restart=True)
    assert len(ctx.lib.flags) == 4


def test_accumulated_samples_reads_the_library(rt_api):
    ctx = _ctx(rt_api)
    assert ctx.accumulated_samples() == 0
    ctx.lib.samples = 1 << 24
    assert ctx.accumulated_samples() == 1 << 24
