"""Geometry updates (rt_update_geometry) at the C-ABI and Python boundary, without a GPU: the symbol, the header's constants against
api.py's, the null-context error, and the argument checks api.Context.update_geometry makes before it calls the library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import types as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "rt_hip.h")).read()


def test_update_symbol_is_exported_and_listed(rt_api):
    assert "rt_update_geometry" in rt_api.ABI_SYMBOLS
    assert hasattr(rt_api.load(), "rt_update_geometry")
    assert re.search(r"int rt_update_geometry\(rt_ctx\* ctx,\s*const rt_vertex\* vertices, uint32_t n_vertices,.*?"
                     r"const rt_sphere\* spheres, uint32_t n_spheres,.*?uint32_t flags\);", _header(), re.S)


@pytest.mark.parametrize("name,attr", [("RT_UPDATE_REBUILD", "UPDATE_REBUILD"), ("RT_STAT_MEGAKERNEL_FALLBACK", "STAT_MEGAKERNEL_FALLBACK"),
                                       ("RT_STAT_SINGLE_PASS", "STAT_SINGLE_PASS"), ("RT_STAT_REFIT", "STAT_REFIT"),
                                       ("RT_STAT_REBUILT", "STAT_REBUILT")])
def test_header_constants_equal_the_python_ones(rt_api, name, attr):
    m = re.search(r"#define %s (\d+)u" % name, _header())
    assert m, name
    assert int(m.group(1)) == getattr(rt_api, attr)


def test_stat_flags_are_distinct_bits(rt_api):
    bits = [rt_api.STAT_MEGAKERNEL_FALLBACK, rt_api.STAT_SINGLE_PASS, rt_api.STAT_REFIT, rt_api.STAT_REBUILT]
    assert all(b & (b - 1) == 0 for b in bits) and len(set(bits)) == 4


def test_rt_stats_layout_is_unchanged(tmp_path):
    """rt_stats does not grow or reorder (callers built against the older header read the same offsets): the update reports
    through the existing flags field.  The header compiled as C against the numpy mirror of types.py."""
    src = ('#include <stdio.h>\n#include "rt_hip.h"\nint main(void){printf("%zu %zu %zu\\n", sizeof(rt_stats), offsetof(rt_stats, flags), '
           'offsetof(rt_stats, grid_build_ms));return 0;}\n')
    exe = str(tmp_path / "stats_layout")
    subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    size, flags, last = map(int, subprocess.check_output([exe]).split())
    assert (size, flags, last) == (144, 108, 136)
    assert (T.STATS.itemsize, T.STATS.fields["flags"][1], T.STATS.fields["grid_build_ms"][1]) == (size, flags, last)


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    v = np.zeros((3, 3), np.float32)
    assert lib.rt_update_geometry(C.c_void_p(0), C.c_void_p(v.ctypes.data), C.c_uint32(3), C.c_void_p(0), C.c_uint32(0), C.c_uint32(0)) == -1
    assert lib.rt_update_geometry(C.c_void_p(0), C.c_void_p(0), C.c_uint32(0), C.c_void_p(0), C.c_uint32(0), C.c_uint32(1)) == -1


class _RecordingLib:
    """Stands in for librt_hip.so: records whether rt_update_geometry was reached."""

    def __init__(self):
        self.calls = 0

    def rt_update_geometry(self, *args):
        self.calls += 1
        return 0

    def rt_get_stats(self, *args):
        return 0

    def rt_last_error(self, *args):
        return b""


def _ctx(api, n_vertices=4, n_spheres=2):
    """A Context that holds no rt_ctx, with the counts an upload would have recorded."""
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = _RecordingLib(), C.c_void_p(0)
    ctx._n_vertices, ctx._n_spheres = n_vertices, n_spheres
    return ctx


def test_update_arguments_are_validated_in_python(rt_api):
    ctx = _ctx(rt_api)
    good = np.zeros((4, 3), np.float32)
    with pytest.raises(TypeError, match="dtype"):
        ctx.update_geometry(good.astype(np.float64))
    with pytest.raises(ValueError, match="shape"):
        ctx.update_geometry(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        ctx.update_geometry(np.zeros(12, np.float32))
    with pytest.raises(ValueError, match="contiguous"):
        ctx.update_geometry(np.zeros((8, 3), np.float32)[::2])
    with pytest.raises(ValueError, match="count"):
        ctx.update_geometry(np.zeros((5, 3), np.float32))
    with pytest.raises(TypeError):
        ctx.update_geometry([[0.0, 0.0, 0.0]] * 4)
    with pytest.raises(TypeError, match="SPHERE"):
        ctx.update_geometry(spheres=np.zeros((2, 5), np.float32))
    with pytest.raises(ValueError, match="count"):
        ctx.update_geometry(spheres=np.zeros(3, T.SPHERE))
    with pytest.raises(ValueError, match="shape"):
        ctx.update_geometry(spheres=np.zeros((1, 2), T.SPHERE))
    assert ctx.lib.calls == 0
    fresh = rt_api.Context.__new__(rt_api.Context)
    fresh.lib, fresh._h = _RecordingLib(), C.c_void_p(0)
    with pytest.raises(rt_api.RtError, match="NOT_UPLOADED"):
        fresh.update_geometry(good)
    assert fresh.lib.calls == 0
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError, match="dtype"):
        ctx.update_geometry(torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="shape"):
        ctx.update_geometry(torch.zeros(4, 2))
    with pytest.raises(ValueError, match="count"):
        ctx.update_geometry(torch.zeros(3, 3))
    assert ctx.lib.calls == 0


def test_valid_arguments_reach_the_library(rt_api):
    ctx = _ctx(rt_api)
    ctx.update_geometry(np.zeros((4, 3), np.float32), spheres=np.zeros(2, T.SPHERE), rebuild=True)
    ctx.update_geometry(spheres=np.zeros(2, T.SPHERE))
    assert ctx.lib.calls == 2
