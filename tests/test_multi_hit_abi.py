"""Multi-hit ray queries (rt_intersect_all) at the C-ABI and Python boundary, without a GPU: the symbol, the header's constants
against api.py's, the argument check that needs no device, and the validation Context.intersect_all does before the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RtRay(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("tmin", C.c_float), ("direction", C.c_float * 3), ("tmax", C.c_float)]


class RtHit(C.Structure):
    _fields_ = [("t", C.c_float), ("u", C.c_float), ("v", C.c_float), ("prim_id", C.c_uint32)]


def test_symbol_is_exported_and_listed(rt_api):
    assert "rt_intersect_all" in rt_api.ABI_SYMBOLS
    assert hasattr(rt_api.load(), "rt_intersect_all")


def test_header_constants_equal_the_python_ones(rt_api):
    header = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    count_all = re.search(r"^#define RT_QUERY_COUNT_ALL (\d+)u", header, re.M)
    most = re.search(r"^#define RT_MULTI_HIT_MAX (\d+)u", header, re.M)
    assert count_all and int(count_all.group(1)) == rt_api.QUERY_COUNT_ALL == 2
    assert most and int(most.group(1)) == rt_api.MULTI_HIT_MAX == 16
    assert rt_api.QUERY_COUNT_ALL & rt_api.QUERY_COUNTERS == 0
    assert re.search(r"int rt_intersect_all\(rt_ctx\* ctx, const rt_ray\* rays, size_t n, uint32_t max_hits,\s*rt_hit\* hits,", header)


def test_null_context_returns_bad_arg(rt_api):
    lib = rt_api.load()
    rays, hits, counts = (RtRay * 1)(), (RtHit * 4)(), (C.c_uint32 * 1)()
    assert lib.rt_intersect_all(C.c_void_p(0), rays, C.c_size_t(1), C.c_uint32(4), hits, counts, C.c_uint32(0)) == -1
    assert lib.rt_intersect_all(C.c_void_p(0), rays, C.c_size_t(0), C.c_uint32(0), None, counts, C.c_uint32(2)) == -1


def _no_context(api):
    """A Context that holds no library and no rt_ctx: validation happens before the library is called."""
    ctx = api.Context.__new__(api.Context)
    ctx.lib, ctx._h = None, None
    return ctx


def test_batches_are_validated_in_python_numpy(rt_api):
    nc = _no_context(rt_api)
    call = rt_api.Context.intersect_all
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
    for bad in (17, -1, 2.0, None, True):
        with pytest.raises(ValueError, match="max_hits"):
            call(nc, good, bad)
    with pytest.raises(ValueError, match="max_hits"):
        call(nc, good, 0)
    with pytest.raises(ValueError, match="max_hits"):
        call(nc, good, 0, count_all=False, counts=np.zeros(4, np.uint32))
    # out: (N, max_hits, 4) float32, C-contiguous
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, out=np.zeros((3, 4, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 4, out=np.zeros((4, 3, 4), np.float32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 4, out=np.zeros((16, 4), np.float32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, out=np.zeros((4, 4, 4), np.float64))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, 4, out=np.zeros((8, 4, 4), np.float32)[::2])
    with pytest.raises(TypeError):
        call(nc, good, 4, out=[[0.0] * 4] * 16)
    # counts: (N,) uint32, C-contiguous
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, counts=np.zeros(3, np.uint32))
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 0, counts=np.zeros(5, np.uint32), count_all=True)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, counts=np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="shape"):
        call(nc, good, 4, counts=np.zeros((4, 1), np.uint32))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, 4, counts=np.zeros(8, np.uint32)[::2])


def test_batches_are_validated_in_python_torch(rt_api):
    torch = pytest.importorskip("torch")
    nc = _no_context(rt_api)
    call = rt_api.Context.intersect_all
    good = torch.zeros(4, 8)
    with pytest.raises(TypeError, match="dtype"):
        call(nc, torch.zeros(4, 8, dtype=torch.float64), 4)
    with pytest.raises(ValueError, match="shape"):
        call(nc, torch.zeros(4, 9), 4)
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, torch.zeros(8, 4).t(), 4)
    with pytest.raises(ValueError, match="max_hits"):
        call(nc, good, 17)
    with pytest.raises(TypeError, match="same kind"):
        call(nc, good, 4, out=np.zeros((4, 4, 4), np.float32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, good, 4, counts=np.zeros(4, np.uint32))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, np.zeros((4, 8), np.float32), 4, out=torch.zeros(4, 4, 4))
    with pytest.raises(TypeError, match="same kind"):
        call(nc, np.zeros((4, 8), np.float32), 4, counts=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, out=torch.zeros(5, 4, 4))
    with pytest.raises(ValueError, match="rows"):
        call(nc, good, 4, counts=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        call(nc, good, 4, counts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="contiguous"):
        call(nc, good, 4, out=torch.zeros(4, 4, 4).transpose(1, 2))
