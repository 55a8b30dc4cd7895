"""The edge-avoiding a-trous denoiser (rt_denoise) on the MI355X: against a float64 numpy statement of the filter,
its NaN / constant-image / in-place / buffer-kind properties, its argument checks, and its quality with the committed defaults."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_raytracer_amd import api, scenes
from gpu_raytracer_amd import types as T

try:
    import torch  # imported before any context exists, so that api.Context brings torch's device runtime up first
except ImportError:
    torch = None

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
KERNEL = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def reference_denoise(rgb, aov, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, demodulate=True, dtype=np.float64):
    """The statement of rt_denoise in numpy (float64 by default): taps in the kernel's order, dy outer, dx inner."""
    rgb, aov = rgb.astype(dtype), aov.astype(dtype)
    A, Z, N = aov[..., 0:3], aov[..., 3], aov[..., 4:7]
    D = np.maximum(A, dtype(1e-3)) if demodulate else np.ones_like(A)
    with np.errstate(all="ignore"):
        c = rgb / D
        h, w = Z.shape
        ys, xs = np.arange(h), np.arange(w)
        for i in range(iterations):
            step = 1 << i
            finite = np.isfinite(c).all(-1)
            inv_sc2 = dtype(1) / (dtype(sigma_color) * dtype(2.0 ** -i)) ** 2
            sw = np.zeros((h, w), dtype)
            sc = np.zeros((h, w, 3), dtype)
            for dy in range(-2, 3):
                qy = ys + step * dy
                for dx in range(-2, 3):
                    qx = xs + step * dx
                    inside = ((qy >= 0) & (qy < h))[:, None] & ((qx >= 0) & (qx < w))[None, :]
                    yy, xx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                    cq, Aq, Zq, Nq = c[yy][:, xx], A[yy][:, xx], Z[yy][:, xx], N[yy][:, xx]
                    ok = inside & np.isfinite(cq).all(-1)
                    ez = np.where((Z == 0) & (Zq == 0), dtype(0), ((Z - Zq) / (dtype(sigma_depth) * np.maximum(Z, Zq))) ** 2)
                    e = (((c - cq) ** 2).sum(-1) * inv_sc2 + ((N - Nq) ** 2).sum(-1) / dtype(sigma_normal) ** 2 + ez +
                         ((A - Aq) ** 2).sum(-1) / dtype(sigma_albedo) ** 2)
                    wq = np.where(ok, dtype(KERNEL[dx + 2]) * dtype(KERNEL[dy + 2]) * np.exp(-e), dtype(0))
                    sw = sw + wq
                    sc = sc + wq[..., None] * np.where(ok[..., None], cq, dtype(0))
            c = np.where(finite[..., None], sc / sw[..., None], c)
        return c * D


def random_case(h, w, seed):
    """A random image and AOVs with zeros, misses (no hit: depth 0, normal 0, sky albedo) and one NaN pixel."""
    rng = np.random.default_rng(seed)
    rgb = rng.uniform(0, 2, (h, w, 3)).astype(F32)
    rgb[rng.random((h, w)) < 0.1] = 0
    aov = np.zeros((h, w, 8), F32)
    aov[..., 0:3] = rng.uniform(0, 1, (h, w, 3))
    aov[..., 0:3][rng.random((h, w)) < 0.05] = 0  # albedo below the demodulation floor
    aov[..., 3] = rng.uniform(1, 5, (h, w))
    n = rng.standard_normal((h, w, 3))
    aov[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True) * rng.uniform(0.5, 1, (h, w, 1))
    aov[..., 7] = rng.uniform(0.25, 1, (h, w))
    miss = rng.random((h, w)) < 0.15
    aov[miss] = [0.1, 0.2, 0.3, 0, 0, 0, 0, 0]
    rgb[h // 2, w // 3] = np.nan
    return rgb, aov


PARAMS = dict(sigma_color=0.8, sigma_normal=0.5, sigma_depth=0.3, sigma_albedo=0.4)


@pytest.fixture(scope="module")
def ctx(rt_api):
    with rt_api.Context() as c:  # no scene: rt_denoise needs none
        yield c


def _rel_err(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    return float(np.max(np.abs(got[fin].astype(np.float64) - want[fin]) / np.maximum(np.abs(want[fin]), 1e-6)))


@pytest.mark.parametrize("demodulate", [True, False])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_against_the_float64_statement(ctx, iterations, demodulate):
    rgb, aov = random_case(23, 37, seed=iterations)
    got = ctx.denoise(rgb, aov, iterations=iterations, demodulate=demodulate, **PARAMS)
    assert got.shape == (23, 37, 3) and got.dtype == F32
    want = reference_denoise(rgb, aov, iterations, demodulate=demodulate, **PARAMS)
    assert _rel_err(got, want) <= 1e-4
    st = ctx.stats()
    assert st["pixels"] == 23 * 37 and st["kernel_ms"] > 0 and st["rays"] == 0


def test_nan_stays_and_does_not_spread(ctx):
    rgb, aov = random_case(23, 37, seed=1)
    got = ctx.denoise(rgb, aov, iterations=5, **PARAMS)
    nan = np.isnan(rgb).any(-1)
    assert nan.sum() == 1
    assert np.all(np.isnan(got[nan])) and np.all(np.isfinite(got[~nan]))


@pytest.mark.parametrize("demodulate", [True, False])
def test_constant_image_within_2_ulp(ctx, demodulate):
    h, w = 40, 56
    rgb = np.full((h, w, 3), [0.3, 0.7, 1.9], F32)
    aov = np.zeros((h, w, 8), F32)
    aov[...] = [0.5, 0.25, 0.8, 2.0, 0, 1, 0, 1]
    got = ctx.denoise(rgb, aov, iterations=5, demodulate=demodulate)
    ulp = np.spacing(rgb)
    assert np.max(np.abs(got - rgb) / ulp) <= 2


def test_host_device_and_in_place_give_identical_bits(ctx):
    rgb, aov = random_case(31, 45, seed=7)
    ref = ctx.denoise(rgb, aov, iterations=4, **PARAMS)
    inplace = rgb.copy()
    assert ctx.denoise(inplace, aov, out=inplace, iterations=4, **PARAMS) is inplace
    np.testing.assert_array_equal(inplace.view(np.uint32), ref.view(np.uint32))
    if torch is None:
        return
    for dev in ("cpu", "cuda:0"):
        trgb, taov = torch.from_numpy(rgb.copy()).to(dev), torch.from_numpy(aov.copy()).to(dev)  # copies: .to("cpu") would share rgb
        out = ctx.denoise(trgb, taov, iterations=4, **PARAMS)
        assert out.device == trgb.device
        np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32), err_msg=dev)
        ctx.denoise(trgb, taov, out=trgb, iterations=4, **PARAMS)
        np.testing.assert_array_equal(trgb.cpu().numpy().view(np.uint32), ref.view(np.uint32), err_msg=dev + " in place")


def _raw_denoise(ctx, dp, rgb, aov, out):
    ptr = lambda a: C.c_void_p(0) if a is None else C.c_void_p(a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)  # noqa: E731
    return ctx.lib.rt_denoise(ctx._h, C.c_void_p(0) if dp is None else C.c_void_p(dp.ctypes.data), ptr(rgb), ptr(aov), ptr(out))


def test_bad_arguments(ctx):
    h, w = 6, 10
    rgb, aov = random_case(h, w, seed=3)
    out = np.full((h, w, 3), 9.0, F32)

    def params(**kw):
        dp = np.zeros((), T.DENOISE_PARAMS)
        dp["width"], dp["height"], dp["iterations"], dp["flags"] = w, h, 2, api.DENOISE_DEMODULATE
        dp["sigma_color"] = dp["sigma_normal"] = dp["sigma_depth"] = dp["sigma_albedo"] = 1.0
        for k, v in kw.items():
            dp[k] = v
        return dp

    assert _raw_denoise(ctx, params(), rgb, aov, out) == 0
    out[...] = 9.0
    bad = [dict(width=0), dict(height=0), dict(width=65535 * 8 + 1), dict(iterations=0), dict(iterations=api.DENOISE_MAX_ITERATIONS + 1),
           dict(flags=2)]
    for s in ("sigma_color", "sigma_normal", "sigma_depth", "sigma_albedo"):
        bad += [{s: 0.0}, {s: -1.0}, {s: np.inf}, {s: np.nan}]
    for b in bad:
        assert _raw_denoise(ctx, params(**b), rgb, aov, out) == -1, b
    assert _raw_denoise(ctx, None, rgb, aov, out) == -1
    assert _raw_denoise(ctx, params(), None, aov, out) == -1
    assert _raw_denoise(ctx, params(), rgb, None, out) == -1
    assert _raw_denoise(ctx, params(), rgb, aov, None) == -1
    assert np.all(out == 9.0), "a rejected call changes nothing"
    if torch is None:
        return
    drgb, daov = torch.from_numpy(rgb).cuda(), torch.from_numpy(aov).cuda()
    dout = torch.full((h, w, 3), 9.0, device="cuda:0")
    assert _raw_denoise(ctx, params(), drgb, aov, out) == -1, "device rgb with host aov"
    assert _raw_denoise(ctx, params(), rgb, aov, dout) == -1, "host in, device out"
    big = torch.zeros(h * w * 8 + 4, device="cuda:0")
    big[1:1 + h * w * 8] = daov.reshape(-1)
    misaligned = big[1:1 + h * w * 8]  # 4 bytes past a 16-byte boundary
    assert misaligned.data_ptr() % 16 == 4
    assert _raw_denoise(ctx, params(), drgb, misaligned, dout) == -1, "aov not 16-byte aligned"
    assert bool((dout == 9.0).all())
    assert _raw_denoise(ctx, params(), drgb, daov, dout) == 0


# quality with the committed defaults -----------------------------------------------------------------------------------------
def _mse(a, b):
    return float(np.mean((a.astype(np.float64) - b) ** 2))


def _quality(rt_api, scene, spp, bounces):
    w = h = 256
    with rt_api.Context() as c:
        c.upload_scene(scene)
        kw = dict(mode=2, max_bounces=bounces, frame_seed=1)
        c.render(w, h, scene.camera, spp=1024, **dict(kw, frame_seed=99))
        ref = c.read_rgb32f()
        c.render(w, h, scene.camera, spp=spp, **kw)
        raw = c.read_rgb32f()
        den = c.denoise(raw, c.aovs(w, h, scene.camera, spp=spp, **kw))
    return _mse(raw, ref), _mse(den, ref)


def test_quality_cornell12(rt_api):
    raw, den = _quality(rt_api, scenes.cornell12(), 4, 4)
    assert den <= 0.5 * raw, (raw, den)


def test_quality_sponza_like(rt_api):
    raw, den = _quality(rt_api, scenes.sponza_like(), 4, 4)
    assert den < raw, (raw, den)


def test_cli_denoise_changes_the_image(tmp_path):
    exe = os.path.join(ROOT, "build", "rt_render")
    plain, den = str(tmp_path / "plain.ppm"), str(tmp_path / "den.ppm")
    subprocess.run([exe, "--size", "96x64", "--spp", "4", "--out", plain], check=True, timeout=120, capture_output=True)
    r = subprocess.run([exe, "--size", "96x64", "--spp", "4", "--denoise", "--out", den], check=True, timeout=120, capture_output=True, text=True)
    assert "denoise:" in r.stdout and "aovs:" in r.stdout
    a, b = open(plain, "rb").read(), open(den, "rb").read()
    assert len(a) == len(b) and a != b
