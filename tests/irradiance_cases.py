"""rt_irradiance's statement (include/rt_hip.h, "Irradiance queries") in numpy float32: the directions a surface point draws from the
frames' generator through their cosine lobe, the origins its paths start from, and the reduction in sample order.  The tests hold the
device to these bits (test_gpu_irradiance.py) and these functions to what they stand for (test_irradiance_cases.py).

The radiance of a sample comes from outside: from Context.radiance along the drawn direction on the device, or a constant field here."""
import numpy as np

from radiance_sh_cases import F32, F32_MAX, MIN_T, U32, next_f32, rng_for  # noqa: F401  (the frames' generator, shared)

PI = F32(3.1415927)  # the f32 the statement names
EXT_EPS = F32(0.001)  # the continuation's origin offset


def _dot(a, b):
    """(a.x*b.x + a.y*b.y) + a.z*b.z, every operation one f32 rounding."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def directions(oracle_mod, points, index, samples, seed, first_sample):
    """d_k of the (n, 8) float32 surface points whose indices in the caller's array are `index` -> (n, samples, 3) float32: the
    generator's first two draws of rng_for(seed + i (mod 2^32), first_sample + k) through the cosine lobe of the frames' diffuse
    continuation, w = N + unit_vector(u1, u2), N where |w|^2 < 1e-12, times 1 / sqrt(|w|^2).  Rows of no-points hold what the
    arithmetic gives; nothing is traced for them."""
    points = np.asarray(points)
    assert points.dtype == F32 and points.ndim == 2 and points.shape[1] == 8
    index = np.asarray(index, np.uint64)
    assert len(index) == len(points)
    pixel_seed = ((np.uint64(seed) + index) & np.uint64(0xFFFFFFFF)).astype(U32)
    sample = ((np.uint64(first_sample) + np.arange(samples, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(U32)
    state = rng_for(pixel_seed[:, None], sample[None, :])
    state, u1 = next_f32(state)
    state, u2 = next_f32(state)
    unit = oracle_mod.unit_vectors(u1, u2)[0].reshape(len(index), samples, 3)
    normal = np.broadcast_to(points[:, None, 4:7], unit.shape)
    with np.errstate(all="ignore"):  # no-points may hold anything
        w = normal + unit
        w = np.where((_dot(w, w) < F32(1e-12))[..., None], normal, w)
        d = w * (F32(1.0) / np.sqrt(_dot(w, w)))[..., None]
    assert d.dtype == F32
    return d


def origins(points):
    """o = P + N * 0.001f per component -> (n, 3) float32."""
    points = np.asarray(points)
    assert points.dtype == F32
    with np.errstate(all="ignore"):
        o = points[:, 0:3] + points[:, 4:7] * EXT_EPS
    assert o.dtype == F32
    return o


def reduce(x):
    """x (n, S, 3) float32 sample radiances -> E (n, 3) float32: from zero, in sample order, then one division and one multiply."""
    n, samples = x.shape[:2]
    assert x.dtype == F32
    total = np.zeros((n, 3), F32)
    for k in range(samples):
        total = total + x[:, k, :]
    return total * (PI / F32(samples))


def is_point(points):
    """Rule 5: every component of P and N finite, and N not (0, 0, 0)."""
    points = np.asarray(points)
    return np.isfinite(points[:, 0:3]).all(1) & np.isfinite(points[:, 4:7]).all(1) & (points[:, 4:7] != 0).any(1)


def blocked_cap_sigma(samples, radius=0.6, height=1.0):
    """The fraction of a cosine-distributed hemisphere that a sphere of `radius` centred at `height` on the normal covers is
    radius^2 / height^2 (the projected solid angle of a cap of half-angle a is pi sin^2 a, and sin a = radius / height) -> (that
    fraction, the standard deviation of its estimate from `samples` independent directions)."""
    f = radius * radius / (height * height)
    return f, np.sqrt(f * (1.0 - f) / samples)
