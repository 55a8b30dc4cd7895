"""rt_radiance_sh's statement (include/rt_hip.h, "Probe queries") in numpy float32: the directions a probe draws from the frames'
generator, the nine basis functions with every operation one f32 rounding, and the projection in sample order.  The tests hold the
device to these bits (test_gpu_radiance_sh.py) and these functions to what they stand for (test_radiance_sh_cases.py).

The radiance of a sample comes from outside: from Context.radiance along the drawn direction on the device, or a constant field here."""
import numpy as np

F32 = np.float32
U32 = np.uint32
F32_MAX = np.finfo(np.float32).max
MIN_T = F32(1e-5)  # RT_MIN_RAY_DISTANCE
SOLID_ANGLE = F32(12.566371)  # 4 pi, the f32 the statement names
Y0_EXACT = 0.28209479  # 1 / (2 sqrt(pi)), the bound's own constant


def rng_for(pixel_seed, sample):
    """The frames' per-sample generator state for uint32 arrays (device_common.h, rng_for)."""
    h = pixel_seed + sample * U32(0x9E3779B9)
    h = h ^ (h >> U32(16))
    h = h * U32(0x7FEB352D)
    h = h ^ (h >> U32(15))
    h = h * U32(0x846CA68B)
    return h ^ (h >> U32(16))


def next_f32(state):
    """One LCG step -> (state, the draw in [0, 1) as float32)."""
    state = state * U32(1664525) + U32(1013904223)
    return state, (state >> U32(8)).astype(F32) / F32(16777216.0)


def directions(oracle_mod, index, samples, seed, first_sample):
    """d_k of the probes whose indices in the caller's array are `index` -> (len(index), samples, 3) float32: the generator's first two
    draws of rng_for(seed + i (mod 2^32), first_sample + k) through unit_vector."""
    index = np.asarray(index, np.uint64)
    pixel_seed = ((np.uint64(seed) + index) & np.uint64(0xFFFFFFFF)).astype(U32)
    sample = ((np.uint64(first_sample) + np.arange(samples, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)).astype(U32)
    state = rng_for(pixel_seed[:, None], sample[None, :])
    state, u1 = next_f32(state)
    state, u2 = next_f32(state)
    return oracle_mod.unit_vectors(u1, u2)[0].reshape(len(index), samples, 3)


def basis(d):
    """Y_0 .. Y_8 at directions d (..., 3) -> (..., 9), in d's dtype (float32: the statement's roundings; float64: the same constants)."""
    t = d.dtype.type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c1, c2, c6, c8 = t(F32(0.4886025)), t(F32(1.0925484)), t(F32(0.31539157)), t(F32(0.5462742))
    return np.stack([np.full(x.shape, t(F32(0.2820948))), c1 * y, c1 * z, c1 * x, c2 * (x * y), c2 * (y * z), c6 * (t(3.0) * (z * z) - t(1.0)),
                     c2 * (x * z), c8 * (x * x - y * y)], axis=-1)


def project(x, d):
    """x (n, S, 3) float32 sample radiances and d (n, S, 3) float32 directions -> sh (n, 9, 3) float32: from zero, in sample order, each
    term one product, then one division and one multiply."""
    n, samples = x.shape[:2]
    y = basis(d)
    assert x.dtype == F32 and y.dtype == F32
    total = np.zeros((n, 9, 3), F32)
    for k in range(samples):
        total = total + x[:, k, None, :] * y[:, k, :, None]
    return total * (SOLID_ANGLE / F32(samples))


def is_probe(probes):
    return np.isfinite(probes[:, 0:3]).all(1)


def constant_field(oracle_mod, n, samples, seed, level, first_sample=0):
    """The statement for n probes in a field of constant radiance `level` (3,) -> sh (n, 9, 3)."""
    d = directions(oracle_mod, np.arange(n), samples, seed, first_sample)
    return project(np.broadcast_to(np.asarray(level, F32), (n, samples, 3)), d)


def check_constant_field(sh, samples, level, label=""):
    """The two bounds of a constant field: the band the sequential f32 sum leaves around sh[0], and six standard deviations of the
    Monte-Carlo noise of the others (4 pi L Y_j has variance 4 pi L^2 under uniform directions).  Prints the figures first."""
    level = np.asarray(level, np.float64)
    sh = sh.astype(np.float64)
    rel0 = np.abs(sh[:, 0, :] / (level * 4.0 * np.pi * Y0_EXACT) - 1.0).max()
    sigma = level * np.sqrt(4.0 * np.pi / samples)
    worst = (np.abs(sh[:, 1:, :]) / sigma).max()
    print(f"{label} S={samples}: sh[0] off by {rel0:.3e} (bound {(samples + 4) * 2.0 ** -24:.3e}), worst other coefficient {worst:.2f} sigma (bound 6)")
    assert rel0 <= (samples + 4) * 2.0 ** -24
    assert worst <= 6.0
