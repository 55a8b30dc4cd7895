"""rt_irradiance's numpy statement (irradiance_cases.py) held to what it stands for, without a GPU: the directions are unit vectors of
the normal's hemisphere with a cosine density (the mean of cos theta is 2/3, a cap of half-angle a holds sin^2 a of them), the origins
and the no-point rule are the statement's, and the reduction is the ordered f32 sum times pi / S."""
import numpy as np
import pytest

import irradiance_cases as ic

F32 = np.float32
SEEDS = (0, 7, 12345, 0xFFFFFFF0)
LEVEL = np.array([1.0, 0.2, 0.7], F32)


def _points(positions, normals):
    p = np.zeros((len(positions), 8), F32)
    p[:, 0:3], p[:, 4:7] = positions, normals
    p.view(np.uint32)[:, 3], p.view(np.uint32)[:, 7] = 0xDEADBEEF, 0xFFFFFFFF  # prim_id, material_id: ignored
    return p


def _unit(n, seed):
    v = np.random.default_rng(seed).standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def test_the_generator_and_the_lobe(oracle_mod):
    """The draws are the frames': rng_for and the LCG of estimator_cases; the direction is normalize(N + unit_vector) written out."""
    import estimator_cases as ec
    seed, first, samples = 0xFFFFFFF0, 5, 7
    index = np.array([0, 15, 16, 66])  # the per-point seed wraps at 16
    points = _points(np.zeros((4, 3)), _unit(4, 1))
    d = ic.directions(oracle_mod, points, index, samples, seed, first)
    assert d.shape == (4, samples, 3) and d.dtype == F32
    for row, i in enumerate(index):
        for k in range(samples):
            h = ec.hash_u32(np.uint32((seed + int(i) + (first + k) * ec.GOLDEN) & 0xFFFFFFFF))
            s1 = (int(h) * 1664525 + 1013904223) & 0xFFFFFFFF
            s2 = (s1 * 1664525 + 1013904223) & 0xFFFFFFFF
            u1, u2 = F32(s1 >> 8) / F32(16777216.0), F32(s2 >> 8) / F32(16777216.0)
            w = points[row, 4:7] + oracle_mod.unit_vectors([u1], [u2])[0][0]
            ww = F32(F32(F32(w[0] * w[0]) + F32(w[1] * w[1])) + F32(w[2] * w[2]))
            assert ww >= F32(1e-12)
            np.testing.assert_array_equal(d[row, k], w * F32(F32(1.0) / np.sqrt(ww)))


def test_a_vanishing_lobe_vector_falls_back_to_the_normal():
    """unit_vector(0, u2) is (0, 0, 1) exactly (z = 1 - 2 * 0, r = 0): with N = (0, 0, -1) w is zero, so d is N."""

    class Pole:
        @staticmethod
        def unit_vectors(u1, u2):
            return np.tile(np.array([0, 0, 1], F32), (np.size(u1), 1)), None

    points = _points(np.zeros((2, 3)), np.array([[0, 0, -1], [0, 0, 1]], F32))
    d = ic.directions(Pole, points, np.arange(2), 3, 0, 0)
    np.testing.assert_array_equal(d[0], np.tile(np.array([0, 0, -1], F32), (3, 1)))
    np.testing.assert_array_equal(d[1], np.tile(np.array([0, 0, 1], F32), (3, 1)))


def test_directions_are_unit_and_in_the_normals_hemisphere(oracle_mod):
    n, samples = 257, 64
    normals = _unit(n, 2)
    points = _points(np.random.default_rng(3).uniform(-2, 2, (n, 3)), normals)
    for seed in SEEDS:
        d = ic.directions(oracle_mod, points, np.arange(n), samples, seed, 3).astype(np.float64)
        off = np.abs(np.linalg.norm(d, axis=-1) - 1.0).max()
        lowest = (d * normals.astype(np.float64)[:, None, :]).sum(-1).min()
        print(f"seed {seed:#x}: |d| off 1 by at most {off:.3e} (bound {4 * 2.0 ** -23:.3e}), lowest cos theta {lowest:.3e}")
        assert off <= 4 * 2.0 ** -23  # the reciprocal square root and the product: a few ulp
        assert lowest >= -1e-6


def test_the_density_is_the_cosine(oracle_mod):
    """For N = (0, 0, 1) d.z is cos theta; under the density cos / pi its mean is 2/3 and its variance 1/2 - 4/9 = 1/18."""
    n, samples = 4096, 64
    points = _points(np.zeros((n, 3)), np.tile(np.array([0, 0, 1], F32), (n, 1)))
    for seed in SEEDS:
        d = ic.directions(oracle_mod, points, np.arange(n), samples, seed, 0)
        mean = d[..., 2].astype(np.float64).mean()
        sigma = np.sqrt(1.0 / 18.0 / (n * samples))
        print(f"seed {seed:#x}: mean cos theta {mean:.6f}, {abs(mean - 2 / 3) / sigma:.2f} sigma from 2/3 (bound 6; a uniform hemisphere has 1/2)")
        assert abs(mean - 2.0 / 3.0) <= 6.0 * sigma
        assert (d[..., 2] >= 0).all()


def test_origins_and_no_points():
    points = _points([[1, 2, 3], [0, 0, 0], [5, 5, 5], [1, 1, 1], [1, 1, 1], [np.inf, 0, 0]], [[0, 0, 2], [0.6, 0, 0.8], [0, 0, 0], [np.nan, 0, 1], [0, -np.inf, 0], [0, 1, 0]])
    np.testing.assert_array_equal(ic.origins(points)[:2], np.array([[1, 2, F32(3) + F32(2) * F32(0.001)], [F32(0.6) * F32(0.001), 0, F32(0.8) * F32(0.001)]], F32))
    assert ic.origins(points).dtype == F32
    assert ic.is_point(points).tolist() == [True, True, False, False, False, False]
    tiny = _points([[0, 0, 0]], [[0, 1e-45, 0]])  # a denormal normal is a normal
    assert ic.is_point(tiny).tolist() == [True]


def test_the_reduction_is_ordered_and_scaled_once():
    """Against a scalar loop written out: from zero, sample by sample, then one division and one multiply."""
    rng = np.random.default_rng(11)
    n, samples = 5, 13
    x = rng.uniform(0, 4, (n, samples, 3)).astype(F32)
    got = ic.reduce(x)
    assert got.dtype == F32 and got.shape == (n, 3)
    for i in range(n):
        for c in range(3):
            total = F32(0.0)
            for k in range(samples):
                total = F32(total + x[i, k, c])
            assert got[i, c] == F32(total * F32(F32(3.1415927) / F32(samples)))
    # the order is part of it: large then small terms are not small then large
    y = np.array([[[2.0 ** 24] * 3] + [[1.0] * 3] * 4], F32)
    assert not np.array_equal(ic.reduce(y), ic.reduce(y[:, ::-1]))


@pytest.mark.parametrize("samples", [1, 3, 64, 65, 256, 4096])
def test_a_constant_field_gives_pi_times_it(samples):
    e = ic.reduce(np.broadcast_to(LEVEL, (4, samples, 3)).copy()).astype(np.float64)
    rel = np.abs(e / (np.pi * LEVEL.astype(np.float64)) - 1.0).max()
    print(f"S={samples}: pi L off by {rel:.3e} (bound {(samples + 4) * 2.0 ** -24:.3e})")
    assert rel <= (samples + 4) * 2.0 ** -24


def hits_sphere(o, d, centre, radius):
    """Whether the rays o + t d, t > 0, (float64) meet the sphere."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    oc = o - np.asarray(centre, np.float64)
    b = (oc * d).sum(-1)
    disc = b * b - (d * d).sum(-1) * ((oc * oc).sum(-1) - radius * radius)
    return (disc > 0) & (-b + np.sqrt(np.maximum(disc, 0)) > 0)


def test_the_blocked_cap(oracle_mod):
    """A sphere of radius 0.6 whose centre stands 1 above the point on its normal covers sin^2 a = 0.36 of a cosine-distributed
    hemisphere, and 1 - cos a = 0.2 of a uniform one: the drawn directions alone decide the bound the device test uses."""
    samples = 4096
    fraction, sigma = ic.blocked_cap_sigma(samples)
    assert abs(fraction - 0.36) < 1e-12 and abs(sigma - np.sqrt(0.36 * 0.64 / samples)) < 1e-15
    assert (fraction - 0.2) / sigma > 20.0
    points = _points([[0, 0, 0]], [[0, 0, 1]])
    o = ic.origins(points)
    for seed in SEEDS:
        d = ic.directions(oracle_mod, points, [0], samples, seed, 0)[0]
        got = hits_sphere(o, d, (0, 0, 1), 0.6).mean()
        print(f"seed {seed:#x}: {got:.4f} of the directions are blocked, {abs(got - fraction) / sigma:.2f} sigma from 0.36 (bound 6)")
        assert abs(got - fraction) <= 6.0 * sigma
