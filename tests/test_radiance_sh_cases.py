"""rt_radiance_sh's numpy statement (radiance_sh_cases.py) held to what it stands for, without a GPU: the nine basis functions are
orthonormal over the sphere (which pins the constants and their order), a constant field projects onto sh[0] alone within the bounds
of the sequential f32 sum and of the Monte-Carlo noise, and sh9_irradiance of a constant field is pi L."""
import numpy as np
import pytest

import radiance_sh_cases as rc
from gpu_raytracer_amd import api

F32 = np.float32
LEVEL = np.array([1.0, 0.2, 0.7], F32)


def _sphere_quadrature(nz=16, nphi=32):
    """Gauss-Legendre in z times the trapezoid rule in phi: exact for the products of two basis functions (polynomials of degree 4)."""
    z, wz = np.polynomial.legendre.leggauss(nz)
    phi = (np.arange(nphi) + 0.5) * (2.0 * np.pi / nphi)
    zz, pp = np.meshgrid(z, phi, indexing="ij")
    r = np.sqrt(1.0 - zz * zz)
    d = np.stack([r * np.cos(pp), r * np.sin(pp), zz], axis=-1).reshape(-1, 3)
    w = np.repeat(wz, nphi) * (2.0 * np.pi / nphi)
    return d, w


def test_the_basis_is_orthonormal_over_the_sphere():
    d, w = _sphere_quadrature()
    assert abs(w.sum() - 4.0 * np.pi) < 1e-12
    y = rc.basis(d)
    assert y.dtype == np.float64 and y.shape == (len(d), 9)
    gram = (y * w[:, None]).T @ y
    print("largest deviation of the Gram matrix from the identity:", np.abs(gram - np.eye(9)).max())
    np.testing.assert_allclose(gram, np.eye(9), rtol=0, atol=1e-6)
    # the order: Y1, Y2, Y3 are y, z, x; Y4, Y5, Y7 are xy, yz, xz; Y6 is zonal; Y8 is x^2 - y^2
    x, yy, z = np.eye(3)
    at = lambda v: rc.basis(np.asarray(v, np.float64)[None, :])[0]
    assert at(yy)[1] > 0.48 and at(z)[2] > 0.48 and at(x)[3] > 0.48 and at(z)[6] > 0.63 and at(x)[8] > 0.54 and at(yy)[8] < -0.54
    s = np.sqrt(0.5)
    assert at([s, s, 0])[4] > 0.54 and at([0, s, s])[5] > 0.54 and at([s, 0, s])[7] > 0.54


def test_the_f32_basis_rounds_each_operation_once():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((1000, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    y = rc.basis(d)
    assert y.dtype == F32
    x, yy, z = d[:, 0], d[:, 1], d[:, 2]
    np.testing.assert_array_equal(y[:, 6], F32(0.31539157) * (F32(3.0) * (z * z) - F32(1.0)))
    np.testing.assert_array_equal(y[:, 8], F32(0.5462742) * (x * x - yy * yy))
    np.testing.assert_array_equal(y[:, 4], F32(1.0925484) * (x * yy))
    assert np.all(y[:, 0] == F32(0.2820948))
    np.testing.assert_allclose(y, rc.basis(d.astype(np.float64)), rtol=0, atol=1e-6)


def test_the_generator_and_the_directions(oracle_mod):
    """The draws are the frames': rng_for and the LCG of estimator_cases, and the directions are unit_vector's, probe-major."""
    import estimator_cases as ec
    seed, first, samples = 0xFFFFFFF0, 5, 7
    index = np.array([0, 15, 16, 66])  # the per-probe seed wraps at 16
    d = rc.directions(oracle_mod, index, samples, seed, first)
    assert d.shape == (4, samples, 3) and d.dtype == F32
    for row, i in enumerate(index):
        for k in range(samples):
            h = ec.hash_u32(np.uint32((seed + int(i) + (first + k) * ec.GOLDEN) & 0xFFFFFFFF))
            s1 = (int(h) * 1664525 + 1013904223) & 0xFFFFFFFF
            s2 = (s1 * 1664525 + 1013904223) & 0xFFFFFFFF
            u1, u2 = F32(s1 >> 8) / F32(16777216.0), F32(s2 >> 8) / F32(16777216.0)
            np.testing.assert_array_equal(d[row, k], oracle_mod.unit_vectors([u1], [u2])[0][0])
    np.testing.assert_allclose(np.linalg.norm(d.astype(np.float64), axis=-1), 1.0, rtol=0, atol=1e-6)


def test_the_projection_is_ordered_and_scaled_once():
    """Against a scalar loop written out: from zero, sample by sample, one product per term, one division and one multiply."""
    rng = np.random.default_rng(11)
    n, samples = 5, 13
    x = rng.uniform(0, 4, (n, samples, 3)).astype(F32)
    d = rng.standard_normal((n, samples, 3))
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)
    got = rc.project(x, d)
    y = rc.basis(d)
    for i in range(n):
        for j in range(9):
            for c in range(3):
                total = F32(0.0)
                for k in range(samples):
                    total = F32(total + F32(x[i, k, c] * y[i, k, j]))
                assert got[i, j, c] == F32(total * F32(F32(12.566371) / F32(samples)))


@pytest.mark.parametrize("samples", [64, 256, 1024, 4096])
def test_a_constant_field_projects_onto_the_first_coefficient(oracle_mod, samples):
    for seed in (0, 7, 12345, 0xFFFFFFF0):
        sh = rc.constant_field(oracle_mod, 67, samples, seed, LEVEL)
        assert sh.shape == (67, 9, 3) and sh.dtype == F32
        rc.check_constant_field(sh, samples, LEVEL, label=f"seed {seed:#x}")


def _normals(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def test_irradiance_of_a_constant_field_is_pi_times_it():
    normals = _normals(64, 5)
    sh = np.zeros((64, 9, 3))
    sh[:, 0, :] = LEVEL.astype(np.float64) * 4.0 * np.pi * rc.Y0_EXACT
    for dtype in (np.float64, np.float32):
        e = api.sh9_irradiance(sh.astype(dtype), normals.astype(dtype))
        assert e.shape == (64, 3) and e.dtype == dtype
        np.testing.assert_allclose(e / (np.pi * LEVEL.astype(np.float64)), 1.0, rtol=0, atol=1e-4)
    # each band's weight: a field that is Y_j itself comes back as A_j Y_j(n)
    bands = (np.pi,) + (2 * np.pi / 3,) * 3 + (np.pi / 4,) * 5
    for j, a in enumerate(bands):
        one = np.zeros((64, 9, 3))
        one[:, j, :] = 1.0
        np.testing.assert_allclose(api.sh9_irradiance(one, normals)[:, 0], a * rc.basis(normals)[:, j], rtol=0, atol=1e-6)


def test_irradiance_on_torch():
    torch = pytest.importorskip("torch")
    normals = _normals(16, 9).astype(F32)
    sh = np.zeros((16, 9, 3), F32)
    sh[:, 0, :] = LEVEL * F32(4.0 * np.pi * rc.Y0_EXACT)
    sh[:, 1:, :] = np.random.default_rng(2).uniform(-1, 1, (16, 8, 3)).astype(F32)
    e = api.sh9_irradiance(torch.from_numpy(sh), torch.from_numpy(normals))
    assert isinstance(e, torch.Tensor) and e.dtype == torch.float32 and tuple(e.shape) == (16, 3)
    np.testing.assert_allclose(e.numpy(), api.sh9_irradiance(sh, normals), rtol=0, atol=1e-5)
    with pytest.raises(TypeError, match="same kind"):
        api.sh9_irradiance(sh, torch.from_numpy(normals))
    with pytest.raises(TypeError, match="same kind"):
        api.sh9_irradiance(torch.from_numpy(sh), normals)
