"""CPU: the likelihood layer (classes, SVGP routing, reverse pass) driven by the test bodies of tests/test_gpu_likelihoods.py
with the device primitives replaced by their NumPy emulation (tests/emulation.py: every tests/fake_*.py, with
tests/fake_likelihood_ops.py for the three likelihood primitives) -- following tests/test_host_emulated.py.  What this does NOT test is the HIP kernel: that is what the same
bodies do under `-m gpu`.  The CPU-only checks of the feature (the quadrature table the library holds, constructors, refusals)
are at the end; they need no device.
"""
import numpy as np
import pytest

import emulation
import test_gpu_likelihoods as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ 1. CPU-only checks
def test_library_gauss_hermite_table_is_numpy_hermgauss():
    """gpk_gauss_hermite(20) -- the constants compiled into the kernel -- against numpy.polynomial.hermite.hermgauss(20).
    Tolerance 4 ulp of each entry: the table was written from hermgauss with 17 significant digits (exact round trip), and
    hermgauss itself (eigenvalues of the companion matrix, one Newton step, weights from the derivative) reproduces its values
    to a few ulp across LAPACK builds."""
    from gpflow_amd import _lib, ops
    x, w = ops.gauss_hermite(20)
    xr, wr = np.polynomial.hermite.hermgauss(20)
    assert x.shape == w.shape == (20,)
    assert np.all(np.abs(x - xr) <= 4 * 2.0 ** -52 * np.abs(xr))
    assert np.all(np.abs(w - wr) <= 4 * 2.0 ** -52 * np.abs(wr))
    assert np.array_equal(x, -x[::-1]) and np.array_equal(w, w[::-1])     # symmetric table
    assert abs(w.sum() / np.sqrt(np.pi) - 1.0) <= 8 * 2.0 ** -53
    with pytest.raises(_lib.GpkError, match="UNSUPPORTED"):
        ops.gauss_hermite(19)
    lib = _lib.load()
    assert lib.gpk_gauss_hermite(20, None, None) == -1
    # the quadrature entry points report a bad likelihood before anything touches a device
    assert lib.gpk_likelihood_varexp_sum(None, 1, None, None, 1, None, 0, 17, None, 0, None, None, 0, 0.0, None, None, None, None,
                                         None, None, 0) == -1
    assert lib.gpk_svgp_elbo_shard_lik(None, 0, None, 8, 2, None, None, 0, 2, 1, 2, 1, None, 0, 1.0, 0, None, 1e-6, 0.0, None, None,
                                       0, 1, None, None, None, 0) == -3


def test_likelihood_constructors_and_links():
    import torch
    import gpflow_amd as gpflow
    L = gpflow.likelihoods
    assert L.DEFAULT_NUM_GAUSS_HERMITE_POINTS == 20
    b = L.Bernoulli()
    assert b.invlink is L.inv_probit and b.device_lik == "bernoulli_probit" and b.device_params() == () and b.parameters == ()
    with pytest.raises(NotImplementedError):
        L.Bernoulli(invlink=torch.sigmoid)
    p = L.Poisson(binsize=2.5)
    assert p.device_params() == (2.5,) and L.Poisson().binsize == 1.0 and L.Poisson(invlink=L.exp).invlink is L.exp
    with pytest.raises(NotImplementedError):
        L.Poisson(invlink=torch.nn.functional.softplus)
    with pytest.raises(ValueError):
        L.Poisson(binsize=0.0)
    s = L.StudentT(scale=0.5, df=4.0)
    assert s.device_params() == (pytest.approx(0.5, rel=1e-15), 4.0) and s.df == 4.0
    assert s.parameters == (s.scale,) and s.scale.trainable
    assert L.StudentT().device_params() == (pytest.approx(1.0, rel=1e-15), 3.0)
    with pytest.raises(ValueError):
        L.StudentT(scale=-1.0)
    for lik in (b, p, s):
        assert isinstance(lik, L.ScalarLikelihood) and isinstance(lik, L.Likelihood)
    x = torch.tensor([-1.0, 0.0, 2.0], dtype=torch.float64)
    np.testing.assert_allclose(L.inv_probit(x).numpy(), 0.5 * (1 + torch.erf(x / np.sqrt(2.0)).numpy()) * 0.998 + 1e-3, rtol=1e-15)
    m = gpflow.models.SVGP(gpflow.kernels.SquaredExponential(), s, np.zeros((4, 2)) + np.arange(4)[:, None])
    assert ".likelihood.scale" in gpflow.utilities.parameter_dict(m) and len(m.trainable_parameters) == 6


def test_refusals_before_touching_the_device():
    """With these likelihoods the reverse pass covers the whitened SVGP with one stationary kernel; the un-whitened form, kernel
    combinations, separate kernels, active_dims and the device-resident trainer say NotImplementedError (no device here: anything
    that reached one would raise something else)."""
    import gpflow_amd as gpflow
    from gpflow_amd import training
    K, L = gpflow.kernels, gpflow.likelihoods
    Z = np.random.default_rng(0).normal(size=(5, 2))
    data = (np.zeros((4, 2)), np.ones((4, 1)))
    for lik in (L.Bernoulli(), L.Poisson(), L.StudentT()):
        refused = [
            gpflow.models.SVGP(K.SquaredExponential(), lik, Z, whiten=False),
            gpflow.models.SVGP(K.Matern32() + K.SquaredExponential(), lik, Z),
            gpflow.models.SVGP(K.SquaredExponential(active_dims=[0]), lik, Z),
            gpflow.models.SVGP(K.SeparateIndependent([K.SquaredExponential()]), lik,
                               gpflow.inducing_variables.SharedIndependentInducingVariables(gpflow.inducing_variables.InducingPoints(Z))),
        ]
        for m in refused:
            with pytest.raises(NotImplementedError):
                m.elbo_and_grad(data)
        for m in refused + [gpflow.models.SVGP(K.SquaredExponential(), lik, Z)]:
            with pytest.raises(NotImplementedError):
                training.SVGPTrainer(m)
