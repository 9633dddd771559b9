"""CPU: the MultiClass layer (classes, SVGP routing, reverse pass) driven by the test bodies of tests/test_gpu_multiclass.py with
the device primitives replaced by their NumPy emulation (tests/emulation.py: every tests/fake_*.py; the MultiClass code is a
row of the table of tests/fake_likelihood_ops.py) -- exactly as tests/test_likelihoods_emulated.py drives tests/test_gpu_likelihoods.py.
What this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The CPU-only checks of the feature
(constructors, refusals, what the library answers before it touches a device) are at the end; they need no device.
"""
import ctypes

import numpy as np
import pytest

import emulation
import test_gpu_multiclass as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def test_library_reports_a_bad_multiclass_likelihood_before_the_device():
    """gpk_likelihood_varexp_sum with code 4 and no parameter array answers GPK_E_ARG (-1) -- not GPK_E_UNSUPPORTED (-3), which is
    what a library without the code says -- with rows = 0 and host buffers in the pointer slots it checks first: nothing is
    launched.  One class, seventeen classes and epsilon outside (0, 1) are GPK_E_ARG too; so is the fused shard's answer."""
    from gpflow_amd import _lib, ops
    assert ops.LIKELIHOOD_CODES["multiclass_robustmax"] == 4
    lib = _lib.load()
    knn, out = _lib.host_doubles([1.0]), _lib.host_doubles([7.0, 7.0])
    nws = int(lib.gpk_reduce_workspace_bytes(0))
    ws = (ctypes.c_double * (nws // 8 + 1))()
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p).value   # noqa: E731

    def call(P, par):
        return lib.gpk_likelihood_varexp_sum(None, 4, par, None, 1, None, 0, P, None, 0, None, knn, 0, 0.0, None, None, None, None,
                                             addr(out), addr(ws), nws)
    assert call(2, None) == -1
    for P, eps in ((1, 1e-3), (17, 1e-3), (2, 0.0), (2, 1.0), (2, -0.5)):
        assert call(P, _lib.host_doubles([eps])) == -1, (P, eps)
    assert list(out) == [7.0, 7.0]                           # (refused: nothing written)
    assert lib.gpk_likelihood_varexp_sum(None, 5, None, None, 1, None, 0, 2, None, 0, None, knn, 0, 0.0, None, None, None, None,
                                         addr(out), addr(ws), nws) == -3
    # the fused shard: the likelihood is checked before the workspace and before anything is launched
    one = _lib.host_doubles([1.0])
    for P, par in ((3, None), (1, _lib.host_doubles([1e-3])), (3, _lib.host_doubles([1.0]))):
        assert lib.gpk_svgp_elbo_shard_lik(None, 0, addr(ws), 8, 2, None, None, 0, 2, 1, 2, P, one, 0, 1.0, 4, par, 1e-6, 0.0, addr(ws),
                                           addr(ws), 1, 1, addr(out), addr(ws), None, 0) == -1, P


def test_multiclass_constructors_and_defaults():
    import torch
    import gpflow_amd as gpflow
    L = gpflow.likelihoods
    r = L.RobustMax(4)
    assert r.num_classes == 4 and r.epsilon == 1e-3 and r.eps_k1 == pytest.approx(1e-3 / 3, rel=1e-15)
    assert L.RobustMax(3, epsilon=0.05).eps_k1 == pytest.approx(0.025, rel=1e-15)
    for bad in (0.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            L.RobustMax(3, epsilon=bad)
    with pytest.raises(ValueError):
        L.RobustMax(1)
    m = L.MultiClass(3)
    assert isinstance(m, L.Likelihood) and not isinstance(m, L.ScalarLikelihood)
    assert isinstance(m.invlink, L.RobustMax) and m.invlink.num_classes == 3 and m.num_classes == 3
    assert m.device_lik == "multiclass_robustmax" and m.device_params() == (1e-3,) and m.parameters == ()
    assert L.MultiClass(3, invlink=L.RobustMax(3, epsilon=0.01)).device_params() == (0.01,)
    for other in (torch.softmax, L.inv_probit, "softmax"):
        with pytest.raises(NotImplementedError):
            L.MultiClass(3, invlink=other)


def test_multiclass_refusals_before_touching_the_device():
    """q_mu of the wrong width is a ValueError at elbo; 17 classes, the un-whitened form, active_dims, a kernel sum and separate
    kernels under elbo_and_grad, and the device-resident trainer, say NotImplementedError (no device here: anything that reached
    one would raise something else)."""
    import gpflow_amd as gpflow
    from gpflow_amd import training
    K, L = gpflow.kernels, gpflow.likelihoods
    Z = np.random.default_rng(0).normal(size=(5, 2))
    data = (np.zeros((4, 2)), np.ones((4, 1)))
    wrong = gpflow.models.SVGP(K.SquaredExponential(), L.MultiClass(3), Z, num_latent_gps=2)
    for fn in (wrong.elbo, wrong.elbo_terms, wrong.elbo_and_grad):
        with pytest.raises(ValueError, match="latent"):
            fn(data)
    big = gpflow.models.SVGP(K.SquaredExponential(), L.MultiClass(17), Z, num_latent_gps=17)
    for fn in (big.elbo, big.elbo_and_grad):
        with pytest.raises(NotImplementedError, match="16"):
            fn(data)
    with pytest.raises(NotImplementedError, match="16"):
        L.MultiClass(17).variational_expectations(None, np.zeros((4, 17)), np.ones((4, 17)), np.zeros((4, 1)))
    lik = L.MultiClass(3)
    refused = [
        gpflow.models.SVGP(K.SquaredExponential(), lik, Z, whiten=False, num_latent_gps=3),
        gpflow.models.SVGP(K.Matern32() + K.SquaredExponential(), lik, Z, num_latent_gps=3),
        gpflow.models.SVGP(K.SquaredExponential(active_dims=[0]), lik, Z, num_latent_gps=3),
        gpflow.models.SVGP(K.SeparateIndependent([K.SquaredExponential() for _ in range(3)]), lik,
                           gpflow.inducing_variables.SharedIndependentInducingVariables(gpflow.inducing_variables.InducingPoints(Z)),
                           num_latent_gps=3),
    ]
    for m in refused:
        with pytest.raises(NotImplementedError):
            m.elbo_and_grad(data)
    for m in refused + [gpflow.models.SVGP(K.SquaredExponential(), lik, Z, num_latent_gps=3)]:
        with pytest.raises(NotImplementedError):
            training.SVGPTrainer(m)
