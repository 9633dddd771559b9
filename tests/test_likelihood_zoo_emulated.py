"""CPU: the Exponential / Gamma / Beta / Ordinal layer (classes, SVGP routing, reverse pass) driven by the test bodies of
tests/test_gpu_likelihood_zoo.py with the device primitives replaced by their NumPy emulation (tests/emulation.py: every
tests/fake_*.py; the eight likelihood codes are the table of tests/fake_likelihood_ops.py) -- following
tests/test_likelihoods_emulated.py.  What this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The
CPU-only checks (the library's answers to bad parameters and unknown codes, the psi routine against mpmath, constructors, refusals)
are at the end; they need no device.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import emulation
import test_gpu_likelihood_zoo as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def _doubles(values):
    return (ctypes.c_double * len(values))(*values) if len(values) else None


def test_library_answers_before_the_device():
    """gpk_likelihood_varexp_sum with rows = 0 and nothing to write: the library judges the code and its parameters on the host, before
    anything touches a device.  Codes 0, 5, 6, 7 are unknown (-3, GPK_E_UNSUPPORTED); the bad parameter sets of the GPU file are
    GPK_E_ARG (-1); the fused shard answers the same."""
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    assert {k: ops.LIKELIHOOD_CODES[k] for k in ("exponential_exp", "gamma_exp", "beta_probit", "ordinal")} == \
        {"exponential_exp": 8, "gamma_exp": 9, "beta_probit": 10, "ordinal": 11}
    assert "logit" not in ops.LIKELIHOOD_CODES and not set(ops.LIKELIHOOD_CODES.values()) & {0, 5, 6, 7}
    knn = _doubles([1.0])
    # HOST memory for out and the workspace: a refused call returns before either is touched (the workspace only has to pass the
    # size and alignment check that comes first)
    out = _doubles([7.0, 7.0])
    need = int(lib.gpk_reduce_workspace_bytes(0))
    buf = np.full(need // 8 + 4, 7.0)
    off = (-buf.ctypes.data % 16) // 8
    ws = buf.ctypes.data + 8 * off

    def answer(code, par):
        return lib.gpk_likelihood_varexp_sum(None, code, _doubles(par), None, 1, None, 0, 2, None, 0, None, knn, 0, 0.0, None, None,
                                             None, None, ctypes.cast(out, ctypes.c_void_p), ctypes.c_void_p(ws), need)
    for code in (0, 5, 6, 7, 12, -1):
        assert answer(code, [1.0]) == -3, code
    for lik, par in T.BAD_PARAMS:
        # (an array of the wrong LENGTH is the wrapper's to refuse -- ops._lik_npar: the library cannot see a length)
        if lik in ("gamma_exp", "beta_probit") or (lik == "ordinal" and len(par) != 1 and ops._lik_npar(lik, list(par)) in (-1, len(par))):
            assert answer(ops.LIKELIHOOD_CODES[lik], [float(v) for v in par]) == -1, (lik, par)
    assert answer(11, [1.0, 2.5, 0.0, 1.0, 2.0]) == -1      # a fractional edge count
    assert list(out) == [7.0, 7.0] and (buf == 7.0).all()


def test_digamma_routine_against_mpmath(tmp_path):
    """gpk_digamma (gpflow_amd/csrc/digamma.h), compiled into a small host program, against mpmath.digamma on a grid over
    [1e-3, 1e3] that includes the neighbourhood of the root 1.4616..., the recurrence threshold 10 and the integers below it -- under
    the ABSOLUTE bound derived beside the routine (`_psi_bound` reads its constants from the header)."""
    import mpmath
    import shutil
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    hdr = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpflow_amd", "csrc")
    src = tmp_path / "psi.cpp"
    src.write_text('#include <cstdio>\n#include "digamma.h"\nint main() { double x; while (std::scanf("%lf", &x) == 1) '
                   'std::printf("%.17g %.17g\\n", gpk_digamma(x), gpk_digamma_abs_bound(x)); return 0; }\n')
    exe = tmp_path / "psi"
    subprocess.run([cxx, "-O2", "-ffp-contract=on", "-I", hdr, str(src), "-o", str(exe)], check=True)
    root = 1.4616321449683623
    grid = np.concatenate([np.geomspace(1e-3, 1e3, 400), root + np.linspace(-1e-3, 1e-3, 41), root * (1 + np.array([-1, 0, 1]) * 2.0 ** -52),
                           10.0 + np.linspace(-1e-6, 1e-6, 21), np.nextafter(10.0, [0.0, 20.0]), np.arange(1.0, 12.0),
                           np.arange(1.0, 12.0) - 2.0 ** -40])
    res = subprocess.run([str(exe)], input="\n".join(repr(float(v)) for v in grid), capture_output=True, text=True, check=True)
    got = np.array([[float(t) for t in line.split()] for line in res.stdout.splitlines()])
    assert got.shape == (grid.size, 2)
    mpmath.mp.dps = 40
    bound = T._psi_bound(grid)
    worst = 0.0
    for x, (v, b), bb in zip(grid, got, bound):
        err = abs(mpmath.mpf(float(v)) - mpmath.digamma(mpmath.mpf(float(x))))
        worst = max(worst, float(err / mpmath.mpf(float(bb))))
        assert float(err) <= float(bb), (x, v, float(err), float(bb))
        assert abs(b - float(bb)) <= 1e-12 * float(bb)      # the routine's own statement of the bound is the same expression
    print(f"gpk_digamma: max error / bound = {worst:.3g} over {grid.size} points")


def test_zoo_constructors_and_links():
    import torch
    import gpflow_amd as gpflow
    L = gpflow.likelihoods
    e, g, b, o = L.Exponential(), L.Gamma(shape=2.5), L.Beta(scale=3.0), L.Ordinal([-1.0, 0.5, 2.0])
    assert e.invlink is L.exp and e.device_lik == "exponential_exp" and e.device_params() == () and e.parameters == ()
    assert g.invlink is L.exp and g.device_params() == (pytest.approx(2.5, rel=1e-15),) and g.parameters == (g.shape,)
    assert L.Gamma().device_params() == (pytest.approx(1.0, rel=1e-15),) and L.Gamma(L.exp, 2.0).device_params()[0] == pytest.approx(2.0)
    assert b.invlink is L.inv_probit and b.device_params() == (pytest.approx(3.0, rel=1e-15),) and b.parameters == (b.scale,)
    assert o.num_bins == 4 and o.parameters == (o.sigma,) and o.sigma.trainable
    assert o.device_params() == (pytest.approx(1.0, rel=1e-15), 3.0, -1.0, 0.5, 2.0)
    assert (e.device_grad_param, g.device_grad_param, b.device_grad_param, o.device_grad_param) == (None, "shape", "scale", "sigma")
    assert L.StudentT.device_grad_param == "scale" and L.Bernoulli.device_grad_param is None and L.Poisson.device_grad_param is None
    assert L.device_grad_param("student_t") == "scale" and L.device_grad_param("ordinal") == "sigma"
    for lik in (e, g, b, o):
        assert isinstance(lik, L.ScalarLikelihood)
    for bad in (lambda: L.Exponential(invlink=torch.nn.functional.softplus), lambda: L.Gamma(invlink=torch.nn.functional.softplus),
                lambda: L.Beta(invlink=torch.sigmoid), lambda: L.Bernoulli(invlink=torch.sigmoid),
                lambda: L.Poisson(invlink=torch.nn.functional.softplus)):
        with pytest.raises(NotImplementedError):
            bad()
    for edges in ([[0.0, 1.0]], [1.0, 1.0], [1.0, 0.0], list(range(16)), [], [0.0, float("inf")]):
        with pytest.raises(ValueError):
            L.Ordinal(edges)
    for bad in (lambda: L.Gamma(shape=-1.0), lambda: L.Beta(scale=-1.0)):
        with pytest.raises(ValueError):
            bad()
    assert L.Ordinal(list(range(15))).num_bins == 16
    m = gpflow.models.SVGP(gpflow.kernels.SquaredExponential(), o, np.zeros((4, 2)) + np.arange(4)[:, None])
    assert ".likelihood.sigma" in gpflow.utilities.parameter_dict(m)


def test_zoo_refusals_before_touching_the_device():
    """The scope of the existing quadrature likelihoods: the un-whitened reverse pass, kernel combinations, separate kernels, the
    device-resident trainer and natural gradients say NotImplementedError."""
    import gpflow_amd as gpflow
    from gpflow_amd import training
    K, L = gpflow.kernels, gpflow.likelihoods
    Z = np.random.default_rng(0).normal(size=(5, 2))
    data = (np.zeros((4, 2)), np.ones((4, 1)) * 0.5)
    for lik in (L.Exponential(), L.Gamma(), L.Beta(), L.Ordinal([0.0, 1.0])):
        refused = [gpflow.models.SVGP(K.SquaredExponential(), lik, Z, whiten=False),
                   gpflow.models.SVGP(K.Matern32() + K.SquaredExponential(), lik, Z)]
        for m in refused:
            with pytest.raises(NotImplementedError):
                m.elbo_and_grad(data)
        for m in refused + [gpflow.models.SVGP(K.SquaredExponential(), lik, Z)]:
            with pytest.raises(NotImplementedError):
                training.SVGPTrainer(m)
