"""CPU: the kernel families Exponential, RationalQuadratic, White and Constant (primitives, fused drivers, reverse pass, model
surface) driven by the test bodies of tests/test_gpu_kernel_families.py with the device primitives replaced by their NumPy
emulation (tests/emulation.py: every tests/fake_*.py; the eight families are in tests/fake_ops.py) -- exactly as
tests/test_lcm_emulated.py drives tests/test_gpu_lcm.py.  What this does NOT test is the HIP kernel: that is what the same bodies do
under `-m gpu`.  The CPU-only checks of the feature (constructors, what the library answers before it touches a device, the
exported functions) are at the end; they need no device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import emulation
import test_gpu_kernel_families as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def test_constructors_exports_and_parameters():
    import gpflow_amd as gpflow
    K = gpflow.kernels
    assert {"Exponential", "RationalQuadratic", "White", "Constant", "Bias", "Static"} <= set(K.__all__)
    assert K.Bias is K.Constant
    assert issubclass(K.Exponential, K.IsotropicStationary) and issubclass(K.RationalQuadratic, K.IsotropicStationary)
    assert issubclass(K.White, K.Static) and issubclass(K.Constant, K.Static) and not issubclass(K.Static, K.Stationary)
    assert {"Exponential": 4, "RationalQuadratic": 5, "White": 6, "Constant": 7}.items() <= gpflow.ops.KERNEL_FAMILIES.items()
    rq = K.RationalQuadratic(variance=1.5, lengthscales=[0.5, 2.0], alpha=0.25, active_dims=[0, 2], name="rq")
    assert isinstance(rq.alpha, gpflow.Parameter) and float(rq.alpha.numpy()) == pytest.approx(0.25) and rq.name == "rq"
    assert rq.alpha in rq.trainable_parameters and len(rq.trainable_parameters) == 3 and rq.ard
    assert float(K.RationalQuadratic().alpha.numpy()) == pytest.approx(1.0)
    with pytest.raises(Exception):
        K.RationalQuadratic(alpha=-1.0)                       # positive()
    with pytest.raises(TypeError):
        K.Exponential(period=2.0)
    with pytest.raises(ValueError, match="active_dims"):
        K.Exponential(lengthscales=[1.0, 2.0, 3.0], active_dims=[0, 1])
    w = K.White(2.5, active_dims=[1], name="w")
    assert float(w.variance.numpy()) == pytest.approx(2.5) and w.name == "w" and list(w.active_dims) == [1]
    assert w.trainable_parameters == (w.variance,) or list(w.trainable_parameters) == [w.variance]
    assert not hasattr(w, "lengthscales") and K.Constant().name == "Constant" and float(K.Constant().variance.numpy()) == pytest.approx(1.0)
    # leaf(): the one notion of a device-built leaf
    assert rq.leaf().family == "RationalQuadratic" and rq.leaf().keywords()["alpha"] == pytest.approx(0.25) \
        and K.Exponential().leaf().keywords().get("alpha") is None
    kw = w.leaf().keywords()
    assert (kw["family"], kw["variance"], float(kw["lengthscales"])) == ("White", pytest.approx(2.5), 1.0) and kw.get("alpha") is None
    from gpflow_amd.kernels.base import is_device_leaf
    assert all(is_device_leaf(k) for k in (rq, w, K.Constant(), K.Exponential(), K.Matern52()))
    assert not is_device_leaf(rq + w) and not is_device_leaf(K.SeparateIndependent([rq, w]))


def test_k_diag_and_sum_flattening_with_static_members(gp):
    K = gp.kernels
    X = np.random.default_rng(0).normal(size=(7, 3))
    for k, v in ((K.Exponential(variance=1.5), 1.5), (K.RationalQuadratic(variance=0.7, alpha=2.0), 0.7), (K.White(0.3), 0.3),
                 (K.Constant(2.0), 2.0)):
        d = k.K_diag(X)
        assert tuple(d.shape) == (7,) and bool((d == float(k.variance.numpy())).all()) and abs(float(d[0]) - v) < 1e-12
        assert tuple(k.K_diag(X.reshape(1, 7, 3)).shape) == (1, 7)
        assert bool((k(X, full_cov=False) == d).all())
    s = K.RBF() + K.White(0.3) + (K.Constant(2.0) + K.Exponential())
    assert isinstance(s, K.Sum) and [type(m).__name__ for m in s.kernels] == ["SquaredExponential", "White", "Constant", "Exponential"]
    p = K.Constant(2.0) * K.Matern32() + K.RationalQuadratic()
    assert [type(m).__name__ for m in p.kernels] == ["Product", "RationalQuadratic"]
    np.testing.assert_allclose(s.K_diag(X).numpy(), 1.0 + 0.3 + 2.0 + 1.0)
    np.testing.assert_allclose(p.K_diag(X).numpy(), 3.0)
    Ks = s.K(X).numpy()                                      # members fold in place: White only on the diagonal of K(X)
    np.testing.assert_allclose(np.diag(Ks), 4.3, atol=1e-12)
    assert np.all(s.K(X, X.copy()).numpy().diagonal() < 4.3 - 0.29)
    assert not K.White(0.3).K(X, X.copy()).numpy().any()


def test_alpha_is_a_value_error_outside_the_rational_quadratic():
    """ops itself, before the library is asked: alpha with another family, and RationalQuadratic without alpha"""
    from gpflow_amd import ops
    for family in ("SquaredExponential", "Matern12", "Exponential", "White", "Constant"):
        with pytest.raises(ValueError, match="alpha"):
            ops._ls_host(1.0, 2, family, 0.5)
    with pytest.raises(ValueError, match="alpha"):
        ops._ls_host(1.0, 2, "RationalQuadratic", None)
    assert list(ops._ls_host([1.0, 2.0], 2, "RationalQuadratic", 0.5)[0]) == [1.0, 2.0, 0.5]
    assert list(ops._ls_host(1.5, 3, "RationalQuadratic", 0.5)[0]) == [1.5, 0.5] and ops._ls_host(1.5, 3, "White")[1] == 0
    from gpflow_amd import gradients
    with pytest.raises(ValueError, match="alpha"):
        gradients.KernelSpec([("Matern32", 1.0, 1.0, 0.5)])
    with pytest.raises(ValueError, match="alpha"):
        gradients.KernelSpec.single(1.0, 1.0, "RationalQuadratic")
    spec = gradients.KernelSpec([("Constant", 2.0, 1.0), ("RationalQuadratic", 0.5, [1.0, 2.0], 0.7), ("White", 0.1, 1.0, None)], "add")
    assert [m.n_shape for m in spec.members] == [0, 3, 0] and spec.kdiag() == pytest.approx(2.6) and not spec.packable
    assert gradients.KernelSpec.single(1.0, [1.0, 2.0], "Exponential").packable


def test_library_answers_for_the_new_families_before_the_device():
    """gpk_kernel_matrix / _combine with host pointers in the slots they check first: a family outside [0, 7] and op 4 for a family
    without alpha are GPK_E_UNSUPPORTED (-3); alpha <= 0 or not finite, read from the trailing slot of ls_host, is GPK_E_ARG (-1);
    empty operands return 0 for every family without a launch; a RationalQuadratic member in the per-latent shards is -3."""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value

    def km(family, ls, n1=0):
        return lib.gpk_kernel_matrix(None, family, addr, n1, 2, None, 0, 0, 2, _lib.host_doubles(ls), 0, 1.0, 0.0, 0, addr, 4)

    def kc(family, op, ls, n1=0):
        return lib.gpk_kernel_matrix_combine(None, family, op, addr, n1, 2, None, 0, 0, 2, _lib.host_doubles(ls), 0, 1.0, 0.0, addr, 4,
                                             addr, 4)
    assert [km(f, [1.0, 1.0]) for f in range(8)] == [0] * 8 and km(8, [1.0]) == -3 and km(-1, [1.0]) == -3
    assert [kc(f, 4, [1.0, 1.0]) for f in range(8)] == [-3] * 5 + [0] + [-3] * 2
    assert kc(5, 5, [1.0, 1.0]) == -1 and kc(5, 0, [1.0, 1.0]) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert km(5, [1.0, bad], n1=3) == -1 and kc(5, 1, [1.0, bad], n1=3) == -1 and kc(5, 4, [1.0, bad], n1=3) == -1, bad
    fam = (ctypes.c_int * 2)(4, 5)
    one = _lib.host_doubles([1.0, 1.0])
    n = int(lib.gpk_svgp_elbo_sep_workspace_bytes(8, 0, 2, 2))
    ws = (ctypes.c_double * (n // 8 + 1))()
    wa = ctypes.cast(ws, ctypes.c_void_p).value
    assert lib.gpk_svgp_elbo_shard_sep(None, fam, addr, 8, 2, 0, None, None, 0, 2, 2, 2, 2, one, 0, one, 0.1, None, 1e-6, 0.0, addr, addr,
                                       addr, addr, wa, n) == -3


def test_header_and_library_export_the_same_functions():
    """the family codes of include/gpk.h are those of ops.KERNEL_FAMILIES, and libgpk.so exports exactly the functions the header
    declares (no entry point was added for the new families: alpha travels in ls_host)"""
    from gpflow_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GPK_KERN_(\w+) (\d+)", text)}
    assert codes == {"SE": 0, "MATERN12": 1, "MATERN32": 2, "MATERN52": 3, "EXPONENTIAL": 4, "RQ": 5, "WHITE": 6, "CONSTANT": 7}
    assert sorted(codes.values()) == sorted(ops.KERNEL_FAMILIES.values())
    declared = set(re.findall(r"\b(gpk_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in declared)
