"""CPU: the Periodic kernel (primitives, the matrix through the warp, every model route of the reverse pass) driven by the test
bodies of tests/test_gpu_periodic.py with the device primitives replaced by their NumPy emulation (tests/emulation.py: every
tests/fake_*.py, tests/fake_periodic_ops.py among them) -- as tests/test_kernel_families_emulated.py drives
tests/test_gpu_kernel_families.py.  What this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The
CPU-only checks of the feature (the constructor, what the library answers before it touches a device, the spec's bookkeeping) are at
the end; they need no device.
"""
import ctypes

import numpy as np
import pytest

import emulation
import test_gpu_periodic as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def test_constructor_exports_and_leaf():
    import gpflow_amd as gpflow
    from gpflow_amd.kernels.base import DeviceLeaf, is_device_leaf
    K = gpflow.kernels
    assert "Periodic" in K.__all__ and issubclass(K.Periodic, DeviceLeaf) and not issubclass(K.Periodic, K.IsotropicStationary)
    assert {"periodic_warp", "periodic_moment_rows", "periodic_adjoint_tail"} <= set(dir(gpflow.ops))
    rq = K.RationalQuadratic(variance=1.5, lengthscales=[0.5, 2.0], alpha=0.25, active_dims=[0, 2])
    k = K.Periodic(rq, period=[1.5, 3.0], name="per")
    assert k.name == "per" and isinstance(k.period, gpflow.Parameter) and list(k.active_dims) == [0, 2] and k.maps_inputs
    assert list(k.trainable_parameters) == [rq.variance, rq.lengthscales, rq.alpha, k.period] and k.leaf_params() == rq.leaf_params() + (k.period,)
    assert is_device_leaf(k) and k.family == "RationalQuadratic" and k.variance is rq.variance
    leaf = k.leaf()
    assert leaf.family == "RationalQuadratic" and leaf.variance == 1.5 and list(leaf.lengthscales) == [1.0, 1.0, 4.0, 4.0] \
        and leaf.keywords()["alpha"] == pytest.approx(0.25)
    iso = K.Periodic(K.SquaredExponential(lengthscales=0.7))
    assert float(iso.period.numpy()) == pytest.approx(1.0) and float(iso.leaf().lengthscales) == pytest.approx(1.4) and iso.leaf().is_plain
    assert iso.has_default_active_dims and not K.SquaredExponential().maps_inputs
    assert (iso + K.White()).kernels[0] is iso and isinstance(iso * K.SquaredExponential(), K.Product)


def test_spec_bookkeeping_for_a_periodic_member():
    """KernelSpec with `periods`: never packable, the user's layout of the shape gradient, names with "period" last"""
    from gpflow_amd import gradients
    from gpflow_amd.leaf import Leaf
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 2.0)], periods=[1.5])
    assert not spec.packable and gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 2.0)]).packable
    assert spec.parameter_names(0) == ("variance", "lengthscales", "period") and spec.n_shape(0) == 2
    assert float(spec.parts[0].base_lengthscales()) == 1.0
    ard = gradients.KernelSpec([Leaf("RationalQuadratic", 1.0, [2.0, 2.0, 3.0, 3.0], alpha=0.5), Leaf("White", 0.1)], "add",
                               periods=[[1.0, 2.0], None])
    assert ard.parameter_names(0) == ("variance", "lengthscales", "alpha", "period") and ard.parameter_names(1) == ("variance",)
    assert ard.n_shape(0) == 5 and ard.n_shape(1) == 0 and list(ard.parts[0].base_lengthscales()) == [1.0, 1.5]
    g = np.arange(5.0)
    parts = ard.split_shape(0, g)
    assert list(parts) == ["lengthscales", "alpha", "period"] and list(parts["lengthscales"]) == [0.0, 1.0] \
        and list(parts["alpha"]) == [2.0] and list(parts["period"]) == [3.0, 4.0]
    with pytest.raises(ValueError, match="period"):
        gradients.KernelSpec([Leaf("White", 0.1)], periods=[1.0])
    with pytest.raises(ValueError, match="period"):
        gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 2.0)], periods=[1.0, 2.0])


def test_library_answers_for_the_periodic_entry_points_before_the_device():
    """gpk_periodic_warp / _moment_rows / _adjoint_tail with host pointers in the slots they check first: d = 33 (2 d > GPK_MAX_D),
    d = 0, a leading dimension that is too small and a period of 0, -1, NaN or Inf are GPK_E_ARG (-1) before any launch; n = 0
    returns 0 without one.  The family codes and km(8) == -3 of test_kernel_families_emulated.py stay as they are."""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 256)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value
    one = _lib.host_doubles([1.0] * 33)

    def warp(d, per=one, ard=0, n=0, ldx=None, ldphi=None):
        return lib.gpk_periodic_warp(None, addr, d if ldx is None else ldx, n, d, per, ard, addr, 2 * d if ldphi is None else ldphi)

    def rows(d, per=one, ard=0, n2=0, ldv=None):
        return lib.gpk_periodic_moment_rows(None, addr, d, n2, d, per, ard, addr, n2 if ldv is None else ldv)

    def tail(d, per=one, ard=0, n1=0, ldr=None):
        return lib.gpk_periodic_adjoint_tail(None, addr, d, addr, 2 * d, addr, 2 * d, addr, 1 + 6 * d if ldr is None else ldr, n1, d, addr, per,
                                             ard, addr, d, addr, 0)
    assert [warp(d) for d in (1, 3, 32)] == [0, 0, 0] and [rows(d) for d in (1, 3, 32)] == [0, 0, 0]
    assert warp(32, ard=1) == 0 and rows(32, ard=1) == 0
    for d in (33, 64, 0, -1):
        assert (warp(d), rows(d), tail(d)) == (-1, -1, -1), d
    assert warp(3, n=-1) == -1 and warp(3, n=5, ldx=2) == -1 and warp(3, n=5, ldphi=5) == -1 and rows(3, n2=5, ldv=4) == -1
    assert tail(3, n1=5, ldr=18) == -1
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        per = _lib.host_doubles([bad, 1.0, 1.0])
        last = _lib.host_doubles([1.0, 1.0, bad])
        assert (warp(3, per, n=5), rows(3, per, n2=5), tail(3, per, n1=5)) == (-1, -1, -1), bad
        assert (warp(3, per), rows(3, per), tail(3, per)) == (-1, -1, -1), bad            # also with nothing to do
        assert (warp(3, last, 1, n=5), rows(3, last, 1, n2=5), tail(3, last, 1, n1=5)) == (-1, -1, -1), bad
        assert warp(3, last, 0) == 0                                                      # (one period: only the first entry is read)
    assert warp(3, None) == -1 and rows(3, None) == -1 and tail(3, None) == -1
    km = lib.gpk_kernel_matrix(None, 8, addr, 0, 2, None, 0, 0, 2, _lib.host_doubles([1.0]), 0, 1.0, 0.0, 0, addr, 4)
    assert km == -3 and sorted(__import__("gpflow_amd").ops.KERNEL_FAMILIES.values()) == list(range(8))
