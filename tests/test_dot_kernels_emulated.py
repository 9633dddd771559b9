"""CPU: the dot-product kernels (primitives, the classes on every forward route, the reverse pass of GPR and SVGP with a row diagonal)
driven by the test bodies of tests/test_gpu_dot_kernels.py with the device primitives replaced by their NumPy emulation
(tests/emulation.py: every tests/fake_*.py) -- as tests/test_periodic_emulated.py drives tests/test_gpu_periodic.py.  What this does NOT test is the HIP kernel: that is what
the same bodies do under `-m gpu`.  The CPU-only checks of the feature (what the library answers before it touches a device, the
leaf and the spec's bookkeeping, the launch list of a constant-diagonal spec) are at the end; they need no device.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import emulation
import test_gpu_dot_kernels as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def test_exports_leaf_and_classes():
    import gpflow_amd as gpflow
    from gpflow_amd import leaf, ops
    from gpflow_amd.kernels.base import DeviceLeaf, is_device_leaf, is_dot_leaf
    K = gpflow.kernels
    assert {"Linear", "Polynomial"} <= set(K.__all__) and issubclass(K.Polynomial, K.Linear) and not issubclass(K.Linear, DeviceLeaf)
    assert {"dot_kernel_matrix", "dot_kernel_matrix_combine", "dot_kernel_diag", "dot_adjoint_tail"} <= set(dir(ops))
    assert sorted(ops.KERNEL_FAMILIES.values()) == list(range(8)) and "Linear" not in ops.KERNEL_FAMILIES
    assert [(f.name, f.code, f.parameters) for f in leaf.DOT_FAMILIES] == [("Linear", 0, ("variance",)), ("Polynomial", 1, ("variance", "offset"))]
    assert [f.name for f in leaf.FAMILIES] == ["SquaredExponential", "Matern12", "Matern32", "Matern52", "Exponential", "RationalQuadratic",
                                               "White", "Constant"]
    k = K.Polynomial(degree=2.0, variance=[0.5, 2.0], offset=0.3, active_dims=[2, 0], name="poly")
    assert k.name == "poly" and list(k.active_dims) == [2, 0] and k.ard and k.degree == 2 and is_dot_leaf(k) and not is_device_leaf(k)
    assert list(k.trainable_parameters) == [k.variance, k.offset] and k.leaf_params() == (k.variance, k.offset)
    lf = k.leaf()
    assert isinstance(lf, leaf.DotLeaf) and lf.family == "Polynomial" and lf.code == 1 and list(lf.variance) == [0.5, 2.0] \
        and lf.offset == pytest.approx(0.3) and lf.degree == 2 and lf.n_variance == 2 and lf.n_shape == 1 and lf.ard
    assert set(lf.keywords()) == {"family", "variance", "offset", "degree"}
    w, ard = lf.host(2)
    assert list(w) == [0.5, 2.0] and ard == 1
    with pytest.raises(ValueError, match="entries"):
        lf.host(3)
    lin = K.Linear().leaf()
    assert set(lin.keywords()) == {"family", "variance"} and lin.n_variance == 1 and lin.n_shape == 0 and lin.host(5)[1] == 0
    assert lf.replace([[1.0, 3.0], 0.7]).degree == 2 and list(lf.replace([[1.0, 3.0], 0.7]).variance) == [1.0, 3.0]
    g = np.arange(1.0)
    assert list(lf.split_shape(g)) == ["lengthscales", "offset"] and lf.split_shape(g)["lengthscales"].size == 0 and lin.split_shape(g[:0])["lengthscales"].size == 0
    with pytest.raises(ValueError):
        leaf.DotLeaf("Linear", 1.0, offset=0.5)
    with pytest.raises(ValueError):
        leaf.DotLeaf("Polynomial", 1.0)
    with pytest.raises(ValueError):
        leaf.DotLeaf("SquaredExponential", 1.0)
    assert isinstance(K.SquaredExponential() + K.Linear(), K.Sum) and isinstance(K.Linear() * K.Polynomial(), K.Product)


def test_spec_bookkeeping_for_dot_members():
    """KernelSpec with DotLeaf members: never packable, no constant diagonal, the counts that cut grads["variance"], names and layouts"""
    from gpflow_amd import gradients
    from gpflow_amd.leaf import DotLeaf, Leaf
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), DotLeaf("Polynomial", [0.5, 1.0, 2.0], offset=0.3, degree=2),
                                 Leaf("White", 0.1), DotLeaf("Linear", 0.8)], ("add", [("mul", [0, 1]), 2, 3]))
    assert not spec.packable and not spec.constant_diagonal and [spec.is_dot(i) for i in range(4)] == [False, True, False, True]
    assert [spec.n_variance(i) for i in range(4)] == [1, 3, 1, 1] and [spec.n_shape(i) for i in range(4)] == [1, 1, 0, 0]
    assert spec.parameter_names(1) == ("variance", "offset") and spec.parameter_names(3) == ("variance",)
    assert gradients.KernelSpec([DotLeaf("Linear", 0.8)]).tree == 0 and not gradients.KernelSpec([DotLeaf("Linear", 0.8)]).packable
    with pytest.raises(ValueError, match="period"):
        gradients.KernelSpec([DotLeaf("Linear", 0.8)], periods=[1.0])
    import torch
    grads = spec.kernel_grads(torch.arange(6.0), [torch.tensor([10.0]), torch.tensor([11.0]), torch.zeros(0), torch.zeros(0)])
    assert [None if v is None else list(v) for v in grads["offset"]] == [None, [11.0], None, None]
    import gpflow_amd as gpflow
    K = gpflow.kernels
    kern = K.SquaredExponential() * K.Polynomial(2, variance=[0.5, 1.0, 2.0]) + K.White() + K.Linear()
    route = gpflow.models.reverse.CovarianceRoute(kern, 3)
    assert route.spec.tree == ("add", [("mul", [0, 1]), 2, 3]) and list(route._variance_cuts()) == [0, 1, 4, 5, 6]
    cut = route.member_grads(grads)
    assert [list(c[0]) for c in cut] == [[0.0], [1.0, 2.0, 3.0], [4.0], [5.0]] and list(cut[1][1]) == [11.0] and len(cut[3]) == 1
    pairs = route.kernel_pairs(grads)
    assert [p for p, _ in pairs] == [kern.kernels[0].kernels[0].variance, kern.kernels[0].kernels[0].lengthscales,
                                     kern.kernels[0].kernels[1].variance, kern.kernels[0].kernels[1].offset, kern.kernels[1].variance,
                                     kern.kernels[2].variance]
    assert list(pairs[2][1]) == [1.0, 2.0, 3.0] and list(pairs[3][1]) == [11.0]


def test_a_constant_diagonal_spec_issues_the_calls_it_issued(monkeypatch):
    """SquaredExponential + White through svgp_elbo_and_grad: no dot_* primitive, no kdiag_rows -- the composed route's launch list for
    the specs that were there is the one tests/test_gradients_cpu.py pins for the packed form, member by member"""
    import types
    import torch
    from gpflow_amd import gradients
    from gpflow_amd.leaf import Leaf
    calls = []

    def logged(name, fn):
        def call(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return call
    proxy = types.SimpleNamespace(**{n: logged(n, fn) for n, fn in emulation.primitives().items()})
    monkeypatch.setattr(gradients, "ops", proxy)
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    M, B, D, P = 16, 40, 3, 2
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), Leaf("White", 0.1)], "add")
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    gradients.svgp_elbo_and_grad(t(rng.normal(size=(M, D))), t(rng.normal(size=(B, D))), t(rng.normal(size=(B, P))),
                                 t(0.3 * rng.normal(size=(M, P))), t(q_sqrt), noise_variance=0.2, jitter=1e-6, kernel_spec=spec)
    assert not [c for c in calls if c.startswith("dot_")] and calls.count("gaussian_varexp_sum") == 1
    assert calls.count("kernel_matrix") == 2 and calls.count("kernel_matrix_combine") == 2 and calls.count("stationary_adjoint_tail") == 2


def test_library_answers_for_the_dot_entry_points_before_the_device():
    """every GPK_E_ARG (-1) / GPK_E_UNSUPPORTED (-3) case of include/gpk.h with host pointers or NULL in the slots checked first, and
    0 without a launch where there is nothing to do; the header's GPK_DOT_* constants; header, _lib._SIGS and the library export the
    same set; the stationary family table is untouched"""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value
    one = _lib.host_doubles([1.0] * 64)

    def km(family=0, n1=0, n2=0, d=3, w=one, ard=0, offset=0.5, degree=2, ldx1=None, ldx2=None, ldk=None, x2=True):
        return lib.gpk_dot_kernel_matrix(None, family, addr, n1, d if ldx1 is None else ldx1, addr if x2 else None, n2, d if ldx2 is None else ldx2,
                                         d, w, ard, offset, degree, 0.0, 0, addr, max(n2, n1, 1) if ldk is None else ldk)

    def kc(family=0, op=1, n1=0, n2=0, d=3, w=one, ard=0, offset=0.5, degree=2, ldg=None, ldo=None):
        return lib.gpk_dot_kernel_matrix_combine(None, family, op, addr, n1, d, addr, n2, d, d, w, ard, offset, degree, 0.0, addr,
                                                 max(n2, 1) if ldg is None else ldg, addr, max(n2, 1) if ldo is None else ldo)

    def kd(family=0, op=0, n=0, d=3, w=one, ard=0, offset=0.5, degree=2, ldx=None):
        return lib.gpk_dot_kernel_diag(None, family, op, addr, n, d if ldx is None else ldx, d, w, ard, offset, degree, addr, addr)

    def tail(n1=0, d=3, ldr=None, lda=None, ldab=None, w=addr, small=addr):
        return lib.gpk_dot_adjoint_tail(None, addr, 1 + d if ldr is None else ldr, addr, d if lda is None else lda, n1, d, w, 0, 0, small, addr,
                                        d if ldab is None else ldab)
    for f in (km, kc, kd):
        assert [f(family=fam, d=d) for fam in (0, 1) for d in (1, 3, 64)] == [0] * 6, f.__name__      # nothing to do: 0, no launch
        assert f(ard=1, d=64) == 0
        for d in (0, -1, 65):
            assert f(d=d) == -1, (f.__name__, d)
        assert f(w=None) == -1
        for fam in (-1, 2, 8):
            assert f(family=fam) == -3, (f.__name__, fam)
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert f(w=_lib.host_doubles([bad, 1.0, 1.0])) == -1 and f(w=_lib.host_doubles([1.0, 1.0, bad]), ard=1) == -1
            assert f(w=_lib.host_doubles([1.0, 1.0, bad]), ard=0) == 0                               # (one weight: only the first entry is read)
            assert f(family=1, offset=bad) == -1
        assert f(w=_lib.host_doubles([-1.0, 0.0, 1.0]), ard=1) == 0                                   # signs are not checked at the C ABI
        for deg in (0, 17, -3):
            assert f(family=1, degree=deg) == -1 and f(family=0, degree=deg) == 0                   # (Linear ignores the degree)
        assert [f(family=1, degree=deg) for deg in (1, 16)] == [0, 0]
    assert km(n1=-1) == -1 and km(n2=-1) == -1 and km(n1=5, n2=5, ldx1=2) == -1 and km(n1=5, n2=5, ldx2=2) == -1 and km(n1=5, n2=7, ldk=6) == -1
    assert km(n1=5, x2=False, ldk=4) == -1 and km(n1=-1, x2=False) == -1
    assert kc(n1=-1) == -1 and kc(n2=-1) == -1 and kc(n1=5, n2=7, ldg=6) == -1 and kc(n1=5, n2=7, ldo=6) == -1
    assert [kc(op=op) for op in (0, 4, -1)] == [-1] * 3 and [kc(op=op) for op in (1, 2, 3)] == [0] * 3
    assert kd(n=-1) == -1 and kd(n=5, ldx=2) == -1 and [kd(op=op) for op in (-1, 4)] == [-1, -1] and [kd(op=op) for op in range(4)] == [0] * 4
    for d in (0, -1, 65):
        assert tail(d=d) == -1
    assert tail(n1=-1) == -1 and tail(n1=5, ldr=3) == -1 and tail(n1=5, lda=2) == -1 and tail(n1=5, ldab=2) == -1
    assert tail(w=None) == -1 and tail(small=None) == -1
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r"#define GPK_DOT_(\w+) (\d+)", text)} == {"LINEAR": 0, "POLYNOMIAL": 1, "MAX_DEGREE": 16}
    assert not [m for m in re.finditer(r"#define GPK_KERN_(\w+) (\d+)", text) if int(m.group(2)) > 7]
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    dot = {"gpk_dot_kernel_matrix", "gpk_dot_kernel_matrix_combine", "gpk_dot_kernel_diag", "gpk_dot_adjoint_tail"}
    assert dot <= declared and declared == set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert lib.gpk_kernel_matrix(None, 8, addr, 0, 2, None, 0, 0, 2, _lib.host_doubles([1.0]), 0, 1.0, 0.0, 0, addr, 4) == -3
