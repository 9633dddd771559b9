"""CPU: the ArcCosine kernel (primitives, the class on every forward route, the reverse pass of GPR, VGP and SVGP, the trees) driven by
the test bodies of tests/test_gpu_arccosine.py with the device primitives replaced by their NumPy emulation -- tests/emulation.py's
modules and tests/fake_arccosine_ops.py, installed here -- as tests/test_vgp_emulated.py drives tests/test_gpu_vgp.py.  What this does
NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The CPU-only checks of the feature (the launch inventory
of gpflow_amd/csrc/arccosine, the exports, what the library answers before it touches a device, the conditioning of the model
problems, the launch list of the reverse pass) are at the end; they need no device.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import emulation
import fake_arccosine_ops
import fake_vgp_ops
import test_gpu_arccosine as T
import test_launch_geometry as G
from gpflow_amd.leaf import ArcLeaf  # noqa: F401  (the feature: without it nothing in this file can pass)

MODULES = emulation.MODULES + (fake_arccosine_ops, fake_vgp_ops)   # (fake_vgp_ops: the VGP case runs the triangular product)


@pytest.fixture
def gp(monkeypatch):
    import gpflow_amd
    from gpflow_amd import ops
    for name, fn in emulation.primitives(MODULES).items():
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, fn)
    return gpflow_amd


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
ARC_CSRC = os.path.join(G.CSRC, "arccosine")
# one row per launch site of gpflow_amd/csrc/arccosine/*.hip (tests/test_launch_geometry.py inventories csrc/*.hip and keeps its own table)
ARC_LAUNCHES = [
    # one 64 x 64 tile per workgroup; the adjoint instantiation finds its slots of `parts` from blockIdx and the tile counts in its arguments
    G.exact("arccosine.hip", "arccos_kernel<ORDER, MODE>", "dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));"),
    G.exact("arccosine.hip", "arccos_diag_kernel<0>", "const dim3 grid((unsigned)gpk_cdiv(n, T));"),
    G.exact("arccosine.hip", "arccos_diag_kernel<1>", "const dim3 grid((unsigned)gpk_cdiv(n, T));"),
    G.exact("arccosine.hip", "arccos_diag_kernel<2>", "const dim3 grid((unsigned)gpk_cdiv(n, T));"),
    G.exact("arccosine.hip", "arccos_adjoint_tail_kernel", "hipLaunchKernelGGL(arccos_adjoint_tail_kernel, dim3(1), dim3(AT_THREADS)"),   # one block, loops inside itself
]


def test_launch_inventory_of_the_arccosine_directory():
    """launch sites == rows, no kernel mentions gridDim, every quoted launch expression stands; a row taken out is seen"""
    sources = G._sources(ARC_CSRC)
    assert sorted(sources) == ["arccosine.hip"]
    assert G.problems(ARC_LAUNCHES, sources) == []
    for row in ARC_LAUNCHES:
        bad = G.problems([r for r in ARC_LAUNCHES if r is not row], sources)
        assert any("launch without a row" in b and row["kernel"] in b for b in bad), (row["kernel"], bad)
    assert {k for _, k in G.kernel_bodies(sources)} == {"arccos_kernel", "arccos_diag_kernel", "arccos_adjoint_tail_kernel"}
    assert "gridDim" not in sources["arccosine.hip"]
    assert G.problems(G.LAUNCHES, G._sources()) == []          # (the sub-directory is not part of that inventory)


def test_exports_header_leaf_and_class():
    import gpflow_amd as gpflow
    from gpflow_amd import _lib, leaf, ops
    from gpflow_amd.kernels.base import DeviceLeaf, is_arc_leaf, is_device_leaf, is_dot_leaf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    arc = {"gpk_arccos_kernel_matrix", "gpk_arccos_kernel_matrix_combine", "gpk_arccos_kernel_diag", "gpk_arccos_adjoint_stage",
           "gpk_arccos_adjoint_tail"}
    lib = _lib.load()
    assert arc <= declared and declared == set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert {n for n in declared if "arccos" in n} == arc                                     # only what the Python layer calls
    assert int(re.search(r"#define GPK_ARC_TILE (\d+)", text).group(1)) == ops.ARC_TILE == fake_arccosine_ops.TILE == 64
    readme = open(os.path.join(root, "README.md")).read()
    assert f"{len(declared)} functions" in readme
    new = set(emulation.primitives(emulation.MODULES + (fake_arccosine_ops,))) - set(emulation.primitives())
    assert new == {"arccos_kernel_matrix", "arccos_kernel_matrix_combine", "arccos_kernel_diag", "arccos_adjoint_parts",
                   "arccos_adjoint_stage", "arccos_adjoint_tail"} and new <= set(dir(ops))
    K = gpflow.kernels
    assert "ArcCosine" in K.__all__ and issubclass(K.ArcCosine, K.Kernel) and not issubclass(K.ArcCosine, DeviceLeaf)
    # neither a stationary family nor a dot-product one
    assert [f.name for f in leaf.DOT_FAMILIES] == ["Linear", "Polynomial"] and "ArcCosine" not in ops.KERNEL_FAMILIES
    assert not [m for m in re.finditer(r"#define GPK_DOT_(\w+) (\d+)", text) if m.group(1) not in ("LINEAR", "POLYNOMIAL", "MAX_DEGREE")]
    with pytest.raises(ValueError, match="not a dot-product family"):
        leaf.DotLeaf("ArcCosine", 1.0)
    k = K.ArcCosine(order=2, variance=0.8, weight_variances=[0.5, 2.0], bias_variance=0.3, active_dims=[2, 0], name="arc")
    assert k.name == "arc" and list(k.active_dims) == [2, 0] and k.ard and k.order == 2
    assert is_arc_leaf(k) and not is_dot_leaf(k) and not is_device_leaf(k) and not is_arc_leaf(K.Linear()) and not is_arc_leaf(K.White())
    assert list(k.trainable_parameters) == [k.variance, k.weight_variances, k.bias_variance] == list(k.leaf_params())
    lf = k.leaf()
    assert isinstance(lf, leaf.ArcLeaf) and lf.family == "ArcCosine" and lf.order == 2 and lf.variance == pytest.approx(0.8) \
        and list(lf.weight_variances) == [0.5, 2.0] and lf.bias_variance == pytest.approx(0.3) and lf.n_weights == 2 and lf.n_shape == 3
    assert lf.parameters == ("variance", "weight_variances", "bias_variance") and not lf.is_plain
    assert set(lf.keywords()) == {"order", "variance", "weight_variances", "bias_variance"}
    w, ard = lf.host(2)
    assert list(w) == [0.5, 2.0] and ard == 1
    with pytest.raises(ValueError, match="entries"):
        lf.host(3)
    with pytest.raises(AttributeError):
        lf.order = 1                                                                           # immutable
    rep = lf.replace([1.5, [1.0, 3.0], 0.7])
    assert rep.order == 2 and rep.variance == 1.5 and list(rep.weight_variances) == [1.0, 3.0] and rep.bias_variance == 0.7
    one = K.ArcCosine().leaf()
    assert one.order == 0 and one.n_weights == 1 and one.n_shape == 2 and one.host(5)[1] == 0 and not one.ard
    g = np.arange(3.0)
    sp = lf.split_shape(g)
    assert list(sp) == ["lengthscales", "weight_variances", "bias_variance"] and sp["lengthscales"].size == 0 \
        and list(sp["weight_variances"]) == [0.0, 1.0] and list(sp["bias_variance"]) == [2.0]
    for bad in (3, -1, 0.5, "0", None, True):
        with pytest.raises(ValueError):
            leaf.ArcLeaf(bad, 1.0)
    assert isinstance(K.SquaredExponential() + K.ArcCosine(), K.Sum) and isinstance(K.ArcCosine() * K.Polynomial(), K.Product)


def test_spec_bookkeeping_for_an_arccosine_member():
    """KernelSpec with an ArcLeaf member: the member class, never packable, no constant diagonal, one variance entry, names and layouts,
    and how CovarianceRoute cuts the gradients"""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd import gradients
    K = gpflow.kernels
    kern = K.SquaredExponential() * K.ArcCosine(1, weight_variances=[0.5, 1.0, 2.0]) + K.Linear(variance=[1.0, 2.0, 3.0])
    route = gpflow.models.reverse.CovarianceRoute(kern, 3)
    spec = route.spec
    assert spec.tree == ("add", [("mul", [0, 1]), 2]) and not spec.packable and not spec.constant_diagonal
    assert [type(p).__name__ for p in spec.parts] == ["StationaryMember", "ArcMember", "DotMember"] and not spec.is_dot(1)
    assert issubclass(gradients.ArcMember, gradients.Member) and gradients.ArcMember.constant_diagonal is False
    assert gradients.ArcMember.leaf_adjoint is gradients.arccos_kernel_adjoint
    assert [spec.n_variance(i) for i in range(3)] == [1, 1, 3] and [spec.n_shape(i) for i in range(3)] == [1, 4, 0]
    assert list(route._variance_cuts()) == [0, 1, 2, 5]
    grads = spec.kernel_grads(torch.arange(5.0), [torch.tensor([10.0]), torch.tensor([11.0, 12.0, 13.0, 14.0]), torch.zeros(0)])
    assert [None if v is None else list(v) for v in grads["weight_variances"]] == [None, [11.0, 12.0, 13.0], None]
    assert [None if v is None else list(v) for v in grads["bias_variance"]] == [None, [14.0], None]
    pairs = route.kernel_pairs(grads)
    arc = kern.kernels[0].kernels[1]
    assert [p for p, _ in pairs] == [kern.kernels[0].kernels[0].variance, kern.kernels[0].kernels[0].lengthscales, arc.variance,
                                     arc.weight_variances, arc.bias_variance, kern.kernels[1].variance]
    assert list(pairs[2][1]) == [1.0] and list(pairs[3][1]) == [11.0, 12.0, 13.0] and list(pairs[4][1]) == [14.0]
    single = gpflow.models.reverse.CovarianceRoute(K.ArcCosine(2), 3)
    assert single.spec.tree == 0 and not single.spec.packable and type(single.spec.parts[0]).__name__ == "ArcMember"


def test_library_answers_for_the_arccos_entry_points_before_the_device():
    """every GPK_E_ARG (-1) / GPK_E_UNSUPPORTED (-3) case of include/gpk.h with host pointers or NULL in the slots checked first, and 0
    without a launch where there is nothing to do"""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value
    one = _lib.host_doubles([1.0] * 64)

    def km(order=0, n1=0, n2=0, d=3, w=one, ard=0, v=1.0, b=0.5, ldx1=None, ldx2=None, ldk=None, x2=True, x1=addr, out=addr):
        return lib.gpk_arccos_kernel_matrix(None, order, x1, n1, d if ldx1 is None else ldx1, addr if x2 else None, n2, d if ldx2 is None else ldx2,
                                            d, w, ard, v, b, 0.0, 0, out, max(n2, n1, 1) if ldk is None else ldk)

    def kc(order=0, op=1, n1=0, n2=0, d=3, w=one, ard=0, v=1.0, b=0.5, ldg=None, ldo=None):
        return lib.gpk_arccos_kernel_matrix_combine(None, order, op, addr, n1, d, addr, n2, d, d, w, ard, v, b, 0.0, addr,
                                                    max(n2, 1) if ldg is None else ldg, addr, max(n2, 1) if ldo is None else ldo)

    def kd(order=0, op=0, n=0, d=3, w=one, ard=0, v=1.0, b=0.5, ldx=None):
        return lib.gpk_arccos_kernel_diag(None, order, op, addr, n, d if ldx is None else ldx, d, w, ard, v, b, addr, addr)

    def st(order=0, n1=0, n2=0, d=3, w=one, ard=0, v=1.0, b=0.5, ldkb=None, ldg=None, parts=addr):
        return lib.gpk_arccos_adjoint_stage(None, order, addr, n1, d, addr, n2, d, d, w, ard, v, b, addr, max(n2, 1) if ldkb is None else ldkb,
                                            addr, max(n2, 1) if ldg is None else ldg, parts)

    def tail(n1=0, n2=0, d=3, w=one, ard=0, ldr=None, lda=None, ldb=None, ldab=None, small=addr, B=addr):
        return lib.gpk_arccos_adjoint_tail(None, addr, 1 + d if ldr is None else ldr, addr, d if lda is None else lda, n1, B,
                                           d if ldb is None else ldb, n2, d, w, ard, addr, addr, small, addr, d if ldab is None else ldab)
    for f in (km, kc, kd, st):
        assert [f(order=o, d=d) for o in (0, 1, 2) for d in (1, 3, 64)] == [0] * 9, f.__name__       # nothing to do: 0, no launch
        assert f(ard=1, d=64) == 0
        for d in (0, -1, 65):
            assert f(d=d) == -1, (f.__name__, d)
        assert f(w=None) == -1
        for o in (-1, 3, 8):
            assert f(order=o) == -3, (f.__name__, o)
        for bad in (float("nan"), float("inf"), -float("inf"), -1.0):
            assert f(w=_lib.host_doubles([bad, 1.0, 1.0])) == -1 and f(w=_lib.host_doubles([1.0, 1.0, bad]), ard=1) == -1
            assert f(w=_lib.host_doubles([1.0, 1.0, bad]), ard=0) == 0                               # (one weight: only the first entry is read)
        assert f(w=_lib.host_doubles([0.0, 0.0, 0.0]), ard=1) == 0                                   # a zero weight is allowed
        for bad in (float("nan"), float("inf"), 0.0, -0.5):
            assert f(b=bad) == -1, (f.__name__, bad)
        for bad in (float("nan"), float("inf")):
            assert f(v=bad) == -1
        assert f(v=-1.0) == 0 and f(v=0.0) == 0                                                      # signs of v are not checked at the C ABI
    assert km(n1=-1) == -1 and km(n2=-1) == -1 and km(n1=5, n2=5, ldx1=2) == -1 and km(n1=5, n2=5, ldx2=2) == -1 and km(n1=5, n2=7, ldk=6) == -1
    assert km(n1=5, x2=False, ldk=4) == -1 and km(n1=-1, x2=False) == -1 and km(n1=5, n2=5, x1=None) == -1 and km(n1=5, n2=5, out=None) == -1
    assert kc(n1=-1) == -1 and kc(n2=-1) == -1 and kc(n1=5, n2=7, ldg=6) == -1 and kc(n1=5, n2=7, ldo=6) == -1
    assert [kc(op=op) for op in (0, 3, -1)] == [-1] * 3 and [kc(op=op) for op in (1, 2)] == [0] * 2
    assert kd(n=-1) == -1 and kd(n=5, ldx=2) == -1 and [kd(op=op) for op in (-1, 4)] == [-1, -1] and [kd(op=op) for op in range(4)] == [0] * 4
    assert st(n1=-1) == -1 and st(n2=-1) == -1 and st(n1=5, n2=7, ldkb=6) == -1 and st(n1=5, n2=7, ldg=6) == -1 and st(n1=5, n2=7, parts=None) == -1
    for d in (0, -1, 65):
        assert tail(d=d) == -1
    assert tail(w=None) == -1 and tail(w=_lib.host_doubles([-1.0])) == -1 and tail(small=None) == -1
    assert tail(n1=-1) == -1 and tail(n2=-1) == -1 and tail(n1=5, ldr=3) == -1 and tail(n1=5, lda=2) == -1 and tail(n1=5, ldb=2) == -1 \
        and tail(n1=5, ldab=2) == -1
    assert lib.gpk_dot_kernel_matrix(None, 2, addr, 0, 3, addr, 0, 3, 3, one, 0, 0.0, 1, 0.0, 0, addr, 1) == -3     # no third GPK_DOT_* code


def test_the_dot_product_builder_still_refuses_the_name(gp):
    import torch
    X = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises((AssertionError, ValueError)):
        gp.ops.dot_kernel_matrix(X, None, family="ArcCosine", variance=1.0)


def test_the_oracle_is_conditioned_for_every_model_problem():
    """the pre-check of tests/test_gpu_arccosine.py's docstring: the oracle's own gradients move by at most 1e-10 -- a hundred times
    below GRAD_TOL -- when every kernel entry and every entry of the row diagonal is perturbed by a relative 4 * 2^-52; the recorded
    figures are not below what is measured here"""
    figs = T.conditioning_figures()
    print({k: f"{v:.1e}" for k, v in figs.items()})
    assert set(figs) == set(T.CONDITIONING_FIGURES)
    for name, v in figs.items():
        assert v <= 1e-10, (name, v)
        assert v <= 1.05 * T.CONDITIONING_FIGURES[name], (name, v, "the figure recorded in the docstring is out of date")


def test_the_margin_of_every_primitive_case():
    """min(1 - |c|) >= 5e-4 over the off-diagonal elements of every build case, both weight forms, rectangular and symmetric"""
    worst = 1.0
    for (n1, n2, d) in T.BUILD_CASES:
        for ard in (False, True):
            worst = min(worst, T._ref_of(0, n1, n2, d, ard)["margin"], T._ref_of(0, n1, n1, d, ard, same=True)["margin"])
    print(f"smallest margin {worst:.2e}")
    assert worst >= T.MIN_MARGIN


def _logged_ops(monkeypatch):
    from gpflow_amd import gradients
    calls = []

    def logged(name, fn):
        def call(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return call
    monkeypatch.setattr(gradients, "ops", types.SimpleNamespace(**{n: logged(n, fn) for n, fn in emulation.primitives(MODULES).items()}))
    return gradients, calls


def test_gpr_lml_and_grad_with_one_arccosine_issues_a_fixed_list_of_primitive_calls(monkeypatch):
    """one build, one factorisation, and for the one covariance adjoint: one stage, one contraction (moment rows + the split-K product)
    and one tail -- no dot_* or stationary primitive"""
    import torch
    gradients, calls = _logged_ops(monkeypatch)
    from gpflow_amd.leaf import ArcLeaf
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    spec = gradients.KernelSpec([ArcLeaf(1, 0.8, [0.8, 1.4, 0.6], 0.7)])
    gradients.gpr_lml_and_grad(t(rng.uniform(-1, 1, size=(40, 3))), t(rng.normal(size=(40, 2))), noise_variance=0.15, kernel_spec=spec)
    arc = [c for c in calls if c.startswith("arccos_")]
    assert arc == ["arccos_kernel_matrix", "arccos_adjoint_parts", "arccos_adjoint_stage", "arccos_adjoint_tail"], calls
    assert calls.count("moment_rows") == 1 and calls.count("potrf_") == 1
    assert not [c for c in calls if c.startswith("dot_") or c in ("kernel_matrix", "kernel_matrix_combine", "kernel_matrix_hadamard",
                                                                   "stationary_adjoint_tail")]
    i = calls.index("arccos_adjoint_stage")
    assert calls[i + 1] == "moment_rows" and calls.index("arccos_adjoint_tail") > i + 1
    assert calls == FIXED_GPR_CALLS, calls


# build; factorisation; the value and K^-1 terms; then the ONE covariance adjoint: scratch, stage, contraction (its right-hand side and
# the product), tail
FIXED_GPR_CALLS = ["arccos_kernel_matrix", "potrf_", "row_stats", "gemm_nt", "gemm_nt", "gemm_nt", "arccos_adjoint_parts",
                   "arccos_adjoint_stage", "moment_rows", "gemm_nt", "arccos_adjoint_tail"]


def test_a_spec_without_an_arccosine_member_issues_the_calls_it_issued(monkeypatch):
    """SquaredExponential + Linear through svgp_elbo_and_grad: no arccos_* primitive appears, and the counts are those that
    tests/test_dot_kernels_emulated.py and tests/test_gradients_cpu.py pin for the members that were there"""
    import torch
    gradients, calls = _logged_ops(monkeypatch)
    from gpflow_amd.leaf import DotLeaf, Leaf
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    M, B, D, P = 16, 40, 3, 2
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), DotLeaf("Linear", 0.8)], "add")
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    gradients.svgp_elbo_and_grad(t(rng.normal(size=(M, D))), t(rng.normal(size=(B, D))), t(rng.normal(size=(B, P))),
                                 t(0.3 * rng.normal(size=(M, P))), t(q_sqrt), noise_variance=0.2, jitter=1e-6, kernel_spec=spec)
    assert not [c for c in calls if c.startswith("arccos_")]
    assert calls.count("kernel_matrix") == 2 and calls.count("dot_kernel_matrix_combine") == 2 and calls.count("stationary_adjoint_tail") == 2 \
        and calls.count("dot_adjoint_tail") == 2 and calls.count("dot_kernel_diag") == 1
