"""CPU: the Coregion kernel (primitives, the class on every forward route, the reverse pass of GPR, VGP and SVGP, the trees) driven by
the test bodies of tests/test_gpu_coregion.py with the device primitives replaced by their NumPy emulation -- tests/emulation.py's
modules and tests/fake_coregion_ops.py, installed here -- as tests/test_arccosine_emulated.py drives tests/test_gpu_arccosine.py.  What
this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The CPU-only checks of the feature (the launch
inventory of gpflow_amd/csrc/coregion, the exports, what the library answers before it touches a device, the conditioning of the model
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
import fake_coregion_ops
import fake_vgp_ops
import test_gpu_coregion as T
import test_launch_geometry as G
from gpflow_amd.leaf import CoregionLeaf  # noqa: F401  (the feature: without it nothing in this file can pass)

# (fake_vgp_ops: the VGP case runs the triangular product; fake_arccosine_ops: the crosses with an ArcCosine leaf)
MODULES = emulation.MODULES + (fake_coregion_ops, fake_vgp_ops, fake_arccosine_ops)


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
CO_CSRC = os.path.join(G.CSRC, "coregion")
# one row per launch site of gpflow_amd/csrc/coregion/*.hip (tests/test_launch_geometry.py inventories csrc/*.hip and keeps its own table)
COREGION_LAUNCHES = [
    # one 64 x 64 tile per workgroup
    G.exact("coregion.hip", "coregion_kernel<MODE>", "dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));"),
    G.exact("coregion.hip", "coregion_diag_kernel", "const dim3 grid((unsigned)gpk_cdiv(n, 256));"),                         # one thread per row
    G.exact("coregion.hip", "coregion_onehot_kernel", "const dim3 grid((unsigned)gpk_cdiv(n, 256), (unsigned)P);"),          # one thread per (label, row)
    G.exact("coregion.hip", "coregion_cov_kernel", "hipLaunchKernelGGL(coregion_cov_kernel, dim3(1), dim3(256)"),           # one block, loops inside itself
    G.exact("coregion.hip", "coregion_adjoint_tail_kernel", "hipLaunchKernelGGL(coregion_adjoint_tail_kernel, dim3(1), dim3(256)"),   # likewise
]


def test_launch_inventory_of_the_coregion_directory():
    """launch sites == rows, no kernel mentions gridDim, every quoted launch expression stands; a row taken out is seen"""
    sources = G._sources(CO_CSRC)
    assert sorted(sources) == ["coregion.hip"]
    assert G.problems(COREGION_LAUNCHES, sources) == []
    for row in COREGION_LAUNCHES:
        bad = G.problems([r for r in COREGION_LAUNCHES if r is not row], sources)
        assert any("launch without a row" in b and row["kernel"] in b for b in bad), (row["kernel"], bad)
    assert {k for _, k in G.kernel_bodies(sources)} == {"coregion_kernel", "coregion_diag_kernel", "coregion_onehot_kernel",
                                                        "coregion_cov_kernel", "coregion_adjoint_tail_kernel"}
    assert "gridDim" not in sources["coregion.hip"] and "atomic" not in sources["coregion.hip"].replace("No atomics", "").replace("no atomics", "")
    assert "getenv" not in sources["coregion.hip"]
    assert G.problems(G.LAUNCHES, G._sources()) == []          # (the sub-directory is not part of that inventory)


def test_exports_header_leaf_and_class():
    import gpflow_amd as gpflow
    from gpflow_amd import _lib, leaf, ops
    from gpflow_amd.kernels.base import DeviceLeaf, is_arc_leaf, is_coregion_leaf, is_device_leaf, is_dot_leaf
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    co = {"gpk_coregion_output_covariance", "gpk_coregion_kernel_matrix", "gpk_coregion_kernel_matrix_combine", "gpk_coregion_kernel_diag",
          "gpk_coregion_onehot_rows", "gpk_coregion_adjoint_tail"}
    lib = _lib.load()
    assert co <= declared and declared == set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert {n for n in declared if "coregion" in n} == co                                    # only what the Python layer calls
    assert int(re.search(r"#define GPK_COREGION_MAX_OUTPUTS (\d+)", text).group(1)) == ops.COREGION_MAX_OUTPUTS == leaf.COREGION_MAX_OUTPUTS \
        == fake_coregion_ops.MAX_OUTPUTS == 64
    assert int(re.search(r"#define GPK_COREGION_MAX_RANK (\d+)", text).group(1)) == ops.COREGION_MAX_RANK == leaf.COREGION_MAX_RANK \
        == fake_coregion_ops.MAX_RANK == 64
    assert "a NaN in row i of X1 makes row i of K NaN and nothing else" in " ".join(text.split()).replace(" * ", " ")
    readme = open(os.path.join(root, "README.md")).read()
    assert f"{len(declared)} functions" in readme
    new = set(emulation.primitives(emulation.MODULES + (fake_coregion_ops,))) - set(emulation.primitives())
    assert new == {"coregion_output_covariance", "coregion_kernel_matrix", "coregion_kernel_matrix_combine", "coregion_kernel_diag",
                   "coregion_onehot_rows", "coregion_adjoint_tail"} and new <= set(dir(ops))
    K = gpflow.kernels
    assert "Coregion" in K.__all__ and issubclass(K.Coregion, K.Kernel) and not issubclass(K.Coregion, DeviceLeaf)
    # no new family code of either table
    assert [f.name for f in leaf.DOT_FAMILIES] == ["Linear", "Polynomial"] and "Coregion" not in ops.KERNEL_FAMILIES
    assert sorted(ops.KERNEL_FAMILIES.values()) == list(range(8))
    k = K.Coregion(3, 2, active_dims=[4], name="icm")
    assert k.name == "icm" and list(k.active_dims) == [4] and k.output_dim == 3 and k.rank == 2
    assert is_coregion_leaf(k) and not is_arc_leaf(k) and not is_dot_leaf(k) and not is_device_leaf(k)
    assert list(k.trainable_parameters) == [k.W, k.kappa] and k.leaf_params() == (k.kappa, k.W)        # the reference's order; the gradients'
    assert k.W.numpy().shape == (3, 2) and np.all(k.W.numpy() == 0.1) and np.all(k.kappa.numpy() == 1.0)
    lf = k.leaf()
    assert isinstance(lf, leaf.CoregionLeaf) and lf.family == "Coregion" and lf.n_outputs == 3 and lf.rank == 2 and lf.n_shape == 6 \
        and lf.n_variance == 3 and not lf.is_plain and lf.parameters == ("kappa", "W") and set(lf.keywords()) == {"W", "kappa"}
    with pytest.raises(AttributeError):
        lf.W = 1.0                                                                              # immutable
    with pytest.raises(ValueError):
        lf.W[0, 0] = 1.0
    rep = lf.replace([np.array([1.0, 2.0, 3.0]), np.arange(6.0).reshape(3, 2)])
    assert list(rep.kappa) == [1.0, 2.0, 3.0] and rep.W[2, 1] == 5.0 and leaf.CoregionLeaf.of([rep.kappa, rep.W]).rank == 2
    g = np.arange(6.0)
    sp = lf.split_shape(g)
    assert list(sp) == ["lengthscales", "W"] and sp["lengthscales"].size == 0 and list(sp["W"]) == list(g)
    for W, kappa in ((np.ones((65, 1)), np.ones(65)), (np.ones((2, 65)), np.ones(2)), (np.ones((2, 2)), np.ones(3)), (np.ones(2), np.ones(2)),
                     (np.ones((0, 1)), np.ones(0))):
        with pytest.raises(ValueError):
            leaf.CoregionLeaf(W, kappa)
    assert isinstance(K.SquaredExponential() * K.Coregion(2, 1), K.Product)


def test_spec_bookkeeping_for_a_coregion_member():
    """KernelSpec with a CoregionLeaf member: the member class, never packable, no constant diagonal, P variance entries, names and
    layouts, and how CovarianceRoute cuts the gradients"""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd import gradients
    K = gpflow.kernels
    kern = K.SquaredExponential(active_dims=[0, 1]) * K.Coregion(3, 2, active_dims=[2]) + K.Linear(variance=[1.0, 2.0, 3.0])
    route = gpflow.models.reverse.CovarianceRoute(kern, 3)
    spec = route.spec
    assert spec.tree == ("add", [("mul", [0, 1]), 2]) and not spec.packable and not spec.constant_diagonal
    assert [type(p).__name__ for p in spec.parts] == ["StationaryMember", "CoregionMember", "DotMember"] and not spec.is_dot(1)
    assert issubclass(gradients.CoregionMember, gradients.Member) and gradients.CoregionMember.constant_diagonal is False
    assert gradients.CoregionMember.leaf_adjoint is gradients.coregion_kernel_adjoint
    assert [spec.n_variance(i) for i in range(3)] == [1, 3, 3] and [spec.n_shape(i) for i in range(3)] == [1, 6, 0]
    assert list(route._variance_cuts()) == [0, 1, 4, 7]
    assert list(spec.cols[1]) == [2] and spec.parameter_names(1) == ("kappa", "W")
    grads = spec.kernel_grads(torch.arange(7.0), [torch.tensor([10.0]), torch.arange(11.0, 17.0), torch.zeros(0)])
    assert [None if v is None else list(v) for v in grads["W"]] == [None, [11.0, 12.0, 13.0, 14.0, 15.0, 16.0], None]
    pairs = route.kernel_pairs(grads)
    se, co = kern.kernels[0].kernels
    assert [p for p, _ in pairs] == [se.variance, se.lengthscales, co.kappa, co.W, kern.kernels[1].variance]
    assert list(pairs[2][1]) == [1.0, 2.0, 3.0] and list(pairs[3][1]) == [11.0, 12.0, 13.0, 14.0, 15.0, 16.0] and list(pairs[4][1]) == [4.0, 5.0, 6.0]
    un = gpflow.models.reverse.to_unconstrained(pairs)
    assert un[co.W].shape == (3, 2) and un[co.kappa].shape == (3,)
    single = gpflow.models.reverse.CovarianceRoute(K.Coregion(2, 1, active_dims=[1]), 2)
    assert single.spec.tree == 0 and not single.spec.packable and type(single.spec.parts[0]).__name__ == "CoregionMember"


def test_library_answers_for_the_coregion_entry_points_before_the_device():
    """every GPK_E_ARG (-1) case of include/gpk.h with host pointers or NULL in the slots checked first, and 0 without a launch where
    there is nothing to do"""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 8192)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value

    def cov(P=3, R=2, ldw=None, ldb=None, W=addr, kappa=addr, B=addr):
        return lib.gpk_coregion_output_covariance(None, W, R if ldw is None else ldw, kappa, P, R, B, P if ldb is None else ldb)

    def km(P=3, n1=0, n2=0, ldx1=1, ldx2=1, ldb=None, ldk=None, x2=True, x1=addr, out=addr, B=addr):
        return lib.gpk_coregion_kernel_matrix(None, x1, n1, ldx1, addr if x2 else None, n2, ldx2, B, P if ldb is None else ldb, P, 0.0, 0, out,
                                              max(n2, n1, 1) if ldk is None else ldk)

    def kc(P=3, op=1, n1=0, n2=0, ldx1=1, ldx2=1, ldb=None, ldg=None, ldo=None, B=addr, G_=addr, out=addr):
        return lib.gpk_coregion_kernel_matrix_combine(None, op, addr, n1, ldx1, addr, n2, ldx2, B, P if ldb is None else ldb, P, 0.0, G_,
                                                      max(n2, 1) if ldg is None else ldg, out, max(n2, 1) if ldo is None else ldo)

    def kd(P=3, op=0, n=0, ldx=1, ldb=None, B=addr, g=addr, out=addr, X=addr):
        return lib.gpk_coregion_kernel_diag(None, op, X, n, ldx, B, P if ldb is None else ldb, P, g, out)

    def hot(P=3, n=0, ldx=1, lde=None, X=addr, E=addr):
        return lib.gpk_coregion_onehot_rows(None, X, n, ldx, P, E, max(n, 1) if lde is None else lde)

    def tail(P=3, R=2, ldbb=None, ldw=None, lddw=None, Bbar=addr, W=addr, dW=addr, dk=addr):
        return lib.gpk_coregion_adjoint_tail(None, Bbar, P if ldbb is None else ldbb, W, R if ldw is None else ldw, P, R, dW,
                                             R if lddw is None else lddw, dk)
    for f in (km, kc, kd, hot):
        assert [f(P=P) for P in (1, 3, 64)] == [0] * 3, f.__name__                                      # nothing to do: 0, no launch
        for P in (0, -1, 65):
            assert f(P=P) == -1, (f.__name__, P)
    for f in (cov, tail):
        for P, R in ((0, 1), (-1, 1), (65, 1), (3, 0), (3, -2), (3, 65)):
            assert f(P=P, R=R) == -1, (f.__name__, P, R)
    assert cov(ldw=1) == -1 and cov(ldb=2) == -1 and cov(W=None) == -1 and cov(kappa=None) == -1 and cov(B=None) == -1
    assert km(n1=-1) == -1 and km(n2=-1) == -1 and km(n1=5, n2=5, ldx1=0) == -1 and km(n1=5, n2=5, ldx2=0) == -1 and km(n1=5, n2=7, ldk=6) == -1
    assert km(ldb=2) == -1 and km(n1=5, x2=False, ldk=4) == -1 and km(n1=-1, x2=False) == -1 and km(n1=5, n2=5, x1=None) == -1 \
        and km(n1=5, n2=5, out=None) == -1 and km(n1=5, n2=5, B=None) == -1
    assert kc(n1=-1) == -1 and kc(n2=-1) == -1 and kc(n1=5, n2=7, ldg=6) == -1 and kc(n1=5, n2=7, ldo=6) == -1 and kc(ldb=2) == -1 \
        and kc(n1=5, n2=5, ldx1=0) == -1 and kc(n1=5, n2=5, B=None) == -1 and kc(n1=5, n2=5, G_=None) == -1 and kc(n1=5, n2=5, out=None) == -1
    assert [kc(op=op) for op in (0, 3, -1)] == [-1] * 3 and [kc(op=op) for op in (1, 2)] == [0] * 2
    assert kd(n=-1) == -1 and kd(n=5, ldx=0) == -1 and kd(ldb=2) == -1 and [kd(op=op) for op in (-1, 3)] == [-1, -1] \
        and [kd(op=op) for op in range(3)] == [0] * 3
    assert kd(n=5, B=None) == -1 and kd(n=5, out=None) == -1 and kd(n=5, X=None) == -1 and kd(n=5, op=1, g=None) == -1
    assert hot(n=-1) == -1 and hot(n=5, ldx=0) == -1 and hot(n=5, lde=4) == -1 and hot(n=5, X=None) == -1 and hot(n=5, E=None) == -1
    assert tail(ldbb=2) == -1 and tail(ldw=1) == -1 and tail(lddw=1) == -1 and tail(Bbar=None) == -1 and tail(W=None) == -1 \
        and tail(dW=None) == -1 and tail(dk=None) == -1
    assert not any(buf), "a refused call wrote"


def test_the_oracle_is_conditioned_for_every_model_problem():
    """the pre-check of tests/test_gpu_coregion.py's docstring: the oracle's own gradients move by at most 1e-10 -- a hundred times
    below GRAD_TOL -- when every kernel entry and every entry of the row diagonal is perturbed by a relative 4 * 2^-52; the recorded
    figures are not below what is measured here"""
    figs = T.conditioning_figures()
    print({k: f"{v:.1e}" for k, v in figs.items()})
    assert set(figs) == set(T.CONDITIONING_FIGURES)
    for name, v in figs.items():
        assert v <= 1e-10, (name, v)
        assert v <= 1.05 * T.CONDITIONING_FIGURES[name], (name, v, "the figure recorded in the docstring is out of date")


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


def test_gpr_lml_and_grad_with_one_coregion_leaf_issues_a_fixed_list_of_primitive_calls(monkeypatch):
    """one build, one factorisation, and for the one covariance adjoint: the one-hot rows, ONE pass over Kbar, the thin contraction and
    the tail -- no dot_*, arccos_* or stationary primitive"""
    import torch
    gradients, calls = _logged_ops(monkeypatch)
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    spec = gradients.KernelSpec([CoregionLeaf(0.1 + 0.5 * rng.normal(size=(3, 2)), [0.7, 1.0, 1.3])])
    X = rng.integers(0, 3, size=(40, 1)).astype(np.float64)
    gradients.gpr_lml_and_grad(t(X), t(rng.normal(size=(40, 2))), noise_variance=0.15, kernel_spec=spec)
    co = [c for c in calls if c.startswith("coregion_")]
    assert co == ["coregion_kernel_matrix", "coregion_onehot_rows", "coregion_adjoint_tail"], calls
    assert calls.count("potrf_") == 1 and calls.count("moment_rows") == 0
    assert not [c for c in calls if c.startswith("dot_") or c.startswith("arccos_") or c in ("kernel_matrix", "kernel_matrix_combine",
                                                                                             "kernel_matrix_hadamard", "stationary_adjoint_tail")]
    assert calls == FIXED_GPR_CALLS, calls


# build; factorisation; the value and K^-1 terms; then the ONE covariance adjoint: the one-hot rows, the pass over Kbar, its small
# transpose and the thin contraction to Bbar, the tail
FIXED_GPR_CALLS = ["coregion_kernel_matrix", "potrf_", "row_stats", "gemm_nt", "gemm_nt", "gemm_nt", "coregion_onehot_rows", "gemm_nt",
                   "transpose", "gemm_nt", "coregion_adjoint_tail"]


def test_a_spec_without_a_coregion_member_issues_the_calls_it_issued(monkeypatch):
    """SquaredExponential + Linear through svgp_elbo_and_grad: no coregion_* primitive appears, and the counts are those that
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
    assert not [c for c in calls if c.startswith("coregion_")]
    assert calls.count("kernel_matrix") == 2 and calls.count("dot_kernel_matrix_combine") == 2 and calls.count("stationary_adjoint_tail") == 2 \
        and calls.count("dot_adjoint_tail") == 2 and calls.count("dot_kernel_diag") == 1
