"""CPU: the ChangePoints kernel (primitives, the class, its node in KernelSpec, the reverse pass of GPR, VGP and SVGP) driven by the
test bodies of tests/test_gpu_changepoints.py with the device primitives replaced by their NumPy emulation -- tests/emulation.py's
modules and tests/fake_changepoints_ops.py, installed here -- as tests/test_arccosine_emulated.py drives tests/test_gpu_arccosine.py.
What this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The CPU-only checks of the feature (the
launch inventory of gpflow_amd/csrc/changepoints, the exports, what the library answers before it touches a device, the conditioning
of the model problems, the call lists of the reverse pass) are at the end; they need no device.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import emulation
import fake_changepoints_ops
import fake_vgp_ops
import test_gpu_changepoints as T
import test_launch_geometry as G
from gpflow_amd.gradients import ChangePointsNode  # noqa: F401  (the feature: without it nothing in this file can pass)

MODULES = emulation.MODULES + (fake_changepoints_ops, fake_vgp_ops)   # (fake_vgp_ops: the VGP case runs the triangular product)


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
CP_CSRC = os.path.join(G.CSRC, "changepoints")
# one row per launch site of gpflow_amd/csrc/changepoints/*.hip (tests/test_launch_geometry.py inventories csrc/*.hip and keeps its own table)
CHANGEPOINT_LAUNCHES = [
    G.exact("changepoints.hip", "changepoint_weights_kernel", "const dim3 grid((unsigned)gpk_cdiv(n, 256));"),          # one thread per row
    # one 64 x 64 tile per workgroup; the stage's instantiation finds its slots of `parts` from blockIdx and the tile count in its arguments
    G.exact("changepoints.hip", "changepoint_tile_kernel<MODE>", "dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));"),
    G.exact("changepoints.hip", "changepoint_tail_rows_kernel", "const dim3 grid((unsigned)gpk_cdiv(n, TAIL_THREADS));"),  # one thread per row; its slot of `red` from blockIdx
    G.exact("changepoints.hip", "changepoint_tail_sum_kernel", "hipLaunchKernelGGL(changepoint_tail_sum_kernel, dim3(1), dim3(64)"),   # one block, loops over the first launch's blocks
]


def test_launch_inventory_of_the_changepoints_directory():
    """launch sites == rows, no kernel mentions gridDim, every quoted launch expression stands; a row taken out is seen"""
    sources = G._sources(CP_CSRC)
    assert sorted(sources) == ["changepoints.hip"]
    assert G.problems(CHANGEPOINT_LAUNCHES, sources) == []
    for row in CHANGEPOINT_LAUNCHES:
        bad = G.problems([r for r in CHANGEPOINT_LAUNCHES if r is not row], sources)
        assert any("launch without a row" in b and row["kernel"] in b for b in bad), (row["kernel"], bad)
    assert {k for _, k in G.kernel_bodies(sources)} == {"changepoint_weights_kernel", "changepoint_tile_kernel", "changepoint_tail_rows_kernel",
                                                        "changepoint_tail_sum_kernel"}
    assert "gridDim" not in sources["changepoints.hip"] and "atomic" not in sources["changepoints.hip"]
    assert G.problems(G.LAUNCHES, G._sources()) == []          # (the sub-directory is not part of that inventory)
    assert "changepoints/changepoints.hip" in open(os.path.join(G.CSRC, "Makefile")).read()


def test_exports_header_and_class():
    import gpflow_amd as gpflow
    from gpflow_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    cp = {"gpk_changepoint_weights", "gpk_changepoint_fold", "gpk_changepoint_adjoint_stage", "gpk_changepoint_adjoint_tail"}
    lib = _lib.load()
    assert cp <= declared and declared == set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in declared)
    assert {n for n in declared if "changepoint" in n} == cp                                  # only what the Python layer calls
    assert int(re.search(r"#define GPK_CP_TILE (\d+)", text).group(1)) == ops.CP_TILE == fake_changepoints_ops.TILE == T.TILE == 64
    assert int(re.search(r"#define GPK_CP_MAX_MEMBERS (\d+)", text).group(1)) == ops.CP_MAX_MEMBERS == fake_changepoints_ops.MAX_MEMBERS == 16
    src = open(os.path.join(CP_CSRC, "changepoints.hip")).read()
    assert int(re.search(r"constexpr int TAIL_THREADS = (\d+);", src).group(1)) == ops.CP_TAIL_ROWS
    readme = open(os.path.join(root, "README.md")).read()
    assert f"{len(declared)} functions" in readme
    new = set(emulation.primitives(emulation.MODULES + (fake_changepoints_ops,))) - set(emulation.primitives())
    assert new == {"changepoint_weights", "changepoint_fold", "changepoint_adjoint_parts", "changepoint_adjoint_stage",
                   "changepoint_adjoint_tail"} and new <= set(dir(ops))
    K = gpflow.kernels
    assert "ChangePoints" in K.__all__ and issubclass(K.ChangePoints, K.Combination) and K.ChangePoints._op == "cp"
    assert K.Sum._op == "add" and K.Product._op == "mul"


def test_library_answers_for_the_changepoint_entry_points_before_the_device():
    """every GPK_E_ARG (-1) / GPK_E_UNSUPPORTED (-3) case of include/gpk.h with host pointers or NULL in the slots checked first, and 0
    without a launch where there is nothing to do"""
    from gpflow_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    addr = ctypes.cast(buf, ctypes.c_void_p).value
    hd = _lib.host_doubles
    loc2, st2 = hd([0.0, 0.5]), hd([1.0, 2.0])

    def w(n=0, ldx=1, C=2, loc=loc2, st=st2, lda=None, x=addr, A=addr):
        return lib.gpk_changepoint_weights(None, x, n, ldx, C, loc, st, A, max(n, 1) if lda is None else lda)

    def fold(op=0, n1=0, n2=0, b=addr, ldki=None, ldacc=None, ldo=None, a=addr, Ki=addr, acc=addr, out=addr):
        m2 = max(n2 if b else n1, 1)
        return lib.gpk_changepoint_fold(None, op, a, b, n1, n2, Ki, m2 if ldki is None else ldki, acc, m2 if ldacc is None else ldacc, 0.0,
                                        out, m2 if ldo is None else ldo)

    def stage(n1=0, n2=0, b=addr, ldkb=None, ldki=None, ldg=None, a=addr, Kbar=addr, Ki=addr, Gm=addr, parts=addr):
        m2 = max(n2 if b else n1, 1)
        return lib.gpk_changepoint_adjoint_stage(None, a, b, n1, n2, Kbar, m2 if ldkb is None else ldkb, Ki, m2 if ldki is None else ldki,
                                                 Gm, m2 if ldg is None else ldg, parts)

    def tail(n=0, ldx=1, C=2, loc=loc2, st=st2, parts=addr, stride=0, ntiles=0, init=None, ldinit=0, red=addr, small=addr, xbar=addr, x=addr):
        return lib.gpk_changepoint_adjoint_tail(None, x, n, ldx, C, loc, st, parts, stride, ntiles, init, ldinit, red, small, xbar)
    for f in (w, tail):
        assert f() == 0 and f(C=0, loc=None, st=None) == 0 and f(C=15, loc=hd(np.arange(15.0)), st=hd([1.0] * 15)) == 0   # nothing to do
        assert f(C=16, loc=hd(np.arange(16.0)), st=hd([1.0] * 16)) == -3 and f(C=40) == -3                                  # T = 17
        assert f(C=-1) == -1 and f(loc=None) == -1 and f(st=None) == -1
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert f(loc=hd([0.0, bad])) == -1 and f(st=hd([1.0, bad])) == -1, (f.__name__, bad)
        assert f(st=hd([1.0, 0.0])) == -1 and f(st=hd([-1.0, 1.0])) == -1 and f(loc=hd([0.5, 0.0])) == -1                   # positive; sorted
        assert f(loc=hd([0.5, 0.5])) == 0                                                                                   # ties are sorted
        assert f(n=-1) == -1 and f(n=5, ldx=0) == -1 and f(n=5, x=None) == -1
    assert w(n=5, lda=4) == -1 and w(n=5, A=None) == -1
    assert tail(n=5, ntiles=-1) == -1 and tail(n=5, ntiles=2, stride=9) == -1 and tail(n=5, init=addr, ldinit=4) == -1
    assert tail(n=5, ntiles=1, stride=5, parts=None) == -1 and tail(n=5, red=None) == -1 and tail(n=5, small=None) == -1 and tail(n=5, xbar=None) == -1
    assert tail(n=5, C=0, loc=None, st=None, red=None, small=None, xbar=None) == 0        # no change point: nothing is written
    for f in (fold, stage):
        assert f() == 0 and f(n1=5) == 0 and f(n2=5) == 0 and f(b=None) == 0
        assert f(n1=-1) == -1 and f(n2=-1) == -1 and f(n1=5, n2=7, ldki=6) == -1 and f(n1=5, b=None, ldki=4) == -1
        assert f(n1=5, n2=7, a=None) == -1 and f(n1=5, n2=7, Ki=None) == -1
    assert [fold(op=op) for op in (-1, 2)] == [-1, -1] and fold(op=1, n1=5, n2=7, ldacc=6) == -1
    assert fold(n1=5, n2=7, ldo=6) == -1 and fold(n1=5, n2=7, out=None) == -1 and fold(op=1, n1=5, n2=7, acc=None) == -1
    assert stage(n1=5, n2=7, ldkb=6) == -1 and stage(n1=5, n2=7, ldg=6) == -1 and stage(n1=5, n2=7, parts=None) == -1 \
        and stage(n1=5, n2=7, Kbar=None) == -1 and stage(n1=5, n2=7, Gm=None) == -1


def test_the_oracle_is_conditioned_for_every_model_problem():
    """the pre-check of tests/test_gpu_changepoints.py's docstring: the oracle's own gradients move by at most 1e-10 -- a hundred times
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
    monkeypatch.setattr(gradients, "ops", types.SimpleNamespace(CP_MAX_MEMBERS=16, **{n: logged(n, fn) for n, fn in emulation.primitives(MODULES).items()}))
    return gradients, calls


def test_gpr_lml_and_grad_with_a_changepoints_node_issues_a_fixed_list_of_changepoint_calls(monkeypatch):
    """three members: the weights once for the build; two folds after the first member's op 0; for the ONE covariance adjoint the
    weights again, one scratch, one stage per member, and one tail per argument"""
    import torch
    gradients, calls = _logged_ops(monkeypatch)
    from gpflow_amd.leaf import Leaf
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    leaves = [Leaf("SquaredExponential", 1.0, 0.5), Leaf("Matern32", 0.8, 0.7), Leaf("Matern52", 0.6, 0.9)]
    spec = gradients.KernelSpec(leaves, ("cp", [0, 1, 2], 0), nodes=[gradients.ChangePointsNode([0.4, -0.3], [3.0, 5.0])])
    _, grads, _ = gradients.gpr_lml_and_grad(t(rng.uniform(-1, 1, size=(40, 3))), t(rng.normal(size=(40, 2))), noise_variance=0.15, kernel_spec=spec)
    cp = [c for c in calls if c.startswith("changepoint_")]
    assert cp == ["changepoint_weights"] + ["changepoint_fold"] * 3 + ["changepoint_weights", "changepoint_adjoint_parts"] + \
        ["changepoint_adjoint_stage"] * 3 + ["changepoint_adjoint_tail"] * 2, cp
    assert calls.count("kernel_matrix") == 6 and calls.count("potrf_") == 1      # every member built once forward, once in the adjoint
    assert list(grads["changepoints"][0]) == ["locations", "steepness"] and grads["changepoints"][0]["locations"].shape == (2,)
    again = gradients.gpr_lml_and_grad(t(rng.uniform(-1, 1, size=(40, 3))), t(rng.normal(size=(40, 2))), noise_variance=0.15, kernel_spec=spec)[1]
    assert again["changepoints"][0]["locations"].shape == (2,)          # (a second evaluation starts from empty sums: `warm`)


def test_a_spec_without_a_changepoints_node_issues_the_calls_it_issued(monkeypatch):
    """a Sum of stationary kernels through svgp_elbo_and_grad: no changepoint_* primitive appears, the grads have no "changepoints"
    key, and the calls are those of the parent commit -- the list below was recorded there"""
    import torch
    gradients, calls = _logged_ops(monkeypatch)
    from gpflow_amd.leaf import Leaf
    rng = np.random.default_rng(0)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    M, B, D, P = 16, 40, 3, 2
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), Leaf("Matern32", 0.8, 0.7)], "add")
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    _, grads, _ = gradients.svgp_elbo_and_grad(t(rng.normal(size=(M, D))), t(rng.normal(size=(B, D))), t(rng.normal(size=(B, P))),
                                               t(0.3 * rng.normal(size=(M, P))), t(q_sqrt), noise_variance=0.2, jitter=1e-6, kernel_spec=spec)
    assert not [c for c in calls if c.startswith("changepoint_")] and "changepoints" not in grads
    assert calls == PARENT_SVGP_SUM_CALLS, calls


# svgp_elbo_and_grad of SquaredExponential + Matern32 (M = 16, B = 40, P = 2, full q_sqrt) as the parent commit issues it
PARENT_SVGP_SUM_CALLS = [
    "kernel_matrix", "kernel_matrix_combine", "kernel_matrix", "kernel_matrix_combine", "potrf_", "combine_parts", "combine_parts",
    "transpose", "row_stats", "gemm_nt", "row_stats", "row_stats", "gaussian_varexp_sum", "gauss_kl_white", "lowrank_axpy",
    "gemm_nt", "gemm_nt", "transpose", "gemm_nt", "transpose", "transpose", "gemm_nt", "combine_parts", "transpose", "gemm_nt",
    "combine_parts", "gemm_nt", "transpose", "gemm_nt", "symmetrize_", "kernel_matrix_hadamard", "moment_rows", "gemm_nt",
    "stationary_adjoint_tail", "kernel_matrix_hadamard", "kernel_matrix_combine", "moment_rows", "gemm_nt",
    "stationary_adjoint_tail", "kernel_matrix_hadamard", "moment_rows", "gemm_nt", "stationary_adjoint_tail",
    "kernel_matrix_hadamard", "kernel_matrix_combine", "moment_rows", "gemm_nt", "stationary_adjoint_tail", "row_stats",
    "transpose", "transpose", "gemm_nt", "combine_parts", "gemm_nt", "combine_parts",
]
