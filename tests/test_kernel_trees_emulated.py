"""CPU: kernel trees of mixed leaf kinds (every ordered pair of kinds in a Sum and a Product, nested trees on every model route)
driven by the test bodies of tests/test_gpu_kernel_trees.py with the device primitives replaced by their NumPy emulation
(tests/emulation.py: every tests/fake_*.py) -- as tests/test_dot_kernels_emulated.py drives tests/test_gpu_dot_kernels.py.  What this does NOT test is the HIP kernels: that
is what the same bodies do under `-m gpu`.  The CPU-only checks are at the end: the guard that holds `KINDS` to the leaf tables, the
conditioning of the oracle for every model tree, the bookkeeping of one three-level tree and the launch list of a constant-diagonal
mixed tree; they need no device.
"""
import types

import numpy as np
import pytest

import emulation
import test_gpu_kernel_trees as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def test_every_kind_of_leaf_has_a_row_of_KINDS():
    """every family of leaf.FAMILIES, every one of leaf.DOT_FAMILIES and every input-map DeviceLeaf exported by gpflow_amd.kernels
    occurs in KINDS: a new kind of leaf fails here until it is crossed with the others"""
    import gpflow_amd as gpflow
    from gpflow_amd import leaf
    from gpflow_amd.kernels.base import DeviceLeaf

    def missing(kinds):
        rows = list(kinds.values())
        device = {k.family for k in rows if k.cls in ("stationary", "static")}
        dot = {k.family for k in rows if k.cls == "dot"}
        mapped = {(k.class_name, k.family) for k in rows if k.cls == "periodic"}
        return ({f.name for f in leaf.FAMILIES} - device) | ({f.name for f in leaf.DOT_FAMILIES} - dot) | (maps - mapped)

    def takes(cls, family):
        try:
            cls(getattr(gpflow.kernels, family)())
        except NotImplementedError:
            return False
        return True
    # an input-map kernel counts once per base family it accepts: the base decides which builder profile the warped inputs meet
    maps = {(n, f.name) for n in gpflow.kernels.__all__ for f in leaf.FAMILIES if isinstance(getattr(gpflow.kernels, n), type)
            and issubclass(getattr(gpflow.kernels, n), DeviceLeaf) and getattr(gpflow.kernels, n).maps_inputs
            and takes(getattr(gpflow.kernels, n), f.name)}
    assert maps == {("Periodic", "SquaredExponential"), ("Periodic", "RationalQuadratic")}
    assert not missing(T.KINDS)
    for name in T.KINDS:                                         # (the guard does fail when a row goes)
        assert missing({k: v for k, v in T.KINDS.items() if k != name}), name
    # every row builds the class it names, and the model trees use every kind
    for name, kind in T.KINDS.items():
        k, pars = kind.make(gpflow.kernels)
        assert type(k).__name__ == kind.class_name and tuple(pars) == kind.names and list(k.trainable_parameters) == list(pars.values()), name
    used = {(k.cls, k.family) for _, kinds, _ in T.TREES.values() for k in kinds.values()}
    assert {("stationary", "SquaredExponential"), ("stationary", "Matern32"), ("stationary", "Exponential"), ("stationary", "RationalQuadratic"),
            ("static", "White"), ("static", "Constant"), ("periodic", "SquaredExponential"), ("periodic", "RationalQuadratic"),
            ("dot", "Linear"), ("dot", "Polynomial")} <= used
    assert len(T.TREES) == 9 and len(T.ROW_TREES) == 7 and len(T.HET_TREES) == 2


@pytest.mark.parametrize("name", list(T.TREES))
def test_the_oracle_is_conditioned_for_every_tree(name):
    """the pre-check of tests/test_gpu_kernel_trees.py's docstring: the oracle's own values and gradients move by at most 1 / 100 of
    the tolerance when every kernel entry and every entry of the row diagonal is perturbed by a relative 4 * 2^-52"""
    vtol, gtol = T._tols(name)
    dv, dg = T.conditioning_figures(name)
    print(f"conditioning {name}: value {dv:.1e} gradient {dg:.1e}")
    assert dv <= vtol / 100 and dg <= gtol / 100, (name, dv, dg)


def test_bookkeeping_of_a_three_level_tree():
    """(Linear(ARD) + Periodic(SE, ARD period)) * (Polynomial(2) + White) + RationalQuadratic(active_dims=[0, 2]) as
    gradient_spec, KernelSpec and CovarianceRoute cut it"""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd.models import reverse
    K = gpflow.kernels
    lin = K.Linear(variance=[0.5, 2.0, 1.25])
    pse = K.SquaredExponential(variance=1.3, lengthscales=[0.6, 0.9, 1.3])
    per = K.Periodic(pse, period=[2.5, 3.0, 3.5])
    pol, wh = K.Polynomial(2, variance=0.7, offset=0.3), K.White(variance=0.3)
    rq = K.RationalQuadratic(variance=0.6, lengthscales=0.5, alpha=0.7, active_dims=[0, 2])
    kern = (lin + per) * (pol + wh) + rq
    route = reverse.CovarianceRoute(kern, 3)
    spec = route.spec
    assert spec.tree == ("add", [("mul", [("add", [0, 1]), ("add", [2, 3])]), 4])
    assert not spec.constant_diagonal and not spec.packable and [spec.is_dot(i) for i in range(5)] == [True, False, True, False, False]
    assert [spec.parameter_names(i) for i in range(5)] == [("variance",), ("variance", "lengthscales", "period"), ("variance", "offset"),
                                                           ("variance",), ("variance", "lengthscales", "alpha")]
    assert [spec.n_shape(i) for i in range(5)] == [0, 6, 1, 0, 2] and [spec.n_variance(i) for i in range(5)] == [3, 1, 1, 1, 1]
    assert [None if c is None else list(c) for c in spec.cols] == [None, None, None, None, [0, 2]]
    assert [p is not None for p in spec.periods] == [False, True, False, False, False]
    assert list(spec.members[1].lengthscales) == [1.2, 1.2, 1.8, 1.8, 2.6, 2.6]                 # the device form: 2 l, pairwise
    assert list(route._variance_cuts()) == [0, 3, 4, 5, 6, 7]
    assert [len(m) for m in route.members] == [1, 3, 2, 1, 3]
    shapes = [torch.zeros(0), torch.arange(10.0, 16.0), torch.tensor([20.0]), torch.zeros(0), torch.tensor([30.0, 31.0])]
    grads = spec.kernel_grads(torch.arange(7.0), shapes)
    assert list(grads) == ["variance", "lengthscales", "period", "offset", "alpha"]
    assert [None if v is None else list(v) for v in grads["period"]] == [None, [13.0, 14.0, 15.0], None, None, None]
    assert [None if v is None else list(v) for v in grads["offset"]] == [None, None, [20.0], None, None]
    assert [None if v is None else list(v) for v in grads["alpha"]] == [None, None, None, None, [31.0]]
    cut = route.member_grads(grads)
    assert [[list(x) for x in c] for c in cut] == [[[0.0, 1.0, 2.0]], [[3.0], [10.0, 11.0, 12.0], [13.0, 14.0, 15.0]], [[4.0], [20.0]], [[5.0]],
                                                   [[6.0], [30.0], [31.0]]]
    pairs = route.kernel_pairs(grads)
    order = [lin.variance, pse.variance, pse.lengthscales, per.period, pol.variance, pol.offset, wh.variance, rq.variance, rq.lengthscales,
             rq.alpha]
    assert [p for p, _ in pairs] == order and list(pairs[0][1]) == [0.0, 1.0, 2.0] and list(pairs[3][1]) == [13.0, 14.0, 15.0]
    assert list(reverse.to_unconstrained(pairs)) == order
    # one instance used twice: two members, one Parameter, which collects the sum
    twice = reverse.CovarianceRoute(lin + lin * K.SquaredExponential(), 3)
    assert twice.spec.tree == ("add", [0, ("mul", [1, 2])]) and twice.members[0] == twice.members[1] == (lin.variance,)
    g2 = twice.spec.kernel_grads(torch.arange(7.0), [torch.zeros(0), torch.zeros(0), torch.tensor([9.0])])
    un = reverse.to_unconstrained(twice.kernel_pairs(g2))
    fg = lin.variance.transform.forward_grad(lin.variance.unconstrained_variable)
    assert len(un) == 3 and np.allclose(un[lin.variance], np.array([0.0 + 3.0, 1.0 + 4.0, 2.0 + 5.0]) * fg, rtol=1e-15)


def test_a_constant_diagonal_mixed_tree_issues_no_row_diagonal_call(monkeypatch):
    """Periodic(RQ) * Matern32 + Constant * White through svgp_elbo_and_grad: no dot_* primitive and no kdiag_rows / diag_adjoint --
    the launch list of a spec with one scalar for a diagonal, member by member (the style of
    test_dot_kernels_emulated.py::test_a_constant_diagonal_spec_issues_the_calls_it_issued)"""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd import gradients
    from gpflow_amd.models import reverse
    calls = []

    def logged(name, fn):
        def call(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return call
    proxy = types.SimpleNamespace(**{n: logged(n, fn) for n, fn in emulation.primitives().items()})
    monkeypatch.setattr(gradients, "ops", proxy)
    for meth in ("kdiag_rows", "diag_adjoint"):
        monkeypatch.setattr(gradients.KernelSpec, meth, logged(meth, getattr(gradients.KernelSpec, meth)))
    kern = T._model_tree(gpflow.kernels, "per(rq)*m32+const*white")[0]
    spec = reverse.CovarianceRoute(kern, 3).spec
    assert spec.constant_diagonal and spec.tree == ("add", [("mul", [0, 1]), ("mul", [2, 3])])
    X, Y, Z, q_mu, q_sqrt = T._problem()
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    gradients.svgp_elbo_and_grad(t(Z), t(X), t(Y), t(q_mu), t(q_sqrt), noise_variance=0.2, jitter=1e-6, kernel_spec=spec)
    assert not [c for c in calls if c.startswith("dot_") or c in ("kdiag_rows", "diag_adjoint")]
    count = {n: calls.count(n) for n in ("kernel_matrix", "kernel_matrix_combine", "kernel_matrix_hadamard", "periodic_warp",
                                         "periodic_moment_rows", "periodic_adjoint_tail", "stationary_adjoint_tail", "gaussian_varexp_sum")}
    # Kuu and Kuf: the first leaf of each Product built (2 + a nested one each: 4), the other three members folded or multiplied in.
    # The adjoints (of Kuu and of Kuf): the two members with a distance go through hadamard / dr2 / dalpha and one tail each; the
    # periodic one warps and adds its own tail; Constant and White read their sums off Kbar.
    # kernel_matrix_combine, per matrix: 2 folds of the build; in the adjoint each of the four members has its sibling folded into its
    # Kb (4), Periodic(RQ) takes dalpha and dr2 (2), Matern32 dr2 (1): 2 x (2 + 7).  periodic_warp: Kuu 1, Kuf 2; the adjoint of Kuu 1 for
    # the fold into Matern32's Kb and 1 for the member's own, of Kuf 2 and 2.
    assert count == {"kernel_matrix": 4, "kernel_matrix_combine": 18, "kernel_matrix_hadamard": 4, "periodic_warp": 9, "periodic_moment_rows": 2,
                     "periodic_adjoint_tail": 2, "stationary_adjoint_tail": 4, "gaussian_varexp_sum": 1}, sorted(count.items())
