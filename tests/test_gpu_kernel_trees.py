"""GPU tests of kernel TREES: every kind of kernel leaf crossed with every other in a Sum and in a Product, and nested trees of mixed
kinds on every model route.  The leaves have their own files (test_gpu_contract.py, test_gpu_kernel_families.py, test_gpu_periodic.py,
test_gpu_dot_kernels.py); what is tested here is where their branches meet in the walkers -- `Combination.K_into` / `K_diag`,
`KernelSpec._build`, `_fold`, `_kd_rows`, `_adjoint`, `_diag_adjoint`, `kernels.base.gradient_spec`, `CovarianceRoute` and the predict
routes -- and, on the device, launches from rbf.hip, dot.hip and periodic.hip into the SAME `out` at different operand widths.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_kernel_trees_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture).

`KINDS` has one row per kind of leaf: a constructor, the longdouble reference of k(X1, X2) with its bound, a torch restatement.  The
references and bounds are the ones the leaves' own files derive (imported, not restated).  A new kind of leaf is a new row: the guard
of tests/test_kernel_trees_emulated.py fails until it is there, and every pair test below then crosses it with the others.

Pair level.  Forward: element by element within a bound COMPOSED from the leaves' bounds (`_tree_ref`; u = 2^-53, no free constant):
a Sum adds the bounds and u |partial sum| per addition; a Product  |v| b_j + |k_j| B + B b_j + u |v k_j|  per factor folded into the
running value v with bound B; + u |k + diag_add| on the diagonal.  Adjoint: torch fp64 autograd on the CPU of sum(Kbar .* K(A, B)) and
of sum(kd_bar .* diag K), 1e-8 in the measure of `_close`; pairs with a member whose dk/dr2 is unbounded at r = 0 (Exponential,
Matern12: `CLAMPED`) 2e-6, the figure and the reason of test_gpu_kernel_families.py.

Model level.  Values 1e-9 relative, gradients 1e-8 (`_close`); trees with an Exponential member 1e-7 / 2e-6.  Shapes B = 50, M = 12,
D = 3, P = 2, inputs uniform in [-1, 1], num_data = 1000.

Condition of the model problems (`conditioning_figures`, asserted in the CPU tier by
test_kernel_trees_emulated.py::test_the_oracle_is_conditioned_for_every_tree): every kernel entry and every entry of the row diagonal
perturbed by a relative 4 * 2^-52 with random signs, in torch on the CPU; the oracle's own values and gradients (GPR; SVGP whitened or
not, full or diagonal q_sqrt; SGPR for the constant-diagonal trees) must move by at most 1 / 100 of the tolerance.  Measured, largest
movement of a value (relative) / of a gradient (measure of `_close`) per tree:
  per(se)*lin+rq[0,2] 7.6e-15 / 5.5e-13, poly2*lin[1]+se 1.9e-14 / 4.2e-13, white*lin+se 4.8e-16 / 1.6e-14,
  per(rq)[1,2]+poly3[0,2]*const 1.1e-15 / 4.4e-14 (7.3e-11 with the row's lengthscale 0.8 on the two active columns: 0.4 here),
  (lin+per(se))*(poly2+white) 2.2e-16 / 1.8e-14, per(se)[0]*per(se)[0,1] 5.3e-14 / 4.3e-13, per(rq)*m32+const*white 1.2e-15 / 1.4e-12,
  exp*lin+white 1.5e-16 / 6.3e-12 (against 1e-7 / 2e-6), lin+lin*se 3.4e-14 / 1.9e-13
-- at least 7000 times below the tolerance.
A new tree, shape or seed needs that check to pass; one that fails gets better-conditioned parameters, never a looser tolerance.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import test_gpu_contract as CT  # noqa: E402
import test_gpu_dot_kernels as DK  # noqa: E402
import test_gpu_kernel_families as KF  # noqa: E402
import test_gpu_periodic as PER  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _padding_untouched, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402

VALUE_TOL, GRAD_TOL = DK.VALUE_TOL, DK.GRAD_TOL                                   # 1e-9, 1e-8
CLAMP_VALUE_TOL, CLAMP_GRAD_TOL = KF.VALUE_TOL["Exponential"], KF.GRAD_TOL["Exponential"]   # 1e-7, 2e-6
CLAMPED = ("Exponential", "Matern12")     # dk/dr2 unbounded at r -> 0: the 1e-36 clamp, exact zeros in the product


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


# ------------------------------------------------------------------------------------------------ the kinds of leaf
class Kind:
    """One kind of leaf.  cls: "stationary" | "static" | "periodic" | "dot"; family: the leaf's family (a Periodic's: its base's);
    values: the hyperparameters in the order of the gradients (variance, lengthscales, alpha, then period | offset); cols: active_dims;
    degree: the Polynomial's.  `but` is the same kind with other values -- the trees of the model tests use it."""

    def __init__(self, cls, family, values, cols=None, degree=None):
        self.cls, self.family, self.values, self.cols, self.degree = cls, family, dict(values), cols, degree

    def but(self, cols="same", degree="same", **values):
        return Kind(self.cls, self.family, dict(self.values, **values), self.cols if cols == "same" else cols,
                    self.degree if degree == "same" else degree)

    @property
    def class_name(self):
        return "Periodic" if self.cls == "periodic" else self.family

    @property
    def names(self):
        return tuple(self.values)

    @property
    def is_dot(self):
        return self.cls == "dot"

    @property
    def wide(self):
        """the launches of a tree with this member disagree on the operand width"""
        return self.cls in ("dot", "periodic")

    def make(self, K):
        """(kernel, {name: Parameter})"""
        v, ad = self.values, ({} if self.cols is None else {"active_dims": list(self.cols)})
        if self.cls == "dot":
            k = K.Linear(variance=v["variance"], **ad) if self.family == "Linear" else \
                K.Polynomial(self.degree, variance=v["variance"], offset=v["offset"], **ad)
            return k, {n: getattr(k, n) for n in v}
        if self.cls == "static":
            k = getattr(K, self.family)(variance=v["variance"])
            return k, {"variance": k.variance}
        base = getattr(K, self.family)(**{n: x for n, x in v.items() if n != "period"}, **ad)
        pars = {n: getattr(base, n) for n in v if n != "period"}
        if self.cls == "periodic":
            k = K.Periodic(base, period=v["period"])
            return k, dict(pars, period=k.period)
        return base, pars

    def ref(self, p, X1, X2):
        """(k(X1, X2) in longdouble, bound) at the values p = {name: array}; X2 None: K(X1, X1).  The leaves' own references."""
        sel = (lambda X: X) if self.cols is None else (lambda X: X[:, self.cols])
        A, B = sel(X1), (None if X2 is None else sel(X2))
        if self.cls == "dot":
            s, ds = DK._sref(A, A if B is None else B, p["variance"])
            return DK._kref(self.family, self.degree, s, ds, offset=float(p.get("offset", 0.0)))
        var, alpha = float(p["variance"]), (float(p["alpha"]) if "alpha" in p else None)
        if self.cls == "periodic":
            return PER._periodic_kref("SE" if self.family == "SquaredExponential" else "RQ", alpha, A, B, var, p["lengthscales"], p["period"])
        if self.family in ("SquaredExponential", "Matern12", "Matern32", "Matern52"):
            return CT._kref(self.family, A, A if B is None else B, var, p["lengthscales"])[:2]
        return KF._kref_new(self.family, A, B, var, p.get("lengthscales"), alpha)[:2]

    def torch(self, lv):
        """(kfun(A, B), kdiag(X)) over the leaf tensors lv = {name: tensor}.  The leaves' own restatements."""
        if self.cls == "dot":
            return DK._lin_torch(lv["variance"], lv.get("offset"), self.degree if self.family == "Polynomial" else None, self.cols)
        if self.cls == "periodic":
            kfun = PER._direct("SE" if self.family == "SquaredExponential" else "RQ", lv["variance"], lv["lengthscales"], lv["period"],
                               lv.get("alpha"), self.cols)
        else:
            kfun = KF._torch_kernel(self.family, lv["variance"], lv.get("lengthscales"), lv.get("alpha"), self.cols)
        return kfun, (lambda X: lv["variance"])


D = 3
# Polynomial: odd degree and offset 0.3 -- the base is negative for many pairs at inputs in [-1, 1] (test_gpu_dot_kernels.OFFSET)
KINDS = {
    "SquaredExponential": Kind("stationary", "SquaredExponential", dict(variance=1.1, lengthscales=[0.5, 0.7, 0.9])),
    "Matern12": Kind("stationary", "Matern12", dict(variance=1.2, lengthscales=0.8)),
    "Matern32": Kind("stationary", "Matern32", dict(variance=0.9, lengthscales=0.7)),
    "Matern52": Kind("stationary", "Matern52", dict(variance=0.75, lengthscales=[0.9, 0.6, 0.8])),
    "Exponential": Kind("stationary", "Exponential", dict(variance=0.8, lengthscales=0.6)),
    "RationalQuadratic": Kind("stationary", "RationalQuadratic", dict(variance=0.6, lengthscales=0.9, alpha=0.7)),
    "White": Kind("static", "White", dict(variance=0.3)),
    "Constant": Kind("static", "Constant", dict(variance=0.8)),
    "Periodic(SE)": Kind("periodic", "SquaredExponential", dict(variance=1.3, lengthscales=[0.6, 0.9, 1.3], period=[2.5, 3.0, 3.5])),
    "Periodic(RQ)": Kind("periodic", "RationalQuadratic", dict(variance=0.7, lengthscales=0.8, alpha=0.7, period=2.7), cols=[1, 2]),
    "Linear": Kind("dot", "Linear", dict(variance=[0.5, 2.0, 1.25])),
    "Polynomial": Kind("dot", "Polynomial", dict(variance=0.7, offset=DK.OFFSET), degree=3),
}


# ------------------------------------------------------------------------------------------------ trees over kinds
# A tree is a tag (a key of `kinds`; one tag used twice is ONE kernel instance) or (op, [children]).
def _tags(tree):
    return [tree] if isinstance(tree, str) else [t for c in tree[1] for t in _tags(c)]


def _make_tree(K, tree, kinds):
    """(kernel, {"tag.name": Parameter}), one kernel object per tag"""
    made, pars = {}, {}

    def walk(node):
        if isinstance(node, str):
            if node not in made:
                made[node], ps = kinds[node].make(K)
                pars.update({f"{node}.{n}": p for n, p in ps.items()})
            return made[node]
        return (K.Sum if node[0] == "add" else K.Product)([walk(c) for c in node[1]])
    return walk(tree), pars


def _sub(d, tag):
    return {k[len(tag) + 1:]: v for k, v in d.items() if k.startswith(tag + ".")}


def _tree_ref(tree, kinds, vals, X1, X2, diag_add=0.0, leaf_ref=None):
    """(K in longdouble, bound) of the tree, the bound composed from the leaves' (the module docstring); children are folded left to
    right, as both routes fold them.  vals: {"tag.name": array}."""
    leaf_ref = leaf_ref or (lambda tag: kinds[tag].ref(_sub(vals, tag), X1, X2))

    def walk(node):
        if isinstance(node, str):
            k, b = leaf_ref(node)
            return np.asarray(k, dtype=LD), np.asarray(b, dtype=LD)
        v, B = walk(node[1][0])
        for c in node[1][1:]:
            k, b = walk(c)
            if node[0] == "add":
                v, B = v + k, B + b
                B = B + U * np.abs(v)
            else:
                B = np.abs(v) * b + np.abs(k) * B + B * b
                v = v * k
                B = B + U * np.abs(v)
        return v, B
    k, b = walk(tree)
    if X2 is None and diag_add != 0.0:
        eye = np.eye(k.shape[0], dtype=LD)
        k = k + LD(diag_add) * eye
        b = b + U * np.abs(k) * eye
    return k, b


def _tree_torch(tree, kinds, lv):
    """(kfun(A, B), kdiag(X)) of the tree over lv = {"tag.name": tensor}"""
    def walk(node):
        if isinstance(node, str):
            return kinds[node].torch(_sub(lv, node))
        parts = [walk(c) for c in node[1]]

        def fold(vals):
            acc = vals[0]
            for v in vals[1:]:
                acc = acc + v if node[0] == "add" else acc * v
            return acc
        return (lambda A, B: fold([f(A, B) for f, _ in parts])), (lambda X: fold([g(X) for _, g in parts]))
    return walk(tree)


def _values(pars):
    return {k: np.asarray(p.numpy(), dtype=np.float64) for k, p in pars.items()}


def _leaves(pars, extra=()):
    lv = {key: _leaf(par.numpy()) for key, par in pars.items()}
    lv.update({k: _leaf(v) for k, v in dict(extra).items()})
    return lv


_RATIO = {}


def _ratio(what, got, ref, bnd):
    """the largest error-to-bound ratio of a comparison that passed, kept per `what` for the record (printed by the pair tests)"""
    err, bnd = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref), np.broadcast_to(np.asarray(bnd, dtype=LD), np.shape(ref))
    r = float(np.max(np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1), 0), initial=0.0))
    _RATIO[what] = max(_RATIO.get(what, 0.0), r)
    return r


# ------------------------------------------------------------------------------------------------ 1. pairs, forward
N1, N2, NSYM, DIAG_ADD = 65, 63, 66, 0.1           # a partial tile each way
PAIRS = [(a, b) for a in KINDS for b in KINDS]    # ORDERED: first child (built) and later child (folded in place)
_PAIR_DATA, _LEAF_REF = {}, {}


def _pair_data():
    if not _PAIR_DATA:
        rng = np.random.default_rng(2024)
        _PAIR_DATA.update(X1=rng.uniform(-1.0, 1.0, size=(N1, D)), X2=rng.uniform(-1.0, 1.0, size=(N2, D)),
                          X=rng.uniform(-1.0, 1.0, size=(NSYM, D)), Kbar=rng.normal(size=(N1, N2)), Ksym=rng.normal(size=(NSYM, NSYM)),
                          kd_bar=rng.normal(size=NSYM))
        _PAIR_DATA["Ksym"] = _PAIR_DATA["Ksym"] + _PAIR_DATA["Ksym"].T
    return _PAIR_DATA


def _leaf_ref(name, vals, symmetric):
    """a kind's reference over the shared pair inputs, computed once (the values are the row's: every pair makes them afresh)"""
    key = (name, symmetric)
    if key not in _LEAF_REF:
        dat = _pair_data()
        _LEAF_REF[key] = KINDS[name].ref(vals, dat["X"] if symmetric else dat["X1"], None if symmetric else dat["X2"])
    return _LEAF_REF[key]


def _spec_of(gp, kern):
    from gpflow_amd.kernels.base import gradient_spec
    return gradient_spec(kern, D)[0]


def _forward_check(gp, name, tree, kinds, layouts, rows=None):
    """one tree, symmetric with diag_add and cross, through Combination.K_into and KernelSpec.build in every layout of `out`, and its
    diagonal; rows: {tag: name of its row of KINDS} where the leaves' references come from the shared cache"""
    dev, dat = _dev(gp), _pair_data()
    kern, pars = _make_tree(gp.kernels, tree, kinds)
    vals = _values(pars)
    spec = _spec_of(gp, kern)
    assert spec.constant_diagonal == (not any(kinds[t].is_dot for t in _tags(tree)))

    def leaf_ref(symmetric):
        return None if rows is None else (lambda tag: _leaf_ref(rows[tag], _sub(vals, tag), symmetric))
    for symmetric in (True, False):
        A, B = (dat["X"], None) if symmetric else (dat["X1"], dat["X2"])
        ref, bnd = _tree_ref(tree, kinds, vals, A, B, DIAG_ADD, leaf_ref(symmetric))
        tA, tB = _on(A, "ld", dev), (None if symmetric else _on(B, "pad", dev))
        shape = (A.shape[0], A.shape[0] if symmetric else B.shape[0])
        for layout in layouts:
            outs = []
            for route in ("K_into", "K_into", "build"):
                out, buf = _on(np.full(shape, -555.0), layout, dev, base=True)
                if route == "K_into":
                    kern.K_into(tA, tB, out, diag_add=DIAG_ADD)
                else:
                    spec.build(tA, tB, out, DIAG_ADD)
                assert _padding_untouched(out, buf), f"{name} {route} {layout}: padding written"
                outs.append(_np(out).copy())
            _within(f"{name} symmetric={symmetric} {layout}", outs[0], ref, bnd)
            _ratio("forward", outs[0], ref, bnd)
            assert _same_bits(outs[0], outs[1]), f"{name} {layout}: a second call differs"
            assert _same_bits(outs[0], outs[2]), f"{name} {layout}: KernelSpec.build differs from Combination.K_into"
        _check_unchanged(name, [tA] + ([] if symmetric else [tB]), [A] + ([] if symmetric else [B]))
    # the diagonal (of the symmetric tree, without diag_add)
    ref, bnd = _tree_ref(tree, kinds, vals, dat["X"], None, 0.0, leaf_ref(True))
    dref, dbnd = np.diag(ref), np.diag(bnd)
    tX = _on(dat["X"], "ld", dev)
    _within(f"{name} K_diag", _np(kern.K_diag(tX)), dref, dbnd)
    if spec.constant_diagonal:
        kd = np.full(NSYM, spec.kdiag())
    else:
        kd = _np(spec.kdiag_rows(tX))
        if all(k.cls in ("dot", "static") for k in kinds.values()):     # the sums and products are the builder's: its diagonal bit for bit
            assert _same_bits(kd, np.diag(_np(spec.build(tX, None)))), f"{name}: kdiag_rows differs from the diagonal of K(X, X)"
    _within(f"{name} kdiag", kd, dref, dbnd)
    _ratio("diagonal", kd, dref, dbnd)
    _check_unchanged(name, [tX], [dat["X"]])
    return spec


def _layouts(kinds):
    return ["c"] + (["ld", "off"] if any(k.wide for k in kinds.values()) else [])      # odd ld / misaligned base: the scalar-store path


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_pair_forward(gp, a, b):
    """Sum and Product of (a, b), symmetric with diag_add and cross, through Combination.K_into and KernelSpec.build: within the
    composed bound of the longdouble tree; inputs unchanged; padding untouched; a second call and the other route bitwise equal;
    K_diag and kdiag_rows / kdiag within the same bound of the reference diagonal"""
    kinds = {"a": KINDS[a], "b": KINDS[b]}
    for op in ("add", "mul"):
        spec = _forward_check(gp, f"{a} {op} {b}", (op, ["a", "b"]), kinds, _layouts(kinds), rows={"a": a, "b": b})
        assert spec.tree == (op, [0, 1])
    if "Polynomial" in (a, b):
        assert (_leaf_ref("Polynomial", None, False)[0] < 0).any(), "the data must reach base < 0 at the odd degree"
    print(f"pair forward {a} {b}: largest error / bound so far {_RATIO}")


# flat combinations of three: diag_add rides in the LAST member's launch alone, whatever kind builds first and folds second
TRIPLES = [("Linear", "Periodic(SE)", "White"), ("Polynomial", "Constant", "Periodic(RQ)"), ("Exponential", "Linear", "Matern32"),
           ("Periodic(SE)", "Polynomial", "SquaredExponential"), ("White", "RationalQuadratic", "Linear")]


@pytest.mark.parametrize("op", ["add", "mul"])
@pytest.mark.parametrize("names", TRIPLES, ids=["-".join(t) for t in TRIPLES])
def test_flat_triples_forward(gp, names, op):
    kinds = dict(zip("abc", (KINDS[n] for n in names)))
    spec = _forward_check(gp, f"{op} of {names}", (op, ["a", "b", "c"]), kinds, _layouts(kinds), rows=dict(zip("abc", names)))
    assert spec.tree == (op, [0, 1, 2])


def test_nested_trees_forward(gp):
    """the trees of the model tests at the pair shapes: a subtree as first child, as a later child (its own matrix; diag_add added on
    the host when it is the last), one instance used twice"""
    for name, (tree, kinds, _) in TREES.items():
        _forward_check(gp, name, tree, kinds, _layouts(kinds))
    print(f"nested forward: largest error / bound so far {_RATIO}")


# ------------------------------------------------------------------------------------------------ 2. pairs, adjoint
def _grad_of(lv, key):
    g = lv[key].grad
    return np.zeros(lv[key].shape) if g is None else g.numpy()


def _shape_ref(lv, tag, kind):
    """the oracle's shape gradient of one member in the user's layout: lengthscales, alpha, then period | offset"""
    parts = [np.reshape(_grad_of(lv, f"{tag}.{n}"), -1) for n in kind.names[1:]]
    return np.concatenate(parts) if parts else np.zeros(0)


_WORST = {}


def _close_rec(route, name, got, ref, tol):
    """`_close`, and the largest error in its measure kept per route for the record"""
    got_ = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, dtype=np.float64)
    ref_ = np.asarray(ref, dtype=np.float64)
    if ref_.size:
        _WORST[route] = max(_WORST.get(route, 0.0), float(np.abs(got_.reshape(ref_.shape) - ref_).max() / max(1.0, np.abs(ref_).max())))
    else:
        assert got_.size == 0, (name, got_.shape)
        return
    _close(name, got, ref, tol)


@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_pair_adjoint(gp, a, b):
    """KernelSpec.adjoint (symmetric and cross) and diag_adjoint of the Sum and the Product of (a, b) against autograd of
    sum(Kbar .* K(A, B)) and sum(kd_bar .* diag K): every member's variance (D entries for the ARD Linear), its shape gradient in the
    user's layout and A_bar.  A pair with a clamped member also runs the cross case on exactly coincident rows, Bm = A[:n2] + 0: the
    clamp's exact zero then lands inside the sibling's Kb."""
    dev, dat = _dev(gp), _pair_data()
    kinds = {"a": KINDS[a], "b": KINDS[b]}
    clamped = kinds["a"].family in CLAMPED or kinds["b"].family in CLAMPED
    tol, rec = (CLAMP_GRAD_TOL, "pair adjoint (clamped)") if clamped else (GRAD_TOL, "pair adjoint")
    cases = [("symmetric", dat["X"], None, dat["Ksym"]), ("cross", dat["X1"], dat["X2"], dat["Kbar"])]
    if clamped:
        cases.append(("coincident", dat["X1"], dat["X1"][:N2] + 0, dat["Kbar"]))
    for op in ("add", "mul"):
        tree = (op, ["a", "b"])
        kern, pars = _make_tree(gp.kernels, tree, kinds)
        spec = _spec_of(gp, kern)
        for case, A, B, Kbar in cases:
            name = f"{a} {op} {b} {case}"
            tA, tK = _on(A, "c", dev), _on(Kbar, "c", dev)
            tB = tA if B is None else _on(B, "c", dev)
            dv, dl, Abar = spec.adjoint(tA, tB, tK, B is None)
            lv = _leaves(pars, {"A": A})
            kfun, _ = _tree_torch(tree, kinds, lv)
            (_t(Kbar) * kfun(lv["A"], lv["A"] if B is None else _t(B))).sum().backward()
            for i, tag in enumerate(("a", "b")):
                _close_rec(rec, f"{name} {tag}.variance", dv[i], np.reshape(_grad_of(lv, f"{tag}.variance"), -1), tol)
                _close_rec(rec, f"{name} {tag} shape", dl[i], _shape_ref(lv, tag, kinds[tag]), tol)
            _close_rec(rec, f"{name} A_bar", Abar, _grad_of(lv, "A"), tol)
            _check_unchanged(name, [tA, tK], [A, Kbar])
        if not spec.constant_diagonal:
            name = f"{a} {op} {b} diagonal"
            tX, tg = _on(dat["X"], "c", dev), _on(dat["kd_bar"], "c", dev)
            dv, dl = spec.diag_adjoint(tX, tg)
            lv = _leaves(pars)
            _, kdiag = _tree_torch(tree, kinds, lv)
            (_t(dat["kd_bar"]) * kdiag(_t(dat["X"]))).sum().backward()
            for i, tag in enumerate(("a", "b")):
                _close_rec(rec + " diagonal", f"{name} {tag}.variance", dv[i], np.reshape(_grad_of(lv, f"{tag}.variance"), -1), tol)
                _close_rec(rec + " diagonal", f"{name} {tag} shape", dl[i], _shape_ref(lv, tag, kinds[tag]), tol)
            _check_unchanged(name, [tX, tg], [dat["X"], dat["kd_bar"]])
    print(f"pair adjoint {a} {b}: largest error so far {_WORST}")


# ------------------------------------------------------------------------------------------------ 3. nested trees through the models
B_, M_, P_ = 50, 12, 2
_K = KINDS
# name -> (tree, {tag: Kind}, options).  Between them every kind sits first, later and nested, over overlapping and over disjoint
# active_dims; "lin+lin*se" uses ONE Linear instance twice (its Parameter collects the sum).  Z_on_data: Z = X[:M].
TREES = {
    "per(se)*lin+rq[0,2]": (("add", [("mul", ["per", "lin"]), "rq"]),
                            {"per": _K["Periodic(SE)"], "lin": _K["Linear"], "rq": _K["RationalQuadratic"].but(cols=[0, 2], lengthscales=0.5)}, {}),
    "poly2*lin[1]+se": (("add", [("mul", ["poly", "lin"]), "se"]),
                        {"poly": _K["Polynomial"].but(degree=2), "lin": _K["Linear"].but(cols=[1], variance=0.8), "se": _K["SquaredExponential"]},
                        {"heteroskedastic": True}),
    "white*lin+se": (("add", [("mul", ["white", "lin"]), "se"]), {"white": _K["White"], "lin": _K["Linear"], "se": _K["SquaredExponential"]}, {}),
    "per(rq)[1,2]+poly3[0,2]*const": (("add", ["per", ("mul", ["poly", "const"])]),
                                      {"per": _K["Periodic(RQ)"].but(lengthscales=0.4), "poly": _K["Polynomial"].but(cols=[0, 2], variance=[0.8, 0.5]),
                                       "const": _K["Constant"]}, {}),
    "(lin+per(se))*(poly2+white)": (("mul", [("add", ["lin", "per"]), ("add", ["poly", "white"])]),
                                    {"lin": _K["Linear"], "per": _K["Periodic(SE)"], "poly": _K["Polynomial"].but(degree=2), "white": _K["White"]},
                                    {"heteroskedastic": True}),
    "per(se)[0]*per(se)[0,1]": (("mul", ["p0", "p01"]),
                                {"p0": _K["Periodic(SE)"].but(cols=[0], lengthscales=0.6, period=2.5),
                                 "p01": _K["Periodic(SE)"].but(cols=[0, 1], lengthscales=[0.7, 0.5], period=[2.2, 3.1], variance=0.9)}, {}),
    "per(rq)*m32+const*white": (("add", [("mul", ["per", "m32"]), ("mul", ["const", "white"])]),
                                {"per": _K["Periodic(RQ)"].but(cols=None, lengthscales=0.8), "m32": _K["Matern32"], "const": _K["Constant"],
                                 "white": _K["White"]}, {}),
    "exp*lin+white": (("add", [("mul", ["exp", "lin"]), "white"]), {"exp": _K["Exponential"], "lin": _K["Linear"], "white": _K["White"]},
                      {"Z_on_data": True}),
    "lin+lin*se": (("add", ["lin", ("mul", ["lin", "se"])]), {"lin": _K["Linear"], "se": _K["SquaredExponential"]}, {}),
}
ROW_TREES = [n for n, (t, kinds, _) in TREES.items() if any(kinds[tag].is_dot for tag in _tags(t))]
CONSTANT_TREES = [n for n in TREES if n not in ROW_TREES]
HET_TREES = [n for n, (_, _, o) in TREES.items() if o.get("heteroskedastic")]
_PROBLEM = {}


def _tols(name):
    clamped = any(k.family in CLAMPED for k in TREES[name][1].values())
    return (CLAMP_VALUE_TOL, CLAMP_GRAD_TOL) if clamped else (VALUE_TOL, GRAD_TOL)


def _problem(on_data=False):
    """B = 50, M = 12, D = 3, P = 2, inputs uniform in [-1, 1]; made once and shared.  on_data: Z = X[:M] exactly."""
    if not _PROBLEM:
        rng = np.random.default_rng(3012)
        X = rng.uniform(-1.0, 1.0, size=(B_, D))
        _PROBLEM.update(X=X, Y=np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(B_, P_)), Z=rng.uniform(-1.0, 1.0, size=(M_, D)),
                        q_mu=0.3 * rng.normal(size=(M_, P_)),
                        q_sqrt=np.stack([np.tril(0.05 * rng.normal(size=(M_, M_))) + 0.6 * np.eye(M_) for _ in range(P_)]),
                        Xnew=rng.uniform(-1.0, 1.0, size=(2, 4, D)))
    p = _PROBLEM
    return p["X"], p["Y"], (p["X"][:M_].copy() if on_data else p["Z"]), p["q_mu"], p["q_sqrt"]


def _model_tree(K, name):
    tree, kinds, opts = TREES[name]
    kern, pars = _make_tree(K, tree, kinds)
    return kern, pars, (lambda lv: _tree_torch(tree, kinds, lv)), opts


HET_A, HET_B = np.array([[-0.1], [0.05], [0.02]]), np.array([0.6])


def _het_noise(lv, X):
    return torch.clamp(X @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2


def _route(route, name):
    return route + (" (clamped)" if _tols(name)[0] == CLAMP_VALUE_TOL else "")


def _agree(route, name, v, ref, forward, tol):
    _WORST[route + " value"] = max(_WORST.get(route + " value", 0.0), abs(v - ref) / abs(ref))
    assert abs(v - ref) <= tol * abs(ref), (name, v, ref)
    assert abs(forward - v) <= tol * abs(v), (name, "forward against *_and_grad", forward, v)


def _grads_rec(route, name, g, pars, lv, tol):
    """`_check_model_grads`, with the largest error kept per route for the record"""
    for key, par in pars.items():
        ref = _grad_of(lv, key).reshape(np.shape(par.unconstrained_variable)) * par.transform.forward_grad(par.unconstrained_variable)
        assert par in g, (name, key)
        _close_rec(route, f"{name} {key}", np.asarray(g[par]), ref, tol)
    _check_model_grads(name, g, pars, lv, tol)


@pytest.mark.parametrize("name", list(TREES))
def test_gpr_trees_vs_autograd_oracle(gp, name):
    """GPR.log_marginal_likelihood (composed from self.kernel(X)) and _and_grad, a Constant mean: every member's Parameters, the noise
    and the mean; the keys of the gradient are exactly the trainable Parameters"""
    gpflow = gp
    kern, pars, tk, opts = _model_tree(gpflow.kernels, name)
    vtol, gtol = _tols(name)
    X, Y, _, _, _ = _problem()
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.1))
    v, g = m.log_marginal_likelihood_and_grad()
    lv = _leaves(pars, {"noise": 0.15, "mean": 0.1})
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=tk(lv)[0])
    Fo.backward()
    _agree(_route("gpr", name), name, v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()), vtol)
    allp = dict(pars, noise=m.likelihood.variance, mean=m.mean_function.c)
    _grads_rec(_route("gpr", name), "gpr " + name, g, allp, lv, gtol)
    assert set(g) == set(allp.values()) == set(m.trainable_parameters)
    print(f"gpr {name}: largest error so far {_WORST}")


def _svgp_model(gpflow, kern, problem, *, whiten, q_diag, het=False):
    X, Y, Z, q_mu, q_sqrt = problem
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    lik = gpflow.likelihoods.Gaussian(scale=gpflow.functions.Linear(A=HET_A.copy(), b=HET_B.copy())) if het else gpflow.likelihoods.Gaussian(0.2)
    m = gpflow.models.SVGP(kern, lik, Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, q_diag=q_diag, whiten=whiten, num_latent_gps=q_mu.shape[1],
                           num_data=1000, mean_function=gpflow.mean_functions.Constant(0.1))
    return m, q_sqrt


def _svgp_oracle(tk, pars, problem, q_sqrt, *, whiten, het):
    X, Y, Z, q_mu, _ = problem
    lv = _leaves(pars, {"Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.1})
    lv.update({"A": _leaf(HET_A), "b": _leaf(HET_B)} if het else {"noise": _leaf(0.2)})
    kfun, kdiag = tk(lv)
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], lv["q_sqrt"], None, None, _het_noise(lv, _t(X)) if het else lv["noise"],
                              num_data=1000, whiten=whiten, mean=lv["mean"], kfun=kfun, kdiag=kdiag(_t(X)))
    return Fo, lv


def _svgp_check(gpflow, name, *, whiten, q_diag, het=False):
    kern, pars, tk, opts = _model_tree(gpflow.kernels, name)
    vtol, gtol = _tols(name)
    problem = _problem(opts.get("Z_on_data", False))
    m, q_sqrt = _svgp_model(gpflow, kern, problem, whiten=whiten, q_diag=q_diag, het=het)
    if name in ROW_TREES:
        assert m._fused_config() is None, "the fused shard takes K_diag for the variance and must decline"
    X, Y = problem[:2]
    v, g = m.elbo_and_grad((X, Y))
    Fo, lv = _svgp_oracle(tk, pars, problem, q_sqrt, whiten=whiten, het=het)
    Fo.backward()
    route = _route("svgp" + (" heteroskedastic" if het else ""), name)
    _agree(route, name, v, float(Fo.detach()), float(m.elbo((X, Y)).cpu()), vtol)
    lik_pars = {"A": m.likelihood.scale.A, "b": m.likelihood.scale.b} if het else {"noise": m.likelihood.variance}
    allp = dict(pars, Z=m.inducing_variable.Z, q_mu=m.q_mu, mean=m.mean_function.c, **lik_pars)
    _grads_rec(route, f"svgp {name}", g, allp, lv, gtol)
    if q_diag:
        _grads_rec(route, f"svgp {name}", g, {"q_sqrt": m.q_sqrt}, lv, gtol)
    else:            # fill-triangular: the unconstrained vector holds the lower-triangular entries
        ref = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
        _close_rec(route, f"svgp {name} q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(ref).reshape(np.shape(g[m.q_sqrt])), gtol)
    assert set(g) == set(allp.values()) | {m.q_sqrt} == set(m.trainable_parameters)
    print(f"svgp {name}: largest error so far {_WORST}")


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("name", list(TREES))
def test_svgp_trees_vs_autograd_oracle(gp, name, whiten, q_diag):
    """SVGP.elbo (composed: the posterior) and elbo_and_grad, num_data = 1000 against B = 50: every member's Parameters, Z, q_mu, q_sqrt,
    the noise and the mean constant; "exp*lin+white" with its inducing points ON data rows"""
    _svgp_check(gp, name, whiten=whiten, q_diag=q_diag)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("name", HET_TREES)
def test_svgp_trees_heteroskedastic_vs_autograd_oracle(gp, name, whiten):
    """Gaussian(scale=Linear(A, b)): dF/d sigma_n^2 per row takes the rows of the tree's diagonal as well"""
    _svgp_check(gp, name, whiten=whiten, q_diag=not whiten, het=True)


def _sgpr_upper_np(X, Y, Kuu, Kuf, kdiag_sum, s2, mean):
    """oracle.gp_oracle.sgpr_upper_bound (gpflow/models/sgpr.py:85-148, one output column) over given covariance matrices"""
    N, M = X.shape[0], Kuu.shape[0]
    L = np.linalg.cholesky(Kuu)
    A = np.linalg.solve(L, Kuf)
    LB = np.linalg.cholesky(np.eye(M) + A @ A.T / s2)
    c = kdiag_sum - np.sum(A * A)
    cn = s2 + c
    A_cn = A / np.sqrt(cn)
    err = (Y - mean) / np.sqrt(cn)
    v = np.linalg.solve(np.linalg.cholesky(np.eye(M) + A_cn @ A_cn.T), A_cn @ err)
    return -0.5 * N * np.log(2 * np.pi * s2) - np.sum(np.log(np.diag(LB))) - 0.5 * np.sum(err ** 2) + 0.5 * np.sum(v * v)


@pytest.mark.parametrize("name", CONSTANT_TREES)
def test_sgpr_constant_diagonal_trees_vs_autograd_oracle(gp, name):
    """SGPR.elbo, objective_and_grad and upper_bound (one output column) for the mixed trees whose diagonal is one scalar"""
    gpflow = gp
    kern, pars, tk, opts = _model_tree(gpflow.kernels, name)
    vtol, gtol = _tols(name)
    X, Y, Z, _, _ = _problem()
    s = gpflow.models.SGPR((X, Y), kern, Z.copy(), noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.1))
    v, g = s.objective_and_grad()
    lv = _leaves(pars, {"noise": 0.15, "Z": Z, "mean": 0.1})
    kfun, kdiag = tk(lv)
    Fo = orcg.sgpr_elbo_torch(_t(X), _t(Y), lv["Z"], None, None, lv["noise"], jitter=1e-6, mean=lv["mean"], kfun=kfun, kdiag=kdiag(_t(X)))
    Fo.backward()
    _agree("sgpr", name, v, float(Fo.detach()), float(s.elbo().cpu()), vtol)
    allp = dict(pars, noise=s.likelihood.variance, Z=s.inducing_variable.Z, mean=s.mean_function.c)
    _grads_rec("sgpr", "sgpr " + name, g, allp, lv, gtol)
    assert set(g) == set(allp.values()) == set(s.trainable_parameters)
    one = gpflow.models.SGPR((X, Y[:, :1]), kern, Z.copy(), noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.1))
    with torch.no_grad():
        tv = {k: _t(p.numpy()) for k, p in pars.items()}
        kf, kd = tk(tv)
        tZ, tX = _t(Z), _t(X)
        want = _sgpr_upper_np(X, Y[:, :1], kf(tZ, tZ).numpy() + 1e-6 * np.eye(M_), kf(tZ, tX).numpy(), B_ * float(kd(tX)), 0.15, 0.1)
    ub = float(one.upper_bound().cpu())
    _WORST["sgpr upper_bound value"] = max(_WORST.get("sgpr upper_bound value", 0.0), abs(ub - want) / abs(want))
    assert abs(ub - want) <= vtol * abs(want), (name, ub, want)
    assert float(one.elbo().cpu()) <= ub
    print(f"sgpr {name}: largest error so far {_WORST}")


def test_scipy_on_a_row_diagonal_tree(gp):
    """optimizers.Scipy for three iterations on SVGP("poly2*lin[1]+se"): its first evaluation IS elbo_and_grad at the start, and the
    objective does not get worse"""
    gpflow = gp
    kern, pars, _, _ = _model_tree(gpflow.kernels, "poly2*lin[1]+se")
    problem = _problem()
    m, _ = _svgp_model(gpflow, kern, problem, whiten=True, q_diag=False)
    data = problem[:2]
    v0, g0 = m.elbo_and_grad(data)
    before = float(m.elbo(data).cpu())
    seen, inner = [], m.elbo_and_grad

    def logged(d):
        seen.append(inner(d))
        return seen[-1]
    m.elbo_and_grad = logged
    res = gpflow.optimizers.Scipy().minimize(m, data, options=dict(maxiter=3))
    del m.elbo_and_grad
    assert len(seen) >= 2 and seen[0][0] == v0 and list(seen[0][1]) == list(g0)
    assert all(_same_bits(np.asarray(seen[0][1][p]), np.asarray(g0[p])) for p in g0)
    after = float(m.elbo(data).cpu())
    assert after >= before and res.fun <= -v0 and abs(res.fun + after) <= 1e-8 * abs(after), (before, after, res.fun)
    assert any(abs(float(np.ravel(p.numpy())[0]) - float(np.ravel(v)[0])) > 1e-6 for p, v in
               ((pars[k], TREES["poly2*lin[1]+se"][1][k.split(".")[0]].values[k.split(".")[1]]) for k in pars)), "no kernel Parameter moved"


# ------------------------------------------------------------------------------------------------ 4. predict
def _kernel_np(tk, pars):
    tv = {k: _t(p.numpy()) for k, p in pars.items()}
    kfun, kdiag = tk(tv)

    def K(A, B=None):
        with torch.no_grad():
            tA = _t(A)
            return kfun(tA, tA if B is None else _t(B)).numpy()
    return K


def _pclose(a, b, tol=VALUE_TOL):
    return np.abs(_np(a) - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", ["per(se)*lin+rq[0,2]", "(lin+per(se))*(poly2+white)", "per(rq)*m32+const*white", "exp*lin+white"])
def test_predict_f_of_trees_in_the_four_covariance_forms(gp, name):
    """SVGP.predict_f fused and through the cached posterior, full_cov x full_output_cov, whitened and not, Xnew [2, 4, D], against a
    NumPy restatement of base_conditional (test_gpu_dot_kernels._posterior_np); GPR.predict_f likewise"""
    gpflow = gp
    kern, pars, tk, opts = _model_tree(gpflow.kernels, name)
    X, Y, Z, q_mu, q_sqrt = _problem(opts.get("Z_on_data", False))
    Xn = _PROBLEM["Xnew"]
    Kf, vtol = _kernel_np(tk, pars), _tols(name)[0]   # (an Exponential member: the reference's own k(x, x) is off by 1e-8)
    nb, n = Xn.shape[:2]
    Kmm = Kf(Z) + 1e-6 * np.eye(M_)
    for whiten in (True, False):
        m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten, num_latent_gps=P_)
        refs = []
        for xb in Xn:                                      # every batch entry is a conditional of its own
            Kmn, Knn = Kf(Z, xb), Kf(xb)
            mean, var = DK._posterior_np(Kmm, Kmn, np.diag(Knn), q_mu, q_sqrt, whiten, False)
            _, cov = DK._posterior_np(Kmm, Kmn, Knn, q_mu, q_sqrt, whiten, True)
            refs.append((mean, var, cov))
        mean, var, cov = (np.stack([r[i] for r in refs]) for i in range(3))
        for post in (None, m.posterior()):
            f = (lambda **kw: m.predict_f(Xn, **kw)) if post is None else (lambda **kw: post.predict_f(Xn, **kw))
            mu, v = f()
            assert tuple(mu.shape) == (nb, n, P_) and _pclose(mu, mean, vtol) and _pclose(v, var, vtol), (name, whiten, post is None)
            mu, v = f(full_cov=True)
            assert tuple(v.shape) == (nb, P_, n, n) and _pclose(mu, mean, vtol) and _pclose(v, cov, vtol), (name, whiten, post is None)
            mu, v = f(full_output_cov=True)
            assert tuple(v.shape) == (nb, n, P_, P_) and _pclose(v, np.stack([[np.diag(r) for r in vb] for vb in var]), vtol)
            mu, v = f(full_cov=True, full_output_cov=True)
            assert tuple(v.shape) == (nb, n, P_, n, P_)
            for p in range(P_):
                assert _pclose(v[:, :, p, :, p], cov[:, p], vtol)
            assert _pclose(v[:, :, 0, :, 1], 0 * cov[:, 0], vtol)
    r = gpflow.models.GPR((X, Y), kern, noise_variance=0.15)
    Kxx = Kf(X) + 0.15 * np.eye(B_)
    for post in (None, r.posterior()):
        f = (lambda **kw: r.predict_f(Xn, **kw)) if post is None else (lambda **kw: post.predict_f(Xn, **kw))
        mu, v = f()
        muc, vc = f(full_cov=True)
        for i, xb in enumerate(Xn):
            Kxn = Kf(X, xb)
            sol = np.linalg.solve(Kxx, Kxn)
            want = Kf(xb) - Kxn.T @ sol
            assert _pclose(mu[i], sol.T @ Y, vtol) and _pclose(muc[i], sol.T @ Y, vtol), (name, post is None)
            assert _pclose(v[i], np.repeat(np.diag(want)[:, None], P_, 1), vtol) and _pclose(vc[i], np.stack([want] * P_), vtol), (name, post is None)


@pytest.mark.parametrize("wrapper", ["separate", "lcm"])
def test_multioutput_wrappers_over_two_mixed_trees(gp, wrapper):
    """SeparateIndependent / LinearCoregionalization over two different mixed trees with shared inducing points, forward only: the
    fused per-latent shards are declined, the ELBO is the sum of the single-latent models (the mixing W = I for that check), predict_f
    is the per-latent conditionals (mixed by a general W) and the reverse pass is refused"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    X, Y, Z, q_mu, q_sqrt = _problem()
    Xn = _PROBLEM["Xnew"][0]
    made = [_model_tree(K, n) for n in ("white*lin+se", "per(rq)[1,2]+poly3[0,2]*const")]
    ks = [mk[0] for mk in made]
    W = np.array([[0.8, -0.3], [0.4, 1.1]])
    lik = gpflow.likelihoods.Gaussian(0.2)

    def model(kern):
        iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))
        return gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2, num_data=120)
    m = model(K.SeparateIndependent(ks) if wrapper == "separate" else K.LinearCoregionalization(ks, W=np.eye(2)))
    assert m._fused_separate_config() is None and m._fused_lcm_config() is None
    total = 0.0
    for p, kp in enumerate(ks):
        one = gpflow.models.SVGP(kp, lik, Z.copy(), q_mu=q_mu[:, p:p + 1], q_sqrt=q_sqrt[p:p + 1], num_data=120)
        total += float(one.elbo((X, Y[:, p:p + 1])).cpu())
    got = float(m.elbo((X, Y)).cpu())
    assert abs(got - total) <= 1e-10 * abs(total), (got, total)
    with pytest.raises(NotImplementedError, match="per-latent"):
        m.elbo_and_grad((X, Y))
    means, vars_ = [], []
    for p, (_, pars, tk, _) in enumerate(made):
        Kf = _kernel_np(tk, pars)
        mean, var = DK._posterior_np(Kf(Z) + 1e-6 * np.eye(M_), Kf(Z, Xn), np.diag(Kf(Xn)), q_mu[:, p:p + 1], q_sqrt[p:p + 1], True, False)
        means.append(mean[:, 0])
        vars_.append(var[:, 0])
    gm, gv = np.stack(means, 1), np.stack(vars_, 1)
    if wrapper == "lcm":
        m = model(K.LinearCoregionalization(ks, W=W))
        gm, gv = gm @ W.T, gv @ (W * W).T
    for post in (None, m.posterior()):
        mu, v = m.predict_f(Xn) if post is None else post.predict_f(Xn)
        assert _pclose(mu, gm) and _pclose(v, gv), (wrapper, post is None)


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_stay_refusals(gp):
    """before anything touches a device: SGPR, NaturalGradient, SVGPTrainer, a quadrature likelihood and the per-latent reverse passes for
    a tree with a dot-product member; SVGPTrainer for a tree with a Periodic or a RationalQuadratic member"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    X, Y, Z, q_mu, q_sqrt = _problem()
    lik = gpflow.likelihoods.Gaussian(0.2)
    for name in ROW_TREES:
        k = _model_tree(K, name)[0]
        for call in (lambda s: s.elbo(), lambda s: s.objective_and_grad(), lambda s: s.upper_bound(), lambda s: s.predict_f(X[:3])):
            with pytest.raises(NotImplementedError, match="SGPR"):
                call(gpflow.models.SGPR((X, Y[:, :1]), k, Z.copy()))
        m = gpflow.models.SVGP(k, lik, Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2)
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(m)
        with pytest.raises(NotImplementedError, match="natural gradients"):
            gpflow.optimizers.NaturalGradient(gamma=0.5).minimize(m, (X, Y))
        mb = gpflow.models.SVGP(k, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1])
        with pytest.raises(NotImplementedError, match="quadrature"):
            mb.elbo_and_grad((X, (Y[:, :1] > 0).astype(np.float64)))
        iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))
        for kern in (K.SeparateIndependent([k, K.SquaredExponential()]), K.LinearCoregionalization([K.SquaredExponential(), k], W=np.eye(2))):
            with pytest.raises(NotImplementedError, match="per-latent"):
                gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2).elbo_and_grad((X, Y))
    for name in CONSTANT_TREES + ["per(se)*lin+rq[0,2]"]:        # a Periodic / RationalQuadratic member: no device-resident trainer
        m = gpflow.models.SVGP(_model_tree(K, name)[0], lik, Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2)
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(m)
    with pytest.raises(NotImplementedError, match="trainer"):
        gpflow.training.SVGPTrainer(gpflow.models.SVGP(K.SquaredExponential() * K.RationalQuadratic(), lik, Z.copy()))


# ------------------------------------------------------------------------------------------------ the conditioning pre-check
EPS_K = 4 * 2.0 ** -52


def _perturbed(f, seed):
    """f with every entry of its result moved by a relative 4 * 2^-52, signs random but fixed per shape"""
    def g(*a):
        out = f(*a)
        if out.dim() == 0:
            return out * (1.0 + EPS_K)
        sign = torch.tensor(np.random.default_rng([seed, *out.shape]).choice([-1.0, 1.0], size=tuple(out.shape)))
        return out * (1.0 + EPS_K * sign)
    return g


def conditioning_figures(name):
    """(largest relative movement of a value, largest movement of a gradient in the measure of `_close`) of the ORACLE's own results
    over every model route of tree `name` when the kernel matrices and the row diagonal are perturbed (module docstring).  CPU only."""
    class _Pars:      # the values a kernel's Parameters would hold, without making one
        def __init__(self, v):
            self.v = np.asarray(v, dtype=np.float64)

        def numpy(self):
            return self.v
    tree, kinds, opts = TREES[name]
    pars = {f"{tag}.{n}": _Pars(v) for tag in dict.fromkeys(_tags(tree)) for n, v in kinds[tag].values.items()}
    tk = lambda lv: _tree_torch(tree, kinds, lv)   # noqa: E731
    problem = _problem(opts.get("Z_on_data", False))
    X, Y, Z, q_mu, q_sqrt = problem
    worst_v = worst_g = 0.0

    def runs(make):
        nonlocal worst_v, worst_g
        res = []
        for perturb in (False, True):
            F, lv = make(perturb)
            F.backward()
            res.append((float(F.detach()), {k: _grad_of(lv, k) for k in lv}))
        (v0, g0), (v1, g1) = res
        worst_v = max(worst_v, abs(v1 - v0) / abs(v0))
        for k in g0:
            worst_g = max(worst_g, float(np.abs(g1[k] - g0[k]).max() / max(1.0, np.abs(g0[k]).max())))

    def ktk(perturb, seed):
        def wrapped(lv):
            kfun, kdiag = tk(lv)
            return (_perturbed(kfun, seed), _perturbed(kdiag, seed + 1)) if perturb else (kfun, kdiag)
        return wrapped

    def gpr(perturb):
        lv = _leaves(pars, {"noise": 0.15, "mean": 0.1})
        return orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=ktk(perturb, 1)(lv)[0]), lv
    runs(gpr)
    for whiten in (True, False):
        for q_diag in (False, True):
            qs = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T) if q_diag else q_sqrt
            for het in ([False, True] if opts.get("heteroskedastic") and q_diag != whiten else [False]):
                runs(lambda perturb: _svgp_oracle(ktk(perturb, 3), pars, problem, qs, whiten=whiten, het=het))
    if name in CONSTANT_TREES:
        def sgpr(perturb):
            lv = _leaves(pars, {"noise": 0.15, "Z": Z, "mean": 0.1})
            kfun, kdiag = ktk(perturb, 5)(lv)
            return orcg.sgpr_elbo_torch(_t(X), _t(Y), lv["Z"], None, None, lv["noise"], jitter=1e-6, mean=lv["mean"], kfun=kfun,
                                        kdiag=kdiag(_t(X))), lv
        runs(sgpr)
    return worst_v, worst_g
