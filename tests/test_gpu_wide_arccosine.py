"""GPU tests of the ArcCosine kernel on WIDE inputs, 65 .. 1024 active columns: gpflow_amd/csrc/wide/wide_arccosine.hip behind the five
`ops.arccos_*` wrappers, `gradients.arccos_kernel_adjoint` and the model routes over them.

There is NO CPU twin: tests/fake_arccosine_ops.py asserts d <= 64, so the kernel is held on the device only.  References are the ones
of tests/test_gpu_arccosine.py: `_arc_ref` / `_diag_ref` (longdouble, a bound per element; its dot-product bound (d + 1) u sum |terms|
holds for any summation order, so it covers the matrix pipe), torch autograd over the direct formula (`_arc_torch`) at 1e-8 by `_close`,
and the oracle's torch forms (value 1e-9 relative, gradients 1e-8).  Inputs are plain normal rows: at d >= 65 the cosines concentrate
near 0, and every case asserts margin >= MIN_MARGIN on its reference, so the clamp and the order-0 singularity stay idle.

Condition of the model problems (`_model`; N = 60, 70 columns, weights 1.3 / 70 so that p ~ 2).  Every kernel entry and every entry of
the row diagonal was perturbed by a relative 4 * 2^-52 with random signs in the oracle, on the CPU (`_perturbed` of
test_gpu_arccosine.py); the oracle's gradients moved by at most, in the measure of `_close`: CONDITIONING_FIGURES below -- at least
10 x under the 1e-8 of the gradients.  A new shape or seed needs that check repeated.
"""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
from test_gpu_arccosine import BIAS, MIN_MARGIN, VAR, _arc_ref, _arc_torch, _diag_ref, _kbar, _kw, _perturbed, _split_parts  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _within  # noqa: E402
from test_gpu_dot_kernels import _weights  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t, _torch_kernel  # noqa: E402

ORDERS = (0, 1, 2)
GRAD_TOL = 1e-8
# the largest move of the oracle's gradients under the perturbation of the module docstring (`conditioning_figures`, CPU, these seeds)
CONDITIONING_FIGURES = {"gpr order 0": 9.8e-15, "gpr order 1": 1.2e-14, "gpr order 2": 1.1e-15, "svgp order 0": 8.6e-15,
                        "svgp order 1": 4.1e-15, "svgp order 2": 4.2e-15, "sum order 1": 1.5e-14}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _rows(n1, n2, d):
    rng = np.random.default_rng(100 * n1 + d)
    return rng.normal(size=(n1, d)), (None if n2 is None else rng.normal(size=(n2, d)))


def _ref(order, X1, X2, w):
    r = _arc_ref(order, X1, X2, w, same=X2 is None)
    assert r["margin"] >= MIN_MARGIN, r["margin"]
    return r


# ------------------------------------------------------------------------------------------------ the builder
# (n1, n2 (None: symmetric), d, ard, layout, lower_only, diag_add)
BUILD_CASES = [
    (1, 1, 65, False, "c", False, 0.0),          # first width past the narrow path, a one-column last slab
    (63, 65, 80, True, "c", False, 0.0),         # d a slab multiple, 64-tile edges, ARD
    (127, 129, 130, True, "ld", False, 0.0),     # ragged last slab, odd leading dimensions: scalar loads
    (130, None, 70, False, "c", False, 0.1),     # symmetric: mirrored tiles, the by-index diagonal
    (257, None, 65, True, "c", True, 0.3),       # lower_only: the sentinel survives above the diagonal tiles
    (3, 2, 1024, False, "c", False, 0.0),        # the maximum width
    (255, 257, 96, False, "off", False, 0.0),    # misaligned base
]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("case", BUILD_CASES, ids=[str(c) for c in BUILD_CASES])
def test_wide_arccos_kernel_matrix(gp, case, order):
    n1, n2, d, ard, layout, lower_only, diag_add = case
    X1, X2 = _rows(n1, n2, d)
    w = _weights(ard, d)
    k, bnd = _ref(order, X1, X2, w)["k"]
    if n2 is None:
        k = k + diag_add * np.eye(n1, dtype=LD)
        bnd = bnd + U * np.abs(k) * np.eye(n1)
    t1, t2 = _on(X1, layout), (None if n2 is None else _on(X2, layout))

    def build(lower):
        out = _on(np.full(k.shape, -555.0), "c") if lower else None
        return _np(gp.ops.arccos_kernel_matrix(t1, t2, out=out, diag_add=diag_add, lower_only=lower, **_kw(order, w)))
    K, name = build(lower_only), f"wide arccos_kernel_matrix order {order}"
    if lower_only:   # on or below the diagonal: the full build's bits; above it, inside a diagonal tile: a correct value; beyond: the sentinel
        full, low = build(False), np.tril(np.ones(k.shape, dtype=bool))
        assert np.array_equal(K[low], full[low]), f"{name}: lower_only differs from the full build"
        up = ~low & (K != -555.0)
        _within(name + " upper", K[up], k[up], bnd[up])
        assert np.all(K[np.triu_indices(n1, 128)] == -555.0), f"{name}: a strictly-upper tile was written"
        K = full
    _within(name, K, k, bnd)
    assert n2 is not None or np.array_equal(K, K.T), f"{name}: not exactly symmetric"
    _check_unchanged(name, [t1] + ([] if n2 is None else [t2]), [X1] + ([] if n2 is None else [X2]))
    assert np.array_equal(build(lower_only), build(lower_only)), f"{name}: a second call differs"


@pytest.mark.parametrize("order", ORDERS)
def test_wide_arccos_nan_row(gp, order):
    """one planted NaN in row 129 of X1 and in row 69 of X2 makes exactly that row / column NaN; every other element keeps its bits"""
    X1, X2 = _rows(130, 70, 65)
    B1, B2 = X1.copy(), X2.copy()
    B1[129, 64] = B2[69, 3] = float("nan")
    kw = _kw(order, _weights(True, 65))
    clean, K = _np(gp.ops.arccos_kernel_matrix(_on(X1), _on(X2), **kw)), _np(gp.ops.arccos_kernel_matrix(_on(B1), _on(B2), **kw))
    bad = np.zeros((130, 70), dtype=bool)
    bad[129, :] = bad[:, 69] = True
    assert np.array_equal(np.isnan(K), bad) and np.array_equal(K[~bad], clean[~bad])


@functools.lru_cache(maxsize=None)
def _big(order):
    """(129, 16300, 65): 2 x 128 tiles of 128 = 256 workgroups, the 128-tile.  The reference over all of it is 2 GB: it is taken on every
    43rd column plus the last 200."""
    X1, X2 = _rows(129, 16300, 65)
    cols = np.union1d(np.arange(0, 16300, 43), np.arange(16100, 16300))
    return X1, X2, cols, _ref(order, X1, X2[cols], 1.3)


@pytest.mark.parametrize("order", ORDERS)
def test_wide_arccos_kernel_matrix_on_the_128_tile(gp, order):
    X1, X2, cols, r = _big(order)
    K = _np(gp.ops.arccos_kernel_matrix(_on(X1), _on(X2), **_kw(order, 1.3)))
    _within(f"128-tile order {order}", K[:, cols], *r["k"])


@pytest.mark.parametrize("order", ORDERS)
def test_wide_arccos_symmetric_build_on_the_128_tile(gp, order):
    """2900 rows are 23 x 24 / 2 = 276 tiles of 128 on or below the diagonal.  The strict lower triangle has the bits of the cross build
    of the same rows (the 128-tile, held to the reference above), and the whole is exactly symmetric."""
    tX = _on(np.random.default_rng(11).normal(size=(2900, 65)))
    kw = _kw(order, 1.3)
    S, C = _np(gp.ops.arccos_kernel_matrix(tX, None, diag_add=0.25, **kw)), _np(gp.ops.arccos_kernel_matrix(tX, tX.clone(), **kw))
    low = np.tril_indices(2900, -1)
    assert np.array_equal(S, S.T) and np.array_equal(S[low], C[low])


# ------------------------------------------------------------------------------------------------ combine, row diagonal
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("op", ["mul", "add"])
@pytest.mark.parametrize("n1,n2,d,layout", [(65, 63, 65, "ld"), (129, None, 130, "c")])
def test_wide_arccos_kernel_matrix_combine(gp, n1, n2, d, layout, op, order):
    X1, X2 = _rows(n1, n2, d)
    w = _weights(True, d)
    k, kb = _ref(order, X1, X2, w)["k"]
    Gl = np.random.default_rng(6).normal(size=k.shape)
    eye = np.eye(n1, dtype=LD) if n2 is None else 0   # diag_add goes onto the COMBINED diagonal, and only where X2 is None
    ref = (Gl * k if op == "mul" else Gl + k) + 0.5 * eye
    bnd = (np.abs(Gl) * kb if op == "mul" else kb) + U * np.abs(ref - 0.5 * eye) + U * np.abs(ref) * eye
    t1, t2, tG = _on(X1, layout), (None if n2 is None else _on(X2, layout)), _on(Gl, layout)
    name = f"wide combine {op} order {order}"
    sep = _np(gp.ops.arccos_kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.5, **_kw(order, w)))
    _within(name, sep, ref, bnd)
    _check_unchanged(name, [tG, t1], [Gl, X1])
    assert gp.ops.arccos_kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.5, out=tG, **_kw(order, w)) is tG   # out is G itself
    assert np.array_equal(_np(tG), sep), f"{name}: aliasing changes the result"


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,d", [(1, 65), (257, 130), (5, 1024)])
def test_wide_arccos_kernel_diag(gp, n, d, order):
    X, _ = _rows(n, None, d)
    g = np.random.default_rng(n + d).normal(size=n)
    gl = g.astype(LD)
    for ard in (False, True):
        w, tX = _weights(ard, d), _on(X, "ld")
        (k, kb), (dk, dkb) = _diag_ref(order, X, w), _diag_ref(order, X, w, what="dp")
        name = f"wide arccos_kernel_diag order {order}"
        _within(name + " k", _np(gp.ops.arccos_kernel_diag(tX, **_kw(order, w))), k, kb)
        for op, ref, bnd in (("mul", gl * k, np.abs(gl) * kb + U * np.abs(gl * k)), ("add", gl + k, kb + U * np.abs(gl + k)),
                             ("dp", gl * dk, np.abs(gl) * dkb + U * np.abs(gl * dk))):
            _within(f"{name} {op}", _np(gp.ops.arccos_kernel_diag(tX, _on(g), op=op, **_kw(order, w))), ref, bnd + LD(1e-300))
        _check_unchanged(name, [tX], [X])


# ------------------------------------------------------------------------------------------------ the adjoint stage
def _check_stage(gp, name, order, X1, X2, w, Kb, cols, r):
    """G, the slot sums of `parts` read in the documented layout and the tile sums against `_arc_ref` on the columns `cols` (Kbar is
    zero elsewhere, and G must be), summed as test_gpu_arccosine.py sums them; the extent of parts; G may be Kbar; a rerun has the bits"""
    n1, n2 = Kb.shape
    tr, tc = -(-n1 // 64), -(-n2 // 64)
    extent = tc * n1 + tr * n2 + tr * tc
    t1, t2 = _on(X1), (None if X2 is None else _on(X2))
    runs = []
    for alias in (False, True):
        parts, tK = _on(np.full(extent + 7, -555.0)), _on(Kb)
        G = gp.ops.arccos_adjoint_stage(t1, t2, tK, parts, out=tK if alias else None, **_kw(order, w))
        assert (G is tK) == alias and (alias or np.array_equal(_np(tK), Kb))
        pn = _np(parts)
        assert np.all(pn[extent:] == -555.0) and not np.any(pn[:extent] == -555.0), f"{name}: the extent of parts"
        runs.append((_np(G).copy(), pn[:extent].copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), f"{name}: a rerun differs"
    G, (rho_s, gam_s, sums) = runs[0][0], _split_parts(runs[0][1], n1, n2)
    rest = np.setdiff1d(np.arange(n2), cols)
    assert np.all(G[:, rest] == 0.0) and np.all(gam_s[:, rest] == 0.0)
    Kl = Kb[:, cols].astype(LD)
    dks, ddks = r["dks"]
    _within(name + " G", G[:, cols], Kl * dks, np.abs(Kl) * ddks + U * np.abs(Kl * dks) + LD(1e-300))
    for what, got, (val, bnd), axis in (("rho", rho_s.sum(0), r["dkp"], 1), ("gamma", gam_s.sum(0)[cols], r["dkq"], 0)):
        t = Kl * val
        _within(f"{name} {what}", got, t.sum(axis),
                (np.abs(Kl) * bnd + U * np.abs(t)).sum(axis) + (Kl.shape[axis] + 2) * U * np.abs(t).sum(axis) + LD(1e-300))
    t = Kl * r["jm"][0]
    _within(name + " sum", np.array(sums.sum()), np.array(t.sum()),
            np.array((np.abs(Kl) * r["jm"][1] + U * np.abs(t)).sum() + (84 + tr * tc + 2) * U * np.abs(t).sum()))


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n1,n2,d,ard", [(130, 70, 65, False), (63, None, 80, True), (129, 16300, 65, False)],
                         ids=["cross130x70x65", "symmetric63x80ard", "cross129x16300x65"])
def test_wide_arccos_adjoint_stage(gp, n1, n2, d, ard, order):
    if n2 == 16300:   # 255 column slots; Kbar lives on the sampled columns of `_big`
        X1, X2, cols, r = _big(order)
        w, Kb = 1.3, np.zeros((n1, n2))
        Kb[:, cols] = np.random.default_rng(8).normal(size=(n1, cols.size))
    else:
        X1, X2 = _rows(n1, n2, d)
        w, Kb = _weights(ard, d), _kbar(n1, n1 if n2 is None else n2, n2 is None)
        cols, r = np.arange(Kb.shape[1]), _ref(order, X1, X2, w)
    _check_stage(gp, f"wide stage order {order}", order, X1, X2, w, Kb, cols, r)


# ------------------------------------------------------------------------------------------------ the whole adjoint
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n1,n2,d,ard", [(130, 70, 65, False), (63, None, 80, True), (300, 257, 130, False)],
                         ids=["cross130x70x65", "symmetric63x80ard", "two_tail_blocks300x257x130"])
def test_wide_arccos_kernel_adjoint_against_autograd(gp, n1, n2, d, ard, order):
    """stage, contraction over [1; B^T] alone, two-launch tail (300 rows: two blocks, the last partial) against autograd of
    sum(Kbar .* K) over the direct formula; a rerun is bit-identical"""
    from gpflow_amd import gradients
    from gpflow_amd.leaf import ArcLeaf
    sym = n2 is None
    X1, X2 = _rows(n1, n2, d)
    w, Kb = _weights(ard, d), _kbar(n1, n1 if sym else n2, sym)
    lv = {"A": _leaf(X1), "v": _leaf(VAR), "w": _leaf(w), "b": _leaf(BIAS)}
    kfun, _ = _arc_torch(order, lv["v"], lv["w"], lv["b"])
    (_t(Kb) * kfun(lv["A"], lv["A"] if sym else _t(X2))).sum().backward()
    tA, tK = _on(X1), _on(Kb)
    tB = tA if sym else _on(X2)
    runs = [gradients.arccos_kernel_adjoint(ArcLeaf(order, VAR, w, BIAS), tA, tB, tK, symmetric=sym) for _ in range(2)]
    assert all(np.array_equal(_np(a), _np(b)) for a, b in zip(*runs)), "a rerun differs"
    (dv, dl, Abar), nw, name = runs[0], (d if ard else 1), f"wide adjoint order {order}"
    _close(name + " variance", dv, lv["v"].grad.numpy().reshape(1), GRAD_TOL)
    _close(name + " weights", dl[:nw], lv["w"].grad.numpy().reshape(-1), GRAD_TOL)
    _close(name + " bias", dl[nw:], lv["b"].grad.numpy().reshape(1), GRAD_TOL)
    _close(name + " A_bar", Abar, lv["A"].grad.numpy(), GRAD_TOL)
    _check_unchanged(name, [tA, tK], [X1, Kb])


# ------------------------------------------------------------------------------------------------ models
N, D, M = 60, 70, 12
SE = dict(variance=0.5, lengthscales=0.9 * np.sqrt(D))


def _model(which):
    """(X, Y, Z, q_mu, q_sqrt [1, M, M], Xn): normal inputs, shared by the model tests and by the CPU conditioning check"""
    rng = np.random.default_rng({"gpr": 21, "svgp": 22, "sum": 23}[which])
    X = rng.normal(size=(N, D))
    Y = np.sin(X[:, :3].sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, 1))
    return X, Y, X[:M] + 0.05 * rng.normal(size=(M, D)), 0.2 * rng.normal(size=(M, 1)), \
        (np.tril(0.1 * rng.normal(size=(M, M))) + 0.5 * np.eye(M))[None], rng.normal(size=(5, D))


def _kernel_torch(which, order, lv):
    kfun, kdiag = _arc_torch(order, lv["variance"], lv["weight_variances"], lv["bias_variance"])
    if which != "sum":
        return kfun, kdiag
    se = _torch_kernel("SquaredExponential", lv["se_variance"], lv["se_lengthscales"])
    return (lambda A, B: kfun(A, B) + se(A, B)), (lambda X: kdiag(X) + lv["se_variance"])


def _oracle(which, order, lv, perturb=False):
    X, Y, _, _, q_sqrt, _ = _model(which)
    kfun, kdiag = _kernel_torch(which, order, lv)
    if perturb:
        kfun, kdiag = _perturbed(kfun, kdiag)
    if which == "svgp":
        return orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], _t(q_sqrt), None, None, lv["noise"], num_data=5 * N, whiten=True,
                                    kfun=kfun, kdiag=kdiag(_t(X)))
    return orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], 0.0, kfun=kfun)


def _leaves(which, Z=None, q_mu=None):
    extra = {"sum": dict(se_variance=SE["variance"], se_lengthscales=SE["lengthscales"]), "svgp": dict(Z=Z, q_mu=q_mu)}.get(which, {})
    return {k: _leaf(v) for k, v in dict(variance=VAR, weight_variances=1.3 / D, bias_variance=BIAS, noise=0.2, **extra).items()}


MODEL_CASES = [("gpr", 0), ("gpr", 1), ("gpr", 2), ("svgp", 0), ("svgp", 1), ("svgp", 2), ("sum", 1)]


def conditioning_figures():
    """{problem: the largest move of the oracle's gradients under `_perturbed`, in the measure of `_close`} -- CPU only"""
    out = {}
    for which, order in MODEL_CASES:
        a, b = (_leaves(which, *_model(which)[2:4]) for _ in range(2))
        _oracle(which, order, a).backward()
        _oracle(which, order, b, perturb=True).backward()
        out[f"{which} order {order}"] = max(float((a[k].grad - b[k].grad).abs().max() / max(1.0, a[k].grad.abs().max())) for k in a)
    return out


@pytest.mark.parametrize("which,order", MODEL_CASES, ids=[f"{w}-order{o}" for w, o in MODEL_CASES])
def test_wide_arccos_models(gp, which, order):
    """GPR and whitened SVGP (full q_sqrt) with ArcCosine(order) over 70 columns, GPR with ArcCosine(1) + SquaredExponential, both over
    70 columns: value and every gradient against the oracle; GPR order 1 also predict_f"""
    gpflow, K = gp, gp.kernels
    X, Y, Z, q_mu, q_sqrt, Xn = _model(which)
    arc = K.ArcCosine(order, variance=VAR, weight_variances=1.3 / D, bias_variance=BIAS)
    kern, pars = arc, {"variance": arc.variance, "weight_variances": arc.weight_variances, "bias_variance": arc.bias_variance}
    if which == "sum":
        se = K.SquaredExponential(**SE)
        kern, pars = arc + se, dict(pars, se_variance=se.variance, se_lengthscales=se.lengthscales)
    if which == "svgp":
        m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_data=5 * N)
        (v, g), again = m.elbo_and_grad((X, Y)), lambda: m.elbo((X, Y))
        pars = dict(pars, Z=m.inducing_variable.Z, q_mu=m.q_mu)
    else:
        m = gpflow.models.GPR((X, Y), kern, noise_variance=0.2)
        (v, g), again = m.log_marginal_likelihood_and_grad(), m.log_marginal_likelihood
    pars["noise"] = m.likelihood.variance
    lv = _leaves(which, Z, q_mu)
    Fo = _oracle(which, order, lv)
    Fo.backward()
    ref = float(Fo.detach())
    assert abs(v - ref) <= 1e-9 * abs(ref) and abs(v - float(again().cpu())) <= 1e-9 * abs(v), (v, ref)
    _check_model_grads(f"{which} order {order}", g, pars, lv, GRAD_TOL)
    if (which, order) == ("gpr", 1):
        with torch.no_grad():
            kfun, tX, tn = _kernel_torch(which, order, lv)[0], _t(X), _t(Xn)
            L = torch.linalg.cholesky(kfun(tX, tX) + 0.2 * torch.eye(N, dtype=torch.float64))
            A = torch.linalg.solve_triangular(L, kfun(tX, tn), upper=False)
            rm, rv = A.T @ torch.linalg.solve_triangular(L, _t(Y), upper=False), torch.diagonal(kfun(tn, tn)) - (A * A).sum(0)
        mu, var = m.predict_f(Xn)
        _close("predict mean", mu, rm.numpy(), 1e-8)
        _close("predict variance", var, rv.numpy().reshape(5, 1), 1e-8)


# ------------------------------------------------------------------------------------------------ refusals
def test_wide_arccos_refusals(gp):
    """d = 1025 is a ValueError before the device; the C entry points refuse, with host pointers in the slots and so without a launch,
    what include/gpk.h says they refuse; Linear over 65 columns is still refused"""
    from gpflow_amd import _lib
    from gpflow_amd.ops import arccos_kernel_diag, arccos_kernel_matrix
    big = torch.zeros((2, 1025), dtype=torch.float64)   # (a host tensor: the width is refused before anything asks where it lives)
    for call in (lambda: arccos_kernel_matrix(big, None), lambda: arccos_kernel_diag(big)):
        with pytest.raises(ValueError, match="64.*1024"):
            call()
    with pytest.raises(ValueError):
        gp.ops.dot_kernel_matrix(_on(np.zeros((2, 65))), None, variance=1.0)
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    a = ctypes.cast(buf, ctypes.c_void_p).value

    def km(order=1, n1=3, d=65, v=1.0, b=1.0, ldx=None, ldk=3, w=a):
        return lib.gpk_wide_arc_kernel_matrix(None, order, a, n1, d if ldx is None else ldx, None, 0, 0, d, w, 0, v, b, 0.0, 0, a, ldk)

    def stage(plen, n1=3, order=1):
        return lib.gpk_wide_arc_adjoint_stage(None, order, a, n1, 65, None, 0, 0, 65, a, 0, 1.0, 1.0, a, 3, a, 3, a, plen)

    def tail(plen=7, slen=66, n1=3, ldr=66):
        return lib.gpk_wide_arc_adjoint_tail(None, a, ldr, a, 65, n1, None, 0, 0, 65, a, 0, a, plen, a, a, slen, a, a, 65)
    assert [km(order=o) for o in (-1, 3)] == [-3, -3] and [km(d=x) for x in (0, 1025)] == [-1, -1] and km(w=None) == -1
    assert [km(v=x) for x in (float("nan"), float("inf"))] == [-1, -1] and [km(b=x) for x in (0.0, -1.0, float("nan"))] == [-1] * 3
    assert km(n1=-1) == -1 and km(ldx=64) == -1 and km(ldk=2) == -1 and km(n1=0) == 0 and km(n1=0, d=1024) == 0
    assert lib.gpk_wide_arc_kernel_matrix_combine(None, 1, 3, a, 3, 65, None, 0, 0, 65, a, 0, 1.0, 1.0, 0.0, a, 3, a, 3) == -1
    assert lib.gpk_wide_arc_kernel_diag(None, 1, 4, a, 3, 65, 65, a, 0, 1.0, 1.0, a, a) == -1
    assert lib.gpk_wide_arc_kernel_diag(None, 1, 1, a, 3, 65, 65, a, 0, 1.0, 1.0, None, a) == -1
    assert stage(6) == -1 and stage(6, order=3) == -3 and stage(0, n1=0) == 0
    assert tail(plen=6) == -1 and tail(slen=65) == -1 and tail(ldr=65) == -1 and tail(n1=0) == 0
