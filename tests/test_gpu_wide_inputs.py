"""GPU tests of the stationary builder on WIDE inputs, 65 .. 1024 active columns (gpflow_amd/csrc/wide/wide_stationary.hip behind
`ops.kernel_matrix`, `kernel_matrix_combine`, `kernel_matrix_hadamard`), the reverse pass and the model routes over it.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_wide_inputs_emulated.py), which never had a width limit:
there they hold the routing, not the kernel.  References: the longdouble expansion with delta = (d + 4) u (|a|^2 + |b|^2), which holds
for any summation order (`_kref`, `_kref_new`), autograd over `_torch_kernel`, and the oracle's torch forms at the tolerances of the
narrow model tests of tests/test_gpu_kernel_families.py (value 1e-9 relative, gradients 1e-8 by `_close`).
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle as orc  # noqa: E402  (checker only)
from oracle import gp_oracle_grad as orcg  # noqa: E402
from gpflow_amd.ops import kernel_matrix as _wrapper_kernel_matrix  # noqa: E402  (the wrappers themselves, whatever `gp.ops` holds)
from gpflow_amd.ops import kernel_matrix_combine as _wrapper_kernel_matrix_combine  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _kref, _np, _on, _within  # noqa: E402
from test_gpu_kernel_families import (_akw, _check_model_grads, _close, _data, _impls, _kref_new, _leaf, _ls, _t,  # noqa: E402
                                      _torch_kernel)

FAMS = [(f, None) for f in ("SquaredExponential", "Matern12", "Matern32", "Matern52", "Exponential")] + [("RationalQuadratic", 1.0)]


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _ref(family, X1, X2, variance, ls, alpha=None, op="k"):
    if family in ("Exponential", "RationalQuadratic"):
        return _kref_new(family, X1, X2, variance, ls, alpha, op)
    k, bnd, zero_ok = _kref(family, X1, X1 if X2 is None else X2, variance, ls, op)
    return k, bnd, (zero_ok & ~np.eye(X1.shape[0], dtype=bool)) if X2 is None else zero_ok


# (n1, n2 (None: symmetric), d, ard, data, layout, lower_only, diag_add).  The tile is a host-side function of (n1, n2, symmetric):
# 128 unless that grid has fewer workgroups than the device has compute units (256), so every row but the last runs the 64-tile.
KM_CASES = [
    (1, 1, 65, False, "far", "c", False, 0.0),            # first width past the narrow path: one full slab run + a one-column slab
    (63, 65, 80, True, "normal", "c", False, 0.0),        # d an exact slab multiple, 64-tile edges, ARD
    (127, 129, 130, True, "normal", "ld", False, 0.0),    # tile edges, ragged last slab, odd leading dimensions
    (130, None, 70, False, "dup", "c", False, 0.1),       # symmetric: mirrored tiles, the mirrored diagonal tile, near duplicates
    (257, None, 65, True, "normal", "c", True, 0.3),      # lower_only: the sentinel above the diagonal tiles stays
    (3, 2, 1024, False, "normal", "c", False, 0.0),       # the maximum width on one ragged tile
    (255, 257, 96, False, "far", "off", False, 0.0),      # cancellation data, misaligned base: scalar loads and stores
    (129, 16300, 65, False, "normal", "c", False, 0.0),   # 2 x 128 tiles of 128 = 256 workgroups: the 128-tile, vector stores, edges
]


@pytest.mark.parametrize("fam", FAMS, ids=[f for f, _ in FAMS])
@pytest.mark.parametrize("case", KM_CASES, ids=[str(c) for c in KM_CASES])
def test_wide_kernel_matrix(gp, case, fam):
    (family, alpha), (n1, n2, d, ard, data, layout, lower_only, diag_add) = fam, case
    X1, X2, _ = _data(n1 + 3 * d, n1, n2, d, data)
    ls = _ls(d, ard)
    k, bnd, _ = _ref(family, X1, X2, 1.7, ls, alpha)
    if X2 is None:
        k = k + diag_add * np.eye(n1, dtype=LD)
        bnd = bnd + U * np.abs(k)
    for who, impl, dev in _impls(gp):
        t1 = _on(X1, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        kw = dict(variance=1.7, lengthscales=ls, family=family, diag_add=diag_add, lower_only=lower_only, **_akw(alpha))
        sentinel = (lambda: _on(np.full(k.shape, -555.0), "c", dev)) if lower_only else (lambda: None)
        K = _np(impl.kernel_matrix(t1, t2, out=sentinel(), **kw))
        name = f"wide kernel_matrix {family} {who}"
        if lower_only:   # below the diagonal tiles: the sentinel, untouched; inside a diagonal tile: a correct value
            low = np.tril(np.ones(k.shape, dtype=bool))
            _within(name, np.where(low, K, 0), np.where(low, k, 0), np.where(low, bnd, 0))
            up = ~low & ~np.isnan(K) & (K != -555.0)
            _within(name + " upper", K[up], k[up], bnd[up])
            if dev != "cpu":   # (the emulation marks what is not written with NaN; no tile reaches 128 columns past the diagonal)
                assert np.all(K[np.triu_indices(n1, 128)] == -555.0), f"{name}: a strictly-upper tile was written"
        else:
            _within(name, K, k, bnd)
            if X2 is None and dev != "cpu":   # (the device's contract; the emulation's matmul does not give it)
                assert np.array_equal(K, K.T), f"{name}: not exactly symmetric"
        _check_unchanged(name, [t1] + ([t2] if t2 is not None else []), [X1] + ([X2] if X2 is not None else []))
        assert np.array_equal(K, _np(impl.kernel_matrix(t1, t2, out=sentinel(), **kw)), equal_nan=True), f"{name}: a second call differs"


def test_wide_symmetric_build_on_the_128_tile(gp):
    """2900 rows are 23 x 24 / 2 = 276 tiles of 128 on or below the diagonal: the symmetric 128-tile grid.  Its lower triangle has the
    bits of the cross build of the same rows (held to the reference by KM_CASES' last row), and the whole is exactly symmetric."""
    X = np.random.default_rng(11).normal(size=(2900, 65))
    tX = gp.ops.to_device(X)
    kw = dict(variance=1.1, lengthscales=0.9 * np.sqrt(65), family="Matern52")
    S, C = _np(gp.ops.kernel_matrix(tX, None, diag_add=0.25, **kw)), _np(gp.ops.kernel_matrix(tX, tX.clone(), **kw))
    assert np.array_equal(S, S.T) or str(gp.ops.device()) == "cpu"   # (as above)
    low = np.tril_indices(2900, -1)
    assert np.array_equal(S[low], C[low]) and np.array_equal(np.diag(S), np.diag(C) + 0.25)


KC_CASES = [(65, 63, 65, "ld"), (129, None, 130, "c")]
BIG = (129, 16300, 65, "c")   # the 128-tile (KM_CASES' last row): 16-byte reads of G, in place on full tiles; one family, the ops differ
KC_PAIRS = [(c, op, f) for c in KC_CASES for op in ("mul", "add", "dr2", "dalpha") for f in FAMS if op != "dalpha" or f[0] == "RationalQuadratic"] \
    + [(BIG, op, FAMS[-1]) for op in ("mul", "add", "dr2", "dalpha")]


@pytest.mark.parametrize("case,op,fam", KC_PAIRS, ids=[f"{c}-{op}-{f}" for c, op, (f, _) in KC_PAIRS])
def test_wide_kernel_matrix_combine(gp, case, op, fam):
    """the bounds of test_gpu_kernel_families.test_kernel_matrix_combine_new_families; `out` is G itself in a second call"""
    (family, alpha), (n1, n2, d, layout) = fam, case
    X1, X2, _ = _data(17 + n1 + d, n1, n2, d, "normal")
    G = np.random.default_rng(n1).normal(size=(n1, n1 if n2 is None else n2))
    ls, diag = _ls(d, False, 0.8), (0.2 if n2 is None else 0.0)
    k, bnd, zero_ok = _ref(family, X1, X2, 1.3, ls, alpha, op if op in ("dr2", "dalpha") else "k")
    g = G.astype(LD)
    if op in ("dr2", "dalpha"):
        ref, rb = k * g, bnd * np.abs(g) + U * np.abs(k * g)
        if X2 is None:
            np.fill_diagonal(ref, 0)
            np.fill_diagonal(rb, 0)
    else:
        ref = k * g if op == "mul" else k + g
        rb = (bnd * np.abs(g) if op == "mul" else bnd) + 2 * U * np.abs(ref)
        if X2 is None:
            ref = ref + diag * np.eye(n1, dtype=LD)
            rb = rb + U * np.abs(ref)
    for who, impl, dev in _impls(gp):
        t1, tG = _on(X1, layout, dev), _on(G, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        kw = dict(variance=1.3, lengthscales=ls, family=family, **_akw(alpha))
        R = _np(impl.kernel_matrix_combine(t1, t2, tG, op=op, diag_add=diag, **kw))
        name = f"wide kernel_matrix_combine {op} {family} {who}"
        if op in ("dr2", "dalpha") and X2 is None:
            assert np.all(np.diagonal(R) == 0), f"{name}: diagonal not exactly zero"
        _within(name, np.where(zero_ok & (R == 0), ref.astype(np.float64), R), ref, rb)
        _check_unchanged(name, [t1, tG], [X1, G])
        if op == "mul" and X2 is not None:
            _within(f"wide kernel_matrix_hadamard {family} {who}", _np(impl.kernel_matrix_hadamard(t1, t2, tG, **kw)), ref, rb)
        impl.kernel_matrix_combine(t1, t2, tG, op=op, diag_add=diag, out=tG, **kw)
        assert np.array_equal(_np(tG), R), f"{name}: in place differs"


@pytest.mark.parametrize("family", ["SquaredExponential", "Matern12"])
def test_wide_nan_row(gp, family):
    """one NaN in X at d = 70 makes exactly its row and column NaN: r2 is not clamped before sqrt sees it"""
    X = np.random.default_rng(4).normal(size=(70, 70))
    X[5, 66] = np.nan
    expect = (np.arange(70)[:, None] == 5) | (np.arange(70)[None, :] == 5)
    for who, impl, dev in _impls(gp):
        tX = _on(X, "c", dev)
        K = _np(impl.kernel_matrix(tX, None, variance=1.2, lengthscales=7.0, family=family))
        assert np.array_equal(np.isnan(K), expect), (who, family)
        D = _np(impl.kernel_matrix_combine(tX, _on(X[:9], "c", dev), _on(np.ones((70, 9)), "c", dev), op="dr2", variance=1.2, lengthscales=7.0,
                                           family=family))
        assert np.array_equal(np.isnan(D), expect[:, :9]), (who, family)


@pytest.mark.parametrize("sym", [True, False], ids=["symmetric", "cross"])
@pytest.mark.parametrize("d,ard", [(70, True), (130, False)])
@pytest.mark.parametrize("fam", [("SquaredExponential", None), ("Matern32", None), ("RationalQuadratic", 0.7)], ids=lambda f: f[0])
def test_wide_stationary_kernel_adjoint(gp, fam, d, ard, sym):
    """gradients.stationary_kernel_adjoint against autograd of sum(Kbar .* K) over the restated kernel"""
    family, alpha = fam
    rng, n1, n2 = np.random.default_rng(d), 40, 30
    A, B = rng.normal(size=(n1, d)), rng.normal(size=(n2, d))
    Kbar = rng.normal(size=(n1, n1 if sym else n2))
    Kbar = Kbar + Kbar.T if sym else Kbar   # (the symmetric form takes a symmetric seed)
    ls = np.sqrt(d) * (0.8 + 0.2 * np.arange(d) / d) if ard else 0.9 * np.sqrt(d)
    t, tA = gp.ops.to_device, gp.ops.to_device(A)
    dvar, dshape, Abar = gp.gradients.stationary_kernel_adjoint(gp.leaf.Leaf(family, 1.3, ls, **_akw(alpha)), tA, tA if sym else t(B),
                                                                t(Kbar), symmetric=sym)
    lv = {"variance": _leaf(1.3), "lengthscales": _leaf(ls), "A": _leaf(A), **({} if alpha is None else {"alpha": _leaf(alpha)})}
    K = _torch_kernel(family, lv["variance"], lv["lengthscales"], lv.get("alpha"))(lv["A"], lv["A"] if sym else _t(B))
    (K * _t(Kbar)).sum().backward()
    shape = np.concatenate([lv["lengthscales"].grad.numpy().reshape(-1)] + ([lv["alpha"].grad.numpy().reshape(-1)] if alpha is not None else []))
    _close(f"{family} variance", dvar, lv["variance"].grad.numpy().reshape(1), 1e-8)
    _close(f"{family} shape", dshape, shape, 1e-8)
    _close(f"{family} A_bar", Abar, lv["A"].grad.numpy(), 1e-8)


def _predict_ref(kfun, X, Y, Xn, noise):
    """GPR posterior at Xn from the restated kernel (gp_oracle.gpr_predict_f with any kfun)"""
    with torch.no_grad():
        tX, tXn = _t(X), _t(Xn)
        Kmm, Kmn, Knn = kfun(tX, tX).numpy(), kfun(tX, tXn).numpy(), np.diag(kfun(tXn, tXn).numpy())
    return orc.base_conditional_with_lm(Kmn, np.linalg.cholesky(orc.add_noise_cov(Kmm, noise)), Knn, Y, full_cov=False, q_sqrt=None, white=False)


@pytest.mark.parametrize("which", ["gpr", "svgp", "sgpr", "sum"])
def test_wide_models(gp, which):
    """value, every gradient and predict_f at five points against the oracle.  Inputs are normal and the lengthscales ~ 0.9 sqrt(d):
    the off-diagonal kernel entries sit near exp(-1.2), so K + noise I is far from the conditioning pre-check."""
    gpflow, K = gp, gp.kernels
    rng = np.random.default_rng(7)
    N, d, M = (50, 100, 8) if which == "svgp" else (40, 70, 6)
    D = d + 3 if which == "sum" else d
    X, Xn = rng.normal(size=(N, D)), rng.normal(size=(5, D))
    Y = np.sin(X[:, :3].sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, 1))
    Z = X[:M] + 0.05 * rng.normal(size=(M, D))
    family = "Matern32" if which == "svgp" else "SquaredExponential"
    ls = 0.9 * np.sqrt(d) if which == "svgp" else 0.9 * np.sqrt(d) * (1.0 + 0.2 * np.arange(d) / d)
    cols = list(range(3, D)) if which == "sum" else None
    kern = getattr(K, family)(variance=1.2, lengthscales=ls, active_dims=cols)
    pars, extra = {"variance": kern.variance, "lengthscales": kern.lengthscales}, {"noise": 0.2}
    if which == "sum":
        lin = K.Linear(variance=0.4, active_dims=[0, 1, 2])
        kern, pars = kern + lin, dict(pars, lin=lin.variance)

    def kf(lv):
        k0 = _torch_kernel(family, lv["variance"], lv["lengthscales"], cols=cols)
        return (lambda A, B: k0(A, B) + lv["lin"] * (A[:, :3] @ B[:, :3].T)) if which == "sum" else k0
    if which in ("gpr", "sum"):
        m = gpflow.models.GPR((X, Y), kern, noise_variance=0.2)
        (v, g), again = m.log_marginal_likelihood_and_grad(), m.log_marginal_likelihood
        oracle = lambda lv: orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], 0.0, kfun=kf(lv))  # noqa: E731
    elif which == "svgp":
        q_mu, q_sqrt = 0.2 * rng.normal(size=(M, 1)), np.tril(0.1 * rng.normal(size=(1, M, M))) + 0.5 * np.eye(M)
        m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_data=5 * N)
        (v, g), again = m.elbo_and_grad((X, Y)), lambda: m.elbo((X, Y))
        pars, extra = dict(pars, Z=m.inducing_variable.Z, q_mu=m.q_mu), dict(extra, Z=Z, q_mu=q_mu)
        oracle = lambda lv: orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], _t(q_sqrt), None, None, lv["noise"],  # noqa: E731
                                                 num_data=5 * N, kfun=kf(lv), kdiag=lv["variance"])
    else:
        m = gpflow.models.SGPR((X, Y), kern, Z.copy(), noise_variance=0.2)
        (v, g), again = m.objective_and_grad(), m.elbo
        pars, extra = dict(pars, Z=m.inducing_variable.Z), dict(extra, Z=Z)
        oracle = lambda lv: orcg.sgpr_elbo_torch(_t(X), _t(Y), lv["Z"], None, None, lv["noise"], jitter=gpflow.config.default_jitter(),  # noqa: E731
                                                 mean=0.0, kfun=kf(lv), kdiag=lv["variance"])
    pars["noise"] = m.likelihood.variance
    lv = {key: _leaf(extra[key] if key in extra else par.numpy()) for key, par in pars.items()}
    Fo = oracle(lv)
    Fo.backward()
    assert abs(v - float(Fo.detach())) <= 1e-9 * abs(float(Fo.detach())) and abs(v - float(again().cpu())) <= 1e-9 * abs(v)
    _check_model_grads(which, g, pars, lv)
    if which == "svgp":
        rm, rv = orc.svgp_predict_f(Xn, Z, q_mu, q_sqrt, variance=1.2, lengthscales=ls, whiten=True, kernel=family)
    elif which == "sgpr":
        rm, rv = orc.sgpr_predict_f(X, Y, Z, Xn, variance=1.2, lengthscales=ls, noise_variance=0.2, jitter=gpflow.config.default_jitter())
    else:
        rm, rv = _predict_ref(kf(lv), X, Y, Xn, 0.2)
    mu, var = m.predict_f(Xn)
    _close(f"{which} predict mean", mu, np.asarray(rm).reshape(5, 1), 1e-8)
    _close(f"{which} predict variance", var, np.asarray(rv).reshape(5, 1), 1e-8)


def test_wide_refusals_and_unchanged_ground(gp):
    """d = 1025 is a ValueError before the device; the narrow C entry points still answer GPK_E_ARG at d = 65; the wide ones refuse
    White / Constant, op 4 for a family without alpha and an alpha that is not positive, without a launch (host pointers in the slots);
    SVGPTrainer refuses a wide leaf; the dot-product builder keeps its limit."""
    from gpflow_amd import _lib, training
    big = torch.zeros((2, 1025), dtype=torch.float64)   # (a host tensor: the width is refused before anything asks where it lives)
    with pytest.raises(ValueError, match="64.*1024"):
        _wrapper_kernel_matrix(big, None, variance=1.0, lengthscales=1.0)
    with pytest.raises(ValueError, match="64.*1024"):
        _wrapper_kernel_matrix_combine(big, None, torch.zeros((2, 2), dtype=torch.float64), op="mul", variance=1.0, lengthscales=1.0)
    with pytest.raises((ValueError, AssertionError)):
        gp.ops.dot_kernel_matrix(_on(np.zeros((2, 65)), "c", str(gp.ops.device())), None, variance=1.0)
    lib = _lib.load()
    buf = (ctypes.c_double * 4096)()
    addr, one = ctypes.cast(buf, ctypes.c_void_p).value, _lib.host_doubles([1.0] * 66)
    assert lib.gpk_kernel_matrix(None, 0, addr, 3, 65, None, 0, 0, 65, one, 0, 1.0, 0.0, 0, addr, 3) == -1
    assert lib.gpk_kernel_matrix_combine(None, 0, 1, addr, 3, 65, None, 0, 0, 65, one, 0, 1.0, 0.0, addr, 3, addr, 3) == -1
    assert lib.gpk_kernel_matrix_hadamard(None, 0, addr, 3, 65, addr, 3, 65, 65, one, 0, 1.0, addr, 3, addr, 3) == -1

    def wk(family=0, n1=3, d=65, alpha=1.0, ldx=None, ldk=3):
        return lib.gpk_wide_kernel_matrix(None, family, addr, n1, d if ldx is None else ldx, None, 0, 0, d, addr, 0, alpha, 1.0, 0.0, 0, addr, ldk)

    def wc(family=0, op=1, n1=3, alpha=1.0):
        return lib.gpk_wide_kernel_matrix_combine(None, family, op, addr, n1, 65, None, 0, 0, 65, addr, 0, alpha, 1.0, 0.0, addr, 3, addr, 3)
    assert [wk(f) for f in (6, 7, 8, -1)] == [-3] * 4 and [wc(f) for f in (6, 7)] == [-3, -3]
    assert [wc(f, op=4) for f in range(5)] == [-3] * 5 and [wc(op=op) for op in (0, 5)] == [-1, -1]
    assert [wk(5, alpha=a) for a in (0.0, -1.0, float("nan"), float("inf"))] == [-1] * 4 and wc(5, op=4, alpha=0.0) == -1
    assert wk(d=0) == -1 and wk(d=1025) == -1 and wk(n1=-1) == -1 and wk(ldx=64) == -1 and wk(ldk=2) == -1
    assert [wk(f, n1=0) for f in range(6)] == [0] * 6 and wc(5, op=4, n1=0) == 0 and wk(n1=0, d=1024) == 0     # nothing to do: no launch
    X = np.random.default_rng(0).normal(size=(20, 70))
    sv = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=7.0), gp.likelihoods.Gaussian(0.1), X[:4].copy(), num_data=20)
    with pytest.raises(NotImplementedError, match="64"):
        training.SVGPTrainer(sv)
