"""GPU tests of the Periodic kernel: the three primitives of gpflow_amd/csrc/periodic.hip (`ops.periodic_warp`, `periodic_moment_rows`,
`periodic_adjoint_tail`), the kernel matrix through the warp, and `kernels.Periodic` on every model route of the reverse pass.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_periodic_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py, with tests/fake_periodic_ops.py for the three primitives
here).  On the device every primitive case also runs the emulation beside it (`_impls`).

References.  Primitives: np.longdouble restatements with bounds derived next to them (u = 2^-53).  The kernel matrix and the models
are compared with the DIRECT formula  k(sum_j sin^2(pi (x_j - x'_j) / p_j) / l_j^2) -- never with the warp: in longdouble for the
matrix, in torch under autograd (oracle/gp_oracle_grad.py through its `kfun=` hook) for the models.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_ops  # noqa: E402
import fake_periodic_ops  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _padding_untouched, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _kfun, _leaf, _svgp_problem, _t, _torch_kernel  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

PI = LD(np.pi) + LD(1.2246467991473532e-16)     # pi to longdouble: the fp64 value and the next term of its expansion
SINCOSPI_C = 4                                  # the bound on sincospi's own error, in units of u at |value| <= 1
VALUE_TOL, GRAD_TOL = 1e-9, 1e-8                # the project's figures for the families evaluated on r2 (test_gpu_kernel_families.py)


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


class _Emulation:
    """the emulated primitives under one roof: the builders of fake_ops, the three of fake_periodic_ops"""
    kernel_matrix = staticmethod(fake_ops.kernel_matrix)
    moment_rows = staticmethod(fake_ops.moment_rows)
    periodic_warp = staticmethod(fake_periodic_ops.periodic_warp)
    periodic_moment_rows = staticmethod(fake_periodic_ops.periodic_moment_rows)
    periodic_adjoint_tail = staticmethod(fake_periodic_ops.periodic_adjoint_tail)


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", _Emulation, "cpu")] if dev != "cpu" else [])


# ------------------------------------------------------------------------------------------------ 1. the warp
def _period(kind, d):
    """"half": one period 0.5 (k p exactly representable); "ard": p_j in {0.5, 1, 1.5, 2} (k p exact as well); "odd": one period 1.7"""
    return 0.5 if kind == "half" else 1.7 if kind == "odd" else 0.5 * (1 + np.arange(d) % 4)


def _warp_data(n, d, period, seed):
    """rows whose |x| / p cycles through 1, 1e2, 1e4, 1e6; from n >= 255 on, rows 0..3 are x = k p exactly, row 10 has a NaN in column
    0 and row 20 an Inf in the last column"""
    rng = np.random.default_rng(seed)
    p = np.broadcast_to(np.asarray(period, dtype=np.float64), (d,))
    X = rng.uniform(-1.0, 1.0, size=(n, d)) * p * (10.0 ** (2 * (np.arange(n) % 4)))[:, None]
    exact = np.zeros((n, d), dtype=bool)
    if n >= 255:
        X[:4] = rng.integers(-40, 41, size=(4, d)) * p
        X[3] *= 1000.0
        exact[:4] = True
        X[10, 0], X[20, d - 1] = np.nan, np.inf
    return X, p, exact


def _warp_ref(X, p):
    """(Phi in longdouble, bound): cos / sin(2 pi x / p) with the argument reduced exactly (fmod of the longdouble quotient) before pi
    enters.  Bound per element u (c + 2 pi |x / p|): the fp64 quotient 2 x / p carries one rounding, pi |delta q| <= 2 pi u |x / p|, and
    sincospi its own c u; + the reference's own 2^-63 (4 + 2 pi |x / p|)."""
    q = 2 * X.astype(LD) / p.astype(LD)
    with np.errstate(all="ignore"):
        r = np.fmod(q, LD(2))
        c, s = np.cos(PI * r), np.sin(PI * r)
        ratio = np.abs(X.astype(LD) / p.astype(LD))
    Phi = np.empty((X.shape[0], 2 * X.shape[1]), dtype=LD)
    Phi[:, 0::2], Phi[:, 1::2] = c, s
    bound = np.repeat(U * (SINCOSPI_C + 2 * PI * ratio) + LD(2.0) ** -63 * (4 + 2 * PI * ratio), 2, axis=1)
    return Phi, bound


WARP_CASES = [(n, d, kind) for n in (1, 255, 257) for d in (1, 3, 32) for kind in ("half", "ard", "odd")]


@pytest.mark.parametrize("n,d,kind", WARP_CASES)
def test_periodic_warp(gp, n, d, kind):
    period = _period(kind, d)
    X, p, exact = _warp_data(n, d, period, 100 * n + d)
    ref, bound = _warp_ref(X, p)
    bad = ~np.isfinite(X)
    finite = ~np.repeat(bad, 2, axis=1)
    for who, impl, dev in _impls(gp):
        tX = _on(X, "ld", dev)
        out, buf = _on(np.full((n, 2 * d), -555.0), "pad", dev, base=True)
        got = impl.periodic_warp(tX, period, out=out)
        assert got is out and _padding_untouched(out, buf), f"{who}: padding written"
        Phi = _np(out)
        name = f"periodic_warp {who}"
        assert np.array_equal(np.isnan(Phi), ~finite), f"{name}: a NaN / Inf entry of X must poison its own (cos, sin) pair and nothing else"
        _within(name, np.where(finite, Phi, 0), np.where(finite, ref, 0), np.where(finite, bound, 0))
        if kind != "odd":   # x = k p: exactly (1, 0)
            ex = np.repeat(exact & ~bad, 2, axis=1)
            want = np.tile([1.0, 0.0], d)[None, :] * np.ones((n, 1))
            assert np.array_equal(Phi[ex], want[ex]), f"{name}: x = k p is not exactly (1, 0)"
        _check_unchanged(name, [tX], [X])
        # what sincospi itself adds: the error against (cos, sin)(pi q) at the SAME fp64 quotient q (the figure recorded in DESIGN 6)
        with np.errstate(all="ignore"):
            own, _ = _warp_ref(np.where(bad, 0.0, 2.0 * X / p) / 2.0, np.ones(d))
        print(f"{name} n={n} d={d} {kind}: largest error of sincospi at the rounded quotient: "
              f"{float(np.max(np.abs(np.where(finite, Phi, 0).astype(LD) - np.where(finite, own, 0))) / U):.3f} u")
        assert np.array_equal(_np(impl.periodic_warp(tX.contiguous(), period)), Phi, equal_nan=True), f"{name}: allocated output differs"


@pytest.mark.parametrize("n,d,kind", [(n, d, kind) for n, d, kind in WARP_CASES if kind != "half"])
def test_periodic_moment_rows(gp, n, d, kind):
    """the first 1 + 4 D rows are moment_rows(periodic_warp(B)) bit for bit; the last 2 D are b cos, b sin (one product each: exact
    to the bit as well), interleaved as Phi is"""
    period = _period(kind, d)
    B, _, _ = _warp_data(n, d, period, 7 * n + d)
    B = np.where(np.isfinite(B), B, 0.25)
    for who, impl, dev in _impls(gp):
        tB = _on(B, "ld", dev)
        Vt = _np(impl.periodic_moment_rows(tB, period))
        Phi = impl.periodic_warp(tB.contiguous(), period)
        assert Vt.shape == (1 + 6 * d, n)
        assert np.array_equal(Vt[:1 + 4 * d], _np(impl.moment_rows(Phi))), f"{who}: moment rows of the warped inputs"
        assert np.array_equal(Vt[1 + 4 * d:], (np.repeat(B, 2, axis=1) * _np(Phi)).T), f"{who}: b cos / b sin rows"
        _check_unchanged(f"periodic_moment_rows {who}", [tB], [B])


# ------------------------------------------------------------------------------------------------ 2. the adjoint tail
TAIL_CASES = [(1, 1), (33, 3), (1025, 3), (1025, 32)]   # one row; d does not divide 1024; rows beyond one pass of 1024 / d; the cap


def _tail_problem(n1, d, symmetric, ard):
    rng = np.random.default_rng(13 * n1 + d + symmetric)
    period = (0.7 + 0.1 * np.arange(d)) if ard else 1.3
    ls = 0.6 + 0.05 * np.arange(d)
    X = rng.normal(size=(n1, d))
    Phi = _np(fake_periodic_ops.periodic_warp(torch.from_numpy(X), period))
    if symmetric:   # B is X, G symmetric with a zero diagonal (op "dr2" of K(X, X))
        G = rng.normal(size=(n1, n1))
        G = G + G.T
        np.fill_diagonal(G, 0.0)
        Bm = X
    else:
        Bm = rng.normal(size=(37, d))
        G = rng.normal(size=(n1, 37))
    R = G @ _np(fake_periodic_ops.periodic_moment_rows(torch.from_numpy(Bm), period)).T
    return X, Phi, rng.normal(size=(n1, 2 * d)), R, ls, period


def _tail_ref(X, Phi, Phibar, R, ls, period):
    """the two formulas of include/gpk.h in longdouble on the same fp64 inputs, and their forward-error bounds.
    X_bar_ij = w (c b_s - s b_c): two products, a difference, the factor w = 2 pi / p (two roundings) -- 6 u w (|c b_s| + |s b_c|).
    dperiod_j = f_j sum_i t_i, t_i = x (s gc - c gs) + (c gbs - s gbc): every t_i within 6 u T_i of its value, T_i the same expression
    with every product taken in magnitude; the sum of n1 terms in ANY order within (n1 - 1) u sum T_i; f_j = pi / (2 p^2 l^2) five
    roundings: (n1 + 16) u f_j sum_i T_i in all.  One period: the sum over j adds (d - 1) u of the summed bound's magnitude."""
    n1, d = X.shape
    p = np.broadcast_to(np.asarray(period, dtype=LD), (d,))
    x, l = X.astype(LD), ls.astype(LD)
    c, s, bc, bs = (a.astype(LD) for a in (Phi[:, 0::2], Phi[:, 1::2], Phibar[:, 0::2], Phibar[:, 1::2]))
    Rl = R.astype(LD)
    gc, gs, gbc, gbs = Rl[:, 1:1 + 2 * d:2], Rl[:, 2:2 + 2 * d:2], Rl[:, 1 + 4 * d::2], Rl[:, 2 + 4 * d::2]
    w = 2 * PI / p
    Xbar = w * (c * bs - s * bc)
    Xbar_bound = 6 * U * w * (np.abs(c * bs) + np.abs(s * bc)) + LD(1e-300)
    f = PI / (2 * p * p * l * l)
    dper = f * (x * (s * gc - c * gs) + (c * gbs - s * gbc)).sum(0)
    T = (np.abs(x) * (np.abs(s * gc) + np.abs(c * gs)) + np.abs(c * gbs) + np.abs(s * gbc)).sum(0)
    dper_bound = (n1 + 16) * U * f * T + LD(1e-300)
    if np.ndim(period) == 0:
        dper, dper_bound = dper.sum().reshape(1), (dper_bound.sum() + (d - 1) * U * (f * T).sum()).reshape(1)
    return dper, dper_bound, Xbar, Xbar_bound


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["cross", "symmetric"])
@pytest.mark.parametrize("n1,d", TAIL_CASES)
def test_periodic_adjoint_tail(gp, n1, d, symmetric, accumulate):
    ard = (n1 + d) % 2 == 0                                  # (1, 1) and (1025, 3): one period per column; the others: one period
    X, Phi, Phibar, R, ls, period = _tail_problem(n1, d, symmetric, ard)
    dper, dper_bound, Xbar, Xbar_bound = _tail_ref(X, Phi, Phibar, R, ls, period)
    rng = np.random.default_rng(n1)
    d0, X0 = rng.normal(size=dper.shape), rng.normal(size=X.shape)
    if accumulate:
        dper, Xbar = dper + d0, Xbar + X0
        dper_bound, Xbar_bound = dper_bound + U * np.abs(dper), Xbar_bound + U * np.abs(Xbar)
    for who, impl, dev in _impls(gp):
        ins = [_on(X, "c", dev), _on(Phi, "c", dev), _on(Phibar, "pad", dev), _on(R, "ld", dev)]
        tl = _on(ls, "c", dev)
        runs = []
        for _ in range(2):
            into = (_on(d0, "c", dev), _on(X0, "c", dev)) if accumulate else None
            got = impl.periodic_adjoint_tail(*ins, tl, period, into=into)
            if accumulate:
                assert got[0] is into[0] and got[1] is into[1]
            runs.append((_np(got[0]).copy(), _np(got[1]).copy()))
        name = f"periodic_adjoint_tail {who}"
        assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]), f"{name}: two runs differ"
        _within(name + " dperiod", runs[0][0], dper, dper_bound)
        _within(name + " X_bar", runs[0][1], Xbar, Xbar_bound)
        _check_unchanged(name, ins + [tl], [X, Phi, Phibar, R, ls])


# ------------------------------------------------------------------------------------------------ 3. the kernel matrix through the warp
def _periodic_kref(base, alpha, X1, X2, variance, ls, period):
    """K by the DIRECT formula in longdouble and the bound of the route through the warp.  The builder sees a = Phi(x) / (2 l): its
    Gram expansion moves r2 by delta_g = (2 d + 4) u (|a|^2 + |b|^2) (test_gpu_contract._kref at width 2 d), and |a|^2 = sum_j
    1 / (4 l_j^2) whatever x is.  The warp's own error e = u (c + 2 pi |x / p|) per entry moves pair j's chord |Phi_j(x) - Phi_j(x')| =
    2 |sin| by at most sqrt(2) (e_x + e_x'), hence r2 by sum_j (2 chord_j t_j + t_j^2) / (4 l_j^2), t_j = sqrt(2) (e_xj + e_x'j).
    k is monotone in r2: the interval k(r2 -+ delta) bounds it; + 8 u |k| for exp / the products and, RationalQuadratic, the
    4 (alpha + 1) log1p(u) u |k| of its exponent (test_gpu_kernel_families._kref_new)."""
    sym = X2 is None
    X2 = X1 if sym else X2
    d = X1.shape[1]
    p, l = np.broadcast_to(np.asarray(period, dtype=LD), (d,)), np.broadcast_to(np.asarray(ls, dtype=LD), (d,))
    dlt = X1.astype(LD)[:, None, :] - X2.astype(LD)[None, :, :]
    sn = np.sin(PI * np.fmod(dlt / p, LD(2)))
    r2 = ((sn / l) ** 2).sum(-1)
    na = (1 / (4 * l * l)).sum()
    e1, e2 = (U * (SINCOSPI_C + 2 * PI * np.abs(x.astype(LD) / p)) for x in (X1, X2))
    t = np.sqrt(LD(2)) * (e1[:, None, :] + e2[None, :, :])
    delta = (2 * d + 4) * U * 2 * na + ((2 * 2 * np.abs(sn) * t + t * t) / (4 * l * l)).sum(-1)
    fam = "RationalQuadratic"
    kf = (lambda r: variance * np.exp(-r / 2)) if base == "SE" else (lambda r: _kfun(fam, r, variance, alpha))
    k = kf(r2)
    bnd = np.maximum(np.abs(kf(np.maximum(r2 - delta, 0)) - k), np.abs(kf(r2 + delta) - k)) + 8 * U * np.abs(k) + LD(1e-300)
    if base == "RQ":
        bnd = bnd + 4 * (LD(alpha) + 1) * np.abs(np.log1p(r2 / (2 * LD(alpha)))) * U * np.abs(k)
    return k, bnd


def _base(K, base, variance=1.3, lengthscales=1.0, **kw):
    return K.SquaredExponential(variance=variance, lengthscales=lengthscales, **kw) if base == "SE" else \
        K.RationalQuadratic(variance=variance, lengthscales=lengthscales, alpha=0.7, **kw)


@pytest.mark.parametrize("symmetric", [False, True], ids=["65x63", "symmetric65"])
@pytest.mark.parametrize("base", ["SE", "RQ"])
def test_kernel_matrix_through_the_warp(gp, base, symmetric):
    """warp, then the unchanged builder with the device-form leaf (lengthscales 2 l, pairwise), against the direct sum of sin^2;
    K(x, x + k p) is the variance within the same bound; K_diag is the variance exactly"""
    K = gp.kernels
    rng = np.random.default_rng(5 + symmetric)
    ls, period = np.array([0.6, 0.9, 1.3]), np.array([0.5, 1.0, 1.5])
    X1 = rng.integers(-2 ** 21, 2 ** 21, size=(65, 3)) / 2.0 ** 20          # a grid on which x + k p is exact
    X2 = None
    if not symmetric:
        X2 = rng.integers(-2 ** 21, 2 ** 21, size=(63, 3)) / 2.0 ** 20
        X2[:10] = X1[:10] + rng.integers(-8, 9, size=(10, 3)) * period     # pair (i, i), i < 10: whole periods apart
    kern = K.Periodic(_base(K, base, 1.7, ls), period=period)
    leaf = kern.leaf()
    assert leaf.family == kern.base_kernel.family and np.array_equal(leaf.lengthscales, np.repeat(2 * ls, 2))
    k, bnd = _periodic_kref(base, 0.7, X1, X2, 1.7, ls, period)
    for who, impl, dev in _impls(gp):
        P1 = impl.periodic_warp(_on(X1, "ld", dev), period, out=_on(np.zeros((65, 6)), "ld", dev))
        P2 = None if symmetric else impl.periodic_warp(_on(X2, "ld", dev), period, out=_on(np.zeros((63, 6)), "pad", dev))
        Kd = _np(impl.kernel_matrix(P1, P2, out=_on(np.zeros(k.shape), "ld", dev), **leaf.keywords()))
        _within(f"periodic kernel matrix {base} {who}", Kd, k, bnd)
        if not symmetric:
            i = np.arange(10)
            assert np.all(np.abs(Kd[i, i].astype(LD) - LD(1.7)) <= bnd[i, i]), f"{who}: K(x, x + k p) is not the variance"
            assert np.all(bnd[i, i] < 1e-13)
    # the kernel object: every way in applies the warp once
    Kx = _np(kern(X1, X2))
    _within(f"Periodic.__call__ {base}", Kx, k, bnd)
    assert np.array_equal(Kx, _np(kern.K(gp.ops.to_device(X1), None if symmetric else gp.ops.to_device(X2))))
    kd = _np(kern(X1, full_cov=False))
    v = float(kern.variance.numpy())                                       # (what the Parameter's transform gives back for 1.7)
    assert kd.shape == (65,) and np.all(kd == v) and np.all(_np(kern.K_diag(X1)) == v) and abs(v - 1.7) < 1e-15


def test_the_warp_is_applied_once_on_every_route(gp):
    """k(X), k(X, X2), k.K on pre-sliced inputs, K_into on slice()'s output, inside a Sum, with active_dims on the base, and batched
    inputs: one matrix"""
    K, t = gp.kernels, gp.ops.to_device
    rng = np.random.default_rng(6)
    X, X2 = rng.normal(size=(40, 4)), rng.normal(size=(30, 4))
    kern = K.Periodic(K.SquaredExponential(variance=1.2, lengthscales=[0.8, 1.1], active_dims=[3, 1]), period=[1.5, 2.5])
    assert list(kern.active_dims) == [3, 1] and not kern.has_default_active_dims
    ref, bnd = _periodic_kref("SE", None, X[:, [3, 1]], X2[:, [3, 1]], 1.2, np.array([0.8, 1.1]), np.array([1.5, 2.5]))
    A = _np(kern(X, X2))
    _within("k(X, X2)", A, ref, bnd)
    assert np.array_equal(A, _np(kern.K(t(X[:, [3, 1]]), t(X2[:, [3, 1]]))))                       # pre-sliced
    assert np.array_equal(A, _np(kern(X[:, [3, 1]], X2[:, [3, 1]], presliced=True)))
    Xs, X2s = kern.slice(t(X), t(X2))
    assert tuple(Xs.shape) == (40, 4) and np.array_equal(A, _np(kern.K_into(Xs, X2s, None)))        # slice() warps: [n, 2 D]
    white = K.White(variance=0.3)
    S = _np((kern + white)(X, X2))                                                                  # Combination.K_into folds it in place
    assert np.array_equal(S, A)
    Ssym = _np((white + kern)(X))                                                                   # ... as a later member: the combine pass
    refs, bnds = _periodic_kref("SE", None, X[:, [3, 1]], None, 1.2, np.array([0.8, 1.1]), np.array([1.5, 2.5]))
    _within("White + Periodic", Ssym, refs + LD(0.3) * np.eye(40, dtype=LD), bnds + 2 * U * np.abs(refs + 0.3))
    P = _np((kern * K.Constant(2.0))(X, X2))
    _within("Periodic * Constant", P, 2 * ref, 2 * bnd + 2 * U * np.abs(2 * ref))
    Kb = _np(kern.K(t(X[:, [3, 1]]).reshape(2, 20, 2), t(X2[:, [3, 1]])))                           # batch dimensions as IsotropicStationary.K
    assert Kb.shape == (2, 20, 30) and np.array_equal(Kb.reshape(40, 30), A)
    assert np.all(_np((kern + white).K_diag(X)) == float(kern.variance.numpy()) + float(white.variance.numpy()))


# ------------------------------------------------------------------------------------------------ 4. models against autograd
def _direct(base, variance, ls, period, alpha=None, cols=None):
    """torch restatement of the DIRECT formula (gpflow/kernels/periodic.py over a base evaluated on r2): kfun(A, B)"""
    def kfun(A, B):
        if cols is not None:
            A, B = A[:, cols], B[:, cols]
        r2 = ((torch.sin(np.pi * (A[:, None, :] - B[None, :, :]) / period) / ls) ** 2).sum(-1)
        return variance * torch.exp(-0.5 * r2) if base == "SE" else variance * (1.0 + 0.5 * r2 / alpha) ** (-alpha)
    return kfun


# (lengthscales, period, active_dims) for inputs with D columns.  A Periodic kernel's lengthscale divides sin(.) in [-1, 1], not a
# distance between standard-normal inputs: r2 <= sum_j 1 / l_j^2 whatever the inputs are.  The lengthscales of _svgp_problem (about
# sqrt(D), sized for r2 ~ 2 D / l^2) would leave r2 < 1 everywhere -- a kernel between 0.6 and 1 whose Kuu over 200 points has a handful
# of eigenvalues above the jitter, so that the un-whitened ELBO's Kuu^-1 amplifies every rounding, the oracle's included, by
# 1 / jitter.  Sized for the sin instead.  The kernel lives on a torus: along dimension j two points decorrelate over
# |sin(pi delta / p)| ~ l, i.e. delta / p ~ l / pi, so the torus holds about prod_j (pi / l_j) independent cells whatever the
# periods are; `_ell` sizes l for about 110 cells over all D columns (D = 4: 0.97, D = 3: 0.66).  With these the REFERENCE's
# Kuu + jitter I over the 200 inducing points of _svgp_problem has a condition number of 9e4 (isotropic) and 1.2e5 (ARD), computed
# from the direct formula in NumPy.  Two active columns pack the same 200 points onto a 2-torus, where a squared-exponential
# Gram matrix degrades much faster: 1.7e7 (the jitter's floor) at l = 0.30, 4.9e5 at 0.20, 5e4 at 0.15.  The active_dims variant
# therefore takes l about 0.15, the conditioning of the other two variants.
# (Two earlier choices for the two active columns, [0.7, 0.55] and [0.33, 0.27], both at the jitter's floor, missed the 1e-8 bar in
#  the un-whitened full-q_sqrt case only: 3.4e-8 on dF/dZ (entries of 7e6) on the device, 1.2e-8 on dF/dperiod under the emulation.)
def _ell(d_active):
    return np.pi / 110.0 ** (1.0 / d_active)


def _variant(which, D):
    if which == "isotropic":
        return _ell(D), 1.7, None
    if which == "ard":
        return _ell(D) * (0.9 + 0.05 * np.arange(D)), 1.5 + 0.25 * np.arange(D), None
    return np.array([0.16, 0.14]), np.array([1.6, 2.1]), [D - 1, 0]                     # active_dims on the base


def _periodic_model_kernel(K, base, which, D):
    ls, period, dims = _variant(which, D)
    bk = _base(K, base, 1.3, ls, **({} if dims is None else {"active_dims": dims}))
    kern = K.Periodic(bk, period=period)
    pars = {"variance": bk.variance, "lengthscales": bk.lengthscales, "period": kern.period}
    if base == "RQ":
        pars["alpha"] = bk.alpha
    assert list(kern.trainable_parameters) == list(bk.trainable_parameters) + [kern.period]

    def torch_kernel(lv):
        return _direct(base, lv["variance"], lv["lengthscales"], lv["period"], lv.get("alpha"), dims)
    return kern, pars, torch_kernel


def _leaves(pars, extra):
    lv = {key: _leaf(par.numpy()) for key, par in pars.items()}
    lv.update({k: _leaf(v) for k, v in extra.items()})
    return lv


_REGRESSION = {}


def _regression_problem():
    if not _REGRESSION:
        rng = np.random.default_rng(53)
        N, M, D, P = 700, 130, 3, 2
        X = rng.normal(size=(N, D))
        _REGRESSION.update(X=X, Y=np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P)), Z=rng.normal(size=(M, D)))
    return _REGRESSION["X"], _REGRESSION["Y"], _REGRESSION["Z"]


def _agree(name, v, ref, fused):
    assert abs(v - ref) <= VALUE_TOL * abs(ref), (name, v, ref)
    assert abs(fused - v) <= VALUE_TOL * abs(v), (name, "fused against composed", fused, v)


@pytest.mark.parametrize("which", ["isotropic", "ard", "active_dims"])
@pytest.mark.parametrize("base", ["SE", "RQ"])
def test_periodic_gpr_and_sgpr_vs_autograd_oracle(gp, base, which):
    gpflow = gp
    X, Y, Z = _regression_problem()
    kern, pars, torch_kernel = _periodic_model_kernel(gpflow.kernels, base, which, X.shape[1])
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15)
    v, g = m.log_marginal_likelihood_and_grad()
    lv = _leaves(pars, {"noise": 0.15})
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], 0.0, kfun=torch_kernel(lv))
    Fo.backward()
    _agree("gpr", v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    _check_model_grads("gpr", g, dict(pars, noise=m.likelihood.variance), lv, GRAD_TOL)
    assert set(g) == set(pars.values()) | {m.likelihood.variance}
    s = gpflow.models.SGPR((X, Y), kern, Z.copy(), noise_variance=0.15)
    v, g = s.objective_and_grad()
    lv = _leaves(pars, {"noise": 0.15, "Z": Z})
    Fo = orcg.sgpr_elbo_torch(_t(X), _t(Y), lv["Z"], None, None, lv["noise"], jitter=1e-6, kfun=torch_kernel(lv), kdiag=lv["variance"])
    Fo.backward()
    _agree("sgpr", v, float(Fo.detach()), float(s.elbo().cpu()))
    _check_model_grads("sgpr", g, dict(pars, noise=s.likelihood.variance, Z=s.inducing_variable.Z), lv, GRAD_TOL)


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("which", ["isotropic", "ard", "active_dims"])
@pytest.mark.parametrize("base", ["SE", "RQ"])
def test_periodic_svgp_vs_autograd_oracle(gp, base, which, whiten, q_diag):
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt, _ = _svgp_problem()
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    kern, pars, torch_kernel = _periodic_model_kernel(gpflow.kernels, base, which, X.shape[1])
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, q_diag=q_diag, whiten=whiten,
                           num_latent_gps=q_mu.shape[1], num_data=1000)
    v, g = m.elbo_and_grad((X, Y))
    lv = _leaves(pars, {"noise": 0.2, "Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt})
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], lv["q_sqrt"], None, None, lv["noise"], num_data=1000, whiten=whiten,
                              kfun=torch_kernel(lv), kdiag=lv["variance"])
    Fo.backward()
    _agree("svgp", v, float(Fo.detach()), float(m.elbo((X, Y)).cpu()))
    assert m._fused_config() is not None
    _check_model_grads("svgp", g, dict(pars, noise=m.likelihood.variance, Z=m.inducing_variable.Z, q_mu=m.q_mu), lv, GRAD_TOL)
    if q_diag:
        _check_model_grads("svgp", g, {"q_sqrt": m.q_sqrt}, lv, GRAD_TOL)
    else:            # fill-triangular: the unconstrained vector holds the lower-triangular entries
        ref = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
        _close("svgp q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(ref).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)


@pytest.mark.parametrize("nested", [False, True], ids=["flat", "nested"])
def test_periodic_in_combinations(gp, nested):
    """Periodic(SE) * SE + White, and the same nested inside a Sum with an RQ over other columns, through GPR and whitened SVGP"""
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(31)
    N, D, M, P = 260, 3, 70, 2
    X = rng.normal(size=(N, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P))
    Z = X[:M] + 0.05 * rng.normal(size=(M, D))
    q_mu = 0.2 * rng.normal(size=(M, P))
    q_sqrt = np.tril(0.1 * rng.normal(size=(P, M, M))) + 0.5 * np.eye(M)
    pse = K.SquaredExponential(variance=1.2, lengthscales=[1.9, 2.1, 2.3])
    per = K.Periodic(pse, period=[1.5, 2.0, 2.5])
    se, wh = K.SquaredExponential(variance=0.9, lengthscales=1.4), K.White(variance=0.3)
    pars = {"p.variance": pse.variance, "p.lengthscales": pse.lengthscales, "p.period": per.period, "se.variance": se.variance,
            "se.lengthscales": se.lengthscales, "white.variance": wh.variance}
    kern = per * se + wh
    if nested:
        rq = K.RationalQuadratic(variance=0.6, lengthscales=0.9, alpha=1.7, active_dims=[0, 2])
        prq = K.Periodic(K.RationalQuadratic(variance=0.5, lengthscales=1.1, alpha=0.8, active_dims=[1]), period=1.9)
        pars.update({"rq.variance": rq.variance, "rq.lengthscales": rq.lengthscales, "rq.alpha": rq.alpha,
                     "prq.variance": prq.base_kernel.variance, "prq.lengthscales": prq.base_kernel.lengthscales,
                     "prq.alpha": prq.base_kernel.alpha, "prq.period": prq.period})
        kern = K.Product([K.Sum([per * se, wh]), K.Sum([rq, prq])])
        route = gpflow.models.reverse.CovarianceRoute(kern, D)
        assert route.spec.tree == ("mul", [("add", [("mul", [0, 1]), 2]), ("add", [3, 4])])
        assert [p is not None for p in route.spec.periods] == [True, False, False, False, True] and not route.spec.packable
        assert [len(m) for m in route.members] == [3, 2, 1, 3, 4]

    def torch_kernel(lv):
        k0 = _direct("SE", lv["p.variance"], lv["p.lengthscales"], lv["p.period"])
        k1 = _torch_kernel("SquaredExponential", lv["se.variance"], lv["se.lengthscales"])
        k2 = _torch_kernel("White", lv["white.variance"])
        first, kd = (lambda A, B: k0(A, B) * k1(A, B) + k2(A, B)), lv["p.variance"] * lv["se.variance"] + lv["white.variance"]
        if not nested:
            return first, kd
        k3 = _torch_kernel("RationalQuadratic", lv["rq.variance"], lv["rq.lengthscales"], lv["rq.alpha"], cols=[0, 2])
        k4 = _direct("RQ", lv["prq.variance"], lv["prq.lengthscales"], lv["prq.period"], lv["prq.alpha"], cols=[1])
        return (lambda A, B: first(A, B) * (k3(A, B) + k4(A, B))), kd * (lv["rq.variance"] + lv["prq.variance"])
    m = gpflow.models.GPR((X, Y[:, :1]), kern, noise_variance=0.2)
    v, g = m.log_marginal_likelihood_and_grad()
    lv = _leaves(pars, {"noise": 0.2})
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y[:, :1]), None, None, lv["noise"], 0.0, kfun=torch_kernel(lv)[0])
    Fo.backward()
    _agree("gpr", v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    _check_model_grads("gpr", g, dict(pars, noise=m.likelihood.variance), lv, GRAD_TOL)
    sv = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=P, num_data=5 * N)
    v, g = sv.elbo_and_grad((X, Y))
    lv = _leaves(pars, {"noise": 0.2, "Z": Z, "q_mu": q_mu})
    kfun, kd = torch_kernel(lv)
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], _t(q_sqrt), None, None, lv["noise"], num_data=5 * N, kfun=kfun, kdiag=kd)
    Fo.backward()
    _agree("svgp", v, float(Fo.detach()), float(sv.elbo((X, Y)).cpu()))
    _check_model_grads("svgp", g, dict(pars, noise=sv.likelihood.variance, Z=sv.inducing_variable.Z, q_mu=sv.q_mu), lv, GRAD_TOL)


def test_svgp_periodic_bernoulli(gp):
    """SVGP(Periodic(SE), Bernoulli): elbo on the fused quadrature shard, and elbo_and_grad against central differences of its own
    elbo at h = 1e-5 (the 1e-5 * max(1, |fd|) bar of test_gpu_gradients.py), the period among the parameters"""
    gpflow = gp
    rng = np.random.default_rng(8)
    N, D, M = 200, 2, 25
    X = rng.normal(size=(N, D))
    Y = (np.sin(2 * np.pi * X[:, :1] / 1.6) + 0.3 * rng.normal(size=(N, 1)) > 0).astype(np.float64)
    bk = gpflow.kernels.SquaredExponential(variance=1.2, lengthscales=[0.8, 1.1])
    k = gpflow.kernels.Periodic(bk, period=[1.5, 2.2])
    m = gpflow.models.SVGP(k, gpflow.likelihoods.Bernoulli(), X[:M].copy(), q_mu=0.2 * rng.normal(size=(M, 1)), num_data=N)
    assert k.period in m.trainable_parameters
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - float(m.elbo((X, Y)).cpu())) <= 1e-9 * abs(v) and np.isfinite(v)
    h = 1e-5
    for par, idx in [(k.period, (0,)), (k.period, (1,)), (bk.variance, ()), (bk.lengthscales, (1,)), (m.inducing_variable.Z, (3, 1)),
                     (m.q_mu, (4, 0))]:
        u0 = np.array(par.unconstrained_variable, dtype=np.float64, copy=True)
        vals = []
        for dlt in (h, -h):
            u = u0.copy()
            u[idx] += dlt
            par.assign_unconstrained(u)
            vals.append(float(m.elbo((X, Y)).cpu()))
        par.assign_unconstrained(u0)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(float(np.asarray(g[par])[idx]) - fd) <= 1e-5 * max(1.0, abs(fd)), (par.name, idx, float(np.asarray(g[par])[idx]), fd)


def test_separate_independent_declines_the_fused_shard_for_a_periodic_member(gp):
    """SeparateIndependent([Periodic(SE), SE]).elbo equals the sum of the two single-latent models at rtol 1e-10, whitened and not:
    the per-latent shards, which hand the builders raw inputs, were declined and the composed path ran"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    rng = np.random.default_rng(9)
    N, D, M, P = 150, 3, 40, 2
    X = rng.normal(size=(N, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P))
    Z = rng.normal(size=(M, D))
    q_mu = 0.2 * rng.normal(size=(M, P))
    q_sqrt = np.tril(0.1 * rng.normal(size=(P, M, M))) + 0.5 * np.eye(M)
    ks = [K.Periodic(K.SquaredExponential(variance=1.2, lengthscales=_ell(D)), period=1.7), K.SquaredExponential(variance=0.8, lengthscales=1.3)]
    for whiten in (True, False):
        m = gpflow.models.SVGP(K.SeparateIndependent(ks), gpflow.likelihoods.Gaussian(0.2), IV.SharedIndependentInducingVariables(
            IV.InducingPoints(Z.copy())), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=P, num_data=3 * N, whiten=whiten)
        assert m._fused_separate_config() is None and m._separate_stationary_members() is None
        total = 0.0
        for p, kp in enumerate(ks):
            one = gpflow.models.SVGP(kp, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu[:, p:p + 1], q_sqrt=q_sqrt[p:p + 1],
                                     num_latent_gps=1, num_data=3 * N, whiten=whiten)
            total += float(one.elbo((X, Y[:, p:p + 1])).cpu())
        got = float(m.elbo((X, Y)).cpu())
        assert abs(got - total) <= 1e-10 * abs(total), (whiten, got, total)


def test_scipy_moves_the_period(gp):
    """optimizers.Scipy on y = sin(2 pi x / 1.7) + noise from period = 1.5: the loss decreases, res.fun is the re-evaluated value, and
    the period moves (the form of test_scipy_moves_alpha)"""
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(10)
    X = rng.uniform(-4.0, 4.0, size=(150, 1))
    Y = np.sin(2 * np.pi * X / 1.7) + 0.1 * rng.normal(size=(150, 1))
    k = K.Periodic(K.SquaredExponential(), period=1.5)
    m = gpflow.models.GPR((X, Y), k, noise_variance=0.5)
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=5))
    after = -float(m.log_marginal_likelihood().cpu())
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert abs(float(k.period.numpy()) - 1.5) > 1e-3


def test_natural_gradient_narrow_route_takes_a_periodic_kernel(gp):
    """natural gradients on q(u) with a Periodic kernel: the narrow route of the reverse pass (one kernel over all columns, full
    q_sqrt) -- one step raises the ELBO"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt, _ = _svgp_problem()
    k = gpflow.kernels.Periodic(gpflow.kernels.SquaredExponential(variance=1.3, lengthscales=_ell(X.shape[1])), period=1.7)
    m = gpflow.models.SVGP(k, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2, num_data=1000)
    before = float(m.elbo((X, Y)).cpu())
    gpflow.optimizers.NaturalGradient(gamma=0.5).minimize(m, (X, Y))
    assert float(m.elbo((X, Y)).cpu()) > before


def test_periodic_refusals(gp):
    """before anything touches a device: a base evaluated on r (NotImplementedError naming the reason), the device-resident trainer,
    more than 32 active columns, a period of the wrong length; and, at the primitives, what the library refuses"""
    gpflow = gp
    K = gpflow.kernels
    for bad in (K.Matern12(), K.Matern32(), K.Matern52(), K.Exponential(), K.White(), K.SquaredExponential() + K.SquaredExponential()):
        with pytest.raises(NotImplementedError, match="r\\^2"):
            K.Periodic(bad)
    rng = np.random.default_rng(11)
    X, Y, Z = rng.normal(size=(30, 2)), rng.normal(size=(30, 1)), rng.normal(size=(8, 2))
    for k in (K.Periodic(K.SquaredExponential()), K.Periodic(K.SquaredExponential()) + K.SquaredExponential()):
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(gpflow.models.SVGP(k, gpflow.likelihoods.Gaussian(0.2), Z.copy()))
    wide = K.Periodic(K.SquaredExponential())
    X33 = rng.normal(size=(5, 33))
    for call in (lambda: wide(X33), lambda: wide(X33, full_cov=False), lambda: wide.slice(gpflow.ops.to_device(X33), None),
                 lambda: gpflow.models.GPR((X33, Y[:5]), wide).log_marginal_likelihood(),
                 lambda: gpflow.models.GPR((X33, Y[:5]), wide).log_marginal_likelihood_and_grad()):
        with pytest.raises(ValueError, match="2 D|columns"):
            call()
    with pytest.raises(ValueError, match="active_dims"):
        K.Periodic(K.SquaredExponential(active_dims=[0, 1]), period=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="period"):
        K.Periodic(K.SquaredExponential(lengthscales=[1.0, 2.0]), period=[1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="period"):
        K.Periodic(K.SquaredExponential(), period=[1.0, 2.0, 3.0])(X)
    with pytest.raises(Exception):
        K.Periodic(K.SquaredExponential(), period=-1.0)                                   # positive()
    for who, impl, dev in _impls(gp):
        tX = _on(X, "c", dev)
        for period in (0.0, -1.0, float("nan"), float("inf"), [1.0, 2.0, 3.0]):
            with pytest.raises(_refused()):
                impl.periodic_warp(tX, period)
            with pytest.raises(_refused()):
                impl.periodic_moment_rows(tX, period)
        with pytest.raises(_refused()):
            impl.periodic_warp(_on(X33, "c", dev), 1.0)
        assert tuple(impl.periodic_warp(tX[:0], 1.0).shape) == (0, 4) and tuple(impl.periodic_moment_rows(tX[:0], 1.0).shape) == (13, 0)
