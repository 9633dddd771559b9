"""kernels.Convolutional over InducingPatches on the device: the patch-response kernels of csrc/conv/conv.hip (ops.conv_*) against a
plain reference that unfolds every patch on the CPU, then the SVGP routes built on them.

Reference: patches by the layout rule of include/gpk.h, the DIFFERENCE form of the squared distance in np.longdouble, the sums as
written there; gradients from torch fp64 autograd over the same formulas.

Bound of Kfu / K_diag, element-wise, u = 2^-53.  The device forms r2 = (|z~|^2 + |x~|^2) - 2 z~.x~ on inputs divided by the
lengthscale: its error is (patch_len + 3) u (|z~|^2 + |x~|^2); |dk/dr2| <= v / 2; the exp, the product with w_p and the scale are four
roundings per term (4 u |term|), and the fixed-order sum of T terms adds T u sum |term|.  Nothing in it is tuned to the device.
M = 65 crosses the kernel's block of 64 inducing patches (GPK_CONV_MBLOCK); P crosses the 16-patch tile at 25 and 40."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_contract import LD, U, _np, _same_bits  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402

GRAD_TOL = 1e-8   # tests/test_gpu_dot_kernels.py: relative to the norm of the reference gradient
GEOMETRIES = [(5, 4, 1, 2, 3), (7, 6, 2, 3, 3), (9, 9, 1, 5, 5), (4, 4, 1, 4, 4), (3, 5, 3, 1, 1)]
V = 1.7
_CASES = {}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _unfold(X, geo):
    """[N, P, h w]: channel, window row, window column; numpy or torch"""
    H, W, C, h, w = geo
    X = X.reshape(-1, H, W, C)
    rows = [X[:, i:i + h, j:j + w, c].reshape(X.shape[0], h * w) for c in range(C) for i in range(H - h + 1) for j in range(W - w + 1)]
    return (torch if torch.is_tensor(X) else np).stack(rows, 1)


def _reference(X, Z, wts, ls, geo):
    """(Kfu, K_diag, their bounds) in longdouble"""
    Xp, Zl, w = _unfold(X, geo).astype(LD), Z.astype(LD), wts.astype(LD)
    P, plen = Xp.shape[1], Xp.shape[2]
    e = LD(V) * np.exp(-((Xp[:, :, None, :] - Zl[None, None]) ** 2).sum(-1) / LD(ls) ** 2 / 2)             # [N, P, M]
    Kfu = (w[None, :, None] * e).sum(1) / P
    xn, zn = (Xp ** 2).sum(-1) / LD(ls) ** 2, (Zl ** 2).sum(-1) / LD(ls) ** 2
    aw = np.abs(w)[None, :, None]
    bfu = U * ((aw * (LD(V) / 2 * (plen + 3) * (xn[:, :, None] + zn[None, None]) + 4 * e)).sum(1) + P * (aw * e).sum(1)) / P
    k = LD(V) * np.exp(-((Xp[:, :, None, :] - Xp[:, None, :, :]) ** 2).sum(-1) / LD(ls) ** 2 / 2)          # [N, P, P]
    k[:, np.arange(P), np.arange(P)] = LD(V)
    ww = w[:, None] * w[None, :]
    Kd = (ww[None] * k).sum((1, 2)) / P ** 2
    off = 1 - np.eye(P)
    bd = U * ((np.abs(ww)[None] * (off * LD(V) / 2 * (plen + 3) * (xn[:, :, None] + xn[:, None, :]) + 4 * k)).sum((1, 2))
              + P * P * (np.abs(ww)[None] * k).sum((1, 2))) / P ** 2
    return Kfu, Kd, bfu, bd


def _case(geo, N=70, M=65):
    """one problem per geometry at the largest N and M, shared: the smaller cases are its leading rows"""
    if geo not in _CASES:
        H, W, C, h, w = geo
        rng = np.random.default_rng(sum(geo))
        P = C * (H - h + 1) * (W - w + 1)
        wts = rng.uniform(0.5, 1.5, size=P)
        if P > 1:   # (P = 1 keeps its one weight: K_diag = w_0^2 v)
            wts[0], wts[-1] = 0.0, -0.7
        X, Z = rng.uniform(size=(N, H * W * C)), rng.uniform(size=(M, h * w))
        ls = 0.8 * np.sqrt(h * w)
        _CASES[geo] = (X, Z, wts, ls)
    return _CASES[geo]


def _kw(geo, wts, ls):
    return dict(geometry=geo, weights=wts, variance=V, lengthscales=ls)


@pytest.mark.parametrize("M", [1, 17, 65])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_kfu_and_kdiag(gp, geo, N, M):
    ops = gp.ops
    X, Z, wts, ls = _case(geo)
    X, Z = X[:N], Z[:M]
    Kfu, Kd, bfu, bd = _reference(X, Z, wts, ls, geo)
    Xd, Zd = ops.to_device(X), ops.to_device(Z)
    buf = torch.full((N + 1, M + 3), -7.0, dtype=torch.float64, device=Xd.device)   # padded ld, a guard row
    got = ops.conv_kfu(Xd, Zd, out=buf[:N, :M], **_kw(geo, wts, ls))
    kd = ops.conv_kdiag(Xd, **_kw(geo, wts, ls))
    r_fu, r_d = np.abs(_np(got).astype(LD) - Kfu) / bfu, np.abs(_np(kd).astype(LD) - Kd) / bd
    print(f"conv {geo} N={N} M={M}: worst error / bound  Kfu {float(r_fu.max()):.3f}  K_diag {float(r_d.max()):.3f}")
    assert (r_fu <= 1).all() and (r_d <= 1).all()
    assert bool((buf[N] == -7.0).all()) and bool((buf[:, M:] == -7.0).all())
    assert _same_bits(_np(ops.conv_kfu(Xd, Zd, **_kw(geo, wts, ls))), _np(got)) and _same_bits(_np(ops.conv_kdiag(Xd, **_kw(geo, wts, ls))), _np(kd))
    if wts.size == 1:
        assert (_np(kd) == wts[0] ** 2 * V).all()


@pytest.mark.parametrize("bad,shift", [(np.nan, 0.0), (np.inf, 0.0), (np.inf, -1.0)])
def test_nonfinite_pixel_marks_its_own_image(gp, bad, shift):
    """shift -1: every inducing patch negative, so z.x = -Inf and r2 = +Inf at the Inf pixel -- exp alone would give a finite 0"""
    ops, geo = gp.ops, (7, 6, 2, 3, 3)
    X, Z, wts, ls = _case(geo)
    X, Zd = X[:3].copy(), ops.to_device(Z[:17] + shift)
    both = lambda: [_np(ops.conv_kfu(ops.to_device(X), Zd, **_kw(geo, wts, ls))), _np(ops.conv_kdiag(ops.to_device(X), **_kw(geo, wts, ls)))]  # noqa: E731
    clean = both()
    X[1, 40] = bad
    for c, g in zip(clean, both()):
        assert (~np.isfinite(g[1])).all() and _same_bits(g[[0, 2]], c[[0, 2]])


def _torch_kfu_kdiag(X, Z, w, v, ls, geo):
    Xp = _unfold(X, geo)
    P = Xp.shape[1]
    Kfu = (w[None, :, None] * v * torch.exp(-((Xp[:, :, None, :] - Z[None, None]) ** 2).sum(-1) / ls ** 2 / 2)).sum(1) / P
    d2 = ((Xp[:, :, None, :] - Xp[:, None, :, :]) ** 2).sum(-1) / ls ** 2
    k = torch.where(torch.eye(P, dtype=torch.bool)[None], v * torch.ones_like(d2), v * torch.exp(-d2 / 2))
    return Kfu, (w[None, :, None] * w[None, None, :] * k).sum((1, 2)) / P ** 2


@pytest.mark.parametrize("M", [1, 17, 65])
@pytest.mark.parametrize("N", [1, 3, 70])
@pytest.mark.parametrize("geo", GEOMETRIES)
def test_adjoints(gp, geo, N, M):
    ops = gp.ops
    X, Z, wts, ls = _case(geo)
    X, Z = X[:N], Z[:M]
    rng = np.random.default_rng(N + M)
    G, c = rng.normal(size=(N, M)), rng.normal(size=N)
    lv = {"Z": _leaf(Z), "w": _leaf(wts), "v": _leaf(V), "ls": _leaf(ls)}
    Kfu, Kd = _torch_kfu_kdiag(_t(X), lv["Z"], lv["w"], lv["v"], lv["ls"], geo)
    ref_fu = torch.autograd.grad((Kfu * _t(G)).sum(), [lv["v"], lv["ls"], lv["Z"], lv["w"]])
    ref_d = torch.autograd.grad((Kd * _t(c)).sum(), [lv["v"], lv["ls"], lv["w"]])
    Xd, Zd = ops.to_device(X), ops.to_device(Z)
    got_fu = ops.conv_kfu_adjoint(Xd, Zd, ops.to_device(G), **_kw(geo, wts, ls))
    got_d = ops.conv_kdiag_adjoint(Xd, ops.to_device(c), **_kw(geo, wts, ls))
    for name, g, r in zip(["dv", "dls", "dZ", "dw", "diag dv", "diag dls", "diag dw"], got_fu + got_d, ref_fu + ref_d):
        _close(f"conv {geo} {name}", _np(g).reshape(-1), r.numpy().reshape(-1), GRAD_TOL)
    assert _np(got_fu[3])[0] != 0.0 and _np(got_d[2])[0] != 0.0   # d/dw of the zero-weight patch
    again = ops.conv_kfu_adjoint(Xd, Zd, ops.to_device(G), **_kw(geo, wts, ls)) + ops.conv_kdiag_adjoint(Xd, ops.to_device(c), **_kw(geo, wts, ls))
    assert all(_same_bits(_np(a), _np(b)) for a, b in zip(again, got_fu + got_d))


# ---- models: (7, 6, 2, 3, 3), N = 70, M = 17, two latents, num_data set ------------------------------------------------------------
GEO = (7, 6, 2, 3, 3)


def _model(gp, lik, *, whiten=True, q_diag=False):
    X, Z, wts, ls = _case(GEO)
    Z = Z[:17].copy()
    rng = np.random.default_rng(5)
    q_mu = 0.3 * rng.normal(size=(17, 2))
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(17, 17))) + 0.6 * np.eye(17) for _ in range(2)])
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    kern = gp.kernels.Convolutional(gp.kernels.SquaredExponential(variance=V, lengthscales=ls), GEO[:2], GEO[3:], weights=wts, colour_channels=2)
    m = gp.models.SVGP(kern, lik, gp.inducing_variables.InducingPatches(Z), q_mu=q_mu, q_sqrt=q_sqrt, q_diag=q_diag, whiten=whiten,
                       num_latent_gps=2, num_data=1000, mean_function=gp.mean_functions.Constant(0.1))
    return m, X, Z, q_mu, q_sqrt


def _elbo_from_cov(Kmm, Kmn, kd, q_mu, q_sqrt, mean, Y, *, whiten, noise, num_data=1000, jitter=1e-6):
    """(ELBO, fmean, fvar [B, P]) of svgp.py:166-181 from GIVEN covariances, torch fp64: conditionals/util.py:67-167, gauss_kl
    (kullback_leiblers.py:98-165), then the Gaussian term, or -- noise None -- the Bernoulli one (probit link with its 1e-3 jitter,
    hermgauss(20))"""
    M, P, B = Kmm.shape[0], q_mu.shape[1], Kmn.shape[1]
    Lm = torch.linalg.cholesky(Kmm + jitter * torch.eye(M, dtype=torch.float64))
    A = torch.linalg.solve_triangular(Lm, Kmn, upper=False)
    fvar = kd - (A * A).sum(0)
    if not whiten:
        A = torch.linalg.solve_triangular(Lm.T, A, upper=True)
    fmean = A.T @ q_mu + mean
    Lq = torch.diag_embed(q_sqrt.T) if q_sqrt.dim() == 2 else torch.tril(q_sqrt)                     # [P, M, M]
    LTA = Lq.transpose(1, 2) @ A
    fvar = (fvar[None] + (LTA * LTA).sum(1)).T
    alpha = q_mu if whiten else torch.linalg.solve_triangular(Lm, q_mu, upper=False)
    LiLq = Lq if whiten else torch.linalg.solve_triangular(Lm.expand(P, M, M), Lq, upper=False)
    kl = 0.5 * ((alpha * alpha).sum() - M * P - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (LiLq * LiLq).sum())
    if not whiten:
        kl = kl + 0.5 * P * torch.log(torch.diagonal(Lm) ** 2).sum()
    if noise is not None:
        ve = -0.5 * np.log(2 * np.pi) - 0.5 * torch.log(noise) - 0.5 * ((Y - fmean) ** 2 + fvar) / noise
    else:
        x, w = np.polynomial.hermite.hermgauss(20)
        f = fmean[..., None] + torch.sqrt(2 * fvar)[..., None] * torch.tensor(x)
        p = 0.5 * (1 + torch.special.erf(f / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
        ve = (torch.log(torch.where(Y[..., None] == 1, p, 1 - p)) * torch.tensor(w / np.sqrt(np.pi))).sum(-1)
    return ve.sum() * (num_data / B) - kl, fmean, fvar


@pytest.mark.parametrize("lik,whiten,q_diag", [("gaussian", True, False), ("gaussian", True, True), ("gaussian", False, False),
                                               ("gaussian", False, True), ("bernoulli", True, False)])
def test_svgp_elbo_grad_and_predict(gp, lik, whiten, q_diag):
    """Value and predict_f against the ELBO of the LONGDOUBLE Kuu / Kuf / K_diag; gradients against autograd of the same ELBO over
    the torch form of the covariances"""
    gauss = lik == "gaussian"
    m, X, Z, q_mu, q_sqrt = _model(gp, gp.likelihoods.Gaussian(0.2) if gauss else gp.likelihoods.Bernoulli(), whiten=whiten, q_diag=q_diag)
    Y = np.sin(X[:, :2] * 3.0) + 0.1 if gauss else (X[:, :2] > 0.5).astype(np.float64)
    kern = m.kernel
    pars = {"v": kern.base_kernel.variance, "ls": kern.base_kernel.lengthscales, "w": kern.weights}
    lv = {k: _leaf(p.numpy()) for k, p in pars.items()}
    lv.update({k: _leaf(a) for k, a in {"Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.1, "noise": 0.2}.items()})
    Kfu, kd = _torch_kfu_kdiag(_t(X), lv["Z"], lv["w"], lv["v"], lv["ls"], GEO)
    Kuu = lv["v"] * torch.exp(-((lv["Z"][:, None, :] - lv["Z"][None]) ** 2).sum(-1) / lv["ls"] ** 2 / 2)
    Fo, _, _ = _elbo_from_cov(Kuu, Kfu.T, kd, lv["q_mu"], lv["q_sqrt"], lv["mean"], _t(Y), whiten=whiten, noise=lv["noise"] if gauss else None)
    Fo.backward()
    _, _, wts, ls = _case(GEO)
    Kfu_ld, kd_ld, _, _ = _reference(X, Z, wts, ls, GEO)
    Zl = Z.astype(LD)
    Kuu_ld = LD(V) * np.exp(-((Zl[:, None, :] - Zl[None]) ** 2).sum(-1) / LD(ls) ** 2 / 2)
    f64 = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))   # noqa: E731
    with torch.no_grad():
        ref, fmean, fvar = _elbo_from_cov(f64(Kuu_ld), f64(Kfu_ld).T, f64(kd_ld), _t(q_mu), _t(q_sqrt), 0.1, _t(Y), whiten=whiten,
                                          noise=torch.tensor(0.2, dtype=torch.float64) if gauss else None)
    ref = float(ref)
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - ref) <= 1e-8 * abs(ref) and abs(float(m.elbo((X, Y)).cpu()) - ref) <= 1e-8 * abs(ref)
    allp = dict(pars, Z=m.inducing_variable.Z, q_mu=m.q_mu, mean=m.mean_function.c, **({"noise": m.likelihood.variance} if gauss else {}))
    _check_model_grads("conv svgp " + lik, g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values()) | {m.q_sqrt}
    if q_diag:
        _check_model_grads("conv svgp", g, {"q_sqrt": m.q_sqrt}, lv, GRAD_TOL)
    else:
        want = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
        _close("conv svgp q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(want).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)
    # predict_f, fused and cached, against each other and against the reference's moments
    for mu, var in (m.predict_f(X), m.posterior().predict_f(X)):
        assert np.abs(_np(mu) - fmean.numpy()).max() <= 1e-8 * np.abs(fmean.numpy()).max()
        assert np.abs(_np(var) - fvar.numpy()).max() <= 1e-8 * np.abs(fvar.numpy()).max()


def test_bernoulli_training_moves_weights_patches_and_lengthscale(gp):
    m, X, _, _, _ = _model(gp, gp.likelihoods.Bernoulli())
    Y = (X[:, :2] > 0.5).astype(np.float64)
    kern = m.kernel
    before = float(m.elbo((X, Y)).cpu())
    w0, Z0, l0 = kern.weights.numpy().copy(), m.inducing_variable.Z.numpy().copy(), float(kern.base_kernel.lengthscales.numpy())
    gp.optimizers.Scipy().minimize(m, (X, Y), options=dict(maxiter=10))
    assert float(m.elbo((X, Y)).cpu()) > before
    assert np.abs(kern.weights.numpy() - w0).max() > 0 and np.abs(m.inducing_variable.Z.numpy() - Z0).max() > 0
    assert float(kern.base_kernel.lengthscales.numpy()) != l0


def _refusals(gp):
    K, se = gp.kernels, gp.kernels.SquaredExponential
    conv = lambda **kw: K.Convolutional(se(), [7, 6], [3, 3], **kw)   # noqa: E731
    Z = np.zeros((4, 9))
    return {
        "matern base": (NotImplementedError, lambda: K.Convolutional(K.Matern32(), [7, 6], [3, 3])),
        "ard base": (NotImplementedError, lambda: K.Convolutional(se(lengthscales=np.ones(9)), [7, 6], [3, 3])),
        "active_dims base": (NotImplementedError, lambda: K.Convolutional(se(active_dims=[0, 1]), [7, 6], [3, 3])),
        "sum base": (NotImplementedError, lambda: K.Convolutional(se() + se(), [7, 6], [3, 3])),
        "in a Sum": (NotImplementedError, lambda: conv() + se()),
        "in a Product": (NotImplementedError, lambda: se() * conv()),
        "in ChangePoints": (NotImplementedError, lambda: K.ChangePoints([conv(), se()], [0.5])),
        "SharedIndependent": (NotImplementedError, lambda: K.SharedIndependent(conv(), 2)),
        "SeparateIndependent": (NotImplementedError, lambda: K.SeparateIndependent([conv(), conv()])),
        "LinearCoregionalization": (NotImplementedError, lambda: K.LinearCoregionalization([conv()], np.ones((2, 1)))),
        "image too large": (ValueError, lambda: K.Convolutional(se(), [65, 64], [3, 3])),
        "patch too long": (ValueError, lambda: K.Convolutional(se(), [28, 28], [9, 8])),
        "patch taller than the image": (ValueError, lambda: K.Convolutional(se(), [4, 8], [5, 2])),
        "patch of height 0": (ValueError, lambda: K.Convolutional(se(), [4, 8], [0, 2])),
        "K(X, X2)": (NotImplementedError, lambda: conv().K(np.zeros((2, 42)))),
        "InducingPoints": (NotImplementedError, lambda: gp.covariances.Kuu(gp.inducing_variables.InducingPoints(Z), conv())),
        "patches with another kernel": (NotImplementedError, lambda: gp.covariances.Kuf(gp.inducing_variables.InducingPatches(Z), se(), np.zeros((2, 9)))),
        "natural gradients": (NotImplementedError, lambda: gp.models.reverse.svgp_routes(_model(gp, gp.likelihoods.Gaussian(0.2))[0], narrow=True)),
        "trainer": (NotImplementedError, lambda: gp.training.SVGPTrainer(_model(gp, gp.likelihoods.Gaussian(0.2))[0])),
        "regression route": (NotImplementedError, lambda: gp.models.reverse.CovarianceRoute(conv())),
    }


@pytest.mark.parametrize("which", ["matern base", "ard base", "active_dims base", "sum base", "in a Sum", "in a Product", "in ChangePoints",
                                   "SharedIndependent", "SeparateIndependent", "LinearCoregionalization", "image too large", "patch too long",
                                   "patch taller than the image", "patch of height 0", "K(X, X2)", "InducingPoints",
                                   "patches with another kernel", "natural gradients", "trainer", "regression route"])
def test_refusals(gp, which, monkeypatch):
    """every refusal is raised before the library is entered: its loader is made to fail"""
    def no_device(*a, **k):
        raise AssertionError("the device library was entered before the refusal")
    monkeypatch.setattr(gp._lib, "load", no_device)
    exc, call = _refusals(gp)[which]
    with pytest.raises(exc):
        call()
