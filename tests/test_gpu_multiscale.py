"""inducing_variables.Multiscale against the SquaredExponential on the device (csrc/multiscale/multiscale.hip): the Kfu / Kuu builders and
their adjoints against the formulas of kufs.py / kuus.py evaluated in np.longdouble on the same fp64 inputs, SVGP forward, reverse and
training against a torch-fp64 autograd restatement, and the refusals before the device.

Bounds, first order in u = 2^-53, per element (E = the exponent's sum, d columns; exp within 1 ulp = 2 u):
  Kfu: r = 1 / (l + s) carries 2 u (the sum, the division); t = (x - z) r 4 u, t^2 8 u, each fma term 9 u and the chain d u, so
       |dE| <= (d + 9) u E and exp(-E / 2) moves by (d + 9) u E / 2; c_m = v prod (l r): 4 u per column; exp 2 u, the product 1 u, the
       reference's own rounding 1 u:                                     |dK| <= ((d + 9) E / 2 + 4 d + 4) u |K|
  Kuu: a = (l + s)^2 3 u; den = (a + a') - l^2 has |d den| <= (4 (a + a') + l^2 + den) u <= 10 u den (den >= l^2, a + a' <= 2 den);
       q 11 u, D^2 3 u, each fma term 14 u and the chain d u; the product l^2 q: 14 u per column, halved by the root, which adds 1 u;
       v sqrt exp: exp 2 u, two products 2 u, the reference 1 u:         |dK| <= ((d + 14) E / 2 + 7 d + 6) u |K|
  kernel_matrix (scales = 0 comparison; the expansion |x|^2 + |y|^2 - 2 x.y on inputs divided by l): each of the three sums (d + 4) u of
       its magnitude, the two additions 2 u: |d r2| <= (d + 6) u (sx + sy + 2 sum |x y| / l^2), then 4 u as above.
  Adjoints: every entry is a sum of terms; with cK the largest coefficient above (+ 2 for Kbar .* K), n + M terms per sum and 4 d + 30
       for the closed-form factors, |d| <= (cK + n + M + 4 d + 30) u MAG, MAG the same closed form with every term replaced by its
       magnitude -- for Kfu in the MOMENT form the device uses, r^2 (sum |G| |x| + |z| sum |G|) and its second-moment analogue, which is
       where S1 - z S0 cancels."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_contract import LD, U, _np, _on, _same_bits  # noqa: E402
from test_gpu_convolutional import GRAD_TOL, _elbo_from_cov  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402

V = 1.7
_CASES = {}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _case(n, M, d, ard, wide=False):
    """(X, Z, S, ls) and the longdouble reference, computed once per shape"""
    key = (n, M, d, ard, wide)
    if key not in _CASES:
        rng = np.random.default_rng(n * 1000 + M + d)
        X, Z = rng.normal(size=(n, d)), rng.normal(size=(M, d))
        S = 10.0 ** rng.uniform(-6, 3, size=(M, d)) if wide else rng.uniform(0.05, 1.5, size=(M, d))
        ls = rng.uniform(0.8, 2.5, size=d) * np.sqrt(d) if ard else 1.3 * np.sqrt(d)
        _CASES[key] = (X, Z, S, ls, _ref(X, Z, S, ls))
    return _CASES[key]


def _ref(X, Z, S, ls):
    """Kfu, Kuu (no jitter) and their bounds, and the pieces the adjoints' closed forms reuse"""
    X, Z, S = X.astype(LD), Z.astype(LD), S.astype(LD)
    d = Z.shape[1]
    l = np.broadcast_to(np.asarray(ls, dtype=LD), (d,))
    r = 1 / (l + S)
    Dfu = X[:, None, :] - Z[None]
    Efu = ((Dfu * r[None]) ** 2).sum(-1)
    Kfu = LD(V) * np.prod(l * r, -1)[None] * np.exp(-Efu / 2)
    a = (l + S) ** 2
    q = 1 / (a[:, None] + a[None] - l ** 2)
    Duu = Z[:, None, :] - Z[None]
    Euu = (Duu ** 2 * q).sum(-1)
    Kuu = LD(V) * np.sqrt(np.prod(l ** 2 * q, -1)) * np.exp(-Euu / 2)
    cfu, cuu = (d + 9) * Efu / 2 + 4 * d + 4, (d + 14) * Euu / 2 + 7 * d + 6
    return dict(Kfu=Kfu, Kuu=Kuu, bfu=cfu * U * np.abs(Kfu), buu=cuu * U * np.abs(Kuu), cfu=cfu, cuu=cuu, l=l, r=r, q=q, Dfu=Dfu, Duu=Duu, a=a)


def _within(name, got, ref, bound):
    err = np.abs(_np(got).astype(LD) - ref)
    ratio = float((err / np.maximum(bound, LD(1e-300))).max()) if err.size else 0.0
    print(f"{name}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


@pytest.mark.parametrize("ard", [False, True])
@pytest.mark.parametrize("d", [1, 3, 64])
@pytest.mark.parametrize("n,M", [(1, 1), (63, 65), (65, 64), (130, 129)])
def test_builders(gp, n, M, d, ard):
    ops = gp.ops
    X, Z, S, ls, ref = _case(n, M, d, ard)
    kw = dict(variance=V, lengthscales=ls)
    Xd, Zd, Sd = _on(X), _on(Z), _on(S)
    rng = np.random.default_rng(3)
    G, Gu = rng.normal(size=(n, M)), rng.normal(size=(M, M))
    _within("Kfu", ops.multiscale_kfu(Xd, Zd, Sd, **kw), ref["Kfu"], ref["bfu"])
    _within("G .* Kfu", ops.multiscale_kfu(Xd, Zd, Sd, _on(G), op="mul", **kw), G * ref["Kfu"], np.abs(G) * ref["bfu"] + U * np.abs(G * ref["Kfu"]))
    _within("G + Kfu", ops.multiscale_kfu(Xd, Zd, Sd, _on(G), op="add", **kw), G + ref["Kfu"], ref["bfu"] + U * np.abs(G + ref["Kfu"]))
    Kuu = _np(ops.multiscale_kuu(Zd, Sd, diag_add=0.25, **kw))
    want = ref["Kuu"] + LD(0.25) * np.eye(M)
    _within("Kuu", Kuu, want, ref["buu"] + U * np.abs(want))
    assert _same_bits(Kuu, Kuu.T)
    diag = LD(V) * np.prod(ref["l"] / np.sqrt(2 * ref["a"] - ref["l"] ** 2), -1) + LD(0.25)
    _within("diag Kuu", np.diagonal(Kuu), diag, np.diagonal(ref["buu"]) + U * np.abs(diag))
    _within("G .* Kuu", ops.multiscale_kuu(Zd, Sd, _on(Gu), op="mul", **kw), Gu * ref["Kuu"], np.abs(Gu) * ref["buu"] + U * np.abs(Gu * ref["Kuu"]))


def test_builders_padded_misaligned_and_wide_scales(gp):
    """odd leading dimensions with a base that is 8- but not 16-byte aligned, in and out; scales over 1e-6 .. 1e3"""
    ops = gp.ops
    n, M, d = 65, 64, 3
    X, Z, S, ls, ref = _case(n, M, d, True, wide=True)
    kw = dict(variance=V, lengthscales=ls)
    Xd, Zd, Sd = _on(X, "off"), _on(Z, "ld"), _on(S, "ld")
    buf = torch.full((n * (M + 3) + 1,), 7.0, dtype=torch.float64, device="cuda")
    out = buf[1:].view(n, M + 3)[:, :M]
    _within("Kfu padded", ops.multiscale_kfu(Xd, Zd, Sd, out=out, **kw), ref["Kfu"], ref["bfu"])
    assert float(buf[0]) == 7.0 and bool((buf[1:].view(n, M + 3)[:, M:] == 7.0).all())
    bufu = torch.full((M * (M + 1) + 1,), 7.0, dtype=torch.float64, device="cuda")
    outu = bufu[1:].view(M, M + 1)[:, :M]
    _within("Kuu padded", ops.multiscale_kuu(Zd, Sd, out=outu, **kw), ref["Kuu"], ref["buu"])
    assert float(bufu[0]) == 7.0 and bool((bufu[1:].view(M, M + 1)[:, M:] == 7.0).all())


@pytest.mark.parametrize("d,ard", [(3, True), (64, False)])
def test_zero_scales_are_the_plain_kernel(gp, d, ard):
    ops = gp.ops
    n, M = 65, 64
    X, Z, _, ls, _ = _case(n, M, d, ard)
    ref = _ref(X, Z, np.zeros_like(Z), ls)
    kw = dict(variance=V, lengthscales=ls)
    Xd, Zd, Sd = _on(X), _on(Z), _on(np.zeros_like(Z))
    l = ref["l"]
    xs, zs = X.astype(LD) / l, Z.astype(LD) / l

    def rbf_bound(a, b, K):
        mag = (a * a).sum(-1)[:, None] + (b * b).sum(-1)[None] + 2 * np.abs(a[:, None, :] * b[None]).sum(-1)
        return ((d + 6) * mag / 2 + 4) * U * np.abs(K)
    _within("Kfu vs kernel_matrix", ops.multiscale_kfu(Xd, Zd, Sd, **kw), _np(ops.kernel_matrix(Xd, Zd, **kw)).astype(LD),
            ref["bfu"] + rbf_bound(xs, zs, ref["Kfu"]))
    _within("Kuu vs kernel_matrix", ops.multiscale_kuu(Zd, Sd, **kw), _np(ops.kernel_matrix(Zd, None, **kw)).astype(LD),
            ref["buu"] + rbf_bound(zs, zs, ref["Kuu"]))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_marks_its_own_row_or_column(gp, bad):
    ops = gp.ops
    n, M, d = 65, 64, 3
    X, Z, S, ls, _ = _case(n, M, d, True)
    kw = dict(variance=V, lengthscales=ls)
    Xb = X.copy()
    Xb[7, 1] = bad
    K = _np(ops.multiscale_kfu(_on(Xb), _on(Z), _on(S), **kw))
    assert np.isnan(K[7]).all() and np.isfinite(np.delete(K, 7, 0)).all()
    if np.isnan(bad):
        for which in ("z", "s"):
            Zb, Sb = Z.copy(), S.copy()
            (Zb if which == "z" else Sb)[5, 2] = bad
            K = _np(ops.multiscale_kfu(_on(X), _on(Zb), _on(Sb), **kw))
            assert np.isnan(K[:, 5]).all() and np.isfinite(np.delete(K, 5, 1)).all()
            Ku = _np(ops.multiscale_kuu(_on(Zb), _on(Sb), **kw))
            assert np.isnan(Ku[5]).all() and np.isnan(Ku[:, 5]).all() and np.isfinite(np.delete(np.delete(Ku, 5, 0), 5, 1)).all()


@pytest.mark.parametrize("n,M,d,ard", [(65, 64, 3, True), (130, 129, 64, False), (130, 129, 64, True)])
def test_adjoints(gp, n, M, d, ard):
    """dZ, dscales, dl, dv of sum Kbar .* Kfu and of sum Kbar .* Kuu (Kbar random, not symmetric) against the longdouble closed forms"""
    ops = gp.ops
    X, Z, S, ls, ref = _case(n, M, d, ard)
    kw = dict(variance=V, lengthscales=ls)
    Xd, Zd, Sd = _on(X), _on(Z), _on(S)
    rng = np.random.default_rng(11)
    l, r, q, Zl, Sl, Xl = ref["l"], ref["r"], ref["q"], Z.astype(LD), S.astype(LD), X.astype(LD)
    red = (lambda g: g) if ard else (lambda g: g.sum(keepdims=True))   # one lengthscale: the sum over the columns

    # ---- Kfu
    Kb = rng.normal(size=(n, M))
    G = Kb.astype(LD) * ref["Kfu"]
    Dl = ref["Dfu"]
    dS = (G[..., None] * (Dl ** 2 * r[None] ** 3 - r[None])).sum(0)
    want = {"dv": (G.sum() / LD(V)).reshape(1), "dl": red(dS.sum(0) + G.sum() / l), "dZ": (G[..., None] * Dl * r[None] ** 2).sum(0), "dS": dS}
    Ga, Xa, Za = np.abs(G), np.abs(Xl), np.abs(Zl)
    A0, A1, A2 = Ga.sum(0)[:, None], Ga.T @ Xa, Ga.T @ (Xa * Xa)
    mS = r ** 3 * (A2 + 2 * Za * A1 + Za * Za * A0) + r * A0
    mag = {"dv": (Ga.sum() / LD(V)).reshape(1), "dl": red(mS.sum(0) + Ga.sum() / l), "dZ": r ** 2 * (A1 + Za * A0), "dS": mS}
    coef = float(ref["cfu"].max()) + 2 + n + M + 4 * d + 30
    got = dict(zip(("dv", "dl", "dZ", "dS"), ops.multiscale_kfu_adjoint(Xd, Zd, Sd, _on(Kb), **kw)))
    again = ops.multiscale_kfu_adjoint(Xd, Zd, Sd, _on(Kb), **kw)
    for (name, g), g2 in zip(got.items(), again):
        _within("Kfu adjoint " + name, g, want[name], coef * U * mag[name])
        assert _same_bits(_np(g), _np(g2)), name

    # ---- Kuu
    Kb = rng.normal(size=(M, M))
    Kl, Du = Kb.astype(LD), ref["Duu"]
    Gs = (Kl + Kl.T) * ref["Kuu"]
    w = Du ** 2 * q ** 2 - q
    da = (Gs[..., None] * w).sum(1) / 2
    F = (Kl * ref["Kuu"]).sum()
    direct = -l * ((Kl * ref["Kuu"])[..., None] * w).sum((0, 1))
    want = {"dv": (F / LD(V)).reshape(1), "dl": red(F / l + direct + (da * 2 * (l + Sl)).sum(0)), "dZ": -(Gs[..., None] * Du * q).sum(1),
            "dS": da * 2 * (l + Sl)}
    Gsa, wa = np.abs(Gs), Du ** 2 * q ** 2 + q
    maa = (Gsa[..., None] * wa).sum(1) / 2
    Fa = np.abs(Kl * ref["Kuu"]).sum()
    mag = {"dv": (Fa / LD(V)).reshape(1), "dl": red(Fa / l + l * (Gsa[..., None] * wa).sum((0, 1)) / 2 + (maa * 2 * (l + Sl)).sum(0)),
           "dZ": (Gsa[..., None] * np.abs(Du) * q).sum(1), "dS": maa * 2 * (l + Sl)}
    coef = float(ref["cuu"].max()) + 2 + 2 * M + 4 * d + 30
    parts = ops.multiscale_adjoint_parts(M, d)
    got = dict(zip(("dv", "dl", "dZ", "dS"), ops.multiscale_kuu_adjoint(Zd, Sd, _on(Kb), parts=parts, **kw)))
    again = ops.multiscale_kuu_adjoint(Zd, Sd, _on(Kb), parts=parts.fill_(float("nan")), **kw)   # (what parts held does not matter)
    for (name, g), g2 in zip(got.items(), again):
        _within("Kuu adjoint " + name, g, want[name], coef * U * mag[name])
        assert _same_bits(_np(g), _np(g2)), name


# ---- model ---------------------------------------------------------------------------------------------------------------------------
def _model(gp, lik, *, whiten=True, q_diag=False):
    rng = np.random.default_rng(5)
    N, M, D, P = 70, 17, 2, 2
    X, Z, S = rng.uniform(size=(N, D)), rng.uniform(size=(M, D)), rng.uniform(0.05, 0.4, size=(M, D))
    q_mu = 0.3 * rng.normal(size=(M, P))
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    kern = gp.kernels.SquaredExponential(variance=V, lengthscales=[0.4, 0.7])
    m = gp.models.SVGP(kern, lik, gp.inducing_variables.Multiscale(Z, S), q_mu=q_mu, q_sqrt=q_sqrt, q_diag=q_diag, whiten=whiten,
                       num_latent_gps=P, num_data=1000, mean_function=gp.mean_functions.Constant(0.1))
    return m, X, Z, S, q_mu, q_sqrt


def _torch_cov(X, Z, S, v, ls):
    """the reference's Kuu, Kuf (kuus.py, kufs.py) in torch fp64"""
    r = 1 / (ls + S)
    Kfu = v * torch.prod(ls * r, -1)[None] * torch.exp(-0.5 * (((X[:, None, :] - Z[None]) * r[None]) ** 2).sum(-1))
    a = (ls + S) ** 2
    q = 1 / (a[:, None] + a[None] - ls ** 2)
    Kuu = v * torch.sqrt(torch.prod(ls ** 2 * q, -1)) * torch.exp(-0.5 * ((Z[:, None, :] - Z[None]) ** 2 * q).sum(-1))
    return Kuu, Kfu


@pytest.mark.parametrize("lik,whiten,q_diag", [("gaussian", True, False), ("gaussian", True, True), ("gaussian", False, False),
                                               ("gaussian", False, True), ("bernoulli", True, False)])
def test_svgp_elbo_grad_and_predict(gp, lik, whiten, q_diag):
    gauss = lik == "gaussian"
    m, X, Z, S, q_mu, q_sqrt = _model(gp, gp.likelihoods.Gaussian(0.2) if gauss else gp.likelihoods.Bernoulli(), whiten=whiten, q_diag=q_diag)
    Y = np.sin(X[:, :2] * 3.0) + 0.1 if gauss else (X[:, :2] > 0.5).astype(np.float64)
    pars = {"v": m.kernel.variance, "ls": m.kernel.lengthscales, "S": m.inducing_variable.scales}
    lv = {k: _leaf(p.numpy()) for k, p in pars.items()}
    lv.update({k: _leaf(a) for k, a in {"Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.1, "noise": 0.2}.items()})
    Kuu, Kfu = _torch_cov(_t(X), lv["Z"], lv["S"], lv["v"], lv["ls"])
    Fo, fmean, fvar = _elbo_from_cov(Kuu, Kfu.T, lv["v"], lv["q_mu"], lv["q_sqrt"], lv["mean"], _t(Y), whiten=whiten,
                                     noise=lv["noise"] if gauss else None)
    Fo.backward()
    ref, fmean, fvar = float(Fo.detach()), fmean.detach(), fvar.detach()
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - ref) <= 1e-8 * abs(ref) and abs(float(m.elbo((X, Y)).cpu()) - ref) <= 1e-8 * abs(ref)
    allp = dict(pars, Z=m.inducing_variable.Z, q_mu=m.q_mu, mean=m.mean_function.c, **({"noise": m.likelihood.variance} if gauss else {}))
    _check_model_grads("multiscale svgp " + lik, g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values()) | {m.q_sqrt}
    if q_diag:
        _check_model_grads("multiscale svgp", g, {"q_sqrt": m.q_sqrt}, lv, GRAD_TOL)
    else:
        want = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
        _close("multiscale svgp q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(want).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)
    if gauss and whiten and not q_diag:   # predict_f, fused and cached, against the reference's moments
        for mu, var in (m.predict_f(X), m.posterior().predict_f(X)):
            assert np.abs(_np(mu) - fmean.numpy()).max() <= 1e-8 * np.abs(fmean.numpy()).max()
            assert np.abs(_np(var) - fvar.numpy()).max() <= 1e-8 * np.abs(fvar.numpy()).max()


def test_scipy_training_raises_the_elbo_and_moves_the_scales(gp):
    m, X, _, S, _, _ = _model(gp, gp.likelihoods.Gaussian(0.2))
    Y = np.sin(X[:, :2] * 3.0) + 0.1
    before = float(m.elbo((X, Y)).cpu())
    gp.optimizers.Scipy().minimize(m, (X, Y), options=dict(maxiter=20))
    assert float(m.elbo((X, Y)).cpu()) > before
    assert np.abs(m.inducing_variable.scales.numpy() - S).max() > 0


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refusals(gp):
    K, iv, se = gp.kernels, gp.inducing_variables, gp.kernels.SquaredExponential
    Z = np.zeros((4, 2))
    ms = lambda: iv.Multiscale(Z, np.ones((4, 2)))   # noqa: E731
    model = lambda: _model(gp, gp.likelihoods.Gaussian(0.2))[0]   # noqa: E731
    return {
        "Matern32": (NotImplementedError, lambda: gp.covariances.Kuu(ms(), K.Matern32())),
        "Sum": (NotImplementedError, lambda: gp.covariances.Kuf(ms(), se() + se(), np.zeros((3, 2)))),
        "Shared wrapper": (NotImplementedError, lambda: gp.covariances.Kuu(iv.SharedIndependentInducingVariables(ms()), K.SharedIndependent(se(), 2))),
        "SGPR": (NotImplementedError, lambda: gp.models.SGPR((np.zeros((3, 2)), np.zeros((3, 1))), se(), ms())),
        "trainer": (NotImplementedError, lambda: gp.training.SVGPTrainer(model())),
        "natural gradients": (NotImplementedError, lambda: gp.models.reverse.svgp_routes(model(), narrow=True)),
        "scales of another shape": (ValueError, lambda: iv.Multiscale(Z, np.ones((4, 3)))),
        "D = 65": (ValueError, lambda: gp.covariances.Kuu(iv.Multiscale(np.zeros((4, 65)), np.ones((4, 65))), se())),
    }


@pytest.mark.parametrize("which", ["Matern32", "Sum", "Shared wrapper", "SGPR", "trainer", "natural gradients", "scales of another shape",
                                   "D = 65"])
def test_refusals(gp, which, monkeypatch):
    """every refusal is raised before the library is entered: its loader is made to fail"""
    def no_device(*a, **k):
        raise AssertionError("the device library was entered before the refusal")
    monkeypatch.setattr(gp._lib, "load", no_device)
    exc, call = _refusals(gp)[which]
    with pytest.raises(exc):
        call()


def test_library_answers_before_the_device(gp):
    """GPK_E_ARG (-1) for every case of include/gpk.h with HOST pointers in the operand slots, and 0 without a launch where there is
    nothing to do"""
    import ctypes as C
    lib = gp._lib.load()
    host = (C.c_double * 8)()
    hp = C.addressof(host)
    ls = gp._lib.host_doubles([1.0])

    def kfu(n=5, ldx=3, M=4, ldz=3, lds=3, d=3, ls=ls, v=1.0, op=0, ldg=4, ldo=4):
        return lib.gpk_multiscale_kfu(None, hp, n, ldx, hp, hp, M, ldz, lds, d, ls, 0, v, op, hp, ldg, hp, ldo)

    def kuu(M=4, ldz=3, lds=3, d=3, ls=ls, v=1.0, op=0, ldg=4, ldo=4):
        return lib.gpk_multiscale_kuu(None, hp, hp, M, ldz, lds, d, ls, 0, v, 0.0, op, hp, ldg, hp, ldo)

    def stage(M=4, ldz=3, lds=3, d=3, ls=ls, v=1.0, ldkb=4, plen=10 ** 6):
        return lib.gpk_multiscale_kuu_adjoint_stage(None, hp, hp, M, ldz, lds, d, ls, 0, v, hp, ldkb, hp, plen)

    def tail(sym=1, M=4, ldz=3, lds=3, d=3, ls=ls, v=1.0, ldsrc=7, slen=10 ** 6, lddz=3, ldds=3):
        return lib.gpk_multiscale_adjoint_tail(None, sym, hp, hp, M, ldz, lds, d, ls, 0, v, hp, ldsrc, slen, hp, hp, lddz, hp, ldds, hp)
    bad_ls = [gp._lib.host_doubles([x]) for x in (0.0, -1.0, float("nan"), float("inf"))]
    for f in (kfu, kuu, stage, tail):
        assert [f(d=x) for x in (0, -1, 65)] == [-1] * 3 and f(M=-1) == -1 and f(ldz=2) == -1 and f(lds=2) == -1
        assert [f(ls=x) for x in bad_ls] == [-1] * 4 and [f(v=x) for x in (0.0, -1.0, float("nan"), float("inf"))] == [-1] * 4
        assert f(M=0) == 0
    assert kfu(n=-1) == -1 and kfu(ldx=2) == -1 and kfu(ldo=3) == -1 and kfu(op=1, ldg=3) == -1 and kfu(op=3) == -1 and kfu(n=0) == 0
    assert kuu(ldo=3) == -1 and kuu(op=1, ldg=3) == -1 and kuu(op=2) == -1
    assert stage(ldkb=3) == -1 and stage(plen=int(lib.gpk_multiscale_parts_len(4, 3)) - 1) == -1
    assert tail(slen=int(lib.gpk_multiscale_parts_len(4, 3)) - 1) == -1 and tail(sym=0, ldsrc=6) == -1 and tail(lddz=2) == -1 and tail(ldds=2) == -1
    assert int(lib.gpk_multiscale_parts_len(130, 3)) == 4 * 130 * 7
