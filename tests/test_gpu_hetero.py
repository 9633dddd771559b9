"""GPU tests of `likelihoods.HeteroskedasticTFPConditional`: its two kernels (`ops.hetero_varexp_sum`, `ops.hetero_predict`) against the
longdouble `_reference`, and its SVGP / VGP routes against central differences of the longdouble reference ELBO (`_check_model`)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_likelihoods as T  # noqa: E402  (helpers only)

U, LD, PI, gp = T.U, T.LD, T.PI, T.gp   # (gp: the module fixture of the likelihood tests)
_np, _bits, _within = T._np, T._bits, T._within
GH = [a.astype(LD) for a in np.polynomial.hermite.hermgauss(20)]
LINKS = ["exp", "softplus"]
RPB = {"exp": 256, "softplus": 64}      # rows per block, include/gpk.h; the grid is clamped at 1024 blocks
VARS = np.array([0.0, 1e-12, 0.5, 4.0])
JITTER, EPS_K = 1e-6, 4 * 2.0 ** -52    # EPS_K: the conditioning pre-check's perturbation (tests/test_gpu_kernel_trees.py)


def _reference(y, m, v, link, x=GH[0], w=GH[1]):
    """((VE [n], dmu [n, 2], dvar [n, 2], predictive variance [n], predictive log density [n], delta [n]), bounds of the first five)
    of include/gpk.h in longdouble, for EXACT operands (the callers' knn - s0 + ssq and fmean + mean_const are exact in fp64).
    Bounds, first order in u.  A node sum: the roundings of sd = sqrt(2 v2) and g = fma(sd, x, m2) move g by at most 2 u |g|, whose
    effect is read off the reference term by term as |term(g (1 + 4u)) - term(g)| (twice the movement: the difference is first order);
    evaluating a term (exp, log1p, log, two quotients, up to five products) is 16 u of the magnitude of its sub-terms; summing H + 2
    terms in any order is (H + 2) u sum |term|.  exp link: exp(z) carries the rounding of z, u |z|, and exp's own ulp.  The closing
    arithmetic of an output (dy, a, at most three products and two sums): 8 u of the sum of its absolute terms.  A log-sum-exp moves by
    at most the largest movement of a term (8 u of its absolute sub-terms) plus (H + 6) u (1 + |result|).  delta: the contract's
    dvar[:, 1] (E[h''] / 2: the derivative of the INTEGRAL by the rule) minus the exact derivative of the RULE, sum w h'(g) x / sd (the
    last two terms of `val`; without a bound, meaningless where v2 = 0); 0 under exp."""
    y, m, v = (np.asarray(a, dtype=LD) for a in (y, m, v))
    (m1, m2), (v1, v2), H, wn = m.T, v.T, len(x), w / np.sqrt(PI)
    dy = y - m1
    a = dy * dy + v1

    def nodes(eps):
        sd = np.sqrt(2 * v2)[:, None]
        g = (m2[:, None] + sd * x) * (1 + LD(eps))
        s = np.exp(g) if link == "exp" else np.where(g > 0, g, 0) + np.log1p(np.exp(-np.abs(g)))
        val = mag = []
        if link == "softplus":
            sig = 1 / (1 + np.exp(-g))
            sr, tau, h2 = sig / s, 1 - sig, 1 / (s * s)
            d2, xs = -2 * sr * h2, x / (sd + (sd == 0))
            val = [np.log(s), sr, (tau * sr - sr * sr) / 2, h2, d2, h2 * (3 * sr * sr - tau * sr), s * s, sr * xs, d2 * xs]
            mag = [1 + np.abs(np.log(s)), sr, (tau * sr + sr * sr) / 2, h2, 2 * sr * h2, h2 * (3 * sr * sr + tau * sr), s * s]
        V = v1[:, None] + s * s
        q = (dy * dy)[:, None] / V
        return ([wn * t for t in val], [wn * t for t in mag], np.log(wn) - np.log(2 * PI) / 2 - (np.log(V) + q) / 2,
                np.abs(np.log(wn)) + 1 + (np.abs(np.log(V)) + q) / 2)
    (t0, mag, t, tmag), (t1, _, te, _) = nodes(0.0), nodes(4 * U)
    E = [s.sum(1) for s in t0]
    R = [(np.abs(q - p) + 16 * U * g).sum(1) + (H + 2) * U * np.abs(p).sum(1) for p, q, g in zip(t0, t1, mag)]
    if link == "exp":   # closed forms, no nodes
        z, z2, o = 2 * v2 - 2 * m2, 2 * v2 + 2 * m2, 0 * m2
        e2, es = np.exp(z), np.exp(z2)
        r2 = 2 * U * (1 + np.abs(z)) * e2
        E, R = [m2, 1 + o, o, e2, -2 * e2, 2 * e2, es, o, 2 * e2], [o, o, o, r2, 2 * r2, 2 * r2, 2 * U * (1 + np.abs(z2)) * es]
    mx = t.max(1)
    ld = mx + np.log(np.exp(t - mx[:, None]).sum(1))
    A, ady = [np.abs(e) for e in E], np.abs(dy)
    val = (-np.log(2 * PI) / 2 - E[0] - a * E[3] / 2, np.stack([dy * E[3], -E[1] - a * E[4] / 2], 1),
           np.stack([-E[3] / 2, -E[2] - a * E[5] / 2], 1), v1 + E[6], ld, E[7] - E[2] + a * (E[8] - E[5]) / 2)
    bnd = (R[0] + a * R[3] / 2 + 8 * U * (1 + A[0] + a * A[3]),
           np.stack([ady * R[3] + 8 * U * ady * A[3], R[1] + a * R[4] / 2 + 8 * U * (A[1] + a * A[4])], 1),
           np.stack([R[3] / 2 + 8 * U * A[3], R[2] + a * R[5] / 2 + 8 * U * (A[2] + a * A[5])], 1),
           R[6] + 2 * U * np.abs(val[3]), (np.abs(te - t) + 8 * U * tmag).max(1) + (H + 6) * U * (1 + np.abs(ld)))
    return val, bnd


def test_the_20_node_rule_against_200_nodes():
    """The contract is the rule, not the integral.  At |m2| <= 2, v2 <= 1 all five outputs of the 20-node rule lie within 2 |20 - 40
    nodes| (the truncation estimate) plus the fp64 bound of the 200-node values: that the rules converge this fast is what is checked."""
    rng = np.random.default_rng(0)
    y, m, v = rng.normal(size=50), np.stack([rng.normal(size=50), rng.uniform(-2, 2, 50)], 1), rng.uniform(0, 1, size=(50, 2))
    r20, b20 = _reference(y, m, v, "softplus")
    r40, r200 = (_reference(y, m, v, "softplus", *(c.astype(LD) for c in np.polynomial.hermite.hermgauss(n)))[0] for n in (40, 200))
    for p, q, r, b in zip(r20, r40, r200, b20):
        assert (np.abs(p - r) <= 2 * np.abs(p - q) + b).all()


def _inputs(link, n, form):
    """operands on a 2^-10 grid, so that fmean + mean_const and knn - s0 + ssq are exact.  form "ssq": the variances {0, 1e-12, 0.5, 4}
    of both latents as ssq alone; "s0": one s0 and knn for both latents; "per": one per latent"""
    rng = np.random.default_rng(n + len(form))
    grid = lambda a: np.round(a * 1024) / 1024   # noqa: E731
    F = grid(np.stack([rng.normal(size=n), rng.uniform(-3, 3, size=n)], 1))
    Y = (F[:, 0] + rng.normal(size=n) * np.exp(0.3 * F[:, 1]))[:, None]
    i, per = np.arange(n), form == "per"
    if form == "ssq":
        ssq, s0, knn = np.stack([VARS[i % 4], VARS[(i // 4) % 4]]), None, [0.0]
        v = ssq.T
    else:
        ssq, s0 = grid(rng.uniform(0, 0.6, size=(2, n))), grid(rng.uniform(0, 0.5, size=(2, n) if per else n))
        knn = [1.25, 0.875] if per else [1.25]
        v = np.asarray(knn)[None, :] - (s0.T if per else s0[:, None]) + ssq.T
    return dict(F=F, Y=Y, ssq=ssq, s0=s0, knn=knn, per=per, mc=0.125, m=F + 0.125, v=v)


def _run(ops, a, link):
    dev = lambda t: None if t is None else ops.to_device(t)   # noqa: E731
    r = ops.hetero_varexp_sum(dev(a["Y"]), dev(a["F"]), s0=dev(a["s0"]), ssq=dev(a["ssq"]), knn=a["knn"], link=link, mean_const=a["mc"],
                              s0_per_latent=a["per"], want_fvar=True, want_rows=True, want_grads=True)
    return [_np(t) for t in r]


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("which,form", [("one", "ssq"), ("below", "s0"), ("above", "per"), ("257", "ssq"), ("far", "ssq")])
def test_stage_and_predict_against_reference(gp, link, which, form):
    """n = 1, a block - 1, a block + 1, 257, one row past the grid clamp (a partial second trip); every variance form; both kernels on
    the same moments; a second call returns the same bits; y = None computes no log density and gives the same moments"""
    ops, n = gp.ops, {"one": 1, "below": RPB[link] - 1, "above": RPB[link] + 1, "257": 257, "far": 1024 * RPB[link] + 1}[which]
    c = _inputs(link, n, form)
    (ve, gm, gv, pvar, pld, _), (b_ve, b_gm, b_gv, b_pvar, b_pld) = _reference(c["Y"][:, 0], c["m"], c["v"], link)
    out, rws, dmu, dvar, fvar = res = _run(ops, c, link)
    mean, var, ld = (_np(t) for t in ops.hetero_predict(*(ops.to_device(c[k]) for k in "mvY"), link=link))
    total = ("out[0]", out, [ve.sum()], [b_ve.sum() + 2 * (n + 2) * U * np.abs(ve).sum()])
    for name, got, ref, bound in [total, ("rows", rws, ve, b_ve), ("dmu", dmu, gm, b_gm), ("dvar", dvar, gv, b_gv),
                                  ("predictive variance", var, pvar, b_pvar), ("predictive log density", ld, pld, b_pld)]:
        _within(f"{link} {n} {form} {name}", got, ref, bound)
    assert np.array_equal(_bits(fvar), _bits(c["v"])) and np.array_equal(_bits(mean), _bits(c["m"][:, 0]))
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(res, _run(ops, c, link))), "a second identical call differs"
    mean2, var2, none = ops.hetero_predict(ops.to_device(c["m"]), ops.to_device(c["v"]), link=link)
    assert none is None and np.array_equal(_bits(_np(mean2)), _bits(mean)) and np.array_equal(_bits(_np(var2)), _bits(var))


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("where,value", [("Y", np.nan), ("Y", np.inf), ("F", np.nan), ("F", -np.inf), ("ssq", np.nan), ("ssq", np.inf),
                                         ("ssq", 400.0)])
def test_nonfinite_row_and_overflow(gp, link, where, value):
    """NaN / Inf in row 37's y, m2 or v1: the row and the sum are NaN; v2 = 400 under exp: the header's IEEE results; no other row moves"""
    c = _inputs(link, RPB[link] + 1, "ssq")
    clean, b = _run(gp.ops, c, link), 37
    moved = c[where].copy()
    moved[(1, b) if value == 400.0 else (0, b) if where == "ssq" else (b, 0) if where == "Y" else (b, 1)] = value
    out, rws, dmu, dvar, _ = _run(gp.ops, {**c, where: moved}, link)
    if value != 400.0:
        assert np.isnan(out[0]) and np.isnan(rws[b]) and np.isnan(dmu[b]).all() and np.isnan(dvar[b]).all()
    elif link == "exp":
        sign = np.sign(c["Y"][b, 0] - c["m"][b, 0])
        assert out[0] == rws[b] == -np.inf and dmu[b].tolist() == [sign * np.inf, np.inf] and dvar[b].tolist() == [-np.inf, -np.inf]
    others = np.arange(c["F"].shape[0]) != b
    assert all(np.array_equal(_bits(g[others]), _bits(r[others])) for g, r in zip((rws, dmu, dvar), clean[1:4]))


def _chol_solve(K, B):   # L^-1 B for K = L L^T in longdouble (numpy.linalg has no longdouble)
    L, X = np.zeros_like(K), np.zeros_like(B)
    for j in range(K.shape[0]):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        X[j] = (B[j] - L[j, :j] @ X[:j]) / L[j, j]
    return X


def _elbo(th, X, Y, link, scale=1.0, vgp=False, bump=0.0):
    """(ELBO, fvar[:, 1], delta of `_reference`) of the whitened model in longdouble, one path: Kuu = K(Z, Z) + jitter I; the SVGP has
    Kuf = K(Z, X) and the row diagonal `variance`, the VGP Z = X, Kuf = Kuu and its diagonal (L^-1 Kuu = L^T: fmean = L q_mu).  variance /
    ls: one SquaredExponential for both latents, or [SquaredExponential, Matern12].  bump: the pre-check, K times 1 + bump * a fixed sign"""
    X = X.astype(LD)
    Z, q_mu, S = (X if vgp else th["Z"]), th["q_mu"], th["q_sqrt"]
    fm, fv = [], []
    for p, (var, ls) in enumerate(zip(np.broadcast_to(th["variance"], 2), np.broadcast_to(th["ls"], 2))):
        def k(A, B, seed):
            r2 = (((A[:, None, :] - B[None, :, :]) / ls) ** 2).sum(-1)
            k_ = var * np.exp(-np.sqrt(r2) if p and np.size(th["ls"]) == 2 else -r2 / 2)
            return k_ * (1 + LD(bump) * np.random.default_rng(seed).choice([-1.0, 1.0], size=r2.shape))
        Kuu = k(Z, Z, 1) + JITTER * np.eye(Z.shape[0], dtype=LD)
        Kuf, kd = (Kuu, np.diagonal(Kuu)) if vgp else (k(Z, X, 2), var * (1 + LD(bump)))
        A = _chol_solve(Kuu, Kuf)
        LTA = A * S[:, p][:, None] if S.ndim == 2 else np.tril(S[p]).T @ A
        fm.append(A.T @ q_mu[:, p] + th["mean"])
        fv.append(kd - (A * A).sum(0) + (LTA * LTA).sum(0))
    logdet = np.log((S if S.ndim == 2 else np.diagonal(S, axis1=1, axis2=2)) ** 2).sum()   # (a full q_sqrt is lower triangular)
    val = _reference(Y[:, 0], np.stack(fm, 1), np.stack(fv, 1), link)[0]
    return val[0].sum() * scale - ((q_mu * q_mu).sum() - q_mu.size - logdet + (S * S).sum()) / 2, fv[1], val[5]


def _check_model(m, pars, th, F, scale, got_elbo, value_and_grad, h=1e-5):
    """elbo(), and per Parameter of `pars` the gradient along a random direction, against the longdouble restatement F and its central
    difference D(h).  Bounds: the tree tests' rule for the fp64 floor, 100 times what the reference itself moves under the conditioning
    pre-check; the formula's truncation h^2 F''' / 6 = |D(2h) - D(h)| / 3, doubled; the dot product, 8 u sum |g_i d_i|.  softplus: the
    contract's gradient is the rule's plus scale * sum_b delta_b d fvar[b, 1] (`_reference`), added to D(h)."""
    th = {**th, **{k: np.asarray(p.numpy(), dtype=LD) for k, p in pars.items()}}
    ref, _, delta = F(th)
    tol = 100 * abs(F(th, EPS_K)[0] - ref)
    assert abs(LD(got_elbo) - ref) <= tol
    if not pars:   # (the reverse pass is refused)
        return pytest.raises(NotImplementedError, value_and_grad)
    val, g = value_and_grad()
    assert abs(LD(val) - ref) <= tol and len(g) == len(m.trainable_parameters)
    rng = np.random.default_rng(7)
    for key, par in pars.items():
        d = rng.normal(size=th[key].shape).astype(LD)
        d = np.tril(d) if d.ndim == 3 else d

        def diff(s, bump=0.0):
            hi, lo = (F({**th, key: th[key] + LD(t) * d}, bump) for t in (s, -s))
            return (hi[0] - lo[0]) / (2 * s), (hi[1] - lo[1]) / (2 * s)
        (D1, dfv), (D2, _), (Db, _) = diff(h), diff(2 * h), diff(h, EPS_K)
        u = par.unconstrained_variable   # the gradient is w.r.t. u: fill_triangular is a permutation, the others are elementwise
        gu = np.reshape(np.asarray(g[par], dtype=np.float64), np.shape(u))
        gc = np.tril(par.transform.forward(gu)) if np.shape(u) != d.shape else gu / par.transform.forward_grad(u)
        gd = gc.reshape(d.shape).astype(LD) * d
        bound = 2 * abs(D2 - D1) / 3 + 100 * abs(Db - D1) + 8 * U * np.abs(gd).sum()
        assert abs(gd.sum() - D1 - scale * (delta * dfv).sum()) <= bound, key


@pytest.mark.parametrize("link", LINKS)
@pytest.mark.parametrize("model", ["svgp-full", "svgp-qdiag", "svgp-separate", "vgp"])
def test_model_elbo_and_grad(gp, model, link):
    """SVGP N = 70, M = 17, d = 3, whitened: one SquaredExponential shared by the latents with a full and a diagonal q_sqrt, forward and
    reverse; SeparateIndependent([SquaredExponential, Matern12]) forward, its reverse pass refused; VGP N = 40; predict_log_density"""
    vgp, q_diag, sep = model == "vgp", model == "svgp-qdiag", model == "svgp-separate"
    N, M, d = (40, 40, 2) if vgp else (70, 17, 3)
    rng, K, I = np.random.default_rng(3), gp.kernels, gp.inducing_variables
    X, Z, q_mu = rng.uniform(-1.5, 1.5, size=(N, d)), rng.uniform(-1.5, 1.5, size=(M, d)), 0.3 * rng.normal(size=(M, 2))
    Y = np.sin(2 * X[:, :1]) + (0.1 + 0.3 * np.abs(X[:, 1:2])) * rng.normal(size=(N, 1))
    q_sqrt = rng.uniform(0.3, 0.9, size=(M, 2)) if q_diag else np.tril(0.05 * rng.normal(size=(2, M, M))) + 0.6 * np.eye(M)
    kern, mean = K.SquaredExponential(variance=1.3, lengthscales=0.8), gp.mean_functions.Constant(0.2)
    lik = gp.likelihoods.HeteroskedasticTFPConditional(scale_transform=link)
    if vgp:
        m = gp.models.VGP((X, Y), kern, lik, mean_function=mean)
        m.q_mu.assign(q_mu)
        m.q_sqrt.assign(q_sqrt)
        pars, scale, elbo, grad = {}, 1.0, m.elbo, m.objective_and_grad
    else:
        iv = I.SharedIndependentInducingVariables(I.InducingPoints(Z.copy())) if sep else Z.copy()
        kern = K.SeparateIndependent([kern, K.Matern12(variance=0.7, lengthscales=1.1)]) if sep else kern
        m = gp.models.SVGP(kern, lik, iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), q_diag=q_diag, num_data=500, mean_function=mean)
        pars, scale = ({} if sep else {"Z": m.inducing_variable.Z}), 500 / 70
        elbo, grad = lambda: m.elbo((X, Y)), lambda: m.elbo_and_grad((X, Y))
    th = dict(variance=[1.3, 0.7] if sep else 1.3, ls=[0.8, 1.1] if sep else 0.8, Z=Z, q_mu=q_mu, q_sqrt=q_sqrt, mean=0.2)
    pars = {} if sep else dict(pars, variance=kern.variance, ls=kern.lengthscales, q_mu=m.q_mu, q_sqrt=m.q_sqrt, mean=mean.c)
    F = lambda t, bump=0.0: _elbo(t, X, Y, link, scale, vgp, bump)   # noqa: E731
    _check_model(m, pars, {k: np.asarray(a, dtype=LD) for k, a in th.items()}, F, scale, float(elbo()), grad)
    val, bnd = _reference(Y[:, 0], *(_np(a) for a in m.predict_f(X)), link)
    _within("predict_log_density", _np(m.predict_log_density((X, Y))), val[4], bnd[4])


def test_scipy_learns_a_noise_level_that_grows_with_x(gp):
    """twenty optimizers.Scipy iterations on y = sin(3 x) + (0.05 + 0.6 x) eps: the ELBO rises, the predictive variance grows with x"""
    X = np.linspace(0, 1, 70)[:, None]
    Y = np.sin(3 * X) + (0.05 + 0.6 * X) * np.random.default_rng(11).normal(size=(70, 1))
    m = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=0.5), gp.likelihoods.HeteroskedasticTFPConditional(),
                       np.linspace(0, 1, 17)[:, None].copy())
    before = float(m.elbo((X, Y)))
    gp.optimizers.Scipy().minimize(m, (X, Y), options=dict(maxiter=20))
    var = _np(m.predict_y(np.array([[0.05], [0.95]]))[1])[:, 0]
    assert float(m.elbo((X, Y))) > before and var[1] > var[0]


HET = lambda gp, **kw: gp.likelihoods.HeteroskedasticTFPConditional(**kw)   # noqa: E731
REFUSALS = [(NotImplementedError, lambda gp: HET(gp, scale_transform="square")),
            (NotImplementedError, lambda gp: HET(gp, distribution_class="StudentT")),
            (ValueError, lambda gp: gp.models.SVGP(gp.kernels.SquaredExponential(), HET(gp), np.zeros((3, 1)), num_latent_gps=3)),
            (ValueError, lambda gp: gp.models.VGP((np.zeros((5, 1)), np.zeros((5, 2))), gp.kernels.SquaredExponential(), HET(gp)))]


@pytest.mark.parametrize("exc,call", REFUSALS)
def test_refusals(gp, exc, call, monkeypatch):
    """a bad link, a bad distribution, three latents, two Y columns: each raised before the library is entered (its loader fails)"""
    monkeypatch.setattr(gp._lib, "load", lambda *a, **k: pytest.fail("the device library was entered before the refusal"))
    with pytest.raises(exc):
        call(gp)


def test_unknown_link_at_the_entry_point(gp):
    """link = 2 answers GPK_E_ARG before a pointer is looked at: the slots hold host memory"""
    lib, host = gp._lib.load(), (gp._lib.c_double * 8)()
    assert lib.gpk_hetero_varexp_sum(None, 2, host, 1, host, 3, None, 0, None, host, 0, 0.0, None, None, None, None, host, host) == -1
    assert lib.gpk_hetero_predict(None, 2, host, host, host, 1, 3, host, host, host) == -1
