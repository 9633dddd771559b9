"""GPU tests of the Exponential / Gamma / Beta / Ordinal likelihoods: the four codes behind `ops.likelihood_varexp_sum` and
`ops.svgp_elbo_shard_lik`, the classes, `SVGP.elbo` / `predict_y` / `predict_log_density` and the reverse pass with them.  The layout
follows tests/test_gpu_likelihoods.py, whose helpers (`_within`, `_mp_map`, `_svgp_problem`, the case table) are reused.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_likelihood_zoo_emulated.py: tests/emulation.py,
the four codes being rows of the table of tests/fake_likelihood_ops.py).

References.  Values: the contract of include/gpk.h restated in np.longdouble (`_reference`) with erfc / loggamma / digamma from mpmath
(40 digits); the model-level 1e-8 comparisons take the same restatement over scipy's fp64 functions (their 1e-15 is far inside that
bar; the mpmath sum over 150 x 4 x 20 Beta nodes would take most of a minute).  Gradients: torch-CPU fp64 autograd of the restated
ELBO.  u = 2^-53; every bound is derived next to its check; the bound of the library's psi is read from gpflow_amd/csrc/digamma.h.
"""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_likelihoods as T  # noqa: E402  (helpers only)
from oracle import gp_oracle as orc  # noqa: E402  (checker only)
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)

U, LD, PI, GH_X, GH_W = T.U, T.LD, T.PI, T.GH_X, T.GH_W
_np, _bits, _within, _refused = T._np, T._bits, T._within, T._refused
A998 = LD(1) - 2 * LD("1e-3")
EDGES5 = (-1.1, -0.3, 0.2, 0.9, 1.7)
EDGES15 = tuple(float(v) for v in np.round(np.linspace(-2.1, 2.1, 15) + 0.03 * np.sin(np.arange(15)), 3))
LIKS = [("exponential_exp", ()), ("gamma_exp", (1.7,)), ("beta_probit", (2.5,)), ("ordinal", (0.6, 5.0) + EDGES5),
        ("ordinal", (1.3, 15.0) + EDGES15)]
LIK_IDS = ["exponential_exp", "gamma_exp", "beta_probit", "ordinal5", "ordinal15"]
MODEL_LIKS, MODEL_IDS = LIKS[:4], LIK_IDS[:4]
GRAD_NAME = {"gamma_exp": "likelihood_shape", "beta_probit": "likelihood_scale", "ordinal": "likelihood_sigma"}
CLOSED = ("exponential_exp", "gamma_exp")


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _psi_bound(x):
    """the ABSOLUTE error bound of gpk_digamma, from the constants next to its derivation (gpflow_amd/csrc/digamma.h)"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpflow_amd", "csrc", "digamma.h")).read()
    c = {k: LD(re.search(r"#define GPK_DIGAMMA_BOUND_%s\s+([0-9.eE+-]+)" % k, src).group(1)) for k in ("RECIP", "LOG", "CONST")}
    x = np.asarray(x, dtype=LD)
    return U * (c["RECIP"] / x + c["LOG"] * np.log(x + 10) + c["CONST"])


# ------------------------------------------------------------------------------------------------ the reference
def _mp_fns():
    import mpmath
    return dict(erfc=lambda z: T._mp_map(mpmath.erfc, z), lgamma=lambda z: T._mp_map(mpmath.loggamma, z),
                digamma=lambda z: T._mp_map(mpmath.digamma, z))


def _f64_fns():
    import scipy.special as sps
    f = lambda fn: (lambda z: fn(np.asarray(z, dtype=np.float64)).astype(LD))   # noqa: E731
    return dict(erfc=f(sps.erfc), lgamma=f(sps.gammaln), digamma=f(sps.digamma))


def _trigamma(z):
    """psi'(z) in fp64: it only enters the BOUNDS (as the sensitivity of psi to its argument's rounding)"""
    import scipy.special as sps
    return sps.polygamma(1, np.asarray(z, dtype=np.float64)).astype(LD)


def _phi(z):
    return np.exp(-z * z / 2) / np.sqrt(2 * PI)


def _reference(lik, par, Y, mu, fv, emu=0.0, efv=0.0, fns=None):
    """The definition (include/gpk.h), in longdouble: (ve, dmu, dvar, dtheta) [rows, P] and a bound on the fp64 error of each.

    Y, mu, fv: the exact operands; emu, efv: how far an fp64 evaluation of mu = fmean + mean_const and fvar = knn - s0 + ssq may sit
    from them.  The error model is that of tests/test_gpu_likelihoods.py::_reference, first order in u:
      * closed forms: e = exp(-mu + fvar / 2) carries exp's 3 ulp, the rounding of its argument and the operand errors (rel_e);
        log 3 ulp; lgamma is allowed 16 ulp of max(|lgamma|, 1); psi its stated absolute bound; every sum 4 u sum |term|;
      * quadrature: the node f_h = fma(sd, x_h, mu) sits within ef of the exact one and moves g, g', dg/dtheta by |g'| ef, |g''| ef,
        |d/df dg/dtheta| ef (closed forms below); the library functions add their own error ("direct", derived per code below);
        the 20-term weighted sum and its four-lane combination 32 u sum_h w_h |.|; dvar divides by sd: relative 4 u + efv / (2 fvar)."""
    fns = fns or _mp_fns()
    Y, mu, fv = (np.asarray(a, dtype=LD) for a in (Y, mu, fv))
    emu, efv = np.broadcast_to(np.asarray(emu, dtype=LD), mu.shape), np.broadcast_to(np.asarray(efv, dtype=LD), mu.shape)
    emu = emu + U * np.abs(mu)
    zero = np.zeros(mu.shape, dtype=LD)
    if lik in CLOSED:
        arg = -mu + fv / 2
        ye = Y * np.exp(arg)
        rel_e = 5 * U + U * np.abs(arg) + emu + efv / 2      # exp 3 ulp, its argument's rounding and operand error, the product y e
        b_dvar = np.abs(ye) * rel_e
        if lik == "exponential_exp":
            ve, dmu = -mu - ye, ye - 1
            b_ve = 4 * U * (np.abs(mu) + np.abs(ye)) + np.abs(ye) * rel_e + emu
            return (ve, dmu, -ye / 2, zero), (b_ve, U * np.abs(dmu) + np.abs(ye) * rel_e, b_dvar, zero)
        sh = LD(par[0])
        lg, ps = fns["lgamma"](np.array([sh]))[0], fns["digamma"](np.array([sh]))[0]
        ly = np.log(Y)
        t = [sh * mu, lg + 0 * mu, (sh - 1) * ly, ye]
        ve, dmu, dth = -t[0] - t[1] + t[2] - t[3], ye - sh, ly - mu - ps
        b_ve = 4 * U * sum(np.abs(x) for x in t) + np.abs(ye) * rel_e + sh * emu + 16 * U * max(abs(lg), 1) + 4 * U * np.abs(t[2])
        b_dth = 4 * U * (np.abs(ly) + np.abs(mu) + abs(ps)) + 4 * U * np.abs(ly) + emu + _psi_bound(sh)
        return (ve, dmu, -ye / 2, dth), (b_ve, U * np.abs(dmu) + np.abs(ye) * rel_e, b_dvar, b_dth)
    x, wn = GH_X.astype(LD), GH_W.astype(LD) / np.sqrt(PI)
    sd = np.sqrt(2 * fv)
    f = mu[..., None] + sd[..., None] * x
    ef = U * (np.abs(f) + np.abs(mu)[..., None]) + np.abs(x) * (sd * (U + efv / (2 * fv)))[..., None] + emu[..., None]
    y = Y[..., None]
    ynan = zero
    if lik == "beta_probit":
        s = LD(par[0])
        m = fns["erfc"](-f / np.sqrt(LD(2))) / 2 * A998 + LD("1e-3")
        al, be = m * s, s - m * s
        # (the clip bounds are the fp64 constants 1e-6 and 1.0 - 1e-6 of the reference: log(1 - yc) at the upper one is sensitive to
        #  the 17th digit of that constant, so the decimal value would be another definition)
        lo, hi = LD(1e-6), LD(1.0 - 1e-6)
        yc = np.where(y < lo, lo, np.where(y > hi, hi, y))
        ly, l1 = np.log(yc) + 0 * f, np.log(1 - yc) + 0 * f
        lgs, pss = fns["lgamma"](np.array([s]))[0], fns["digamma"](np.array([s]))[0]
        lga, lgb, pa, pb = fns["lgamma"](al), fns["lgamma"](be), fns["digamma"](al), fns["digamma"](be)
        ta, tb = _trigamma(al), _trigamma(be)
        Tm = ly - l1 - pa + pb                                  # dg/dalpha at fixed scale
        dphi = s * A998 * _phi(f)                               # dalpha/df
        g = (al - 1) * ly + (be - 1) * l1 + lgs - lga - lgb
        g1 = dphi * Tm
        g2 = -f * g1 - dphi * dphi * (ta + tb)
        gt = m * ly + (1 - m) * l1 + pss - m * pa - (1 - m) * pb
        gt1 = dphi / s * (Tm - al * ta + be * tb)
        # direct errors.  m: erfc 16 ulp and the jitter arithmetic, 20 u m; so alpha carries 21 u alpha and beta that plus u beta.
        # They move g by |T| 21 u alpha (dg/dalpha = T), psi(alpha), psi(beta) by psi' times them.  lgamma: 16 ulp of max(|.|, 1) each;
        # log 3 ulp, 1 - yc one rounding (u in the logarithm); products and the five-term sum 8 u sum |term|.
        da, db = 21 * U * al, 21 * U * al + U * be
        d_g = np.abs(Tm) * da + 16 * U * (np.maximum(np.abs(lga), 1) + np.maximum(np.abs(lgb), 1) + max(abs(lgs), 1)) \
            + 8 * U * (np.abs((al - 1) * ly) + np.abs((be - 1) * l1) + abs(lgs) + np.abs(lga) + np.abs(lgb)) \
            + 2 * U * (np.abs(al - 1) + np.abs(be - 1))
        d_T = _psi_bound(al) + _psi_bound(be) + ta * da + tb * db + 8 * U * (np.abs(ly) + np.abs(l1) + np.abs(pa) + np.abs(pb)) + U
        d_g1 = np.abs(g1) * (8 + f * f) * U + dphi * d_T       # exp(-f^2 / 2): 3 ulp + the argument's u f^2, the products
        d_gt = _psi_bound(s) + m * _psi_bound(al) + (1 - m) * _psi_bound(be) + 20 * U * m * (np.abs(ly) + np.abs(l1) + np.abs(pa) + np.abs(pb)) \
            + m * ta * da + (1 - m) * tb * db \
            + 8 * U * (np.abs(m * ly) + np.abs((1 - m) * l1) + abs(pss) + np.abs(m * pa) + np.abs((1 - m) * pb))
    else:
        sig, n = LD(par[0]), int(par[1])
        edges = np.asarray(par[2:], dtype=LD)
        ok = (Y >= 0) & (Y <= n) & (Y == np.floor(Y))
        yi = np.where(ok, Y, 0).astype(np.int64)
        ynan = np.where(ok, LD(0), LD("nan"))
        has_l, has_r = (yi < n)[..., None], (yi > 0)[..., None]
        el = np.concatenate([edges, [LD(0)]])[yi][..., None]      # (a finite stand-in at the open ends, masked below)
        er = np.concatenate([[LD(0)], edges])[yi][..., None]
        zl, zr = (el - f) / sig, (er - f) / sig
        up = np.where(has_r, zr >= 0, False)                      # zr = -inf at the first bin: the left side
        za, zb = np.where(up, zr, -zl), np.where(up, zl, -zr)
        fa, fb = np.where(up, has_r, has_l), np.where(up, has_l, has_r)   # is that end finite
        Ea = np.where(fa, fns["erfc"](za / np.sqrt(LD(2))) / 2, LD(1))     # erfc(-inf) / 2 = 1
        Eb = np.where(fb, fns["erfc"](zb / np.sqrt(LD(2))) / 2, LD(0))     # erfc(+inf) / 2 = 0
        D = A998 * (Ea - Eb)
        q = D + LD("1e-6")
        pl, pr = np.where(has_l, _phi(zl), 0), np.where(has_r, _phi(zr), 0)
        zpl, zpr = np.where(has_l, zl * pl, 0), np.where(has_r, zr * pr, 0)
        g = np.log(q)
        g1 = -A998 * (pl - pr) / (sig * q)
        g2 = -A998 * (zpl - zpr) / (sig * sig * q) - g1 * g1
        gt = -A998 * (zpl - zpr) / (sig * q)
        gt1 = -A998 * ((zl * zpl - pl) - (zr * zpr - pr)) / (sig * sig * q) - gt * g1
        # direct errors.  z: a subtraction, a division and the scaling by 1 / sqrt 2, 3 u relative; erfc answers a relative argument
        # error d with (z^2 + 1) d relative, and has 16 ulp of its own: (20 + 3 z^2) u of each finite term; the difference 2 u D.
        # exp(-z^2 / 2): 3 ulp and 3 u z^2 from its argument, the products: (8 + 3 z^2) u of each density term.
        dD = A998 * U * (np.where(fa, Ea * (20 + 3 * za * za), 0) + np.where(fb, Eb * (20 + 3 * zb * zb), 0)) + 2 * U * np.abs(D)
        d_g = dD / q + 4 * U * (1 + np.abs(g))
        d_g1 = A998 * U * (pl * (8 + 3 * zl * zl) + pr * (8 + 3 * zr * zr)) / (sig * q) + np.abs(g1) * (dD / q + 6 * U)
        d_gt = A998 * U * (np.abs(zpl) * (9 + 3 * zl * zl) + np.abs(zpr) * (9 + 3 * zr * zr)) / (sig * q) + np.abs(gt) * (dD / q + 6 * U)
    S = lambda v: (v * wn).sum(-1)   # noqa: E731
    ve, dmu, dth = S(g) + ynan, S(g1) + ynan, S(gt) + ynan
    dvar = S(g1 * x) / sd + ynan
    b_ve = S(np.abs(g1) * ef + d_g) + 32 * U * S(np.abs(g))
    b_dmu = S(np.abs(g2) * ef + d_g1) + 32 * U * S(np.abs(g1))
    b_dvar = (S(np.abs(x) * (np.abs(g2) * ef + d_g1)) + 32 * U * S(np.abs(g1 * x))) / sd + np.abs(dvar) * (4 * U + efv / (2 * fv))
    b_dth = S(np.abs(gt1) * ef + d_gt) + 32 * U * S(np.abs(gt))
    return (ve, dmu, dvar, dth), (b_ve, b_dmu, b_dvar, b_dth)


def _labels(lik, par, rng, shape):
    if lik == "exponential_exp":
        return rng.exponential(size=shape)
    if lik == "gamma_exp":
        return rng.gamma(2.0, size=shape)
    if lik == "beta_probit":
        y = rng.beta(2, 3, size=shape)
        flat = y.reshape(-1)
        for i, v in enumerate((0.0, 1.0, 1e-9)):    # the clip on both sides
            if flat.size > i + 1:
                flat[i + 1] = v
        return y
    n = int(par[1])
    y = rng.integers(0, n + 1, size=shape).astype(np.float64)
    flat = y.reshape(-1)
    k = min(flat.size, n + 1)
    flat[:k] = np.arange(n, n - k, -1)              # every bin occurs, the two open ones first
    return y


def _kernel_inputs(lik, par, case):
    rows, P, per, layout = case
    rng = np.random.default_rng(rows * 31 + P)
    Y = _labels(lik, par, rng, (rows, P))
    F = rng.normal(size=(rows, P)) * (0.7 if lik in CLOSED else 1.5)
    s0 = rng.uniform(0, 0.5, size=(P, rows) if per else (rows,))
    ssq = rng.uniform(0, 0.6, size=(P, rows))
    knn = list(1.0 + 0.1 * np.arange(P)) if per else [1.2]
    return Y, F, s0, ssq, knn


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("case", T.KERNEL_CASES + [T.BIG_CASE], ids=str)
@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_zoo_varexp_sum_contract(gp, lik, par, case):
    """The contract rules of tests/test_gpu_likelihoods.py for the four new codes: every output under its derived bound, inputs
    bitwise unchanged, a second call bit-identical, rows = 0 writes [0, 0], the call without the optional operands.  The last slot of
    the table is the 70001-row grid-stride trip for the closed forms and (257, 2, per, "c") for the codes whose reference is mpmath."""
    from gpflow_amd import ops
    if case == T.BIG_CASE and lik not in CLOSED:
        case = (257, 2, True, "c")
    rows, P, per, layout = case
    Y, F, s0, ssq, knn = _kernel_inputs(lik, par, case)
    mc = 0.1
    s0c = (s0.T if per else s0[:, None]).astype(LD)
    knl = np.asarray(knn, dtype=LD)[None, :]
    fv = knl - s0c + ssq.T.astype(LD)
    efv = 2 * U * (np.abs(knl) + np.abs(s0c) + ssq.T)
    mu = F.astype(LD) + LD(mc)
    (ve, dmu, dvar, dth), (b_ve, b_dmu, b_dvar, b_dth) = _reference(lik, par, Y, mu, fv, emu=U * np.abs(mu), efv=efv)
    Yfull = np.concatenate([Y, np.full((rows, 2 if P % 2 else 1), np.nan)], axis=1) if layout == "ld" else Y
    tYf = ops.to_device(Yfull)
    tY = tYf[:, :P]
    tF, ts0, tss = ops.to_device(F), ops.to_device(s0), ops.to_device(ssq)

    def call():
        return ops.likelihood_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, lik=lik, params=par, mean_const=mc, s0_per_latent=per,
                                         want_fvar=True, want_rows=True, want_grads=True)
    out, rws, gmu, gvar, fvar = call()
    n = rows * P    # sums: the terms' own bounds + 2 (n + 2) u sum |term| for the two-stage reduction over n terms
    _within(f"{lik} out[0]", _np(out)[0:1], [ve.sum()], [b_ve.sum() + 2 * (n + 2) * U * np.abs(ve).sum()])
    _within(f"{lik} out[1]", _np(out)[1:2], [dth.sum()], [b_dth.sum() + 2 * (n + 2) * U * np.abs(dth).sum()])
    if lik == "exponential_exp":
        assert float(_np(out)[1]) == 0.0
    _within(f"{lik} rows", _np(rws), ve.sum(1), b_ve.sum(1) + 2 * (P + 2) * U * np.abs(ve).sum(1))
    _within(f"{lik} dmu", _np(gmu), dmu, b_dmu)
    _within(f"{lik} dvar", _np(gvar), dvar, b_dvar)
    _within(f"{lik} fvar", _np(fvar), fv, efv + LD(1e-300))
    for t, a in ((tYf, Yfull), (tF, F), (ts0, s0), (tss, ssq)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    again = call()
    for first, second in zip((out, rws, gmu, gvar, fvar), again):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"
    if rows == 0:
        assert _np(out).tolist() == [0.0, 0.0]
    if rows:
        only = ops.likelihood_varexp_sum(tY, tF, s0=None, ssq=None, knn=[knn[0]], lik=lik, params=par)
        assert only[1] is None and only[2] is None and only[3] is None and only[4] is None
        (ve0, _, _, _), (b0, _, _, _) = _reference(lik, par, Y, F.astype(LD), np.full((rows, P), LD(knn[0])), emu=0.0, efv=0.0)
        _within(f"{lik} out[0], fvar = knn", _np(only[0])[0:1], [ve0.sum()], [b0.sum() + 2 * (n + 2) * U * np.abs(ve0).sum()])


# ------------------------------------------------------------------------------------------------ 2. refusals
BAD_PARAMS = [("gamma_exp", (0.0,)), ("gamma_exp", (-1.0,)), ("gamma_exp", ()), ("beta_probit", (0.0,)), ("beta_probit", ()),
              ("ordinal", ()), ("ordinal", (0.6,)), ("ordinal", (0.0, 2.0, 0.0, 1.0)), ("ordinal", (-1.0, 2.0, 0.0, 1.0)),
              ("ordinal", (1.0, 2.0, 0.0)),                                       # an edge missing
              ("ordinal", (1.0, 16.0) + tuple(float(i) for i in range(16))),      # 16 edges
              ("ordinal", (1.0, 0.0)),                                            # no edge
              ("ordinal", (1.0, 2.0, 0.5, 0.5)), ("ordinal", (1.0, 3.0, 0.0, 1.0, 0.5)),   # equal, decreasing
              ("ordinal", (1.0, 2.0, 0.0, float("inf"))), ("ordinal", (1.0, 2.0, float("nan"), 1.0)),
              ("exponential_exp", (1.0,)), ("logit", ())]


def test_zoo_refuses_out_of_contract(gp):
    """A missing or non-positive shape / scale / sigma, 16 edges, equal, decreasing or non-finite edges, an unknown name: refused on
    the device and by the emulation -- through the stand-alone entry point and through the fused shard."""
    from gpflow_amd import ops
    Y = ops.to_device(np.ones((3, 2)) * 0.5)
    for lik, par in BAD_PARAMS:
        with pytest.raises(_refused()):
            ops.likelihood_varexp_sum(Y, Y, s0=None, ssq=None, knn=[1.0], lik=lik, params=par)
    Y17 = ops.to_device(np.ones((3, 17)) * 0.5)
    with pytest.raises(_refused()):
        ops.likelihood_varexp_sum(Y17, Y17, s0=None, ssq=None, knn=[1.0], lik="exponential_exp")
    Z = ops.to_device(np.random.default_rng(0).normal(size=(5, 2)))
    for lik, par in (("gamma_exp", (0.0,)), ("ordinal", (1.0, 2.0, 0.5, 0.5))):
        with pytest.raises(_refused()):
            ops.svgp_elbo_shard_lik(Z, Z, ops.to_device(np.ones((5, 1))), ops.to_device(np.zeros((5, 1))),
                                    ops.to_device(np.eye(5)[None]), variance=1.0, lengthscales=1.0, lik=lik, params=par, jitter=1e-6)


# ------------------------------------------------------------------------------------------------ 3. non-finite inputs
NONFINITE = [(i, w) for i in range(4) for w in ("Y", "fmean", "ssq")] + [(3, w) for w in ("label2.5", "label-1", "label_n+1")]


@pytest.mark.parametrize("which,where", NONFINITE, ids=[f"{LIK_IDS[i]}-{w}" for i, w in NONFINITE])
def test_zoo_varexp_sum_nonfinite(gp, which, where):
    """A NaN planted in Y, fmean or ssq -- and, Ordinal, a label that is no integer in [0, n] -- reaches out, its own row of rows_out
    and its own entry of dmu / dvar, and nothing else: every other entry is bit-identical to the clean run."""
    from gpflow_amd import ops
    lik, par = LIKS[which]
    rows, P, b, p = 41, 3, 17, 1
    Y, F, s0, ssq, knn = _kernel_inputs(lik, par, (rows, P, False, "c"))

    def run(Y, F, ssq):
        r = ops.likelihood_varexp_sum(ops.to_device(Y), ops.to_device(F), s0=ops.to_device(s0), ssq=ops.to_device(ssq), knn=knn,
                                      lik=lik, params=par, want_rows=True, want_grads=True)
        return [_np(t) for t in r[:4]]
    clean = run(Y, F, ssq)
    assert all(np.isfinite(a).all() for a in clean)
    arrs = {"Y": Y.copy(), "fmean": F.copy(), "ssq": ssq.copy()}
    if where == "ssq":
        arrs[where][p, b] = np.nan
    elif where.startswith("label"):
        arrs["Y"][b, p] = {"label2.5": 2.5, "label-1": -1.0, "label_n+1": par[1] + 1.0}[where]
    else:
        arrs[where][b, p] = np.nan
    out, rws, gmu, gvar = run(arrs["Y"], arrs["fmean"], arrs["ssq"])
    assert np.isnan(out[0])
    hit_rows = np.zeros(rows, dtype=bool); hit_rows[b] = True
    hit = np.zeros((rows, P), dtype=bool); hit[b, p] = True
    assert np.isnan(rws[b]) and np.array_equal(_bits(rws[~hit_rows]), _bits(clean[1][~hit_rows]))
    for name, got, ref in (("dmu", gmu, clean[2]), ("dvar", gvar, clean[3])):
        assert np.isnan(got[b, p]), name
        assert np.array_equal(_bits(got[~hit]), _bits(ref[~hit])), name
    if lik == "exponential_exp":
        assert out[1] == 0.0
    elif not (lik == "gamma_exp" and where == "ssq"):   # (dVE/dshape = log y - mu - psi does not read the variance)
        assert np.isnan(out[1])


# ------------------------------------------------------------------------------------------------ 5. models
def _likelihood(gp, lik, par):
    L = gp.likelihoods
    if lik == "ordinal":
        o = L.Ordinal(par[2:])
        o.sigma.assign(par[0])
        return o
    return {"exponential_exp": lambda: L.Exponential(), "gamma_exp": lambda: L.Gamma(shape=par[0]),
            "beta_probit": lambda: L.Beta(scale=par[0])}[lik]()


def _problem(lik, par, M, N, D, P, seed, q_diag, whiten=True):
    X, _, Z, q_mu, q_sqrt = T._svgp_problem("student_t", M, N, D, P, seed, q_diag, whiten)
    return X, _labels(lik, par, np.random.default_rng(seed + 1000), (N, P)), Z, q_mu, q_sqrt


def _model(gp, lik, par, Z, q_mu, q_sqrt, *, whiten=True, num_data=None, mean=0.2, shared=False, ls=0.9, var=1.3):
    k = gp.kernels.SquaredExponential(variance=var, lengthscales=ls)
    iv = gp.inducing_variables.InducingPoints(Z.copy())
    if shared:
        k = gp.kernels.SharedIndependent(k, q_mu.shape[1])
        iv = gp.inducing_variables.SharedIndependentInducingVariables(iv)
    return gp.models.SVGP(k, _likelihood(gp, lik, par), iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), q_diag=q_sqrt.ndim == 2,
                          whiten=whiten, num_data=num_data, mean_function=gp.mean_functions.Constant(mean))


def _oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, *, whiten, mean=0.2, ls=0.9, var=1.3):
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=var, lengthscales=ls, whiten=whiten, mean=mean)
    K = None if whiten else orc.Kuu(Z, variance=var, lengthscales=ls, jitter=orc.DEFAULT_JITTER)
    kl = orc.gauss_kl(q_mu, q_sqrt, K)
    ve = _reference(lik, par, Y, fmean, fvar, fns=_f64_fns())[0][0]
    return float(ve.sum()), float(kl)


@pytest.mark.parametrize("P,shared", [(1, False), (4, True)], ids=["P1", "shared4"])
@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "qdiag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["white", "unwhite"])
@pytest.mark.parametrize("lik,par", MODEL_LIKS, ids=MODEL_IDS)
def test_zoo_svgp_elbo_against_oracle_and_quadrature(gp, lik, par, whiten, q_diag, P, shared):
    """SVGP.elbo through gpk_svgp_elbo_shard_lik in every form of the shard, 1e-8 relative (the project's ELBO bar); a two-shard
    split of the rows sums to the one-shard terms."""
    M, N, D = 40, 150, 2
    X, Y, Z, q_mu, q_sqrt = _problem(lik, par, M, N, D, P, 11, q_diag, whiten)
    ve, kl = _oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, whiten=whiten)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, whiten=whiten, num_data=5000, shared=shared)
    assert m._fused_config() is not None
    ref = ve * 5000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"elbo {got!r} reference {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
    whole = _np(m.elbo_terms((X, Y)))
    a, b = _np(m.elbo_terms((X[:70], Y[:70]))), _np(m.elbo_terms((X[70:], Y[70:])))
    assert abs(a[0] + b[0] - whole[0]) <= 1e-12 * abs(ve) * 50 and a[1] == whole[1] == b[1]
    assert abs(whole[1] - kl) <= 1e-9 * abs(kl)


def test_zoo_svgp_elbo_composed_path(gp):
    """SeparateIndependent kernels: the composed path through likelihood.variational_expectations (the same kernel)."""
    lik, par = LIKS[2]
    M, N, D, P = 30, 90, 2, 2
    X, Y, Z, q_mu, q_sqrt = _problem(lik, par, M, N, D, P, 12, False)
    hyp = [(1.3, 0.9), (0.7, 1.4)]
    k = gp.kernels.SeparateIndependent([gp.kernels.SquaredExponential(variance=v, lengthscales=l) for v, l in hyp])
    iv = gp.inducing_variables.SharedIndependentInducingVariables(gp.inducing_variables.InducingPoints(Z.copy()))
    m = gp.models.SVGP(k, _likelihood(gp, lik, par), iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), whiten=True)
    assert m._fused_config() is None
    ve = kl = 0.0
    for p, (v, l) in enumerate(hyp):
        a, b = _oracle_terms(lik, par, X, Y[:, p:p + 1], Z, q_mu[:, p:p + 1], q_sqrt[p:p + 1], whiten=True, mean=0.0, ls=l, var=v)
        ve, kl = ve + a, kl + b
    assert abs(float(m.elbo((X, Y))) - (ve - kl)) <= 1e-8 * abs(ve - kl)
    with pytest.raises(NotImplementedError):
        m.elbo_and_grad((X, Y))


def _ld_density_terms(lik, par, f, y):
    """(E[y|f], Var[y|f], log p(y|f)) of the contract at nodes f [..., H] with labels y [..., 1], longdouble over scipy's functions"""
    fn = _f64_fns()
    if lik in CLOSED:
        sh = LD(par[0]) if par else LD(1)
        lam = np.exp(f)
        lg = fn["lgamma"](np.array([sh]))[0]
        return sh * lam, sh * lam * lam, -sh * f - lg + (sh - 1) * np.log(y) - y / lam
    if lik == "beta_probit":
        s = LD(par[0])
        m = fn["erfc"](-f / np.sqrt(LD(2))) / 2 * A998 + LD("1e-3")
        yc = np.clip(y, LD(1e-6), LD(1.0 - 1e-6))
        lp = (m * s - 1) * np.log(yc) + (s - m * s - 1) * np.log(1 - yc) + fn["lgamma"](np.array([s]))[0] - fn["lgamma"](m * s) \
            - fn["lgamma"](s - m * s)
        return m, (m - m * m) / (s + 1), lp
    sig, n = LD(par[0]), int(par[1])
    e = np.asarray(par[2:], dtype=LD)
    Phi = lambda z: fn["erfc"](-z / np.sqrt(LD(2))) / 2 * A998 + LD("1e-3")   # noqa: E731
    left = np.concatenate([Phi((e - f[..., None]) / sig), np.full(f.shape + (1,), 1 - LD("1e-3"))], axis=-1)
    right = np.concatenate([np.full(f.shape + (1,), LD("1e-3")), Phi((e - f[..., None]) / sig)], axis=-1)
    phi = left - right                                     # [..., H, n + 1]
    k = np.arange(n + 1).astype(LD)
    mean = (phi * k).sum(-1)
    yi = np.broadcast_to(y, f.shape).astype(np.int64)
    return mean, (phi * k * k).sum(-1) - mean * mean, np.log(np.take_along_axis(phi, yi[..., None], axis=-1)[..., 0] + LD("1e-6"))


@pytest.mark.parametrize("lik,par", MODEL_LIKS, ids=MODEL_IDS)
def test_zoo_predict_y_and_log_density(gp, lik, par):
    """predict_y / predict_log_density through the base class's 20-node sums, against the same sums of the oracle's q(f) in
    longdouble: 1e-8 absolute on O(1) quantities, the bar of tests/test_gpu_likelihoods.py."""
    M, N, D, P = 40, 60, 2, 2
    X, Y, Z, q_mu, q_sqrt = _problem(lik, par, M, N, D, P, 14, False)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, shared=True)
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=1.3, lengthscales=0.9, mean=0.2)
    mu, v = fmean.astype(LD), fvar.astype(LD)
    x, wn = GH_X.astype(LD), GH_W.astype(LD) / np.sqrt(PI)
    f = mu[..., None] + np.sqrt(2 * v)[..., None] * x
    cm, cv, lp = _ld_density_terms(lik, par, f, Y.astype(LD)[..., None])
    E = (cm * wn).sum(-1)
    V = ((cv + cm * cm) * wn).sum(-1) - E * E
    t = np.log(wn) + lp
    top = t.max(-1, keepdims=True)
    lden = (top[..., 0] + np.log(np.exp(t - top).sum(-1))).sum(1)
    gE, gV = m.predict_y(X)
    gl = m.predict_log_density((X, Y))
    assert gl.shape == (N,)
    for name, got, ref in (("E_y", gE, E), ("V_y", gV, V), ("log density", gl, lden)):
        err = float(np.abs(_np(got).astype(LD) - ref).max() / max(1.0, float(np.abs(ref).max())))
        print(f"{lik} predict {name}: max error {err:.3g}")
        assert err <= 1e-8, name


def test_zoo_exp_link_predictions_against_lognormal_closed_forms(gp):
    """Exponential / Gamma predict_mean_and_var integrate shape exp(f) and shape exp(2 f) (1 + shape) against N(mu, v): the lognormal
    moments E_y = shape exp(mu + v / 2), E[y^2] = shape (1 + shape) exp(2 mu + 2 v).  For v <= 0.5 the 20-node truncation of
    exp(2 f) (a = 2 sqrt(2 v) <= 2: remainder a^40 20! / (40! 2^20) < 1e-17 relative) is negligible and rounding is left: exp 3 ulp
    with an argument error u |f|, the products and the sum -- (32 + 2 fmax) u of the positive terms; the variance subtracts E_y^2."""
    from gpflow_amd import ops
    rng = np.random.default_rng(3)
    mu, v = rng.normal(size=(200, 2)), rng.uniform(0.01, 0.5, size=(200, 2))
    for lik, sh in ((gp.likelihoods.Exponential(), 1.0), (gp.likelihoods.Gamma(shape=1.7), 1.7)):
        E, V = lik.predict_mean_and_var(None, ops.to_device(mu), ops.to_device(v))
        s = LD(sh)
        Er = s * np.exp(mu.astype(LD) + v.astype(LD) / 2)
        E2 = s * (1 + s) * np.exp(2 * mu.astype(LD) + 2 * v.astype(LD))
        fmax = np.abs(mu) + np.sqrt(2 * v) * np.abs(GH_X).max()
        _within(f"{type(lik).__name__} E_y", _np(E), Er, (32 + fmax) * U * Er)
        _within(f"{type(lik).__name__} V_y", _np(V), E2 - Er * Er, (32 + 2 * fmax) * U * (E2 + 2 * Er * Er) + LD(1e-17) * E2)


def test_zoo_ordinal_phi_rows_sum_to_one_minus_jitters(gp):
    """Ordinal._make_phi: the bin probabilities telescope to inv_probit(+inf) - inv_probit(-inf) = 0.998; n + 1 differences of values
    <= 1, each an erf of 16 ulp: (n + 1) 24 u."""
    from gpflow_amd import ops
    lik = _likelihood(gp, "ordinal", LIKS[3][1])
    F = np.random.default_rng(5).normal(size=(50, 2)) * 2
    phi = _np(lik._make_phi(ops.to_device(F)))
    assert phi.shape == (50, 2, 6) and (phi >= -48 * U).all()    # (a far bin is the difference of two rounded values near 0 or 1)
    assert np.abs(phi.sum(-1) - 0.998).max() <= 6 * 24 * U


# ------------------------------------------------------------------------------------------------ 6. gradients
def _torch_ve(lik, par, fmean, fvar, Y):
    """sum of the variational expectations of the contract on torch-CPU fp64 tensors (par: floats, the trainable one a tensor)"""
    if lik in CLOSED:
        ye = Y * torch.exp(-fmean + fvar / 2)
        if lik == "exponential_exp":
            return (-fmean - ye).sum()
        sh = par[0]
        return (-sh * fmean - torch.lgamma(sh) + (sh - 1) * torch.log(Y) - ye).sum()
    x, wn = torch.tensor(GH_X), torch.tensor(GH_W / np.sqrt(np.pi))
    f = fmean[..., None] + torch.sqrt(2 * fvar)[..., None] * x
    y = Y[..., None]
    Phi = lambda z: 0.5 * torch.special.erfc(-z / math.sqrt(2.0))   # noqa: E731
    if lik == "beta_probit":
        s = par[0]
        m = Phi(f) * (1 - 2e-3) + 1e-3
        al, be = m * s, s - m * s
        yc = torch.clamp(y, 1e-6, 1 - 1e-6)
        g = (al - 1) * torch.log(yc) + (be - 1) * torch.log(1 - yc) + torch.lgamma(s) - torch.lgamma(al) - torch.lgamma(be)
    else:
        sig, n = par[0], int(par[1])
        e = torch.tensor(np.asarray(par[2:], dtype=np.float64))
        yi = Y.long()
        has_l, has_r = (yi < n)[..., None], (yi > 0)[..., None]
        el = torch.cat([e, torch.zeros(1, dtype=torch.float64)])[yi][..., None]     # (finite stand-ins at the open ends: an
        er = torch.cat([torch.zeros(1, dtype=torch.float64), e])[yi][..., None]     #  infinite z would put 0 * inf into the graph)
        Pl = torch.where(has_l, Phi((el - f) / sig), torch.ones_like(f))
        Pr = torch.where(has_r, Phi((er - f) / sig), torch.zeros_like(f))
        g = torch.log((1 - 2e-3) * (Pl - Pr) + 1e-6)
    return (g * wn).sum()


def _torch_elbo(lik, par, X, Y, Z, q_mu, q_sqrt, variance, ls, mean, *, num_data, jitter=1e-6):
    """the whitened ELBO as tests/test_gpu_likelihoods.py::_torch_elbo writes it, with the stages of this file"""
    M, B = Z.shape[0], X.shape[0]
    Kmm = orcg._rbf(Z, Z, variance, ls) + jitter * torch.eye(M, dtype=torch.float64)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kmm), orcg._rbf(Z, X, variance, ls), upper=False)
    fvar = variance - (A * A).sum(0)
    fmean = A.T @ q_mu + mean
    P = q_mu.shape[1]
    if q_sqrt.dim() == 2:
        LTA = A[None, :, :] * q_sqrt.T[:, :, None]
        kl = 0.5 * ((q_mu * q_mu).sum() - M * P - torch.log(q_sqrt ** 2).sum() + (q_sqrt ** 2).sum())
    else:
        Lq = torch.tril(q_sqrt)
        LTA = Lq.transpose(1, 2) @ A
        kl = 0.5 * ((q_mu * q_mu).sum() - M * P - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())
    fvar = (fvar[None, :] + (LTA * LTA).sum(1)).T
    return _torch_ve(lik, par, fmean, fvar, Y) * (num_data / B) - kl


def _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, *, variance, ls, mean, num_data):
    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    v = {"Z": t(Z, True), "q_mu": t(q_mu, True), "q_sqrt": t(q_sqrt, True), "variance": t(variance, True),
         "lengthscales": t(np.atleast_1d(ls), True), "mean_const": t(mean, True)}
    tpar = par
    if lik in GRAD_NAME:
        v[GRAD_NAME[lik]] = t(par[0], True)
        tpar = (v[GRAD_NAME[lik]],) + tuple(par[1:])
    F = _torch_elbo(lik, tpar, t(X), t(Y), v["Z"], v["q_mu"], v["q_sqrt"], v["variance"], v["lengthscales"], v["mean_const"],
                    num_data=num_data)
    F.backward()
    return float(F.detach()), {k: a.grad.detach().numpy().copy() for k, a in v.items()}


@pytest.mark.parametrize("M,B,D,P,q_diag,ard", [(150, 300, 3, 2, False, True), (64, 200, 2, 1, True, False),
                                                (130, 140, 2, 3, True, True)], ids=["full-P2", "qdiag-P1", "qdiag-P3"])
@pytest.mark.parametrize("lik,par", MODEL_LIKS, ids=MODEL_IDS)
def test_zoo_svgp_elbo_and_grad_vs_autograd(gp, lik, par, M, B, D, P, q_diag, ard):
    """gradients.svgp_elbo_and_grad(likelihood=...) against autograd of the restated ELBO at the project's whitened tolerances: value
    1e-9 relative, every gradient 1e-8 of max(1, its largest entry) -- the Gamma shape, Beta scale and Ordinal sigma included."""
    from gpflow_amd import gradients, ops
    X, Y, Z, q_mu, q_sqrt = _problem(lik, par, M, B, D, P, 21, q_diag)
    ls = np.sqrt(D) * (0.8 + 0.05 * np.arange(D)) if ard else 1.3
    t = ops.to_device
    q_in = q_sqrt if q_diag else q_sqrt + np.triu(np.ones((M, M)), 1)[None] * 0.37   # junk above the diagonal is ignored
    F, g, info = gradients.svgp_elbo_and_grad(t(Z), t(X), t(Y), t(q_mu), t(q_in), variance=1.3, lengthscales=ls, noise_variance=None,
                                              jitter=1e-6, scale=1000.0 / B, mean_const=0.1, likelihood=(lik, par))
    ops.check_info(info)
    v, go = _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=ls, mean=0.1, num_data=1000)
    print(f"value {float(F.cpu()[0])!r} autograd {v!r}")
    assert abs(float(F.cpu()[0]) - v) <= 1e-9 * abs(v)
    assert "noise_variance" not in g and set(g) == set(go)
    for name, ref in go.items():
        got = _np(g[name]).reshape(ref.shape)
        tol = 1e-8 * max(1.0, np.abs(ref).max())
        print(f"{name}: max error {np.abs(got - ref).max():.3g} tolerance {tol:.3g}")
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=name)


@pytest.mark.parametrize("lik,par", MODEL_LIKS[1:], ids=MODEL_IDS[1:])
def test_zoo_model_elbo_and_grad_chains_the_transform(gp, lik, par):
    """SVGP.elbo_and_grad: value == the fused forward, and the likelihood's own Parameter (named by the class's `device_grad_param`)
    is among the gradients, chained through its positive transform."""
    X, Y, Z, q_mu, q_sqrt = _problem(lik, par, 50, 180, 2, 1, 32, False)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, num_data=2000)
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - float(m.elbo((X, Y)))) <= 1e-9 * abs(v)
    _, go = _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=0.9, mean=0.2, num_data=2000)
    name = type(m.likelihood).device_grad_param
    assert "likelihood_" + name == GRAD_NAME[lik]
    prm = getattr(m.likelihood, name)
    assert prm in g and m.q_sqrt in g and m.inducing_variable.Z in g
    ref = go[GRAD_NAME[lik]] * prm.transform.forward_grad(prm.unconstrained_variable)
    np.testing.assert_allclose(np.ravel(g[prm]), np.ravel(ref), rtol=0, atol=1e-8 * max(1.0, abs(float(ref))))
    np.testing.assert_allclose(g[m.inducing_variable.Z], go["Z"], rtol=0, atol=1e-8 * max(1.0, np.abs(go["Z"]).max()))


def test_zoo_scipy_optimiser_gamma_and_ordinal(gp):
    """optimizers.Scipy raises the ELBO of a small Gamma regression and of a three-grade Ordinal set monotonically over successive
    short runs; the Ordinal model's predict_y mean orders the grades of the separable set."""
    rng = np.random.default_rng(41)
    Xg = rng.uniform(-2, 2, size=(80, 1))
    Yg = rng.gamma(2.0, np.exp(np.sin(2 * Xg)) / 2.0)
    mg = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=1.0), gp.likelihoods.Gamma(shape=1.5), Xg[::8].copy())
    Xo = np.concatenate([rng.normal(size=(40, 1)) * 0.25 + c for c in (-2.0, 0.0, 2.0)])
    Yo = np.repeat(np.arange(3.0), 40)[:, None]
    mo = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=1.0), gp.likelihoods.Ordinal([-1.0, 1.0]), Xo[::10].copy())
    for m, data in ((mg, (Xg, Yg)), (mo, (Xo, Yo))):
        vals = [float(m.elbo(data))]
        for _ in range(5):
            gp.optimizers.Scipy().minimize(m, data, options=dict(maxiter=3))
            vals.append(float(m.elbo(data)))
        print("ELBO per round:", vals)
        assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0] + 1
    mean = _np(mo.predict_y(Xo)[0])[:, 0]
    assert mean[:40].max() < mean[40:80].min() and mean[40:80].max() < mean[80:].min()
