"""CPU emulation of the Exponential / Gamma / Beta / Ordinal codes of the likelihood primitives -- TEST INFRASTRUCTURE ONLY, the
companion of tests/fake_multiclass_ops.py for lik = "exponential_exp", "gamma_exp", "beta_probit", "ordinal" (include/gpk.h:
GPK_LIK_EXPONENTIAL_EXP .. GPK_LIK_ORDINAL).  `likelihood_varexp_sum` and `svgp_elbo_shard_lik` delegate every other name to
fake_multiclass_ops (which delegates the three first scalar codes to fake_likelihood_ops); the new ones are NumPy fp64 written from
the stated contract, with scipy's erfc / gammaln / digamma:

  * fvar = knn - s0 + ssq unclamped, mu = fmean + mean_const, e = exp(-mu + fvar / 2);
  * "exponential_exp", "gamma_exp": the closed forms; "beta_probit", "ordinal": the 20-node sums with the exact derivatives of the
    sum w.r.t. mu and fvar;
  * out[1] = the sum of dVE/dtheta of the code's one trainable parameter (shape, scale, sigma), 0.0 for "exponential_exp";
  * a non-finite label adds y - y to every output of its element; an Ordinal label that is no integer in [0, n] makes its element's
    outputs NaN (out[1] included);
  * what the device refuses (GPK_E_ARG) is an AssertionError here.
The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import scipy.special as sps
import torch

import fake_multiclass_ops
import fake_ops

NAMES = ("exponential_exp", "gamma_exp", "beta_probit", "ordinal")
_np = fake_multiclass_ops._np


def _check(lik, params):
    params = [float(v) for v in params]
    if lik == "exponential_exp":
        assert len(params) == 0, params
    elif lik in ("gamma_exp", "beta_probit"):
        assert len(params) == 1 and params[0] > 0.0, params            # a missing or non-positive shape / scale: GPK_E_ARG
    else:
        assert len(params) >= 2 and params[0] > 0.0, params            # sigma
        n = params[1]
        assert n == np.floor(n) and 1 <= n <= 15, params               # 1 .. 15 edges
        assert len(params) == 2 + int(n), params
        e = np.asarray(params[2:])
        assert np.isfinite(e).all() and (np.diff(e) > 0).all(), params  # finite, strictly increasing
    return params


def likelihood_varexp_sum(Y, fmean, *, s0, ssq, knn, lik, params=(), mean_const=0.0, s0_per_latent=False, want_fvar=False,
                          want_rows=False, want_grads=False):
    if lik not in NAMES:
        return fake_multiclass_ops.likelihood_varexp_sum(Y, fmean, s0=s0, ssq=ssq, knn=knn, lik=lik, params=params,
                                                         mean_const=mean_const, s0_per_latent=s0_per_latent, want_fvar=want_fvar,
                                                         want_rows=want_rows, want_grads=want_grads)
    rows, P = fmean.shape
    assert 1 <= P <= 16, P
    par = _check(lik, params)
    knn = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=np.float64)), (P,))
    fv = np.tile(knn[None, :], (rows, 1)).astype(np.float64)
    if s0 is not None:
        fv = fv - (_np(s0).T if s0_per_latent else _np(s0)[:, None])
    if ssq is not None:
        fv = fv + _np(ssq).T
    mu = _np(fmean) + mean_const
    y = _np(Y)[:, :P]
    with np.errstate(all="ignore"):
        ynan = y - y
        dth = np.zeros_like(mu)
        if lik in ("exponential_exp", "gamma_exp"):
            ye = y * np.exp(-mu + 0.5 * fv)
            if lik == "exponential_exp":
                ve, dmu = -mu - ye, ye - 1.0
            else:
                shape = par[0]
                ve = -shape * mu - sps.gammaln(shape) + (shape - 1.0) * np.log(y) - ye
                dmu = ye - shape
                dth = np.log(y) - mu - sps.digamma(shape)
            dvar = -0.5 * ye
        else:
            x, w = np.polynomial.hermite.hermgauss(20)
            wn = w / np.sqrt(np.pi)
            sd = np.sqrt(2.0 * fv)
            f = mu[..., None] + sd[..., None] * x
            phi = lambda z: np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)   # noqa: E731
            if lik == "beta_probit":
                scale = par[0]
                m = 0.5 * sps.erfc(-f / np.sqrt(2.0)) * (1.0 - 2e-3) + 1e-3
                al = m * scale
                be = scale - al
                yc = np.where(y < 1e-6, 1e-6, np.where(y > 1.0 - 1e-6, 1.0 - 1e-6, y))[..., None]
                ly, l1 = np.log(yc), np.log(1.0 - yc)
                pa, pb = sps.digamma(al), sps.digamma(be)
                g = (al - 1.0) * ly + (be - 1.0) * l1 + sps.gammaln(scale) - sps.gammaln(al) - sps.gammaln(be)
                gp = scale * (1.0 - 2e-3) * phi(f) * (ly - l1 - pa + pb)
                gt = m * ly + (1.0 - m) * l1 + sps.digamma(scale) - m * pa - (1.0 - m) * pb
            else:
                sigma, n = par[0], int(par[1])
                ok = (y >= 0) & (y <= n) & (y == np.floor(y))
                yi = np.where(ok, y, 0).astype(np.int64)
                ynan = np.where(ok, 0.0, np.nan)
                left = np.concatenate([par[2:], [np.inf]])[yi][..., None]
                right = np.concatenate([[-np.inf], par[2:]])[yi][..., None]
                zl, zr = (left - f) / sigma, (right - f) / sigma
                up = zr >= 0
                za, zb = np.where(up, zr, -zl), np.where(up, zl, -zr)
                D = (1.0 - 2e-3) * 0.5 * (sps.erfc(za / np.sqrt(2.0)) - sps.erfc(zb / np.sqrt(2.0)))
                pl = np.where(np.isfinite(left), phi(zl), 0.0)
                pr = np.where(np.isfinite(right), phi(zr), 0.0)
                tl = np.where(np.isfinite(left), zl * pl, 0.0)
                tr = np.where(np.isfinite(right), zr * pr, 0.0)
                den = sigma * (D + 1e-6)
                g = np.log(D + 1e-6)
                gp = -(1.0 - 2e-3) * (pl - pr) / den
                gt = -(1.0 - 2e-3) * (tl - tr) / den
            ve = (g * wn).sum(-1)
            dmu = (gp * wn).sum(-1)
            dvar = (gp * x * wn).sum(-1) / sd
            dth = (gt * wn).sum(-1)
            if lik == "ordinal":
                dth = dth + ynan
        ve, dmu, dvar = ve + ynan, dmu + ynan, dvar + ynan
        out = torch.tensor([ve.sum(), dth.sum() if lik != "exponential_exp" else 0.0], dtype=torch.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    return (out, t(ve.sum(1)) if want_rows else None, t(dmu) if want_grads else None, t(dvar) if want_grads else None,
            t(fv) if want_fvar else None)


def svgp_elbo_shard_lik(Z, Xb, Yb, q_mu, q_sqrt, *, variance, lengthscales, lik, params=(), jitter, mean_const=0.0,
                        family="SquaredExponential", ws=None, out=None, info=None, whiten=True):
    """the stage swap of fake_likelihood_ops.svgp_elbo_shard_lik with the stages of this file: fake_ops.svgp_elbo_shard runs with its
    `gaussian_varexp_sum` replaced for the duration of the call."""
    if lik not in NAMES:
        return fake_multiclass_ops.svgp_elbo_shard_lik(Z, Xb, Yb, q_mu, q_sqrt, variance=variance, lengthscales=lengthscales, lik=lik,
                                                       params=params, jitter=jitter, mean_const=mean_const, family=family, ws=ws,
                                                       out=out, info=info, whiten=whiten)
    _check(lik, params)

    def stage(Y, fmean, *, s0, ssq, knn, noise_variance, mean_const=0.0, s0_per_latent=False, want_fvar=False):
        res = likelihood_varexp_sum(Y, fmean, s0=s0, ssq=ssq, knn=knn, lik=lik, params=params, mean_const=mean_const,
                                    s0_per_latent=s0_per_latent, want_fvar=want_fvar)
        return res[0][0:1], res[4]

    saved = fake_ops.gaussian_varexp_sum
    fake_ops.gaussian_varexp_sum = stage
    try:
        return fake_ops.svgp_elbo_shard(Z, Xb, Yb, q_mu, q_sqrt, variance=variance, lengthscales=lengthscales, noise_variance=1.0,
                                        jitter=jitter, mean_const=mean_const, family=family, ws=ws, out=out, info=info, whiten=whiten)
    finally:
        fake_ops.gaussian_varexp_sum = saved
