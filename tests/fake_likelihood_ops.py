"""CPU emulation of the likelihood primitives of `gpflow_amd.ops` -- TEST INFRASTRUCTURE ONLY, the companion of tests/fake_ops.py
for `gauss_hermite`, `likelihood_varexp_sum` and `svgp_elbo_shard_lik` (include/gpk.h: gpk_gauss_hermite,
gpk_likelihood_varexp_sum, gpk_svgp_elbo_shard_lik).  NumPy fp64, written from the stated contract:

  * fvar = knn - s0 + ssq, mu = fmean + mean_const; no clamp of fvar (a negative value gives NaN through the square root);
  * "bernoulli_probit" and "student_t": sum_h (w_h / sqrt pi) g(mu + sqrt(2 fvar) x_h) over hermgauss(20), with the exact
    derivatives of that sum w.r.t. mu and fvar; "poisson_exp": the closed form;
  * a non-finite label adds y - y to every output of its element; NaN / Inf in fmean / fvar travel through the arithmetic;
  * what the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED) is an AssertionError here.
The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import scipy.special as sps
import torch

import fake_ops

LIKELIHOOD_CODES = {"bernoulli_probit": 1, "poisson_exp": 2, "student_t": 3}
_NPAR = {"bernoulli_probit": 0, "poisson_exp": 1, "student_t": 2}


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def gauss_hermite(n=20):
    assert n == 20, n    # gpk_gauss_hermite: GPK_E_UNSUPPORTED
    return np.polynomial.hermite.hermgauss(20)


def _check_lik(lik, params):
    assert lik in LIKELIHOOD_CODES, lik
    params = [float(v) for v in params]
    assert len(params) == _NPAR[lik], (lik, params)
    assert all(v > 0.0 for v in params), params    # binsize / scale / df: GPK_E_ARG
    return params


def likelihood_varexp_sum(Y, fmean, *, s0, ssq, knn, lik, params=(), mean_const=0.0, s0_per_latent=False, want_fvar=False,
                          want_rows=False, want_grads=False):
    rows, P = fmean.shape
    assert 1 <= P <= 16, P    # gpk_likelihood_varexp_sum: GPK_E_ARG outside 1 .. 16 latents
    par = _check_lik(lik, params)
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
        dsc = np.zeros_like(mu)
        if lik == "poisson_exp":
            e = np.exp(mu + 0.5 * fv) * par[0]
            ve = y * mu - e - sps.gammaln(y + 1.0) + y * np.log(par[0])
            dmu, dvar = y - e, -0.5 * e
        else:
            x, w = gauss_hermite(20)
            wn = w / np.sqrt(np.pi)
            sd = np.sqrt(2.0 * fv)
            f = mu[..., None] + sd[..., None] * x
            if lik == "bernoulli_probit":
                sgn = np.where(y == 1.0, 1.0, -1.0)[..., None]
                q = 0.5 * sps.erfc(-sgn * f / np.sqrt(2.0)) * (1.0 - 2e-3) + 1e-3
                g = np.log(q)
                gp = sgn * (1.0 - 2e-3) * np.exp(-0.5 * f * f) / np.sqrt(2.0 * np.pi) / q
            else:
                scale, df = par
                r = (y[..., None] - f) / scale
                c0 = sps.gammaln(0.5 * (df + 1.0)) - sps.gammaln(0.5 * df) - 0.5 * (np.log(scale * scale) + np.log(df) + np.log(np.pi))
                g = c0 - 0.5 * (df + 1.0) * np.log1p(r * r / df)
                gp = (df + 1.0) * r / (scale * (df + r * r))
                dsc = ((((df + 1.0) * r * r / (df + r * r) - 1.0) / scale) * wn).sum(-1)
            ve = (g * wn).sum(-1)
            dmu = (gp * wn).sum(-1)
            dvar = (gp * x * wn).sum(-1) / sd
        ve, dmu, dvar = ve + ynan, dmu + ynan, dvar + ynan
        out = torch.tensor([ve.sum(), dsc.sum()], dtype=torch.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    return (out, t(ve.sum(1)) if want_rows else None, t(dmu) if want_grads else None, t(dvar) if want_grads else None,
            t(fv) if want_fvar else None)


def svgp_elbo_shard_lik(Z, Xb, Yb, q_mu, q_sqrt, *, variance, lengthscales, lik, params=(), jitter, mean_const=0.0,
                        family="SquaredExponential", ws=None, out=None, info=None, whiten=True):
    """gpk_svgp_elbo_shard_lik is gpk_svgp_elbo_shard with another last stage; so is its emulation: fake_ops.svgp_elbo_shard
    runs with its `gaussian_varexp_sum` replaced by the quadrature stage for the duration of the call."""
    _check_lik(lik, params)

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
