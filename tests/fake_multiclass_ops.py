"""CPU emulation of the MultiClass / RobustMax code of the likelihood primitives -- TEST INFRASTRUCTURE ONLY, the companion of
tests/fake_likelihood_ops.py for lik = "multiclass_robustmax" (include/gpk.h: GPK_LIK_MULTICLASS_ROBUSTMAX).  `likelihood_varexp_sum`
and `svgp_elbo_shard_lik` delegate the three scalar codes to fake_likelihood_ops; the new one is NumPy fp64 written from the stated
contract:

  * P = number of classes, 2 <= P <= 16; params = (epsilon,), 0 < epsilon < 1; Y has ONE column, the label of the row;
  * fvar = knn - s0 + ssq is returned unclamped; the value clamps 2 fvar_y and fvar_k at 1e-10 by COMPARISON (a NaN stays NaN),
    and where a clamp is active the derivative w.r.t. that variance is exactly 0;
  * VE_b = p log(1 - eps) + (1 - p) log(eps / (P - 1)), p = sum_h (w_h / sqrt pi) prod_{k != y} c_kh, with the exact derivatives of
    that sum w.r.t. all P means and variances of the row;
  * out = [sum_b VE_b, 0]; a label that is no integer in [0, P) makes every output of its row NaN, and nothing else;
  * what the device refuses (GPK_E_ARG) is an AssertionError here.
The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import scipy.special as sps
import torch

import fake_likelihood_ops
import fake_ops

NAME = "multiclass_robustmax"
_np = fake_likelihood_ops._np


def _check(P, params):
    params = [float(v) for v in params]
    assert len(params) == 1, params                # a missing epsilon: GPK_E_ARG
    assert 0.0 < params[0] < 1.0, params           # GPK_E_ARG
    assert 2 <= P <= 16, P                         # GPK_E_ARG
    return params[0]


def _clamp(v, lo):
    """max(v, lo) as a comparison: NaN stays NaN.  Returns (clamped, clamp active)"""
    active = v < lo
    return np.where(active, lo, v), active


def likelihood_varexp_sum(Y, fmean, *, s0, ssq, knn, lik, params=(), mean_const=0.0, s0_per_latent=False, want_fvar=False,
                          want_rows=False, want_grads=False):
    if lik != NAME:
        return fake_likelihood_ops.likelihood_varexp_sum(Y, fmean, s0=s0, ssq=ssq, knn=knn, lik=lik, params=params,
                                                         mean_const=mean_const, s0_per_latent=s0_per_latent, want_fvar=want_fvar,
                                                         want_rows=want_rows, want_grads=want_grads)
    rows, P = fmean.shape
    eps = _check(P, params)
    knn = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=np.float64)), (P,))
    fv = np.tile(knn[None, :], (rows, 1)).astype(np.float64)
    if s0 is not None:
        fv = fv - (_np(s0).T if s0_per_latent else _np(s0)[:, None])
    if ssq is not None:
        fv = fv + _np(ssq).T
    mu = _np(fmean) + mean_const
    y = _np(Y)[:, 0] if rows else np.zeros(0)
    with np.errstate(all="ignore"):
        ok = (y >= 0) & (y < P) & (y == np.floor(y))
        yi = np.where(ok, y, 0).astype(np.int64)
        ynan = np.where(ok, 0.0, np.nan)
        on = np.zeros((rows, P), dtype=bool)
        on[np.arange(rows), yi] = True
        x, w = np.polynomial.hermite.hermgauss(20)
        wn = w / np.sqrt(np.pi)
        mu_y, fv_y = mu[on], fv[on]
        tv, cy = _clamp(2.0 * fv_y, 1e-10)
        vk, ck = _clamp(fv, 1e-10)
        s, sdk = np.sqrt(tv), np.sqrt(vk)
        X = mu_y[:, None] + s[:, None] * x                                             # [rows, H]
        d = (X[:, None, :] - mu[:, :, None]) / sdk[:, :, None]                         # [rows, P, H]
        c = 0.5 * sps.erfc(-d / np.sqrt(2.0)) * (1.0 - 2e-4) + 1e-4
        t = (1.0 - 2e-4) * np.exp(-0.5 * d * d) / np.sqrt(2.0 * np.pi) / (sdk[:, :, None] * c)
        c = np.where(on[:, :, None], 1.0, c)
        t = np.where(on[:, :, None], 0.0, t)
        wp = np.prod(c, axis=1) * wn                                                   # [rows, H]
        p = wp.sum(-1)
        l1, l0 = np.log1p(-eps), np.log(eps / (P - 1))
        kap = l1 - l0
        ve = p * l1 + (1.0 - p) * l0 + ynan
        a1 = (wp[:, None, :] * t).sum(-1)                                              # [rows, P]
        a2 = (wp[:, None, :] * t * d).sum(-1)
        a3 = (wp[:, None, :] * t * x).sum(-1)
        dmu = np.where(on, kap * a1.sum(1, keepdims=True), -kap * a1)
        dvar_y = np.where(cy, 0.0, kap * a3.sum(1) / s)
        dvar_k = np.where(ck, 0.0, -kap * a2 / (2.0 * sdk))
        dvar = np.where(on, dvar_y[:, None], dvar_k)
        dmu, dvar = dmu + ynan[:, None], dvar + ynan[:, None]
        out = torch.tensor([ve.sum(), 0.0], dtype=torch.float64)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    return (out, t_(ve) if want_rows else None, t_(dmu) if want_grads else None, t_(dvar) if want_grads else None,
            t_(fv) if want_fvar else None)


def svgp_elbo_shard_lik(Z, Xb, Yb, q_mu, q_sqrt, *, variance, lengthscales, lik, params=(), jitter, mean_const=0.0,
                        family="SquaredExponential", ws=None, out=None, info=None, whiten=True):
    """the stage swap of fake_likelihood_ops.svgp_elbo_shard_lik with the MultiClass stage: fake_ops.svgp_elbo_shard runs with its
    `gaussian_varexp_sum` replaced for the duration of the call."""
    if lik != NAME:
        return fake_likelihood_ops.svgp_elbo_shard_lik(Z, Xb, Yb, q_mu, q_sqrt, variance=variance, lengthscales=lengthscales, lik=lik,
                                                       params=params, jitter=jitter, mean_const=mean_const, family=family, ws=ws,
                                                       out=out, info=info, whiten=whiten)
    _check(q_mu.shape[1], params)
    assert Yb.shape[1] == 1, Yb.shape

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
