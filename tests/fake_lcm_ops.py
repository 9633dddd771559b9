"""CPU emulation of the LinearCoregionalization primitives -- TEST INFRASTRUCTURE ONLY: `mixed_gaussian_varexp_sum`,
`svgp_elbo_shard_lcm` and `svgp_elbo_lcm_workspace` of gpflow_amd/ops.py in NumPy fp64, written from the contract in include/gpk.h
(gpk_mixed_gaussian_varexp_sum, gpk_svgp_elbo_shard_lcm):

  * L latents, P outputs, W [P, L], 1 <= L, P <= 16; gvar = knn - s0 + ssq over the latents (in this order);
  * f = gmean W^T + mean_const (the constant AFTER the mixing), fvar = gvar (W^2)^T, not clamped;
  * out = [sum VE, d sum VE / d s2]; dgmu = ((Y - f) W) / s2; dW = ((Y - f)^T gmean - W .* colsum(gvar)) / s2;
  * rows = 0 gives out = [0, 0] and dW = 0;
  * what the device refuses (GPK_E_ARG) is an AssertionError here.
The fused shard is fake_ops' per-latent chain ending in the mixing stage: the stage is an argument of `fake_ops._shard_sep`.  The
names are NOT added to fake_ops.  The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
LOG2PI = float(np.log(2.0 * np.pi))


def _weights(W, L):
    W = np.ascontiguousarray(_np(W) if isinstance(W, torch.Tensor) else np.asarray(W, dtype=np.float64), dtype=np.float64)
    assert W.ndim == 2 and W.shape[1] == L, (W.shape, L)
    assert 1 <= L <= 16 and 1 <= W.shape[0] <= 16, W.shape     # GPK_E_ARG
    return W


def mixed_gaussian_varexp_sum(Y, gmean, W, *, s0, ssq, knn, noise_variance, mean_const=0.0, s0_per_latent=False,
                              want_moments=False, want_grads=False):
    rows, L = gmean.shape
    W = _weights(W, L)
    P = W.shape[0]
    s2 = float(noise_variance)
    assert s2 > 0.0, s2                                          # GPK_E_ARG
    knn = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=np.float64)), (L,))
    gv = np.tile(knn[None, :], (rows, 1)).astype(np.float64)
    if s0 is not None:
        gv = gv - (_np(s0).T if s0_per_latent else _np(s0)[:, None])
    if ssq is not None:
        gv = gv + _np(ssq).T
    gm = _np(gmean)
    with np.errstate(all="ignore"):
        # (explicit loops over l and p: NumPy's matmul would skip nothing, but 0 * NaN must stay NaN term by term as on the device)
        f = np.zeros((rows, P))
        fv = np.zeros((rows, P))
        for l in range(L):
            f = f + W[None, :, l] * gm[:, l:l + 1]
            fv = fv + (W[None, :, l] ** 2) * gv[:, l:l + 1]
        f = f + mean_const
        dy = _np(Y)[:, :P] - f
        q = dy * dy + fv
        ve = -0.5 * LOG2PI - 0.5 * np.log(s2) - 0.5 * q / s2
        d2 = -0.5 / s2 + 0.5 * q / (s2 * s2)
        dg = np.zeros((rows, L))
        for p in range(P):
            dg = dg + W[None, p, :] * dy[:, p:p + 1]
        dg = dg / s2
        dW = np.zeros((P, L))
        for b in range(rows):
            dW = dW + (dy[b][:, None] * gm[b][None, :] - W * gv[b][None, :])
        dW = dW / s2
        out = torch.tensor([ve.sum() if rows else 0.0, d2.sum() if rows else 0.0], dtype=torch.float64)
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    return (out, t_(f) if want_moments else None, t_(fv) if want_moments else None, t_(dg) if want_grads else None,
            t_(dW) if want_grads else None)


def svgp_elbo_lcm_workspace(m, rows, d, L, P):
    return torch.empty(1, dtype=torch.float64)


def svgp_elbo_shard_lcm(Z, Xb, Yb, q_mu, q_sqrt, W, *, variances, lengthscales, families, noise_variance, jitter, mean_const=0.0,
                        ws=None, out=None, info=None):
    """fake_ops' per-latent chain over the L latents, ending in the mixing stage"""
    W = _weights(W, q_mu.shape[1])
    assert Yb.shape[1] == W.shape[0], (Yb.shape, W.shape)
    assert float(noise_variance) > 0.0

    def stage(Y, fmean, **kw):
        return mixed_gaussian_varexp_sum(Y, fmean, W, noise_variance=noise_variance, **kw)[0][0:1], None

    return fake_ops._shard_sep(Z, Xb, Yb, q_mu, q_sqrt, stage, variances=variances, lengthscales=lengthscales, families=families,
                               jitter=jitter, mean_const=mean_const, out=out)
