"""CPU emulation of `ops.switched_varexp_sum` (include/gpk.h: gpk_switched_varexp_sum) -- TEST INFRASTRUCTURE ONLY, the companion of
tests/fake_likelihood_ops.py for a switched likelihood.  NumPy fp64, written from the stated contract:

  * row b's task is its label in column `ylab` of Y (default: the last), read by the Coregion rule: valid when the DOUBLE lies inside
    (-1, T), then truncated toward zero; anything else (NaN, +-Inf, <= -1, >= T) is invalid;
  * a row is evaluated by its own member: the member's row of `fake_likelihood_ops.LIKELIHOODS`, or for "gaussian" (params =
    (variance,)) the closed form VE = -log(2 pi) / 2 - log(s2) / 2 - ((y - mu)^2 + v) / (2 s2) with dmu = (y - mu) / s2,
    dvar = -1 / (2 s2), dVE/ds2 = -1 / (2 s2) + ((y - mu)^2 + v) / (2 s2^2), and y - y added to VE, dmu, dvar;
  * out[0] = the sum of VE, out[1 + t] = the sum of dVE/dtheta_t over task t's rows (0.0 for a member without a trainable parameter
    and for a task without rows); a row with an invalid label is NaN in rows, dmu, dvar and out[0], and in no out[1 + t];
  * fvar = knn - s0 + ssq, unclamped, for every row;
  * what the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED) is an AssertionError here.
The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_likelihood_ops
import fake_ops

_np = fake_ops._np
_MEMBERS = ("gaussian", "bernoulli_probit", "poisson_exp", "student_t", "exponential_exp", "gamma_exp", "beta_probit")


def _gaussian(par, y, mu, fv):
    s2 = par[0]
    ynan = y - y
    q = (y - mu) ** 2 + fv
    ve = -0.5 * np.log(2.0 * np.pi) - 0.5 * np.log(s2) - 0.5 * q / s2
    return ve + ynan, (y - mu) / s2 + ynan, -0.5 / s2 + ynan + np.zeros_like(mu), -0.5 / s2 + 0.5 * q / (s2 * s2)


def _member(name, params, P):
    """(checked params, evaluation) of one member"""
    assert name in _MEMBERS, name                     # GPK_E_UNSUPPORTED (codes 4, 5 - 7, 11) / no such name
    params = [float(v) for v in params]
    if name == "gaussian":
        assert len(params) == 1 and params[0] > 0.0, params   # GPK_E_ARG
        return params, _gaussian
    check, evaluate = fake_likelihood_ops.LIKELIHOODS[name]
    return check(params, P), evaluate


def _tasks(labels, T):
    """the task of every label, -1 for an invalid one (csrc/label.h)"""
    with np.errstate(invalid="ignore"):
        ok = (labels > -1.0) & (labels < float(T))
    return np.where(ok, np.trunc(np.where(ok, labels, 0.0)), -1).astype(np.int64)


def switched_varexp_sum(Y, fmean, *, s0, ssq, knn, members, ylab=None, mean_const=0.0, s0_per_latent=False, want_fvar=False,
                        want_rows=False, want_grads=False):
    rows, P = fmean.shape
    members = list(members)
    T = len(members)
    assert 1 <= T <= 16 and 1 <= P <= 16, (T, P)     # GPK_E_ARG
    Yn = _np(Y)
    ylab = Yn.shape[1] - 1 if ylab is None else int(ylab)
    assert P <= ylab < Yn.shape[1], (P, ylab)         # GPK_E_ARG
    table = [_member(name, params, P) for name, params in members]
    knn = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=np.float64)), (P,))
    fv = np.tile(knn[None, :], (rows, 1)).astype(np.float64)
    if s0 is not None:
        fv = fv - (_np(s0).T if s0_per_latent else _np(s0)[:, None])
    if ssq is not None:
        fv = fv + _np(ssq).T
    mu = _np(fmean) + mean_const
    y = Yn[:, :P]
    task = _tasks(Yn[:, ylab], T)
    ve, dmu, dvar = (np.full((rows, P), np.nan) for _ in range(3))
    out = np.zeros(1 + T)
    with np.errstate(all="ignore"):
        for t, (par, evaluate) in enumerate(table):
            sel = task == t
            if not sel.any():
                continue
            v, dm, dv, dth = evaluate(par, y[sel], mu[sel], fv[sel])
            ve[sel], dmu[sel], dvar[sel] = v, dm, dv
            out[1 + t] = np.sum(dth)
        out[0] = ve.sum()
    t_ = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))   # noqa: E731
    return (t_(out), t_(ve.sum(1)) if want_rows else None, t_(dmu) if want_grads else None, t_(dvar) if want_grads else None,
            t_(fv) if want_fvar else None)
