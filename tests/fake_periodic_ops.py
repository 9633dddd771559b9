"""CPU emulation of the Periodic kernel's three primitives -- TEST INFRASTRUCTURE ONLY: `periodic_warp`, `periodic_moment_rows` and
`periodic_adjoint_tail` of gpflow_amd/ops.py in NumPy fp64, written from the contract in include/gpk.h ("the Periodic kernel's input
warp"):

  * the warp is (cos, sin)(pi q) of the ONE rounded quotient q = 2 x / p, reduced exactly (np.fmod is exact) before pi enters, so that
    x = k p gives exactly (1, 0) and a large |x| / p loses nothing beyond that quotient's rounding; NaN / Inf give NaN;
  * the moment rows are [1 ; Phi^T ; (Phi^2)^T ; (b cos)^T, (b sin)^T interleaved], their first 1 + 4 D rows those of
    fake_ops.moment_rows at the warped inputs;
  * the tail is the two formulas of the header, `into` = accumulate.
What the device refuses (GPK_E_ARG, or the ValueError ops raises before it) is an AssertionError here: D outside [1, 32], a period
of the wrong length or one that is not positive and finite.  The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
MAX_D = 32


def _periods(period, d):
    assert 1 <= d <= MAX_D, d                                                             # GPK_E_ARG (ops: ValueError)
    p = np.atleast_1d(np.asarray(period, dtype=np.float64))
    assert p.ndim == 1 and p.size in (1, d), (p.shape, d)                                 # (ops: ValueError)
    assert np.all(np.isfinite(p)) and np.all(p > 0.0), p                                  # GPK_E_ARG
    return np.broadcast_to(p, (d,)), p.size > 1


def _sincospi(q):
    """(sin, cos)(pi q), exact at the multiples of 1/2"""
    with np.errstate(all="ignore"):
        r = np.fmod(q, 2.0)                                                               # exact; (-2, 2)
        r = np.where(r > 1.0, r - 2.0, np.where(r < -1.0, r + 2.0, r))                    # [-1, 1], exact
        s, c = np.sin(np.pi * r), np.cos(np.pi * r)
        s = np.where((r == 0.0) | (np.abs(r) == 1.0), 0.0, np.where(np.abs(r) == 0.5, np.sign(r), s))
        c = np.where(np.abs(r) == 0.5, 0.0, np.where(r == 0.0, 1.0, np.where(np.abs(r) == 1.0, -1.0, c)))
        bad = ~np.isfinite(q)
        return np.where(bad, np.nan, s), np.where(bad, np.nan, c)


def _warp(X, period):
    X = _np(X)
    n, d = X.shape
    p, _ = _periods(period, d)
    with np.errstate(all="ignore"):
        s, c = _sincospi(2.0 * X / p)
    Phi = np.empty((n, 2 * d))
    Phi[:, 0::2], Phi[:, 1::2] = c, s
    return Phi


def periodic_warp(X, period, out=None):
    Phi = torch.from_numpy(_warp(X, period))
    if out is None:
        return Phi
    assert tuple(out.shape) == tuple(Phi.shape)
    out.copy_(Phi)
    return out


def periodic_moment_rows(B, period):
    Bn = _np(B)
    n2, d = Bn.shape
    Phi = _warp(Bn, period)
    Vt = np.empty((1 + 6 * d, n2))
    Vt[0] = 1.0
    Vt[1:1 + 2 * d] = Phi.T
    Vt[1 + 2 * d:1 + 4 * d] = (Phi * Phi).T
    with np.errstate(all="ignore"):
        Vt[1 + 4 * d:] = (np.repeat(Bn, 2, axis=1) * Phi).T
    return torch.from_numpy(Vt)


def periodic_adjoint_tail(X, Phi, Phibar, R, ls, period, *, into=None):
    Xn, Pn, Pb, Rn, l = _np(X), _np(Phi), _np(Phibar), _np(R), _np(ls).reshape(-1)
    n1, d = Xn.shape
    p, ard = _periods(period, d)
    assert Pn.shape == (n1, 2 * d) and Pb.shape == (n1, 2 * d) and Rn.shape == (n1, 1 + 6 * d) and l.shape == (d,)
    c, s = Pn[:, 0::2], Pn[:, 1::2]
    gc, gs = Rn[:, 1:1 + 2 * d:2], Rn[:, 2:2 + 2 * d:2]
    gbc, gbs = Rn[:, 1 + 4 * d::2], Rn[:, 2 + 4 * d::2]
    Xbar = (2.0 * np.pi / p) * (c * Pb[:, 1::2] - s * Pb[:, 0::2])
    dper = (np.pi / (2.0 * p * p * l * l)) * (Xn * (s * gc - c * gs) + (c * gbs - s * gbc)).sum(0)
    if not ard:
        dper = dper.sum().reshape(1)
    dper, Xbar = torch.from_numpy(np.ascontiguousarray(dper)), torch.from_numpy(np.ascontiguousarray(Xbar))
    if into is None:
        return dper, Xbar
    into[0].add_(dper)
    into[1].add_(Xbar)
    return into
