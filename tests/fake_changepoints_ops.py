"""CPU emulation of the ChangePoints kernel's primitives -- TEST INFRASTRUCTURE ONLY: `changepoint_weights`, `changepoint_fold`,
`changepoint_adjoint_stage`, `changepoint_adjoint_tail` (and the scratch helper `changepoint_adjoint_parts`) of gpflow_amd/ops.py in
NumPy fp64, written from the contract in include/gpk.h ("ChangePoints kernel"):

  * sig_j = 1 / (1 + exp(-z)), 1 - sig_j = 1 / (1 + exp(+z)) with z = s_j (x - l_j) + (x - x): no subtraction from 1, saturation is
    exactly 0 or 1, a NaN or an Inf in x makes every weight of the row NaN;
  * the tile passes form w = a_r b_c first, then w * Ki;
  * the stage's `parts` have the header's layout (per 64-wide tile column / tile row), the tail sums them in slot order.
What the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED, or the error ops raises before it) is an AssertionError here, except the two
refusals the kernel class relies on (ValueError for mismatched lengths, NotImplementedError for more than 16 members).  The product
never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
TILE, MAX_MEMBERS = 64, 16


def _points(locations, steepness):
    loc = np.asarray(locations, dtype=np.float64).reshape(-1)
    st = np.asarray(steepness, dtype=np.float64).reshape(-1)
    if st.size != loc.size:
        raise ValueError(f"changepoints: {loc.size} locations and {st.size} steepness entries")
    if loc.size + 1 > MAX_MEMBERS:
        raise NotImplementedError(f"changepoints: more than {MAX_MEMBERS} member kernels")
    assert np.all(np.isfinite(loc)) and np.all(np.isfinite(st)) and np.all(st > 0) and np.all(np.diff(loc) >= 0), (loc, st)   # GPK_E_ARG
    return loc, st


def _column(x):
    xn = _np(x)
    if xn.ndim == 2 and xn.shape[1] == 1:
        xn = xn[:, 0]
    assert xn.ndim == 1
    return xn


def _sigmoids(xn, loc, st):
    """(sig [C, n], 1 - sig [C, n])"""
    with np.errstate(all="ignore"):
        z = st[:, None] * (xn[None, :] - loc[:, None]) + (xn - xn)[None, :]
        return 1.0 / (1.0 + np.exp(-z)), 1.0 / (1.0 + np.exp(z))


def _weights(xn, loc, st):
    sig, comp = _sigmoids(xn, loc, st)
    with np.errstate(all="ignore"):
        one = (1.0 + (xn - xn))[None, :]
        return np.concatenate([one, sig]) * np.concatenate([comp, np.ones((1, xn.size))])


def _ret(R, out):
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64))
    if out is None:
        return Rt
    assert tuple(out.shape) == tuple(Rt.shape)
    out.copy_(Rt)
    return out


def changepoint_weights(x, *, locations, steepness, out=None):
    loc, st = _points(locations, steepness)
    return _ret(_weights(_column(x), loc, st), out)


def changepoint_fold(a, b, Ki, acc=None, *, diag_add=0.0, out=None):
    an, Kn = _np(a), _np(Ki)
    n1, n2 = Kn.shape
    assert an.shape == (n1,) and (b is not None or n1 == n2) and (b is None or _np(b).shape == (n2,))
    assert acc is None or tuple(acc.shape) == (n1, n2)
    with np.errstate(all="ignore"):
        R = (an[:, None] * (an if b is None else _np(b))[None, :]) * Kn
        if acc is not None:
            R = _np(acc) + R
        if b is None:
            R = R + diag_add * np.eye(n1)
    return _ret(R, out)


def changepoint_adjoint_parts(T, n1, n2, device_=None):
    tr, tc = -(-int(n1) // TILE), -(-int(n2) // TILE)
    return torch.full((int(T), tc * int(n1) + tr * int(n2)), float("nan"), dtype=torch.float64)


def changepoint_adjoint_stage(a, b, Kbar, Ki, parts, *, out=None):
    an, Kb, Kn = _np(a), _np(Kbar).copy(), _np(Ki).copy()
    n1, n2 = Kb.shape
    bn = an if b is None else _np(b)
    assert Kn.shape == (n1, n2) and an.shape == (n1,) and bn.shape == (n2,)
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    assert parts.dim() == 1 and parts.numel() >= tc * n1 + tr * n2
    with np.errstate(all="ignore"):
        G = Kb * (an[:, None] * bn[None, :])
        e = Kb * Kn
        tp, tq = e * bn[None, :], e * an[:, None]
        pn = np.empty(tc * n1 + tr * n2)
        for t in range(tc):
            pn[t * n1:(t + 1) * n1] = tp[:, t * TILE:(t + 1) * TILE].sum(1)
        for t in range(tr):
            pn[tc * n1 + t * n2:tc * n1 + (t + 1) * n2] = tq[t * TILE:(t + 1) * TILE].sum(0)
    parts[:pn.size].copy_(torch.from_numpy(pn))
    return _ret(G, out)


def changepoint_adjoint_tail(x, *, locations, steepness, parts=None, n_other=0, columns=False, init=None):
    loc, st = _points(locations, steepness)
    xn = _column(x)
    n, C = xn.size, loc.size
    tt = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64))  # noqa: E731
    if n == 0 or C == 0:
        return tt(np.zeros(C)), tt(np.zeros(C)), tt(np.zeros(n))
    with np.errstate(all="ignore"):
        abar = np.zeros((C + 1, n)) if init is None else _np(init).copy()
        assert abar.shape == (C + 1, n)
        if parts is not None:
            pn = _np(parts)
            n1, n2 = (int(n_other), n) if columns else (n, int(n_other))
            tr, tc = -(-n1 // TILE), -(-n2 // TILE)
            assert pn.shape[0] == C + 1 and pn.shape[1] >= tc * n1 + tr * n2
            off, nt = (tc * n1, tr) if columns else (0, tc)
            for t in range(nt):
                abar = abar + pn[:, off + t * n:off + (t + 1) * n]
        sig, comp = _sigmoids(xn, loc, st)
        A = _weights(xn, loc, st)
        tbar = abar[1:] * A[1:] * comp - abar[:-1] * A[:-1] * sig
        dl = -st * tbar.sum(1)
        ds = (tbar * (xn[None, :] - loc[:, None])).sum(1)
        xbar = (st[:, None] * tbar).sum(0)
    return tt(dl), tt(ds), tt(xbar)
