"""CPU emulation of the ArcCosine kernel's primitives -- TEST INFRASTRUCTURE ONLY: `arccos_kernel_matrix`, `arccos_kernel_matrix_combine`,
`arccos_kernel_diag`, `arccos_adjoint_stage`, `arccos_adjoint_tail` (and the scratch helper `arccos_adjoint_parts`) of gpflow_amd/ops.py
in NumPy fp64, written from the contract in include/gpk.h ("ArcCosine kernel"):

  * s = sum_j (x_j w_j) y_j + b: the product x w first (one rounding), the sum over j ascending from 0.0, b last; p = s(x, x) by the
    same chain, so p of a row is the same number as first and as second argument;
  * the acos argument eps + (1 - 2 eps) c, clamped by comparisons that a NaN fails; cos theta = the clamped argument,
    sin theta = sqrt((1 - cos)(1 + cos));
  * X2 None: the diagonal takes the argument 1.0 - 1e-15 BY INDEX; in the adjoint stage its angular derivative is zero;
  * the symmetric build takes the elements on or below the diagonal and mirrors them: exactly symmetric; `lower_only` leaves what is
    strictly above the diagonal unwritten (NaN here); the combine ops and the adjoint stage never mirror;
  * the row diagonal is the closed form variance jf p^order;
  * the stage's `parts` have the header's layout (per 64-wide tile column / tile row / tile), the tail sums them in slot order.
What the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED, or the ValueError ops raises before it) is an AssertionError here.  The product
never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
MAX_D, TILE = 64, 64
EPS = 1e-15
SCALE = 1.0 - 2.0 * EPS
CT_DIAG = 1.0 - EPS


def _leaf(order, variance, weight_variances, bias_variance, d):
    """(order, v, w [d], b)"""
    assert not isinstance(order, bool) and order in (0, 1, 2), order                       # GPK_E_UNSUPPORTED (ops: ValueError)
    assert 1 <= d <= MAX_D, d                                                              # GPK_E_ARG (ops: ValueError)
    w = np.asarray(weight_variances, dtype=np.float64)
    assert w.ndim == 0 or (w.ndim == 1 and w.size == d), (w.shape, d)                      # (ops: ValueError)
    assert np.all(np.isfinite(w)) and np.all(w >= 0), w                                    # GPK_E_ARG
    v, b = float(variance), float(bias_variance)
    assert np.isfinite(v) and np.isfinite(b) and b > 0, (v, b)                             # GPK_E_ARG
    return int(order), v, np.broadcast_to(w, (d,)), b


def _dot(X1, X2, w):
    with np.errstate(all="ignore"):
        a, b = _np(X1) * w, _np(X2)
        s = np.zeros((a.shape[0], b.shape[0]))
        for j in range(a.shape[1]):
            s = a[:, j, None] * b[None, :, j] + s
    return s


def _norm(X, w, b):
    Xn = _np(X)
    with np.errstate(all="ignore"):
        p = np.zeros(Xn.shape[0])
        for j in range(Xn.shape[1]):
            p = (Xn[:, j] * w[j]) * Xn[:, j] + p
        return p + b


def _pieces(order, X1, X2, w, b, same, want_d=False):
    """(J m, and with want_d: dk/ds, dk/dp, dk/dq, all over variance / pi) element by element"""
    with np.errstate(all="ignore"):
        p, q = _norm(X1, w, b), _norm(X2, w, b)
        rp, rq = np.sqrt(p), np.sqrt(q)
        rr = rp[:, None] * rq[None, :]
        c = (_dot(X1, X2, w) + b) / rr
        arg = SCALE * c + EPS
        ct = np.where(arg > 1.0, 1.0, np.where(arg < -1.0, -1.0, arg))
        diag = np.eye(*ct.shape, dtype=bool) if same else np.zeros(ct.shape, dtype=bool)
        ct = np.where(diag, rr * 0.0 + CT_DIAG, ct)                  # (a NaN or Inf in the row reaches its diagonal element)
        pt = np.pi - np.arccos(ct)
        sn = np.sqrt((1.0 - ct) * (1.0 + ct))
        J1 = sn + pt * ct
        J = pt if order == 0 else J1 if order == 1 else 3.0 * sn * ct + pt * (1.0 + 2.0 * ct * ct)
        m = np.ones_like(rr) if order == 0 else rr if order == 1 else p[:, None] * q[None, :]
        jm = J * m
        if not want_d:
            return jm
        D = 1.0 / sn if order == 0 else pt if order == 1 else 4.0 * J1
        D = np.where(diag, 0.0, D)
        sd = SCALE * D
        h = 0.5 * (order * J - sd * np.where(diag, 1.0, c))
        P, Q, RP, RQ = p[:, None], q[None, :], rp[:, None], rq[None, :]
        dks = sd / rr if order == 0 else sd if order == 1 else sd * rr
        dkp = h / P if order == 0 else h * RQ / RP if order == 1 else h * Q
        dkq = h / Q if order == 0 else h * RP / RQ if order == 1 else h * P
        return jm, dks, dkp, dkq


def _ret(R, out):
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64))
    if out is None:
        return Rt
    assert tuple(out.shape) == tuple(Rt.shape)
    out.copy_(Rt)
    return out


def arccos_kernel_matrix(X1, X2, *, order=0, variance=1.0, weight_variances=1.0, bias_variance=1.0, diag_add=0.0, lower_only=False, out=None):
    n1, d = X1.shape
    assert X2 is None or X2.shape[1] == d
    if n1 == 0 or (X2 is not None and X2.shape[0] == 0):
        return _ret(np.zeros((n1, n1 if X2 is None else X2.shape[0])), out)
    order, v, w, b = _leaf(order, variance, weight_variances, bias_variance, d)
    with np.errstate(all="ignore"):
        K = (v * (1.0 / np.pi)) * _pieces(order, X1, X1 if X2 is None else X2, w, b, X2 is None)
        if X2 is None:
            K = np.tril(K) + np.tril(K, -1).T + diag_add * np.eye(n1)
            if lower_only:
                K = np.where(np.triu(np.ones_like(K), 1) > 0, np.nan, K)
    return _ret(K, out)


def arccos_kernel_matrix_combine(X1, X2, G, *, op, order=0, variance=1.0, weight_variances=1.0, bias_variance=1.0, diag_add=0.0, out=None):
    assert op in ("mul", "add"), op                                                        # GPK_E_ARG (ops: ValueError)
    n1, d = X1.shape
    n2 = n1 if X2 is None else X2.shape[0]
    assert tuple(G.shape) == (n1, n2)
    if n1 == 0 or n2 == 0:
        return _ret(np.zeros((n1, n2)), out)
    order, v, w, b = _leaf(order, variance, weight_variances, bias_variance, d)
    with np.errstate(all="ignore"):
        K = (v * (1.0 / np.pi)) * _pieces(order, X1, X1 if X2 is None else X2, w, b, X2 is None)
        R = K * _np(G) if op == "mul" else K + _np(G)
        if X2 is None:
            R = R + diag_add * np.eye(n1)
    return _ret(R, out)


def arccos_kernel_diag(X, g=None, *, op="k", order=0, variance=1.0, weight_variances=1.0, bias_variance=1.0, out=None):
    assert op in ("k", "mul", "add", "dp") and (op == "k") == (g is None), op             # GPK_E_ARG (ops: ValueError)
    n, d = X.shape
    order, v, w, b = _leaf(order, variance, weight_variances, bias_variance, d)
    with np.errstate(all="ignore"):
        p = _norm(X, w, b)
        if op == "dp":
            k = 0.0 * p if order == 0 else p * 0.0 + v if order == 1 else 6.0 * v * p
        else:
            k = v * (p * 0.0 + 1.0) if order == 0 else v * p if order == 1 else 3.0 * v * p * p
        R = k if op == "k" else _np(g) + k if op == "add" else _np(g) * k
    return _ret(R, out)


def arccos_adjoint_parts(n1, n2, device_=None):
    tr, tc = -(-int(n1) // TILE), -(-int(n2) // TILE)
    return torch.full((tc * int(n1) + tr * int(n2) + tr * tc,), float("nan"), dtype=torch.float64)


def arccos_adjoint_stage(X1, X2, Kbar, parts, *, order=0, variance=1.0, weight_variances=1.0, bias_variance=1.0, out=None):
    n1, d = X1.shape
    n2 = n1 if X2 is None else X2.shape[0]
    assert tuple(Kbar.shape) == (n1, n2)
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    assert parts.dim() == 1 and parts.numel() >= tc * n1 + tr * n2 + tr * tc
    if n1 == 0 or n2 == 0:
        return _ret(np.zeros((n1, n2)), out)
    order, v, w, b = _leaf(order, variance, weight_variances, bias_variance, d)
    vpi = v * (1.0 / np.pi)
    Kb = _np(Kbar)
    with np.errstate(all="ignore"):
        jm, dks, dkp, dkq = _pieces(order, X1, X1 if X2 is None else X2, w, b, X2 is None, want_d=True)
        G = Kb * (vpi * dks)
        tp, tq, tk = Kb * (vpi * dkp), Kb * (vpi * dkq), Kb * jm
        pn = np.empty(tc * n1 + tr * n2 + tr * tc)
        for t in range(tc):
            pn[t * n1:(t + 1) * n1] = tp[:, t * TILE:(t + 1) * TILE].sum(1)
        for t in range(tr):
            pn[tc * n1 + t * n2:tc * n1 + (t + 1) * n2] = tq[t * TILE:(t + 1) * TILE].sum(0)
        for ty in range(tr):
            for tx in range(tc):
                pn[tc * n1 + tr * n2 + ty * tc + tx] = tk[ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE].sum()
    parts[:pn.size].copy_(torch.from_numpy(pn))
    return _ret(G, out)


def arccos_adjoint_tail(R, A, Bm, parts, *, weight_variances):
    Rn, An, pn = _np(R), _np(A), _np(parts)
    n1, d = An.shape
    symmetric = Bm is None
    Bn = An if symmetric else _np(Bm)
    n2 = Bn.shape[0]
    w = np.asarray(weight_variances, dtype=np.float64)
    assert Rn.shape[0] == n1 and Rn.shape[1] >= 1 + d and 1 <= d <= MAX_D and (w.ndim == 0 or (w.ndim == 1 and w.size == d))
    assert np.all(np.isfinite(w)) and np.all(w >= 0)                                       # GPK_E_ARG
    ard = w.ndim == 1
    wn = np.broadcast_to(w, (d,))
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))  # noqa: E731
    if n1 == 0 or n2 == 0:
        return tt(np.zeros(1)), tt(np.zeros(d if ard else 1)), tt(np.zeros(1)), tt(np.zeros((n1, d)))
    with np.errstate(all="ignore"):
        rho = np.zeros(n1)
        for t in range(tc):
            rho = rho + pn[t * n1:(t + 1) * n1]
        gam = np.zeros(n2)
        for t in range(tr):
            gam = gam + pn[tc * n1 + t * n2:tc * n1 + (t + 1) * n2]
        dv = pn[tc * n1 + tr * n2:tc * n1 + tr * n2 + tr * tc].sum() * (1.0 / np.pi)
        GB = Rn[:, 1:1 + d]
        if symmetric:
            rho = rho + gam
            dw = (An * (GB + rho[:, None] * An)).sum(0)
            db = (Rn[:, 0] + rho).sum()
            Abar = 2.0 * wn * GB + 2.0 * wn * An * rho[:, None]
        else:
            dw = (An * (GB + rho[:, None] * An)).sum(0) + (gam[:, None] * Bn * Bn).sum(0)
            db = (Rn[:, 0] + rho).sum() + gam.sum()
            Abar = wn * GB + 2.0 * wn * An * rho[:, None]
        if not ard:
            dw = dw.sum().reshape(1)
    return tt(np.reshape(dv, 1)), tt(dw), tt(np.reshape(db, 1)), tt(Abar)
