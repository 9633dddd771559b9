"""CPU emulation of the dot-product kernels' four primitives -- TEST INFRASTRUCTURE ONLY: `dot_kernel_matrix`,
`dot_kernel_matrix_combine`, `dot_kernel_diag` and `dot_adjoint_tail` of gpflow_amd/ops.py in NumPy fp64, written from the contract in
include/gpk.h ("dot-product kernels"):

  * s = sum_j (x_j w_j) y_j: the product x w first (one rounding), the sum over j ascending, one column at a time (the device's chain is
    an fma, here a product and a sum: both within d u sum_j |w_j x_j y_j| of the exact sum of the rounded x w terms);
  * Polynomial: base = s + offset, the power base * base * ... left to right; dk/ds = degree * base^(degree - 1), exactly 1 at degree 1;
  * the symmetric build (X2 None) takes the elements on or below the diagonal and mirrors them: exactly symmetric; `lower_only`
    leaves what is strictly above the diagonal unwritten (NaN here); the combine ops never mirror and "ds" does not zero the diagonal;
  * the row diagonal sums the same chain: bit for bit the diagonal of the symmetric build;
  * the tail is the three formulas of the header.
What the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED, or the ValueError / NotImplementedError ops raises before it) is an
AssertionError here.  The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
MAX_D, MAX_DEGREE = 64, 16
FAMILIES = ("Linear", "Polynomial")


def _leaf(family, variance, offset, degree, d):
    """(w [d], offset, degree)"""
    assert family in FAMILIES, family                                                      # GPK_E_UNSUPPORTED
    assert 1 <= d <= MAX_D, d                                                              # GPK_E_ARG (ops: ValueError)
    w = np.asarray(variance, dtype=np.float64)
    assert w.ndim == 0 or (w.ndim == 1 and w.size == d), (w.shape, d)                      # (ops: ValueError)
    assert np.all(np.isfinite(w)), w                                                       # GPK_E_ARG
    if family == "Linear":
        assert offset is None and degree is None, "offset / degree given to Linear"       # (ops: ValueError)
        return np.broadcast_to(w, (d,)), 0.0, 1
    assert offset is not None and degree is not None, "Polynomial needs offset and degree"
    assert np.isfinite(float(offset)), offset                                              # GPK_E_ARG
    assert float(degree) == int(degree) and 1 <= int(degree) <= MAX_DEGREE, degree         # (ops: NotImplementedError) / GPK_E_ARG
    return np.broadcast_to(w, (d,)), float(offset), int(degree)


def _s(X1, X2, w):
    with np.errstate(all="ignore"):
        a, b = _np(X1) * w, _np(X2)
        s = np.zeros((a.shape[0], b.shape[0]))
        for j in range(a.shape[1]):
            s = a[:, j, None] * b[None, :, j] + s
    return s


def _power(base, degree):
    p = base
    with np.errstate(all="ignore"):
        for _ in range(1, degree):
            p = p * base
    return p


def _profile(family, s, offset, degree, what="k"):
    with np.errstate(all="ignore"):
        if what == "k":
            return s if family == "Linear" else _power(s + offset, degree)
        if family == "Linear" or degree == 1:
            return np.ones_like(s)
        return float(degree) * _power(s + offset, degree - 1)


def _ret(R, out):
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64))
    if out is None:
        return Rt
    assert tuple(out.shape) == tuple(Rt.shape)
    out.copy_(Rt)
    return out


def dot_kernel_matrix(X1, X2, *, family="Linear", variance, offset=None, degree=None, diag_add=0.0, lower_only=False, out=None):
    n1, d = X1.shape
    assert X2 is None or X2.shape[1] == d
    if n1 == 0 or (X2 is not None and X2.shape[0] == 0):
        return _ret(np.zeros((n1, n1 if X2 is None else X2.shape[0])), out)
    w, off, deg = _leaf(family, variance, offset, degree, d)
    K = _profile(family, _s(X1, X1 if X2 is None else X2, w), off, deg)
    if X2 is None:
        K = np.tril(K) + np.tril(K, -1).T + diag_add * np.eye(n1)
        if lower_only:
            K = np.where(np.triu(np.ones_like(K), 1) > 0, np.nan, K)
    return _ret(K, out)


def dot_kernel_matrix_combine(X1, X2, G, *, op, family="Linear", variance, offset=None, degree=None, diag_add=0.0, out=None):
    assert op in ("mul", "add", "ds"), op                                                  # GPK_E_ARG
    n1, d = X1.shape
    n2 = n1 if X2 is None else X2.shape[0]
    assert tuple(G.shape) == (n1, n2)
    if n1 == 0 or n2 == 0:
        return _ret(np.zeros((n1, n2)), out)
    w, off, deg = _leaf(family, variance, offset, degree, d)
    s = _s(X1, X1 if X2 is None else X2, w)
    with np.errstate(all="ignore"):
        if op == "ds":
            R = _profile(family, s, off, deg, "ds") * _np(G)
        else:
            K = _profile(family, s, off, deg)
            R = K * _np(G) if op == "mul" else K + _np(G)
            if X2 is None:
                R = R + diag_add * np.eye(n1)
    return _ret(R, out)


def dot_kernel_diag(X, g=None, *, op="k", family="Linear", variance, offset=None, degree=None, out=None):
    assert op in ("k", "mul", "add", "ds") and (op == "k") == (g is None), op             # GPK_E_ARG (ops: ValueError)
    n, d = X.shape
    w, off, deg = _leaf(family, variance, offset, degree, d)
    Xn = _np(X)
    with np.errstate(all="ignore"):
        s = np.zeros(n)
        for j in range(d):
            s = (Xn[:, j] * w[j]) * Xn[:, j] + s
        k = _profile(family, s, off, deg, "ds" if op == "ds" else "k")
        R = k if op == "k" else _np(g) + k if op == "add" else _np(g) * k
    return _ret(R, out)


def dot_adjoint_tail(R, A, w, *, symmetric):
    Rn, An, wn = _np(R), _np(A), _np(w).reshape(-1)
    n1, d = An.shape
    assert Rn.shape[0] == n1 and Rn.shape[1] >= 1 + d and wn.size in (1, d) and 1 <= d <= MAX_D
    ard = wn.size == d and d > 1
    GB = Rn[:, 1:1 + d]
    dw = (An * GB).sum(0)
    if not ard:
        dw = dw.sum().reshape(1)
    doff = Rn[:, 0].sum().reshape(1)
    Abar = (2.0 if symmetric else 1.0) * np.broadcast_to(wn, (d,)) * GB
    return (torch.from_numpy(np.ascontiguousarray(dw)), torch.from_numpy(doff), torch.from_numpy(np.ascontiguousarray(Abar)))
