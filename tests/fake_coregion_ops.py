"""CPU emulation of the Coregion kernel's primitives -- TEST INFRASTRUCTURE ONLY: `coregion_output_covariance`, `coregion_kernel_matrix`,
`coregion_kernel_matrix_combine`, `coregion_kernel_diag`, `coregion_onehot_rows`, `coregion_adjoint_tail` of gpflow_amd/ops.py in NumPy
fp64, written from the contract in include/gpk.h ("Coregion kernel"):

  * B = W W^T + diag(kappa): the sum over r ascending from 0.0, kappa added last on the diagonal; exactly symmetric;
  * the label of a row is its one column truncated toward zero, valid when the DOUBLE satisfies -1 < x < P; anything else (NaN, +-Inf,
    x <= -1, x >= P) makes its row / column of K, its entry of the row diagonal and its column of the one-hot rows NaN, nothing else;
  * an element of K has the bits of B[l, l']; `lower_only` leaves what is strictly above the diagonal unwritten;
  * the row diagonal is read from B;
  * the tail: dW = (Bbar + Bbar^T) W summed over b ascending, dkappa = diag(Bbar).
What the device refuses (GPK_E_ARG, or the ValueError ops raises before it) is an AssertionError here.  The product never imports
this file.
"""
from __future__ import annotations

import numpy as np
import torch

import fake_ops

_np = fake_ops._np
MAX_OUTPUTS, MAX_RANK = 64, 64


def _leaf(W, kappa):
    W, kappa = np.asarray(W, dtype=np.float64), np.asarray(kappa, dtype=np.float64)
    assert W.ndim == 2 and kappa.ndim == 1 and kappa.shape[0] == W.shape[0], (W.shape, kappa.shape)           # (ops: ValueError)
    assert 1 <= W.shape[0] <= MAX_OUTPUTS and 1 <= W.shape[1] <= MAX_RANK, W.shape                             # GPK_E_ARG (ops: ValueError)
    return W, kappa


def _B(W, kappa):
    W, kappa = _leaf(W, kappa)
    with np.errstate(all="ignore"):
        B = np.zeros((W.shape[0], W.shape[0]))
        for r in range(W.shape[1]):
            B = W[:, r, None] * W[None, :, r] + B
        B[np.diag_indices_from(B)] += kappa
    return B


def _labels(X, P):
    """(labels with 0 in the place of an invalid one, valid)"""
    assert X.dim() == 2 and X.shape[1] == 1, tuple(X.shape)                                                    # (ops: ValueError)
    x = _np(X)[:, 0]
    with np.errstate(all="ignore"):
        valid = (x > -1.0) & (x < float(P))
        return np.where(valid, np.trunc(np.where(valid, x, 0.0)), 0.0).astype(np.int64), valid


def _gather(X1, X2, B):
    P = B.shape[0]
    l1, v1 = _labels(X1, P)
    l2, v2 = (l1, v1) if X2 is None else _labels(X2, P)
    return np.where(v1[:, None] & v2[None, :], B[l1][:, l2], np.nan)


def _ret(R, out):
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64))
    if out is None:
        return Rt
    assert tuple(out.shape) == tuple(Rt.shape)
    out.copy_(Rt)
    return out


def coregion_output_covariance(W, kappa, *, device_=None, out=None):
    return _ret(_B(W, kappa), out)


def coregion_kernel_matrix(X1, X2, *, W, kappa, diag_add=0.0, lower_only=False, out=None):
    B = _B(W, kappa)
    n1 = X1.shape[0]
    assert X1.dim() == 2 and X1.shape[1] == 1 and (X2 is None or (X2.dim() == 2 and X2.shape[1] == 1))
    if n1 == 0 or (X2 is not None and X2.shape[0] == 0):
        return _ret(np.zeros((n1, n1 if X2 is None else X2.shape[0])), out)
    with np.errstate(all="ignore"):
        K = _gather(X1, X2, B)
        if X2 is None:
            K = K + diag_add * np.eye(n1)
            if lower_only:    # what is strictly above the diagonal is not written: it keeps what `out` held (NaN in a fresh one)
                K = np.where(np.triu(np.ones_like(K), 1) > 0, np.nan if out is None else _np(out), K)
    return _ret(K, out)


def coregion_kernel_matrix_combine(X1, X2, G, *, op, W, kappa, diag_add=0.0, out=None):
    assert op in ("mul", "add"), op                                                                            # GPK_E_ARG (ops: ValueError)
    B = _B(W, kappa)
    n1 = X1.shape[0]
    n2 = n1 if X2 is None else X2.shape[0]
    assert tuple(G.shape) == (n1, n2)
    if n1 == 0 or n2 == 0:
        return _ret(np.zeros((n1, n2)), out)
    with np.errstate(all="ignore"):
        K = _gather(X1, X2, B)
        R = _np(G) * K if op == "mul" else _np(G) + K
        if X2 is None:
            R = R + diag_add * np.eye(n1)
    return _ret(R, out)


def coregion_kernel_diag(X, g=None, *, op="k", W, kappa, out=None):
    assert op in ("k", "mul", "add") and (op == "k") == (g is None), op                                       # GPK_E_ARG (ops: ValueError)
    B = _B(W, kappa)
    l, v = _labels(X, B.shape[0])
    with np.errstate(all="ignore"):
        k = np.where(v, B[l, l], np.nan)
        R = k if op == "k" else _np(g) + k if op == "add" else _np(g) * k
    return _ret(R, out)


def coregion_onehot_rows(X, n_outputs):
    P = int(n_outputs)
    assert 1 <= P <= MAX_OUTPUTS                                                                               # GPK_E_ARG (ops: ValueError)
    l, v = _labels(X, P)
    E = (l[None, :] == np.arange(P)[:, None]).astype(np.float64)
    return _ret(np.where(v[None, :], E, np.nan), None)


def coregion_adjoint_tail(Bbar, *, W):
    Wn, Bb = np.asarray(W, dtype=np.float64), _np(Bbar)
    assert Wn.ndim == 2 and Bb.shape == (Wn.shape[0], Wn.shape[0]) and 1 <= Wn.shape[0] <= MAX_OUTPUTS and 1 <= Wn.shape[1] <= MAX_RANK
    with np.errstate(all="ignore"):
        S = Bb + Bb.T
        dW = np.zeros_like(Wn)
        for b in range(Wn.shape[0]):
            dW = S[:, b, None] * Wn[None, b, :] + dW
    return _ret(np.diag(Bb).copy(), None), _ret(dW, None)
