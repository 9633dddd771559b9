"""CPU emulation of `gpflow_amd.ops.tril_product` (include/gpk.h: gpk_tril_product) -- TEST INFRASTRUCTURE ONLY.

The contract it reproduces, including what the HIP kernel does NOT compute:
  * nothing above the diagonal of L or of any S_r is read (both are masked before anything else looks at them);
  * a term L[i, k] S_r[k, j] exists exactly for j <= k <= i.  NumPy's matrix product over zero-filled triangles would form
    0 x NaN for the masked partners of a NaN inside a triangle; here the non-finite entries inside the triangles are taken out of
    the product and the entries they REACH (P_r[i0, j <= k0] for L[i0, k0]; P_r[i >= k0, j0] for S_r[k0, j0]) are set to NaN
    afterwards -- the device gives NaN there for a NaN and may give an infinity for an infinity, which this emulation does not tell apart;
  * T is written on and below the diagonal only; `product_out` keeps everything else, a fresh T is zero there;
  * `parts`, when given, must have the documented extent [R, ceil(n / 128), n]; it is filled like the device fills it (entry
    [r, t, i] for t <= i // 128 is the sum over tile column t, everything else is left alone) and ssq is the sum over t in order.
The product never imports this file.
"""
import numpy as np
import torch

from fake_ops import _np

TRIL_TILE = 128


def tril_product_parts(n, R, device_=None):
    return torch.empty((R, -(-n // TRIL_TILE) if n > 0 else 0, n), dtype=torch.float64)


def tril_product(L, S, *, rowscale=None, want_ssq=True, want_product=False, parts=None, product_out=None):
    n, R = L.shape[0], S.shape[0]
    assert L.shape[1] >= n and tuple(S.shape[1:2]) == (n,) and S.shape[2] >= n, (L.shape, S.shape)
    want_product = want_product or product_out is not None
    assert want_ssq or want_product, "neither output"                                    # GPK_E_ARG
    assert rowscale is None or (want_product and tuple(rowscale.shape) == (R, n))        # GPK_E_ARG: rowscale goes with T
    low = np.tril(np.ones((n, n), dtype=bool))
    Ln = np.where(low, _np(L)[:, :n], 0.0)
    Sn = np.where(low[None], _np(S)[:, :, :n], 0.0)
    badL, badS = ~np.isfinite(Ln), ~np.isfinite(Sn)
    P = np.where(badL, 0.0, Ln)[None] @ np.where(badS, 0.0, Sn)
    reach = (badL.astype(np.float64)[None] @ np.broadcast_to(low.astype(np.float64), (R, n, n))) \
        + (low.astype(np.float64)[None] @ badS.astype(np.float64))
    P = np.where(low[None], np.where(reach > 0, np.nan, P), 0.0)
    ssq = T = None
    if want_ssq:
        nt = -(-n // TRIL_TILE) if n > 0 else 0
        if parts is not None:
            assert tuple(parts.shape) == (R, nt, n) and parts.is_contiguous(), parts.shape
        acc = np.zeros((R, n))
        for t in range(nt):
            rows = slice(t * TRIL_TILE, n)
            col = (P[:, rows, t * TRIL_TILE:(t + 1) * TRIL_TILE] ** 2).sum(-1)
            acc[:, rows] += col
            if parts is not None:
                parts[:, t, rows] = torch.from_numpy(col)
        ssq = torch.from_numpy(acc)
    if want_product:
        T = product_out if product_out is not None else torch.zeros((R, n, n), dtype=torch.float64)
        assert T.shape[0] == R and T.shape[1] == n and T.shape[2] >= n, T.shape
        scaled = P if rowscale is None else _np(rowscale)[:, :, None] * P
        Tn = T.numpy()   # (a view: the writes below land in T, padded or not)
        Tn[:, :, :n][np.broadcast_to(low, (R, n, n))] = scaled[np.broadcast_to(low, (R, n, n))]
    return ssq, T
