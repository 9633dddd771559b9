"""CPU emulation of the `gpflow_amd.ops` primitives -- TEST INFRASTRUCTURE ONLY.

`gpflow_amd/gradients.py` is a composition of device primitives.  There is no GPU in the build container, so the
composition itself (operand order, transposes, which triangle / K range each GEMM may assume) is validated here by
swapping `gradients.ops` for this module in a CPU test and comparing with the autograd oracle.  The emulation
reproduces the CONTRACT of each primitive, including what the HIP kernels do NOT compute:
  * gemm_nt(b_tri=1): for column tile n0 the K range starts at n0 & ~15 -- B[j, kk < n0] is never read;
    b_tri=2: the K range ends at n0 + 128 -- B[j, kk >= n0 + 128] is never read (poisoned with NaN here);
  * gemm_nt(c_lower): 128 x 128 tiles strictly above the diagonal are skipped (left at their initial value);
  * potrf_ reads only the lower triangle of the square block and leaves / zeroes the upper one;
  * transpose(mode=1) keeps only the lower triangle of its input.
The covariance builders (`kernel_matrix`, `kernel_matrix_hadamard`, `kernel_matrix_combine`) and the fused wrappers that take
`family` know the eight families of include/gpk.h (next to the family codes) and the keyword `alpha`:
  * the Materns: r = sqrt(max(r2, 1e-36)); -2 dk/dr2 is 0 where r2 <= 1e-36 (a NaN r2 is not clamped);
  * Exponential: variance exp(-r / 2), r = sqrt(max(r2, 1e-36)); -2 dk/dr2 = variance exp(-r / 2) / (2 r), 0 where r2 <= 1e-36;
  * RationalQuadratic: u = r2 / (2 alpha), k = variance exp(-alpha log1p(u)), -2 dk/dr2 = variance exp(-(alpha + 1) log1p(u)),
    dk/dalpha = k (u / (1 + u) - log1p(u)) (op "dalpha": exact zeros on the diagonal of the symmetric form, as "dr2");
  * White: variance on the diagonal when X2 is None, zeros for ANY X2 given (never by comparing values); Constant: variance
    everywhere; both without reading X (a NaN there does not reach the output), -2 dk/dr2 = 0;
  * what the device refuses (GPK_E_ARG / GPK_E_UNSUPPORTED) is an AssertionError here: "dalpha" for another family, alpha missing,
    <= 0 or not finite, alpha given to another family, a RationalQuadratic member in the per-latent shard.
The fused chains end in a stage they are GIVEN: `_shard` (shared kernel) and `_shard_sep` (one kernel per latent) take it as an
argument; the public functions pass the Gaussian stage, tests/fake_likelihood_ops.py and tests/fake_lcm_ops.py pass theirs.  Every
emulated name is defined in one module only (tests/emulation.py checks it and installs them all).
The product never imports this file.
"""
from __future__ import annotations

import numpy as np
import scipy.linalg as sla
import torch

NB = 128


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


KERNEL_FAMILIES = {"SquaredExponential": 0, "Matern12": 1, "Matern32": 2, "Matern52": 3, "Exponential": 4, "RationalQuadratic": 5,
                   "White": 6, "Constant": 7}    # include/gpk.h: GPK_KERN_SE .. GPK_KERN_CONSTANT


def device():
    return torch.device("cpu")


def to_device(x, dtype=torch.float64):
    # always a private copy, like a host -> device transfer (in-place primitives must never reach the caller's array)
    if isinstance(x, torch.Tensor):
        return x.to(dtype=dtype).contiguous()
    return torch.tensor(np.array(x, dtype=np.float64, copy=True), dtype=dtype).contiguous()


def _ls(lengthscales, d):
    return np.broadcast_to(np.asarray(lengthscales, dtype=np.float64), (d,))


def _k(X1, X2, variance, lengthscales, family="SquaredExponential"):
    a, b = _np(X1) / _ls(lengthscales, X1.shape[1]), _np(X2) / _ls(lengthscales, X1.shape[1])
    r2 = -2.0 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    if family == "SquaredExponential":
        return variance * np.exp(-0.5 * r2)
    r = np.sqrt(np.maximum(r2, 1e-36))           # stationaries.py:113-114
    if family == "Matern12":
        return variance * np.exp(-r)
    if family == "Matern32":
        return variance * (1.0 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r)
    if family == "Matern52":
        return variance * (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)
    raise KeyError(family)


def _dr2(X1, X2, variance, lengthscales, family):
    """-2 dk/dr2 at the scaled squared distance (zero where the 1e-36 clamp is active)."""
    a, b = _np(X1) / _ls(lengthscales, X1.shape[1]), _np(X2) / _ls(lengthscales, X1.shape[1])
    r2 = -2.0 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    if family == "SquaredExponential":
        return variance * np.exp(-0.5 * r2)
    ok = ~(r2 <= 1e-36)                          # (a NaN r2 is not clamped: it comes out as NaN, like tf.maximum's gradient)
    r = np.sqrt(np.where(ok, r2, 1.0))
    if family == "Matern12":
        f = variance * np.exp(-r) / r
    elif family == "Matern32":
        f = 3.0 * variance * np.exp(-np.sqrt(3.0) * r)
    elif family == "Matern52":
        f = (5.0 / 3.0) * variance * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)
    else:
        raise KeyError(family)
    return np.where(ok, f, 0.0)


def _alpha(family, alpha):
    if family == "RationalQuadratic":
        assert alpha is not None, "RationalQuadratic needs alpha"                         # (ops: ValueError)
        assert np.isfinite(float(alpha)) and float(alpha) > 0.0, alpha                     # GPK_E_ARG
        return float(alpha)
    assert alpha is None, f"alpha given to {family}"                                      # (ops: ValueError)
    assert family in KERNEL_FAMILIES, family
    return None


def _profile(X1, X2, variance, lengthscales, family, alpha, what="k"):
    """k, -2 dk/dr2 ("dr2") or dk/dalpha ("dalpha") for [n1, n2]; X2 None = K(X1, X1)"""
    n1, n2 = X1.shape[0], (X1 if X2 is None else X2).shape[0]
    if family in ("White", "Constant"):
        if what != "k":
            return np.zeros((n1, n2))
        if family == "Constant":
            return np.full((n1, n2), float(variance))
        return float(variance) * np.eye(n1) if X2 is None else np.zeros((n1, n2))
    if family not in ("Exponential", "RationalQuadratic"):   # the four first families: the formulas the contract tables compare bits with
        return (_k if what == "k" else _dr2)(X1, X1 if X2 is None else X2, variance, lengthscales, family)
    a, b = _np(X1) / _ls(lengthscales, X1.shape[1]), _np(X1 if X2 is None else X2) / _ls(lengthscales, X1.shape[1])
    r2 = -2.0 * a @ b.T + (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :]
    if family == "Exponential":
        if what == "k":
            return variance * np.exp(-0.5 * np.sqrt(np.where(r2 < 1e-36, 1e-36, r2)))
        ok = ~(r2 <= 1e-36)
        r = np.sqrt(np.where(ok, r2, 1.0))
        return np.where(ok, variance * np.exp(-0.5 * r) / (2.0 * r), 0.0)
    u = r2 / (2.0 * alpha)
    l1p = np.log1p(u)
    if what == "k":
        return variance * np.exp(-alpha * l1p)
    if what == "dr2":
        return variance * np.exp(-(alpha + 1.0) * l1p)
    return variance * np.exp(-alpha * l1p) * (u / (1.0 + u) - l1p)


def _ret(R, out):
    Rt = torch.from_numpy(np.ascontiguousarray(R, dtype=np.float64))
    if out is None:
        return Rt
    out.copy_(Rt)
    return out


def kernel_matrix(X1, X2, *, variance, lengthscales, family="SquaredExponential", diag_add=0.0, lower_only=False, alpha=None,
                  out=None):
    alpha = _alpha(family, alpha)
    with np.errstate(all="ignore"):
        K = _profile(X1, X2, variance, lengthscales, family, alpha)
        if X2 is None:
            K = K + diag_add * np.eye(K.shape[0])
            if lower_only:   # tiles strictly above the diagonal are not written
                K = np.where(np.triu(np.ones_like(K), 1) > 0, np.nan, K)
    return _ret(K, out)


def kernel_matrix_hadamard(X1, X2, G, *, variance, lengthscales, family="SquaredExponential", alpha=None, out=None):
    assert X2 is not None and tuple(G.shape) == (X1.shape[0], X2.shape[0])
    alpha = _alpha(family, alpha)
    with np.errstate(all="ignore"):
        return _ret(_profile(X1, X2, variance, lengthscales, family, alpha) * _np(G), out)


def kernel_matrix_combine(X1, X2, G, *, op, variance, lengthscales, family="SquaredExponential", diag_add=0.0, alpha=None, out=None):
    assert op in ("mul", "add", "dr2", "dalpha"), op                                       # GPK_E_ARG
    assert op != "dalpha" or family == "RationalQuadratic", (op, family)                   # GPK_E_UNSUPPORTED
    alpha = _alpha(family, alpha)
    with np.errstate(all="ignore"):
        if op in ("dr2", "dalpha"):
            R = _profile(X1, X2, variance, lengthscales, family, alpha, op) * _np(G)
            if X2 is None:
                np.fill_diagonal(R, 0.0)
        else:
            K = _profile(X1, X2, variance, lengthscales, family, alpha)
            R = K * _np(G) if op == "mul" else K + _np(G)
            if X2 is None:
                R = R + diag_add * np.eye(R.shape[0])
    return _ret(R, out)


def _invd(n, batch, mark):
    """Stand-in for the diagonal-block inverses: the emulation solves with L itself, the tensor only carries a marker
    (+1: belongs to L, -1: to L^T from transpose_factor) so that a wrong pairing is caught."""
    return torch.full((batch * (-(-n // NB)) * NB * NB,), mark, dtype=torch.float64)


def invd_alloc(n, batch=1):
    return _invd(n, batch, 0.0)


def _chol_info(K):
    """(L, info): info = j + 1 of the first pivot that is not > 0 -- non-positive or NaN (include/gpk.h, "info") -- tested
    explicitly on every pivot (LAPACK does not promise to raise on a NaN one).  Row by row, so that a row of L is a function
    of the rows of K up to it and of nothing else: rows < info - 1 are final and bitwise what a successful factorisation of
    the same leading rows gives; the rest is NaN."""
    n = K.shape[0]
    L = np.full_like(K, np.nan)
    with np.errstate(all="ignore"):
        for j in range(n):
            row = sla.solve_triangular(L[:j, :j], K[j, :j], lower=True, check_finite=False) if j else K[j, :0]
            piv = K[j, j] - row @ row
            if not piv > 0:
                return L, j + 1
            L[j, :j], L[j, j], L[j, j + 1:] = row, np.sqrt(piv), 0.0
    return L, 0


def potrf_(T, n, *, zero_upper=False, invd=None, identity_rows=False):
    if identity_rows:
        assert T.dim() == 2 and T.shape[0] >= 2 * n
        T[T.shape[0] - n:] = torch.eye(n, dtype=T.dtype)
    if T.dim() == 3:
        infos = []
        for b in range(T.shape[0]):
            _, info = potrf_(T[b], n, zero_upper=zero_upper)
            infos.append(int(info[0]))
        return _invd(n, T.shape[0], +1.0), torch.tensor(infos, dtype=torch.int32)
    assert T.dim() == 2 and T.shape[1] == n and T.stride(1) == 1
    K = np.tril(_np(T[:n]))
    K = K + np.tril(K, -1).T          # only the lower triangle is read
    L, bad = _chol_info(K)
    if bad:   # rows before the bad pivot are final (they depend on nothing after them); everything else is left as it was
        up = np.triu(_np(T[:bad - 1]), 1)
        T[:bad - 1] = torch.from_numpy(L[:bad - 1] + (0.0 if zero_upper else up))
        return _invd(n, 1, +1.0), torch.tensor([bad], dtype=torch.int32)
    E = _np(T[n:])
    S = sla.solve_triangular(L, E.T, lower=True, check_finite=False).T if E.shape[0] else E
    up = np.triu(_np(T[:n]), 1)
    T[:n] = torch.from_numpy(L + (0.0 if zero_upper else up))
    T[n:] = torch.from_numpy(S)
    return _invd(n, 1, +1.0), torch.zeros(1, dtype=torch.int32)


def check_info(info, what="Cholesky"):
    from gpflow_amd._lib import GpkError
    bad = _np(info)
    if np.any(bad != 0):
        raise GpkError(f"{what} decomposition was not successful: non-positive pivot at column {int(bad[bad != 0][0]) - 1}")


def trtri_blocks(L):
    return _invd(L.shape[0], 1, +1.0)


def transpose_factor(L, invd):
    assert float(invd.reshape(-1)[0]) == 1.0
    return torch.tril(L).t().contiguous(), _invd(L.shape[0], 1, -1.0)


def trsm_(B, L, invd, *, trans=0):
    """trans=0: B <- B L^-T given (L, invd); trans=1: B <- B L^-1 given (LT, invdT)."""
    n = L.shape[0]
    if trans == 0:
        assert float(invd.reshape(-1)[0]) == 1.0, "trans=0 needs (L, invd)"
        Ll = np.tril(_np(L))
        B.copy_(torch.from_numpy(sla.solve_triangular(Ll, _np(B).T, lower=True, check_finite=False).T))
    else:
        assert float(invd.reshape(-1)[0]) == -1.0, "trans=1 needs (LT, invdT) from transpose_factor"
        Ll = np.triu(_np(L)).T      # the argument is L^T (upper); only that triangle is read
        # B L^-1 = (L^-T B^T)^T
        B.copy_(torch.from_numpy(sla.solve_triangular(Ll.T, _np(B).T, lower=False, check_finite=False).T))
    return B


def gemm_nt(A, B, *, alpha=1.0, beta=0.0, C=None, b_tri=0, c_lower=False, a_tri=0, k_split=False, zero_skipped=True):
    # the device refuses these flag values (gpk_gemm_nt: GPK_E_ARG)
    assert b_tri in (0, 1, 2) and a_tri in (0, 1, 2), (b_tri, a_tri)
    if k_split:   # batch entries = consecutive K chunks of one product; the structure statements are about the unsplit column index
        assert A.dim() == 3 and B.dim() == 3 and A.shape[0] == B.shape[0] and A.shape[2] % 16 == 0
        if b_tri:   # the hint must be TRUE of the concatenated B as well: the device skips the K ranges it declares zero
            B2 = _np(torch.cat(list(B), dim=1))
            assert np.all((np.tril(B2, -1) if b_tri == 1 else np.triu(B2, 1)) == 0), "b_tri set on a K-split B without that structure"
    if a_tri:   # the hint must be TRUE: the device kernel skips the K range it declares zero
        A2 = _np(torch.cat(list(A), dim=1)) if k_split else _np(A if A.dim() == 2 else A[0])
        assert np.all((np.tril(A2, -1) if a_tri == 1 else np.triu(A2, 1)) == 0), "a_tri set on a matrix without that structure"
    batched = A.dim() == 3 or B.dim() == 3
    A3 = A if A.dim() == 3 else A.unsqueeze(0)
    B3 = B if B.dim() == 3 else B.unsqueeze(0)
    batch = max(A3.shape[0], B3.shape[0])
    m, k = A3.shape[1], A3.shape[2]
    n = B3.shape[1]
    assert B3.shape[2] == k
    if C is None:
        assert beta == 0.0
        C = torch.zeros((batch, m, n) if batched else (m, n), dtype=torch.float64)
        if not c_lower or not zero_skipped:
            C.fill_(float("nan"))     # every entry must be written by the kernel (zero_skipped=False: skipped tiles stay uninitialised)
    C3 = C if C.dim() == 3 else C.unsqueeze(0)
    for z in range(batch):
        a = _np(A3[z if A3.shape[0] > 1 else 0])
        b = _np(B3[z if B3.shape[0] > 1 else 0]).copy()
        for n0 in range(0, n, NB):
            n1 = min(n0 + NB, n)
            kb, ke = 0, k
            koff = z * k if k_split else 0
            if b_tri == 1:
                kb = min(max(n0 - koff, 0) & ~15, k)
            elif b_tri == 2:
                ke = max(min(n0 + NB - koff, k), kb)
            prod = a[:, kb:ke] @ b[n0:n1, kb:ke].T
            for m0 in range(0, m, NB):
                m1 = min(m0 + NB, m)
                if c_lower and n0 > m0 + NB - 1:
                    continue
                old = _np(C3[z, m0:m1, n0:n1])
                new = alpha * prod[m0:m1] + (beta * old if beta != 0.0 else 0.0)
                C3[z, m0:m1, n0:n1] = torch.from_numpy(new)
    return C


def transpose(X, *, mode=0, out=None):
    Y = X
    if mode == 1:
        Y = torch.tril(X)
    elif mode == 2:
        Y = torch.triu(X)
    R = Y.transpose(-1, -2).clone(memory_format=torch.contiguous_format)   # always new storage, like the kernel's output
    if out is None:
        return R
    out.copy_(R)
    return out


def row_stats(At, *, V=None, W=None, want_sumsq=True):
    a = _np(At)
    sumsq = torch.from_numpy((a * a).sum(1)) if want_sumsq else None
    mv = torch.from_numpy(a @ _np(V)) if V is not None else None
    wsq = torch.from_numpy(((a * a) @ (_np(W) ** 2)).T.copy()) if W is not None else None
    return sumsq, mv, wsq


def _noise(noise_variance, rows):
    """The (noise_variance, noise_rows) pair of the C-ABI: a constant, or one variance per row -> [rows, 1]."""
    if isinstance(noise_variance, (torch.Tensor, np.ndarray)) and int(np.prod(tuple(noise_variance.shape))) != 1:
        nv = _np(noise_variance).reshape(-1)
        assert nv.size == rows, (nv.size, rows)
        return nv[:, None]
    return float(noise_variance)


def diag_add_(A, v):
    """gpk_diag_add: A[i,i] += v[i] in place"""
    v = to_device(v).reshape(-1)
    n = min(A.shape[0], A.shape[1])
    assert v.numel() == n
    idx = torch.arange(n)
    A[idx, idx] += v
    return A


def gaussian_varexp_sum(Y, fmean, *, s0, ssq, knn, noise_variance, mean_const=0.0, s0_per_latent=False,
                        want_fvar=False):
    P = fmean.shape[1]
    assert 1 <= P <= 16, P    # gpk_gaussian_varexp_sum: GPK_E_ARG outside 1 .. 16 latents
    knn = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=np.float64)), (P,)) if np.size(knn) in (1, P) else None
    fv = np.tile(knn[None, :], (fmean.shape[0], 1)).astype(np.float64)
    if s0 is not None:
        fv = fv - (_np(s0).T if s0_per_latent else _np(s0)[:, None])
    if ssq is not None:
        fv = fv + _np(ssq).T
    nv = _noise(noise_variance, fmean.shape[0])
    ve = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(nv) \
        - 0.5 * ((_np(Y) - _np(fmean) - mean_const) ** 2 + fv) / nv
    return torch.tensor([ve.sum()], dtype=torch.float64), (torch.from_numpy(fv) if want_fvar else None)


def gauss_kl_white(q_mu, q_sqrt):
    M, P = q_mu.shape
    assert M >= 1 and P >= 1, (M, P)    # gpk_gauss_kl_white: GPK_E_ARG
    if q_sqrt.dim() == 2:      # q_diag: std-devs [M, P]
        s = _np(q_sqrt)
        kl = 0.5 * ((_np(q_mu) ** 2).sum() - M * P - np.log(s ** 2).sum() + (s * s).sum())
        return torch.tensor([kl], dtype=torch.float64)
    Lq = np.tril(_np(q_sqrt))
    kl = 0.5 * ((_np(q_mu) ** 2).sum() - M * P - np.log(np.diagonal(Lq, axis1=1, axis2=2) ** 2).sum() + (Lq * Lq).sum())
    return torch.tensor([kl], dtype=torch.float64)


def combine_parts(parts, *, alpha=1.0, lower=False, diag_scale=1.0, out=None):
    p3 = _np(parts if parts.dim() == 3 else parts.unsqueeze(0))
    if lower:   # entries above the diagonal may be NaN (unwritten tiles of a lower-only GEMM): never read
        p3 = np.where(np.tril(np.ones(p3.shape[1:], dtype=bool))[None], p3, 0.0)
    r = alpha * p3.sum(0)
    if lower:
        r = np.tril(r)
        r[np.diag_indices(min(r.shape))] *= diag_scale
    t = torch.from_numpy(r)
    if out is not None:
        out.copy_(t)
        return out
    return t


def sumsq(A, *, upper_only=False):
    a = _np(A)
    if upper_only:
        a = np.triu(a)
    return torch.tensor([(a * a).sum()], dtype=torch.float64)


def sum_log_diag(L):
    L3 = L if L.dim() == 3 else L.unsqueeze(0)
    assert min(L3.shape[1], L3.shape[2]) >= 1, tuple(L.shape)    # gpk_sum_log_diag: GPK_E_ARG for n = 0
    return torch.from_numpy(np.log(np.diagonal(_np(L3), axis1=1, axis2=2)).sum(1))


def row_dot(A, B):
    return torch.from_numpy((_np(A) * _np(B)).sum(1))


def project(At, LqT):
    """ssq [P, rows] = sum_j (At Lq_p)[b, j]^2 with LqT[p] = tril(q_sqrt_p)^T (already triangular-clean)."""
    a = _np(At)
    return torch.from_numpy(np.stack([(((a[p] if a.ndim == 3 else a) @ _np(LqT[p]).T) ** 2).sum(1)
                                      for p in range(LqT.shape[0])]))


def gpr_lml(X, Y, *, variance, lengthscales, noise_variance, mean_const=0.0, family="SquaredExponential", alpha=None, ws=None):
    """The fused driver, emulated by the same chain of primitives it runs (drivers.hip: gpk_gpr_lml)."""
    _alpha(family, alpha)
    n, P = Y.shape
    assert n >= 1 and P >= 1, (n, P)    # gpk_gpr_lml: GPK_E_ARG
    T = torch.empty((n + P, n), dtype=torch.float64)
    nv = _noise(noise_variance, n)
    kernel_matrix(X, None, variance=variance, lengthscales=lengthscales, family=family, alpha=alpha,
                  diag_add=0.0 if isinstance(nv, np.ndarray) else nv, lower_only=True, out=T[:n])
    if isinstance(nv, np.ndarray):
        diag_add_(T[:n], torch.from_numpy(nv[:, 0].copy()))
    T[n:] = (Y - mean_const).t()
    _, info = potrf_(T, n)
    if int(info[0]):
        return torch.full((1,), float("nan"), dtype=torch.float64), info
    lml = -0.5 * sumsq(T[n:])[0] - 0.5 * n * P * np.log(2 * np.pi) - P * sum_log_diag(T[:n])[0]
    return lml.reshape(1), info


def svgp_elbo_sep_workspace(m, rows, d, P):
    return torch.empty(1, dtype=torch.float64)


def _gaussian_stage(noise_variance):
    """the last stage of the fused chains as their public forms run it (the workers below take theirs as an argument)"""
    def stage(Y, fmean, **kw):
        return gaussian_varexp_sum(Y, fmean, noise_variance=noise_variance, **kw)
    return stage


def _shard_sep(Z, Xb, Yb, q_mu, q_sqrt, stage, *, variances, lengthscales, families, jitter, mean_const=0.0, out=None):
    """The per-latent chain (whitened; one kernel per latent; full q_sqrt) up to its last stage: `stage` takes the operands of
    gaussian_varexp_sum but the noise and returns its pair -- the Gaussian stage for gpk_svgp_elbo_shard_sep, the mixing stage for
    gpk_svgp_elbo_shard_lcm."""
    assert "RationalQuadratic" not in list(families), "no slot for alpha in the per-latent shard"   # GPK_E_UNSUPPORTED
    P = q_mu.shape[1]
    M, rows = Z.shape[-2], Xb.shape[0]
    assert 1 <= P <= 16 and M >= 1, (P, M)    # gpk_svgp_elbo_shard_sep: GPK_E_ARG
    ls = np.asarray(lengthscales, dtype=np.float64)
    T = torch.empty((P, M + rows, M), dtype=torch.float64)
    for p in range(P):
        Zp = Z if Z.dim() == 2 else Z[p]
        kw = dict(variance=float(variances[p]), lengthscales=ls[p], family=families[p])
        kernel_matrix(Zp, None, diag_add=jitter, lower_only=True, out=T[p, :M], **kw)
        if rows:
            kernel_matrix(Xb, Zp, out=T[p, M:], **kw)
    _, inf = potrf_(T, M)
    res = torch.full((2,), float("nan"), dtype=torch.float64)   # undefined after a failed factorisation: poisoned
    if not bool((inf != 0).any()):
        res.zero_()
        s0 = torch.stack([row_stats(T[p, M:].contiguous(), V=q_mu[:, p:p + 1].contiguous())[0] for p in range(P)])
        fmean = torch.stack([row_stats(T[p, M:].contiguous(), V=q_mu[:, p:p + 1].contiguous())[1][:, 0] for p in range(P)], dim=1)
        ssq = project(T[:, M:], transpose(q_sqrt, mode=1))
        ve, _ = stage(Yb, fmean.contiguous(), s0=s0, ssq=ssq, knn=[float(v) for v in variances], mean_const=mean_const,
                      s0_per_latent=True)
        res[0] = ve[0]
        res[1] = gauss_kl_white(q_mu, q_sqrt)[0]
    if out is not None:
        out.copy_(res)
        res = out
    return res, inf


def svgp_elbo_shard_sep(Z, Xb, Yb, q_mu, q_sqrt, *, variances, lengthscales, families, noise_variance, jitter, mean_const=0.0,
                        ws=None, out=None, info=None):
    """gpk_svgp_elbo_shard_sep emulated by its chain of primitives, ending in the Gaussian stage"""
    return _shard_sep(Z, Xb, Yb, q_mu, q_sqrt, _gaussian_stage(noise_variance), variances=variances, lengthscales=lengthscales,
                      families=families, jitter=jitter, mean_const=mean_const, out=out)


def svgp_elbo_workspace(m, rows, d, P, q_diag, whiten=True):
    return torch.empty(1, dtype=torch.float64)


def svgp_elbo_shard(Z, Xb, Yb, q_mu, q_sqrt, *, variance, lengthscales, noise_variance, jitter, mean_const=0.0,
                    family="SquaredExponential", alpha=None, ws=None, out=None, info=None, whiten=True):
    """gpk_svgp_elbo_shard emulated by its own chain of primitives, ending in the Gaussian stage"""
    return _shard(Z, Xb, Yb, q_mu, q_sqrt, _gaussian_stage(noise_variance), variance=variance, lengthscales=lengthscales, jitter=jitter,
                  mean_const=mean_const, family=family, alpha=alpha, out=out, whiten=whiten)


def _shard(Z, Xb, Yb, q_mu, q_sqrt, stage, *, variance, lengthscales, jitter, mean_const=0.0, family="SquaredExponential", alpha=None,
           out=None, whiten=True):
    """The shared-kernel chain (whitened, or un-whitened on one trapezoid) up to its last stage: `stage` takes the operands of
    gaussian_varexp_sum but the noise and returns its pair -- the Gaussian stage for gpk_svgp_elbo_shard, a quadrature stage for
    gpk_svgp_elbo_shard_lik (fake_likelihood_ops)."""
    _alpha(family, alpha)
    M, rows, P = Z.shape[0], Xb.shape[0], q_mu.shape[1]
    assert 1 <= P <= 16 and M >= 1, (P, M)    # gpk_svgp_elbo_shard: GPK_E_ARG
    kw = dict(variance=variance, lengthscales=lengthscales, family=family, alpha=alpha)
    if not whiten and q_sqrt.dim() == 2:
        # un-whitened, diagonal q_sqrt: [Kuu ; Kfu ; q_mu^T ; I] -> A^T, (Lm^-1 q_mu)^T, Lm^-T (drivers.hip, round 5)
        T = torch.empty((M + rows + P + M, M), dtype=torch.float64)
        kernel_matrix(Z, None, diag_add=jitter, lower_only=True, out=T[:M], **kw)
        if rows:
            kernel_matrix(Xb, Z, out=T[M:M + rows], **kw)
        T[M + rows:M + rows + P] = q_mu.t()
        _, inf = potrf_(T, M, identity_rows=True)
        res = torch.full((2,), float("nan"), dtype=torch.float64)   # undefined after a failed factorisation: poisoned
        if int(inf[0]) == 0:
            res.zero_()
            At = T[M:M + rows].contiguous()
            LinvT = T[M + rows + P:].contiguous()
            A2 = gemm_nt(At, LinvT, b_tri=1) if rows else At
            s0 = row_stats(At)[0] if rows else torch.zeros(0, dtype=torch.float64)
            _, fmean, ssq = row_stats(A2, V=q_mu, W=q_sqrt, want_sumsq=False) if rows else (None, torch.zeros((0, P), dtype=torch.float64), torch.zeros((P, 0), dtype=torch.float64))
            ve, _ = stage(Yb, fmean, s0=s0, ssq=ssq, knn=[variance], mean_const=mean_const)
            res[0] = ve[0]
            kinv = (np.triu(_np(LinvT)) ** 2).sum(1)
            w = _np(q_sqrt)
            res[1] = 0.5 * float((_np(T[M + rows:M + rows + P]) ** 2).sum()) + 0.5 * float((kinv[:, None] * w ** 2).sum()) \
                - 0.5 * float(np.log(w ** 2).sum()) - 0.5 * M * P + P * float(np.log(np.diagonal(_np(T[:M]))).sum())
        if out is not None:
            out.copy_(res)
            res = out
        return res, inf
    if not whiten:
        T = torch.empty((M + rows + P + P * M, M), dtype=torch.float64)
        kernel_matrix(Z, None, diag_add=jitter, lower_only=True, out=T[:M], **kw)
        if rows:
            kernel_matrix(Xb, Z, out=T[M:M + rows], **kw)
        T[M + rows:M + rows + P] = q_mu.t()
        T[M + rows + P:] = transpose(q_sqrt, mode=1).reshape(P * M, M)
        _, inf = potrf_(T, M)
        res = torch.full((2,), float("nan"), dtype=torch.float64)   # undefined after a failed factorisation: poisoned
        if int(inf[0]) == 0:
            res.zero_()
            At = T[M:M + rows].contiguous()
            V = T[M + rows:M + rows + P].t().contiguous()
            GT = T[M + rows + P:].reshape(P, M, M).contiguous()
            s0, fmean, _ = row_stats(At, V=V)
            ssq = project(At, GT)
            ve, _ = stage(Yb, fmean, s0=s0, ssq=ssq, knn=[variance], mean_const=mean_const)
            res[0] = ve[0]
            Lq = np.tril(_np(q_sqrt))
            res[1] = 0.5 * float((_np(T[M + rows:M + rows + P]) ** 2).sum()) + 0.5 * float((_np(GT) ** 2).sum()) - 0.5 * M * P \
                - 0.5 * float(np.log(np.diagonal(Lq, axis1=1, axis2=2) ** 2).sum()) \
                + P * float(np.log(np.diagonal(_np(T[:M]))).sum())
        if out is not None:
            out.copy_(res)
            res = out
        return res, inf
    T = torch.empty((M + rows, M), dtype=torch.float64)
    kernel_matrix(Z, None, diag_add=jitter, lower_only=True, out=T[:M], **kw)
    if rows:
        kernel_matrix(Xb, Z, out=T[M:], **kw)
    _, inf = potrf_(T, M)
    res = torch.full((2,), float("nan"), dtype=torch.float64)   # undefined after a failed factorisation: poisoned
    if int(inf[0]) == 0:
        res.zero_()
        At = T[M:]
        if q_sqrt.dim() == 2:
            s0, fmean, wsq = row_stats(At, V=q_mu, W=q_sqrt)
            ssq = wsq
        else:
            s0, fmean, _ = row_stats(At, V=q_mu)
            ssq = project(At.contiguous(), transpose(q_sqrt, mode=1))
        ve, _ = stage(Yb, fmean, s0=s0, ssq=ssq, knn=[variance], mean_const=mean_const)
        res[0] = ve[0]
        res[1] = gauss_kl_white(q_mu, q_sqrt)[0]
    if out is not None:
        out.copy_(res)
        res = out
    return res, inf


# ---- reverse-pass glue (include/gpk.h: gpk_moment_rows, gpk_stationary_adjoint_tail, gpk_adam_step, gpk_symmetrize) ----
def moment_rows(B):
    Bt = B.t()
    return torch.cat([torch.ones((1, B.shape[0]), dtype=torch.float64), Bt, Bt * Bt], 0).contiguous()


def stationary_adjoint_tail(R, A, ls, *, variance, symmetric, sum_kbar_k=None, into=None, dvar_add=0.0):
    D = A.shape[1]
    rs, GB, GB2 = R[:, 0:1], R[:, 1:1 + D], R[:, 1 + D:]
    T = GB - A * rs
    if symmetric:
        Abar = T * (2.0 / (ls * ls))
        dls = -(A * Abar).sum(0) / ls
    else:
        Abar = T / (ls * ls)
        dls = (GB2 - A * (GB + T)).sum(0) / ls ** 3
    dvar = (rs.sum() if sum_kbar_k is None else sum_kbar_k.reshape(())) / variance + dvar_add
    if into is not None:
        small, acc = into
        small[0:1] += dvar.reshape(1)
        small[1:] += dls
        acc += Abar
        return small[0:1], small[1:], acc
    small = torch.cat([dvar.reshape(1), dls])
    return small[0:1], small[1:], Abar


def adam_step_(p, g, m, v, *, beta1, beta2, epsilon, step, maximise=False):
    gg = -g if maximise else g
    m.mul_(beta1).add_(gg, alpha=1.0 - beta1)
    v.mul_(beta2).addcmul_(gg, gg, value=1.0 - beta2)
    p.addcdiv_(m, v.sqrt().add_(epsilon), value=-step)
    return p


def symmetrize_(S):
    S.copy_(0.5 * (S + S.t()))
    return S


def lowrank_axpy(alpha, X, U, V):
    assert 0 < U.shape[1] <= 16 and tuple(V.shape) == (X.shape[1], U.shape[1]) and U.shape[0] == X.shape[0]   # gpk_lowrank_axpy
    return alpha * X + U @ V.t()
