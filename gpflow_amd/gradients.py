"""Reverse pass of the SVGP hot path (what turns "ELBO steps/s" into "training steps/s").

The reference gets these gradients from TensorFlow autodiff over `SVGP.elbo` (`optimizers/scipy.py:322-331`,
`models/training_mixins.py:59-78`, the Adam loop of `gps_for_big_data.pct.py:207-228`).  Here the adjoint of each
stage of the whitened ELBO is written out and executed with the same device primitives as the forward pass --
the fp64 MFMA GEMM (plain / triangular-K / lower-only), the trapezoidal Cholesky with its fused solve (which also
delivers Lm^-T from appended identity rows, so no triangular solve is left in the backward), the covariance builder (and its `G .* K` variant) -- so the backward is, like the
forward, a short list of big GEMM-shaped launches:

    forward   Kuu, Kfu -> Lm, At = Kfu Lm^-T -> fmean = At q_mu, s0 = rowsum(At^2), W_p = At Lq_p, ssq = rowsum(W_p^2)
              F = scale * sum var_exp(fmean, sigma^2 - s0 + ssq) - KL[q || N(0, I)]
    backward  At_bar = r q_mu^T - 2 c P At + 2 c sum_p W_p Lq_p^T              r = dF/dfmean, c = dF/dfvar
              q_mu_bar = At^T r - q_mu,   Lq_bar_p = 2 c tril(At^T W_p) - tril(Lq_p) + diag(1 / Lq_p)
              Kfu_bar = At_bar Lm^-1,     Lm_bar = -tril(Kfu_bar^T At)
              Kuu_bar = sym( Lm^-T Phi(Lm^T Lm_bar) Lm^-1 )                    (Cholesky adjoint; Phi = tril, half diagonal)
              kernel parameters and Z from  G = Kbar .* K  contracted with [1, x, x^2]   (SquaredExponential)

Small O(M^2) / O(B P) elementwise steps (masks, the residual r, the final [M, 2D+1] contractions) are torch
device ops -- glue between the kernels, never a fallback: every function here needs the HIP library.

All arrays are fp64 device tensors; gradients are returned w.r.t. the CONSTRAINED quantities (variance,
lengthscales, noise variance, Z, q_mu, q_sqrt); `SVGP.elbo_and_grad` chains them through the parameter transforms.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import collections
import os

import numpy as np
import torch

from . import ops
from .leaf import ArcLeaf, CoregionLeaf, DotLeaf, Leaf

LOG2PI = float(np.log(2.0 * np.pi))

# The reverse pass has two independent branches after Kfu_bar: {q_mu_bar, Lq_bar} (two long-K products, 544 workgroups
# each) and {Lm_bar -> Cholesky adjoint -> Kuu adjoint} (M^3 products of 256 tiles: one workgroup per CU, time of the
# longest tile).  On a device they run on two streams so that the under-filled launches share the chip.
OVERLAP_BRANCHES = True
# the side branch's chip-filling GEMMs start only when the main branch's HBM-bound preparation is enqueued (_SideBranch.release)
GATE_SIDE_BRANCH = os.environ.get("GPFLOW_AMD_GATE_SIDE_BRANCH", "1") != "0"
# K chunks of the triangular x triangular products of the Cholesky adjoint (1 = unsplit)
TRI_PRODUCT_CHUNKS = int(os.environ.get("GPFLOW_AMD_TRI_PRODUCT_CHUNKS", "4"))
TRI_PRODUCT_MIN_N = 1024   # below this the unsplit launches are short anyway
_side_streams: Dict[int, "torch.cuda.Stream"] = {}


def _side_stream(dev: torch.device):
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _side_streams:
        # (a LOW-priority side stream -- hipStreamCreateWithPriority, wrapped as an ExternalStream -- was tried in round 6 so that the main
        #  branch's short kernels would win the freed slots: training step 6.02 -> 6.9 ms, profiles/r06_ab_train_side_branch.log)
        _side_streams[idx] = torch.cuda.Stream(device=dev)
    return _side_streams[idx]


def splitk_gemm_nt(A: torch.Tensor, Bt: torch.Tensor, *, c_lower: bool = False, target_wgs: int = 1100,
                   alpha: float = 1.0, diag_scale: float = 1.0) -> torch.Tensor:
    """alpha A Bt^T for a LONG inner dimension and few output tiles (At^T r, At^T W, G [1, x, x^2]): the K range is cut
    into chunks that run as the batch dimension of one launch (strided views, no copies) and the partial products are
    summed by ops.combine_parts in a fixed order -- without the split a [2048, 2048] lower-only output is 136 workgroups
    each walking K = 8192 (33 TFLOP/s), and an [M, 17] output is 16 workgroups.  target_wgs ~ two full rounds of the 512
    resident workgroups (A/B on the training step: 272 workgroups 8.08 ms, 544 7.9, 1088 7.65, 2176 7.78).
    c_lower=True returns tril(.) (exact zeros above the diagonal) with the diagonal multiplied by diag_scale."""
    m, k = A.shape
    n = Bt.shape[0]
    tm, tn = -(-m // 128), -(-n // 128)
    tiles = tm * tn
    if c_lower:   # tiles on or below the diagonal
        tiles = sum(min(tn, i + 1) for i in range(tm))
    chunks = 1
    while chunks * 2 * tiles <= target_wgs and k % (chunks * 2) == 0 and (k // (chunks * 2)) % 16 == 0 \
            and k // (chunks * 2) >= 256:
        chunks *= 2
    if chunks == 1:
        R = ops.gemm_nt(A, Bt, c_lower=c_lower, alpha=alpha, zero_skipped=False)   # (combine_parts(lower) never reads above the diagonal)
        return ops.combine_parts(R, lower=True, diag_scale=diag_scale) if c_lower else R
    kc = k // chunks
    A3 = torch.as_strided(A, (chunks, m, kc), (kc, A.stride(0), 1), A.storage_offset())
    B3 = torch.as_strided(Bt, (chunks, n, kc), (kc, Bt.stride(0), 1), Bt.storage_offset())
    return ops.combine_parts(ops.gemm_nt(A3, B3, c_lower=c_lower, zero_skipped=False), alpha=alpha, lower=c_lower, diag_scale=diag_scale)


def _tril(x: torch.Tensor) -> torch.Tensor:
    """band_part(x, -1, 0) of [M, M] or [P, M, M] as a fresh tensor (one 16-byte-access pass per matrix)."""
    if x.dim() == 2:
        return ops.combine_parts(x, lower=True)
    out = torch.empty_like(x)
    for p in range(x.shape[0]):
        ops.combine_parts(x[p], lower=True, out=out[p])
    return out


def _phi_(T: torch.Tensor) -> torch.Tensor:
    """Phi(T): lower triangle with the diagonal halved (a fresh tensor)."""
    return ops.combine_parts(T, lower=True, diag_scale=0.5)


def cholesky_adjoint(LT: torch.Tensor, LinvT: torch.Tensor, Lbar: torch.Tensor, before_products=None) -> torch.Tensor:
    """Symmetric K_bar with  <K_bar, dK> = <L_bar, dL>  for K = L L^T:  K_bar = sym(L^-T Phi(L^T L_bar) L^-1), with
    LT = L^T, LinvT = L^-T (both upper, zero below the diagonal) and L_bar lower.  Three triangular-K GEMMs; the
    explicit inverse comes for free from the factorisation (identity rows appended to the trapezoid).
    before_products: called once the HBM-bound preparation is enqueued (see _SideBranch.release: the side branch's big GEMM is gated on it)."""
    # every B operand below is the transpose of a lower-triangular matrix: B[j, kk] = 0 for kk < j  -> b_tri = 1
    # (a_tri: A is triangular as well -- upper L^T / L^-T, lower Phi -- so a tile's K range is the intersection of both)
    LbarT = ops.transpose(Lbar)
    if before_products is not None:
        before_products()
    n = LT.shape[0]
    chunks = TRI_PRODUCT_CHUNKS if (TRI_PRODUCT_CHUNKS > 1 and n >= TRI_PRODUCT_MIN_N and n % (16 * TRI_PRODUCT_CHUNKS) == 0) else 1
    if chunks == 1:
        T1 = ops.gemm_nt(LT, LbarT, b_tri=1, a_tri=1)                        # L^T L_bar
        Y = ops.gemm_nt(_phi_(T1), LinvT, b_tri=1, a_tri=2)                  # Phi L^-1        (lower)
        S = ops.gemm_nt(LinvT, ops.transpose(Y, mode=1), b_tri=1, a_tri=1)   # L^-T (Phi L^-1)
        return ops.symmetrize_(S)
    # Each of the three products is 256 output tiles whose K ranges differ by a factor of sixteen -- the launch lasts as long as the tile
    # that walks all of K (245 us at M = 2048 for 5.7 GFLOP).  As K chunks in the batch dimension of ONE launch (strided views; the
    # triangular hints refer to the unsplit column index, ops.gemm_nt k_split) the non-empty tiles fill the chip about once, and the sum of
    # the partial products is the pass that applied Phi / tril anyway.
    kc = n // chunks

    def split(X):
        return torch.as_strided(X, (chunks, X.shape[0], kc), (kc, X.stride(0), 1), X.storage_offset())

    T1 = ops.combine_parts(ops.gemm_nt(split(LT), split(LbarT), b_tri=1, a_tri=1, k_split=True), lower=True, diag_scale=0.5)   # Phi(L^T L_bar)
    Y = ops.combine_parts(ops.gemm_nt(split(T1), split(LinvT), b_tri=1, a_tri=2, k_split=True), lower=True)                   # Phi L^-1 (lower)
    S = ops.combine_parts(ops.gemm_nt(split(LinvT), split(ops.transpose(Y)), b_tri=1, a_tri=1, k_split=True))               # L^-T (Phi L^-1)
    return ops.symmetrize_(S)


_ls_cache: "collections.OrderedDict" = collections.OrderedDict()


def ls_device(lengthscales, D: int, device) -> torch.Tensor:
    """Lengthscales as a [D] device tensor.  A host array -> device copy from pageable memory BLOCKS the host until the stream
    has drained; in the tail of a reverse pass that serialised ~80 short launches behind an idle GPU (1 ms of a 6.5-ms training
    step, profiles/r04_train_timeline_before.txt).  The tensors are therefore made once per set of values -- the gradient entry
    points ask for them BEFORE they enqueue their first kernel -- and found here by the adjoints."""
    a = np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscales, dtype=np.float64), (D,)))
    key = (a.tobytes(), str(device))
    t = _ls_cache.get(key)
    if t is None:
        t = torch.as_tensor(a.copy(), device=device)
        _ls_cache[key] = t
        while len(_ls_cache) > 32:
            _ls_cache.popitem(last=False)
    return t


def stationary_kernel_adjoint(leaf: Leaf, A: torch.Tensor, Bm: torch.Tensor, Kbar: torch.Tensor, *, symmetric: bool, packed_into=None,
                              dvar_add: float = 0.0, return_packed: bool = False, moments=None):
    """Adjoint of K = variance * f(r(A / ls, Bm / ls)) [n1, n2] given Kbar [n1, n2], `leaf` of one of the stationary families
    (stationaries.py:209-210 SquaredExponential, :254-313 Matern12 / 32 / 52; Exponential; RationalQuadratic with its `alpha`; the
    static families have no distance and never come here: StaticMember.adjoint).

    Returns (d/dvariance, shape gradient, A_bar [n1, D]); the shape gradient is laid out like the leaf's `ls_host` for every family:
    d/dlengthscales as the leaf holds them ([1] isotropic, else [D]), then one entry per extra.  With symmetric=True (Bm is A, Kbar
    symmetric) A_bar collects both arguments.  B_bar of the non-symmetric case is not needed on this path (B = the minibatch).

    With r2 the scaled squared distance, dF/dtheta = sum_ij Kbar_ij dK_ij/dr2 dr2_ij/dtheta.  G = Kbar .* (-2 dK/dr2) is
    one elementwise pass that recomputes r2 from the inputs (`gpk_kernel_matrix_combine` op 3); for the
    SquaredExponential -2 dK/dr2 = K, so G also carries d/dvariance = sum(Kbar .* K) / variance; the Matern families
    take that sum from a second pass (op 1).  d/dvariance = sum(Kbar .* K) / variance holds for every family.  An extra `x` of
    the family (the RationalQuadratic's alpha) adds d/dx = sum(Kbar .* dK/dx) (op "d" + x: "dalpha", into the same buffer).

    moments: a callable that builds the right-hand side Vt of the contraction R = G Vt^T in place of ops.moment_rows(Bm); its first
    1 + 2 D rows must be those moment rows (an input-map kernel appends the rows its own tail needs: PeriodicMember.adjoint), and R
    is handed back as a fourth result."""
    n1, D = A.shape
    variance, lengthscales = leaf.variance, leaf.lengthscales
    ls = ls_device(lengthscales, D, A.device)
    dextras = []
    if leaf.family == "SquaredExponential":
        G = ops.kernel_matrix_hadamard(A, Bm, Kbar, variance=variance, lengthscales=lengthscales)   # Kbar .* K
        sum_kbar_k = None
    else:
        kw = leaf.keywords()
        G = ops.kernel_matrix_hadamard(A, Bm, Kbar, **kw)
        sum_kbar_k = G.sum()
        for name in leaf.row.extras:
            dextras.append(ops.kernel_matrix_combine(A, None if symmetric else Bm, Kbar, op="d" + name, out=G, **kw).sum().reshape(1))
        ops.kernel_matrix_combine(A, None if symmetric else Bm, Kbar, op="dr2", out=G, **kw)
    Vt = ops.moment_rows(Bm) if moments is None else moments()   # [1, B, B^2]^T
    R = splitk_gemm_nt(G, Vt)                        # [n1, 1 + 2D] = G [1, B, B^2]: row sums rs, G B, G B^2
    # one launch for what follows (it was a dozen elementwise / reduction launches on [n1, D] arrays):  T = G B - A rs;
    # both arguments (symmetric):  A_bar = 2 T / ls^2,  d/dls = (2 sum A^2 rs - 2 sum A GB) / ls^3 = -sum(A A_bar) / ls
    # else:  A_bar = T / ls^2,  d/dls = sum(GB2 - 2 A GB + A^2 rs) / ls^3 = sum(GB2 - A (GB + T)) / ls^3;  d/dvariance = sum(rs) / variance
    # (packed_into = (small [1 + D], A_bar) of an earlier adjoint of the SAME kernel: the results are added to it in the same launch;
    #  return_packed: (small, A_bar) instead of the three views)
    dvar, dls, Abar = ops.stationary_adjoint_tail(R if moments is None else R[:, :1 + 2 * D],   # (a view: ldr stays R's width)
                                                  A if A.is_contiguous() else A.contiguous(), ls, variance=variance, symmetric=symmetric,
                                                  sum_kbar_k=sum_kbar_k, into=packed_into, dvar_add=dvar_add)
    if return_packed:
        return (packed_into[0] if packed_into is not None else dls._base), Abar
    if moments is not None:
        return dvar, torch.cat([_ls_grad(dls, leaf), *dextras]), Abar, R
    return dvar, torch.cat([_ls_grad(dls, leaf), *dextras]), Abar


def _ls_grad(dl: torch.Tensor, leaf: Leaf) -> torch.Tensor:
    """d/dlengthscales as the leaf holds them: an isotropic one has ONE lengthscale, the sum of the per-column entries"""
    return dl.sum().reshape(1) if leaf.n_lengthscales == 1 else dl


def dot_kernel_adjoint(leaf: DotLeaf, A: torch.Tensor, Bm: torch.Tensor, Kbar: torch.Tensor, *, symmetric: bool):
    """Adjoint of a dot-product leaf K = k(s), s_ik = sum_j w_j a_ij b_kj (kernels/linears.py: Linear k = s, Polynomial k = (s + offset)^degree)
    given Kbar [n1, n2].  Returns (d/dvariance [1], or [D] for an ARD variance; shape gradient: [d/doffset] for the Polynomial, empty for
    Linear; A_bar [n1, D]); symmetric=True (Bm is A, Kbar symmetric): A_bar collects both arguments.

    G = Kbar .* dk/ds is one pass that recomputes s (`gpk_dot_kernel_matrix_combine` op 3; Linear: dk/ds = 1, G is Kbar itself and nothing
    is launched).  dF/dw_j = sum_i a_ij (G B)_ij, dF/da_ij = w_j (G B)_ij and dF/doffset = sum G all come from ONE contraction
    R = G [1, B] and the one-launch tail ops.dot_adjoint_tail.  The right-hand side is ops.moment_rows(Bm), its B^2 rows unused: one
    launch, where a narrower [1; B^T] is a fill, a transpose and a concatenation; the D extra columns of R cost a GEMM nothing
    measurable at D <= 64 (chosen by the number of launches; neither has been timed)."""
    D = A.shape[1]
    if leaf.ard and leaf.n_variance != D:
        raise ValueError(f"variance has {leaf.n_variance} entries, input dimension is {D}")
    G = Kbar if leaf.family == "Linear" else ops.dot_kernel_matrix_combine(A, None if symmetric else Bm, Kbar, op="ds", **leaf.keywords())
    R = splitk_gemm_nt(G if G.is_contiguous() else G.contiguous(), ops.moment_rows(Bm))   # [n1, 1 + 2 D]: row sums, G B, (G B^2 unused)
    dw, doff, Abar = ops.dot_adjoint_tail(R, A if A.is_contiguous() else A.contiguous(), ls_device(leaf.variance, leaf.n_variance, A.device),
                                          symmetric=symmetric)
    return dw, (doff if leaf.row.extras else doff[:0]), Abar


def arccos_kernel_adjoint(leaf: ArcLeaf, A: torch.Tensor, Bm: torch.Tensor, Kbar: torch.Tensor, *, symmetric: bool):
    """Adjoint of an ArcCosine leaf (kernels/misc.py) given Kbar [n1, n2].  Returns (d/dvariance [1]; shape gradient:
    d/dweight_variances [1 or D], then d/dbias_variance [1]; A_bar [n1, D]); symmetric=True (Bm is A, Kbar symmetric): A_bar collects
    both arguments and the diagonal of K(A, A) is the by-index one (include/gpk.h).

    K depends on the inputs and on (w, b) through s_ik, p_i and q_k.  ONE stage (ops.arccos_adjoint_stage) recomputes them per tile and
    leaves G = Kbar .* dk/ds and the per-tile partials of rho_i = sum_k Kbar_ik dk/dp_i, gamma_k = sum_i Kbar_ik dk/dq_k and
    sum Kbar .* k / variance; ONE contraction R = G [1, B] (the right-hand side is ops.moment_rows(Bm), as in dot_kernel_adjoint);
    ONE one-workgroup tail (ops.arccos_adjoint_tail) that adds the norm terms 2 w_j a_ij rho_i, sum_i rho_i a_ij^2, sum_k gamma_k b_kj^2."""
    D = A.shape[1]
    if leaf.ard and leaf.n_weights != D:
        raise ValueError(f"weight_variances has {leaf.n_weights} entries, input dimension is {D}")
    A = A if A.is_contiguous() else A.contiguous()
    Bm = A if symmetric else (Bm if Bm.is_contiguous() else Bm.contiguous())
    parts = ops.arccos_adjoint_parts(A.shape[0], Bm.shape[0], A.device)
    G = ops.arccos_adjoint_stage(A, None if symmetric else Bm, Kbar if Kbar.is_contiguous() else Kbar.contiguous(), parts, **leaf.keywords())
    R = splitk_gemm_nt(G, ops.moment_rows(Bm))   # [n1, 1 + 2 D]: row sums, G B, (G B^2 unused)
    dv, dw, db, Abar = ops.arccos_adjoint_tail(R, A, None if symmetric else Bm, parts, weight_variances=leaf.weight_variances)
    return dv, torch.cat([dw, db]), Abar


class Member:
    """One leaf of a KernelSpec as the tree walkers call it: its host values (`leaf`: a value of leaf.py that answers its protocol),
    the input columns it sees (`cols`: an index array, or None for all), a Periodic leaf's `period`, and every answer that depends on
    the KIND of leaf.  This base class holds what every kind shares: the builders (the leaf's `builders`, looked up on `ops` by name at
    the call), `n_variance`, `parameter_names`, `n_shape` and `split_shape` as the leaf answers them, `adjoint(A, Bm, Kbar, symmetric)`
    -> (d/dvariance [n_variance], shape gradient, A_bar over the member's columns, or None for no input gradient) through the kind's
    `leaf_adjoint` function; and what the kinds built by `gpk_kernel_matrix` share (stationary, static, periodic): K(x, x) = variance
    as one host value.  RowDiagonalMember holds what the kinds with a diagonal that depends on the row share.

    Where the next kind plugs in: one value type in leaf.py that answers the protocol, three thin `ops` wrappers (matrix, combine,
    row diagonal) over `ops._pair_builder` / `ops._row_diagonal`, one kernel class on kernels.base.RowDiagonalLeaf, and here one
    subclass of RowDiagonalMember with its `leaf_adjoint`, `diag_adjoint` and `warm`, entered in MEMBER_OF_LEAF."""
    constant_diagonal = True
    n_variance = property(lambda self: self.leaf.n_variance)
    matrix = property(lambda self: self.leaf.builders[0])     # the kind's builders, by their names in `ops`
    combine = property(lambda self: self.leaf.builders[1])

    def __init__(self, leaf, cols=None, period=None):
        self.leaf, self.cols, self.period, self._idx = leaf, cols, period, {}

    def index(self, device) -> torch.Tensor:
        """`cols` as a device tensor, made once per device"""
        key = str(device)
        if key not in self._idx:
            self._idx[key] = torch.as_tensor(self.cols, device=device)
        return self._idx[key]

    def columns(self, X):
        """the active columns as a contiguous copy (None stays None)"""
        if X is None or self.cols is None:
            return X
        return X.index_select(1, self.index(X.device)).contiguous()

    view = columns   # what the builders get

    def build(self, X1, X2, out, diag_add: float = 0.0):
        return getattr(ops, self.matrix)(self.view(X1), self.view(X2), diag_add=diag_add, lower_only=False, out=out, **self.leaf.keywords())

    def fold(self, X1, X2, G, op: str, diag_add: float = 0.0):
        """G <- G .* K(X1, X2) or G + K(X1, X2) in place (K recomputed in registers, no second matrix)"""
        return getattr(ops, self.combine)(self.view(X1), self.view(X2), G, op=op, diag_add=diag_add, out=G, **self.leaf.keywords())

    def kdiag(self) -> float:
        return self.leaf.variance

    def diag_adjoint(self, X, bar):
        """(d/dvariance, shape gradient) of sum_b bar_b K(x_b, x_b): a constant diagonal collects the sum of what reaches it"""
        return bar.sum().reshape(1), bar.new_zeros(self.n_shape())

    def adjoint(self, A, Bm, Kbar, symmetric):
        Ai = self.view(A)
        Bi = Ai if (symmetric and Bm is A) else self.view(Bm)   # (the identity decides whether a second copy is launched)
        dv, dl, Ab = self.leaf_adjoint(self.leaf, Ai, Bi, Kbar, symmetric=symmetric)
        return dv.reshape(-1), dl, Ab

    def warm(self, device, D: int) -> None:
        """device copies of what the adjoint's tails read, made now (see `ls_device`); D: the width of the full inputs"""

    def parameter_names(self) -> tuple:
        return self.leaf.parameters

    def n_shape(self) -> int:
        return self.leaf.n_shape

    def split_shape(self, g) -> dict:
        return self.leaf.split_shape(g)


class StationaryMember(Member):
    """a leaf with a distance (leaf.FAMILIES, has_distance)"""
    leaf_adjoint = staticmethod(stationary_kernel_adjoint)

    def warm(self, device, D: int) -> None:
        ls_device(self.leaf.lengthscales, D if self.cols is None else len(self.cols), device)


class StaticMember(Member):
    """White, Constant: no distance, so no lengthscale and no input gradient, and no contraction is launched"""

    def adjoint(self, A, Bm, Kbar, symmetric):
        # d/dvariance = sum(Kbar .* K) / variance read off directly: every entry (Constant), the diagonal of K(A, A) (White:
        # NOT through the X2-given hadamard, which is zeros for it), nothing where White sees two sets of points
        dv = Kbar.sum() if self.leaf.family == "Constant" else torch.diagonal(Kbar).sum() if symmetric else Kbar.new_zeros(())
        dl = Kbar.new_zeros(0)
        return dv.reshape(1), dl, None


class RowDiagonalMember(Member):
    """a leaf whose K(x, x) depends on the row (leaf.py: `constant_diagonal` False): `kdiag_rows` / `fold_kdiag` through the leaf's row
    diagonal builder take the place of the one host value, and `diag_adjoint` is the kind's own"""
    constant_diagonal = False

    def kdiag(self) -> float:
        raise NotImplementedError(f"K(x, x) of a {self.leaf.family} member depends on the row: this caller takes the diagonal for one "
                                  "scalar and has not been converted to KernelSpec.kdiag_rows")

    def kdiag_rows(self, X) -> torch.Tensor:
        """K(x_b, x_b) as a fresh [rows] tensor"""
        return getattr(ops, self.leaf.builders[2])(self.view(X), **self.leaf.keywords())

    def fold_kdiag(self, X, acc, op: str) -> None:
        """acc <- acc .* K(x_b, x_b) or acc + K(x_b, x_b) in place"""
        getattr(ops, self.leaf.builders[2])(self.view(X), acc, op=op, out=acc, **self.leaf.keywords())

    def rows(self, X):
        """the member's view of X, contiguous: what a `diag_adjoint` contracts with"""
        Xi = self.view(X)
        return Xi if Xi.is_contiguous() else Xi.contiguous()


def _moment_sums(g: torch.Tensor, Xi: torch.Tensor) -> torch.Tensor:
    """m [1 + 2 D] = (sum_b g_b, sum_b g_b x_bj, sum_b g_b x_bj^2) from ONE thin product of g [rows] with ops.moment_rows(Xi)"""
    return ops.gemm_nt(g.reshape(1, -1), ops.moment_rows(Xi))[0]


class DotMember(RowDiagonalMember):
    """a dot-product leaf (leaf.DotLeaf: Linear, Polynomial), built and folded by the `gpk_dot_*` entry points.  The variance gradient
    has D entries when the variance is ARD, the shape gradient is [d/doffset] or empty."""
    leaf_adjoint = staticmethod(dot_kernel_adjoint)

    def diag_adjoint(self, X, bar):
        """g = bar .* dkd/ds and, from `_moment_sums`, d/dw_j = sum_b g_b x_bj^2 and d/doffset = sum_b g_b"""
        leaf, Xi = self.leaf, self.rows(X)
        m = _moment_sums(bar if leaf.family == "Linear" else ops.dot_kernel_diag(Xi, bar, op="ds", **leaf.keywords()), Xi)
        dw = m[1 + Xi.shape[1]:]
        return (dw if leaf.ard else dw.sum().reshape(1)), (m[0:1] if leaf.row.extras else m[:0])

    def warm(self, device, D: int) -> None:
        ls_device(self.leaf.variance, self.leaf.n_variance, device)   # (the weights of the dot-product tail)


class ArcMember(RowDiagonalMember):
    """an ArcCosine leaf (leaf.ArcLeaf), built and folded by the `gpk_arccos_*` entry points: K(x, x) = variance jf p(x)^order.  One
    variance entry, the shape gradient is d/dweight_variances [1 or D], then d/dbias_variance."""
    leaf_adjoint = staticmethod(arccos_kernel_adjoint)

    def diag_adjoint(self, X, bar):
        """d/dvariance = sum_b bar_b kd_b / variance (the diagonal at variance 1); g = bar .* dkd/dp and, from `_moment_sums`,
        d/dw_j = sum_b g_b x_bj^2 and d/dbias = sum_b g_b"""
        leaf, Xi = self.leaf, self.rows(X)
        kw = leaf.keywords()
        dv = ops.arccos_kernel_diag(Xi, bar, op="mul", **dict(kw, variance=1.0)).sum().reshape(1)
        m = _moment_sums(ops.arccos_kernel_diag(Xi, bar, op="dp", **kw), Xi)
        dw = m[1 + Xi.shape[1]:]
        return dv, torch.cat([dw if leaf.ard else dw.sum().reshape(1), m[0:1]])


def coregion_kernel_adjoint(leaf: CoregionLeaf, A: torch.Tensor, Bm: torch.Tensor, Kbar: torch.Tensor, *, symmetric: bool):
    """Adjoint of a Coregion leaf K[i, k] = B[l_i, l'_k], B = W W^T + diag(kappa) (kernels/misc.py), given Kbar [n1, n2]; A [n1, 1] and
    Bm [n2, 1] are the label columns.  Returns (d/dkappa [P], d/dW [P R] flattened row-major, None: labels have no gradient).

    Bbar[a, b] = sum_{i: l_i = a} sum_{k: l'_k = b} Kbar[i, k] = (E1 Kbar E2^T)[a, b] with the one-hot rows E = ops.coregion_onehot_rows.
    Kbar is read ONCE, by the long contraction T = Kbar E2^T [n1, P] -- `splitk_gemm_nt(Kbar, E2)`, Kbar the GEMM's first operand as G
    is in the other adjoints; the second, thin contraction Bbar = E1 T = gemm_nt(E1, T^T) [P, P] takes T transposed (one small launch
    over n1 x P).  The other orientation, splitk_gemm_nt(E2, Kbar) [P, n1], needs no transpose and was measured 9 - 11 % slower at
    8192 x 8192 ("Coregion kernel").  Then the one-workgroup tail: d/dW = (Bbar + Bbar^T) W, d/dkappa = diag(Bbar).
    The same formulas serve K(A, A) with a symmetric Kbar: Bbar collects both arguments."""
    P = leaf.n_outputs
    A = A if A.is_contiguous() else A.contiguous()
    E1 = ops.coregion_onehot_rows(A, P)
    E2 = E1 if (symmetric or Bm is A) else ops.coregion_onehot_rows(Bm if Bm.is_contiguous() else Bm.contiguous(), P)
    T = splitk_gemm_nt(Kbar if Kbar.is_contiguous() else Kbar.contiguous(), E2)    # [n1, P]: the one pass over Kbar
    Bbar = ops.gemm_nt(E1, ops.transpose(T))                                       # [P, P]
    dk, dW = ops.coregion_adjoint_tail(Bbar, W=leaf.W)
    return dk, dW.reshape(-1), None


class CoregionMember(RowDiagonalMember):
    """a Coregion leaf (leaf.CoregionLeaf), built and folded by the `gpk_coregion_*` entry points over its ONE label column:
    K(x, x) = B[l, l].  The gradient slot the spec calls "variance" holds d/dkappa [P] (as the ARD variance of a DotMember has D
    entries); the shape gradient is d/dW [P R]; there is no input gradient."""
    leaf_adjoint = staticmethod(coregion_kernel_adjoint)

    def diag_adjoint(self, X, bar):
        """dbar_a = sum_{b: l_b = a} bar_b from ONE thin product of bar with the one-hot rows; kd = sum_r W[l, r]^2 + kappa[l], so
        d/dkappa = dbar and d/dW[a, :] = 2 dbar_a W[a, :]"""
        leaf, Xi = self.leaf, self.rows(X)
        dbar = ops.gemm_nt(bar.reshape(1, -1), ops.coregion_onehot_rows(Xi, leaf.n_outputs))[0]      # [P]
        Wd = ls_device(leaf.W.reshape(-1), leaf.n_shape, bar.device).reshape(leaf.n_outputs, leaf.rank)
        return dbar, (2.0 * dbar[:, None] * Wd).reshape(-1)

    def warm(self, device, D: int) -> None:
        ls_device(self.leaf.W.reshape(-1), self.leaf.n_shape, device)   # (the W of diag_adjoint)


class PeriodicMember(StationaryMember):
    """a Periodic leaf (kernels/periodic.py): a stationary member whose view of the inputs adds the warp Phi (ops.periodic_warp) after
    the column selection.  `leaf` is in the DEVICE form -- the base family over the 2 D_i warped columns with lengthscales 2 l, an ARD
    one repeated pairwise; `period` is 0-d or [D_i].  The gradients come back in the user's form: d/dl (one, or D_i), the extras, then
    d/dperiod last in the shape gradient, and an input gradient over the D_i columns."""

    def view(self, X):
        X = self.columns(X)
        return X if X is None else ops.periodic_warp(X if X.is_contiguous() else X.contiguous(), self.period)

    def base_lengthscales(self):
        """the lengthscales as the user holds them: the device form halved (exact), an ARD one un-paired"""
        ls = self.leaf.lengthscales
        return (ls if ls.ndim == 0 or ls.size == 1 else ls.reshape(-1)[0::2]) / 2.0

    def adjoint(self, A, Bm, Kbar, symmetric):
        """the stationary adjoint of the device-form leaf at the warped inputs -- with the extra moment rows of the period gradient
        riding in its one contraction -- then ops.periodic_adjoint_tail"""
        leaf, per = self.leaf, self.period
        Ai = self.columns(A)
        Bi = Ai if (symmetric and Bm is A) else self.columns(Bm)
        same = Bi is Ai
        Ai = Ai if Ai.is_contiguous() else Ai.contiguous()
        Bi = Ai if same else (Bi if Bi.is_contiguous() else Bi.contiguous())
        PA = ops.periodic_warp(Ai, per)
        PB = PA if Bi is Ai else ops.periodic_warp(Bi, per)
        dv, dl, Pbar, R = stationary_kernel_adjoint(leaf, PA, PB, Kbar, symmetric=symmetric,
                                                    moments=lambda: ops.periodic_moment_rows(Bi, per))
        nls = leaf.n_lengthscales   # entries of dl in front of the extras: d/dl = 2 d/d(2 l), the two columns of a pair added
        g_ls = 2.0 * dl[:1] if nls == 1 else 2.0 * (dl[0:nls:2] + dl[1:nls:2])
        dper, Ab = ops.periodic_adjoint_tail(Ai, PA, Pbar, R, ls_device(self.base_lengthscales(), Ai.shape[1], Ai.device), per)
        dl = torch.cat([g_ls, dl[nls:], dper])
        return dv.reshape(-1), dl, Ab

    def warm(self, device, D: int) -> None:
        Di = D if self.cols is None else len(self.cols)   # (the periodic tail at the base's width, the stationary tail at the warped one)
        ls_device(self.base_lengthscales(), Di, device)
        ls_device(self.leaf.lengthscales, 2 * Di, device)

    def parameter_names(self) -> tuple:
        return self.leaf.parameters + ("period",)

    def n_shape(self) -> int:
        return max(self.leaf.n_lengthscales // 2, 1) + len(self.leaf.extras) + int(self.period.size)

    def split_shape(self, g) -> dict:
        """the user's form: the lengthscale entries are what precedes the extras and the trailing period entries"""
        nper, nex = int(self.period.size), len(self.leaf.extras)
        nls = g.shape[0] - nper - nex
        return {"lengthscales": g[:nls], **{name: g[nls + j:nls + j + 1] for j, name in enumerate(self.leaf.row.extras)}, "period": g[nls + nex:]}


# leaf type -> member class: the one place where the four kinds of leaf are listed (a Leaf: StaticMember / PeriodicMember are chosen
# by its values, in the constructor of KernelSpec)
MEMBER_OF_LEAF = {Leaf: StationaryMember, DotLeaf: DotMember, ArcLeaf: ArcMember, CoregionLeaf: CoregionMember}


class ChangePointsNode:
    """The host values of one ChangePoints node of a KernelSpec tree (kernels/changepoints.py): `locations` [C] SORTED (a stable
    argsort of the given ones, `permutation`: sorted[j] = given[permutation[j]]), `steepness` [C] paired with the sorted locations as
    the reference pairs them (`scalar_steepness`: one value stands for all C), and `switch_dim`, a column of the UNSLICED inputs."""

    def __init__(self, locations, steepness, switch_dim: int = 0):
        loc = np.asarray(locations, dtype=np.float64).reshape(-1)
        st = np.asarray(steepness, dtype=np.float64)
        self.scalar_steepness = st.ndim == 0
        if not self.scalar_steepness and st.reshape(-1).size != loc.size:
            raise ValueError(f"ChangePoints: {st.reshape(-1).size} steepness entries for {loc.size} locations")
        if int(switch_dim) < 0:
            raise ValueError("ChangePoints: switch_dim must not be negative")
        if loc.size + 1 > ops.CP_MAX_MEMBERS:
            raise NotImplementedError(f"ChangePoints: more than {ops.CP_MAX_MEMBERS} member kernels")
        self.permutation = np.argsort(loc, kind="stable")
        self.locations = loc[self.permutation]
        self.steepness = np.broadcast_to(st.reshape(-1) if not self.scalar_steepness else st, (loc.size,)).copy()
        self.switch_dim = int(switch_dim)

    @property
    def n_members(self) -> int:
        return self.locations.size + 1


class KernelSpec:
    """What the reverse pass needs to know about the covariance function: ONE kernel leaf, or a Sum / Product of leaves -- flat, or
    nested (a Product of Sums, ...: `op` a tree, see __init__) -- over the same or different input columns (gpflow/kernels/base.py:216-220
    `Sum`, :305-315 `Product`; the reference differentiates `tf.add_n` / `tf.multiply` of the member matrices with autodiff).
    members: leaves (the value types of leaf.py), given as such or as tuples (family, variance, lengthscales[, alpha]); op: None | "add" |
    "mul" | tree.

    The constructor chooses ONE member object per leaf (`parts`) from the one mapping MEMBER_OF_LEAF, leaf type -> member class (a Leaf
    with a period: a PeriodicMember; a static one: a StaticMember), the only place where the kind of a leaf is asked.  The next kind
    plugs in there: one leaf type that answers the protocol of leaf.py, three thin `ops` wrappers, one kernel class on
    kernels.base.RowDiagonalLeaf, one member class with its `diag_adjoint` and `leaf_adjoint`.  Everything else here is about the TREE: `_build`, `_constant`, `_kd`, `_kd_rows`,
    `_diag_adjoint`, `_dkd` and `_adjoint` are the only walkers, and at a leaf each is one call on the member object.

    A third kind of node, ("cp", [children], k), is a ChangePoints combination (kernels/changepoints.py): K = sum_i (a_i b_i^T) .* K_i
    with weights from the node's own values `nodes[k]` (a ChangePointsNode).  Every walker dispatches on it first (`_build_cp`,
    `_adjoint_cp`, the "cp" branches of `_kd_rows` and `_diag_adjoint`; `_constant` is False, `_kd` and `_dkd` raise).  Its gradients
    (d/dlocations, d/dsteepness) do not fit the per-member lists: `adjoint` / `diag_adjoint` add them up on the spec from `warm()` on,
    and `kernel_grads` hands them out under "changepoints" and empties the sums.  A spec without such a node issues the calls it issued.

    A member's SHAPE gradient -- the `dl` entry of `adjoint` -- is laid out like the leaf's `ls_host`: the lengthscale entries, then the
    extras (a periodic member: then the period); a static member's is empty.  A spec with a dot-product member has no
    `constant_diagonal`: `kdiag()` / `dkdiag()` raise, `kdiag_rows(X)` and `diag_adjoint(X, kd_bar)` take their place.

      build    the combined matrix, members folded in place by the builders' combine pass (no second matrix);
      kdiag    K(x, x): sum or product of the members' host values, dkdiag[i] = d kdiag / d variance_i;
      adjoint  member i sees  Kbar (Sum)  or  Kbar .* prod_{j != i} k_j  (Product: formed by the same in-place combine pass);
               the input gradients of the members are scattered back into the columns each read, and add up."""

    def __init__(self, members, op=None, cols=None, periods=None, nodes=None):
        """members: leaves or tuples, see the class; cols[i]: the input columns member i sees (its `active_dims` as an index
        list, kernels/base.py:90-109) or None for all of them; periods[i]: None, or the period (0-d or [D_i]) of a Periodic member,
        whose leaf is then in the device form (PeriodicMember); nodes[k]: the values of the tree's ChangePoints node
        ("cp", [children], k) -- a ChangePointsNode, the one kind of node with parameters of its own."""
        self.nodes = list(nodes or [])
        self._node_grads = None
        self.members = [m if isinstance(m, tuple(MEMBER_OF_LEAF)) else Leaf(*m[:3], alpha=m[3] if len(m) > 3 else None) for m in members]
        # op: "add" | "mul" for a flat combination of all members, or a TREE for nested ones (a Product of Sums, ...):
        # (op, [children]) with a child either a member index or another such pair -- e.g. ("mul", [("add", [0, 1]), 2]) is
        # (k0 + k1) * k2 (kernels/base.py:223-329: a Combination holds kernels, which may be Combinations of the other kind).
        # Kept as ONE tree: the leaf 0 for one member (whatever combination is wrapped round it), (op, [0 .. n-1]) for a flat one.
        n = len(self.members)
        if op in ("add", "mul"):
            op = (op, list(range(n)))
        elif (n > 1 or nodes) and not isinstance(op, (tuple, list)):
            raise ValueError("a kernel combination needs op 'add' or 'mul'")
        self.tree = 0 if n == 1 and not self.nodes else self._check_tree(op, n)
        for nd in self._cp_nodes(self.tree):
            if nd[2] >= len(self.nodes) or len(nd[1]) != self.nodes[nd[2]].n_members:
                raise ValueError("a ChangePoints node has one child per regime: len(locations) + 1")
        cols = [None] * len(self.members) if cols is None else list(cols)
        if len(cols) != len(self.members):
            raise ValueError("one column selection per member")
        self.cols = [None if c is None else np.asarray(c, dtype=np.int64).reshape(-1) for c in cols]
        periods = [None] * len(self.members) if periods is None else list(periods)
        if len(periods) != len(self.members):
            raise ValueError("one period (or None) per member")
        self.periods = [None if p is None else np.asarray(p, dtype=np.float64) for p in periods]
        for leaf, p in zip(self.members, self.periods):
            if p is not None and (not isinstance(leaf, Leaf) or leaf.is_static or p.ndim > 1 or (leaf.n_lengthscales > 1 and leaf.n_lengthscales % 2)):
                raise ValueError("a periodic member is a leaf with a distance over the warped columns, its period 0-d or [D]")
        self.parts = [PeriodicMember(leaf, c, p) if p is not None else StaticMember(leaf, c) if isinstance(leaf, Leaf) and leaf.is_static
                      else MEMBER_OF_LEAF[type(leaf)](leaf, c) for leaf, c, p in zip(self.members, self.cols, self.periods)]

    @staticmethod
    def single(variance, lengthscales, family="SquaredExponential", alpha=None):
        return KernelSpec([Leaf(family, variance, lengthscales, alpha=alpha)], None)

    @property
    def packable(self) -> bool:
        """one member whose two adjoints fit the packed tail of `_covariance_tail` ([variance, lengthscales] and A_bar in one launch)"""
        return self.n == 1 and not self.nodes and self.cols[0] is None and self.periods[0] is None and self.members[0].is_plain

    @staticmethod
    def _check_tree(node, n):
        seen = []

        def walk(nd):
            if isinstance(nd, (int, np.integer)):
                seen.append(int(nd))
                return int(nd)
            if len(nd) == 3 and nd[0] == "cp":     # ("cp", [children], node index): one child per regime
                _, ch, k = nd
                if not isinstance(k, (int, np.integer)) or k in seen_nodes or len(ch) < 1:
                    raise ValueError("a ChangePoints node is ('cp', [children], index of its values in `nodes`)")
                seen_nodes.append(int(k))
                return ("cp", [walk(c) for c in ch], int(k))
            op, ch = nd
            if op not in ("add", "mul") or len(ch) < 1:
                raise ValueError("a combination node is ('add' | 'mul', [children])")
            return (op, [walk(c) for c in ch])
        seen_nodes = []
        out = walk(node)
        if sorted(seen) != list(range(n)):
            raise ValueError("every member must appear exactly once in the combination tree")
        if sorted(seen_nodes) != list(range(len(seen_nodes))):
            raise ValueError("the ChangePoints nodes of the tree are numbered 0 .. in `nodes`")
        return out

    @property
    def n(self) -> int:
        return len(self.members)

    def is_dot(self, i: int) -> bool:
        """member i is a dot-product leaf (leaf.DotLeaf: Linear, Polynomial): its own builders, and a diagonal that depends on the row"""
        return isinstance(self.members[i], DotLeaf)

    def n_variance(self, i: int) -> int:
        """entries of member i's variance gradient: 1, or D for the ARD variance of a dot-product member"""
        return self.parts[i].n_variance

    def build(self, X1, X2, out=None, diag_add: float = 0.0):
        return self._build(self.tree, X1, X2, out, diag_add)

    def _build(self, node, X1, X2, out, diag_add=0.0):
        if isinstance(node, int):
            return self.parts[node].build(X1, X2, out, diag_add)
        if node[0] == "cp":
            return self._build_cp(node, X1, X2, out, diag_add)
        op, ch = node
        if len(ch) == 1:
            return self._build(ch[0], X1, X2, out, diag_add)
        last = len(ch) - 1
        out = self._build(ch[0], X1, X2, out)
        for j, c in enumerate(ch[1:], start=1):
            if isinstance(c, int):      # a leaf folds in place; diag_add rides in the LAST member's launch
                self.parts[c].fold(X1, X2, out, op, diag_add=diag_add if j == last else 0.0)
            else:                        # a sub-combination needs its own matrix once
                tmp = self._build(c, X1, X2, None)
                out.add_(tmp) if op == "add" else out.mul_(tmp)
        if X2 is None and diag_add != 0.0 and not isinstance(ch[last], int):    # (X2 given: ignored, as every leaf launch ignores it)
            out.diagonal().add_(float(diag_add))
        return out

    @classmethod
    def _cp_nodes(cls, node):
        """the ChangePoints nodes under `node`, in traversal order"""
        if isinstance(node, int):
            return []
        return ([node] if node[0] == "cp" else []) + [nd for c in node[1] for nd in cls._cp_nodes(c)]

    def _cp_weights(self, k: int, X):
        """A [T, rows] of node k over the switch column of the UNSLICED inputs"""
        nd = self.nodes[k]
        if nd.switch_dim >= X.shape[1]:
            raise ValueError(f"ChangePoints: switch_dim {nd.switch_dim} is outside the {X.shape[1]} input columns")
        return ops.changepoint_weights(X[:, nd.switch_dim], locations=nd.locations, steepness=nd.steepness)

    def _build_cp(self, node, X1, X2, out, diag_add=0.0):
        """the first child is built into `out` and weighted in place (op 0); every further child is built once into ONE reused
        temporary and folded in (op 1: one read of each, one write of `out`); diag_add rides in the LAST fold"""
        _, ch, k = node
        A = self._cp_weights(k, X1)
        B = None if X2 is None else self._cp_weights(k, X2)
        last = len(ch) - 1
        out = self._build(ch[0], X1, X2, out)
        ops.changepoint_fold(A[0], None if B is None else B[0], out, diag_add=diag_add if last == 0 else 0.0, out=out)
        tmp = None
        for j, c in enumerate(ch[1:], start=1):
            tmp = self._build(c, X1, X2, tmp)
            ops.changepoint_fold(A[j], None if B is None else B[j], tmp, out, diag_add=diag_add if j == last else 0.0, out=out)
        return out

    def _constant(self, node) -> bool:
        """every member under `node` has a constant diagonal: the node's diagonal is one host value (never under a ChangePoints node:
        its weights depend on the row)"""
        if isinstance(node, int):
            return self.parts[node].constant_diagonal
        return node[0] != "cp" and all(self._constant(c) for c in node[1])

    @property
    def constant_diagonal(self) -> bool:
        """K(x, x) is one host scalar, `kdiag()`: every member stationary, periodic or static.  A dot-product member makes it a function
        of the row: `kdiag_rows(X)` and `diag_adjoint`."""
        return self._constant(self.tree)

    def _kd(self, node) -> float:
        if isinstance(node, int):
            return self.parts[node].kdiag()
        if node[0] == "cp":
            raise NotImplementedError("K(x, x) of a ChangePoints node depends on the row: this caller takes the diagonal for one scalar "
                                      "and has not been converted to KernelSpec.kdiag_rows")
        vals = [self._kd(c) for c in node[1]]
        return float(np.prod(vals)) if node[0] == "mul" else float(np.sum(vals))

    def kdiag(self) -> float:
        return self._kd(self.tree)

    def _kd_rows(self, node, X):
        """K(x, x) under `node`: a host float (a constant subtree) or a fresh [rows] tensor"""
        if self._constant(node):
            return self._kd(node)
        if isinstance(node, int):
            return self.parts[node].kdiag_rows(X)
        if node[0] == "cp":     # sum_i a_i^2 kd_i, the weight formed first as the fold forms it: the diagonal of the built matrix
            A, acc = self._cp_weights(node[2], X), None
            for i, c in enumerate(node[1]):
                term = (A[i] * A[i]) * self._kd_rows(c, X)
                acc = term if acc is None else acc + term
            return acc
        op, ch = node
        rows = [c for c in ch if not self._constant(c)]
        acc = self._kd_rows(rows[0], X)
        for c in rows[1:]:
            if isinstance(c, int):      # a leaf folds in place, as in `_build`
                self.parts[c].fold_kdiag(X, acc, op)
            else:
                sub = self._kd_rows(c, X)
                acc.add_(sub) if op == "add" else acc.mul_(sub)
        const = [self._kd(c) for c in ch if self._constant(c)]
        if const:                       # the constant members enter as one scalar
            acc.add_(float(np.sum(const))) if op == "add" else acc.mul_(float(np.prod(const)))
        return acc

    def kdiag_rows(self, X) -> torch.Tensor:
        """K(x_b, x_b) for the rows of X [B, D] as a [B] device tensor: leaves through ops.dot_kernel_diag, combinations folded by its
        ops "mul" / "add" and by scalars for the members with a constant diagonal"""
        kd = self._kd_rows(self.tree, X)
        return kd if torch.is_tensor(kd) else torch.full((X.shape[0],), float(kd), dtype=torch.float64, device=X.device)

    def diag_adjoint(self, X, kd_bar):
        """([d/dvariance_i], [shape gradient_i]) of sum_b kd_bar_b K(x_b, x_b), members in index order, laid out as `adjoint` lays
        them out (Member.diag_adjoint, DotMember.diag_adjoint).  For a Product the other children's diagonals enter as in `_adjoint`."""
        acc = {"dv": [None] * self.n, "dl": [None] * self.n}
        self._diag_adjoint(self.tree, X, kd_bar if kd_bar.is_contiguous() else kd_bar.contiguous(), acc)
        return acc["dv"], acc["dl"]

    def _diag_adjoint(self, node, X, bar, acc):
        if isinstance(node, int):
            acc["dv"][node], acc["dl"][node] = self.parts[node].diag_adjoint(X, bar)
            return
        if node[0] == "cp":     # child i sees bar .* a_i^2; the weights see 2 a_i kd_i bar, and one tail turns them into the node's gradients
            _, ch, k = node
            A = self._cp_weights(k, X)
            init = torch.empty_like(A)
            for i, c in enumerate(ch):
                init[i] = (2.0 * A[i]) * self._kd_rows(c, X) * bar
                self._diag_adjoint(c, X, bar * (A[i] * A[i]), acc)
            nd = self.nodes[k]
            dl, ds, _ = ops.changepoint_adjoint_tail(X[:, nd.switch_dim], locations=nd.locations, steepness=nd.steepness, init=init)
            self._add_node_grads(k, dl, ds)
            return
        op, ch = node
        for jc, c in enumerate(ch):
            b = bar
            if op == "mul":
                b = bar.clone()
                for jo, o in enumerate(ch):
                    if jo != jc:
                        b.mul_(self._kd_rows(o, X))
            self._diag_adjoint(c, X, b, acc)

    def _dkd(self, node) -> dict:
        if isinstance(node, int):
            return {node: 1.0}
        if node[0] == "cp":
            raise NotImplementedError("K(x, x) of a ChangePoints node depends on the row: KernelSpec.diag_adjoint takes the place of dkdiag")
        op, ch = node
        kd = self._kd(node)
        out = {}
        for c in ch:
            fac = kd / self._kd(c) if op == "mul" else 1.0
            for i, d in self._dkd(c).items():
                out[i] = fac * d
        return out

    def dkdiag(self):
        d = self._dkd(self.tree)
        return [d[i] for i in range(self.n)]

    def warm(self, device, D: int) -> "KernelSpec":
        """device copies of the members' lengthscales, made now (see `ls_device`)"""
        for m in self.parts:
            m.warm(device, D)
        self._node_grads = None     # a gradient evaluation begins: what `adjoint` / `diag_adjoint` add up for the nodes starts empty
        return self

    def _add_node_grads(self, k: int, dl, ds) -> None:
        """d/dlocations (sorted order) and d/dsteepness (per change point) of node k from one tail, added to what this evaluation has"""
        if self._node_grads is None:
            self._node_grads = [None] * len(self.nodes)
        have = self._node_grads[k]
        self._node_grads[k] = (dl, ds) if have is None else (have[0] + dl, have[1] + ds)

    def adjoint(self, A, Bm, Kbar, symmetric: bool):
        """([d/dvariance_i [1]], [shape gradient_i: d/dlengthscales_i, then d/dalpha_i], A_bar [n1, D]) given Kbar, members in index
        order"""
        acc = {"dv": [None] * self.n, "dl": [None] * self.n, "Abar": None}
        self._adjoint(self.tree, A, Bm, Kbar, symmetric, acc)
        return acc["dv"], acc["dl"], (acc["Abar"] if acc["Abar"] is not None else torch.zeros_like(A))   # (static members only: zero)

    @staticmethod
    def _abar(acc, A):
        """acc["Abar"] to add into in place: begun as zeros like A where no input gradient has reached it yet"""
        if acc["Abar"] is None:
            acc["Abar"] = torch.zeros_like(A)
        return acc["Abar"]

    def _adjoint(self, node, A, Bm, Kbar, symmetric, acc):
        if isinstance(node, int):
            m = self.parts[node]
            acc["dv"][node], acc["dl"][node], Ab = m.adjoint(A, Bm, Kbar, symmetric)   # (dv [1]; an ARD dot-product member: [D])
            if Ab is None:          # no input gradient
                return
            if all(c is None for c in self.cols):
                acc["Abar"] = Ab if acc["Abar"] is None else acc["Abar"] + Ab
            elif m.cols is None:
                self._abar(acc, A).add_(Ab)
            else:   # scatter the member's input gradient back into the columns it read
                self._abar(acc, A).index_add_(1, m.index(A.device), Ab)
            return
        if node[0] == "cp":
            return self._adjoint_cp(node, A, Bm, Kbar, symmetric, acc)
        op, ch = node
        for jc, c in enumerate(ch):
            Kb = Kbar
            if op == "mul":          # d/dK_c = Kbar .* prod of the OTHER children's matrices
                Kb = Kbar.clone()
                for jo, o in enumerate(ch):
                    if jo == jc:
                        continue
                    if isinstance(o, int):
                        self.parts[o].fold(A, None if symmetric else Bm, Kb, "mul")
                    else:
                        Kb.mul_(self._build(o, A, None if symmetric else Bm, None))
            self._adjoint(c, A, Bm, Kb, symmetric, acc)

    def _adjoint_cp(self, node, A, Bm, Kbar, symmetric, acc):
        """K = sum_i (a_i b_i^T) .* K_i.  Per child: K_i built into ONE reused temporary, ONE stage call that overwrites it with the
        child's seed G = Kbar .* (a_i b_i^T) and leaves the tile partials of the weight adjoints, the child's own adjoint with G.  After
        the last child one tail per argument: the node's d/dlocations, d/dsteepness, and the gradient of the switch column, which is
        added into A_bar (symmetric: both arguments)."""
        _, ch, k = node
        nd = self.nodes[k]
        B2 = None if symmetric else Bm
        Kbar = Kbar if Kbar.is_contiguous() else Kbar.contiguous()
        W1 = self._cp_weights(k, A)
        W2 = None if symmetric else self._cp_weights(k, Bm)
        n1, n2 = Kbar.shape
        parts = ops.changepoint_adjoint_parts(len(ch), n1, n2, A.device)
        tmp = None
        for i, c in enumerate(ch):
            tmp = self._build(c, A, B2, tmp)
            G = ops.changepoint_adjoint_stage(W1[i], None if symmetric else W2[i], Kbar, tmp, parts[i], out=tmp)
            self._adjoint(c, A, Bm, G, symmetric, acc)
        kw = dict(locations=nd.locations, steepness=nd.steepness, parts=parts)
        dl, ds, xbar = ops.changepoint_adjoint_tail(A[:, nd.switch_dim], n_other=n2, columns=False, **kw)
        dl2, ds2, xbar2 = ops.changepoint_adjoint_tail((A if symmetric else Bm)[:, nd.switch_dim], n_other=n1, columns=True, **kw)
        self._add_node_grads(k, dl + dl2, ds + ds2)
        self._abar(acc, A)[:, nd.switch_dim] += (xbar + xbar2) if symmetric else xbar

    def pack(self, dvs, dls):
        """gradient entries: one member -> ("variance" [1], "lengthscales" [D or 1]) as before; several -> "variance" [n] and
        "lengthscales" a list of per-member tensors"""
        if self.n == 1:
            return dvs[0], dls[0]
        return torch.cat(dvs), list(dls)

    def parameter_names(self, i: int) -> tuple:
        """names of member i's hyperparameters in the order of its gradients: the leaf's, then a periodic member's "period" """
        return self.parts[i].parameter_names()

    def n_shape(self, i: int) -> int:
        """entries of member i's shape gradient: Leaf.n_shape, and for a periodic member the user's lengthscales, the extras, the period"""
        return self.parts[i].n_shape()

    def split_shape(self, i: int, g) -> dict:
        """member i's shape gradient as {"lengthscales": ..., <extra>: [1], ..., "period": ...}"""
        return self.parts[i].split_shape(g)

    def kernel_grads(self, g_var, g_shape) -> dict:
        """the kernel's entries of a `grads` dict from what `pack` returned: "variance", "lengthscales" (a static member's is empty)
        and -- only when a member has one -- "alpha" and "period": one tensor for one member, else a list with None for the members
        without"""
        if self.n == 1:
            return {"variance": g_var, **self.split_shape(0, g_shape), **self._changepoint_grads()}
        split = [self.split_shape(i, g) for i, g in enumerate(g_shape)]
        return {"variance": g_var, **{name: [p.get(name) for p in split] for name in dict.fromkeys(k for p in split for k in p)},
                **self._changepoint_grads()}

    def _changepoint_grads(self) -> dict:
        """{"changepoints": [{"locations": [C], "steepness": [C or 1]}, ...]}, one entry per ChangePoints node in node order -- the
        locations' gradient back in the GIVEN order (through the sort's permutation), a scalar steepness collecting the sum; what the
        `adjoint` / `diag_adjoint` calls since `warm` added up.  No node: no key."""
        if not self.nodes:
            return {}
        out = []
        for k, nd in enumerate(self.nodes):
            have = None if self._node_grads is None else self._node_grads[k]
            C = nd.locations.size
            dl = have[0] if have is not None else torch.zeros(C, dtype=torch.float64)
            ds = have[1] if have is not None else torch.zeros(C, dtype=torch.float64)
            given = torch.zeros_like(dl)
            if C:
                given[torch.as_tensor(nd.permutation, device=dl.device)] = dl
            out.append({"locations": given, "steepness": ds.sum().reshape(1) if nd.scalar_steepness else ds})
        self._node_grads = None
        return {"changepoints": out}


class _Seed:
    """The seeds of the data term  scale * sum_bp var_exp(fmean_bp, fvar_bp):  r = dF/dfmean [B, P]  and  c = dF/dfvar  in the form
    the likelihood gives it:
      a scalar          Gaussian, one noise variance:  c = -scale / (2 s2)  for every (b, p);
      a vector [B]      Gaussian, one noise variance per row (heteroskedastic, round 5): a row scaling of the factors the scalar
                        multiplied (elementwise glue on [B, M] arrays);
      a matrix [B, P]   a quadrature likelihood (Bernoulli, Poisson, StudentT; `lik_grads` = the kernel's dmu, dvar): the per-row form
                        with W_p scaled by its own column, and sum_p c_bp where that form has P c_b;
      given (r, c)      a later stage mixes the latents (LinearCoregionalization): r [B, P] and the scalar c arrive ready-made, already
                        carrying `scale` -- the scalar form with nothing derived from Yb.
    The methods are the places where c enters the two SVGP passes; each issues the calls of the form it holds, so the passes read as
    their derivation and the scalar path costs what it cost."""

    def __init__(self, Yb, fmean, *, scale, mean_const, noise_variance=None, lik_grads=None, given=None):
        self.B, self.P = fmean.shape
        self.scale, self.nv = scale, noise_variance
        self.Yb, self.fmean, self.mean_const = Yb, fmean, mean_const
        if given is not None:
            self.r, self.c = given[0], float(given[1])
        elif lik_grads is not None:
            self.r = lik_grads[0].mul_(scale)                                           # dF/dfmean [B, P]
            self.c = lik_grads[1].mul_(scale)                                           # dF/dfvar  [B, P]
        elif torch.is_tensor(noise_variance) and noise_variance.dim() >= 1:
            self.nv = nv = noise_variance.reshape(-1)
            self.c = (-0.5 * scale) / nv                                                # dF/dfvar per row [B]
            self.r = (scale / nv)[:, None] * (Yb - fmean - mean_const)                  # dF/dfmean [B, P]
        else:
            self.c = -0.5 * scale / noise_variance                                      # dF/dfvar (every b, p)
            self.r = torch.sub(Yb, fmean)                                               # dF/dfmean [B, P] = (scale / s2) (y - f - m)
            if mean_const != 0.0:
                self.r.sub_(mean_const)
            self.r.mul_(scale / noise_variance)
        self.dim = self.c.dim() if torch.is_tensor(self.c) else 0

    @property
    def scalar(self) -> bool:
        return self.dim == 0

    def add_W_LqT(self, Atb, W, Lq):
        """Atb += 2 sum_p c W_p Lq_p^T  (Lq_p lower: b_tri 2).  Returns (Wg, ag): the (row-scaled) W and the factor with which the
        q_sqrt products  ag tril(At^T Wg_p)  carry the same c."""
        if self.dim == 0:
            Wg, ag = W, 2.0 * self.c
        else:                                                                           # rows of W_p scaled by c_b / c_bp
            Wg, ag = W * (self.c[None, :, None] if self.dim == 1 else self.c.t()[:, :, None]), 2.0
        for p in range(self.P):
            ops.gemm_nt(Wg[p], Lq[p], alpha=ag, beta=1.0, C=Atb, b_tri=2)
        return Wg, ag

    def add_At(self, Atb, At):
        """Atb += -2 (sum_p c) At"""
        if self.dim == 0:
            Atb.add_(At, alpha=-2.0 * self.c * self.P)
        elif self.dim == 1:
            Atb.addcmul_(At, self.c[:, None], value=-2.0 * self.P)
        else:
            Atb.addcmul_(At, self.c.sum(1)[:, None], value=-2.0)

    def add_qdiag_term(self, Atb, At, q_sqrt, s=None):
        """q_diag, per column m:  Atb += 2 At .* (c (q^2 - 1)^T) = 2c At (sum_p q_mp^2 - P)  -- the W and the At term of the full form
        in one; with s = sum_p q_mp^2 given (the un-whitened pass, whose At term is separate) the weight is s itself."""
        if self.dim == 2:
            Atb.addcmul_(At, ops.gemm_nt(self.c, q_sqrt * q_sqrt - 1.0), value=2.0)
            return
        w = lambda: (((q_sqrt * q_sqrt).sum(1) - self.P) if s is None else s)[None, :]  # noqa: E731
        if self.dim == 1:
            Atb.addcmul_(At * (2.0 * self.c)[:, None], w())
        else:
            Atb.addcmul_(At, (2.0 * self.c) * w())

    def weighted_colsq(self, A, At):
        """q_diag:  2 sum_b c At[b, m]^2  as [M, 1] or, per latent, [M, P]  (A = At^T)"""
        if self.dim == 2:
            return ops.gemm_nt(A * A, self.c.t().contiguous(), alpha=2.0)
        if self.dim == 1:
            return (2.0 * ((At * At) * self.c[:, None]).sum(0))[:, None]
        return (2.0 * self.c) * ops.row_stats(A)[0][:, None]

    def csum(self):
        """sum_bp c: what every fvar's Knn = kdiag collects"""
        return self.c.sum() if self.dim == 2 else self.c.sum() * self.P if self.dim == 1 else self.c * self.B * self.P

    def crows(self):
        """sum_p c_bp per row [B]: what the Knn = K(x_b, x_b) of row b's fvar collects when the diagonal depends on the row"""
        if self.dim == 2:
            return self.c.sum(1)
        if self.dim == 1:
            return self.c * self.P
        return torch.full((self.B,), float(self.c) * self.P, dtype=self.fmean.dtype, device=self.fmean.device)

    def kdiag_bar(self, spec: "KernelSpec"):
        """the `knn_bar` of _covariance_tail: the scalar `csum` for a spec with a constant diagonal, else the rows `crows`"""
        return self.csum() if spec.constant_diagonal else self.crows()

    def noise_grad(self, ve, s0, ssq, kdiag):
        """dF/d sigma^2 of the Gaussian likelihood: [1], or one entry per row (likelihood parameters are then reached through
        Gaussian.noise_param_grads).  kdiag: the host scalar, or the rows [B] of a diagonal that depends on the row."""
        B, P, scale, nv = self.B, self.P, self.scale, self.nv
        if self.dim == 1:
            # dF/d sigma_n^2 = scale sum_p (-1 / (2 s2_n) + ((y - f)^2 + fvar) / (2 s2_n^2))
            fvar = (kdiag - s0)[:, None] + ssq.t()
            resid = self.Yb - self.fmean - self.mean_const
            return scale * (-0.5 * P / nv + 0.5 * (resid * resid + fvar).sum(1) / (nv * nv))
        # sum_bp ((y - f)^2 + fvar) recovered from the forward value:  ve = B P k0 - Q / (2 s2)
        #   d/ds2 = scale (-B P / (2 s2) + Q / (2 s2^2)) = (scale / s2) (B P (k0 - 1/2) - ve)          (two launches)
        k0 = -0.5 * LOG2PI - 0.5 * float(np.log(nv))
        return torch.mul(ve, -scale / nv).add_(scale / nv * B * P * (k0 - 0.5)).reshape(1)


_ROW_DIAGONAL = "a dot-product, ArcCosine or Coregion member (Linear, Polynomial, ArcCosine, Coregion): K(x, x) depends on the row, which is not built into "


def _knn_terms(spec: KernelSpec, Xb, s0):
    """(knn, s0, K(x, x)) as the Gaussian data term takes the first two and _Seed.noise_grad the third.  A constant diagonal: the
    host scalar, s0 untouched.  A diagonal that depends on the row (rows kd [B]): the C ABI keeps its host-scalar knn, so knn = 0
    and s0 - kd go in; the kernel's (knn - s0) + ssq is then (kd - s0) + ssq in the reference's order, 0 - x being exact."""
    if spec.constant_diagonal:
        kd = spec.kdiag()
        return [kd], s0, kd
    kd = spec.kdiag_rows(Xb)
    return [0.0], s0 - kd, kd


def _factorise(spec: KernelSpec, Z, X, jitter):
    """trapezoid = [Kuu + jitter I ; Kfu ; I]: the factorisation returns Lm, At = Kfu Lm^-T and, from the identity rows, Lm^-T
    itself -- the explicit inverse that turns every triangular solve of the backward into one GEMM.  Returns (Lm, At, Lm^-T, info)."""
    M, n = Z.shape[0], X.shape[0]
    T = torch.empty((M + n + M, M), dtype=torch.float64, device=Z.device)
    spec.build(Z, None, T[:M], diag_add=jitter)                                         # Kuu + jitter I
    if n:
        spec.build(X, Z, T[M:M + n])                                                    # Kfu
    _, info = ops.potrf_(T, M, zero_upper=True, identity_rows=True)                     # (the last M rows: I -> Lm^-T)
    return T[:M], T[M:M + n], T[M + n:], info


def _project(At, q_mu, q_sqrt, **fmean_stats):
    """The rows' statistics under q(u):  s0 = rowsum(At^2), fmean = At q_mu, ssq = rowsum(W_p^2) with W_p = At Lq_p  [P, B, M].
    Returns (s0, fmean, ssq, Lq, LqT, W); q_diag (q_sqrt [M, P] of standard deviations: svgp.py:90-148, conditionals/util.py:149,
    164) never forms W -- one pass with weights, Lq = LqT = W = None.  `fmean_stats` goes to the fmean pass of the full form."""
    if q_sqrt.dim() == 2:
        return (*ops.row_stats(At, V=q_mu, W=q_sqrt.contiguous()), None, None, None)    # rowsum(At^2), At q_mu, sum_k At^2 q^2
    P = q_sqrt.shape[0]
    Lq = _tril(q_sqrt)                                                                  # band_part(q_sqrt, -1, 0)
    LqT = ops.transpose(q_sqrt, mode=1)                                                 # [P, M, M] = tril(q_sqrt)^T
    s0, fmean, _ = ops.row_stats(At, V=q_mu, **fmean_stats)                             # rowsum(At^2), At q_mu
    W = ops.gemm_nt(At, LqT, b_tri=1)                                                   # [P, B, M]: W_p = At Lq_p
    ssq = torch.stack([ops.row_stats(W[p])[0] for p in range(P)])                       # [P, B]
    return s0, fmean, ssq, Lq, LqT, W


def _covariance_tail(spec: KernelSpec, Z, Xb, Kuf_bar, LT, LinvT, Lbar, knn_bar, *, first=None, packed=False, before_products=None):
    """From Kuf_bar [M, B] and Lm_bar to (d/dvariance, d/dlengthscales, Z_bar):  Kuu_bar by the Cholesky adjoint (LT = Lm^T), the
    kernel adjoints of Kuf and of Kuu, and  knn_bar * d kdiag / d variance_i  for the Knn = kdiag in every fvar.
    first: the Kuf adjoint where the caller already has it (SGPR sums it over the shards); before_products: see cholesky_adjoint.
    A spec without a constant diagonal (a dot-product member): knn_bar is dF/dKnn per ROW of Xb [B] (_Seed.crows) and the members'
    variance and offset gradients collect sum_b knn_bar_b d K(x_b, x_b) / d theta (KernelSpec.diag_adjoint); Z does not enter Knn."""
    Kuu_bar = cholesky_adjoint(LT, LinvT, Lbar, before_products=before_products)
    if not spec.constant_diagonal:
        dv1, dl1, Zb1 = first if first is not None else spec.adjoint(Z, Xb, Kuf_bar, symmetric=False)
        dv2, dl2, Zb2 = spec.adjoint(Z, Z, Kuu_bar, symmetric=True)
        dv3, dl3 = spec.diag_adjoint(Xb, knn_bar)
        g_var, g_ls = spec.pack([a + b + c for a, b, c in zip(dv1, dv2, dv3)], [a + b + c for a, b, c in zip(dl1, dl2, dl3)])
        return g_var, g_ls, Zb1 + Zb2
    dkd = spec.dkdiag()
    if packed:
        # one stationary kernel over all input columns: the second adjoint ADDS its variance / lengthscale / Z gradients to the
        # first one's in its own tail launch, and the Knn term of d/dvariance rides along (no elementwise launches at all)
        leaf = spec.members[0]
        into = stationary_kernel_adjoint(leaf, Z, Xb, Kuf_bar, symmetric=False, dvar_add=knn_bar * dkd[0], return_packed=True)
        small_g, Zbar = stationary_kernel_adjoint(leaf, Z, Z, Kuu_bar, symmetric=True, packed_into=into, return_packed=True)
        return small_g[0:1], _ls_grad(small_g[1:], leaf), Zbar
    dv1, dl1, Zb1 = first if first is not None else spec.adjoint(Z, Xb, Kuf_bar, symmetric=False)
    dv2, dl2, Zb2 = spec.adjoint(Z, Z, Kuu_bar, symmetric=True)
    g_var, g_ls = spec.pack([a + b + knn_bar * dk for a, b, dk in zip(dv1, dv2, dkd)], [a + b for a, b in zip(dl1, dl2)])
    return g_var, g_ls, Zb1 + Zb2


class _SideBranch:
    """The {q_mu_bar, Lq_bar} branch of the whitened reverse pass, beside the main one ({Lm_bar -> Cholesky adjoint -> kernel adjoints})
    that is enqueued inside the `with`: `prep()` -> (first result, *arguments of products), `products(*arguments)` -> second result;
    `results` = (first, second) once the block has ended.

    On a device (and OVERLAP_BRANCHES) the branch runs on the side stream: prep at the fork, products when the main branch calls
    `release` (cholesky_adjoint's before_products).  Without one, both run inline after the main branch."""

    def __init__(self, like: torch.Tensor, prep, products):
        self.prep, self.products = prep, products
        self.dev = like.device
        self.side = _side_stream(self.dev) if (OVERLAP_BRANCHES and like.is_cuda) else None
        self.pending = False
        self.results = None

    def __enter__(self):
        if self.side is not None:
            # The side branch reads A, W, r, Lq, q_mu (allocated on the main stream) and allocates its split-K partials from
            # the side stream's pool (~270 MB per latent at M = 2048).  The join sits in __exit__: if anything on the
            # main branch raises, the caller still waits for the side stream before its locals go back to the allocator.
            self.main = torch.cuda.current_stream(self.dev)
            self.side.wait_stream(self.main)
            with torch.cuda.stream(self.side):
                self.first, *self.args = self.prep()
            self.pending = True
            if not GATE_SIDE_BRANCH:
                self.release()
        return self

    # The main branch is the LONGER one (Lm_bar, three dependent M^3 products, two kernel adjoints: ~2.5 ms against ~1.6) and
    # its short HBM-bound kernels starve while a chip-filling GEMM of the other stream has workgroups waiting for a slot: the
    # combine / transpose pair behind the Lm_bar product took 298 + 239 us beside the side branch's GEMM, 41 + 11 us alone
    # (profiles/r06_train_timeline_before.txt).  So the side branch's GEMMs wait until that preparation is enqueued; from
    # there on the main branch only runs under-filled products that are bound by their longest tile, not by the CUs they get.
    def release(self):
        if not self.pending:
            return
        self.pending = False
        with torch.cuda.stream(self.side):
            if GATE_SIDE_BRANCH:
                ev = torch.cuda.Event()
                ev.record(self.main)
                self.side.wait_event(ev)
            self.second = self.products(*self.args)

    def __exit__(self, exc_type, exc, tb):
        if self.side is not None:
            if exc_type is None:
                self.release()
            self.main.wait_stream(self.side)
        if exc_type is None:
            if self.side is not None:
                self.first.record_stream(self.main)
                self.second.record_stream(self.main)
            else:
                self.first, *args = self.prep()
                self.second = self.products(*args)
            self.results = (self.first, self.second)
        return False


def svgp_elbo_and_grad(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor,
                       *, variance: float = None, lengthscales=None, noise_variance: float, jitter: float, scale: float = 1.0,
                       mean_const: float = 0.0, kl_weight: float = 1.0, family: str = "SquaredExponential",
                       kernel_spec: "KernelSpec" = None, likelihood=None, alpha=None
                       ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """F = scale * sum_b var_exp_b - kl_weight * KL for the whitened SVGP with a stationary kernel (or, `kernel_spec`, a Sum /
    Product of stationary kernels: then grads["variance"] is [n_members] and grads["lengthscales"] a list), a Gaussian likelihood
    and a full q_sqrt [P, M, M], and dF/d{variance, lengthscales, noise_variance, Z, q_mu, q_sqrt, mean_const}.

    `family` is any name of ops.KERNEL_FAMILIES; "RationalQuadratic" takes `alpha` and adds grads["alpha"] [1] (for a `kernel_spec` with
    several members: a list, None where a member has no alpha); a static family (White, Constant) has an empty grads["lengthscales"].

    Returns (F [1], grads, info).  `scale` = num_data / minibatch size (svgp.py:176-180).  For a row shard of a
    data-parallel step pass the GLOBAL scale and kl_weight = 1 / world_size: the SUM over ranks of F and of every
    gradient is then the full-batch value (one all-reduce of the packed gradient, distributed.all_reduce_grads).

    likelihood = (name, params) of ops.likelihood_varexp_sum (Bernoulli, Poisson, StudentT) replaces the Gaussian: the variational
    expectations and the seeds r = dF/dfmean, c = dF/dfvar -- now one value per (row, latent) -- come from the quadrature kernel;
    `noise_variance` is ignored, grads has no "noise_variance" and, where the likelihood class names a `device_grad_param`, a
    "likelihood_<that name>" (StudentT and Beta: "likelihood_scale", Gamma: "likelihood_shape", Ordinal: "likelihood_sigma")."""
    M, D = Z.shape
    P = q_mu.shape[1]
    q_diag = q_sqrt.dim() == 2
    if tuple(q_sqrt.shape) not in ((P, M, M), (M, P)):
        raise ValueError("svgp_elbo_and_grad needs q_sqrt [P, M, M] or, for q_diag, [M, P]")
    dev = Z.device
    spec = kernel_spec if kernel_spec is not None else KernelSpec.single(variance, lengthscales, family, alpha)
    spec.warm(dev, D)   # (device copies of the lengthscales BEFORE the first kernel is enqueued: see ls_device)

    # ---------------------------------------------------------------- forward (intermediates kept)
    if likelihood is not None and not spec.constant_diagonal:
        raise NotImplementedError(_ROW_DIAGONAL + "the quadrature likelihoods' reverse pass")
    fwd = _svgp_forward(spec, Z, Xb, q_mu, q_sqrt, jitter)
    s0, fmean, ssq = fwd.s0, fwd.fmean, fwd.ssq
    if likelihood is not None:
        ve, dmu, dvar, lik_grads = _likelihood_stage(likelihood, Yb, fmean, s0=s0, ssq=ssq, knn=[spec.kdiag()], mean_const=mean_const)
    else:
        knn, s0_knn, kd = _knn_terms(spec, Xb, s0)
        ve, _ = ops.gaussian_varexp_sum(Yb, fmean, s0=s0_knn, ssq=ssq, knn=knn, noise_variance=noise_variance,
                                        mean_const=mean_const)
    kl = ops.gauss_kl_white(q_mu, q_sqrt)
    F = torch.mul(ve, scale).sub_(kl, alpha=kl_weight)

    # ---------------------------------------------------------------- backward
    seed = _Seed(Yb, fmean, scale=scale, mean_const=mean_const, noise_variance=noise_variance,
                 lik_grads=(dmu, dvar) if likelihood is not None else None)
    g_var, g_ls, Zbar, g_qmu, g_qs = _svgp_backward(spec, Z, Xb, q_mu, q_sqrt, fwd, seed, kl_weight)
    grads = spec.kernel_grads(g_var, g_ls)
    if likelihood is None:
        grads["noise_variance"] = seed.noise_grad(ve, s0, ssq, kd)
    grads.update({"Z": Zbar, "q_mu": g_qmu, "q_sqrt": g_qs, "mean_const": seed.r.sum().reshape(1)})
    if likelihood is not None:
        grads.update({name: g * scale for name, g in lik_grads.items()})
    return F, grads, fwd.info


def _likelihood_stage(likelihood, Y, fmean, *, s0, ssq, knn, mean_const):
    """The variational-expectation stage of a reverse pass for likelihood = (name, params): (sum VE [1], dmu, dvar [rows, P], {grad
    name: dVE/dparameter [1]}).  A name of ops.LIKELIHOOD_CODES is one ops.likelihood_varexp_sum call, and its gradient -- where the
    likelihood class names a `device_grad_param` -- is "likelihood_<that name>".  "switched": params is the member table of
    ops.switched_varexp_sum, the task label is the last column of Y, and the gradients are "likelihood_<t>", one per task."""
    if likelihood[0] == "switched":
        out, _, dmu, dvar, _ = ops.switched_varexp_sum(Y, fmean, s0=s0, ssq=ssq, knn=knn, members=likelihood[1], mean_const=mean_const,
                                                       want_grads=True)
        return out[0:1], dmu, dvar, {f"likelihood_{t}": out[1 + t:2 + t] for t in range(len(likelihood[1]))}
    out, _, dmu, dvar, _ = ops.likelihood_varexp_sum(Y, fmean, s0=s0, ssq=ssq, knn=knn, lik=likelihood[0], params=likelihood[1],
                                                     mean_const=mean_const, want_grads=True)
    from .likelihoods import device_grad_param
    name = device_grad_param(likelihood[0])   # (the one Parameter whose derivative the kernel returns as out[1])
    return out[0:1], dmu, dvar, ({} if name is None else {"likelihood_" + name: out[1:2]})


class _SvgpForward:
    """What the whitened forward keeps for its backward: Lm, At = Kfu Lm^-T, Lm^-T, info (_factorise) and s0, fmean, ssq, Lq, LqT, W
    (_project)."""

    def __init__(self, factors, stats):
        self.L, self.At, self.LinvT, self.info = factors
        self.s0, self.fmean, self.ssq, self.Lq, self.LqT, self.W = stats


def _svgp_forward(spec: KernelSpec, Z, Xb, q_mu, q_sqrt, jitter) -> _SvgpForward:
    """the part of the whitened forward in front of the likelihood: factorisation and the rows' statistics under q(u)"""
    factors = _factorise(spec, Z, Xb, jitter)
    return _SvgpForward(factors, _project(factors[1], q_mu, q_sqrt))


def _svgp_backward(spec: KernelSpec, Z, Xb, q_mu, q_sqrt, fwd: _SvgpForward, seed: _Seed, kl_weight: float):
    """The whitened reverse pass from the seeds (r = dF/dfmean, c = dF/dfvar: _Seed) of the data term and -kl_weight KL to
    (d/dvariance, d/dlengthscales, Z_bar, q_mu_bar, q_sqrt_bar).  A stage between the latent moments and the likelihood (the mixing
    of a LinearCoregionalization model) only changes the seed: svgp_elbo_and_grad_lcm runs this once per latent."""
    P = q_mu.shape[1]
    q_diag = q_sqrt.dim() == 2
    L, At, LinvT, Lq, W = fwd.L, fwd.At, fwd.LinvT, fwd.Lq, fwd.W
    r = seed.r
    plain = not q_diag and seed.scalar and P <= 16
    # (plain: r q_mu^T - 2 c P At in ONE pass over At; it was a K = P GEMM, then an axpy pass behind the products below)
    Atb = ops.lowrank_axpy(-2.0 * seed.c * P, At, r, q_mu) if plain else ops.gemm_nt(r, q_mu)  # r q_mu^T  [B, M]
    if q_diag:
        seed.add_qdiag_term(Atb, At, q_sqrt)                                            # + 2c At (sum_p q_p^2 - P) per column
    else:
        Wg, ag = seed.add_W_LqT(Atb, W, Lq)                                             # + 2c sum_p W_p Lq_p^T
        if not plain:
            seed.add_At(Atb, At)                                                        # - 2 c P At
    A = ops.transpose(At)                                                               # [M, B]
    Kfu_bar = ops.gemm_nt(Atb, LinvT, b_tri=1)                                          # At_bar Lm^-1  [B, M]
    Kuf_bar = ops.transpose(Kfu_bar)                                                    # [M, B]

    # branch_q in two parts: its HBM-bound preparation (At^T r, the transposes of W) and its chip-filling GEMMs
    def branch_q_prep():
        # At^T r - q_mu: a thin product -- ONE pass over A (gpk_row_stats' At V form), not a GEMM with a 64-column tile for P columns
        # (that launch took 67 us alone and 523 us beside the main branch's product, profiles/r06_train_timeline_fused_glue.txt)
        g_mu = ops.row_stats(A, V=r, want_sumsq=False)[1].sub_(q_mu, alpha=kl_weight)
        return g_mu, (None if q_diag else [ops.transpose(Wg[p]) for p in range(P)])

    def branch_q_products(WgT):
        if q_diag:   # d/dq = 2c colsum(At^2) q - (q - 1/q)   (KL of a diagonal q: kullback_leiblers.py:131-133,146-148)
            return seed.weighted_colsq(A, At) * q_sqrt - kl_weight * (q_sqrt - 1.0 / q_sqrt)
        g = torch.stack([splitk_gemm_nt(A, WgT[p], c_lower=True, alpha=ag) for p in range(P)]) if P > 1 else \
            splitk_gemm_nt(A, WgT[0], c_lower=True, alpha=ag).unsqueeze(0)
        g.sub_(Lq, alpha=kl_weight)                                                     # 2c tril(At^T W_p) - Lq_p
        g.diagonal(dim1=1, dim2=2).add_(kl_weight / Lq.diagonal(dim1=1, dim2=2))
        return g

    one_kernel = spec.packable and seed.scalar                   # (the packed tail of _covariance_tail)
    LT = ops.transpose(L, mode=1)
    with _SideBranch(Z, branch_q_prep, branch_q_products) as branch:
        Lbar = splitk_gemm_nt(Kuf_bar, A, c_lower=True, alpha=-1.0)                     # -tril(Kfu_bar^T At)
        g_var, g_ls, Zbar = _covariance_tail(spec, Z, Xb, Kuf_bar, LT, LinvT, Lbar, seed.kdiag_bar(spec), packed=one_kernel,
                                             before_products=branch.release)
    g_qmu, g_qs = branch.results
    return g_var, g_ls, Zbar, g_qmu, g_qs


def svgp_elbo_and_grad_lcm(Zs, Xs, Yb: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor, W, *, kernel_specs,
                           noise_variance: float, jitter: float, scale: float = 1.0, mean_const: float = 0.0,
                           kl_weight: float = 1.0):
    """svgp_elbo_and_grad for a LinearCoregionalization model: L latent GPs (latent l: kernel_specs[l] over Zs[l] [M, D_l] and the
    minibatch as its kernel sees it, Xs[l]) mixed into the P columns of Yb by W [P, L] (host array), f = W g + mean_const; whitened,
    q_mu [M, L], full q_sqrt [L, M, M], Gaussian likelihood with one noise variance.

    The seeds of latent l depend on the forward of EVERY latent, so the pass has three phases: the per-latent forwards (intermediates
    kept), ONE mixing stage (ops.mixed_gaussian_varexp_sum: F's data term, dF/dgmean, dF/dW, dF/ds2), then the per-latent backward of
    svgp_elbo_and_grad seeded with r_l = scale dgmu[:, l] and the scalar c_l = -scale sum_p W_pl^2 / (2 s2).
    Returns (F [1], grads, infos): grads["latents"] is the list of per-latent {"variance", "lengthscales", "Z", "q_mu" [M, 1], "q_sqrt"
    [1, M, M]}; "W" [P, L], "noise_variance" [1] and "mean_const" [1] belong to the mixing stage."""
    W = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
    Lnum = len(kernel_specs)
    M = q_mu.shape[0]
    if W.ndim != 2 or W.shape[1] != Lnum or q_mu.shape[1] != Lnum or tuple(q_sqrt.shape) != (Lnum, M, M):
        raise ValueError("svgp_elbo_and_grad_lcm needs W [P, L], q_mu [M, L] and a full q_sqrt [L, M, M] for its L kernel_specs")
    if not all(spec.constant_diagonal for spec in kernel_specs):
        raise NotImplementedError(_ROW_DIAGONAL + "the mixing stage (one knn per latent)")
    for spec, Z in zip(kernel_specs, Zs):
        spec.warm(Z.device, Z.shape[1])
    # ---------------------------------------------------------------- phase 1: the latents' forwards
    cols = [(q_mu[:, l:l + 1].contiguous(), q_sqrt[l:l + 1].contiguous()) for l in range(Lnum)]
    fwds = [_svgp_forward(kernel_specs[l], Zs[l], Xs[l], *cols[l], jitter) for l in range(Lnum)]
    gmean = torch.cat([f.fmean for f in fwds], dim=1)                                   # [B, L]
    s0, ssq = torch.stack([f.s0 for f in fwds]), torch.cat([f.ssq for f in fwds])       # [L, B]
    # ---------------------------------------------------------------- phase 2: the mixing stage
    out, fmean, _, dgmu, dW = ops.mixed_gaussian_varexp_sum(Yb, gmean, W, s0=s0, ssq=ssq, knn=[spec.kdiag() for spec in kernel_specs],
                                                            noise_variance=noise_variance, mean_const=mean_const,
                                                            s0_per_latent=True, want_moments=True, want_grads=True)
    kl = ops.gauss_kl_white(q_mu, q_sqrt)
    F = torch.mul(out[0:1], scale).sub_(kl, alpha=kl_weight)
    r = dgmu.mul_(scale)                                                                # dF/dgmean [B, L]
    c = -0.5 * scale / noise_variance * (W * W).sum(0)                                  # dF/dgvar[:, l]: the same for every row
    # ---------------------------------------------------------------- phase 3: the latents' backwards
    latents = []
    for l in range(Lnum):
        seed = _Seed(Yb, fwds[l].fmean, scale=scale, mean_const=0.0, noise_variance=noise_variance,
                     given=(r[:, l:l + 1].contiguous(), c[l]))
        g_var, g_ls, Zbar, g_qmu, g_qs = _svgp_backward(kernel_specs[l], Zs[l], Xs[l], *cols[l], fwds[l], seed, kl_weight)
        latents.append({**kernel_specs[l].kernel_grads(g_var, g_ls), "Z": Zbar, "q_mu": g_qmu, "q_sqrt": g_qs})
    P = W.shape[0]
    grads = {"latents": latents, "W": dW.mul_(scale), "noise_variance": out[1:2] * scale,
             "mean_const": ((Yb[:, :P] - fmean).sum() * (scale / noise_variance)).reshape(1)}
    return F, grads, torch.cat([f.info.reshape(-1) for f in fwds])


def gpr_lml_and_grad(X: torch.Tensor, Y: torch.Tensor, *, variance: float = None, lengthscales=None, noise_variance: float,
                     mean_const: float = 0.0, family: str = "SquaredExponential", kernel_spec: "KernelSpec" = None,
                     alpha=None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """GPR.log_marginal_likelihood (gpr.py:91-107) and its gradient w.r.t. {variance, lengthscales, noise_variance,
    mean_const} for a SquaredExponential kernel -- what `optimizers/scipy.py:322-331` asks TF autodiff for.

        L = chol(K + s2 I),  alpha = L^-1 (Y - m),  LML = -0.5 |alpha|^2 - 0.5 N P log 2pi - P sum log diag L
        K_bar = 0.5 (beta beta^T - P K^-1),  beta = K^-1 (Y - m)        d/ds2 = tr K_bar,   d/dm = sum beta

    The trapezoid is [K + s2 I ; (Y - m)^T ; I]: the identity rows return L^-T, so K^-1 = L^-T L^-1 and beta are GEMMs
    (no triangular solve), and the kernel-parameter contraction is the same G = K_bar .* K pass as for the SVGP."""
    N, D = X.shape
    P = Y.shape[1]
    dev = X.device
    spec = kernel_spec if kernel_spec is not None else KernelSpec.single(variance, lengthscales, family, alpha)
    spec.warm(dev, D)   # (device copies of the lengthscales BEFORE the first kernel is enqueued: see ls_device)
    T = torch.empty((N + P + N, N), dtype=torch.float64, device=dev)
    het = torch.is_tensor(noise_variance) and noise_variance.dim() >= 1   # one variance per data row (heteroskedastic likelihood)
    if het:
        spec.build(X, None, T[:N])
        ops.diag_add_(T[:N], noise_variance)                                            # add_likelihood_noise_cov, model_utils.py:46-50
    else:
        spec.build(X, None, T[:N], diag_add=noise_variance)
    T[N:N + P] = (Y - mean_const).t()
    invd, info = ops.potrf_(T, N, zero_upper=True, identity_rows=True)                  # (the last N rows: I -> L^-T, N^3/3)
    L, alphat, LinvT = T[:N], T[N:N + P], T[N + P:]
    a2 = ops.row_stats(alphat)[0].sum()
    lml = -0.5 * a2 - 0.5 * N * P * LOG2PI - P * torch.log(torch.diagonal(L)).sum()
    # beta^T = alpha^T L^-1  [P, N];  K^-1 = L^-T (L^-T)^T, lower tiles only
    betat = ops.gemm_nt(alphat, LinvT, b_tri=1)
    Kbar = ops.gemm_nt(LinvT, LinvT, b_tri=1, c_lower=True, a_tri=1)               # (both factors upper: N^3/3 multiply-adds)
    beta = betat.t().contiguous()                                                       # [N, P]
    ops.gemm_nt(beta, beta, alpha=0.5, beta=-0.5 * P, C=Kbar, c_lower=True)             # 0.5 beta beta^T - 0.5 P K^-1
    low = torch.tril(Kbar)
    Kbar = low + torch.tril(low, -1).t()                                                # symmetric, full
    dvs, dlss, _ = spec.adjoint(X, X, Kbar, symmetric=True)
    dvar, dls = spec.pack(dvs, dlss)
    # d LML / d sigma_n^2 = Kbar_nn: their sum for a constant noise variance, the vector for a heteroskedastic likelihood
    grads = {**spec.kernel_grads(dvar, dls),
             "noise_variance": torch.diagonal(Kbar).clone() if het else torch.diagonal(Kbar).sum().reshape(1),
             "mean_const": betat.sum().reshape(1)}
    return lml.reshape(1), grads, info


def sgpr_elbo_and_grad(Z: torch.Tensor, X: torch.Tensor, Y: torch.Tensor, *, variance: float = None, lengthscales=None,
                       noise_variance: float, jitter: float, mean_const: float = 0.0,
                       family: str = "SquaredExponential", group=None, sharded: bool = False,
                       num_data: Optional[int] = None, kernel_spec: "KernelSpec" = None, alpha=None
                       ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """SGPR.elbo (sgpr.py:181-290) and its gradient w.r.t. {variance, lengthscales, noise_variance, Z, mean_const}.
    With At = Kfu Lm^-T, S = At^T At, a = At^T err, q = |At|^2, e2 = |err|^2, B = I + S / s2, w = B^-1 a / s2:

        F     = -N P log(2 pi)/2 - P (logdet B / 2 + N log(s2)/2 + (N var - q) / (2 s2)) - e2 / (2 s2) + a^T w / (2 s2)
        B_bar = -(P B^-1 + w w^T) / 2,   S_bar = B_bar / s2,   a_bar = w / s2,   q_bar = P / (2 s2)
        At_bar = At (2 S_bar + 2 q_bar I) + err a_bar^T        -> then exactly the SVGP chain: Kfu_bar, Lm_bar, Kuu_bar, kernel

    `sharded=True` (NEW: the reference is single process): (X, Y) is THIS rank's row shard (possibly empty), `num_data`
    the global row count.  The forward statistics (S, a, e2, q) are summed over `group` as in models/sgpr.py; everything
    of size M x M after that is replicated.  The reverse pass is linear in what the shards contribute -- At_bar, Kfu_bar,
    -tril(Kfu_bar^T At) and the Kuf part of the kernel adjoint are per-shard -- so ONE more all-reduce of the packed
    (Lm_bar part [M, M], d/dvariance, d/dlengthscales, Z_bar, d/dmean) gives every rank the complete gradient: two
    collectives of M^2 + O(M) doubles per evaluation, none proportional to the data."""
    M, D = Z.shape
    n, P = Y.shape
    dev = Z.device
    # het: `noise_variance` a tensor [n] of one sigma_n^2 per row of THIS shard (a heteroskedastic Gaussian likelihood, sgpr.py:207-211).
    # With w_n = 1 / sigma_n^2 the statistics become S = At^T W At, a = At^T W err, e2 = sum w err^2, q = sum w |At_n|^2 and the bound is
    # the constant-noise one with s2 = 1 plus -P/2 (sum log sigma_n^2 + var sum w_n); At_bar and d/dmean pick up w_n per row, and
    #     dF/dw_n = (a_n^T (2 S_bar + 2 q_bar I) a_n) / 2 + sum_p (a_n . a_bar_p) err_np - sum_p err_np^2 / 2 - P var / 2,
    #     dF/dsigma_n^2 = -w_n^2 dF/dw_n - P w_n / 2        (one entry per row; grads["noise_variance"] is then [n], local to the shard)
    het = torch.is_tensor(noise_variance) and noise_variance.dim() >= 1
    if het:
        wn = (1.0 / noise_variance.reshape(-1)).contiguous()
        swn = torch.sqrt(wn)
        s2 = 1.0
    else:
        s2 = float(noise_variance)
    N = int(num_data) if num_data is not None else n
    if not sharded and N != n:
        raise ValueError("num_data differs from the number of rows of a model that is not sharded")
    # (kernel_spec: a Sum / Product of stationary kernels, members possibly over different input columns -- round 5)
    spec = kernel_spec if kernel_spec is not None else KernelSpec.single(variance, lengthscales, family, alpha)
    if not spec.constant_diagonal:
        raise NotImplementedError(_ROW_DIAGONAL + "SGPR: its statistics take sum_n K(x_n, x_n) as N times one scalar")
    spec.warm(dev, D)   # (device copies of the lengthscales BEFORE the first kernel is enqueued: see ls_device)
    kdiag = spec.kdiag()
    nmem = spec.n
    nlsm = [spec.n_shape(i) for i in range(nmem)]           # shape-gradient entries per member (lengthscales: 1 = isotropic; + extras)

    def all_reduce(t):
        if sharded:
            import torch.distributed as dist
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        return t

    eye = torch.eye(M, dtype=torch.float64, device=dev)
    L, At, LinvT, info = _factorise(spec, Z, X, jitter)
    err = (Y - mean_const).contiguous()
    stats = torch.zeros(M * M + M * P + 4, dtype=torch.float64, device=dev)
    if n:
        A = ops.transpose(At)                                                           # [M, n]
        if het:   # rows scaled by 1 / sigma_n (elementwise glue on [n, M] / [n, P])
            Aw = ops.transpose((At * swn[:, None]).contiguous())
            errw = (err * swn[:, None]).contiguous()
            stats[-4], stats[-3] = -torch.log(wn).sum(), wn.sum()                      # sum log sigma_n^2, sum 1 / sigma_n^2
        else:
            Aw, errw = A, err
        stats[:M * M] = torch.tril(splitk_gemm_nt(Aw, Aw, c_lower=True)).reshape(-1)
        stats[M * M:M * M + M * P] = splitk_gemm_nt(Aw, errw.t().contiguous()).reshape(-1)
        stats[-2], stats[-1] = ops.sumsq(errw)[0], (ops.sumsq(Aw)[0] if het else ops.sumsq(At)[0])
    all_reduce(stats)                                                                   # ---- exchange 1: S, a, e2, q (+ the two noise sums)
    Slow = stats[:M * M].reshape(M, M)
    S = Slow + torch.tril(Slow, -1).t()
    a = stats[M * M:M * M + M * P].reshape(M, P)
    e2, q = stats[-2], stats[-1]
    sum_log_s2, sum_w = (stats[-4], stats[-3]) if het else (N * float(np.log(s2)), N / s2)
    T2 = torch.empty((2 * M + P, M), dtype=torch.float64, device=dev)
    T2[:M] = S / s2 + eye
    T2[M:M + P] = a.t() / s2
    _, info2 = ops.potrf_(T2, M, zero_upper=True, identity_rows=True)
    LB, ct, LBinvT = T2[:M], T2[M:M + P], T2[M + P:]
    half_logdet_b = ops.sum_log_diag(LB)[0]
    F = (-0.5 * N * P * LOG2PI - P * (half_logdet_b + 0.5 * sum_log_s2 + 0.5 * (kdiag * sum_w - q / s2))
         - 0.5 * (e2 / s2 - ops.sumsq(ct)[0]))
    # ---- backward: the M x M tail (replicated)
    Binv = ops.gemm_nt(LBinvT, LBinvT, b_tri=1, a_tri=1)                                # B^-1 = LB^-T LB^-1
    wt = ops.gemm_nt(ct.contiguous(), LBinvT, b_tri=1)                                  # w^T = c^T LB^-1  [P, M]
    w = wt.t().contiguous()                                                             # [M, P]
    Bbar = -0.5 * P * Binv
    ops.gemm_nt(w, w, alpha=-0.5, beta=1.0, C=Bbar)                                     # - w w^T / 2
    Ssym = (2.0 / s2) * Bbar + (P / s2) * eye                                           # 2 S_bar + 2 q_bar I
    abar = w / s2
    # ---- this shard's rows
    # packed per-shard sums: [Lm_bar part (M x M), d/dvariance per member, d/dlengthscales per member, Z_bar (M x D), d/dmean]
    nl_tot = sum(nlsm)
    part = torch.zeros(M * M + nmem + nl_tot + M * D + 1, dtype=torch.float64, device=dev)
    o = M * M
    g_noise_rows = None
    if n:
        Atb = ops.gemm_nt(err, abar)                                                    # err a_bar^T  [n, M]
        if het:
            G = ops.gemm_nt(At, Ssym)                                                   # At (2 S_bar + 2 q_bar I)
            Au = ops.gemm_nt(At, abar.t().contiguous())                                 # (a_n . a_bar_p)  [n, P]
            dF_dw = 0.5 * (G * At).sum(1) + (Au * err).sum(1) - 0.5 * (err * err).sum(1) - 0.5 * P * kdiag
            g_noise_rows = -(wn * wn) * dF_dw - 0.5 * P * wn
            Atb = (Atb + G) * wn[:, None]
        else:
            ops.gemm_nt(At, Ssym, alpha=1.0, beta=1.0, C=Atb)                           # + At (2 S_bar + 2 q_bar I)
        Kfu_bar = ops.gemm_nt(Atb, LinvT, b_tri=1)
        Kuf_bar = ops.transpose(Kfu_bar)
        part[:M * M] = torch.tril(splitk_gemm_nt(Kuf_bar, A, c_lower=True, alpha=-1.0)).reshape(-1)
        dv1, dl1, Zb1 = spec.adjoint(Z, X, Kuf_bar, symmetric=False)
        part[o:o + nmem] = torch.cat(dv1)
        part[o + nmem:o + nmem + nl_tot] = torch.cat([d.reshape(-1) for d in dl1])
        part[o + nmem + nl_tot:o + nmem + nl_tot + M * D] = Zb1.reshape(-1)
        part[-1] = ((err - Au) * wn[:, None]).sum() if het else (err / s2 - ops.gemm_nt(At, abar.t().contiguous())).sum()
    all_reduce(part)                                                                    # ---- exchange 2: the shards' sums
    Lbar = part[:o].reshape(M, M)
    dv1 = [part[o + i].reshape(1) for i in range(nmem)]
    offs = np.concatenate([[0], np.cumsum(nlsm)])
    dl1 = [part[o + nmem + offs[i]:o + nmem + offs[i + 1]] for i in range(nmem)]
    Zb1, g_mean = part[o + nmem + nl_tot:o + nmem + nl_tot + M * D].reshape(M, D), part[-1]
    g_var, g_ls, Zbar = _covariance_tail(spec, Z, None, None, ops.transpose(L, mode=1), LinvT, Lbar, -0.5 * P * sum_w,
                                         first=(dv1, dl1, Zb1))             # (Knn = kdiag in the trace term: -P var sum_w / 2)
    if het:
        g_noise = g_noise_rows if g_noise_rows is not None else torch.zeros(0, dtype=torch.float64, device=dev)
    else:
        wa, ww = (w * a).sum(), (w * w).sum()
        g_noise = (-P * (-0.5 * (M - torch.diagonal(Binv).sum()) / s2 + 0.5 * N / s2 - 0.5 * (N * kdiag - q) / s2 ** 2)
                   + 0.5 * e2 / s2 ** 2 - 0.5 * wa / s2 ** 2 - 0.5 * ww / s2).reshape(1)
    status = torch.maximum(info, info2)
    grads = {**spec.kernel_grads(g_var, g_ls), "noise_variance": g_noise, "Z": Zbar,
             "mean_const": g_mean.reshape(1)}
    return F.reshape(1), grads, status


def svgp_elbo_and_grad_unwhitened(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor,
                                  q_sqrt: torch.Tensor, *, variance: float = None, lengthscales=None, noise_variance: float,
                                  jitter: float, scale: float = 1.0, mean_const: float = 0.0, kl_weight: float = 1.0,
                                  family: str = "SquaredExponential", kernel_spec: "KernelSpec" = None, alpha=None
                       ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """The `whiten=False` SVGP: q(u) = N(q_mu, Lq Lq^T) on u itself (conditionals/util.py:137-139, kullback_leiblers.py:
    98-165 with K = Kuu).  With Linv = Lm^-1 (from the identity rows of the trapezoid):

        forward   A2t = At Linv,  fmean = A2t q_mu,  W_p = A2t Lq_p,  fvar = var - rowsum(At^2) + rowsum(W_p^2)
                  KL = 0.5 sum_p (|Linv q_mu_p|^2 - M - log|Lq_p|^2 + |Linv Lq_p|_F^2) + P sum log diag Lm
        backward  A2t_bar = r q_mu^T + 2c sum_p W_p Lq_p^T,   At_bar = -2cP At + A2t_bar Linv^T,
                  Linv_bar = tril(At^T A2t_bar) - k (alpha q_mu^T + sum_p V_p Lq_p^T)      (alpha = Linv q_mu, V_p = Linv Lq_p)
                  Lm_bar   = -tril(Kfu_bar^T At) - tril(Linv^T Linv_bar Linv^T) - k P diag(1 / Lm)
    and then the same Cholesky / kernel adjoints as the whitened path.  q_diag (q_sqrt [M, P] of standard deviations;
    conditionals/util.py:147-149, kullback_leiblers.py:131-133, 146-152) is the same algebra with Lq_p = diag(q_p): W_p =
    A2t diag(q_p) is never formed (row statistics with weights), sum_p V_p Lq_p^T = Linv diag(sum_p q_p^2), and the trace
    term is sum_m (Kuu^-1)_mm sum_p q_mp^2 with diag(Kuu^-1) = column sums of Linv^2.  Reached through `SVGP.elbo_and_grad` /
    `SVGPTrainer` when `whiten=False`; parity vs the autograd oracle on the emulated primitives
    (tests/test_gradients_cpu.py) and on the GPU (tests/test_gpu_gradients.py)."""
    M, D = Z.shape
    P = q_mu.shape[1]
    q_diag = q_sqrt.dim() == 2
    if tuple(q_sqrt.shape) not in ((P, M, M), (M, P)):
        raise ValueError("svgp_elbo_and_grad_unwhitened needs q_sqrt [P, M, M] or, for q_diag, [M, P]")
    dev = Z.device
    # (kernel_spec: a Sum / Product of stationary kernels, members possibly over different input columns -- round 5)
    spec = kernel_spec if kernel_spec is not None else KernelSpec.single(variance, lengthscales, family, alpha)
    spec.warm(dev, D)   # (device copies of the lengthscales BEFORE the first kernel is enqueued: see ls_device)
    k = float(kl_weight)
    L, At, LinvT, info = _factorise(spec, Z, Xb, jitter)
    Linv = ops.transpose(LinvT)                                                         # lower
    A2t = ops.gemm_nt(At, LinvT, b_tri=1)                                               # At Linv   (util.py:139)
    s0 = ops.row_stats(At)[0]
    alphat = ops.gemm_nt(q_mu.t().contiguous(), Linv, b_tri=2)                          # (Linv q_mu)^T  [P, M]
    if q_diag:
        qd = q_sqrt.contiguous()
        s = (qd * qd).sum(1)                                                            # sum_p q_mp^2  [M]
        _, fmean, ssq = _project(A2t, q_mu, qd)[:3]                                     # A2t q_mu, sum_m A2t^2 q_mp^2
        kinv_diag = ops.row_stats(LinvT)[0]                                             # diag(Kuu^-1) = rowsum((Lm^-T)^2)
        kl = 0.5 * (ops.sumsq(alphat)[0] - M * P - torch.log(qd * qd).sum() + (kinv_diag * s).sum()) \
            + P * ops.sum_log_diag(L)[0]
    else:
        _, fmean, ssq, Lq, LqT, W = _project(A2t, q_mu, q_sqrt, want_sumsq=False)       # W_p = A2t Lq_p  [P, B, M]
        V = ops.gemm_nt(Linv, LqT, b_tri=1, a_tri=2)                                    # [P, M, M]: V_p = Linv Lq_p
        if V.dim() == 2:
            V = V.unsqueeze(0)
        kl = 0.5 * (ops.sumsq(alphat)[0] - M * P - torch.log(Lq.diagonal(dim1=1, dim2=2) ** 2).sum()
                    + sum(ops.sumsq(V[p])[0] for p in range(P))) + P * ops.sum_log_diag(L)[0]
    knn, s0_knn, kd = _knn_terms(spec, Xb, s0)
    ve, _ = ops.gaussian_varexp_sum(Yb, fmean, s0=s0_knn, ssq=ssq, knn=knn, noise_variance=noise_variance,
                                    mean_const=mean_const)
    F = scale * ve - k * kl
    # ---- backward
    seed = _Seed(Yb, fmean, scale=scale, mean_const=mean_const, noise_variance=noise_variance)
    r = seed.r
    A2tb = ops.gemm_nt(r, q_mu)                                                         # r q_mu^T
    if q_diag:
        seed.add_qdiag_term(A2tb, A2t, qd, s)                                           # + 2c A2t diag(sum_p q_p^2)
    else:
        Wg, ag = seed.add_W_LqT(A2tb, W, Lq)                                            # + 2c sum_p W_p Lq_p^T
    Atb = ops.gemm_nt(A2tb, Linv, b_tri=2)                                              # A2t_bar Linv^T
    seed.add_At(Atb, At)                                                                # - 2 c P At
    A = ops.transpose(At)
    A2 = ops.transpose(A2t)
    Kfu_bar = ops.gemm_nt(Atb, LinvT, b_tri=1)
    Kuf_bar = ops.transpose(Kfu_bar)
    # q(u) gradients: data part through A2t, KL part through Kuu^-1
    Kinv_qmu_t = ops.gemm_nt(alphat, LinvT, b_tri=1)                                    # (Linv^T alpha)^T  [P, M]
    g_qmu = ops.row_stats(A2, V=r, want_sumsq=False)[1] - k * Kinv_qmu_t.t()
    if q_diag:   # d/dq_mp = 2c colsum(A2t^2)_m q_mp - k ((Kuu^-1)_mm q_mp - 1 / q_mp)
        g_qs = seed.weighted_colsq(A2, A2t) * qd - k * (kinv_diag[:, None] * qd - 1.0 / qd)
    else:
        g_qs = torch.stack([splitk_gemm_nt(A2, ops.transpose(Wg[p]), c_lower=True, alpha=ag) for p in range(P)])
        for p in range(P):
            KinvLq = ops.gemm_nt(LinvT, ops.transpose(V[p], mode=1), b_tri=1, a_tri=1)  # Linv^T V_p = Kuu^-1 Lq_p (V_p lower)
            g_qs[p] -= k * torch.tril(KinvLq)
        g_qs.diagonal(dim1=1, dim2=2).add_(k / Lq.diagonal(dim1=1, dim2=2))
    # Linv_bar (lower) and its pull-back to Lm
    Linv_bar = splitk_gemm_nt(A, ops.transpose(A2tb), c_lower=True)         # tril(At^T A2t_bar)
    Linv_bar -= k * torch.tril(ops.gemm_nt(alphat.t().contiguous(), q_mu))              # alpha q_mu^T
    if q_diag:
        Linv_bar -= k * torch.tril(Linv) * s[None, :]                                   # Linv diag(sum_p q_p^2)
    for p in range(0 if q_diag else P):
        Linv_bar -= k * torch.tril(ops.gemm_nt(V[p], Lq[p], b_tri=2))                   # V_p Lq_p^T
    X1 = ops.gemm_nt(LinvT, ops.transpose(Linv_bar, mode=1), b_tri=1, a_tri=1)                   # Linv^T Linv_bar (Linv_bar lower)
    X2 = ops.gemm_nt(X1, Linv, b_tri=2)                                                 # (.) Linv^T
    Lbar = splitk_gemm_nt(Kuf_bar, A, c_lower=True, alpha=-1.0) - torch.tril(X2)
    Lbar.diagonal().sub_(k * P / L.diagonal())
    g_var, g_ls, Zbar = _covariance_tail(spec, Z, Xb, Kuf_bar, ops.transpose(L, mode=1), LinvT, Lbar, seed.kdiag_bar(spec))
    grads = {**spec.kernel_grads(g_var, g_ls), "noise_variance": seed.noise_grad(ve, s0, ssq, kd),
             "Z": Zbar, "q_mu": g_qmu, "q_sqrt": g_qs, "mean_const": r.sum().reshape(1)}
    return F, grads, info


def vgp_elbo_and_grad(X: torch.Tensor, Y: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor, *, kernel_spec: "KernelSpec",
                      jitter: float, mean_const: float = 0.0, noise_variance: Optional[float] = None, likelihood=None
                      ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor], torch.Tensor]:
    """VGP.elbo (gpflow/models/vgp.py:131-155) and its gradient: the full variational GP, q(f) = N(L q_mu + m, L S S^T L^T) with
    L = chol(K(X, X) + jitter I) and S_r = tril(q_sqrt[r]) -- the whitened conditional at the data, both factors N x N lower triangular.

        forward   fmean = L q_mu + m,   fvar[n, r] = sum_j (L S_r)[n, j]^2      (ops.tril_product: the product is not stored)
                  F = sum var_exp(fmean, fvar) - KL[q(v) || N(0, I)]
        backward  r = dF/dfmean, c = dF/dfvar [N, R];   T_bar_r = 2 diag(c_r) L S_r  (ops.tril_product in store mode)
                  L_bar = tril(r q_mu^T) + sum_r tril(T_bar_r S_r^T),   S_bar_r = tril(L^T T_bar_r) - S_r + diag(1 / S_r),
                  q_mu_bar = L^T r - q_mu,   K_bar = cholesky_adjoint(L_bar),  kernel parameters from K_bar (symmetric adjoint)

    Gaussian likelihood with one `noise_variance`, or likelihood = (name, params) of ops.likelihood_varexp_sum (then `noise_variance` is
    ignored and the seeds are the quadrature kernel's own dmu, dvar; "multiclass_robustmax": Y is one column of labels, R classes).
    The trapezoid is [K + jitter I ; I], as in gpr_lml_and_grad: the identity rows come back as L^-T, which the Cholesky adjoint needs.
    Returns (F [1], grads, info): grads as svgp_elbo_and_grad names them, without "Z"."""
    N, D = X.shape
    R = q_mu.shape[1]
    if tuple(q_mu.shape) != (N, R) or tuple(q_sqrt.shape) != (R, N, N):
        raise ValueError("vgp_elbo_and_grad needs q_mu [N, R] and a full q_sqrt [R, N, N] for the N rows of X")
    if (noise_variance is None) == (likelihood is None):
        raise ValueError("vgp_elbo_and_grad: one of noise_variance (Gaussian) and likelihood = (name, params)")
    if noise_variance is not None and torch.is_tensor(noise_variance) and noise_variance.dim() >= 1:
        raise NotImplementedError("vgp_elbo_and_grad: one noise variance (a heteroskedastic Gaussian likelihood is outside the VGP's reverse pass)")
    dev = X.device
    spec = kernel_spec
    spec.warm(dev, D)   # (device copies of the lengthscales BEFORE the first kernel is enqueued: see ls_device)
    q_mu, q_sqrt = q_mu.contiguous(), q_sqrt.contiguous()
    # ---------------------------------------------------------------- forward
    T = torch.empty((2 * N, N), dtype=torch.float64, device=dev)
    spec.build(X, None, T[:N], diag_add=jitter)                                         # K + jitter I
    _, info = ops.potrf_(T, N, zero_upper=True, identity_rows=True)                     # (the last N rows: I -> L^-T)
    L, LinvT = T[:N], T[N:]
    ssq, _ = ops.tril_product(L, q_sqrt)                                                # [R, N]
    fmean = ops.row_stats(L, V=q_mu, want_sumsq=False)[1]                               # L q_mu  [N, R] (one pass over L)
    if likelihood is not None:
        ve, dmu, dvar, lik_grads = _likelihood_stage(likelihood, Y, fmean, s0=None, ssq=ssq, knn=[0.0], mean_const=mean_const)
    else:
        ve, _ = ops.gaussian_varexp_sum(Y, fmean, s0=None, ssq=ssq, knn=[0.0], noise_variance=noise_variance, mean_const=mean_const)
    kl = ops.gauss_kl_white(q_mu, q_sqrt)
    F = torch.sub(ve, kl)
    # ---------------------------------------------------------------- backward
    seed = _Seed(Y, fmean, scale=1.0, mean_const=mean_const, noise_variance=noise_variance,
                 lik_grads=(dmu, dvar) if likelihood is not None else None)
    r = seed.r
    if seed.scalar:
        rowscale = torch.full((R, N), 2.0 * seed.c, dtype=torch.float64, device=dev)
    else:
        rowscale = seed.c.t().mul(2.0).contiguous()
    _, Tb = ops.tril_product(L, q_sqrt, rowscale=rowscale, want_ssq=False, want_product=True)   # T_bar_r (zeros above the diagonal)
    Lq = _tril(q_sqrt)                                                                  # band_part(q_sqrt, -1, 0): the GEMMs read stored zeros
    LT = ops.transpose(L, mode=1)
    Lbar = ops.gemm_nt(r, q_mu, c_lower=True)                                           # r q_mu^T (the lower tiles)
    for p in range(R):
        ops.gemm_nt(Tb[p], Lq[p], beta=1.0, C=Lbar, a_tri=2, b_tri=2, c_lower=True)     # + T_bar_p S_p^T
    Lbar = _tril(Lbar)
    g_qs = torch.stack([_tril(ops.gemm_nt(LT, ops.transpose(Tb[p]), a_tri=1, b_tri=1, c_lower=True)) for p in range(R)])   # tril(L^T T_bar_p)
    g_qs.sub_(Lq)
    g_qs.diagonal(dim1=1, dim2=2).add_(1.0 / Lq.diagonal(dim1=1, dim2=2))
    g_qmu = ops.row_stats(LT, V=r.contiguous(), want_sumsq=False)[1].sub_(q_mu)         # L^T r - q_mu
    Kbar = cholesky_adjoint(LT, LinvT, Lbar)
    dvs, dlss, _ = spec.adjoint(X, X, Kbar, symmetric=True)
    g_var, g_ls = spec.pack(dvs, dlss)
    grads = spec.kernel_grads(g_var, g_ls)
    if likelihood is None:
        grads["noise_variance"] = seed.noise_grad(ve, None, ssq, 0.0)
    grads.update({"q_mu": g_qmu, "q_sqrt": g_qs, "mean_const": r.sum().reshape(1)})
    if likelihood is not None:
        grads.update({name: g.clone() for name, g in lik_grads.items()})
    return F, grads, info
