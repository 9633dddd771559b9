"""Device primitives: thin, typed wrappers from torch fp64 HIP tensors to the C-ABI of libgpk.so.

torch is plumbing here (device memory, the current HIP stream, dlpack-style pointers); all arithmetic
happens in the hand-written kernels.  Every function validates device/dtype/layout and raises --
nothing silently falls back to torch math or to the CPU.
"""
from __future__ import annotations

import collections
from functools import partial
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .leaf import FAMILIES, ArcLeaf, CoregionLeaf, DotLeaf, Leaf

NB = 128
KERNEL_FAMILIES = {f.name: f.code for f in FAMILIES}                      # name -> GPK_KERN_* (include/gpk.h)
STATIC_FAMILIES = tuple(f.name for f in FAMILIES if not f.has_distance)   # the inputs are never read, no lengthscale or input gradient
MAX_D = 64


def device() -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.GpkError("gpflow_amd needs a HIP device (torch.cuda.is_available() is False); "
                            "there is no CPU path")
    return torch.device("cuda", torch.cuda.current_device())


def to_device(x, dtype=torch.float64) -> torch.Tensor:
    """NumPy / torch / scalar -> contiguous fp64 tensor on the current HIP device."""
    if isinstance(x, torch.Tensor):
        t = x.to(device=device(), dtype=dtype)
    else:
        t = torch.as_tensor(np.asarray(x, dtype=np.float64), dtype=dtype, device=device())
    return t.contiguous()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(t: torch.Tensor, name: str, ndim: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.GpkError(f"{name}: tensor must live on the HIP device (got {t.device})")
    if t.dtype != torch.float64:
        raise _lib.GpkError(f"{name}: dtype must be float64 (got {t.dtype})")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")


def _rowmajor(t: torch.Tensor, name: str) -> int:
    """Leading dimension of a 2-D row-major view (last stride 1)."""
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a matrix, got shape {tuple(t.shape)}")
    rows, cols = t.shape
    if rows == 0 or cols == 0:   # no elements: the strides of an empty tensor mean nothing (include/gpk.h, empty operands)
        return max(cols, 1)
    if cols > 1 and t.stride(1) != 1:
        raise _lib.GpkError(f"{name}: last dimension must be contiguous")
    return t.stride(0) if rows > 1 else cols


INFO_HANDOFF_TIMEOUT = 2 ** 31 - 1   # include/gpk.h: status of a factorisation whose internal hand-off never arrived


def _ws(nbytes: int) -> torch.Tensor:
    return torch.empty((max(int(nbytes), 8) + 7) // 8, dtype=torch.float64, device=device())


def _ls_host(lengthscales, d: int, family: str = "SquaredExponential", alpha=None):
    """(host array, ard) of the C-ABI for a leaf given by keywords: Leaf.host"""
    return Leaf(family, 1.0, lengthscales, alpha=alpha).host(d)


def _noise_args(noise_variance, rows: int):
    """(scalar, device pointer | None, keep-alive) for the (noise_variance, noise_rows) pair of the C-ABI: a float is the constant
    noise of a homoskedastic Gaussian likelihood; a tensor / array with `rows` entries is one variance per data row
    (Gaussian(variance=Function | scale=Function), likelihoods/scalar_continuous.py:92-111)."""
    if isinstance(noise_variance, (torch.Tensor, np.ndarray)) and int(np.prod(tuple(noise_variance.shape))) != 1:
        nv = to_device(noise_variance).reshape(-1).contiguous()
        if nv.numel() != rows:
            raise ValueError(f"per-row noise variances: expected {rows} entries, got {nv.numel()}")
        return 1.0, nv.data_ptr(), nv
    return float(noise_variance), None, None


# ------------------------------------------------------------------------------------------------
_COLUMNS_DIFFER = "X1 and X2 must have the same number of columns"


def _kernel_operands(X1, X2, G, out, *, x2_optional: bool = True, zero_new: bool = False, columns_differ: str = _COLUMNS_DIFFER):
    """What the kernel_matrix* wrappers check before they look at the leaf: devices and dtypes, the shapes of X2 (None: K(X1, X1),
    where the wrapper allows it) / G (None: no second factor) / out (allocated when None, zero-filled if `zero_new`), d in
    [1, MAX_D].  Returns (n1, n2, d, out); n1 == 0 or n2 == 0: nothing to compute, the wrapper returns `out` (and X2 = NULL would
    mean K(X1, X1) at the C-ABI)."""
    _chk(X1, "X1", 2)
    n1, d = X1.shape
    if X2 is not None or not x2_optional:
        _chk(X2, "X2", 2)
    if G is not None:
        _chk(G, "G", 2)
    if X2 is not None and X2.shape[1] != d:
        raise ValueError(columns_differ)
    n2 = X2.shape[0] if X2 is not None else n1
    if G is not None and tuple(G.shape) != (n1, n2):
        raise ValueError("inconsistent shapes")
    if d < 1 or d > MAX_D:
        raise ValueError(f"input dimension {d} outside [1, {MAX_D}]")
    if out is None:
        out = torch.empty((n1, n2), dtype=torch.float64, device=X1.device)
        if zero_new:
            out.zero_()
    _chk(out, "out", 2)
    return n1, n2, d, out


def _x2_args(X2, n2):
    """(pointer, rows, leading dimension) of the optional second input"""
    return (X2.data_ptr(), n2, _rowmajor(X2, "X2")) if X2 is not None else (None, n2, 0)


# the op names of each kind of leaf and their codes at the C-ABI (include/gpk.h); "k", the row diagonal itself, only in the *_diag entry points
_STATIONARY_OPS = {"mul": 1, "add": 2, "dr2": 3, "dalpha": 4}
_DOT_OPS = {"k": 0, "mul": 1, "add": 2, "ds": 3}
_ARC_OPS = {"k": 0, "mul": 1, "add": 2, "dp": 3}
_COREGION_OPS = {"k": 0, "mul": 1, "add": 2}
_LABELS = (1, "the Coregion kernel reads ONE column of task labels")   # a required width and what a message says of it


def _check_op(name: str, op: str, allowed) -> None:
    if op not in allowed:
        quoted = [repr(o) for o in allowed]
        raise ValueError(f"{name}: op {op!r} is not {', '.join(quoted[:-1])} or {quoted[-1]}")


def _pair_builder(entry: str, X1, X2, G, out, op, codes, leaf, diag_add, lower_only, width=None, x2_optional=True,
                  columns_differ=_COLUMNS_DIFFER):
    """The one body of the kernel_matrix* wrappers of every kind of leaf: `_kernel_operands`, the empty-result return, the leaf's
    C-ABI arguments, the call of `entry` and `_lib.check`.  `op` (None: the entry point takes none) is looked up in `codes`; `leaf()`
    makes the leaf, whose `abi(d)` gives its arguments, the code in front (leaf.py, the protocol); `diag_add` / `lower_only` None: the
    entry point has no such argument; G None: no second factor; `x2_optional`, `columns_differ`: as `_kernel_operands` takes them.
    `width` (`_LABELS`): the kind reads exactly that many columns, its entry points take no `d` and no code, and `leaf()` gives the
    arguments themselves -- the kind's table on the device, a launch of its own -- whatever the sizes."""
    lib = _lib.load()
    n1, n2, d, out = _kernel_operands(X1, X2, G, out, x2_optional=x2_optional, zero_new=lower_only, columns_differ=columns_differ)
    if width is not None:
        if d != width[0]:
            raise ValueError(f"{entry[4:]}: {width[1]}, got {d}")
        args = leaf()
    if n1 == 0 or n2 == 0:
        return out
    head, dims = (), ()
    if width is None:
        args = leaf().abi(d)
        head, dims, args = args[:1], (d,), args[1:]
    rc = getattr(lib, entry)(_stream(), *head, *(() if op is None else (codes[op],)), X1.data_ptr(), n1,
                             _rowmajor(X1, "X1"), *_x2_args(X2, n2), *dims, *args,
                             *(() if diag_add is None else (float(diag_add),)), *(() if lower_only is None else (int(lower_only),)),
                             *(() if G is None else (G.data_ptr(), _rowmajor(G, "G"))), out.data_ptr(), _rowmajor(out, "out"))
    _lib.check(rc, entry)
    return out


def _row_diagonal(entry: str, name: str, codes, X, g, out, op, leaf, width=None):
    """The one body of the *_kernel_diag wrappers: the operand checks of a row diagonal over X [n, D] -- the width, the op (the keys
    of `codes`, "k" first), g given exactly when the op is not "k", g and `out` contiguous [n] -- the empty-result return, the leaf's
    C-ABI arguments (`leaf`, `width`: as `_pair_builder`), the call of `entry` and `_lib.check`.  `name`: the wrapper's, for the messages."""
    lib = _lib.load()
    _chk(X, "X", 2)
    n, d = X.shape
    if width is not None and d != width[0]:
        raise ValueError(f"{name}: {width[1]}, got {d}")
    if width is None and (d < 1 or d > MAX_D):
        raise ValueError(f"input dimension {d} outside [1, {MAX_D}]")
    _check_op(name, op, codes)
    if (op == "k") != (g is None):
        with_g = [repr(o) for o in codes if o != "k"]
        raise ValueError(f"{name}: g goes with the ops {', '.join(with_g[:-1])} and {with_g[-1]} and only with them")
    if g is not None:
        _chk(g, "g", 1)
        if g.shape[0] != n or not g.is_contiguous():
            raise ValueError(f"{name}: g must be a contiguous [n]")
    if width is not None:
        args = leaf()
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=X.device)
    _chk(out, "out", 1)
    if out.shape[0] != n or not out.is_contiguous():
        raise ValueError(f"{name}: out must be a contiguous [n]")
    if n == 0:
        return out
    head, dims = (), ()
    if width is None:
        args = leaf().abi(d)
        head, dims, args = args[:1], (d,), args[1:]
    rc = getattr(lib, entry)(_stream(), *head, codes[op], X.data_ptr(), n, _rowmajor(X, "X"), *dims, *args,
                             None if g is None else g.data_ptr(), out.data_ptr())
    _lib.check(rc, entry)
    return out


def kernel_matrix(X1: torch.Tensor, X2: Optional[torch.Tensor], *, variance: float, lengthscales,
                  family: str = "SquaredExponential", diag_add: float = 0.0, lower_only: bool = False,
                  alpha=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K(X1, X2) (or K(X1, X1) + diag_add I when X2 is None) -> [n1, n2]."""
    return _pair_builder("gpk_kernel_matrix", X1, X2, None, out, None, None,
                         partial(Leaf, family, variance, lengthscales, alpha=alpha), diag_add, lower_only)


def kernel_matrix_hadamard(X1: torch.Tensor, X2: torch.Tensor, G: torch.Tensor, *, variance: float, lengthscales,
                           family: str = "SquaredExponential", alpha=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """G .* K(X1, X2) with K recomputed on the fly -> [n1, n2] (the elementwise factor of the kernel backward)."""
    return _pair_builder("gpk_kernel_matrix_hadamard", X1, X2, G, out, None, None,
                         partial(Leaf, family, variance, lengthscales, alpha=alpha), None, None,
                         x2_optional=False, columns_differ="inconsistent shapes")


def kernel_matrix_combine(X1: torch.Tensor, X2: Optional[torch.Tensor], G: torch.Tensor, *, op: str, variance: float,
                          lengthscales, family: str = "SquaredExponential", diag_add: float = 0.0, alpha=None,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = G .* K(X1, X2) (op "mul"), G + K(X1, X2) (op "add") or G .* (-2 dK/dr2)(X1, X2) (op "dr2": the factor of the
    lengthscale / input gradients of a stationary kernel; r2 = scaled squared distance), K recomputed on the fly; `out`
    may be G itself.  X2 None: K(X1, X1); `diag_add` goes onto the diagonal of the combined result ("mul" / "add"), and
    "dr2" writes exact zeros on the diagonal.  op "dalpha" ("RationalQuadratic" only): G .* dK/dalpha, diagonal as "dr2"."""
    return _pair_builder("gpk_kernel_matrix_combine", X1, X2, G, out, op, _STATIONARY_OPS,
                         partial(Leaf, family, variance, lengthscales, alpha=alpha), diag_add, None)


# ------------------------------------------------------------------------------------------------ dot-product kernels (dot.hip)
def dot_kernel_matrix(X1: torch.Tensor, X2: Optional[torch.Tensor], *, family: str = "Linear", variance, offset=None, degree=None,
                      diag_add: float = 0.0, lower_only: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K(X1, X2) (or K(X1, X1) + diag_add I when X2 is None) -> [n1, n2] of a dot-product leaf: "Linear" (X1 * variance) X2^T, or
    "Polynomial" (that + offset)^degree.  `variance` one weight or [D].  The symmetric build is exactly symmetric (include/gpk.h)."""
    return _pair_builder("gpk_dot_kernel_matrix", X1, X2, None, out, None, None,
                         partial(DotLeaf, family, variance, offset, degree), diag_add, lower_only)


def dot_kernel_matrix_combine(X1: torch.Tensor, X2: Optional[torch.Tensor], G: torch.Tensor, *, op: str, family: str = "Linear", variance,
                              offset=None, degree=None, diag_add: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = G .* K(X1, X2) (op "mul"), G + K(X1, X2) (op "add") or G .* dK/ds (op "ds": s the weighted dot product; Polynomial
    degree (s + offset)^(degree - 1), Linear 1), K recomputed on the fly; `out` may be G itself.  X2 None: K(X1, X1); `diag_add`
    goes onto the diagonal of the combined result ("mul" / "add"); "ds" does NOT zero the diagonal."""
    _check_op("dot_kernel_matrix_combine", op, ("mul", "add", "ds"))
    return _pair_builder("gpk_dot_kernel_matrix_combine", X1, X2, G, out, op, _DOT_OPS,
                         partial(DotLeaf, family, variance, offset, degree), diag_add, None)


def dot_kernel_diag(X: torch.Tensor, g: Optional[torch.Tensor] = None, *, op: str = "k", family: str = "Linear", variance, offset=None,
                    degree=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row diagonal kd [n] of a dot-product leaf over the rows of X [n, D] (op "k"), or g .* kd ("mul"), g + kd ("add"),
    g .* dkd/ds ("ds") with g [n]; `out` may be g.  kd is the diagonal of dot_kernel_matrix(X, None), bit for bit."""
    return _row_diagonal("gpk_dot_kernel_diag", "dot_kernel_diag", _DOT_OPS, X, g, out, op,
                         partial(DotLeaf, family, variance, offset, degree))


def dot_adjoint_tail(R: torch.Tensor, A: torch.Tensor, w: torch.Tensor, *, symmetric: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d/dvariance [1 or D], d/doffset [1], A_bar [n1, D]) of a dot-product leaf from R [n1, >= 1 + D] = G [1, B] (G = Kbar .* dK/ds),
    the first kernel argument A [n1, D] and the weights as a device tensor, [1] or -- ARD -- [D] (include/gpk.h:
    gpk_dot_adjoint_tail) -- one launch, bit-identical when repeated."""
    lib = _lib.load()
    _chk(R, "R", 2)
    _chk(A, "A", 2)
    _chk(w, "w", 1)
    n1, d = A.shape
    if R.shape[0] != n1 or R.shape[1] < 1 + d or w.shape[0] not in (1, d) or not w.is_contiguous() or d < 1 or d > MAX_D:
        raise ValueError("dot_adjoint_tail: R must be [n1, >= 1 + D], w a contiguous [1] or [D], D in [1, 64]")
    ard = int(w.shape[0] == d and d > 1)
    nw = d if ard else 1
    small = torch.empty(nw + 1, dtype=torch.float64, device=A.device)
    Abar = torch.empty((n1, d), dtype=torch.float64, device=A.device)
    rc = lib.gpk_dot_adjoint_tail(_stream(), R.data_ptr(), _rowmajor(R, "R"), A.data_ptr(), _rowmajor(A, "A"), n1, d, w.data_ptr(), ard,
                                  int(bool(symmetric)), small.data_ptr(), Abar.data_ptr(), _rowmajor(Abar, "A_bar"))
    _lib.check(rc, "gpk_dot_adjoint_tail")
    return small[:nw], small[nw:], Abar


# ------------------------------------------------------------------------------------------------ ArcCosine kernel (arccosine/arccosine.hip)
ARC_TILE = 64   # include/gpk.h: GPK_ARC_TILE


def arccos_kernel_matrix(X1: torch.Tensor, X2: Optional[torch.Tensor], *, order: int = 0, variance=1.0, weight_variances=1.0,
                         bias_variance=1.0, diag_add: float = 0.0, lower_only: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K(X1, X2) (or K(X1, X1) + diag_add I when X2 is None) -> [n1, n2] of an ArcCosine leaf of order 0, 1 or 2.  `weight_variances`
    one weight or [D].  The symmetric build is exactly symmetric and takes its diagonal by index (include/gpk.h)."""
    return _pair_builder("gpk_arccos_kernel_matrix", X1, X2, None, out, None, None,
                         partial(ArcLeaf, order, variance, weight_variances, bias_variance), diag_add, lower_only)


def arccos_kernel_matrix_combine(X1: torch.Tensor, X2: Optional[torch.Tensor], G: torch.Tensor, *, op: str, order: int = 0, variance=1.0,
                                 weight_variances=1.0, bias_variance=1.0, diag_add: float = 0.0,
                                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = G .* K(X1, X2) (op "mul") or G + K(X1, X2) (op "add"), K recomputed on the fly; `out` may be G itself.  X2 None: K(X1, X1)
    with the diagonal by index; `diag_add` goes onto the diagonal of the combined result."""
    _check_op("arccos_kernel_matrix_combine", op, ("mul", "add"))
    return _pair_builder("gpk_arccos_kernel_matrix_combine", X1, X2, G, out, op, _ARC_OPS,
                         partial(ArcLeaf, order, variance, weight_variances, bias_variance), diag_add, None)


def arccos_kernel_diag(X: torch.Tensor, g: Optional[torch.Tensor] = None, *, op: str = "k", order: int = 0, variance=1.0,
                       weight_variances=1.0, bias_variance=1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row diagonal kd [n] = variance jf p^order (jf = 1, 1, 3) of an ArcCosine leaf over the rows of X [n, D] (op "k"), or
    g .* kd ("mul"), g + kd ("add"), g .* dkd/dp ("dp") with g [n]; `out` may be g.  The closed form: NOT the diagonal of
    arccos_kernel_matrix(X, None) bit for bit (include/gpk.h)."""
    return _row_diagonal("gpk_arccos_kernel_diag", "arccos_kernel_diag", _ARC_OPS, X, g, out, op,
                         partial(ArcLeaf, order, variance, weight_variances, bias_variance))


def arccos_adjoint_parts(n1: int, n2: int, device_=None) -> torch.Tensor:
    """the scratch operand `parts` of arccos_adjoint_stage / _tail: tc n1 + tr n2 + tr tc doubles, tr / tc the tile rows / columns of
    ARC_TILE (include/gpk.h: its documented extent); its contents at entry do not matter"""
    tr, tc = -(-int(n1) // ARC_TILE), -(-int(n2) // ARC_TILE)
    return torch.empty(tc * int(n1) + tr * int(n2) + tr * tc, dtype=torch.float64, device=device_ or device())


def arccos_adjoint_stage(X1: torch.Tensor, X2: Optional[torch.Tensor], Kbar: torch.Tensor, parts: torch.Tensor, *, order: int = 0,
                         variance=1.0, weight_variances=1.0, bias_variance=1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass over Kbar [n1, n2]: returns G = Kbar .* dK/ds (`out` may be Kbar itself) and fills `parts` (arccos_adjoint_parts) with
    the per-tile sums of Kbar .* dK/dp (by row), Kbar .* dK/dq (by column) and Kbar .* K / variance.  X2 None: K(X1, X1), the diagonal
    by index.  Deterministic: a second call gives the same bits."""
    lib = _lib.load()
    n1, n2, d, out = _kernel_operands(X1, X2, Kbar, out)
    _chk(parts, "parts", 1)
    tr, tc = -(-n1 // ARC_TILE), -(-n2 // ARC_TILE)
    if not parts.is_contiguous() or parts.numel() < tc * n1 + tr * n2 + tr * tc:
        raise ValueError(f"arccos_adjoint_stage: parts must be a contiguous [>= {tc * n1 + tr * n2 + tr * tc}] (ops.arccos_adjoint_parts)")
    if n1 == 0 or n2 == 0:
        return out
    order, w, ard, v, b = ArcLeaf(order, variance, weight_variances, bias_variance).abi(d)
    rc = lib.gpk_arccos_adjoint_stage(_stream(), order, X1.data_ptr(), n1, _rowmajor(X1, "X1"), *_x2_args(X2, n2), d, w, ard, v, b,
                                      Kbar.data_ptr(), _rowmajor(Kbar, "Kbar"), out.data_ptr(), _rowmajor(out, "out"), parts.data_ptr())
    _lib.check(rc, "gpk_arccos_adjoint_stage")
    return out


def arccos_adjoint_tail(R: torch.Tensor, A: torch.Tensor, Bm: Optional[torch.Tensor], parts: torch.Tensor, *,
                        weight_variances) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d/dvariance [1], d/dweight_variances [1 or D], d/dbias_variance [1], A_bar [n1, D]) of an ArcCosine leaf from R [n1, >= 1 + D]
    = G [1, B], the `parts` of arccos_adjoint_stage, the first kernel argument A [n1, D] and the second Bm [n2, D] (None: symmetric --
    Bm is A, Kbar symmetric, A_bar collects both arguments); include/gpk.h: gpk_arccos_adjoint_tail -- one launch, bit-identical
    when repeated."""
    lib = _lib.load()
    _chk(R, "R", 2)
    _chk(A, "A", 2)
    _chk(parts, "parts", 1)
    n1, d = A.shape
    if Bm is not None:
        _chk(Bm, "Bm", 2)
    n2 = n1 if Bm is None else Bm.shape[0]
    w = np.asarray(weight_variances, dtype=np.float64)
    tr, tc = -(-n1 // ARC_TILE), -(-n2 // ARC_TILE)
    if R.shape[0] != n1 or R.shape[1] < 1 + d or d < 1 or d > MAX_D or (Bm is not None and Bm.shape[1] != d) or w.ndim > 1 \
            or (w.ndim == 1 and w.size != d) or not parts.is_contiguous() or parts.numel() < tc * n1 + tr * n2 + tr * tc:
        raise ValueError("arccos_adjoint_tail: R must be [n1, >= 1 + D], Bm [n2, D], weight_variances one weight or [D], D in [1, 64], "
                         "parts the stage's (ops.arccos_adjoint_parts)")
    ard = int(w.ndim == 1)
    nw = d if ard else 1
    small = torch.zeros(nw + 2, dtype=torch.float64, device=A.device)
    Abar = torch.zeros((n1, d), dtype=torch.float64, device=A.device) if n2 == 0 else torch.empty((n1, d), dtype=torch.float64, device=A.device)
    if n1 == 0 or n2 == 0:
        return small[:1], small[1:1 + nw], small[1 + nw:], Abar
    rg = torch.empty(n1 + n2, dtype=torch.float64, device=A.device)
    rc = lib.gpk_arccos_adjoint_tail(_stream(), R.data_ptr(), _rowmajor(R, "R"), A.data_ptr(), _rowmajor(A, "A"), n1,
                                     None if Bm is None else Bm.data_ptr(), 0 if Bm is None else _rowmajor(Bm, "Bm"), n2, d,
                                     _lib.host_doubles(np.atleast_1d(w).tolist()), ard, parts.data_ptr(), rg.data_ptr(), small.data_ptr(),
                                     Abar.data_ptr(), _rowmajor(Abar, "A_bar"))
    _lib.check(rc, "gpk_arccos_adjoint_tail")
    return small[:1], small[1:1 + nw], small[1 + nw:], Abar


# ------------------------------------------------------------------------------------------------ ChangePoints kernel (changepoints/changepoints.hip)
CP_TILE, CP_MAX_MEMBERS, CP_TAIL_ROWS = 64, 16, 256   # include/gpk.h: GPK_CP_TILE, GPK_CP_MAX_MEMBERS; rows per workgroup of the tail


def _cp_points(locations, steepness):
    """(C, host locations, host steepness) of the gpk_changepoint_* entry points: `locations` [C] SORTED, `steepness` [C] positive"""
    loc = np.asarray(locations, dtype=np.float64).reshape(-1)
    st = np.asarray(steepness, dtype=np.float64).reshape(-1)
    if st.size != loc.size:
        raise ValueError(f"changepoints: {loc.size} locations and {st.size} steepness entries")
    if loc.size + 1 > CP_MAX_MEMBERS:
        raise NotImplementedError(f"changepoints: more than {CP_MAX_MEMBERS} member kernels")
    return int(loc.size), _lib.host_doubles(loc.tolist() or [0.0]), _lib.host_doubles(st.tolist() or [1.0])


def _cp_column(x, name: str):
    """(pointer, rows, stride) of a switch column: an [n] or [n, 1] view, e.g. X[:, switch_dim] of a row-major X"""
    _chk(x, name)
    if x.dim() == 2 and x.shape[1] == 1:
        x = x[:, 0]
    if x.dim() != 1:
        raise ValueError(f"{name}: the switch column is [n] (a view such as X[:, switch_dim])")
    n = x.shape[0]
    ld = int(x.stride(0)) if n > 1 else 1
    if ld < 1:
        raise ValueError(f"{name}: the switch column needs a positive stride")
    return x.data_ptr(), n, ld


def _cp_vector(v, n: int, name: str):
    _chk(v, name, 1)
    if v.shape[0] != n or not v.is_contiguous():
        raise ValueError(f"{name} must be a contiguous [{n}]")
    return v.data_ptr()


def changepoint_weights(x: torch.Tensor, *, locations, steepness, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A [T, n], T = len(locations) + 1: row i holds a_i(x_r) = sig_{i-1}(x_r) (1 - sig_i(x_r)) over the switch column x (include/gpk.h,
    "ChangePoints kernel"): saturated sigmoids are exactly 0 or 1, a NaN / Inf in x makes that row's weights NaN."""
    lib = _lib.load()
    C, loc, st = _cp_points(locations, steepness)
    px, n, ldx = _cp_column(x, "x")
    if out is None:
        out = torch.empty((C + 1, n), dtype=torch.float64, device=x.device)
    _chk(out, "out", 2)
    if tuple(out.shape) != (C + 1, n):
        raise ValueError(f"changepoint_weights: out must be [{C + 1}, {n}]")
    if n == 0:
        return out
    _lib.check(lib.gpk_changepoint_weights(_stream(), px, n, ldx, C, loc, st, out.data_ptr(), _rowmajor(out, "out")), "gpk_changepoint_weights")
    return out


def changepoint_fold(a: torch.Tensor, b: Optional[torch.Tensor], Ki: torch.Tensor, acc: Optional[torch.Tensor] = None, *,
                     diag_add: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = (a b^T) .* Ki (acc None) or acc + (a b^T) .* Ki in ONE pass; b None: b is a (Ki square; an exactly symmetric Ki stays
    exactly symmetric) and diag_add goes onto the diagonal.  `out` may be Ki (acc None) or acc; allocated when None."""
    lib = _lib.load()
    _chk(Ki, "Ki", 2)
    n1, n2 = Ki.shape
    if b is None and n1 != n2:
        raise ValueError("changepoint_fold: b None needs a square Ki")
    pa = _cp_vector(a, n1, "a")
    pb = None if b is None else _cp_vector(b, n2, "b")
    if acc is not None:
        _chk(acc, "acc", 2)
        if tuple(acc.shape) != (n1, n2):
            raise ValueError("inconsistent shapes")
    if out is None:
        out = torch.empty((n1, n2), dtype=torch.float64, device=Ki.device)
    _chk(out, "out", 2)
    if tuple(out.shape) != (n1, n2):
        raise ValueError("inconsistent shapes")
    if n1 == 0 or n2 == 0:
        return out
    rc = lib.gpk_changepoint_fold(_stream(), 0 if acc is None else 1, pa, pb, n1, n2, Ki.data_ptr(), _rowmajor(Ki, "Ki"),
                                  None if acc is None else acc.data_ptr(), 0 if acc is None else _rowmajor(acc, "acc"), float(diag_add),
                                  out.data_ptr(), _rowmajor(out, "out"))
    _lib.check(rc, "gpk_changepoint_fold")
    return out


def changepoint_adjoint_parts(T: int, n1: int, n2: int, device_=None) -> torch.Tensor:
    """the scratch operand `parts` of changepoint_adjoint_stage / _tail for T members: [T, tc n1 + tr n2] doubles, tr / tc the tile
    rows / columns of CP_TILE (include/gpk.h: the documented extent per member); its contents at entry do not matter"""
    tr, tc = -(-int(n1) // CP_TILE), -(-int(n2) // CP_TILE)
    return torch.empty((int(T), tc * int(n1) + tr * int(n2)), dtype=torch.float64, device=device_ or device())


def changepoint_adjoint_stage(a: torch.Tensor, b: Optional[torch.Tensor], Kbar: torch.Tensor, Ki: torch.Tensor, parts: torch.Tensor, *,
                              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One pass over Kbar and Ki [n1, n2]: returns G = Kbar .* (a b^T) (`out` may be Ki itself; Kbar is never written) and fills
    `parts` (ONE member's row of changepoint_adjoint_parts) with the per-tile sums of Kbar Ki b_c (by row) and Kbar Ki a_r (by
    column).  b None: b is a, every element computed.  Deterministic: a second call gives the same bits."""
    lib = _lib.load()
    _chk(Kbar, "Kbar", 2)
    _chk(Ki, "Ki", 2)
    n1, n2 = Kbar.shape
    if tuple(Ki.shape) != (n1, n2) or (b is None and n1 != n2):
        raise ValueError("inconsistent shapes")
    pa = _cp_vector(a, n1, "a")
    pb = None if b is None else _cp_vector(b, n2, "b")
    _chk(parts, "parts", 1)
    tr, tc = -(-n1 // CP_TILE), -(-n2 // CP_TILE)
    if not parts.is_contiguous() or parts.numel() < tc * n1 + tr * n2:
        raise ValueError(f"changepoint_adjoint_stage: parts must be a contiguous [>= {tc * n1 + tr * n2}] (ops.changepoint_adjoint_parts)")
    if out is None:
        out = torch.empty((n1, n2), dtype=torch.float64, device=Kbar.device)
    _chk(out, "out", 2)
    if tuple(out.shape) != (n1, n2):
        raise ValueError("inconsistent shapes")
    if n1 == 0 or n2 == 0:
        return out
    rc = lib.gpk_changepoint_adjoint_stage(_stream(), pa, pb, n1, n2, Kbar.data_ptr(), _rowmajor(Kbar, "Kbar"), Ki.data_ptr(),
                                           _rowmajor(Ki, "Ki"), out.data_ptr(), _rowmajor(out, "out"), parts.data_ptr())
    _lib.check(rc, "gpk_changepoint_adjoint_stage")
    return out


def changepoint_adjoint_tail(x: torch.Tensor, *, locations, steepness, parts: Optional[torch.Tensor] = None, n_other: int = 0,
                             columns: bool = False, init: Optional[torch.Tensor] = None
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d/dlocations [C] (sorted order), d/dsteepness [C], xbar [n]) for ONE argument of the kernel with its switch column x [n].
    The weight adjoints are `init` [T, n] (None: zeros) plus the sums of the stage's partials: `parts` [T, tc n1 + tr n2]
    (ops.changepoint_adjoint_parts, every member's row filled by its stage call); columns False: x is the first argument (n = n1,
    n_other = n2), True: the second (n = n2, n_other = n1).  parts None: `init` alone (the diagonal path).  Fixed summation order: a
    second call is bit-identical."""
    lib = _lib.load()
    C, loc, st = _cp_points(locations, steepness)
    px, n, ldx = _cp_column(x, "x")
    dev = x.device
    small = torch.zeros(2 * C, dtype=torch.float64, device=dev)
    xbar = torch.zeros(n, dtype=torch.float64, device=dev)
    pp, stride, ntiles = None, 0, 0
    if parts is not None:
        _chk(parts, "parts", 2)
        n1, n2 = (int(n_other), n) if columns else (n, int(n_other))
        tr, tc = -(-n1 // CP_TILE), -(-n2 // CP_TILE)
        if not parts.is_contiguous() or parts.shape[0] != C + 1 or parts.shape[1] < tc * n1 + tr * n2:
            raise ValueError(f"changepoint_adjoint_tail: parts must be a contiguous [{C + 1}, >= {tc * n1 + tr * n2}]")
        stride, ntiles = int(parts.shape[1]), (tr if columns else tc)
        pp = parts.data_ptr() + (8 * tc * n1 if columns else 0)
    if init is not None:
        _chk(init, "init", 2)
        if tuple(init.shape) != (C + 1, n):
            raise ValueError(f"changepoint_adjoint_tail: init must be [{C + 1}, {n}]")
    if n == 0 or C == 0:
        return small[:C], small[C:], xbar
    red = torch.empty(-(-n // CP_TAIL_ROWS) * 2 * C, dtype=torch.float64, device=dev)
    rc = lib.gpk_changepoint_adjoint_tail(_stream(), px, n, ldx, C, loc, st, pp if ntiles else None, stride, ntiles,
                                          None if init is None else init.data_ptr(), 0 if init is None else _rowmajor(init, "init"),
                                          red.data_ptr(), small.data_ptr(), xbar.data_ptr())
    _lib.check(rc, "gpk_changepoint_adjoint_tail")
    return small[:C], small[C:], xbar


# ------------------------------------------------------------------------------------------------ Coregion kernel (coregion/coregion.hip)
COREGION_MAX_OUTPUTS, COREGION_MAX_RANK = 64, 64   # include/gpk.h: GPK_COREGION_MAX_OUTPUTS, GPK_COREGION_MAX_RANK
_coregion_cache: "collections.OrderedDict" = collections.OrderedDict()


def _cached(key, make):
    """a small device tensor found by the VALUES it was made from (as gradients.ls_device finds lengthscales): a host -> device copy
    from pageable memory blocks the host, so each set of values is uploaded, and B built, once"""
    t = _coregion_cache.get(key)
    if t is None:
        t = _coregion_cache[key] = make()
        while len(_coregion_cache) > 64:
            _coregion_cache.popitem(last=False)
    return t


def _coregion_host(W, kappa):
    """(W [P, R], kappa [P]) as contiguous host arrays, checked as CoregionLeaf checks them"""
    leaf = CoregionLeaf(W, kappa)
    return np.ascontiguousarray(leaf.W), np.ascontiguousarray(leaf.kappa)


def _coregion_on_device(a: np.ndarray, dev) -> torch.Tensor:
    return _cached(("host", a.shape, a.tobytes(), str(dev)), lambda: torch.as_tensor(a.copy(), device=dev))


def coregion_output_covariance(W, kappa, *, device_=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """B = W W^T + diag(kappa) [P, P] on the device from the HOST arrays W [P, R] and kappa [P], as a CoregionLeaf holds them
    (gpk_coregion_output_covariance: one workgroup, exactly symmetric, bit-identical when repeated).  Without `out` the result is
    cached by the values of (W, kappa): the first call costs two small uploads and the launch, a second call with the same values
    neither -- the caller must not write to it.  With `out` ([P, P], any leading dimension) the launch is made into it."""
    lib = _lib.load()
    Wh, kh = _coregion_host(W, kappa)
    P, R = Wh.shape
    dev = torch.device(device_) if device_ is not None else (out.device if out is not None else device())

    def build(B):
        Wd, kd = _coregion_on_device(Wh, dev), _coregion_on_device(kh, dev)
        rc = lib.gpk_coregion_output_covariance(_stream(), Wd.data_ptr(), R, kd.data_ptr(), P, R, B.data_ptr(), _rowmajor(B, "B"))
        _lib.check(rc, "gpk_coregion_output_covariance")
        return B
    if out is not None:
        _chk(out, "out", 2)
        if tuple(out.shape) != (P, P):
            raise ValueError(f"coregion_output_covariance: out must be [{P}, {P}]")
        return build(out)
    return _cached(("B", Wh.shape, Wh.tobytes(), kh.tobytes(), str(dev)),
                   lambda: build(torch.empty((P, P), dtype=torch.float64, device=dev)))


def _coregion_table(W, kappa, X):
    """what a Coregion leaf hands `_pair_builder` / `_row_diagonal` for `leaf()`: (pointer, leading dimension, P) of B on X's device"""
    B = coregion_output_covariance(W, kappa, device_=X.device)
    return B.data_ptr(), B.shape[1], B.shape[0]


def coregion_kernel_matrix(X1: torch.Tensor, X2: Optional[torch.Tensor], *, W, kappa, diag_add: float = 0.0, lower_only: bool = False,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K(X1, X2)[i, k] = B[l_i, l'_k] (or K(X1, X1) + diag_add I when X2 is None) -> [n1, n2] over the label columns X1 [n1, 1],
    X2 [n2, 1]; W [P, R], kappa [P] host arrays.  Exact: the bits of B; exactly symmetric; an invalid label (include/gpk.h) makes its row /
    column NaN."""
    return _pair_builder("gpk_coregion_kernel_matrix", X1, X2, None, out, None, None, partial(_coregion_table, W, kappa, X1),
                         diag_add, lower_only, _LABELS)


def coregion_kernel_matrix_combine(X1: torch.Tensor, X2: Optional[torch.Tensor], G: torch.Tensor, *, op: str, W, kappa,
                                   diag_add: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = G .* K(X1, X2) (op "mul") or G + K(X1, X2) (op "add"), K gathered on the fly; `out` may be G itself.  X2 None: K(X1, X1),
    `diag_add` goes onto the diagonal of the combined result."""
    _check_op("coregion_kernel_matrix_combine", op, ("mul", "add"))
    return _pair_builder("gpk_coregion_kernel_matrix_combine", X1, X2, G, out, op, _COREGION_OPS, partial(_coregion_table, W, kappa, X1),
                         diag_add, None, _LABELS)


def coregion_kernel_diag(X: torch.Tensor, g: Optional[torch.Tensor] = None, *, op: str = "k", W, kappa,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The row diagonal kd [n] = B[l_i, l_i] over the label column X [n, 1] (op "k"), or g .* kd ("mul"), g + kd ("add") with g [n];
    `out` may be g.  Read from B: bit for bit the diagonal of coregion_kernel_matrix(X, None)."""
    return _row_diagonal("gpk_coregion_kernel_diag", "coregion_kernel_diag", _COREGION_OPS, X, g, out, op,
                         partial(_coregion_table, W, kappa, X), _LABELS)


def coregion_onehot_rows(X: torch.Tensor, n_outputs: int) -> torch.Tensor:
    """E [P, n] with E[a, i] = 1 where the label of row i of X [n, 1] is a, else 0 (column i NaN for an invalid label): the right-hand
    side of the Coregion adjoint's contractions (gradients.coregion_kernel_adjoint), as moment_rows is for the dot-product kernels."""
    lib = _lib.load()
    _chk(X, "X", 2)
    n, d = X.shape
    P = int(n_outputs)
    if d != 1 or not 1 <= P <= COREGION_MAX_OUTPUTS:
        raise ValueError(f"coregion_onehot_rows: X must be one column of labels and n_outputs in 1 ... {COREGION_MAX_OUTPUTS}")
    E = torch.empty((P, n), dtype=torch.float64, device=X.device)
    if n == 0:
        return E
    rc = lib.gpk_coregion_onehot_rows(_stream(), X.data_ptr(), n, _rowmajor(X, "X"), P, E.data_ptr(), n)
    _lib.check(rc, "gpk_coregion_onehot_rows")
    return E


def coregion_adjoint_tail(Bbar: torch.Tensor, *, W) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d/dkappa [P] = diag(Bbar), d/dW [P, R] = (Bbar + Bbar^T) W) from Bbar [P, P] on the device and the host array W [P, R]
    (gpk_coregion_adjoint_tail: one workgroup, bit-identical when repeated)."""
    lib = _lib.load()
    _chk(Bbar, "Bbar", 2)
    Wh = np.ascontiguousarray(np.asarray(W, dtype=np.float64))
    if Wh.ndim != 2 or tuple(Bbar.shape) != (Wh.shape[0], Wh.shape[0]) or not 1 <= Wh.shape[0] <= COREGION_MAX_OUTPUTS \
            or not 1 <= Wh.shape[1] <= COREGION_MAX_RANK:
        raise ValueError("coregion_adjoint_tail: W must be [P, R] with P, R in 1 ... 64 and Bbar [P, P]")
    P, R = Wh.shape
    Wd = _coregion_on_device(Wh, Bbar.device)
    dW = torch.empty((P, R), dtype=torch.float64, device=Bbar.device)
    dk = torch.empty(P, dtype=torch.float64, device=Bbar.device)
    rc = lib.gpk_coregion_adjoint_tail(_stream(), Bbar.data_ptr(), _rowmajor(Bbar, "Bbar"), Wd.data_ptr(), R, P, R, dW.data_ptr(), R,
                                       dk.data_ptr())
    _lib.check(rc, "gpk_coregion_adjoint_tail")
    return dk, dW


def diag_add_(A: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """A[i,i] += v[i] in place (add_noise_cov with a per-row variance, utilities/model_utils.py:33-38) -- gpk_diag_add."""
    lib = _lib.load()
    _chk(A, "A", 2)
    v = to_device(v).reshape(-1).contiguous()
    n = min(A.shape[0], A.shape[1])
    if v.numel() != n:
        raise ValueError("diag_add_: one value per diagonal entry")
    _lib.check(lib.gpk_diag_add(_stream(), A.data_ptr(), n, _rowmajor(A, "A"), v.data_ptr()), "gpk_diag_add")
    return A


def invd_alloc(n: int, batch: int = 1) -> torch.Tensor:
    lib = _lib.load()
    return torch.empty(int(lib.gpk_invd_elems(n, batch)), dtype=torch.float64, device=device())


def potrf_(T: torch.Tensor, n: int, *, zero_upper: bool = False,
           invd: Optional[torch.Tensor] = None, identity_rows: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """In-place trapezoidal Cholesky of T [(n+extra), n] or batched [b, (n+extra), n].
    Returns (invd, info) -- info is a device int32 tensor (0 ok, j+1 first bad pivot).

    identity_rows=True (2-D only): the LAST n rows of T are overwritten with the identity by the library and come back
    as L^-T at a third of the cost of n dense rows (gpk_potrf_inv) -- the caller leaves them uninitialised."""
    lib = _lib.load()
    _chk(T, "T")
    if T.dim() == 2:
        batch, rows, cols, stride = 1, T.shape[0], T.shape[1], 0
        lda = _rowmajor(T, "T")
    elif T.dim() == 3:
        batch, rows, cols = T.shape
        stride = int(T.stride(0))
        lda = _rowmajor(T[0], "T")
    else:
        raise ValueError("T must be 2-D or 3-D")
    if cols != n or rows < n:
        raise ValueError(f"T has shape {tuple(T.shape)}, expected [.., n+extra, n] with n={n}")
    if invd is None:
        invd = invd_alloc(n, batch)
    info = torch.zeros(batch, dtype=torch.int32, device=T.device)
    if identity_rows:
        if T.dim() != 2 or rows < 2 * n:
            raise ValueError("identity_rows needs a 2-D T with at least 2 n rows")
        rc = lib.gpk_potrf_inv(_stream(), T.data_ptr(), n, rows - 2 * n, lda, invd.data_ptr(), int(zero_upper),
                               info.data_ptr())
        _lib.check(rc, "gpk_potrf_inv")
        return invd, info
    rc = lib.gpk_potrf(_stream(), T.data_ptr(), n, rows - n, lda, batch, stride, invd.data_ptr(),
                       int(zero_upper), info.data_ptr())
    _lib.check(rc, "gpk_potrf")
    return invd, info


def check_info(info: torch.Tensor, what: str = "Cholesky") -> None:
    """Synchronising check of the factorisation status (the reference raises InvalidArgumentError
    'Cholesky decomposition was not successful' from tf.linalg.cholesky on CPU)."""
    bad = info.cpu().numpy()
    if np.any(bad != 0):
        j = int(bad[np.nonzero(bad)[0][0]])
        if j >= INFO_HANDOFF_TIMEOUT:   # include/gpk.h, "info": an internal stream hand-off of the factorisation timed out
            raise _lib.GpkError(f"{what} decomposition failed: an internal stream hand-off timed out (status INT_MAX); "
                                "the result is undefined")
        raise _lib.GpkError(f"{what} decomposition was not successful: non-positive pivot at column {j - 1}")


def trtri_blocks(L: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _chk(L, "L", 2)
    n = L.shape[0]
    invd = invd_alloc(n, 1)
    rc = lib.gpk_trtri_blocks(_stream(), L.data_ptr(), n, _rowmajor(L, "L"), 1, 0, invd.data_ptr())
    _lib.check(rc, "gpk_trtri_blocks")
    return invd


def transpose_factor(L: torch.Tensor, invd: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    lib = _lib.load()
    _chk(L, "L", 2)
    n = L.shape[0]
    LT = torch.empty((n, n), dtype=torch.float64, device=L.device)
    invdT = torch.empty_like(invd)
    rc = lib.gpk_transpose_factor(_stream(), L.data_ptr(), _rowmajor(L, "L"), invd.data_ptr(), n,
                                  LT.data_ptr(), n, invdT.data_ptr())
    _lib.check(rc, "gpk_transpose_factor")
    return LT, invdT


def trsm_(B: torch.Tensor, L: torch.Tensor, invd: torch.Tensor, *, trans: int = 0) -> torch.Tensor:
    """In place: trans=0  B <- B L^-T (pass L, invd);  trans=1  B <- B L^-1 (pass LT, invdT)."""
    lib = _lib.load()
    _chk(B, "B", 2)
    _chk(L, "L", 2)
    n = L.shape[0]
    if B.shape[1] != n:
        raise ValueError(f"B has {B.shape[1]} columns, factor is {n}x{n}")
    rc = lib.gpk_trsm(_stream(), int(trans), L.data_ptr(), _rowmajor(L, "L"), invd.data_ptr(), n,
                      B.data_ptr(), B.shape[0], _rowmajor(B, "B"), 1, 0, 0)
    _lib.check(rc, "gpk_trsm")
    return B


def gemm_nt(A: torch.Tensor, B: torch.Tensor, *, alpha: float = 1.0, beta: float = 0.0,
            C: Optional[torch.Tensor] = None, b_tri: int = 0, c_lower: bool = False, a_tri: int = 0,
            k_split: bool = False, zero_skipped: bool = True) -> torch.Tensor:
    """C = alpha A B^T + beta C.  A [m,k] or [b,m,k]; B [n,k] or [b,n,k].  b_tri: 1 B upper (B[j,kk] = 0 for kk < j),
    2 B lower; a_tri: the same statement about A (1 upper, 2 lower) -- zeros must be stored; only the K ranges shrink.
    k_split: the batch entries are consecutive K chunks of ONE triangular product (strided views of its operands); b_tri / a_tri
    then refer to the unsplit column index and the caller sums the partial products (combine_parts).
    c_lower without C: the tiles above the diagonal, which the kernel skips, are zero-filled first -- unless zero_skipped=False (a caller
    that never reads them, e.g. combine_parts(lower=True) behind a split-K product: the fill of 8 x 2048^2 partials was 72 us)."""
    lib = _lib.load()
    _chk(A, "A")
    _chk(B, "B")
    batched = A.dim() == 3 or B.dim() == 3
    A3 = A if A.dim() == 3 else A.unsqueeze(0)
    B3 = B if B.dim() == 3 else B.unsqueeze(0)
    batch = max(A3.shape[0], B3.shape[0])
    m, k = A3.shape[1], A3.shape[2]
    n = B3.shape[1]
    if B3.shape[2] != k:
        raise ValueError("inner dimensions differ")
    if C is None:
        if beta != 0.0:
            raise ValueError("beta != 0 needs C")
        C = torch.empty((batch, m, n) if batched else (m, n), dtype=torch.float64, device=A.device)
        if c_lower and zero_skipped:
            C.zero_()
    C3 = C if C.dim() == 3 else C.unsqueeze(0)
    sA = int(A3.stride(0)) if A3.shape[0] > 1 else 0
    sB = int(B3.stride(0)) if B3.shape[0] > 1 else 0
    sC = int(C3.stride(0)) if C3.shape[0] > 1 else 0
    rc = lib.gpk_gemm_nt(_stream(), m, n, k, float(alpha), A3.data_ptr(), _rowmajor(A3[0], "A"),
                         B3.data_ptr(), _rowmajor(B3[0], "B"), float(beta), C3.data_ptr(),
                         _rowmajor(C3[0], "C"), int(b_tri) | (int(a_tri) << 4) | (0x100 if k_split else 0), int(c_lower), batch, sA, sB, sC)
    _lib.check(rc, "gpk_gemm_nt")
    return C


def transpose(X: torch.Tensor, *, mode: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[.., j, i] = X[.., i, j]; mode 1 keeps only the lower triangle of X, 2 only the upper."""
    lib = _lib.load()
    _chk(X, "X")
    X3 = X if X.dim() == 3 else X.unsqueeze(0)
    b, r, c = X3.shape
    if out is None:
        out = torch.empty((b, c, r) if X.dim() == 3 else (c, r), dtype=torch.float64, device=X.device)
    O3 = out if out.dim() == 3 else out.unsqueeze(0)
    rc = lib.gpk_transpose(_stream(), X3.data_ptr(), r, c, _rowmajor(X3[0], "X"), O3.data_ptr(),
                           _rowmajor(O3[0], "out"), int(mode), b,
                           int(X3.stride(0)) if b > 1 else 0, int(O3.stride(0)) if b > 1 else 0)
    _lib.check(rc, "gpk_transpose")
    return out


def row_stats(At: torch.Tensor, *, V: Optional[torch.Tensor] = None, W: Optional[torch.Tensor] = None,
              want_sumsq: bool = True):
    """(sumsq [rows], mv [rows,P] = At V, wsq [P,rows] = sum_k (At W)^2) -- any may be None."""
    lib = _lib.load()
    _chk(At, "At", 2)
    rows, m = At.shape
    P = 0
    for name, t in (("V", V), ("W", W)):
        if t is not None:
            _chk(t, name, 2)
            if t.shape[0] != m or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous [m, P]")
            P = t.shape[1]
    sumsq = torch.empty(rows, dtype=torch.float64, device=At.device) if want_sumsq else None
    mv = torch.empty((rows, P), dtype=torch.float64, device=At.device) if V is not None else None
    wsq = torch.empty((P, rows), dtype=torch.float64, device=At.device) if W is not None else None
    rc = lib.gpk_row_stats(_stream(), At.data_ptr(), rows, m, _rowmajor(At, "At"),
                           V.data_ptr() if V is not None else None,
                           W.data_ptr() if W is not None else None, P, 1.0, 0.0,
                           sumsq.data_ptr() if sumsq is not None else None,
                           mv.data_ptr() if mv is not None else None,
                           wsq.data_ptr() if wsq is not None else None)
    _lib.check(rc, "gpk_row_stats")
    return sumsq, mv, wsq


def row_dot(A: torch.Tensor, B: torch.Tensor) -> torch.Tensor:
    """out[i] = sum_j A[i,j] B[i,j]"""
    lib = _lib.load()
    _chk(A, "A", 2)
    _chk(B, "B", 2)
    if A.shape != B.shape:
        raise ValueError("shape mismatch")
    out = torch.empty(A.shape[0], dtype=torch.float64, device=A.device)
    rc = lib.gpk_row_dot(_stream(), A.data_ptr(), _rowmajor(A, "A"), B.data_ptr(), _rowmajor(B, "B"),
                         A.shape[0], A.shape[1], 1.0, 0.0, out.data_ptr())
    _lib.check(rc, "gpk_row_dot")
    return out


def project(At: torch.Tensor, LqT: torch.Tensor) -> torch.Tensor:
    """ssq [P, rows] = sum_j (At_p Lq_p)[b, j]^2 with LqT [P, m, m] = tril(q_sqrt_p)^T.  At [rows, m]: one matrix shared by
    the P latents; At [P, rows, m] (any batch stride, unit column stride): one per latent (SeparateIndependent)."""
    lib = _lib.load()
    _chk(LqT, "LqT", 3)
    P = LqT.shape[0]
    if At.dim() == 3:
        if At.dtype != torch.float64 or At.shape[0] != P or At.stride(2) != 1:
            raise ValueError("batched At must be float64 [P, rows, m] with unit column stride")
        rows, m = At.shape[1], At.shape[2]
        ldat, stride_at = At.stride(1), At.stride(0)
    else:
        _chk(At, "At", 2)
        rows, m = At.shape
        ldat, stride_at = _rowmajor(At, "At"), 0
    if LqT.shape[1] != m or LqT.shape[2] != m or not LqT.is_contiguous():
        raise ValueError("LqT must be contiguous [P, m, m]")
    ssq = torch.empty((P, rows), dtype=torch.float64, device=At.device)
    nbytes = int(lib.gpk_project_workspace_bytes(rows, m, P))
    ws = _ws(nbytes)
    rc = lib.gpk_project_batched(_stream(), At.data_ptr(), rows, m, ldat, stride_at, LqT.data_ptr(), m, P,
                                 ssq.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_project_batched")
    return ssq


def project_stats(At: torch.Tensor, LqT: torch.Tensor, V: torch.Tensor):
    """(s0 [rows], fmean [rows, P] = At V, ssq [P, rows]): `project` and the row statistics of the same At [rows, m] in one
    driver call, as the fused SVGP step takes them (gpk_project_stats)."""
    lib = _lib.load()
    _chk(At, "At", 2)
    _chk(LqT, "LqT", 3)
    _chk(V, "V", 2)
    rows, m = At.shape
    P = LqT.shape[0]
    if LqT.shape[1] != m or LqT.shape[2] != m or not LqT.is_contiguous():
        raise ValueError("LqT must be contiguous [P, m, m]")
    if V.shape != (m, P) or not V.is_contiguous():
        raise ValueError("V must be contiguous [m, P]")
    s0 = torch.empty(rows, dtype=torch.float64, device=At.device)
    fmean = torch.empty((rows, P), dtype=torch.float64, device=At.device)
    ssq = torch.empty((P, rows), dtype=torch.float64, device=At.device)
    ws = _ws(int(lib.gpk_project_workspace_bytes(rows, m, P)))
    rc = lib.gpk_project_stats(_stream(), At.data_ptr(), rows, m, _rowmajor(At, "At"), LqT.data_ptr(), m, P, V.data_ptr(),
                               s0.data_ptr(), fmean.data_ptr(), ssq.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_project_stats")
    return s0, fmean, ssq


TRIL_TILE = 128   # include/gpk.h: GPK_TRIL_TILE


def tril_product_parts(n: int, R: int, device_=None) -> torch.Tensor:
    """the scratch operand `parts` [R, tiles, n] of tril_product (include/gpk.h: gpk_tril_product; contents at entry do not matter)"""
    lib = _lib.load()
    return torch.empty((R, int(lib.gpk_tril_product_tiles(int(n))), n), dtype=torch.float64, device=device_ or device())


def tril_product(L: torch.Tensor, S: torch.Tensor, *, rowscale: Optional[torch.Tensor] = None, want_ssq: bool = True,
                 want_product: bool = False, parts: Optional[torch.Tensor] = None, product_out: Optional[torch.Tensor] = None):
    """(ssq [R, n] | None, T [R, n, n] | None) of the product of lower-triangular matrices P_r = tril(L) tril(S_r), L [n, n], S [R, n, n]
    (any leading dimension and batch stride, unit column stride; nothing above either diagonal is read): ssq[r, i] = sum_j P_r[i, j]^2
    without storing the product -- the marginal variances of the VGP's q(f) -- and / or T_r = diag(rowscale[r]) P_r (rowscale [R, n],
    None: ones) below the diagonal: the seed of its reverse pass.  A fresh T is zero above the diagonal; `product_out` [R, n, >= n] is
    written on and below the diagonal only.  parts: the scratch [R, tiles, n] (tril_product_parts), allocated when None."""
    lib = _lib.load()
    _chk(L, "L", 2)
    _chk(S, "S", 3)
    n = L.shape[0]
    R = S.shape[0]
    if L.shape[1] < n or S.shape[1] != n or S.shape[2] < n:
        raise ValueError(f"tril_product: L must be [n, n] and S [R, n, n], got {tuple(L.shape)} and {tuple(S.shape)}")
    if S.numel() and n > 1 and S.stride(2) != 1:
        raise _lib.GpkError("S: last dimension must be contiguous")
    want_product = want_product or product_out is not None
    if not (want_ssq or want_product):
        raise ValueError("tril_product: neither the row sums nor the product was asked for")
    if rowscale is not None:
        _chk(rowscale, "rowscale", 2)
        if not want_product or tuple(rowscale.shape) != (R, n) or not rowscale.is_contiguous():
            raise ValueError("tril_product: rowscale is a contiguous [R, n] and goes with the stored product")
    ssq = torch.empty((R, n), dtype=torch.float64, device=L.device) if want_ssq else None
    if want_ssq:
        if parts is None:
            parts = tril_product_parts(n, R, L.device)
        _chk(parts, "parts", 3)
        if tuple(parts.shape) != (R, int(lib.gpk_tril_product_tiles(n)), n) or not parts.is_contiguous():
            raise ValueError("tril_product: parts must be a contiguous [R, tiles, n]")
    T = None
    if want_product:
        T = product_out if product_out is not None else torch.zeros((R, n, n), dtype=torch.float64, device=L.device)
        _chk(T, "product_out", 3)
        if T.shape[0] != R or T.shape[1] != n or T.shape[2] < n or (T.numel() and n > 1 and T.stride(2) != 1):
            raise ValueError("tril_product: product_out must be [R, n, >= n] with unit column stride")
    if n == 0 or R == 0:
        return ssq, T
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.gpk_tril_product(_stream(), L.data_ptr(), n, _rowmajor(L, "L"), S.data_ptr(), _rowmajor(S[0], "S"),
                              int(S.stride(0)) if R > 1 else 0, R, ptr(ssq), ptr(parts) if want_ssq else None, ptr(rowscale), ptr(T),
                              _rowmajor(T[0], "product_out") if T is not None else 0, int(T.stride(0)) if T is not None and R > 1 else 0)
    _lib.check(rc, "gpk_tril_product")
    return ssq, T


def gaussian_varexp_sum(Y: torch.Tensor, fmean: torch.Tensor, *, s0: Optional[torch.Tensor],
                        ssq: Optional[torch.Tensor], knn: Sequence[float], noise_variance,
                        mean_const: float = 0.0, s0_per_latent: bool = False, want_fvar: bool = False):
    """Sum over rows/outputs of the Gaussian variational expectations; returns (scalar tensor, fvar|None).
    noise_variance: a float, or one variance per row [rows] (heteroskedastic likelihood)."""
    lib = _lib.load()
    _chk(Y, "Y", 2)
    _chk(fmean, "fmean", 2)
    rows, P = fmean.shape
    if not fmean.is_contiguous():
        raise ValueError("fmean must be contiguous")
    out = torch.empty(1, dtype=torch.float64, device=Y.device)
    fvar = torch.empty((rows, P), dtype=torch.float64, device=Y.device) if want_fvar else None
    ws = _ws(int(lib.gpk_reduce_workspace_bytes(rows)))
    knn = list(np.atleast_1d(np.asarray(knn, dtype=np.float64)))
    per = int(len(knn) > 1)
    nv, nv_rows, _keep = _noise_args(noise_variance, rows)
    rc = lib.gpk_gaussian_varexp_sum(_stream(), Y.data_ptr(), _rowmajor(Y, "Y"), fmean.data_ptr(), rows, P,
                                     s0.data_ptr() if s0 is not None else None, int(s0_per_latent),
                                     ssq.data_ptr() if ssq is not None else None,
                                     _lib.host_doubles(knn), per, nv, nv_rows, float(mean_const),
                                     fvar.data_ptr() if fvar is not None else None, out.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_gaussian_varexp_sum")
    return out, fvar


LIKELIHOOD_CODES = {"bernoulli_probit": 1, "poisson_exp": 2, "student_t": 3, "multiclass_robustmax": 4,   # include/gpk.h: GPK_LIK_*
                    "exponential_exp": 8, "gamma_exp": 9, "beta_probit": 10, "ordinal": 11}               # (5 - 7: unassigned)
_LIKELIHOOD_NPAR = {"bernoulli_probit": 0, "poisson_exp": 1, "student_t": 2, "multiclass_robustmax": 1,
                    "exponential_exp": 0, "gamma_exp": 1, "beta_probit": 1}   # ("ordinal": see _lik_npar)
ROW_LIKELIHOODS = ("multiclass_robustmax",)   # the latents of a row are coupled: Y is ONE column of labels, P >= 2 classes
ORDINAL_MAX_EDGES = 15


def _lik_npar(lik: str, params) -> int:
    """how many parameters the code takes: a fixed count, or for "ordinal" (sigma, n, e_0 .. e_{n-1}) the 2 + n its own second
    entry announces (n an integer in 1 .. ORDINAL_MAX_EDGES; -1, which no length equals, when it is not)"""
    if lik != "ordinal":
        return _LIKELIHOOD_NPAR[lik]
    if len(params) < 2 or not (params[1] == int(params[1]) if np.isfinite(params[1]) else False) \
            or not 1 <= int(params[1]) <= ORDINAL_MAX_EDGES:
        return -1
    return 2 + int(params[1])


def _lik_args(lik: str, params):
    """(code, host array | None) of the (lik, lik_params_host) pair of the C-ABI: params is () for "bernoulli_probit" and
    "exponential_exp", (binsize,) for "poisson_exp", (scale, df) for "student_t", (epsilon,) for "multiclass_robustmax", (shape,) for
    "gamma_exp", (scale,) for "beta_probit", (sigma, n, e_0, ..., e_{n-1}) for "ordinal" (n <= 15 bin edges).  The VALUES are the
    library's to judge (GPK_E_ARG)."""
    if lik not in LIKELIHOOD_CODES:
        raise ValueError(f"unknown likelihood {lik!r}: one of {sorted(LIKELIHOOD_CODES)}")
    params = [float(v) for v in params]
    if len(params) != _lik_npar(lik, params):
        raise ValueError(f"likelihood {lik!r}: wrong number of parameters ({len(params)})")
    return LIKELIHOOD_CODES[lik], (_lib.host_doubles(params) if params else None)


def _lik_y_columns(lik: str, P: int) -> int:
    """how many columns of Y the likelihood reads: P, or one label column for a ROW_LIKELIHOODS member (which needs P >= 2 classes)"""
    if lik not in ROW_LIKELIHOODS:
        return P
    if P < 2:
        raise ValueError(f"likelihood {lik!r} needs at least two classes (P = {P})")
    return 1


def _mixing_weights(W, L: int):
    """W [P, L] as a host array for the (W_host) argument of the C-ABI; 1 <= L, P <= 16 (include/gpk.h)."""
    Wh = np.ascontiguousarray(W.detach().cpu().numpy() if isinstance(W, torch.Tensor) else np.asarray(W, dtype=np.float64),
                              dtype=np.float64)
    if Wh.ndim != 2 or Wh.shape[1] != L:
        raise ValueError(f"W must be [P, L] with L = {L} latents, got shape {tuple(Wh.shape)}")
    if not (1 <= L <= 16 and 1 <= Wh.shape[0] <= 16):
        raise ValueError(f"mixing of L = {L} latents into P = {Wh.shape[0]} outputs: both must lie in [1, 16]")
    return Wh


def mixed_gaussian_varexp_sum(Y: torch.Tensor, gmean: torch.Tensor, W, *, s0: Optional[torch.Tensor], ssq: Optional[torch.Tensor],
                              knn: Sequence[float], noise_variance: float, mean_const: float = 0.0, s0_per_latent: bool = False,
                              want_moments: bool = False, want_grads: bool = False):
    """Gaussian variational expectations of linearly mixed latents (gpk_mixed_gaussian_varexp_sum): f = gmean W^T + mean_const,
    fvar = gvar (W^2)^T with gvar = knn - s0 + ssq over the L latents; Y [rows, P], gmean [rows, L], W [P, L] (host or device).
    Returns (out [2], fmean | None, fvar | None, dgmu | None, dW | None): out[0] = sum over rows and outputs, out[1] = its
    derivative w.r.t. the noise variance; fmean, fvar [rows, P] (want_moments); dgmu [rows, L] = d out[0] / d gmean and
    dW [P, L] = d out[0] / d W (want_grads)."""
    lib = _lib.load()
    _chk(Y, "Y", 2)
    _chk(gmean, "gmean", 2)
    rows, L = gmean.shape
    if not gmean.is_contiguous():
        raise ValueError("gmean must be contiguous")
    Wh = _mixing_weights(W, L)
    P = Wh.shape[0]
    if Y.shape[0] != rows or Y.shape[1] < P:
        raise ValueError("Y must have one row per row of gmean and at least P columns")
    for name, t, shape in (("s0", s0, (L, rows) if s0_per_latent else (rows,)), ("ssq", ssq, (L, rows))):
        if t is not None:
            _chk(t, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous {shape}")
    if not float(noise_variance) > 0.0:
        raise ValueError("noise_variance must be positive")

    def new(*shape):
        return torch.empty(shape, dtype=torch.float64, device=Y.device)
    out = new(2)
    fmean, fvar = (new(rows, P), new(rows, P)) if want_moments else (None, None)
    dgmu, dW = (new(rows, L), new(P, L)) if want_grads else (None, None)
    ws = _ws(int(lib.gpk_mixed_varexp_workspace_bytes(rows, L, P)))
    knn = list(np.atleast_1d(np.asarray(knn, dtype=np.float64)))
    if len(knn) not in (1, L):
        raise ValueError(f"knn: one value, or one per latent ({L})")
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.gpk_mixed_gaussian_varexp_sum(_stream(), Y.data_ptr(), _rowmajor(Y, "Y"), gmean.data_ptr(), rows, L, P,
                                           _lib.host_doubles(Wh.reshape(-1).tolist()), ptr(s0), int(s0_per_latent), ptr(ssq),
                                           _lib.host_doubles(knn), int(len(knn) > 1), float(noise_variance), float(mean_const),
                                           ptr(fmean), ptr(fvar), ptr(dgmu), ptr(dW), out.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_mixed_gaussian_varexp_sum")
    return out, fmean, fvar, dgmu, dW


def gauss_hermite(n: int = 20) -> Tuple[np.ndarray, np.ndarray]:
    """(x [n], w [n]) = numpy.polynomial.hermite.hermgauss(n) as the kernels hold it (gpk_gauss_hermite; host only, n = 20)."""
    lib = _lib.load()
    x, w = (_lib.c_double * int(n))(), (_lib.c_double * int(n))()
    _lib.check(lib.gpk_gauss_hermite(int(n), x, w), "gpk_gauss_hermite")
    return np.array(x, dtype=np.float64), np.array(w, dtype=np.float64)


def likelihood_varexp_sum(Y: torch.Tensor, fmean: torch.Tensor, *, s0: Optional[torch.Tensor], ssq: Optional[torch.Tensor],
                          knn: Sequence[float], lik: str, params=(), mean_const: float = 0.0, s0_per_latent: bool = False,
                          want_fvar: bool = False, want_rows: bool = False, want_grads: bool = False):
    """Gauss-Hermite variational expectations of a non-Gaussian scalar likelihood (gpk_likelihood_varexp_sum), fvar = knn - s0 + ssq.
    Returns (out [2], rows | None, dmu | None, dvar | None, fvar | None): out[0] = sum over rows and outputs, out[1] = its
    derivative w.r.t. the code's one trainable parameter (StudentT scale, Gamma shape, Beta scale, Ordinal sigma; 0 otherwise); rows [rows] = sums over the outputs; dmu, dvar [rows, P] = d/dfmean,
    d/dfvar of every term.  "multiclass_robustmax" (params = (epsilon,)): Y is ONE column of class labels, the P >= 2 latents of a
    row are its classes, rows [rows] is the row's value and dmu, dvar its derivatives w.r.t. all P means and variances."""
    lib = _lib.load()
    _chk(Y, "Y", 2)
    _chk(fmean, "fmean", 2)
    rows, P = fmean.shape
    if not fmean.is_contiguous():
        raise ValueError("fmean must be contiguous")
    if Y.shape[0] != rows or Y.shape[1] < _lik_y_columns(lik, P):
        raise ValueError("Y must have one row per row of fmean and at least P columns (one label column for 'multiclass_robustmax')")
    for name, t, shape in (("s0", s0, (P, rows) if s0_per_latent else (rows,)), ("ssq", ssq, (P, rows))):
        if t is not None:
            _chk(t, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous {shape}")
    code, par = _lik_args(lik, params)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float64, device=Y.device)
    out = new(2)
    fvar = new(rows, P) if want_fvar else None
    rws = new(rows) if want_rows else None
    dmu, dvar = (new(rows, P), new(rows, P)) if want_grads else (None, None)
    ws = _ws(int(lib.gpk_reduce_workspace_bytes(rows)))
    knn = list(np.atleast_1d(np.asarray(knn, dtype=np.float64)))
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.gpk_likelihood_varexp_sum(_stream(), code, par, Y.data_ptr(), _rowmajor(Y, "Y"), fmean.data_ptr(), rows, P,
                                       ptr(s0), int(s0_per_latent), ptr(ssq), _lib.host_doubles(knn), int(len(knn) > 1),
                                       float(mean_const), ptr(fvar), ptr(rws), ptr(dmu), ptr(dvar), out.data_ptr(),
                                       ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_likelihood_varexp_sum")
    return out, rws, dmu, dvar, fvar


# the members of a switched likelihood's table (gpk_switched_varexp_sum): there, and only there, code 0 is a Gaussian with params =
# (variance,); the others are the scalar codes of LIKELIHOOD_CODES without "ordinal" (an edge table per task)
SWITCHED_MEMBERS = {"gaussian": 0, **{name: LIKELIHOOD_CODES[name] for name in
                                      ("bernoulli_probit", "poisson_exp", "student_t", "exponential_exp", "gamma_exp", "beta_probit")}}
SWITCHED_MAX_TASKS = 16


def _switched_table(members):
    """(T, codes, params [T][2]) as host arrays from a sequence of (name, params): the VALUES are the library's to judge"""
    members = list(members)
    if not 1 <= len(members) <= SWITCHED_MAX_TASKS:
        raise ValueError(f"a switched likelihood takes 1 .. {SWITCHED_MAX_TASKS} members, got {len(members)}")
    codes, flat = [], []
    for name, params in members:
        if name not in SWITCHED_MEMBERS:
            raise ValueError(f"unknown member {name!r} of a switched likelihood: one of {sorted(SWITCHED_MEMBERS)}")
        params = [float(v) for v in params]
        if len(params) != (1 if name == "gaussian" else _LIKELIHOOD_NPAR[name]):
            raise ValueError(f"switched likelihood member {name!r}: wrong number of parameters ({len(params)})")
        codes.append(SWITCHED_MEMBERS[name])
        flat += (params + [0.0, 0.0])[:2]
    return len(members), (_lib.c_int * len(codes))(*codes), _lib.host_doubles(flat)


def switched_varexp_sum(Y: torch.Tensor, fmean: torch.Tensor, *, s0: Optional[torch.Tensor], ssq: Optional[torch.Tensor],
                        knn: Sequence[float], members, ylab: Optional[int] = None, mean_const: float = 0.0,
                        s0_per_latent: bool = False, want_fvar: bool = False, want_rows: bool = False, want_grads: bool = False):
    """Variational expectations of a switched likelihood (gpk_switched_varexp_sum): row b is scored by members[t], t the task label in
    column `ylab` of Y (default: the last), read as the Coregion kernel reads a label; the values are Y[:, :P].  members: a sequence
    of (name, params), name in SWITCHED_MEMBERS ("gaussian": params = (variance,)).  Returns (out [1 + T], rows | None, dmu | None,
    dvar | None, fvar | None): out[0] = the sum over rows and outputs, out[1 + t] = its derivative w.r.t. member t's one trainable
    parameter (Gaussian variance, StudentT scale, Gamma shape, Beta scale; 0 otherwise, and for a task without rows); a row with an
    invalid label is NaN in rows, dmu, dvar and out[0]."""
    lib = _lib.load()
    _chk(Y, "Y", 2)
    _chk(fmean, "fmean", 2)
    rows, P = fmean.shape
    if not fmean.is_contiguous():
        raise ValueError("fmean must be contiguous")
    ylab = Y.shape[1] - 1 if ylab is None else int(ylab)
    if Y.shape[0] != rows or not P <= ylab < Y.shape[1]:
        raise ValueError("Y must have one row per row of fmean, P value columns and the label column `ylab` behind them")
    for name, t, shape in (("s0", s0, (P, rows) if s0_per_latent else (rows,)), ("ssq", ssq, (P, rows))):
        if t is not None:
            _chk(t, name)
            if tuple(t.shape) != shape or not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous {shape}")
    T, codes, par = _switched_table(members)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float64, device=Y.device)
    out = new(1 + T)
    fvar = new(rows, P) if want_fvar else None
    rws = new(rows) if want_rows else None
    dmu, dvar = (new(rows, P), new(rows, P)) if want_grads else (None, None)
    parts = new((1 + T) * int(lib.gpk_switched_varexp_blocks(rows, P)))
    knn = list(np.atleast_1d(np.asarray(knn, dtype=np.float64)))
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    rc = lib.gpk_switched_varexp_sum(_stream(), T, codes, par, Y.data_ptr(), _rowmajor(Y, "Y"), ylab, fmean.data_ptr(), rows, P,
                                     ptr(s0), int(s0_per_latent), ptr(ssq), _lib.host_doubles(knn), int(len(knn) > 1),
                                     float(mean_const), ptr(fvar), ptr(rws), ptr(dmu), ptr(dvar), out.data_ptr(), parts.data_ptr())
    _lib.check(rc, "gpk_switched_varexp_sum")
    return out, rws, dmu, dvar, fvar


def gauss_kl_white(q_mu: torch.Tensor, q_sqrt: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    _chk(q_mu, "q_mu", 2)
    _chk(q_sqrt, "q_sqrt")
    m, P = q_mu.shape
    q_diag = int(q_sqrt.dim() == 2)
    if not (q_mu.is_contiguous() and q_sqrt.is_contiguous()):
        raise ValueError("q_mu / q_sqrt must be contiguous")
    out = torch.empty(1, dtype=torch.float64, device=q_mu.device)
    ws = _ws(int(lib.gpk_reduce_workspace_bytes(m)))
    rc = lib.gpk_gauss_kl_white(_stream(), q_mu.data_ptr(), q_sqrt.data_ptr(), m, P, q_diag,
                                out.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_gauss_kl_white")
    return out


def sum_log_diag(L: torch.Tensor) -> torch.Tensor:
    """sum_i log L[i,i] for L [n,>=n] or batched [b,n,>=n] -> [b]."""
    lib = _lib.load()
    _chk(L, "L")
    L3 = L if L.dim() == 3 else L.unsqueeze(0)
    b = L3.shape[0]
    n = min(L3.shape[1], L3.shape[2])
    out = torch.empty(b, dtype=torch.float64, device=L.device)
    rc = lib.gpk_sum_log_diag(_stream(), L3.data_ptr(), n, _rowmajor(L3[0], "L"), b,
                              int(L3.stride(0)) if b > 1 else 0, out.data_ptr())
    _lib.check(rc, "gpk_sum_log_diag")
    return out


def combine_parts(parts: torch.Tensor, *, alpha: float = 1.0, lower: bool = False, diag_scale: float = 1.0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """alpha * sum_p parts[p] for parts [np, m, n] (or [m, n]: one part), summed in the order p = 0, 1, ...; with
    lower=True the result is lower-triangular (zeros above the diagonal, which is never read -- a lower-only GEMM leaves
    those tiles unwritten) and its diagonal is multiplied by diag_scale (0.5: the Phi of the Cholesky adjoint)."""
    lib = _lib.load()
    _chk(parts, "parts")
    p3 = parts if parts.dim() == 3 else parts.unsqueeze(0)
    if p3.dim() != 3:
        raise ValueError("parts must be [np, m, n] or [m, n]")
    npart, m, n = p3.shape
    ldp = _rowmajor(p3[0], "parts")
    stride = int(p3.stride(0)) if npart > 1 else 0
    if out is None:
        out = torch.empty((m, n), dtype=torch.float64, device=parts.device)
    _chk(out, "out", 2)
    rc = lib.gpk_combine_parts(_stream(), p3.data_ptr(), npart, stride, m, n, ldp, float(alpha), int(lower),
                               float(diag_scale), out.data_ptr(), _rowmajor(out, "out"))
    _lib.check(rc, "gpk_combine_parts")
    return out


def sumsq(A: torch.Tensor, *, upper_only: bool = False) -> torch.Tensor:
    lib = _lib.load()
    _chk(A, "A", 2)
    out = torch.empty(1, dtype=torch.float64, device=A.device)
    ws = _ws(int(lib.gpk_reduce_workspace_bytes(A.shape[0])))
    rc = lib.gpk_sumsq(_stream(), A.data_ptr(), A.shape[0], A.shape[1], _rowmajor(A, "A"), int(upper_only),
                       out.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_sumsq")
    return out


# ------------------------------------------------------------------------------------------------ reverse-pass glue
def moment_rows(B: torch.Tensor) -> torch.Tensor:
    """[1; B^T; (B^T)^2] as [1 + 2 D, n2] for B [n2, D]: the right-hand side of G [1, B, B^2] (gradients.stationary_kernel_adjoint)."""
    lib = _lib.load()
    _chk(B, "B", 2)
    n2, d = B.shape
    Vt = torch.empty((1 + 2 * d, n2), dtype=torch.float64, device=B.device)
    rc = lib.gpk_moment_rows(_stream(), B.data_ptr(), _rowmajor(B, "B"), n2, d, Vt.data_ptr(), n2)
    _lib.check(rc, "gpk_moment_rows")
    return Vt


def stationary_adjoint_tail(R: torch.Tensor, A: torch.Tensor, ls: torch.Tensor, *, variance: float, symmetric: bool,
                            sum_kbar_k: Optional[torch.Tensor] = None, into: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                            dvar_add: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d/dvariance [1], d/dlengthscales [D], A_bar [n1, D]) from R [n1, 1 + 2 D] = G [1, B, B^2], the first kernel argument A
    [n1, D] and the lengthscales as a [D] device tensor (include/gpk.h: gpk_stationary_adjoint_tail) -- one launch.
    into = (small [1 + D], A_bar) of an earlier call: the results are ADDED to them (and views of them returned); dvar_add is added
    to d/dvariance."""
    lib = _lib.load()
    _chk(R, "R", 2)
    _chk(A, "A", 2)
    _chk(ls, "ls", 1)
    n1, d = A.shape
    if R.shape != (n1, 1 + 2 * d) or ls.shape[0] != d or not ls.is_contiguous():
        raise ValueError("stationary_adjoint_tail: R must be [n1, 1 + 2 D], ls a contiguous [D]")
    if sum_kbar_k is not None:
        _chk(sum_kbar_k, "sum_kbar_k")
    if into is None:
        Abar = torch.empty((n1, d), dtype=torch.float64, device=A.device)
        small = torch.empty(1 + d, dtype=torch.float64, device=A.device)
    else:
        small, Abar = into
        _chk(small, "into[0]", 1)
        _chk(Abar, "into[1]", 2)
        if small.shape[0] != 1 + d or tuple(Abar.shape) != (n1, d) or not small.is_contiguous():
            raise ValueError("stationary_adjoint_tail: into must be (small [1 + D], A_bar [n1, D])")
    rc = lib.gpk_stationary_adjoint_tail(_stream(), R.data_ptr(), _rowmajor(R, "R"), A.data_ptr(), _rowmajor(A, "A"), n1, d,
                                         ls.data_ptr(), float(variance), int(bool(symmetric)),
                                         None if sum_kbar_k is None else sum_kbar_k.data_ptr(), Abar.data_ptr(), _rowmajor(Abar, "A_bar"),
                                         small.data_ptr(), int(into is not None), float(dvar_add))
    _lib.check(rc, "gpk_stationary_adjoint_tail")
    return small[0:1], small[1:], Abar


# ------------------------------------------------------------------------------------------------ the Periodic kernel's input warp
def _period_host(period, d: int):
    """(host array, ard_period) of the C-ABI: one period, or one per input column.  2 d columns must fit the builders."""
    if d < 1 or 2 * d > MAX_D:
        raise ValueError(f"periodic warp: input dimension {d} outside [1, {MAX_D // 2}] (the warped inputs have 2 D columns, at most {MAX_D})")
    p = np.atleast_1d(np.asarray(period, dtype=np.float64))
    if p.ndim != 1 or p.size not in (1, d):
        raise ValueError(f"period has shape {p.shape}, input dimension is {d}")
    return _lib.host_doubles(p.tolist()), int(p.size > 1)


def periodic_warp(X: torch.Tensor, period, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Phi(X) [n, 2 D] for X [n, D]: Phi[:, 2 j] = cos(2 pi x_j / p_j), Phi[:, 2 j + 1] = sin(2 pi x_j / p_j) (include/gpk.h:
    gpk_periodic_warp); `period` a scalar or [D], host values."""
    lib = _lib.load()
    _chk(X, "X", 2)
    n, d = X.shape
    per, ard = _period_host(period, d)
    if out is None:
        out = torch.empty((n, 2 * d), dtype=torch.float64, device=X.device)
    _chk(out, "out", 2)
    if tuple(out.shape) != (n, 2 * d):
        raise ValueError("periodic_warp: out must be [n, 2 D]")
    rc = lib.gpk_periodic_warp(_stream(), X.data_ptr(), _rowmajor(X, "X"), n, d, per, ard, out.data_ptr(), _rowmajor(out, "out"))
    _lib.check(rc, "gpk_periodic_warp")
    return out


def periodic_moment_rows(B: torch.Tensor, period) -> torch.Tensor:
    """[1; Phi(B)^T; (Phi(B)^2)^T; (b cos)^T, (b sin)^T interleaved] as [1 + 6 D, n2] for B [n2, D]: the right-hand side of the one
    contraction behind a Periodic kernel's adjoint (gradients.KernelSpec._adjoint).  Its first 1 + 4 D rows are moment_rows(periodic_warp(B))."""
    lib = _lib.load()
    _chk(B, "B", 2)
    n2, d = B.shape
    per, ard = _period_host(period, d)
    Vt = torch.empty((1 + 6 * d, n2), dtype=torch.float64, device=B.device)
    rc = lib.gpk_periodic_moment_rows(_stream(), B.data_ptr(), _rowmajor(B, "B"), n2, d, per, ard, Vt.data_ptr(), max(n2, 1))
    _lib.check(rc, "gpk_periodic_moment_rows")
    return Vt


def periodic_adjoint_tail(X: torch.Tensor, Phi: torch.Tensor, Phibar: torch.Tensor, R: torch.Tensor, ls: torch.Tensor, period, *,
                          into: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d/dperiod [1] or [D], X_bar [n1, D]) of a Periodic kernel from its first argument X [n1, D], Phi = periodic_warp(X), Phibar
    [n1, 2 D] (the A_bar of stationary_adjoint_tail at the warped inputs), R [n1, 1 + 6 D] = G periodic_moment_rows(B)^T and the BASE
    lengthscales as a [D] device tensor (include/gpk.h: gpk_periodic_adjoint_tail) -- one launch.  d/dperiod covers both arguments of
    K.  into = (d/dperiod, X_bar) of an earlier call: the results are ADDED to them."""
    lib = _lib.load()
    for t, name in ((X, "X"), (Phi, "Phi"), (Phibar, "Phibar"), (R, "R")):
        _chk(t, name, 2)
    _chk(ls, "ls", 1)
    n1, d = X.shape
    per, ard = _period_host(period, d)
    if tuple(Phi.shape) != (n1, 2 * d) or tuple(Phibar.shape) != (n1, 2 * d) or tuple(R.shape) != (n1, 1 + 6 * d) or ls.shape[0] != d \
            or not ls.is_contiguous():
        raise ValueError("periodic_adjoint_tail: Phi and Phibar must be [n1, 2 D], R [n1, 1 + 6 D], ls a contiguous [D]")
    np_ = d if ard else 1
    if into is None:
        dper = torch.empty(np_, dtype=torch.float64, device=X.device)
        Xbar = torch.empty((n1, d), dtype=torch.float64, device=X.device)
    else:
        dper, Xbar = into
        _chk(dper, "into[0]", 1)
        _chk(Xbar, "into[1]", 2)
        if dper.shape[0] != np_ or tuple(Xbar.shape) != (n1, d) or not dper.is_contiguous():
            raise ValueError("periodic_adjoint_tail: into must be (d/dperiod [1 or D], X_bar [n1, D])")
    rc = lib.gpk_periodic_adjoint_tail(_stream(), X.data_ptr(), _rowmajor(X, "X"), Phi.data_ptr(), _rowmajor(Phi, "Phi"),
                                       Phibar.data_ptr(), _rowmajor(Phibar, "Phibar"), R.data_ptr(), _rowmajor(R, "R"), n1, d,
                                       ls.data_ptr(), per, ard, Xbar.data_ptr(), _rowmajor(Xbar, "X_bar"), dper.data_ptr(),
                                       int(into is not None))
    _lib.check(rc, "gpk_periodic_adjoint_tail")
    return dper, Xbar


def adam_step_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, *, beta1: float, beta2: float, epsilon: float,
               step: float, maximise: bool = False) -> torch.Tensor:
    """tf.keras Adam on one contiguous variable, in place (p, m, v): one launch instead of seven (include/gpk.h: gpk_adam_step).
    step = lr sqrt(1 - beta2^t) / (1 - beta1^t); maximise=True takes g as the gradient of the quantity to MAXIMISE."""
    lib = _lib.load()
    for t, name in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(t, name)
        if not t.is_contiguous() or t.numel() != p.numel():
            raise ValueError(f"adam_step_: {name} must be contiguous and of the variable's size")
    rc = lib.gpk_adam_step(_stream(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), float(beta1), float(beta2),
                           float(epsilon), float(step), int(bool(maximise)))
    _lib.check(rc, "gpk_adam_step")
    return p


def lowrank_axpy(alpha: float, X: torch.Tensor, U: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """alpha X + U V^T for X [m, n], thin U [m, k], V [n, k], k <= 16, as a fresh tensor: one pass over X (gpk_lowrank_axpy)."""
    lib = _lib.load()
    _chk(X, "X", 2)
    _chk(U, "U", 2)
    _chk(V, "V", 2)
    m, n = X.shape
    k = U.shape[1]
    if U.shape[0] != m or tuple(V.shape) != (n, k) or not 0 < k <= 16:
        raise ValueError("lowrank_axpy: X [m, n], U [m, k], V [n, k], k <= 16")
    out = torch.empty((m, n), dtype=torch.float64, device=X.device)
    rc = lib.gpk_lowrank_axpy(_stream(), float(alpha), X.data_ptr(), _rowmajor(X, "X"), U.data_ptr(), _rowmajor(U, "U"), V.data_ptr(),
                              _rowmajor(V, "V"), m, n, k, out.data_ptr(), n)
    _lib.check(rc, "gpk_lowrank_axpy")
    return out


def symmetrize_(S: torch.Tensor) -> torch.Tensor:
    """S = (S + S^T) / 2 in place for a square S (one launch)."""
    lib = _lib.load()
    _chk(S, "S", 2)
    if S.shape[0] != S.shape[1]:
        raise ValueError("symmetrize_: square matrix expected")
    rc = lib.gpk_symmetrize(_stream(), S.data_ptr(), S.shape[0], _rowmajor(S, "S"))
    _lib.check(rc, "gpk_symmetrize")
    return S


# ------------------------------------------------------------------------------------------------ fused
def gpr_lml(X: torch.Tensor, Y: torch.Tensor, *, variance: float, lengthscales, noise_variance,
            mean_const: float = 0.0, family: str = "SquaredExponential", alpha=None,
            ws: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(LML scalar tensor, info) -- gpk_gpr_lml.  noise_variance: a float, or one variance per data row [n]."""
    lib = _lib.load()
    _chk(X, "X", 2)
    _chk(Y, "Y", 2)
    n, d = X.shape
    P = Y.shape[1]
    if Y.shape[0] != n:
        raise ValueError("X and Y row counts differ")
    nbytes = int(lib.gpk_gpr_lml_workspace_bytes(n, d, P))
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _ws(nbytes)
    out = torch.empty(1, dtype=torch.float64, device=X.device)
    info = torch.zeros(1, dtype=torch.int32, device=X.device)
    leaf = Leaf(family, variance, lengthscales, alpha=alpha)
    ls, ard = leaf.host(d)
    nv, nv_rows, _keep = _noise_args(noise_variance, n)
    rc = lib.gpk_gpr_lml(_stream(), leaf.code, X.data_ptr(), n, d, _rowmajor(X, "X"),
                         Y.data_ptr(), P, _rowmajor(Y, "Y"), ls, ard, leaf.variance,
                         nv, nv_rows, float(mean_const), out.data_ptr(), info.data_ptr(),
                         ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_gpr_lml")
    return out, info



class HostMailbox:
    """Scalars of a step delivered into pinned, device-mapped host memory by a kernel store (gpk_publish_host) instead of
    device-to-host copies + a stream synchronise: `post(src, info)` enqueues one tiny kernel behind the step on the current
    stream, `wait()` spins on the sequence word that kernel writes last and returns (values, info).  The reference reads
    the same scalar with `.numpy()` on the ELBO tensor (svgp.py:181 -> optimizers / monitoring); here that read costs a few
    microseconds instead of 90 - 150 us per step (two blit copies + hipStreamSynchronize, profiles/r03_step_timeline.txt).
    Falls back to nothing: a wait that times out raises."""

    def __init__(self, n: int = 2):
        if not 1 <= n <= 16:
            raise ValueError("HostMailbox holds 1..16 doubles")
        device()  # raises without a HIP device
        self.n = int(n)
        self._buf = torch.zeros(n + 1, dtype=torch.float64).pin_memory()
        self._vals = self._buf.numpy()[:n]
        self._tail = self._buf.numpy()[n:].view(np.int32)  # [info, seq]
        self._seq = 0

    def post(self, src: torch.Tensor, info: Optional[torch.Tensor] = None) -> int:
        lib = _lib.load()
        _chk(src, "src")
        if src.numel() < self.n or not src.is_contiguous():
            raise ValueError("src must be a contiguous tensor with at least n elements")
        if info is not None and (not info.is_cuda or info.dtype != torch.int32):
            raise _lib.GpkError("info must be an int32 tensor on the HIP device")
        self._seq = (self._seq % 0x7FFFFFF0) + 1
        rc = lib.gpk_publish_host(_stream(), src.data_ptr(), self.n, info.data_ptr() if info is not None else None,
                                  self._buf.data_ptr(), self._seq)
        _lib.check(rc, "gpk_publish_host")
        return self._seq

    def wait(self, timeout_s: float = 30.0):
        import time as _time
        tail, seq = self._tail, self._seq
        spins, t0 = 0, None
        while int(tail[1]) != seq:
            spins += 1
            if spins & 0x3FFF == 0:
                now = _time.perf_counter()
                t0 = t0 or now
                if now - t0 > timeout_s:
                    raise _lib.GpkError("HostMailbox.wait timed out (the publishing kernel never ran)")
        return self._vals.copy(), int(tail[0])


def _shard_setup(Z, Xb, Yb, q_mu, q_sqrt, ws, out, info, *, y_columns, workspace_bytes, latents: Optional[int] = None):
    """What the four svgp_elbo_shard* wrappers share: the operand checks, the contiguity of the variational parameters, and `ws` (of
    `workspace_bytes(m, rows, d, n)` bytes at least) / `out` [2] / `info`, allocated where not given.  n = the columns of q_mu;
    y_columns(n): the columns Yb must have (the likelihood's rule).  latents None: one kernel, Z [m, d], q_sqrt full or diagonal,
    info [1]; else the shards with one kernel per latent, `latents` of them given: Z [m, d] (shared) or [n, m, d], q_sqrt
    [n, m, m], info [n].  Returns (m, d, rows, n, ws, out, info)."""
    per_latent = latents is not None
    for name, t in (("Xb", Xb), ("Yb", Yb), ("q_mu", q_mu)) if per_latent else (("Z", Z), ("Xb", Xb), ("Yb", Yb), ("q_mu", q_mu)):
        _chk(t, name, 2)
    if per_latent:
        _chk(Z, "Z")
    _chk(q_sqrt, "q_sqrt", 3 if per_latent else None)
    m, d = Z.shape[-2], Z.shape[-1]
    rows, n = Xb.shape[0], q_mu.shape[1]
    if (per_latent and Z.dim() != 2 and (Z.dim() != 3 or Z.shape[0] != n)) or Xb.shape[1] != d or Yb.shape[0] != rows \
            or Yb.shape[1] != y_columns(n) or q_mu.shape[0] != m or (per_latent and (tuple(q_sqrt.shape) != (n, m, m) or latents != n)):
        raise ValueError("inconsistent shapes")
    if not (q_mu.is_contiguous() and q_sqrt.is_contiguous() and (Z.is_contiguous() or not per_latent)):
        raise ValueError(("Z / " if per_latent else "") + "q_mu / q_sqrt must be contiguous")
    nbytes = int(workspace_bytes(m, rows, d, n))
    if ws is None or ws.numel() * 8 < nbytes:
        ws = _ws(nbytes)
    if out is None:
        out = torch.empty(2, dtype=torch.float64, device=Xb.device)
    if info is None:
        info = torch.zeros(n if per_latent else 1, dtype=torch.int32, device=Xb.device)
    return m, d, rows, n, ws, out, info


def _latent_hypers(variances, lengthscales, families, n: int, d: int):
    """(family codes, (ls_host, ard, variances_host)) of the per-latent shards: variances [n], lengthscales [n] (isotropic) or
    [n, d], families [n] names (leaf.latent_keywords makes them from leaves)"""
    ls = np.asarray(lengthscales, dtype=np.float64)
    var = np.asarray(variances, dtype=np.float64).reshape(-1)
    if var.size != n or ls.shape[0] != n or (ls.ndim == 2 and ls.shape[1] != d) or ls.ndim > 2:
        raise ValueError("variances / lengthscales: one entry (row) per latent")
    fam = (_lib.C.c_int * n)(*[KERNEL_FAMILIES[f] for f in families])
    return fam, (_lib.host_doubles(ls.reshape(-1).tolist()), int(ls.ndim == 2), _lib.host_doubles(var.tolist()))


def svgp_elbo_sep_workspace(m: int, rows: int, d: int, P: int) -> torch.Tensor:
    lib = _lib.load()
    return _ws(int(lib.gpk_svgp_elbo_sep_workspace_bytes(m, rows, d, P)))


def svgp_elbo_shard_sep(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor, *,
                        variances, lengthscales, families, noise_variance, jitter: float, mean_const: float = 0.0,
                        ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        info: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Whitened shard with one kernel PER latent (SeparateIndependent): Z [m, d] (shared) or [P, m, d]; variances [P],
    lengthscales [P] (isotropic) or [P, d], families [P] names; q_sqrt [P, m, m].  out[0] = sum_b var_exp_b, out[1] = KL;
    info [P].  Returns (out, info)."""
    lib = _lib.load()
    m, d, rows, P, ws, out, info = _shard_setup(Z, Xb, Yb, q_mu, q_sqrt, ws, out, info, y_columns=lambda P: P, latents=len(families),
                                                workspace_bytes=lib.gpk_svgp_elbo_sep_workspace_bytes)
    fam, hypers = _latent_hypers(variances, lengthscales, families, P, d)
    nv, nv_rows, _keep = _noise_args(noise_variance, rows)
    rc = lib.gpk_svgp_elbo_shard_sep(_stream(), fam, Z.data_ptr(), m, d, 0 if Z.dim() == 2 else m * d, Xb.data_ptr(), Yb.data_ptr(), rows,
                                     _rowmajor(Xb, "Xb"), _rowmajor(Yb, "Yb"), d, P, *hypers, nv, nv_rows, float(jitter),
                                     float(mean_const), q_mu.data_ptr(), q_sqrt.data_ptr(), out.data_ptr(), info.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_svgp_elbo_shard_sep")
    return out, info


def svgp_elbo_lcm_workspace(m: int, rows: int, d: int, L: int, P: int) -> torch.Tensor:
    lib = _lib.load()
    return _ws(int(lib.gpk_svgp_elbo_lcm_workspace_bytes(m, rows, d, L, P)))


def svgp_elbo_shard_lcm(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor, W, *,
                        variances, lengthscales, families, noise_variance: float, jitter: float, mean_const: float = 0.0,
                        ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                        info: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Whitened shard of a LinearCoregionalization model: L latents with one kernel each -- Z [m, d] (shared) or [L, m, d],
    variances [L], lengthscales [L] or [L, d], families [L], q_mu [m, L], q_sqrt [L, m, m] as svgp_elbo_shard_sep takes them --
    mixed into the P columns of Yb by W [P, L] (host or device): f = W g + mean_const.  out[0] = sum_b var_exp_b, out[1] = KL
    over the L latents; info [L].  Returns (out, info)."""
    lib = _lib.load()
    _chk(q_mu, "q_mu", 2)
    Wh = _mixing_weights(W, q_mu.shape[1])
    P = Wh.shape[0]
    m, d, rows, L, ws, out, info = _shard_setup(Z, Xb, Yb, q_mu, q_sqrt, ws, out, info, y_columns=lambda L: P, latents=len(families),
                                                workspace_bytes=lambda m, rows, d, L: lib.gpk_svgp_elbo_lcm_workspace_bytes(m, rows, d, L, P))
    fam, hypers = _latent_hypers(variances, lengthscales, families, L, d)
    if not float(noise_variance) > 0.0:
        raise ValueError("noise_variance must be positive")
    rc = lib.gpk_svgp_elbo_shard_lcm(_stream(), fam, Z.data_ptr(), m, d, 0 if Z.dim() == 2 else m * d, Xb.data_ptr(), Yb.data_ptr(), rows,
                                     _rowmajor(Xb, "Xb"), _rowmajor(Yb, "Yb"), d, L, P, _lib.host_doubles(Wh.reshape(-1).tolist()),
                                     *hypers, float(noise_variance), float(jitter), float(mean_const), q_mu.data_ptr(),
                                     q_sqrt.data_ptr(), out.data_ptr(), info.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_svgp_elbo_shard_lcm")
    return out, info


def svgp_elbo_workspace(m: int, rows: int, d: int, P: int, q_diag: bool, whiten: bool = True) -> torch.Tensor:
    lib = _lib.load()
    return _ws(int(lib.gpk_svgp_elbo_workspace_bytes(m, rows, d, P, int(q_diag), int(bool(whiten)))))


def svgp_elbo_shard(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor,
                    q_sqrt: torch.Tensor, *, variance: float, lengthscales, noise_variance,
                    jitter: float, mean_const: float = 0.0, family: str = "SquaredExponential", alpha=None,
                    ws: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                    info: Optional[torch.Tensor] = None, whiten: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """One shard of SVGP.elbo: out[0] = sum_b var_exp_b over this shard, out[1] = KL.  Returns (out, info).
    whiten=False: KL against N(0, Kuu) and the un-whitened conditional, on one factorisation (full or diagonal q_sqrt)."""
    lib = _lib.load()
    whiten = int(bool(whiten))
    m, d, rows, P, ws, out, info = _shard_setup(
        Z, Xb, Yb, q_mu, q_sqrt, ws, out, info, y_columns=lambda P: P,
        workspace_bytes=lambda m, rows, d, P: lib.gpk_svgp_elbo_workspace_bytes(m, rows, d, P, int(q_sqrt.dim() == 2), whiten))
    q_diag = int(q_sqrt.dim() == 2)
    leaf = Leaf(family, variance, lengthscales, alpha=alpha)
    ls, ard = leaf.host(d)
    nv, nv_rows, _keep = _noise_args(noise_variance, rows)
    rc = lib.gpk_svgp_elbo_shard(_stream(), leaf.code, Z.data_ptr(), m, _rowmajor(Z, "Z"),
                                 Xb.data_ptr(), Yb.data_ptr(), rows, _rowmajor(Xb, "Xb"),
                                 _rowmajor(Yb, "Yb"), d, P, ls, ard, leaf.variance,
                                 nv, nv_rows, float(jitter), float(mean_const),
                                 q_mu.data_ptr(), q_sqrt.data_ptr(), q_diag, whiten, out.data_ptr(),
                                 info.data_ptr(), ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_svgp_elbo_shard")
    return out, info


def svgp_elbo_shard_lik(Z: torch.Tensor, Xb: torch.Tensor, Yb: torch.Tensor, q_mu: torch.Tensor, q_sqrt: torch.Tensor, *,
                        variance: float, lengthscales, lik: str, params=(), jitter: float, mean_const: float = 0.0,
                        family: str = "SquaredExponential", alpha=None, ws: Optional[torch.Tensor] = None,
                        out: Optional[torch.Tensor] = None, info: Optional[torch.Tensor] = None,
                        whiten: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """svgp_elbo_shard with a non-Gaussian likelihood (lik, params as likelihood_varexp_sum) in place of the noise variance:
    out[0] = sum_b of the quadrature variational expectations over this shard, out[1] = KL.  Same forms, same workspace.
    "multiclass_robustmax": Yb is ONE column of labels."""
    lib = _lib.load()
    whiten = int(bool(whiten))
    m, d, rows, P, ws, out, info = _shard_setup(
        Z, Xb, Yb, q_mu, q_sqrt, ws, out, info, y_columns=lambda P: _lik_y_columns(lik, P),
        workspace_bytes=lambda m, rows, d, P: lib.gpk_svgp_elbo_workspace_bytes(m, rows, d, P, int(q_sqrt.dim() == 2), whiten))
    q_diag = int(q_sqrt.dim() == 2)
    code, par = _lik_args(lik, params)
    leaf = Leaf(family, variance, lengthscales, alpha=alpha)
    ls, ard = leaf.host(d)
    rc = lib.gpk_svgp_elbo_shard_lik(_stream(), leaf.code, Z.data_ptr(), m, _rowmajor(Z, "Z"), Xb.data_ptr(),
                                     Yb.data_ptr(), rows, _rowmajor(Xb, "Xb"), _rowmajor(Yb, "Yb"), d, P, ls, ard,
                                     leaf.variance, code, par, float(jitter), float(mean_const), q_mu.data_ptr(),
                                     q_sqrt.data_ptr(), q_diag, whiten, out.data_ptr(), info.data_ptr(),
                                     ws.data_ptr(), ws.numel() * 8)
    _lib.check(rc, "gpk_svgp_elbo_shard_lik")
    return out, info
