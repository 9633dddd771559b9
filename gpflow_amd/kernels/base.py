"""Kernel ABC: the __call__ contract and active_dims slicing of gpflow/kernels/base.py:90-214."""
from __future__ import annotations

import abc
from typing import Optional, Sequence, Union

import numpy as np
import torch

from ..base import Module
from .. import ops
from ..leaf import BY_NAME, Leaf

ActiveDims = Union[slice, Sequence[int]]


class Kernel(Module, metaclass=abc.ABCMeta):
    def __init__(self, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        self.name = name or type(self).__name__
        if active_dims is None:
            active_dims = slice(None, None, None)
        if not isinstance(active_dims, slice):
            active_dims = np.array(active_dims, dtype=int)
        self._active_dims = active_dims

    @property
    def active_dims(self):
        return self._active_dims

    @property
    def has_default_active_dims(self) -> bool:
        """True when every input column is active (active_dims was None / slice(None)); an index list is never the
        default, even if it happens to enumerate all columns."""
        d = self._active_dims
        return isinstance(d, slice) and d == slice(None, None, None)

    def slice(self, X: torch.Tensor, X2: Optional[torch.Tensor] = None):
        """gpflow/kernels/base.py:90-109"""
        dims = self._active_dims
        if isinstance(dims, slice):
            if self.has_default_active_dims:
                return X, X2
            X = X[..., dims]
            X2 = X2[..., dims] if X2 is not None else None
        else:
            idx = torch.as_tensor(dims, device=X.device)
            X = X.index_select(-1, idx)
            X2 = X2.index_select(-1, idx) if X2 is not None else None
        return X.contiguous(), (X2.contiguous() if X2 is not None else None)

    @abc.abstractmethod
    def K(self, X, X2=None):
        raise NotImplementedError

    @abc.abstractmethod
    def K_diag(self, X):
        raise NotImplementedError

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        """Device contract used by the covariance dispatchers, conditionals and posteriors: K(X, X2) (K(X, X) +
        diag_add I when X2 is None) written into `out` (allocated when None); inputs are already sliced by the caller.
        Stationary kernels and their sums / products override this with fused device builds; this generic version
        only serves kernels that define K alone."""
        K = self.K(X, X2)
        if X2 is None and diag_add != 0.0:
            K.diagonal().add_(float(diag_add))
        if out is None:
            return K
        out.copy_(K)
        return out

    def __add__(self, other: "Kernel") -> "Kernel":
        """gpflow/kernels/base.py:216-217"""
        return Sum([self, other])

    def __mul__(self, other: "Kernel") -> "Kernel":
        """gpflow/kernels/base.py:219-220"""
        return Product([self, other])

    def __call__(self, X, X2=None, *, full_cov: bool = True, presliced: bool = False):
        """gpflow/kernels/base.py:195-214"""
        if (not full_cov) and (X2 is not None):
            raise ValueError("Ambiguous inputs: `not full_cov` and `X2` are not compatible.")
        X = ops.to_device(X)
        X2 = ops.to_device(X2) if X2 is not None else None
        if not presliced:
            X, X2 = self.slice(X, X2)
        if not full_cov:
            return self.K_diag(X)
        return self.K(X, X2)


class DeviceLeaf(Kernel):
    """A kernel that gpk_kernel_matrix builds from host hyperparameters (the stationary and the static families): `family` names its
    row of leaf.FAMILIES, `leaf()` is its current values and `leaf_params()` the Parameters behind them, in the same order;
    K_diag = variance.  `maps_inputs`: `slice` does more than select columns (Periodic warps them), so `leaf()` goes with the output of
    `slice` only -- whoever hands a builder inputs it did not get from `slice` must decline such a kernel."""
    family: Optional[str] = None
    device_leaf = True
    maps_inputs = False

    def leaf_params(self) -> tuple:
        return tuple(getattr(self, name) for name in BY_NAME[self.family].parameters)

    def leaf(self) -> Leaf:
        return Leaf.of(self.family, [p.numpy() for p in self.leaf_params()])

    def K_diag(self, X) -> torch.Tensor:
        """stationaries.py:82-83, `Static.K_diag`: exactly the variance"""
        X = ops.to_device(X)
        return torch.full(X.shape[:-1], float(self.variance.numpy()), dtype=torch.float64, device=X.device)

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        return ops.kernel_matrix(X, X2, diag_add=diag_add, lower_only=lower_only, out=out, **self.leaf().keywords())

    def K_fold(self, X, X2, out, op: str, diag_add: float = 0.0):
        """out <- out .* K or out + K in place (K recomputed in registers: one read + one write of `out`, no second matrix); the
        row-diagonal leaves answer it too (RowDiagonalLeaf), and Combination.K_into asks nothing else of a member"""
        return ops.kernel_matrix_combine(X, X2, out, op=op, diag_add=diag_add, out=out, **self.leaf().keywords())


def is_device_leaf(k) -> bool:
    """True for a DeviceLeaf of a known family.  The one notion reverse_leaf and the model routes share."""
    return bool(getattr(k, "device_leaf", False)) and getattr(k, "family", None) in ops.KERNEL_FAMILIES


class RowDiagonalLeaf(Kernel):
    """A kernel leaf whose K(x, x) depends on the row, built by the entry points of its own kind (`leaf_kind`: "dot" kernels/linears.py,
    "arc" and "coregion" kernels/misc.py): never a DeviceLeaf, so every fused route that takes K_diag for the variance declines it and
    the composed routes run.  Written once here, over `leaf()` (a value of leaf.py that answers its protocol), the leaf's `builders` --
    looked up on `ops` by name at the call -- and `check_width(d)`, the ValueError before the device for a width the kernel cannot see:
    K, K_into, K_fold, K_diag.  A class gives `leaf_kind`, its constructor, `leaf_params()`, `leaf()` and `check_width`."""
    leaf_kind: Optional[str] = None

    def _builder(self, which: int, X, *args, **kw):
        self.check_width(X.shape[-1])
        leaf = self.leaf()
        return getattr(ops, leaf.builders[which])(X, *args, **kw, **leaf.keywords())

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        return self._builder(0, X, X2, diag_add=diag_add, lower_only=lower_only, out=out)

    def K_fold(self, X, X2, out, op: str, diag_add: float = 0.0):
        """out <- out .* K or out + K in place, as DeviceLeaf.K_fold"""
        return self._builder(1, X, X2, out, op=op, diag_add=diag_add, out=out)

    def K(self, X, X2=None) -> torch.Tensor:
        """leading batch dimensions as IsotropicStationary.K: flattened to rows and restored"""
        X = ops.to_device(X)
        D = X.shape[-1]
        if X2 is None:
            if X.dim() == 2:
                return self.K_into(X, None, None)
            lead, n = X.shape[:-2], X.shape[-2]
            return torch.stack([self.K_into(x.contiguous(), None, None) for x in X.reshape(-1, n, D)]).reshape(*lead, n, n)
        X2 = ops.to_device(X2)
        Kf = self.K_into(X.reshape(-1, D).contiguous(), X2.reshape(-1, D).contiguous(), None)
        return Kf.reshape(*X.shape[:-1], *X2.shape[:-1])

    def K_diag(self, X) -> torch.Tensor:
        """the row diagonal on the device (the kind's *_kernel_diag entry point); leading batch dimensions allowed"""
        X = ops.to_device(X)
        return self._builder(2, X.reshape(-1, X.shape[-1]).contiguous()).reshape(X.shape[:-1])


def _leaf_kind(k):
    return getattr(k, "leaf_kind", None)


def is_dot_leaf(k) -> bool:
    """True for a dot-product kernel (kernels/linears.py: Linear, Polynomial), built by gpk_dot_kernel_matrix.  A kernel has ONE
    `leaf_kind`, and a DeviceLeaf none: this, `is_arc_leaf`, `is_coregion_leaf` and `is_device_leaf` never hold together."""
    return _leaf_kind(k) == "dot"


def is_arc_leaf(k) -> bool:
    """True for an ArcCosine kernel (kernels/misc.py), built by gpk_arccos_kernel_matrix: each element needs both row norms and an acos."""
    return _leaf_kind(k) == "arc"


def is_coregion_leaf(k) -> bool:
    """True for a Coregion kernel (kernels/misc.py), built by gpk_coregion_kernel_matrix: an element is a gather from the output
    covariance, the diagonal depends on the row's task label."""
    return _leaf_kind(k) == "coregion"


def has_row_diagonal_leaf(k) -> bool:
    """a leaf whose K(x, x) depends on the row: one with a `leaf_kind` (the dot-product kernels, ArcCosine, Coregion)"""
    return _leaf_kind(k) is not None


class Combination(Kernel):
    """A list of kernels reduced elementwise (gpflow/kernels/base.py:223-329); nested instances of the same class are
    flattened (:247-255).  Every member slices its own active_dims, so the combination itself never slices."""

    _op = None  # "add" | "mul"; "cp": kernels/changepoints.py, which overrides every method here that reads it

    def __init__(self, kernels: Sequence[Kernel], name: Optional[str] = None):
        super().__init__(name=name)
        if not all(isinstance(k, Kernel) for k in kernels):
            raise TypeError("can only combine Kernel instances")
        flat = []
        for k in kernels:
            flat.extend(k.kernels if isinstance(k, self.__class__) else [k])
        self.kernels = flat

    @property
    def on_separate_dimensions(self) -> bool:
        """gpflow/kernels/base.py:257-280"""
        if any(isinstance(k.active_dims, slice) for k in self.kernels):
            return False
        dims = [np.asarray(k.active_dims) for k in self.kernels]
        for i, di in enumerate(dims):
            for dj in dims[i + 1:]:
                if np.any(di.reshape(-1, 1) == dj.reshape(1, -1)):
                    return False
        return True

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        """The first member is built into `out`; every further member that can (`K_fold`: the device-built and the dot-product
        leaves) folds itself in place, any other is built into a matrix of its own once."""
        X = ops.to_device(X)
        X2 = ops.to_device(X2) if X2 is not None else None
        ks = list(self.kernels)
        last = len(ks) - 1
        k0 = ks[0]
        Xs, X2s = k0.slice(X, X2)
        out = k0.K_into(Xs, X2s, out, diag_add=diag_add if last == 0 else 0.0, lower_only=False)
        for i, k in enumerate(ks[1:], start=1):
            Xs, X2s = k.slice(X, X2)
            dadd = diag_add if i == last else 0.0
            if hasattr(k, "K_fold"):
                k.K_fold(Xs, X2s, out, self._op, diag_add=dadd)
            else:
                Ki = k.K_into(Xs, X2s, None)
                out.add_(Ki) if self._op == "add" else out.mul_(Ki)
                if X2 is None and dadd != 0.0:
                    out.diagonal().add_(float(dadd))
        return out

    def K(self, X, X2=None) -> torch.Tensor:
        X = ops.to_device(X)
        if X.dim() != 2 or (X2 is not None and ops.to_device(X2).dim() != 2):
            raise NotImplementedError("kernel combinations take [N, D] inputs")
        return self.K_into(X, X2, None)

    def K_diag(self, X) -> torch.Tensor:
        outs = [k(X, full_cov=False) for k in self.kernels]
        acc = outs[0].clone()
        for o in outs[1:]:
            acc = acc + o if self._op == "add" else acc * o
        return acc

    def __call__(self, X, X2=None, *, full_cov: bool = True, presliced: bool = False):
        """gpflow/kernels/base.py:283-293: members slice for themselves unless presliced."""
        if (not full_cov) and (X2 is not None):
            raise ValueError("Ambiguous inputs: `not full_cov` and `X2` are not compatible.")
        if presliced:
            raise NotImplementedError("presliced inputs to a kernel combination")
        return self.K_diag(X) if not full_cov else self.K(X, X2)


def reverse_leaf(k, input_dim=None):
    """(leaf, period or None, leaf_params) of a kernel that is ONE leaf the reverse pass covers, else None: an isotropic-stationary or a
    static kernel that the device builds, a Periodic one over such a base (`leaf` in the device form, the warp left to the spec: its
    `periods`), a dot-product one, an ArcCosine one, or a Coregion one.  A Periodic kernel's width is checked here, before anything touches the device, wherever its
    active columns can be counted: an index list, or a slice of `input_dim` columns."""
    from .periodic import Periodic
    from .stationaries import IsotropicStationary
    from .statics import Static
    periodic = isinstance(k, Periodic)
    if not (((periodic or isinstance(k, (IsotropicStationary, Static))) and is_device_leaf(k)) or has_row_diagonal_leaf(k)):
        return None
    if periodic and not isinstance(k.active_dims, slice):
        k.check_width(len(k.active_dims))
    elif periodic and input_dim is not None:
        k.check_width(len(np.arange(int(input_dim))[k.active_dims]))
    return k.leaf(), (k.period.numpy() if periodic else None), k.leaf_params()


def gradient_spec(kernel, input_dim=None):
    """gradients.KernelSpec + [(variance Parameter, lengthscales Parameter)] for the kernels the reverse pass covers beyond a
    single stationary one: a Sum / Product of isotropic-stationary members, flat or nested (kernels/base.py:216-220, 305-315; the
    end of round 5: a Product of Sums and the like -- the spec then carries the combination tree).  Members may
    carry their own `active_dims` (kernels/base.py:90-109): the spec then builds and differentiates each member on its own columns
    and scatters its input gradient back (round 5) -- `input_dim`, the number of input columns, resolves slices.  None if `kernel`
    is not such a combination."""
    from .. import gradients
    if not isinstance(kernel, Combination):
        return None
    # leaves in traversal order (with what reverse_leaf says of each) + the tree over their indices (a flat combination: one node)
    ks, found, nodes = [], [], []

    def walk(k):
        if isinstance(k, Combination) and k._op == "cp":   # ChangePoints: a node with values of its own, numbered as it is met
            nodes.append(k.node())
            index = len(nodes) - 1
            return ("cp", [walk(c) for c in k.kernels], index)
        if isinstance(k, Combination):
            return (k._op, [walk(c) for c in k.kernels])
        found.append(reverse_leaf(k, input_dim))
        if found[-1] is None:      # (not one of its leaves)
            raise NotImplementedError("gradients of a kernel combination: Sums / Products (possibly nested) of isotropic-stationary, "
                                      "Periodic, static, dot-product (Linear, Polynomial), ArcCosine and Coregion members (kernels/base.py:216-220, 305-315)")
        ks.append(k)
        return len(ks) - 1
    tree = walk(kernel)
    cols = []
    for k in ks:
        if k.has_default_active_dims:
            cols.append(None)
        elif isinstance(k.active_dims, slice):
            if input_dim is None:
                raise NotImplementedError("gradients of a kernel combination with sliced active_dims need the input dimension")
            cols.append(np.arange(int(input_dim))[k.active_dims])
        else:
            cols.append(np.asarray(k.active_dims, dtype=np.int64))
    leaves, periods, params = zip(*found)     # (a Periodic member: the columns are its base's, the warp is the spec's -- `periods`)
    return gradients.KernelSpec(leaves, tree, cols=cols, periods=periods, nodes=nodes), list(params)


def changepoint_nodes(kernel) -> list:
    """the ChangePoints kernels under `kernel` in the order `gradient_spec` numbers their nodes (each as it is met, before its members)"""
    if not isinstance(kernel, Combination):
        return []
    return ([kernel] if kernel._op == "cp" else []) + [n for c in kernel.kernels for n in changepoint_nodes(c)]


class Sum(Combination):
    """gpflow/kernels/base.py:318-321"""
    _op = "add"


class Product(Combination):
    """gpflow/kernels/base.py:324-329"""
    _op = "mul"
