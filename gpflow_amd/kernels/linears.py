"""Dot-product kernels (gpflow/kernels/linears.py): Linear and Polynomial.

    Linear      K = (X * variance) X2^T                      K_diag = sum_j variance_j x_j^2
    Polynomial  K = (Linear.K + offset)^degree               K_diag = (Linear.K_diag + offset)^degree

Built in one pass by gpk_dot_kernel_matrix (csrc/dot.hip), folded into a Sum / Product in place by gpk_dot_kernel_matrix_combine.
They are NOT DeviceLeafs: their diagonal depends on the row, and every fused route that takes K_diag for the variance
(`kernels.base.is_device_leaf`) declines them; the composed routes run.  `is_dot_leaf` is their predicate, `leaf()` a leaf.DotLeaf."""
from __future__ import annotations

from typing import Optional

import torch

from ..base import Parameter, positive
from .. import ops
from ..leaf import DOT_BY_NAME, DotLeaf, check_degree
from .base import ActiveDims, Kernel


class Linear(Kernel):
    """linears.py `Linear`: `variance` one weight, or one per active input column (ARD)"""
    dot_family = "Linear"

    def __init__(self, variance=1.0, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        super().__init__(active_dims=active_dims, name=name)
        self.variance = Parameter(variance, transform=positive())
        v = self.variance.numpy()
        if v.ndim > 1:
            raise ValueError(f"variance of shape {v.shape}: one weight, or one per active input column")
        if v.ndim == 1 and not isinstance(self._active_dims, slice) and v.shape[0] != len(self._active_dims):   # gpflow/kernels/base.py:158-178
            raise ValueError(f"Size of `active_dims` {self._active_dims} does not match size of ard parameter ({v.shape[0]})")

    @property
    def ard(self) -> bool:
        return self.variance.numpy().ndim > 0

    def leaf_params(self) -> tuple:
        return tuple(getattr(self, name) for name in DOT_BY_NAME[self.dot_family].parameters)

    def leaf(self) -> DotLeaf:
        return DotLeaf.of(self.dot_family, [p.numpy() for p in self.leaf_params()], degree=getattr(self, "degree", None))

    def check_width(self, d: int) -> None:
        """ValueError, before the device, for an ARD variance that does not fit the d input columns the kernel sees"""
        v = self.variance.numpy()
        if v.ndim == 1 and v.shape[0] != d:
            raise ValueError(f"variance has {v.shape[0]} entries, the kernel sees {d} input columns")

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        self.check_width(X.shape[-1])
        return ops.dot_kernel_matrix(X, X2, diag_add=diag_add, lower_only=lower_only, out=out, **self.leaf().keywords())

    def K_fold(self, X, X2, out, op: str, diag_add: float = 0.0):
        """out <- out .* K or out + K in place, as DeviceLeaf.K_fold"""
        return ops.dot_kernel_matrix_combine(X, X2, out, op=op, diag_add=diag_add, out=out, **self.leaf().keywords())

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
        """the row diagonal on the device (gpk_dot_kernel_diag): the diagonal of K(X, X) bit for bit; leading batch dimensions allowed"""
        X = ops.to_device(X)
        self.check_width(X.shape[-1])
        return ops.dot_kernel_diag(X.reshape(-1, X.shape[-1]).contiguous(), **self.leaf().keywords()).reshape(X.shape[:-1])


class Polynomial(Linear):
    """linears.py `Polynomial`; `degree` is a constant: integral, 1 ... 16 (the device takes the power as a product)"""
    dot_family = "Polynomial"

    def __init__(self, degree=3.0, variance=1.0, offset=1.0, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        self.degree = check_degree(degree)     # NotImplementedError before anything else
        super().__init__(variance=variance, active_dims=active_dims, name=name)
        self.offset = Parameter(offset, transform=positive())
