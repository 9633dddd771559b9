"""Dot-product kernels (gpflow/kernels/linears.py): Linear and Polynomial.

    Linear      K = (X * variance) X2^T                      K_diag = sum_j variance_j x_j^2
    Polynomial  K = (Linear.K + offset)^degree               K_diag = (Linear.K_diag + offset)^degree

Built in one pass by gpk_dot_kernel_matrix (csrc/dot.hip), folded into a Sum / Product in place by gpk_dot_kernel_matrix_combine.
They are NOT DeviceLeafs: their diagonal depends on the row, and every fused route that takes K_diag for the variance
(`kernels.base.is_device_leaf`) declines them; the composed routes run.  `is_dot_leaf` is their predicate, `leaf()` a leaf.DotLeaf."""
from __future__ import annotations

from typing import Optional

from ..base import Parameter, positive
from ..leaf import DOT_BY_NAME, DotLeaf, check_degree
from .base import ActiveDims, RowDiagonalLeaf


class Linear(RowDiagonalLeaf):
    """linears.py `Linear`: `variance` one weight, or one per active input column (ARD)"""
    leaf_kind, dot_family = "dot", "Linear"

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


class Polynomial(Linear):
    """linears.py `Polynomial`; `degree` is a constant: integral, 1 ... 16 (the device takes the power as a product)"""
    dot_family = "Polynomial"

    def __init__(self, degree=3.0, variance=1.0, offset=1.0, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        self.degree = check_degree(degree)     # NotImplementedError before anything else
        super().__init__(variance=variance, active_dims=active_dims, name=name)
        self.offset = Parameter(offset, transform=positive())
