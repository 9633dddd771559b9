"""The ArcCosine kernel (gpflow/kernels/misc.py): the covariance of an infinitely wide one-layer network (Cho & Saul, 2009).

    s(x, y) = sum_j weight_variances_j x_j y_j + bias_variance          p(x) = s(x, x)
    theta   = acos(eps + (1 - 2 eps) s / (sqrt p(x) sqrt p(y)))
    K       = (variance / pi) J_order(theta) p(x)^(order/2) p(y)^(order/2)         K_diag = variance (J_order(0) / pi) p(x)^order

Built in one pass by gpk_arccos_kernel_matrix (csrc/arccosine/arccosine.hip), folded into a Sum / Product in place by
gpk_arccos_kernel_matrix_combine.  Like the dot-product kernels it is NOT a DeviceLeaf -- its diagonal depends on the row, so every
fused route that takes K_diag for the variance (`kernels.base.is_device_leaf`) declines it and the composed routes run -- and it is not
a dot-product leaf either: each element needs both row norms and an acos.  `is_arc_leaf` is its predicate, `leaf()` a leaf.ArcLeaf.
K(X, X) takes its diagonal by index (include/gpk.h); K_diag is the closed form, a relative 1.4e-8 from it at order 0, as in the reference.

The Coregion kernel (gpflow/kernels/misc.py), the intrinsic-coregionalisation (multi-task) kernel over ONE column of task labels:

    B = W W^T + diag(kappa)  [output_dim, output_dim]          K(x, y) = B[l(x), l(y)]          K_diag(x) = B[l(x), l(x)]

the usual recipe being `k_data(active_dims=[0 .. D-1]) * Coregion(output_dim=P, rank=R, active_dims=[D])`.  Built by
gpk_coregion_kernel_matrix (csrc/coregion/coregion.hip: a gather from B staged in LDS), folded into a Sum / Product in place by
gpk_coregion_kernel_matrix_combine -- the launch the recipe's Product makes.  Not a DeviceLeaf, not a dot-product leaf, not an ArcCosine
one: `is_coregion_leaf` is its predicate, `leaf()` a leaf.CoregionLeaf.  A label is the column truncated toward zero, valid inside
(-1, output_dim); an invalid one makes its row / column of K NaN (include/gpk.h)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..base import Parameter, positive
from .. import ops
from ..leaf import ARC_PARAMETERS, COREGION_PARAMETERS, ArcLeaf, CoregionLeaf, check_coregion_sizes, check_order
from .base import ActiveDims, RowDiagonalLeaf


class ArcCosine(RowDiagonalLeaf):
    """misc.py `ArcCosine`: `order` 0, 1 or 2 (a constant; anything else raises ValueError, as the reference does);
    `weight_variances` one weight, or one per active input column (ARD)"""
    leaf_kind = "arc"
    implemented_orders = {0, 1, 2}

    def __init__(self, order: int = 0, variance=1.0, weight_variances=1.0, bias_variance=1.0, active_dims: Optional[ActiveDims] = None,
                 name: Optional[str] = None):
        self.order = check_order(order)     # ValueError before anything else
        super().__init__(active_dims=active_dims, name=name)
        self.variance = Parameter(variance, transform=positive())
        self.weight_variances = Parameter(weight_variances, transform=positive())
        self.bias_variance = Parameter(bias_variance, transform=positive())
        if self.variance.numpy().ndim > 0 or self.bias_variance.numpy().ndim > 0:
            raise ValueError("variance and bias_variance are scalars")
        w = self.weight_variances.numpy()
        if w.ndim > 1:
            raise ValueError(f"weight_variances of shape {w.shape}: one weight, or one per active input column")
        if w.ndim == 1 and not isinstance(self._active_dims, slice) and w.shape[0] != len(self._active_dims):   # gpflow/kernels/base.py:158-178
            raise ValueError(f"Size of `active_dims` {self._active_dims} does not match size of ard parameter ({w.shape[0]})")

    @property
    def ard(self) -> bool:
        return self.weight_variances.numpy().ndim > 0

    def leaf_params(self) -> tuple:
        return tuple(getattr(self, name) for name in ARC_PARAMETERS)

    def leaf(self) -> ArcLeaf:
        return ArcLeaf.of(self.order, [p.numpy() for p in self.leaf_params()])

    def check_width(self, d: int) -> None:
        """ValueError, before the device, for ARD weights that do not fit the d input columns the kernel sees"""
        w = self.weight_variances.numpy()
        if w.ndim == 1 and w.shape[0] != d:
            raise ValueError(f"weight_variances has {w.shape[0]} entries, the kernel sees {d} input columns")


class Coregion(RowDiagonalLeaf):
    """misc.py `Coregion`: `W` [output_dim, rank] unconstrained, initial 0.1 * ones; `kappa` [output_dim] positive, initial ones;
    `output_dim` in 1 ... 64 and `rank` in 1 ... 64 (anything else raises ValueError); exactly ONE active input column, the task label"""
    leaf_kind = "coregion"

    def __init__(self, output_dim: int, rank: int, *, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        self.output_dim, self.rank = check_coregion_sizes(output_dim, rank)     # ValueError before anything else
        super().__init__(active_dims=active_dims, name=name)
        if not isinstance(self._active_dims, slice) and len(self._active_dims) != 1:
            raise ValueError(f"Coregion(active_dims={list(self._active_dims)}): exactly one active input column, the task label")
        self.W = Parameter(0.1 * np.ones((self.output_dim, self.rank)))
        self.kappa = Parameter(np.ones(self.output_dim), transform=positive())

    def leaf_params(self) -> tuple:
        """(kappa, W): the order of the gradients (leaf.COREGION_PARAMETERS); the Parameters themselves are W, then kappa"""
        return tuple(getattr(self, name) for name in COREGION_PARAMETERS)

    def leaf(self) -> CoregionLeaf:
        W, kappa = self.W.numpy(), self.kappa.numpy()
        if W.shape != (self.output_dim, self.rank) or kappa.shape != (self.output_dim,):
            raise ValueError(f"W of shape {W.shape} and kappa of shape {kappa.shape}: [{self.output_dim}, {self.rank}] and [{self.output_dim}]")
        return CoregionLeaf(W, kappa)

    @staticmethod
    def check_width(d: int) -> None:
        """ValueError, before the device, unless the kernel sees exactly one input column"""
        if d != 1:
            raise ValueError(f"Coregion: the kernel sees {d} input columns; exactly one active column (the task label) is needed: "
                             "set active_dims=[column]")

    def output_covariance(self) -> torch.Tensor:
        """B = W W^T + diag(kappa) [output_dim, output_dim], on the device (a fresh tensor)"""
        return ops.coregion_output_covariance(**self.leaf().keywords()).clone()

    def output_variance(self) -> torch.Tensor:
        """diag(B) = sum_r W[:, r]^2 + kappa [output_dim], on the device"""
        return torch.diagonal(ops.coregion_output_covariance(**self.leaf().keywords())).clone()
