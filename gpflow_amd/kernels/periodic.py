"""The Periodic kernel (gpflow/kernels/periodic.py) over a base kernel evaluated on r^2:

    k(x, x') = base(r^2),   r^2 = sum_j sin^2(pi (x_j - x'_j) / p_j) / l_j^2

With a_j = 2 pi x_j / p_j and the warp Phi(x) = (cos a_1, sin a_1, ..., cos a_D, sin a_D):  |Phi_j(x) - Phi_j(x')|^2 =
4 sin^2(pi (x_j - x'_j) / p_j).  So the kernel is the BASE family on the warped inputs Phi(X) [n, 2 D] with lengthscales 2 l_j for both
columns of pair j -- one HIP pass over the rows (gpk_periodic_warp: (rows) D sincospi, where a sin per pair inside the builder would
cost n1 n2 D) and then every builder, fused driver and adjoint of the stationary families at width 2 D.

The one rule that keeps the warp applied exactly once: `slice` returns WARPED inputs and `leaf()` is the device-form leaf that goes
with them, as every `k.slice(...)` + `k.leaf().keywords()` / `k.K_into(...)` route expects; `K` takes the column-selected, un-warped
inputs (the reference's contract for K) and warps them itself.  Code that hands a builder RAW inputs on the strength of
`is_device_leaf` must ask `maps_inputs` first (SVGP._separate_stationary_members does)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..base import Parameter, positive
from .. import ops
from ..leaf import Leaf
from .base import DeviceLeaf, Kernel
from .stationaries import IsotropicStationary, RationalQuadratic, SquaredExponential


class Periodic(DeviceLeaf):
    maps_inputs = True

    def __init__(self, base_kernel: IsotropicStationary, period=1.0, name: Optional[str] = None):
        if not isinstance(base_kernel, (SquaredExponential, RationalQuadratic)):
            raise NotImplementedError(
                "Periodic: the base must be SquaredExponential or RationalQuadratic -- families evaluated on r^2, for which the kernel "
                "is the base on the warped inputs (cos, sin)(2 pi x / period).  A base evaluated on r (Matern, Exponential) has a "
                "different distance in the reference, which the warp does not give; it is not built")
        Kernel.__init__(self, name=name)
        self._active_dims = base_kernel._active_dims      # the base's: it selects the columns, this kernel warps them
        self.base_kernel = base_kernel
        self.period = Parameter(period, transform=positive())
        base_kernel._validate_ard_active_dims(self.period)
        p, ls = self.period.numpy(), base_kernel.lengthscales.numpy()
        if p.ndim > 1 or (p.ndim == 1 and ls.ndim == 1 and p.shape[0] != ls.shape[0]):
            raise ValueError(f"Periodic: period of shape {p.shape} does not fit lengthscales of shape {ls.shape}")

    # ---- what a DeviceLeaf answers --------------------------------------------------------------
    @property
    def family(self) -> str:
        return self.base_kernel.family

    @property
    def variance(self) -> Parameter:
        return self.base_kernel.variance

    def leaf_params(self) -> tuple:
        """the base's Parameters, then the period: the order of the gradients (gradients.KernelSpec.parameter_names)"""
        return self.base_kernel.leaf_params() + (self.period,)

    def leaf(self) -> Leaf:
        """the DEVICE form: the base's leaf over the 2 D warped columns, lengthscales 2 l (an ARD one repeated pairwise)"""
        base = self.base_kernel.leaf()
        ls = 2.0 * base.lengthscales
        return base.replace([base.variance, ls if ls.size == 1 else np.repeat(ls.reshape(-1), 2), *base.extras])

    def check_width(self, d: int) -> None:
        """ValueError, before the device, for d active input columns the warp cannot take: 2 d beyond the builder's width, or a period /
        lengthscales of another length"""
        if 2 * d > ops.MAX_D:
            raise ValueError(f"Periodic over {d} active input columns: the warped inputs have 2 D = {2 * d} columns, the covariance "
                             f"builder takes at most {ops.MAX_D}")
        for par, what in ((self.period, "period"), (self.base_kernel.lengthscales, "lengthscales")):
            v = par.numpy()
            if v.ndim == 1 and v.shape[0] not in (1, d):
                raise ValueError(f"Periodic: {what} has {v.shape[0]} entries, the kernel sees {d} input columns")

    def warp(self, X: torch.Tensor) -> torch.Tensor:
        """Phi(X) [..., 2 D] of column-selected inputs [..., D]"""
        X = ops.to_device(X)
        self.check_width(X.shape[-1])
        return ops.periodic_warp(X.reshape(-1, X.shape[-1]), self.period.numpy()).reshape(*X.shape[:-1], 2 * X.shape[-1])

    def slice(self, X, X2=None):
        """the base's column selection, then the warp: what K_into, the fused drivers and `leaf()` take"""
        X, X2 = self.base_kernel.slice(X, X2)
        return self.warp(X), (self.warp(X2) if X2 is not None else None)

    def K(self, X, X2=None) -> torch.Tensor:
        """column-selected, un-warped inputs (the reference's K); batch dimensions as IsotropicStationary.K"""
        X = self.warp(X)
        if X2 is None:
            if X.dim() == 2:
                return self.K_into(X, None, None)
            lead, n = X.shape[:-2], X.shape[-2]
            return torch.stack([self.K_into(x.contiguous(), None, None) for x in X.reshape(-1, n, X.shape[-1])]).reshape(*lead, n, n)
        X2 = self.warp(X2)
        Kf = self.K_into(X.reshape(-1, X.shape[-1]), X2.reshape(-1, X2.shape[-1]), None)
        return Kf.reshape(*X.shape[:-1], *X2.shape[:-1])

    def __call__(self, X, X2=None, *, full_cov: bool = True, presliced: bool = False):
        """gpflow/kernels/base.py:195-214 -- with the base's column selection, since K warps for itself"""
        if (not full_cov) and (X2 is not None):
            raise ValueError("Ambiguous inputs: `not full_cov` and `X2` are not compatible.")
        X = ops.to_device(X)
        X2 = ops.to_device(X2) if X2 is not None else None
        if not presliced:
            X, X2 = self.base_kernel.slice(X, X2)
        if not full_cov:
            self.check_width(X.shape[-1])
            return self.K_diag(X)
        return self.K(X, X2)
