"""Static kernels (gpflow/kernels/statics.py): covariances that do not depend on the distance between the inputs.  They
are device-built leaves like the stationary ones -- `gpk_kernel_matrix` fills them without reading X, and inside a Sum /
Product they fold in place through `gpk_kernel_matrix_combine`."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..base import Parameter, positive
from .. import ops
from .base import ActiveDims, Kernel


class Static(Kernel):
    """statics.py `Static`.  `family` names the device code; the builder decides White's diagonal by whether X2 is None, never by
    comparing values, as `White.K` does."""
    family = "Constant"
    device_leaf = True

    def __init__(self, variance=1.0, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        super().__init__(active_dims=active_dims, name=name)
        self.variance = Parameter(variance, transform=positive())

    def K_diag(self, X) -> torch.Tensor:
        """`Static.K_diag`: fill(X.shape[:-1], variance)"""
        X = ops.to_device(X)
        return torch.full(X.shape[:-1], float(self.variance.numpy()), dtype=torch.float64, device=X.device)

    def hyper(self):
        """(family, variance, lengthscales) as host values for the C-ABI; a static kernel has no lengthscale and hands the
        builder a dummy 1.0 that is never read."""
        return self.family, float(self.variance.numpy()), np.asarray(1.0, dtype=np.float64)

    def hyper_alpha(self):
        return None

    def hyper_extra(self) -> dict:
        return {}

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        family, var, ls = self.hyper()
        return ops.kernel_matrix(X, X2, variance=var, lengthscales=ls, family=family, diag_add=diag_add,
                                 lower_only=lower_only, out=out)

    def K(self, X, X2=None) -> torch.Tensor:
        X = ops.to_device(X)
        if X.dim() != 2 or (X2 is not None and ops.to_device(X2).dim() != 2):
            raise NotImplementedError("static kernels take [N, D] inputs")
        return self.K_into(X, ops.to_device(X2) if X2 is not None else None, None)


class White(Static):
    """statics.py `White`: variance * I for K(X), zeros [N, N2] for K(X, X2) -- even if X2 equals X in value."""
    family = "White"


class Constant(Static):
    """statics.py `Constant`: variance everywhere."""
    family = "Constant"


Bias = Constant  # the reference's alias
