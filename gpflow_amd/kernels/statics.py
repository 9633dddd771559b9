"""Static kernels (gpflow/kernels/statics.py): covariances that do not depend on the distance between the inputs.  They
are device-built leaves like the stationary ones -- `gpk_kernel_matrix` fills them without reading X, and inside a Sum /
Product they fold in place through `gpk_kernel_matrix_combine`."""
from __future__ import annotations

from typing import Optional

import torch

from ..base import Parameter, positive
from .. import ops
from .base import ActiveDims, DeviceLeaf


class Static(DeviceLeaf):
    """statics.py `Static`.  `family` names the device code; the builder decides White's diagonal by whether X2 is None, never by
    comparing values, as `White.K` does."""
    family = "Constant"

    def __init__(self, variance=1.0, active_dims: Optional[ActiveDims] = None, name: Optional[str] = None):
        super().__init__(active_dims=active_dims, name=name)
        self.variance = Parameter(variance, transform=positive())

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
