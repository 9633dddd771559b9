"""The ChangePoints kernel (gpflow/kernels/changepoints.py): a combination that switches between covariance regimes along ONE input
column -- a time series whose lengthscale changes at t = 3, say.

    sig_j(x) = 1 / (1 + exp(-s_j (x - l_j)))          l sorted, s_j > 0 (a scalar steepness stands for all C)
    a_i(x)   = sig_{i-1}(x) (1 - sig_i(x))            i = 0 .. C        (sig_{-1} = 1, 1 - sig_C = 1)
    K(x, y)  = sum_i a_i(x) k_i(x, y) a_i(y)          K_diag(x) = sum_i a_i(x)^2 k_i(x, x)

with x the column `switch_dim` of the UNSLICED input; every member slices its own `active_dims`.  The weights come from
gpk_changepoint_weights and each member's matrix is weighted and added in ONE pass by gpk_changepoint_fold
(csrc/changepoints/changepoints.hip): the first member is built into the result and weighted in place, every further member is built
once into one reused temporary.  It is the one combination with parameters of its own (`locations`, `steepness`); in the reverse pass
it is a node of its own kind in gradients.KernelSpec.  K(x, x) depends on the row, so every fused route declines it and the composed
routes run (models.reverse.has_row_diagonal)."""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..base import Parameter, positive
from .. import ops
from .base import Combination, Kernel


class ChangePoints(Combination):
    """changepoints.py `ChangePoints(kernels, locations, steepness=1.0, switch_dim=0)`; nested instances are NOT flattened (each has
    its own change points).  `locations` may be given in any order: they reach the device sorted (a stable argsort on the host) and
    their gradient comes back in the given order, as through the reference's tf.sort; `steepness[j]` goes with the j-th SORTED
    location, as in the reference."""

    _op = "cp"
    max_members = ops.CP_MAX_MEMBERS

    def __init__(self, kernels: Sequence[Kernel], locations, steepness=1.0, switch_dim: int = 0, name: Optional[str] = None):
        Kernel.__init__(self, name=name)
        kernels = list(kernels)
        if not all(isinstance(k, Kernel) for k in kernels):
            raise TypeError("can only combine Kernel instances")
        loc = np.asarray(locations, dtype=np.float64)
        if loc.ndim > 1 or len(kernels) != loc.size + 1:
            raise ValueError(f"ChangePoints: {len(kernels)} kernels need {len(kernels) - 1} locations, got {loc.size}")
        st = np.asarray(steepness, dtype=np.float64)
        if st.ndim > 1 or (st.ndim == 1 and st.size != loc.size):
            raise ValueError(f"ChangePoints: a steepness list needs one entry per location ({loc.size}), got {st.size}")
        if int(switch_dim) != switch_dim or int(switch_dim) < 0:
            raise ValueError("ChangePoints: switch_dim is a column index and must not be negative")
        if len(kernels) > self.max_members:
            raise NotImplementedError(f"ChangePoints: more than {self.max_members} member kernels")
        self.kernels = kernels
        self.locations = Parameter(loc.reshape(-1))
        self.steepness = Parameter(st, transform=positive())
        self.switch_dim = int(switch_dim)

    def node(self):
        """the node's current host values as the reverse pass and the builders take them (gradients.ChangePointsNode)"""
        from ..gradients import ChangePointsNode
        return ChangePointsNode(self.locations.numpy(), self.steepness.numpy(), self.switch_dim)

    def node_params(self) -> tuple:
        return self.locations, self.steepness

    def weights(self, X) -> torch.Tensor:
        """A [T, rows]: a_i over the switch column of the unsliced X"""
        nd = self.node()
        if self.switch_dim >= X.shape[-1]:
            raise ValueError(f"ChangePoints: switch_dim {self.switch_dim} is outside the {X.shape[-1]} input columns")
        return ops.changepoint_weights(X[:, self.switch_dim], locations=nd.locations, steepness=nd.steepness)

    def K_into(self, X, X2, out, *, diag_add: float = 0.0, lower_only: bool = False):
        X = ops.to_device(X)
        X2 = ops.to_device(X2) if X2 is not None else None
        A = self.weights(X)
        B = None if X2 is None else self.weights(X2)
        ks = list(self.kernels)
        last = len(ks) - 1
        Xs, X2s = ks[0].slice(X, X2)
        out = ks[0].K_into(Xs, X2s, out)
        ops.changepoint_fold(A[0], None if B is None else B[0], out, diag_add=diag_add if last == 0 else 0.0, out=out)
        tmp = None
        for i, k in enumerate(ks[1:], start=1):
            Xs, X2s = k.slice(X, X2)
            tmp = k.K_into(Xs, X2s, tmp)
            ops.changepoint_fold(A[i], None if B is None else B[i], tmp, out, diag_add=diag_add if i == last else 0.0, out=out)
        return out

    def K(self, X, X2=None) -> torch.Tensor:
        X = ops.to_device(X)
        if X.dim() != 2 or (X2 is not None and ops.to_device(X2).dim() != 2):
            raise NotImplementedError("kernel combinations take [N, D] inputs")
        return self.K_into(X, X2, None)

    def K_diag(self, X) -> torch.Tensor:
        """sum_i a_i^2 kd_i with the weight formed first, as the fold forms it: bit for bit the diagonal of K(X, X) wherever every
        member's own K_diag is (vectors of length n: torch elementwise, not the hot path)"""
        X = ops.to_device(X)
        A, acc = self.weights(X), None
        for i, k in enumerate(self.kernels):
            term = (A[i] * A[i]) * k(X, full_cov=False)
            acc = term if acc is None else acc + term
        return acc
