"""The Convolutional kernel (gpflow/kernels/convolutional.py): a base kernel over the patches of an image, summed with one weight per
patch.  Its inducing variable is inducing_variables.InducingPatches, and its three covariances come from three places: Kuu is the base
kernel over the inducing patches (the stationary builder), Kfu and K_diag are the patch-response kernels of csrc/conv/conv.hip, which
stage an image in LDS and never materialise its patches."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..base import Parameter
from .. import ops
from .base import Kernel
from .stationaries import SquaredExponential


class Convolutional(Kernel):
    """convolutional.py: `image_shape` [H, W], `patch_shape` [h, w], `colour_channels` C; an input row is the image [H, W, C] flattened
    with the channel fastest, every channel an image of its own.  Built here for ONE SquaredExponential base kernel with a scalar
    lengthscale over all patch elements; the limits of include/gpk.h (H W C <= 4096, h w <= 64) are a ValueError.  K(X, X2) -- N x N2 x
    P^2 base-kernel evaluations, needed only by the dense models and full_cov=True -- is not built."""
    patch_kernel = True

    def __init__(self, base_kernel: Kernel, image_shape, patch_shape, weights=None, colour_channels: int = 1, name: Optional[str] = None):
        super().__init__(name=name)
        if type(base_kernel) is not SquaredExponential or base_kernel.ard or not base_kernel.has_default_active_dims:
            raise NotImplementedError("Convolutional: the base kernel is one SquaredExponential with a scalar lengthscale and default "
                                      "active_dims (ARD and the other families are not built into the patch-response kernels)")
        self.geometry = ops.conv_geometry(image_shape, patch_shape, colour_channels)
        self.image_shape, self.patch_shape, self.colour_channels = tuple(self.geometry[:2]), tuple(self.geometry[3:]), self.geometry[2]
        self.base_kernel = base_kernel
        w = np.ones(self.num_patches) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (self.num_patches,):
            raise ValueError(f"Convolutional: weights must be [{self.num_patches}], one per patch")
        self.weights = Parameter(w)

    @property
    def num_patches(self) -> int:
        return ops.conv_num_patches(self.geometry)

    @property
    def patch_len(self) -> int:
        return self.patch_shape[0] * self.patch_shape[1]

    def keywords(self) -> dict:
        """what the ops.conv_* wrappers take: the geometry and the current host values"""
        return dict(geometry=self.geometry, weights=self.weights.numpy(), variance=float(self.base_kernel.variance.numpy()),
                    lengthscales=float(self.base_kernel.lengthscales.numpy()))

    def get_patches(self, X) -> torch.Tensor:
        """[N, P, h w]: every patch of every image, in the kernel's order -- a host-side unfold for users, on no model route"""
        H, W, C, h, w = self.geometry
        X = np.asarray(X.cpu() if torch.is_tensor(X) else X, dtype=np.float64).reshape(-1, H, W, C)
        win = np.lib.stride_tricks.sliding_window_view(X, (h, w), axis=(1, 2))          # [N, oh, ow, C, h, w]
        return torch.as_tensor(np.ascontiguousarray(win.transpose(0, 3, 1, 2, 4, 5)).reshape(X.shape[0], self.num_patches, h * w))

    def K(self, X, X2=None):
        raise NotImplementedError("Convolutional.K(X, X2): the N x N2 x P^2 form is not built (GPR, SGPR, VGP and full_cov=True need it); "
                                  "SVGP over InducingPatches takes Kuu, Kuf and K_diag")

    def K_into(self, X, X2, out, **kwargs):
        return self.K(X, X2)

    def K_diag(self, X) -> torch.Tensor:
        X = ops.to_device(X)
        return ops.conv_kdiag(X.reshape(-1, X.shape[-1]).contiguous(), **self.keywords()).reshape(X.shape[:-1])

    def Kuu_into(self, Z, out, *, diag_add: float = 0.0, lower_only: bool = False):
        """the base kernel over the inducing patches"""
        return self.base_kernel.K_into(Z, None, out, diag_add=diag_add, lower_only=lower_only)

    def Kfu_into(self, X, Z, out):
        return ops.conv_kfu(X, Z, out=out, **self.keywords())
