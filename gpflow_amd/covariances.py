"""Kuu / Kuf (gpflow/covariances/{kuus,kufs}.py, multioutput/{kuus,kufs}.py) for the inducing-point x
stationary-kernel pairs on the path.  The reference dispatches on (inducing type, kernel type) with
multipledispatch; here the same table is a plain isinstance ladder."""
from __future__ import annotations

import torch

from . import ops
from .inducing_variables import (InducingPatches, InducingPoints, Multiscale, SeparateIndependentInducingVariables,
                                 SharedIndependentInducingVariables)
from .kernels import Kernel, LinearCoregionalization, MultioutputKernel, SeparateIndependent, SharedIndependent, SquaredExponential


def _pairs(inducing_variable, kernel):
    """(Z tensor, latent kernel) per latent GP for the Separate* combinations
    (multioutput/kuus.py:65-121, kufs.py:63-115)."""
    if isinstance(kernel, (SeparateIndependent, LinearCoregionalization)):   # (the latter: Kuu / Kuf of its L LATENT GPs)
        ks = list(kernel.latent_kernels)
    elif isinstance(kernel, SharedIndependent):
        ks = None
    else:
        raise NotImplementedError(f"Kuu/Kuf: unsupported kernel {type(kernel).__name__}")
    if isinstance(inducing_variable, SeparateIndependentInducingVariables):
        zs = [iv.Z.device_value() for iv in inducing_variable.inducing_variable_list]
    elif isinstance(inducing_variable, SharedIndependentInducingVariables):
        zs = None
    else:
        raise NotImplementedError(f"Kuu/Kuf: unsupported inducing variable {type(inducing_variable).__name__}")
    L = len(ks) if ks is not None else len(zs)
    if ks is None:
        ks = [kernel.kernel] * L
    if zs is None:
        zs = [inducing_variable.inducing_variable.Z.device_value()] * L
    if len(ks) != len(zs):
        raise ValueError("number of kernels and of inducing-variable sets differ")
    return list(zip(zs, ks))


def patch_pair(inducing_variable, kernel) -> bool:
    """True for (InducingPatches, Convolutional) -- kuus.py / kufs.py register exactly this pair -- and NotImplementedError for either
    half with anything else, before the device is touched"""
    patches, conv = isinstance(inducing_variable, InducingPatches), bool(getattr(kernel, "patch_kernel", False))
    if patches != conv:
        raise NotImplementedError(f"Kuu/Kuf: ({type(inducing_variable).__name__}, {type(kernel).__name__}) -- a Convolutional kernel "
                                  "goes with InducingPatches, and InducingPatches with no other kernel")
    return patches


def multiscale_pair(inducing_variable, kernel) -> bool:
    """True for (Multiscale, SquaredExponential) -- the one pair kuus.py / kufs.py register for Multiscale -- and NotImplementedError for
    Multiscale, bare or inside a multi-output wrapper, with anything else, before the device is touched"""
    inner = getattr(inducing_variable, "inducing_variables", ())
    if any(isinstance(v, Multiscale) for v in inner):
        raise NotImplementedError("Kuu/Kuf: Multiscale inducing variables inside Shared / SeparateIndependentInducingVariables are not built: "
                                  "the multi-output rows of kuus.py / kufs.py take inducing points")
    if not isinstance(inducing_variable, Multiscale):
        return False
    if type(kernel) is not SquaredExponential:
        raise NotImplementedError(f"Kuu/Kuf: (Multiscale, {type(kernel).__name__}) -- Multiscale inducing variables go with one "
                                  "SquaredExponential kernel: no other family, combination, Periodic, Convolutional or multi-output wrapper")
    return True


def multiscale_operands(inducing_variable, kernel, X=None):
    """(Z, scales, X) on the device as the multiscale builders take them: all three sliced by the kernel's `active_dims`; a width above
    ops.MAX_D is a ValueError before the device"""
    dims, D = kernel._active_dims, int(inducing_variable.Z.shape[1])
    width = len(range(D)[dims]) if isinstance(dims, slice) else len(dims)
    if width > ops.MAX_D:
        raise ValueError(f"Multiscale: {width} input columns, the builders take up to {ops.MAX_D}")
    Zs, Ss = kernel.slice(inducing_variable.Z.device_value(), inducing_variable.scales.device_value())
    return Zs, Ss, (None if X is None else kernel.slice(ops.to_device(X), None)[0])


def multiscale_Kuu(inducing_variable, kernel, out=None, *, jitter: float = 0.0):
    Zs, Ss, _ = multiscale_operands(inducing_variable, kernel)
    leaf = kernel.leaf()
    return ops.multiscale_kuu(Zs, Ss, variance=leaf.variance, lengthscales=leaf.lengthscales, diag_add=jitter, out=out)


def multiscale_Kfu(inducing_variable, kernel, Xnew, out=None):
    Zs, Ss, Xs = multiscale_operands(inducing_variable, kernel, Xnew)
    leaf = kernel.leaf()
    return ops.multiscale_kfu(Xs, Zs, Ss, variance=leaf.variance, lengthscales=leaf.lengthscales, out=out)


def Kuu(inducing_variable, kernel, *, jitter: float = 0.0) -> torch.Tensor:
    """[M,M] (InducingPoints x Kernel: kuus.py:24-34; Multiscale x SquaredExponential: kuus.py:37-57; Shared x Shared:
    multioutput/kuus.py:49-62) or [L,M,M] (any Separate combination: multioutput/kuus.py:65-121)."""
    if multiscale_pair(inducing_variable, kernel):
        return multiscale_Kuu(inducing_variable, kernel, jitter=jitter)
    if patch_pair(inducing_variable, kernel):
        return kernel.Kuu_into(inducing_variable.Z.device_value(), None, diag_add=jitter)
    if isinstance(inducing_variable, InducingPoints) and not isinstance(kernel, MultioutputKernel):
        Z = inducing_variable.Z.device_value()
        Zs, _ = kernel.slice(Z, None)
        return kernel.K_into(Zs, None, None, diag_add=jitter)
    if isinstance(inducing_variable, SharedIndependentInducingVariables) and isinstance(kernel, SharedIndependent):
        return Kuu(inducing_variable.inducing_variable, kernel.kernel, jitter=jitter)
    pairs = _pairs(inducing_variable, kernel)
    return torch.stack([k.K_into(k.slice(z, None)[0], None, None, diag_add=jitter) for z, k in pairs], dim=0)


def Kfu(inducing_variable, kernel, Xnew) -> torch.Tensor:
    """K(Xnew, Z): the row-major [N,M] (or [L,N,M]) layout the device solves consume."""
    if multiscale_pair(inducing_variable, kernel):   # (refused, or its width checked, before Xnew is copied to the device)
        return multiscale_Kfu(inducing_variable, kernel, Xnew)
    if patch_pair(inducing_variable, kernel):   # (a half pair is refused here, before Xnew is copied to the device)
        return kernel.Kfu_into(ops.to_device(Xnew), inducing_variable.Z.device_value(), None)
    Xnew = ops.to_device(Xnew)
    if isinstance(inducing_variable, InducingPoints) and not isinstance(kernel, MultioutputKernel):
        Z = inducing_variable.Z.device_value()
        Xs, Zs = kernel.slice(Xnew, Z)
        return kernel.K_into(Xs, Zs, None)
    if isinstance(inducing_variable, SharedIndependentInducingVariables) and isinstance(kernel, SharedIndependent):
        return Kfu(inducing_variable.inducing_variable, kernel.kernel, Xnew)
    pairs = _pairs(inducing_variable, kernel)
    outs = []
    for z, k in pairs:
        Xs, Zs = k.slice(Xnew, z)
        outs.append(k.K_into(Xs, Zs, None))
    return torch.stack(outs, dim=0)


def Kuf(inducing_variable, kernel, Xnew) -> torch.Tensor:
    """[M,N] (kufs.py:25-34, multioutput/kufs.py:49-60) or [L,M,N] (kufs.py:63-115) -- returned as a
    transposed view of the [N,M] buffer built by Kfu."""
    return Kfu(inducing_variable, kernel, Xnew).transpose(-1, -2)
