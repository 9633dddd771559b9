"""Kernels on the hot path (gpflow/kernels): stationary and static families built by the HIP covariance builder, the Periodic kernel over them (an input warp in front of the builder), the dot-product kernels Linear and Polynomial (their own builder), the ArcCosine kernel (its own builder too), the Coregion kernel over a column of task labels (a gather from its output covariance), their sums and
products (`+` / `*`, kernels/base.py:216-329), plus the multi-output wrappers SharedIndependent / SeparateIndependent
and the mixing kernel LinearCoregionalization."""
from .base import Combination, Kernel, Product, Sum
from .stationaries import (Stationary, IsotropicStationary, SquaredExponential, Matern12, Matern32,
                           Matern52, Exponential, RationalQuadratic)
from .statics import Static, White, Constant, Bias
from .periodic import Periodic
from .linears import Linear, Polynomial
from .misc import ArcCosine, Coregion
from .changepoints import ChangePoints
from .multioutput import MultioutputKernel, SharedIndependent, SeparateIndependent, LinearCoregionalization

RBF = SquaredExponential  # gpflow/kernels/__init__.py:50

__all__ = ["Kernel", "Combination", "Sum", "Product", "Stationary", "IsotropicStationary", "SquaredExponential", "RBF", "Matern12",
           "Matern32", "Matern52", "Exponential", "RationalQuadratic", "Static", "White", "Constant", "Bias", "Periodic", "Linear", "Polynomial", "ArcCosine", "Coregion", "ChangePoints", "MultioutputKernel", "SharedIndependent", "SeparateIndependent",
           "LinearCoregionalization"]
