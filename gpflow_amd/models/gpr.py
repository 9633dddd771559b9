"""GPR (gpflow/models/gpr.py:36-196)."""
from __future__ import annotations

from typing import Optional

import torch

from .. import ops, posteriors
from ..kernels import Kernel
from ..kernels.base import is_device_leaf
from ..likelihoods import Gaussian
from ..logdensities import multivariate_normal
from ..mean_functions import MeanFunction
from .model import GPModel
from .training_mixins import InternalDataTrainingLossMixin


class GPR(GPModel, InternalDataTrainingLossMixin):
    def __init__(self, data, kernel: Kernel, mean_function: Optional[MeanFunction] = None,
                 noise_variance=None, likelihood: Optional[Gaussian] = None):
        assert (noise_variance is None) or (likelihood is None), \
            "Cannot set both `noise_variance` and `likelihood`."
        if likelihood is None:
            if noise_variance is None:
                noise_variance = 1.0
            likelihood = Gaussian(noise_variance)
        X, Y = data
        self.data = (ops.to_device(X), ops.to_device(Y))  # data_input_to_tensor, models/util.py:91-107
        if self.data[0].dim() != 2 or self.data[1].dim() != 2 or self.data[0].shape[0] != self.data[1].shape[0]:
            raise ValueError("data must be (X [N,D], Y [N,P])")
        super().__init__(kernel, likelihood, mean_function, num_latent_gps=self.data[1].shape[-1])
        self._ws = None

    def maximum_log_likelihood_objective(self):
        return self.log_marginal_likelihood()

    def log_marginal_likelihood(self) -> torch.Tensor:
        """gpr.py:91-107.  With a stationary kernel and a constant mean the whole chain
        K -> +noise -> cholesky -> triangular_solve -> reductions is ONE C-ABI call (gpk_gpr_lml);
        otherwise it is composed from the same primitives."""
        X, Y = self.data
        c = self.mean_function.constant_value()
        if is_device_leaf(self.kernel) and c is not None:
            Xs, _ = self.kernel.slice(X, None)
            out, info = ops.gpr_lml(Xs, Y, noise_variance=self.likelihood.noise_for(X), mean_const=c, ws=self._ws,
                                    **self.kernel.leaf().keywords())
            ops.check_info(info)
            return out[0]
        K = self.kernel(X)
        n = K.shape[0]
        if self.likelihood.is_heteroskedastic:   # add_likelihood_noise_cov, model_utils.py:46-50
            ops.diag_add_(K, self.likelihood.noise_for(X))
        else:
            idx = torch.arange(n, device=K.device)
            K[idx, idx] += self.likelihood.noise_variance()  # add_noise_cov, model_utils.py:33-38
        _, info = ops.potrf_(K, n, zero_upper=True)
        ops.check_info(info)
        m = self.mean_function(X)
        return multivariate_normal(Y, m, K).sum()

    def log_marginal_likelihood_and_grad(self):
        """(LML as a float, {Parameter: dLML/d(unconstrained value) as NumPy}) for the trainable parameters -- what
        `optimizers/scipy.py:322-331` obtains from TF autodiff.  SquaredExponential or Matern12 / 32 / 52 kernel (with `active_dims`) or a Sum /
        Product of them, constant / zero mean, constant or heteroskedastic noise (gradients.gpr_lml_and_grad); anything else raises
        NotImplementedError."""
        from .. import gradients
        from . import reverse
        lik = self.likelihood
        route, c = reverse.regression_route(self)   # (refused before anything touches the device)
        X, Y = self.data
        _, Xs, _ = route.inputs(None, X)            # active_dims (kernels/base.py:90-109); nothing is differentiated w.r.t. X
        # (a heteroskedastic likelihood: d LML / d sigma_n^2 per row, chained through the noise function's own reverse pass)
        lml, g, info = gradients.gpr_lml_and_grad(Xs, Y, noise_variance=lik.noise_for(X), mean_const=c, kernel_spec=route.spec)
        ops.check_info(info)
        pairs = route.kernel_pairs(g) + reverse.noise_pairs(lik, X, g["noise_variance"]) \
            + reverse.mean_pairs(self.mean_function, g["mean_const"].cpu().numpy())
        # with parameter priors this is the log POSTERIOR density and its gradient: -training_loss (model.py:56-76)
        return self._add_log_prior(float(lml.cpu()[0]), reverse.to_unconstrained(pairs))

    objective_and_grad = log_marginal_likelihood_and_grad   # what optimizers.Scipy calls

    def posterior(self, precompute_cache=posteriors.PrecomputeCacheType.TENSOR) -> posteriors.GPRPosterior:
        """gpr.py:146-175"""
        return posteriors.GPRPosterior(kernel=self.kernel, data=self.data, likelihood=self.likelihood,
                                       mean_function=self.mean_function,
                                       precompute_cache=posteriors._validate_precompute_cache_type(precompute_cache)
                                       if precompute_cache is not None else None)

    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """gpr.py:178-190: fused (no-cache) prediction."""
        return self.posterior(posteriors.PrecomputeCacheType.NOCACHE).fused_predict_f(
            Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
