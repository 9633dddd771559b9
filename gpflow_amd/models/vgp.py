"""VGP (gpflow/models/vgp.py:36-180): the full -- non-sparse -- variational GP, any likelihood."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import config, ops
from ..base import Parameter, triangular
from ..conditionals import conditional
from ..kernels import Kernel
from ..likelihoods import Gaussian, Likelihood, SwitchedLikelihood
from ..mean_functions import MeanFunction
from .model import GPModel
from .training_mixins import InternalDataTrainingLossMixin


class VGP(GPModel, InternalDataTrainingLossMixin):
    """q(f) = N(L q_mu + m(X), L S S^T L^T) with L = chol(K(X, X) + jitter I), S_r = tril(q_sqrt[r]): the whitened representation at
    the N data points themselves (vgp.py:38-52).  q_mu [N, R] starts at zero and q_sqrt [R, N, N] at the identity, so q starts at the
    prior.  Its hot path is the product of the two N x N triangles, of which only the row sums of squares are needed
    (ops.tril_product).

    Scope (reverse.vgp_scope, refused when the model is built): a single-output kernel, a zero or constant mean, a Gaussian likelihood
    with one noise variance or any likelihood with a `device_lik` (MultiClass: one latent per class, Y one column of labels), or a
    SwitchedLikelihood (the last column of Y is the task label; at most 16 latents)."""

    def __init__(self, data, kernel: Kernel, likelihood: Likelihood, mean_function: Optional[MeanFunction] = None,
                 num_latent_gps: Optional[int] = None):
        X, Y = data
        if num_latent_gps is None:
            num_latent_gps = self.calc_num_latent_gps_from_data(data, kernel, likelihood)
        super().__init__(kernel, likelihood, mean_function, num_latent_gps)
        n = int(np.shape(X)[0])
        if len(np.shape(X)) != 2 or len(np.shape(Y)) != 2 or int(np.shape(Y)[0]) != n:
            raise ValueError("data must be (X [N, D], Y [N, P])")
        self.num_data = n
        self.q_mu = Parameter(np.zeros((n, self.num_latent_gps)))                                            # [N, R]
        self.q_sqrt = Parameter(np.array([np.eye(n) for _ in range(self.num_latent_gps)]), transform=triangular())   # [R, N, N]
        from . import reverse
        reverse.vgp_scope(self)   # (refused before anything touches the device)
        self.data = (ops.to_device(X), ops.to_device(Y))   # data_input_to_tensor, models/util.py:91-107

    @staticmethod
    def calc_num_latent_gps_from_data(data, kernel, likelihood) -> int:
        """model.py:142-151, with the cases the reference handles in calc_num_latent_gps: a MultiClass likelihood has one latent per
        class, not per column of Y; a SwitchedLikelihood one per VALUE column of Y (GPModel's rule: the last column is the task label)"""
        if hasattr(likelihood, "num_classes"):
            return int(likelihood.num_classes)
        return GPModel.calc_num_latent_gps_from_data(data, kernel, likelihood)

    def maximum_log_likelihood_objective(self):
        return self.elbo()

    def elbo(self) -> torch.Tensor:
        """vgp.py:131-155: sum of the variational expectations at q(f)'s marginals minus KL[q(v) || N(0, I)]"""
        from . import reverse
        reverse.vgp_scope(self)
        X, Y = self.data
        q_mu, q_sqrt = self.q_mu.device_value().contiguous(), self.q_sqrt.device_value().contiguous()
        N = X.shape[0]
        Xs, _ = self.kernel.slice(X, None)
        K = self.kernel.K_into(Xs, None, None, diag_add=config.default_jitter())
        _, info = ops.potrf_(K, N, zero_upper=True)                        # L (zeros above the diagonal)
        ssq, _ = ops.tril_product(K, q_sqrt)                               # fvar^T [R, N]
        f_mean = ops.row_stats(K, V=q_mu, want_sumsq=False)[1] + self.mean_function(X)
        var_exp = self.likelihood.variational_expectations(X, f_mean, ssq.t().contiguous(), Y)
        kl = ops.gauss_kl_white(q_mu, q_sqrt)
        ops.check_info(info)
        return var_exp.sum() - kl[0]

    def elbo_and_grad(self):
        """(ELBO as a float, {Parameter: dELBO/d(unconstrained value) as NumPy}) for the trainable parameters -- what
        `optimizers/scipy.py:322-331` obtains from TF autodiff (gradients.vgp_elbo_and_grad; scope: reverse.vgp_route)."""
        from .. import gradients
        from . import reverse
        lik = self.likelihood
        route, c = reverse.vgp_route(self)   # (refused before anything touches the device)
        X, Y = self.data
        _, Xs, _ = route.inputs(None, X)     # active_dims (kernels/base.py:90-109); nothing is differentiated w.r.t. X
        gaussian, switched = isinstance(lik, Gaussian), isinstance(lik, SwitchedLikelihood)
        kw = dict(noise_variance=lik.noise_variance()) if gaussian else \
            dict(likelihood=("switched", lik.device_members()) if switched else (lik.device_lik, lik.device_params()))
        F, g, info = gradients.vgp_elbo_and_grad(Xs, Y, self.q_mu.device_value(), self.q_sqrt.device_value(), kernel_spec=route.spec,
                                                 jitter=config.default_jitter(), mean_const=c, **kw)
        ops.check_info(info)
        if gaussian:
            lik_pairs = reverse.noise_pairs(lik, X, g["noise_variance"])
        elif switched:   # (out[1 + t] of the stage: task t's Parameter, a Gaussian member's variance included)
            lik_pairs = [(par, g[f"likelihood_{t}"].cpu().numpy()) for t, par in enumerate(lik.device_grad_params()) if par is not None]
        else:
            name = getattr(lik, "device_grad_param", None)   # (the Parameter the kernel's out[1] differentiates, if the class has one)
            lik_pairs = [(getattr(lik, name), g["likelihood_" + name].cpu().numpy())] if name else []
        pairs = route.kernel_pairs(g) + lik_pairs + [(self.q_mu, g["q_mu"].cpu().numpy()), (self.q_sqrt, g["q_sqrt"].cpu().numpy())] \
            + reverse.mean_pairs(self.mean_function, g["mean_const"].cpu().numpy())
        return self._add_log_prior(float(F.cpu()[0]), reverse.to_unconstrained(pairs))

    objective_and_grad = elbo_and_grad   # what optimizers.Scipy calls

    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """vgp.py:157-180: the whitened conditional on the data points, plus the mean"""
        X, _ = self.data
        mu, var = conditional(Xnew, X, self.kernel, self.q_mu.device_value(), q_sqrt=self.q_sqrt.device_value(), full_cov=full_cov,
                              full_output_cov=full_output_cov, white=True)
        return mu + self.mean_function(ops.to_device(Xnew)), var
