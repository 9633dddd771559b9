"""SVGP (gpflow/models/svgp.py:37-261)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import config, kullback_leiblers, ops, posteriors
from ..base import Parameter, positive, triangular
from ..conditionals import conditional
from ..inducing_variables import (InducingPoints, SharedIndependentInducingVariables,
                                  inducingpoint_wrapper)
from ..kernels import Kernel
from ..kernels.base import is_device_leaf
from ..leaf import latent_keywords
from ..likelihoods import Gaussian, Likelihood, MultiClass, ScalarLikelihood, SwitchedLikelihood
from ..mean_functions import MeanFunction
from .model import GPModel
from .reverse import shared_pair
from .training_mixins import ExternalDataTrainingLossMixin


class SVGP(GPModel, ExternalDataTrainingLossMixin):
    def __init__(self, kernel: Kernel, likelihood: Likelihood, inducing_variable, *,
                 mean_function: Optional[MeanFunction] = None, num_latent_gps: int = 1,
                 q_diag: bool = False, q_mu=None, q_sqrt=None, whiten: bool = True, num_data=None):
        super().__init__(kernel, likelihood, mean_function, num_latent_gps)
        self.num_data = num_data
        self.whiten = whiten
        self.inducing_variable = inducingpoint_wrapper(inducing_variable)
        num_inducing = self.inducing_variable.num_inducing
        self._init_variational_parameters(num_inducing, q_mu, q_sqrt, q_diag)
        self._ws = None

    def _init_variational_parameters(self, num_inducing, q_mu, q_sqrt, q_diag) -> None:
        """svgp.py:90-148"""
        q_mu = np.zeros((num_inducing, self.num_latent_gps)) if q_mu is None else q_mu
        self.q_mu = Parameter(q_mu)  # [M, P]
        if q_sqrt is None:
            if q_diag:
                self.q_sqrt = Parameter(np.ones((num_inducing, self.num_latent_gps)), transform=positive())
            else:
                eye = np.array([np.eye(num_inducing) for _ in range(self.num_latent_gps)])
                self.q_sqrt = Parameter(eye, transform=triangular())  # [P, M, M]
        else:
            q_sqrt = np.asarray(q_sqrt, dtype=np.float64)
            if q_diag:
                assert q_sqrt.ndim == 2
                self.num_latent_gps = q_sqrt.shape[1]
                self.q_sqrt = Parameter(q_sqrt, transform=positive())  # [M, L|P]
            else:
                assert q_sqrt.ndim == 3
                self.num_latent_gps = q_sqrt.shape[0]
                self.q_sqrt = Parameter(q_sqrt, transform=triangular())  # [L|P, M, M]

    def prior_kl(self) -> torch.Tensor:
        """svgp.py:153-156"""
        return kullback_leiblers.prior_kl(self.inducing_variable, self.kernel, self.q_mu.device_value(),
                                          self.q_sqrt.device_value(), whiten=self.whiten)

    def maximum_log_likelihood_objective(self, data):
        return self.elbo(data)

    # ---- fused device path ---------------------------------------------------------------------
    def _fused_config(self):
        """(stationary kernel, Z tensor, mean constant) when the whole ELBO shard is one C-ABI call:
        Gaussian likelihood or one of the quadrature likelihoods (Bernoulli, Poisson, StudentT, MultiClass: gpk_svgp_elbo_shard_lik), constant
        mean, and one stationary kernel shared by all latents (plain kernel +
        InducingPoints, or SharedIndependent + SharedIndependentInducingVariables); whitened or not, full or diagonal q_sqrt."""
        if not (isinstance(self.likelihood, Gaussian) or self._device_likelihood()):
            return None
        c = self.mean_function.constant_value()
        if c is None:
            return None
        k, iv = shared_pair(self.kernel, self.inducing_variable)
        if not (is_device_leaf(k) and isinstance(iv, InducingPoints)):
            return None
        return k, iv.Z.device_value(), c

    def _device_likelihood(self) -> bool:
        """a non-Gaussian likelihood whose variational expectations the library computes (ops.LIKELIHOOD_CODES), at most 16 latents;
        MultiClass raises where its classes and the latents do not fit (see below) instead of falling back"""
        lik = self.likelihood
        if isinstance(lik, MultiClass):   # one latent per class, coupled within a row: no chunking past the kernel's 16
            lik.check_device_classes(self.q_mu.shape[1])   # (ValueError: latents != classes; NotImplementedError: more than 16)
            return True
        return isinstance(lik, ScalarLikelihood) and lik.device_lik in ops.LIKELIHOOD_CODES and self.q_mu.shape[1] <= 16

    def _switched_likelihood(self) -> bool:
        """a SwitchedLikelihood with at most 16 latents: the composed ELBO and the quadrature reverse pass take it; the fused shard
        (gpk_svgp_elbo_shard_lik: one code per launch) does not, so `_device_likelihood` stays false for it"""
        return isinstance(self.likelihood, SwitchedLikelihood) and self.q_mu.shape[1] <= 16

    def _fused_separate_config(self):
        """(member kernels, Z [m, d] | [P, m, d], mean constant) when the ELBO shard of a SeparateIndependent model is one
        C-ABI call (gpk_svgp_elbo_shard_sep): whitened, Gaussian likelihood, constant mean, full q_sqrt, stationary members
        over all input columns, inducing POINTS shared by the latents or one equally sized set per latent."""
        from ..kernels import SeparateIndependent
        from ..inducing_variables import SeparateIndependentInducingVariables
        if not self.whiten or not isinstance(self.likelihood, Gaussian):
            return None
        c = self.mean_function.constant_value()
        if c is None:
            return None
        sep = self._separate_stationary_members()
        return None if sep is None else sep + (c,)

    def _separate_stationary_members(self, kernel_class=None):
        """(member kernels, Z [m, d] | [P, m, d]) for SeparateIndependent (or `kernel_class`: LinearCoregionalization, whose members
        are its latents) stationary members over all input columns and inducing points (shared, or one equally sized set per
        latent), full q_sqrt; else None."""
        from ..kernels import SeparateIndependent
        from ..inducing_variables import SeparateIndependentInducingVariables
        if self.q_sqrt.device_value().dim() != 3:
            return None
        k, iv = self.kernel, self.inducing_variable
        if not isinstance(k, kernel_class or SeparateIndependent):
            return None
        # (a kernel that maps its inputs -- Periodic -- is declined: these routes hand the builders RAW inputs; the composed path runs)
        if not all(is_device_leaf(kk) and kk.has_default_active_dims and not kk.maps_inputs for kk in k.kernels):
            return None
        if isinstance(iv, SharedIndependentInducingVariables) and isinstance(iv.inducing_variable, InducingPoints):
            return k.kernels, iv.inducing_variable.Z.device_value().contiguous()
        if isinstance(iv, SeparateIndependentInducingVariables) and len(iv.inducing_variable_list) == len(k.kernels) \
                and all(isinstance(v, InducingPoints) for v in iv.inducing_variable_list):
            Zs = [v.Z.device_value() for v in iv.inducing_variable_list]
            if len({tuple(z.shape) for z in Zs}) == 1:
                return k.kernels, torch.stack(Zs).contiguous()
        return None

    def _check_mixing_widths(self, Y) -> None:
        """LinearCoregionalization: W [P, L] against its L member kernels, the L columns of q_mu and the P columns of Y -- a
        ValueError before anything touches the device"""
        from ..kernels import LinearCoregionalization
        if not isinstance(self.kernel, LinearCoregionalization):
            return
        W = self.kernel.mixing_host()
        if W.shape[1] != self.q_mu.shape[1]:
            raise ValueError(f"LinearCoregionalization: {W.shape[1]} latent kernels, but q_mu has {self.q_mu.shape[1]} columns "
                             "(num_latent_gps is the number of LATENT GPs)")
        if np.shape(Y)[-1] != W.shape[0]:
            raise ValueError(f"LinearCoregionalization: W mixes into {W.shape[0]} outputs, Y has {np.shape(Y)[-1]} columns")

    def _fused_lcm_config(self):
        """(member kernels, Z [m, d] | [L, m, d], W [P, L], mean constant) when the ELBO shard of a LinearCoregionalization model
        is one C-ABI call (gpk_svgp_elbo_shard_lcm): the conditions of `_fused_separate_config` on its L latents, and a CONSTANT
        noise variance (the mixing stage has no per-row form); at most 16 latents and 16 outputs."""
        from ..kernels import LinearCoregionalization
        if not isinstance(self.kernel, LinearCoregionalization):
            return None
        W = self.kernel.mixing_host()
        if not self.whiten or not isinstance(self.likelihood, Gaussian) or self.likelihood.is_heteroskedastic:
            return None
        c = self.mean_function.constant_value()
        if c is None or max(W.shape) > 16:
            return None
        sep = self._separate_stationary_members(LinearCoregionalization)
        return None if sep is None else sep + (W, c)

    def _unwhitened_shared_factor_config(self):
        """(stationary kernel, Z) when the un-whitened ELBO can run on ONE factorisation of Kuu: one stationary kernel
        shared by the latents over inducing points, full q_sqrt."""
        if self.whiten or self.q_sqrt.device_value().dim() != 3:
            return None
        k, iv = shared_pair(self.kernel, self.inducing_variable)
        if not (is_device_leaf(k) and isinstance(iv, InducingPoints)):
            return None
        return k, iv.Z.device_value()

    def _elbo_terms_unwhitened(self, X, Y, k, Z):
        """whiten=False on one trapezoid.  The reference factors Kuu twice per ELBO -- `prior_kl` -> `gauss_kl(K=Kuu)`
        (kullback_leiblers.py:107) and the conditional (conditionals/util.py:67) -- and so did the composed path here: two
        latency chains of 16 panels each (profiles/r04_unwhitened_timeline_before.txt).  Here [Kuu + jitter I ; Kfu ; q_mu^T ;
        tril(q_sqrt_p)^T] goes through ONE factorisation: the minibatch rows come back as A^T = Kfu Lm^-T (util.py:125), the
        others as (Lm^-1 q_mu)^T and (Lm^-1 Lq_p)^T, i.e. the Mahalanobis and trace terms of the KL (:114, :152) -- and, read as
        the whitened parameters of the same q, everything the conditional needs without its second triangular solve (below).
        Cm shape: 4.45 ms (two factorisations) -> 3.72 (one) -> 2.63 ms (no Lm^-T solve of the minibatch rows)."""
        Xs, Zs = k.slice(X, Z)
        q_mu, q_sqrt = self.q_mu.device_value(), self.q_sqrt.device_value()
        M, P = q_mu.shape
        B = Xs.shape[0]
        T = torch.empty((M + B + P + P * M, M), dtype=torch.float64, device=Xs.device)
        k.K_into(Zs, None, T[:M], diag_add=config.default_jitter(), lower_only=True)
        if B:
            k.K_into(Xs, Zs, T[M:M + B])
        T[M + B:M + B + P] = q_mu.t()
        ops.transpose(q_sqrt.contiguous(), mode=1, out=T[M + B + P:].view(P, M, M))       # tril(q_sqrt_p)^T
        _, info = ops.potrf_(T, M)
        # KL[q || N(0, Kuu)]  (kullback_leiblers.py:98-165)
        mahalanobis = ops.sumsq(T[M + B:M + B + P])[0]
        trace = ops.sumsq(T[M + B + P:])[0]
        logdet_qcov = torch.log(torch.diagonal(q_sqrt, dim1=-2, dim2=-1) ** 2).sum()
        kl = 0.5 * (mahalanobis - float(M * P) - logdet_qcov + trace + float(P) * 2.0 * ops.sum_log_diag(T[:M])[0])
        # q(f) at the minibatch (posteriors.py:828-841 -> conditionals/util.py:128-167).  The un-whitened q(u) = N(q_mu, Lq Lq^T)
        # IS the whitened q(v), v = Lm^-1 u, with mean Lm^-1 q_mu and square root G_p = Lm^-1 Lq_p (lower triangular again) --
        # exactly the two blocks of rows the KL needed: fmean = A^T (Lm^-1 q_mu)  and  sum_j (Lq^T Lm^-T A)_j^2 = sum_j (G^T A)_j^2
        # (util.py:139-164 with the Lm^-T solve of the N columns of A folded into the M x M factor).  No second triangular
        # solve of the minibatch rows: M^2 B flop and a 1-ms chain of launches less than the literal form.
        At = T[M:M + B]
        V = T[M + B:M + B + P].t().contiguous()                   # Lm^-1 q_mu  [M, P]
        GT = T[M + B + P:].view(P, M, M)                          # G_p^T (upper): the LqT operand of the projection
        s0, f_mean, _ = ops.row_stats(At, V=V)
        ssq = ops.project(At, GT)
        f_var = (k.K_diag(Xs)[None, :] - s0[None, :] + ssq).t().contiguous()
        f_mean = f_mean + self.mean_function(X)
        var_exp = self.likelihood.variational_expectations(X, f_mean, f_var, Y)
        ops.check_info(info)
        return torch.stack([var_exp.sum(), kl])

    def _elbo_terms_unwhitened_separate(self, X, Y, kernels, Z):
        """`_elbo_terms_unwhitened` for one kernel PER latent (SeparateIndependent): the P trapezoids [Kuu_p ; Kfu_p ; q_mu_p^T ;
        tril(q_sqrt_p)^T] go through ONE batched factorisation; per latent the extra rows are A_p^T, (Lm_p^-1 q_mu_p)^T and
        G_p^T = (Lm_p^-1 Lq_p)^T -- KL terms and whitened parameters of the same q at once (kullback_leiblers.py:98-165 batched
        over K [L,M,M]; conditionals/util.py:566-629 with white = False)."""
        q_mu, q_sqrt = self.q_mu.device_value(), self.q_sqrt.device_value()
        M, P = q_mu.shape
        B = X.shape[0]
        T = torch.empty((P, M + B + 1 + M, M), dtype=torch.float64, device=X.device)
        for p, kp in enumerate(kernels):
            Zp = Z if Z.dim() == 2 else Z[p]
            kp.K_into(Zp, None, T[p, :M], diag_add=config.default_jitter(), lower_only=True)
            if B:
                kp.K_into(X, Zp, T[p, M:M + B])
        T[:, M + B] = q_mu.t()
        ops.transpose(q_sqrt.contiguous(), mode=1, out=T[:, M + B + 1:])                 # tril(q_sqrt_p)^T
        _, info = ops.potrf_(T, M)
        arow = T[:, M + B].contiguous()                                                  # [P, M]: (Lm_p^-1 q_mu_p)^T
        GT = T[:, M + B + 1:].contiguous()                                               # [P, M, M]: G_p^T (upper)
        mahalanobis = ops.sumsq(arow)[0]
        trace = ops.sumsq(GT.reshape(P * M, M))[0]
        logdet_qcov = torch.log(torch.diagonal(q_sqrt, dim1=-2, dim2=-1) ** 2).sum()
        kl = 0.5 * (mahalanobis - float(M * P) - logdet_qcov + trace + 2.0 * ops.sum_log_diag(T[:, :M]).sum())
        s0s, mus = [], []
        for p in range(P):
            s0, mu, _ = ops.row_stats(T[p, M:M + B], V=arow[p].reshape(M, 1).contiguous())
            s0s.append(s0)
            mus.append(mu[:, 0])
        ssq = ops.project(T[:, M:M + B], GT)                                             # [P, B]: sum_j (G_p^T A_p)_j^2
        kdiag = torch.stack([kp.K_diag(X) for kp in kernels])                            # [P, B]
        f_var = (kdiag - torch.stack(s0s) + ssq).t().contiguous()
        f_mean = torch.stack(mus, dim=-1) + self.mean_function(X)
        var_exp = self.likelihood.variational_expectations(X, f_mean, f_var, Y)
        ops.check_info(info)
        return torch.stack([var_exp.sum(), kl])

    def elbo_terms(self, data):
        """(sum_b var_exp_b over the given rows, KL) as a 2-element device tensor -- the two pieces
        svgp.py:172-174 combines; the first is what gets all-reduced when the minibatch is sharded."""
        if isinstance(self.likelihood, MultiClass):   # (refused before anything touches the device)
            self.likelihood.check_device_classes(self.q_mu.shape[1])
        self._check_mixing_widths(data[1])
        X, Y = ops.to_device(data[0]), ops.to_device(data[1])
        fused = self._fused_config()
        if fused is not None:
            k, Z, c = fused
            Xs, Zs = k.slice(X, Z)
            m, rows, d, P = Zs.shape[0], Xs.shape[0], Zs.shape[1], self.q_mu.shape[1]
            q_sqrt = self.q_sqrt.device_value()
            key = (m, rows, d, P, q_sqrt.dim() == 2, bool(self.whiten))
            if self._ws is None or self._ws[0] != key:
                self._ws = (key, ops.svgp_elbo_workspace(m, rows, d, P, q_sqrt.dim() == 2, self.whiten))
            if isinstance(self.likelihood, Gaussian):
                out, info = ops.svgp_elbo_shard(Zs, Xs, Y, self.q_mu.device_value(), q_sqrt, noise_variance=self.likelihood.noise_for(X),
                                                jitter=config.default_jitter(), mean_const=c, ws=self._ws[1], whiten=self.whiten,
                                                **k.leaf().keywords())
            else:
                out, info = ops.svgp_elbo_shard_lik(Zs, Xs, Y, self.q_mu.device_value(), q_sqrt,
                                                    lik=self.likelihood.device_lik, params=self.likelihood.device_params(),
                                                    jitter=config.default_jitter(), mean_const=c, ws=self._ws[1], whiten=self.whiten,
                                                    **k.leaf().keywords())
            ops.check_info(info)
            return out
        sep = self._fused_separate_config()
        if sep is not None:
            kernels, Zs, c = sep
            P, m, d, rows = len(kernels), Zs.shape[-2], Zs.shape[-1], X.shape[0]
            members = latent_keywords([k.leaf() for k in kernels], d)
            key = ("sep", m, rows, d, P)
            if self._ws is None or self._ws[0] != key:
                self._ws = (key, ops.svgp_elbo_sep_workspace(m, rows, d, P))
            out, info = ops.svgp_elbo_shard_sep(Zs, X.contiguous(), Y, self.q_mu.device_value(), self.q_sqrt.device_value(),
                                                noise_variance=self.likelihood.noise_for(X),
                                                jitter=config.default_jitter(), mean_const=c, ws=self._ws[1], **members)
            ops.check_info(info)
            return out
        lcm = self._fused_lcm_config()
        if lcm is not None:
            kernels, Zs, W, c = lcm
            members = latent_keywords([k.leaf() for k in kernels], Zs.shape[-1])
            L, m, d, rows = len(kernels), Zs.shape[-2], Zs.shape[-1], X.shape[0]
            key = ("lcm", m, rows, d, L, W.shape[0])
            if self._ws is None or self._ws[0] != key:
                self._ws = (key, ops.svgp_elbo_lcm_workspace(m, rows, d, L, W.shape[0]))
            out, info = ops.svgp_elbo_shard_lcm(Zs, X.contiguous(), Y, self.q_mu.device_value(), self.q_sqrt.device_value(), W,
                                                noise_variance=float(self.likelihood.noise_for(X)),
                                                jitter=config.default_jitter(), mean_const=c, ws=self._ws[1], **members)
            ops.check_info(info)
            return out
        shared = self._unwhitened_shared_factor_config()
        if shared is not None:
            return self._elbo_terms_unwhitened(X, Y, *shared)
        if not self.whiten:
            members = self._separate_stationary_members()
            if members is not None:
                return self._elbo_terms_unwhitened_separate(X, Y, *members)
        kl = self.prior_kl()
        f_mean, f_var = self.predict_f(X, full_cov=False, full_output_cov=False)
        var_exp = self.likelihood.variational_expectations(X, f_mean, f_var, Y)
        return torch.stack([var_exp.sum(), kl])

    def elbo(self, data) -> torch.Tensor:
        """svgp.py:166-181"""
        X = data[0]
        terms = self.elbo_terms(data)
        if self.num_data is not None:
            scale = float(self.num_data) / float(X.shape[0])
        else:
            scale = 1.0
        return terms[0] * scale - terms[1]

    def elbo_and_grad(self, data):
        """(ELBO on `data` as a float, {Parameter: dELBO/d(unconstrained value) as NumPy}) for the trainable parameters
        -- the pair `optimizers/scipy.py:322-331` gets from TF autodiff over `training_loss_closure(data)`.  Whitened or
        not, SquaredExponential or Matern12 / 32 / 52 kernel (with `active_dims`; shared by the latents or one per latent) or a Sum /
        Product of them, Gaussian likelihood (constant or heteroskedastic noise), or -- whitened, one kernel -- a quadrature likelihood
        (Bernoulli, Poisson, StudentT, MultiClass: the reverse pass seeded per (row, latent) by the kernel's own d/dfmean, d/dfvar);
        InducingPoints, full or diagonal q_sqrt; or a LinearCoregionalization kernel (whitened, full q_sqrt, one noise variance: the
        per-latent passes around one mixing stage, `_elbo_and_grad_lcm`): the scope of reverse.svgp_routes, refused before anything
        touches the device.
        For minibatch training keep the variables on the device instead: training.SVGPTrainer."""
        from .. import gradients
        from . import reverse
        lik = self.likelihood
        quad, switched = isinstance(lik, (ScalarLikelihood, MultiClass, SwitchedLikelihood)), isinstance(lik, SwitchedLikelihood)
        routes, c, separate = reverse.svgp_routes(self, quadrature=quad)
        self._check_mixing_widths(data[1])
        X, Y = ops.to_device(data[0]), ops.to_device(data[1])
        from ..kernels import LinearCoregionalization
        if isinstance(self.kernel, LinearCoregionalization):
            return self._elbo_and_grad_lcm(routes, c, X, Y)
        kw = dict(jitter=config.default_jitter(), scale=reverse.minibatch_scale(self.num_data, X.shape[0]), mean_const=c)
        if quad:
            kw.update(noise_variance=None,
                      likelihood=("switched", lik.device_members()) if switched else (lik.device_lik, lik.device_params()))
        else:
            kw["noise_variance"] = lik.noise_for(X)
        fn = gradients.svgp_elbo_and_grad if self.whiten else gradients.svgp_elbo_and_grad_unwhitened
        q_mu, q_sqrt = self.q_mu.device_value(), self.q_sqrt.device_value()
        # one route; or SeparateIndependent (conditionals/util.py:566-629): L independent single-output problems that share the
        # likelihood, the mean constant and the rows of the minibatch -- ELBO and the shared gradients are their sums, taken on the host
        Fv, kernel_pairs, zgrads, hosts, noise_rows = 0.0, [], {}, [], []
        for p_, (route, iv) in enumerate(routes):
            cols = slice(p_, p_ + 1) if separate else slice(None)
            Zs, Xs, scatter = route.inputs(iv.Z.device_value(), X)
            F, g, info = fn(Zs, Xs, Y[:, cols].contiguous(), q_mu[:, cols].contiguous(), q_sqrt[cols].contiguous(),
                            kernel_spec=route.spec, **kw)
            ops.check_info(info)
            Fv += float(F.cpu()[0])
            kernel_pairs += route.kernel_pairs(g)
            # (the kernel's entries went through route.kernel_pairs; in a combination each is a list with one entry per member)
            kernel_names = {"variance", "lengthscales", "alpha", "period", "offset", "changepoints", "Z"} \
                | {n for i in range(route.spec.n) for n in route.spec.parameter_names(i)}
            host = {n: g[n].cpu().numpy() for n in g if n not in kernel_names}
            gz = scatter(g["Z"]).cpu().numpy()
            zgrads[id(iv.Z)] = (iv.Z, zgrads[id(iv.Z)][1] + gz if id(iv.Z) in zgrads else gz)   # shared Z: contributions add up
            hosts.append(host)
            noise_rows.append(g.get("noise_variance"))     # (on the device: what the noise Function's reverse pass takes)
        total = lambda n: sum((h[n] for h in hosts[1:]), hosts[0][n])  # noqa: E731
        q_pairs = [(self.q_mu, np.concatenate([h["q_mu"] for h in hosts], axis=1)),
                   (self.q_sqrt, np.concatenate([h["q_sqrt"] for h in hosts], axis=0))]
        if switched:   # (out[1 + t] of the stage: task t's Parameter, a Gaussian member's variance included)
            lik_pairs = [(par, hosts[0][f"likelihood_{t}"]) for t, par in enumerate(lik.device_grad_params()) if par is not None]
        elif quad:
            name = getattr(lik, "device_grad_param", None)   # (the Parameter the kernel's out[1] differentiates, if the class has one)
            lik_pairs = [(getattr(lik, name), hosts[0]["likelihood_" + name])] if name else []
        else:
            # (the latents share the likelihood: their per-row dF/d sigma_n^2 add up before the noise Function's reverse pass)
            g_noise = total("noise_variance")
            if lik.is_heteroskedastic:
                g_noise = ops.to_device(np.asarray(g_noise)) if separate else noise_rows[0]
            lik_pairs = reverse.noise_pairs(lik, X, g_noise)
        # (the order of the pairs is the order of the returned dict, which optimizers.Scipy packs by: the noise comes before q(u)
        #  unless the route is a combination)
        noise_first = not quad and not routes[0][0].is_combination
        pairs = kernel_pairs + list(zgrads.values()) + (lik_pairs + q_pairs if noise_first else q_pairs + lik_pairs) \
            + reverse.mean_pairs(self.mean_function, total("mean_const"))
        return self._add_log_prior(Fv, reverse.to_unconstrained(pairs))   # (+ log prior density of the trainable parameters: model.py:56-76)

    def _elbo_and_grad_lcm(self, routes, c, X, Y):
        """`elbo_and_grad` of a LinearCoregionalization model (the scope of reverse.svgp_routes for it): the per-latent passes share
        the mixing stage, which also carries the gradients of W, the noise variance and the mean constant."""
        from .. import gradients
        from . import reverse
        lik = self.likelihood
        ins = [route.inputs(iv.Z.device_value(), X) for route, iv in routes]
        F, g, info = gradients.svgp_elbo_and_grad_lcm(
            [i[0] for i in ins], [i[1] for i in ins], Y, self.q_mu.device_value(), self.q_sqrt.device_value(), self.kernel.W.numpy(),
            kernel_specs=[route.spec for route, _ in routes], noise_variance=float(lik.noise_for(X)),
            jitter=config.default_jitter(), scale=reverse.minibatch_scale(self.num_data, X.shape[0]), mean_const=c)
        ops.check_info(info)
        kernel_pairs, zgrads = [], {}
        for (route, iv), (_, _, scatter), gl in zip(routes, ins, g["latents"]):
            kernel_pairs += route.kernel_pairs(gl)
            gz = scatter(gl["Z"]).cpu().numpy()
            zgrads[id(iv.Z)] = (iv.Z, zgrads[id(iv.Z)][1] + gz if id(iv.Z) in zgrads else gz)   # shared Z: contributions add up
        q_pairs = [(self.q_mu, torch.cat([gl["q_mu"] for gl in g["latents"]], dim=1).cpu().numpy()),
                   (self.q_sqrt, torch.cat([gl["q_sqrt"] for gl in g["latents"]], dim=0).cpu().numpy())]
        pairs = kernel_pairs + [(self.kernel.W, g["W"].cpu().numpy())] + list(zgrads.values()) \
            + reverse.noise_pairs(lik, X, g["noise_variance"]) + q_pairs + reverse.mean_pairs(self.mean_function, g["mean_const"].cpu().numpy())
        return self._add_log_prior(float(F.cpu()[0]), reverse.to_unconstrained(pairs))

    def posterior(self, precompute_cache=posteriors.PrecomputeCacheType.TENSOR):
        """svgp.py:210-240"""
        return posteriors.create_posterior(self.kernel, self.inducing_variable, self.q_mu, self.q_sqrt,
                                           whiten=self.whiten, mean_function=self.mean_function,
                                           precompute_cache=precompute_cache)

    def predict_f(self, Xnew, full_cov: bool = False, full_output_cov: bool = False):
        """svgp.py:243-255"""
        return self.posterior(posteriors.PrecomputeCacheType.NOCACHE).fused_predict_f(
            Xnew, full_cov=full_cov, full_output_cov=full_output_cov)
