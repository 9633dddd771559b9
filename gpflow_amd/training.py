"""Device-resident training loop for the SVGP, whitened or not (SquaredExponential kernel, Gaussian likelihood) -- the caller
of the hot path that SURVEY 8f row 1 names: the Adam loop of `gps_for_big_data.pct.py:207-228`
(`tf.optimizers.Adam().minimize(model.training_loss_closure(iter), model.trainable_variables)`).

The reference keeps variables in TF and differentiates through them; here the big variables (q_mu, q_sqrt, Z) and their
Adam moments stay in HBM, the handful of scalar hyper-parameters live on the host in unconstrained form (their
constrained values are C-ABI arguments), and one step is
    gradients.svgp_elbo_and_grad  ->  (multi-GPU: one all-reduce of the packed gradient)  ->  Adam update.
The update rule and defaults are tf.keras Adam's (lr 1e-3, beta 0.9 / 0.999, epsilon 1e-7, bias-corrected step size).
The Adam arithmetic on the device tensors is one launch per variable (`gpk_adam_step`).
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import config, distributed, gradients, ops


class _Adam:
    def __init__(self, lr: float, b1: float, b2: float, eps: float):
        self.lr, self.b1, self.b2, self.eps, self.t = lr, b1, b2, eps, 0
        self.m: Dict[str, object] = {}
        self.v: Dict[str, object] = {}

    def step_size(self) -> float:
        return self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)

    def update_device(self, name: str, p: torch.Tensor, g: torch.Tensor) -> None:
        if name not in self.m:
            self.m[name], self.v[name] = torch.zeros_like(p), torch.zeros_like(p)
        m, v = self.m[name], self.v[name]
        # (one launch per variable -- gpk_adam_step -- instead of seven elementwise passes over q_sqrt's M^2 entries)
        ops.adam_step_(p, g.contiguous(), m, v, beta1=self.b1, beta2=self.b2, epsilon=self.eps, step=self.step_size())

    def update_host(self, name: str, p: np.ndarray, g: np.ndarray) -> np.ndarray:
        if name not in self.m:
            self.m[name], self.v[name] = np.zeros_like(p), np.zeros_like(p)
        self.m[name] = self.b1 * self.m[name] + (1.0 - self.b1) * g
        self.v[name] = self.b2 * self.v[name] + (1.0 - self.b2) * g * g
        return p - self.step_size() * self.m[name] / (np.sqrt(self.v[name]) + self.eps)


class SVGPTrainer:
    """Adam on -ELBO for `model` (SVGP: whitened or un-whitened, full or diagonal q_sqrt, SquaredExponential / Matern kernel with
    or without `active_dims` -- or a Sum / Product of such kernels, flat or nested, or one kernel per latent over shared inducing points --, Gaussian likelihood with a constant variance or a noise Function of the inputs, InducingPoints, constant or zero mean).  Honours `Parameter.trainable` (including a trainable
    `Constant.c`).  A step whose Kuu factorisation fails raises and leaves variables and Adam moments untouched.

        trainer = SVGPTrainer(model, learning_rate=1e-3)
        for Xb, Yb in batches:            # device or host arrays; with torch.distributed initialised each rank passes
            elbo = trainer.step((Xb, Yb))  # ITS row shard of the global minibatch (global_batch = total rows)
        trainer.sync_to_model()           # write the trained values back into the model's Parameters
    """

    def __init__(self, model, *, learning_rate: float = 1e-3, beta_1: float = 0.9, beta_2: float = 0.999,
                 epsilon: float = 1e-7, natgrad_gamma: Optional[float] = None, group=None):
        """natgrad_gamma: if given, (q_mu, q_sqrt) take a natural-gradient step of that size per iteration
        (optimizers/natgrad.py; natgrad.natgrad_update on the device) and Adam handles the remaining parameters -- the
        hybrid recipe of the reference's natural-gradient notebook, from ONE gradient evaluation per step."""
        # NotImplementedError outside the scope of the reverse pass (models/reverse.py).  One route per covariance function: one for a
        # stationary kernel or a Sum / Product of them (flat or nested, members over their own columns), P for one kernel per latent
        # over SHARED inducing points (BASELINE config C5, separate): P single-output problems that share Z, the likelihood, the mean
        # constant and the minibatch rows; their objectives and shared gradients add up (conditionals/util.py:566-629).  The
        # covariance spec is rebuilt from the trainer's current member values every step (CovarianceRoute.spec_at).
        from .inducing_variables import SharedIndependentInducingVariables
        from .kernels import LinearCoregionalization, SeparateIndependent
        from .models import reverse
        if isinstance(model.kernel, LinearCoregionalization):
            raise NotImplementedError("the trainer does not cover LinearCoregionalization: its step has no mixing stage "
                                      "(SVGP.elbo_and_grad with optimizers.Scipy does)")
        if isinstance(model.kernel, SeparateIndependent) and not isinstance(model.inducing_variable, SharedIndependentInducingVariables):
            raise NotImplementedError("the trainer with separate kernels per latent: shared inducing points")
        if reverse.has_row_diagonal(model.kernel):
            raise NotImplementedError(f"the trainer's device step takes K(x, x) for one scalar: {reverse.ROW_DIAGONAL} is not built into "
                                      "it -- SVGP.elbo_and_grad with optimizers.Scipy covers it")
        routes, c, self.separate = reverse.svgp_routes(model)
        if any(p is not None for r, _ in routes for p in r.spec.periods):
            raise NotImplementedError("the trainer keeps (variance, lengthscales) per kernel on the device side of its step: no Periodic "
                                      "member (its period, and a leaf that is not its Parameters' values) -- SVGP.elbo_and_grad with "
                                      "optimizers.Scipy covers it")
        if not all(leaf.is_plain for r, _ in routes for leaf in r.spec.members):
            raise NotImplementedError("the trainer keeps (variance, lengthscales) per kernel on the device side of its step: no "
                                      "RationalQuadratic (alpha), White or Constant (no lengthscales) members -- SVGP.elbo_and_grad "
                                      "with optimizers.Scipy covers them")
        iv = routes[0][1]
        self.routes = [r for r, _ in routes]
        lik = model.likelihood
        self.q_diag = model.q_sqrt.numpy().ndim == 2
        if self.q_diag and natgrad_gamma is not None:
            raise NotImplementedError("natural gradients need the full q_sqrt [P, M, M] (optimizers/natgrad.py:280-368)")
        # priors (MAP, model.py:47-76: the loss is -(ELBO + sum of the log prior densities of ALL trainable parameters)): on the
        # host-side hyper-parameters their gradient is added on the host every step; on the device-resident variables (Z, q_mu,
        # q_sqrt) it is evaluated and added on the device (`_device_prior`, round 5)
        self.model, self.group = model, group
        self.natgrad_gamma = None if natgrad_gamma is None else float(natgrad_gamma)
        self.mean_const = c
        self.opt = _Adam(learning_rate, beta_1, beta_2, epsilon)
        # host side: unconstrained scalars (their constrained values are host arguments of the C-ABI).  One host entry per distinct
        # Parameter (a Parameter shared by several members or latents -- k + k, tied lengthscales -- collects the SUM of its members'
        # gradients, as autodiff returns it): "variance" / "lengthscales" for one stationary kernel, else member i of route r reads
        # "kvar_<a>" / "kls_<b>"
        plain = not self.separate and not self.routes[0].is_combination
        self.host, self.member_names, seen = {}, [], {}
        for route in self.routes:
            self.member_names.append([])
            for pars in route.members:
                for par, pre, name in zip(pars, ("kvar", "kls"), ("variance", "lengthscales")):
                    if id(par) not in seen:
                        seen[id(par)] = name if plain else f"{pre}_{len(seen)}"
                        self.host[seen[id(par)]] = par
                self.member_names[-1].append(tuple(seen[id(par)] for par in pars))
        # noise: a constant variance, or (a heteroskedastic Gaussian likelihood, likelihoods/scalar_continuous.py:52-111) the Parameters of
        # the noise Function -- they stay on the host like the other hyper-parameters; sigma_n^2 at the minibatch rows is formed on the
        # device every step and dF/d sigma_n^2 comes back per row, chained through the Function there (Gaussian.noise_param_grads)
        self.het = lik.is_heteroskedastic
        self.noise_pars = []
        if self.het:
            fn = lik.variance if lik.variance is not None else lik.scale       # (is_heteroskedastic: a Function)
            self.noise_pars = list(fn.parameters)
            for i, p in enumerate(self.noise_pars):
                self.host[f"noise_fn_{i}"] = p
        else:
            self.host["noise_variance"] = lik.variance
        for par, _ in reverse.mean_pairs(model.mean_function, None):
            # Constant.c is a trainable Parameter like any other (gpflow/functions.py:173-192): it joins the host set
            if np.size(par.numpy()) != 1:
                raise NotImplementedError("the reverse pass covers a scalar Constant mean")
            self.host["mean_const"] = par
        self.u = {n: np.array(p.unconstrained_variable, dtype=np.float64, copy=True) for n, p in self.host.items()}
        # device side (identity / fill-triangular transforms: the constrained array IS the variable)
        self.dev = {"Z": ops.to_device(iv.Z.numpy()).clone(), "q_mu": ops.to_device(model.q_mu.numpy()).clone(),
                    "q_sqrt": ops.to_device(model.q_sqrt.numpy()).clone()}
        self.dev_params = {"Z": iv.Z, "q_mu": model.q_mu, "q_sqrt": model.q_sqrt}
        self.q_lower = 0.0
        if self.q_diag:
            # q_sqrt [M, P] holds standard deviations under positive() = softplus (+ an optional lower bound,
            # utilities/bijectors.py:27-45): the DEVICE variable is the unconstrained one, q = softplus(u) + lower is formed
            # on the device every step and the gradient is chained through sigmoid(u) there
            from .base import Chain, Shift, Softplus
            t = model.q_sqrt.transform
            if isinstance(t, Chain) and len(t.bijectors) == 2 and isinstance(t.bijectors[0], Shift) \
                    and isinstance(t.bijectors[1], Softplus):
                self.q_lower = float(t.bijectors[0].shift)
            elif not isinstance(t, Softplus):
                raise NotImplementedError("the trainer covers the softplus transform of a diagonal q_sqrt")
            self.dev["q_sqrt"] = ops.to_device(np.asarray(model.q_sqrt.unconstrained_variable, dtype=np.float64)).clone()
        self.last_info: Optional[int] = None   # factorisation status of the last step (0 = ok), checked every step

    def constrained(self, name: str) -> np.ndarray:
        return np.asarray(self.host[name].transform.forward(self.u[name]), dtype=np.float64)

    def _device_prior(self, name: str):
        """(log prior density as a 0-d device tensor, its gradient w.r.t. the device variable) of a device-resident variable
        carrying a prior -- gpflow/base.py:201-224 evaluated where the variable lives.  Z and q_mu have identity transforms; a full
        q_sqrt is its own constrained value (fill-triangular: a permutation, unit Jacobian; only the lower triangle is a variable);
        a diagonal q_sqrt is kept unconstrained on the device, q = softplus(u) + lower."""
        from .base import PriorOn
        from .priors import grad_log_prob_device, log_prob_device
        p = self.dev_params[name]
        x = self.dev[name]
        if name == "q_sqrt" and self.q_diag:
            sig = torch.sigmoid(x)
            if p.prior_on == PriorOn.CONSTRAINED:
                q = torch.nn.functional.softplus(x) + self.q_lower
                return log_prob_device(p.prior, q), grad_log_prob_device(p.prior, q) * sig
            # prior on the unconstrained value, density reported in the constrained space: - log |dq/du| = - log sigmoid(u)
            return log_prob_device(p.prior, x) - torch.log(sig).sum(), grad_log_prob_device(p.prior, x) - (1.0 - sig)
        if name == "q_sqrt":
            low = torch.tril(x)
            if p.prior_on == PriorOn.CONSTRAINED:      # the constrained value is the whole [P, M, M] array, zeros included
                return log_prob_device(p.prior, low), torch.tril(grad_log_prob_device(p.prior, low))
            mask = torch.tril(torch.ones_like(x[0], dtype=torch.bool))
            vec = low[:, mask]                          # the unconstrained vector: the lower-triangular entries
            g = torch.zeros_like(x)
            g[:, mask] = grad_log_prob_device(p.prior, vec)
            return log_prob_device(p.prior, vec), g
        return log_prob_device(p.prior, x), grad_log_prob_device(p.prior, x)

    def step(self, data, *, global_batch: Optional[int] = None) -> torch.Tensor:
        """One Adam step on the minibatch (or this rank's shard of it); returns the objective BEFORE the update -- the ELBO
        estimate plus the log prior density of every trainable parameter that carries a prior, i.e. -training_loss
        (models/model.py:56-76), the same quantity `SVGP.elbo_and_grad` reports -- as a device tensor [1] (no host
        synchronisation beyond the scalar-gradient read-back)."""
        import torch.distributed as dist
        from .models import reverse
        Xb, Yb = ops.to_device(data[0]), ops.to_device(data[1])
        world = dist.get_world_size(self.group) if (dist.is_available() and dist.is_initialized()) else 1
        rows = int(global_batch) if global_batch is not None else Xb.shape[0] * world
        scale = reverse.minibatch_scale(self.model.num_data, rows)
        if self.het:
            # SIDE EFFECT, by design: the noise Function evaluates itself from its own Parameters, so the trainer's current values of
            # them are written into the model on every step -- unlike the kernel / Z / q parameters, which reach the model only through
            # sync_to_model().  Between steps the model therefore holds the NEW noise parameters next to the kernel, Z and q of the last
            # sync: call sync_to_model() before evaluating model.elbo() / predict_* mid-training.
            for i, p in enumerate(self.noise_pars):              # the Function reads its Parameters: the trainer's current values
                p.assign_unconstrained(self.u[f"noise_fn_{i}"])
            noise = self.model.likelihood.noise_for(Xb)          # sigma_n^2 at the rows of this (shard of the) minibatch  [B]
        else:
            noise = float(self.constrained("noise_variance"))
        if "mean_const" in self.host:
            self.mean_const = float(np.ravel(self.constrained("mean_const"))[0])
        fn = gradients.svgp_elbo_and_grad if self.model.whiten else gradients.svgp_elbo_and_grad_unwhitened
        q_sqrt = torch.nn.functional.softplus(self.dev["q_sqrt"]) + self.q_lower if self.q_diag else self.dev["q_sqrt"]
        if self.separate and Yb.shape[1] != len(self.routes):
            raise ValueError(f"{len(self.routes)} separate kernels need {len(self.routes)} output columns, got {Yb.shape[1]}")
        F, info, g, g_q = None, None, {}, ([], [])

        def add(name, t):   # per-member and per-latent gradients onto their (possibly shared) entries
            g[name] = g[name] + t if name in g else t
        for p_, (route, names) in enumerate(zip(self.routes, self.member_names)):
            cols = slice(p_, p_ + 1) if self.separate else slice(None)
            Zs, Xs, scatter = route.inputs(self.dev["Z"], Xb)      # active_dims (kernels/base.py:90-109)
            spec = route.spec_at([(float(np.ravel(self.constrained(nv))[0]), self.constrained(nl)) for nv, nl in names])
            Fp, gp, ip = fn(Zs, Xs, Yb[:, cols].contiguous(), self.dev["q_mu"][:, cols].contiguous(), q_sqrt[cols].contiguous(),
                            noise_variance=noise, jitter=config.default_jitter(), scale=scale, mean_const=self.mean_const,
                            kl_weight=1.0 / world, kernel_spec=spec)
            F = Fp if F is None else F + Fp
            info = ip if info is None else torch.maximum(info, ip)
            for (nv, nl), (gv, gl) in zip(names, route.member_grads(gp)):
                add(nv, gv)
                add(nl, gl)
            add("Z", scatter(gp["Z"]))
            add("noise_variance", gp["noise_variance"])
            add("mean_const", gp["mean_const"])
            g_q[0].append(gp["q_mu"])
            g_q[1].append(gp["q_sqrt"])
        g["q_mu"], g["q_sqrt"] = (g_q[0][0], g_q[1][0]) if not self.separate else (torch.cat(g_q[0], dim=1), torch.cat(g_q[1], dim=0))
        if self.het:
            # per-row dF/d sigma_n^2 -> the noise Function's parameters (this shard's rows; summed over the ranks below)
            rows_g = g.pop("noise_variance")
            acc = {}
            for par, gv in self.model.likelihood.noise_param_grads(Xb, rows_g):
                acc[id(par)] = acc[id(par)] + gv if id(par) in acc else gv
            for i, p in enumerate(self.noise_pars):
                g[f"noise_fn_{i}"] = acc[id(p)].reshape(-1).contiguous() if id(p) in acc else \
                    torch.zeros(int(np.size(self.u[f"noise_fn_{i}"])), dtype=torch.float64, device=Xb.device)
        if self.q_diag:
            g["q_sqrt"] = g["q_sqrt"] * torch.sigmoid(self.dev["q_sqrt"])      # d softplus(u) / du
        g["_status"] = info.to(torch.float64).reshape(-1)[:1]   # rides in the packed all-reduce: > 0 iff ANY rank failed
        F, g = distributed.all_reduce_grads(F, g, self.group)
        # The factorisation status decides whether this step may be applied at all: after a failed Cholesky of Kuu the
        # gradients are garbage, and applying them would poison the variables AND the Adam moments for good (the
        # reference raises from tf.linalg.cholesky at this point).  It rides in the step's one read-back and, with
        # several ranks, in the packed gradient all-reduce (summed), so every rank takes the same decision.
        status = g.pop("_status")
        hnames = list(self.host)                                 # variance, lengthscales, noise (constant or Function parameters), [mean]
        hsizes = [1 if n == "mean_const" else int(g[n].numel()) for n in hnames]
        small = torch.cat([g[n].reshape(-1)[:sz] for n, sz in zip(hnames, hsizes)] + [status])
        small = small.cpu().numpy()                              # the step's one read-back: 4 + |lengthscales| doubles (+ the noise Function's)
        self.last_info = int(small[-1])
        if self.last_info != 0:
            from ._lib import GpkError
            # (summed over the ranks: pivot columns are far below 2^31, so a sum that reaches INT_MAX contains a timed-out hand-off)
            if self.last_info >= ops.INFO_HANDOFF_TIMEOUT:
                raise GpkError("the factorisation of Kuu failed: an internal stream hand-off timed out (status INT_MAX)" +
                               ("" if world == 1 else " on at least one rank") + "; the step was NOT applied")
            raise GpkError("Cholesky decomposition of Kuu was not successful" +
                           (f" (non-positive pivot at column {self.last_info - 1})" if world == 1 else
                            " on at least one rank") + "; the step was NOT applied")
        adam_names = ("Z", "q_mu", "q_sqrt")
        nat = None
        if self.natgrad_gamma is not None:
            # into temporaries first: natgrad_update has a status check of its own ("precision (step too long?)"); if it
            # raises, neither q(u), nor the Adam step counter, nor any moment has been touched
            from . import natgrad
            adam_names = ("Z",)
            nat = natgrad.natgrad_update(self.dev["q_mu"], self.dev["q_sqrt"], -g["q_mu"], -g["q_sqrt"], self.natgrad_gamma)
        # MAP (model.py:47-76): the priors of the device-resident variables, evaluated BEFORE anything is updated
        log_prior = 0.0
        for name, par in self.dev_params.items():
            if par.prior is not None and par.trainable:
                if name != "Z" and nat is not None:
                    raise NotImplementedError("a prior on q_mu / q_sqrt together with natural-gradient steps on q(u)")
                lp, gp = self._device_prior(name)
                g[name] = g[name] + gp
                log_prior = log_prior + lp
        self.opt.t += 1
        if nat is not None:
            self.dev["q_mu"].copy_(nat[0])
            self.dev["q_sqrt"].copy_(nat[1])
        for name in adam_names:                                  # minimise -F
            if self.dev_params[name].trainable:
                self.opt.update_device(name, self.dev[name], -g[name])
        offs = np.concatenate([[0], np.cumsum(hsizes)])
        parts = {n: small[offs[i]:offs[i + 1]] for i, n in enumerate(hnames)}
        for name, p in self.host.items():
            if not p.trainable:
                continue
            gu = -parts[name].reshape(self.u[name].shape) * p.transform.forward_grad(self.u[name])
            if p.prior is not None:   # loss = -(ELBO + log prior): the prior's part, evaluated at the trainer's current value
                p.assign_unconstrained(self.u[name])
                gu = gu - p.log_prior_density_grad()
                log_prior = log_prior + p.log_prior_density()
            self.u[name] = self.opt.update_host(name, self.u[name], gu)
        return F + log_prior

    def sync_to_model(self) -> None:
        for name, p in self.host.items():
            p.assign_unconstrained(self.u[name])
        for name, p in self.dev_params.items():
            v = self.dev[name].cpu().numpy()
            if name == "q_sqrt" and self.q_diag:
                p.assign_unconstrained(v)
            else:
                p.assign(np.tril(v) if name == "q_sqrt" else v)
