"""What the model-level entry points of the hand-written reverse pass share (SVGP.elbo_and_grad, GPR / SGPR.objective_and_grad,
training.SVGPTrainer, optimizers.NaturalGradient): which models are covered, how ONE covariance function reaches `gradients.*`
(always as a `gradients.KernelSpec`), and how what comes back becomes {Parameter: d objective / d(unconstrained value)}."""
from __future__ import annotations

import numpy as np
import torch

from .. import gradients
from ..base import FillTriangular
from ..inducing_variables import (InducingPoints, SeparateIndependentInducingVariables, SharedIndependentInducingVariables)
from ..kernels import LinearCoregionalization, SeparateIndependent, SharedIndependent
from ..kernels.base import Combination, changepoint_nodes, gradient_spec, has_row_diagonal_leaf, reverse_leaf
from ..kernels.periodic import Periodic
from ..likelihoods import Gaussian, SwitchedLikelihood
from ..mean_functions import Constant


def shared_pair(kernel, inducing_variable):
    """(kernel, inducing variable) with SharedIndependent + SharedIndependentInducingVariables unwrapped: P latents over one Kuu / Kuf
    (BASELINE config C5)"""
    if isinstance(kernel, SharedIndependent) and isinstance(inducing_variable, SharedIndependentInducingVariables):
        return kernel.kernel, inducing_variable.inducing_variable
    return kernel, inducing_variable


def sliced(k, Z, X):
    """Inputs restricted to the kernel's active_dims + the scatter of a gradient w.r.t. the sliced Z back to Z's shape
    (gpflow/kernels/base.py:90-109: the kernel only ever sees these columns, so dF/dZ is zero elsewhere)."""
    if k.has_default_active_dims:
        return Z, X, (lambda gz: gz)
    Xs, Zs = k.slice(X, Z)
    dims = k._active_dims
    cols = torch.arange(Z.shape[1], device=Z.device)[dims] if isinstance(dims, slice) else torch.as_tensor(dims, device=Z.device)

    def scatter(gz):
        full = torch.zeros_like(Z)
        full.index_add_(1, cols, gz)   # (a repeated active column collects both contributions, like tf.gather's gradient)
        return full
    return Zs, Xs, scatter


def minibatch_scale(num_data, rows) -> float:
    """svgp.py:172-174: the data term of a minibatch of `rows` rows stands for `num_data` rows"""
    return 1.0 if num_data is None else float(num_data) / float(rows)


def _supported_stationary(k) -> bool:
    """a leaf of the reverse pass (kernels.base.reverse_leaf) with a constant diagonal: an isotropic-stationary kernel, a static one, or
    a Periodic kernel over a stationary base"""
    return reverse_leaf(k) is not None and not has_row_diagonal_leaf(k)


ROW_DIAGONAL = "a dot-product, ArcCosine or Coregion kernel or member (Linear, Polynomial, ArcCosine, Coregion), whose K(x, x) depends on the row,"


def has_row_diagonal(k) -> bool:
    """a dot-product kernel (kernels/linears.py) or an ArcCosine or Coregion kernel (kernels/misc.py) anywhere under k -- in a Sum / Product, or
    behind a multi-output wrapper"""
    if has_row_diagonal_leaf(k) or getattr(k, "_op", None) == "cp":   # (a ChangePoints: its weights depend on the row)
        return True
    members = [k.kernel] if isinstance(k, SharedIndependent) else getattr(k, "kernels", [])
    return any(has_row_diagonal(m) for m in members)


class CovarianceRoute:
    """One covariance function as the reverse pass takes it: `spec` (gradients.KernelSpec), `members` [the Parameters of each leaf,
    in the leaf's order: DeviceLeaf.leaf_params] in the spec's order, the inputs as `gradients.*` gets them and the scatter of dF/dZ
    back to Z's columns.
      one SquaredExponential / Matern kernel: a one-member spec over ALL columns of inputs sliced by its `active_dims` out here
        (a spec with `cols` would leave the packed covariance tail of gradients.svgp_elbo_and_grad);
      one Periodic kernel: the same, sliced by its BASE's `active_dims` -- the columns only; the warp is the spec's (`periods`);
      a Sum / Product of them, flat or nested: kernels.base.gradient_spec -- the spec slices for its members itself.
    Anything else raises NotImplementedError."""

    def __init__(self, kernel, input_dim=None):
        self.kernel = kernel
        self._columns_of = kernel.base_kernel if isinstance(kernel, Periodic) else kernel   # whose `slice` selects columns and no more
        self.is_combination = isinstance(kernel, Combination)
        self.nodes = [k.node_params() for k in changepoint_nodes(kernel)]   # (locations, steepness) per ChangePoints node, in node order
        if self.is_combination:
            self.spec, self.members = gradient_spec(kernel, input_dim)
            return
        found = reverse_leaf(kernel, input_dim)
        if found is None:
            raise NotImplementedError("gradients: a SquaredExponential / Matern / Exponential / RationalQuadratic / White / Constant / "
                                      "Periodic / Linear / Polynomial / ArcCosine / Coregion kernel, or a Sum / Product (possibly nested) of them")
        leaf, period, params = found
        self.spec, self.members = gradients.KernelSpec([leaf], periods=[period]), [params]

    def inputs(self, Z, X):
        """(Z, X, scatter) as passed to `gradients.*`; Z None (GPR): X alone is sliced"""
        if self.is_combination:
            return Z, X.contiguous(), (lambda gz: gz)
        if Z is None:
            return None, self._columns_of.slice(X, None)[0].contiguous(), None
        return sliced(self._columns_of, Z, X)

    def spec_at(self, values):
        """the spec with the members' values replaced, each laid out as its `members` entry (the trainer's current values)"""
        if any(p is not None for p in self.spec.periods):
            raise NotImplementedError("a Periodic member's leaf is not its Parameters' values (lengthscales 2 l over the warped columns)")
        return gradients.KernelSpec([leaf.replace(vals) for leaf, vals in zip(self.spec.members, values)], self.spec.tree, self.spec.cols)

    def member_grads(self, g):
        """[(d/dvariance_i [1], ...)] from the `grads` of a `gradients.*` call, each entry laid out as the member's `members` entry: the
        one place that knows the two packings of KernelSpec.pack / kernel_grads (one member: "variance" [1] and one tensor per name;
        several: "variance" [n] and one list per name)"""
        one = self.spec.n == 1
        gv = g["variance"].reshape(-1)
        cut = self._variance_cuts()
        return [(gv[cut[i]:cut[i + 1]],) + tuple((g[name] if one else g[name][i]).reshape(-1) for name in self.spec.parameter_names(i)[1:])
                for i in range(self.spec.n)]

    def _variance_cuts(self):
        """where member i's entries of grads["variance"] begin: one each, D for the ARD variance of a dot-product member"""
        return np.concatenate([[0], np.cumsum([self.spec.n_variance(i) for i in range(self.spec.n)])]).astype(int)

    def kernel_pairs(self, g):
        """[(Parameter, dF/d constrained as NumPy)] of the members, in member order (the variances come back in one copy)"""
        gv, cut = g["variance"].reshape(-1).cpu().numpy(), self._variance_cuts()
        pairs = [(par, gv[cut[i]:cut[i + 1]] if j == 0 else gr.cpu().numpy())
                 for i, (pars, grs) in enumerate(zip(self.members, self.member_grads(g))) for j, (par, gr) in enumerate(zip(pars, grs))]
        for (loc, steep), gn in zip(self.nodes, g.get("changepoints", [])):   # a ChangePoints node's own Parameters, in node order
            pairs += [(loc, gn["locations"].cpu().numpy()), (steep, gn["steepness"].cpu().numpy().reshape(steep.numpy().shape))]
        return pairs


def noise_pairs(lik, X, g_noise, reduce=None):
    """[(Parameter, gradient)] of a Gaussian likelihood's noise: the `variance` Parameter, or -- heteroskedastic, g_noise = dF/d sigma_n^2
    per row of X on the device -- the Parameters of the noise Function (Gaussian.noise_param_grads).  reduce: applied to each Function
    gradient before it is read back (SGPR: the sum over the row shards)."""
    if not lik.is_heteroskedastic:
        return [(lik.variance, g_noise.cpu().numpy() if torch.is_tensor(g_noise) else g_noise)]
    out = []
    for par, gv in lik.noise_param_grads(X, g_noise):
        out.append((par, (gv if reduce is None else reduce(gv.contiguous())).cpu().numpy()))
    return out


def mean_pairs(mean_function, g_mean):
    """a Constant mean with a parameter (Zero is a Constant without one, functions.py:195-204)"""
    return [(mean_function.c, g_mean)] if isinstance(mean_function, Constant) and hasattr(mean_function, "c") else []


def to_unconstrained(pairs):
    """{Parameter: dF/d(unconstrained value)} from [(Parameter, dF/d constrained value)], trainable Parameters only, keys in the order of
    their first pair (optimizers.Scipy packs its vector in it).  A Parameter that occurs twice (k + k, tied lengthscales) collects the
    sum, as autodiff returns it; fill-triangular is a linear embedding: the vector entries are the lower-triangular ones."""
    out = {}
    for par, gc in pairs:
        if not par.trainable:
            continue
        u = par.unconstrained_variable
        if isinstance(par.transform, FillTriangular):
            gu = par.transform.inverse(np.asarray(gc, dtype=np.float64)).reshape(u.shape)
        else:
            gu = np.asarray(gc, dtype=np.float64).reshape(u.shape) * par.transform.forward_grad(u)
        out[par] = out[par] + gu if par in out else gu
    return out


# ---- scope: one check per model family, before anything touches the device ---------------------------------------------------------
def _gaussian_noise(lik, heteroskedastic=True) -> bool:
    return isinstance(lik, Gaussian) and (lik.has_variance_parameter or (heteroskedastic and lik.is_heteroskedastic))


def svgp_routes(model, *, quadrature: bool = False, narrow: bool = False):
    """([(CovarianceRoute, InducingPoints)], mean constant, separate) for an SVGP inside the reverse pass, else NotImplementedError: whitened or
    not, InducingPoints, constant mean, Gaussian likelihood (a variance Parameter or a noise Function), and
      one SquaredExponential / Matern kernel, with `active_dims`, possibly shared by the latents (SharedIndependent +
        SharedIndependentInducingVariables), full or diagonal q_sqrt -- one route;
      a Sum / Product of such kernels, full or diagonal q_sqrt -- one route;
      SeparateIndependent over shared or separate inducing points, every member ONE SquaredExponential / Matern kernel, full
        q_sqrt -- one route per latent, and `separate` is True (also for a single member: the callers name and slice by it).
    quadrature (a Bernoulli / Poisson / StudentT / MultiClass likelihood, `likelihood=` of gradients.svgp_elbo_and_grad): whitened,
    one kernel over all input columns, at most 16 latents.  narrow (natural gradients on q(u)): one kernel over all input columns,
    full q_sqrt, constant noise.  A LinearCoregionalization kernel: `_lcm_routes` -- one route per latent, and its own refusals.
    A dot-product kernel or member (Linear, Polynomial; `has_row_diagonal`): the plain routes of the first two lines only -- with
    quadrature, narrow, SeparateIndependent or LinearCoregionalization it is refused here, by the limit it breaks."""
    k, iv = model.kernel, model.inducing_variable
    if has_row_diagonal(k):   # Linear / Polynomial: covered by the plain route alone -- every other one takes K(x, x) for one scalar
        limit = "the quadrature likelihoods' reverse pass: its variational expectations take K(x, x) as one value per latent" if quadrature \
            else "natural gradients: their reverse pass is the packed one-kernel form with a scalar K(x, x)" if narrow \
            else "the per-latent reverse passes (SeparateIndependent, LinearCoregionalization): one scalar K(x, x) per latent" \
            if isinstance(k, (SeparateIndependent, LinearCoregionalization)) else None
        if limit is not None:
            raise NotImplementedError(f"gradients: {ROW_DIAGONAL} is not built into {limit}")
    if isinstance(k, LinearCoregionalization):
        return _lcm_routes(model, quadrature=quadrature, narrow=narrow)
    plain = not (quadrature or narrow)
    lik_ok = (model.whiten and (model._device_likelihood() or model._switched_likelihood())) if quadrature \
        else _gaussian_noise(model.likelihood, not narrow)
    q_full = model.q_sqrt.numpy().ndim == 3
    separate = isinstance(k, SeparateIndependent)
    if separate and plain:
        ivs = list(iv.inducing_variable_list) if isinstance(iv, SeparateIndependentInducingVariables) else \
            [iv.inducing_variable] * len(k.kernels) if isinstance(iv, SharedIndependentInducingVariables) else []
        pairs, ok = list(zip(k.kernels, ivs)), q_full and len(ivs) == len(k.kernels) and all(_supported_stationary(kk) for kk in k.kernels)
    else:
        pairs, ok = [shared_pair(k, iv)], q_full or not narrow
        if isinstance(pairs[0][0], Combination):          # (as the model's own kernel only: not shared through SharedIndependent)
            ok = ok and plain and pairs[0][0] is k
        elif not plain:
            ok = ok and pairs[0][0].has_default_active_dims
    c = model.mean_function.constant_value()
    if not (ok and lik_ok and c is not None and all(isinstance(v, InducingPoints) for _, v in pairs)):
        raise NotImplementedError(
            "gradients: SVGP over InducingPoints with a constant mean and a SquaredExponential / Matern kernel (shared by independent "
            "latents, or one per latent with a full q_sqrt) or a Sum / Product of them, and a Gaussian likelihood -- or, whitened with one "
            "kernel over all input columns and at most 16 latents, a Bernoulli / Poisson / StudentT / MultiClass likelihood; natural "
            "gradients: one kernel over all input columns, full q_sqrt, constant noise")
    return [(CovarianceRoute(kk, int(v.Z.shape[1])), v) for kk, v in pairs], float(c), separate


def _latent_inducing_points(iv, n):
    """the inducing variable of each of n latents: shared, or one per latent; [] where they do not fit"""
    if isinstance(iv, SeparateIndependentInducingVariables):
        return list(iv.inducing_variable_list) if len(iv.inducing_variable_list) == n else []
    return [iv.inducing_variable] * n if isinstance(iv, SharedIndependentInducingVariables) else []


def _lcm_routes(model, *, quadrature, narrow):
    """svgp_routes for a LinearCoregionalization kernel: one route per LATENT, `separate` True.  The reverse pass of the mixing stage
    (gradients.svgp_elbo_and_grad_lcm) covers the whitened model with a full q_sqrt, a Gaussian likelihood with a `variance`
    Parameter, a constant mean and one SquaredExponential / Matern kernel per latent over shared or per-latent inducing points;
    every other form is refused here by the limit it breaks."""
    k, lik = model.kernel, model.likelihood
    no = lambda what: NotImplementedError(f"gradients: LinearCoregionalization {what}")   # noqa: E731
    if narrow:
        raise no("is outside the natural gradients (one kernel over all input columns, no mixing stage)")
    if quadrature or not isinstance(lik, Gaussian):
        raise no("with a non-Gaussian likelihood: the quadrature likelihoods on the mixed outputs run forward only (SVGP.elbo)")
    if lik.is_heteroskedastic or not lik.has_variance_parameter:
        raise no("with a heteroskedastic likelihood: the mixing stage takes ONE noise variance, held as a `variance` Parameter")
    if not model.whiten:
        raise no("un-whitened: the reverse pass of the mixing stage is whitened only")
    if model.q_sqrt.numpy().ndim != 3:
        raise no("with a diagonal q_sqrt: the reverse pass of the mixing stage takes the full q_sqrt [L, M, M]")
    c = model.mean_function.constant_value()
    if c is None:
        raise no("needs a constant mean")
    ivs = _latent_inducing_points(model.inducing_variable, len(k.kernels))
    if not ivs or not all(isinstance(v, InducingPoints) for v in ivs) or not all(_supported_stationary(kk) for kk in k.kernels):
        raise no("needs one SquaredExponential / Matern kernel per latent over inducing points, shared or one set per latent")
    W = k.W.numpy()
    if W.ndim != 2 or W.shape[1] != len(k.kernels) or model.q_mu.shape[1] != len(k.kernels) or max(W.shape) > 16:
        raise no(f"needs W [P, L] and q_mu [M, L] for its L = {len(k.kernels)} latents, at most 16 latents and 16 outputs")
    return [(CovarianceRoute(kk, int(v.Z.shape[1])), v) for kk, v in zip(k.kernels, ivs)], float(c), True


def vgp_scope(model):
    """The mean constant of a VGP inside its device paths, else NotImplementedError -- checked when the model is BUILT and again by
    every route, before anything touches the device: a single-output kernel, a zero or constant mean, and a Gaussian likelihood with
    one noise variance or a likelihood whose variational expectations the library computes (`device_lik`; at most 16 latents, which
    for MultiClass are its classes), or a SwitchedLikelihood with at most 16 latents."""
    from ..kernels import MultioutputKernel
    from .. import ops
    lik, R = model.likelihood, model.q_mu.shape[1]
    no = lambda what: NotImplementedError(f"VGP: {what}")   # noqa: E731
    if isinstance(model.kernel, MultioutputKernel):
        raise no("a multi-output kernel is not built into the full variational model (one kernel shared by the latents)")
    if isinstance(lik, Gaussian):
        if lik.is_heteroskedastic:
            raise no("a heteroskedastic Gaussian likelihood is not built into the full variational model (one noise variance)")
    elif isinstance(lik, SwitchedLikelihood):
        if R > 16:
            raise no("a SwitchedLikelihood with more than 16 latents (the columns of one call of its stage)")
    elif getattr(lik, "device_lik", "") not in ops.LIKELIHOOD_CODES:
        raise no(f"the likelihood {type(lik).__name__} has no variational-expectation kernel on the device (`device_lik`)")
    elif hasattr(lik, "check_device_classes"):
        lik.check_device_classes(R)   # (ValueError: latents != classes; NotImplementedError: more than 16)
    c = model.mean_function.constant_value()
    if c is None:
        raise no("a zero or constant mean function")
    return float(c)


def vgp_route(model):
    """(CovarianceRoute, mean constant) for a VGP inside the reverse pass (gradients.vgp_elbo_and_grad), else NotImplementedError:
    `vgp_scope`, any kernel tree the route takes, a trainable Gaussian noise held as a `variance` Parameter, at most 16 latents for a
    quadrature likelihood (its kernel's columns per call)."""
    c = vgp_scope(model)
    lik = model.likelihood
    if isinstance(lik, Gaussian):
        if not lik.has_variance_parameter:
            raise NotImplementedError("VGP gradients: a Gaussian likelihood with its noise held as a `variance` Parameter")
    elif model.q_mu.shape[1] > 16:
        raise NotImplementedError("VGP gradients: at most 16 latents with a quadrature likelihood")
    return CovarianceRoute(model.kernel, model.data[0].shape[1]), c


def regression_route(model):
    """(CovarianceRoute, mean constant) for a GPR / SGPR inside the reverse pass, else NotImplementedError"""
    c = model.mean_function.constant_value()
    if c is None or not _gaussian_noise(model.likelihood):
        raise NotImplementedError("gradients: SquaredExponential / Matern kernel (or a Sum / Product of them), constant mean, Gaussian "
                                  "likelihood with a noise variance held as a `variance` Parameter, or a noise Function of the inputs")
    return CovarianceRoute(model.kernel, model.data[0].shape[1]), float(c)
