"""Likelihoods: Gaussian (gpflow/likelihoods/scalar_continuous.py:41-148) -- the conjugate case that keeps the whole ELBO on
the dense path -- and the scalar non-conjugate ones whose variational expectations are Gauss-Hermite quadrature on the device
(Bernoulli, Poisson, Ordinal: scalar_discrete.py; StudentT, Exponential, Gamma, Beta: scalar_continuous.py; ScalarLikelihood:
base.py; Poisson, Exponential and Gamma under the exp link in the reference's closed forms), and MultiClass with the
RobustMax link (multiclass.py), whose latents are coupled under one quadrature sum per row."""
from __future__ import annotations

from math import lgamma, log, pi, sqrt
from typing import Optional

import numpy as np
import torch

from . import config, ops
from .base import Module, Parameter, positive
from .functions import Function
from .logdensities import gaussian

LOG2PI = float(np.log(2 * np.pi))


class Likelihood(Module):
    pass


class Gaussian(Likelihood):
    """Gaussian(variance=None, *, scale=None, variance_lower_bound=None), scalar_continuous.py:41-148.  `variance` / `scale` is a
    constant (a positive Parameter) or a Function of the inputs (gpflow/functions.py) -- a heteroskedastic likelihood whose value is
    clipped from below at the lower bound when it is evaluated (utilities/parameter_or_function.py:45-58)."""

    def __init__(self, variance=None, *, scale=None, variance_lower_bound: Optional[float] = None):
        self.variance_lower_bound = (config.default_likelihood_positive_minimum()
                                     if variance_lower_bound is None else float(variance_lower_bound))
        self.scale_lower_bound = sqrt(self.variance_lower_bound)
        if scale is None:
            if variance is None:
                variance = 1.0
            self.variance = self._prepare(variance, self.variance_lower_bound)
            self.scale = None
        else:
            assert variance is None, "Cannot set both `variance` and `scale`."
            self.variance = None
            self.scale = self._prepare(scale, self.scale_lower_bound)

    @staticmethod
    def _prepare(value, lower_bound: float):
        """prepare_parameter_or_function (utilities/parameter_or_function.py:27-39)"""
        if isinstance(value, Function):
            return value
        # (a Parameter handed in is re-wrapped like any other value, as the reference does: the NEW Parameter carries the lower-bound
        #  transform -- an identity- or otherwise-transformed one would let the optimiser take the variance below the bound --
        #  and inherits prior / trainable, base.py:155-161)
        return Parameter(value, transform=positive(lower=lower_bound))

    @property
    def is_heteroskedastic(self) -> bool:
        """The noise depends on the inputs (variance / scale is a Function)."""
        return isinstance(self.variance if self.variance is not None else self.scale, Function)

    @property
    def has_variance_parameter(self) -> bool:
        """Constant noise held as a `variance` Parameter -- what the hand-written reverse passes differentiate."""
        return isinstance(self.variance, Parameter)

    def noise_variance(self) -> float:
        """scalar_continuous.py:92-105 (constant-variance case)"""
        if self.is_heteroskedastic:
            raise ValueError("the noise variance of this likelihood depends on the inputs: use noise_for(X) / variance_at(X)")
        if self.variance is not None:
            return float(self.variance.numpy())
        return float(self.scale.numpy()) ** 2

    def _variance(self, X):
        """scalar_continuous.py:92-105: a float (constant) or a device tensor [..., N, Q] (Function, clipped at the lower bound)."""
        if not self.is_heteroskedastic:
            return self.noise_variance()
        if self.variance is not None:
            return torch.clamp(self.variance(ops.to_device(X)), min=self.variance_lower_bound)
        return torch.clamp(self.scale(ops.to_device(X)), min=self.scale_lower_bound) ** 2

    def noise_for(self, X):
        """What the device entry points take as `noise_variance`: the constant as a float, or one variance per row of X as a
        device tensor [N] -- variance_at(X) squeezed (model_utils.py:46-50, sgpr.py:207)."""
        if not self.is_heteroskedastic:
            return self.noise_variance()
        X = ops.to_device(X)
        if X.dim() != 2:
            raise ValueError("noise_for expects X [N, D]")
        return self.variance_at(X)[:, 0].contiguous()

    def noise_param_grads(self, X, g_noise):
        """[(Parameter, dF/d(constrained value))] of the noise function's parameters, given g_noise [N] = dF/d sigma_n^2 at the rows of
        X (what the per-row reverse passes return as "noise_variance") -- the chain rule through _variance (clip at the lower
        bound: no gradient where the function sits below it; scale: d s^2 = 2 s ds) and the Function itself."""
        X = ops.to_device(X)
        fn = self.variance if self.variance is not None else self.scale
        raw = fn(X)
        g = g_noise.reshape(-1, 1)
        if raw.shape[-1] != 1:
            raise NotImplementedError("gradients of a heteroskedastic noise function with more than one output column")
        if self.variance is not None:
            gbar = g * (raw > self.variance_lower_bound)
        else:
            gbar = g * (2.0 * torch.clamp(raw, min=self.scale_lower_bound)) * (raw > self.scale_lower_bound)
        return fn.backward(X, gbar)

    def variance_at(self, X) -> torch.Tensor:
        """scalar_continuous.py:107-111: [..., N, 1]"""
        X = ops.to_device(X)
        v = self._variance(X)
        if not torch.is_tensor(v):
            return torch.full(X.shape[:-1] + (1,), v, dtype=torch.float64, device=X.device)
        return torch.broadcast_to(v, X.shape[:-1] + (1,))

    def log_prob(self, X, F, Y):
        return gaussian(ops.to_device(Y), ops.to_device(F), self._variance(X)).sum(-1)

    def predict_mean_and_var(self, X, Fmu, Fvar):
        """scalar_continuous.py:127-130"""
        return Fmu.clone(), Fvar + self._variance(X)

    def predict_log_density(self, X, Fmu, Fvar, Y):
        """scalar_continuous.py:132-136"""
        return gaussian(ops.to_device(Y), Fmu, Fvar + self._variance(X)).sum(-1)

    def variational_expectations(self, X, Fmu, Fvar, Y) -> torch.Tensor:
        """scalar_continuous.py:139-148 -- per-row values [N] (elementwise glue; the summed form used
        by SVGP.elbo runs in gpk_gaussian_varexp_sum)."""
        v = self._variance(X)
        Y = ops.to_device(Y)
        logv = torch.log(v) if torch.is_tensor(v) else float(np.log(v))
        return (-0.5 * LOG2PI - 0.5 * logv - 0.5 * ((Y - Fmu) ** 2 + Fvar) / v).sum(-1)


DEFAULT_NUM_GAUSS_HERMITE_POINTS = 20   # quadrature/gauss_hermite.py


def inv_probit(x: torch.Tensor) -> torch.Tensor:
    """utilities/ops.py inv_probit: the probit link with its 1e-3 jitter"""
    jitter = 1e-3
    return 0.5 * (1.0 + torch.special.erf(x / sqrt(2.0))) * (1 - 2 * jitter) + jitter


exp = torch.exp   # the Poisson link (the reference passes tf.exp)


class ScalarLikelihood(Likelihood):
    """likelihoods/base.py ScalarLikelihood: one latent per output column, everything elementwise over [N, P]; integrals against
    N(f | mu, v) are 20-point Gauss-Hermite sums, sum_h (w_h / sqrt pi) g(mu + sqrt(2 v) x_h) (quadrature/gauss_hermite.py).
    `variational_expectations`, the hot one, runs in gpk_likelihood_varexp_sum; the prediction-side integrals are elementwise
    device glue over the [20] node table, like the Gaussian methods above.  No clamp of Fvar anywhere: a negative value gives NaN
    through the square root, as in the reference."""

    device_lik: str = ""   # the likelihood's name in ops.LIKELIHOOD_CODES
    # the attribute name of the ONE trainable Parameter whose derivative the kernel returns as out[1] (include/gpk.h), or None:
    # the reverse pass reports it as grads["likelihood_" + device_grad_param]
    device_grad_param: Optional[str] = None

    def device_params(self) -> tuple:
        """the lik_params_host of the C-ABI at the current parameter values"""
        return ()

    # elementwise pieces, F and Y broadcastable device tensors
    def _log_density(self, F, Y):
        raise NotImplementedError

    def _conditional_mean(self, F):
        raise NotImplementedError

    def _conditional_variance(self, F):
        raise NotImplementedError

    def log_prob(self, X, F, Y):
        return self._log_density(ops.to_device(F), ops.to_device(Y)).sum(-1)

    def conditional_mean(self, X, F):
        return self._conditional_mean(ops.to_device(F))

    def conditional_variance(self, X, F):
        return self._conditional_variance(ops.to_device(F))

    @staticmethod
    def _nodes(like: torch.Tensor):
        """(x [H], w / sqrt(pi) [H]) next to `like`: the table the kernels use (ops.gauss_hermite)"""
        x, w = ops.gauss_hermite(DEFAULT_NUM_GAUSS_HERMITE_POINTS)
        return (torch.as_tensor(x, dtype=torch.float64, device=like.device),
                torch.as_tensor(w / np.sqrt(np.pi), dtype=torch.float64, device=like.device))

    def _points(self, Fmu, Fvar):
        """f_h = mu + sqrt(2 v) x_h as [..., H], and the normalised weights [H]"""
        Fmu, Fvar = ops.to_device(Fmu), ops.to_device(Fvar)
        x, wn = self._nodes(Fmu)
        return Fmu[..., None] + torch.sqrt(2.0 * Fvar)[..., None] * x, wn

    def variational_expectations(self, X, Fmu, Fvar, Y) -> torch.Tensor:
        """base.py ScalarLikelihood.variational_expectations -- per-row values [N], summed over the P outputs; the kernel takes
        at most 16 output columns per call."""
        Fmu, Fvar, Y = ops.to_device(Fmu), ops.to_device(Fvar), ops.to_device(Y)
        lead, P = Fmu.shape[:-1], Fmu.shape[-1]
        Fm, Fv, Yd = Fmu.reshape(-1, P), Fvar.reshape(-1, P), Y.reshape(-1, P)
        total = None
        for c0 in range(0, P, 16):
            c1 = min(c0 + 16, P)
            rows = ops.likelihood_varexp_sum(Yd[:, c0:c1], Fm[:, c0:c1].contiguous(), s0=None, ssq=Fv[:, c0:c1].t().contiguous(),
                                             knn=[0.0], lik=self.device_lik, params=self.device_params(), want_rows=True)[1]
            total = rows if total is None else total + rows
        return total.reshape(lead)

    def predict_mean_and_var(self, X, Fmu, Fvar):
        """base.py: E_y = int E[y|f], V_y = int (Var[y|f] + E[y|f]^2) - E_y^2"""
        f, wn = self._points(Fmu, Fvar)
        cm = self._conditional_mean(f)
        E_y = (cm * wn).sum(-1)
        V_y = ((self._conditional_variance(f) + cm * cm) * wn).sum(-1) - E_y * E_y
        return E_y, V_y

    def predict_log_density(self, X, Fmu, Fvar, Y):
        """base.py: log int p(y|f) N(f) df in log space, logsumexp_h(log(w_h / sqrt pi) + log p(y | f_h)), summed over P -> [N]"""
        f, wn = self._points(Fmu, Fvar)
        return torch.logsumexp(torch.log(wn) + self._log_density(f, ops.to_device(Y)[..., None]), dim=-1).sum(-1)


class Bernoulli(ScalarLikelihood):
    """Bernoulli(invlink=inv_probit), scalar_discrete.py: log p(y|f) = log(y == 1 ? p : 1 - p), p = inv_probit(f).  Only the probit
    link is built.  A non-finite label gives NaN (the comparison alone would read it as class 0)."""

    device_lik = "bernoulli_probit"

    def __init__(self, invlink=inv_probit):
        if invlink is not inv_probit:
            raise NotImplementedError("Bernoulli: only the inv_probit link is implemented")
        self.invlink = invlink

    def _log_density(self, F, Y):
        return self._log_density_of_p(inv_probit(F), Y)

    def _conditional_mean(self, F):
        return inv_probit(F)

    def _conditional_variance(self, F):
        p = inv_probit(F)
        return p - p * p

    def predict_mean_and_var(self, X, Fmu, Fvar):
        """scalar_discrete.py: closed form under the probit link"""
        p = inv_probit(ops.to_device(Fmu) / torch.sqrt(1 + ops.to_device(Fvar)))
        return p, p - p * p

    def predict_log_density(self, X, Fmu, Fvar, Y):
        p = self.predict_mean_and_var(X, Fmu, Fvar)[0]
        return self._log_density_of_p(p, ops.to_device(Y)).sum(-1)

    @staticmethod
    def _log_density_of_p(p, Y):
        return torch.log(torch.where(Y == 1, p, 1 - p)) + (Y - Y)


class Poisson(ScalarLikelihood):
    """Poisson(invlink=exp, binsize=1.0), scalar_discrete.py: log p = y log(lambda) - lambda - lgamma(y + 1), lambda = exp(f) binsize.
    Only the exp link is built; its variational expectations are the reference's closed form."""

    device_lik = "poisson_exp"

    def __init__(self, invlink=exp, binsize: float = 1.0):
        if invlink not in (exp, np.exp):
            raise NotImplementedError("Poisson: only the exp link is implemented")
        self.invlink = exp
        self.binsize = float(binsize)
        if not self.binsize > 0.0:
            raise ValueError("Poisson: binsize must be positive")

    def device_params(self) -> tuple:
        return (self.binsize,)

    def _log_density(self, F, Y):
        return Y * (F + log(self.binsize)) - torch.exp(F) * self.binsize - torch.lgamma(Y + 1.0)

    def _conditional_mean(self, F):
        return torch.exp(F) * self.binsize

    def _conditional_variance(self, F):
        return torch.exp(F) * self.binsize


class StudentT(ScalarLikelihood):
    """StudentT(scale=1.0, df=3.0), scalar_continuous.py: `scale` a positive Parameter, `df` a plain float."""

    device_lik = "student_t"
    device_grad_param = "scale"

    def __init__(self, scale=1.0, df: float = 3.0):
        self.df = float(df)
        self.scale = Parameter(scale, transform=positive())

    def device_params(self) -> tuple:
        return (float(self.scale.numpy()), self.df)

    def _log_density(self, F, Y):
        """logdensities.py student_t"""
        scale, df = float(self.scale.numpy()), self.df
        const = lgamma(0.5 * (df + 1.0)) - lgamma(0.5 * df) - 0.5 * (log(scale * scale) + log(df) + log(pi))
        return const - 0.5 * (df + 1.0) * torch.log(1.0 + ((Y - F) / scale) ** 2 / df)

    def _conditional_mean(self, F):
        return F

    def _conditional_variance(self, F):
        scale = float(self.scale.numpy())
        return torch.full_like(F, scale * scale * self.df / (self.df - 2.0))


def _exp_link_only(name: str, invlink):
    if invlink not in (exp, np.exp):
        raise NotImplementedError(f"{name}: only the exp link is implemented")
    return exp


class Exponential(ScalarLikelihood):
    """Exponential(invlink=exp), scalar_continuous.py: log p = -log(lambda) - y / lambda, lambda = exp(f) (logdensities.py exponential).
    Only the exp link is built; its variational expectations are the reference's closed form."""

    device_lik = "exponential_exp"

    def __init__(self, invlink=exp):
        self.invlink = _exp_link_only("Exponential", invlink)

    def _log_density(self, F, Y):
        return -F - Y * torch.exp(-F)

    def _conditional_mean(self, F):
        return torch.exp(F)

    def _conditional_variance(self, F):
        return torch.exp(2.0 * F)


class Gamma(ScalarLikelihood):
    """Gamma(invlink=exp, shape=1.0), scalar_continuous.py: `shape` a positive Parameter, the latent sets the scale exp(f):
    log p = -shape f - lgamma(shape) + (shape - 1) log y - y exp(-f) (logdensities.py gamma).  Only the exp link is built; its
    variational expectations are the reference's closed form."""

    device_lik = "gamma_exp"
    device_grad_param = "shape"

    def __init__(self, invlink=exp, shape=1.0):
        self.invlink = _exp_link_only("Gamma", invlink)
        self.shape = Parameter(shape, transform=positive())

    def device_params(self) -> tuple:
        return (float(self.shape.numpy()),)

    def _log_density(self, F, Y):
        shape = float(self.shape.numpy())
        return -shape * F - lgamma(shape) + (shape - 1.0) * torch.log(Y) - Y * torch.exp(-F)

    def _conditional_mean(self, F):
        return float(self.shape.numpy()) * torch.exp(F)

    def _conditional_variance(self, F):
        return float(self.shape.numpy()) * torch.exp(2.0 * F)


class Beta(ScalarLikelihood):
    """Beta(invlink=inv_probit, scale=1.0), scalar_continuous.py: the latent sets the mean m = inv_probit(f) of a Beta density with
    alpha = m scale, beta = scale - alpha; `scale` a positive Parameter.  The label is clipped into [1e-6, 1 - 1e-6]
    (logdensities.py beta).  Only the probit link is built."""

    device_lik = "beta_probit"
    device_grad_param = "scale"

    def __init__(self, invlink=inv_probit, scale=1.0):
        if invlink is not inv_probit:
            raise NotImplementedError("Beta: only the inv_probit link is implemented")
        self.invlink = invlink
        self.scale = Parameter(scale, transform=positive())

    def device_params(self) -> tuple:
        return (float(self.scale.numpy()),)

    def _log_density(self, F, Y):
        scale = float(self.scale.numpy())
        alpha = inv_probit(F) * scale
        beta = scale - alpha
        yc = torch.clamp(Y, 1e-6, 1.0 - 1e-6)
        return (alpha - 1.0) * torch.log(yc) + (beta - 1.0) * torch.log(1.0 - yc) + lgamma(scale) - torch.lgamma(alpha) \
            - torch.lgamma(beta)

    def _conditional_mean(self, F):
        return inv_probit(F)

    def _conditional_variance(self, F):
        m = inv_probit(F)
        return (m - m * m) / (float(self.scale.numpy()) + 1.0)


class Ordinal(ScalarLikelihood):
    """Ordinal(bin_edges), scalar_discrete.py: labels are the integers 0 .. K - 1 of K = len(bin_edges) + 1 ordered bins of the real
    line; p(y = k | f) = inv_probit((e_k - f) / sigma) - inv_probit((e_{k-1} - f) / sigma) with e_{-1} = -inf, e_{K-1} = +inf, and
    log p has 1e-6 added inside the logarithm.  `bin_edges` are fixed (1-D, strictly increasing, at most ops.ORDINAL_MAX_EDGES of
    them: the kernel takes the table by value); `sigma` is a positive Parameter.  A label that is no integer in [0, K) gives NaN
    (the choice the kernel makes, include/gpk.h: the reference would index garbage)."""

    device_lik = "ordinal"
    device_grad_param = "sigma"

    def __init__(self, bin_edges):
        edges = np.array(bin_edges, dtype=np.float64)
        if edges.ndim != 1 or edges.size < 1:
            raise ValueError("Ordinal: bin_edges must be a 1-D sequence of at least one edge")
        if edges.size > ops.ORDINAL_MAX_EDGES:
            raise ValueError(f"Ordinal: at most {ops.ORDINAL_MAX_EDGES} bin edges, got {edges.size}")
        if not (np.isfinite(edges).all() and (np.diff(edges) > 0).all()):
            raise ValueError("Ordinal: bin_edges must be finite and strictly increasing")
        self.bin_edges = edges
        self.num_bins = edges.size + 1
        self.sigma = Parameter(1.0, transform=positive())

    def device_params(self) -> tuple:
        return (float(self.sigma.numpy()), float(self.bin_edges.size)) + tuple(float(e) for e in self.bin_edges)

    def _scaled_edges(self, like: torch.Tensor):
        """(e_k / sigma with +inf appended, the same with -inf in front), each [K]"""
        e = torch.as_tensor(self.bin_edges / float(self.sigma.numpy()), dtype=torch.float64, device=like.device)
        inf = torch.full((1,), float("inf"), dtype=torch.float64, device=like.device)
        return torch.cat([e, inf]), torch.cat([-inf, e])

    def _make_phi(self, F):
        """p(y = k | f) for every bin as a last axis [..., K]; every row sums to 1 - 2e-3 (the two outermost jitters)"""
        F = ops.to_device(F)
        left, right = self._scaled_edges(F)
        fs = (F / float(self.sigma.numpy()))[..., None]
        return inv_probit(left - fs) - inv_probit(right - fs)

    def _log_density(self, F, Y):
        left, right = self._scaled_edges(F)
        ok = (Y >= 0) & (Y <= self.bin_edges.size) & (Y == torch.floor(Y))
        idx = torch.where(ok, Y, torch.zeros_like(Y)).long()
        fs = F / float(self.sigma.numpy())
        lp = torch.log(inv_probit(left[idx] - fs) - inv_probit(right[idx] - fs) + 1e-6)
        return lp + torch.where(ok, torch.zeros_like(Y), torch.full_like(Y, float("nan")))

    def _conditional_mean(self, F):
        phi = self._make_phi(F)
        return phi @ torch.arange(self.num_bins, dtype=phi.dtype, device=phi.device)

    def _conditional_variance(self, F):
        phi = self._make_phi(F)
        k = torch.arange(self.num_bins, dtype=phi.dtype, device=phi.device)
        mean = phi @ k
        return phi @ (k * k) - mean * mean


def device_grad_param(device_lik: str) -> Optional[str]:
    """the `device_grad_param` of the ScalarLikelihood class that runs as `device_lik` (None: no such class, or no such Parameter)"""
    for cls in ScalarLikelihood.__subclasses__():
        if cls.device_lik == device_lik:
            return cls.device_grad_param
    return None


class RobustMax:
    """RobustMax(num_classes, epsilon=1e-3), multiclass.py: the class with the largest latent gets probability 1 - epsilon, every
    other one epsilon / (num_classes - 1).  epsilon is a plain float (not trainable, as in the reference)."""

    def __init__(self, num_classes: int, epsilon: float = 1e-3):
        self.num_classes = int(num_classes)
        self.epsilon = float(epsilon)
        if self.num_classes < 2:
            raise ValueError("RobustMax: at least two classes")
        if not 0.0 < self.epsilon < 1.0:
            raise ValueError("RobustMax: epsilon must lie in (0, 1)")

    @property
    def eps_k1(self) -> float:
        return self.epsilon / (self.num_classes - 1.0)

    def __call__(self, F):
        """one-hot [..., C] with 1 - epsilon on the argmax of F and eps_k1 elsewhere"""
        F = ops.to_device(F)
        hot = torch.nn.functional.one_hot(torch.argmax(F, dim=-1), self.num_classes).to(F.dtype)
        return hot * (1.0 - self.epsilon - self.eps_k1) + self.eps_k1

    @staticmethod
    def _labels(Y, C: int):
        """(class index [N], 0 | NaN [N]) of a label column [N, 1]: a label that is no integer in [0, C) gives NaN (the choice the
        kernel makes, include/gpk.h: the reference would index garbage)"""
        y = Y.reshape(-1)
        ok = (y >= 0) & (y < C) & (y == torch.floor(y))
        return torch.where(ok, y, torch.zeros_like(y)).long(), torch.where(ok, torch.zeros_like(y), torch.full_like(y, float("nan")))

    def prob_is_largest(self, Y, mu, var, gh_x, gh_w):
        """P(f_y > f_k for all k != y) under independent N(mu_k, var_k), [N, 1]: the Gauss-Hermite sum over the label's latent of the
        product of the other latents' normal CDFs (with the reference's clamps and its 1e-4 CDF jitter)."""
        Y, mu, var = ops.to_device(Y), ops.to_device(mu), ops.to_device(var)
        gh_x = torch.as_tensor(gh_x, dtype=torch.float64, device=mu.device)
        gh_w = torch.as_tensor(gh_w, dtype=torch.float64, device=mu.device)
        idx, ynan = self._labels(Y, self.num_classes)
        on = torch.nn.functional.one_hot(idx, self.num_classes).to(mu.dtype)                       # [N, C]
        mu_y, var_y = (on * mu).sum(1, keepdim=True), (on * var).sum(1, keepdim=True)
        X = mu_y + torch.sqrt(torch.clamp(2.0 * var_y, min=1e-10)) * gh_x                          # [N, H]
        dist = (X[:, None, :] - mu[:, :, None]) / torch.sqrt(torch.clamp(var, min=1e-10))[:, :, None]
        cdfs = 0.5 * torch.special.erfc(-dist / sqrt(2.0)) * (1.0 - 2e-4) + 1e-4
        cdfs = cdfs * (1.0 - on)[:, :, None] + on[:, :, None]
        return torch.prod(cdfs, dim=1) @ (gh_w / sqrt(pi)).reshape(-1, 1) + ynan[:, None]


class MultiClass(Likelihood):
    """MultiClass(num_classes, invlink=None), multiclass.py: labels Y [N, 1] in 0 .. C - 1, one latent per class.  Only the
    RobustMax link (the default) is built; Softmax is Monte-Carlo in the reference.  `variational_expectations`, the hot one, runs
    in gpk_likelihood_varexp_sum (GPK_LIK_MULTICLASS_ROBUSTMAX); the prediction-side integrals are device glue over the 20-node
    table.  The C latents of a row are coupled, so they cannot be chunked like the columns of a ScalarLikelihood: C <= 16."""

    device_lik = "multiclass_robustmax"
    MAX_DEVICE_CLASSES = 16

    def __init__(self, num_classes: int, invlink=None):
        self.num_classes = int(num_classes)
        if invlink is None:
            invlink = RobustMax(self.num_classes)
        if not isinstance(invlink, RobustMax):
            raise NotImplementedError("MultiClass: only the RobustMax link is implemented")
        if invlink.num_classes != self.num_classes:
            raise ValueError("MultiClass: the link has another number of classes")
        self.invlink = invlink

    def device_params(self) -> tuple:
        return (self.invlink.epsilon,)

    def check_device_classes(self, num_latents=None):
        """ValueError if the latents are not one per class; NotImplementedError past the kernel's limit"""
        if num_latents is not None and int(num_latents) != self.num_classes:
            raise ValueError(f"MultiClass({self.num_classes}) needs {self.num_classes} latent GPs, got {int(num_latents)}")
        if self.num_classes > self.MAX_DEVICE_CLASSES:
            raise NotImplementedError(f"MultiClass: at most {self.MAX_DEVICE_CLASSES} classes (the latents of a row are coupled in "
                                      f"one kernel pass and cannot be chunked), got {self.num_classes}")

    def _flat(self, *tensors):
        out = []
        for t in tensors:
            t = ops.to_device(t)
            out.append(t.reshape(-1, t.shape[-1]))
        return out

    def log_prob(self, X, F, Y):
        F, Y = ops.to_device(F), ops.to_device(Y)
        Ff, Yf = self._flat(F, Y)
        idx, ynan = RobustMax._labels(Yf, self.num_classes)
        hits = torch.argmax(Ff, dim=-1) == idx
        eps = self.invlink.epsilon
        lp = torch.where(hits, torch.full_like(ynan, log(1.0 - eps)), torch.full_like(ynan, log(self.invlink.eps_k1))) + ynan
        return lp.reshape(F.shape[:-1])

    def conditional_mean(self, X, F):
        return self.invlink(F)

    def conditional_variance(self, X, F):
        p = self.invlink(F)
        return p - p * p

    def variational_expectations(self, X, Fmu, Fvar, Y) -> torch.Tensor:
        """multiclass.py MultiClass._variational_expectations: p log(1 - eps) + (1 - p) log(eps / (C - 1)) per row, [N]"""
        self.check_device_classes(tuple(Fmu.shape)[-1])   # (refused before anything touches the device)
        Fmu = ops.to_device(Fmu)
        Fm, Fv, Yd = self._flat(Fmu, Fvar, Y)
        rows = ops.likelihood_varexp_sum(Yd[:, :1], Fm.contiguous(), s0=None, ssq=Fv.t().contiguous(), knn=[0.0], lik=self.device_lik,
                                         params=self.device_params(), want_rows=True)[1]
        return rows.reshape(Fmu.shape[:-1])

    def _density(self, Fm, Fv, Yd):
        """_predict_non_logged_density on flat operands: p (1 - eps) + (1 - p) eps / (C - 1), [N]"""
        x, w = ops.gauss_hermite(DEFAULT_NUM_GAUSS_HERMITE_POINTS)
        p = self.invlink.prob_is_largest(Yd, Fm, Fv, x, w)[:, 0]
        return p * (1.0 - self.invlink.epsilon) + (1.0 - p) * self.invlink.eps_k1

    def predict_mean_and_var(self, X, Fmu, Fvar):
        """multiclass.py: the density of every class in turn, ([..., C], ps - ps^2)"""
        Fmu = ops.to_device(Fmu)
        Fm, Fv = self._flat(Fmu, Fvar)
        ps = torch.stack([self._density(Fm, Fv, torch.full((Fm.shape[0], 1), float(i), dtype=Fm.dtype, device=Fm.device))
                          for i in range(self.num_classes)], dim=1).reshape(Fmu.shape[:-1] + (self.num_classes,))
        return ps, ps - ps * ps

    def predict_log_density(self, X, Fmu, Fvar, Y):
        Fmu = ops.to_device(Fmu)
        Fm, Fv, Yd = self._flat(Fmu, Fvar, Y)
        return torch.log(self._density(Fm, Fv, Yd[:, :1])).reshape(Fmu.shape[:-1])


class SwitchedLikelihood(Likelihood):
    """SwitchedLikelihood(likelihood_list), likelihoods/misc.py: the last column of Y is a task label and each row is scored by its own
    task's likelihood; Y[..., :-1] are the values.  The label is read as the Coregion kernel reads one (truncation toward zero, valid
    inside (-1, T)); a row with an invalid label gives NaN.  Members: `Gaussian` with one `variance` Parameter, or a ScalarLikelihood
    whose `device_lik` is in ops.SWITCHED_MEMBERS (Bernoulli, Poisson, StudentT, Exponential, Gamma, Beta) -- anything else is refused
    when the likelihood is built.  `variational_expectations`, the hot one, is ONE launch for all tasks (gpk_switched_varexp_sum); the
    densities are elementwise device glue over the members' own.  Without Y there is no task: the conditional moments and
    predict_mean_and_var raise, as in the reference."""

    def __init__(self, likelihood_list):
        members = list(likelihood_list)
        if not 1 <= len(members) <= ops.SWITCHED_MAX_TASKS:
            raise ValueError(f"SwitchedLikelihood: 1 .. {ops.SWITCHED_MAX_TASKS} members, got {len(members)}")
        for t, lik in enumerate(members):
            why = self._refusal(lik)
            if why is not None:
                raise NotImplementedError(f"SwitchedLikelihood: member {t} ({type(lik).__name__}) {why}")
        self.likelihoods = members

    @staticmethod
    def _refusal(lik) -> Optional[str]:
        """why `lik` cannot be a member, or None"""
        if isinstance(lik, Gaussian):
            if lik.is_heteroskedastic:
                return "has a noise Function: a member's noise is one `variance` Parameter"
            return None if lik.has_variance_parameter else "holds its noise as `scale=`: a member's noise is one `variance` Parameter"
        if isinstance(lik, SwitchedLikelihood):
            return "is itself switched: a row has one task label"
        if isinstance(lik, MultiClass):
            return "couples the latents of a row: the per-row choice is between scalar likelihoods"
        if isinstance(lik, Ordinal):
            return "needs an edge table per task, which the switched stage's table of three constants per task does not hold"
        if isinstance(lik, ScalarLikelihood) and lik.device_lik in ops.SWITCHED_MEMBERS:
            return None
        return "has no body in the switched variational-expectation stage (ops.SWITCHED_MEMBERS)"

    @property
    def num_tasks(self) -> int:
        return len(self.likelihoods)

    def device_members(self) -> tuple:
        """the (name, params) table of ops.switched_varexp_sum at the current parameter values"""
        return tuple(("gaussian", (lik.noise_variance(),)) if isinstance(lik, Gaussian) else (lik.device_lik, lik.device_params())
                     for lik in self.likelihoods)

    def device_grad_params(self) -> list:
        """per task, the member's Parameter that out[1 + t] of the stage differentiates, or None"""
        return [lik.variance if isinstance(lik, Gaussian) else
                (getattr(lik, lik.device_grad_param) if lik.device_grad_param else None) for lik in self.likelihoods]

    def _tasks(self, Y):
        """(values [..., P], task index [..., 1] with 0 in place of an invalid one, 0 | NaN [..., 1]) of Y [..., P + 1]"""
        Y = ops.to_device(Y)
        lab = Y[..., -1:]
        ok = (lab > -1.0) & (lab < float(self.num_tasks))
        task = torch.where(ok, torch.trunc(lab), torch.zeros_like(lab)).long()
        return Y[..., :-1], task, torch.where(ok, torch.zeros_like(lab), torch.full_like(lab, float("nan")))

    def _select(self, per_member, task, nan):
        """per_member[t] where task == t, plus the NaN of an invalid label"""
        out = per_member[0]
        for t in range(1, self.num_tasks):
            out = torch.where(task == t, per_member[t], out)
        return out + nan

    @staticmethod
    def _member_log_density(lik, F, Yv, extra_var=None):
        if isinstance(lik, Gaussian):
            v = lik.noise_variance()
            return gaussian(Yv, F, v if extra_var is None else extra_var + v)
        return lik._log_density(F, Yv)

    def log_prob(self, X, F, Y):
        F = ops.to_device(F)
        Yv, task, nan = self._tasks(Y)
        return self._select([self._member_log_density(lik, F, Yv) for lik in self.likelihoods], task, nan).sum(-1)

    def predict_log_density(self, X, Fmu, Fvar, Y):
        """log int p(y | f) N(f | mu, v) df per element by the row's own member (Gaussian: closed form; Bernoulli: its closed form;
        the others: the 20-node log-sum-exp of ScalarLikelihood), summed over the outputs -> [N]"""
        Fmu, Fvar = ops.to_device(Fmu), ops.to_device(Fvar)
        Yv, task, nan = self._tasks(Y)
        per = []
        for lik in self.likelihoods:
            if isinstance(lik, Gaussian):
                per.append(self._member_log_density(lik, Fmu, Yv, extra_var=Fvar))
            elif isinstance(lik, Bernoulli):
                per.append(lik._log_density_of_p(lik.predict_mean_and_var(X, Fmu, Fvar)[0], Yv))
            else:
                f, wn = lik._points(Fmu, Fvar)
                per.append(torch.logsumexp(torch.log(wn) + lik._log_density(f, Yv[..., None]), dim=-1))
        return self._select(per, task, nan).sum(-1)

    def variational_expectations(self, X, Fmu, Fvar, Y) -> torch.Tensor:
        """misc.py SwitchedLikelihood.variational_expectations -- per-row values [N], summed over the P outputs; the kernel takes at
        most 16 output columns per call"""
        Fmu, Fvar, Y = ops.to_device(Fmu), ops.to_device(Fvar), ops.to_device(Y)
        lead, P = Fmu.shape[:-1], Fmu.shape[-1]
        if Y.shape[-1] != P + 1:
            raise ValueError(f"SwitchedLikelihood: Y needs {P} value columns and the task label behind them, got {Y.shape[-1]} columns")
        Fm, Fv, Yd = Fmu.reshape(-1, P), Fvar.reshape(-1, P), Y.reshape(-1, P + 1)
        members = self.device_members()
        total = None
        for c0 in range(0, P, 16):
            c1 = min(c0 + 16, P)
            rows = ops.switched_varexp_sum(Yd[:, c0:], Fm[:, c0:c1].contiguous(), s0=None, ssq=Fv[:, c0:c1].t().contiguous(), knn=[0.0],
                                           members=members, ylab=P - c0, want_rows=True)[1]
            total = rows if total is None else total + rows
        return total.reshape(lead)

    def _needs_task(self, what):
        raise NotImplementedError(f"SwitchedLikelihood.{what}: without Y there is no task label to choose a member by")

    def predict_mean_and_var(self, X, Fmu, Fvar):
        self._needs_task("predict_mean_and_var")

    def conditional_mean(self, X, F):
        self._needs_task("conditional_mean")

    def conditional_variance(self, X, F):
        self._needs_task("conditional_variance")
