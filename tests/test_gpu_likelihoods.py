"""GPU tests of the non-Gaussian likelihoods (Bernoulli / Poisson / StudentT): the quadrature kernel behind
`ops.likelihood_varexp_sum`, the fused shard `ops.svgp_elbo_shard_lik`, the likelihood classes, `SVGP.elbo` / `predict_y` /
`predict_log_density` and the reverse pass `SVGP.elbo_and_grad` with these likelihoods.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_likelihoods_emulated.py imports them without this
module's `gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py, with tests/fake_likelihood_ops.py).

References.  Values: oracle/gp_oracle.py gives q(f) (`svgp_predict_f`) and the KL (`gauss_kl`); the Gauss-Hermite sum over
numpy.polynomial.hermite.hermgauss(20) is written here (`_reference`), in np.longdouble with erfc / lgamma from mpmath (40
digits).  Gradients: a torch-CPU fp64 autograd restatement of the same ELBO (`_torch_elbo`), which differentiates the same
quadrature sum.  u = 2^-53 throughout; every bound is derived next to its check.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle as orc  # noqa: E402  (checker only)
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)

U = 2.0 ** -53
LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
GH_X, GH_W = np.polynomial.hermite.hermgauss(20)
LIKS = [("bernoulli_probit", ()), ("poisson_exp", (0.7,)), ("student_t", (0.8, 3.0))]
LIK_IDS = [name for name, _ in LIKS]


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _refused():
    """what an out-of-contract call raises: GpkError / ValueError from the device wrapper, AssertionError from the emulation"""
    from gpflow_amd._lib import GpkError
    return (GpkError, ValueError, AssertionError)


# ------------------------------------------------------------------------------------------------ the reference
def _mp_map(fn, z):
    """elementwise mpmath function on a longdouble array, in and out without loss (a longdouble is the sum of two doubles)"""
    import mpmath
    mpmath.mp.dps = 40
    z = np.asarray(z, dtype=LD)
    out = np.empty(z.shape, dtype=LD)
    fi, fo = z.reshape(-1), out.reshape(-1)
    for i in range(fi.size):
        hi = float(fi[i])
        v = fn(mpmath.mpf(hi) + mpmath.mpf(float(fi[i] - LD(hi))))
        vh = float(v)
        fo[i] = LD(vh) + LD(float(v - mpmath.mpf(vh)))
    return out


def _erfc_ld(z):
    import mpmath
    return _mp_map(mpmath.erfc, z)


def _lgamma_ld(z):
    import mpmath
    return _mp_map(mpmath.loggamma, z)


def _erfc_f64(z):
    import scipy.special
    return scipy.special.erfc(np.asarray(z, dtype=np.float64)).astype(LD)


def _reference(lik, par, Y, mu, fv, emu=0.0, efv=0.0, erfc=_erfc_ld):
    """The definition, in longdouble: (ve, dmu, dvar, dscale) [rows, P] and a bound on the fp64 error of each.

    Y, mu, fv: the exact operands (longdouble); emu, efv: how far an fp64 evaluation of mu = fmean + mean_const and
    fvar = knn - s0 + ssq may sit from them.  Error model of one element, first order in u:
      * the node  f_h = fma(sd, x_h, mu),  sd = sqrt(2 fvar):   |df_h| <= u (|f_h| + |mu|) + |x_h| sd (u + efv / (2 fvar)) + emu   (=: ef)
      * a node value g(f_h) moves by |g'(f_h)| ef and carries the library functions' own error.  The OpenCL fp64 limits, which the
        device math library states it meets, are erfc 16 ulp, exp 3, log 3, log1p 2; the few multiplications around them add
        less than 5 more:  24 u (1 + |g|)  ("cg").  g' and its derivative g'' (closed forms below) do the same for the two
        derivative outputs ("cp"; the Bernoulli g' holds exp(-f^2 / 2), whose ARGUMENT error u f^2 is a relative error of the value)
      * the 20-term weighted sum, its four-lane combination and the products w_h g_h: 32 u sum_h w_h |g_h|
      * dvar divides by sd:  relative 4 u + efv / (2 fvar) more.
    For the Bernoulli likelihood |g'| = 0.998 phi(f) / q <= 0.4 / 1e-3: the sensitivity of log inv_probit is bounded by the jitter."""
    Y, mu, fv = (np.asarray(a, dtype=LD) for a in (Y, mu, fv))
    emu, efv = np.broadcast_to(np.asarray(emu, dtype=LD), mu.shape), np.broadcast_to(np.asarray(efv, dtype=LD), mu.shape)
    emu = emu + U * np.abs(mu)
    zero = np.zeros(mu.shape, dtype=LD)
    if lik == "poisson_exp":
        b = LD(par[0])
        arg = mu + fv / 2
        e = np.exp(arg) * b
        t = [Y * mu, e, _lgamma_ld(Y + 1), Y * np.log(b)]
        ve = t[0] - t[1] - t[2] + t[3]
        rel_e = 4 * U + U * np.abs(arg) + emu + efv / 2            # exp: 3 ulp + the rounding and the operand error of its argument
        # lgamma has no stated ulp limit: allowed 16 ulp of max(|lgamma|, 1), the loosest limit the specification gives a function
        b_ve = 4 * U * sum(np.abs(x) for x in t) + e * rel_e + np.abs(Y) * emu + 16 * U * np.maximum(np.abs(t[2]), 1)
        return (ve, Y - e, -e / 2, zero), (b_ve, U * np.abs(Y - e) + e * rel_e, e * rel_e, zero)
    x, wn = GH_X.astype(LD), GH_W.astype(LD) / np.sqrt(PI)
    sd = np.sqrt(2 * fv)
    f = mu[..., None] + sd[..., None] * x
    ef = U * (np.abs(f) + np.abs(mu)[..., None]) + np.abs(x) * (sd * (U + efv / (2 * fv)))[..., None] + emu[..., None]
    y = Y[..., None]
    if lik == "bernoulli_probit":
        sgn = np.where(y == 1, LD(1), LD(-1))
        a, eps = LD(1) - 2 * LD("1e-3"), LD("1e-3")
        q = erfc(-sgn * f / np.sqrt(LD(2))) / 2 * a + eps
        g = np.log(q)
        g1 = sgn * a * np.exp(-f * f / 2) / np.sqrt(2 * PI) / q
        g2 = -f * g1 - g1 * g1
        gmag, cp = 1 + np.abs(g), 40 + f * f
        gs = gs1 = np.zeros(f.shape, dtype=LD)
    else:
        scale, df = LD(par[0]), LD(par[1])
        lg = _lgamma_ld(np.array([(df + 1) / 2, df / 2]))
        consts = [lg[0], lg[1], np.log(scale * scale) / 2, np.log(df) / 2, np.log(PI) / 2]
        r = (y - f) / scale
        den = df + r * r
        lp = (df + 1) / 2 * np.log1p(r * r / df)
        g = consts[0] - consts[1] - consts[2] - consts[3] - consts[4] - lp
        g1 = (df + 1) * r / (scale * den)
        g2 = -(df + 1) * (df - r * r) / (scale * scale * den * den)
        gmag, cp = 1 + sum(abs(c) for c in consts) + lp + (df + 1), 24 + 0 * f
        gs = ((df + 1) * r * r / den - 1) / scale
        gs1 = -(df + 1) * 2 * r * df / (den * den) / (scale * scale)
    S = lambda v: (v * wn).sum(-1)   # noqa: E731
    ve, dmu = S(g), S(g1)
    dvar = S(g1 * x) / sd
    b_ve = S(np.abs(g1) * ef + 24 * U * gmag) + 32 * U * S(np.abs(g))
    b_dmu = S(np.abs(g2) * ef + cp * U * np.abs(g1)) + 32 * U * S(np.abs(g1))
    b_dvar = (S(np.abs(x) * (np.abs(g2) * ef + cp * U * np.abs(g1))) + 32 * U * S(np.abs(g1 * x))) / sd \
        + np.abs(dvar) * (4 * U + efv / (2 * fv))
    b_dsc = S(np.abs(gs1) * ef + 24 * U * (np.abs(gs) + 1 / LD(par[0] if par else 1))) + 32 * U * S(np.abs(gs))
    return (ve, dmu, dvar, S(gs)), (b_ve, b_dmu, b_dvar, b_dsc)


def _labels(lik, rng, shape):
    if lik == "bernoulli_probit":
        return (rng.uniform(size=shape) < 0.5).astype(np.float64)
    if lik == "poisson_exp":
        return rng.poisson(3.0, size=shape).astype(np.float64)
    return rng.normal(size=shape) * 1.5


def _within(name, got, ref, bound):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    if err.size:
        worst = int(np.argmax(err / np.maximum(bound, LD(1e-300))))
        print(f"{name}: max error / bound = {float((err / np.maximum(bound, LD(1e-300))).reshape(-1)[worst]):.3g} "
              f"(error {float(err.reshape(-1)[worst]):.3g})")
    bad = ~(err <= bound)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} entries over the bound"


# ------------------------------------------------------------------------------------------------ 2. the kernel
# (rows, P, per-latent s0 / knn, layout of Y: "c" contiguous, "ld" odd leading dimension)
KERNEL_CASES = [
    (0, 1, False, "c"),        # zero rows: out = [0, 0], nothing else written
    (1, 1, False, "c"),        # size 1: one lane group of one wave
    (67, 4, True, "ld"),       # P = 4: four rows per wave pass, a partial last pass; per-latent s0 / knn; odd ld of Y
    (130, 5, False, "c"),      # P = 5 does not divide 16: three rows per pass, one idle lane group
    (33, 16, True, "ld"),      # P = 16 (maximum): one row per pass
    (257, 1, False, "ld"),     # P = 1: sixteen rows per pass, more than one block
]
# more passes than 1024 blocks x 4 waves: the grid-stride loop (closed-form / elementary-function likelihoods only: the
# Bernoulli reference evaluates erfc in mpmath)
BIG_CASE = (70001, 1, False, "c")


def _kernel_inputs(lik, case):
    rows, P, per, layout = case
    rng = np.random.default_rng(rows * 31 + P)
    Y = _labels(lik, rng, (rows, P))
    F = rng.normal(size=(rows, P)) * (0.7 if lik == "poisson_exp" else 1.5)
    s0 = rng.uniform(0, 0.5, size=(P, rows) if per else (rows,))
    ssq = rng.uniform(0, 0.6, size=(P, rows))
    knn = list(1.0 + 0.1 * np.arange(P)) if per else [1.2]
    return Y, F, s0, ssq, knn


@pytest.mark.parametrize("case", KERNEL_CASES + [BIG_CASE], ids=str)
@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_likelihood_varexp_sum_contract(gp, lik, par, case):
    """The contract rules of test_gpu_contract.py for the quadrature kernel: error under the derived bound (`_reference`), inputs
    bitwise unchanged, a second call bit-identical, rows = 0 writes 0.  A sum's error is measured against sum |term|: the Poisson
    terms change sign."""
    from gpflow_amd import ops
    if case == BIG_CASE and lik == "bernoulli_probit":
        case = (257, 2, True, "c")      # (the same slot of the table: two latents, eight rows per pass)
    rows, P, per, layout = case
    Y, F, s0, ssq, knn = _kernel_inputs(lik, case)
    mc = 0.1
    s0c = (s0.T if per else s0[:, None]).astype(LD)
    knl = np.asarray(knn, dtype=LD)[None, :]
    fv = knl - s0c + ssq.T.astype(LD)
    efv = 2 * U * (np.abs(knl) + np.abs(s0c) + ssq.T)             # two roundings: knn - s0, then + ssq
    mu = F.astype(LD) + LD(mc)
    (ve, dmu, dvar, dsc), (b_ve, b_dmu, b_dvar, b_dsc) = _reference(lik, par, Y, mu, fv, emu=U * np.abs(mu), efv=efv)
    Yfull = np.concatenate([Y, np.full((rows, 2 if P % 2 else 1), np.nan)], axis=1) if layout == "ld" else Y
    tYf = ops.to_device(Yfull)
    tY = tYf[:, :P]
    tF, ts0, tss = ops.to_device(F), ops.to_device(s0), ops.to_device(ssq)

    def call():
        return ops.likelihood_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, lik=lik, params=par, mean_const=mc, s0_per_latent=per,
                                         want_fvar=True, want_rows=True, want_grads=True)
    out, rws, gmu, gvar, fvar = call()
    # sums: the terms' own bounds + 2 (n + 2) u sum |term| for the two-stage reduction over n terms
    n = rows * P
    _within(f"{lik} out[0]", _np(out)[0:1], [ve.sum()], [b_ve.sum() + 2 * (n + 2) * U * np.abs(ve).sum()])
    _within(f"{lik} out[1]", _np(out)[1:2], [dsc.sum()], [b_dsc.sum() + 2 * (n + 2) * U * np.abs(dsc).sum()])
    if lik != "student_t":
        assert float(_np(out)[1]) == 0.0
    _within(f"{lik} rows", _np(rws), ve.sum(1), b_ve.sum(1) + 2 * (P + 2) * U * np.abs(ve).sum(1))
    _within(f"{lik} dmu", _np(gmu), dmu, b_dmu)
    _within(f"{lik} dvar", _np(gvar), dvar, b_dvar)
    _within(f"{lik} fvar", _np(fvar), fv, efv + LD(1e-300))
    for t, a in ((tYf, Yfull), (tF, F), (ts0, s0), (tss, ssq)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    again = call()
    for first, second in zip((out, rws, gmu, gvar, fvar), again):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"
    if rows == 0:
        assert _np(out).tolist() == [0.0, 0.0]
    # without the optional operands and outputs: fvar = knn, only the sums
    if rows:
        only = ops.likelihood_varexp_sum(tY, tF, s0=None, ssq=None, knn=[knn[0]], lik=lik, params=par)
        assert only[1] is None and only[2] is None and only[3] is None and only[4] is None
        (ve0, _, _, _), (b0, _, _, _) = _reference(lik, par, Y, F.astype(LD), np.full((rows, P), LD(knn[0])), emu=0.0, efv=0.0)
        _within(f"{lik} out[0], fvar = knn", _np(only[0])[0:1], [ve0.sum()], [b0.sum() + 2 * (n + 2) * U * np.abs(ve0).sum()])


def test_likelihood_varexp_sum_refuses_out_of_contract(gp):
    """17 latents, an unknown likelihood, a missing or non-positive parameter: refused on the device and by the emulation."""
    from gpflow_amd import ops
    Y = ops.to_device(np.zeros((3, 17)))
    with pytest.raises(_refused()):
        ops.likelihood_varexp_sum(Y, Y, s0=None, ssq=None, knn=[1.0], lik="bernoulli_probit")
    Y = ops.to_device(np.ones((3, 2)))
    for lik, par in (("logit", ()), ("student_t", (1.0,)), ("student_t", (-1.0, 3.0)), ("student_t", (1.0, 0.0)),
                     ("poisson_exp", (0.0,)), ("poisson_exp", ())):
        with pytest.raises(_refused()):
            ops.likelihood_varexp_sum(Y, Y, s0=None, ssq=None, knn=[1.0], lik=lik, params=par)
    with pytest.raises(_refused()):
        ops.gauss_hermite(19)
    Z = ops.to_device(np.random.default_rng(0).normal(size=(5, 2)))
    with pytest.raises(_refused()):
        ops.svgp_elbo_shard_lik(Z, Z, ops.to_device(np.ones((5, 1))), ops.to_device(np.zeros((5, 1))),
                                ops.to_device(np.eye(5)[None]), variance=1.0, lengthscales=1.0, lik="student_t", params=(0.0, 3.0),
                                jitter=1e-6)


# ------------------------------------------------------------------------------------------------ 6. non-finite inputs
@pytest.mark.parametrize("where", ["Y", "fmean", "ssq"])
@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_likelihood_varexp_sum_nonfinite(gp, lik, par, where):
    """A NaN planted in Y, fmean or ssq reaches out[0], its own row of rows_out and its own entry of dmu / dvar -- and nothing
    else: every other entry is bit-identical to the clean run."""
    from gpflow_amd import ops
    rows, P, b, p = 41, 3, 17, 1
    Y, F, s0, ssq, knn = _kernel_inputs(lik, (rows, P, False, "c"))

    def run(Y, F, ssq):
        r = ops.likelihood_varexp_sum(ops.to_device(Y), ops.to_device(F), s0=ops.to_device(s0), ssq=ops.to_device(ssq), knn=knn,
                                      lik=lik, params=par, want_rows=True, want_grads=True)
        return [_np(t) for t in r[:4]]
    clean = run(Y, F, ssq)
    assert all(np.isfinite(a).all() for a in clean)
    arrs = {"Y": Y.copy(), "fmean": F.copy(), "ssq": ssq.copy()}
    if where == "ssq":
        arrs[where][p, b] = np.nan
    else:
        arrs[where][b, p] = np.nan
    out, rws, gmu, gvar = run(arrs["Y"], arrs["fmean"], arrs["ssq"])
    assert np.isnan(out[0])
    hit_rows = np.zeros(rows, dtype=bool); hit_rows[b] = True
    hit = np.zeros((rows, P), dtype=bool); hit[b, p] = True
    assert np.isnan(rws[b]) and np.array_equal(_bits(rws[~hit_rows]), _bits(clean[1][~hit_rows]))
    for name, got, ref in (("dmu", gmu, clean[2]), ("dvar", gvar, clean[3])):
        assert np.isnan(got[b, p]), name
        assert np.array_equal(_bits(got[~hit]), _bits(ref[~hit])), name
    if lik == "student_t":
        assert np.isnan(out[1])
    else:
        assert out[1] == 0.0


# ------------------------------------------------------------------------------------------------ 3. the method, independently
def test_poisson_quadrature_defaults_against_closed_forms(gp):
    """Poisson.predict_mean_and_var is the generic quadrature of E[y|f] = Var[y|f] = exp(f) binsize; under N(mu, v) the mean is
    exp(mu + v / 2) binsize in closed form and the variance E_y + E_y^2 (exp(v) - 1).  20 nodes integrate exp(sqrt(2 v) x) against
    exp(-x^2) with a truncation error below 1e-17 relative for v <= 4 (remainder a^40 20! / (40! 2^20), a = sqrt(2 v) <= 2.83), so
    what is left is rounding: exp 3 ulp with an argument error u |f| (relative), the product and the 20-term sum -- 32 u plus
    u max|f_h| relative, all terms positive.  The second moment holds exp(2 f): its remainder (a doubled) is only negligible for
    v <= 0.5, and the variance subtracts E_y^2: its bound carries the cancellation."""
    from gpflow_amd import ops
    rng = np.random.default_rng(3)
    lik = gp.likelihoods.Poisson(binsize=0.7)
    mu = 2.0 * rng.normal(size=(200, 2))
    v = rng.uniform(0.01, 4.0, size=(200, 2))
    E, _ = lik.predict_mean_and_var(None, ops.to_device(mu), ops.to_device(v))
    ref = np.exp(mu.astype(LD) + v.astype(LD) / 2) * LD(0.7)
    fmax = np.abs(mu) + np.sqrt(2 * v) * np.abs(GH_X).max()
    _within("Poisson E_y", _np(E), ref, (32 + fmax) * U * ref)
    v = rng.uniform(0.01, 0.5, size=(200, 2))
    E, V = lik.predict_mean_and_var(None, ops.to_device(mu), ops.to_device(v))
    Er = np.exp(mu.astype(LD) + v.astype(LD) / 2) * LD(0.7)
    Vr = Er + Er * Er * np.expm1(v.astype(LD))
    fmax = np.abs(mu) + np.sqrt(2 * v) * np.abs(GH_X).max()
    _within("Poisson V_y", _np(V), Vr, (32 + 2 * fmax) * U * (Er + 2 * Er * Er * np.exp(v.astype(LD))))
    # the closed-form variational expectations are what the kernel computes (checked above against the same formula);
    # the class method returns the row sums
    Y = _labels("poisson_exp", rng, (200, 2))
    ve = lik.variational_expectations(None, ops.to_device(mu), ops.to_device(v), ops.to_device(Y))
    (r, _, _, _), (b, _, _, _) = _reference("poisson_exp", (0.7,), Y, mu.astype(LD), v.astype(LD))
    _within("Poisson variational_expectations", _np(ve), r.sum(1), b.sum(1) + 8 * U * np.abs(r).sum(1))


def test_student_t_predictions_are_exact_moments(gp):
    """StudentT.predict_mean_and_var = (Fmu, Fvar + scale^2 df / (df - 2)): the quadrature integrates polynomials of degree <= 39
    exactly, so only rounding is left -- sum_h w_h / sqrt(pi) = 1 and the 20 products to 32 u of sum |term|."""
    from gpflow_amd import ops
    rng = np.random.default_rng(4)
    lik = gp.likelihoods.StudentT(scale=0.8, df=5.0)
    mu, v = rng.normal(size=(100, 3)) * 2, rng.uniform(0.01, 3.0, size=(100, 3))
    E, V = lik.predict_mean_and_var(None, ops.to_device(mu), ops.to_device(v))
    c = LD(0.8) ** 2 * 5 / 3
    wn = GH_W / np.sqrt(np.pi)
    f = mu[..., None] + np.sqrt(2 * v)[..., None] * GH_X
    _within("StudentT E_y", _np(E), mu.astype(LD), 32 * U * (np.abs(f) * wn).sum(-1))
    _within("StudentT V_y", _np(V), v.astype(LD) + c, 32 * U * (((f * f + float(c)) * wn).sum(-1) + mu * mu))
    assert float(lik.conditional_variance(None, ops.to_device(mu))[0, 0]) == pytest.approx(float(c), rel=4 * U)
    np.testing.assert_array_equal(_np(lik.conditional_mean(None, ops.to_device(mu))), mu)


def test_bernoulli_predictions_closed_form(gp):
    """Bernoulli.predict_mean_and_var is the closed form p = inv_probit(mu / sqrt(1 + v)), (p, p - p^2) -- NOT the 20-node sum,
    from which it differs by 2e-5 (the jitter is applied after the integral instead of inside it): only a loose comparison of the two."""
    from gpflow_amd import ops
    rng = np.random.default_rng(5)
    lik = gp.likelihoods.Bernoulli()
    mu, v = rng.normal(size=(100, 2)) * 2, rng.uniform(0.01, 3.0, size=(100, 2))
    E, V = lik.predict_mean_and_var(None, ops.to_device(mu), ops.to_device(v))
    z = mu.astype(LD) / np.sqrt(1 + v.astype(LD))
    p = _erfc_ld(-z / np.sqrt(LD(2))) / 2 * (LD(1) - 2 * LD("1e-3")) + LD("1e-3")
    # erf 16 ulp (the OpenCL limit) of a value <= 1, the argument's two roundings through |d inv_probit| <= 0.4, the jitter arithmetic
    _within("Bernoulli E_y", _np(E), p, 24 * U * (1 + np.abs(z)))
    _within("Bernoulli V_y", _np(V), p - p * p, 56 * U * (1 + np.abs(z)))
    Y = _labels("bernoulli_probit", rng, (100, 2))
    ld = lik.predict_log_density(None, ops.to_device(mu), ops.to_device(v), ops.to_device(Y))
    ref = np.log(np.where(Y == 1, p, 1 - p)).sum(1)
    _within("Bernoulli predict_log_density", _np(ld), ref, 2 * 1e3 * 32 * U * (1 + np.abs(z)).sum(1))   # |d log q| <= dq / 1e-3
    Eq, _ = gp.likelihoods.ScalarLikelihood.predict_mean_and_var(lik, None, ops.to_device(mu), ops.to_device(v))
    assert float(np.abs(_np(Eq) - _np(E)).max()) < 1e-4
    lp = lik.log_prob(None, ops.to_device(mu), ops.to_device(Y))
    f = mu.astype(LD)
    q = _erfc_ld(-np.where(Y == 1, 1, -1) * f / np.sqrt(LD(2))) / 2 * (LD(1) - 2 * LD("1e-3")) + LD("1e-3")
    _within("Bernoulli log_prob", _np(lp), np.log(q).sum(1), 2 * 1e3 * 24 * U * np.ones(100))


# ------------------------------------------------------------------------------------------------ 4. models
def _svgp_problem(lik, M, N, D, P, seed, q_diag, whiten=True, ls=0.9, var=1.3):
    """whiten=False: the same q(u) expressed un-whitened (q_mu -> Lm q_mu, q_sqrt -> Lm q_sqrt; a diagonal q_sqrt scaled by
    diag(Kuu^-1)^-1/2), so that q(f) stays of order one -- an arbitrary un-whitened q against an ill-conditioned Kuu gives latent
    values of 1e3 and more, where exp(f) of the Poisson link overflows."""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N, D))
    Z = X[:M] + 0.05 * rng.normal(size=(M, D))
    q_mu = 0.4 * rng.normal(size=(M, P))
    if q_diag:
        q_sqrt = rng.uniform(0.3, 0.9, size=(M, P))
    else:
        q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    if not whiten:
        Kmm = orc.Kuu(Z, variance=var, lengthscales=ls, jitter=orc.DEFAULT_JITTER)
        Lm = np.linalg.cholesky(Kmm)
        q_mu = Lm @ q_mu
        q_sqrt = q_sqrt / np.sqrt(np.diag(np.linalg.inv(Kmm)))[:, None] if q_diag else np.stack([Lm @ q for q in q_sqrt])
    Y = _labels(lik, rng, (N, P))
    return X, Y, Z, q_mu, q_sqrt


def _likelihood(gp, lik, par):
    L = gp.likelihoods
    return {"bernoulli_probit": lambda: L.Bernoulli(), "poisson_exp": lambda: L.Poisson(binsize=par[0]),
            "student_t": lambda: L.StudentT(scale=par[0], df=par[1])}[lik]()


def _model(gp, lik, par, Z, q_mu, q_sqrt, *, whiten=True, num_data=None, mean=0.2, shared=False, ls=0.9, var=1.3):
    k = gp.kernels.SquaredExponential(variance=var, lengthscales=ls)
    iv = gp.inducing_variables.InducingPoints(Z.copy())
    if shared:
        k = gp.kernels.SharedIndependent(k, q_mu.shape[1])
        iv = gp.inducing_variables.SharedIndependentInducingVariables(iv)
    return gp.models.SVGP(k, _likelihood(gp, lik, par), iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), q_diag=q_sqrt.ndim == 2,
                          whiten=whiten, num_data=num_data, mean_function=gp.mean_functions.Constant(mean))


def _oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, *, whiten, mean=0.2, ls=0.9, var=1.3, erfc=_erfc_ld):
    """(sum of the variational expectations, KL): q(f) and the KL from the oracle, the quadrature from `_reference`"""
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=var, lengthscales=ls, whiten=whiten, mean=mean)
    K = None if whiten else orc.Kuu(Z, variance=var, lengthscales=ls, jitter=orc.DEFAULT_JITTER)
    kl = orc.gauss_kl(q_mu, q_sqrt, K)
    ve = _reference(lik, par, Y, fmean, fvar, erfc=erfc)[0][0]
    return float(ve.sum()), float(kl)


@pytest.mark.parametrize("P,shared", [(1, False), (4, True)], ids=["P1", "shared4"])
@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "qdiag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["white", "unwhite"])
@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_svgp_elbo_against_oracle_and_quadrature(gp, lik, par, whiten, q_diag, P, shared):
    """SVGP.elbo through gpk_svgp_elbo_shard_lik in every form of the shard, 1e-8 relative (the project's ELBO bar); the num_data
    scaling; a two-shard split of the rows sums to the one-shard terms."""
    M, N, D = 40, 150, 2
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, M, N, D, P, 11, q_diag, whiten)
    ve, kl = _oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, whiten=whiten)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, whiten=whiten, num_data=5000, shared=shared)
    assert m._fused_config() is not None
    ref = ve * 5000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"elbo {got!r} reference {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
    m.num_data = None
    assert abs(float(m.elbo((X, Y))) - (ve - kl)) <= 1e-8 * abs(ve - kl)
    whole = _np(m.elbo_terms((X, Y)))
    a, b = _np(m.elbo_terms((X[:70], Y[:70]))), _np(m.elbo_terms((X[70:], Y[70:])))
    # the shards regroup the same N P terms (each computed from its own row only): 2 (N P + 2) u sum |term| <= 1e-12 |sum| here
    assert abs(a[0] + b[0] - whole[0]) <= 1e-12 * abs(ve) * 50 and a[1] == whole[1] == b[1]
    assert abs(whole[1] - kl) <= 1e-9 * abs(kl)


def test_svgp_elbo_composed_paths(gp):
    """SeparateIndependent kernels have no fused driver with these likelihoods: the composed path goes through
    likelihood.variational_expectations (the same kernel), whitened and un-whitened."""
    lik, par = LIKS[2]
    M, N, D, P = 30, 90, 2, 2
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, M, N, D, P, 12, False)
    hyp = [(1.3, 0.9), (0.7, 1.4)]
    for whiten in (True, False):
        if not whiten:   # (an un-whitened q of order one for both members: see _svgp_problem)
            Lms = [np.linalg.cholesky(orc.Kuu(Z, variance=v, lengthscales=l, jitter=orc.DEFAULT_JITTER)) for v, l in hyp]
            q_mu = np.stack([Lms[p] @ q_mu[:, p] for p in range(P)], axis=1)
            q_sqrt = np.stack([Lms[p] @ q_sqrt[p] for p in range(P)])
        k = gp.kernels.SeparateIndependent([gp.kernels.SquaredExponential(variance=v, lengthscales=l) for v, l in hyp])
        iv = gp.inducing_variables.SharedIndependentInducingVariables(gp.inducing_variables.InducingPoints(Z.copy()))
        m = gp.models.SVGP(k, _likelihood(gp, lik, par), iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), whiten=whiten)
        assert m._fused_config() is None and m._fused_separate_config() is None
        ve = kl = 0.0
        for p, (v, l) in enumerate(hyp):
            a, b = _oracle_terms(lik, par, X, Y[:, p:p + 1], Z, q_mu[:, p:p + 1], q_sqrt[p:p + 1], whiten=whiten, mean=0.0, ls=l, var=v)
            ve, kl = ve + a, kl + b
        assert abs(float(m.elbo((X, Y))) - (ve - kl)) <= 1e-8 * abs(ve - kl)
        with pytest.raises(NotImplementedError):
            m.elbo_and_grad((X, Y))


def test_svgp_elbo_c3_size(gp):
    """Once at the C3 size (M = 1024, B = 8192): the side schedule of the factorisation with the quadrature stage behind it."""
    if not torch.cuda.is_available():
        pytest.skip("full size on the GPU only")
    lik, par = LIKS[0]
    M, N, D = 1024, 8192, 8
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, M, N, D, 1, 13, False)
    ls = float(np.sqrt(D))
    ve, kl = _oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, whiten=True, ls=ls, erfc=_erfc_f64)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, num_data=100000, ls=ls)
    ref = ve * 100000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"C3 elbo {got!r} reference {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)


@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_predict_y_and_log_density(gp, lik, par):
    """predict_y / predict_log_density through the class methods, against the same integrals of the oracle's q(f) in longdouble
    (Bernoulli: its closed forms).  1e-8 absolute on O(1) quantities, the bar of the predict_f tests next door (1e-9) times the
    sensitivity of these smooth maps, which stays below 10 here."""
    M, N, D, P = 40, 60, 2, 2
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, M, N, D, P, 14, False)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, shared=True)
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=1.3, lengthscales=0.9, mean=0.2)
    mu, v = fmean.astype(LD), fvar.astype(LD)
    x, wn = GH_X.astype(LD), GH_W.astype(LD) / np.sqrt(PI)
    f = mu[..., None] + np.sqrt(2 * v)[..., None] * x
    y = Y[..., None]
    if lik == "bernoulli_probit":
        p = _erfc_ld(-(mu / np.sqrt(1 + v)) / np.sqrt(LD(2))) / 2 * (LD(1) - 2 * LD("1e-3")) + LD("1e-3")
        E, V, lden = p, p - p * p, np.log(np.where(Y == 1, p, 1 - p)).sum(1)
    else:
        if lik == "poisson_exp":
            cm = cv = np.exp(f) * LD(par[0])
            lp = y * (f + np.log(LD(par[0]))) - cm - _lgamma_ld(Y + 1)[..., None]
        else:
            s, df = LD(par[0]), LD(par[1])
            cm, cv = f, np.full(f.shape, s * s * df / (df - 2))
            lg = _lgamma_ld(np.array([(df + 1) / 2, df / 2]))
            lp = lg[0] - lg[1] - (np.log(s * s) + np.log(df) + np.log(PI)) / 2 - (df + 1) / 2 * np.log1p(((y - f) / s) ** 2 / df)
        E = (cm * wn).sum(-1)
        V = ((cv + cm * cm) * wn).sum(-1) - E * E
        t = np.log(wn) + lp
        top = t.max(-1, keepdims=True)
        lden = (top[..., 0] + np.log(np.exp(t - top).sum(-1))).sum(1)
    gE, gV = m.predict_y(X)
    gl = m.predict_log_density((X, Y))
    assert gl.shape == (N,)
    for name, got, ref in (("E_y", gE, E), ("V_y", gV, V), ("log density", gl, lden)):
        err = float(np.abs(_np(got).astype(LD) - ref).max() / max(1.0, float(np.abs(ref).max())))
        print(f"{lik} predict {name}: max error {err:.3g}")
        assert err <= 1e-8, name


# ------------------------------------------------------------------------------------------------ 5. gradients
def _torch_elbo(lik, X, Y, Z, q_mu, q_sqrt, variance, ls, mean, par, *, num_data, jitter=1e-6):
    """The whitened ELBO with a quadrature likelihood on torch-CPU fp64 tensors, for autograd: the conditional and the KL as
    oracle/gp_oracle_grad.svgp_elbo_torch writes them, the 20-node sum of log p(y | f_h) in place of the Gaussian term."""
    M, B = Z.shape[0], X.shape[0]
    Kmm = orcg._rbf(Z, Z, variance, ls) + jitter * torch.eye(M, dtype=torch.float64)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kmm), orcg._rbf(Z, X, variance, ls), upper=False)
    fvar = variance - (A * A).sum(0)
    fmean = A.T @ q_mu + mean
    P = q_mu.shape[1]
    if q_sqrt.dim() == 2:
        LTA = A[None, :, :] * q_sqrt.T[:, :, None]
        kl = 0.5 * ((q_mu * q_mu).sum() - M * P - torch.log(q_sqrt ** 2).sum() + (q_sqrt ** 2).sum())
    else:
        Lq = torch.tril(q_sqrt)
        LTA = Lq.transpose(1, 2) @ A
        kl = 0.5 * ((q_mu * q_mu).sum() - M * P - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())
    fvar = (fvar[None, :] + (LTA * LTA).sum(1)).T
    if lik == "poisson_exp":
        ve = Y * fmean - torch.exp(fmean + fvar / 2) * par[0] - torch.lgamma(Y + 1) + Y * math.log(par[0])
    else:
        x, wn = torch.tensor(GH_X), torch.tensor(GH_W / np.sqrt(np.pi))
        f = fmean[..., None] + torch.sqrt(2 * fvar)[..., None] * x
        y = Y[..., None]
        if lik == "bernoulli_probit":
            p = 0.5 * (1 + torch.special.erf(f / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3
            g = torch.log(torch.where(y == 1, p, 1 - p))
        else:
            s, df = par
            g = torch.lgamma(torch.tensor((df + 1) / 2, dtype=torch.float64)) - torch.lgamma(torch.tensor(df / 2, dtype=torch.float64)) \
                - 0.5 * (torch.log(s * s) + math.log(df) + math.log(math.pi)) - 0.5 * (df + 1) * torch.log(1 + ((y - f) / s) ** 2 / df)
        ve = (g * wn).sum(-1)
    return ve.sum() * (num_data / B) - kl


def _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, *, variance, ls, mean, num_data):
    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    v = {"Z": t(Z, True), "q_mu": t(q_mu, True), "q_sqrt": t(q_sqrt, True), "variance": t(variance, True),
         "lengthscales": t(np.atleast_1d(ls), True), "mean_const": t(mean, True)}
    tpar = par
    if lik == "student_t":
        v["likelihood_scale"] = t(par[0], True)
        tpar = (v["likelihood_scale"], par[1])
    F = _torch_elbo(lik, t(X), t(Y), v["Z"], v["q_mu"], v["q_sqrt"], v["variance"], v["lengthscales"], v["mean_const"], tpar,
                    num_data=num_data)
    F.backward()
    return float(F.detach()), {k: a.grad.detach().numpy().copy() for k, a in v.items()}


@pytest.mark.parametrize("M,B,D,P,q_diag,ard", [(150, 300, 3, 2, False, True), (64, 200, 2, 1, True, False),
                                                (130, 140, 2, 3, True, True)], ids=["full-P2", "qdiag-P1", "qdiag-P3"])
@pytest.mark.parametrize("lik,par", LIKS, ids=LIK_IDS)
def test_svgp_elbo_and_grad_vs_autograd(gp, lik, par, M, B, D, P, q_diag, ard):
    """gradients.svgp_elbo_and_grad(likelihood=...) against autograd of the restated ELBO, at the tolerances of the whitened case of
    test_gpu_gradients.py: value 1e-9 relative, every gradient 1e-8 of max(1, its largest entry) -- Z, q_sqrt and the StudentT
    scale included."""
    from gpflow_amd import gradients, ops
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, M, B, D, P, 21, q_diag)
    ls = np.sqrt(D) * (0.8 + 0.05 * np.arange(D)) if ard else 1.3
    t = ops.to_device
    q_in = q_sqrt if q_diag else q_sqrt + np.triu(np.ones((M, M)), 1)[None] * 0.37   # junk above the diagonal is ignored
    F, g, info = gradients.svgp_elbo_and_grad(t(Z), t(X), t(Y), t(q_mu), t(q_in), variance=1.3, lengthscales=ls, noise_variance=None,
                                              jitter=1e-6, scale=1000.0 / B, mean_const=0.1, likelihood=(lik, par))
    ops.check_info(info)
    v, go = _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=ls, mean=0.1, num_data=1000)
    print(f"value {float(F.cpu()[0])!r} autograd {v!r}")
    assert abs(float(F.cpu()[0]) - v) <= 1e-9 * abs(v)
    assert "noise_variance" not in g and set(g) == set(go)
    for name, ref in go.items():
        got = _np(g[name]).reshape(ref.shape)
        tol = 1e-8 * max(1.0, np.abs(ref).max())
        print(f"{name}: max error {np.abs(got - ref).max():.3g} tolerance {tol:.3g}")
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=name)


def test_model_elbo_and_grad_and_optimiser(gp):
    """SVGP.elbo_and_grad chains the device gradients through the parameter transforms (value == the fused forward; the StudentT
    scale is among the gradients), and gpflow.optimizers.Scipy raises the ELBO of a Bernoulli classifier on a separable two-class
    toy set monotonically over successive short runs."""
    rng = np.random.default_rng(31)
    lik, par = LIKS[2]
    X, Y, Z, q_mu, q_sqrt = _svgp_problem(lik, 50, 180, 2, 1, 32, False)
    m = _model(gp, lik, par, Z, q_mu, q_sqrt, num_data=2000)
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - float(m.elbo((X, Y)))) <= 1e-9 * abs(v)
    assert m.likelihood.scale in g and m.q_sqrt in g and m.inducing_variable.Z in g and m.mean_function.c in g
    _, go = _autograd(lik, par, X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=0.9, mean=0.2, num_data=2000)
    sc = m.likelihood.scale
    ref = go["likelihood_scale"] * sc.transform.forward_grad(sc.unconstrained_variable)
    np.testing.assert_allclose(np.ravel(g[sc]), np.ravel(ref), rtol=0, atol=1e-8 * max(1.0, abs(float(ref))))
    np.testing.assert_allclose(g[m.inducing_variable.Z], go["Z"], rtol=0, atol=1e-8 * max(1.0, np.abs(go["Z"]).max()))
    # two separable classes
    Xc = np.concatenate([rng.normal(size=(60, 2)) * 0.4 + 1.5, rng.normal(size=(60, 2)) * 0.4 - 1.5])
    Yc = np.concatenate([np.ones((60, 1)), np.zeros((60, 1))])
    Zc = Xc[::6].copy()
    c = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=1.0), gp.likelihoods.Bernoulli(), Zc)
    vals = [float(c.elbo((Xc, Yc)))]
    for _ in range(5):
        gp.optimizers.Scipy().minimize(c, (Xc, Yc), options=dict(maxiter=3))
        vals.append(float(c.elbo((Xc, Yc))))
    print("ELBO per round:", vals)
    assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0] + 10
    p, _ = c.predict_y(Xc)
    assert ((_np(p)[:, 0] > 0.5) == (Yc[:, 0] == 1)).all()
