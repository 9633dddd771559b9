"""GPU tests of the variational-expectation stages (gpflow_amd/csrc/varexp.hip) at EXTREME arguments: the regimes a model in training
reaches and the tables of tests/test_gpu_likelihoods.py, test_gpu_likelihood_zoo.py, test_gpu_multiclass.py, test_gpu_contract.py and
test_gpu_lcm.py never enter -- |mean| up to 37, variances from 1e-12 to 400 (exactly 0 too), labels and parameters at the ends of
their ranges, the two 1e-10 clamps of MultiClass at their boundaries, noise from 1e-12 to 1e12.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_likelihood_edges_emulated.py).

References: the existing ones, imported and not copied -- test_gpu_likelihoods._reference, test_gpu_likelihood_zoo._reference,
test_gpu_multiclass._mc_reference (np.longdouble with erfc / loggamma / digamma from mpmath), the Gaussian sum of
test_gpu_contract.test_gaussian_varexp_sum_contract and test_gpu_lcm._mixed_reference -- with the bounds they derive.  One thing is
added to those bounds here: the underflow FLOOR.  Where a result is subnormal a relative bound underflows to 0, while an operation
whose result is subnormal errs by up to 2^-1075 instead of u relative; fewer than 2^15 such operations feed one element, so every
per-element bound gets 2^-1060 and every sum's bound that once per term.  The bound of every tabled element is asserted finite and
positive before it is used, and no element is left out of a comparison.

Variances reach the kernel in the two ways a caller produces them: exactly (knn = [0.0], s0 = None, ssq = fvar: efv = 0) and by
cancellation as test_multiclass_clamp does it (knn = 1.2, s0 = knn + ssq - target, efv = 2 u (|knn| + |s0| + ssq)) -- the second for
targets >= 1e-9 only, so that efv / (2 fvar) <= 5e-7 and the first-order error model of the references stays valid (asserted).

Shapes: a table has at most ~120 elements and runs with P = 1 (sixteen rows per wave pass) and with P = 3 (five rows per pass, one idle
lane group, a partial last pass; the table rolled by a third per column so that every regime meets every group position; the labels
in a view with an odd leading dimension).  The reference of a table is computed once (functools.lru_cache) and shared.
"""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_lcm as LCM  # noqa: E402  (the mixed stage's reference)
import test_gpu_likelihood_zoo as Z  # noqa: E402  (reference and model helpers)
import test_gpu_likelihoods as T  # noqa: E402  (reference and model helpers)
import test_gpu_multiclass as MC  # noqa: E402  (reference)
from test_gpu_contract import _sum_bound  # noqa: E402

U, LD = T.U, T.LD
_np, _bits = T._np, T._bits
FLOOR = LD(2) ** -1060
MU_GRID = (0.0, 4.0, -4.0, 8.0, -8.0, 12.0, -12.0, 20.0, -20.0, 37.0, -37.0)
FV_GRID = (1e-12, 1e-9, 1e-6, 1e-3, 1.0, 25.0, 100.0, 400.0)     # at +-37 with 400 the nodes reach |f| = 190: erfc and exp(-f^2 / 2) are 0
OLD = ("bernoulli_probit", "poisson_exp", "student_t")            # the codes whose reference is test_gpu_likelihoods._reference
CLOSED = ("poisson_exp",) + Z.CLOSED
NO_PARAM_GRAD = ("bernoulli_probit", "poisson_exp", "exponential_exp")
QMU_FACTOR = 6.0    # test_edges_svgp_elbo_saturated: the fp64 oracle holds the 1e-8 bar at this factor for all seven codes


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _reference(lik, *a, **kw):
    return (T._reference if lik in OLD else Z._reference)(lik, *a, **kw)


def _under(name, got, ref, bound, terms=1, positive=True):
    """|got - ref| <= bound + terms * FLOOR for EVERY entry, after asserting that the reference is finite and the bound finite and
    positive (a bound of exactly 0 only where the reference is exactly 0, or with positive=False where equality is the claim)."""
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
    assert np.isfinite(ref).all(), f"{name}: the reference is not finite"
    assert np.isfinite(bound).all() and (bound >= 0).all(), f"{name}: {int((~(np.isfinite(bound) & (bound >= 0))).sum())} bounds are not finite"
    if positive:
        assert (bound[ref != 0] > 0).all(), f"{name}: a bound is 0"
    bound = bound + terms * FLOOR
    err = np.abs(got.astype(LD) - ref)
    if err.size:
        ratio = np.where(np.isnan(err), np.inf, err / bound).reshape(-1)
        worst = int(np.argmax(ratio))
        print(f"{name}: max error / bound = {float(ratio[worst]):.3g} (error {float(err.reshape(-1)[worst]):.3g})")
    bad = ~(err <= bound)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} entries over the bound; first at flat index {int(np.argmax(bad.reshape(-1)))}"


# ------------------------------------------------------------------------------------------------ 1. the regime tables, scalar codes
YPOS = (5e-324, 1e-300, 1.0, 1e3, 1e300)
YBETA = (0.0, 1e-6, float(np.nextafter(1e-6, 1.0)), 0.5, 1.0 - 1e-6, 1.0)
# id -> (code, params, labels).  A NEW CODE BRINGS ITS ROWS HERE along with its row in LIKS of its own file (NEXT.md).
TABLES = {
    "bernoulli": ("bernoulli_probit", (), (1.0, 0.0, 0.5, -1.0, 2.0)),     # 0.5, -1, 2: no labels; `y == 1 ? p : 1 - p` reads class 0
    "poisson-0.7": ("poisson_exp", (0.7,), (0.0, 1.0, 1e6, 1e15)),
    "poisson-1e-6": ("poisson_exp", (1e-6,), (0.0, 1.0, 1e6, 1e15)),
    "poisson-1e6": ("poisson_exp", (1e6,), (0.0, 1.0, 1e6, 1e15)),
    "exponential": ("exponential_exp", (), YPOS),
    "gamma-1.7": ("gamma_exp", (1.7,), YPOS),
    "gamma-1.0": ("gamma_exp", (1.0,), YPOS),                               # (shape - 1) log y is a 0 * log
    "student-0.8-3": ("student_t", (0.8, 3.0), (0.0, 1e3, -1e3)),
    "student-1e-3-3": ("student_t", (1e-3, 3.0), (0.0, 1e3, -1e3)),
    "student-1e4-3": ("student_t", (1e4, 3.0), (0.0, 1e3, -1e3)),
    "student-0.8-0.5": ("student_t", (0.8, 0.5), (0.0, 1e3, -1e3)),
    "student-0.8-1e6": ("student_t", (0.8, 1e6), (0.0, 1e3, -1e3)),
    "beta-2.5": ("beta_probit", (2.5,), YBETA),
    "beta-0.05": ("beta_probit", (0.05,), YBETA),                           # alpha, beta down to 5e-5
    "beta-400": ("beta_probit", (400.0,), YBETA),
    "ordinal1-1e-3": ("ordinal", (1e-3, 1.0, 0.0), (0.0, 1.0)),
    "ordinal1-0.6": ("ordinal", (0.6, 1.0, 0.0), (0.0, 1.0)),
    "ordinal1-1e3": ("ordinal", (1e3, 1.0, 0.0), (0.0, 1.0)),
    "ordinal5": ("ordinal", (0.6, 5.0) + Z.EDGES5, (0.0, 2.0, 5.0)),        # both open bins and a middle one; at mu = +-37 the
    "ordinal15": ("ordinal", (1.3, 15.0) + Z.EDGES15, (0.0, 7.0, 15.0)),    # bin is many sigma away: D underflows, g -> log 1e-6
    "ordinal-narrow": ("ordinal", (0.6, 2.0, 0.0, 1e-9), (0.0, 1.0, 2.0)),
}
MODES = [("P1", 1, False), ("P3", 3, False), ("P1-cancel", 1, True), ("P3-cancel", 3, True)]


def _admitted(lik, y, mu, fv):
    """the part of the grid a code's table keeps: the closed forms stay below the overflow of their exp (that is
    test_edges_closed_form_overflow_and_gamma_zero_label)"""
    if lik == "poisson_exp":
        return mu + fv / 2 <= 700
    if lik in Z.CLOSED:
        with np.errstate(over="ignore"):
            return -mu + fv / 2 <= 600 and bool(np.isfinite(y * np.exp(-mu + fv / 2)))
    return True


def _elements(tid):
    """the 88 grid points (mu, fvar) of a table, each with one label: label (i + j) mod n at grid point (i, j), or the next one
    the code admits there, so that every label meets every mean and every variance"""
    lik, par, labels = TABLES[tid]
    y, mu, fv = [], [], []
    for i, m in enumerate(MU_GRID):
        for j, v in enumerate(FV_GRID):
            for t in range(len(labels)):
                lab = labels[(i + j + t) % len(labels)]
                if _admitted(lik, lab, m, v):
                    y.append(lab); mu.append(m); fv.append(v)
                    break
    return np.array(y), np.array(mu), np.array(fv)


@functools.lru_cache(maxsize=None)
def _table_reference(tid, cancel):
    """(labels, means, s0 | None, ssq, knn, exact fvar, efv, values, bounds) of a table's elements; computed once per (table, way the
    variance arrives) and shared by the tests and the two tiers"""
    lik, par, _ = TABLES[tid]
    y, mu, target = _elements(tid)
    if cancel:
        keep = target >= 1e-9
        y, mu, target = y[keep], mu[keep], target[keep]
        knn = 1.2
        ssq = target + 0.3
        s0 = knn + ssq - target
        fv = LD(knn) - s0.astype(LD) + ssq.astype(LD)
        efv = 2 * U * (abs(LD(knn)) + np.abs(s0).astype(LD) + ssq.astype(LD))      # two roundings: knn - s0, then + ssq
        assert (np.abs(fv - target) <= efv).all() and (efv / (2 * fv) <= 5e-7).all()
    else:
        knn, s0, ssq = 0.0, None, target
        fv, efv = target.astype(LD), np.zeros(target.shape, dtype=LD)
    vals, bounds = _reference(lik, par, y, mu.astype(LD), fv, emu=0.0, efv=efv)
    return y, mu, s0, ssq, knn, fv, efv, vals, bounds


@pytest.mark.parametrize("mode,P,cancel", MODES, ids=[m[0] for m in MODES])
@pytest.mark.parametrize("tid", list(TABLES))
def test_edges_scalar_regime_tables(gp, tid, mode, P, cancel):
    """Every output of a scalar code under its derived bound (+ the floor) on the table's whole grid, fvar_out against efv (exact
    variances: to the bit), inputs bitwise unchanged, a second call bit-identical."""
    from gpflow_amd import ops
    lik, par, _ = TABLES[tid]
    y, mu, s0, ssq, knn, fv, efv, (ve, dmu, dvar, dth), (b_ve, b_dmu, b_dvar, b_dth) = _table_reference(tid, cancel)
    n = y.size
    assert 60 <= n <= 120
    idx = np.stack([np.roll(np.arange(n), p * (n // 3)) for p in range(P)], axis=1)     # [rows, P]: element of (row, latent)
    Y, F = y[idx], np.ascontiguousarray(mu[idx])
    Yfull = np.concatenate([Y, np.full((n, 2 if P % 2 else 1), np.nan)], axis=1) if P > 1 else Y.copy()   # P = 3: ld = 5
    SS = np.ascontiguousarray(ssq[idx].T)
    S0 = None if s0 is None else np.ascontiguousarray(s0[idx].T)
    tYf, tF, tss = ops.to_device(Yfull), ops.to_device(F), ops.to_device(SS)
    ts0 = None if S0 is None else ops.to_device(S0)
    tY = tYf[:, :P]

    def call():
        return ops.likelihood_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=[knn], lik=lik, params=par, mean_const=0.0,
                                         s0_per_latent=S0 is not None, want_fvar=True, want_rows=True, want_grads=True)
    out, rws, gmu, gvar, fvar = call()
    tag = f"{tid} {mode}"
    ne = n * P     # sums: the terms' own bounds + 2 (ne + 2) u sum |term| for the two-stage reduction, the floor once per term
    _under(f"{tag} out[0]", _np(out)[0:1], [ve[idx].sum()], [b_ve[idx].sum() + 2 * (ne + 2) * U * np.abs(ve[idx]).sum()], terms=ne)
    if lik in NO_PARAM_GRAD:
        assert float(_np(out)[1]) == 0.0
    else:
        _under(f"{tag} out[1]", _np(out)[1:2], [dth[idx].sum()], [b_dth[idx].sum() + 2 * (ne + 2) * U * np.abs(dth[idx]).sum()], terms=ne)
    _under(f"{tag} rows", _np(rws), ve[idx].sum(1), b_ve[idx].sum(1) + 2 * (P + 2) * U * np.abs(ve[idx]).sum(1), terms=P)
    _under(f"{tag} dmu", _np(gmu), dmu[idx], b_dmu[idx])
    _under(f"{tag} dvar", _np(gvar), dvar[idx], b_dvar[idx])
    _under(f"{tag} fvar", _np(fvar), fv[idx], efv[idx], positive=cancel)
    for t, a in ((tYf, Yfull), (tF, F), (tss, SS)) + (() if S0 is None else ((ts0, S0),)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    again = call()
    for first, second in zip((out, rws, gmu, gvar, fvar), again):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"


# ------------------------------------------------------------------------------------------------ 2. MultiClass
MC_SPREAD = (0.0, 4.0, 12.0, 30.0)
# the first four straddle the two different clamps, 2 v < 1e-10 (the label's latent) and v < 1e-10 (any other), with both boundaries
# exactly: 2 * 0.5e-10 == 1e-10 in fp64 (a doubling is exact), and 1e-10 itself
MC_VARS = (0.4e-10, 0.5e-10, 0.7e-10, 1e-10, 1e-6, 1.0, 100.0)


def _mc_table(C):
    """rows: spread of the means x the one odd variance x (on the label's latent | on the next one) x label (first | last class)"""
    Y, mu, fv, clamped = [], [], [], []
    for s in MC_SPREAD:
        for v in MC_VARS:
            for other in (0, 1):
                for lab in (0, C - 1):
                    k = (lab + other) % C
                    f = np.ones(C)
                    f[k] = v
                    c = np.zeros(C, dtype=bool)
                    c[k] = (v < 1e-10) if other else (2.0 * v < 1e-10)
                    Y.append(float(lab)); mu.append(np.linspace(-s, s, C)); fv.append(f); clamped.append(c)
    return np.array(Y), np.array(mu), np.array(fv), np.array(clamped)


@functools.lru_cache(maxsize=None)
def _mc_table_reference(C):
    Y, mu, fv, clamped = _mc_table(C)
    return MC._mc_reference(MC.EPS, Y, mu.astype(LD), fv.astype(LD), emu=0.0, efv=0.0)


@pytest.mark.parametrize("C", [2, 3, 16])
def test_edges_multiclass_regime_table(gp, C):
    """lik_multiclass_kernel with eight, five and one row per wave pass: every output under the bound of `_mc_reference` (+ the
    floor: dmu and dvar are subnormal or 0 where phi(d) underflows), dvar of a clamped variance == 0.0 exactly and of no other,
    fvar_out the UNCLAMPED variance to the bit; the label column sits in a view with an odd leading dimension."""
    from gpflow_amd import ops
    Y, mu, fv, clamped = _mc_table(C)
    rows = Y.size
    assert rows <= 120 and int(clamped.sum()) == 4 * 2 * (1 + 3)     # per spread and label: 0.4e-10 on the label's latent, three on the other
    (ve, dmu, dvar, _), (b_ve, b_dmu, b_dvar) = _mc_table_reference(C)
    assert (dvar[clamped] == 0).all() and (b_dvar[clamped] == 0).all(), "the reference clamps where the fp64 comparison does"
    Yfull = np.concatenate([Y[:, None], np.full((rows, 2), np.nan)], axis=1)
    SS = np.ascontiguousarray(fv.T)
    tYf, tF, tss = ops.to_device(Yfull), ops.to_device(mu), ops.to_device(SS)
    tY = tYf[:, :1]

    def call():
        return ops.likelihood_varexp_sum(tY, tF, s0=None, ssq=tss, knn=[0.0], lik=MC.LIK, params=(MC.EPS,), want_fvar=True,
                                         want_rows=True, want_grads=True)
    out, rws, gmu, gvar, fvar = call()
    tag = f"multiclass C={C}"
    _under(f"{tag} out[0]", _np(out)[0:1], [ve.sum()], [b_ve.sum() + 2 * (rows + 2) * U * np.abs(ve).sum()], terms=rows)
    assert float(_np(out)[1]) == 0.0
    _under(f"{tag} rows", _np(rws), ve, b_ve)
    _under(f"{tag} dmu", _np(gmu), dmu, b_dmu)
    _under(f"{tag} dvar", _np(gvar), dvar, b_dvar)
    assert (_np(gvar)[clamped] == 0.0).all(), "dvar of a clamped variance is exactly 0"
    live = ~clamped & (np.abs(dvar) > 2 * (b_dvar + FLOOR))     # (elsewhere 0 is within the bound: phi(d) underflows)
    assert (_np(gvar)[live] != 0.0).all(), "dvar of an unclamped variance was zeroed"
    on = np.arange(C)[None, :] == Y[:, None]
    edge = on & (fv == 0.5e-10)     # 2 v == 1e-10 exactly on the label's latent: a boundary that is NOT clamped; a `<=` shows where
    assert edge.sum() == 2 * len(MC_SPREAD) and live[edge].any()   # dvar is live (two classes with equal means: dp/dv is 0)
    assert np.array_equal(_bits(_np(fvar)), _bits(fv)), "fvar_out is the unclamped variance"
    for t, a in ((tYf, Yfull), (tF, mu), (tss, SS)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    for first, second in zip((out, rws, gmu, gvar, fvar), call()):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"


# ------------------------------------------------------------------------------------------------ 3. the Gaussian and the mixed stage
GAUSS_NOISE = [1e-12, 1.0, 1e12, "rows"]


def _residuals(rng, shape):
    """|Y - f| from 1e-8 to 1e8, both signs"""
    n = int(np.prod(shape))
    return (np.geomspace(1e-8, 1e8, n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0))[rng.permutation(n)].reshape(shape)


@pytest.mark.parametrize("P", [1, 3])
@pytest.mark.parametrize("noise", GAUSS_NOISE, ids=[str(v) for v in GAUSS_NOISE])
def test_edges_gaussian_varexp_sum(gp, noise, P):
    """gpk_gaussian_varexp_sum with the noise variance at 1e-12, 1 and 1e12 and per row over geomspace(1e-8, 1e8), residuals up to
    1e8, variances over FV_GRID: the reference and the bound (relative to sum |term|) of test_gaussian_varexp_sum_contract."""
    from gpflow_amd import ops
    rows = 67
    rng = np.random.default_rng(5 + P)
    F = rng.normal(size=(rows, P))
    Y = F + 0.1 + _residuals(rng, (rows, P))
    fvt = rng.choice(FV_GRID, size=(P, rows))
    knn, ssq = [1.2], fvt + 0.3
    s0 = 1.2 + ssq - fvt                                                                # [P, rows]
    nv = np.geomspace(1e-8, 1e8, rows)[rng.permutation(rows)] if noise == "rows" else noise
    fv = LD(1.2) - s0.T.astype(LD) + ssq.T.astype(LD)
    nvl = np.asarray(nv, dtype=LD)[:, None] if noise == "rows" else LD(nv)
    terms = -0.5 * np.log(2 * np.pi * LD(1)) - 0.5 * np.log(nvl) - 0.5 * ((Y.astype(LD) - F - 0.1) ** 2 + fv) / nvl
    terms = np.broadcast_to(terms, (rows, P))
    Yfull = np.concatenate([Y, np.full((rows, 2 if P % 2 else 1), np.nan)], axis=1)     # an odd leading dimension
    tYf, tF, ts0, tss = ops.to_device(Yfull), ops.to_device(F), ops.to_device(s0), ops.to_device(ssq)
    nvt = ops.to_device(nv) if noise == "rows" else nv

    def call():
        return ops.gaussian_varexp_sum(tYf[:, :P], tF, s0=ts0, ssq=tss, knn=knn, noise_variance=nvt, mean_const=0.1,
                                       s0_per_latent=True, want_fvar=True)
    out, fvar = call()
    tag = f"gaussian noise={noise} P={P}"
    _under(f"{tag} out", _np(out)[0:1], [terms.sum()], [LD(_sum_bound(terms.astype(np.float64), terms.size, 12))], terms=terms.size)
    _under(f"{tag} fvar", _np(fvar), fv, 2 * U * (np.abs(fv) + np.abs(s0.T) + ssq.T))
    for t, a in ((tYf, Yfull), (tF, F), (ts0, s0), (tss, ssq)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    again = call()
    assert np.array_equal(_bits(_np(out)), _bits(_np(again[0]))) and np.array_equal(_bits(_np(fvar)), _bits(_np(again[1])))


@pytest.mark.parametrize("L,P", [(3, 2), (2, 5)])
@pytest.mark.parametrize("noise", [1e-12, 1.0, 1e12])
def test_edges_mixed_gaussian_varexp_sum(gp, noise, L, P):
    """gpk_mixed_gaussian_varexp_sum with W drawn from {0, 1e-8, 1, 1e4} (every value occurs), the noise at 1e-12, 1 and 1e12 and
    residuals up to 1e8: every output under the bound of test_gpu_lcm._mixed_reference."""
    from gpflow_amd import ops
    rows = 41
    rng = np.random.default_rng(100 * L + P)
    gm = rng.normal(size=(rows, L))
    W = rng.permutation(np.array([0.0, 1e-8, 1.0, 1e4, -1.0, -1e4, -1e-8, 1.0, 0.0, 1e4])[:P * L]).reshape(P, L)
    assert set(np.abs(W).ravel()) == {0.0, 1e-8, 1.0, 1e4}
    Y = gm @ W.T + 0.1 + _residuals(rng, (rows, P))
    s0, ssq, knn = rng.uniform(0, 0.5, size=(L, rows)), rng.choice(FV_GRID, size=(L, rows)), list(1.0 + 0.1 * np.arange(L))
    ref = LCM._mixed_reference(Y, gm, W, s0, ssq, knn, noise, 0.1, True)
    Yfull = np.concatenate([Y, np.full((rows, 2 if P % 2 else 1), np.nan)], axis=1)
    tYf, tg, ts0, tss = ops.to_device(Yfull), ops.to_device(gm), ops.to_device(s0), ops.to_device(ssq)

    def call():
        return ops.mixed_gaussian_varexp_sum(tYf[:, :P], tg, W, s0=ts0, ssq=tss, knn=knn, noise_variance=noise, mean_const=0.1,
                                             s0_per_latent=True, want_moments=True, want_grads=True)
    out, fm, fv, dg, dW = call()
    tag = f"mixed noise={noise} L={L} P={P}"
    _under(f"{tag} out", _np(out), ref["out"], ref["eout"], terms=rows * P)
    _under(f"{tag} fmean", _np(fm), ref["f"], ref["ef"])
    _under(f"{tag} fvar", _np(fv), ref["fv"], ref["efv"])
    _under(f"{tag} dgmu", _np(dg), ref["dg"], ref["edg"])
    _under(f"{tag} dW", _np(dW), ref["dW"], ref["edW"], terms=rows)
    for t, a in ((tYf, Yfull), (tg, gm), (ts0, s0), (tss, ssq)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    for first, second in zip((out, fm, fv, dg, dW), call()):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"


# ------------------------------------------------------------------------------------------------ 4. the edge statements of include/gpk.h
EDGE_ROWS, EDGE_P, EDGE_AT = 7, 3, (4, 1)     # the planted element: row 4, latent 1
EDGE_LIKS = [("bernoulli_probit", ()), ("student_t", (0.8, 3.0)), ("beta_probit", (2.5,)), ("ordinal", (0.6, 5.0) + Z.EDGES5),
             ("poisson_exp", (0.7,)), ("exponential_exp", ()), ("gamma_exp", (1.7,))]
EDGE_IDS = [lik for lik, _ in EDGE_LIKS]


def _edge_inputs(lik, par):
    """7 x 3 ordinary elements (fvar = 1 or 0.25, |mu| <= 4) around the one that a test replaces"""
    rng = np.random.default_rng(17)
    F = rng.uniform(-4, 4, size=(EDGE_ROWS, EDGE_P))
    fv = rng.choice([0.25, 1.0], size=(EDGE_ROWS, EDGE_P))
    fv[EDGE_AT] = 1.0
    Y = T._labels(lik, rng, F.shape) if lik in OLD else Z._labels(lik, par, rng, F.shape)
    return Y, F, fv


def _edge_run(ops, lik, par, Y, F, fv):
    r = ops.likelihood_varexp_sum(ops.to_device(Y), ops.to_device(F), s0=None, ssq=ops.to_device(np.ascontiguousarray(fv.T)), knn=[0.0],
                                  lik=lik, params=par, want_rows=True, want_grads=True, want_fvar=True)
    assert np.array_equal(_bits(_np(r[4])), _bits(fv))
    return [_np(t) for t in r[:4]]


def _others_unchanged(got, clean):
    """every element but EDGE_AT (and every row but its row) bit-identical to the clean run"""
    hit = np.zeros((EDGE_ROWS, EDGE_P), dtype=bool); hit[EDGE_AT] = True
    hit_rows = hit.any(1)
    assert np.array_equal(_bits(got[1][~hit_rows]), _bits(clean[1][~hit_rows])), "rows"
    for name, a, b in (("dmu", got[2], clean[2]), ("dvar", got[3], clean[3])):
        assert np.array_equal(_bits(a[~hit]), _bits(b[~hit])), name


@pytest.mark.parametrize("lik,par", EDGE_LIKS, ids=EDGE_IDS)
def test_edges_fvar_exactly_zero(gp, lik, par):
    """fvar == 0 exactly.  Quadrature codes: sd = 0, every node is mu, so VE and dmu are the one-point values g(mu) and g'(mu) --
    within the bound of the model with every sd term dropped, which is `_reference` at fvar = 1e-4000 (longdouble: sd x_h is then
    below an ulp of everything it is added to) -- and dvar = (sum_h w g'(mu) x_h) / 0 is NaN or +-Inf.  Closed forms: finite and in
    bound.  Every other element is bit-identical to the run in which that element has fvar = 1."""
    from gpflow_amd import ops
    Y, F, fv = _edge_inputs(lik, par)
    clean = _edge_run(ops, lik, par, Y, F, fv)
    assert all(np.isfinite(a).all() for a in clean)
    fv0 = fv.copy(); fv0[EDGE_AT] = 0.0
    got = _edge_run(ops, lik, par, Y, F, fv0)
    out, rws, gmu, gvar = got
    _others_unchanged(got, clean)
    fvl = fv0.astype(LD)
    if lik not in CLOSED:
        fvl[EDGE_AT] = LD("1e-4000")
    (ve, dmu, dvar, dth), (b_ve, b_dmu, b_dvar, b_dth) = _reference(lik, par, Y, F.astype(LD), fvl)
    ne = EDGE_ROWS * EDGE_P
    _under(f"{lik} fvar = 0: rows", rws, ve.sum(1), b_ve.sum(1) + 2 * (EDGE_P + 2) * U * np.abs(ve).sum(1), terms=EDGE_P)
    _under(f"{lik} fvar = 0: dmu", gmu, dmu, b_dmu)
    _under(f"{lik} fvar = 0: out[0]", out[0:1], [ve.sum()], [b_ve.sum() + 2 * (ne + 2) * U * np.abs(ve).sum()], terms=ne)
    if lik in NO_PARAM_GRAD:
        assert out[1] == 0.0
    else:
        _under(f"{lik} fvar = 0: out[1]", out[1:2], [dth.sum()], [b_dth.sum() + 2 * (ne + 2) * U * np.abs(dth).sum()], terms=ne)
    if lik in CLOSED:
        _under(f"{lik} fvar = 0: dvar", gvar, dvar, b_dvar)
    else:
        assert not np.isfinite(gvar[EDGE_AT]), gvar[EDGE_AT]
        assert int((~np.isfinite(gvar)).sum()) == 1, "exactly one element is not finite"


def _ieee_closed(lik, par, y, mu, fv):
    """the contract's closed forms (include/gpk.h) in NumPy fp64, in the contract's order: (VE, dmu, dvar, dVE/dtheta)"""
    import scipy.special as sps
    with np.errstate(all="ignore"):
        y, mu, fv = np.float64(y), np.float64(mu), np.float64(fv)
        if lik == "poisson_exp":
            e = np.exp(mu + fv / 2) * par[0]
            return y * mu - e - sps.gammaln(y + 1.0) + y * np.log(par[0]), y - e, -e / 2, np.float64(0.0)
        ye = y * np.exp(-mu + fv / 2)
        if lik == "exponential_exp":
            return -mu - ye, -1.0 + ye, -ye / 2, np.float64(0.0)
        sh = par[0]
        return -sh * mu - sps.gammaln(sh) + (sh - 1.0) * np.log(y) - ye, -sh + ye, -ye / 2, -mu - sps.digamma(sh) + np.log(y)


def _same_class(got, want):
    """NaN with NaN, +-Inf with the same Inf"""
    return bool(np.isnan(got)) if np.isnan(want) else bool(got == want)


NINF, PINF, NAN = -np.inf, np.inf, np.nan
# (code, params, label, mean, variance of the planted element) -> the IEEE class of (VE, dmu, dvar, out[1]); None: finite.
# Overflow inside a closed form: exp(720) = Inf.  Gamma with y = 0: log y as it comes, -Inf, and 0 * -Inf = NaN for shape 1.
IEEE_CASES = [
    (("poisson_exp", (0.7,), 3.0, 700.0, 40.0), (NINF, NINF, NINF, None)),
    (("exponential_exp", (), 1.0, -700.0, 40.0), (NINF, PINF, NINF, None)),
    (("exponential_exp", (), 0.0, -700.0, 40.0), (NAN, NAN, NAN, None)),              # 0 * Inf
    (("gamma_exp", (1.7,), 1.0, -700.0, 40.0), (NINF, PINF, NINF, None)),
    (("gamma_exp", (1.7,), 0.0, -700.0, 40.0), (NAN, NAN, NAN, NINF)),
    (("gamma_exp", (1.0,), 1.0, -700.0, 40.0), (NINF, PINF, NINF, None)),
    (("gamma_exp", (1.0,), 0.0, -700.0, 40.0), (NAN, NAN, NAN, NINF)),
    (("gamma_exp", (1.7,), 0.0, 0.3, 0.5), (NINF, None, None, NINF)),                 # y e = 0 exactly: dmu = -shape, dvar = -0
    (("gamma_exp", (1.0,), 0.0, 0.3, 0.5), (NAN, None, None, NINF)),
]


@pytest.mark.parametrize("case,want", IEEE_CASES, ids=[f"{c[0]}{list(c[1])}-y{c[2]:g}-mu{c[3]:g}" for c, _ in IEEE_CASES])
def test_edges_closed_form_overflow_and_gamma_zero_label(gp, case, want):
    """Poisson with mu + fvar / 2 = 720, Exponential and Gamma with -mu + fvar / 2 = 720 (y = 1 and y = 0), Gamma with y = 0: the
    element's outputs are the IEEE results of the contract's formulas in the contract's order (`_ieee_closed`) -- +-Inf, NaN for
    0 * Inf -- out[0] and out[1] follow, and every other element is bit-identical to the clean run.  The tabled classes are asserted
    against `_ieee_closed` first, and the count of non-finite entries of each output against the table: one or none."""
    from gpflow_amd import ops
    lik, par, y, mu, fvp = case
    Y, F, fv = _edge_inputs(lik, par)
    clean = _edge_run(ops, lik, par, Y, F, fv)
    assert all(np.isfinite(a).all() for a in clean)
    Y[EDGE_AT], F[EDGE_AT], fv[EDGE_AT] = y, mu, fvp
    ieee = _ieee_closed(lik, par, y, mu, fvp)
    for v, w in zip(ieee, want):
        assert np.isfinite(v) if w is None else _same_class(v, w), (ieee, want)
    got = _edge_run(ops, lik, par, Y, F, fv)
    out, rws, gmu, gvar = got
    _others_unchanged(got, clean)
    for name, a, v, w in (("rows", rws[EDGE_AT[0]], ieee[0], want[0]), ("dmu", gmu[EDGE_AT], ieee[1], want[1]),
                          ("dvar", gvar[EDGE_AT], ieee[2], want[2])):
        if w is None:     # y = 0 and a finite e: y e = 0 exactly, so dmu == -shape and dvar == 0 (the y - y added last makes it +0)
            assert a == v, (name, a, v)
        else:
            assert _same_class(a, w), (name, a, w)
    assert _same_class(out[0], want[0]), out
    if want[3] is None:
        assert np.isfinite(out[1]) and (lik == "gamma_exp" or out[1] == 0.0), out
    else:
        assert _same_class(out[1], want[3]), out
    for name, a, w in (("rows", rws, want[0]), ("dmu", gmu, want[1]), ("dvar", gvar, want[2])):
        assert int((~np.isfinite(a)).sum()) == (0 if w is None else 1), name


# ------------------------------------------------------------------------------------------------ 5. one model-level case
SAT_CASES = [(lik, par, False) for lik, par in T.LIKS + Z.MODEL_LIKS] + [(lik, par, True) for lik, par in Z.MODEL_LIKS]
SAT_IDS = [f"{lik}-{'qdiag' if d else 'full'}" for lik, _, d in SAT_CASES]


@pytest.mark.parametrize("lik,par,q_diag", SAT_CASES, ids=SAT_IDS)
def test_edges_svgp_elbo_saturated(gp, lik, par, q_diag):
    """SVGP.elbo with a saturated posterior: the first M data rows ARE the inducing points, q_mu x QMU_FACTOR, q_sqrt x 1e-3, whitened
    -- fvar falls to 1e-6 next to an inducing point, |fmean| reaches 5 -- against the oracle at the project's ELBO bar, 1e-8 |ref|."""
    M, N, D, P = 40, 150, 2, 1
    if lik in OLD:
        X, Y, Zi, q_mu, q_sqrt = T._svgp_problem(lik, M, N, D, P, 11, q_diag, True)
    else:
        X, Y, Zi, q_mu, q_sqrt = Z._problem(lik, par, M, N, D, P, 11, q_diag, True)
    X[:M] = Zi
    q_mu, q_sqrt = q_mu * QMU_FACTOR, q_sqrt * 1e-3
    if lik in OLD:
        ve, kl = T._oracle_terms(lik, par, X, Y, Zi, q_mu, q_sqrt, whiten=True, erfc=T._erfc_f64)
        m = T._model(gp, lik, par, Zi, q_mu, q_sqrt, whiten=True, num_data=5000)
    else:
        ve, kl = Z._oracle_terms(lik, par, X, Y, Zi, q_mu, q_sqrt, whiten=True)
        m = Z._model(gp, lik, par, Zi, q_mu, q_sqrt, whiten=True, num_data=5000)
    assert m._fused_config() is not None
    ref = ve * 5000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"{lik} saturated elbo {got!r} reference {ref!r}: relative error / 1e-8 = {abs(got - ref) / abs(ref) / 1e-8:.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
