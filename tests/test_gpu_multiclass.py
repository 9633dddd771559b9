"""GPU tests of the MultiClass likelihood with the RobustMax link: the row-coupled quadrature kernel behind
`ops.likelihood_varexp_sum(lik="multiclass_robustmax")`, the fused shard `ops.svgp_elbo_shard_lik`, the classes `RobustMax` /
`MultiClass`, `SVGP.elbo` / `predict_y` / `predict_log_density` and the reverse pass `SVGP.elbo_and_grad` with this likelihood.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_multiclass_emulated.py imports them without this
module's `gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py, the code being a row of the table of
tests/fake_likelihood_ops.py).

References.  Values: oracle/gp_oracle.py gives q(f) (`svgp_predict_f`) and the KL (`gauss_kl`); the definition of the likelihood
(GPflow 2.9.2 likelihoods/multiclass.py) is restated here in np.longdouble with erfc from mpmath at 40 digits (`_mc_reference`).
Gradients: a torch-CPU fp64 autograd restatement of the same ELBO (`_torch_elbo_mc`).  u = 2^-53 throughout; every bound is
derived next to its check.  Helpers shared with tests/test_gpu_likelihoods.py are imported from there.
"""
import functools
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
from test_gpu_likelihoods import GH_W, GH_X, LD, PI, U, _bits, _erfc_f64, _erfc_ld, _np, _refused, _svgp_problem, _within  # noqa: E402

LIK = "multiclass_robustmax"
EPS = 1e-3


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


# ------------------------------------------------------------------------------------------------ the reference
def _mc_reference(eps, Y, mu, fv, emu=0.0, efv=0.0, erfc=_erfc_ld, erfc_ulp=16):
    """The definition in longdouble: (ve [rows], dmu [rows, C], dvar [rows, C], p [rows]) and a bound on the fp64 error of the
    first three.  Y [rows] integer labels, mu / fv [rows, C] the exact operands; emu, efv: how far an fp64 evaluation of
    mu = fmean + mean_const and fvar = knn - s0 + ssq may sit from them.  Error model of one row, first order in u, in the terms of
    test_gpu_likelihoods._reference (the device library's stated limits: erfc 16 ulp, exp 3, log 3; erfc_ulp is raised where the
    REFERENCE's erfc is itself only fp64):
      * a clamped variance is the constant 1e-10: no operand error; otherwise sqrt(v) carries  4 u + efv / (2 v)  relative ("rs",
        which also covers the rounding of the division by it)
      * the node  X_h = fma(s, x_h, mu_y):  eX = u |X_h| + |x_h| s rs_y + emu_y
      * d_kh = (X_h - mu_k) / sqrt(v_k):  ed = (eX + emu_k + u |X_h - mu_k|) / sqrt(v_k) + |d| rs_k
      * c_kh = erfc(-d / sqrt 2) / 2 * a + 1e-4, a = 1 - 2e-4:  dc = a phi(d) (ed + 2 u |d|)  from its argument, erfc_ulp u of the
        erfc value and 4 u for the arithmetic: relative  rc = (a phi (ed + 2 u |d|) + (erfc_ulp + 4) u c) / c.  The division is
        safe: c >= 1e-4, which is what bounds the factors' relative errors
      * Pi_h = prod_{k != y} c_kh: the relative error of a product of C - 1 factors is the sum of theirs, plus u per
        multiplication:  rP = sum_{k != y} (rc + u)
      * p = sum_h wn_h Pi_h:  sum_h wn Pi rP  +  32 u sum_h wn Pi  (the weighted 20-term sum and its shuffle combination)
      * VE = p l1 + (1 - p) l0:  kappa ep + 8 u (|l1| p + |l0| (1 - p))   (two host logs at 3 ulp, the arithmetic)
      * t_kh = a phi(d) / (sqrt(v_k) c):  exp 3 ulp with an argument error u d^2 (relative of the value) and |d| ed from d itself,
        rc and rs_k from the divisors, the products:  rt = |d| ed + u d^2 + rc + rs_k + 12 u
      * a1_k = sum_h wn Pi t,  a2_k = sum_h wn Pi t d,  a3_k = sum_h wn Pi t x_h:  each term's relative error rP + rt (a2: + ed on d)
        and 32 u sum |term| for the sum;  dmu_k = -kappa a1,  dvar_k = -kappa a2 / (2 sqrt v_k) (division: rs_k more), kappa to 8 u
      * the label's latent sums the others' a1 / a3 in class order:  their bounds add up, (C + 2) u sum |term| for the C-term sum,
        and dvar_y divides by s (rs_y more).
    Where a clamp is active the derivative w.r.t. that variance is exactly 0: bound 0."""
    Y = np.asarray(Y).astype(np.int64)
    mu, fv = np.asarray(mu, dtype=LD), np.asarray(fv, dtype=LD)
    rows, C = mu.shape
    emu = np.broadcast_to(np.asarray(emu, dtype=LD), mu.shape) + U * np.abs(mu)
    efv = np.broadcast_to(np.asarray(efv, dtype=LD), mu.shape)
    on = np.zeros((rows, C), dtype=bool)
    on[np.arange(rows), Y] = True
    x, wn = GH_X.astype(LD), GH_W.astype(LD) / np.sqrt(PI)
    lo = LD("1e-10")
    a = LD(1) - 2 * LD("1e-4")
    mu_y, v_y, emu_y, efv_y = mu[on], fv[on], emu[on], efv[on]
    cy, ck = 2 * v_y < lo, fv < lo
    tv, vk = np.where(cy, lo, 2 * v_y), np.where(ck, lo, fv)
    s, sdk = np.sqrt(tv), np.sqrt(vk)
    rs_y = 4 * U + np.where(cy, 0, efv_y / np.where(cy, 1, v_y) / 2)
    rs_k = 4 * U + np.where(ck, 0, efv / np.where(ck, 1, fv) / 2)
    X = mu_y[:, None] + s[:, None] * x                                                       # [rows, H]
    eX = U * np.abs(X) + np.abs(x) * (s * rs_y)[:, None] + emu_y[:, None]
    diff = X[:, None, :] - mu[:, :, None]                                                    # [rows, C, H]
    d = diff / sdk[:, :, None]
    ed = (eX[:, None, :] + emu[:, :, None] + U * np.abs(diff)) / sdk[:, :, None] + np.abs(d) * rs_k[:, :, None]
    phi = np.exp(-d * d / 2) / np.sqrt(2 * PI)
    c = erfc(-d / np.sqrt(LD(2))) / 2 * a + LD("1e-4")
    rc = (a * phi * (ed + 2 * U * np.abs(d)) + (erfc_ulp + 4) * U * c) / c
    t = a * phi / (sdk[:, :, None] * c)
    rt = np.abs(d) * ed + U * d * d + rc + rs_k[:, :, None] + 12 * U
    off = ~on[:, :, None]
    c, t = np.where(off, c, LD(1)), np.where(off, t, LD(0))
    rP = np.where(off, rc + U, LD(0)).sum(1)                                                 # [rows, H]
    wP = np.prod(c, axis=1) * wn                                                             # [rows, H]
    p = wP.sum(-1)
    ep = (wP * rP).sum(-1) + 32 * U * p
    l1, l0 = np.log1p(-LD(eps)), np.log(LD(eps) / (C - 1))
    kap = l1 - l0
    ve = p * l1 + (1 - p) * l0
    b_ve = kap * ep + 8 * U * (np.abs(l1) * p + np.abs(l0) * (1 - p))
    wPt = wP[:, None, :] * t                                                                 # [rows, C, H]
    rel = rP[:, None, :] + rt
    a1, a2, a3 = wPt.sum(-1), (wPt * d).sum(-1), (wPt * x).sum(-1)
    e1 = (wPt * rel).sum(-1) + 40 * U * a1
    e2 = (wPt * (np.abs(d) * rel + ed)).sum(-1) + 40 * U * (wPt * np.abs(d)).sum(-1)
    m3 = (wPt * np.abs(x)).sum(-1)
    e3 = (wPt * np.abs(x) * rel).sum(-1) + 40 * U * m3
    dmu_k, b_dmu_k = -kap * a1, kap * e1
    dvar_k = -kap * a2 / (2 * sdk)
    b_dvar_k = kap * e2 / (2 * sdk) + np.abs(dvar_k) * rs_k
    dmu_y = kap * a1.sum(1)
    b_dmu_y = kap * e1.sum(1) + (C + 2) * U * np.abs(dmu_y)
    dvar_y = kap * a3.sum(1) / s
    b_dvar_y = kap * (e3.sum(1) + (C + 2) * U * m3.sum(1)) / s + np.abs(dvar_y) * rs_y
    dmu = np.where(on, dmu_y[:, None], dmu_k)
    b_dmu = np.where(on, b_dmu_y[:, None], b_dmu_k)
    dvar = np.where(on, np.where(cy, 0, dvar_y)[:, None], np.where(ck, 0, dvar_k))
    b_dvar = np.where(on, np.where(cy, 0, b_dvar_y)[:, None], np.where(ck, 0, b_dvar_k))
    return (ve, dmu, dvar, p), (b_ve, b_dmu, b_dvar)


def _mc_labels(rng, rows, C):
    """uniform over 0 .. C - 1; whenever rows >= C the first and the last class are made to occur"""
    y = rng.integers(0, C, size=rows).astype(np.float64)
    if rows >= C:
        y[0], y[rows - 1] = 0.0, float(C - 1)
    return y


# ------------------------------------------------------------------------------------------------ 1. the kernel
# (rows, C, per-latent s0 / knn, layout of Y: "c" one contiguous column, "ld" padded with NaN columns to an odd leading dimension)
KERNEL_CASES = [
    (0, 2, False, "c"),        # zero rows: out = [0, 0], nothing else written
    (1, 2, False, "c"),        # one lane group pair
    (67, 3, True, "ld"),       # C does not divide 16: five rows per pass, one idle group; a partial last pass
    (130, 5, False, "c"),      # three rows per pass
    (33, 16, True, "ld"),      # one row per pass; maximum C
    (257, 2, False, "ld"),     # eight rows per pass, more than one block
]
# more passes (4200 rows, one per pass) than 1024 blocks x 4 waves: the grid-stride loop.  1.26M mpmath calls are too slow: the
# reference's erfc is SciPy's fp64 one, and the bound is widened by its error (below).
BIG_CASE = (4200, 16, False, "c")


def _mc_inputs(case):
    rows, C, per, layout = case
    rng = np.random.default_rng(rows * 31 + C)
    Y = _mc_labels(rng, rows, C)
    F = rng.normal(size=(rows, C)) * 1.5
    s0 = rng.uniform(0, 0.5, size=(C, rows) if per else (rows,))
    ssq = rng.uniform(0, 0.6, size=(C, rows))
    knn = list(1.0 + 0.1 * np.arange(C)) if per else [1.2]
    return Y, F, s0, ssq, knn


def _exact_operands(F, s0, ssq, knn, per, mc):
    """(mu, fv) in longdouble and the distance (emu, efv) an fp64 evaluation may sit from them"""
    s0c = (s0.T if per else s0[:, None]).astype(LD)
    knl = np.asarray(knn, dtype=LD)[None, :]
    fv = knl - s0c + ssq.T.astype(LD)
    efv = 2 * U * (np.abs(knl) + np.abs(s0c) + ssq.T)             # two roundings: knn - s0, then + ssq
    mu = F.astype(LD) + LD(mc)
    return mu, fv, U * np.abs(mu), efv


@functools.lru_cache(maxsize=None)
def _case_reference(case):
    """computed once per case and shared (the emulated and the device tier, the contract test's two calls)"""
    rows, C, per, layout = case
    Y, F, s0, ssq, knn = _mc_inputs(case)
    mu, fv, emu, efv = _exact_operands(F, s0, ssq, knn, per, 0.1)
    big = case == BIG_CASE
    # SciPy's erfc (Cephes) states a peak relative error of 1.3e-15 = 12 u over its domain: 16 u more on the erfc value
    main = _mc_reference(EPS, Y, mu, fv, emu=emu, efv=efv, erfc=_erfc_f64 if big else _erfc_ld, erfc_ulp=32 if big else 16)
    plain = _mc_reference(EPS, Y, F.astype(LD), np.full((rows, C), LD(knn[0])), erfc=_erfc_f64 if big else _erfc_ld,
                          erfc_ulp=32 if big else 16) if rows else None
    return main, plain, fv, efv


@pytest.mark.parametrize("case", KERNEL_CASES + [BIG_CASE], ids=str)
def test_multiclass_varexp_sum_contract(gp, case):
    """The contract rules of test_likelihood_varexp_sum_contract for the row-coupled kernel: every output under the bound derived
    in `_mc_reference`, inputs bitwise unchanged, a second call bit-identical, rows = 0 writes [0, 0], out[1] == 0, and the call
    without optional operands and outputs.  Y is ONE column; in the "ld" layout it is followed by NaN columns that must not be
    read (an odd leading dimension)."""
    from gpflow_amd import ops
    rows, C, per, layout = case
    Y, F, s0, ssq, knn = _mc_inputs(case)
    mc = 0.1
    ((ve, dmu, dvar, _), (b_ve, b_dmu, b_dvar)), plain, fv, efv = _case_reference(case)
    Yfull = np.concatenate([Y[:, None], np.full((rows, 2), np.nan)], axis=1) if layout == "ld" else Y[:, None].copy()
    tYf = ops.to_device(Yfull)
    tY = tYf[:, :1]
    tF, ts0, tss = ops.to_device(F), ops.to_device(s0), ops.to_device(ssq)

    def call():
        return ops.likelihood_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, lik=LIK, params=(EPS,), mean_const=mc, s0_per_latent=per,
                                         want_fvar=True, want_rows=True, want_grads=True)
    out, rws, gmu, gvar, fvar = call()
    # the sum over rows: the rows' own bounds + 2 (rows + 2) u sum |VE_b| for the two-stage reduction (each row counts ONCE)
    _within("out[0]", _np(out)[0:1], [ve.sum()], [b_ve.sum() + 2 * (rows + 2) * U * np.abs(ve).sum()])
    assert float(_np(out)[1]) == 0.0
    _within("rows", _np(rws), ve, b_ve)
    _within("dmu", _np(gmu), dmu, b_dmu)
    _within("dvar", _np(gvar), dvar, b_dvar)
    _within("fvar", _np(fvar), fv, efv + LD(1e-300))
    for t, a in ((tYf, Yfull), (tF, F), (ts0, s0), (tss, ssq)):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    again = call()
    for first, second in zip((out, rws, gmu, gvar, fvar), again):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"
    if rows == 0:
        assert _np(out).tolist() == [0.0, 0.0]
    else:   # without the optional operands and outputs: fvar = knn, only the sums
        only = ops.likelihood_varexp_sum(tY, tF, s0=None, ssq=None, knn=[knn[0]], lik=LIK, params=(EPS,))
        assert only[1] is None and only[2] is None and only[3] is None and only[4] is None
        (ve0, _, _, _), (b0, _, _) = plain
        _within("out[0], fvar = knn", _np(only[0])[0:1], [ve0.sum()], [b0.sum() + 2 * (rows + 2) * U * np.abs(ve0).sum()])
        assert float(_np(only[0])[1]) == 0.0


def test_multiclass_clamp(gp):
    """Rows whose fvar -- of the label's latent (rows 0 - 2) and of another latent (rows 3 - 5) -- sits at -0.3, at 0 and at 1e-12
    through the choice of s0: the value is the reference's with the clamp (no NaN from the square root: the reference clamps for
    this likelihood), dvar of the clamped latent is exactly 0.0, every neighbour within its bound, fvar_out unclamped.  Rows
    6 - 8 are ordinary."""
    from gpflow_amd import ops
    rows, C = 9, 3
    rng = np.random.default_rng(77)
    Y = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2], dtype=np.float64)
    F = rng.normal(size=(rows, C)) * 1.5
    ssq = rng.uniform(0.1, 0.6, size=(C, rows))
    knn = [1.0, 1.1, 1.2]
    s0 = rng.uniform(0, 0.5, size=(C, rows))
    clamped = np.zeros((rows, C), dtype=bool)
    for b, target in enumerate([-0.3, 0.0, 1e-12, -0.3, 0.0, 1e-12]):
        k = int(Y[b]) if b < 3 else (int(Y[b]) + 1) % C
        s0[k, b] = knn[k] + ssq[k, b] - target                    # fvar = knn - s0 + ssq = target up to rounding: far below 1e-10
        clamped[b, k] = True
    mu, fv, emu, efv = _exact_operands(F, s0, ssq, knn, True, 0.0)
    assert (np.abs(fv[clamped] - np.tile([-0.3, 0.0, 1e-12], 2)) < 1e-15).all()
    (ve, dmu, dvar, _), (b_ve, b_dmu, b_dvar) = _mc_reference(EPS, Y, mu, fv, emu=emu, efv=efv)
    assert (dvar[clamped] == 0).all() and (b_dvar[clamped] == 0).all()
    out, rws, gmu, gvar, fvar = ops.likelihood_varexp_sum(ops.to_device(Y[:, None]), ops.to_device(F), s0=ops.to_device(s0),
                                                          ssq=ops.to_device(ssq), knn=knn, lik=LIK, params=(EPS,), s0_per_latent=True,
                                                          want_fvar=True, want_rows=True, want_grads=True)
    assert np.isfinite(_np(rws)).all()
    _within("rows", _np(rws), ve, b_ve)
    _within("dmu", _np(gmu), dmu, b_dmu)
    _within("dvar", _np(gvar), dvar, b_dvar)
    assert (_np(gvar)[clamped] == 0.0).all() and (_np(gvar)[~clamped] != 0.0).all()
    _within("fvar", _np(fvar), fv, efv + LD(1e-300))
    _within("out[0]", _np(out)[0:1], [ve.sum()], [b_ve.sum() + 2 * (rows + 2) * U * np.abs(ve).sum()])


def test_multiclass_refusals(gp):
    """One class, seventeen classes, epsilon = 0, epsilon = 1, a missing epsilon: refused on the device and by the emulation, by
    the kernel entry point and by the fused shard."""
    from gpflow_amd import ops

    def call(C, par):
        F = ops.to_device(np.zeros((3, C)))
        return ops.likelihood_varexp_sum(ops.to_device(np.zeros((3, 1))), F, s0=None, ssq=None, knn=[1.0], lik=LIK, params=par)
    assert np.isfinite(_np(call(2, (EPS,))[0])).all()
    for C, par in ((1, (EPS,)), (17, (EPS,)), (3, (0.0,)), (3, (1.0,)), (3, ())):
        with pytest.raises(_refused()):
            call(C, par)
    Z = ops.to_device(np.random.default_rng(0).normal(size=(5, 2)))
    for C, par in ((1, (EPS,)), (17, (EPS,)), (3, (0.0,)), (3, (1.0,)), (3, ())):
        with pytest.raises(_refused()):
            ops.svgp_elbo_shard_lik(Z, Z, ops.to_device(np.zeros((5, 1))), ops.to_device(np.zeros((5, C))),
                                    ops.to_device(np.ones((5, C))), variance=1.0, lengthscales=1.0, lik=LIK, params=par, jitter=1e-6)


@pytest.mark.parametrize("what", ["Y=nan", "fmean=nan", "ssq=nan", "Y=3", "Y=-1", "Y=0.5"])
def test_multiclass_nonfinite_and_bad_labels(gp, what):
    """A NaN planted in Y[17], fmean[17, 1] or ssq[1, 17], or the label 3, -1 or 0.5 in row 17 of a 3-class problem: out[0],
    rows_out[17] and all three entries of dmu[17] and dvar[17] are NaN -- the row is the unit -- and every other row of every output
    is bit-identical to the clean run."""
    from gpflow_amd import ops
    rows, C, b = 41, 3, 17
    Y, F, s0, ssq, knn = _mc_inputs((rows, C, False, "c"))

    def run(Y, F, ssq):
        r = ops.likelihood_varexp_sum(ops.to_device(Y[:, None]), ops.to_device(F), s0=ops.to_device(s0), ssq=ops.to_device(ssq),
                                      knn=knn, lik=LIK, params=(EPS,), want_rows=True, want_grads=True)
        return [_np(t) for t in r[:4]]
    clean = run(Y, F, ssq)
    assert all(np.isfinite(a).all() for a in clean)
    Y2, F2, ssq2 = Y.copy(), F.copy(), ssq.copy()
    where, value = what.split("=")
    value = float(value)
    if where == "Y":
        Y2[b] = value
    elif where == "fmean":
        F2[b, 1] = value
    else:
        ssq2[1, b] = value
    out, rws, gmu, gvar = run(Y2, F2, ssq2)
    assert np.isnan(out[0]) and out[1] == 0.0
    keep = np.ones(rows, dtype=bool); keep[b] = False
    assert np.isnan(rws[b]) and np.array_equal(_bits(rws[keep]), _bits(clean[1][keep]))
    for name, got, ref in (("dmu", gmu, clean[2]), ("dvar", gvar, clean[3])):
        assert np.isnan(got[b]).all(), name
        assert np.array_equal(_bits(got[keep]), _bits(ref[keep])), name


# ------------------------------------------------------------------------------------------------ 2. the method, independently
TWO_CLASS_TRUNCATION = 4.2e-7   # >= the measured 20-node truncation error on the inputs below (docstring)


def test_two_class_closed_form(gp):
    """For C = 2 the integral is closed:  p = (1 - 2e-4) Phi((mu_y - mu_k) / sqrt(v_y + v_k)) + 1e-4,  up to the truncation error
    of 20 nodes -- a property of the method, not of the code under test.  On the 2000 rows below (mu ~ 1.5 N(0, 1), v in
    [0.7, 1.8], seed 5) the longdouble restatement of the 20-node sum differs from the closed form by at most 4.11e-7 (measured
    on the CPU; the worst rows are those with v_y / v_k near its largest, 2.5, and other seeds of the same recipe give 3.2e-7 to
    4.9e-7; fp64 erfc in the 80000 node values, whose 1e-16 does not show at this size).  The test re-measures it, holds it under
    TWO_CLASS_TRUNCATION = 4.2e-7, and allows the device 4 x that, read back through rows_out:  p = (VE - l0) / (l1 - l0)."""
    from gpflow_amd import ops
    rng = np.random.default_rng(5)
    rows = 2000
    mu = 1.5 * rng.normal(size=(rows, 2))
    v = rng.uniform(0.7, 1.8, size=(rows, 2))
    Y = _mc_labels(rng, rows, 2)
    yi = Y.astype(int)
    ar = np.arange(rows)
    z = (mu[ar, yi] - mu[ar, 1 - yi]).astype(LD) / np.sqrt(v.astype(LD).sum(1))
    closed = _erfc_ld(-z / np.sqrt(LD(2))) / 2 * (LD(1) - 2 * LD("1e-4")) + LD("1e-4")
    (_, _, _, p_ref), _ = _mc_reference(EPS, Y, mu, v, erfc=_erfc_f64)
    trunc = float(np.abs(p_ref - closed).max())
    print(f"20-node truncation error, measured: {trunc:.3g}")
    assert trunc <= TWO_CLASS_TRUNCATION
    rws = ops.likelihood_varexp_sum(ops.to_device(Y[:, None]), ops.to_device(mu), s0=None, ssq=ops.to_device(v.T.copy()), knn=[0.0],
                                    lik=LIK, params=(EPS,), want_rows=True)[1]
    l1, l0 = math.log1p(-EPS), math.log(EPS)
    p_dev = (_np(rws) - l0) / (l1 - l0)
    err = float(np.abs(p_dev.astype(LD) - closed).max())
    print(f"device against the closed form: {err:.3g}")
    assert err <= 4 * TWO_CLASS_TRUNCATION


# ------------------------------------------------------------------------------------------------ 3. the classes
def _density_ld(eps, Y, mu, v, erfc=_erfc_ld):
    """_predict_non_logged_density in longdouble: p (1 - eps) + (1 - p) eps / (C - 1)"""
    p = _mc_reference(eps, Y, mu, v, erfc=erfc)[0][3]
    return p * (1 - LD(eps)) + (1 - p) * LD(eps) / (mu.shape[1] - 1)


def test_robustmax_and_class_methods(gp):
    """RobustMax.__call__ / prob_is_largest and MultiClass.log_prob / conditional_mean / conditional_variance /
    variational_expectations / predict_mean_and_var / predict_log_density against the longdouble definition on [60, 4] inputs.
    1e-8 absolute on these O(1) quantities, the bar and the reasoning of test_predict_y_and_log_density (the maps are smooth with
    sensitivities below 10; log of a density >= eps / (C - 1) = 3.3e-4 magnifies 1e-12 to 3e-9).  The rows of the predicted mean
    sum to what the definition gives -- not to 1: the CDF jitter is inside the integrals -- so normalisation is not asserted."""
    from gpflow_amd import ops
    L = gp.likelihoods
    N, C, eps = 60, 4, 0.02
    rng = np.random.default_rng(8)
    mu, v = rng.normal(size=(N, C)) * 1.5, rng.uniform(0.05, 2.0, size=(N, C))
    Y = _mc_labels(rng, N, C)
    link = L.RobustMax(C, epsilon=eps)
    lik = L.MultiClass(C, invlink=link)
    t = ops.to_device
    # the link
    hot = _np(link(t(mu)))
    ref_hot = np.full((N, C), eps / (C - 1)); ref_hot[np.arange(N), mu.argmax(1)] = 1 - eps
    np.testing.assert_allclose(hot, ref_hot, rtol=0, atol=4 * U)
    np.testing.assert_allclose(_np(lik.conditional_mean(None, t(mu))), ref_hot, rtol=0, atol=4 * U)
    np.testing.assert_allclose(_np(lik.conditional_variance(None, t(mu))), ref_hot - ref_hot ** 2, rtol=0, atol=8 * U)
    lp = _np(lik.log_prob(None, t(mu), t(Y[:, None])))
    assert lp.shape == (N,)
    np.testing.assert_allclose(lp, np.where(mu.argmax(1) == Y, np.log(1 - eps), np.log(eps / (C - 1))), rtol=0, atol=8 * U)
    # the integrals
    (ve, _, _, p), _ = _mc_reference(eps, Y, mu, v)
    x, w = ops.gauss_hermite(20)
    got_p = _np(link.prob_is_largest(t(Y[:, None]), t(mu), t(v), x, w))
    assert got_p.shape == (N, 1)
    checks = [("prob_is_largest", got_p[:, 0], p),
              ("variational_expectations", _np(lik.variational_expectations(None, t(mu), t(v), t(Y[:, None]))), ve)]
    E, V = lik.predict_mean_and_var(None, t(mu), t(v))
    ps = np.stack([_density_ld(eps, np.full(N, i), mu, v) for i in range(C)], axis=1)
    checks += [("E_y", _np(E), ps), ("V_y", _np(V), ps - ps * ps),
               ("log density", _np(lik.predict_log_density(None, t(mu), t(v), t(Y[:, None]))), np.log(_density_ld(eps, Y, mu, v)))]
    for name, got, ref in checks:
        assert got.shape == ref.shape, name
        err = float(np.abs(got.astype(LD) - ref).max() / max(1.0, float(np.abs(ref).max())))
        print(f"{name}: max error {err:.3g}")
        assert err <= 1e-8, name
    # leading batch dimensions are flattened and restored
    ve3 = lik.variational_expectations(None, t(mu.reshape(3, 20, C)), t(v.reshape(3, 20, C)), t(Y.reshape(3, 20, 1)))
    assert tuple(ve3.shape) == (3, 20) and np.array_equal(_bits(_np(ve3).reshape(-1)), _bits(checks[1][1]))


# ------------------------------------------------------------------------------------------------ 4. models
def _mc_problem(M, N, D, C, seed, q_diag, whiten=True, ls=0.9, var=1.3):
    """the construction of test_gpu_likelihoods._svgp_problem with one column of class labels"""
    X, _, Z, q_mu, q_sqrt = _svgp_problem("bernoulli_probit", M, N, D, C, seed, q_diag, whiten, ls=ls, var=var)
    Y = _mc_labels(np.random.default_rng(seed + 1000), N, C)[:, None]
    return X, Y, Z, q_mu, q_sqrt


def _mc_model(gp, C, Z, q_mu, q_sqrt, *, whiten=True, num_data=None, mean=0.2, shared=False, ls=0.9, var=1.3, eps=EPS):
    k = gp.kernels.SquaredExponential(variance=var, lengthscales=ls)
    iv = gp.inducing_variables.InducingPoints(Z.copy())
    if shared:
        k = gp.kernels.SharedIndependent(k, C)
        iv = gp.inducing_variables.SharedIndependentInducingVariables(iv)
    lik = gp.likelihoods.MultiClass(C, invlink=gp.likelihoods.RobustMax(C, epsilon=eps))
    return gp.models.SVGP(k, lik, iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), q_diag=q_sqrt.ndim == 2, whiten=whiten, num_data=num_data,
                          mean_function=gp.mean_functions.Constant(mean))


def _mc_oracle_terms(X, Y, Z, q_mu, q_sqrt, *, whiten, mean=0.2, ls=0.9, var=1.3, erfc=_erfc_ld, eps=EPS):
    """(sum of the variational expectations, KL): q(f) and the KL from the oracle, the quadrature from `_mc_reference`"""
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=var, lengthscales=ls, whiten=whiten, mean=mean)
    K = None if whiten else orc.Kuu(Z, variance=var, lengthscales=ls, jitter=orc.DEFAULT_JITTER)
    kl = orc.gauss_kl(q_mu, q_sqrt, K)
    ve = _mc_reference(eps, Y[:, 0], fmean, fvar, erfc=erfc)[0][0]
    return float(ve.sum()), float(kl)


@pytest.mark.parametrize("C,shared", [(3, False), (4, True)], ids=["C3", "shared4"])
@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "qdiag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["white", "unwhite"])
def test_svgp_elbo_multiclass(gp, whiten, q_diag, C, shared):
    """SVGP.elbo through gpk_svgp_elbo_shard_lik in every form of the shard, 1e-8 relative (the project's ELBO bar); the num_data
    scaling; a 70 / 80 split of the rows sums to the one-shard terms (the bound of test_svgp_elbo_against_oracle_and_quadrature);
    the KL is identical across shards."""
    M, N, D = 40, 150, 2
    X, Y, Z, q_mu, q_sqrt = _mc_problem(M, N, D, C, 11, q_diag, whiten)
    ve, kl = _mc_oracle_terms(X, Y, Z, q_mu, q_sqrt, whiten=whiten)
    m = _mc_model(gp, C, Z, q_mu, q_sqrt, whiten=whiten, num_data=5000, shared=shared)
    assert m._fused_config() is not None
    ref = ve * 5000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"elbo {got!r} reference {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
    m.num_data = None
    assert abs(float(m.elbo((X, Y))) - (ve - kl)) <= 1e-8 * abs(ve - kl)
    whole = _np(m.elbo_terms((X, Y)))
    a, b = _np(m.elbo_terms((X[:70], Y[:70]))), _np(m.elbo_terms((X[70:], Y[70:])))
    assert abs(a[0] + b[0] - whole[0]) <= 1e-12 * abs(ve) * 50 and a[1] == whole[1] == b[1]
    assert abs(whole[1] - kl) <= 1e-9 * abs(kl)


def test_svgp_elbo_multiclass_composed_paths(gp):
    """SeparateIndependent kernels have no fused driver with this likelihood: the composed path goes through
    MultiClass.variational_expectations (the same kernel), whitened and un-whitened; elbo_and_grad refuses."""
    M, N, D, C = 30, 90, 2, 3
    X, Y, Z, q_mu0, q_sqrt0 = _mc_problem(M, N, D, C, 12, False)
    hyp = [(1.3, 0.9), (0.7, 1.4), (1.0, 1.1)]
    for whiten in (True, False):
        q_mu, q_sqrt = q_mu0, q_sqrt0
        if not whiten:   # (an un-whitened q of order one for every member: see _svgp_problem)
            Lms = [np.linalg.cholesky(orc.Kuu(Z, variance=v, lengthscales=l, jitter=orc.DEFAULT_JITTER)) for v, l in hyp]
            q_mu = np.stack([Lms[p] @ q_mu0[:, p] for p in range(C)], axis=1)
            q_sqrt = np.stack([Lms[p] @ q_sqrt0[p] for p in range(C)])
        k = gp.kernels.SeparateIndependent([gp.kernels.SquaredExponential(variance=v, lengthscales=l) for v, l in hyp])
        iv = gp.inducing_variables.SharedIndependentInducingVariables(gp.inducing_variables.InducingPoints(Z.copy()))
        m = gp.models.SVGP(k, gp.likelihoods.MultiClass(C), iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), whiten=whiten)
        assert m._fused_config() is None and m._fused_separate_config() is None
        fm, fvs, kl = [], [], 0.0
        for p, (v, l) in enumerate(hyp):
            a, b = orc.svgp_predict_f(X, Z, q_mu[:, p:p + 1], q_sqrt[p:p + 1], variance=v, lengthscales=l, whiten=whiten, mean=0.0)
            fm.append(a[:, 0]); fvs.append(b[:, 0])
            K = None if whiten else orc.Kuu(Z, variance=v, lengthscales=l, jitter=orc.DEFAULT_JITTER)
            kl += float(orc.gauss_kl(q_mu[:, p:p + 1], q_sqrt[p:p + 1], K))
        ve = float(_mc_reference(EPS, Y[:, 0], np.stack(fm, 1), np.stack(fvs, 1))[0][0].sum())
        got = float(m.elbo((X, Y)))
        print(f"whiten={whiten}: elbo {got!r} reference {ve - kl!r}")
        assert abs(got - (ve - kl)) <= 1e-8 * abs(ve - kl)
        with pytest.raises(NotImplementedError):
            m.elbo_and_grad((X, Y))


def test_svgp_elbo_multiclass_at_size(gp):
    """Once at size (M = 1024, N = 8192, D = 8, C = 10; q_diag, whitened, SharedIndependent -- the reference's classification
    recipe): the side schedule of the factorisation with the row-coupled stage behind it.  Reference erfc in fp64 (1.6M values)."""
    if not torch.cuda.is_available():
        pytest.skip("full size on the GPU only")
    M, N, D, C = 1024, 8192, 8, 10
    ls = float(np.sqrt(D))
    X, Y, Z, q_mu, q_sqrt = _mc_problem(M, N, D, C, 13, True, ls=ls)
    ve, kl = _mc_oracle_terms(X, Y, Z, q_mu, q_sqrt, whiten=True, ls=ls, erfc=_erfc_f64)
    m = _mc_model(gp, C, Z, q_mu, q_sqrt, num_data=100000, ls=ls, shared=True)
    assert m._fused_config() is not None
    ref = ve * 100000 / N - kl
    got = float(m.elbo((X, Y)))
    print(f"at size: elbo {got!r} reference {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= 1e-8 * abs(ref)


def test_predict_y_and_log_density_multiclass(gp):
    """SVGP.predict_y / predict_log_density with MultiClass(3) against the same integrals of the oracle's q(f) in longdouble, 1e-8
    absolute (test_predict_y_and_log_density's bar)."""
    M, N, D, C = 40, 60, 2, 3
    X, Y, Z, q_mu, q_sqrt = _mc_problem(M, N, D, C, 14, False)
    m = _mc_model(gp, C, Z, q_mu, q_sqrt, shared=True)
    fmean, fvar = orc.svgp_predict_f(X, Z, q_mu, q_sqrt, variance=1.3, lengthscales=0.9, mean=0.2)
    ps = np.stack([_density_ld(EPS, np.full(N, i), fmean, fvar) for i in range(C)], axis=1)
    lden = np.log(_density_ld(EPS, Y[:, 0], fmean, fvar))
    gE, gV = m.predict_y(X)
    gl = m.predict_log_density((X, Y))
    assert gl.shape == (N,) and gE.shape == (N, C)
    for name, got, ref in (("E_y", gE, ps), ("V_y", gV, ps - ps * ps), ("log density", gl, lden)):
        err = float(np.abs(_np(got).astype(LD) - ref).max() / max(1.0, float(np.abs(ref).max())))
        print(f"predict {name}: max error {err:.3g}")
        assert err <= 1e-8, name


# ------------------------------------------------------------------------------------------------ 5. gradients
def _torch_elbo_mc(X, Y, Z, q_mu, q_sqrt, variance, ls, mean, eps, *, num_data, jitter=1e-6, want_fvar=False):
    """The whitened ELBO with the MultiClass likelihood on torch-CPU fp64 tensors, for autograd: the conditional and the KL as
    test_gpu_likelihoods._torch_elbo writes them; the quadrature of the definition with torch.clamp(min=1e-10), torch.special.erf
    and a one-hot mask for k != y."""
    M, B = Z.shape[0], X.shape[0]
    Kmm = orcg._rbf(Z, Z, variance, ls) + jitter * torch.eye(M, dtype=torch.float64)
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(Kmm), orcg._rbf(Z, X, variance, ls), upper=False)
    fvar = variance - (A * A).sum(0)
    fmean = A.T @ q_mu + mean
    C = q_mu.shape[1]
    if q_sqrt.dim() == 2:
        LTA = A[None, :, :] * q_sqrt.T[:, :, None]
        kl = 0.5 * ((q_mu * q_mu).sum() - M * C - torch.log(q_sqrt ** 2).sum() + (q_sqrt ** 2).sum())
    else:
        Lq = torch.tril(q_sqrt)
        LTA = Lq.transpose(1, 2) @ A
        kl = 0.5 * ((q_mu * q_mu).sum() - M * C - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())
    fvar = (fvar[None, :] + (LTA * LTA).sum(1)).T                                            # [B, C]
    on = torch.nn.functional.one_hot(Y[:, 0].long(), C).to(torch.float64)
    x, wn = torch.tensor(GH_X), torch.tensor(GH_W / np.sqrt(np.pi))
    mu_y, v_y = (on * fmean).sum(1, keepdim=True), (on * fvar).sum(1, keepdim=True)
    Xh = mu_y + torch.sqrt(torch.clamp(2 * v_y, min=1e-10)) * x                              # [B, H]
    d = (Xh[:, None, :] - fmean[:, :, None]) / torch.sqrt(torch.clamp(fvar, min=1e-10))[:, :, None]
    cdf = 0.5 * (1 + torch.special.erf(d / math.sqrt(2.0))) * (1 - 2e-4) + 1e-4
    cdf = cdf * (1 - on)[:, :, None] + on[:, :, None]
    p = (torch.prod(cdf, dim=1) * wn).sum(-1)
    ve = p * math.log1p(-eps) + (1 - p) * math.log(eps / (C - 1))
    F = ve.sum() * (num_data / B) - kl
    return (F, fvar) if want_fvar else F


def _autograd_mc(X, Y, Z, q_mu, q_sqrt, *, variance, ls, mean, num_data, eps=EPS):
    t = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=g)  # noqa: E731
    v = {"Z": t(Z, True), "q_mu": t(q_mu, True), "q_sqrt": t(q_sqrt, True), "variance": t(variance, True),
         "lengthscales": t(np.atleast_1d(ls), True), "mean_const": t(mean, True)}
    F, fvar = _torch_elbo_mc(t(X), t(Y), v["Z"], v["q_mu"], v["q_sqrt"], v["variance"], v["lengthscales"], v["mean_const"], eps,
                             num_data=num_data, want_fvar=True)
    F.backward()
    return float(F.detach()), {k: a.grad.detach().numpy().copy() for k, a in v.items()}, fvar.detach().numpy()


@pytest.mark.parametrize("M,B,D,C,q_diag,ard", [(150, 300, 3, 3, False, True), (64, 200, 2, 2, True, False),
                                                (130, 140, 2, 5, True, True)], ids=["full-C3", "qdiag-C2", "qdiag-C5"])
def test_svgp_elbo_and_grad_multiclass_vs_autograd(gp, M, B, D, C, q_diag, ard):
    """gradients.svgp_elbo_and_grad(likelihood=("multiclass_robustmax", (eps,))) with a ONE-column Yb against autograd of the
    restated ELBO, at the tolerances of test_svgp_elbo_and_grad_vs_autograd: value 1e-9 relative, every gradient 1e-8 of max(1, its
    largest entry).  No variance of the reference sits within 1e-6 of a clamp (asserted), so the derivative is smooth there."""
    from gpflow_amd import gradients, ops
    X, Y, Z, q_mu, q_sqrt = _mc_problem(M, B, D, C, 21, q_diag)
    ls = np.sqrt(D) * (0.8 + 0.05 * np.arange(D)) if ard else 1.3
    t = ops.to_device
    q_in = q_sqrt if q_diag else q_sqrt + np.triu(np.ones((M, M)), 1)[None] * 0.37   # junk above the diagonal is ignored
    F, g, info = gradients.svgp_elbo_and_grad(t(Z), t(X), t(Y), t(q_mu), t(q_in), variance=1.3, lengthscales=ls, noise_variance=None,
                                              jitter=1e-6, scale=1000.0 / B, mean_const=0.1, likelihood=(LIK, (EPS,)))
    ops.check_info(info)
    v, go, fvar = _autograd_mc(X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=ls, mean=0.1, num_data=1000)
    assert (np.abs(fvar - 1e-10) > 1e-6).all() and (np.abs(2 * fvar - 1e-10) > 1e-6).all()
    print(f"value {float(F.cpu()[0])!r} autograd {v!r}")
    assert abs(float(F.cpu()[0]) - v) <= 1e-9 * abs(v)
    assert "noise_variance" not in g and set(g) == set(go)
    for name, ref in go.items():
        got = _np(g[name]).reshape(ref.shape)
        tol = 1e-8 * max(1.0, np.abs(ref).max())
        print(f"{name}: max error {np.abs(got - ref).max():.3g} tolerance {tol:.3g}")
        np.testing.assert_allclose(got, ref, rtol=0, atol=tol, err_msg=name)


def test_model_elbo_and_grad_and_optimiser_multiclass(gp):
    """SVGP.elbo_and_grad on a MultiClass(3) model: its value equals elbo (1e-9), the Z gradient matches autograd (1e-8), epsilon
    has no gradient entry; gpflow.optimizers.Scipy raises the ELBO of a classifier on three separable Gaussian blobs (60 points
    each, M = 18) monotonically over successive short runs, after which argmax predict_y recovers every training label."""
    rng = np.random.default_rng(31)
    C = 3
    X, Y, Z, q_mu, q_sqrt = _mc_problem(50, 180, 2, C, 32, False)
    m = _mc_model(gp, C, Z, q_mu, q_sqrt, num_data=2000)
    assert m.likelihood.parameters == ()
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - float(m.elbo((X, Y)))) <= 1e-9 * abs(v)
    assert m.q_sqrt in g and m.q_mu in g and m.inducing_variable.Z in g and m.mean_function.c in g
    assert len(g) == len(m.trainable_parameters)
    _, go, _ = _autograd_mc(X, Y, Z, q_mu, q_sqrt, variance=1.3, ls=0.9, mean=0.2, num_data=2000)
    np.testing.assert_allclose(g[m.inducing_variable.Z], go["Z"], rtol=0, atol=1e-8 * max(1.0, np.abs(go["Z"]).max()))
    # three separable blobs
    centres = np.array([[2.0, 0.0], [-1.0, 1.8], [-1.0, -1.8]])
    Xc = np.concatenate([rng.normal(size=(60, 2)) * 0.3 + c for c in centres])
    Yc = np.repeat(np.arange(3.0), 60)[:, None]
    Zc = Xc[::10].copy()
    assert Zc.shape[0] == 18
    c = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=1.0), gp.likelihoods.MultiClass(3), Zc, num_latent_gps=3,
                       q_diag=True, whiten=True)
    vals = [float(c.elbo((Xc, Yc)))]
    for _ in range(5):
        gp.optimizers.Scipy().minimize(c, (Xc, Yc), options=dict(maxiter=3))
        vals.append(float(c.elbo((Xc, Yc))))
    print("ELBO per round:", vals)
    assert all(b >= a for a, b in zip(vals, vals[1:])) and vals[-1] > vals[0] + 10
    p, _ = c.predict_y(Xc)
    assert (np.argmax(_np(p), axis=1) == Yc[:, 0]).all()
