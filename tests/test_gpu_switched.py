"""GPU tests of the switched likelihood: the primitive `ops.switched_varexp_sum` (gpk_switched_varexp_sum, one launch that scores every
row by its own task's likelihood), `likelihoods.SwitchedLikelihood`, and the VGP / SVGP routes that carry it, forward and reverse.

The model-level bodies also run in the CPU tier against the NumPy emulation (tests/test_switched_emulated.py imports them without
this module's `gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py with tests/fake_switched_ops.py).

References and bounds.  Per element, the longdouble `_reference` of tests/test_gpu_likelihoods.py (Bernoulli, Poisson, StudentT) and
tests/test_gpu_likelihood_zoo.py (Exponential, Gamma, Beta) with the bound each derives, imported and applied to every row with its
own task's code; for the Gaussian member the closed form in longdouble with a bound derived here (`_gaussian_reference`).  A sum is
held to its terms' bounds plus the 2 (n + 2) u sum |term| those files allow the two-stage reduction.  Gradients of the models:
torch-CPU fp64 autograd of a restated ELBO, at the tolerances of tests/test_gpu_vgp.py and of the zoo's autograd test.
"""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_switched_ops  # noqa: E402
import test_gpu_likelihood_zoo as Z  # noqa: E402  (reference and helpers only)
import test_gpu_likelihoods as T  # noqa: E402  (reference and helpers only)
import test_gpu_vgp as V  # noqa: E402  (restatement, tolerances and helpers only)
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)

U, LD, PI = T.U, T.LD, T.PI
_np, _bits, _within, _refused = T._np, T._bits, T._within, T._refused
_t, _close = V._t, V._close

# the two instantiations of the kernel: LIGHT holds neither Beta nor Poisson (the bodies that call lgamma on the device), HEAVY both
LIGHT = [("gaussian", (0.6,)), ("student_t", (0.8, 3.0)), ("bernoulli_probit", ()), ("exponential_exp", ()), ("gamma_exp", (1.7,))]
HEAVY = [("beta_probit", (2.5,)), ("gaussian", (0.6,)), ("poisson_exp", (0.7,)), ("student_t", (0.8, 3.0)), ("gamma_exp", (1.7,)),
         ("bernoulli_probit", ())]
# the far trip's members: elementary functions only (the other references evaluate erfc / digamma in mpmath, node by node)
BIG = {"light": [("gaussian", (0.6,)), ("exponential_exp", ()), ("gamma_exp", (1.7,))],
       "heavy": [("gaussian", (0.6,)), ("poisson_exp", (0.7,)), ("gamma_exp", (1.7,))]}
TRAINABLE = ("gaussian", "student_t", "gamma_exp", "beta_probit")


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _table(kind, n, big=False):
    base = BIG[kind] if big else (LIGHT if kind == "light" else HEAVY)
    return [base[i % len(base)] for i in range(n)]


# ------------------------------------------------------------------------------------------------ the reference
def _gaussian_reference(par, Y, mu, fv, emu, efv):
    """The Gaussian member in longdouble, (ve, dmu, dvar, dVE/ds2) and a bound on the fp64 error of each, first order in u.
    dy = y - mu carries the operand error emu (+ u |mu| for the addition of mean_const) and one rounding: e_dy = emu + u |mu| + u |dy|.
    q = dy^2 + fvar: 2 |dy| e_dy + efv, and two roundings (none where the compiler contracts them into an fma): + 2 u q.
    c0 = -log(2 pi) / 2 - log(s2) / 2 is formed on the host: log 3 ulp and two roundings, 4 u (|c0| + 1).  Each quotient by s2 and
    each product by 0.5 is one rounding; the final sums one more: 4 u of the sum of the terms' magnitudes covers them."""
    s2 = LD(par[0])
    Y, mu, fv = (np.asarray(a, dtype=LD) for a in (Y, mu, fv))
    dy = Y - mu
    q = dy * dy + fv
    c0 = -np.log(2 * PI) / 2 - np.log(s2) / 2
    e_dy = emu + U * np.abs(mu) + U * np.abs(dy)
    e_q = 2 * np.abs(dy) * e_dy + efv + 2 * U * np.abs(q)
    ve, dmu, dvar = c0 - q / (2 * s2), dy / s2, -1 / (2 * s2) + 0 * mu
    dsc = -1 / (2 * s2) + q / (2 * s2 * s2)
    b_ve = e_q / (2 * s2) + 4 * U * (abs(c0) + 1) + 4 * U * (abs(c0) + np.abs(q) / (2 * s2))
    b_dmu = e_dy / s2 + 2 * U * np.abs(dmu)
    b_dvar = 2 * U * np.abs(dvar)
    b_dsc = e_q / (2 * s2 * s2) + 4 * U * (1 / (2 * s2) + np.abs(q) / (2 * s2 * s2))
    return (ve, dmu, dvar, dsc), (b_ve, b_dmu, b_dvar, b_dsc)


def _member_reference(name, par, Y, mu, fv, emu, efv):
    if name == "gaussian":
        return _gaussian_reference(par, Y, mu, fv, emu, efv)
    if name in ("bernoulli_probit", "poisson_exp", "student_t"):
        return T._reference(name, par, Y, mu, fv, emu=emu, efv=efv)
    return Z._reference(name, par, Y, mu, fv, emu=emu, efv=efv)


def _switched_reference(members, Y, task, mu, fv, emu, efv):
    """row by row with the row's own member: four [rows, P] arrays and their bounds; NaN in the rows without a task"""
    val = [np.full(mu.shape, LD("nan"), dtype=LD) for _ in range(4)]
    bnd = [np.zeros(mu.shape, dtype=LD) for _ in range(4)]
    for t, (name, par) in enumerate(members):
        sel = task == t
        if sel.any():
            v, b = _member_reference(name, par, Y[sel], mu[sel], fv[sel], emu[sel], efv[sel])
            for i in range(4):
                val[i][sel], bnd[i][sel] = v[i], b[i]
    return val, bnd


def _values(name, rng, shape):
    if name in ("gaussian",):
        return rng.normal(size=shape) * 1.5
    if name in ("bernoulli_probit", "poisson_exp", "student_t"):
        return T._labels(name, rng, shape)
    return Z._labels(name, None, rng, shape)


# ------------------------------------------------------------------------------------------------ 1. the contract
# (rows, P, T, arrangement of the tasks, per-latent s0 / knn, layout of Y: "c" contiguous, "ld" NaN columns behind the label that make
#  the leading dimension ODD: P + 1 + (1 if P is odd else 2), i.e. 7, 19 and 3 for the cases below)
CASES = [
    (0, 1, 2, "rr", False, "c"),           # zero rows: out = 0, nothing else written
    (1, 1, 1, "rr", False, "c"),           # one lane group of one wave, one task
    (67, 4, 3, "rr", True, "ld"),          # four rows of different tasks per pass, a partial last pass; per-latent s0 / knn
    (130, 5, 2, "random", False, "c"),     # P = 5 does not divide 16: an idle lane group
    (33, 16, 16, "rr", True, "ld"),        # one row per pass, every row another task, the largest table
    (257, 1, 4, "sorted", False, "ld"),    # uniform waves, boundary waves, more than one block
    (40, 2, 4, "skip2", False, "c"),       # task 2 has no rows: out[3] == 0 exactly
]
BIG_CASE = (70001, 1, 3, "random", False, "c")   # more passes than 1024 blocks x 4 waves: the far trip of the grid-stride loop
_CASE_CACHE = {}


def _arrangement(how, rows, ntasks, rng):
    if how == "rr":
        return np.arange(rows) % ntasks
    if how == "skip2":
        return np.array([0, 1, 3])[np.arange(rows) % 3]
    task = rng.integers(0, ntasks, size=rows)
    return np.sort(task) if how == "sorted" else task


def _case(case, kind):
    """inputs, the longdouble reference and its bounds for one (case, instantiation): computed once, shared, never modified"""
    key = (case, kind)
    if key in _CASE_CACHE:
        return _CASE_CACHE[key]
    rows, P, ntasks, how, per, layout = case
    members = _table(kind, ntasks, big=case == BIG_CASE)
    rng = np.random.default_rng(rows * 31 + P + (7 if kind == "heavy" else 0))
    task = _arrangement(how, rows, ntasks, rng)
    Yv, F = np.zeros((rows, P)), np.zeros((rows, P))
    for t, (name, _) in enumerate(members):
        sel = task == t
        Yv[sel] = _values(name, rng, (int(sel.sum()), P))
        F[sel] = rng.normal(size=(int(sel.sum()), P)) * (0.7 if name in ("poisson_exp", "exponential_exp", "gamma_exp") else 1.5)
    lab = task + rng.uniform(0, 0.9, size=rows)              # truncation toward zero: the fraction is ignored
    pad = np.full((rows, 1 if P % 2 else 2), np.nan) if layout == "ld" else np.zeros((rows, 0))
    Yfull = np.concatenate([Yv, lab[:, None], pad], axis=1)
    s0 = rng.uniform(0, 0.5, size=(P, rows) if per else (rows,))
    ssq = rng.uniform(0, 0.6, size=(P, rows))
    knn = list(1.0 + 0.1 * np.arange(P)) if per else [1.2]
    mc = 0.1
    s0c = (s0.T if per else s0[:, None]).astype(LD)
    knl = np.asarray(knn, dtype=LD)[None, :]
    fv = knl - s0c + ssq.T.astype(LD)
    efv = 2 * U * (np.abs(knl) + np.abs(s0c) + ssq.T)        # two roundings: knn - s0, then + ssq
    mu = F.astype(LD) + LD(mc)
    val, bnd = _switched_reference(members, Yv.astype(LD), task, mu, fv, U * np.abs(mu), efv + 0 * mu)
    out = dict(members=members, task=task, Yfull=Yfull, F=F, s0=s0, ssq=ssq, knn=knn, mc=mc, per=per, P=P, fv=fv, efv=efv,
               val=val, bnd=bnd)
    _CASE_CACHE[key] = out
    return out


def _checks(c, res):
    """[(name, what one call gave, the longdouble reference, the bound)] over every output; the sums carry the summation term of the
    likelihood tests.  The entries of out that the contract makes an exact 0 are asserted here and are not in the list."""
    out, rws, gmu, gvar, fvar = (None if r is None else _np(r) for r in res)
    (ve, dmu, dvar, dth), (b_ve, b_dmu, b_dvar, b_dth) = c["val"], c["bnd"]
    rows, P = ve.shape
    n = rows * P
    checks = [("out[0]", out[0:1], [ve.sum()], [b_ve.sum() + 2 * (n + 2) * U * np.abs(ve).sum()])]
    for t, (name, _) in enumerate(c["members"]):
        sel = c["task"] == t
        nt = int(sel.sum()) * P
        if name not in TRAINABLE or nt == 0:
            assert out[1 + t] == 0.0 and not np.signbit(out[1 + t]), (t, name, out[1 + t])
        else:
            checks.append((f"out[{1 + t}] ({name})", out[1 + t:2 + t], [dth[sel].sum()],
                           [b_dth[sel].sum() + 2 * (nt + 2) * U * np.abs(dth[sel]).sum()]))
    return checks + [("rows", rws, ve.sum(1), b_ve.sum(1) + 2 * (P + 2) * U * np.abs(ve).sum(1)), ("dmu", gmu, dmu, b_dmu),
                     ("dvar", gvar, dvar, b_dvar), ("fvar", fvar, c["fv"], c["efv"] + LD(1e-300))]


def _check_against_reference(tag, c, res):
    """every output of one call under its bound"""
    for name, got, ref, bound in _checks(c, res):
        _within(f"{tag} {name}", got, ref, bound)


@pytest.mark.parametrize("kind", ["light", "heavy"])
@pytest.mark.parametrize("case", CASES + [BIG_CASE], ids=str)
def test_switched_varexp_sum_contract(gp, case, kind):
    """every output under the derived bound, inputs bitwise unchanged, a second call bit-identical, rows = 0 writes zeros, a task
    without rows and a member without a trainable parameter give an exact 0, the call without the optional operands"""
    from gpflow_amd import ops
    c = _case(case, kind)
    rows, P = c["F"].shape
    tYf = ops.to_device(c["Yfull"])
    tY = tYf[:, :P + 1]
    tF, ts0, tss = ops.to_device(c["F"]), ops.to_device(c["s0"]), ops.to_device(c["ssq"])

    def call():
        return ops.switched_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=c["knn"], members=c["members"], mean_const=c["mc"],
                                       s0_per_latent=c["per"], want_fvar=True, want_rows=True, want_grads=True)
    res = call()
    assert tuple(res[0].shape) == (1 + len(c["members"]),)
    _check_against_reference(f"{kind} {case}", c, res)
    for t, a in ((tYf, c["Yfull"]), (tF, c["F"]), (ts0, c["s0"]), (tss, c["ssq"])):
        assert np.array_equal(_bits(_np(t)), _bits(a)), "an input was modified"
    for first, second in zip(res, call()):
        assert np.array_equal(_bits(_np(first)), _bits(_np(second))), "a second identical call differs"
    if rows == 0:
        assert _np(res[0]).tolist() == [0.0] * (1 + len(c["members"]))
        return
    only = ops.switched_varexp_sum(tY, tF, s0=None, ssq=None, knn=[c["knn"][0]], members=c["members"], ylab=P)
    assert all(o is None for o in only[1:])
    val0, bnd0 = _switched_reference(c["members"], c["Yfull"][:, :P].astype(LD), c["task"], c["F"].astype(LD),
                                     np.full((rows, P), LD(c["knn"][0])), np.zeros((rows, P), dtype=LD), np.zeros((rows, P), dtype=LD))
    _within("out[0], fvar = knn", _np(only[0])[0:1], [val0[0].sum()], [bnd0[0].sum() + 2 * (rows * P + 2) * U * np.abs(val0[0]).sum()])


@pytest.mark.parametrize("kind", ["light", "heavy"])
@pytest.mark.parametrize("case", CASES + [BIG_CASE], ids=str)
def test_device_and_emulation_agree_within_the_bounds(gp, case, kind):
    """the primitive and tests/fake_switched_ops.py on the same inputs: each is held to the longdouble reference by the same bounds,
    and the two results are compared DIRECTLY, output by output, within the sum of their two bounds (each sits within one bound of
    the reference, so twice the bound is what the triangle inequality gives and nothing wider is allowed)"""
    from gpflow_amd import ops
    c = _case(case, kind)
    P = c["P"]
    kw = dict(knn=c["knn"], members=c["members"], mean_const=c["mc"], s0_per_latent=c["per"], want_fvar=True, want_rows=True,
              want_grads=True)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    emu = fake_switched_ops.switched_varexp_sum(t(c["Yfull"][:, :P + 1]), t(c["F"]), s0=t(c["s0"]), ssq=t(c["ssq"]), **kw)
    dev = ops.switched_varexp_sum(ops.to_device(c["Yfull"])[:, :P + 1], ops.to_device(c["F"]), s0=ops.to_device(c["s0"]),
                                  ssq=ops.to_device(c["ssq"]), **kw)
    _check_against_reference(f"emulation {kind} {case}", c, emu)
    _check_against_reference(f"device {kind} {case}", c, dev)
    for (name, got_dev, _, bound), (_, got_emu, _, _) in zip(_checks(c, dev), _checks(c, emu)):
        _within(f"device against emulation {kind} {case} {name}", got_dev, np.asarray(got_emu, dtype=LD), 2 * np.asarray(bound, dtype=LD))


# ------------------------------------------------------------------------------------------------ 2. refusals of the library
PLANT = 0x7FF8DEADBEEF1234   # (a NaN payload: any write changes the bits)


def _raw(ops, lib, T_, codes, params, Y, ylab, fmean, P, out, rws, parts, knn=(1.0,)):
    rows = fmean.shape[0]
    return lib.gpk_switched_varexp_sum(ops._stream(), T_, (ctypes.c_int * max(len(codes), 1))(*codes),
                                       (ctypes.c_double * max(len(params), 1))(*params), Y.data_ptr(), Y.stride(0), ylab,
                                       fmean.data_ptr(), rows, P, None, 0, None, (ctypes.c_double * len(knn))(*knn), 0, 0.0, None,
                                       rws.data_ptr(), None, None, out.data_ptr(), parts.data_ptr())


def test_refusals_of_the_library_write_nothing(gp):
    """T = 0, T = 17, P = 17, ylab < P: GPK_E_ARG; codes 4, 5, 11: GPK_E_UNSUPPORTED; each member's bad parameter: GPK_E_ARG -- every
    one with out, rows_out and parts left as they were (planted bytes)"""
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    rows = 9
    planted = lambda n: ops.to_device(np.full(n, PLANT, dtype=np.uint64).view(np.float64))  # noqa: E731
    out, rws, parts = planted(18), planted(rows), planted(18 * 8)
    Y = ops.to_device(np.ones((rows, 18)))
    F = ops.to_device(np.zeros((rows, 17)))
    F1 = F[:, :1].contiguous()
    ok2 = ([0, 3], [0.5, 0.0, 0.8, 3.0])
    bad = [("T = 0", -1, (0, [], [], 1, F1, 1)), ("T = 17", -1, (17, [1] * 17, [0.0] * 34, 1, F1, 1)),
           ("P = 17", -1, (2,) + ok2 + (17, F, 17)), ("ylab < P", -1, (2,) + ok2 + (1, F[:, :2].contiguous(), 2)),
           ("ylab == P - 1", -1, (2,) + ok2 + (0, F1, 1))]
    bad += [(f"code {code}", -3, (2, [0, code], [0.5, 0.0, 0.5, 2.0], 1, F1, 1)) for code in (4, 5, 11)]
    bad += [(f"bad parameter of code {code}", -1, (2, [1, code], [0.0, 0.0] + list(par), 1, F1, 1))
            for code, par in ((0, (0.0, 0.0)), (0, (-1.0, 0.0)), (0, (float("nan"), 0.0)), (2, (0.0, 0.0)), (3, (-1.0, 3.0)),
                              (3, (1.0, 0.0)), (9, (0.0, 0.0)), (10, (-2.0, 0.0)))]
    for what, status, (T_, codes, params, ylab, fm, P) in bad:
        rc = _raw(ops, lib, T_, codes, params, Y, ylab, fm, P, out, rws, parts)
        assert rc == status, (what, rc)
        for name, buf in (("out", out), ("rows_out", rws), ("parts", parts)):
            assert (_np(buf).view(np.uint64) == PLANT).all(), (what, name)
    # the wrapper refuses what it can see itself, and passes the library's answer on
    for members in ([], [("gaussian", (0.5,))] * 17, [("ordinal", (1.0, 1.0, 0.0))], [("gaussian", ())], [("student_t", (0.0, 3.0))]):
        with pytest.raises(_refused()):
            ops.switched_varexp_sum(Y[:, :2], F1, s0=None, ssq=None, knn=[1.0], members=members)
    with pytest.raises(_refused()):
        ops.switched_varexp_sum(Y[:, :2], F[:, :2].contiguous(), s0=None, ssq=None, knn=[1.0], members=[("gaussian", (0.5,))])


# ------------------------------------------------------------------------------------------------ 3. invalid and non-finite input
NF_MEMBERS = [("gaussian", (0.6,)), ("bernoulli_probit", ()), ("student_t", (0.8, 3.0))]


def _nf_inputs():
    rows, P = 41, 3
    rng = np.random.default_rng(5)
    task = np.arange(rows) % 3
    Yv = np.where((task == 1)[:, None], (rng.uniform(size=(rows, P)) < 0.5).astype(np.float64), rng.normal(size=(rows, P)))
    return Yv, task.astype(np.float64), rng.normal(size=(rows, P)), rng.uniform(0, 0.5, size=rows), rng.uniform(0, 0.6, size=(P, rows))


def _nf_run(Yv, lab, F, s0, ssq):
    from gpflow_amd import ops
    r = ops.switched_varexp_sum(ops.to_device(np.concatenate([Yv, lab[:, None]], axis=1)), ops.to_device(F), s0=ops.to_device(s0),
                                ssq=ops.to_device(ssq), knn=[1.2], members=NF_MEMBERS, want_rows=True, want_grads=True, want_fvar=True)
    return [_np(t) for t in r]


@pytest.mark.parametrize("label", [float("nan"), float("inf"), float("-inf"), -1.0, 3.0, -1.5, 2.5, -0.5])
def test_invalid_task_label_makes_its_row_nan_and_nothing_else(gp, label):
    """NaN, +-Inf, <= -1, >= T: the row's rows_out, dmu, dvar and out[0] are NaN, fvar is the clean run's, every other row has the
    clean run's bits, no out[1 + t] is NaN.  2.5 is task 2 and -0.5 is task 0 (truncation toward zero): the clean run's bits throughout."""
    Yv, lab, F, s0, ssq = _nf_inputs()
    b = 17 if label != -0.5 else 18                 # (row 17 is task 2, row 18 task 0)
    assert lab[17] == 2.0 and lab[18] == 0.0
    clean = _nf_run(Yv, lab, F, s0, ssq)
    assert all(np.isfinite(a).all() for a in clean)
    lab2 = lab.copy()
    lab2[b] = label
    out, rws, gmu, gvar, fvar = _nf_run(Yv, lab2, F, s0, ssq)
    if label in (2.5, -0.5):
        for got, ref in zip((out, rws, gmu, gvar, fvar), clean):
            assert np.array_equal(_bits(got), _bits(ref))
        return
    others = np.arange(Yv.shape[0]) != b
    assert np.isnan(out[0]) and np.isnan(rws[b]) and np.isnan(gmu[b]).all() and np.isnan(gvar[b]).all()
    assert np.isfinite(out[1:]).all() and out[2] == 0.0
    assert np.array_equal(_bits(out[1]), _bits(clean[0][1]))        # (task 0's rows are untouched: the same sum, the same order)
    assert np.array_equal(_bits(fvar), _bits(clean[4]))
    for got, ref in ((rws, clean[1]), (gmu, clean[2]), (gvar, clean[3])):
        assert np.array_equal(_bits(got[others]), _bits(ref[others]))


@pytest.mark.parametrize("where", ["Y", "fmean", "ssq"])
@pytest.mark.parametrize("b", [15, 16, 17], ids=["gaussian", "bernoulli", "student_t"])
def test_nonfinite_value_follows_the_members_rule(gp, where, b):
    """a NaN in a value column of Y, in fmean or in ssq at (b, 1): out[0], the row's rows_out and the element's dmu / dvar are NaN (where
    the member's formula reads the operand: the Gaussian's dmu does not read the variance, its dvar only sees a NaN label), the task's own out[1 + t] where it has a parameter, and
    nothing else -- every other entry has the clean run's bits"""
    Yv, lab, F, s0, ssq = _nf_inputs()
    p, t = 1, b % 3
    clean = _nf_run(Yv, lab, F, s0, ssq)
    arrs = {"Y": Yv.copy(), "fmean": F.copy(), "ssq": ssq.copy()}
    if where == "ssq":
        arrs[where][p, b] = np.nan
    else:
        arrs[where][b, p] = np.nan
    out, rws, gmu, gvar, fvar = _nf_run(arrs["Y"], lab, arrs["fmean"], s0, arrs["ssq"])
    hit = np.zeros(F.shape, dtype=bool)
    hit[b, p] = True
    rows_hit = hit.any(1)
    assert np.isnan(out[0]) and np.isnan(rws[b])
    gauss = NF_MEMBERS[t][0] == "gaussian"   # its dmu = (y - mu) / s2 does not read the variance, its dvar = -1 / (2 s2) reads nothing
    for name, got, ref, reached in (("dmu", gmu, clean[2], not (gauss and where == "ssq")),
                                    ("dvar", gvar, clean[3], not (gauss and where != "Y"))):
        assert np.isnan(got[b, p]) if reached else np.array_equal(_bits(got[b, p]), _bits(ref[b, p])), (name, where)
    assert np.array_equal(_bits(rws[~rows_hit]), _bits(clean[1][~rows_hit]))
    assert np.array_equal(_bits(gmu[~hit]), _bits(clean[2][~hit])) and np.array_equal(_bits(gvar[~hit]), _bits(clean[3][~hit]))
    for u in range(3):
        if u == t and NF_MEMBERS[u][0] in TRAINABLE:
            assert np.isnan(out[1 + u]), (u, out)
        else:
            assert np.array_equal(_bits(out[1 + u]), _bits(clean[0][1 + u])), (u, out)


# ------------------------------------------------------------------------------------------------ 4. placement independence
@pytest.mark.parametrize("kind", ["light", "heavy"])
def test_an_elements_outputs_do_not_depend_on_where_its_row_sits(gp, kind):
    """the same rows sorted by task and randomly permuted: dmu, dvar, fvar and rows_out, un-permuted, are bit-identical; a rerun is
    bit-identical in everything, out included"""
    from gpflow_amd import ops
    c = _case((257, 1, 4, "sorted", False, "ld"), kind)
    rows, P = c["F"].shape
    Yc = np.ascontiguousarray(c["Yfull"][:, :P + 1])
    perm = np.random.default_rng(3).permutation(rows)

    def run(order):
        r = ops.switched_varexp_sum(ops.to_device(Yc[order]), ops.to_device(c["F"][order]), s0=ops.to_device(c["s0"][order]),
                                    ssq=ops.to_device(np.ascontiguousarray(c["ssq"][:, order])), knn=c["knn"], members=c["members"],
                                    want_fvar=True, want_rows=True, want_grads=True)
        return [_np(t) for t in r]
    a, b, b2 = run(np.arange(rows)), run(perm), run(perm)
    for x, y in zip(b, b2):
        assert np.array_equal(_bits(x), _bits(y)), "a rerun differs"
    inv = np.argsort(perm)
    for name, x, y in zip(("rows", "dmu", "dvar", "fvar"), a[1:], b[1:]):
        assert np.array_equal(_bits(x), _bits(y[inv])), name


# ------------------------------------------------------------------------------------------------ 5. scratch
def test_parts_is_scratch_with_a_documented_extent(gp):
    """parts filled with 0xFF and with another call's leftovers, between guard zones: the same bits, the guards untouched"""
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    c = _case((257, 1, 4, "sorted", False, "ld"), "heavy")
    rows, P = c["F"].shape
    ntasks = len(c["members"])
    codes = [ops.SWITCHED_MEMBERS[n] for n, _ in c["members"]]
    params = [v for _, par in c["members"] for v in (list(par) + [0.0, 0.0])[:2]]
    extent = (1 + ntasks) * int(lib.gpk_switched_varexp_blocks(rows, P))
    assert extent == (1 + ntasks) * 5                         # 257 rows, 16 per pass: 17 passes, four per block
    G = 64
    tY, tF = ops.to_device(np.ascontiguousarray(c["Yfull"][:, :P + 1])), ops.to_device(c["F"])
    results = []
    for fill in ("ff", "leftovers"):
        buf = ops.to_device(np.full(extent + 2 * G, PLANT, dtype=np.uint64).view(np.float64))
        parts = buf[G:G + extent]
        if fill == "ff":
            parts.copy_(ops.to_device(np.full(extent, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64).view(np.float64)))
        else:   # what a call on other data leaves behind
            assert _raw(ops, lib, ntasks, codes, params, tY, P, (tF * 0.5).contiguous(), P, ops.to_device(np.zeros(1 + ntasks)),
                        ops.to_device(np.zeros(rows)), parts, knn=(0.7,)) == 0
        out, rws = ops.to_device(np.zeros(1 + ntasks)), ops.to_device(np.zeros(rows))
        assert _raw(ops, lib, ntasks, codes, params, tY, P, tF, P, out, rws, parts, knn=(1.2,)) == 0
        results.append((_np(out), _np(rws)))
        guards = _np(buf).view(np.uint64)
        assert (guards[:G] == PLANT).all() and (guards[G + extent:] == PLANT).all(), fill
    for x, y in zip(*results):
        assert np.array_equal(_bits(x), _bits(y))
    assert np.isfinite(results[0][0]).all()


# ------------------------------------------------------------------------------------------------ 6. / 7. the models
JITTER = V.JITTER
MODEL_TABLES = {"studentt-gaussian": [("student_t", (0.7, 4.0)), ("gaussian", (0.3,))],
                "bernoulli-poisson": [("bernoulli_probit", ()), ("poisson_exp", (1.0,))]}


def _member_objects(gp, table):
    Ls = gp.likelihoods
    make = {"student_t": lambda p: Ls.StudentT(scale=p[0], df=p[1]), "gaussian": lambda p: Ls.Gaussian(p[0]),
            "bernoulli_probit": lambda p: Ls.Bernoulli(), "poisson_exp": lambda p: Ls.Poisson(binsize=p[0]),
            "gamma_exp": lambda p: Ls.Gamma(shape=p[0]), "exponential_exp": lambda p: Ls.Exponential(),
            "beta_probit": lambda p: Ls.Beta(scale=p[0])}
    return [make[name](par) for name, par in table]


def _ve_member_torch(name, par, fmean, fvar, Y):
    if name == "poisson_exp":
        b = par[0]
        return (Y * fmean - torch.exp(fmean + fvar / 2) * b - torch.lgamma(Y + 1.0) + Y * math.log(b)).sum()
    if name == "beta_probit":
        return Z._torch_ve(name, par, fmean, fvar, Y)
    return V._ve_torch(name, par, fmean, fvar, Y)


def _ve_switched_torch(table, tpars, fmean, fvar, Y):
    """the sum of the variational expectations, each row under its own member (the task: the last column of Y, truncated)"""
    task = torch.trunc(Y[:, -1]).long()
    total = torch.zeros((), dtype=torch.float64)
    for t, (name, _) in enumerate(table):
        sel = task == t
        if bool(sel.any()):
            total = total + _ve_member_torch(name, tpars[t], fmean[sel], fvar[sel], Y[sel][:, :-1])
    return total


def _leaf(a):
    return torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)


def _lik_leaves(table):
    """(the members' parameters with the trainable one a leaf tensor, {task: leaf})"""
    tpars, leaves = [], {}
    for t, (name, par) in enumerate(table):
        if name in TRAINABLE:
            leaves[t] = _leaf(par[0])
            tpars.append((leaves[t],) + tuple(par[1:]))
        else:
            tpars.append(tuple(par))
    return tpars, leaves


def _recipe_data(table, N, seed):
    """the coregionalisation recipe's data: X = [x, task], Y = [value, task], the tasks stacked one after the other"""
    rng = np.random.default_rng(seed)
    task = np.repeat(np.arange(len(table)), N // len(table))
    x = rng.uniform(-1.5, 1.5, size=task.size)
    f = np.sin(2 * x + task)
    y = np.zeros(task.size)
    for t, (name, _) in enumerate(table):
        s = task == t
        y[s] = {"student_t": lambda: f[s] + 0.3 * rng.normal(size=int(s.sum())), "gaussian": lambda: f[s] + 0.3 * rng.normal(size=int(s.sum())),
                "bernoulli_probit": lambda: (f[s] + 0.3 * rng.normal(size=int(s.sum())) > 0).astype(np.float64),
                "poisson_exp": lambda: rng.poisson(np.exp(0.5 * f[s] + 0.5)).astype(np.float64)}[name]()
    X = np.stack([x, task.astype(np.float64)], axis=1)
    Y = np.stack([y, task.astype(np.float64)], axis=1)
    n = task.size
    q_mu = 0.3 * rng.normal(size=(n, 1))
    q_sqrt = (np.tril(0.05 * rng.normal(size=(n, n))) + 0.6 * np.eye(n))[None]
    return X, Y, q_mu, q_sqrt


W0, KAPPA0 = np.array([[0.6], [-0.4]]), np.array([0.9, 1.2])


def _recipe_kernel(gp):
    K = gp.kernels
    co = K.Coregion(2, 1, active_dims=[1])
    co.W.assign(W0)
    co.kappa.assign(KAPPA0)
    return K.SquaredExponential(variance=1.3, lengthscales=0.8, active_dims=[0]) * co


def _recipe_kfun(v):
    def kfun(A, B):
        Bm = v["W"] @ v["W"].T + torch.diag(v["kappa"])
        return orcg._rbf(A[:, :1], B[:, :1], v["variance"], v["lengthscales"]) * Bm[A[:, 1].long()][:, B[:, 1].long()]
    return kfun


def _vgp(gp, name, seed=11):
    table = MODEL_TABLES[name]
    X, Y, q_mu, q_sqrt = _recipe_data(table, 64, seed)
    lik = gp.likelihoods.SwitchedLikelihood(_member_objects(gp, table))
    m = gp.models.VGP((X, Y), _recipe_kernel(gp), lik, mean_function=gp.mean_functions.Constant(0.2))
    assert m.num_latent_gps == 1 and m.q_mu.shape == (64, 1)
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    return m, table, (X, Y)


def _vgp_autograd(m, table, data):
    X, Y = data
    se, co = m.kernel.kernels
    v = {"variance": _leaf(se.variance.numpy()), "lengthscales": _leaf(np.atleast_1d(se.lengthscales.numpy())), "W": _leaf(co.W.numpy()),
         "kappa": _leaf(co.kappa.numpy()), "q_mu": _leaf(m.q_mu.numpy()), "q_sqrt": _leaf(m.q_sqrt.numpy()),
         "mean": _leaf(m.mean_function.c.numpy())}
    current = [(n, (float(p.numpy()),) + tuple(par[1:])) if p is not None else (n, par)
               for (n, par), p in zip(table, m.likelihood.device_grad_params())]
    tpars, leaves = _lik_leaves(current)
    N, R = v["q_mu"].shape
    fmean, fvar, _ = V._torch_moments(_t(X), v["q_mu"], v["q_sqrt"], _recipe_kfun(v), v["mean"])
    S = torch.tril(v["q_sqrt"])
    kl = 0.5 * ((v["q_mu"] ** 2).sum() - N * R - torch.log(torch.diagonal(S, dim1=1, dim2=2) ** 2).sum() + (S * S).sum())
    F = _ve_switched_torch(current, tpars, fmean, fvar, _t(Y)) - kl
    F.backward()
    grads = {k: a.grad.detach().numpy().copy() for k, a in v.items()}
    return float(F.detach()), grads, {t: a.grad.detach().numpy().copy() for t, a in leaves.items()}


def _check_model_grads(name, pars, lik, g, go, glik, q_sqrt, extra=0):
    """every trainable Parameter's d/d(unconstrained) against autograd's constrained gradient chained through its transform"""
    lik_pars = {t: p for t, p in enumerate(lik.device_grad_params()) if p is not None}
    assert set(lik_pars) == set(glik), (name, set(lik_pars), set(glik))
    assert set(g) == set(pars.values()) | set(lik_pars.values()) | {q_sqrt}, name
    for key, par in list(pars.items()) + [(t, p) for t, p in lik_pars.items()]:
        u = par.unconstrained_variable
        ref = (glik[key] if isinstance(key, int) else go[key]).reshape(np.shape(u)) * par.transform.forward_grad(u)
        _close(f"{name} {key}", np.asarray(g[par]), ref, V.GRAD_TOL)


@pytest.mark.parametrize("name", list(MODEL_TABLES))
def test_vgp_recipe_elbo_and_grad_against_autograd(gp, name):
    """SquaredExponential(active_dims=[0]) * Coregion(2, 1, active_dims=[1]) with a switched likelihood: elbo() against the restatement
    1e-8, objective_and_grad() 1e-9 in the value and 1e-8 in every trainable parameter -- the kernel's, q_mu, q_sqrt, the mean constant
    and each task's own parameter through its transform (the Gaussian member's variance included)"""
    m, table, data = _vgp(gp, name)
    ref, go, glik = _vgp_autograd(m, table, data)
    got = float(m.elbo())
    print(f"{name}: elbo {got!r} restatement {ref!r}")
    assert abs(got - ref) <= V.ELBO_TOL * abs(ref)
    v, g = m.objective_and_grad()
    assert abs(v - ref) <= V.VALUE_TOL * abs(ref)
    se, co = m.kernel.kernels
    pars = {"variance": se.variance, "lengthscales": se.lengthscales, "W": co.W, "kappa": co.kappa, "q_mu": m.q_mu,
            "mean": m.mean_function.c}
    _check_model_grads(name, pars, m.likelihood, g, go, glik, m.q_sqrt)
    refq = m.q_sqrt.transform.inverse(np.tril(go["q_sqrt"]))
    _close(f"{name} q_sqrt", np.asarray(g[m.q_sqrt]), refq.reshape(np.shape(g[m.q_sqrt])), V.GRAD_TOL)
    assert len(g) == len(m.trainable_parameters)


def _log_density_torch(name, par, mu, var, y):
    """log int p(y | f) N(f | mu, var) df of one member, elementwise, torch-CPU fp64"""
    if name == "gaussian":
        return -0.5 * (math.log(2 * math.pi) + torch.log(var + par[0]) + (y - mu) ** 2 / (var + par[0]))
    if name == "bernoulli_probit":
        p = 0.5 * (1 + torch.special.erf(mu / torch.sqrt(1 + var) / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3
        return torch.log(torch.where(y == 1, p, 1 - p))
    x, wn = torch.tensor(V.GH_X), torch.tensor(V.GH_W / np.sqrt(np.pi))
    f = mu[..., None] + torch.sqrt(2 * var)[..., None] * x
    if name == "poisson_exp":
        lp = y[..., None] * (f + math.log(par[0])) - torch.exp(f) * par[0] - torch.lgamma(y + 1.0)[..., None]
    else:
        s, df = par
        lp = math.lgamma((df + 1) / 2) - math.lgamma(df / 2) - 0.5 * (math.log(s * s) + math.log(df) + math.log(math.pi)) \
            - 0.5 * (df + 1) * torch.log(1 + ((y[..., None] - f) / s) ** 2 / df)
    return torch.logsumexp(torch.log(wn) + lp, dim=-1)


@pytest.mark.parametrize("name", list(MODEL_TABLES))
def test_vgp_predict_log_density_and_the_refused_predictions(gp, name):
    """predict_log_density: the row's own member over the model's predict_f moments, 1e-8 of max(1, |.|) as the likelihood tests hold
    it; a row with an invalid task is NaN; predict_y has no task to go by and raises"""
    m, table, (X, Y) = _vgp(gp, name)
    Xn, Yn = X[::5].copy(), Y[::5].copy()
    got = _np(m.predict_log_density((Xn, Yn)))
    mu, var = (torch.tensor(_np(a)) for a in m.predict_f(Xn))
    ref = torch.stack([_log_density_torch(n, par, mu[:, 0], var[:, 0], _t(Yn[:, 0])) for n, par in table])
    ref = ref[Yn[:, 1].astype(int), torch.arange(Yn.shape[0])].numpy()
    assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())
    Yn[2, 1] = 2.0
    bad = _np(m.predict_log_density((Xn, Yn)))
    assert np.isnan(bad[2]) and np.array_equal(_bits(np.delete(bad, 2)), _bits(np.delete(got, 2)))
    with pytest.raises(NotImplementedError):
        m.predict_y(Xn)


def test_scipy_lowers_the_objective_and_moves_each_tasks_parameter(gp):
    """optimizers.Scipy on the recipe's model, a few iterations one at a time: the training loss never rises and ends lower, and both
    the StudentT scale and the Gaussian variance have moved"""
    m, table, data = _vgp(gp, "studentt-gaussian", seed=51)
    m.q_mu.assign(np.zeros_like(m.q_mu.numpy()))
    m.q_sqrt.assign(np.eye(64)[None])
    before = [float(p.numpy()) for p in m.likelihood.device_grad_params()]
    losses = [float(m.training_loss())]
    for _ in range(4):
        gp.optimizers.Scipy().minimize(m, options=dict(maxiter=2))
        losses.append(float(m.training_loss()))
    print("training loss per round:", losses)
    assert all(b <= a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0] - 1.0
    after = [float(p.numpy()) for p in m.likelihood.device_grad_params()]
    assert all(a != b for a, b in zip(before, after)), (before, after)


def _svgp_problem(table, M, B, seed, q_diag):
    X, Y, _, _ = _recipe_data(table, B, seed)
    rng = np.random.default_rng(seed + 1)
    Zx = rng.uniform(-1.5, 1.5, size=(M, 1))
    q_mu = 0.3 * rng.normal(size=(M, 1))
    q_sqrt = rng.uniform(0.3, 0.9, size=(M, 1)) if q_diag else (np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M))[None]
    return X, Y, Zx, q_mu, q_sqrt


def _svgp_torch_elbo(table, tpars, X, Y, Zt, q_mu, q_sqrt, kfun, kdiag, mean, num_data):
    """the whitened ELBO of tests/test_gpu_likelihood_zoo.py::_torch_elbo with any kernel and the switched stage"""
    M, B = Zt.shape[0], X.shape[0]
    A = torch.linalg.solve_triangular(torch.linalg.cholesky(kfun(Zt, Zt) + JITTER * torch.eye(M, dtype=torch.float64)), kfun(Zt, X),
                                      upper=False)
    fmean = A.T @ q_mu + mean
    if q_sqrt.dim() == 2:
        LTA = A[None, :, :] * q_sqrt.T[:, :, None]
        kl = 0.5 * ((q_mu * q_mu).sum() - M - torch.log(q_sqrt ** 2).sum() + (q_sqrt ** 2).sum())
    else:
        Lq = torch.tril(q_sqrt)
        LTA = Lq.transpose(1, 2) @ A
        kl = 0.5 * ((q_mu * q_mu).sum() - M - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())
    fvar = ((kdiag(X) - (A * A).sum(0))[None, :] + (LTA * LTA).sum(1)).T
    return _ve_switched_torch(table, tpars, fmean, fvar, Y) * (num_data / B) - kl


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "qdiag"])
@pytest.mark.parametrize("name", list(MODEL_TABLES))
def test_svgp_elbo_and_grad_against_autograd(gp, name, q_diag):
    """whitened SVGP, M = 32, B = 120, a SquaredExponential over the one input column, the task label in Y alone: elbo() on the
    composed path (the fused shard declines a switched likelihood) 1e-8, elbo_and_grad() at the zoo's tolerances -- 1e-9 in the value,
    1e-8 of max(1, largest entry) in every gradient, each task's parameter chained through its transform"""
    table = MODEL_TABLES[name]
    X2, Y, Zx, q_mu, q_sqrt = _svgp_problem(table, 32, 120, 23, q_diag)
    X = X2[:, :1].copy()
    lik = gp.likelihoods.SwitchedLikelihood(_member_objects(gp, table))
    m = gp.models.SVGP(gp.kernels.SquaredExponential(variance=1.3, lengthscales=0.8), lik, Zx.copy(), q_mu=q_mu.copy(),
                       q_sqrt=q_sqrt.copy(), q_diag=q_diag, whiten=True, num_data=1000, mean_function=gp.mean_functions.Constant(0.2))
    assert m._fused_config() is None and not m._device_likelihood() and m._switched_likelihood()
    v = {"variance": _leaf(1.3), "lengthscales": _leaf([0.8]), "Z": _leaf(Zx), "q_mu": _leaf(q_mu), "q_sqrt": _leaf(q_sqrt),
         "mean": _leaf(0.2)}
    tpars, leaves = _lik_leaves(table)
    kfun = lambda A, B: orcg._rbf(A, B, v["variance"], v["lengthscales"])  # noqa: E731
    F = _svgp_torch_elbo(table, tpars, _t(X), _t(Y), v["Z"], v["q_mu"], v["q_sqrt"], kfun, lambda A: v["variance"] + 0 * A[:, 0],
                         v["mean"], 1000)
    F.backward()
    ref = float(F.detach())
    got = float(m.elbo((X, Y)))
    print(f"{name}: elbo {got!r} restatement {ref!r}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
    val, g = m.elbo_and_grad((X, Y))
    assert abs(val - ref) <= 1e-9 * abs(ref)
    go = {k: a.grad.detach().numpy().copy() for k, a in v.items()}
    glik = {t: a.grad.detach().numpy().copy() for t, a in leaves.items()}
    pars = {"variance": m.kernel.variance, "lengthscales": m.kernel.lengthscales, "Z": m.inducing_variable.Z, "q_mu": m.q_mu,
            "mean": m.mean_function.c}
    if q_diag:
        pars["q_sqrt"] = m.q_sqrt
    _check_model_grads(name, pars, lik, g, go, glik, m.q_sqrt)
    if not q_diag:
        refq = m.q_sqrt.transform.inverse(np.tril(go["q_sqrt"]))
        _close(f"{name} q_sqrt", np.asarray(g[m.q_sqrt]), refq.reshape(np.shape(g[m.q_sqrt])), 1e-8)


def test_svgp_elbo_with_the_coregion_product_runs_forward_only(gp):
    """the recipe's kernel at SVGP scale: elbo() on the composed path against the restatement 1e-8; its reverse pass stays refused
    (a row-diagonal member under the quadrature reverse pass) before the device is touched"""
    table = MODEL_TABLES["studentt-gaussian"]
    X, Y, Zx, q_mu, q_sqrt = _svgp_problem(table, 32, 120, 29, False)
    Zf = np.concatenate([Zx, (np.arange(32) % 2)[:, None].astype(np.float64)], axis=1)
    lik = gp.likelihoods.SwitchedLikelihood(_member_objects(gp, table))
    m = gp.models.SVGP(_recipe_kernel(gp), lik, Zf.copy(), q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), whiten=True, num_data=1000)
    v = {"variance": _t(1.3), "lengthscales": _t([0.8]), "W": _t(W0), "kappa": _t(KAPPA0)}
    kfun = _recipe_kfun(v)
    Bm = v["W"] @ v["W"].T + torch.diag(v["kappa"])
    tpars = [(_t(par[0]),) + tuple(par[1:]) if n in TRAINABLE else tuple(par) for n, par in table]
    ref = float(_svgp_torch_elbo(table, tpars, _t(X), _t(Y), _t(Zf), _t(q_mu), _t(q_sqrt), kfun,
                                 lambda A: v["variance"] * torch.diagonal(Bm)[A[:, 1].long()], _t(0.0), 1000))
    got = float(m.elbo((X, Y)))
    print(f"coregion product: elbo {got!r} restatement {ref!r}")
    assert abs(got - ref) <= 1e-8 * abs(ref)
    with pytest.raises(NotImplementedError):
        m.elbo_and_grad((X, Y))
