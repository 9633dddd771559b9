"""GPU tests of the ChangePoints kernel: the four primitives of gpflow_amd/csrc/changepoints/changepoints.hip (`ops.changepoint_weights`,
`_fold`, `_adjoint_stage`, `_adjoint_tail`), `kernels.ChangePoints` and its node in `gradients.KernelSpec` (build, kdiag_rows, adjoint,
diag_adjoint), and the models: GPR, SVGP in its four parametrisations, VGP, the posteriors, optimizers.Scipy.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_changepoints_emulated.py imports them without this
module's `gpu` mark and gives them an emulated `gp` fixture).  On the device every primitive case also runs the emulation beside it.

References.  Primitives: an np.longdouble evaluation of the formulas of include/gpk.h with a bound per element, first order in
u = 2^-53 (`_cp_ref`).  z = s (x - l): the difference and the product round once each, 2 u |z|.  E = exp(-z) carries that error of
its argument plus EXP_ULP = 3 ulp (the OpenCL full-profile bound the ROCm device library is built to; one ulp is at most 2 u of the
value): rel E <= 2 u |z| + 2 EXP_ULP u.  1 + E rounds once and the reciprocal once, and d sig / sig = (E / (1 + E)) rel E, where
E / (1 + E) is the OTHER side's sigmoid: rel sig <= (2 u |z| + 2 EXP_ULP u) (1 - sig) + 2 u, and the same with the sides swapped.
a_i is one product more.  Every bound gets TINY = 1e-300 on top: where exp overflows the double gives exactly 0 and the
longdouble something below 1e-308.  Fold and stage: the products round once each; a sum of m terms in a fixed order adds
(m - 1) u sum |terms|.  The tail: the same rules composed over its formulas (`_tail_ref`).
The adjoint whole: torch autograd of the formula to ADJ_TOL = 1e-9 in the measure of `_close`; inputs uniform in [-1, 1],
locations (-0.3, 0.4), steepness (3, 5): |z| <= 7, no weight is saturated, every derivative is a smooth O(1) function and a sum of
up to 9100 terms carries no more than its largest term's rounding error relative to the largest entry.
Models: torch under autograd (oracle/gp_oracle_grad.py through its `kfun=` / `kdiag=` hooks; VGP: the restated ELBO of
tests/test_gpu_vgp.py); values 1e-9 relative, gradients 1e-8 through `_check_model_grads` -- the project's figures.

Condition of the model problems (B = 40, P = 2, D = 3, M = 16, inputs uniform in [-1, 1]: test_gpu_dot_kernels._problem(3, 16)).  Every
kernel entry and every entry of the row diagonal was perturbed by a relative 4 * 2^-52 with random signs in the oracle, on the CPU
(`conditioning_figures`, asserted at <= 1e-10 by tests/test_changepoints_emulated.py); the oracle's own gradients moved by at most,
in the measure of `_close`: CONDITIONING_FIGURES below.  A new shape or seed needs that check repeated.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_changepoints_ops  # noqa: E402
import test_gpu_dot_kernels as DK  # noqa: E402
import test_gpu_kernel_trees as TR  # noqa: E402
import test_gpu_vgp as VG  # noqa: E402
from test_gpu_contract import LD, U, _bits, _check_unchanged, _np, _on, _padding_untouched, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

VALUE_TOL, GRAD_TOL = 1e-9, 1e-8
ADJ_TOL = 1e-9
EXP_ULP = 3
TINY = LD(1e-300)
TILE = 64
# the largest move of the oracle's gradients under the perturbation of the module docstring, per problem (CPU, this file's seeds)
CONDITIONING_FIGURES = {"gpr": 1.1e-14, "svgp": 1.9e-13, "svgp heteroskedastic": 1.5e-13, "vgp bernoulli": 8.0e-15}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


class _Emulation:
    changepoint_weights = staticmethod(fake_changepoints_ops.changepoint_weights)
    changepoint_fold = staticmethod(fake_changepoints_ops.changepoint_fold)
    changepoint_adjoint_parts = staticmethod(fake_changepoints_ops.changepoint_adjoint_parts)
    changepoint_adjoint_stage = staticmethod(fake_changepoints_ops.changepoint_adjoint_stage)
    changepoint_adjoint_tail = staticmethod(fake_changepoints_ops.changepoint_adjoint_tail)


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", _Emulation, "cpu")] if dev != "cpu" else [])


# ------------------------------------------------------------------------------------------------ the longdouble reference
def _cp_ref(x, loc, st):
    """dict of (value, bound) pairs in longdouble: "A" [T, n], and "sig" / "comp" [C, n] with their RELATIVE bounds"""
    x, loc, st = np.asarray(x, dtype=LD).reshape(-1), np.asarray(loc, dtype=LD).reshape(-1), np.asarray(st, dtype=LD).reshape(-1)
    with np.errstate(all="ignore"):
        z = st[:, None] * (x[None, :] - loc[:, None])
        sig, comp = 1 / (1 + np.exp(-z)), 1 / (1 + np.exp(z))
        relz = 2 * U * np.abs(z) + 2 * EXP_ULP * U
        rs, rc = relz * comp + 2 * U, relz * sig + 2 * U
        one, zero = np.ones((1, x.size), dtype=LD), np.zeros((1, x.size), dtype=LD)
        A = np.concatenate([one, sig]) * np.concatenate([comp, one])
        rA = np.concatenate([zero, rs]) + np.concatenate([rc, zero]) + U
    return dict(A=(A, np.abs(A) * rA + TINY), sig=(sig, rs), comp=(comp, rc), rA=rA)


def _points(C, seed=0):
    """C sorted locations in (-0.8, 0.8) and C steepness values in (0.5, 5)"""
    rng = np.random.default_rng(40 + C + seed)
    return np.sort(rng.uniform(-0.8, 0.8, size=C)), rng.uniform(0.5, 5.0, size=C)


MEMBERS = (1, 2, 3, 16)
SIZES = (1, 63, 64, 65, 130, 300)     # 300: a second workgroup of the one-thread-per-row kernels (256 rows each)


# ------------------------------------------------------------------------------------------------ 1. the weights
@pytest.mark.parametrize("T", MEMBERS)
@pytest.mark.parametrize("n", SIZES)
def test_changepoint_weights(gp, n, T):
    """a_i(x_r) over a switch column that is a strided view (column 1 of an [n, 3] matrix), into a padded `out`: within the bound,
    padding untouched, inputs unchanged, the layout of x without influence on the bits"""
    rng = np.random.default_rng(n + T)
    X = rng.uniform(-1.0, 1.0, size=(n, 3))
    loc, st = _points(T - 1)
    ref, bnd = _cp_ref(X[:, 1], loc, st)["A"]
    for who, impl, dev in _impls(gp):
        tX = _on(X, "ld", dev)
        out, buf = _on(np.full((T, n), -555.0), "pad", dev, base=True)
        got = impl.changepoint_weights(tX[:, 1], locations=loc, steepness=st, out=out)
        assert got is out and _padding_untouched(out, buf), f"{who}: padding written"
        _within(f"changepoint_weights {who}", _np(out), ref, bnd)
        fresh = impl.changepoint_weights(_on(X[:, 1].copy(), "c", dev), locations=loc, steepness=st)
        assert _same_bits(_np(fresh), _np(out)), f"{who}: the layout of x changes the result"
        _check_unchanged(f"changepoint_weights {who}", [tX], [X])


def test_changepoint_weights_saturate_exactly(gp):
    """steepness 1e3 and inputs straddling the locations: beyond |x - l| = 0.8 the sigmoids are EXACTLY 0 or 1 (exp overflows to Inf or
    underflows to 0), a member on the far side of a change point weighs exactly 0 and the member inside weighs exactly 1; close to a
    location the weights stay within the bound; |x| = 1e300 saturates without a NaN"""
    loc, st = np.array([-1.0, 2.0]), np.array([1e3, 1e3])
    x = np.array([-1.0 - 1e-3, -1.0, -1.0 + 1e-3, -1.9, -0.1, 0.5, 1.2, 2.0 - 1e-4, 2.0 + 1e-4, 2.9, 40.0, -1e300, 1e300])
    ref, bnd = _cp_ref(x, loc, st)["A"]
    for who, impl, dev in _impls(gp):
        A = _np(impl.changepoint_weights(_on(x, "c", dev), locations=loc, steepness=st))
        _within(f"saturation {who}", A, ref, bnd)
        assert np.all(np.isfinite(A)), who
        for r, want in ((3, [1.0, 0.0, 0.0]), (4, [0.0, 1.0, 0.0]), (5, [0.0, 1.0, 0.0]), (6, [0.0, 1.0, 0.0]), (9, [0.0, 0.0, 1.0]),
                        (10, [0.0, 0.0, 1.0]), (11, [1.0, 0.0, 0.0]), (12, [0.0, 0.0, 1.0])):
            assert _same_bits(A[:, r], np.array(want)), (who, r, A[:, r])
        assert 0.0 < A[0, 2] < 1.0 and 0.0 < A[1, 2] < 1.0 and A[2, 2] == 0.0          # beside the first location: a smooth mix of 0 and 1
        assert A[0, 1] == 0.5 and A[1, 1] == 0.5                                         # on it: sigmoid(0) twice


@pytest.mark.parametrize("planted", [float("nan"), float("inf"), -float("inf")], ids=["nan", "inf", "-inf"])
def test_changepoint_nan_reaches_its_own_row_only(gp, planted):
    """a NaN or an Inf in the switch column makes every weight of THAT row NaN and no other; through the fold: exactly that row and
    that column of K"""
    n1, n2, C = 130, 70, 2
    rng = np.random.default_rng(5)
    x1, x2 = rng.uniform(-1, 1, size=n1), rng.uniform(-1, 1, size=n2)
    b1, b2 = x1.copy(), x2.copy()
    b1[129], b2[3] = planted, planted
    loc, st = _points(C)
    Ki, acc = rng.normal(size=(n1, n2)), rng.normal(size=(n1, n2))
    bad = np.zeros((n1, n2), dtype=bool)
    bad[129, :] = True
    bad[:, 3] = True
    for who, impl, dev in _impls(gp):
        kw = dict(locations=loc, steepness=st)
        Ac, Bc = impl.changepoint_weights(_on(x1, "c", dev), **kw), impl.changepoint_weights(_on(x2, "c", dev), **kw)
        Ab, Bb = impl.changepoint_weights(_on(b1, "c", dev), **kw), impl.changepoint_weights(_on(b2, "c", dev), **kw)
        rows = np.broadcast_to(np.arange(n1) == 129, (C + 1, n1))
        assert np.array_equal(np.isnan(_np(Ab)), rows) and _same_bits(_np(Ab)[~rows], _np(Ac)[~rows]), who
        for i in range(C + 1):
            clean = _np(impl.changepoint_fold(Ac[i], Bc[i], _on(Ki, "c", dev), _on(acc, "c", dev)))
            K = _np(impl.changepoint_fold(Ab[i], Bb[i], _on(Ki, "c", dev), _on(acc, "c", dev)))
            assert np.array_equal(np.isnan(K), bad) and _same_bits(K[~bad], clean[~bad]), (who, i)


# ------------------------------------------------------------------------------------------------ 2. the fold
FOLD_CASES = [(1, 1), (63, 65), (64, 64), (65, 130), (130, 70), (130, 130)]
LAYOUTS = ("c", "ld", "off", "pad")


def _fold_ref(a, b, Ki, acc, diag_add, symmetric):
    al, bl, Kl = a.astype(LD), b.astype(LD), Ki.astype(LD)
    t = al[:, None] * bl[None, :] * Kl
    ref, bnd = t, 2 * U * np.abs(t)
    if acc is not None:
        ref = acc.astype(LD) + t
        bnd = bnd + U * np.abs(ref)
    if symmetric:
        eye = np.eye(Ki.shape[0], dtype=LD)
        ref = ref + LD(diag_add) * eye
        bnd = bnd + U * np.abs(ref) * eye
    return ref, bnd + TINY


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n1,n2", FOLD_CASES)
def test_changepoint_fold(gp, n1, n2, layout):
    """both ops, in place (out is Ki for op 0, acc for op 1) and into a fresh output: within the bound, bitwise the same either way,
    padding untouched, the operands that are not `out` unchanged; diag_add is ignored with b given"""
    rng = np.random.default_rng(100 * n1 + n2)
    a, b = rng.normal(size=n1), rng.normal(size=n2)
    Ki, acc = rng.normal(size=(n1, n2)), rng.normal(size=(n1, n2))
    for who, impl, dev in _impls(gp):
        ta, tb = _on(a, "c", dev), _on(b, "c", dev)
        for op in (0, 1):
            ref, bnd = _fold_ref(a, b, Ki, acc if op else None, 0.0, False)
            name = f"changepoint_fold {who} op {op}"
            tK, kbuf = _on(Ki, layout, dev, base=True)
            tacc, abuf = _on(acc, "pad" if layout == "c" else layout, dev, base=True)
            out, obuf = (tacc, abuf) if op else (tK, kbuf)
            got = impl.changepoint_fold(ta, tb, tK, tacc if op else None, diag_add=9.0, out=out)          # in place
            assert got is out and _padding_untouched(out, obuf), f"{name}: padding written"
            _within(name, _np(out), ref, bnd)
            if op:
                _check_unchanged(name, [tK], [Ki])
            tK2, tacc2 = _on(Ki, "ld", dev), _on(acc, "c", dev)
            sep = impl.changepoint_fold(ta, tb, tK2, tacc2 if op else None)                                # a fresh output
            assert _same_bits(_np(sep), _np(out)), f"{name}: aliasing or the layout changes the result"
            _check_unchanged(name, [tK2, tacc2, ta, tb], [Ki, acc, a, b])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_changepoint_fold_symmetric(gp, n, layout):
    """b None: an exactly symmetric Ki (and acc) gives an EXACTLY symmetric result -- the weight a_r a_c is formed first -- and
    diag_add lands on the diagonal of the result, nowhere else"""
    rng = np.random.default_rng(n)
    a = rng.normal(size=n)
    Ki, acc = rng.normal(size=(n, n)), rng.normal(size=(n, n))
    Ki, acc = Ki + Ki.T, acc + acc.T
    for who, impl, dev in _impls(gp):
        ta = _on(a, "c", dev)
        for op in (0, 1):
            ref, bnd = _fold_ref(a, a, Ki, acc if op else None, 0.25, True)
            name = f"changepoint_fold symmetric {who} op {op}"
            tK, tacc = _on(Ki, layout, dev), _on(acc, layout, dev)
            out, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
            impl.changepoint_fold(ta, None, tK, tacc if op else None, diag_add=0.25, out=out)
            got = _np(out).copy()
            assert _padding_untouched(out, buf) and _same_bits(got, got.T), f"{name}: not exactly symmetric"
            _within(name, got, ref, bnd)
            plain = _np(impl.changepoint_fold(ta, None, tK, tacc if op else None))
            assert _same_bits(plain - np.diag(np.diag(plain)), got - np.diag(np.diag(got))), f"{name}: diag_add reached off the diagonal"
            assert _same_bits(plain, _np(impl.changepoint_fold(ta, ta, tK, tacc if op else None))), f"{name}: b = a given differs"
            _check_unchanged(name, [tK, tacc, ta], [Ki, acc, a])


# ------------------------------------------------------------------------------------------------ 3. the adjoint stage
STAGE_CASES = [(130, 70, False), (63, 63, True), (64, 64, False), (1, 1, False), (65, 130, False), (130, 130, True)]
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


def _split_parts(parts, n1, n2):
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    return parts[:tc * n1].reshape(tc, n1), parts[tc * n1:tc * n1 + tr * n2].reshape(tr, n2)


def _ff(count, dev):
    return torch.full((count,), -1, dtype=torch.int64, device=dev).view(torch.float64)


@pytest.mark.parametrize("n1,n2,symmetric", STAGE_CASES)
def test_changepoint_adjoint_stage(gp, n1, n2, symmetric):
    """G = Kbar .* (a b^T) and EVERY slot of `parts` against the longdouble sums of its own tile; `parts` pre-filled with 0xFF bytes and
    a guard zone behind its extent: every slot of the extent is written, the guard keeps its bytes; two calls bit-identical; Kbar
    unchanged; G may alias Ki"""
    rng = np.random.default_rng(7 + n1 + n2)
    a = rng.normal(size=n1)
    b = a if symmetric else rng.normal(size=n2)
    Kb, Ki = rng.normal(size=(n1, n2)), rng.normal(size=(n1, n2))
    if symmetric:
        Kb, Ki = Kb + Kb.T, Ki + Ki.T
    al, bl, Kbl, Kil = a.astype(LD), b.astype(LD), Kb.astype(LD), Ki.astype(LD)
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    extent = tc * n1 + tr * n2
    G = Kbl * (al[:, None] * bl[None, :])
    tp, tq = Kbl * Kil * bl[None, :], Kbl * Kil * al[:, None]
    rows = np.stack([tp[:, t * TILE:(t + 1) * TILE].sum(1) for t in range(tc)])
    rows_b = np.stack([(min(TILE, n2 - t * TILE) + 1) * U * np.abs(tp[:, t * TILE:(t + 1) * TILE]).sum(1) for t in range(tc)])
    cols = np.stack([tq[t * TILE:(t + 1) * TILE].sum(0) for t in range(tr)])
    cols_b = np.stack([(min(TILE, n1 - t * TILE) + 1) * U * np.abs(tq[t * TILE:(t + 1) * TILE]).sum(0) for t in range(tr)])
    for who, impl, dev in _impls(gp):
        ta, tb = _on(a, "c", dev), (None if symmetric else _on(b, "c", dev))
        name = f"changepoint_adjoint_stage {who}"
        runs = []
        for rep in range(2):
            parts = _ff(extent + 9, dev)
            tKb, tKi = _on(Kb, "ld", dev), _on(Ki, "pad", dev)
            Gd = impl.changepoint_adjoint_stage(ta, tb, tKb, tKi, parts[:extent + 9])
            _check_unchanged(name, [tKb, tKi], [Kb, Ki])
            pb = _bits(_np(parts))
            assert np.all(pb[extent:] == FF) and not np.any(pb[:extent] == FF), f"{name}: the extent of parts"
            runs.append((_np(Gd).copy(), _np(parts)[:extent].copy()))
        assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), f"{name}: a rerun differs"
        tKi, buf = _on(Ki, "off", dev, base=True)
        tKb = _on(Kb, "c", dev)
        parts = impl.changepoint_adjoint_parts(3, n1, n2, dev)
        assert tuple(parts.shape) == (3, extent)
        Ga = impl.changepoint_adjoint_stage(ta, tb, tKb, tKi, parts[1], out=tKi)                           # G aliases Ki
        assert Ga is tKi and _padding_untouched(tKi, buf) and _same_bits(_np(tKi), runs[0][0]) and _same_bits(_np(parts[1]), runs[0][1])
        _check_unchanged(name, [tKb, ta], [Kb, a])
        _within(name + " G", runs[0][0], G, 2 * U * np.abs(G) + TINY)
        got_r, got_c = _split_parts(runs[0][1], n1, n2)
        _within(name + " row slots", got_r, rows, rows_b + TINY)
        _within(name + " column slots", got_c, cols, cols_b + TINY)


# ------------------------------------------------------------------------------------------------ 4. the adjoint tail
def _tail_ref(x, loc, st, abar, dabar):
    """(d/dl, d/ds, xbar) with bounds from the weight adjoints abar [T, n] (bound dabar), the header's formulas in longdouble"""
    r = _cp_ref(x, loc, st)
    (A, _), (sig, rs), (comp, rc), rA = r["A"], r["sig"], r["comp"], r["rA"]
    xl, ll, sl = np.asarray(x, dtype=LD), np.asarray(loc, dtype=LD), np.asarray(st, dtype=LD)
    n = xl.size
    t1, t2 = abar[1:] * A[1:] * comp, abar[:-1] * A[:-1] * sig
    d1 = np.abs(A[1:] * comp) * dabar[1:] + np.abs(t1) * (rA[1:] + rc + 2 * U)
    d2 = np.abs(A[:-1] * sig) * dabar[:-1] + np.abs(t2) * (rA[:-1] + rs + 2 * U)
    tb = t1 - t2
    dt = d1 + d2 + U * (np.abs(t1) + np.abs(t2))
    dl = -sl * tb.sum(1)
    dlb = sl * (dt.sum(1) + (n + 1) * U * np.abs(tb).sum(1)) + U * np.abs(dl)
    dx = xl[None, :] - ll[:, None]
    ds = (tb * dx).sum(1)
    dsb = (dt * np.abs(dx)).sum(1) + (n + 3) * U * np.abs(tb * dx).sum(1)
    xb = (sl[:, None] * tb).sum(0)
    xbb = (sl[:, None] * dt).sum(0) + (sl.size + 2) * U * np.abs(sl[:, None] * tb).sum(0)
    return (dl, dlb + TINY), (ds, dsb + TINY), (xb, xbb + TINY)


@pytest.mark.parametrize("source", ["rows", "columns", "rows+init", "init"])
@pytest.mark.parametrize("n,n_other,T", [(1, 1, 2), (63, 65, 3), (130, 70, 16), (300, 64, 3), (65, 130, 2)])
def test_changepoint_adjoint_tail(gp, n, n_other, T, source):
    """the formulas of include/gpk.h in longdouble over random partials, a random initial [T, n] (or none) and a strided switch
    column: for the rows (the first tc n1 slots of every member) and for the columns (the tr n2 behind them), and from `init` alone
    (the diagonal path).  n = 300: a second workgroup.  A second call is bit-identical; the inputs keep their bits"""
    C = T - 1
    rng = np.random.default_rng(17 * n + T)
    X = rng.uniform(-1.0, 1.0, size=(n, 2))
    loc, st = _points(C, seed=1)
    columns = source == "columns"
    n1, n2 = (n_other, n) if columns else (n, n_other)
    tr, tc = -(-n1 // TILE), -(-n2 // TILE)
    parts = rng.normal(size=(T, tc * n1 + tr * n2))
    init = rng.normal(size=(T, n)) if "init" in source else None
    abar, dabar = np.zeros((T, n), dtype=LD), np.zeros((T, n), dtype=LD)
    if init is not None:
        abar = abar + init.astype(LD)
    if source != "init":
        sl = parts[:, tc * n1:].reshape(T, tr, n) if columns else parts[:, :tc * n1].reshape(T, tc, n)
        abar = abar + sl.astype(LD).sum(1)
        dabar = (sl.shape[1] + 1) * U * (np.abs(sl).sum(1) + (0 if init is None else np.abs(init)))
    (dl, dlb), (ds, dsb), (xb, xbb) = _tail_ref(X[:, 1], loc, st, abar, dabar)
    for who, impl, dev in _impls(gp):
        tX, tp = _on(X, "ld", dev), _on(parts, "c", dev)
        ti = None if init is None else _on(init, "pad", dev)
        kw = dict(locations=loc, steepness=st, init=ti)
        if source != "init":
            kw.update(parts=tp, n_other=n_other, columns=columns)
        runs = [tuple(_np(v).copy() for v in impl.changepoint_adjoint_tail(tX[:, 1], **kw)) for _ in range(2)]
        name = f"changepoint_adjoint_tail {who} {source}"
        assert all(_same_bits(p, q) for p, q in zip(*runs)), f"{name}: two runs differ"
        _within(name + " d/dlocations", runs[0][0], dl, dlb)
        _within(name + " d/dsteepness", runs[0][1], ds, dsb)
        _within(name + " xbar", runs[0][2], xb, xbb)
        _check_unchanged(name, [tX, tp] + ([] if ti is None else [ti]), [X, parts] + ([] if init is None else [init]))


def test_primitive_refusals_leave_the_output_unchanged(gp):
    """what the library (GPK_E_ARG / GPK_E_UNSUPPORTED), the wrappers (ValueError / NotImplementedError) or the emulation
    (AssertionError) refuse, each replayed with outputs that must keep their bits"""
    n = 40
    rng = np.random.default_rng(2)
    x, a, Ki = rng.uniform(-1, 1, size=n), rng.normal(size=n), rng.normal(size=(n, n))
    no = _refused() + (NotImplementedError,)
    for who, impl, dev in _impls(gp):
        tx, ta = _on(x, "c", dev), _on(a, "c", dev)
        out, A3, parts = _on(np.full((n, n), -555.0), "c", dev), _on(np.full((3, n), -555.0), "c", dev), _on(np.full((3, 2 * n), -555.0), "c", dev)
        tK = _on(Ki, "c", dev)
        with pytest.raises(NotImplementedError):                                     # T = 17
            impl.changepoint_weights(tx, locations=np.linspace(-1, 1, 16), steepness=np.ones(16))
        with pytest.raises(NotImplementedError):
            impl.changepoint_adjoint_tail(tx, locations=np.linspace(-1, 1, 16), steepness=np.ones(16))
        with pytest.raises(ValueError):                                              # mismatched lengths
            impl.changepoint_weights(tx, locations=[0.0, 0.5], steepness=[1.0], out=A3)
        for kw in (dict(locations=[0.5, 0.0], steepness=[1.0, 1.0]), dict(locations=[0.0, 0.5], steepness=[1.0, 0.0]),
                   dict(locations=[0.0, 0.5], steepness=[1.0, -2.0]), dict(locations=[0.0, float("nan")], steepness=[1.0, 1.0]),
                   dict(locations=[0.0, 0.5], steepness=[1.0, float("inf")])):      # unsorted; steepness <= 0; not finite
            with pytest.raises(no):
                impl.changepoint_weights(tx, out=A3, **kw)
            with pytest.raises(no):
                impl.changepoint_adjoint_tail(tx, parts=parts, n_other=n, **kw)
        for call in (lambda: impl.changepoint_weights(tx, locations=[0.0], steepness=[1.0], out=A3),             # out has T = 3 rows
                     lambda: impl.changepoint_fold(ta[:5], None, tK, out=out),
                     lambda: impl.changepoint_fold(ta, ta[:5], tK, out=out),
                     lambda: impl.changepoint_fold(ta, None, tK, out[:, :5], out=out),
                     lambda: impl.changepoint_adjoint_stage(ta, None, tK, tK[:, :5], parts[0], out=out),
                     lambda: impl.changepoint_adjoint_stage(ta, None, tK, tK, parts[0][:5], out=out),
                     lambda: impl.changepoint_adjoint_tail(tx, locations=[0.0, 0.5], steepness=[1.0, 1.0], parts=parts[:2], n_other=n),
                     lambda: impl.changepoint_adjoint_tail(tx, locations=[0.0, 0.5], steepness=[1.0, 1.0], parts=parts[:, :7], n_other=n),
                     lambda: impl.changepoint_adjoint_tail(tx, locations=[0.0, 0.5], steepness=[1.0, 1.0], init=A3[:2])):
            with pytest.raises(_refused()):
                call()
        assert np.all(_np(out) == -555.0) and np.all(_np(A3) == -555.0) and np.all(_np(parts) == -555.0), f"{who}: a refused call wrote"
        _check_unchanged(who, [tK, tx, ta], [Ki, x, a])
        assert tuple(impl.changepoint_weights(tx[:0], locations=[0.0], steepness=[1.0]).shape) == (2, 0)
        dl, ds, xb = impl.changepoint_adjoint_tail(tx, locations=[], steepness=[], init=A3[:1])                  # C = 0: nothing to return
        assert dl.numel() == 0 and ds.numel() == 0 and np.all(_np(xb) == 0.0)


# ------------------------------------------------------------------------------------------------ 5. trees with ChangePoints nodes
# A tree is a tag (a key of `kinds`), (op, [children]) or ("cp", [children], {locations, steepness[, switch_dim]}); the ChangePoints
# nodes are numbered as they are met, before their members: "cp0", "cp1", ... name their Parameters.
def _make_tree(K, tree, kinds):
    pars, made, count = {}, {}, [0]

    def walk(node):
        if isinstance(node, str):
            if node not in made:
                made[node], ps = kinds[node].make(K)
                pars.update({f"{node}.{n}": p for n, p in ps.items()})
            return made[node]
        if node[0] == "cp":
            tag = f"cp{count[0]}"
            count[0] += 1
            k = K.ChangePoints([walk(c) for c in node[1]], node[2]["locations"], node[2]["steepness"], switch_dim=node[2].get("switch_dim", 0))
            pars[f"{tag}.locations"], pars[f"{tag}.steepness"] = k.locations, k.steepness
            return k
        return (K.Sum if node[0] == "add" else K.Product)([walk(c) for c in node[1]])
    return walk(tree), pars


def _weights_torch(X, loc, st, sd):
    x = X[:, sd]
    z = st * (x[:, None] - torch.sort(loc.reshape(-1))[0][None, :])
    one = torch.ones_like(x)[:, None]
    return torch.cat([one, torch.sigmoid(z)], 1) * torch.cat([torch.sigmoid(-z), one], 1)      # [n, T]


def _tree_torch(tree, kinds, lv):
    """(kfun(A, B), kdiag(X)) of the tree over lv = {"tag.name": tensor}: the formula of the module docstring under autograd"""
    count = [0]

    def walk(node):
        if isinstance(node, str):
            return kinds[node].torch(TR._sub(lv, node))
        if node[0] == "cp":
            tag = f"cp{count[0]}"
            count[0] += 1
            parts = [walk(c) for c in node[1]]
            loc, st, sd = lv[f"{tag}.locations"], lv[f"{tag}.steepness"], node[2].get("switch_dim", 0)

            def kfun(A, B):
                wa = _weights_torch(A, loc, st, sd)
                wb = wa if A is B else _weights_torch(B, loc, st, sd)
                return sum(wa[:, i, None] * f(A, B) * wb[None, :, i] for i, (f, _) in enumerate(parts))

            def kdiag(X):
                wa = _weights_torch(X, loc, st, sd)
                return sum(wa[:, i] ** 2 * g(X) for i, (_, g) in enumerate(parts))
            return kfun, kdiag
        parts = [walk(c) for c in node[1]]

        def fold(vals):
            acc = vals[0]
            for v in vals[1:]:
                acc = acc + v if node[0] == "add" else acc * v
            return acc
        return (lambda A, B: fold([f(A, B) for f, _ in parts])), (lambda X: fold([g(X) for _, g in parts]))
    return walk(tree)


def _tree_ref(tree, kinds, vals, X1, X2):
    """(K in longdouble, bound) of a tree whose root is a ChangePoints node over leaves: the leaves' own references and bounds, the
    weights' (`_cp_ref`), and the roundings of the fold -- w = a_r b_c, w k, the running sum"""
    _, ch, v = tree
    sd = v.get("switch_dim", 0)
    order = np.argsort(np.asarray(v["locations"], dtype=np.float64), kind="stable")
    loc, st = np.asarray(vals["cp0.locations"]).reshape(-1)[order], np.broadcast_to(vals["cp0.steepness"], (len(ch) - 1,))
    (A, dA), (B, dB) = _cp_ref(X1[:, sd], loc, st)["A"], _cp_ref((X1 if X2 is None else X2)[:, sd], loc, st)["A"]
    acc, bnd = None, None
    for i, tag in enumerate(ch):
        k, kb = kinds[tag].ref(TR._sub(vals, tag), X1, X2)
        w = A[i][:, None] * B[i][None, :]
        dw = np.abs(A[i])[:, None] * dB[i][None, :] + dA[i][:, None] * np.abs(B[i])[None, :] + dA[i][:, None] * dB[i][None, :] + U * np.abs(w)
        t = w * k
        dt = np.abs(w) * kb + np.abs(k) * dw + dw * kb + U * np.abs(t)
        acc, bnd = (t, dt) if acc is None else (acc + t, bnd + dt + U * np.abs(acc + t))
    return acc, bnd + TINY


_K = TR.KINDS
CP3 = ("cp", ["se", "m32", "lin"], dict(locations=(-0.3, 0.4), steepness=(3.0, 5.0)))
CP3_KINDS = {"se": _K["SquaredExponential"], "m32": _K["Matern32"], "lin": _K["Linear"]}
_DATA = {}


def _data():
    """130 x 70 and 130 symmetric, three input columns uniform in [-1, 1]; made once"""
    if not _DATA:
        rng = np.random.default_rng(2041)
        _DATA.update(X1=rng.uniform(-1.0, 1.0, size=(130, 3)), X2=rng.uniform(-1.0, 1.0, size=(70, 3)), Kbar=rng.normal(size=(130, 70)),
                     Ksym=rng.normal(size=(130, 130)), kd_bar=rng.normal(size=130))
        _DATA["Ksym"] = _DATA["Ksym"] + _DATA["Ksym"].T
    return _DATA


def _spec_of(kern):
    from gpflow_amd.kernels.base import gradient_spec
    return gradient_spec(kern, 3)[0]


def test_kernel_forward_against_longdouble(gp):
    """K, K_into with diag_add, KernelSpec.build, K_diag and kdiag_rows of ChangePoints([SquaredExponential, Matern32, Linear]) against
    the longdouble formula, symmetric and cross, into padded outputs; the two routes bitwise equal; the symmetric matrix EXACTLY
    symmetric"""
    dev, dat = _dev(gp), _data()
    kern, pars = _make_tree(gp.kernels, CP3, CP3_KINDS)
    vals = TR._values(pars)
    spec = _spec_of(kern)
    assert spec.tree == ("cp", [0, 1, 2], 0) and not spec.constant_diagonal and not spec.packable and len(spec.nodes) == 1
    for symmetric in (True, False):
        A, B = (dat["X1"], None) if symmetric else (dat["X1"], dat["X2"])
        ref, bnd = _tree_ref(CP3, CP3_KINDS, vals, A, B)
        if symmetric:
            eye = np.eye(130, dtype=LD)
            ref = ref + LD(0.1) * eye
            bnd = bnd + U * np.abs(ref) * eye
        tA, tB = _on(A, "ld", dev), (None if symmetric else _on(B, "pad", dev))
        outs = []
        for route in ("K_into", "K_into", "build"):
            out, buf = _on(np.full(ref.shape, -555.0), "ld", dev, base=True)
            kern.K_into(tA, tB, out, diag_add=0.1) if route == "K_into" else spec.build(tA, tB, out, 0.1)
            assert _padding_untouched(out, buf), f"{route}: padding written"
            outs.append(_np(out).copy())
        _within(f"ChangePoints K symmetric={symmetric}", outs[0], ref, bnd)
        assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2]), "routes or calls differ"
        if symmetric:
            members_symmetric = all(_same_bits(_np(k(A)), _np(k(A)).T) for k in kern.kernels)
            assert members_symmetric or dev == "cpu", "the device builders mirror: every member matrix is exactly symmetric"
            assert not members_symmetric or _same_bits(outs[0], outs[0].T), "K(X, X) is not exactly symmetric"
            off = ~np.eye(130, dtype=bool)
            assert _same_bits(_np(kern(A))[off], outs[0][off]), "diag_add reached off the diagonal"
        else:
            assert _same_bits(_np(kern(A, B)), outs[0])
        _check_unchanged("forward", [tA] + ([] if symmetric else [tB]), [A] + ([] if symmetric else [B]))
    # the diagonal: sum_i a_i^2 kd_i, the leaves' diagonals from their own references
    X = dat["X1"]
    A, dA = _cp_ref(X[:, 0], vals["cp0.locations"], vals["cp0.steepness"])["A"]
    dref, dbnd = 0, 0
    for i, tag in enumerate(CP3[1]):
        k, kb = CP3_KINDS[tag].ref(TR._sub(vals, tag), X, None)
        kd, kdb = np.diag(k), np.diag(kb)
        t = A[i] * A[i] * kd
        dref, dbnd = dref + t, dbnd + np.abs(A[i] * A[i]) * kdb + 2 * np.abs(A[i] * kd) * dA[i] + 3 * U * np.abs(t) + U * np.abs(dref + t)
    tX = _on(X, "ld", dev)
    _within("K_diag", _np(kern.K_diag(tX)), dref, dbnd + TINY)
    _within("kdiag_rows", _np(spec.kdiag_rows(tX)), dref, dbnd + TINY)
    assert _same_bits(_np(kern(X, full_cov=False)), _np(spec.kdiag_rows(tX)))


def test_k_diag_is_the_diagonal_of_k_bit_for_bit(gp):
    """where every member's own K_diag is the diagonal of its matrix bit for bit -- the stationary members on the device, whose
    builders take the diagonal by index (the NumPy emulation of the stationary builder does not, so there the dot-product members
    stand in) -- K_diag and kdiag_rows are the diagonal of K(X, X): the weight a_r a_r is formed first on both sides.  C = 0 is the
    member's own matrix; a scalar steepness stands for all"""
    K = gp.kernels
    X = _data()["X1"]
    stationary = [K.SquaredExponential(variance=1.1, lengthscales=0.5), K.Matern32(variance=0.9, lengthscales=0.7, active_dims=[1, 2]),
                  K.Matern52(variance=0.7)]
    dots = [K.Linear(variance=[0.5, 2.0, 1.25]), K.Linear(variance=0.7, active_dims=[1, 2]), K.Constant(0.8)]
    holds = []
    for members in (stationary, dots):
        k = K.ChangePoints(members, [0.4, -0.3], 4.0)
        Kxx = _np(k(X))
        holds.append(all(_same_bits(_np(m(X, full_cov=False)), np.diag(_np(m(X)))) for m in members))
        if holds[-1]:
            assert _same_bits(_np(k(X, full_cov=False)), np.diag(Kxx)) and _same_bits(_np(_spec_of(k).kdiag_rows(gp.ops.to_device(X))), np.diag(Kxx))
    assert holds[1] and (holds[0] or _dev(gp) == "cpu"), holds
    same = K.ChangePoints(k.kernels, [-0.3, 0.4], [4.0, 4.0])
    assert _same_bits(_np(same(X)), Kxx), "a scalar steepness, or the order the locations are given in, changes the matrix"
    m = K.Matern32(variance=0.9, lengthscales=0.7)
    one = K.ChangePoints([m], [])
    assert _same_bits(_np(one(X, X[:70])), _np(m(X, X[:70]))) and _same_bits(_np(one(X, full_cov=False)), _np(m(X, full_cov=False)))


TREES = {
    "cp3": (CP3, CP3_KINDS),
    "cp+white": (("add", [("cp", ["se", "m32"], dict(locations=(0.1,), steepness=4.0)), "white"]),
                 {"se": _K["SquaredExponential"], "m32": _K["Matern32"], "white": _K["White"]}),
    "cp*const": (("mul", [("cp", [("add", ["se", "lin"]), "per"], dict(locations=(0.0,), steepness=(3.0,), switch_dim=1)), "const"]),
                 {"se": _K["SquaredExponential"], "lin": _K["Linear"], "per": _K["Periodic(SE)"], "const": _K["Constant"]}),
    "cp in cp": (("cp", [("cp", ["se", "m32"], dict(locations=(-0.4,), steepness=5.0, switch_dim=2)), "lin", "rq"],
                  dict(locations=(0.4, -0.2), steepness=(3.0, 6.0))),
                 {"se": _K["SquaredExponential"], "m32": _K["Matern32"], "lin": _K["Linear"], "rq": _K["RationalQuadratic"]}),
}


def _check_spec_grads(name, spec, pars, lv, dv, dl, route):
    """every member's variance and shape gradient, and the nodes' locations and steepness, against the leaves' .grad"""
    grads = spec.kernel_grads(*spec.pack(dv, dl))
    pairs = route.kernel_pairs(grads)
    seen = set()
    for par, g in pairs:
        key = [k for k, p in pars.items() if p is par][0]
        seen.add(key)
        ref = lv[key].grad
        ref = np.zeros(np.shape(par.numpy())) if ref is None else ref.numpy()
        _close(f"{name} {key}", np.asarray(g), ref.reshape(np.shape(g)), ADJ_TOL)
    assert seen == set(pars), (name, set(pars) - seen)
    return grads


@pytest.mark.parametrize("name", list(TREES))
def test_adjoint_against_autograd(gp, name):
    """KernelSpec.adjoint (symmetric and cross) and diag_adjoint against torch autograd of sum(Kbar .* K(A, B)) and of
    sum(kd_bar .* diag K): every member Parameter, every node's locations (in the GIVEN order) and steepness, and A_bar with the
    switch column's share; 130 x 70, no weight saturated"""
    dev, dat = _dev(gp), _data()
    tree, kinds = TREES[name]
    kern, pars = _make_tree(gp.kernels, tree, kinds)
    route = gp.models.reverse.CovarianceRoute(kern, 3)
    spec = route.spec
    for case, A, B, Kbar in (("symmetric", dat["X1"], None, dat["Ksym"]), ("cross", dat["X1"], dat["X2"], dat["Kbar"])):
        tA, tK = _on(A, "c", dev), _on(Kbar, "c", dev)
        tB = tA if B is None else _on(B, "c", dev)
        spec.warm(tA.device, 3)
        dv, dl, Abar = spec.adjoint(tA, tB, tK, B is None)
        lv = TR._leaves(pars, {"A": A})
        kfun, _ = _tree_torch(tree, kinds, lv)
        (_t(Kbar) * kfun(lv["A"], lv["A"] if B is None else _t(B))).sum().backward()
        _check_spec_grads(f"{name} {case}", spec, pars, lv, dv, dl, route)
        _close(f"{name} {case} A_bar", Abar, lv["A"].grad.numpy(), ADJ_TOL)
        _check_unchanged(name, [tA, tK], [A, Kbar])
    tX, tg = _on(dat["X1"], "c", dev), _on(dat["kd_bar"], "c", dev)
    spec.warm(tX.device, 3)
    dv, dl = spec.diag_adjoint(tX, tg)
    lv = TR._leaves(pars)
    _, kdiag = _tree_torch(tree, kinds, lv)
    (_t(dat["kd_bar"]) * kdiag(_t(dat["X1"]))).sum().backward()
    _check_spec_grads(f"{name} diagonal", spec, pars, lv, dv, dl, route)
    _check_unchanged(name, [tX, tg], [dat["X1"], dat["kd_bar"]])


def test_unsorted_locations_get_their_gradients_in_the_given_order(gp):
    """locations given as (0.4, -0.3): the device sees them sorted, steepness[j] goes with the j-th SORTED location (as the reference
    pairs them), and d/dlocations comes back in the given order"""
    dev, dat = _dev(gp), _data()
    K = gp.kernels
    mk = lambda loc, st: K.ChangePoints([K.SquaredExponential(lengthscales=0.5), K.Matern32(), K.Matern52(variance=0.6)], loc, st)  # noqa: E731
    given, srt = mk([0.4, -0.3], [3.0, 5.0]), mk([-0.3, 0.4], [3.0, 5.0])
    assert list(given.locations.numpy()) == [0.4, -0.3] and list(given.node().locations) == [-0.3, 0.4] and list(given.node().permutation) == [1, 0]
    tA, tB, tK = _on(dat["X1"], "c", dev), _on(dat["X2"], "c", dev), _on(dat["Kbar"], "c", dev)
    out = []
    for k in (given, srt):
        route = gp.models.reverse.CovarianceRoute(k, 3)
        route.spec.warm(tA.device, 3)
        dv, dl, _ = route.spec.adjoint(tA, tB, tK, False)
        g = route.spec.kernel_grads(*route.spec.pack(dv, dl))["changepoints"]
        assert len(g) == 1 and set(g[0]) == {"locations", "steepness"}
        out.append((_np(g[0]["locations"]), _np(g[0]["steepness"])))
    assert _same_bits(out[0][0], out[1][0][::-1]) and _same_bits(out[0][1], out[1][1]) and out[0][0][0] != out[0][0][1]
    pairs = gp.models.reverse.CovarianceRoute(given, 3)
    assert pairs.nodes == [(given.locations, given.steepness)]


# ------------------------------------------------------------------------------------------------ 6. models against autograd
D, M = 3, 16
MODEL_TREE = ("add", [("cp", ["se", "m32", "lin"], dict(locations=(0.4, -0.3), steepness=(3.0, 5.0))), "white"])
MODEL_KINDS = {"se": _K["SquaredExponential"].but(cols=[1, 2], lengthscales=[0.5, 0.7]), "m32": _K["Matern32"],
               "lin": _K["Linear"].but(cols=[1, 2], variance=[0.5, 1.25]), "white": _K["White"].but(variance=0.05)}
SCALAR_TREE = ("cp", ["se", "m32"], dict(locations=(0.1,), steepness=4.0))
HET_A, HET_B = np.array([[-0.1], [0.05], [0.02]]), np.array([0.6])


def _model(K, tree=MODEL_TREE):
    kern, pars = _make_tree(K, tree, MODEL_KINDS)
    return kern, pars, (lambda lv: _tree_torch(tree, MODEL_KINDS, lv))


def _perturbed(kfun, kdiag, seed=5):
    """the kernel and its diagonal with every entry moved by a relative 4 * 2^-52, signs random but fixed per shape"""
    signs = {}

    def sgn(shape):
        if shape not in signs:
            signs[shape] = torch.tensor(np.random.default_rng(seed + len(signs)).choice([-1.0, 1.0], size=shape))
        return signs[shape]
    return (lambda A, B: (lambda k: k * (1 + 4 * 2.0 ** -52 * sgn(tuple(k.shape))))(kfun(A, B))), \
        (lambda X: (lambda k: k * (1 + 4 * 2.0 ** -52 * sgn(tuple(k.shape))))(kdiag(X)))


def _vgp_q(N):
    rng = np.random.default_rng(33)
    return 0.3 * rng.normal(size=(N, 2)), np.stack([np.tril(0.05 * rng.normal(size=(N, N))) + 0.6 * np.eye(N) for _ in range(2)])


def _oracle_grads(problem, model, perturb, whiten=True, het=False):
    """{name: gradient} of the oracle for one model problem, with the kernel perturbed or not (the conditioning check)"""
    import gpflow_amd
    X, Y, Z, q_mu, q_sqrt = problem
    _, pars, tk = _model(gpflow_amd.kernels)
    lv = DK._leaves(pars, {"noise": 0.15, "mean": 0.2, "Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt})
    kfun, kdiag = tk(lv)
    if perturb:
        kfun, kdiag = _perturbed(kfun, kdiag)
    if model == "gpr":
        F = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=kfun)
    elif model == "vgp":
        qm, qs = _vgp_q(X.shape[0])
        lv["q_mu"], lv["q_sqrt"] = _leaf(qm), _leaf(qs)
        F = VG._torch_elbo("bernoulli_probit", (), _t(X), _t((Y > 0).astype(np.float64)), lv["q_mu"], lv["q_sqrt"], kfun, lv["mean"])
    else:
        noise = lv["noise"]
        if het:
            lv["A"], lv["b"] = _leaf(HET_A), _leaf(HET_B)
            noise = torch.clamp(_t(X) @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2
        F = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], lv["q_sqrt"], None, None, noise, num_data=1000, whiten=whiten,
                                 mean=lv["mean"], kfun=kfun, kdiag=kdiag(_t(X)))
    F.backward()
    return {k: t.grad.numpy().copy() for k, t in lv.items() if t.grad is not None}


def conditioning_figures():
    """{problem: the largest move of the oracle's gradients, in the measure of `_close`} -- CPU only; CONDITIONING_FIGURES records it"""
    problem = DK._problem(D, M)
    out = {}
    for name, model, kw in (("gpr", "gpr", {}), ("svgp", "svgp", {}), ("svgp heteroskedastic", "svgp", dict(het=True)), ("vgp bernoulli", "vgp", {})):
        worst = 0.0
        for whiten in ((True, False) if model == "svgp" else (True,)):
            a, b = _oracle_grads(problem, model, False, whiten, **kw), _oracle_grads(problem, model, True, whiten, **kw)
            worst = max([worst] + [float(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(a[k]).max())) for k in a])
        out[name] = worst
    return out


@pytest.mark.parametrize("which", ["tree", "scalar steepness"])
def test_gpr_vs_autograd_oracle(gp, which):
    """GPR.log_marginal_likelihood, _and_grad and predict_f, N = 40, a constant mean: every member Parameter, `locations` (given
    unsorted), `steepness` (per point, and one scalar for all), the noise and the mean constant"""
    gpflow = gp
    X, Y, _, _, _ = DK._problem(D, M)
    kern, pars, tk = _model(gpflow.kernels, MODEL_TREE if which == "tree" else SCALAR_TREE)
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.2))
    v, g = m.log_marginal_likelihood_and_grad()
    lv = DK._leaves(pars, {"noise": 0.15, "mean": 0.2})
    kfun, kdiag = tk(lv)
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=kfun)
    Fo.backward()
    DK._agree(f"gpr {which}", v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    allp = dict(pars, noise=m.likelihood.variance, mean=m.mean_function.c)
    _check_model_grads(f"gpr {which}", g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values())
    Xn = np.random.default_rng(4).uniform(-1, 1, size=(7, D))
    with torch.no_grad():
        tX, tn = _t(X), _t(Xn)
        Kxx = kfun(tX, tX).numpy() + 0.15 * np.eye(X.shape[0])
        Kxn, Knn, kd = kfun(tX, tn).numpy(), kfun(tn, tn).numpy(), kdiag(tn).numpy()
    sol = np.linalg.solve(Kxx, Kxn)
    close = lambda a, b: np.abs(_np(a) - b).max() <= 1e-9 * max(1.0, np.abs(b).max())   # noqa: E731
    mu, var = m.predict_f(Xn, full_cov=True)
    assert close(mu, sol.T @ (Y - 0.2) + 0.2) and close(var[0], Knn - Kxn.T @ sol)
    mu, var = m.predict_f(Xn)
    assert close(var[:, 0], kd - (Kxn * sol).sum(0))


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_vs_autograd_oracle(gp, whiten, q_diag):
    """SVGP.elbo (composed: the posterior) and elbo_and_grad in the four parametrisations, num_data = 1000 against B = 40: the member
    Parameters, `locations`, `steepness`, Z (its switch column included), q_mu, q_sqrt, the noise and the mean constant"""
    kern, pars, tk = _model(gp.kernels)
    DK._svgp_check(gp, "svgp changepoints", kern, pars, tk, DK._problem(D, M), whiten=whiten, q_diag=q_diag)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_heteroskedastic_and_shared_vs_autograd_oracle(gp, whiten):
    """Gaussian(scale=Linear(A, b)): dF/d sigma_n^2 per row takes the rows of the diagonal; and the kernel shared through
    SharedIndependent over SharedIndependentInducingVariables, forward (the reverse pass takes a combination as the model's own kernel)"""
    gpflow = gp
    kern, pars, tk = _model(gpflow.kernels)
    lik = gpflow.likelihoods.Gaussian(scale=gpflow.functions.Linear(A=HET_A.copy(), b=HET_B.copy()))

    def noise_of(lv, X):
        return torch.clamp(X @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2
    DK._svgp_check(gpflow, "svgp heteroskedastic", kern, pars, tk, DK._problem(D, M), whiten=whiten, q_diag=False, lik=lik,
                   lik_pars={"A": lik.scale.A, "b": lik.scale.b}, noise_of=noise_of)
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    IV = gpflow.inducing_variables
    plain = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten, num_latent_gps=2)
    shared = gpflow.models.SVGP(gpflow.kernels.SharedIndependent(kern, 2), gpflow.likelihoods.Gaussian(0.2),
                                IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy())), q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten,
                                num_latent_gps=2)
    assert shared._fused_config() is None
    a, b = float(plain.elbo((X, Y)).cpu()), float(shared.elbo((X, Y)).cpu())
    assert abs(a - b) <= 1e-12 * abs(a), (a, b)


def test_vgp_bernoulli_vs_autograd(gp):
    """VGP with a Bernoulli likelihood and a constant mean: value, forward ELBO, and every gradient against autograd of the restated ELBO"""
    gpflow = gp
    X, Y, _, _, _ = DK._problem(D, M)
    Yb = (Y > 0).astype(np.float64)
    kern, pars, tk = _model(gpflow.kernels)
    m = gpflow.models.VGP((X, Yb), kern, gpflow.likelihoods.Bernoulli(), mean_function=gpflow.mean_functions.Constant(0.2))
    q_mu, q_sqrt = _vgp_q(X.shape[0])
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    v, g = m.objective_and_grad()
    lv = DK._leaves(pars, {"q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.2})
    Fo = VG._torch_elbo("bernoulli_probit", (), _t(X), _t(Yb), lv["q_mu"], lv["q_sqrt"], tk(lv)[0], lv["mean"])
    Fo.backward()
    DK._agree("vgp", v, float(Fo.detach()), float(m.elbo()))
    allp = dict(pars, q_mu=m.q_mu, mean=m.mean_function.c)
    _check_model_grads("vgp", g, allp, lv, GRAD_TOL)
    ref = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
    _close("vgp q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(ref).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)
    assert set(g) == set(allp.values()) | {m.q_sqrt}


def test_predict_f_in_the_four_covariance_forms(gp):
    """SVGP.predict_f and the cached posterior, full_cov x full_output_cov, whitened and not, against a NumPy restatement"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    kern, pars, tk = _model(gpflow.kernels)
    kfun, kdiag = tk({k: _t(p.numpy()) for k, p in pars.items()})
    Xn = np.random.default_rng(4).uniform(-1, 1, size=(7, D))
    tZ, tn = _t(Z), _t(Xn)
    Kmm = kfun(tZ, tZ).numpy() + 1e-6 * np.eye(M)
    Kmn, Knn, Kd = kfun(tZ, tn).numpy(), kfun(tn, tn).numpy(), kdiag(tn).numpy()
    close = lambda a, b: np.abs(_np(a) - b).max() <= 1e-9 * max(1.0, np.abs(b).max())   # noqa: E731
    for whiten in (True, False):
        m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten, num_latent_gps=2)
        mean, var = DK._posterior_np(Kmm, Kmn, Kd, q_mu, q_sqrt, whiten, False)
        _, cov = DK._posterior_np(Kmm, Kmn, Knn, q_mu, q_sqrt, whiten, True)
        for post in (None, m.posterior()):
            f = (lambda **kw: m.predict_f(Xn, **kw)) if post is None else (lambda **kw: post.predict_f(Xn, **kw))
            mu, v = f()
            assert close(mu, mean) and close(v, var), (whiten, post is None)
            mu, v = f(full_cov=True)
            assert close(mu, mean) and close(v, cov)
            mu, v = f(full_output_cov=True)
            assert close(v, np.stack([np.diag(r) for r in var]))
            mu, v = f(full_cov=True, full_output_cov=True)
            assert tuple(v.shape) == (7, 2, 7, 2) and close(v[:, 0, :, 0], cov[0]) and close(v[:, 1, :, 1], cov[1]) and close(v[:, 0, :, 1], 0 * cov[0])


def test_scipy_moves_the_change_point(gp):
    """ten optimizers.Scipy iterations on a GPR whose data have a variance jump at 0: the objective at the accepted iterates decreases
    monotonically, and `locations` and `steepness` move"""
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(10)
    X = np.sort(rng.uniform(-1.0, 1.0, size=(60, 1)), axis=0)
    Y = np.where(X < 0.0, 0.1, 1.0) * np.sin(12.0 * X) + 0.05 * rng.normal(size=(60, 1))
    k = K.ChangePoints([K.SquaredExponential(variance=0.3, lengthscales=0.3), K.SquaredExponential(variance=0.3, lengthscales=0.3)], [0.4], 5.0)
    m = gpflow.models.GPR((X, Y), k, noise_variance=0.1)
    seen, inner = [], m.objective_and_grad

    def logged():
        v, g = inner()
        seen.append((np.concatenate([np.ravel(p.unconstrained_variable) for p in g]).copy(), -float(v)))
        return v, g
    m.objective_and_grad = logged
    accepted = []

    def callback(xk):
        accepted.append([f for x, f in seen if np.array_equal(x, xk)][-1])
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=10), callback=callback)
    del m.objective_and_grad
    after = -float(m.log_marginal_likelihood().cpu())
    assert len(accepted) >= 2 and all(b < a for a, b in zip([before] + accepted, accepted)), (before, accepted)
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert abs(float(k.locations.numpy()[0]) - 0.4) > 1e-3 and abs(float(k.steepness.numpy()) - 5.0) > 1e-4


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals(gp):
    """before anything touches a device: the constructor, and every model route that takes K_diag for one scalar -- each by the
    limit it breaks, with the message the row-diagonal leaves get"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    from gpflow_amd.models.reverse import has_row_diagonal
    se = K.SquaredExponential
    with pytest.raises(ValueError, match="locations"):
        K.ChangePoints([se(), se()], [0.0, 1.0])
    with pytest.raises(ValueError, match="locations"):
        K.ChangePoints([se(), se(), se()], [0.0])
    with pytest.raises(ValueError, match="steepness"):
        K.ChangePoints([se(), se(), se()], [0.0, 1.0], [1.0])
    with pytest.raises(ValueError, match="switch_dim"):
        K.ChangePoints([se(), se()], [0.0], switch_dim=-1)
    with pytest.raises(NotImplementedError, match="16"):
        K.ChangePoints([se() for _ in range(17)], np.linspace(-1, 1, 16))
    with pytest.raises(TypeError):
        K.ChangePoints([se(), "x"], [0.0])
    with pytest.raises(Exception):
        K.ChangePoints([se(), se()], [0.0], steepness=-1.0)                               # positive()
    assert len(K.ChangePoints([se() for _ in range(16)], np.linspace(-1, 1, 15)).kernels) == 16
    cp = K.ChangePoints([se(), K.Matern32()], [0.1], 3.0)
    nested = K.ChangePoints([cp, se()], [0.5])
    assert nested.kernels[0] is cp and len(nested.kernels) == 2 and cp._op == "cp"        # not flattened
    assert isinstance(cp + K.White(), K.Sum) and isinstance(cp * K.Constant(), K.Product) and "ChangePoints" in K.__all__
    assert {cp.locations, cp.steepness} <= set(cp.trainable_parameters) and len(list(cp.trainable_parameters)) == 6
    assert has_row_diagonal(cp) and has_row_diagonal(cp + K.White()) and has_row_diagonal(K.SharedIndependent(cp, 2)) and not has_row_diagonal(se() + se())
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    with pytest.raises(ValueError, match="switch_dim"):
        K.ChangePoints([se(), se()], [0.0], switch_dim=3).K_into(torch.zeros((4, 3), dtype=torch.float64), None, None)
    lik = gpflow.likelihoods.Gaussian(0.2)
    for k in (cp, cp + K.White()):
        with pytest.raises(NotImplementedError, match="SGPR"):
            gpflow.models.SGPR((X, Y), k, Z.copy()).elbo()
        with pytest.raises(NotImplementedError, match="SGPR"):
            gpflow.models.SGPR((X, Y), k, Z.copy()).objective_and_grad()
        m = gpflow.models.SVGP(k, lik, Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2)
        assert m._fused_config() is None
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(m)
        with pytest.raises(NotImplementedError, match="natural gradients"):
            gpflow.optimizers.NaturalGradient(gamma=0.5).minimize(m, (X, Y))
        mb = gpflow.models.SVGP(k, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1])
        with pytest.raises(NotImplementedError, match="quadrature"):
            mb.elbo_and_grad((X, (Y[:, :1] > 0).astype(np.float64)))
    iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))
    for kern in (K.SeparateIndependent([cp, se()]), K.LinearCoregionalization([se(), cp], W=np.eye(2))):
        m = gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2)
        assert m._fused_separate_config() is None and m._fused_lcm_config() is None
        with pytest.raises(NotImplementedError, match="per-latent"):
            m.elbo_and_grad((X, Y))
    from gpflow_amd import gradients
    from gpflow_amd.leaf import Leaf
    leaves = [Leaf("SquaredExponential", 1.0, 0.5), Leaf("Matern32", 1.0, 0.5)]
    node = gradients.ChangePointsNode([0.1], 3.0)
    spec = gradients.KernelSpec(leaves, ("cp", [0, 1], 0), nodes=[node])
    assert not spec.constant_diagonal and not spec.packable
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.kdiag()
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.dkdiag()
    with pytest.raises(ValueError, match="one child per regime"):
        gradients.KernelSpec(leaves, ("cp", [0, 1], 0), nodes=[gradients.ChangePointsNode([0.1, 0.2], 3.0)])
    with pytest.raises(ValueError):
        gradients.KernelSpec(leaves, ("cp", [0, 1], 1), nodes=[node])
    with pytest.raises(ValueError):
        gradients.ChangePointsNode([0.1, 0.2], [3.0])
    with pytest.raises(ValueError):
        gradients.ChangePointsNode([0.1], 3.0, switch_dim=-1)
    with pytest.raises(NotImplementedError):
        gradients.ChangePointsNode(np.linspace(0, 1, 16), 3.0)
    one = gradients.KernelSpec(leaves[:1], ("cp", [0], 0), nodes=[gradients.ChangePointsNode([], 1.0)])
    assert one.tree == ("cp", [0], 0) and not one.packable
    plain = gradients.KernelSpec(leaves, "add")
    assert plain.nodes == [] and "changepoints" not in plain.kernel_grads(torch.zeros(2), [torch.zeros(1), torch.zeros(1)])
