"""GPU tests of the dot-product kernels: the four primitives of gpflow_amd/csrc/dot.hip (`ops.dot_kernel_matrix`, `dot_kernel_matrix_combine`,
`dot_kernel_diag`, `dot_adjoint_tail`), `kernels.Linear` / `kernels.Polynomial` on every forward route, and the reverse pass of GPR and
SVGP with a diagonal that depends on the row.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_dot_kernels_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture).  On the device every primitive case also runs the emulation beside it (`_impls`).

References.  Primitives: np.longdouble evaluations of the direct formula, the bound derived next to each (u = 2^-53).  Models: torch
under autograd (oracle/gp_oracle_grad.py through its `kfun=` / `kdiag=` hooks, kdiag the per-row tensor of the batch) or a NumPy
restatement; values 1e-9 relative, gradients 1e-8 through `_check_model_grads` -- the project's figures for the families evaluated on r2.

Condition of the model problems.  Kuu of a pure Linear kernel has rank D, so the shapes are those at which the reference itself is
stable: B = 40, P = 2, inputs uniform in [-1, 1], Linear ARD at D = 6, M = 5 and everything else at D = 3, M = 16 (a SquaredExponential
member has l = 0.5).  Every kernel entry -- and every entry of the row diagonal -- of the problems below (`_problem`, their seeds) was
perturbed by a relative 4 * 2^-52 with random signs, in torch on the CPU; the oracle's own gradients (GPR, and SVGP whitened or not,
full or diagonal q_sqrt; every leaf) moved by at most, in the measure of `_close`: Linear ARD 3.6e-13, Polynomial(3) 1.6e-12,
SE + Linear 1.6e-13, SE * Linear 1.6e-14, SE * Polynomial(2) 3.0e-14, (SE + Linear) * Matern32 1.4e-14, SE + Linear(active_dims)
1.4e-13, Linear ARD under the heteroskedastic likelihood 3.7e-13 -- at least 6000 times below the 1e-8 tolerance.  A new shape or
seed needs that check repeated.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_dot_ops  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _padding_untouched, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t, _torch_kernel  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

VALUE_TOL, GRAD_TOL = 1e-9, 1e-8
TINY = LD(1e-300)


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


class _Emulation:
    dot_kernel_matrix = staticmethod(fake_dot_ops.dot_kernel_matrix)
    dot_kernel_matrix_combine = staticmethod(fake_dot_ops.dot_kernel_matrix_combine)
    dot_kernel_diag = staticmethod(fake_dot_ops.dot_kernel_diag)
    dot_adjoint_tail = staticmethod(fake_dot_ops.dot_adjoint_tail)


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", _Emulation, "cpu")] if dev != "cpu" else [])


# ------------------------------------------------------------------------------------------------ references
LEAVES = [("Linear", None)] + [("Polynomial", deg) for deg in (1, 2, 3, 7, 16)]
OFFSET = 0.3          # with inputs in [-1, 1] and weights in [0.5, 2]: s < -0.3 for many pairs, so base < 0 at the odd degrees


def _kw(family, degree, w):
    return dict(family=family, variance=w) if family == "Linear" else dict(family=family, variance=w, offset=OFFSET, degree=degree)


def _weights(ard, d):
    return 0.5 + 1.5 * ((np.arange(d) * 7) % 11) / 10.0 if ard else 1.3


def _sref(X1, X2, w):
    """s = sum_j w_j a_j b_j in longdouble, and the bound of the device's evaluation: x w is rounded once (u |w a b| per term) and the
    fma chain over the d columns adds at most d u sum_j |w_j a_j b_j| (term j passes through d - j + 1 <= d roundings) -- in all
    (d + 1) u T, T = sum_j |w_j a_j b_j|, taken as gamma = k u / (1 - k u) for the higher orders."""
    d = X1.shape[1]
    wl = np.broadcast_to(np.asarray(w, dtype=LD), (d,))
    terms = X1.astype(LD)[:, None, :] * wl * X2.astype(LD)[None, :, :]
    T = np.abs(terms).sum(-1)
    k = (d + 1) * LD(U)
    return terms.sum(-1), k / (1 - k) * T + TINY


def _power(base, n):
    p = np.ones_like(base)
    for _ in range(n):
        p = p * base
    return p


def _kref(family, degree, s, ds, what="k", offset=OFFSET):
    """(k or dk/ds in longdouble, bound) from s and its bound ds.  Linear: k = s, dk/ds = 1 exactly.  Polynomial: base = s + offset
    carries one more rounding, e = ds + u |base|; |base^n - (base + e')^n| <= (|base| + e)^n - |base|^n for |e'| <= e -- to first order
    the n |base|^(n-1) e of the derivation, the remainder being all there is where base is near 0 -- and the n - 1 products of the power
    add (n - 1) u |k|; dk/ds = degree base^(degree - 1): the same with n = degree - 1, and one more product for the factor `degree`."""
    if family == "Linear":
        return (s, ds) if what == "k" else (np.ones_like(s), np.zeros_like(s))
    base = s + LD(offset)            # (offset=: the value a caller's Parameter holds, where that is not OFFSET to the bit)
    e = ds + U * np.abs(base)
    n = degree if what == "k" else degree - 1
    if n == 0:
        return np.ones_like(s), np.zeros_like(s)
    val = _power(base, n)
    bnd = _power(np.abs(base) + e, n) - _power(np.abs(base), n) + (n - 1) * U * (np.abs(val) + _power(np.abs(base) + e, n) - _power(np.abs(base), n))
    if what == "ds":
        val, bnd = degree * val, degree * bnd + U * np.abs(degree * val)
    return val, bnd + TINY


# ------------------------------------------------------------------------------------------------ 1. the builder
BUILD_CASES = [(1, 1, 1), (63, 65, 3), (64, 64, 64), (130, 70, 5)]   # smallest; a partial tile each way; full tile at GPK_MAX_D (64 KB LDS); ragged tiles
LAYOUTS = ["c", "ld", "off", "pad"]                                    # "ld" / "off": odd ldk / misaligned K, the scalar-store path


def _inputs(n1, n2, d, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, size=(n1, d)), rng.uniform(-1.0, 1.0, size=(n2, d))


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n1,n2,d", BUILD_CASES)
def test_dot_kernel_matrix(gp, n1, n2, d, layout, ard):
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    w = _weights(ard, d)
    s, ds = _sref(X1, X2, w)
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "ld", dev), _on(X2, "pad" if layout == "c" else "c", dev)
        for family, degree in LEAVES:
            ref, bnd = _kref(family, degree, s, ds)
            out, buf = _on(np.full((n1, n2), -555.0), layout, dev, base=True)
            got = impl.dot_kernel_matrix(t1, t2, out=out, diag_add=9.0, **_kw(family, degree, w))   # (diag_add: ignored with X2 given)
            name = f"dot_kernel_matrix {who} {family} {degree}"
            assert got is out and _padding_untouched(out, buf), f"{name}: padding written"
            _within(name, _np(out), ref, bnd)
            if family == "Polynomial" and degree in (3, 7) and n1 > 1:
                assert (ref < 0).any(), "the data must reach base < 0 at an odd degree"
        _check_unchanged(f"dot_kernel_matrix {who}", [t1, t2], [X1, X2])
        fresh = impl.dot_kernel_matrix(t1.contiguous(), t2.contiguous(), **_kw("Polynomial", 3, w))
        assert _same_bits(_np(fresh), _np(impl.dot_kernel_matrix(t1, t2, **_kw("Polynomial", 3, w)))), f"{who}: the layout of X changes the result"


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dot_kernel_matrix_symmetric(gp, layout, ard):
    """129 x 129, d = 4 (three tile rows, the last one a single row): K(X, X) + diag_add I is EXACTLY symmetric (the mirror), a
    lower_only build has bit for bit the lower triangle of the full one, and nothing outside the view is written"""
    n, d = 129, 4
    X, _ = _inputs(n, 1, d, 77)
    w = _weights(ard, d)
    s, ds = _sref(X, X, w)
    eye = np.eye(n, dtype=LD)
    for who, impl, dev in _impls(gp):
        tX = _on(X, "col", dev)
        for family, degree in LEAVES:
            ref, bnd = _kref(family, degree, s, ds)
            name = f"symmetric {who} {family} {degree}"
            out, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
            impl.dot_kernel_matrix(tX, None, out=out, diag_add=0.25, **_kw(family, degree, w))
            Kf = _np(out).copy()
            assert _padding_untouched(out, buf), f"{name}: padding written"
            assert _same_bits(Kf, Kf.T), f"{name}: not exactly symmetric"
            _within(name, np.tril(Kf), np.tril(ref + LD(0.25) * eye), np.tril(bnd + U * np.abs(ref + 0.25) * eye))
            low, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
            impl.dot_kernel_matrix(tX, None, out=low, diag_add=0.25, lower_only=True, **_kw(family, degree, w))
            assert _padding_untouched(low, buf) and _same_bits(np.tril(_np(low)), np.tril(Kf)), f"{name}: lower_only differs from the full build"
            plain = _np(impl.dot_kernel_matrix(tX, None, **_kw(family, degree, w)))
            assert _same_bits(plain - np.diag(np.diag(plain)), Kf - np.diag(np.diag(Kf))), f"{name}: diag_add reached off the diagonal"
        _check_unchanged(f"symmetric {who}", [tX], [X])


@pytest.mark.parametrize("symmetric", [False, True], ids=["130x70", "symmetric129"])
@pytest.mark.parametrize("layout", ["c", "ld", "off"])
def test_dot_kernel_matrix_combine(gp, layout, symmetric):
    """ops mul / add / ds with `out` aliasing G (and not); diag_add lands on the diagonal of the COMBINED result; "ds" with X2 = None
    does NOT zero the diagonal (s_ii depends on the parameters)"""
    n1, n2, d = (129, 129, 4) if symmetric else (130, 70, 5)
    X1, X2 = _inputs(n1, n2, d, 5 + symmetric)
    X2 = X1 if symmetric else X2
    rng = np.random.default_rng(6)
    G = rng.normal(size=(n1, n2))
    w = _weights(True, d)
    s, ds = _sref(X1, X2, w)
    eye = np.eye(n1, n2, dtype=LD) if symmetric else 0
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "c", dev), (None if symmetric else _on(X2, "ld", dev))
        for family, degree in LEAVES:
            kw = _kw(family, degree, w)
            k, kb = _kref(family, degree, s, ds)
            dk, dkb = _kref(family, degree, s, ds, "ds")
            Gl = G.astype(LD)
            want = {"mul": (Gl * k + 0.5 * eye, np.abs(Gl) * kb + U * np.abs(Gl * k) + U * np.abs(Gl * k + 0.5) * eye),
                    "add": (Gl + k + 0.5 * eye, kb + U * np.abs(Gl + k) + U * np.abs(Gl + k + 0.5) * eye),
                    "ds": (Gl * dk, np.abs(Gl) * dkb + U * np.abs(Gl * dk))}
            for op, (ref, bnd) in want.items():
                name = f"combine {who} {family} {degree} {op}"
                tG, buf = _on(G, layout, dev, base=True)
                got = impl.dot_kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.5, out=tG, **kw)      # in place
                assert got is tG and _padding_untouched(tG, buf), f"{name}: padding written"
                _within(name, _np(tG), ref, bnd + TINY)
                tG2 = _on(G, "pad", dev)
                sep = impl.dot_kernel_matrix_combine(t1, t2, tG2, op=op, diag_add=0.5, **kw)             # a fresh output
                assert _same_bits(_np(sep), _np(tG)), f"{name}: aliasing changes the result"
                _check_unchanged(name, [tG2], [G])
            if symmetric and family == "Polynomial" and degree == 3:
                dsd = np.diag(_np(impl.dot_kernel_matrix_combine(t1, None, _on(G, "c", dev), op="ds", **kw)))
                assert np.all(dsd != 0.0), "op ds must not zero the diagonal"
        _check_unchanged(f"combine {who}", [t1] + ([] if symmetric else [t2]), [X1] + ([] if symmetric else [X2]))


# ------------------------------------------------------------------------------------------------ 2. the row diagonal
@pytest.mark.parametrize("d", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 63, 257])
def test_dot_kernel_diag(gp, n, d):
    """all four ops over a padded ldx; within the builder's own bound of the direct formula, and -- the sums being the builder's -- the
    diagonal of the built K(X, X) bit for bit"""
    X, _ = _inputs(n, 1, d, 9 * n + d)
    g = np.random.default_rng(n + d).normal(size=n)
    for ard in (False, True):
        w = _weights(ard, d)
        wl = np.broadcast_to(np.asarray(w, dtype=LD), (d,))
        terms = X.astype(LD) * wl * X.astype(LD)
        s, ds = terms.sum(-1), (d + 1) * U / (1 - (d + 1) * U) * np.abs(terms).sum(-1) + TINY
        for who, impl, dev in _impls(gp):
            tX = _on(X, "pad", dev)
            for family, degree in LEAVES:
                kw = _kw(family, degree, w)
                k, kb = _kref(family, degree, s, ds)
                dk, dkb = _kref(family, degree, s, ds, "ds")
                name = f"dot_kernel_diag {who} {family} {degree}"
                kd = _np(impl.dot_kernel_diag(tX, **kw))
                _within(name + " k", kd, k, kb)
                assert _same_bits(kd, np.diag(_np(impl.dot_kernel_matrix(tX, None, **kw)))), f"{name}: differs from the diagonal of K(X, X)"
                gl = g.astype(LD)
                for op, ref, bnd in (("mul", gl * k, np.abs(gl) * kb + U * np.abs(gl * k)), ("add", gl + k, kb + U * np.abs(gl + k)),
                                     ("ds", gl * dk, np.abs(gl) * dkb + U * np.abs(gl * dk))):
                    tg = _on(g, "c", dev)
                    got = impl.dot_kernel_diag(tX, tg, op=op, out=tg, **kw)                               # out aliases g
                    assert got is tg
                    _within(f"{name} {op}", _np(tg), ref, bnd + TINY)
                    tg2 = _on(g, "c", dev)
                    assert _same_bits(_np(impl.dot_kernel_diag(tX, tg2, op=op, **kw)), _np(tg)) and _same_bits(_np(tg2), g)
            _check_unchanged(f"dot_kernel_diag {who}", [tX], [X])


# ------------------------------------------------------------------------------------------------ 3. the adjoint tail
@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["cross", "symmetric"])
@pytest.mark.parametrize("d", [1, 3, 64])
@pytest.mark.parametrize("n1", [1, 255, 513])
def test_dot_adjoint_tail(gp, n1, d, symmetric, ard):
    """the three formulas of include/gpk.h in longdouble.  d/dw_j = sum_i a_ij R_i,1+j: n1 products and a sum of n1 terms in some fixed
    order, every term through at most n1 + 1 roundings: (n1 + 1) u sum_i |a R|; one weight: the d column sums add (d - 1) u of their
    magnitudes.  d/doffset = sum_i R_i0: (n1 - 1) u sum |R_i0|.  A_bar = w R (one product; the factor 2 is exact): u |w R|.  A second
    call is bit-identical."""
    rng = np.random.default_rng(17 * n1 + d + symmetric)
    A = rng.uniform(-1.0, 1.0, size=(n1, d))
    R = rng.normal(size=(n1, 1 + 2 * d))                       # as wide as G moment_rows(B)^T: the B^2 columns are not read
    w = np.atleast_1d(_weights(ard, d)).astype(np.float64)
    Al, Rl, wl = A.astype(LD), R.astype(LD), np.broadcast_to(w.astype(LD), (d,))
    dw, dwb = (Al * Rl[:, 1:1 + d]).sum(0), (n1 + 1) * U * np.abs(Al * Rl[:, 1:1 + d]).sum(0)
    if w.size == 1:
        dw, dwb = dw.sum().reshape(1), (dwb.sum() + (d - 1) * U * np.abs(Al * Rl[:, 1:1 + d]).sum()).reshape(1)
    doff, doffb = Rl[:, 0].sum().reshape(1), ((n1 - 1) * U * np.abs(Rl[:, 0]).sum()).reshape(1)
    Abar = (2 if symmetric else 1) * wl * Rl[:, 1:1 + d]
    for who, impl, dev in _impls(gp):
        tR, tA, tw = _on(R, "ld", dev), _on(A, "pad", dev), _on(w, "c", dev)
        runs = [tuple(_np(x).copy() for x in impl.dot_adjoint_tail(tR, tA, tw, symmetric=symmetric)) for _ in range(2)]
        name = f"dot_adjoint_tail {who}"
        assert all(_same_bits(a, b) for a, b in zip(*runs)), f"{name}: two runs differ"
        _within(name + " d/dw", runs[0][0], dw, dwb + TINY)
        _within(name + " d/doffset", runs[0][1], doff, doffb + TINY)
        _within(name + " A_bar", runs[0][2], Abar, U * np.abs(Abar) + TINY)
        _check_unchanged(name, [tR, tA, tw], [R, A, w])


# ------------------------------------------------------------------------------------------------ 4. NaN / Inf
@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_dot_nonfinite_rows_propagate_as_through_a_matmul(gp, bad):
    """a NaN / Inf in row i of X1 makes row i of K non-finite and leaves every other row finite; in the symmetric build column i as
    well; the row diagonal likewise.  Padding rows are staged as zeros: a NaN in the last row of a partial tile stays in its row."""
    n1, n2, d = 70, 66, 3
    X1, X2 = _inputs(n1, n2, d, 3)
    X1[5, 1] = bad
    X1[69, 2] = bad
    rows = np.zeros(n1, dtype=bool)
    rows[[5, 69]] = True
    w = _weights(True, d)
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "c", dev), _on(X2, "c", dev)
        for family, degree in (("Linear", None), ("Polynomial", 3)):
            kw = _kw(family, degree, w)
            K = _np(impl.dot_kernel_matrix(t1, t2, **kw))
            assert np.array_equal(~np.isfinite(K), np.broadcast_to(rows[:, None], K.shape)), f"{who} {family}: cross"
            Ks = _np(impl.dot_kernel_matrix(t1, None, **kw))
            assert np.array_equal(~np.isfinite(Ks), rows[:, None] | rows[None, :]), f"{who} {family}: symmetric"
            G = _on(np.ones((n1, n2)), "c", dev)
            for op in ("mul", "add", "ds") if family == "Polynomial" else ("mul", "add"):
                C = _np(impl.dot_kernel_matrix_combine(t1, t2, G, op=op, **kw))
                assert np.array_equal(~np.isfinite(C), np.broadcast_to(rows[:, None], C.shape)), f"{who} {family} {op}"
            assert np.array_equal(~np.isfinite(_np(impl.dot_kernel_diag(t1, **kw))), rows), f"{who} {family}: diagonal"
            if np.isnan(bad):
                assert np.isnan(K[rows]).all() and np.isnan(Ks[rows]).all()
        _check_unchanged(f"nonfinite {who}", [t1, t2], [X1, X2])


# ------------------------------------------------------------------------------------------------ 5. the kernel classes, forward
def _lin_np(X, X2, w, offset=None, degree=None, cols=None):
    """NumPy restatement of gpflow/kernels/linears.py: (X * variance) X2^T, then (. + offset)^degree; X2 None: K(X, X)"""
    X2 = X if X2 is None else X2
    if cols is not None:
        X, X2 = X[:, cols], X2[:, cols]
    s = (X * w) @ X2.T
    return s if degree is None else (s + offset) ** degree


def test_kernel_classes_forward(gp):
    """K, K_into, K_diag, active_dims, batch dimensions, and a dot member inside Sum / Product folded in place"""
    gpflow = gp
    K = gpflow.kernels
    from gpflow_amd.kernels.base import is_device_leaf, is_dot_leaf
    rng = np.random.default_rng(12)
    X, X2 = rng.uniform(-1, 1, size=(40, 4)), rng.uniform(-1, 1, size=(30, 4))
    lin = K.Linear(variance=[0.5, 2.0], active_dims=[3, 1])
    pol = K.Polynomial(3, variance=0.7, offset=0.4)
    assert is_dot_leaf(lin) and is_dot_leaf(pol) and not is_device_leaf(lin) and not is_device_leaf(pol) and lin.ard and not pol.ard
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()   # noqa: E731
    assert rel(_np(lin(X, X2)), _lin_np(X, X2, [0.5, 2.0], cols=[3, 1])) < 1e-14
    assert rel(_np(pol(X, X2)), _lin_np(X, X2, 0.7, 0.4, 3)) < 1e-14
    for k, ref in ((lin, _lin_np(X, None, [0.5, 2.0], cols=[3, 1])), (pol, _lin_np(X, None, 0.7, 0.4, 3))):
        Kxx = _np(k(X))
        assert rel(Kxx, ref) < 1e-14 and _same_bits(Kxx, Kxx.T)
        assert _same_bits(_np(k(X, full_cov=False)), np.diag(Kxx))                                # the row diagonal, on the device
        Xs = k.slice(gpflow.ops.to_device(X), None)[0]
        assert _same_bits(_np(k.K_into(Xs, None, None, diag_add=0.5)), Kxx + 0.5 * np.eye(40))
        assert tuple(k.K_diag(gpflow.ops.to_device(X).reshape(2, 20, 4)[..., :Xs.shape[1]]).shape) == (2, 20)
    Kb = _np(pol.K(gpflow.ops.to_device(X).reshape(2, 20, 4), gpflow.ops.to_device(X2)))
    assert Kb.shape == (2, 20, 30) and _same_bits(Kb.reshape(40, 30), _np(pol(X, X2)))
    se = K.SquaredExponential(variance=1.1, lengthscales=0.5)
    kse = _np(se(X, X2))
    assert rel(_np((se + lin)(X, X2)), kse + _lin_np(X, X2, [0.5, 2.0], cols=[3, 1])) < 1e-14
    assert rel(_np((se * pol)(X, X2)), kse * _lin_np(X, X2, 0.7, 0.4, 3)) < 1e-14
    assert rel(_np((lin + se)(X, X2)), kse + _lin_np(X, X2, [0.5, 2.0], cols=[3, 1])) < 1e-14         # a dot member first
    nested = (se + lin) * K.Matern32(variance=0.9, lengthscales=0.7)
    kd = _np(nested(X, full_cov=False))
    assert rel(kd, (1.1 + (X[:, [3, 1]] ** 2 * [0.5, 2.0]).sum(1)) * 0.9) < 1e-14 and rel(kd, np.diag(_np(nested(X)))) < 1e-14
    # the covariance dispatchers
    iv = gpflow.inducing_variables.InducingPoints(X2.copy())
    assert rel(_np(gpflow.covariances.Kuf(iv, lin, X)), _lin_np(X2, X, [0.5, 2.0], cols=[3, 1])) < 1e-14
    assert rel(_np(gpflow.covariances.Kuu(iv, pol, jitter=1e-3)), _lin_np(X2, None, 0.7, 0.4, 3) + 1e-3 * np.eye(30)) < 1e-14


# ------------------------------------------------------------------------------------------------ 6. models against autograd
def _lin_torch(w, offset=None, degree=None, cols=None):
    """torch restatement of linears.py: (kfun(A, B), kdiag(X))"""
    def kfun(A, B):
        if cols is not None:
            A, B = A[:, cols], B[:, cols]
        s = (A * w) @ B.T
        return s if degree is None else (s + offset) ** degree

    def kdiag(X):
        if cols is not None:
            X = X[:, cols]
        s = (X * X * w).sum(1)
        return s if degree is None else (s + offset) ** degree
    return kfun, kdiag


def _mk_linear(K):
    k = K.Linear(variance=0.5 + 0.25 * np.arange(6))
    return k, {"variance": k.variance}, lambda lv: _lin_torch(lv["variance"])


def _mk_poly3(K):
    k = K.Polynomial(3.0, variance=0.7, offset=0.4)
    return k, {"variance": k.variance, "offset": k.offset}, lambda lv: _lin_torch(lv["variance"], lv["offset"], 3)


def _se(K):
    se = K.SquaredExponential(variance=1.1, lengthscales=0.5)
    return se, {"se.variance": se.variance, "se.lengthscales": se.lengthscales}, \
        (lambda lv: _torch_kernel("SquaredExponential", lv["se.variance"], lv["se.lengthscales"]))


def _mk_sum(K, cols=None):
    (se, pars, k0), lin = _se(K), K.Linear(variance=0.8 if cols is None else [0.8, 0.5], **({} if cols is None else {"active_dims": cols}))

    def tk(lv):
        a, (b, bd) = k0(lv), _lin_torch(lv["lin.variance"], cols=cols)
        return (lambda A, B: a(A, B) + b(A, B)), (lambda X: lv["se.variance"] + bd(X))
    return se + lin, dict(pars, **{"lin.variance": lin.variance}), tk


def _mk_prod(K, degree=None):
    (se, pars, k0) = _se(K)
    lin = K.Linear(variance=0.8) if degree is None else K.Polynomial(degree, variance=[0.8, 0.5, 1.2], offset=0.3)
    pars = dict(pars, **{"lin.variance": lin.variance}, **({} if degree is None else {"lin.offset": lin.offset}))

    def tk(lv):
        a, (b, bd) = k0(lv), _lin_torch(lv["lin.variance"], lv.get("lin.offset"), degree)
        return (lambda A, B: a(A, B) * b(A, B)), (lambda X: lv["se.variance"] * bd(X))
    return se * lin, pars, tk


def _mk_nested(K):
    (se, pars, k0), lin, m32 = _se(K), K.Linear(variance=0.8), K.Matern32(variance=0.9, lengthscales=0.7)
    pars = dict(pars, **{"lin.variance": lin.variance, "m32.variance": m32.variance, "m32.lengthscales": m32.lengthscales})

    def tk(lv):
        a, (b, bd), c = k0(lv), _lin_torch(lv["lin.variance"]), _torch_kernel("Matern32", lv["m32.variance"], lv["m32.lengthscales"])
        return (lambda A, B: (a(A, B) + b(A, B)) * c(A, B)), (lambda X: (lv["se.variance"] + bd(X)) * lv["m32.variance"])
    return (se + lin) * m32, pars, tk


# name -> (D, M, maker): the shapes of the module docstring
KERNELS = {"linear_ard": (6, 5, _mk_linear), "poly3": (3, 16, _mk_poly3), "se+linear": (3, 16, _mk_sum), "se*linear": (3, 16, _mk_prod),
           "se*poly2": (3, 16, lambda K: _mk_prod(K, 2)), "(se+linear)*m32": (3, 16, _mk_nested),
           "se+linear[2,0]": (3, 16, lambda K: _mk_sum(K, [2, 0]))}
_PROBLEMS = {}


def _problem(D, M):
    """B = 40, P = 2, inputs uniform in [-1, 1]; made once per shape and shared"""
    if (D, M) not in _PROBLEMS:
        rng = np.random.default_rng(1000 * D + M)
        B, P = 40, 2
        X = rng.uniform(-1.0, 1.0, size=(B, D))
        Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(B, P))
        Z = rng.uniform(-1.0, 1.0, size=(M, D))
        q_mu = 0.3 * rng.normal(size=(M, P))
        q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
        _PROBLEMS[(D, M)] = (X, Y, Z, q_mu, q_sqrt)
    return _PROBLEMS[(D, M)]


def _leaves(pars, extra):
    lv = {key: _leaf(par.numpy()) for key, par in pars.items()}
    lv.update({k: _leaf(v) for k, v in extra.items()})
    return lv


def _agree(name, v, ref, forward):
    assert abs(v - ref) <= VALUE_TOL * abs(ref), (name, v, ref)
    assert abs(forward - v) <= VALUE_TOL * abs(v), (name, "forward against *_and_grad", forward, v)


@pytest.mark.parametrize("which", ["linear_ard", "poly3", "se+linear", "se*poly2"])
def test_gpr_vs_autograd_oracle(gp, which):
    """GPR.log_marginal_likelihood (composed from self.kernel(X)) and _and_grad, N = 40, a constant mean: every kernel Parameter (each
    ARD weight, the offset), the noise and the mean constant"""
    gpflow = gp
    D, M, make = KERNELS[which]
    X, Y, _, _, _ = _problem(D, M)
    kern, pars, tk = make(gpflow.kernels)
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.2))
    v, g = m.log_marginal_likelihood_and_grad()
    lv = _leaves(pars, {"noise": 0.15, "mean": 0.2})
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=tk(lv)[0])
    Fo.backward()
    _agree("gpr " + which, v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    allp = dict(pars, noise=m.likelihood.variance, mean=m.mean_function.c)
    _check_model_grads("gpr " + which, g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values())


def _svgp_check(gpflow, name, kern, pars, tk, problem, *, whiten, q_diag, lik=None, lik_pars=None, noise_of=None, shared=False):
    X, Y, Z, q_mu, q_sqrt = problem
    P = q_mu.shape[1]
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    lik = gpflow.likelihoods.Gaussian(0.2) if lik is None else lik
    IV = gpflow.inducing_variables
    iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy())) if shared else Z.copy()
    m = gpflow.models.SVGP(gpflow.kernels.SharedIndependent(kern, P) if shared else kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, q_diag=q_diag,
                           whiten=whiten, num_latent_gps=P, num_data=1000, mean_function=gpflow.mean_functions.Constant(0.1))
    assert m._fused_config() is None, "the fused shard takes K_diag for the variance and must decline"
    v, g = m.elbo_and_grad((X, Y))
    lv = _leaves(pars, {"Z": Z, "q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.1})
    if lik_pars is None:
        lv["noise"] = _leaf(0.2)
        noise, lik_pars = lv["noise"], {"noise": lik.variance}
    else:
        lv.update({k: _leaf(p.numpy()) for k, p in lik_pars.items()})
        noise = noise_of(lv, _t(X))
    kfun, kdiag = tk(lv)
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], lv["q_sqrt"], None, None, noise, num_data=1000, whiten=whiten,
                              mean=lv["mean"], kfun=kfun, kdiag=kdiag(_t(X)))
    Fo.backward()
    _agree(name, v, float(Fo.detach()), float(m.elbo((X, Y)).cpu()))
    Zp = m.inducing_variable.inducing_variable.Z if shared else m.inducing_variable.Z
    allp = dict(pars, Z=Zp, q_mu=m.q_mu, mean=m.mean_function.c, **lik_pars)
    _check_model_grads(name, g, allp, lv, GRAD_TOL)
    if q_diag:
        _check_model_grads(name, g, {"q_sqrt": m.q_sqrt}, lv, GRAD_TOL)
    else:            # fill-triangular: the unconstrained vector holds the lower-triangular entries
        ref = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
        _close(name + " q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(ref).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)
    assert set(g) == set(allp.values()) | {m.q_sqrt}


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("which", ["linear_ard", "poly3", "se+linear", "se*linear"])
def test_svgp_vs_autograd_oracle(gp, which, whiten, q_diag):
    """SVGP.elbo (composed: the posterior) and elbo_and_grad, num_data = 1000 against B = 40: the kernel Parameters, Z, q_mu, q_sqrt, the
    noise and the mean constant"""
    D, M, make = KERNELS[which]
    kern, pars, tk = make(gp.kernels)
    _svgp_check(gp, f"svgp {which}", kern, pars, tk, _problem(D, M), whiten=whiten, q_diag=q_diag)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("which", ["(se+linear)*m32", "se+linear[2,0]", "se*poly2"])
def test_svgp_trees_and_active_dims_vs_autograd_oracle(gp, which, whiten):
    """a nested tree, a Linear member with `active_dims` (ARD over the two columns it sees), an ARD Polynomial in a Product"""
    D, M, make = KERNELS[which]
    kern, pars, tk = make(gp.kernels)
    if which == "(se+linear)*m32":
        route = gp.models.reverse.CovarianceRoute(kern, D)
        assert route.spec.tree == ("mul", [("add", [0, 1]), 2]) and not route.spec.constant_diagonal and not route.spec.packable
        assert [route.spec.is_dot(i) for i in range(3)] == [False, True, False]
    _svgp_check(gp, f"svgp {which}", kern, pars, tk, _problem(D, M), whiten=whiten, q_diag=not whiten)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_heteroskedastic_vs_autograd_oracle(gp, whiten):
    """Gaussian(scale=Linear(A, b)): dF/d sigma_n^2 per row takes the rows of the diagonal as well"""
    gpflow = gp
    D, M, make = KERNELS["linear_ard"]
    kern, pars, tk = make(gpflow.kernels)
    A0, b0 = np.array([[-0.1], [0.05], [0.02], [0.0], [0.03], [-0.04]]), np.array([0.6])
    lik = gpflow.likelihoods.Gaussian(scale=gpflow.functions.Linear(A=A0.copy(), b=b0.copy()))

    def noise_of(lv, X):
        return torch.clamp(X @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2
    _svgp_check(gpflow, "svgp heteroskedastic", kern, pars, tk, _problem(D, M), whiten=whiten, q_diag=False, lik=lik,
                lik_pars={"A": lik.scale.A, "b": lik.scale.b}, noise_of=noise_of)


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
def test_svgp_shared_independent_linear_vs_autograd_oracle(gp, q_diag):
    """SharedIndependent(Linear) over SharedIndependentInducingVariables: one route, the kernel unwrapped"""
    D, M, make = KERNELS["linear_ard"]
    kern, pars, tk = make(gp.kernels)
    _svgp_check(gp, "svgp shared", kern, pars, tk, _problem(D, M), whiten=True, q_diag=q_diag, shared=True)


# ------------------------------------------------------------------------------------------------ 7. forward routes
def _posterior_np(Kmm, Kmn, Knn, q_mu, q_sqrt, whiten, full_cov):
    """conditionals/util.py base_conditional + the q(u) terms in NumPy: (mean [N, P], var [N, P] or [P, N, N])"""
    L = np.linalg.cholesky(Kmm)
    A = np.linalg.solve(L, Kmn)
    fv = Knn - A.T @ A if full_cov else Knn - (A * A).sum(0)
    if not whiten:
        A = np.linalg.solve(L.T, A)
    mean = A.T @ q_mu
    out = []
    for p in range(q_mu.shape[1]):
        LTA = (np.tril(q_sqrt[p]).T if q_sqrt.ndim == 3 else np.diag(q_sqrt[:, p])) @ A
        out.append(fv + (LTA.T @ LTA if full_cov else (LTA * LTA).sum(0)))
    return mean, (np.stack(out) if full_cov else np.stack(out, axis=1))


@pytest.mark.parametrize("which", ["poly3", "se+linear"])
def test_predict_f_in_the_four_covariance_forms(gp, which):
    """SVGP.predict_f fused and through the cached posterior, full_cov x full_output_cov, whitened and not, against a NumPy
    restatement; GPR.predict_f / predict_y likewise; the shape of predict_f_samples"""
    gpflow = gp
    D, M, make = KERNELS[which]
    X, Y, Z, q_mu, q_sqrt = _problem(D, M)
    kern, pars, tk = make(gpflow.kernels)
    kfun, kdiag = tk({k: _t(p.numpy()) for k, p in pars.items()})
    Xn = np.random.default_rng(4).uniform(-1, 1, size=(7, D))
    Kmm = kfun(_t(Z), _t(Z)).numpy() + 1e-6 * np.eye(M)
    Kmn, Knn = kfun(_t(Z), _t(Xn)).numpy(), kfun(_t(Xn), _t(Xn)).numpy()
    close = lambda a, b: np.abs(_np(a) - b).max() <= 1e-9 * max(1.0, np.abs(b).max())   # noqa: E731
    for whiten in (True, False):
        m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten, num_latent_gps=2)
        mean, var = _posterior_np(Kmm, Kmn, np.diag(Knn), q_mu, q_sqrt, whiten, False)
        _, cov = _posterior_np(Kmm, Kmn, Knn, q_mu, q_sqrt, whiten, True)
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
        assert tuple(m.predict_f_samples(Xn, num_samples=3).shape) == (3, 7, 2)
    r = gpflow.models.GPR((X, Y), kern, noise_variance=0.15)
    Kxx = kfun(_t(X), _t(X)).numpy() + 0.15 * np.eye(X.shape[0])
    Kxn = kfun(_t(X), _t(Xn)).numpy()
    sol = np.linalg.solve(Kxx, Kxn)
    mu, v = r.predict_f(Xn)
    assert close(mu, sol.T @ Y) and close(v[:, 0], np.diag(Knn - Kxn.T @ sol))
    mu, v = r.predict_f(Xn, full_cov=True)
    assert close(v[0], Knn - Kxn.T @ sol)
    _, vy = r.predict_y(Xn)
    assert close(vy[:, 0], np.diag(Knn - Kxn.T @ sol) + 0.15)


def test_svgp_elbo_with_bernoulli(gp):
    """a quadrature likelihood, forward: the composed ELBO against the model's own pieces -- the variational expectations of the
    likelihood at predict_f's moments and the prior KL -- and its reverse pass refused"""
    gpflow = gp
    D, M, make = KERNELS["poly3"]
    X, Y, Z, q_mu, q_sqrt = _problem(D, M)
    kern, _, _ = make(gpflow.kernels)
    Yb = (Y[:, :1] > 0).astype(np.float64)
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1], num_data=200)
    assert m._fused_config() is None
    fm, fv = m.predict_f(X)
    want = float(m.likelihood.variational_expectations(gpflow.ops.to_device(X), fm, fv, gpflow.ops.to_device(Yb)).sum().cpu()) * 5.0 \
        - float(m.prior_kl().cpu())
    got = float(m.elbo((X, Yb)).cpu())
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
    # fvar holds the ROW diagonal: with the variance in its place the value moves
    kd = _np(kern(X, full_cov=False))
    assert np.abs(kd - kd.mean()).max() > 0.1
    with pytest.raises(NotImplementedError, match="quadrature"):
        m.elbo_and_grad((X, Yb))


@pytest.mark.parametrize("wrapper", ["separate", "lcm"])
def test_multioutput_wrappers_with_a_linear_member(gp, wrapper):
    """SeparateIndependent([Linear, SE + Linear]) equals the sum of its single-latent models; LinearCoregionalization with W = I and
    the same members equals it as well (the mixing is the identity); both decline the fused per-latent shards, and their reverse pass
    is refused"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    X, Y, Z, q_mu, q_sqrt = _problem(6, 5)
    ks = [K.Linear(variance=0.5 + 0.25 * np.arange(6)), K.SquaredExponential(variance=1.1, lengthscales=0.5) + K.Linear(variance=0.8)]
    kern = K.SeparateIndependent(ks) if wrapper == "separate" else K.LinearCoregionalization(ks, W=np.eye(2))
    iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2, num_data=120)
    assert m._fused_separate_config() is None and m._fused_lcm_config() is None
    total = 0.0
    for p, kp in enumerate(ks):
        one = gpflow.models.SVGP(kp, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu[:, p:p + 1], q_sqrt=q_sqrt[p:p + 1], num_data=120)
        total += float(one.elbo((X, Y[:, p:p + 1])).cpu())
    got = float(m.elbo((X, Y)).cpu())
    assert abs(got - total) <= 1e-10 * abs(total), (got, total)
    kd = _np(kern(X, full_cov=False, full_output_cov=False))
    assert np.abs(kd[:, 0] - (X * X * (0.5 + 0.25 * np.arange(6))).sum(1)).max() < 1e-14
    with pytest.raises(NotImplementedError, match="per-latent"):
        m.elbo_and_grad((X, Y))


def test_scipy_lowers_the_loss_and_moves_the_linear_variance(gp):
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(10)
    X = rng.uniform(-1.0, 1.0, size=(40, 1))
    Y = 1.5 * X + 0.3 * np.sin(6 * X) + 0.05 * rng.normal(size=(40, 1))
    lin = K.Linear(variance=0.2)
    m = gpflow.models.GPR((X, Y), K.SquaredExponential(lengthscales=0.5) + lin, noise_variance=0.1)
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=5))
    after = -float(m.log_marginal_likelihood().cpu())
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert abs(float(lin.variance.numpy()) - 0.2) > 1e-3


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(gp):
    """before anything touches a device: the constructors, and every model route that takes K_diag for one scalar -- each by the limit
    it breaks; at the primitives, what the library refuses"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    for bad in (2.5, 0, 17, -1, float("nan"), "3"):
        with pytest.raises(NotImplementedError, match="integral degree 1 ... 16: the power is a product, not pow"):
            K.Polynomial(degree=bad)
    assert K.Polynomial(degree=3.0).degree == 3 and K.Polynomial(degree=16).degree == 16 and isinstance(K.Polynomial().degree, int)
    with pytest.raises(ValueError, match="active_dims"):
        K.Linear(variance=[1.0, 2.0, 3.0], active_dims=[0, 1])
    with pytest.raises(ValueError):
        K.Linear(variance=[[1.0]])
    with pytest.raises(Exception):
        K.Linear(variance=-1.0)                                                           # positive()
    with pytest.raises(Exception):
        K.Polynomial(offset=-0.5)
    X, Y, Z, q_mu, q_sqrt = _problem(3, 16)
    with pytest.raises(ValueError, match="entries"):
        K.Linear(variance=[1.0, 2.0])(X)                                                  # ARD width against the inputs
    lik = gpflow.likelihoods.Gaussian(0.2)
    for k in (K.Linear(), K.SquaredExponential() + K.Polynomial(2)):
        with pytest.raises(NotImplementedError, match="SGPR"):
            gpflow.models.SGPR((X, Y), k, Z.copy()).elbo()
        with pytest.raises(NotImplementedError, match="SGPR"):
            gpflow.models.SGPR((X, Y), k, Z.copy()).objective_and_grad()
        m = gpflow.models.SVGP(k, lik, Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2)
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(m)
        with pytest.raises(NotImplementedError, match="natural gradients"):
            gpflow.optimizers.NaturalGradient(gamma=0.5).minimize(m, (X, Y))
        mb = gpflow.models.SVGP(k, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1])
        with pytest.raises(NotImplementedError, match="quadrature"):
            mb.elbo_and_grad((X, (Y[:, :1] > 0).astype(np.float64)))
    iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))
    for kern in (K.SeparateIndependent([K.Linear(), K.SquaredExponential()]),
                 K.LinearCoregionalization([K.SquaredExponential(), K.Polynomial(2)], W=np.eye(2))):
        with pytest.raises(NotImplementedError, match="per-latent"):
            gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2).elbo_and_grad((X, Y))
    from gpflow_amd import gradients
    from gpflow_amd.leaf import DotLeaf, Leaf
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), DotLeaf("Linear", 0.8)], "add")
    assert not spec.constant_diagonal and gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5)]).constant_diagonal
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.kdiag()
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.dkdiag()
    for who, impl, dev in _impls(gp):
        tX = _on(X, "c", dev)
        for kw in (dict(family="Polynomial", variance=1.0, offset=0.1, degree=17), dict(family="Polynomial", variance=1.0, offset=0.1, degree=0),
                   dict(family="Polynomial", variance=1.0, offset=float("nan"), degree=2), dict(family="Linear", variance=float("inf")),
                   dict(family="Linear", variance=[1.0, 2.0]), dict(family="ArcCosine", variance=1.0),
                   dict(family="Linear", variance=1.0, offset=0.1, degree=2), dict(family="Polynomial", variance=1.0)):
            with pytest.raises(_refused() + (NotImplementedError,)):      # (a degree out of range: NotImplementedError, as the classes)
                impl.dot_kernel_matrix(tX, None, **kw)
            with pytest.raises(_refused() + (NotImplementedError,)):
                impl.dot_kernel_diag(tX, **kw)
        with pytest.raises(_refused()):
            impl.dot_kernel_matrix_combine(tX, None, _on(np.ones((40, 40)), "c", dev), op="dr2", family="Linear", variance=1.0)
        assert tuple(impl.dot_kernel_matrix(tX[:0], tX, family="Linear", variance=1.0).shape) == (0, 40)
        assert tuple(impl.dot_kernel_matrix(tX, tX[:0], family="Linear", variance=1.0).shape) == (40, 0)
