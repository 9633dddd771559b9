"""GPU tests of the ArcCosine kernel: the five primitives of gpflow_amd/csrc/arccosine/arccosine.hip (`ops.arccos_kernel_matrix`,
`_combine`, `_diag`, `_adjoint_stage`, `_adjoint_tail`), `kernels.ArcCosine` on every forward route, the reverse pass of GPR, VGP and
SVGP, and the kernel crossed with every other kind of leaf in Sum and Product trees.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_arccosine_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture).  On the device every primitive case also runs the emulation beside it (`_impls`).

References.  Primitives: an np.longdouble evaluation of the formulas of include/gpk.h, the bound derived per element next to it
(`_arc_ref`; u = 2^-53, first order in u): the (d + 1) u of the fma chains in s, p, q and the rounding of "+ b"; the two square roots,
their product and the quotient c = s / (rp rq); one rounding of the acos argument; acos itself, ACOS_ULP = 4 ulp (the OpenCL
full-profile bound the ROCm device library is built to) on top of the argument's error amplified by 1 / sin theta; pi as a double;
sin theta = sqrt((1 - cos)(1 + cos)); the products of J, the powers of p and q and v / pi.  Each case asserts on the reference that
min(1 - |c|) over the off-diagonal elements is at least 5e-4, so that no bound is inflated by a 1 / sin theta near a coincidence.
The tail: the header's formulas in longdouble over random operands.  `arccos_kernel_adjoint` whole: torch autograd of the formula,
the diagonal of cos theta of K(A, A) replaced by the constant 1 - eps, to ADJ_TOL = 1e-9 in the measure of `_close`: with
1 - |c| >= 5e-4, sin theta >= 0.031 and the order-0 derivative 1 / sin theta moves by (d + 2) u / sin^3 theta <= 3e-11 of itself under
the roundings of c on either side; the sums of up to 9100 such terms carry no more than their largest term's error relative to the
largest gradient entry, so 1e-9 leaves a factor 30 and is a hundred times below what a wrong term would show.
Models: torch under autograd (oracle/gp_oracle_grad.py through its `kfun=` / `kdiag=` hooks; VGP: the restated ELBO of
tests/test_gpu_vgp.py); values 1e-9 relative, gradients 1e-8 through `_check_model_grads` -- the project's figures.

Condition of the model problems (B = 40, P = 2, D = 3, M = 16, inputs uniform in [-1, 1]: test_gpu_dot_kernels._problem(3, 16)).  Every
kernel entry and every entry of the row diagonal was perturbed by a relative 4 * 2^-52 with random signs in the oracle, on the CPU
(`conditioning_figures`, asserted at <= 1e-10 by tests/test_arccosine_emulated.py); the oracle's own gradients moved by at most, in the
measure of `_close`: CONDITIONING_FIGURES below.  A new shape or seed needs that check repeated.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_arccosine_ops  # noqa: E402
import test_gpu_dot_kernels as DK  # noqa: E402
import test_gpu_kernel_trees as TR  # noqa: E402
import test_gpu_vgp as VG  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _padding_untouched, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

VALUE_TOL, GRAD_TOL = 1e-9, 1e-8
ADJ_TOL = 1e-9
ACOS_ULP = 4
MIN_MARGIN = 5e-4
TINY = LD(1e-300)
PI = LD("3.14159265358979323846264338327950288")
EPS64 = np.float64(1e-15)
SCALE64 = np.float64(1.0) - np.float64(2.0) * EPS64
CT_DIAG64 = np.float64(1.0) - EPS64
ORDERS = (0, 1, 2)
BIAS, VAR = 0.7, 0.8
JF = (1.0, 1.0, 3.0)
# the largest move of the oracle's gradients under the perturbation of the module docstring, per problem (CPU, this file's seeds)
CONDITIONING_FIGURES = {"gpr order 0": 7.2e-15, "gpr order 1": 2.5e-13, "gpr order 2": 1.9e-14, "svgp order 0": 5.5e-14,
                        "svgp order 1": 7.4e-11, "svgp order 2": 4.7e-11, "svgp heteroskedastic": 4.3e-14, "vgp bernoulli": 5.2e-15}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


class _Emulation:
    arccos_kernel_matrix = staticmethod(fake_arccosine_ops.arccos_kernel_matrix)
    arccos_kernel_matrix_combine = staticmethod(fake_arccosine_ops.arccos_kernel_matrix_combine)
    arccos_kernel_diag = staticmethod(fake_arccosine_ops.arccos_kernel_diag)
    arccos_adjoint_parts = staticmethod(fake_arccosine_ops.arccos_adjoint_parts)
    arccos_adjoint_stage = staticmethod(fake_arccosine_ops.arccos_adjoint_stage)
    arccos_adjoint_tail = staticmethod(fake_arccosine_ops.arccos_adjoint_tail)


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", _Emulation, "cpu")] if dev != "cpu" else [])


def _kw(order, w):
    return dict(order=order, variance=VAR, weight_variances=w, bias_variance=BIAS)


# ------------------------------------------------------------------------------------------------ the longdouble reference
def _norm_ref(X, w, b):
    """p = sum_j w_j x_j^2 + b and its bound: the chain's (d + 1) u over the (positive) terms, one rounding for "+ b" """
    d = X.shape[1]
    wl = np.broadcast_to(np.asarray(w, dtype=LD), (d,))
    terms = X.astype(LD) * wl * X.astype(LD)
    k = (d + 1) * LD(U)
    p = terms.sum(-1) + LD(b)
    dp = k / (1 - k) * np.abs(terms).sum(-1)
    return p, dp + U * (np.abs(p) + dp)


def _arc_ref(order, X1, X2, w, b=BIAS, v=VAR, same=False):
    """Everything the primitives compute, element by element, in longdouble with its bound: a dict of (value, bound) pairs --
    "k" the kernel, "jm" = J m (k without v / pi), "dks" / "dkp" / "dkq" its derivatives with respect to s, p_i and q_k -- and
    "margin" = min(1 - |c|) over the elements that are not on a by-index diagonal."""
    X2 = X1 if same else X2
    s0, ds0 = DK._sref(X1, X2, w)
    s = s0 + LD(b)
    ds = ds0 + U * (np.abs(s) + ds0)
    (p, dp), (q, dq) = _norm_ref(X1, w, b), _norm_ref(X2, w, b)
    rel_p, rel_q = dp / (p - dp), dq / (q - dq)
    rp, rq = np.sqrt(p), np.sqrt(q)
    rel_rp, rel_rq = 0.5 * rel_p + U, 0.5 * rel_q + U                        # sqrt halves the relative error; its own rounding
    P, Q, RP, RQ = p[:, None], q[None, :], rp[:, None], rq[None, :]
    rr = RP * RQ
    rel_rr = rel_rp[:, None] + rel_rq[None, :] + U
    c = s / rr
    dc = ds / rr + np.abs(c) * (rel_rr + U)
    diag = np.eye(*c.shape, dtype=bool) if same else np.zeros(c.shape, dtype=bool)
    margin = float(np.min(np.where(diag, 1.0, 1.0 - np.abs(c))))
    arg = LD(SCALE64) * c + LD(EPS64)
    darg = LD(SCALE64) * dc + U * np.abs(arg)
    arg, darg = np.where(diag, LD(CT_DIAG64), arg), np.where(diag, LD(0), darg)
    arg = np.clip(arg, -1, 1)                                                   # (1-Lipschitz; MIN_MARGIN keeps it idle)
    th = np.arccos(arg)
    sin_lo = np.sqrt(np.maximum(1 - np.minimum(np.abs(arg) + darg, 1) ** 2, TINY))
    dth = darg / sin_lo + ACOS_ULP * 2 * U * np.abs(th)                         # ulp(theta) <= 2 u theta
    pt = PI - th
    dpt = dth + U * np.abs(pt) + LD(1.3e-16)                                    # pi as a double
    om, op_ = 1 - arg, 1 + arg
    sn = np.sqrt(om * op_)
    rel_sn = 0.5 * ((darg + U * om) / np.maximum(om - darg, TINY) + (darg + U * op_) / np.maximum(op_ - darg, TINY) + U) + U
    dsn = sn * rel_sn
    J1 = sn + pt * arg
    dJ1 = dsn + dpt * np.abs(arg) + np.abs(pt) * darg + dpt * darg + U * np.abs(pt * arg) + U * (sn + np.abs(pt * arg))
    if order == 0:
        J, dJ = pt, dpt
        D = 1 / sn
        dD = D * (rel_sn / (1 - rel_sn) + U)
    elif order == 1:
        J, dJ, D, dD = J1, dJ1, pt, dpt
    else:
        t1 = 3 * sn * arg
        dt1 = 3 * (dsn * np.abs(arg) + sn * darg + dsn * darg) + 2 * U * np.abs(t1)
        t2 = 1 + 2 * arg * arg
        dt2 = 4 * np.abs(arg) * darg + 2 * darg * darg + 3 * U * np.abs(t2)
        t3 = pt * t2
        dt3 = dpt * t2 + np.abs(pt) * dt2 + dpt * dt2 + U * np.abs(t3)
        J, dJ = t1 + t3, dt1 + dt3 + U * (np.abs(t1) + np.abs(t3))
        D, dD = 4 * J1, 4 * dJ1
    if order == 0:
        m, dm = np.ones_like(rr), np.zeros_like(rr)
    elif order == 1:
        m, dm = rr, rr * rel_rr
    else:
        m = P * Q
        dm = m * (rel_p[:, None] + rel_q[None, :] + U)
    jm = J * m
    djm = dJ * m + np.abs(J) * dm + dJ * dm + U * np.abs(jm)
    vpi = LD(v) / PI
    k = vpi * jm
    dk = np.abs(vpi) * djm + 3 * U * np.abs(k)                                  # v * (1 / pi) as doubles: two roundings and pi's own
    # the derivatives; the by-index diagonal has no angular part
    D, dD = np.where(diag, LD(0), D), np.where(diag, LD(0), dD)
    cc, dcc = np.where(diag, LD(1), c), np.where(diag, LD(0), dc)
    sd = LD(SCALE64) * D
    dsd = LD(SCALE64) * dD + U * np.abs(sd)
    inner = order * J - sd * cc
    dinner = order * dJ + np.abs(cc) * dsd + np.abs(sd) * dcc + dsd * dcc + U * np.abs(sd * cc) + U * (np.abs(order * J) + np.abs(sd * cc))
    h = 0.5 * vpi * inner
    dh = np.abs(0.5 * vpi) * dinner + 4 * U * np.abs(h)
    if order == 0:
        dks = vpi * sd / rr
        ddks = np.abs(vpi) / rr * dsd + np.abs(dks) * (rel_rr + 5 * U)
        dkp, dkq = h / P, h / Q
        ddkp, ddkq = dh / P + np.abs(dkp) * (rel_p[:, None] + U), dh / Q + np.abs(dkq) * (rel_q[None, :] + U)
    elif order == 1:
        dks = vpi * sd
        ddks = np.abs(vpi) * dsd + 4 * U * np.abs(dks)
        dkp, dkq = h * RQ / RP, h * RP / RQ
        both = rel_rp[:, None] + rel_rq[None, :] + 2 * U
        ddkp, ddkq = dh * RQ / RP + np.abs(dkp) * both, dh * RP / RQ + np.abs(dkq) * both
    else:
        dks = vpi * sd * rr
        ddks = np.abs(vpi) * rr * dsd + np.abs(dks) * (rel_rr + 5 * U)
        dkp, dkq = h * Q, h * P
        ddkp, ddkq = dh * Q + np.abs(dkp) * (rel_q[None, :] + U), dh * P + np.abs(dkq) * (rel_p[:, None] + U)
    return dict(k=(k, dk + TINY), jm=(jm, djm + TINY), dks=(dks, ddks + TINY), dkp=(dkp, ddkp + TINY), dkq=(dkq, ddkq + TINY), margin=margin,
                p=(p, dp))


def _diag_ref(order, X, w, b=BIAS, v=VAR, what="k"):
    """the closed-form row diagonal v jf p^order, or its derivative with respect to p, with the bound of its few products"""
    p, dp = _norm_ref(X, w, b)
    v = LD(v)
    if what == "k":
        val = [v * np.ones_like(p), v * p, 3 * v * p * p][order]
        bnd = [0 * p, np.abs(v) * dp + U * np.abs(val), 3 * np.abs(v) * (2 * p * dp + dp * dp) + 3 * U * np.abs(val)][order]
    else:
        val = [0 * p, v * np.ones_like(p), 6 * v * p][order]
        bnd = [0 * p, 0 * p, 6 * np.abs(v) * dp + 2 * U * np.abs(val)][order]
    return val, bnd + TINY


# ------------------------------------------------------------------------------------------------ 1. the builder
BUILD_CASES = DK.BUILD_CASES   # (1, 1, 1), (63, 65, 3), (64, 64, 64), (130, 70, 5): smallest; a partial tile each way; GPK_MAX_D; ragged tiles
LAYOUTS = DK.LAYOUTS           # c / ld / off / pad
_weights, _inputs = DK._weights, DK._inputs
_REFS = {}


def _ref_of(order, n1, n2, d, ard, same=False):
    """the reference of a build case, computed once and shared by the tests that need it"""
    key = (order, n1, n2, d, ard, same)
    if key not in _REFS:
        X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
        _REFS[key] = _arc_ref(order, X1, X2, _weights(ard, d), same=same)
        assert _REFS[key]["margin"] >= MIN_MARGIN, (key, _REFS[key]["margin"])
    return _REFS[key]


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n1,n2,d", BUILD_CASES)
def test_arccos_kernel_matrix(gp, n1, n2, d, layout, ard):
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    w = _weights(ard, d)
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "ld", dev), _on(X2, "pad" if layout == "c" else "c", dev)
        for order in ORDERS:
            ref, bnd = _ref_of(order, n1, n2, d, ard)["k"]
            out, buf = _on(np.full((n1, n2), -555.0), layout, dev, base=True)
            got = impl.arccos_kernel_matrix(t1, t2, out=out, diag_add=9.0, **_kw(order, w))   # (diag_add: ignored with X2 given)
            name = f"arccos_kernel_matrix {who} order {order}"
            assert got is out and _padding_untouched(out, buf), f"{name}: padding written"
            _within(name, _np(out), ref, bnd)
        _check_unchanged(f"arccos_kernel_matrix {who}", [t1, t2], [X1, X2])
        fresh = impl.arccos_kernel_matrix(t1.contiguous(), t2.contiguous(), **_kw(1, w))
        assert _same_bits(_np(fresh), _np(impl.arccos_kernel_matrix(t1, t2, **_kw(1, w)))), f"{who}: the layout of X changes the result"


SYM_CASES = [(1, 1), (63, 3), (64, 64), (130, 5)]


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,d", SYM_CASES)
def test_arccos_kernel_matrix_symmetric(gp, n, d, layout, ard):
    """K(X, X) + diag_add I is EXACTLY symmetric (the mirror), a lower_only build has bit for bit the lower triangle of the full one,
    nothing outside the view is written, and the diagonal is the by-index value (v / pi) J(acos(1 - eps)) p_i^order -- which is not
    the closed-form K_diag"""
    X, _ = _inputs(n, n, d, 100 * n + d)
    w = _weights(ard, d)
    eye = np.eye(n, dtype=LD)
    for who, impl, dev in _impls(gp):
        tX = _on(X, "col", dev)
        for order in ORDERS:
            r = _ref_of(order, n, n, d, ard, same=True)
            ref, bnd = r["k"]
            name = f"symmetric {who} order {order}"
            out, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
            impl.arccos_kernel_matrix(tX, None, out=out, diag_add=0.25, **_kw(order, w))
            Kf = _np(out).copy()
            assert _padding_untouched(out, buf), f"{name}: padding written"
            assert _same_bits(Kf, Kf.T), f"{name}: not exactly symmetric"
            _within(name, np.tril(Kf), np.tril(ref + LD(0.25) * eye), np.tril(bnd + U * np.abs(ref + 0.25) * eye))
            low, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
            impl.arccos_kernel_matrix(tX, None, out=low, diag_add=0.25, lower_only=True, **_kw(order, w))
            assert _padding_untouched(low, buf) and _same_bits(np.tril(_np(low)), np.tril(Kf)), f"{name}: lower_only differs from the full build"
            plain = _np(impl.arccos_kernel_matrix(tX, None, **_kw(order, w)))
            assert _same_bits(plain - np.diag(np.diag(plain)), Kf - np.diag(np.diag(Kf))), f"{name}: diag_add reached off the diagonal"
            # the diagonal by index: J at acos(1 - eps) EXACTLY, times p^order
            p, dp = r["p"]
            th = np.arccos(LD(CT_DIAG64))
            sn = np.sqrt((1 - LD(CT_DIAG64)) * (1 + LD(CT_DIAG64)))
            Jd = [PI - th, sn + (PI - th) * LD(CT_DIAG64), 3 * sn * LD(CT_DIAG64) + (PI - th) * (1 + 2 * LD(CT_DIAG64) ** 2)][order]
            want = LD(VAR) / PI * Jd * p ** order
            assert np.all(np.abs(want - np.diag(ref)) <= 8 * U * np.abs(want) + np.diag(bnd))
            _within(name + " diagonal by index", np.diag(plain), np.diag(ref), np.diag(bnd))
            if order == 0:
                kd = _np(impl.arccos_kernel_diag(tX, **_kw(order, w)))
                rel = np.abs(kd - np.diag(plain)) / kd
                assert np.all((rel > 1e-8) & (rel < 2e-8)), f"{name}: K_diag is the closed form, 1.4e-8 from the built diagonal"
        _check_unchanged(f"symmetric {who}", [tX], [X])


@pytest.mark.parametrize("symmetric", [False, True], ids=["130x70", "symmetric130"])
@pytest.mark.parametrize("layout", ["c", "ld", "off"])
def test_arccos_kernel_matrix_combine(gp, layout, symmetric):
    """ops mul / add with `out` aliasing G (and not); diag_add lands on the diagonal of the COMBINED result; X2 = None takes the
    diagonal by index"""
    n1, n2, d = (130, 130, 5) if symmetric else (130, 70, 5)
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    G = np.random.default_rng(6).normal(size=(n1, n2))
    w = _weights(True, d)
    eye = np.eye(n1, n2, dtype=LD) if symmetric else 0
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "c", dev), (None if symmetric else _on(X2, "ld", dev))
        for order in ORDERS:
            kw = _kw(order, w)
            k, kb = _ref_of(order, n1, n2, d, True, same=symmetric)["k"]
            Gl = G.astype(LD)
            want = {"mul": (Gl * k + 0.5 * eye, np.abs(Gl) * kb + U * np.abs(Gl * k) + U * np.abs(Gl * k + 0.5) * eye),
                    "add": (Gl + k + 0.5 * eye, kb + U * np.abs(Gl + k) + U * np.abs(Gl + k + 0.5) * eye)}
            for op, (ref, bnd) in want.items():
                name = f"combine {who} order {order} {op}"
                tG, buf = _on(G, layout, dev, base=True)
                got = impl.arccos_kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.5, out=tG, **kw)      # in place
                assert got is tG and _padding_untouched(tG, buf), f"{name}: padding written"
                _within(name, _np(tG), ref, bnd + TINY)
                tG2 = _on(G, "pad", dev)
                sep = impl.arccos_kernel_matrix_combine(t1, t2, tG2, op=op, diag_add=0.5, **kw)             # a fresh output
                assert _same_bits(_np(sep), _np(tG)), f"{name}: aliasing changes the result"
                _check_unchanged(name, [tG2], [G])
        _check_unchanged(f"combine {who}", [t1] + ([] if symmetric else [t2]), [X1] + ([] if symmetric else [X2]))


# ------------------------------------------------------------------------------------------------ 2. the row diagonal
@pytest.mark.parametrize("n,d", [(1, 1), (63, 3), (64, 64), (130, 5)])
def test_arccos_kernel_diag(gp, n, d):
    """all four ops over a padded ldx, every order: the closed form v jf p^order within the bound of its chain and products"""
    X, _ = _inputs(n, n, d, 100 * n + d)
    g = np.random.default_rng(n + d).normal(size=n)
    for ard in (False, True):
        w = _weights(ard, d)
        for who, impl, dev in _impls(gp):
            tX = _on(X, "pad", dev)
            for order in ORDERS:
                kw = _kw(order, w)
                k, kb = _diag_ref(order, X, w)
                dk, dkb = _diag_ref(order, X, w, what="dp")
                name = f"arccos_kernel_diag {who} order {order}"
                _within(name + " k", _np(impl.arccos_kernel_diag(tX, **kw)), k, kb)
                gl = g.astype(LD)
                for op, ref, bnd in (("mul", gl * k, np.abs(gl) * kb + U * np.abs(gl * k)), ("add", gl + k, kb + U * np.abs(gl + k)),
                                     ("dp", gl * dk, np.abs(gl) * dkb + U * np.abs(gl * dk))):
                    tg = _on(g, "c", dev)
                    got = impl.arccos_kernel_diag(tX, tg, op=op, out=tg, **kw)                               # out aliases g
                    assert got is tg
                    _within(f"{name} {op}", _np(tg), ref, bnd + TINY)
                    tg2 = _on(g, "c", dev)
                    assert _same_bits(_np(impl.arccos_kernel_diag(tX, tg2, op=op, **kw)), _np(tg)) and _same_bits(_np(tg2), g)
            _check_unchanged(f"arccos_kernel_diag {who}", [tX], [X])


# ------------------------------------------------------------------------------------------------ 3. the adjoint stage
def _split_parts(parts, n1, n2):
    """(rho slots [tc, n1], gamma slots [tr, n2], tile sums [tr, tc]) by the header's layout"""
    tr, tc = -(-n1 // 64), -(-n2 // 64)
    a, b = tc * n1, tc * n1 + tr * n2
    return parts[:a].reshape(tc, n1), parts[a:b].reshape(tr, n2), parts[b:b + tr * tc].reshape(tr, tc)


def _kbar(n1, n2, symmetric):
    Kb = np.random.default_rng(7 + n1).normal(size=(n1, n2))
    if symmetric:          # a heavy diagonal: what the by-index rule keeps out of the angular derivative
        Kb = Kb + Kb.T + 50.0 * np.eye(n1)
    return Kb


STAGE_CASES = [(130, 70, 5, False), (63, 63, 3, True), (64, 64, 64, False)]   # (the last: GPK_MAX_D, 64 KB of slabs beside the stage's own 27 KB)
STAGE_IDS = ["cross130x70", "symmetric63", "cross64x64xMAX_D"]


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("n1,n2,d,symmetric", STAGE_CASES, ids=STAGE_IDS)
def test_arccos_adjoint_stage(gp, n1, n2, d, symmetric, ard):
    """G = Kbar .* dk/ds element by element, and rho, gamma and sum(Kbar .* k) / v recovered from the slots of `parts`, against the
    longdouble reference; every slot of the documented extent is written and nothing beyond it; G may alias Kbar; a rerun is
    bit-identical.  Sums: each term carries its own bound, and a sum of N terms in a fixed order adds N u sum |terms|."""
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    w = _weights(ard, d)
    Kb = _kbar(n1, n2, symmetric)
    Kl = Kb.astype(LD)
    tr, tc = -(-n1 // 64), -(-n2 // 64)
    extent = tc * n1 + tr * n2 + tr * tc
    for who, impl, dev in _impls(gp):
        t1, t2 = _on(X1, "ld", dev), (None if symmetric else _on(X2, "pad", dev))
        for order in ORDERS:
            r = _ref_of(order, n1, n2, d, ard, same=symmetric)
            kw = _kw(order, w)
            name = f"arccos_adjoint_stage {who} order {order}"
            runs = []
            for rep in range(2):
                parts = _on(np.full(extent + 7, -555.0), "c", dev)
                tK = _on(Kb, "ld", dev)
                G = impl.arccos_adjoint_stage(t1, t2, tK, parts, **kw)
                _check_unchanged(name, [tK], [Kb])
                pn = _np(parts)
                assert np.all(pn[extent:] == -555.0) and not np.any(pn[:extent] == -555.0), f"{name}: the extent of parts"
                runs.append((_np(G).copy(), pn[:extent].copy()))
            assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), f"{name}: a rerun differs"
            tK, buf = _on(Kb, "off", dev, base=True)
            parts = impl.arccos_adjoint_parts(n1, n2, dev)
            assert parts.numel() == extent
            Ga = impl.arccos_adjoint_stage(t1, t2, tK, parts, out=tK, **kw)                                   # G aliases Kbar
            assert Ga is tK and _padding_untouched(tK, buf) and _same_bits(_np(tK), runs[0][0]) and _same_bits(_np(parts), runs[0][1])
            dks, ddks = r["dks"]
            _within(name + " G", runs[0][0], Kl * dks, np.abs(Kl) * ddks + U * np.abs(Kl * dks) + TINY)
            rho_s, gam_s, sums = _split_parts(runs[0][1], n1, n2)
            for what, got, (val, bnd), axis, n in (("rho", rho_s.sum(0), r["dkp"], 1, n2), ("gamma", gam_s.sum(0), r["dkq"], 0, n1)):
                t = Kl * val
                _within(f"{name} {what}", got, t.sum(axis), (np.abs(Kl) * bnd + U * np.abs(t)).sum(axis) + (n + 2) * U * np.abs(t).sum(axis) + TINY)
            t = Kl * r["jm"][0]
            _within(name + " sum", np.array(sums.sum()), np.array(t.sum()),
                    np.array((np.abs(Kl) * r["jm"][1] + U * np.abs(t)).sum() + (84 + tr * tc + 2) * U * np.abs(t).sum()))
        _check_unchanged(f"arccos_adjoint_stage {who}", [t1] + ([] if symmetric else [t2]), [X1] + ([] if symmetric else [X2]))


# ------------------------------------------------------------------------------------------------ 4. the adjoint tail
@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("symmetric", [False, True], ids=["cross", "symmetric"])
@pytest.mark.parametrize("n1,n2,d", [(1, 1, 1), (130, 70, 64), (130, 70, 5), (63, 65, 3)])
def test_arccos_adjoint_tail(gp, n1, n2, d, symmetric, ard):
    """the formulas of include/gpk.h in longdouble over random R, parts, A, B.  d = 64, n1 = 130: every thread walks several rows;
    d = 5 does not divide 1024.  Every sum of N terms in a fixed order: (N + 2) u sum |terms| (products included); rho and gamma are
    sums of tc / tr slots first.  A second call is bit-identical."""
    n2 = n1 if symmetric else n2
    rng = np.random.default_rng(17 * n1 + d + symmetric)
    A, B = rng.uniform(-1.0, 1.0, size=(n1, d)), rng.uniform(-1.0, 1.0, size=(n2, d))
    R = rng.normal(size=(n1, 1 + 2 * d))                       # as wide as G moment_rows(B)^T: the B^2 columns are not read
    tr, tc = -(-n1 // 64), -(-n2 // 64)
    parts = rng.normal(size=tc * n1 + tr * n2 + tr * tc)
    w = np.asarray(_weights(ard, d), dtype=np.float64)
    Al, Bl, Rl, wl = A.astype(LD), (A if symmetric else B).astype(LD), R.astype(LD), np.broadcast_to(w.astype(LD), (d,))
    rs, gs, ss = _split_parts(parts.astype(LD), n1, n2)
    rho, gam = rs.sum(0), gs.sum(0)
    drho, dgam = tc * U * np.abs(rs).sum(0), tr * U * np.abs(gs).sum(0)
    if symmetric:
        rho, drho = rho + gam, drho + dgam + U * np.abs(rho + gam)
    GB = Rl[:, 1:1 + d]
    tA = Al * (GB + rho[:, None] * Al)
    aA = np.abs(Al) * (np.abs(GB) + np.abs(rho[:, None] * Al))
    dw, dwb = tA.sum(0), (n1 + 6) * U * aA.sum(0) + (np.abs(Al * Al) * drho[:, None]).sum(0)
    db, dbb = (Rl[:, 0] + rho).sum(), (n1 + 3) * U * (np.abs(Rl[:, 0]) + np.abs(rho)).sum() + drho.sum()
    if not symmetric:
        tB = gam[:, None] * Bl * Bl
        dw, dwb = dw + tB.sum(0), dwb + (n1 + n2 + 6) * U * np.abs(tB).sum(0) + (np.abs(Bl * Bl) * dgam[:, None]).sum(0) + (n2 + 2) * U * aA.sum(0)
        db, dbb = db + gam.sum(), dbb + (n1 + n2 + 3) * U * np.abs(gam).sum() + dgam.sum() + (n2 + 2) * U * (np.abs(Rl[:, 0]) + np.abs(rho)).sum()
    if not ard:
        dw, dwb = dw.sum().reshape(1), (dwb.sum() + (d - 1) * U * (aA.sum() + (0 if symmetric else np.abs(tB).sum()))).reshape(1)
    dv, dvb = ss.sum() / PI, ((tr * tc + 70) * U * np.abs(ss).sum() / PI).reshape(1)
    two = 2 if symmetric else 1
    Abar = two * wl * GB + 2 * wl * Al * rho[:, None]
    Abarb = 4 * U * (np.abs(two * wl * GB) + np.abs(2 * wl * Al * rho[:, None])) + np.abs(2 * wl * Al) * drho[:, None]
    for who, impl, dev in _impls(gp):
        tR, tAA, tB_, tp = _on(R, "ld", dev), _on(A, "pad", dev), (None if symmetric else _on(B, "ld", dev)), _on(parts, "c", dev)
        runs = [tuple(_np(x).copy() for x in impl.arccos_adjoint_tail(tR, tAA, tB_, tp, weight_variances=w)) for _ in range(2)]
        name = f"arccos_adjoint_tail {who}"
        assert all(_same_bits(a, b) for a, b in zip(*runs)), f"{name}: two runs differ"
        _within(name + " d/dvariance", runs[0][0], np.reshape(dv, 1), dvb + TINY)
        _within(name + " d/dweights", runs[0][1], dw, dwb + TINY)
        _within(name + " d/dbias", runs[0][2], np.reshape(db, 1), np.reshape(dbb, 1) + TINY)
        _within(name + " A_bar", runs[0][3], Abar, Abarb + TINY)
        _check_unchanged(name, [tR, tAA, tp] + ([] if symmetric else [tB_]), [R, A, parts] + ([] if symmetric else [B]))


# ------------------------------------------------------------------------------------------------ 5. the whole adjoint against autograd
def _arc_torch(order, v, w, b, cols=None):
    """torch restatement of gpflow/kernels/misc.py: (kfun(A, B), kdiag(X)).  Called with the same tensor OBJECT twice (X2 is None in
    the reference) the diagonal of cos theta is the constant 1 - eps, as the library takes it by index."""
    def norms(X):
        return (X * X * w).sum(1) + b

    def kfun(A, B):
        same = A is B
        if cols is not None:
            A = A[:, cols]
            B = A if same else B[:, cols]
        p, q = norms(A), norms(B)
        c = ((A * w) @ B.T + b) / (torch.sqrt(p)[:, None] * torch.sqrt(q)[None, :])
        arg = float(EPS64) + float(SCALE64) * c
        if same:
            arg = torch.where(torch.eye(A.shape[0], dtype=torch.bool), torch.tensor(float(CT_DIAG64), dtype=torch.float64), arg)
        th = torch.acos(arg)
        sn, cs, pt = torch.sin(th), torch.cos(th), np.pi - th
        J = pt if order == 0 else sn + pt * cs if order == 1 else 3.0 * sn * cs + pt * (1.0 + 2.0 * cs * cs)
        return v / np.pi * J * (p[:, None] ** (order / 2.0) if order else 1.0) * (q[None, :] ** (order / 2.0) if order else 1.0)

    def kdiag(X):
        if cols is not None:
            X = X[:, cols]
        return v * JF[order] * norms(X) ** order if order else v * torch.ones(X.shape[0], dtype=torch.float64)
    return kfun, kdiag


@pytest.mark.parametrize("ard", [False, True], ids=["one_weight", "ard"])
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n1,n2,d,symmetric", STAGE_CASES[:2], ids=STAGE_IDS[:2])
def test_arccos_kernel_adjoint_against_autograd(gp, n1, n2, d, symmetric, order, ard):
    """gradients.arccos_kernel_adjoint -- stage, contraction, tail -- against autograd of sum(Kbar .* K): d/dvariance, every weight, the
    bias and A_bar; the symmetric Kbar has a heavy diagonal, which an angular derivative at 1 / sin(4.5e-8) would turn into 1e9"""
    from gpflow_amd import gradients
    from gpflow_amd.leaf import ArcLeaf
    dev = _dev(gp)
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    w = _weights(ard, d)
    Kb = _kbar(n1, n2, symmetric)
    lv = {"A": _leaf(X1), "v": _leaf(VAR), "w": _leaf(w), "b": _leaf(BIAS)}
    kfun, _ = _arc_torch(order, lv["v"], lv["w"], lv["b"])
    (_t(Kb) * kfun(lv["A"], lv["A"] if symmetric else _t(X2))).sum().backward()
    tA, tK = _on(X1, "c", dev), _on(Kb, "c", dev)
    tB = tA if symmetric else _on(X2, "c", dev)
    dv, dl, Abar = gradients.arccos_kernel_adjoint(ArcLeaf(order, VAR, w, BIAS), tA, tB, tK, symmetric=symmetric)
    nw = d if ard else 1
    name = f"adjoint order {order}"
    _close(name + " variance", dv, lv["v"].grad.numpy().reshape(1), ADJ_TOL)
    _close(name + " weights", dl[:nw], lv["w"].grad.numpy().reshape(-1), ADJ_TOL)
    _close(name + " bias", dl[nw:], lv["b"].grad.numpy().reshape(1), ADJ_TOL)
    _close(name + " A_bar", Abar, lv["A"].grad.numpy(), ADJ_TOL)
    _check_unchanged(name, [tA, tK], [X1, Kb])


# ------------------------------------------------------------------------------------------------ 6. NaN / Inf, refusals at the primitives
@pytest.mark.parametrize("planted", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_arccos_nan_reaches_its_own_row_and_column_only(gp, planted):
    """(130, 70, 5): a NaN (or an Inf, which the quotient turns into one) in row 129 of X1 (the far row tile) and in row 69 of X2 (the far column tile) makes exactly that row and
    that column of K NaN -- the clamp lets it through -- and every other element keeps its bits; the combine ops, the adjoint stage
    and the row diagonal likewise; the symmetric build: row and column 129"""
    n1, n2, d = 130, 70, 5
    X1, X2 = _inputs(n1, n2, d, 100 * n1 + d)
    B1, B2 = X1.copy(), X2.copy()
    B1[129, 2] = planted
    B2[69, 4] = planted
    bad = np.zeros((n1, n2), dtype=bool)
    bad[129, :] = True
    bad[:, 69] = True
    w = _weights(True, d)
    G = np.random.default_rng(3).normal(size=(n1, n2))
    for who, impl, dev in _impls(gp):
        c1, c2, t1, t2 = _on(X1, "c", dev), _on(X2, "c", dev), _on(B1, "c", dev), _on(B2, "c", dev)
        for order in ORDERS:
            kw = _kw(order, w)
            name = f"nan {who} order {order}"
            clean, K = _np(impl.arccos_kernel_matrix(c1, c2, **kw)), _np(impl.arccos_kernel_matrix(t1, t2, **kw))
            assert np.array_equal(np.isnan(K), bad) and _same_bits(K[~bad], clean[~bad]), name
            for op in ("mul", "add"):
                cleanc = _np(impl.arccos_kernel_matrix_combine(c1, c2, _on(G, "c", dev), op=op, **kw))
                C = _np(impl.arccos_kernel_matrix_combine(t1, t2, _on(G, "c", dev), op=op, **kw))
                assert np.array_equal(np.isnan(C), bad) and _same_bits(C[~bad], cleanc[~bad]), f"{name} {op}"
            pc, pb = impl.arccos_adjoint_parts(n1, n2, dev), impl.arccos_adjoint_parts(n1, n2, dev)
            Gc, Gb = _np(impl.arccos_adjoint_stage(c1, c2, _on(G, "c", dev), pc, **kw)), _np(impl.arccos_adjoint_stage(t1, t2, _on(G, "c", dev), pb, **kw))
            assert np.array_equal(np.isnan(Gb), bad) and _same_bits(Gb[~bad], Gc[~bad]), f"{name} stage"
            rho, gam, _ = _split_parts(_np(pb), n1, n2)
            assert np.array_equal(np.isnan(rho.sum(0)), np.arange(n1) >= 0) and np.array_equal(np.isnan(gam.sum(0)), np.arange(n2) >= 0), \
                f"{name}: every row meets column 69 and every column row 129"
            Ks = _np(impl.arccos_kernel_matrix(t1, None, **kw))
            rows = np.arange(n1) == 129
            assert np.array_equal(np.isnan(Ks), rows[:, None] | rows[None, :]), f"{name} symmetric"
            assert np.array_equal(~np.isfinite(_np(impl.arccos_kernel_diag(t1, **kw))), rows), f"{name} diagonal"
        _check_unchanged(f"nan {who}", [t1, t2], [B1, B2])


def test_primitive_refusals_leave_the_output_unchanged(gp):
    """what the library (GPK_E_ARG / GPK_E_UNSUPPORTED), the wrappers (ValueError) or the emulation (AssertionError) refuse, each
    replayed with an output that must keep its bits"""
    n, d = 40, 3
    X, _ = _inputs(n, n, d, 1)
    ok = dict(order=1, variance=VAR, weight_variances=1.3, bias_variance=BIAS)
    bads = [dict(ok, order=3), dict(ok, order=-1), dict(ok, weight_variances=-1.0), dict(ok, weight_variances=float("nan")),
            dict(ok, weight_variances=[1.0, 2.0]), dict(ok, weight_variances=[1.0, float("inf"), 1.0]), dict(ok, bias_variance=0.0),
            dict(ok, bias_variance=-0.5), dict(ok, bias_variance=float("nan")), dict(ok, variance=float("inf")), dict(ok, variance=float("nan"))]
    for who, impl, dev in _impls(gp):
        tX = _on(X, "c", dev)
        out, g, parts = _on(np.full((n, n), -555.0), "c", dev), _on(np.full(n, -555.0), "c", dev), _on(np.full(2 * n + 1, -555.0), "c", dev)
        for kw in bads:
            for call in (lambda: impl.arccos_kernel_matrix(tX, None, out=out, **kw),
                         lambda: impl.arccos_kernel_matrix_combine(tX, None, out, op="mul", out=out, **kw),
                         lambda: impl.arccos_kernel_diag(tX, g, op="mul", out=g, **kw),
                         lambda: impl.arccos_adjoint_stage(tX, None, out, parts, out=out, **kw)):
                with pytest.raises(_refused()):
                    call()
        for call in (lambda: impl.arccos_kernel_matrix_combine(tX, None, out, op="ds", out=out, **ok),
                     lambda: impl.arccos_kernel_diag(tX, g, op="ds", out=g, **ok),
                     lambda: impl.arccos_kernel_diag(tX, g, op="k", out=g, **ok),
                     lambda: impl.arccos_adjoint_stage(tX, None, out, parts[:5], out=out, **ok),
                     lambda: impl.arccos_adjoint_tail(out, tX, None, parts, weight_variances=-1.0),
                     lambda: impl.arccos_adjoint_tail(out[:, :3], tX, None, parts, weight_variances=1.0)):
            with pytest.raises(_refused()):
                call()
        assert np.all(_np(out) == -555.0) and np.all(_np(g) == -555.0) and np.all(_np(parts) == -555.0), f"{who}: a refused call wrote"
        assert tuple(impl.arccos_kernel_matrix(tX[:0], tX, **ok).shape) == (0, n)
        if who == "ops":          # the dot-product builder still refuses the name
            with pytest.raises(_refused() + (NotImplementedError,)):
                gp.ops.dot_kernel_matrix(tX, None, family="ArcCosine", variance=1.0)


# ------------------------------------------------------------------------------------------------ 7. the class, forward
def _arc_np(order, X, X2, v, w, b, cols=None):
    same = X2 is None
    kfun, _ = _arc_torch(order, v, _t(w), b, cols)
    tX = _t(X)
    return kfun(tX, tX if same else _t(X2)).numpy()


def test_kernel_class_forward(gp):
    """K, K_into, K_diag, active_dims, batch dimensions, the covariance dispatchers, and the predicates"""
    gpflow = gp
    K = gpflow.kernels
    from gpflow_amd.kernels.base import DeviceLeaf, is_arc_leaf, is_device_leaf, is_dot_leaf, reverse_leaf
    from gpflow_amd.models.reverse import has_row_diagonal
    rng = np.random.default_rng(12)
    X, X2 = rng.uniform(-1, 1, size=(40, 4)), rng.uniform(-1, 1, size=(30, 4))
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()   # noqa: E731
    for order in ORDERS:
        k = K.ArcCosine(order, variance=0.8, weight_variances=[0.5, 2.0], bias_variance=0.7, active_dims=[3, 1])
        assert is_arc_leaf(k) and not is_dot_leaf(k) and not is_device_leaf(k) and not isinstance(k, DeviceLeaf) and k.ard
        assert has_row_diagonal(k) and has_row_diagonal(K.SquaredExponential() * k) and has_row_diagonal(K.SharedIndependent(k, 2))
        assert reverse_leaf(k) is not None and reverse_leaf(k)[2] == (k.variance, k.weight_variances, k.bias_variance)
        assert rel(_np(k(X, X2)), _arc_np(order, X, X2, 0.8, [0.5, 2.0], 0.7, [3, 1])) < 1e-12
        Kxx = _np(k(X))
        assert rel(Kxx, _arc_np(order, X, None, 0.8, [0.5, 2.0], 0.7, [3, 1])) < 1e-12 and _same_bits(Kxx, Kxx.T)
        kd = _np(k(X, full_cov=False))
        p = (X[:, [3, 1]] ** 2 * [0.5, 2.0]).sum(1) + 0.7
        assert rel(kd, 0.8 * JF[order] * p ** order) < 1e-14 and rel(kd, np.diag(Kxx)) < 1e-7
        Xs = k.slice(gpflow.ops.to_device(X), None)[0]
        assert _same_bits(_np(k.K_into(Xs, None, None, diag_add=0.5)), Kxx + 0.5 * np.eye(40))
        assert tuple(k.K_diag(gpflow.ops.to_device(X).reshape(2, 20, 4)[..., :Xs.shape[1]]).shape) == (2, 20)
    k = K.ArcCosine(2, variance=0.8, weight_variances=1.3, bias_variance=0.7)
    Kb = _np(k.K(gpflow.ops.to_device(X).reshape(2, 20, 4), gpflow.ops.to_device(X2)))
    assert Kb.shape == (2, 20, 30) and _same_bits(Kb.reshape(40, 30), _np(k(X, X2)))
    iv = gpflow.inducing_variables.InducingPoints(X2.copy())
    assert rel(_np(gpflow.covariances.Kuf(iv, k, X)), _arc_np(2, X2, X, 0.8, 1.3, 0.7)) < 1e-12
    assert rel(_np(gpflow.covariances.Kuu(iv, k, jitter=1e-3)), _arc_np(2, X2, None, 0.8, 1.3, 0.7) + 1e-3 * np.eye(30)) < 1e-12


# ------------------------------------------------------------------------------------------------ 8. models against autograd
D, M = 3, 16


def _mk_arc(K, order):
    """order 1: ARD weights over active_dims [2, 0]"""
    cols = [2, 0] if order == 1 else None
    k = K.ArcCosine(order, variance=VAR, weight_variances=[0.8, 1.4] if order == 1 else (1.3, None, 0.9)[order], bias_variance=BIAS,
                    **({} if cols is None else {"active_dims": cols}))
    pars = {"variance": k.variance, "weight_variances": k.weight_variances, "bias_variance": k.bias_variance}
    return k, pars, (lambda lv: _arc_torch(order, lv["variance"], lv["weight_variances"], lv["bias_variance"], cols))


def _perturbed(kfun, kdiag, seed=5):
    """the kernel and its diagonal with every entry moved by a relative 4 * 2^-52, signs random but fixed per shape"""
    signs = {}

    def sgn(shape):
        if shape not in signs:
            signs[shape] = torch.tensor(np.random.default_rng(seed + len(signs)).choice([-1.0, 1.0], size=shape))
        return signs[shape]
    return (lambda A, B: (lambda k: k * (1 + 4 * 2.0 ** -52 * sgn(tuple(k.shape))))(kfun(A, B))), \
        (lambda X: (lambda k: k * (1 + 4 * 2.0 ** -52 * sgn(tuple(k.shape))))(kdiag(X)))


def _oracle_grads(problem, order, model, perturb, whiten=True, het=False):
    """{name: gradient} of the oracle for one model problem, with the kernel perturbed or not (the conditioning check)"""
    X, Y, Z, q_mu, q_sqrt = problem
    cols = [2, 0] if order == 1 else None
    lv = {"variance": _leaf(VAR), "weight_variances": _leaf([0.8, 1.4] if order == 1 else (1.3, None, 0.9)[order]), "bias_variance": _leaf(BIAS),
          "noise": _leaf(0.15), "mean": _leaf(0.2), "Z": _leaf(Z), "q_mu": _leaf(q_mu), "q_sqrt": _leaf(q_sqrt)}
    kfun, kdiag = _arc_torch(order, lv["variance"], lv["weight_variances"], lv["bias_variance"], cols)
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


HET_A, HET_B = np.array([[-0.1], [0.05], [0.02]]), np.array([0.6])


def conditioning_figures():
    """{problem: the largest move of the oracle's gradients, in the measure of `_close`} -- CPU only; CONDITIONING_FIGURES records it"""
    problem = DK._problem(D, M)
    out = {}
    cases = [(f"gpr order {o}", o, "gpr", {}) for o in ORDERS] + [(f"svgp order {o}", o, "svgp", {}) for o in ORDERS] + \
        [("svgp heteroskedastic", 0, "svgp", dict(het=True)), ("vgp bernoulli", 0, "vgp", {})]
    for name, order, model, kw in cases:
        worst = 0.0
        for whiten in ((True, False) if model == "svgp" else (True,)):
            a, b = _oracle_grads(problem, order, model, False, whiten, **kw), _oracle_grads(problem, order, model, True, whiten, **kw)
            worst = max([worst] + [float(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(a[k]).max())) for k in a])
        out[name] = worst
    return out


@pytest.mark.parametrize("order", ORDERS)
def test_gpr_vs_autograd_oracle(gp, order):
    """GPR.log_marginal_likelihood, _and_grad and predict_f, N = 40, a constant mean: the three kernel Parameters (order 1: each ARD
    weight, over active_dims), the noise and the mean constant"""
    gpflow = gp
    X, Y, _, _, _ = DK._problem(D, M)
    kern, pars, tk = _mk_arc(gpflow.kernels, order)
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.2))
    v, g = m.log_marginal_likelihood_and_grad()
    lv = DK._leaves(pars, {"noise": 0.15, "mean": 0.2})
    kfun, kdiag = tk(lv)
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=kfun)
    Fo.backward()
    DK._agree(f"gpr order {order}", v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    allp = dict(pars, noise=m.likelihood.variance, mean=m.mean_function.c)
    _check_model_grads(f"gpr order {order}", g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values())
    # predict
    Xn = np.random.default_rng(4).uniform(-1, 1, size=(7, D))
    with torch.no_grad():
        tX, tn = _t(X), _t(Xn)
        Kxx = kfun(tX, tX).numpy() + 0.15 * np.eye(X.shape[0])
        Kxn, Knn = kfun(tX, tn).numpy(), kfun(tn, tn).numpy()
    sol = np.linalg.solve(Kxx, Kxn)
    close = lambda a, b: np.abs(_np(a) - b).max() <= 1e-9 * max(1.0, np.abs(b).max())   # noqa: E731
    mu, var = m.predict_f(Xn, full_cov=True)
    assert close(mu, sol.T @ (Y - 0.2) + 0.2) and close(var[0], Knn - Kxn.T @ sol)
    mu, var = m.predict_f(Xn)
    with torch.no_grad():
        kd = kdiag(tn).numpy()
    assert close(var[:, 0], kd - (Kxn * sol).sum(0))


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
@pytest.mark.parametrize("order", ORDERS)
def test_svgp_vs_autograd_oracle(gp, order, whiten, q_diag):
    """SVGP.elbo (composed: the posterior) and elbo_and_grad in the four parametrisations, num_data = 1000 against B = 40: the kernel
    Parameters, Z, q_mu, q_sqrt, the noise and the mean constant"""
    kern, pars, tk = _mk_arc(gp.kernels, order)
    DK._svgp_check(gp, f"svgp order {order}", kern, pars, tk, DK._problem(D, M), whiten=whiten, q_diag=q_diag)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_heteroskedastic_and_shared_vs_autograd_oracle(gp, whiten):
    """Gaussian(scale=Linear(A, b)): dF/d sigma_n^2 per row takes the rows of the diagonal as well; and the kernel shared through
    SharedIndependent over SharedIndependentInducingVariables"""
    gpflow = gp
    kern, pars, tk = _mk_arc(gpflow.kernels, 0)
    lik = gpflow.likelihoods.Gaussian(scale=gpflow.functions.Linear(A=HET_A.copy(), b=HET_B.copy()))

    def noise_of(lv, X):
        return torch.clamp(X @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2
    DK._svgp_check(gpflow, "svgp heteroskedastic", kern, pars, tk, DK._problem(D, M), whiten=whiten, q_diag=False, lik=lik,
                   lik_pars={"A": lik.scale.A, "b": lik.scale.b}, noise_of=noise_of)
    kern, pars, tk = _mk_arc(gpflow.kernels, 2)
    DK._svgp_check(gpflow, "svgp shared", kern, pars, tk, DK._problem(D, M), whiten=whiten, q_diag=not whiten, shared=True)


def _vgp_q(N):
    rng = np.random.default_rng(33)
    return 0.3 * rng.normal(size=(N, 2)), np.stack([np.tril(0.05 * rng.normal(size=(N, N))) + 0.6 * np.eye(N) for _ in range(2)])


def test_vgp_bernoulli_vs_autograd(gp):
    """VGP with a Bernoulli likelihood and a constant mean: value, forward ELBO, and every gradient against autograd of the restated ELBO"""
    gpflow = gp
    X, Y, _, _, _ = DK._problem(D, M)
    Yb = (Y > 0).astype(np.float64)
    kern, pars, tk = _mk_arc(gpflow.kernels, 0)
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


def test_scipy_trains_the_three_parameters(gp):
    gpflow = gp
    rng = np.random.default_rng(10)
    X = rng.uniform(-1.0, 1.0, size=(40, 2))
    Y = np.abs(X[:, :1]) + 0.5 * X[:, 1:] + 0.05 * rng.normal(size=(40, 1))
    k = gpflow.kernels.ArcCosine(1, variance=0.5, weight_variances=0.6, bias_variance=0.4)
    m = gpflow.models.GPR((X, Y), k, noise_variance=0.1)
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=5))
    after = -float(m.log_marginal_likelihood().cpu())
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert all(abs(float(p.numpy()) - p0) > 1e-4 for p, p0 in ((k.variance, 0.5), (k.weight_variances, 0.6), (k.bias_variance, 0.4)))


def test_svgp_elbo_with_bernoulli_forward_only(gp):
    """a quadrature likelihood, forward: the composed ELBO against the model's own pieces, and its reverse pass refused"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    kern, _, _ = _mk_arc(gpflow.kernels, 2)
    Yb = (Y[:, :1] > 0).astype(np.float64)
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1], num_data=200)
    assert m._fused_config() is None
    fm, fv = m.predict_f(X)
    want = float(m.likelihood.variational_expectations(gpflow.ops.to_device(X), fm, fv, gpflow.ops.to_device(Yb)).sum().cpu()) * 5.0 \
        - float(m.prior_kl().cpu())
    got = float(m.elbo((X, Yb)).cpu())
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
    kd = _np(kern(X, full_cov=False))
    assert np.abs(kd - kd.mean()).max() > 0.1                  # fvar holds the ROW diagonal
    with pytest.raises(NotImplementedError, match="quadrature"):
        m.elbo_and_grad((X, Yb))


@pytest.mark.parametrize("order", [0, 2])
def test_predict_f_in_the_four_covariance_forms(gp, order):
    """SVGP.predict_f fused and through the cached posterior, full_cov x full_output_cov, whitened and not, against a NumPy restatement"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    kern, pars, tk = _mk_arc(gpflow.kernels, order)
    kfun, kdiag = tk({k: _t(p.numpy()) for k, p in pars.items()})
    Xn = np.random.default_rng(4).uniform(-1, 1, size=(7, D))
    tZ, tn = _t(Z), _t(Xn)
    Kmm = kfun(tZ, tZ).numpy() + 1e-6 * np.eye(M)
    Kmn, Knn = kfun(tZ, tn).numpy(), kfun(tn, tn).numpy()
    Kd = kdiag(tn).numpy()            # the marginal variances take the closed-form diagonal, the full covariance the built matrix
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


@pytest.mark.parametrize("wrapper", ["separate", "lcm"])
def test_multioutput_wrappers_with_an_arccosine_member(gp, wrapper):
    """SeparateIndependent([ArcCosine(1), SE + ArcCosine(0)]) equals the sum of its single-latent models; LinearCoregionalization with
    W = I likewise; both decline the fused per-latent shards, and their reverse pass is refused"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    ks = [K.ArcCosine(1, variance=VAR, weight_variances=[0.8, 1.4, 0.6], bias_variance=BIAS),
          K.SquaredExponential(variance=1.1, lengthscales=0.5) + K.ArcCosine(0, variance=0.6, weight_variances=1.3, bias_variance=BIAS)]
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
    with pytest.raises(NotImplementedError, match="per-latent"):
        m.elbo_and_grad((X, Y))


# ------------------------------------------------------------------------------------------------ 9. trees: crossed with every other kind
class ArcKind(TR.Kind):
    """a row like those of test_gpu_kernel_trees.KINDS for the ArcCosine leaf: constructor, longdouble reference with its bound, torch"""

    def __init__(self, order, values, cols=None):
        super().__init__("arc", "ArcCosine", values, cols)
        self.order = order

    class_name = "ArcCosine"
    is_dot = True      # (what the tree helpers ask: a diagonal that depends on the row)
    wide = True

    def make(self, K):
        v, ad = self.values, ({} if self.cols is None else {"active_dims": list(self.cols)})
        k = K.ArcCosine(self.order, **v, **ad)
        return k, {n: getattr(k, n) for n in v}

    def ref(self, p, X1, X2):
        sel = (lambda X: X) if self.cols is None else (lambda X: X[:, self.cols])
        r = _arc_ref(self.order, sel(X1), None if X2 is None else sel(X2), p["weight_variances"], float(p["bias_variance"]),
                     float(p["variance"]), same=X2 is None)
        assert r["margin"] >= MIN_MARGIN, r["margin"]
        return r["k"]

    def torch(self, lv):
        return _arc_torch(self.order, lv["variance"], lv["weight_variances"], lv["bias_variance"], self.cols)


OTHERS = ["SquaredExponential", "Matern32", "RationalQuadratic", "White", "Constant", "Periodic(SE)", "Linear", "Polynomial"]
ARCS = [ArcKind(0, dict(variance=VAR, weight_variances=1.3, bias_variance=BIAS)),
        ArcKind(1, dict(variance=0.6, weight_variances=[0.8, 1.4, 0.6], bias_variance=0.5)),
        ArcKind(2, dict(variance=0.9, weight_variances=[0.7, 1.2, 0.9], bias_variance=BIAS))]
_CROSS_DATA = {}


def _cross_data():
    """the shapes of test_gpu_kernel_trees (a partial tile each way) with inputs of this file's own: seed 2036 keeps min(1 - |c|) of the
    three ArcCosine leaves at 1.5e-3 or more (ArcKind.ref asserts MIN_MARGIN); two active columns out of three would not -- 66 points
    in the plane have near-parallel pairs at every seed tried -- so `active_dims` is left to the model tests"""
    if not _CROSS_DATA:
        rng = np.random.default_rng(2036)
        _CROSS_DATA.update(X1=rng.uniform(-1.0, 1.0, size=(TR.N1, TR.D)), X2=rng.uniform(-1.0, 1.0, size=(TR.N2, TR.D)),
                           X=rng.uniform(-1.0, 1.0, size=(TR.NSYM, TR.D)), Kbar=rng.normal(size=(TR.N1, TR.N2)),
                           Ksym=rng.normal(size=(TR.NSYM, TR.NSYM)), kd_bar=rng.normal(size=TR.NSYM))
        _CROSS_DATA["Ksym"] = _CROSS_DATA["Ksym"] + _CROSS_DATA["Ksym"].T
    return _CROSS_DATA


CROSSES = [(other, first) for other in OTHERS for first in (True, False)]
CROSS_IDS = [f"{'ArcCosine-' + o if f else o + '-ArcCosine'}" for o, f in CROSSES]


def _cross(i, other, first):
    """(kinds, tree children in order): the ArcCosine's order rotates over the cases"""
    kinds = {"arc": ARCS[i % 3], "o": TR.KINDS[other]}
    return kinds, (["arc", "o"] if first else ["o", "arc"])


@pytest.mark.parametrize("other,first", CROSSES, ids=CROSS_IDS)
def test_cross_forward(gp, other, first):
    """Sum and Product of ArcCosine and one leaf of another kind, as first child (built) and as second (folded in place), symmetric
    with diag_add and cross, through Combination.K_into and KernelSpec.build: within the bound composed from the leaves' own; a second
    call and the other route bitwise equal; padding untouched; K_diag and kdiag_rows within the bound of the closed-form diagonal"""
    dev, dat = _dev(gp), _cross_data()
    kinds, ch = _cross(CROSSES.index((other, first)), other, first)
    for op in ("add", "mul"):
        tree = (op, ch)
        name = f"{ch} {op}"
        kern, pars = TR._make_tree(gp.kernels, tree, kinds)
        vals = TR._values(pars)
        spec = TR._spec_of(gp, kern)
        assert not spec.constant_diagonal and spec.tree == (op, [0, 1]) and not spec.packable
        for symmetric in (True, False):
            A, B = (dat["X"], None) if symmetric else (dat["X1"], dat["X2"])
            ref, bnd = TR._tree_ref(tree, kinds, vals, A, B, TR.DIAG_ADD)
            tA, tB = _on(A, "ld", dev), (None if symmetric else _on(B, "pad", dev))
            shape = (A.shape[0], A.shape[0] if symmetric else B.shape[0])
            for layout in ("c", "ld", "off"):
                outs = []
                for route in ("K_into", "K_into", "build"):
                    out, buf = _on(np.full(shape, -555.0), layout, dev, base=True)
                    kern.K_into(tA, tB, out, diag_add=TR.DIAG_ADD) if route == "K_into" else spec.build(tA, tB, out, TR.DIAG_ADD)
                    assert _padding_untouched(out, buf), f"{name} {route} {layout}: padding written"
                    outs.append(_np(out).copy())
                _within(f"{name} symmetric={symmetric} {layout}", outs[0], ref, bnd)
                assert _same_bits(outs[0], outs[1]) and _same_bits(outs[0], outs[2]), f"{name} {layout}: routes or calls differ"
            _check_unchanged(name, [tA] + ([] if symmetric else [tB]), [A] + ([] if symmetric else [B]))
        # the diagonal: the other leaf's from its reference, the ArcCosine's the closed form
        ak, av = kinds["arc"], TR._sub(vals, "arc")
        Xa = dat["X"] if ak.cols is None else dat["X"][:, ak.cols]
        ad, adb = _diag_ref(ak.order, Xa, av["weight_variances"], float(av["bias_variance"]), float(av["variance"]))
        ok_, okb = kinds["o"].ref(TR._sub(vals, "o"), dat["X"], None)
        od, odb = np.diag(ok_), np.diag(okb)
        dref = ad + od if op == "add" else ad * od
        dbnd = (adb + odb if op == "add" else np.abs(ad) * odb + np.abs(od) * adb + adb * odb) + 2 * U * np.abs(dref)
        tX = _on(dat["X"], "ld", dev)
        _within(f"{name} K_diag", _np(kern.K_diag(tX)), dref, dbnd)
        _within(f"{name} kdiag_rows", _np(spec.kdiag_rows(tX)), dref, dbnd)


@pytest.mark.parametrize("other,first", CROSSES, ids=CROSS_IDS)
def test_cross_adjoint(gp, other, first):
    """KernelSpec.adjoint (symmetric and cross) and diag_adjoint of the same trees against autograd of sum(Kbar .* K(A, B)) and
    sum(kd_bar .* diag K): every member's variance, its shape gradient in the user's layout and A_bar"""
    dev, dat = _dev(gp), _cross_data()
    kinds, ch = _cross(CROSSES.index((other, first)), other, first)
    for op in ("add", "mul"):
        tree = (op, ch)
        kern, pars = TR._make_tree(gp.kernels, tree, kinds)
        spec = TR._spec_of(gp, kern)
        for case, A, B, Kbar in (("symmetric", dat["X"], None, dat["Ksym"]), ("cross", dat["X1"], dat["X2"], dat["Kbar"])):
            name = f"{ch} {op} {case}"
            tA, tK = _on(A, "c", dev), _on(Kbar, "c", dev)
            tB = tA if B is None else _on(B, "c", dev)
            dv, dl, Abar = spec.adjoint(tA, tB, tK, B is None)
            lv = TR._leaves(pars, {"A": A})
            kfun, _ = TR._tree_torch(tree, kinds, lv)
            (_t(Kbar) * kfun(lv["A"], lv["A"] if B is None else _t(B))).sum().backward()
            for i, tag in enumerate(ch):
                _close(f"{name} {tag}.variance", dv[i], np.reshape(TR._grad_of(lv, f"{tag}.variance"), -1), GRAD_TOL)
                sref = TR._shape_ref(lv, tag, kinds[tag])
                assert sref.size == np.asarray(dl[i].cpu()).size, (name, tag)
                if sref.size:
                    _close(f"{name} {tag} shape", dl[i], sref, GRAD_TOL)
            _close(f"{name} A_bar", Abar, TR._grad_of(lv, "A"), GRAD_TOL)
            _check_unchanged(name, [tA, tK], [A, Kbar])
        name = f"{ch} {op} diagonal"
        tX, tg = _on(dat["X"], "c", dev), _on(dat["kd_bar"], "c", dev)
        dv, dl = spec.diag_adjoint(tX, tg)
        lv = TR._leaves(pars)
        _, kdiag = TR._tree_torch(tree, kinds, lv)
        (_t(dat["kd_bar"]) * kdiag(_t(dat["X"]))).sum().backward()
        for i, tag in enumerate(ch):
            _close(f"{name} {tag}.variance", dv[i], np.reshape(TR._grad_of(lv, f"{tag}.variance"), -1), GRAD_TOL)
            sref = TR._shape_ref(lv, tag, kinds[tag])
            if sref.size:
                _close(f"{name} {tag} shape", dl[i], sref, GRAD_TOL)
        _check_unchanged(name, [tX, tg], [dat["X"], dat["kd_bar"]])


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(gp):
    """before anything touches a device: the constructor, and every model route that takes K_diag for one scalar -- each by the limit
    it breaks"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    for bad in (3, -1, 0.5, "1", None, True):
        with pytest.raises(ValueError, match="order is not implemented"):
            K.ArcCosine(order=bad)
    assert K.ArcCosine().order == 0 and K.ArcCosine(2).order == 2 and isinstance(K.ArcCosine(1.0).order, int)
    with pytest.raises(ValueError, match="active_dims"):
        K.ArcCosine(weight_variances=[1.0, 2.0, 3.0], active_dims=[0, 1])
    with pytest.raises(ValueError):
        K.ArcCosine(weight_variances=[[1.0]])
    with pytest.raises(Exception):
        K.ArcCosine(bias_variance=-1.0)                                                   # positive()
    X, Y, Z, q_mu, q_sqrt = DK._problem(D, M)
    with pytest.raises(ValueError, match="entries"):
        K.ArcCosine(weight_variances=[1.0, 2.0])(X)                                       # ARD width against the inputs
    lik = gpflow.likelihoods.Gaussian(0.2)
    for k in (K.ArcCosine(1), K.SquaredExponential() + K.ArcCosine(2)):
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
    for kern in (K.SeparateIndependent([K.ArcCosine(), K.SquaredExponential()]),
                 K.LinearCoregionalization([K.SquaredExponential(), K.ArcCosine(2)], W=np.eye(2))):
        with pytest.raises(NotImplementedError, match="per-latent"):
            gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2).elbo_and_grad((X, Y))
    from gpflow_amd import gradients
    from gpflow_amd.leaf import ArcLeaf, Leaf
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), ArcLeaf(1, 0.8, [1.0, 2.0, 3.0], 0.7)], "add")
    assert not spec.constant_diagonal and not spec.packable and spec.n_variance(1) == 1 and spec.n_shape(1) == 4
    assert spec.parameter_names(1) == ("variance", "weight_variances", "bias_variance")
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.kdiag()
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.dkdiag()
    with pytest.raises(ValueError, match="period"):
        gradients.KernelSpec([ArcLeaf(0, 1.0)], periods=[1.0])
