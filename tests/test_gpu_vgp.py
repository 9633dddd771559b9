"""GPU tests of the full variational GP: the primitive `ops.tril_product` (gpflow_amd/csrc/vgp/tril_product.hip), the reverse pass
`gradients.vgp_elbo_and_grad` and `models.VGP` on every route.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_vgp_emulated.py imports them without this module's `gpu`
mark and gives them an emulated `gp` fixture).  On the device every primitive case also runs the emulation beside it (`_impls`).

References.  Primitive: np.longdouble evaluation of the definition, the bound derived in `_reference`.  Models: torch on the CPU in
fp64 -- a restatement of the reference's VGP.elbo (gpflow/models/vgp.py:131-155: dense L @ tril(q_sqrt), 20-point Gauss-Hermite) --
evaluated for the values and differentiated by autograd for the gradients; SciPy's multivariate normal for the closed form.
Tolerances: ELBO 1e-8 relative (the bar of the SVGP tests of the same likelihoods, tests/test_gpu_likelihoods.py), the value of the
gradient routine 1e-9 relative and every gradient 1e-8 of max(1, its largest entry) (tests/test_gpu_gradients.py), predictions 1e-9.
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
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_vgp_ops  # noqa: E402
from test_gpu_contract import LD, U, _bits, _check_unchanged, _np, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _close, _t, _torch_kernel  # noqa: E402
from test_gpu_likelihood_zoo import _torch_ve  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

T = 128                     # the kernel's tile edge (include/gpk.h: GPK_TRIL_TILE)
JITTER = 1e-6               # config.default_jitter()
ELBO_TOL, VALUE_TOL, GRAD_TOL, PREDICT_TOL = 1e-8, 1e-9, 1e-8, 1e-9
GH_X, GH_W = np.polynomial.hermite.hermgauss(20)
PATTERN = -7.25e11          # what outputs and padding are pre-filled with (finite, so a bitwise comparison cannot be fooled by NaN != NaN)


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", fake_vgp_ops, "cpu")] if dev != "cpu" else [])


# ------------------------------------------------------------------------------------------------ 1. the primitive
SIZES = [1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 2]   # a partial tile, the exact tile, one past it, K ranges of three tile blocks beside one of one
LATENTS = [1, 3]
LAYOUTS = ["c", "ld"]       # contiguous; ld = n + 3 for L, every S_r and T, with an odd batch stride for S and T
MODES = ["ssq", "product", "both"]
_REF = {}


def _reference(n, R):
    """(L, S, rowscale, P, ssq, bound of P, bound of ssq) of one shape, computed once and never modified; L and S are FULL matrices
    (what is above the diagonals must not matter), P = tril(L) tril(S_r) in longdouble.

    Bounds (u = 2^-53, gamma_k = k u / (1 - k u)).  P[i, j] is a sum of at most n products; in whatever order the MFMA, the VALU
    slabs and the K loop add them, a term passes through at most n roundings (its product -- none under fma -- and at most n - 1
    additions), so  |dP[i, j]| <= gamma_n a_ij,  a = |L| |S_r| over the triangles.  ssq[i] = sum_j P^2: the computed square differs by
    2 P dP + dP^2, to first order 2 gamma_n a^2 (|P| <= a), and the sum of the at most n squares -- the fma chain over a lane's blocks,
    the four shuffle steps, the two waves, the tile columns; adding an exact zero costs nothing -- again at most n roundings per term,
    gamma_n sum_j a^2.  Together  |d ssq[i]| <= 3 gamma_n sum_j a_ij^2  to first order; the tests allow twice that (the higher orders,
    and n against n + 1).  The stored product is rowscale * P with one more rounding:  gamma_n a |rowscale| + u |rowscale P|, twice
    that allowed as well."""
    if (n, R) not in _REF:
        rng = np.random.default_rng(1000 * n + R)
        L = rng.normal(size=(n, n)) + np.diag(1.0 + rng.random(n))
        S = 0.3 * rng.normal(size=(R, n, n)) + 0.6 * np.eye(n)
        rs = rng.normal(size=(R, n))
        Lt, St = np.tril(L), np.tril(S)
        P = np.stack([Lt.astype(LD) @ St[r].astype(LD) for r in range(R)])
        a = np.stack([np.abs(Lt) @ np.abs(St[r]) for r in range(R)]).astype(LD)
        g = n * LD(U) / (1 - n * LD(U))
        ssq = (P * P).sum(-1)
        bssq = 2 * 3 * g * (a * a).sum(-1)
        bP = 2 * (g * a * np.abs(rs)[:, :, None] + LD(U) * np.abs(rs[:, :, None] * P))
        for v in (L, S, rs, P, ssq, bP, bssq):
            v.setflags(write=False)
        _REF[(n, R)] = (L, S, rs, P, ssq, bP, bssq)
    return _REF[(n, R)]


def _place(x, layout, dev, fill=PATTERN):
    """NumPy [n, n] or [R, n, n] -> (view, allocation) on `dev`: "c" contiguous; "ld" rows n + 3 apart and -- 3-D -- entries an ODD
    number of elements apart; everything outside the view holds `fill`."""
    x = np.asarray(x, dtype=np.float64)
    if layout == "c":
        v = torch.tensor(x, dtype=torch.float64, device=dev)
        return v, v
    n = x.shape[-1]
    ld = n + 3
    if x.ndim == 2:
        buf = torch.full((n * ld,), fill, dtype=torch.float64, device=dev)
        v = torch.as_strided(buf, (n, n), (ld, 1))
    else:
        stride = n * ld + (1 if (n * ld) % 2 == 0 else 2)
        buf = torch.full((x.shape[0] * stride,), fill, dtype=torch.float64, device=dev)
        v = torch.as_strided(buf, (x.shape[0], n, n), (stride, ld, 1))
    v.copy_(torch.tensor(x, dtype=torch.float64))
    return v, buf


def _outside_lower(v, buf):
    """the elements of `buf` that are not on or below the diagonal of an entry of its view v [R, n, n] (or all of it outside v)"""
    idx = np.zeros((), dtype=np.int64)
    for size, stride in zip(v.shape, v.stride()):
        idx = idx[..., None] + np.arange(size, dtype=np.int64) * stride
    n = v.shape[-1]
    inside = np.zeros(buf.numel(), dtype=bool)
    inside[idx[:, np.tril(np.ones((n, n), dtype=bool))].reshape(-1)] = True
    return _np(buf).reshape(-1)[~inside]


def _run(ops, dev, n, R, layout, mode, parts=None):
    """one call in `mode` on `dev`: (ssq | None, lower triangle of T | None, T's view, T's allocation, the input tensors)"""
    L, S, rs = _reference(n, R)[:3]
    tL, _ = _place(L, layout, dev)
    tS, _ = _place(S, layout, dev)
    trs = torch.tensor(rs, dtype=torch.float64, device=dev)
    kw = dict(want_ssq=mode != "product", parts=parts)
    tT = bufT = None
    if mode != "ssq":
        tT, bufT = _place(np.full((R, n, n), PATTERN), layout, dev)
        kw.update(rowscale=trs, product_out=tT)
    ssq, got = ops.tril_product(tL, tS, **kw)
    assert (got is tT) and ((ssq is None) == (mode == "product"))
    return (None if ssq is None else _np(ssq)), tT, bufT, (tL, tS, trs)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("R", LATENTS)
@pytest.mark.parametrize("n", SIZES)
def test_tril_product_against_longdouble(gp, n, R, layout):
    """ssq-only, product-only and both at once within the bounds of `_reference`; nothing above the diagonal of T or in its padding
    is written; the inputs are unchanged; a second call gives the same bits; ssq does not depend on whether the product is stored."""
    L, S, rs, P, ssq_ref, bP, bssq = _reference(n, R)
    low = np.tril(np.ones((n, n), dtype=bool))
    for who, ops, dev in _impls(gp):
        seen = {}
        for mode in MODES:
            name = f"tril_product {who} n={n} R={R} {layout} {mode}"
            ssq, tT, bufT, ins = _run(ops, dev, n, R, layout, mode)
            ssq2, tT2, _, _ = _run(ops, dev, n, R, layout, mode)
            _check_unchanged(name, ins, [L, S, rs])
            if ssq is not None:
                assert ssq.shape == (R, n)
                _within(name + " ssq", ssq, ssq_ref, bssq)
                assert _same_bits(ssq, ssq2), f"{name}: two calls differ"
                assert _same_bits(ssq, seen.setdefault("ssq", ssq)), f"{name}: ssq depends on the mode"
                print(f"{name}: largest ssq error / bound {float(np.max(np.abs(ssq.astype(LD) - ssq_ref) / bssq)):.3g}")
            if tT is not None:
                got = _np(tT)
                _within(name + " T", np.where(low, got, 0.0), np.where(low, rs[:, :, None] * P, 0), np.where(low, bP, 0))
                assert np.all(_bits(_outside_lower(tT, bufT)) == _bits(np.array([PATTERN]))[0]), f"{name}: written outside the lower triangles"
                assert _same_bits(got, _np(tT2)), f"{name}: two calls differ"
                assert _same_bits(got, seen.setdefault("T", got)), f"{name}: T depends on the mode"


def test_tril_product_wrapper_conveniences_and_refusals(gp):
    """a fresh T is zero above the diagonal; rowscale None means ones; n = 0 and R = 0 give empty results; what the wrapper refuses"""
    n, R = T + 1, 3
    L, S, rs, P = _reference(n, R)[:4]
    for who, ops, dev in _impls(gp):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=dev)  # noqa: E731
        _, Tf = ops.tril_product(t(L), t(S), want_ssq=False, want_product=True)
        got = _np(Tf)
        assert np.array_equal(got[:, ~np.tril(np.ones((n, n), dtype=bool))], np.zeros((R, n * (n - 1) // 2))), who
        _, Tone = ops.tril_product(t(L), t(S), rowscale=t(np.ones((R, n))), want_ssq=False, want_product=True)
        assert _same_bits(got, _np(Tone)), f"{who}: rowscale None is not rowscale 1"
        ssq, none = ops.tril_product(t(L), t(S))
        assert none is None and tuple(ssq.shape) == (R, n)
        e_ssq, e_T = ops.tril_product(t(np.zeros((0, 0))), t(np.zeros((R, 0, 0))), want_product=True)
        assert tuple(e_ssq.shape) == (R, 0) and tuple(e_T.shape) == (R, 0, 0)
        z_ssq, _ = ops.tril_product(t(L), t(np.zeros((0, n, n))))
        assert tuple(z_ssq.shape) == (0, n)
        with pytest.raises(_refused()):
            ops.tril_product(t(L), t(S), want_ssq=False)                                  # neither output
        with pytest.raises(_refused()):
            ops.tril_product(t(L), t(S), rowscale=t(rs))                                  # rowscale without the product
        with pytest.raises(_refused()):
            ops.tril_product(t(L), t(S[:, :n - 1, :n - 1]))                               # shapes differ
        with pytest.raises(_refused()):
            ops.tril_product(t(L), t(S), parts=t(np.zeros((R, 1, n))))                    # parts of another extent


# ------------------------------------------------------------------------------------------------ 2. triangle and non-finite contract
def _filled_above(x, value):
    out = np.array(x, dtype=np.float64, copy=True)
    n = x.shape[-1]
    out[..., np.triu(np.ones((n, n), dtype=bool), 1)] = value
    return out


def test_nothing_above_either_diagonal_is_read(gp):
    """NaN, then 1e300, above both diagonals: ssq and T are bit-identical to the zero-filled run"""
    n, R = 2 * T + 1, 3
    L, S, rs = _reference(n, R)[:3]
    for who, ops, dev in _impls(gp):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=dev)  # noqa: E731
        base = ops.tril_product(t(_filled_above(L, 0.0)), t(_filled_above(S, 0.0)), rowscale=t(rs), want_product=True)
        for junk in (float("nan"), 1e300):
            got = ops.tril_product(t(_filled_above(L, junk)), t(_filled_above(S, junk)), rowscale=t(rs), want_product=True)
            assert _same_bits(_np(got[0]), _np(base[0])) and _same_bits(_np(got[1]), _np(base[1])), (who, junk)
        assert np.isfinite(_np(base[0])).all() and np.isfinite(_np(base[1])).all()


# (i0, k0) of a NaN planted in L, (r, k0, j0) of one planted in S_r: in the last, one-row, tile of n = 2 T + 1; and in the middle of
# tiles, where the masked partners of the planted entry share its MFMA block -- rows above k0 of the same 16 x 16 block, columns right
# of k0 -- and a zero-filled product would carry the NaN to them
L_PLANTS = [(2 * T, T + 2), (2 * T, 2 * T), (T + 72, T + 12), (T + 72, T + 70), (37, 35)]
S_PLANTS = [(1, 2 * T, 5), (1, 2 * T, 2 * T), (1, T + 72, 70), (2, T + 72, T + 66), (0, 37, 35)]


@pytest.mark.parametrize("plant", L_PLANTS)
def test_a_nan_in_L_reaches_its_own_row_only(gp, plant):
    """exactly row i0 of ssq is NaN, for every latent; of T exactly the entries [i0, j <= k0]"""
    n, R = 2 * T + 1, 3
    L, S = _reference(n, R)[:2]
    i0, k0 = plant
    Lp = np.array(L, copy=True)
    Lp[i0, k0] = float("nan")
    want = np.zeros((R, n), dtype=bool)
    want[:, i0] = True
    wantT = np.zeros((R, n, n), dtype=bool)
    wantT[:, i0, :k0 + 1] = True
    for who, ops, dev in _impls(gp):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=dev)  # noqa: E731
        ssq, Tp = ops.tril_product(t(Lp), t(S), want_product=True)
        assert np.array_equal(np.isnan(_np(ssq)), want), (who, plant)
        assert np.array_equal(np.isnan(_np(Tp)), wantT), (who, plant)


@pytest.mark.parametrize("plant", S_PLANTS)
def test_a_nan_in_S_reaches_the_rows_from_its_own_down(gp, plant):
    """exactly the rows i >= k0 of latent r are NaN in ssq; of T exactly the entries [r, i >= k0, j0]"""
    n, R = 2 * T + 1, 3
    L, S = _reference(n, R)[:2]
    r, k0, j0 = plant
    Sp = np.array(S, copy=True)
    Sp[r, k0, j0] = float("nan")
    want = np.zeros((R, n), dtype=bool)
    want[r, k0:] = True
    wantT = np.zeros((R, n, n), dtype=bool)
    wantT[r, k0:, j0] = True
    for who, ops, dev in _impls(gp):
        t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, device=dev)  # noqa: E731
        ssq, Tp = ops.tril_product(t(L), t(Sp), want_product=True)
        assert np.array_equal(np.isnan(_np(ssq)), want), (who, plant)
        assert np.array_equal(np.isnan(_np(Tp)), wantT), (who, plant)


# ------------------------------------------------------------------------------------------------ 3. the scratch operand
@pytest.mark.parametrize("n,R", [(2 * T + 1, 3), (T - 1, 1)])
def test_parts_is_scratch_with_a_documented_extent(gp, n, R):
    """`parts` [R, ceil(n / T), n] poisoned (all NaN, then all 0x7F bytes) between two guard zones: the results are the bits of a run
    on a fresh scratch, and the guards keep theirs"""
    GUARD = 64
    nt = -(-n // T)
    for who, ops, dev in _impls(gp):
        base, _, _, _ = _run(ops, dev, n, R, "c", "ssq")
        assert tuple(ops.tril_product_parts(n, R).shape) == (R, nt, n)
        for poison in ("nan", "0x7f"):
            raw = np.full(R * nt * n + 2 * GUARD, np.nan) if poison == "nan" else \
                np.frombuffer(b"\x7f" * (8 * (R * nt * n + 2 * GUARD)), dtype=np.float64).copy()
            guard = np.frombuffer(b"\x5a" * (8 * GUARD), dtype=np.float64)
            raw[:GUARD] = guard
            raw[-GUARD:] = guard
            buf = torch.tensor(raw, dtype=torch.float64, device=dev)
            parts = buf[GUARD:GUARD + R * nt * n].view(R, nt, n)
            got, _, _, _ = _run(ops, dev, n, R, "c", "ssq", parts=parts)
            after = _np(buf)
            assert _same_bits(got, base), (who, poison)
            assert _same_bits(after[:GUARD], guard) and _same_bits(after[-GUARD:], guard), (who, poison, "a guard zone was written")


def test_refusals_of_the_library_write_nothing():
    """GPK_E_ARG (-1) before any launch for every case of include/gpk.h, with HOST buffers in the pointer slots (a refused call
    enqueues nothing, so they are never dereferenced): nothing is written; n == 0 or R == 0 returns 0 and writes nothing either"""
    from gpflow_amd import _lib
    lib = _lib.load()
    assert lib.gpk_tril_product_tiles(0) == 0 and [lib.gpk_tril_product_tiles(k) for k in (1, T, T + 1, 3 * T + 2)] == [1, 1, 2, 4]
    bufs = [(ctypes.c_double * 64)(*([PATTERN] * 64)) for _ in range(6)]
    L, S, ssq, parts, rs, Tp = (ctypes.cast(b, ctypes.c_void_p).value for b in bufs)

    def call(n=4, ldl=4, lds=4, R=2, L=L, S=S, ssq=ssq, parts=parts, rs=None, Tp=None, ldt=4):
        return lib.gpk_tril_product(None, L, n, ldl, S, lds, 16, R, ssq, parts, rs, Tp, ldt, 16)
    assert call(n=-1) == -1 and call(R=-1) == -1
    assert call(ldl=3) == -1 and call(lds=3) == -1 and call(Tp=Tp, ldt=3) == -1
    assert call(L=None) == -1 and call(S=None) == -1
    assert call(ssq=None) == -1                                  # neither output
    assert call(parts=None) == -1                                # the row sums need their scratch
    assert call(rs=rs) == -1                                     # rowscale goes with the stored product
    assert call(n=0) == 0 and call(R=0) == 0 and call(n=0, L=None, S=None, ssq=None, parts=None) == 0
    for b in bufs:
        assert list(b) == [PATTERN] * 64


# ------------------------------------------------------------------------------------------------ 4. model values
def _data(lik, N, D, R, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.5, 1.5, size=(N, D))
    f = np.sin(X.sum(1, keepdims=True) + np.arange(R)[None, :])
    if lik == "gaussian" or lik == "student_t":
        Y = f + 0.3 * rng.normal(size=(N, R))
    elif lik == "bernoulli_probit":
        Y = (f + 0.3 * rng.normal(size=(N, R)) > 0).astype(np.float64)
    elif lik in ("exponential_exp", "gamma_exp"):
        Y = rng.exponential(size=(N, R)) * np.exp(0.5 * f) + 0.05
    else:
        Y = rng.integers(0, R, size=(N, 1)).astype(np.float64)
    q_mu = 0.3 * rng.normal(size=(N, R))
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(N, N))) + 0.6 * np.eye(N) for _ in range(R)])
    return X, Y, q_mu, q_sqrt


def _ve_torch(lik, par, fmean, fvar, Y):
    """sum of the variational expectations on torch-CPU fp64 tensors (par: floats, a trainable one a tensor)"""
    if lik == "gaussian":
        s2 = par[0]
        return (-0.5 * math.log(2 * math.pi) - 0.5 * torch.log(s2) - 0.5 * ((Y - fmean) ** 2 + fvar) / s2).sum()
    if lik in ("exponential_exp", "gamma_exp"):
        return _torch_ve(lik, par, fmean, fvar, Y)
    x, wn = torch.tensor(GH_X), torch.tensor(GH_W / np.sqrt(np.pi))
    if lik == "multiclass_robustmax":   # multiclass.py: the quadrature of the definition, as tests/test_gpu_multiclass.py restates it
        C, eps = fmean.shape[1], par[0]
        on = torch.nn.functional.one_hot(Y[:, 0].long(), C).to(torch.float64)
        mu_y, v_y = (on * fmean).sum(1, keepdim=True), (on * fvar).sum(1, keepdim=True)
        Xh = mu_y + torch.sqrt(torch.clamp(2 * v_y, min=1e-10)) * x
        d = (Xh[:, None, :] - fmean[:, :, None]) / torch.sqrt(torch.clamp(fvar, min=1e-10))[:, :, None]
        cdf = 0.5 * (1 + torch.special.erf(d / math.sqrt(2.0))) * (1 - 2e-4) + 1e-4
        cdf = cdf * (1 - on)[:, :, None] + on[:, :, None]
        p = (torch.prod(cdf, dim=1) * wn).sum(-1)
        return (p * math.log1p(-eps) + (1 - p) * math.log(eps / (C - 1))).sum()
    f = fmean[..., None] + torch.sqrt(2 * fvar)[..., None] * x
    y = Y[..., None]
    if lik == "bernoulli_probit":
        p = 0.5 * (1 + torch.special.erf(f / math.sqrt(2.0))) * (1 - 2e-3) + 1e-3
        g = torch.log(torch.where(y == 1, p, 1 - p))
    else:
        assert lik == "student_t"
        s, df = par
        g = torch.lgamma(torch.tensor((df + 1) / 2, dtype=torch.float64)) - torch.lgamma(torch.tensor(df / 2, dtype=torch.float64)) \
            - 0.5 * (torch.log(s * s) + math.log(df) + math.log(math.pi)) - 0.5 * (df + 1) * torch.log(1 + ((y - f) / s) ** 2 / df)
    return (g * wn).sum()


def _torch_moments(X, q_mu, q_sqrt, kfun, mean):
    """(fmean [N, R], fvar [N, R], L) of q(f) at the data: vgp.py:138-152 with the dense product L @ tril(q_sqrt)"""
    N = X.shape[0]
    L = torch.linalg.cholesky(kfun(X, X) + JITTER * torch.eye(N, dtype=torch.float64))
    LS = L[None] @ torch.tril(q_sqrt)
    return L @ q_mu + mean, (LS * LS).sum(-1).T, L


def _torch_elbo(lik, par, X, Y, q_mu, q_sqrt, kfun, mean):
    """VGP.elbo (vgp.py:131-155) on torch-CPU fp64 tensors: for the values, and for autograd"""
    N, R = q_mu.shape
    fmean, fvar, _ = _torch_moments(X, q_mu, q_sqrt, kfun, mean)
    S = torch.tril(q_sqrt)
    kl = 0.5 * ((q_mu * q_mu).sum() - N * R - torch.log(torch.diagonal(S, dim1=1, dim2=2) ** 2).sum() + (S * S).sum())
    return _ve_torch(lik, par, fmean, fvar, Y) - kl


def _likelihood(gp, lik):
    """(likelihood object, its parameters as the restatement takes them, the name of the trainable one | None)"""
    Ls = gp.likelihoods
    return {"gaussian": lambda: (Ls.Gaussian(0.3), (0.3,), "variance"),
            "bernoulli_probit": lambda: (Ls.Bernoulli(), (), None),
            "exponential_exp": lambda: (Ls.Exponential(), (), None),
            "gamma_exp": lambda: (Ls.Gamma(shape=1.6), (1.6,), "shape"),
            "student_t": lambda: (Ls.StudentT(scale=0.7, df=4.0), (0.7, 4.0), "scale"),
            "multiclass_robustmax": lambda: (Ls.MultiClass(3), (1e-3,), None)}[lik]()


def _se(variance=1.3, ls=0.9):
    return lambda A, B: orcg._rbf(A, B, variance, ls)


def _closed_form(X, Y, s2, mean, variance=1.3, ls=0.9):
    """The optimum of the Gaussian case in whitened coordinates, in NumPy: Sigma = (I + L^T L / s2)^-1, q_mu = Sigma L^T (y - m) / s2,
    q_sqrt = chol(Sigma), the ELBO there written out, and log N(y | m, K + (s2 + jitter) I) from SciPy.  The jitter sits in the
    VGP's prior, so the marginal it bounds is that of K + jitter I under noise s2."""
    from scipy.stats import multivariate_normal
    N = X.shape[0]
    K = _np(_se(variance, ls)(_t(X), _t(X))) + JITTER * np.eye(N)
    L = np.linalg.cholesky(K)
    Sigma = np.linalg.inv(np.eye(N) + L.T @ L / s2)
    q_mu = Sigma @ L.T @ (Y - mean) / s2
    q_sqrt = np.linalg.cholesky(Sigma)
    LS = L @ q_sqrt
    fmean, fvar = L @ q_mu + mean, (LS * LS).sum(1, keepdims=True)
    ve = (-0.5 * np.log(2 * np.pi) - 0.5 * np.log(s2) - 0.5 * ((Y - fmean) ** 2 + fvar) / s2).sum()
    kl = 0.5 * ((q_mu ** 2).sum() - N - np.log(np.diag(q_sqrt) ** 2).sum() + (q_sqrt ** 2).sum())
    logpdf = float(multivariate_normal.logpdf(Y[:, 0], mean=np.full(N, mean), cov=K + s2 * np.eye(N)))
    return q_mu, q_sqrt[None], float(ve - kl), logpdf


def test_closed_form_identity_in_numpy():
    """at the closed-form optimum the bound is tight: the ELBO written out in NumPy equals SciPy's log density (no device involved)"""
    X, Y, _, _ = _data("gaussian", 150, 2, 1, 5)
    _, _, elbo, logpdf = _closed_form(X, Y, 0.3, 0.2)
    assert abs(elbo - logpdf) <= 1e-10 * abs(logpdf), (elbo, logpdf)


def test_gaussian_vgp_at_its_optimum_is_the_gpr(gp):
    """VGP.elbo() at the closed-form optimum == GPR(noise_variance = s2 + jitter).log_marginal_likelihood() == SciPy's logpdf, 1e-8"""
    N, s2, c = 150, 0.3, 0.2
    X, Y, _, _ = _data("gaussian", N, 2, 1, 5)
    q_mu, q_sqrt, elbo_np, logpdf = _closed_form(X, Y, s2, c)
    assert abs(elbo_np - logpdf) <= 1e-10 * abs(logpdf)
    K = gp.kernels
    m = gp.models.VGP((X, Y), K.SquaredExponential(variance=1.3, lengthscales=0.9), gp.likelihoods.Gaussian(s2),
                      mean_function=gp.mean_functions.Constant(c))
    assert m.q_mu.shape == (N, 1) and m.q_sqrt.shape == (1, N, N) and m.num_latent_gps == 1
    assert np.array_equal(m.q_mu.numpy(), np.zeros((N, 1))) and np.array_equal(m.q_sqrt.numpy(), np.eye(N)[None])
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    got = float(m.elbo())
    gpr = gp.models.GPR((X, Y), K.SquaredExponential(variance=1.3, lengthscales=0.9), mean_function=gp.mean_functions.Constant(c),
                        noise_variance=s2 + JITTER)
    lml = float(gpr.log_marginal_likelihood())
    print(f"VGP elbo {got!r} GPR lml {lml!r} SciPy {logpdf!r}")
    assert abs(got - lml) <= ELBO_TOL * abs(lml) and abs(got - logpdf) <= ELBO_TOL * abs(logpdf)
    assert float(m.maximum_log_likelihood_objective()) == got and abs(float(m.training_loss()) + got) <= 1e-12 * abs(got)


VALUE_LIKS = ["exponential_exp", "bernoulli_probit", "student_t", "multiclass_robustmax"]   # closed form, per-node, a trained parameter, coupled latents


@pytest.mark.parametrize("lik", VALUE_LIKS)
def test_vgp_elbo_against_the_restated_reference(gp, lik):
    """random q_mu, q_sqrt (junk above the diagonal of what the restatement gets -- the Parameter keeps the triangle only): elbo()
    against the restatement, 1e-8 relative"""
    N, D = 150, 2
    R = 3 if lik == "multiclass_robustmax" else 2
    X, Y, q_mu, q_sqrt = _data(lik, N, D, R, 11)
    likelihood, par, _ = _likelihood(gp, lik)
    m = gp.models.VGP((X, Y), gp.kernels.SquaredExponential(variance=1.3, lengthscales=0.9), likelihood,
                      mean_function=gp.mean_functions.Constant(0.2))
    assert m.num_latent_gps == R
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    tpar = tuple(torch.tensor(p, dtype=torch.float64) if i == 0 and lik == "student_t" else p for i, p in enumerate(par))
    ref = float(_torch_elbo(lik, tpar, _t(X), _t(Y), _t(q_mu), _t(q_sqrt + np.triu(np.ones((N, N)), 1) * 0.37), _se(), 0.2))
    got = float(m.elbo())
    print(f"{lik}: elbo {got!r} restatement {ref!r} relative error {abs(got - ref) / abs(ref):.3g}")
    assert abs(got - ref) <= ELBO_TOL * abs(ref)


# ------------------------------------------------------------------------------------------------ 5. gradients
GRAD_LIKS = ["gaussian", "bernoulli_probit", "gamma_exp", "multiclass_robustmax"]
KPAR = dict(v0=1.3, l0=0.8, v1=0.7, l1=1.1)


def _sum_kernel(gp):
    K = gp.kernels
    return K.SquaredExponential(variance=KPAR["v0"], lengthscales=KPAR["l0"], active_dims=[0]) \
        + K.Matern32(variance=KPAR["v1"], lengthscales=KPAR["l1"], active_dims=[1])


def _sum_kfun(v):
    k0 = _torch_kernel("SquaredExponential", v["v0"], v["l0"], cols=[0])
    k1 = _torch_kernel("Matern32", v["v1"], v["l1"], cols=[1])
    return lambda A, B: k0(A, B) + k1(A, B)


def _grad_model(gp, lik, seed=21):
    N, D = 150, 2
    R = 3 if lik == "multiclass_robustmax" else 2
    X, Y, q_mu, q_sqrt = _data(lik, N, D, R, seed)
    likelihood, par, trained = _likelihood(gp, lik)
    m = gp.models.VGP((X, Y), _sum_kernel(gp), likelihood, mean_function=gp.mean_functions.Constant(0.2))
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    return m, (X, Y), par, trained


def _autograd_at(gp, m, lik, data, par, trained):
    """(value, {name: gradient w.r.t. the constrained value}) of the restated ELBO at the model's CURRENT parameter values"""
    X, Y = data
    leaf = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=True)  # noqa: E731
    k0, k1 = m.kernel.kernels
    v = {"v0": leaf(k0.variance.numpy()), "l0": leaf(k0.lengthscales.numpy()), "v1": leaf(k1.variance.numpy()),
         "l1": leaf(k1.lengthscales.numpy()), "q_mu": leaf(m.q_mu.numpy()), "q_sqrt": leaf(m.q_sqrt.numpy()),
         "mean": leaf(m.mean_function.c.numpy())}
    tpar = par
    if trained is not None:
        v["lik"] = leaf(getattr(m.likelihood, trained).numpy())
        tpar = (v["lik"],) + tuple(par[1:])
    F = _torch_elbo(lik, tpar, _t(X), _t(Y), v["q_mu"], v["q_sqrt"], _sum_kfun(v), v["mean"])
    F.backward()
    return float(F.detach()), {k: a.grad.detach().numpy().copy() for k, a in v.items()}


def _check_grads(name, m, g, go, trained):
    """every trainable Parameter's d/d(unconstrained) against autograd's constrained gradient chained through the transform
    (fill-triangular: the vector entries ARE the lower-triangular ones)"""
    k0, k1 = m.kernel.kernels
    pars = {"v0": k0.variance, "l0": k0.lengthscales, "v1": k1.variance, "l1": k1.lengthscales, "q_mu": m.q_mu, "mean": m.mean_function.c}
    if trained is not None:
        pars["lik"] = getattr(m.likelihood, trained)
    assert set(g) == set(pars.values()) | {m.q_sqrt} and len(g) == len(m.trainable_parameters), name
    for key, par in pars.items():
        u = par.unconstrained_variable
        ref = go[key].reshape(np.shape(u)) * par.transform.forward_grad(u)
        _close(f"{name} {key}", np.asarray(g[par]), ref, GRAD_TOL)
    ref = m.q_sqrt.transform.inverse(np.tril(go["q_sqrt"]))
    _close(f"{name} q_sqrt", np.asarray(g[m.q_sqrt]), ref.reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)


@pytest.mark.parametrize("lik", GRAD_LIKS)
def test_objective_and_grad_against_autograd(gp, lik):
    """VGP.objective_and_grad() with SquaredExponential(active_dims=[0]) + Matern32(active_dims=[1]) and a constant mean against
    torch-CPU fp64 autograd of the restated ELBO: the value 1e-9, every trainable parameter 1e-8 -- both members' variances and
    lengthscales, q_mu, q_sqrt, the likelihood's own parameter (Gaussian variance, Gamma shape) and the mean constant"""
    m, data, par, trained = _grad_model(gp, lik)
    v, g = m.objective_and_grad()
    ref, go = _autograd_at(gp, m, lik, data, par, trained)
    print(f"{lik}: value {v!r} autograd {ref!r}")
    assert abs(v - ref) <= VALUE_TOL * abs(ref)
    assert abs(v - float(m.elbo())) <= VALUE_TOL * abs(v)
    _check_grads(lik, m, g, go, trained)


@pytest.mark.parametrize("lik", ["gaussian", "bernoulli_probit"])
def test_q_sqrt_gradient_is_exactly_zero_above_the_diagonal(gp, lik):
    """gradients.vgp_elbo_and_grad with junk above the diagonal of q_sqrt: the same bits as without it, and exact zeros there"""
    N, D, R = 150, 2, 2
    X, Y, q_mu, q_sqrt = _data(lik, N, D, R, 33)
    t = gp.ops.to_device
    spec = gp.gradients.KernelSpec.single(1.3, 0.9)
    kw = dict(noise_variance=0.3) if lik == "gaussian" else dict(likelihood=(lik, ()))
    junk = q_sqrt + np.triu(np.ones((N, N)), 1)[None] * 0.37
    F0, g0, _ = gp.gradients.vgp_elbo_and_grad(t(X), t(Y), t(q_mu), t(q_sqrt), kernel_spec=spec, jitter=JITTER, mean_const=0.1, **kw)
    F1, g1, info = gp.gradients.vgp_elbo_and_grad(t(X), t(Y), t(q_mu), t(junk), kernel_spec=spec, jitter=JITTER, mean_const=0.1, **kw)
    gp.ops.check_info(info)
    gq = _np(g1["q_sqrt"])
    assert gq.shape == (R, N, N) and np.array_equal(gq[:, np.triu(np.ones((N, N), dtype=bool), 1)], np.zeros((R, N * (N - 1) // 2)))
    assert _same_bits(_np(F0), _np(F1)) and all(_same_bits(_np(g0[k]), _np(g1[k])) for k in ("q_mu", "q_sqrt", "variance", "lengthscales"))
    assert ("noise_variance" in g1) == (lik == "gaussian")


# ------------------------------------------------------------------------------------------------ 6. routes
@pytest.mark.parametrize("full_cov", [False, True])
def test_predict_f_is_the_whitened_conditional(gp, full_cov):
    """predict_f == conditional(Xnew, X, kernel, q_mu, q_sqrt=q_sqrt, white=True) + mean bit for bit, and the restatement 1e-9"""
    N, D, R = 150, 2, 2
    X, Y, q_mu, q_sqrt = _data("gaussian", N, D, R, 41)
    Xnew = np.random.default_rng(42).uniform(-1.5, 1.5, size=(37, D))
    kern = gp.kernels.SquaredExponential(variance=1.3, lengthscales=0.9)
    m = gp.models.VGP((X, Y), kern, gp.likelihoods.Gaussian(0.3), mean_function=gp.mean_functions.Constant(0.2))
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    mu, var = m.predict_f(Xnew, full_cov=full_cov)
    cmu, cvar = gp.conditionals.conditional(Xnew, X, kern, m.q_mu.device_value(), q_sqrt=m.q_sqrt.device_value(), white=True, full_cov=full_cov)
    assert _same_bits(_np(mu), _np(cmu + 0.2)) and _same_bits(_np(var), _np(cvar))
    k = _se()
    tX, tN = _t(X), _t(Xnew)
    L = torch.linalg.cholesky(k(tX, tX) + JITTER * torch.eye(N, dtype=torch.float64))
    A = torch.linalg.solve_triangular(L, k(tX, tN), upper=False)                          # [N, new]
    SA = torch.tril(_t(q_sqrt)).transpose(1, 2) @ A                                       # [R, N, new]
    rmu = A.T @ _t(q_mu) + 0.2
    if full_cov:
        rvar = (k(tN, tN) - A.T @ A)[None] + SA.transpose(1, 2) @ SA
    else:
        rvar = (1.3 - (A * A).sum(0))[:, None] + (SA * SA).sum(1).T
    _close("predict_f mean", mu, rmu.numpy(), PREDICT_TOL)
    _close("predict_f var", var, rvar.numpy(), PREDICT_TOL)
    ymu, yvar = m.predict_y(Xnew)
    assert tuple(ymu.shape) == (37, R) and bool(torch.isfinite(yvar).all())
    assert tuple(m.predict_log_density((X[:5], Y[:5])).shape) == (5,) and tuple(m.predict_f_samples(Xnew[:4], 3).shape) == (3, 4, R)


def test_scipy_lowers_the_objective_of_a_bernoulli_model(gp):
    """optimizers.Scipy, five iterations one at a time: the training loss never rises and ends lower; the gradient at the final point
    agrees with autograd there"""
    lik = "bernoulli_probit"
    N, D = 150, 2
    X, Y, _, _ = _data(lik, N, D, 1, 51)
    m = gp.models.VGP((X, Y), _sum_kernel(gp), gp.likelihoods.Bernoulli(), mean_function=gp.mean_functions.Constant(0.0))
    losses = [float(m.training_loss())]
    for _ in range(5):
        gp.optimizers.Scipy().minimize(m, options=dict(maxiter=1))
        losses.append(float(m.training_loss()))
    print("training loss per iteration:", losses)
    assert all(b <= a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0] - 1.0
    v, g = m.objective_and_grad()
    ref, go = _autograd_at(gp, m, lik, (X, Y), (), None)
    assert abs(v - ref) <= VALUE_TOL * abs(ref) and abs(v + losses[-1]) <= VALUE_TOL * abs(v)
    _check_grads("after Scipy", m, g, go, None)


def test_refusals_come_before_any_device_call(gp, monkeypatch):
    """heteroskedastic Gaussian noise, a multi-output kernel, a likelihood without `device_lik`, MultiClass with the wrong number of
    latents: NotImplementedError (ValueError for the last) when the model is built, with not one call into gpflow_amd.ops"""
    ops = gp.ops
    X, Y, _, _ = _data("gaussian", 20, 2, 1, 61)
    K, Ls = gp.kernels, gp.likelihoods

    class NoDevice(Ls.ScalarLikelihood):
        device_lik = ""
    het = Ls.Gaussian(scale=gp.functions.Linear(A=np.ones((2, 1)), b=np.ones(1)))
    assert het.is_heteroskedastic
    shared = K.SharedIndependent(K.SquaredExponential(), output_dim=1)
    calls = []
    for name in dir(ops):
        fn = getattr(ops, name)
        if not name.startswith("_") and callable(fn) and not isinstance(fn, type):
            monkeypatch.setattr(ops, name, (lambda n, f: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(name, fn))
    for kern, lik, exc in ((K.SquaredExponential(), het, NotImplementedError), (shared, Ls.Gaussian(0.1), NotImplementedError),
                           (K.SquaredExponential(), NoDevice(), NotImplementedError)):
        with pytest.raises(exc):
            gp.models.VGP((X, Y), kern, lik)
    with pytest.raises(ValueError):
        gp.models.VGP((X, Y), K.SquaredExponential(), Ls.MultiClass(3), num_latent_gps=2)
    mean = gp.mean_functions.Linear(A=np.ones((2, 1)), b=np.zeros(1))
    with pytest.raises(NotImplementedError):
        gp.models.VGP((X, Y), K.SquaredExponential(), Ls.Gaussian(0.1), mean_function=mean)
    assert calls == [], calls
