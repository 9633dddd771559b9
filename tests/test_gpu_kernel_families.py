"""GPU tests of the kernel families added to the covariance builder -- Exponential, RationalQuadratic, White, Constant: the
primitives (`ops.kernel_matrix`, `kernel_matrix_combine` with its fourth op "dalpha", `kernel_matrix_hadamard`), the fused
drivers that forward a family, the reverse pass (`gradients.*`, `KernelSpec` with `alpha` and static members) and the model surface.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_kernel_families_emulated.py imports them without this
module's `gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py).  On the device every primitive case also runs the
emulation beside it (`_impls`: test_gpu_contract's pair, tests/fake_ops.py, which knows the eight families).

References.  Primitives: the method of test_gpu_contract._kref -- the same expansion formula in np.longdouble and a bound derived
from it (`_kref_new`, u = 2^-53).  Fused paths and gradients: torch autograd through the unchanged oracle
(oracle/gp_oracle_grad.py: svgp_elbo_torch, gpr_lml_torch, sgpr_elbo_torch with `kfun` / `kdiag`) over torch restatements of the
four kernels (`_torch_kernel`), alpha a leaf tensor.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_ops  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _kdata, _np, _on, _within  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

STATIC = ("White", "Constant")
# (family, alpha): RationalQuadratic at a heavy-tailed, the default and a near-SquaredExponential alpha
FAMS = [("Exponential", None), ("RationalQuadratic", 0.3), ("RationalQuadratic", 1.0), ("RationalQuadratic", 4.0), ("White", None),
        ("Constant", None)]
FAM_IDS = [f if a is None else f"{f}-{a}" for f, a in FAMS]


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    """where `gp.ops` keeps its tensors: the HIP device, or the CPU under the emulation"""
    return str(gp.ops.device())


def _impls(gp):
    """test_gpu_contract._impls for the extended primitives: gp.ops, and beside a real device the emulation on the same inputs"""
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("fake_ops", fake_ops, "cpu")] if dev != "cpu" else [])


def _akw(alpha):
    return {} if alpha is None else {"alpha": alpha}


# ------------------------------------------------------------------------------------------------ 1. the primitive contract
def _kfun(family, r2, variance, alpha=None, op="k"):
    """test_gpu_contract._kfun restated for the new stationary families, in longdouble: k, -2 dk/dr2 ("dr2"), dk/dalpha ("dalpha")
    and d(dk/dalpha)/dr2 ("dalpha_dr2", for the bound of the one profile that is not monotone in r2)"""
    r2 = np.asarray(r2, dtype=LD)
    if family == "Exponential":
        if op == "dr2":
            ok = r2 > 1e-36
            r = np.sqrt(np.where(ok, r2, 1))
            return np.where(ok, variance * np.exp(-r / 2) / (2 * r), 0)
        return variance * np.exp(-np.sqrt(np.maximum(r2, LD(1e-36))) / 2)
    assert family == "RationalQuadratic"
    a = LD(alpha)
    u = r2 / (2 * a)
    l1p = np.log1p(u)
    k = variance * np.exp(-a * l1p)
    if op == "k":
        return k
    if op == "dr2":
        return variance * np.exp(-(a + 1) * l1p)
    g = u / (1 + u) - l1p
    if op == "dalpha":
        return k * g
    # d/dr2 of k g:  (k' g + k g') / (2 alpha),  k' = -alpha k / (1 + u),  g' = -u / (1 + u)^2
    return (-a * k / (1 + u) * g - k * u / (1 + u) ** 2) / (2 * a)


def _kref_new(family, X1, X2, variance, ls, alpha=None, op="k"):
    """Reference (k | -2 dk/dr2 | dk/dalpha)(X1, X2 or X1) in longdouble, its bound and `zero_ok`, by the method of
    test_gpu_contract._kref.  delta = (d + 4) u (|a|^2 + |b|^2) is what the fp64 expansion (scaling by 1 / ls included) can move r2 by.
      k and -2 dk/dr2 of both families are monotone in r2: the interval f(r2 -+ delta) bounds a correctly evaluated profile; + 8 u |f|
      for exp / sqrt / log1p / the products (a few ulp each); RationalQuadratic: + 4 (alpha + 1) log1p(u) u |f| -- the exponential's
      ARGUMENT (alpha + 1) log1p(u) carries a relative error of a few u, which exp turns into that absolute error of its value.
      dk/dalpha = k (u / (1 + u) - log1p(u)) is not monotone in r2: the larger of the endpoint deviations and |d f / d r2| delta, plus
      the same two ulp terms taken on |k| -- the factor g = u / (1 + u) - log1p(u) lies in [-log1p(u), 0] and is a difference of two
      terms of size <= log1p(u), so its rounding error is a few u log1p(u), absolute, and enters multiplied by |k|, not by |k g|.
    White / Constant: exact, no bound of their own.  zero_ok: where the 1e-36 clamp of the Exponential's dr2 may legitimately switch
    to 0 (r2 - delta <= 1e-36), off the diagonal of the symmetric form (which is exactly 0 by contract and compared as such)."""
    sym = X2 is None
    X2 = X1 if sym else X2
    n1, n2 = X1.shape[0], X2.shape[0]
    none = np.zeros((n1, n2), dtype=bool)
    if family in STATIC:
        k = np.zeros((n1, n2), dtype=LD)
        if op == "k":
            k = k + variance if family == "Constant" else (variance * np.eye(n1, dtype=LD) if sym else k)
        return k, np.zeros((n1, n2), dtype=LD), none
    d = X1.shape[1]
    lsv = np.broadcast_to(np.asarray(ls, dtype=LD), (d,))
    a, b = X1.astype(LD) / lsv, X2.astype(LD) / lsv
    na, nb = (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
    r2 = -2 * (a @ b.T) + na + nb
    delta = (d + 4) * U * (na + nb)
    lo, hi = np.maximum(r2 - delta, 0), r2 + delta
    f = _kfun(family, r2, variance, alpha, op)
    bnd = np.maximum(np.abs(_kfun(family, lo, variance, alpha, op) - f), np.abs(_kfun(family, hi, variance, alpha, op) - f))
    mag = np.abs(f)
    if op == "dalpha":
        bnd = np.maximum(bnd, np.abs(_kfun(family, r2, variance, alpha, "dalpha_dr2")) * delta)
        mag = np.abs(_kfun(family, r2, variance, alpha, "k"))
    bnd = bnd + 8 * U * mag + LD(1e-300)
    if family == "RationalQuadratic":
        bnd = bnd + 4 * (LD(alpha) + 1) * np.abs(np.log1p(r2 / (2 * LD(alpha)))) * U * mag
    zero_ok = (r2 - delta <= 1e-36) if (op == "dr2" and family == "Exponential") else none
    if sym:
        zero_ok = zero_ok & ~np.eye(n1, dtype=bool)
    return f, bnd, zero_ok


def _data(case_seed, n1, n2, d, kind):
    """(X1, X2 | None, planted): test_gpu_contract._kdata; for "dup" data of a cross case X2 is X1 moved by 1e-9 (pair (i, i) sits at
    the clamp) and one pair is planted exactly coincident, X2[2] = X1[0] -- its r2 is rounding noise on either side of the clamp"""
    rng = np.random.default_rng(case_seed)
    cross_dup = kind == "dup" and n2 == n1
    X1 = _kdata(rng, n1, d, "normal" if cross_dup else kind)
    if n2 is None:
        return X1, None, None
    if cross_dup:
        X2 = X1 + 1e-9 * rng.normal(size=X1.shape)
        X2[2] = X1[0]
        return X1, X2, (0, 2)
    return X1, _kdata(rng, n2, d, kind), None


def _ls(d, ard, c=0.9):
    return (0.6 + 0.05 * np.arange(d)) if ard else c * np.sqrt(d)


# (n1, n2 (None: symmetric), d, ard, data, layout, lower_only, diag_add) -- the shapes of test_gpu_contract.KM_CASES
KM_CASES = [
    (1, 1, 1, False, "normal", "c", False, 0.0),        # sizes 1
    (0, 5, 2, False, "normal", "c", False, 0.0),        # empty operands
    (63, 65, 3, True, "normal", "c", False, 0.0),       # tile edges 63 / 65, ARD
    (127, 129, 16, True, "normal", "ld", False, 0.0),   # tile edges, odd leading dimensions
    (255, 257, 8, False, "far", "off", False, 0.0),     # offset data (cancellation), misaligned pointers
    (64, 64, 2, False, "dup", "c", False, 0.0),         # near-duplicate pairs: the Exponential clamp
    (130, None, 4, False, "dup", "c", False, 0.1),      # symmetric + diag_add, near duplicates
    (257, None, 5, True, "normal", "c", True, 0.3),     # lower_only + diag_add: unwritten upper tiles keep their value
    (100, 70, 64, False, "normal", "col", False, 0.0),  # d = 64 (the maximum), column slices
]
# ops x (n1, n2, d, data, layout)
KC_CASES = [(op, 65, 63, 3, "normal", "ld") for op in ("mul", "add", "dr2", "dalpha")] \
    + [(op, 129, None, 2, "normal", "c") for op in ("mul", "add", "dr2", "dalpha")] \
    + [("dr2", 64, 64, 2, "dup", "c"), ("dr2", 130, None, 3, "normal", "off"), ("dalpha", 130, None, 3, "normal", "off")]


@pytest.mark.parametrize("fam", FAMS, ids=FAM_IDS)
@pytest.mark.parametrize("case", KM_CASES, ids=[str(c) for c in KM_CASES])
def test_kernel_matrix_new_families(gp, case, fam):
    (family, alpha), (n1, n2, d, ard, data, layout, lower_only, diag_add) = fam, case
    X1, X2, _ = _data(n1 + 3 * d, n1, n2, d, data)
    ls = _ls(d, ard)
    k, bnd, _ = _kref_new(family, X1, X2, 1.7, ls, alpha)
    if X2 is None:
        k = k + diag_add * np.eye(n1, dtype=LD)
        bnd = bnd + U * np.abs(k)
    for who, impl, dev in _impls(gp):
        t1 = _on(X1, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        out = _on(np.full(k.shape, -555.0), "c", dev) if lower_only else None
        K = _np(impl.kernel_matrix(t1, t2, variance=1.7, lengthscales=ls, family=family, diag_add=diag_add, lower_only=lower_only,
                                   out=out, **_akw(alpha)))
        name = f"kernel_matrix {family} {who}"
        if lower_only:   # only the lower triangle is defined; above it: the untouched sentinel / NaN, or a correct value
            low = np.tril(np.ones(k.shape, dtype=bool))
            _within(name, np.where(low, K, 0), np.where(low, k, 0), np.where(low, bnd, 0))
            up = ~low & ~np.isnan(K) & (K != -555.0)
            _within(name + " upper", K[up], k[up], bnd[up])
        else:
            _within(name, K, k, bnd)
        _check_unchanged(name, [t1] + ([t2] if t2 is not None else []), [X1] + ([X2] if X2 is not None else []))


# (op "dalpha" exists for the RationalQuadratic alone; its refusal for the others: test_refusals)
KC_PAIRS = [(c, f) for c in KC_CASES for f in FAMS if c[0] != "dalpha" or f[0] == "RationalQuadratic"]


@pytest.mark.parametrize("case,fam", KC_PAIRS, ids=[f"{c}-{f}-{a}" for c, (f, a) in KC_PAIRS])
def test_kernel_matrix_combine_new_families(gp, case, fam):
    (family, alpha), (op, n1, n2, d, data, layout) = fam, case
    X1, X2, planted = _data(17 + n1 + d, n1, n2, d, data)
    G = np.random.default_rng(n1).normal(size=(n1, n1 if n2 is None else n2))
    ls, diag = _ls(d, False, 0.8), (0.2 if n2 is None else 0.0)
    k, bnd, zero_ok = _kref_new(family, X1, X2, 1.3, ls, alpha, op if op in ("dr2", "dalpha") else "k")
    g = G.astype(LD)
    if op in ("dr2", "dalpha"):
        ref, rb = k * g, bnd * np.abs(g) + U * np.abs(k * g)
        if X2 is None:
            np.fill_diagonal(ref, 0)
            np.fill_diagonal(rb, 0)
    else:
        ref = k * g if op == "mul" else k + g
        rb = (bnd * np.abs(g) if op == "mul" else bnd) + 2 * U * np.abs(ref)
        if X2 is None:
            ref = ref + diag * np.eye(n1, dtype=LD)
            rb = rb + U * np.abs(ref)
    keep = np.ones(ref.shape, dtype=bool)
    if planted is not None:
        keep[planted] = False     # (the one exactly coincident pair: noise-level r2, not comparable)
    for who, impl, dev in _impls(gp):
        t1, tG = _on(X1, layout, dev), _on(G, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        R = _np(impl.kernel_matrix_combine(t1, t2, tG, op=op, variance=1.3, lengthscales=ls, family=family, diag_add=diag, **_akw(alpha)))
        name = f"kernel_matrix_combine {op} {family} {who}"
        if op in ("dr2", "dalpha") and X2 is None:
            assert np.all(np.diagonal(R) == 0), f"{name}: diagonal not exactly zero"
        Rc = np.where(zero_ok & (R == 0), ref.astype(np.float64), R)
        _within(name, Rc[keep], ref[keep], rb[keep])
        _check_unchanged(name, [t1, tG], [X1, G])
        if op == "mul" and X2 is not None:
            H = _np(impl.kernel_matrix_hadamard(t1, t2, tG, variance=1.3, lengthscales=ls, family=family, **_akw(alpha)))
            _within(f"kernel_matrix_hadamard {family} {who}", H, ref, rb)


def test_white_and_constant_are_exact(gp):
    """White: variance I (+ diag_add I) for X2 None, exact zeros for ANY X2 given -- a clone of X included; "add" with X2 given
    leaves G bit-identical (in place and into a second buffer), "mul" gives exact zeros.  Constant: variance everywhere and
    variance + diag_add on the diagonal."""
    rng = np.random.default_rng(3)
    X, G = rng.normal(size=(130, 3)), rng.normal(size=(130, 130))
    for who, impl, dev in _impls(gp):
        tX, kw = _on(X, "c", dev), dict(variance=1.7, lengthscales=1.0)
        K = _np(impl.kernel_matrix(tX, None, family="White", diag_add=0.25, **kw))
        assert np.array_equal(K, (1.7 + 0.25) * np.eye(130)), who
        assert not _np(impl.kernel_matrix(tX, tX.clone(), family="White", **kw)).any(), who
        assert not _np(impl.kernel_matrix(tX, tX, family="White", **kw)).any(), who          # the same tensor as X2: still "X2 given"
        tG = _on(G, "c", dev)
        assert np.array_equal(_np(impl.kernel_matrix_combine(tX, tX.clone(), tG, op="add", family="White", **kw)), G), who
        impl.kernel_matrix_combine(tX, tX.clone(), tG, op="add", family="White", out=tG, **kw)
        assert np.array_equal(_np(tG), G), who
        assert not _np(impl.kernel_matrix_combine(tX, tX.clone(), tG, op="mul", family="White", **kw)).any(), who
        assert not _np(impl.kernel_matrix_hadamard(tX, tX.clone(), tG, family="White", **kw)).any(), who
        S = _np(impl.kernel_matrix_combine(tX, None, tG, op="add", family="White", diag_add=0.5, **kw))
        off = ~np.eye(130, dtype=bool)                                # symmetric "add": G untouched off the diagonal, + variance + diag_add on it
        assert np.array_equal(S[off], G[off]) and np.allclose(np.diag(S), np.diag(G) + 2.2, rtol=0, atol=4 * U * (np.abs(G).max() + 2.2)), who
        C = _np(impl.kernel_matrix(tX, None, family="Constant", diag_add=0.25, **kw))
        assert np.array_equal(C, np.full((130, 130), 1.7) + 0.25 * np.eye(130)), who
        assert np.array_equal(_np(impl.kernel_matrix(tX, _on(X[:70], "c", dev), family="Constant", **kw)), np.full((130, 70), 1.7)), who


def test_nan_row_reaches_the_distance_families_only(gp):
    """A NaN in one row of X makes exactly that row and column of an Exponential / RationalQuadratic matrix NaN (the clamp does not
    swallow it) and leaves White and Constant finite: they are filled without reading X."""
    X = np.random.default_rng(4).normal(size=(70, 3))
    X[5, 1] = np.nan
    expect = np.zeros((70, 70), dtype=bool)
    expect[5, :] = expect[:, 5] = True
    for who, impl, dev in _impls(gp):
        tX = _on(X, "c", dev)
        for family, alpha in FAMS:
            K = _np(impl.kernel_matrix(tX, None, variance=1.2, lengthscales=0.9, family=family, **_akw(alpha)))
            if family in STATIC:
                assert np.isfinite(K).all(), (who, family)
            else:
                assert np.array_equal(np.isnan(K), expect), (who, family)
                D = _np(impl.kernel_matrix_combine(tX, _on(X[:9], "c", dev), _on(np.ones((70, 9)), "c", dev), op="dr2", variance=1.2,
                                                   lengthscales=0.9, family=family, **_akw(alpha)))
                assert np.array_equal(np.isnan(D), expect[:, :9]), (who, family)


def test_refusals(gp):
    """Outside the contract, on the device (GpkError / ValueError) and in the emulation (AssertionError): "dalpha" for a family
    without alpha; alpha missing, <= 0 or NaN; alpha for another family; a RationalQuadratic member in the per-latent shard."""
    rng = np.random.default_rng(5)
    X, G = rng.normal(size=(20, 2)), rng.normal(size=(20, 20))
    for who, impl, dev in _impls(gp):
        tX, tG, kw = _on(X, "c", dev), _on(G, "c", dev), dict(variance=1.0, lengthscales=1.0)
        for family in ("SquaredExponential", "Exponential", "White", "Constant"):
            with pytest.raises(_refused()):
                impl.kernel_matrix_combine(tX, None, tG, op="dalpha", family=family, **kw)
        for alpha in (None, 0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(_refused()):
                impl.kernel_matrix(tX, None, family="RationalQuadratic", **kw, **_akw(alpha))
            with pytest.raises(_refused()):
                impl.kernel_matrix_combine(tX, tX.clone(), tG, op="mul", family="RationalQuadratic", **kw, **_akw(alpha))
        with pytest.raises(_refused()):
            impl.kernel_matrix(tX, None, family="Matern32", alpha=1.0, **kw)
        with pytest.raises(_refused()):
            impl.gpr_lml(tX, _on(G[:, :1], "c", dev), noise_variance=0.1, family="Exponential", alpha=1.0, **kw)
        Z, q_mu = _on(X[:8], "c", dev), _on(rng.normal(size=(8, 2)), "c", dev)
        q_sqrt = _on(np.stack([np.eye(8)] * 2), "c", dev)
        with pytest.raises(_refused()):
            impl.svgp_elbo_shard_sep(Z, tX, _on(G[:, :2], "c", dev), q_mu, q_sqrt, variances=[1.0, 1.0], lengthscales=[1.0, 1.0],
                                     families=["Exponential", "RationalQuadratic"], noise_variance=0.1, jitter=1e-6)


def test_zero_ok_sets_are_what_the_cases_plant():
    """CPU, the longdouble reference alone: the entries a comparison may leave to the clamp (`zero_ok`) are none for "normal" and
    "far" data and, for "dup" data, at most the near-duplicate pairs the case plants (the diagonal of a symmetric form is exact
    zero by contract and never in the set)."""
    for n1, n2, d, ard, data, *_ in KM_CASES:
        if n1 == 0:
            continue
        X1, X2, _ = _data(n1 + 3 * d, n1, n2, d, data)
        _check_zero_ok(X1, X2, data, _ls(d, ard), 1.7)
    for _, n1, n2, d, data, _ in KC_CASES:
        X1, X2, _ = _data(17 + n1 + d, n1, n2, d, data)
        _check_zero_ok(X1, X2, data, _ls(d, False, 0.8), 1.3)


def _check_zero_ok(X1, X2, data, ls, variance):
    for family, alpha in FAMS:
        for op in ("k", "dr2") + (("dalpha",) if family == "RationalQuadratic" else ()):
            z = _kref_new(family, X1, X2, variance, ls, alpha, op)[2]
            if data != "dup" or not (family == "Exponential" and op == "dr2"):
                assert not z.any(), (family, op, data, X1.shape)
                continue
            i, j = np.nonzero(z)
            if X2 is None:   # rows (2m, 2m + 1) are the planted near duplicates
                assert np.all((i // 2 == j // 2) & (i != j)), (family, op)
            else:            # pair (i, i), and the exactly coincident (0, 2)
                assert np.all((i == j) | ((i == 0) & (j == 2))), (family, op)
            assert z.any()   # (the case does reach the clamp)


# ------------------------------------------------------------------------------------------------ 2. fused paths and gradients
def _torch_kernel(family, variance, ls=None, alpha=None, cols=None):
    """torch restatement of one kernel (GPflow 2.9.2 stationaries.py / statics.py): kfun(A, B).  White gives variance * I only when
    called with the same tensor OBJECT twice (X2 is None in the reference), zeros otherwise."""
    def kfun(A, B):
        if family == "White":
            return variance * torch.eye(A.shape[0], dtype=torch.float64) if A is B else \
                variance * torch.zeros((A.shape[0], B.shape[0]), dtype=torch.float64)
        if family == "Constant":
            return variance * torch.ones((A.shape[0], B.shape[0]), dtype=torch.float64)
        same = A is B
        if cols is not None:
            A = A[:, cols]
            B = A if same else B[:, cols]
        if family in ("SquaredExponential", "Matern12", "Matern32", "Matern52"):
            return orcg._rbf(A, B, variance, ls, family)
        r2 = orcg._sqdist(A / ls, B / ls)
        if family == "Exponential":
            return variance * torch.exp(-0.5 * torch.sqrt(torch.clamp(r2, min=1e-36)))
        return variance * (1.0 + 0.5 * r2 / alpha) ** (-alpha)
    return kfun


def _leaf(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64, requires_grad=True)


def _t(x):
    return torch.tensor(np.asarray(x, dtype=np.float64), dtype=torch.float64)


VALUE_TOL = {"RationalQuadratic": 1e-9, "Exponential": 1e-7}     # (the Matern32 / 52 and the Matern12 figures of test_gpu_gradients.py)
GRAD_TOL = {"RationalQuadratic": 1e-8, "Exponential": 2e-6}
# (Exponential: d exp(-r / 2) / dr2 = -exp(-r / 2) / (4 r) is unbounded at r -> 0, as for Matern12: the oracle differentiates the
#  expansion formula, whose diagonal r2_ii is rounding noise, amplified by 1 / r; the product writes that factor as exact zeros.)
LEAVES = [("Exponential", None), ("RationalQuadratic", 0.7)]


def _close(name, got, ref, tol):
    got = np.asarray(got.cpu().numpy() if hasattr(got, "cpu") else got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.abs(got.reshape(ref.shape) - ref).max() <= tol * max(1.0, np.abs(ref).max()), \
        (name, np.abs(got.reshape(ref.shape) - ref).max(), np.abs(ref).max())


def _svgp_problem(seed=52):
    M, B, D, P = 200, 520, 4, 2
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(B, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(B, P))
    Z = rng.normal(size=(M, D))
    q_mu = 0.3 * rng.normal(size=(M, P))
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
    return X, Y, Z, q_mu, q_sqrt, np.sqrt(D) * (0.8 + 0.05 * np.arange(D))


@pytest.mark.parametrize("whiten", [True, False])
@pytest.mark.parametrize("fam", LEAVES, ids=[f for f, _ in LEAVES])
def test_single_leaf_svgp_elbo_and_grad_vs_autograd_oracle(gp, fam, whiten):
    """gradients.svgp_elbo_and_grad (whitened) / _unwhitened with family= (and alpha=), ARD lengthscales, and the fused forward
    ops.svgp_elbo_shard of the same family, against autograd over the restated kernel."""
    family, alpha = fam
    gradients, ops = gp.gradients, gp.ops
    X, Y, Z, q_mu, q_sqrt, ls = _svgp_problem()
    B = X.shape[0]
    t = ops.to_device
    fn = gradients.svgp_elbo_and_grad if whiten else gradients.svgp_elbo_and_grad_unwhitened
    F, g, info = fn(t(Z), t(X), t(Y), t(q_mu), t(q_sqrt), jitter=1e-6, scale=1000.0 / B, mean_const=0.1, family=family, variance=1.3,
                    lengthscales=ls, noise_variance=0.2, **_akw(alpha))
    ops.check_info(info)
    lv = {"variance": _leaf(1.3), "lengthscales": _leaf(ls), "noise_variance": _leaf(0.2), "Z": _leaf(Z), "q_mu": _leaf(q_mu),
          "q_sqrt": _leaf(q_sqrt), "mean_const": _leaf(0.1)}
    if alpha is not None:
        lv["alpha"] = _leaf(alpha)
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], lv["q_sqrt"], None, None, lv["noise_variance"], num_data=1000,
                              mean=lv["mean_const"], whiten=whiten,
                              kfun=_torch_kernel(family, lv["variance"], lv["lengthscales"], lv.get("alpha")), kdiag=lv["variance"])
    Fo.backward()
    v = float(Fo.detach())
    assert abs(float(F.cpu()[0]) - v) <= VALUE_TOL[family] * abs(v)
    assert ("alpha" in g) == (alpha is not None)
    for name, leaf in lv.items():
        _close(f"{family} {name}", g[name], leaf.grad.numpy(), GRAD_TOL[family])
    out, info = ops.svgp_elbo_shard(t(Z), t(X), t(Y), t(q_mu), t(q_sqrt), variance=1.3, lengthscales=ls, noise_variance=0.2, jitter=1e-6,
                                    mean_const=0.1, family=family, whiten=whiten, **_akw(alpha))
    ops.check_info(info)
    fused = float(out.cpu()[0]) * 1000.0 / B - float(out.cpu()[1])
    assert abs(fused - v) <= VALUE_TOL[family] * abs(v)


@pytest.mark.parametrize("fam", LEAVES, ids=[f for f, _ in LEAVES])
def test_single_leaf_gpr_and_sgpr_gradients_vs_autograd_oracle(gp, fam):
    family, alpha = fam
    gradients, ops = gp.gradients, gp.ops
    rng = np.random.default_rng(53)
    N, M, D, P = 700, 130, 3, 2
    X = rng.normal(size=(N, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P))
    Z = rng.normal(size=(M, D))
    ls = np.sqrt(D) * (0.8 + 0.05 * np.arange(D))
    kw = dict(variance=1.4, lengthscales=ls, noise_variance=0.15, family=family, **_akw(alpha))
    t = ops.to_device

    def leaves():
        lv = {"variance": _leaf(1.4), "lengthscales": _leaf(ls), "noise_variance": _leaf(0.15), "mean_const": _leaf(0.2)}
        if alpha is not None:
            lv["alpha"] = _leaf(alpha)
        return lv, _torch_kernel(family, lv["variance"], lv["lengthscales"], lv.get("alpha"))
    F, g, info = gradients.gpr_lml_and_grad(t(X), t(Y), mean_const=0.2, **kw)
    ops.check_info(info)
    lv, kfun = leaves()
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise_variance"], lv["mean_const"], kfun=kfun)
    Fo.backward()
    v = float(Fo.detach())
    assert abs(float(F.cpu()[0]) - v) <= VALUE_TOL[family] * abs(v)
    for name, leaf in lv.items():
        _close(f"gpr {family} {name}", g[name], leaf.grad.numpy(), GRAD_TOL[family])
    out, info = ops.gpr_lml(t(X), t(Y), mean_const=0.2, **kw)
    ops.check_info(info)
    assert abs(float(out.cpu()[0]) - v) <= VALUE_TOL[family] * abs(v)
    F, g, info = gradients.sgpr_elbo_and_grad(t(Z), t(X), t(Y), jitter=1e-6, mean_const=0.2, **kw)
    ops.check_info(info)
    lv, kfun = leaves()
    lv["Z"] = _leaf(Z)
    Fo = orcg.sgpr_elbo_torch(_t(X), _t(Y), lv["Z"], None, None, lv["noise_variance"], jitter=1e-6, mean=lv["mean_const"], kfun=kfun,
                              kdiag=lv["variance"])
    Fo.backward()
    v = float(Fo.detach())
    assert abs(float(F.cpu()[0]) - v) <= VALUE_TOL[family] * abs(v)
    for name, leaf in lv.items():
        _close(f"sgpr {family} {name}", g[name], leaf.grad.numpy(), GRAD_TOL[family])


def _combination(K, which):
    """(kernel, [(Parameter, leaf name)], torch kfun / kdiag factory) of the two combinations of the issue"""
    if which == "se+white":
        se, wh = K.SquaredExponential(variance=1.2, lengthscales=[0.9, 1.1, 1.3]), K.White(variance=0.3)
        pars = {"se.variance": se.variance, "se.lengthscales": se.lengthscales, "white.variance": wh.variance}

        def torch_kernel(lv):
            k0 = _torch_kernel("SquaredExponential", lv["se.variance"], lv["se.lengthscales"])
            k1 = _torch_kernel("White", lv["white.variance"])
            return (lambda A, B: k0(A, B) + k1(A, B)), lv["se.variance"] + lv["white.variance"]
        return se + wh, pars, torch_kernel
    c, m32 = K.Constant(variance=0.8), K.Matern32(variance=1.1, lengthscales=[1.0, 1.4, 0.7])
    rq = K.RationalQuadratic(variance=0.6, lengthscales=0.9, alpha=1.7, active_dims=[0, 2])
    pars = {"const.variance": c.variance, "m32.variance": m32.variance, "m32.lengthscales": m32.lengthscales,
            "rq.variance": rq.variance, "rq.lengthscales": rq.lengthscales, "rq.alpha": rq.alpha}

    def torch_kernel(lv):
        k0, k1 = _torch_kernel("Constant", lv["const.variance"]), _torch_kernel("Matern32", lv["m32.variance"], lv["m32.lengthscales"])
        k2 = _torch_kernel("RationalQuadratic", lv["rq.variance"], lv["rq.lengthscales"], lv["rq.alpha"], cols=[0, 2])
        return (lambda A, B: k0(A, B) * k1(A, B) + k2(A, B)), lv["const.variance"] * lv["m32.variance"] + lv["rq.variance"]
    return c * m32 + rq, pars, torch_kernel


def _check_model_grads(name, g, pars, lv, tol=1e-8):
    """every Parameter's dF/d(unconstrained) against the oracle's constrained gradient chained through the transform"""
    for key, par in pars.items():
        ref = lv[key].grad.numpy().reshape(np.shape(par.unconstrained_variable)) * par.transform.forward_grad(par.unconstrained_variable)
        assert par in g, (name, key)
        _close(f"{name} {key}", np.asarray(g[par]), ref, tol)


@pytest.mark.parametrize("which", ["se+white", "const*m32+rq"])
def test_combinations_with_static_and_rq_members_in_the_reverse_pass(gp, which):
    """SquaredExponential + White, and the nested Constant * Matern32 + RationalQuadratic(active_dims=[0, 2]) (the spec carries a
    tree), through the composed route: whitened SVGP.elbo_and_grad and GPR.log_marginal_likelihood_and_grad against autograd --
    every member's variance, its lengthscales where it has them, alpha, Z, the noise and the chain to the unconstrained variables."""
    gpflow = gp
    rng = np.random.default_rng(31)
    N, D, M, P = 260, 3, 70, 2
    X = rng.normal(size=(N, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P))
    Z = X[:M] + 0.05 * rng.normal(size=(M, D))
    q_mu = 0.2 * rng.normal(size=(M, P))
    q_sqrt = np.tril(0.1 * rng.normal(size=(P, M, M))) + 0.5 * np.eye(M)
    kern, pars, torch_kernel = _combination(gpflow.kernels, which)
    if which != "se+white":
        route = gpflow.models.reverse.CovarianceRoute(kern, D)
        assert route.spec.tree == ("add", [("mul", [0, 1]), 2]) and [m.keywords().get("alpha") for m in route.spec.members[:2]] == [None, None] \
            and route.spec.members[2].keywords()["alpha"] == pytest.approx(1.7)
        assert [len(m) for m in route.members] == [1, 2, 3]

    def leaves(extra):
        lv = {key: _leaf(par.numpy()) for key, par in pars.items()}
        lv.update({k: _leaf(v) for k, v in extra.items()})
        return lv
    # GPR
    m = gpflow.models.GPR((X, Y[:, :1]), kern, noise_variance=0.2)
    v, g = m.log_marginal_likelihood_and_grad()
    lv = leaves({"noise": 0.2})
    kfun, _ = torch_kernel(lv)
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y[:, :1]), None, None, lv["noise"], 0.0, kfun=kfun)
    Fo.backward()
    assert abs(v - float(Fo.detach())) <= 1e-9 * abs(float(Fo.detach()))
    assert abs(v - float(m.log_marginal_likelihood().cpu())) <= 1e-9 * abs(v)
    _check_model_grads("gpr", g, dict(pars, noise=m.likelihood.variance), lv)
    assert set(g) == set(pars.values()) | {m.likelihood.variance}
    # SVGP, whitened
    sv = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=P, num_data=5 * N)
    v, g = sv.elbo_and_grad((X, Y))
    lv = leaves({"noise": 0.2, "Z": Z, "q_mu": q_mu})
    kfun, kd = torch_kernel(lv)
    Fo = orcg.svgp_elbo_torch(_t(X), _t(Y), lv["Z"], lv["q_mu"], _t(q_sqrt), None, None, lv["noise"], num_data=5 * N, kfun=kfun, kdiag=kd)
    Fo.backward()
    assert abs(v - float(Fo.detach())) <= 1e-9 * abs(float(Fo.detach()))
    assert abs(v - float(sv.elbo((X, Y)).cpu())) <= 1e-9 * abs(v)
    _check_model_grads("svgp", g, dict(pars, noise=sv.likelihood.variance, Z=sv.inducing_variable.Z, q_mu=sv.q_mu), lv)


def test_white_in_a_sum_is_noise(gp):
    """GPR(RBF + White) is GPR(RBF) with the noise variance raised by White's variance: "X2 is None" end to end (K(X) carries the
    White diagonal, nothing else does)."""
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(7)
    X = rng.normal(size=(300, 3))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(300, 1))
    a = gpflow.models.GPR((X, Y), K.RBF(variance=1.3, lengthscales=[0.9, 1.2, 0.8]) + K.White(variance=0.35), noise_variance=0.2)
    b = gpflow.models.GPR((X, Y), K.RBF(variance=1.3, lengthscales=[0.9, 1.2, 0.8]), noise_variance=0.2 + 0.35)
    la, lb = float(a.log_marginal_likelihood().cpu()), float(b.log_marginal_likelihood().cpu())
    assert abs(la - lb) <= 1e-12 * abs(lb)
    va, _ = a.log_marginal_likelihood_and_grad()
    assert abs(va - lb) <= 1e-12 * abs(lb)
    Xn = rng.normal(size=(40, 3))
    (ma, sa), (mb, sb) = a.predict_f(Xn), b.predict_f(Xn)      # K(Xn, X) has no White term: the latent means agree
    np.testing.assert_allclose(_np(ma), _np(mb), rtol=0, atol=1e-10)
    np.testing.assert_allclose(_np(sa), _np(sb) + 0.35, rtol=0, atol=1e-10)   # (Knn = K_diag carries White's variance)


# ------------------------------------------------------------------------------------------------ 3. the public surface
def test_svgp_rational_quadratic_bernoulli(gp):
    """SVGP(RationalQuadratic, Bernoulli): elbo (the fused quadrature shard), predict_y and elbo_and_grad against central
    differences of its own elbo (the 1e-5 * max(1, |fd|) bar of test_gpu_gradients.py), alpha among the parameters."""
    gpflow = gp
    rng = np.random.default_rng(8)
    N, D, M = 200, 2, 25
    X = rng.normal(size=(N, D))
    Y = (np.sin(2 * X[:, :1]) + 0.3 * rng.normal(size=(N, 1)) > 0).astype(np.float64)
    k = gpflow.kernels.RationalQuadratic(variance=1.2, lengthscales=[0.8, 1.1], alpha=0.7)
    m = gpflow.models.SVGP(k, gpflow.likelihoods.Bernoulli(), X[:M].copy(), q_mu=0.2 * rng.normal(size=(M, 1)), num_data=N)
    assert isinstance(k.alpha, gpflow.Parameter) and k.alpha in m.trainable_parameters
    v, g = m.elbo_and_grad((X, Y))
    assert abs(v - float(m.elbo((X, Y)).cpu())) <= 1e-9 * abs(v) and np.isfinite(v)
    mu, var = m.predict_y(X[:30])
    assert tuple(mu.shape) == (30, 1) and bool(((_np(mu) > 0) & (_np(mu) < 1)).all()) and bool((_np(var) > 0).all())
    h = 1e-5
    for par, idx in [(k.alpha, ()), (k.variance, ()), (k.lengthscales, (1,)), (m.inducing_variable.Z, (3, 1)), (m.q_mu, (4, 0))]:
        u0 = np.array(par.unconstrained_variable, dtype=np.float64, copy=True)
        vals = []
        for dlt in (h, -h):
            u = u0.copy()
            u[idx] += dlt
            par.assign_unconstrained(u)
            vals.append(float(m.elbo((X, Y)).cpu()))
        par.assign_unconstrained(u0)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(float(np.asarray(g[par])[idx]) - fd) <= 1e-5 * max(1.0, abs(fd)), (par.name, idx, float(np.asarray(g[par])[idx]), fd)


def test_separate_independent_with_an_exponential_member(gp):
    """SeparateIndependent([Exponential, Matern32]).elbo on the fused per-latent shard (gpk_svgp_elbo_shard_sep) against the sum of
    the two single-latent models over the same inducing points, at rtol 1e-10."""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    rng = np.random.default_rng(9)
    N, D, M, P = 150, 3, 40, 2
    X = rng.normal(size=(N, D))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, P))
    Z = rng.normal(size=(M, D))
    q_mu = 0.2 * rng.normal(size=(M, P))
    q_sqrt = np.tril(0.1 * rng.normal(size=(P, M, M))) + 0.5 * np.eye(M)
    ks = [K.Exponential(variance=1.2, lengthscales=0.9), K.Matern32(variance=0.8, lengthscales=1.3)]
    m = gpflow.models.SVGP(K.SeparateIndependent(ks), gpflow.likelihoods.Gaussian(0.2), IV.SharedIndependentInducingVariables(
        IV.InducingPoints(Z.copy())), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=P, num_data=3 * N)
    assert m._fused_separate_config() is not None
    total = 0.0
    for p, kp in enumerate(ks):
        one = gpflow.models.SVGP(kp, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu[:, p:p + 1], q_sqrt=q_sqrt[p:p + 1],
                                 num_latent_gps=1, num_data=3 * N)
        total += float(one.elbo((X, Y[:, p:p + 1])).cpu())
    got = float(m.elbo((X, Y)).cpu())
    assert abs(got - total) <= 1e-10 * abs(total)


def test_scipy_moves_alpha(gp):
    """optimizers.Scipy lowers the loss of a GPR(RationalQuadratic + White) over five iterations and moves alpha."""
    gpflow = gp
    K = gpflow.kernels
    rng = np.random.default_rng(10)
    X = rng.normal(size=(150, 2))
    Y = np.sin(2 * X[:, :1]) + 0.5 * np.cos(X[:, 1:]) + 0.1 * rng.normal(size=(150, 1))
    rq = K.RationalQuadratic(lengthscales=[1.0, 1.0])
    m = gpflow.models.GPR((X, Y), rq + K.White(variance=0.5), noise_variance=0.5)
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=5))
    after = -float(m.log_marginal_likelihood().cpu())
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert abs(float(rq.alpha.numpy()) - 1.0) > 1e-3


def test_model_level_refusals(gp):
    """NotImplementedError, each naming its reason, before anything touches a device: a RationalQuadratic member on the fused
    per-latent shards (SeparateIndependent, LinearCoregionalization); the device-resident trainer with RationalQuadratic, White
    or Constant.  The trainer takes Exponential: its parameter set is (variance, lengthscales)."""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    rng = np.random.default_rng(11)
    X, Y, Z = rng.normal(size=(30, 2)), rng.normal(size=(30, 2)), rng.normal(size=(8, 2))
    iv = lambda: IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))  # noqa: E731
    lik = gpflow.likelihoods.Gaussian(0.2)
    sep = gpflow.models.SVGP(K.SeparateIndependent([K.RationalQuadratic(), K.Matern32()]), lik, iv(), num_latent_gps=2)
    with pytest.raises(NotImplementedError, match="alpha"):
        sep.elbo((X, Y))
    lcm = gpflow.models.SVGP(K.LinearCoregionalization([K.SquaredExponential(), K.RationalQuadratic()], np.ones((2, 2))), lik, iv(),
                             num_latent_gps=2)
    with pytest.raises(NotImplementedError, match="alpha"):
        lcm.elbo((X, Y))
    for k in (K.RationalQuadratic(), K.SquaredExponential() + K.White(), K.Constant() * K.Matern32(), K.Constant()):
        with pytest.raises(NotImplementedError, match="trainer"):
            gpflow.training.SVGPTrainer(gpflow.models.SVGP(k, gpflow.likelihoods.Gaussian(0.2), Z.copy()))
    sv = gpflow.models.SVGP(K.Exponential(lengthscales=[1.0, 1.0]), gpflow.likelihoods.Gaussian(0.2), Z.copy(), num_data=30)
    tr = gpflow.training.SVGPTrainer(sv, learning_rate=0.01)
    first = float(tr.step((X, Y[:, :1])).cpu()[0])
    tr.sync_to_model()
    assert abs(first - float(gpflow.models.SVGP(K.Exponential(lengthscales=[1.0, 1.0]), gpflow.likelihoods.Gaussian(0.2), Z.copy(),
                                                num_data=30).elbo((X, Y[:, :1])).cpu())) <= 1e-7 * abs(first)
