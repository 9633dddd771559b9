"""GPU tests of the Coregion kernel: the six primitives of gpflow_amd/csrc/coregion/coregion.hip (`ops.coregion_output_covariance`,
`_kernel_matrix`, `_kernel_matrix_combine`, `_kernel_diag`, `_onehot_rows`, `_adjoint_tail`), `kernels.Coregion` on every forward route,
the reverse pass of GPR, VGP and SVGP, and the kernel crossed with every other kind of leaf in Sum and Product trees.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_coregion_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture).  On the device every primitive case also runs the emulation beside it (`_impls`).

References.  The output covariance: np.longdouble, bound gamma_R sum_r |W_ar W_br| (an fma chain of R terms; gamma_k = k u / (1 - k u),
u = 2^-53), on the diagonal u |B_aa| more for "+ kappa", plus TINY.  The builder, the row diagonal and the one-hot rows are EXACT: held
bit for bit to B[l, l'] with the primitive's own B (held to its reference first); a combine op adds one rounding, u |result|.  The
adjoint: Bbar in longdouble by np.add.at; a cell is a sum of m = (rows with label a) x (columns with label b) entries of Kbar times
exact ones and zeros, in whatever order the two contractions take: gamma_(m-1) sum |terms|; the tail's chains of P products of
(Bbar_ab + Bbar_ba) W_br: gamma_(2P) sum |terms|.  And torch autograd on B[l][:, l'] at ADJ_TOL = 1e-9 in the measure of `_close`.
Models: torch under autograd (oracle/gp_oracle_grad.py through its `kfun=` / `kdiag=` hooks; VGP: the restated ELBO of
tests/test_gpu_vgp.py); values 1e-9 relative, gradients 1e-8 through `_check_model_grads` -- the project's figures.

Condition of the model problems (N = 40 rows, two data columns in [-1, 1] and the label column, P = 3 tasks, R = 2, M = 16, Z's labels
cycling 0, 1, 2: `_problem`).  Every kernel entry and every entry of the row diagonal was perturbed by a relative 4 * 2^-52 with random
signs in the oracle, on the CPU (`conditioning_figures`, asserted at <= 1e-10 by tests/test_coregion_emulated.py); the oracle's own
gradients moved by at most, in the measure of `_close`: CONDITIONING_FIGURES below.  A new shape or seed needs that check repeated.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_coregion_ops  # noqa: E402
import test_gpu_arccosine as AR  # noqa: E402
import test_gpu_dot_kernels as DK  # noqa: E402
import test_gpu_kernel_trees as TR  # noqa: E402
import test_gpu_vgp as VG  # noqa: E402
from test_gpu_contract import LD, U, _check_unchanged, _np, _on, _padding_untouched, _same_bits, _within  # noqa: E402
from test_gpu_kernel_families import _check_model_grads, _close, _leaf, _t  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

VALUE_TOL, GRAD_TOL = 1e-9, 1e-8
ADJ_TOL = 1e-9
TINY = LD(1e-300)
LAYOUTS = ["c", "ld", "off", "pad"]
# the largest move of the oracle's gradients under the perturbation of the module docstring, per problem (CPU, this file's seeds)
CONDITIONING_FIGURES = {"gpr coregion": 6.3e-13, "gpr se*coregion": 1.4e-15, "gpr se+coregion": 1.9e-14, "svgp se*coregion": 4.6e-13,
                        "svgp heteroskedastic": 4.3e-13, "vgp gaussian": 2.1e-14}


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    return str(gp.ops.device())


class _Emulation:
    coregion_output_covariance = staticmethod(fake_coregion_ops.coregion_output_covariance)
    coregion_kernel_matrix = staticmethod(fake_coregion_ops.coregion_kernel_matrix)
    coregion_kernel_matrix_combine = staticmethod(fake_coregion_ops.coregion_kernel_matrix_combine)
    coregion_kernel_diag = staticmethod(fake_coregion_ops.coregion_kernel_diag)
    coregion_onehot_rows = staticmethod(fake_coregion_ops.coregion_onehot_rows)
    coregion_adjoint_tail = staticmethod(fake_coregion_ops.coregion_adjoint_tail)


def _impls(gp):
    dev = _dev(gp)
    return [("ops", gp.ops, dev)] + ([("emulation", _Emulation, "cpu")] if dev != "cpu" else [])


def _gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ data shared by the primitive cases
_LEAVES, _LABELS, _BS = {}, {}, {}


def _wk(P, R):
    """(W [P, R], kappa [P]) of a case, made once"""
    if (P, R) not in _LEAVES:
        rng = np.random.default_rng(100 * P + R)
        _LEAVES[(P, R)] = (0.1 + 0.5 * rng.normal(size=(P, R)), rng.uniform(0.5, 1.5, size=P))
    return _LEAVES[(P, R)]


def _kw(P, R):
    W, kappa = _wk(P, R)
    return dict(W=W, kappa=kappa)


def _wide(n, P, seed, plant=True):
    """a [n, 3] array whose column 2 holds the labels: rng.integers(0, P) plus a fractional part in [0, 0.9]; one -0.5 (label 0) is
    planted where n > 1.  Returns (X, labels)"""
    key = (n, P, seed, plant)
    if key not in _LABELS:
        rng = np.random.default_rng(seed)
        X = rng.uniform(-1.0, 1.0, size=(n, 3))
        X[:, 2] = rng.integers(0, P, size=n) + rng.uniform(0.0, 0.9, size=n)
        if plant and n > 1:
            X[n // 2, 2] = -0.5
        _LABELS[key] = (X, np.trunc(X[:, 2]).astype(np.int64))
    return _LABELS[key]


def _col(X, dev, layout="c"):
    """the label column of a wider X on `dev`: an [n, 1] view with ldx = 3 (or wider, by `layout`)"""
    return _on(X, layout, dev)[:, 2:3]


def _B_of(impl, P, R, dev):
    """the primitive's own B on the host (held to its reference by test_coregion_output_covariance), once per implementation"""
    key = (impl is _Emulation, P, R)
    if key not in _BS:
        out = _on(np.zeros((P, P)), "c", dev)
        impl.coregion_output_covariance(**_kw(P, R), out=out)
        _BS[key] = _np(out).copy()
    return _BS[key]


# ------------------------------------------------------------------------------------------------ 1. the output covariance
@pytest.mark.parametrize("layout", ["c", "pad"])
@pytest.mark.parametrize("P,R", [(1, 1), (3, 2), (17, 5), (64, 64)])
def test_coregion_output_covariance(gp, P, R, layout):
    W, kappa = _wk(P, R)
    Wl = W.astype(LD)
    ref = Wl @ Wl.T + np.diag(kappa.astype(LD))
    bnd = _gamma(R) * (np.abs(Wl) @ np.abs(Wl).T) + U * np.abs(ref) * np.eye(P, dtype=LD) + TINY
    for who, impl, dev in _impls(gp):
        runs = []
        for rep in range(2):
            out, buf = _on(np.full((P, P), -555.0), layout, dev, base=True)
            got = impl.coregion_output_covariance(W, kappa, out=out)
            assert got is out and _padding_untouched(out, buf), f"{who}: padding written"
            runs.append(_np(out).copy())
        _within(f"coregion_output_covariance {who}", runs[0], ref, bnd)
        assert _same_bits(runs[0], runs[0].T), f"{who}: B is not exactly symmetric"
        assert _same_bits(runs[0], runs[1]), f"{who}: a second call differs"
        cached = impl.coregion_output_covariance(W, kappa, device_=dev)
        assert _same_bits(_np(cached), runs[0]), f"{who}: the cached B differs"


def test_the_cached_output_covariance_is_found_by_value(gp):
    """ops only: a second call with the same VALUES returns the same tensor (no upload, no launch); other values another"""
    if _dev(gp) == "cpu":      # (the emulation has no cache)
        return
    W, kappa = _wk(3, 2)
    a, b = gp.ops.coregion_output_covariance(W, kappa), gp.ops.coregion_output_covariance(W.copy(), kappa.copy())
    assert a is b and gp.ops.coregion_output_covariance(W + 1.0, kappa) is not a


# ------------------------------------------------------------------------------------------------ 2. the builder
BUILD_CASES = [(1, 1, 3, 2), (63, 65, 3, 2), (64, 64, 3, 2), (64, 64, 64, 64), (130, 70, 3, 2)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n1,n2,P,R", BUILD_CASES)
def test_coregion_kernel_matrix(gp, n1, n2, P, R, layout):
    """K[i, k] has the BITS of B[l_i, l'_k], in every layout of K, the label columns taken from a wider X; padding untouched; diag_add
    ignored with X2 given"""
    (X1, l1), (X2, l2) = _wide(n1, P, 10 * n1 + P), _wide(n2, P, 10 * n2 + P + 1)
    for who, impl, dev in _impls(gp):
        B = _B_of(impl, P, R, dev)
        t1, t2 = _col(X1, dev), _col(X2, dev, "pad")
        out, buf = _on(np.full((n1, n2), -555.0), layout, dev, base=True)
        got = impl.coregion_kernel_matrix(t1, t2, out=out, diag_add=9.0, **_kw(P, R))   # (diag_add: ignored with X2 given)
        name = f"coregion_kernel_matrix {who}"
        assert got is out and _padding_untouched(out, buf), f"{name}: padding written"
        assert _same_bits(_np(out), B[l1][:, l2]), f"{name}: not the bits of B[l, l']"
        _check_unchanged(name, [t1, t2], [X1[:, 2:3], X2[:, 2:3]])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", [1, 63, 64, 130])
def test_coregion_kernel_matrix_symmetric(gp, n, layout):
    """K(X, X) + diag_add I is EXACTLY symmetric without a mirror pass, a lower_only build has bit for bit the lower triangle of the full
    one and leaves the rest untouched, diag_add lands on the diagonal only"""
    P, R = 3, 2
    X, l = _wide(n, P, 10 * n + P)
    for who, impl, dev in _impls(gp):
        B = _B_of(impl, P, R, dev)
        tX = _col(X, dev)
        name = f"symmetric {who}"
        out, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
        impl.coregion_kernel_matrix(tX, None, out=out, diag_add=0.25, **_kw(P, R))
        Kf = _np(out).copy()
        assert _padding_untouched(out, buf), f"{name}: padding written"
        assert _same_bits(Kf, Kf.T), f"{name}: not exactly symmetric"
        plain = _np(impl.coregion_kernel_matrix(tX, None, **_kw(P, R)))
        assert _same_bits(plain, B[l][:, l]), f"{name}: not the bits of B[l, l]"
        want = plain.copy()
        want[np.diag_indices(n)] = np.diag(plain) + 0.25
        assert _same_bits(Kf, want), f"{name}: diag_add reached off the diagonal, or is not one addition on it"
        low, buf = _on(np.full((n, n), -555.0), layout, dev, base=True)
        impl.coregion_kernel_matrix(tX, None, out=low, diag_add=0.25, lower_only=True, **_kw(P, R))
        Kl = _np(low)
        assert _padding_untouched(low, buf) and _same_bits(np.tril(Kl), np.tril(Kf)), f"{name}: lower_only differs from the full build"
        up = np.triu(np.ones((n, n), dtype=bool), 1)
        assert np.all(Kl[up] == -555.0), f"{name}: lower_only wrote above the diagonal"
        _check_unchanged(name, [tX], [X[:, 2:3]])


@pytest.mark.parametrize("symmetric", [False, True], ids=["130x70", "symmetric63"])
@pytest.mark.parametrize("layout", ["c", "ld", "off"])
def test_coregion_kernel_matrix_combine(gp, layout, symmetric):
    """ops mul / add with `out` aliasing G (and not); diag_add lands on the diagonal of the COMBINED result; one rounding"""
    P, R = 3, 2
    n1, n2 = (63, 63) if symmetric else (130, 70)
    (X1, l1), (X2, l2) = _wide(n1, P, 10 * n1 + P), _wide(n2, P, 10 * n2 + P + 1)
    if symmetric:
        X2, l2 = X1, l1
    G = np.random.default_rng(6).normal(size=(n1, n2))
    eye = np.eye(n1, dtype=LD) if symmetric else 0
    for who, impl, dev in _impls(gp):
        k = _B_of(impl, P, R, dev)[l1][:, l2].astype(LD)
        t1, t2 = _col(X1, dev), (None if symmetric else _col(X2, dev, "ld"))
        Gl = G.astype(LD)
        want = {"mul": (Gl * k + 0.5 * eye, U * np.abs(Gl * k) + U * np.abs(Gl * k + 0.5) * eye),
                "add": (Gl + k + 0.5 * eye, U * np.abs(Gl + k) + U * np.abs(Gl + k + 0.5) * eye)}
        for op, (ref, bnd) in want.items():
            name = f"combine {who} {op}"
            tG, buf = _on(G, layout, dev, base=True)
            got = impl.coregion_kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.5, out=tG, **_kw(P, R))      # in place
            assert got is tG and _padding_untouched(tG, buf), f"{name}: padding written"
            _within(name, _np(tG), ref, bnd + TINY)
            tG2 = _on(G, "pad", dev)
            sep = impl.coregion_kernel_matrix_combine(t1, t2, tG2, op=op, diag_add=0.5, **_kw(P, R))             # a fresh output
            assert _same_bits(_np(sep), _np(tG)), f"{name}: aliasing changes the result"
            _check_unchanged(name, [tG2], [G])


# ------------------------------------------------------------------------------------------------ 3. the row diagonal, the one-hot rows
@pytest.mark.parametrize("n", [1, 63, 257])
def test_coregion_kernel_diag(gp, n):
    """ops 0 .. 2; bit for bit the diagonal of the symmetric build"""
    P, R = 3, 2
    X, l = _wide(n, P, 10 * n + P)
    g = np.random.default_rng(n).normal(size=n)
    for who, impl, dev in _impls(gp):
        tX = _col(X, dev)
        kd = _np(impl.coregion_kernel_diag(tX, **_kw(P, R)))
        assert _same_bits(kd, np.diag(_np(impl.coregion_kernel_matrix(tX, None, **_kw(P, R))))), f"{who}: not the diagonal of K(X, X)"
        assert _same_bits(kd, _B_of(impl, P, R, dev)[l, l])
        gl, kl = g.astype(LD), kd.astype(LD)
        for op, ref in (("mul", gl * kl), ("add", gl + kl)):
            tg = _on(g, "c", dev)
            got = impl.coregion_kernel_diag(tX, tg, op=op, out=tg, **_kw(P, R))                                   # out aliases g
            assert got is tg
            _within(f"coregion_kernel_diag {who} {op}", _np(tg), ref, U * np.abs(ref) + TINY)
            tg2 = _on(g, "c", dev)
            assert _same_bits(_np(impl.coregion_kernel_diag(tX, tg2, op=op, **_kw(P, R))), _np(tg)) and _same_bits(_np(tg2), g)


@pytest.mark.parametrize("P", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 70, 257])
def test_coregion_onehot_rows(gp, n, P):
    X, l = _wide(n, P, 10 * n + P)
    want = (l[None, :] == np.arange(P)[:, None]).astype(np.float64)
    for who, impl, dev in _impls(gp):
        E = impl.coregion_onehot_rows(_col(X, dev), P)
        assert tuple(E.shape) == (P, n) and E.is_contiguous() and _same_bits(_np(E), want), who


# ------------------------------------------------------------------------------------------------ 4. invalid labels
@pytest.mark.parametrize("planted", [float("nan"), float("inf"), -1.0, 3.0, 6.0], ids=["nan", "inf", "minus_one", "P", "P_plus_3"])
def test_an_invalid_label_reaches_its_own_row_and_column_only(gp, planted):
    """(63, 65), P = 3: an invalid label in row 40 of X1, then in row 64 of X2, makes exactly that row / column of K and of the combined
    results, that entry of the diagonal and that column of the one-hot rows NaN; everything else keeps the bits of the clean run"""
    P, R, n1, n2 = 3, 2, 63, 65
    (X1, _), (X2, _) = _wide(n1, P, 10 * n1 + P), _wide(n2, P, 10 * n2 + P + 1)
    B1, B2 = X1.copy(), X2.copy()
    B1[40, 2] = planted
    B2[64, 2] = planted
    G = np.random.default_rng(3).normal(size=(n1, n2))
    kw = _kw(P, R)
    for who, impl, dev in _impls(gp):
        c1, c2, t1, t2 = _col(X1, dev), _col(X2, dev), _col(B1, dev), _col(B2, dev)
        for a, b, rows, cols in ((t1, c2, [40], []), (c1, t2, [], [64]), (t1, t2, [40], [64])):
            bad = np.zeros((n1, n2), dtype=bool)
            bad[rows, :] = True
            bad[:, cols] = True
            name = f"invalid label {who} rows {rows} cols {cols}"
            clean, K = _np(impl.coregion_kernel_matrix(c1, c2, **kw)), _np(impl.coregion_kernel_matrix(a, b, **kw))
            assert np.array_equal(np.isnan(K), bad) and _same_bits(K[~bad], clean[~bad]), name
            for op in ("mul", "add"):
                cleanc = _np(impl.coregion_kernel_matrix_combine(c1, c2, _on(G, "c", dev), op=op, **kw))
                C = _np(impl.coregion_kernel_matrix_combine(a, b, _on(G, "c", dev), op=op, **kw))
                assert np.array_equal(np.isnan(C), bad) and _same_bits(C[~bad], cleanc[~bad]), f"{name} {op}"
        Ks, Kc = _np(impl.coregion_kernel_matrix(t1, None, **kw)), _np(impl.coregion_kernel_matrix(c1, None, **kw))
        r = np.arange(n1) == 40
        sym_bad = r[:, None] | r[None, :]
        assert np.array_equal(np.isnan(Ks), sym_bad) and _same_bits(Ks[~sym_bad], Kc[~sym_bad]), f"{who} symmetric"
        kd, kdc = _np(impl.coregion_kernel_diag(t1, **kw)), _np(impl.coregion_kernel_diag(c1, **kw))
        assert np.array_equal(np.isnan(kd), r) and _same_bits(kd[~r], kdc[~r]), f"{who} diagonal"
        E, Ec = _np(impl.coregion_onehot_rows(t1, P)), _np(impl.coregion_onehot_rows(c1, P))
        assert np.array_equal(np.isnan(E), np.broadcast_to(r, (P, n1))) and _same_bits(E[:, ~r], Ec[:, ~r]), f"{who} one-hot rows"
        _check_unchanged(f"invalid label {who}", [t1, t2], [B1[:, 2:3], B2[:, 2:3]])


# ------------------------------------------------------------------------------------------------ 5. the adjoint
ADJ_CASES = [(130, 70, False, 3, 2), (63, 63, True, 3, 2), (64, 64, False, 64, 64)]
ADJ_IDS = ["cross130x70", "symmetric63", "cross64x64P64"]


def _kbar(n1, n2, symmetric):
    Kb = np.random.default_rng(7 + n1).normal(size=(n1, n2))
    return Kb + Kb.T if symmetric else Kb


def _bbar_ref(Kb, l1, l2, P):
    """(Bbar in longdouble by np.add.at, its bound: a cell is a sum of m = cnt1[a] cnt2[b] terms in any order)"""
    Bb, Ab = np.zeros((P, P), dtype=LD), np.zeros((P, P), dtype=LD)
    np.add.at(Bb, (l1[:, None], l2[None, :]), Kb.astype(LD))
    np.add.at(Ab, (l1[:, None], l2[None, :]), np.abs(Kb).astype(LD))
    m = np.bincount(l1, minlength=P)[:, None] * np.bincount(l2, minlength=P)[None, :]
    return Bb, _gamma(np.maximum(m - 1, 0)) * Ab


@pytest.mark.parametrize("P,R", [(1, 1), (3, 2), (17, 5), (64, 64)])
def test_coregion_adjoint_tail(gp, P, R):
    """dW = (Bbar + Bbar^T) W and dkappa = diag(Bbar) over a random Bbar in a padded layout; a second call is bit-identical"""
    W, _ = _wk(P, R)
    Bb = np.random.default_rng(P + R).normal(size=(P, P))
    S, Wl = Bb.astype(LD) + Bb.astype(LD).T, W.astype(LD)
    for who, impl, dev in _impls(gp):
        tB = _on(Bb, "ld", dev)
        runs = [tuple(_np(x).copy() for x in impl.coregion_adjoint_tail(tB, W=W)) for _ in range(2)]
        assert all(_same_bits(a, b) for a, b in zip(*runs)), f"{who}: two runs differ"
        assert _same_bits(runs[0][0], np.diag(Bb)), f"{who}: dkappa is diag(Bbar)"
        _within(f"coregion_adjoint_tail {who} dW", runs[0][1], S @ Wl, _gamma(2 * P) * (np.abs(S) @ np.abs(Wl)) + TINY)
        _check_unchanged(who, [tB], [Bb])


def _coregion_torch(W, kappa, col=None):
    """torch restatement of gpflow/kernels/misc.py `Coregion`: (kfun(A, B), kdiag(X)); the label is the column cast to an integer"""
    def lab(X):
        return (X[:, -1] if col is None else X[:, col]).detach().to(torch.int64)

    def Bm():
        return W @ W.T + torch.diag(kappa)

    def kfun(A, B):
        return Bm()[lab(A)][:, lab(B)]

    def kdiag(X):
        return torch.diagonal(Bm())[lab(X)]
    return kfun, kdiag


@pytest.mark.parametrize("n1,n2,symmetric,P,R", ADJ_CASES, ids=ADJ_IDS)
def test_coregion_kernel_adjoint(gp, n1, n2, symmetric, P, R):
    """gradients.coregion_kernel_adjoint and CoregionMember.adjoint -- one-hot rows, the one pass over Kbar, the thin contraction, the
    tail -- against the longdouble Bbar with its derived bound and against autograd of sum(Kbar .* B[l][:, l']); no input gradient; a
    second call is bit-identical"""
    from gpflow_amd import gradients
    from gpflow_amd.leaf import CoregionLeaf
    dev = _dev(gp)
    (X1, l1), (X2, l2) = _wide(n1, P, 10 * n1 + P), _wide(n2, P, 10 * n2 + P + 1)
    if symmetric:
        X2, l2 = X1, l1
    W, kappa = _wk(P, R)
    Kb = _kbar(n1, n2, symmetric)
    leaf = CoregionLeaf(W, kappa)
    tA, tK = _on(X1, "c", dev), _on(Kb, "c", dev)
    tB = tA if symmetric else _on(X2, "c", dev)
    member = gradients.CoregionMember(leaf, np.array([2]))
    runs = []
    for rep in range(2):
        dk, dW, Ab = member.adjoint(tA, tB, tK, symmetric)
        assert Ab is None and tuple(dk.shape) == (P,) and tuple(dW.shape) == (P * R,)
        runs.append((_np(dk).copy(), _np(dW).copy()))
    assert _same_bits(runs[0][0], runs[1][0]) and _same_bits(runs[0][1], runs[1][1]), "a second call differs"
    Bb, dB = _bbar_ref(Kb, l1, l2, P)
    Wl = W.astype(LD)
    S, dS = Bb + Bb.T, dB + dB.T
    _within("adjoint d/dkappa", runs[0][0], np.diag(Bb), np.diag(dB) + TINY)
    _within("adjoint d/dW", runs[0][1].reshape(P, R), S @ Wl, dS @ np.abs(Wl) + _gamma(2 * P) * ((np.abs(S) + dS) @ np.abs(Wl)) + TINY)
    lv = {"W": _leaf(W), "kappa": _leaf(kappa)}
    kfun, _ = _coregion_torch(lv["W"], lv["kappa"], 2)
    (_t(Kb) * kfun(_t(X1), _t(X2))).sum().backward()
    _close("adjoint d/dkappa against autograd", runs[0][0], lv["kappa"].grad.numpy(), ADJ_TOL)
    _close("adjoint d/dW against autograd", runs[0][1], lv["W"].grad.numpy().reshape(-1), ADJ_TOL)
    _check_unchanged("adjoint", [tA, tK], [X1, Kb])
    # the row diagonal's adjoint
    bar = np.random.default_rng(n1).normal(size=n1)
    dk, dW = member.diag_adjoint(tA, _on(bar, "c", dev))
    lv = {"W": _leaf(W), "kappa": _leaf(kappa)}
    (_t(bar) * _coregion_torch(lv["W"], lv["kappa"], 2)[1](_t(X1))).sum().backward()
    _close("diag_adjoint d/dkappa", dk, lv["kappa"].grad.numpy(), ADJ_TOL)
    _close("diag_adjoint d/dW", dW, lv["W"].grad.numpy().reshape(-1), ADJ_TOL)


# ------------------------------------------------------------------------------------------------ 6. refusals at the primitives
def test_primitive_refusals_leave_the_output_unchanged(gp):
    """what the library (GPK_E_ARG), the wrappers (ValueError) or the emulation (AssertionError) refuse, each replayed with an output
    that must keep its bits"""
    n = 40
    X, _ = _wide(n, 3, 1)
    ok = _kw(3, 2)
    rng = np.random.default_rng(0)
    bads = [dict(W=rng.normal(size=(65, 2)), kappa=np.ones(65)), dict(W=rng.normal(size=(3, 65)), kappa=np.ones(3)),
            dict(W=rng.normal(size=(3, 2)), kappa=np.ones(4)), dict(W=rng.normal(size=(3,)), kappa=np.ones(3)),
            dict(W=np.zeros((0, 2)), kappa=np.ones(0)), dict(W=np.zeros((3, 0)), kappa=np.ones(3))]
    for who, impl, dev in _impls(gp):
        tX, tW = _col(X, dev), _on(X, "c", dev)
        out, g = _on(np.full((n, n), -555.0), "c", dev), _on(np.full(n, -555.0), "c", dev)
        small = _on(np.full((3, 3), -555.0), "c", dev)
        for kw in bads:
            for call in (lambda: impl.coregion_kernel_matrix(tX, None, out=out, **kw),
                         lambda: impl.coregion_kernel_matrix_combine(tX, None, out, op="mul", out=out, **kw),
                         lambda: impl.coregion_kernel_diag(tX, g, op="mul", out=g, **kw),
                         lambda: impl.coregion_output_covariance(kw["W"], kw["kappa"], out=small)):
                with pytest.raises(_refused()):
                    call()
        for call in (lambda: impl.coregion_kernel_matrix_combine(tX, None, out, op="ds", out=out, **ok),
                     lambda: impl.coregion_kernel_diag(tX, g, op="ds", out=g, **ok),
                     lambda: impl.coregion_kernel_diag(tX, g, op="k", out=g, **ok),
                     lambda: impl.coregion_kernel_matrix(tW, None, out=out, **ok),                   # more than one column
                     lambda: impl.coregion_kernel_diag(tW, **ok),
                     lambda: impl.coregion_onehot_rows(tX, 65),
                     lambda: impl.coregion_onehot_rows(tX, 0),
                     lambda: impl.coregion_adjoint_tail(out, W=ok["W"])):
            with pytest.raises(_refused()):
                call()
        assert np.all(_np(out) == -555.0) and np.all(_np(g) == -555.0) and np.all(_np(small) == -555.0), f"{who}: a refused call wrote"
        assert tuple(impl.coregion_kernel_matrix(tX[:0], tX, **ok).shape) == (0, n)


# ------------------------------------------------------------------------------------------------ 7. the class, forward
def _coregion_np(X, X2, W, kappa, col):
    B = W @ W.T + np.diag(kappa)
    l1 = np.trunc(X[..., col]).astype(int)
    l2 = l1 if X2 is None else np.trunc(X2[..., col]).astype(int)
    return B[l1][:, l2]


def _se_np(X, X2, v, ls, cols):
    A, B = X[:, cols] / ls, (X if X2 is None else X2)[:, cols] / ls
    return v * np.exp(-0.5 * ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))


def test_kernel_class_forward(gp):
    """K, K_into, K_diag, active_dims, batch dimensions, the output covariance, the trees of the coregionalisation recipe, the
    covariance dispatchers, the predicates and the ValueErrors"""
    gpflow = gp
    K = gpflow.kernels
    from gpflow_amd.kernels.base import DeviceLeaf, is_arc_leaf, is_coregion_leaf, is_device_leaf, is_dot_leaf, reverse_leaf
    from gpflow_amd.models.reverse import has_row_diagonal
    W, kappa = _wk(3, 2)
    (X, l), (X2, l2) = _wide(40, 3, 12), _wide(30, 3, 13)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()   # noqa: E731
    k = K.Coregion(3, 2, active_dims=[2])
    assert np.array_equal(k.W.numpy(), 0.1 * np.ones((3, 2))) and np.array_equal(k.kappa.numpy(), np.ones(3))
    k.W.assign(W)
    k.kappa.assign(kappa)
    assert is_coregion_leaf(k) and not is_arc_leaf(k) and not is_dot_leaf(k) and not is_device_leaf(k) and not isinstance(k, DeviceLeaf)
    assert not is_coregion_leaf(K.Linear()) and not is_coregion_leaf(K.ArcCosine()) and not is_coregion_leaf(K.White())
    assert has_row_diagonal(k) and has_row_diagonal(K.SquaredExponential() * k) and has_row_diagonal(K.SharedIndependent(k, 2))
    assert reverse_leaf(k) is not None and reverse_leaf(k)[2] == (k.kappa, k.W)
    Bn = W @ W.T + np.diag(kappa)
    assert rel(_np(k.output_covariance()), Bn) < 1e-14 and rel(_np(k.output_variance()), np.diag(Bn)) < 1e-14
    assert rel(_np(k(X, X2)), _coregion_np(X, X2, W, kappa, 2)) < 1e-14
    Kxx = _np(k(X))
    assert rel(Kxx, _coregion_np(X, None, W, kappa, 2)) < 1e-14 and _same_bits(Kxx, Kxx.T)
    kd = _np(k(X, full_cov=False))
    assert _same_bits(kd, np.diag(Kxx)) and rel(kd, (W[l] ** 2).sum(1) + kappa[l]) < 1e-14
    Xs = k.slice(gpflow.ops.to_device(X), None)[0]
    assert tuple(Xs.shape) == (40, 1) and _same_bits(_np(k.K_into(Xs, None, None, diag_add=0.5)), Kxx + 0.5 * np.eye(40))
    assert tuple(k.K_diag(Xs.reshape(2, 20, 1)).shape) == (2, 20)
    Kb = _np(k.K(Xs.reshape(2, 20, 1), gpflow.ops.to_device(X2[:, 2:3])))
    assert Kb.shape == (2, 20, 30) and _same_bits(Kb.reshape(40, 30), _np(k(X, X2)))
    Kbb = _np(k.K(Xs.reshape(2, 20, 1)))
    assert Kbb.shape == (2, 20, 20) and _same_bits(Kbb[1], Kxx[20:, 20:])
    # the recipe: SE(active_dims=[0, 1]) * Coregion(3, 2, active_dims=[2]), and the Sum
    se = K.SquaredExponential(variance=1.1, lengthscales=0.5, active_dims=[0, 1])
    sn = lambda A, B: _se_np(A, B, 1.1, 0.5, [0, 1])   # noqa: E731
    assert rel(_np((se * k)(X, X2)), sn(X, X2) * _coregion_np(X, X2, W, kappa, 2)) < 1e-13
    assert rel(_np((se + k)(X, X2)), sn(X, X2) + _coregion_np(X, X2, W, kappa, 2)) < 1e-13
    assert rel(_np((se * k)(X)), sn(X, None) * _coregion_np(X, None, W, kappa, 2)) < 1e-13
    assert rel(_np((se * k)(X, full_cov=False)), 1.1 * kd) < 1e-14 and rel(_np((se + k)(X, full_cov=False)), 1.1 + kd) < 1e-14
    iv = gpflow.inducing_variables.InducingPoints(X2.copy())
    assert rel(_np(gpflow.covariances.Kuf(iv, se * k, X)), sn(X2, X) * _coregion_np(X2, X, W, kappa, 2)) < 1e-13
    assert rel(_np(gpflow.covariances.Kuu(iv, k, jitter=1e-3)), _coregion_np(X2, None, W, kappa, 2) + 1e-3 * np.eye(30)) < 1e-13
    # ValueError before the device
    for bad in (dict(output_dim=0, rank=1), dict(output_dim=65, rank=1), dict(output_dim=3, rank=0), dict(output_dim=3, rank=65),
                dict(output_dim=2.5, rank=1), dict(output_dim=3, rank=2, active_dims=[0, 1]), dict(output_dim=3, rank=2, active_dims=[])):
        with pytest.raises(ValueError):
            K.Coregion(**bad)
    with pytest.raises(ValueError, match="one active column"):
        K.Coregion(3, 2)(X)                                                               # every column active: three of them
    assert K.Coregion(64, 64).leaf().n_shape == 4096 and isinstance(K.Coregion(1, 1) + se, K.Sum)


# ------------------------------------------------------------------------------------------------ 8. models against autograd
N, DD, NT, RK, M = 40, 2, 3, 2, 16    # rows, data columns, tasks, rank, inducing points
_PROBLEM = {}


def _problem():
    """X [40, 3]: two data columns in [-1, 1] and the label column; Y [40, 2]; Z [16, 3] with labels cycling 0, 1, 2; made once"""
    if not _PROBLEM:
        rng = np.random.default_rng(3016)
        X = np.concatenate([rng.uniform(-1.0, 1.0, size=(N, DD)), rng.integers(0, NT, size=(N, 1)).astype(np.float64)], axis=1)
        Y = np.sin(X[:, :DD].sum(1, keepdims=True)) + 0.3 * X[:, 2:3] + 0.1 * rng.normal(size=(N, 2))
        Z = np.concatenate([rng.uniform(-1.0, 1.0, size=(M, DD)), (np.arange(M) % NT)[:, None].astype(np.float64)], axis=1)
        q_mu = 0.3 * rng.normal(size=(M, 2))
        q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(2)])
        W = 0.1 + 0.5 * rng.normal(size=(NT, RK))
        kappa = rng.uniform(0.5, 1.5, size=NT)
        _PROBLEM.update(data=(X, Y, Z, q_mu, q_sqrt), W=W, kappa=kappa)
    return _PROBLEM


class CoregionKind(TR.Kind):
    """a row like those of test_gpu_kernel_trees.KINDS for the Coregion leaf: constructor, exact reference, torch.  `values` are in the
    order of the gradients: kappa (the slot the spec calls "variance"), then W"""

    def __init__(self, values, col=2):
        super().__init__("coregion", "Coregion", values, [col])

    class_name = "Coregion"
    is_dot = True      # (what the tree helpers ask: a diagonal that depends on the row)
    wide = True

    def make(self, K):
        W, kappa = np.asarray(self.values["W"], dtype=np.float64), np.asarray(self.values["kappa"], dtype=np.float64)
        k = K.Coregion(W.shape[0], W.shape[1], active_dims=list(self.cols))
        k.W.assign(W)
        k.kappa.assign(kappa)
        return k, {"kappa": k.kappa, "W": k.W}

    def ref(self, p, X1, X2):
        """B in longdouble with the output covariance's bound, gathered: the gather itself is exact"""
        Wl, kl = np.asarray(p["W"], dtype=LD), np.asarray(p["kappa"], dtype=LD)
        B = Wl @ Wl.T + np.diag(kl)
        bnd = _gamma(Wl.shape[1]) * (np.abs(Wl) @ np.abs(Wl).T) + U * np.abs(B) * np.eye(B.shape[0], dtype=LD) + TINY
        l1 = np.trunc(X1[:, self.cols[0]]).astype(int)
        l2 = l1 if X2 is None else np.trunc(X2[:, self.cols[0]]).astype(int)
        return B[l1][:, l2], bnd[l1][:, l2]

    def torch(self, lv):
        return _coregion_torch(lv["W"], lv["kappa"], self.cols[0])


def _model_kinds():
    p = _problem()
    return {"se": TR.Kind("stationary", "SquaredExponential", dict(variance=1.0, lengthscales=0.5), cols=[0, 1]),
            "co": CoregionKind(dict(kappa=p["kappa"], W=p["W"]))}


MODEL_TREES = {"coregion": "co", "se*coregion": ("mul", ["se", "co"]), "se+coregion": ("add", ["se", "co"])}


def _mk(K, which):
    """(kernel, {"tag.name": Parameter}, lv -> (kfun, kdiag))"""
    kinds, tree = _model_kinds(), MODEL_TREES[which]
    kern, pars = TR._make_tree(K, tree, kinds)
    return kern, pars, (lambda lv: TR._tree_torch(tree, kinds, lv))


HET_A, HET_B = np.array([[-0.1], [0.05], [0.02]]), np.array([0.6])


def _vgp_q():
    rng = np.random.default_rng(33)
    return 0.3 * rng.normal(size=(N, 2)), np.stack([np.tril(0.05 * rng.normal(size=(N, N))) + 0.6 * np.eye(N) for _ in range(2)])


def _oracle_grads(which, model, perturb, whiten=True, q_diag=False, het=False):
    """{name: gradient} of the oracle for one model problem, with the kernel perturbed or not (the conditioning check)"""
    p = _problem()
    X, Y, Z, q_mu, q_sqrt = p["data"]
    if q_diag:
        q_sqrt = np.ascontiguousarray(np.diagonal(q_sqrt, axis1=1, axis2=2).T)
    kinds, tree = _model_kinds(), MODEL_TREES[which]
    lv = {"co.kappa": _leaf(p["kappa"]), "co.W": _leaf(p["W"]), "noise": _leaf(0.15), "mean": _leaf(0.2), "Z": _leaf(Z), "q_mu": _leaf(q_mu),
          "q_sqrt": _leaf(q_sqrt)}
    if which != "coregion":
        lv.update({"se.variance": _leaf(1.0), "se.lengthscales": _leaf(0.5)})
    kfun, kdiag = TR._tree_torch(tree, kinds, lv)
    if perturb:
        kfun, kdiag = AR._perturbed(kfun, kdiag)
    if model == "gpr":
        F = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=kfun)
    elif model == "vgp":
        qm, qs = _vgp_q()
        lv["q_mu"], lv["q_sqrt"] = _leaf(qm), _leaf(qs)
        F = VG._torch_elbo("gaussian", (lv["noise"],), _t(X), _t(Y), lv["q_mu"], lv["q_sqrt"], kfun, lv["mean"])
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
    out = {}
    cases = [(f"gpr {w}", w, "gpr", [{}]) for w in MODEL_TREES] + \
        [("svgp se*coregion", "se*coregion", "svgp", [dict(whiten=w, q_diag=q) for w in (True, False) for q in (False, True)]),
         ("svgp heteroskedastic", "se*coregion", "svgp", [dict(whiten=w, het=True) for w in (True, False)]),
         ("vgp gaussian", "se*coregion", "vgp", [{}])]
    for name, which, model, kws in cases:
        worst = 0.0
        for kw in kws:
            a, b = _oracle_grads(which, model, False, **kw), _oracle_grads(which, model, True, **kw)
            worst = max([worst] + [float(np.abs(a[k] - b[k]).max() / max(1.0, np.abs(a[k]).max())) for k in a])
        out[name] = worst
    return out


@pytest.mark.parametrize("which", list(MODEL_TREES))
def test_gpr_vs_autograd_oracle(gp, which):
    """GPR.log_marginal_likelihood, _and_grad: kappa, W, the data kernel's Parameters, the noise and the mean constant"""
    gpflow = gp
    X, Y, _, _, _ = _problem()["data"]
    kern, pars, tk = _mk(gpflow.kernels, which)
    m = gpflow.models.GPR((X, Y), kern, noise_variance=0.15, mean_function=gpflow.mean_functions.Constant(0.2))
    v, g = m.log_marginal_likelihood_and_grad()
    lv = DK._leaves(pars, {"noise": 0.15, "mean": 0.2})
    Fo = orcg.gpr_lml_torch(_t(X), _t(Y), None, None, lv["noise"], lv["mean"], kfun=tk(lv)[0])
    Fo.backward()
    DK._agree(f"gpr {which}", v, float(Fo.detach()), float(m.log_marginal_likelihood().cpu()))
    allp = dict(pars, noise=m.likelihood.variance, mean=m.mean_function.c)
    _check_model_grads(f"gpr {which}", g, allp, lv, GRAD_TOL)
    assert set(g) == set(allp.values())


@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "q_diag"])
@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_vs_autograd_oracle(gp, whiten, q_diag):
    """SVGP.elbo (composed: the posterior) and elbo_and_grad in the four parametrisations, num_data = 1000 against B = 40: kappa, W, the
    data kernel's Parameters, Z, q_mu, q_sqrt, the noise and the mean constant; the label column of Z gets exactly 0"""
    kern, pars, tk = _mk(gp.kernels, "se*coregion")
    DK._svgp_check(gp, "svgp se*coregion", kern, pars, tk, _problem()["data"], whiten=whiten, q_diag=q_diag)


@pytest.mark.parametrize("whiten", [True, False], ids=["whitened", "unwhitened"])
def test_svgp_heteroskedastic_and_shared_vs_autograd_oracle(gp, whiten):
    """Gaussian(scale=Linear(A, b)) over all three columns -- per-task noise is its special case; and, forward, the kernel shared
    through SharedIndependent over SharedIndependentInducingVariables"""
    gpflow = gp
    kern, pars, tk = _mk(gpflow.kernels, "se*coregion")
    lik = gpflow.likelihoods.Gaussian(scale=gpflow.functions.Linear(A=HET_A.copy(), b=HET_B.copy()))

    def noise_of(lv, X):
        return torch.clamp(X @ lv["A"] + lv["b"], min=1e-3)[:, 0] ** 2
    DK._svgp_check(gpflow, "svgp heteroskedastic", kern, pars, tk, _problem()["data"], whiten=whiten, q_diag=False, lik=lik,
                   lik_pars={"A": lik.scale.A, "b": lik.scale.b}, noise_of=noise_of)
    # forward: the Product shared through SharedIndependent gives the ELBO of the plain model (a combination behind the wrapper has no
    # reverse pass, whatever its members)
    X, Y, Z, q_mu, q_sqrt = _problem()["data"]
    K, IV = gpflow.kernels, gpflow.inducing_variables
    kw = dict(q_mu=q_mu, q_sqrt=q_sqrt, whiten=whiten, num_latent_gps=2, num_data=1000)
    plain = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), **kw)
    shared = gpflow.models.SVGP(K.SharedIndependent(kern, 2), gpflow.likelihoods.Gaussian(0.2),
                                IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy())), **kw)
    a, b = float(plain.elbo((X, Y)).cpu()), float(shared.elbo((X, Y)).cpu())
    assert np.isfinite(a) and abs(a - b) <= 1e-12 * abs(a), (a, b)


def test_vgp_gaussian_vs_autograd(gp):
    """VGP with the Gaussian likelihood and a constant mean: value, forward ELBO, and every gradient against autograd of the restated ELBO"""
    gpflow = gp
    X, Y, _, _, _ = _problem()["data"]
    kern, pars, tk = _mk(gpflow.kernels, "se*coregion")
    m = gpflow.models.VGP((X, Y), kern, gpflow.likelihoods.Gaussian(0.15), mean_function=gpflow.mean_functions.Constant(0.2))
    q_mu, q_sqrt = _vgp_q()
    m.q_mu.assign(q_mu)
    m.q_sqrt.assign(q_sqrt)
    v, g = m.objective_and_grad()
    lv = DK._leaves(pars, {"q_mu": q_mu, "q_sqrt": q_sqrt, "mean": 0.2, "noise": 0.15})
    Fo = VG._torch_elbo("gaussian", (lv["noise"],), _t(X), _t(Y), lv["q_mu"], lv["q_sqrt"], tk(lv)[0], lv["mean"])
    Fo.backward()
    DK._agree("vgp", v, float(Fo.detach()), float(m.elbo()))
    allp = dict(pars, q_mu=m.q_mu, mean=m.mean_function.c, noise=m.likelihood.variance)
    _check_model_grads("vgp", g, allp, lv, GRAD_TOL)
    ref = m.q_sqrt.transform.inverse(np.tril(lv["q_sqrt"].grad.numpy()))
    _close("vgp q_sqrt", np.asarray(g[m.q_sqrt]), np.asarray(ref).reshape(np.shape(g[m.q_sqrt])), GRAD_TOL)
    assert set(g) == set(allp.values()) | {m.q_sqrt}


def test_the_label_column_of_Z_gets_exactly_zero(gp):
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = _problem()["data"]
    kern, _, _ = _mk(gpflow.kernels, "se*coregion")
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), Z.copy(), q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2, num_data=1000)
    _, g = m.elbo_and_grad((X, Y))
    gz = np.asarray(g[m.inducing_variable.Z]).reshape(M, 3)
    assert np.all(gz[:, 2] == 0.0) and np.abs(gz[:, :2]).max() > 1e-3


def test_scipy_trains_W_and_kappa(gp):
    gpflow = gp
    X, Y, _, _, _ = _problem()["data"]
    k = gpflow.kernels.SquaredExponential(lengthscales=0.5, active_dims=[0, 1]) * gpflow.kernels.Coregion(NT, RK, active_dims=[2])
    co = k.kernels[1]
    m = gpflow.models.GPR((X, Y[:, :1]), k, noise_variance=0.1)
    before = -float(m.log_marginal_likelihood().cpu())
    res = gpflow.optimizers.Scipy().minimize(m, options=dict(maxiter=5))
    after = -float(m.log_marginal_likelihood().cpu())
    assert after < before and abs(res.fun - after) <= 1e-8 * abs(after)
    assert np.abs(co.W.numpy() - 0.1).max() > 1e-4 and np.abs(co.kappa.numpy() - 1.0).max() > 1e-4


def test_svgp_elbo_with_bernoulli_forward_only(gp):
    """a quadrature likelihood, forward: the composed ELBO against the model's own pieces, and its reverse pass refused"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = _problem()["data"]
    kern, _, _ = _mk(gpflow.kernels, "se*coregion")
    Yb = (Y[:, :1] > 0).astype(np.float64)
    m = gpflow.models.SVGP(kern, gpflow.likelihoods.Bernoulli(), Z.copy(), q_mu=q_mu[:, :1], q_sqrt=q_sqrt[:1], num_data=200)
    assert m._fused_config() is None
    fm, fv = m.predict_f(X)
    want = float(m.likelihood.variational_expectations(gpflow.ops.to_device(X), fm, fv, gpflow.ops.to_device(Yb)).sum().cpu()) * 5.0 \
        - float(m.prior_kl().cpu())
    got = float(m.elbo((X, Yb)).cpu())
    assert np.isfinite(got) and abs(got - want) <= 1e-12 * abs(want)
    kd = _np(kern(X, full_cov=False))
    assert np.abs(kd - kd.mean()).max() > 0.05                  # fvar holds the ROW diagonal
    with pytest.raises(NotImplementedError, match="quadrature"):
        m.elbo_and_grad((X, Yb))


def test_predict_f_in_the_four_covariance_forms(gp):
    """SVGP.predict_f fused and through the cached posterior, full_cov x full_output_cov, whitened and not, against a NumPy restatement"""
    gpflow = gp
    X, Y, Z, q_mu, q_sqrt = _problem()["data"]
    kern, pars, tk = _mk(gpflow.kernels, "se*coregion")
    kfun, kdiag = tk({k: _t(p.numpy()) for k, p in pars.items()})
    Xn, _ = _wide(7, NT, 4, plant=False)
    tZ, tn = _t(Z), _t(Xn)
    Kmm = kfun(tZ, tZ).numpy() + 1e-6 * np.eye(M)
    Kmn, Knn = kfun(tZ, tn).numpy(), kfun(tn, tn).numpy()
    Kd = kdiag(tn).numpy()
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


# ------------------------------------------------------------------------------------------------ 9. trees: crossed with every other kind
OTHERS = AR.OTHERS + ["ArcCosine"]
_CROSS_DATA = {}


def _cross_kinds(other):
    co = CoregionKind(dict(kappa=_wk(3, 2)[1], W=_wk(3, 2)[0]))
    return {"co": co, "o": AR.ARCS[1] if other == "ArcCosine" else TR.KINDS[other]}


def _cross_data():
    """the shapes of test_gpu_kernel_trees (a partial tile each way); column 2 holds the labels (an integer in 0 .. 2 plus a fraction in
    [0, 0.9]) and is an ordinary input to the other kind of leaf; seed 2036 keeps the ArcCosine leaf's min(1 - |c|) above its margin
    (ArcKind.ref asserts it)"""
    if not _CROSS_DATA:
        rng = np.random.default_rng(2036)

        def inputs(n):
            X = rng.uniform(-1.0, 1.0, size=(n, TR.D))
            X[:, 2] = rng.integers(0, 3, size=n) + rng.uniform(0.0, 0.9, size=n)
            return X
        _CROSS_DATA.update(X1=inputs(TR.N1), X2=inputs(TR.N2), X=inputs(TR.NSYM), Kbar=rng.normal(size=(TR.N1, TR.N2)),
                           Ksym=rng.normal(size=(TR.NSYM, TR.NSYM)), kd_bar=rng.normal(size=TR.NSYM))
        _CROSS_DATA["Ksym"] = _CROSS_DATA["Ksym"] + _CROSS_DATA["Ksym"].T
    return _CROSS_DATA


CROSSES = [(other, first) for other in OTHERS for first in (True, False)]
CROSS_IDS = [f"{'Coregion-' + o if f else o + '-Coregion'}" for o, f in CROSSES]


@pytest.mark.parametrize("other,first", CROSSES, ids=CROSS_IDS)
def test_cross_forward(gp, other, first):
    """Sum and Product of Coregion and one leaf of another kind, as first child (built) and as second (folded in place), symmetric with
    diag_add and cross, through Combination.K_into and KernelSpec.build: within the bound composed from the leaves' own; a second call
    and the other route bitwise equal; padding untouched; K_diag and kdiag_rows against the built diagonal's references"""
    dev, dat = _dev(gp), _cross_data()
    kinds = _cross_kinds(other)
    ch = ["co", "o"] if first else ["o", "co"]
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
        # the diagonal: Coregion's is the diagonal of its reference; the other leaf's likewise, except ArcCosine's closed form
        cd, cdb = (np.diag(x) for x in kinds["co"].ref(TR._sub(vals, "co"), dat["X"], None))
        if other == "ArcCosine":
            ak, av = kinds["o"], TR._sub(vals, "o")
            od, odb = AR._diag_ref(ak.order, dat["X"], av["weight_variances"], float(av["bias_variance"]), float(av["variance"]))
        else:
            od, odb = (np.diag(x) for x in kinds["o"].ref(TR._sub(vals, "o"), dat["X"], None))
        dref = cd + od if op == "add" else cd * od
        dbnd = (cdb + odb if op == "add" else np.abs(cd) * odb + np.abs(od) * cdb + cdb * odb) + 2 * U * np.abs(dref)
        tX = _on(dat["X"], "ld", dev)
        _within(f"{name} K_diag", _np(kern.K_diag(tX)), dref, dbnd)
        _within(f"{name} kdiag_rows", _np(spec.kdiag_rows(tX)), dref, dbnd)


@pytest.mark.parametrize("other,first", CROSSES, ids=CROSS_IDS)
def test_cross_adjoint(gp, other, first):
    """KernelSpec.adjoint (symmetric and cross) and diag_adjoint of the same trees against autograd of sum(Kbar .* K(A, B)) and
    sum(kd_bar .* diag K): d/dkappa in the variance slot, d/dW as the shape gradient, the other member's gradients, and A_bar -- to
    which Coregion adds nothing"""
    dev, dat = _dev(gp), _cross_data()
    kinds = _cross_kinds(other)
    ch = ["co", "o"] if first else ["o", "co"]
    first_name = {"co": "kappa", "o": "variance"}
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
                _close(f"{name} {tag}.{first_name[tag]}", dv[i], np.reshape(TR._grad_of(lv, f"{tag}.{first_name[tag]}"), -1), GRAD_TOL)
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
            _close(f"{name} {tag}.{first_name[tag]}", dv[i], np.reshape(TR._grad_of(lv, f"{tag}.{first_name[tag]}"), -1), GRAD_TOL)
            sref = TR._shape_ref(lv, tag, kinds[tag])
            if sref.size:
                _close(f"{name} {tag} shape", dl[i], sref, GRAD_TOL)
        _check_unchanged(name, [tX, tg], [dat["X"], dat["kd_bar"]])


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(gp):
    """before anything touches a device: every model route that takes K_diag for one scalar -- each by the limit it breaks"""
    gpflow = gp
    K, IV = gpflow.kernels, gpflow.inducing_variables
    X, Y, Z, q_mu, q_sqrt = _problem()["data"]
    lik = gpflow.likelihoods.Gaussian(0.2)
    co = lambda: K.Coregion(NT, RK, active_dims=[2])   # noqa: E731
    for k in (co(), K.SquaredExponential(active_dims=[0, 1]) * co()):
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
    for kern in (K.SeparateIndependent([co(), K.SquaredExponential()]),
                 K.LinearCoregionalization([K.SquaredExponential(), co()], W=np.eye(2))):
        with pytest.raises(NotImplementedError, match="per-latent"):
            gpflow.models.SVGP(kern, lik, iv, q_mu=q_mu, q_sqrt=q_sqrt, num_latent_gps=2).elbo_and_grad((X, Y))
    from gpflow_amd import gradients
    from gpflow_amd.leaf import CoregionLeaf, Leaf
    W, kappa = _wk(3, 2)
    spec = gradients.KernelSpec([Leaf("SquaredExponential", 1.0, 0.5), CoregionLeaf(W, kappa)], "add", cols=[[0, 1], [2]])
    assert not spec.constant_diagonal and not spec.packable and spec.n_variance(1) == 3 and spec.n_shape(1) == 6
    assert spec.parameter_names(1) == ("kappa", "W")
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.kdiag()
    with pytest.raises(NotImplementedError, match="depends on the row"):
        spec.dkdiag()
    with pytest.raises(ValueError, match="period"):
        gradients.KernelSpec([CoregionLeaf(W, kappa)], periods=[1.0])
