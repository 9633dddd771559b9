"""Non-finite footprint tests: every `gpflow_amd.ops` primitive that `tests/fake_ops.py` emulates is held to NaN / Inf
PROPAGATION -- a non-finite value in a region the contract says is read comes out, exactly where the operation's definition
puts it, and nowhere else.  (`test_gpu_contract.py` uses NaN only as poison in regions that must NOT be read.)

Why it matters: every caller decides success from the factorisation status `info` alone and nothing in the package tests a
result with isfinite, so a primitive that turns NaN into a number yields a plausible, wrong ELBO with info == 0 -- where the
reference (GPflow on TensorFlow) returns NaN.

Each case runs the primitive twice on identical inputs, clean and with ONE planted value, and checks
  must-set:        every output entry the definition makes non-finite is non-finite, with the class (NaN / +Inf / -Inf) of an
                   fp64 NumPy evaluation of the same formula (np.isnan / np.isposinf / np.isneginf, never NaN bit patterns);
  must-stay-clean: every entry outside the footprint is BIT-IDENTICAL to the clean run.  Elementwise / row / column operations
                   have an exact footprint; factorisation and solves get the region of the mathematical data dependence,
                   widened to whole GPK_NB = 128 column blocks (a product with an explicit block inverse turns NaN * 0 into
                   NaN inside a block) -- entries in between are left unconstrained;
  inputs of non-underscore functions are bitwise unchanged.
+-Inf is planted where one infinite term fixes the class whatever the summation order (gemm_nt, row_dot, row_stats,
kernel_matrix and the exact operations); each such input is first checked on the CPU to give ONE class per output entry
(no sum with both signs of infinity, no read zero times the planted value).

Every test is parametrised over the implementation: the `fake_ops` half runs in the CPU tier and states the emulator's
contract, the `ops` half is marked gpu.  The guard at the end fails when a shared primitive has no case table here.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_ops  # noqa: E402
from test_gpu_contract import (GEMM_CASES, NOT_PRIMITIVES, _bits, _gemm_inputs, _np, _on, _same_bits, _spd, _svgp_inputs,  # noqa: E402
                               shared_primitives)

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
NB = 128
FAMILIES = ["SquaredExponential", "Matern12", "Matern32", "Matern52"]
NF_TABLES = {}     # primitive name -> its non-finite case table (filled next to each table)
PLANTS = {}        # primitive name -> planted runs executed in this process (printed by the guard: the PR's case count)


@pytest.fixture(params=[pytest.param("fake_ops"), pytest.param("ops", marks=pytest.mark.gpu)])
def impl(request):
    """(module, device, name): the emulator on the CPU, or the device library (needs the `gpu` fixture)."""
    if request.param == "ops":
        request.getfixturevalue("gpu")
        from gpflow_amd import ops
        return ops, "cuda", "ops"
    return fake_ops, "cpu", "fake_ops"


# ------------------------------------------------------------------------------------------------ helpers
def _cls(x):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    x = np.asarray(x, dtype=np.float64)
    return np.where(np.isnan(x), 1, np.where(np.isposinf(x), 2, np.where(np.isneginf(x), 3, 0)))


def _vcls(val):
    return int(_cls(val))


def _check(name, got, clean, want):
    """want per entry: 0 bitwise the clean run, 1 / 2 / 3 NaN / +Inf / -Inf, -1 unconstrained."""
    got, clean = np.asarray(got, dtype=np.float64), np.asarray(clean, dtype=np.float64)
    want = np.broadcast_to(np.asarray(want), got.shape)
    assert got.shape == clean.shape, (name, got.shape, clean.shape)
    c = _cls(got)
    miss = (want > 0) & (c != want)
    if miss.any():
        i = np.argwhere(miss)[0]
        raise AssertionError(f"{name}: must-set: {int(miss.sum())} entries lack the planted class; first at {tuple(i)}: "
                             f"got {got[tuple(i)]!r}, class wanted {int(want[tuple(i)])} (1 NaN, 2 +Inf, 3 -Inf)")
    leak = (want == 0) & (_bits(got) != _bits(clean))
    if leak.any():
        i = np.argwhere(leak)[0]
        raise AssertionError(f"{name}: must-stay-clean: {int(leak.sum())} entries outside the footprint differ from the clean "
                             f"run; first at {tuple(i)}: got {got[tuple(i)]!r}, clean {clean[tuple(i)]!r}")


def _plant(arrays, inp, idx, val):
    out = {k: (np.array(v, dtype=np.float64, copy=True) if isinstance(v, np.ndarray) else v) for k, v in arrays.items()}
    if idx is None:
        out[inp] = val
    else:
        out[inp][idx] = val
    return out


def _count(name, k=1):
    PLANTS[name] = PLANTS.get(name, 0) + k


def _footprint(name, who, run, arrays, inp, idx, val, fp, clean=None, ref=None):
    """One planted run of `run(arrays) -> {output name: array}` against the clean one.  fp: {output: [index, ...]}, the stated
    footprint (outputs not named stay bitwise clean).  ref(arrays) -> the same outputs by the plain fp64 NumPy formula: its
    non-finite set must BE the stated footprint, and it gives the class.  For +-Inf it must have no NaN on the footprint (one
    class per entry: no inf - inf, no 0 * inf) -- a CPU check of the INPUT, made before the result is looked at."""
    clean = run(arrays) if clean is None else clean
    planted = _plant(arrays, inp, idx, val)
    r = None
    if ref is not None:
        with np.errstate(all="ignore"):
            r = ref(planted)
    wants = {}
    for out, c in clean.items():
        want = np.zeros(np.shape(c), dtype=np.int64)
        for sl in fp.get(out, []):
            want[sl] = 1
        if r is not None:
            rr = np.asarray(r[out], dtype=np.float64)
            assert np.array_equal(~np.isfinite(rr), want == 1), f"{name}[{inp}{idx}={val}] {out}: the formula's footprint is not the stated one"
            if np.isinf(val):
                assert not np.isnan(rr).any(), f"{name}[{inp}{idx}={val}] {out}: this input has no single class per entry"
            want = np.where(want == 1, _cls(rr), 0)
        elif not np.isnan(val):
            want = np.where(want == 1, _vcls(val), 0)      # exact operations: the value itself arrives
        wants[out] = want
    got = run(planted)
    for out, c in clean.items():
        _check(f"{name} {who} [{inp}{idx} = {val}] -> {out}", got[out], c, wants[out])
    _count(name)
    return got


def _unchanged(name, pairs):
    for t, a in pairs:
        assert _same_bits(_np(t), a), f"{name}: an input was modified"


def _pick(cands, n):
    """the candidates that exist in a dimension of size n, `last` included"""
    return sorted({c for c in cands if 0 <= c < n} | {n - 1})


# ------------------------------------------------------------------------------------------------ GEMM
# the shapes of the contract table (every launch kind), minus the empty ones (nothing is read) and alpha == 0 (whether
# alpha = 0 skips the product is outside this contract) -- the latter stays in for the plant in C
GEMM_NF = [c for c in GEMM_CASES if min(c[0], c[1], c[2]) > 0]
NF_TABLES["gemm_nt"] = GEMM_NF
ROWS_AT = (0, 63, 64, 127, 128)      # wave / tile / leaf edges (+ the last row)
KS_AT = (0, 15, 16)                  # K-slab edges (+ K - 1)


def _gemm_run(mod, dev, case, arrs, **kw):
    m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
    lay = layout if batch == 0 else "c"
    tA, tB, tC = _on(arrs["A"], lay, dev), _on(arrs["B"], lay, dev), _on(arrs["C"], lay, dev)
    got = _np(mod.gemm_nt(tA, tB, alpha=alpha, beta=beta, C=tC, b_tri=b_tri, c_lower=c_lower, **kw))
    _unchanged("gemm_nt", [(tA, arrs["A"]), (tB, arrs["B"])])
    return {"C": got}


def _gemm_written(case):
    """[m, n] mask of the entries the call writes (c_lower: 128 x 128 tiles strictly above the diagonal are skipped)."""
    m, n, c_lower = case[0], case[1], case[6]
    m0, n0 = (np.arange(m) // NB * NB)[:, None], (np.arange(n) // NB * NB)[None, :]
    return ~(n0 > m0 + NB - 1) if c_lower else np.ones((m, n), dtype=bool)


@pytest.mark.parametrize("case", GEMM_NF, ids=[str(c) for c in GEMM_NF])
def test_gemm_nt_nonfinite(impl, case):
    """A[i, kk] reaches row i of C, B[j, kk] column j, C[i, j] (beta != 0) that entry; skipped c_lower tiles keep their
    sentinel even inside a NaN row; with a batch only the planted entry's part.  b_tri: the plant goes into the K range of
    B that holds real data (kk >= j upper, kk <= j lower), and A is not planted there: a NaN in A meets the structural
    zeros of B, and whether a declared zero is read depends on the tile kind -- NaN * 0 cannot be stated."""
    mod, dev, who = impl
    m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
    A, _, B, C0 = _gemm_inputs(case)
    arrs = {"A": A, "B": B, "C": C0}
    run = lambda a: _gemm_run(mod, dev, case, a)   # noqa: E731
    clean = run(arrs)
    written = _gemm_written(case)
    nb = abs(batch)
    z = nb - 1        # a batched operand is planted in its LAST entry

    def fp_row(i):    # -> index list selecting row i (of part z) where written
        cols = np.nonzero(written[i])[0]
        return [((z, i, cols) if batch else (i, cols))]

    def fp_col(j):
        rows = np.nonzero(written[:, j])[0]
        if batch > 0:
            return [(z, rows, j)]
        if batch < 0:     # broadcast B: every part
            return [(slice(None), rows, j)]
        return [(rows, j)]

    ref = None
    if alpha != 0.0:
        for i in _pick(ROWS_AT, m) if not b_tri else []:
            for kk in _pick(KS_AT, k):
                _footprint("gemm_nt", who, run, arrs, "A", (z, i, kk) if batch else (i, kk), NAN, {"C": fp_row(i)}, clean)
        for j in _pick(ROWS_AT, n):
            ks = _pick(KS_AT, k)
            if b_tri == 1:
                ks = [kk for kk in {j, min(j + 1, k - 1), k - 1} if j <= kk < k]
            elif b_tri == 2:
                ks = [kk for kk in {0, 15, 16, min(j, k - 1)} if kk <= j and kk < k]
            for kk in ks:
                _footprint("gemm_nt", who, run, arrs, "B", (z, j, kk) if batch > 0 else (j, kk), NAN, {"C": fp_col(j)}, clean)
        if not b_tri:
            # +-Inf: one infinite term per sum (a single planted entry, no zero among the data it multiplies: checked by ref)
            def ref(a):
                A3, B3 = (a["A"] if batch else a["A"][None]), (a["B"] if batch > 0 else a["B"][None])
                C3 = a["C"] if batch else a["C"][None]
                out = np.stack([alpha * (A3[min(q, A3.shape[0] - 1)] @ B3[min(q, B3.shape[0] - 1)].T)
                                + (beta * C3[q] if beta != 0 else 0.0) for q in range(max(nb, 1))])
                out = np.where(written[None], out, 0.0)
                return {"C": out if batch else out[0]}
            _footprint("gemm_nt", who, run, arrs, "A", (z, 0, 0) if batch else (0, 0), PINF, {"C": fp_row(0)}, clean, ref)
            _footprint("gemm_nt", who, run, arrs, "B", (z, n - 1, k - 1) if batch > 0 else (n - 1, k - 1), NINF,
                       {"C": fp_col(n - 1)}, clean, ref)
    if beta != 0.0:   # C[i, j] is read and reaches C[i, j] only (beta == 0: C is NaN throughout and never read -- every case above)
        for i, j in {(0, 0), (m - 1, n - 1), (min(64, m - 1), min(63, n - 1))}:
            if written[i, j]:
                _footprint("gemm_nt", who, run, arrs, "C", (z, i, j) if batch else (i, j), NAN,
                           {"C": [(z, i, j) if batch else (i, j)]}, clean)


# (parts Z, m, n, K per part): the batch entries are consecutive K chunks of one product
KSPLIT_NF = [(3, 70, 65, 32), (2, 130, 140, 48)]   # three chunks of two slabs, partial tiles; generic tiles over grid.y
# (a_tri, m, n, k): A upper (1) / lower (2) triangular, stored zeros
ATRI_NF = [(1, 200, 150, 200), (2, 200, 150, 200)]
NF_TABLES["gemm_nt"] = GEMM_NF + KSPLIT_NF + ATRI_NF


@pytest.mark.parametrize("case", KSPLIT_NF, ids=str)
def test_gemm_nt_k_split_nonfinite(impl, case):
    """k_split: a plant in chunk z of A (B) makes row i (column j) of PART z non-finite and no other part."""
    mod, dev, who = impl
    Z, m, n, kc = case
    rng = np.random.default_rng(Z + m + n)
    arrs = {"A": rng.normal(size=(Z, m, kc)), "B": rng.normal(size=(Z, n, kc))}

    def run(a):
        tA, tB = _on(a["A"], "c", dev), _on(a["B"], "c", dev)
        got = _np(mod.gemm_nt(tA, tB, k_split=True))
        _unchanged("gemm_nt k_split", [(tA, a["A"]), (tB, a["B"])])
        return {"C": got}
    clean = run(arrs)
    ref = lambda a: {"C": np.einsum("zik,zjk->zij", a["A"], a["B"])}   # noqa: E731
    for z in (0, Z - 1):
        for i, kk in ((0, 0), (m - 1, kc - 1), (min(64, m - 1), 16)):
            _footprint("gemm_nt", who, run, arrs, "A", (z, i, kk), NAN, {"C": [(z, i)]}, clean, ref)
        for j, kk in ((0, 15), (n - 1, 0), (min(63, n - 1), kc - 1)):
            _footprint("gemm_nt", who, run, arrs, "B", (z, j, kk), NAN, {"C": [(z, slice(None), j)]}, clean, ref)
    _footprint("gemm_nt", who, run, arrs, "A", (Z - 1, 1, 1), PINF, {"C": [(Z - 1, 1)]}, clean, ref)


@pytest.mark.parametrize("case", ATRI_NF, ids=str)
def test_gemm_nt_a_tri_nonfinite(impl, case):
    """a_tri: a plant inside the K range of A that holds real data (kk >= i upper, kk <= i lower) reaches row i.  B is not
    planted: its column kk meets the structural zeros of A (NaN * 0 cannot be stated, as for b_tri)."""
    mod, dev, who = impl
    a_tri, m, n, k = case
    rng = np.random.default_rng(a_tri + m)
    A = rng.normal(size=(m, k))
    arrs = {"A": np.triu(A) if a_tri == 1 else np.tril(A), "B": rng.normal(size=(n, k))}

    def run(a):
        tA, tB = _on(a["A"], "c", dev), _on(a["B"], "c", dev)
        got = _np(mod.gemm_nt(tA, tB, a_tri=a_tri))
        _unchanged("gemm_nt a_tri", [(tA, a["A"]), (tB, a["B"])])
        return {"C": got}
    clean = run(arrs)
    spots = ((0, 0), (63, 199), (128, 128), (199, 199)) if a_tri == 1 else ((0, 0), (63, 15), (128, 128), (199, 0))
    for i, kk in spots:
        _footprint("gemm_nt", who, run, arrs, "A", (i, kk), NAN, {"C": [(i,)]}, clean)


# ------------------------------------------------------------------------------------------------ kernel matrices
# (family, ARD, kind) -- kind: rect 130 x 70 (X2 given; full + ragged 64-tiles), sym 130 (mirror tiles, ragged edge),
# lower 130 (lower_only: tiles strictly above the diagonal are not written).  (The mirror tile's store through LDS is an
# A/B knob of the experimental build, off in the product library: it has no case here.)
KM_NF = [(f, ard, kind) for f in FAMILIES for ard in (False, True) for kind in ("rect", "sym", "lower")]
NF_TABLES["kernel_matrix"] = KM_NF
KM_D = 3


def _km_inputs(family, ard, kind):
    rng = np.random.default_rng(FAMILIES.index(family) * 8 + ard * 4 + len(kind))
    arrs = {"X1": rng.normal(size=(130, KM_D)), "ls": (0.7 + 0.1 * np.arange(KM_D)) if ard else np.array([0.9]), "variance": 1.7}
    if kind == "rect":
        arrs["X2"] = rng.normal(size=(70, KM_D))
    return arrs


def _lsarg(ls):
    return ls if ls.size > 1 else float(ls[0])


@pytest.mark.parametrize("case", KM_NF, ids=[str(c) for c in KM_NF])
def test_kernel_matrix_nonfinite(impl, case):
    """X1[i, dd] reaches row i (symmetric: row AND column i, the column through the mirror tile), X2[j, dd] column j; a NaN
    lengthscale or variance reaches everything written.  The three Matern families are the point: r = sqrt(max(r2, 1e-36))
    has to let a NaN r2 through.  An infinite coordinate gives r2 = +Inf or Inf - Inf entry by entry: the class of
    fake_ops._k on the same input (entries it leaves finite are not constrained)."""
    mod, dev, who = impl
    family, ard, kind = case
    arrs = _km_inputs(family, ard, kind)
    sym, lower = kind != "rect", kind == "lower"
    n1, n2 = 130, (130 if sym else 70)
    low = np.tril(np.ones((n1, n2), dtype=bool))

    def run(a):
        t1 = _on(a["X1"], "ld", dev)
        t2 = None if sym else _on(a["X2"], "ld", dev)
        out = _on(np.full((n1, n2), -555.0), "c", dev) if lower else None
        K = _np(mod.kernel_matrix(t1, t2, variance=a["variance"], lengthscales=_lsarg(a["ls"]), family=family,
                                  diag_add=0.3 if sym else 0.0, lower_only=lower, out=out))
        _unchanged("kernel_matrix", [(t1, a["X1"])] + ([] if sym else [(t2, a["X2"])]))
        return K
    clean = run(arrs)

    def one(inp, idx, val, want):
        got = run(_plant(arrs, inp, idx, val))
        if lower:   # only the lower triangle is defined; above it a skipped tile keeps its sentinel
            want = np.where(low, want, -1)
            if who == "ops":
                t = np.arange(n1) // 64
                skipped = t[None, :] > t[:, None]
                assert np.all(got[skipped] == -555.0), "kernel_matrix lower_only: a skipped tile was written"
        _check(f"kernel_matrix {who} {case} [{inp}{idx} = {val}]", got, clean, want)
        _count("kernel_matrix")

    for i in (0, 63, 64, 129):
        want = np.zeros((n1, n2), dtype=np.int64)
        want[i, :] = 1
        if sym:
            want[:, i] = 1
        one("X1", (i, i % KM_D), NAN, want)
    for j in (() if sym else (0, 63, 64, 69)):
        want = np.zeros((n1, n2), dtype=np.int64)
        want[:, j] = 1
        one("X2", (j, j % KM_D), NAN, want)
    one("ls", (KM_D - 1 if ard else 0,), NAN, np.ones((n1, n2), dtype=np.int64))
    one("variance", None, NAN, np.ones((n1, n2), dtype=np.int64))
    for i, val in ((64, PINF), (129, NINF)):
        p = _plant(arrs, "X1", (i, 1), val)
        with np.errstate(all="ignore"):
            r = fake_ops._k(p["X1"], p["X1"] if sym else p["X2"], 1.7, p["ls"], family) + (0.3 * np.eye(n1) if sym else 0.0)
        fpm = np.zeros((n1, n2), dtype=bool)
        fpm[i, :] = True
        if sym:
            fpm[:, i] = True
        assert np.all(np.isfinite(r[~fpm]))
        one("X1", (i, 1), val, np.where(fpm, np.where(np.isfinite(r), -1, _cls(r)), 0))


# (op, family, symmetric (X2 None))
KC_NF = [(op, f, sym) for op in ("mul", "add", "dr2") for f in FAMILIES for sym in (False, True)]
NF_TABLES["kernel_matrix_combine"] = KC_NF
NF_TABLES["kernel_matrix_hadamard"] = [c for c in KC_NF if c[0] == "mul" and not c[2]]


@pytest.mark.parametrize("case", KC_NF, ids=[str(c) for c in KC_NF])
def test_kernel_matrix_combine_nonfinite(impl, case):
    """The same footprints through G .* k, G + k and G .* (-2 dk/dr2) (70 x 66, or 70 symmetric: no mirror shortcut here) --
    except that op dr2 with X2 None keeps EXACT zeros on the diagonal whatever is planted (include/gpk.h) -- and G[i, j]
    reaches that one entry.  kernel_matrix_hadamard is op mul with X2 given: run on the same plants."""
    mod, dev, who = impl
    op, family, sym = case
    ard = bool((FAMILIES.index(family) + sym) % 2)
    rng = np.random.default_rng(FAMILIES.index(family) * 6 + len(op) + sym)
    n1, n2 = 70, (70 if sym else 66)
    arrs = {"X1": rng.normal(size=(n1, KM_D)), "G": rng.normal(size=(n1, n2)),
            "ls": (0.7 + 0.1 * np.arange(KM_D)) if ard else np.array([0.9]), "variance": 1.3}
    if not sym:
        arrs["X2"] = rng.normal(size=(n2, KM_D))
    names = ["combine"] + (["hadamard"] if op == "mul" and not sym else [])

    def run_on(m_, d_, a):
        t1, tG = _on(a["X1"], "c", d_), _on(a["G"], "ld", d_)
        t2 = None if sym else _on(a["X2"], "c", d_)
        kw = dict(variance=a["variance"], lengthscales=_lsarg(a["ls"]), family=family)
        res = {"combine": _np(m_.kernel_matrix_combine(t1, t2, tG, op=op, diag_add=0.2 if sym else 0.0, **kw))}
        if "hadamard" in names:
            res["hadamard"] = _np(m_.kernel_matrix_hadamard(t1, t2, tG, **kw))
        _unchanged("kernel_matrix_combine", [(t1, a["X1"]), (tG, a["G"])] + ([] if sym else [(t2, a["X2"])]))
        return res
    run = lambda a: run_on(mod, dev, a)   # noqa: E731
    clean = run(arrs)
    diag = np.eye(n1, n2, dtype=bool) & (sym and op == "dr2")

    def one(inp, idx, val, want):
        got = run(_plant(arrs, inp, idx, val))
        want = np.where(diag, 0, want)       # dr2, X2 None: the diagonal stays the exact zero of the clean run
        for nm in names:
            _check(f"kernel_matrix_{nm} {who} {case} [{inp}{idx} = {val}]", got[nm], clean[nm], want)
            _count("kernel_matrix_" + nm)
        if diag.any():
            assert np.all(np.diagonal(got["combine"]) == 0)

    for i in (0, 63, 64, 69):
        want = np.zeros((n1, n2), dtype=np.int64)
        want[i, :] = 1
        if sym:
            want[:, i] = 1
        one("X1", (i, i % KM_D), NAN, want)
    for j in (() if sym else (0, 63, 64, 65)):
        want = np.zeros((n1, n2), dtype=np.int64)
        want[:, j] = 1
        one("X2", (j, j % KM_D), NAN, want)
    one("ls", (KM_D - 1 if ard else 0,), NAN, np.ones((n1, n2), dtype=np.int64))
    one("variance", None, NAN, np.ones((n1, n2), dtype=np.int64))
    for i, j in ((0, 1), (69, 64), (64, 64)):
        want = np.zeros((n1, n2), dtype=np.int64)
        want[i, j] = 1
        one("G", (i, j), NAN, want)
    # an infinite coordinate: the class of the emulator's formula (fake_ops._k / _dr2 through kernel_matrix_combine)
    p = _plant(arrs, "X1", (64, 1), PINF)
    with np.errstate(all="ignore"):
        r = run_on(fake_ops, "cpu", p)["combine"]
    fpm = np.zeros((n1, n2), dtype=bool)
    fpm[64, :] = True
    if sym:
        fpm[:, 64] = True
    assert np.all(np.isfinite(r[~fpm]))
    one("X1", (64, 1), PINF, np.where(fpm, np.where(np.isfinite(r), -1, _cls(r)), 0))


# ------------------------------------------------------------------------------------------------ Cholesky and solves
# (n, extra rows, batch, [(i, j) plants in the lower triangle of K], [(e, c) plants in the extra rows])
POTRF_NF = [
    (100, 5, 0, [(50, 50), (50, 3), (99, 0), (0, 0)], [(2, 0), (4, 57), (0, 99)]),               # a single leaf
    (129, 3, 0, [(128, 128), (128, 5), (64, 64), (127, 126)], [(1, 128), (0, 100), (2, 0)]),     # leaf + 1: the first blocked factorisation
    (600, 4, 0, [(520, 520), (599, 513), (530, 10), (512, 511)], [(3, 513), (0, 130), (1, 599), (2, 511)]),  # the plant in the second 512-column group
    (130, 3, 3, [(70, 2), (129, 129), (128, 0)], [(1, 64), (0, 129)]),                            # batched: planted in entry 1 of 3
]
NF_TABLES["potrf_"] = POTRF_NF


def _potrf_problem(n, extra, batch, tail=0):
    rng = np.random.default_rng(n + extra + batch)
    Ts = []
    for _ in range(max(batch, 1)):
        K, E = _spd(rng, n, extra)
        T = np.vstack([K, E, np.full((tail, n), NAN)])     # (identity_rows: the caller leaves the last n rows uninitialised)
        T[:n][np.triu_indices(n, 1)] = NAN                # never read
        Ts.append(T)
    return np.stack(Ts) if batch else Ts[0]


def _potrf_run(mod, dev, T0, n, identity_rows=False):
    tT = _on(T0, "c", dev)
    invd, info = mod.potrf_(tT, n, identity_rows=identity_rows)
    return {"T": _np(tT), "invd": _np(invd), "info": _np(info).astype(np.int64)}


@pytest.mark.parametrize("case", POTRF_NF, ids=[str(c[:3]) for c in POTRF_NF])
def test_potrf_nonfinite(impl, case):
    """A plant at K[i, j], i >= j: row i of L is the first to depend on it (L[i, j] and with it the pivot i), so info == i + 1,
    rows < i of L and the diagonal-block inverses left of block(i) are bitwise the clean run's.  NaN, 0.0 and -Inf ON the
    diagonal: info == i + 1 as well (a non-positive or NaN pivot).
    A plant in an extra row E[e, c] never meets a pivot: info == 0, L, the block inverses and every other row are bitwise
    clean; X = E L^-T is a forward substitution along the row, X[e, j] = (E[e, j] - sum_{k < j} X[e, k] L[j, k]) / L[j, j], so
    row e is NaN from column c on and clean left of c -- left of c's 128-column block once explicit block inverses are used."""
    mod, dev, who = impl
    n, extra, batch, kplants, eplants = case
    T0 = _potrf_problem(n, extra, batch)
    clean = _potrf_run(mod, dev, T0, n)
    assert np.all(clean["info"] == 0)
    nblk = -(-n // NB)
    b = 1 if batch else None
    at = (lambda *ix: (b,) + ix) if batch else (lambda *ix: ix)   # noqa: E731
    for (i, j) in kplants:
        for val in ((NAN, 0.0, NINF) if i == j else (NAN,)):
            T1 = T0.copy()
            T1[at(i, j)] = val
            got = _potrf_run(mod, dev, T1, n)
            tag = f"potrf_ {who} n={n} K[{i},{j}] = {val}"
            info = got["info"]
            assert info[b or 0] == i + 1, (tag, info)
            wantT = np.full(T0.shape, -1, dtype=np.int64)
            wantT[at(slice(0, i))] = 0
            winv = np.full((max(batch, 1), nblk, NB * NB), -1, dtype=np.int64)
            winv[b or 0, :i // NB] = 0
            if batch:      # the other batch entries: untouched by the plant altogether
                assert np.all(np.delete(info, b) == 0), (tag, info)
                for q in (0, 2):
                    wantT[q] = 0
                    winv[q] = 0
            _check(tag + " -> T", got["T"], clean["T"], wantT)
            _check(tag + " -> invd", got["invd"].reshape(winv.shape), clean["invd"].reshape(winv.shape), winv)
            _count("potrf_")
    for (e, c) in eplants:
        T1 = T0.copy()
        T1[at(n + e, c)] = NAN
        got = _potrf_run(mod, dev, T1, n)
        tag = f"potrf_ {who} n={n} E[{e},{c}] = nan"
        assert np.all(got["info"] == 0), (tag, got["info"])
        wantT = np.zeros(T0.shape, dtype=np.int64)
        wantT[at(n + e, slice(c // NB * NB, c))] = -1
        wantT[at(n + e, slice(c, n))] = 1
        _check(tag + " -> T", got["T"], clean["T"], wantT)
        _check(tag + " -> invd", got["invd"], clean["invd"], 0)
        _count("potrf_")


# (n, extra rows, [(e, c)]) -- identity_rows=True: T = [K; E; n rows the call makes the identity and returns as L^-T]
POTRF_INV_NF = [(100, 4, [(0, 0), (3, 57), (1, 99)]), (300, 3, [(2, 0), (0, 129), (1, 299), (2, 255)])]
NF_TABLES["potrf_"] = POTRF_NF + POTRF_INV_NF


@pytest.mark.parametrize("case", POTRF_INV_NF, ids=[str(c[:2]) for c in POTRF_INV_NF])
def test_potrf_identity_rows_nonfinite(impl, case):
    """identity_rows=True: the same row footprint for a plant in an extra row; L, the block inverses, the other extra rows
    and L^-T (the last n rows) are bitwise clean."""
    mod, dev, who = impl
    n, extra, eplants = case
    T0 = _potrf_problem(n, extra, 0, tail=n)
    clean = _potrf_run(mod, dev, T0, n, identity_rows=True)
    assert np.all(clean["info"] == 0) and np.all(np.isfinite(clean["T"][n + extra:]))
    for (e, c) in eplants:
        T1 = T0.copy()
        T1[n + e, c] = NAN
        got = _potrf_run(mod, dev, T1, n, identity_rows=True)
        tag = f"potrf_(identity_rows) {who} n={n} E[{e},{c}] = nan"
        assert np.all(got["info"] == 0), (tag, got["info"])
        wantT = np.zeros(T0.shape, dtype=np.int64)
        wantT[n + e, c // NB * NB:c] = -1
        wantT[n + e, c:] = 1
        _check(tag + " -> T", got["T"], clean["T"], wantT)
        _check(tag + " -> invd", got["invd"], clean["invd"], 0)
        _count("potrf_")


# (n, rows of B)
SOLVE_NF = [(100, 6), (129, 5), (300, 4)]   # one block; block edge + 1 (a one-row last block); three blocks
for _name in ("trsm_", "trtri_blocks", "transpose_factor"):
    NF_TABLES[_name] = SOLVE_NF


def _solve_problem(n, rows):
    rng = np.random.default_rng(n + rows)
    K, B = _spd(rng, n, rows)
    L = np.linalg.cholesky(K)
    L[np.triu_indices(n, 1)] = NAN     # above the diagonal: never read, in the clean run and in every planted one
    return L, B


@pytest.mark.parametrize("n,rows", SOLVE_NF)
def test_trsm_nonfinite(impl, n, rows):
    """trans = 0, X = B L^-T: forward along the row -- B[r, c] makes row r NaN from column c on, clean left of c's block.
    trans = 1, X = B L^-1: X[r, j] = (B[r, j] - sum_{k > j} X[r, k] L[k, j]) / L[j, j], backward along the row -- NaN up to
    column c, clean right of c's block.  Other rows bitwise clean; the NaN above the diagonal of L is still not read."""
    mod, dev, who = impl
    L, B = _solve_problem(n, rows)
    tL = _on(L, "c", dev)
    invd = mod.trtri_blocks(tL)
    LT, invdT = mod.transpose_factor(tL, invd)

    def run(Bx, trans):
        tB = _on(Bx, "ld", dev)
        mod.trsm_(tB, tL if trans == 0 else LT, invd if trans == 0 else invdT, trans=trans)
        return _np(tB)
    for trans in (0, 1):
        clean = run(B, trans)
        assert np.all(np.isfinite(clean))
        for r, c in [(0, 0), (rows - 1, n - 1), (1, min(57, n - 1)), (2, min(127, n - 1)), (3, min(128, n - 1))]:
            B1 = B.copy()
            B1[r, c] = NAN
            want = np.zeros(B.shape, dtype=np.int64)
            c0, c1 = c // NB * NB, min((c // NB + 1) * NB, n)
            want[r, c0:c1] = -1
            if trans == 0:
                want[r, c:] = 1
            else:
                want[r, :c + 1] = 1
            _check(f"trsm_ {who} n={n} trans={trans} B[{r},{c}] = nan", run(B1, trans), clean, want)
            _count("trsm_")
    _unchanged("trsm_", [(tL, L)])


@pytest.mark.parametrize("n,rows", SOLVE_NF)
def test_trtri_blocks_and_transpose_factor_nonfinite(impl, n, rows):
    """transpose_factor is exact: L[i, j] (i >= j) arrives at LT[j, i], Inf bit-exact, nothing else changes -- the block
    inverses it transposes were taken from the clean L, so invdT is bitwise clean.
    trtri_blocks reads the diagonal blocks: a plant at L[i, j] inside block b makes entry (i, j) of inverse b NaN (inv[i, j]
    = -(sum_k L[i, k] inv[k, j]) / L[i, i] holds L[i, j] inv[j, j]) and leaves every other block bitwise clean.  (The emulator keeps no
    inverses -- its invd is a marker -- so must-set is checked on the device only.)"""
    mod, dev, who = impl
    L, _ = _solve_problem(n, rows)
    nblk = -(-n // NB)
    tL = _on(L, "c", dev)
    invd = mod.trtri_blocks(tL)
    LT, invdT = (_np(x) for x in mod.transpose_factor(tL, invd))
    inv0 = _np(invd).reshape(nblk, NB, NB)
    spots = [(0, 0), (n - 1, n - 1), (n - 1, (n - 1) // NB * NB), (min(70, n - 1), 3)]
    for i, j in spots:
        for val in (NAN, PINF, NINF):
            L1 = L.copy()
            L1[i, j] = val
            t1 = _on(L1, "c", dev)
            LT1, invdT1 = (_np(x) for x in mod.transpose_factor(t1, invd))
            want = np.zeros((n, n), dtype=np.int64)
            want[j, i] = _vcls(val)
            _check(f"transpose_factor {who} n={n} L[{i},{j}] = {val} -> LT", LT1, LT, want)
            _check(f"transpose_factor {who} n={n} L[{i},{j}] = {val} -> invdT", invdT1, invdT, 0)
            _unchanged("transpose_factor", [(t1, L1)])
            _count("transpose_factor")
        L1 = L.copy()
        L1[i, j] = NAN
        t1 = _on(L1, "c", dev)
        inv1 = _np(mod.trtri_blocks(t1)).reshape(nblk, NB, NB)
        want = np.zeros(inv0.shape, dtype=np.int64)
        want[i // NB] = -1
        if who == "ops":
            want[i // NB, i % NB, j % NB] = 1
        _check(f"trtri_blocks {who} n={n} L[{i},{j}] = nan", inv1, inv0, want)
        _unchanged("trtri_blocks", [(t1, L1)])
        _count("trtri_blocks")


# ------------------------------------------------------------------------------------------------ exact operations
NF_TABLES["transpose"] = [(65, 64, 0, 0, "ld"), (65, 64, 1, 0, "off"), (64, 129, 2, 0, "col"), (17, 16, 1, 4, "c")]
# (rows, cols, mode, batch, layout): plain with odd ld; lower / upper kept; batched


@pytest.mark.parametrize("case", NF_TABLES["transpose"], ids=str)
def test_transpose_nonfinite(impl, case):
    """X[i, j] in the kept triangle arrives at out[j, i] -- NaN and both infinities, bit-exact -- and nowhere else."""
    mod, dev, who = impl
    rows, cols, mode, batch, layout = case
    X = np.random.default_rng(rows + cols).normal(size=(batch, rows, cols) if batch else (rows, cols))

    def run(a):
        t = _on(a["X"], layout, dev)
        r = _np(mod.transpose(t, mode=mode))
        _unchanged("transpose", [(t, a["X"])])
        return {"out": r}
    clean = run({"X": X})
    spots = {0: [(0, 0), (rows - 1, cols - 1), (31, 33)], 1: [(0, 0), (rows - 1, 3), (min(33, rows - 1), min(31, cols - 1))],
             2: [(0, 0), (3, cols - 1), (31, 33)]}[mode]
    for i, j in spots:
        for val in (NAN, PINF, NINF):
            idx, oidx = ((batch - 1, i, j), (batch - 1, j, i)) if batch else ((i, j), (j, i))
            _footprint("transpose", who, run, {"X": X}, "X", idx, val, {"out": [oidx]}, clean)


NF_TABLES["symmetrize_"] = [(33, "ld"), (129, "off")]


@pytest.mark.parametrize("n,layout", NF_TABLES["symmetrize_"])
def test_symmetrize_nonfinite(impl, n, layout):
    """(S + S^T) / 2: S[i, j] reaches [i, j] and [j, i] with its own class (Inf + finite, halved), nothing else."""
    mod, dev, who = impl
    S = np.random.default_rng(n).normal(size=(n, n))

    def run(a):
        t = _on(a["S"], layout, dev)
        mod.symmetrize_(t)
        return {"S": _np(t)}
    clean = run({"S": S})
    for i, j in ((0, 0), (n - 1, 0), (5, n - 1), (n - 1, n - 1), (32, 31)):
        for val in (NAN, PINF, NINF):
            _footprint("symmetrize_", who, run, {"S": S}, "S", (i, j), val, {"S": [(i, j), (j, i)]}, clean)


NF_TABLES["diag_add_"] = [(65, 64, "ld"), (64, 130, "off")]


@pytest.mark.parametrize("r,c,layout", NF_TABLES["diag_add_"])
def test_diag_add_nonfinite(impl, r, c, layout):
    """A[i, i] += v[i]: a plant in v[i] or A[i, i] reaches A[i, i]; one off the diagonal stays where it is (untouched)."""
    mod, dev, who = impl
    rng = np.random.default_rng(r + c)
    arrs = {"A": rng.normal(size=(r, c)), "v": rng.normal(size=min(r, c))}

    def run(a):
        t, tv = _on(a["A"], layout, dev), _on(a["v"], "c", dev)
        mod.diag_add_(t, tv)
        _unchanged("diag_add_", [(tv, a["v"])])
        return {"A": _np(t)}
    clean = run(arrs)
    last = min(r, c) - 1
    for val in (NAN, PINF, NINF):
        for i in (0, last, 32):
            _footprint("diag_add_", who, run, arrs, "v", (i,), val, {"A": [(i, i)]}, clean)
            _footprint("diag_add_", who, run, arrs, "A", (i, i), val, {"A": [(i, i)]}, clean)
        _footprint("diag_add_", who, run, arrs, "A", (1, 0), val, {"A": [(1, 0)]}, clean)
        _footprint("diag_add_", who, run, arrs, "A", (r - 1, c - 1) if r != c else (0, c - 1), val,
                   {"A": [(r - 1, c - 1) if r != c else (0, c - 1)]}, clean)


NF_TABLES["moment_rows"] = [(257, 3, "ld"), (64, 8, "off")]


@pytest.mark.parametrize("n2,d,layout", NF_TABLES["moment_rows"])
def test_moment_rows_nonfinite(impl, n2, d, layout):
    """[1; B^T; (B^T)^2]: B[r, c] reaches rows 1 + c and 1 + d + c of column r (-Inf squares to +Inf), nothing else."""
    mod, dev, who = impl
    B = np.random.default_rng(n2 + d).normal(size=(n2, d))

    def run(a):
        t = _on(a["B"], layout, dev)
        r = _np(mod.moment_rows(t))
        _unchanged("moment_rows", [(t, a["B"])])
        return {"out": r}
    ref = lambda a: {"out": np.concatenate([np.ones((1, n2)), a["B"].T, a["B"].T ** 2], 0)}   # noqa: E731
    clean = run({"B": B})
    for r_, c_ in ((0, 0), (n2 - 1, d - 1), (63, 1)):
        for val in (NAN, PINF, NINF):
            _footprint("moment_rows", who, run, {"B": B}, "B", (r_, c_), val, {"out": [(1 + c_, r_), (1 + d + c_, r_)]}, clean, ref)


# (nparts, m, n, alpha, lower, diag_scale)
NF_TABLES["combine_parts"] = [(4, 70, 66, -0.5, False, 1.0), (3, 130, 130, 1.0, True, 0.5),
                              # the count-selected instantiations combine_parts_kernel<8 / 16 / 32> and, at 33, the run-time loop
                              (8, 70, 66, -0.5, False, 1.0), (16, 130, 130, 1.0, True, 0.5), (32, 70, 66, -0.5, False, 1.0),
                              (33, 130, 130, 1.0, True, 0.5)]


@pytest.mark.parametrize("case", NF_TABLES["combine_parts"], ids=str)
def test_combine_parts_nonfinite(impl, case):
    """parts[p, i, j] reaches out[i, j] (alpha's sign on an infinity); lower: a NaN above the diagonal is not read."""
    mod, dev, who = impl
    npart, m, n, alpha, lower, dscale = case
    parts = np.random.default_rng(npart + m).normal(size=(npart, m, n))
    if lower:
        parts[:, ~np.tril(np.ones((m, n), dtype=bool))] = 0.0

    def run(a):
        t = _on(a["parts"], "c", dev)
        r = _np(mod.combine_parts(t, alpha=alpha, lower=lower, diag_scale=dscale))
        _unchanged("combine_parts", [(t, a["parts"])])
        return {"out": r}

    def ref(a):
        r = alpha * a["parts"].sum(0)
        if lower:
            r = np.where(np.tril(np.ones((m, n), dtype=bool)), r, 0.0)
            r[np.diag_indices(min(m, n))] *= dscale
        return {"out": r}
    clean = run({"parts": parts})
    for p, i, j in ((0, 0, 0), (npart - 1, m - 1, n - 1), (1, 64, 63), (npart - 1, m - 1, 0)):
        for val in (NAN, PINF, NINF):
            _footprint("combine_parts", who, run, {"parts": parts}, "parts", (p, i, j), val, {"out": [(i, j)]}, clean, ref)
    if lower:   # above the diagonal: never read
        _footprint("combine_parts", who, run, {"parts": parts}, "parts", (1, 0, n - 1), NAN, {}, clean)


NF_TABLES["lowrank_axpy"] = [(65, 130, 16, "ld"), (300, 63, 5, "off"),
                             (2049, 66, 16, "c")]   # one row past the clamp of gridDim.y: row 2048 is blockIdx.y = 0's second trip


@pytest.mark.parametrize("m,n,k,layout", NF_TABLES["lowrank_axpy"])
def test_lowrank_axpy_nonfinite(impl, m, n, k, layout):
    """alpha X + U V^T: X[i, j] reaches [i, j], U[i, kk] row i, V[j, kk] column j -- exactly."""
    mod, dev, who = impl
    rng = np.random.default_rng(m + n + k)
    arrs = {"X": rng.normal(size=(m, n)), "U": rng.normal(size=(m, k)), "V": rng.normal(size=(n, k))}

    def run(a):
        ts = [_on(a[x], layout, dev) for x in ("X", "U", "V")]
        r = _np(mod.lowrank_axpy(-0.7, *ts))
        _unchanged("lowrank_axpy", zip(ts, (a["X"], a["U"], a["V"])))
        return {"out": r}
    ref = lambda a: {"out": -0.7 * a["X"] + a["U"] @ a["V"].T}   # noqa: E731
    clean = run(arrs)
    for val in (NAN, PINF, NINF):
        for i, j in ((0, 0), (m - 1, n - 1), (64, 62)):
            _footprint("lowrank_axpy", who, run, arrs, "X", (i, j), val, {"out": [(i, j)]}, clean, ref)
        for i, kk in ((0, 0), (m - 1, k - 1)):   # (m - 1: past the clamp, the row of a second trip)
            _footprint("lowrank_axpy", who, run, arrs, "U", (i, kk), val, {"out": [(i,)]}, clean, ref)
        for j, kk in ((0, k - 1), (n - 1, 0)):
            _footprint("lowrank_axpy", who, run, arrs, "V", (j, kk), val, {"out": [(slice(None), j)]}, clean, ref)


NF_TABLES["adam_step_"] = [(257, True), (5000, False),
                           (1048577, False)]   # one element past the grid clamp of 4096 x 256: the last element is a second trip


@pytest.mark.parametrize("n,maxi", NF_TABLES["adam_step_"])
def test_adam_step_nonfinite(impl, n, maxi):
    """A NaN in g[i] makes p, m and v NaN at i and nowhere else; one in p[i] stays in p[i] (m and v do not read p)."""
    mod, dev, who = impl
    rng = np.random.default_rng(n)
    arrs = {"p": rng.normal(size=n), "g": rng.normal(size=n), "m": rng.normal(size=n), "v": rng.uniform(0.1, 1, size=n)}

    def run(a):
        tp, tg, tm, tv = (_on(a[x], "c", dev) for x in ("p", "g", "m", "v"))
        mod.adam_step_(tp, tg, tm, tv, beta1=0.9, beta2=0.999, epsilon=1e-7, step=0.01, maximise=maxi)
        _unchanged("adam_step_", [(tg, a["g"])])
        return {"p": _np(tp), "m": _np(tm), "v": _np(tv)}
    clean = run(arrs)
    for i in _pick((0, 255, 256, 1048575), n):   # (and n - 1)
        _footprint("adam_step_", who, run, arrs, "g", (i,), NAN, {"p": [(i,)], "m": [(i,)], "v": [(i,)]}, clean)
        _footprint("adam_step_", who, run, arrs, "p", (i,), NAN, {"p": [(i,)]}, clean)


# ------------------------------------------------------------------------------------------------ reductions
NF_TABLES["row_stats"] = [(70, 65, 5, "ld"), (257, 128, 16, "c")]   # a second chunk of 4 latents, odd ld; P = 16, block edge


@pytest.mark.parametrize("rows,m,P,layout", NF_TABLES["row_stats"])
def test_row_stats_nonfinite(impl, rows, m, P, layout):
    """At[b, kk] reaches row b of every output (sumsq[b], mv[b, :], wsq[:, b]: every latent); V[kk, p] column p of mv only;
    W[kk, p] latent p of wsq only."""
    mod, dev, who = impl
    rng = np.random.default_rng(rows + m + P)
    arrs = {"At": rng.normal(size=(rows, m)), "V": rng.normal(size=(m, P)), "W": rng.normal(size=(m, P))}

    def run(a):
        tA, tV, tW = _on(a["At"], layout, dev), _on(a["V"], "c", dev), _on(a["W"], "c", dev)
        s, v, w = mod.row_stats(tA, V=tV, W=tW)
        _unchanged("row_stats", [(tA, a["At"]), (tV, a["V"]), (tW, a["W"])])
        return {"sumsq": _np(s), "mv": _np(v), "wsq": _np(w)}
    ref = lambda a: {"sumsq": (a["At"] ** 2).sum(1), "mv": np.einsum("bk,kp->bp", a["At"], a["V"]),   # noqa: E731
                     "wsq": np.einsum("bk,kp->pb", a["At"] ** 2, a["W"] ** 2)}
    clean = run(arrs)
    for val in (NAN, PINF, NINF):
        for b, kk in ((0, 0), (rows - 1, m - 1), (63, 15), (64, 16)):
            _footprint("row_stats", who, run, arrs, "At", (b, kk), val,
                       {"sumsq": [(b,)], "mv": [(b,)], "wsq": [(slice(None), b)]}, clean, ref)
        for kk, p in ((0, 0), (m - 1, P - 1), (16, 4)):
            _footprint("row_stats", who, run, arrs, "V", (kk, p), val, {"mv": [(slice(None), p)]}, clean, ref)
            _footprint("row_stats", who, run, arrs, "W", (kk, p), val, {"wsq": [(p,)]}, clean, ref)


NF_TABLES["row_dot"] = [(255, 256, "ld"), (64, 65, "col"), (257, 513, "off")]


@pytest.mark.parametrize("rows,cols,layout", NF_TABLES["row_dot"])
def test_row_dot_nonfinite(impl, rows, cols, layout):
    """A[i, j] or B[i, j] reaches out[i] only."""
    mod, dev, who = impl
    rng = np.random.default_rng(rows * 3 + cols)
    arrs = {"A": rng.normal(size=(rows, cols)), "B": rng.normal(size=(rows, cols))}

    def run(a):
        tA, tB = _on(a["A"], layout, dev), _on(a["B"], layout, dev)
        r = _np(mod.row_dot(tA, tB))
        _unchanged("row_dot", [(tA, a["A"]), (tB, a["B"])])
        return {"out": r}
    ref = lambda a: {"out": np.einsum("ij,ij->i", a["A"], a["B"])}   # noqa: E731
    clean = run(arrs)
    for val in (NAN, PINF, NINF):
        for i, j in ((0, 0), (rows - 1, cols - 1), (63, 64)):
            _footprint("row_dot", who, run, arrs, "A", (i, j), val, {"out": [(i,)]}, clean, ref)
        _footprint("row_dot", who, run, arrs, "B", (rows - 1, 0), val, {"out": [(rows - 1,)]}, clean, ref)


# (rows, m, P, batched At, layout) -- the contract table's launch kinds with rows > 0
NF_TABLES["project"] = [(1, 16, 1, False, "c"), (40, 128, 2, False, "c"), (300, 129, 2, False, "ld"), (257, 128, 4, False, "c"),
                        (65, 64, 3, True, "c"), (129, 96, 2, False, "off")]


@pytest.mark.parametrize("case", NF_TABLES["project"], ids=str)
def test_project_nonfinite(impl, case):
    """ssq[p, b] = |At[b] Lq_p|^2: At[b, kk] reaches row b in EVERY latent (batched At [P, rows, m]: in its own latent only);
    LqT[p][a, c], a <= c -- the triangle that holds Lq_p -- reaches latent p only, every row."""
    mod, dev, who = impl
    rows, m, P, batched, layout = case
    rng = np.random.default_rng(rows + m + P)
    Lq = np.tril(rng.normal(size=(P, m, m)))
    arrs = {"At": rng.normal(size=(P, rows, m) if batched else (rows, m)), "LqT": np.ascontiguousarray(np.swapaxes(Lq, 1, 2))}

    def run(a):
        tA, tQ = _on(a["At"], layout, dev), _on(a["LqT"], "c", dev)
        r = _np(mod.project(tA, tQ))
        _unchanged("project", [(tA, a["At"]), (tQ, a["LqT"])])
        return {"ssq": r}
    ref = lambda a: {"ssq": np.stack([(((a["At"][p] if batched else a["At"]) @ a["LqT"][p].T) ** 2).sum(1) for p in range(P)])}   # noqa: E731
    clean = run(arrs)
    for b, kk in {(0, 0), (rows - 1, m - 1), (min(63, rows - 1), 15), (min(64, rows - 1), min(64, m - 1))}:
        if batched:
            _footprint("project", who, run, arrs, "At", (P - 1, b, kk), NAN, {"ssq": [(P - 1, b)]}, clean, ref)
        else:
            _footprint("project", who, run, arrs, "At", (b, kk), NAN, {"ssq": [(slice(None), b)]}, clean, ref)
    for p, a_, c_ in {(0, 0, 0), (P - 1, 0, m - 1), (P - 1, m - 1, m - 1), (0, min(3, m - 1), min(15, m - 1))}:
        _footprint("project", who, run, arrs, "LqT", (p, a_, c_), NAN, {"ssq": [(p,)]}, clean, ref)


# (rows, P, per-latent s0 / knn, noise per row, layout of Y)
NF_TABLES["gaussian_varexp_sum"] = [(70, 3, False, True, "ld"), (257, 5, True, False, "off"), (512, 16, True, True, "col")]


@pytest.mark.parametrize("case", NF_TABLES["gaussian_varexp_sum"], ids=str)
def test_gaussian_varexp_sum_nonfinite(impl, case):
    """A NaN in Y, fmean, s0, ssq or the per-row noise makes the sum NaN; fvar = knn - s0 + ssq is NaN at the entries s0 / ssq
    feed and bitwise clean elsewhere.  A negative noise variance gives NaN (its log); zero gives the class of the formula:
    -log(0) / 2 = +Inf against -(positive) / 0 = -Inf in the same term, NaN."""
    mod, dev, who = impl
    rows, P, per, het, layout = case
    rng = np.random.default_rng(rows + P)
    arrs = {"Y": rng.normal(size=(rows, P)), "F": rng.normal(size=(rows, P)), "s0": rng.uniform(0, 0.5, size=(P, rows) if per else (rows,)),
            "ssq": rng.uniform(0, 0.3, size=(P, rows)), "nv": rng.uniform(0.1, 0.5, size=rows) if het else 0.3}
    knn = list(1.0 + 0.1 * np.arange(P)) if per else [1.2]

    def run_on(m_, d_, a):
        tY, tF, ts0, tss = _on(a["Y"], layout, d_), _on(a["F"], "c", d_), _on(a["s0"], "c", d_), _on(a["ssq"], "c", d_)
        nvt = _on(a["nv"], "c", d_) if het else a["nv"]
        out, fvar = m_.gaussian_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, noise_variance=nvt, mean_const=0.1, s0_per_latent=per,
                                           want_fvar=True)
        _unchanged("gaussian_varexp_sum", [(tY, a["Y"]), (tF, a["F"]), (ts0, a["s0"]), (tss, a["ssq"])])
        return {"out": _np(out), "fvar": _np(fvar)}
    run = lambda a: run_on(mod, dev, a)   # noqa: E731

    def ref(a):     # the stated formula, term by term
        fv = np.asarray(knn)[None, :] - (a["s0"].T if per else a["s0"][:, None]) + a["ssq"].T
        nv = a["nv"][:, None] if het else a["nv"]
        ve = -0.5 * np.log(2 * np.pi) - 0.5 * np.log(nv) - 0.5 * ((a["Y"] - a["F"] - 0.1) ** 2 + fv) / nv
        return {"out": np.array([np.broadcast_to(ve, (rows, P)).sum()]), "fvar": fv}
    clean = run(arrs)
    b, p = rows - 1, P - 1
    _footprint("gaussian_varexp_sum", who, run, arrs, "Y", (b, p), NAN, {"out": [(0,)]}, clean, ref)
    _footprint("gaussian_varexp_sum", who, run, arrs, "Y", (0, 0), NAN, {"out": [(0,)]}, clean, ref)
    _footprint("gaussian_varexp_sum", who, run, arrs, "F", (63, 0), NAN, {"out": [(0,)]}, clean, ref)
    _footprint("gaussian_varexp_sum", who, run, arrs, "s0", (p, b) if per else (b,), NAN,
               {"out": [(0,)], "fvar": [(b, p) if per else (b,)]}, clean, ref)
    _footprint("gaussian_varexp_sum", who, run, arrs, "ssq", (0, 64), NAN, {"out": [(0,)], "fvar": [(64, 0)]}, clean, ref)
    if het:
        _footprint("gaussian_varexp_sum", who, run, arrs, "nv", (1,), NAN, {"out": [(0,)]}, clean, ref)
        _footprint("gaussian_varexp_sum", who, run, arrs, "nv", (b,), -0.2, {"out": [(0,)]}, clean, ref)
        _footprint("gaussian_varexp_sum", who, run, arrs, "nv", (2,), 0.0, {"out": [(0,)]}, clean, ref)
    else:
        for val in (NAN, -0.2, 0.0):
            _footprint("gaussian_varexp_sum", who, run, arrs, "nv", None, val, {"out": [(0,)]}, clean, ref)


# (m, P, q_diag)
NF_TABLES["gauss_kl_white"] = [(17, 5, True), (129, 4, False), (40, 1, False)]


@pytest.mark.parametrize("m,P,q_diag", NF_TABLES["gauss_kl_white"])
def test_gauss_kl_white_nonfinite(impl, m, P, q_diag):
    """A NaN in q_mu, or in q_sqrt on or below the diagonal, gives NaN; above the diagonal it is not read.  The diagonal enters
    through log(d^2) and d^2: zero gives +Inf, and a negative entry the bitwise result of its absolute value."""
    mod, dev, who = impl
    rng = np.random.default_rng(m + P)
    if q_diag:
        qs = np.exp(0.3 * rng.normal(size=(m, P)))
    else:
        qs = np.tril(0.1 * rng.normal(size=(P, m, m)))
        qs[:, np.arange(m), np.arange(m)] = np.exp(0.3 * rng.normal(size=(P, m)))
    arrs = {"q_mu": rng.normal(size=(m, P)), "qs": qs}

    def run(a):
        tm, tq = _on(a["q_mu"], "c", dev), _on(a["qs"], "c", dev)
        r = _np(mod.gauss_kl_white(tm, tq))
        _unchanged("gauss_kl_white", [(tm, a["q_mu"]), (tq, a["qs"])])
        return {"kl": r}

    def ref(a):
        L = a["qs"] if q_diag else np.tril(a["qs"])
        d = L if q_diag else np.diagonal(L, axis1=1, axis2=2)
        return {"kl": np.array([0.5 * ((a["q_mu"] ** 2).sum() - m * P - np.log(d ** 2).sum() + (L * L).sum())])}
    clean = run(arrs)
    hit = {"kl": [(0,)]}
    for idx in ((0, 0), (m - 1, P - 1)):
        _footprint("gauss_kl_white", who, run, arrs, "q_mu", idx, NAN, hit, clean, ref)
    dspots = [(0, 0), (m - 1, P - 1)] if q_diag else [(0, 0, 0), (P - 1, m - 1, m - 1)]
    for idx in dspots + ([] if q_diag else [(P - 1, m - 1, 0), (0, min(16, m - 1), 15)]):
        _footprint("gauss_kl_white", who, run, arrs, "qs", idx, NAN, hit, clean, ref)
    for idx in dspots:
        _footprint("gauss_kl_white", who, run, arrs, "qs", idx, 0.0, hit, clean, ref)
        _footprint("gauss_kl_white", who, run, arrs, "qs", idx, -qs[idx], {}, clean, ref)    # |d| gives the same bits
    if not q_diag:
        for idx in ((0, 0, m - 1), (P - 1, m - 2, m - 1)):
            _footprint("gauss_kl_white", who, run, arrs, "qs", idx, NAN, {}, clean, ref)     # above the diagonal: not read


NF_TABLES["sum_log_diag"] = [(129, 0), (257, 3)]


@pytest.mark.parametrize("n,batch", NF_TABLES["sum_log_diag"])
def test_sum_log_diag_nonfinite(impl, n, batch):
    """A zero diagonal entry gives -Inf, a negative or NaN one NaN -- in its own batch entry; the others are bitwise clean.  Off the
    diagonal nothing is read."""
    mod, dev, who = impl
    rng = np.random.default_rng(n)
    L = rng.normal(size=(max(batch, 1), n, n))
    L[:, np.arange(n), np.arange(n)] = np.exp(rng.normal(size=(max(batch, 1), n)))
    arrs = {"L": L if batch else L[0]}

    def run(a):
        t = _on(a["L"], "c", dev)
        r = _np(mod.sum_log_diag(t))
        _unchanged("sum_log_diag", [(t, a["L"])])
        return {"out": r}
    ref = lambda a: {"out": np.log(np.diagonal(a["L"] if batch else a["L"][None], axis1=1, axis2=2)).sum(1)}   # noqa: E731
    clean = run(arrs)
    z = 1 if batch else 0
    for i in (0, n - 1, 128):
        for val in (0.0, -0.5, NAN):
            _footprint("sum_log_diag", who, run, arrs, "L", (z, i, i) if batch else (i, i), val, {"out": [(z,)]}, clean, ref)
    _footprint("sum_log_diag", who, run, arrs, "L", (z, 1, 0) if batch else (1, 0), NAN, {}, clean, ref)


# (rows, cols, upper_only, layout)
NF_TABLES["sumsq"] = [(255, 257, True, "ld"), (1025, 64, False, "off")]


@pytest.mark.parametrize("case", NF_TABLES["sumsq"], ids=str)
def test_sumsq_nonfinite(impl, case):
    """A NaN gives NaN and an infinity +Inf; upper_only: below the diagonal nothing is read."""
    mod, dev, who = impl
    rows, cols, upper, layout = case
    A = np.random.default_rng(rows + cols).normal(size=(rows, cols))

    def run(a):
        t = _on(a["A"], layout, dev)
        r = _np(mod.sumsq(t, upper_only=upper))
        _unchanged("sumsq", [(t, a["A"])])
        return {"out": r}
    ref = lambda a: {"out": np.array([((np.triu(a["A"]) if upper else a["A"]) ** 2).sum()])}   # noqa: E731
    clean = run({"A": A})
    for i, j in ((0, 0), (min(rows, cols) - 1, cols - 1), (3, cols - 1)):
        for val in (NAN, PINF, NINF):
            _footprint("sumsq", who, run, {"A": A}, "A", (i, j), val, {"out": [(0,)]}, clean, ref)
    if upper:
        for i, j in ((1, 0), (rows - 1, 0), (rows - 1, rows - 2)):
            _footprint("sumsq", who, run, {"A": A}, "A", (i, j), NAN, {}, clean, ref)
    else:
        _footprint("sumsq", who, run, {"A": A}, "A", (rows - 1, 0), NAN, {"out": [(0,)]}, clean, ref)


NF_TABLES["stationary_adjoint_tail"] = [(257, 3, False), (300, 8, True)]


@pytest.mark.parametrize("n1,d,sym", NF_TABLES["stationary_adjoint_tail"])
def test_stationary_adjoint_tail_nonfinite(impl, n1, d, sym):
    """R = [rs, GB, GB2].  rs[i] enters T[i, :] = GB[i] - A[i] rs[i], so row i of A_bar, every d/dls (column sums over T) and
    d/dvariance (the sum of rs) are NaN; GB[i, dd] enters T[i, dd] only: A_bar[i, dd] and d/dls[dd]; GB2[i, dd] (read by the
    non-symmetric form only) reaches d/dls[dd] alone.  All other rows of A_bar are bitwise clean."""
    mod, dev, who = impl
    rng = np.random.default_rng(n1 + d)
    arrs = {"R": rng.normal(size=(n1, 1 + 2 * d)), "A": rng.normal(size=(n1, d)), "ls": 0.5 + rng.uniform(size=d)}

    def run(a):
        tR, tA, tl = _on(a["R"], "c", dev), _on(a["A"], "c", dev), _on(a["ls"], "c", dev)
        sv, sl, Ab = mod.stationary_adjoint_tail(tR, tA, tl, variance=1.4, symmetric=sym)
        _unchanged("stationary_adjoint_tail", [(tR, a["R"]), (tA, a["A"]), (tl, a["ls"])])
        return {"dvar": _np(sv), "dls": _np(sl), "Abar": _np(Ab)}
    clean = run(arrs)
    for i in (0, n1 - 1, 255, 256):
        _footprint("stationary_adjoint_tail", who, run, arrs, "R", (i, 0), NAN,
                   {"dvar": [(0,)], "dls": [slice(None)], "Abar": [(i,)]}, clean)
        dd = i % d
        _footprint("stationary_adjoint_tail", who, run, arrs, "R", (i, 1 + dd), NAN, {"dls": [(dd,)], "Abar": [(i, dd)]}, clean)
        _footprint("stationary_adjoint_tail", who, run, arrs, "R", (i, 1 + d + dd), NAN, {} if sym else {"dls": [(dd,)]}, clean)


# ------------------------------------------------------------------------------------------------ fused drivers
FORMS = [(True, False), (True, True), (False, False), (False, True)]    # (whiten, q_diag)
NF_TABLES["svgp_elbo_shard"] = [(f, w, q) for f in FAMILIES for (w, q) in FORMS]


def _driver_check(tag, plant, clean, got, kuu, kl_clean):
    """out[0] is NaN; a plant that cannot reach Kuu leaves info == 0; the whitened KL does not read the minibatch."""
    out, info = got
    assert np.isnan(out[0]), f"{tag} [{plant}]: out[0] = {out[0]!r} (info {info}) -- the planted NaN was swallowed"
    if not kuu:
        assert np.all(info == 0), (tag, plant, info)
    if kl_clean:
        assert _same_bits(out[1], clean[0][1]), f"{tag} [{plant}]: the whitened KL changed: {out[1]!r} vs {clean[0][1]!r}"


@pytest.mark.parametrize("family,whiten,q_diag", NF_TABLES["svgp_elbo_shard"])
def test_svgp_elbo_shard_nonfinite(impl, family, whiten, q_diag):
    """M = 40, 60 rows, P = 2, per-row noise.  A NaN in Xb, Yb, the noise rows, q_mu, tril(q_sqrt), a lengthscale, the variance
    or mean_const: out[0] is NaN (the Matern families are the point: the clamp of r2 must not swallow it).  The whitened KL is
    bitwise the clean value for a plant in the minibatch.  A NaN in Z: info != 0 or a NaN result, never a finite value
    with info == 0."""
    mod, dev, who = impl
    M, rows, d, P = 40, 60, 2, 2
    rng = np.random.default_rng(FAMILIES.index(family) * 4 + whiten * 2 + q_diag)
    Z, X, Y, q_mu, qs = _svgp_inputs(rng, M, rows, d, P, q_diag)
    ard = bool(FAMILIES.index(family) % 2)
    arrs = {"Z": Z, "Xb": X, "Yb": Y, "q_mu": q_mu, "qs": qs, "nv": rng.uniform(0.1, 0.3, size=rows),
            "ls": np.array([0.9, 1.1]) if ard else np.array([0.9]), "variance": 1.1, "mean_const": 0.05}

    def run(a):
        tX, tY = _on(a["Xb"], "ld", dev), _on(a["Yb"], "ld", dev)
        out, info = mod.svgp_elbo_shard(_on(a["Z"], "c", dev), tX, tY, _on(a["q_mu"], "c", dev), _on(a["qs"], "c", dev), whiten=whiten,
                                        variance=a["variance"], lengthscales=_lsarg(a["ls"]), noise_variance=_on(a["nv"], "c", dev),
                                        jitter=1e-6, mean_const=a["mean_const"], family=family)
        _unchanged("svgp_elbo_shard", [(tX, a["Xb"]), (tY, a["Yb"])])
        return _np(out), _np(info).astype(np.int64)
    clean = run(arrs)
    assert np.all(clean[1] == 0) and np.all(np.isfinite(clean[0])), clean
    tag = f"svgp_elbo_shard {who} {family} whiten={whiten} q_diag={q_diag}"
    qidx = (5, 1) if q_diag else (1, 5, 2)
    # (input, index, may reach Kuu, whitened KL must stay bitwise)
    for inp, idx, kuu, kl in (("Xb", (7, 1), False, True), ("Yb", (5, 1), False, True), ("nv", (9,), False, True), ("q_mu", (3, 1), False, False),
                              ("qs", qidx, False, False), ("ls", (len(arrs["ls"]) - 1,), True, False), ("variance", None, True, False),
                              ("mean_const", None, False, False)):
        _driver_check(tag, f"{inp}{idx}", clean, run(_plant(arrs, inp, idx, NAN)), kuu, kl and whiten)
        _count("svgp_elbo_shard")
    out, info = run(_plant(arrs, "Z", (4, 0), NAN))
    assert info[0] != 0 or np.isnan(out[0]), f"{tag} [Z]: finite {out!r} with info == 0"
    _count("svgp_elbo_shard")


NF_TABLES["svgp_elbo_shard_sep"] = [(65, 50, 4, "c"), (129, 64, 4, "ld")]   # all four families, one per latent; leaf edges


@pytest.mark.parametrize("M,rows,P,layout", NF_TABLES["svgp_elbo_shard_sep"])
def test_svgp_elbo_shard_sep_nonfinite(impl, M, rows, P, layout):
    """One kernel per latent (SquaredExponential, Matern32, Matern52, Matern12): the same statements, and a NaN in latent p's
    lengthscale or variance may change info[p] only -- the other latents' status stays 0."""
    mod, dev, who = impl
    rng = np.random.default_rng(M + rows)
    Z, X, Y, q_mu, qs = _svgp_inputs(rng, M, rows, 2, P, False)
    families = ["SquaredExponential", "Matern32", "Matern52", "Matern12"][:P]
    arrs = {"Z": Z, "Xb": X, "Yb": Y, "q_mu": q_mu, "qs": qs, "nv": rng.uniform(0.1, 0.3, size=rows),
            "ls": 0.8 + 0.1 * np.arange(P), "variances": 1.0 + 0.1 * np.arange(P), "mean_const": 0.05}

    def run(a):
        tX, tY = _on(a["Xb"], layout, dev), _on(a["Yb"], layout, dev)
        out, info = mod.svgp_elbo_shard_sep(_on(a["Z"], "c", dev), tX, tY, _on(a["q_mu"], "c", dev), _on(a["qs"], "c", dev),
                                            variances=list(a["variances"]), lengthscales=list(a["ls"]), families=families,
                                            noise_variance=_on(a["nv"], "c", dev), jitter=1e-6, mean_const=a["mean_const"])
        _unchanged("svgp_elbo_shard_sep", [(tX, a["Xb"]), (tY, a["Yb"])])
        return _np(out), _np(info).astype(np.int64)
    clean = run(arrs)
    assert np.all(clean[1] == 0) and np.all(np.isfinite(clean[0])), clean
    tag = f"svgp_elbo_shard_sep {who} M={M}"
    for inp, idx, kl in (("Xb", (7, 1), True), ("Xb", (rows - 1, 0), True), ("Yb", (5, P - 1), True), ("nv", (9,), True),
                         ("q_mu", (3, 1), False), ("qs", (P - 1, 5, 2), False), ("mean_const", None, False)):
        _driver_check(tag, f"{inp}{idx}", clean, run(_plant(arrs, inp, idx, NAN)), False, kl)
        _count("svgp_elbo_shard_sep")
    for p in range(P):
        for inp in ("ls", "variances"):
            out, info = run(_plant(arrs, inp, (p,), NAN))
            assert np.isnan(out[0]), f"{tag} [{inp}[{p}] ({families[p]})]: out[0] = {out[0]!r} (info {info})"
            assert np.all(np.delete(info, p) == 0), f"{tag} [{inp}[{p}]]: another latent's status changed: {info}"
            _count("svgp_elbo_shard_sep")
    out, info = run(_plant(arrs, "Z", (4, 0), NAN))
    assert np.any(info != 0) or np.isnan(out[0]), f"{tag} [Z]: finite {out!r} with info == 0"
    _count("svgp_elbo_shard_sep")


# (n, P, family)
NF_TABLES["gpr_lml"] = [(60, 2, f) for f in FAMILIES] + [(129, 1, "Matern52"), (300, 2, "Matern32")]


@pytest.mark.parametrize("n,P,family", NF_TABLES["gpr_lml"])
def test_gpr_lml_nonfinite(impl, n, P, family):
    """A NaN in Y, the per-row noise, a lengthscale, the variance or mean_const: the LML is NaN.  A NaN in X: info != 0 or a NaN
    LML, never a finite value with info == 0."""
    mod, dev, who = impl
    rng = np.random.default_rng(n + P)
    ard = bool(FAMILIES.index(family) % 2)
    arrs = {"X": rng.normal(size=(n, 2)), "Y": rng.normal(size=(n, P)), "nv": rng.uniform(0.1, 0.3, size=n),
            "ls": np.array([0.8, 1.0]) if ard else np.array([0.8]), "variance": 1.2, "mean_const": 0.1}

    def run(a):
        tX, tY = _on(a["X"], "c", dev), _on(a["Y"], "c", dev)
        out, info = mod.gpr_lml(tX, tY, variance=a["variance"], lengthscales=_lsarg(a["ls"]), noise_variance=_on(a["nv"], "c", dev),
                                mean_const=a["mean_const"], family=family)
        _unchanged("gpr_lml", [(tX, a["X"]), (tY, a["Y"])])
        return _np(out), _np(info).astype(np.int64)
    clean = run(arrs)
    assert clean[1][0] == 0 and np.isfinite(clean[0][0]), clean
    tag = f"gpr_lml {who} n={n} {family}"
    for inp, idx, kuu in (("Y", (5, P - 1), False), ("Y", (n - 1, 0), False), ("nv", (9,), True), ("ls", (len(arrs["ls"]) - 1,), True),
                          ("variance", None, True), ("mean_const", None, False)):
        _driver_check(tag, f"{inp}{idx}", clean, run(_plant(arrs, inp, idx, NAN)), kuu, False)
        _count("gpr_lml")
    for idx in ((7, 1), (n - 1, 0)):
        out, info = run(_plant(arrs, "X", idx, NAN))
        assert info[0] != 0 or np.isnan(out[0]), f"{tag} [X{idx}]: finite {out!r} with info == 0"
        _count("gpr_lml")


# ------------------------------------------------------------------------------------------------ model level
def _kernel(gpflow, name, **kw):
    return getattr(gpflow.kernels, name)(**kw)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["Matern32", "SquaredExponential"])    # (SquaredExponential: the control)
@pytest.mark.parametrize("where", ["X", "lengthscale"])
def test_gpr_model_nonfinite(gpu, family, where):
    """GPR with a NaN in X or a NaN lengthscale raises GpkError (the factorisation's status) or returns a NaN LML."""
    import gpflow_amd as gpflow
    from gpflow_amd import _lib
    rng = np.random.default_rng(0)
    X = rng.normal(size=(120, 2))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(120, 1))
    if where == "X":
        X[17, 1] = NAN
    m = gpflow.models.GPR((X, Y), _kernel(gpflow, family, lengthscales=0.9), noise_variance=0.1)
    if where == "lengthscale":   # (assign refuses NaN, as the reference does; an optimiser step writes the unconstrained value)
        m.kernel.lengthscales.assign_unconstrained(NAN)
        assert np.isnan(m.kernel.lengthscales.numpy())
    try:
        lml = float(m.log_marginal_likelihood())
    except _lib.GpkError:
        return
    assert np.isnan(lml), f"GPR({family}) with a NaN {where}: finite LML {lml!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["Matern52", "SquaredExponential"])    # (SquaredExponential: the control)
def test_svgp_model_nonfinite(gpu, family):
    """SVGP.elbo and elbo_and_grad on a minibatch with one NaN coordinate return a NaN value."""
    import gpflow_amd as gpflow
    rng = np.random.default_rng(1)
    X = rng.normal(size=(200, 2))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(200, 1))
    Z = X[:32] + 0.01 * rng.normal(size=(32, 2))
    m = gpflow.models.SVGP(_kernel(gpflow, family, lengthscales=0.9), gpflow.likelihoods.Gaussian(0.1), Z, num_data=2000)
    assert np.isfinite(float(m.elbo((X, Y))))
    X[7, 1] = NAN
    elbo = float(m.elbo((X, Y)))
    assert np.isnan(elbo), f"SVGP({family}).elbo with a NaN coordinate: {elbo!r}"
    v, _ = m.elbo_and_grad((X, Y))
    assert np.isnan(float(v)), f"SVGP({family}).elbo_and_grad with a NaN coordinate: value {float(v)!r}"


# ------------------------------------------------------------------------------------------------ CPU-tier guard
NOT_COVERED = dict(NOT_PRIMITIVES, check_info="reads the status word only: covered by the potrf_ cases (info == i + 1 on both sides)")


def test_every_shared_primitive_has_a_nonfinite_table():
    """A primitive shared by fake_ops and ops without a non-finite case table here fails this test (or it is listed in
    NOT_COVERED with the reason)."""
    shared = shared_primitives()
    missing = [n for n in shared if n not in NF_TABLES and n not in NOT_COVERED]
    assert not missing, f"shared primitives without a non-finite case table: {missing}"
    stale = [n for n in list(NF_TABLES) + list(NOT_COVERED) if n not in shared]
    assert not stale, f"tables for names that are no longer shared primitives: {stale}"
    assert all(len(t) > 0 for t in NF_TABLES.values())
    print("planted runs in this process:", {k: PLANTS[k] for k in sorted(PLANTS)})
