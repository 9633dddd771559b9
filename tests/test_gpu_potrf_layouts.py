"""The trapezoidal Cholesky and the solves against a factor, held to a LAPACK reference in every operand layout.

gpk_potrf_core decides twice.  The shape decisions (potrf_plan.h) are pinned by tests/test_potrf_plan.py.  The operand decisions are
taken at enqueue time, from the parity of lda, the 16-byte alignment of A and the parity of the batch stride: flag word or event for
"panel solved", split or whole rest-update, fused in-group kernel or per-block GEMM loop, progressive first group or the re-plan, the
vector loads of the leaf, the GEMM variant.  Every other potrf_ call of the suite hands over a fresh contiguous tensor, so there lda == n
and the fallbacks run only where n happens to be odd.  Here ONE table (POTRF_ROWS) names, per shape, the plan features it is there for
and the layouts (_on of test_gpu_contract.py) it runs in:
  c / pad / bpad   aligned: the fast kernels, with lda != n (pad) or a padded batch stride (bpad);
  ld / off / col / bodd   odd lda, a base one element in, a column slice, an odd batch stride: the generic GEMM kernel everywhere, the
                   per-block group loop, events instead of flag words, the re-plan of a progressive first group.
CPU tier (no device): every row is pinned to its feature column through tests/potrf_plan_dump.cpp, and every row x layout runs through
fake_ops.potrf_ on CPU tensors under the same checker -- which proves the checker and the layouts before a device is involved.
GPU tier, per row x layout: status, values (normwise backward errors with c = 4 and elementwise against LAPACK), the strict upper
triangle, nothing written outside the view, a second call bitwise equal, pad bitwise equal to c, and the GEMM kinds that ran.
A new layout case goes into POTRF_ROWS (factorisation) or SOLVE_SHAPES / SOLVE_L_LAYOUTS (solves) below.
"""
import ctypes as C
import functools
import hashlib

import numpy as np
import pytest
import scipy.linalg as sla
import torch

from test_gpu_contract import (LD, NAN, U, _bits, _chol_checks, _np, _on, _padding_untouched, _same_bits, _spd, fake_ops)
from test_potrf_plan import NB, dumper, group_ends, path, plan, progressive_ends  # noqa: F401  (dumper: a fixture)

ALIGNED = ("c", "pad", "bpad")          # every operand predicate as in c: the same kernels on the same grids
UNALIGNED = ("ld", "off", "col", "bodd")


class Row:
    def __init__(self, n, extra, batch, zero_upper, layouts, pins, identity=False):
        self.n, self.extra, self.batch, self.zero_upper, self.layouts, self.pins, self.identity = n, extra, batch, zero_upper, layouts, pins, identity
        self.id = "n%d_x%d_b%d%s" % (n, extra, batch, "_inv" if identity else "")


# The feature column: what tests/potrf_plan_dump.cpp prints for the shape (bulk_cus 224, flags usable); test_rows_are_on_their_branches
# holds every row to it, so a retuned threshold cannot move a row off its branch unnoticed.
#   path / xstream / ends / prog / tiled: as in test_potrf_plan.PINS;  flags, splits: flag_candidate / rest_split_candidate panels;
#   split_rem: split candidates with a remainder (c3 < n);  tile64: rest_tile64_candidate panels;  wide / queue: panels wider than
#   128 columns / with the tile queue;  cap: bulk.cap;  replan_ends: group ends after plan_extra_rows(false)
POTRF_ROWS = [
    # the extra rows ride through the panel solves (R = n + extra)
    Row(640, 130, 1, True, ("c", "pad", "ld", "off", "col"),
        dict(path="ride", ends=[], prog=[], tiled=0, flags=4, splits=4, split_rem=2, tile64=0, R=770)),
    # X stream: a 3- and a 2-block fused group (staged kernel), split rest-updates with and without a remainder
    Row(640, 1024, 1, False, ("c", "pad", "ld", "off", "col"),
        dict(path="X", xstream="X", ends=[384, 640], prog=[], tiled=0, flags=4, splits=4, split_rem=2, tile64=0)),
    # the same plus the progressive first group and tiled rest-updates (pipelined group kernel); in ld / off / col: the re-plan
    Row(640, 6144, 1, True, ("c", "pad", "ld", "off", "col"),
        dict(path="X", xstream="X", ends=[384, 640], prog=[128, 256, 384], tiled=1, flags=4, splits=4, split_rem=2, tile64=0,
             replan_ends=[384, 640])),
    # tiled rest-updates with one 64 x 64-tile panel (pre64 when aligned, the generic 64 x 64 tile otherwise), three groups
    Row(896, 3000, 1, False, ("c", "pad", "ld", "off"),
        dict(path="X", xstream="X", ends=[384, 768, 896], prog=[], tiled=1, flags=6, splits=5, split_rem=3, tile64=1)),
    # tail zone: 256-column groups (2-block fused), then single-block groups at 896 / 1024 / 1152
    Row(1152, 1024, 1, True, ("c", "pad", "ld", "off"),
        dict(path="X tail_zone", xstream="X", ends=[256, 512, 768, 896, 1024, 1152], prog=[], tiled=0, flags=8, splits=8, split_rem=6,
             tile64=0)),
    # large: one 640-wide panel on the masked stream with the tile queue, 28 narrow panels on Bs, extra rows on the masked stream
    Row(4224, 300, 1, False, ("c", "pad", "off"),
        dict(path="large X", xstream="B_masked", ends=[640, 1152, 1664, 2176, 2688, 3200, 3712, 4224], prog=[], tiled=0, flags=21,
             splits=21, split_rem=19, tile64=0, wide=1, queue=1)),
    # batched: cap 320, fused batched group solve (bodd: the per-block loop)
    Row(384, 1024, 2, True, ("c", "bpad", "bodd"),
        dict(path="X", xstream="X", ends=[256, 384], prog=[], tiled=0, flags=2, splits=2, split_rem=0, tile64=0, cap=320)),
    # batched ride
    Row(130, 7, 3, False, ("c", "bpad", "bodd"),
        dict(path="ride", ends=[], prog=[], tiled=0, flags=1, splits=1, split_rem=0, tile64=0, cap=320, R=137)),
    # batched ride whose second strip waits in-kernel with 4 x 57 = 228 workgroups: capped at the 224 compute units of the bulk
    # stream's mask (56 per problem), so one workgroup per problem walks two row blocks (tests/test_potrf_schedule.py, assertion 7)
    Row(1152, 8, 4, True, ("c",),
        dict(path="ride", ends=[], prog=[], tiled=0, flags=8, splits=8, split_rem=6, tile64=0, cap=320, R=1160)),
    # gpk_potrf_inv: the identity rows are written by the call (set_identity with lda != n) and shorten the groups' row ranges
    Row(640, 1024, 1, False, ("pad", "ld"),
        dict(path="X", xstream="X", ends=[384, 640], prog=[], tiled=0, flags=4, splits=4, split_rem=2, tile64=0), identity=True),
]
ROW_LAYOUTS = [(row, layout) for row in POTRF_ROWS for layout in row.layouts]
ROW_LAYOUT_IDS = ["%s-%s" % (row.id, layout) for row, layout in ROW_LAYOUTS]


# ------------------------------------------------------------------------------------------------ CPU tier: the plan pins
@pytest.mark.parametrize("row", POTRF_ROWS, ids=[r.id for r in POTRF_ROWS])
def test_rows_are_on_their_branches(dumper, row):
    n, want = row.n, row.pins
    extra = row.extra + (n if row.identity else 0)
    whole, panels = plan(dumper, n, extra, row.batch, n if row.identity else 0)
    assert path(whole) == want["path"]
    if "xstream" in want:
        assert whole["X"] == want["xstream"]
    assert whole["R"] == want.get("R", n)
    assert group_ends(panels) == want["ends"]
    assert progressive_ends(panels) == want["prog"]
    assert whole["progressive_candidate"] == (1 if want["prog"] else 0)
    assert whole["rest_tiled"] == want["tiled"]
    assert sum(q["flag_candidate"] for q in panels) == want["flags"]
    split = [q for q in panels if q["rest_split_candidate"]]
    assert len(split) == want["splits"] and sum(1 for q in split if q["c3"] < n) == want["split_rem"]
    assert sum(q["rest_tile64_candidate"] for q in panels) == want["tile64"]
    wide = sum(1 for q in panels if q["c1"] - q["c0"] > NB)
    assert wide == want.get("wide", 0) and sum(q["rest_tile_queue"] for q in panels) == want.get("queue", 0)
    if whole["large"]:   # narrow panels on Bs, flag candidates except where a group of the masked stream ends
        assert len(panels) - wide == 28 and all(q["narrow"] and q["rest_stream"] == "Bs" for q in panels[wide:])
        assert [q["flag_candidate"] for q in panels] == [0 if (q["x_group_end"] or q["c1"] == n or not q["narrow"]) else 1 for q in panels]
    if "cap" in want:
        assert whole["bulk.cap"] == want["cap"]
    if want["prog"]:     # what ld / off / col get: the groups planned again, no progressive block
        assert whole["prog_end"] == want["prog"][-1]
        _, again = plan(dumper, n, extra, row.batch, n if row.identity else 0, replan=1)
        assert group_ends(again) == want["replan_ends"] and progressive_ends(again) == []


def test_table_covers_every_layout_and_both_zero_upper():
    assert {layout for _, layout in ROW_LAYOUTS} == set(ALIGNED) | set(UNALIGNED)
    assert abs(sum(1 for r in POTRF_ROWS if r.zero_upper) - sum(1 for r in POTRF_ROWS if not r.zero_upper)) <= 1


# ------------------------------------------------------------------------------------------------ inputs and references, once per shape
class Ref:
    """Inputs (_spd of test_gpu_contract.py, rng = default_rng(n + extra)) and the float64 LAPACK reference of one table row."""

    def __init__(self, row):
        n = row.n
        rng = np.random.default_rng(n + row.extra)
        self.K, self.E, self.L, self.X = [], [], [], []
        for _ in range(row.batch):
            K, E = _spd(rng, n, row.extra)
            if row.identity:
                E = np.vstack([E, np.eye(n)])
            Lr = np.linalg.cholesky(K)
            self.K.append(K)
            self.E.append(E)
            self.L.append(Lr)
            self.X.append(sla.solve_triangular(Lr, E.T, lower=True, check_finite=False).T)
        self.up = np.triu(np.ones((n, n), dtype=bool), 1)

    def input(self, row):
        """[K; E] with the strict upper triangle NaN (never read), the identity rows of gpk_potrf_inv NaN (written by the call)"""
        n, Ts = row.n, []
        for K, E in zip(self.K, self.E):
            T = np.vstack([K, E])
            T[:n][self.up] = NAN
            if row.identity:
                T[T.shape[0] - n:] = NAN
            Ts.append(T)
        return np.stack(Ts) if row.batch > 1 else Ts[0]


@functools.lru_cache(maxsize=None)
def _ref(row):
    return Ref(row)


def _backward_errors_f64(who, T, K, E, n):
    """_chol_checks' two normwise backward errors (c = 4) with the residuals evaluated in float64 (above n = 513 a longdouble product
    takes minutes).  Evaluated this way, LAPACK's own factor and solve sit at <= 3.5e-4 (K - L L^T) and <= 1.6e-5 (E - X L^T) of the
    bound on the single-problem shapes of the table: the evaluation's own rounding is far below what the bound allows."""
    L = np.tril(T[:n])
    r1, b1 = np.linalg.norm(K - L @ L.T), 4 * (n + 1) * U * np.linalg.norm(K)
    print(f"  {who}: |K - LL^T|_F / bound = {r1 / b1:.3e}")
    assert r1 <= b1, f"potrf {who}: |K - LL^T|"
    if E.shape[0]:
        X = T[n:]
        r2, b2 = np.linalg.norm(E - X @ L.T), 4 * (n + 1) * U * np.linalg.norm(X) * np.linalg.norm(L)
        print(f"  {who}: |E - XL^T|_F / bound = {r2 / b2:.3e}")
        assert r2 <= b2, f"potrf {who}: |E - X L^T|"


def _first_bad(err, tol):
    i = int(np.argmax(err > tol))
    return "%d entries over %g, first at (row %d, column %d), error %.3e" % (int((err > tol).sum()), tol, i // err.shape[1], i % err.shape[1],
                                                                            err.reshape(-1)[i])


def _check_values(who, row, got):
    """check 2: normwise backward errors (c = 4), elementwise against LAPACK (test_potrf_trapezoid's tolerances: 5e-13 on L, 1e-11 on
    the solved rows; a blocked float64 re-implementation with explicit 128-block inverses differs from LAPACK by <= 8e-15 on these
    inputs), and the strict upper triangle: exact zeros with zero_upper, else bitwise the NaNs that went in."""
    ref, n = _ref(row), row.n
    up_in = np.full((n, n), NAN)
    for b in range(row.batch):
        T = got[b] if row.batch > 1 else got
        tag = f"{who} [{b}]" if row.batch > 1 else who
        up = T[:n][ref.up]
        if row.zero_upper:
            assert np.all(_bits(up) == 0), f"potrf {tag}: zero_upper"
        else:
            assert _same_bits(up, up_in[ref.up]), f"potrf {tag}: upper triangle written"
        Tl = np.vstack([np.tril(T[:n]), T[n:]])
        assert np.all(np.isfinite(Tl)), f"potrf {tag}: {int((~np.isfinite(Tl)).sum())} non-finite entries, first at flat index " \
                                        f"{int(np.argmax(~np.isfinite(Tl).reshape(-1)))} of a [{Tl.shape[0]}, {n}] result"
        eL, eX = np.abs(Tl[:n] - ref.L[b]), np.abs(Tl[n:] - ref.X[b])
        print(f"  {tag}: max |L - L_ref| = {eL.max():.3e}, max |X - X_ref| = {eX.max() if eX.size else 0.0:.3e}")
        assert eL.max() <= 5e-13, f"potrf {tag}: L against LAPACK: " + _first_bad(eL, 5e-13)
        if eX.size:
            assert eX.max() <= 1e-11, f"potrf {tag}: solved rows against LAPACK: " + _first_bad(eX, 1e-11)
        if n <= 513:
            # (residuals in longdouble; the upper triangle was checked above, on the result itself)
            _chol_checks(tag, Tl, ref.K[b].astype(LD), ref.E[b].astype(LD), n, True, None)
        else:
            _backward_errors_f64(tag, Tl, ref.K[b], ref.E[b], n)


def _check_info(who, info):
    """check 1: 0 for every batch entry; INT_MAX is a lost hand-off between the factorisation's streams, not a bad pivot"""
    from gpflow_amd import ops
    st = _np(info)
    assert not np.any(st == ops.INFO_HANDOFF_TIMEOUT), f"potrf {who}: status INT_MAX (ops.INFO_HANDOFF_TIMEOUT): an internal hand-off timed out, {st}"
    assert np.all(st == 0), f"potrf {who}: not positive definite? status {st}"


def _factor(impl, dev, row, layout):
    tT, buf = _on(_ref(row).input(row), layout, dev, base=True)
    _, info = impl.potrf_(tT, row.n, zero_upper=row.zero_upper, identity_rows=row.identity)
    return tT, buf, info


def _checked(who, impl, dev, row, layout):
    """one factorisation in `layout` under checks 1 - 3; returns the result"""
    tT, buf, info = _factor(impl, dev, row, layout)
    _check_info(who, info)
    got = _np(tT)
    _check_values(who, row, got)
    assert _padding_untouched(tT, buf), f"potrf {who}: written outside the view (layout {layout})"     # check 3
    return got


# ------------------------------------------------------------------------------------------------ CPU tier: the checker on fake_ops
_fake_c = {}


@pytest.mark.parametrize("row,layout", ROW_LAYOUTS, ids=ROW_LAYOUT_IDS)
def test_potrf_layout_emulated(row, layout):
    """Every row x layout through fake_ops.potrf_ on CPU tensors in that layout, under checks 1 - 3 and 5 of the device tier."""
    got = _checked("fake_ops", fake_ops, "cpu", row, layout)
    if layout == "c":
        _fake_c[row] = got
    elif layout in ALIGNED:
        if row not in _fake_c:
            _fake_c[row] = _np(_factor(fake_ops, "cpu", row, "c")[0])
        assert _same_bits(got, _fake_c[row]), f"fake_ops: {layout} differs from c"


# ------------------------------------------------------------------------------------------------ GPU tier
_dev_c = {}         # row -> result in layout c
_dev_digest = {}    # (row, layout) -> digest of the result
_dev_kinds = {}     # (row, layout) -> GEMM launches per kind of one factorisation


def _c_result(row):
    from gpflow_amd import ops
    if row not in _dev_c:
        _dev_c[row] = _np(_factor(ops, "cuda", row, "c")[0])
    return _dev_c[row]


def _profiled(row, layout):
    """check 7: one factorisation with the GEMM profiling facility on (a call of its own: the profiler puts event records between the
    chain's kernels); returns (launches per kind, result, status)"""
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    tT, buf = _on(_ref(row).input(row), layout, "cuda", base=True)
    torch.cuda.synchronize()
    lib.gpk_profile_gemm_enable(1)
    try:
        _, info = ops.potrf_(tT, row.n, zero_upper=row.zero_upper, identity_rows=row.identity)
        torch.cuda.synchronize()
        kinds = {}
        for kind in range(1, 7):
            ms, cnt, fl = C.c_double(), C.c_long(), C.c_double()
            assert lib.gpk_profile_gemm_collect_kind(kind, 0.0, C.byref(ms), C.byref(cnt), C.byref(fl)) == 0
            kinds[kind] = cnt.value
    finally:
        lib.gpk_profile_gemm_enable(0)
        lib.gpk_profile_gemm_collect(None, None, None)   # drops the records
    return kinds, tT, buf, info


@pytest.mark.gpu
@pytest.mark.parametrize("row,layout", ROW_LAYOUTS, ids=ROW_LAYOUT_IDS)
def test_potrf_layout(gpu, row, layout):
    from gpflow_amd import ops
    who = f"device {row.id} {layout}"
    got = _checked(who, ops, "cuda", row, layout)                               # checks 1 - 3
    tT2, _, _ = _factor(ops, "cuda", row, layout)
    assert _same_bits(_np(tT2), got), f"potrf {who}: a second call differs"     # check 4
    _dev_digest[(row, layout)] = hashlib.sha1(np.ascontiguousarray(got).tobytes()).hexdigest()
    if layout == "c":
        _dev_c[row] = got
    elif layout in ALIGNED:
        # check 5.  The plan depends on the shape only and every operand predicate (parity of lda and of the batch stride, alignment of
        # every block address) has the same value as in c: the same kernels on the same grids with the same arithmetic.  A difference
        # means that an address computation uses n where it means lda (or rows * n where it means the batch stride).
        same = _same_bits(got, _c_result(row))
        print(f"  {who}: bitwise equal to c: {same}")
        if not same:
            d = np.argwhere(_bits(got) != _bits(_c_result(row)))
            raise AssertionError(f"potrf {who}: {len(d)} entries differ from layout c, first at {tuple(d[0])}, last at {tuple(d[-1])}")
    else:
        # check 6 (reported, not asserted): do the unaligned layouts agree with each other, and with c?
        mine = _dev_digest[(row, layout)]
        for other in UNALIGNED:
            if other != layout and (row, other) in _dev_digest:
                print(f"  {who}: bitwise equal to {other}: {_dev_digest[(row, other)] == mine}")
        if (row, "c") in _dev_digest:
            print(f"  {who}: bitwise equal to c: {_dev_digest[(row, 'c')] == mine}")
    # check 7: which GEMM kernels ran
    kinds, tTp, bufp, infop = _profiled(row, layout)
    _dev_kinds[(row, layout)] = kinds
    print(f"  {who}: GEMM launches per kind {kinds}")
    _check_info(who + " (profiled call)", infop)
    _check_values(who + " (profiled call)", row, _np(tTp))
    assert _padding_untouched(tTp, bufp), f"potrf {who} (profiled call): written outside the view"
    if layout in UNALIGNED:
        # gemm_small_ok, gemm_fast_ok and gemm_pre64_ok all require 16-byte aligned rows of both operands in every batch entry
        # (gemm_rows_16b), and every product of the factorisation has a block of A as an operand: the generic kernel is what is left
        assert all(kinds[k] == 0 for k in range(1, 6)) and kinds[6] > 0, (who, kinds)
    else:
        if (row, "c") not in _dev_kinds:
            _dev_kinds[(row, "c")] = _profiled(row, "c")[0]
        assert kinds[1] > 0 and kinds == _dev_kinds[(row, "c")], (who, kinds, _dev_kinds[(row, "c")])


# ------------------------------------------------------------------------------------------------ solves with the FACTOR in a layout
# (n, rows): 4 blocks, fused on the staged kernel;  the pipelined kernel, rows not a multiple of 32;  a 4 + 1 split, second group unfused
SOLVE_SHAPES = [(512, 1024), (384, 4128), (640, 1040)]
SOLVE_L_LAYOUTS = ["c", "pad", "ld", "off"]     # pad: fused with ldl != n;  ld / off: the per-block loop at >= 1024 rows
SOLVE_B_LAYOUTS = ["c", "ld", "off"]
SOLVE_CASES_L = [(n, rows, lay) for n, rows in SOLVE_SHAPES for lay in SOLVE_L_LAYOUTS]


@functools.lru_cache(maxsize=None)
def _solve_ref(n, rows):
    K, B = _spd(np.random.default_rng(n + rows), n, rows)
    L = np.linalg.cholesky(K)
    Lp = L.copy()
    Lp[np.triu_indices(n, 1)] = NAN      # never read
    return L, Lp, B


_invd_c = {}    # (who, n, rows) -> block inverses of the contiguous factor


def _solves_in_layout(who, impl, dev, n, rows, lay):
    """trtri_blocks -> trsm_(trans 0): B L^-T;  transpose_factor -> trsm_(trans 1): B L^-1, the factor (for trans 1: the LT that
    transpose_factor returns, copied) in layout `lay`, B in every layout of SOLVE_B_LAYOUTS.  test_solves_contract's bound,
    |B - X L^T|_F <= 4 (n + 1) u |X|_F |L|_F, residual in float64."""
    L, Lp, B = _solve_ref(n, rows)
    tL, bufL = _on(Lp, lay, dev, base=True)
    invd = impl.trtri_blocks(tL)
    if (who, n, rows) not in _invd_c:
        _invd_c[(who, n, rows)] = _np(impl.trtri_blocks(_on(Lp, "c", dev)))
    # the leaf's vector and scalar loads feed the same arithmetic
    assert _same_bits(_np(invd), _invd_c[(who, n, rows)]), f"trtri_blocks {who}: L in layout {lay} differs from contiguous L"
    LT, invdT = impl.transpose_factor(tL, invd)
    assert _same_bits(_np(LT), L.T), f"transpose_factor {who}: L in layout {lay}"
    tLT, bufLT = _on(_np(LT), lay, dev, base=True)
    for layB in SOLVE_B_LAYOUTS:
        for trans in (0, 1):
            tB, bufB = _on(B, layB, dev, base=True)
            impl.trsm_(tB, tL if trans == 0 else tLT, invd if trans == 0 else invdT, trans=trans)
            X = _np(tB)
            assert np.all(np.isfinite(X)), (who, lay, layB, trans)
            r = np.linalg.norm(B - (X @ L.T if trans == 0 else X @ L))
            bound = 4 * (n + 1) * U * np.linalg.norm(X) * np.linalg.norm(L)
            print(f"  trsm_ {who} L {lay} B {layB} trans {trans}: residual / bound = {r / bound:.3e}")
            assert r <= bound, (who, lay, layB, trans, r, bound)
            assert _padding_untouched(tB, bufB), f"trsm_ {who}: written outside B (L {lay}, B {layB}, trans {trans})"
    assert _same_bits(_np(tL), Lp) and _padding_untouched(tL, bufL), f"solves {who}: L (layout {lay}) or its padding was modified"
    assert _same_bits(_np(tLT), L.T) and _padding_untouched(tLT, bufLT), f"solves {who}: LT (layout {lay}) or its padding was modified"


@pytest.mark.parametrize("n,rows,lay", SOLVE_CASES_L)
def test_solves_factor_layout_emulated(n, rows, lay):
    _solves_in_layout("fake_ops", fake_ops, "cpu", n, rows, lay)


@pytest.mark.gpu
@pytest.mark.parametrize("n,rows,lay", SOLVE_CASES_L)
def test_solves_factor_layout(gpu, n, rows, lay):
    from gpflow_amd import ops
    _solves_in_layout("device", ops, "cuda", n, rows, lay)


# ------------------------------------------------------------------------------------------------ the invd contract
@pytest.mark.gpu
def test_misaligned_invd_is_refused(gpu):
    """include/gpk.h: invd is 16-byte aligned (the leaf stores the block inverses 16 bytes at a time).  One that is not is refused with
    GPK_E_ARG by the five entry points that take one, on the host, before anything is launched: the operands here are never written
    (NaN in, the same NaN out) and nothing is ever run with such a buffer."""
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    n, rows = 256, 8
    T = torch.full((n + rows, n), NAN, dtype=torch.float64, device="cuda")
    Tinv = torch.full((2 * n + rows, n), NAN, dtype=torch.float64, device="cuda")
    LT = torch.full((n, n), NAN, dtype=torch.float64, device="cuda")
    whole = torch.full((int(lib.gpk_invd_elems(n, 1)) + 1,), NAN, dtype=torch.float64, device="cuda")
    good, bad = whole[:-1], whole[1:]
    assert good.data_ptr() % 16 == 0 and bad.data_ptr() % 16 == 8
    other = torch.full_like(good, NAN)
    info = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    E_ARG = -1
    with pytest.raises(_lib.GpkError):
        ops.potrf_(T, n, invd=bad)
    with pytest.raises(_lib.GpkError):
        ops.potrf_(Tinv, n, invd=bad, identity_rows=True)
    with pytest.raises(_lib.GpkError):
        ops.trsm_(T[n:], T[:n], bad, trans=0)
    with pytest.raises(_lib.GpkError):
        ops.transpose_factor(T[:n], bad)
    assert lib.gpk_potrf(s, T.data_ptr(), n, rows, n, 1, 0, bad.data_ptr(), 0, info.data_ptr()) == E_ARG
    assert lib.gpk_potrf_inv(s, Tinv.data_ptr(), n, rows, n, bad.data_ptr(), 0, info.data_ptr()) == E_ARG
    assert lib.gpk_trtri_blocks(s, T.data_ptr(), n, n, 1, 0, bad.data_ptr()) == E_ARG
    for trans in (0, 1):
        assert lib.gpk_trsm(s, trans, T.data_ptr(), n, bad.data_ptr(), n, T[n:].data_ptr(), rows, n, 1, 0, 0) == E_ARG
    assert lib.gpk_transpose_factor(s, T.data_ptr(), n, bad.data_ptr(), n, LT.data_ptr(), n, other.data_ptr()) == E_ARG
    assert lib.gpk_transpose_factor(s, T.data_ptr(), n, other.data_ptr(), n, LT.data_ptr(), n, bad.data_ptr()) == E_ARG
    torch.cuda.synchronize()
    for t in (T, Tinv, LT, whole, other):
        assert np.all(_bits(_np(t)) == _bits(np.array([NAN]))[0]), "a refused call wrote to an operand"
    assert int(info.cpu()[0]) == 77, "a refused call wrote the status word"
