"""The workspace contract of include/gpk.h (Conventions, "workspace"), held on the device for every entry point that takes a caller's
workspace: (a) its contents at entry do not matter, (b) nothing outside the first *_workspace_bytes bytes is touched, (c) a null or
short workspace is refused with GPK_E_WORKSPACE and nothing written, (d) a base that is not 16-byte aligned is refused with GPK_E_ARG.

How a row is run.  WS_ROWS names, per row, the EXISTING test of that entry point and the arguments it is called with here.  The base run
calls that test function as it stands -- its inputs, its reference and its tolerance -- with `ops._ws` swapped (pytest's monkeypatch)
for an allocator that carves the workspace, zero-filled, out of the middle of a larger allocation.  Every device call the test makes is
recorded with its operands and the bits of its results.  The poisoned runs replay those recorded calls on the same operand tensors, so
the reference is computed once per row, and compare the results with the base run bit for bit.  The only floating-point tolerance in
this file is therefore the one the named test applies (cited in the row's `tol`; gpk_svgp_elbo_shard_lik has no test that takes a
shape, so _lik_shard_against_oracle below runs the problem, the oracle and the two tolerances of its model-level tests); bit-identity
needs none: the library has no floating-point atomics and fixed summation orders, which tests/test_gpu_contract.py asserts call by call.

Observed on an MI355X: all 85 rows pass as the library stands (no fix was needed), and the six alignment rows are bitwise their
256-byte-aligned runs.  A scratch build with kl_white_kernel's `*zero_word = 0` removed and elbo_layout asking for 256 bytes less failed
37 of the 46 shard and likelihood tests it was run on: the whitened Gaussian rows by their bits under 0xFF, the un-whitened ones by the guard zone behind the workspace.

What the library keeps in a caller's workspace between the launches of one call, from reading drivers.hip, varexp.hip, reduce.hip,
gemm.hip (epilogue 1) and potrf.hip, and which launch OF THE SAME CALL writes each before it is read:

  word / slots                         where                                   written by                          read by
  -----------------------------------  --------------------------------------  ----------------------------------  ----------------------------
  tail_ticket (int32), the only        ElboWs.part2 + MAXPART + 32 doubles;    kl_white_kernel, thread 0 of block  varexp_kernel<true>:
  integer word in a workspace          whitened Gaussian shards only           0 (`*zero_word = 0`), on the         atomicAdd, compared with
                                                                               caller's stream, or as late_work    gridDim.x - 1.  Never an index
                                                                               on the rest-update stream, which    or a loop bound: a stale value
                                                                               gpk_potrf_core joins before it      leaves out[0] unwritten, it
                                                                               returns                             cannot fault
  part0 [nb] block partials            ElboWs.part0                            varexp_kernel<false|true>, the      final_sum_kernel (count = nb),
                                                                               quadrature and the mixed stage:     or the last block of
                                                                               every block writes part[blockIdx]   varexp_kernel<true> (gridDim.x)
  part1 [nb]                           ElboWs.part1                            kl_white_kernel (whitened);         final_sum_kernel
                                                                               sumsq_kernel over a^T (un-whitened)
  part2 [nb], then [P] log det q and   ElboWs.part2, un-whitened forms only    sumsq_kernel / kl_unwhite_diag_     final_sum_kernel (4 or 3 terms,
  [1] log det Lm at part2 + MAXPART                                            kernel; sum_log_diag_sq_kernel,     counts nb, P, 1)
                                                                               sum_log_diag_kernel
  slot partials [P][2 ceil(m/128)]     ElboWs.proj; the whole workspace of     GEMM epilogue 1: every tile writes  sum_parts_kernel or
  [rows]                               gpk_project*                            all BN / 64 slots of its rows, and  varexp_kernel<true>, nt slots
                                                                               make_gemm_plan takes 64-wide tiles  per row
                                                                               only where they cover the same
                                                                               slots as the 128-wide ones
  part [nb], part1 [nb] of the         ws, ws + MAXPART doubles                the stage-1 kernel of the entry     final_sum_kernel
  reductions (gaussian_, likelihood_,                                          point
  gauss_kl_white, sumsq, gpr_lml)
  dW block partials [nb][P L]          ws + 2 MAXPART doubles (mixed stage)    mixed_varexp_kernel: every block    combine_parts_kernel, nb parts
                                                                               writes all P L entries
  logdet [1]                           LmlWs.logdet                            sum_log_diag_kernel                 final_sum_kernel

  The trapezoids (T, Kfu, arow, LqT), invd, s0, fmean, ssq and V are matrices and vectors that a builder, a transpose or a solve of
  the call writes before the first read.  Never written and not to be read: the padding columns [m, align_up(m, 8)) of every
  trapezoid row, the padding rows up to align_up(rows, 32) and the 32 spare rows behind the tail, the upper tiles of a lower-only
  Kuu, and the part of part2 between the last single term and the ticket.
  The reading found no word used as an index or loop bound and no read of a slot that its own call does not write.  The hand-off
  words and the status word `info` are not in the workspace (the library's own 4 KB allocation, the caller's `info`) and are never
  poisoned here.

Per row (test_workspace_row): the base run; the workspace filled with 0xFF bytes (doubles NaN, int words -1) and with 0x7F bytes
(doubles 1.4e306, finite: a clamp or comparison that swallows NaN would hide a read that this exposes; int words 2139062143); the
workspace as a call of ANOTHER row of the same entry point left it (the opposite whiten form where the entry point has one, the next
larger workspace otherwise); three calls in a row on one poisoned workspace; guard zones of 4 KB on either side of the workspace
bitwise intact after every run; the operands bitwise unchanged; the refusals, replayed on the C ABI with the recorded arguments.
test_workspace_alignment: a base that is 16 mod 256.
"""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GUARD = 4096        # bytes of guard zone on either side of a workspace
SENTINEL = 0xA5     # every guard byte
GPK_E_ARG, GPK_E_WORKSPACE = -1, -2

Row = collections.namedtuple("Row", "id entry ops_fn test args size tol m whiten")
# entry: the C entry point;  ops_fn: the gpflow_amd.ops function whose device calls are recorded;  test: (module, function) of the
# existing test that is the base run, called with the `gpu` / `gp` fixture value and `args`;  size: (symbol, arguments) of the
# *_workspace_bytes call that sizes the FIRST recorded call;  tol: where that test's tolerance is written;  m: the M of the row where
# the entry point has one;  whiten: the form, where the entry point has forms


def _shard_rows():
    rows = []
    # (M, rows): one leaf block, no side schedule, M % 8 = 4, rows % 32 != 0 | two leaf blocks, the extra rows ride through the panels,
    # M % 8 = 2 | side schedule (late work on the rest-update stream), a fused group solve, M % 8 = 4, rows % 32 = 13 | no rows: [0, KL]
    shapes = [(100, 300), (130, 40), (300, 333), (130, 0)]
    d = 8
    for (M, n), P, whiten, q_diag in [(s, P, w, q) for s in shapes for P in (1, 3) for w in (1, 0) for q in (0, 1)]:
        # (P = 1 un-whitened with a full q_sqrt takes the `skip` branch of gpk_potrf_core: tri_prefilled)
        rows.append(Row("shard-M%d-n%d-P%d-%s-%s" % (M, n, P, "white" if whiten else "unwhite", "qdiag" if q_diag else "full"),
                        "gpk_svgp_elbo_shard", "svgp_elbo_shard", ("test_gpu_contract", "test_svgp_elbo_shard_contract"),
                        ((M, n, d, P, bool(q_diag), bool(whiten), "c"),), ("gpk_svgp_elbo_workspace_bytes", (M, n, d, P, q_diag, whiten)),
                        "tests/test_gpu_contract.py:1017-1021 (_fused_bound against the emulation, the KL's reduction bound)", M, whiten))
    for lik, (M, n, q_diag), whiten in [(l, s, w) for l in ("student_t", "multiclass_robustmax") for s in ((300, 333, 0), (130, 40, 1))
                                        for w in (1, 0)]:
        rows.append(Row("lik-%s-M%d-n%d-%s-%s" % (lik, M, n, "white" if whiten else "unwhite", "qdiag" if q_diag else "full"),
                        "gpk_svgp_elbo_shard_lik", "svgp_elbo_shard_lik", ("test_gpu_workspace", "_lik_shard_against_oracle"),
                        (lik, M, n, 3, bool(q_diag), bool(whiten)), ("gpk_svgp_elbo_workspace_bytes", (M, n, 8, 3, q_diag, whiten)),
                        "tests/test_gpu_likelihoods.py:441,446 and tests/test_gpu_multiclass.py:439,443 (1e-8 of the ELBO, 1e-9 of the KL)",
                        M, whiten))
    for (M, n), P in [(s, P) for s in shapes for P in (2, 3)]:
        rows.append(Row("sep-M%d-n%d-P%d" % (M, n, P), "gpk_svgp_elbo_shard_sep", "svgp_elbo_shard_sep",
                        ("test_gpu_contract", "test_svgp_elbo_shard_sep_contract"), (M, n, P, "c"),
                        ("gpk_svgp_elbo_sep_workspace_bytes", (M, n, 2, P)), "tests/test_gpu_contract.py:1051-1053", M, None))
    for (M, n), (L, P) in [(s, lp) for s in shapes for lp in ((2, 3), (3, 2))]:
        rows.append(Row("lcm-M%d-n%d-L%d-P%d" % (M, n, L, P), "gpk_svgp_elbo_shard_lcm", "svgp_elbo_shard_lcm",
                        ("test_gpu_lcm", "test_svgp_elbo_shard_lcm_contract"), ((M, n, L, P, "c", False, False),),
                        ("gpk_svgp_elbo_lcm_workspace_bytes", (M, n, 8 if M >= 200 else 2, L, P)), "tests/test_gpu_lcm.py:324-326", M, None))
    # n = 1: one element; 130: two leaf blocks, n % 8 = 2; 300: the factorisation's own streams, n % 8 = 4; one heteroskedastic row
    for n, P, family, het in [(1, 1, "SquaredExponential", False), (1, 3, "Matern12", False), (130, 1, "Matern52", False),
                              (130, 3, "Matern32", True), (130, 3, "SquaredExponential", False), (300, 1, "Matern32", False),
                              (300, 3, "Matern52", False)]:
        rows.append(Row("gpr-n%d-P%d-%s%s" % (n, P, family, "-het" if het else ""), "gpk_gpr_lml", "gpr_lml",
                        ("test_gpu_contract", "test_gpr_lml_contract"), (n, P, family, het), ("gpk_gpr_lml_workspace_bytes", (n, 2, P)),
                        "tests/test_gpu_contract.py:1076-1082 (backward-error bound against the fp64 reference)", n, None))
    return rows


def _primitive_rows():
    """At most three cases of each primitive's own table: the empty one, the smallest, the first whose launcher reports more than one
    stage-1 partial; plus, for the two projections whose tables hold no m % 8 != 0, one shape of that kind run through the same test."""
    red = "gpk_reduce_workspace_bytes"
    proj, projtol = ("test_gpu_contract", "test_project_contract"), "tests/test_gpu_contract.py:899-914"
    stats, statstol = ("test_gpu_step_tail", "test_fused_statistics_against_numpy"), "tests/test_gpu_step_tail.py:10-16,62-67"

    def P(id, entry, fn, test, args, size, tol, m=None):
        return Row(id, entry, fn, test, args, size, tol, m, None)
    return [
        # gpk_project (ops.project always enters through gpk_project_batched; these rows forward its stride-0 calls to gpk_project)
        P("project-empty", "gpk_project", "project", proj, ((0, 16, 1, False, "c"),), ("gpk_project_workspace_bytes", (0, 16, 1)), projtol, 16),
        P("project-one-row", "gpk_project", "project", proj, ((1, 16, 1, False, "c"),), ("gpk_project_workspace_bytes", (1, 16, 1)), projtol, 16),
        # m = 129: nt = 2 ceil(129 / 128) = 4 slot partials per row, on the 64 x 128 few-rows tile (gemm_plan.h: 64-wide tiles would
        # leave the fourth slot unwritten)
        P("project-four-slots", "gpk_project", "project", proj, ((300, 129, 2, False, "ld"),), ("gpk_project_workspace_bytes", (300, 129, 2)),
          projtol, 129),
        P("project-batched", "gpk_project_batched", "project", proj, ((65, 64, 3, True, "c"),), ("gpk_project_workspace_bytes", (65, 64, 3)),
          projtol, 64),
        P("project-batched-m100", "gpk_project_batched", "project", proj, ((40, 100, 3, True, "c"),),   # (not in PROJECT_CASES: m % 8 = 4)
          ("gpk_project_workspace_bytes", (40, 100, 3)), projtol, 100),
        # gpk_project_stats: (64, 128, 1) the statistics out of the GEMM, nt = 2; (130, 80, 3) gpk_row_stats in front, small tiles
        P("project-stats-in-gemm", "gpk_project_stats", "project_stats", stats, (64, 128, 1), ("gpk_project_workspace_bytes", (64, 128, 1)),
          statstol, 128),
        P("project-stats-row-stats", "gpk_project_stats", "project_stats", stats, (130, 80, 3), ("gpk_project_workspace_bytes", (130, 80, 3)),
          statstol, 80),
        P("project-stats-m100", "gpk_project_stats", "project_stats", stats, (300, 100, 3),   # (not in ISSUE_SHAPES: m % 8 = 4)
          ("gpk_project_workspace_bytes", (300, 100, 3)), statstol, 100),
        # gpk_gaussian_varexp_sum: nblocks_for (reduce_device.h) gives one block of RB = 256 threads per 256 elements: 255 x 4 -> 4
        P("varexp-empty", "gpk_gaussian_varexp_sum", "gaussian_varexp_sum", ("test_gpu_contract", "test_gaussian_varexp_sum_contract"),
          ((0, 1, False, False, "c"),), (red, (0,)), "tests/test_gpu_contract.py:781-789"),
        P("varexp-one", "gpk_gaussian_varexp_sum", "gaussian_varexp_sum", ("test_gpu_contract", "test_gaussian_varexp_sum_contract"),
          ((1, 1, False, False, "c"),), (red, (1,)), "tests/test_gpu_contract.py:781-789"),
        P("varexp-four-blocks", "gpk_gaussian_varexp_sum", "gaussian_varexp_sum", ("test_gpu_contract", "test_gaussian_varexp_sum_contract"),
          ((255, 4, True, False, "ld"),), (red, (255,)), "tests/test_gpu_contract.py:781-789"),
        # gpk_likelihood_varexp_sum: a block is RB / 64 = 4 wave passes of quad_rows_per_pass rows; 67 rows x 4 latents: 17 passes, 5 blocks
        P("lik-varexp-empty", "gpk_likelihood_varexp_sum", "likelihood_varexp_sum", ("test_gpu_likelihoods", "test_likelihood_varexp_sum_contract"),
          ("student_t", (0.8, 3.0), (0, 1, False, "c")), (red, (0,)), "tests/test_gpu_likelihoods.py:224-233"),
        P("lik-varexp-one", "gpk_likelihood_varexp_sum", "likelihood_varexp_sum", ("test_gpu_likelihoods", "test_likelihood_varexp_sum_contract"),
          ("student_t", (0.8, 3.0), (1, 1, False, "c")), (red, (1,)), "tests/test_gpu_likelihoods.py:224-233"),
        P("lik-varexp-five-blocks", "gpk_likelihood_varexp_sum", "likelihood_varexp_sum",
          ("test_gpu_likelihoods", "test_likelihood_varexp_sum_contract"), ("student_t", (0.8, 3.0), (67, 4, True, "ld")), (red, (67,)),
          "tests/test_gpu_likelihoods.py:224-233"),
        # gpk_mixed_gaussian_varexp_sum: mixed_blocks (varexp.hip): 4 wave passes of 64 / max(L, P) rows per block; 67 rows, L 3, P 5:
        # 12 rows per pass, 6 passes, 2 blocks -- two [P L] partials of dW
        P("mixed-empty", "gpk_mixed_gaussian_varexp_sum", "mixed_gaussian_varexp_sum", ("test_gpu_lcm", "test_mixed_gaussian_varexp_sum_contract"),
          ((0, 2, 3, "per", True, True, "c"),), ("gpk_mixed_varexp_workspace_bytes", (0, 2, 3)), "tests/test_gpu_lcm.py:156-161"),
        P("mixed-one", "gpk_mixed_gaussian_varexp_sum", "mixed_gaussian_varexp_sum", ("test_gpu_lcm", "test_mixed_gaussian_varexp_sum_contract"),
          ((1, 1, 1, "shared", True, False, "c"),), ("gpk_mixed_varexp_workspace_bytes", (1, 1, 1)), "tests/test_gpu_lcm.py:156-161"),
        P("mixed-two-blocks", "gpk_mixed_gaussian_varexp_sum", "mixed_gaussian_varexp_sum",
          ("test_gpu_lcm", "test_mixed_gaussian_varexp_sum_contract"), ((67, 3, 5, "shared", True, True, "ld"),),
          ("gpk_mixed_varexp_workspace_bytes", (67, 3, 5)), "tests/test_gpu_lcm.py:156-161"),
        # gpk_gauss_kl_white (m > 0: no empty case): nblocks_for(P m m) = 261 blocks at (129, 4)
        P("kl-one", "gpk_gauss_kl_white", "gauss_kl_white", ("test_gpu_contract", "test_gauss_kl_white_contract"), (1, 1, False), (red, (1,)),
          "tests/test_gpu_contract.py:829", 1),
        P("kl-261-blocks", "gpk_gauss_kl_white", "gauss_kl_white", ("test_gpu_contract", "test_gauss_kl_white_contract"), (129, 4, False),
          (red, (129,)), "tests/test_gpu_contract.py:829", 129),
        # gpk_sumsq: gpk_launch_sumsq_stage1 gives one block per row, at most MAXPART: 255 partials
        P("sumsq-empty", "gpk_sumsq", "sumsq", ("test_gpu_contract", "test_sumsq_contract"), ((0, 4, False, "c"),), (red, (0,)),
          "tests/test_gpu_contract.py:724"),
        P("sumsq-one", "gpk_sumsq", "sumsq", ("test_gpu_contract", "test_sumsq_contract"), ((1, 1, True, "c"),), (red, (1,)),
          "tests/test_gpu_contract.py:724"),
        P("sumsq-255-blocks", "gpk_sumsq", "sumsq", ("test_gpu_contract", "test_sumsq_contract"), ((255, 257, True, "ld"),), (red, (255,)),
          "tests/test_gpu_contract.py:724"),
    ]


WS_ROWS = _shard_rows() + _primitive_rows()
ROW_BY_ID = {r.id: r for r in WS_ROWS}
HAS_M = ("gpk_project", "gpk_project_batched", "gpk_project_stats", "gpk_gauss_kl_white", "gpk_gpr_lml", "gpk_svgp_elbo_shard",
         "gpk_svgp_elbo_shard_lik", "gpk_svgp_elbo_shard_sep", "gpk_svgp_elbo_shard_lcm")   # entry points with a matrix dimension M (or n)


# ------------------------------------------------------------------------------------------------ CPU tier: the table is complete
def _workspace_entry_points():
    from gpflow_amd import _lib
    return sorted(name for name, (_, args) in _lib._SIGS.items() if args[-2:] == [_lib.c_void_p, _lib.c_size_t])


def test_every_workspace_entry_point_has_rows():
    """A fourteenth entry point that takes (void* ws, size_t ws_bytes) fails here until WS_ROWS has a row for it."""
    from gpflow_amd import _lib
    names = _workspace_entry_points()
    assert len(names) >= 13 and "gpk_svgp_elbo_shard_lcm" in names and "gpk_sumsq" in names, names
    covered = {r.entry for r in WS_ROWS}
    assert covered == set(names), (sorted(set(names) - covered), sorted(covered - set(names)))
    sizes = sorted(name for name in _lib._SIGS if name.endswith("_workspace_bytes"))
    assert sorted({r.size[0] for r in WS_ROWS}) == sizes, sizes
    assert len(ROW_BY_ID) == len(WS_ROWS), "row ids must be unique"


def test_every_entry_point_with_an_m_has_a_padded_row():
    """where the entry point has an M, some row has M % 8 != 0 (padding columns in the trapezoid: ld = align_up(M, 8)); the fused
    drivers: EVERY row with a factorisation larger than one element"""
    for entry in HAS_M:
        ms = [r.m for r in WS_ROWS if r.entry == entry]
        assert ms and all(m is not None for m in ms), entry
        assert any(m % 8 for m in ms), (entry, ms)
    for r in WS_ROWS:
        if r.entry.startswith("gpk_svgp") or (r.entry == "gpk_gpr_lml" and r.m > 1):
            assert r.m % 8, r.id
    assert {r.entry for r in WS_ROWS if r.m is not None} == set(HAS_M)


def test_size_functions_answer_without_a_device():
    """every row's size query answers (the library loads without a device), is a multiple of 8, and a partner exists for every row"""
    from gpflow_amd import _lib
    lib = _lib.load()
    for r in WS_ROWS:
        n = int(getattr(lib, r.size[0])(*r.size[1]))
        assert n % 8 == 0 and n >= 0, (r.id, n)
        assert _partner(r, lib).id != r.id


# ------------------------------------------------------------------------------------------------ the base run of the two _lik rows
def _lik_shard_against_oracle(gp, lik, M, rows, P, q_diag, whiten):
    """gpk_svgp_elbo_shard_lik at the shapes of this file: the problem and the reference of tests/test_gpu_likelihoods.py
    (_svgp_problem, _oracle_terms) and tests/test_gpu_multiclass.py (_mc_problem, _mc_oracle_terms) with the input dimension and
    lengthscale of their at-size tests (D = 8, sqrt(D)), and their tolerances: 1e-8 of the ELBO, 1e-9 of the KL."""
    import test_gpu_likelihoods as TL
    import test_gpu_multiclass as TM
    from oracle import gp_oracle as orc
    ops = gp.ops
    D, N, ls = 8, max(M, rows), float(np.sqrt(8))
    if lik == "multiclass_robustmax":
        par = (TM.EPS,)
        X, Y, Z, q_mu, q_sqrt = TM._mc_problem(M, N, D, P, 21, q_diag, whiten, ls=ls)
        X, Y = X[:rows], Y[:rows]
        ve, kl = TM._mc_oracle_terms(X, Y, Z, q_mu, q_sqrt, whiten=whiten, ls=ls, erfc=TL._erfc_f64)
    else:
        par = dict(TL.LIKS)[lik]
        X, Y, Z, q_mu, q_sqrt = TL._svgp_problem(lik, M, N, D, P, 21, q_diag, whiten, ls=ls)
        X, Y = X[:rows], Y[:rows]
        ve, kl = TL._oracle_terms(lik, par, X, Y, Z, q_mu, q_sqrt, whiten=whiten, ls=ls, erfc=TL._erfc_f64)
    t = ops.to_device
    out, info = ops.svgp_elbo_shard_lik(t(Z), t(X), t(Y), t(q_mu), t(q_sqrt), variance=1.3, lengthscales=ls, lik=lik, params=par,
                                        jitter=orc.DEFAULT_JITTER, mean_const=0.2, whiten=whiten)
    o = out.cpu().numpy()
    assert int(info.cpu().numpy()[0]) == 0
    print("lik shard", lik, M, rows, "device", o, "oracle", (ve, kl), "rel err", abs(o[0] - o[1] - (ve - kl)) / abs(ve - kl), abs(o[1] - kl) / abs(kl))
    assert abs(o[0] - o[1] - (ve - kl)) <= 1e-8 * abs(ve - kl)
    assert abs(o[1] - kl) <= 1e-9 * abs(kl)


# ------------------------------------------------------------------------------------------------ the allocator behind ops._ws
class Workspaces:
    """Stands in for ops._ws.  Every workspace is a view of `length` bytes -- the request rounded up to 8, as ops._ws sizes it -- whose
    base is 256-byte aligned (+ `offset`), carved from the middle of a larger allocation with GUARD bytes of SENTINEL on either side.
    fill: the byte every workspace byte is set to before it is handed out; None: the bytes stay as the previous call on `arena` left
    them (all workspaces then start at the same address of one arena)."""

    def __init__(self, device):
        self.device, self.fill, self.offset, self.arena = device, 0, 0, None
        self.handed, self.requests = [], []

    def use_arena(self, capacity, fill):
        import torch
        self.arena = torch.empty(GUARD + 512 + capacity + GUARD, dtype=torch.uint8, device=self.device)
        self.arena.fill_(fill)
        self.fill = None

    def fresh(self, fill, offset=0):
        self.arena, self.fill, self.offset = None, fill, offset

    def __call__(self, nbytes):
        import torch
        n = (int(nbytes) + 7) // 8 * 8
        length = max(n, 8)     # (ops._ws never hands out an empty tensor; with n = 0 those 8 bytes belong to the guard)
        buf = self.arena if self.arena is not None else torch.empty(GUARD + 512 + length + GUARD, dtype=torch.uint8, device=self.device)
        start = GUARD + (-(buf.data_ptr() + GUARD)) % 256 + self.offset
        assert start + n + GUARD <= buf.numel()
        buf[:start] = SENTINEL
        buf[start + n:] = SENTINEL
        if self.fill is not None and n:
            buf[start:start + n] = self.fill
        ws = buf[start:start + length].view(torch.float64)
        assert ws.data_ptr() % 256 == self.offset and ws.numel() * 8 == length
        self.handed.append((buf, start, n))
        self.requests.append(int(nbytes))
        return ws

    def check_guards(self, what):
        import torch
        torch.cuda.synchronize()
        assert self.handed, "%s: no workspace was asked for" % what
        for buf, start, n in self.handed:
            assert bool((buf[:start] == SENTINEL).all()), "%s: the guard zone in front of the workspace was written" % what
            assert bool((buf[start + n:] == SENTINEL).all()), "%s: the guard zone behind the %d workspace bytes was written" % (what, n)
        self.handed = []


def _tensors(x):
    import torch
    if isinstance(x, torch.Tensor):
        yield x
    elif isinstance(x, (list, tuple)):
        for y in x:
            yield from _tensors(y)
    elif isinstance(x, dict):
        for y in x.values():
            yield from _tensors(y)


def _snapshot(x):
    """the bytes of every tensor in x (results: out, info, the optional outputs; operands: every tensor argument), in order"""
    return [t.detach().cpu().contiguous().numpy().tobytes() for t in _tensors(x)]


Base = collections.namedtuple("Base", "calls need")   # calls: [(args, kwargs, result bytes, operand bytes)] of a base run
_BASES = {}   # (row id, offset of the workspace's base) -> Base: computed once, shared by the tests that need it, never modified
TAKES_GP = ("test_gpu_lcm", "test_gpu_likelihoods", "test_gpu_workspace")   # modules whose test bodies take the package, not the device


class Harness:
    """one test's patches (all through pytest's monkeypatch), the recorded base runs and their replays"""

    def __init__(self, monkeypatch, gp):
        from gpflow_amd import _lib
        self.gp, self.ops, self.lib = gp, gp.ops, _lib.load()
        self.real = {name: getattr(self.lib, name) for name in _workspace_entry_points()}   # (before anything is wrapped)
        self.alloc = Workspaces(gp.ops.device())
        self.mp = monkeypatch
        monkeypatch.setattr(gp.ops, "_ws", self.alloc)
        self.cargs = None

    def wrap_c(self, m, row):
        """the row's C function behind a wrapper that keeps the arguments of its last call"""
        real = self.real[row.entry]
        if row.entry == "gpk_project":   # ops.project always enters through gpk_project_batched: forward its stride-0 calls
            def forward(*a):
                if a[5] != 0:
                    raise AssertionError("a batched call in a gpk_project row")
                self.cargs = a[:5] + a[6:]
                return real(*self.cargs)
            m.setattr(self.lib, "gpk_project_batched", forward)
        else:
            def keep(*a):
                self.cargs = a
                return real(*a)
            m.setattr(self.lib, row.entry, keep)

    def base(self, row, offset=0):
        """The existing test of the entry point, as it stands, on a zero-filled workspace; every device call of ops.<ops_fn> it makes
        is recorded.  It asserts its own tolerance (and info == 0)."""
        if (row.id, offset) in _BASES:
            return _BASES[row.id, offset]
        import importlib
        fn = globals()[row.test[1]] if row.test[0] == "test_gpu_workspace" else getattr(importlib.import_module(row.test[0]), row.test[1])
        real_fn = getattr(self.ops, row.ops_fn)
        calls = []

        def recorder(*args, **kwargs):
            ret = real_fn(*args, **kwargs)
            if any(t.is_cuda for t in _tensors((args, kwargs))):
                calls.append([args, kwargs, _snapshot(ret), None])
            return ret
        self.alloc.fresh(0, offset)
        self.alloc.requests = []
        self.cargs = None
        with self.mp.context() as m:
            m.setattr(self.ops, row.ops_fn, recorder)
            self.wrap_c(m, row)
            fn(self.gp if row.test[0] in TAKES_GP else self.ops.device(), *row.args)
        self.alloc.check_guards(row.id + ", base run")
        assert calls and self.cargs is not None, "%s: the test made no device call of ops.%s into %s" % (row.id, row.ops_fn, row.entry)
        need = self.alloc.requests[0]
        assert need == int(getattr(self.lib, row.size[0])(*row.size[1])), (row.id, need, row.size)
        for c in calls:
            c[3] = _snapshot((c[0], c[1]))
        _BASES[row.id, offset] = Base(calls, need)
        return _BASES[row.id, offset]

    def replay(self, row, what, only_first=False):
        """the recorded calls of the row again, on whatever the allocator hands out now: results bitwise the base run's, guards intact,
        operands unchanged"""
        base = self.base(row)
        with self.mp.context() as m:
            self.wrap_c(m, row)
            for i, (args, kwargs, want, operands) in enumerate(base.calls[:1] if only_first else base.calls):
                got = _snapshot(getattr(self.ops, row.ops_fn)(*args, **kwargs))
                tag = "%s, %s, call %d" % (row.id, what, i)
                self.alloc.check_guards(tag)
                assert got == want, tag + ": the result differs from the run on a zero-filled workspace"
                assert _snapshot((args, kwargs)) == operands, tag + ": an operand was modified"


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _partner(row, lib):
    """the row whose leftovers this row runs on: another row of the same entry point -- of the opposite whiten form where there is
    one (part2 changes its role) -- with the next larger workspace, or the largest there is"""
    others = [r for r in WS_ROWS if r.entry == row.entry and r.id != row.id]
    if row.whiten is not None:
        others = [r for r in others if r.whiten != row.whiten]
    size = lambda r: int(getattr(lib, r.size[0])(*r.size[1]))   # noqa: E731
    larger = sorted((r for r in others if size(r) >= size(row)), key=lambda r: (size(r), r.id))
    return larger[0] if larger else max(others, key=lambda r: (size(r), r.id))


@pytest.mark.gpu
@pytest.mark.parametrize("row", WS_ROWS, ids=[r.id for r in WS_ROWS])
def test_workspace_row(gp, monkeypatch, row):
    import torch
    h = Harness(monkeypatch, gp)
    base = h.base(row)                                   # 1. zero-filled: the named test's own tolerance, info == 0
    for fill in (0xFF, 0x7F):                            # 2. poisoned; 4. guards and operands (in every replay)
        h.alloc.fresh(fill)
        h.replay(row, "workspace filled with 0x%02X" % fill)
    partner = _partner(row, h.lib)                       # 2. the leftovers of a different row
    pbase = h.base(partner)
    h.alloc.use_arena(max(base.need, pbase.need), 0xFF)
    h.replay(partner, "the partner's run on the arena", only_first=True)
    h.replay(row, "workspace as %s left it" % partner.id)
    h.alloc.use_arena(base.need, 0xFF)                   # 3. three calls in a row on one poisoned workspace
    for i in range(3):
        h.replay(row, "call %d of three on one workspace that started as 0xFF" % i, only_first=True)
    # 5. refusals, on the C ABI with the arguments of the first recorded call; nothing may be written: not the results (out, info and
    # the optional outputs), not the workspace or the guards around it
    h.alloc.fresh(0x7F)
    args, kwargs = base.calls[0][:2]
    with monkeypatch.context() as m:
        h.wrap_c(m, row)
        ret = getattr(h.ops, row.ops_fn)(*args, **kwargs)
    torch.cuda.synchronize()
    buf, start, n = h.alloc.handed[-1]
    cargs, need, real = h.cargs, base.need, h.real[row.entry]
    assert cargs[-1] == max(need, 8) and cargs[-2] == buf.data_ptr() + start
    for t in _tensors(ret):
        t.fill_(7)
    before = (_snapshot(ret), buf.cpu().numpy().tobytes())
    ptr = cargs[-2]
    refusals = [(None, need, GPK_E_WORKSPACE), (ptr + 8, need, GPK_E_ARG)]   # NULL; a base of 8 mod 16
    if need >= 8:
        refusals += [(ptr, need - 8, GPK_E_WORKSPACE), (ptr, 0, GPK_E_WORKSPACE)]
    for p, nbytes, code in refusals:
        rc = real(*(tuple(cargs[:-2]) + (p, nbytes)))
        torch.cuda.synchronize()
        tag = "%s: ws %s, ws_bytes %d of %d" % (row.id, "NULL" if p is None else "base + %d" % (p - ptr), nbytes, need)
        assert rc == code, "%s: returned %d, expected %d" % (tag, rc, code)
        assert (_snapshot(ret), buf.cpu().numpy().tobytes()) == before, tag + ": the refused call wrote something"


# 6. one row per driver (the shard in both roles of part2): a base that is 16-byte but not 256-byte aligned
ALIGNMENT_ROWS = ["shard-M300-n333-P3-white-full", "shard-M300-n333-P1-unwhite-full", "lik-student_t-M300-n333-white-full", "sep-M300-n333-P3",
                  "lcm-M300-n333-L2-P3", "gpr-n300-P3-Matern52"]


@pytest.mark.gpu
@pytest.mark.parametrize("rid", ALIGNMENT_ROWS)
def test_workspace_alignment(gp, monkeypatch, rid):
    """base = 16 mod 256: the named test runs as it stands (info == 0, its tolerance).  Whether the bits are those of the 256-byte-aligned
    run is printed, not asserted: the contract asks for 16 bytes and promises the same bits for the same base alignment only."""
    row = ROW_BY_ID[rid]
    h = Harness(monkeypatch, gp)
    aligned, shifted = h.base(row), h.base(row, offset=16)
    same = all(a[2] == b[2] for a, b in zip(aligned.calls, shifted.calls))
    print("%s: the run on a base of 16 mod 256 is %s the 256-byte-aligned run" % (rid, "bitwise" if same else "NOT bitwise"))
