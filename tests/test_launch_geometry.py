"""CPU-tier inventory of every kernel launch of gpflow_amd/csrc/*.hip and of what fixes its grid.

A launcher that clamps its grid leaves the rest to a gridDim-stride loop in the kernel; one that picks a template instantiation from
a count leaves the other counts to another body.  The second trip of such a loop, or the other instantiation, is the half of a branch
that a reference test at a small shape never runs.  LAUNCHES has one row per launch site:

  exact    one element, row, tile or problem per thread or block (or one block that loops inside itself): the kernel's body does not
           mention gridDim, so the grid is the whole geometry and the primitive's own case table covers it;
  strided  a clamp (or a count-selected instantiation) and a loop: every clamp names its value and GPU cases of a reference test on
           each side of it -- `near`: the loop's single trip / the instantiated count, `far`: a further, partial trip / the other body;
  planned  the grid is a plan computed on the host and pinned, field by field, by the owner the row names.

The guards are plain text scans: they read kernel names at launch sites, `__global__` definitions and the quoted expressions,
nothing else.  A new launch fails the first guard until it has a row; a kernel that starts to mention gridDim fails the second until
its row is strided and brings cases on both sides; a clamp that moves fails the third at the row to re-derive; a case that leaves its
table fails the fourth.
"""
import glob
import importlib
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gpflow_amd", "csrc")
sys.path.insert(0, HERE)

EXACT, STRIDED, PLANNED = "exact", "strided", "planned"


def exact(file, kernel, expr):
    return dict(file=file, kernel=kernel, kind=EXACT, exprs=[expr])


def planned(file, kernel, expr, owner, covers=()):
    return dict(file=file, kernel=kernel, kind=PLANNED, exprs=[expr], owner=owner, covers=tuple(covers))


def strided(file, kernel, *clamps, covers=()):
    return dict(file=file, kernel=kernel, kind=STRIDED, exprs=[c["expr"] for c in clamps], clamps=clamps, covers=tuple(covers))


def clamp(expr, value, near=(), far=(), uncovered=None):
    """expr: occurs literally in the row's file.  value: the clamp in words.  near / far: (test module, expression of its case table in
    that module -- or None: `case` is text of the module's source --, case).  uncovered: why a loop has no far side to test."""
    return dict(expr=expr, value=value, near=list(near), far=list(far), uncovered=uncovered)


C = "test_gpu_contract"
LAUNCHES = [
    # ---- reduce.hip
    exact("reduce.hip", "sum_parts_kernel", "dim3 grid((unsigned)gpk_cdiv(rows, 256), (unsigned)P);"),
    strided("reduce.hip", "combine_parts_kernel<NP>",
            clamp("(unsigned)(m < 65535 ? m : 65535)", "gridDim.y = min(m, 65535), rows strided",
                  near=[(C, "COMBINE_CASES", (5, 257, 300, 2.0, True, 1.0, "c"))],
                  far=[(C, "COMBINE_CASES", (2, 65537, 3, 1.0, False, 1.0, "c"))]),
            clamp("case 32: GPK_COMBINE(32); break;", "NP = nparts for 1, 2, 4, 8, 16, 32 (loads hoisted), else the run-time loop of NP = 0",
                  near=[(C, "COMBINE_CASES", (n, 130, 66, -0.5, False, 1.0, "c")) for n in (8, 16, 32)]
                  + [(C, "COMBINE_CASES", (n, 65, 63, 2.0, False, 1.0, "ld")) for n in (8, 16, 32)],
                  far=[(C, "COMBINE_CASES", (33, 130, 66, -0.5, False, 1.0, "c")), (C, "COMBINE_CASES", (33, 65, 63, 2.0, False, 1.0, "ld")),
                       (C, "COMBINE_CASES", (5, 257, 300, 2.0, True, 1.0, "c"))])),
    exact("reduce.hip", "final_sum_kernel", "hipLaunchKernelGGL(final_sum_kernel, dim3(1), dim3(RB)"),   # one block, loops inside itself
    strided("reduce.hip", "sumsq_kernel",
            clamp("rows < GPK_REDUCE_MAXPART ? rows : GPK_REDUCE_MAXPART", "min(rows, 1024) blocks, rows strided",
                  near=[(C, "SUMSQ_CASES", (255, 257, True, "ld"))], far=[(C, "SUMSQ_CASES", (1025, 64, False, "off"))])),
    strided("reduce.hip", "kl_white_kernel",
            clamp("const int nb = nblocks_for(elems);", "one block per 1024 elements (four trips), at most 1024 blocks (reduce_device.h)",
                  near=[(C, "KL_CASES", (129, 4, False))], far=[(C, "KL_CASES", (1100, 1, False))])),
    exact("reduce.hip", "sum_log_diag_kernel", "hipLaunchKernelGGL(sum_log_diag_kernel, dim3((unsigned)(batch > 0 ? batch : 1)), dim3(RB)"),
    strided("reduce.hip", "kl_unwhite_diag_kernel",
            clamp("m < GPK_REDUCE_MAXPART ? m : GPK_REDUCE_MAXPART", "min(M, 1024) blocks, inducing points strided, a block_sum per trip",
                  near=[(C, "SVGP_CASES", (1024, 64, 8, 2, True, False, "c"))], far=[(C, "SVGP_CASES", (1100, 64, 8, 2, True, False, "c"))])),
    exact("reduce.hip", "sum_log_diag_sq_kernel", "hipLaunchKernelGGL(sum_log_diag_sq_kernel, dim3((unsigned)(batch > 0 ? batch : 1)), dim3(RB)"),
    # ---- gemm.hip
    planned("gemm.hip", "KERNEL", "const dim3 grid(p.grid_x, p.grid_y, p.grid_z);", "tests/test_gpu_gemm_launch.py",
            covers=("gemm_nt_kernel", "gemm_nt_pre64", "gemm_nt_fast")),   # launch_tiled<KERNEL, MAX_LDS>
    planned("gemm.hip", "gemm_nt_small", "hipLaunchKernelGGL(gemm_nt_small, grid, dim3(p.threads), p.lds_bytes", "tests/test_gpu_gemm_launch.py"),
    strided("gemm.hip", "gemm_nt_empty_k_kernel",
            clamp("(unsigned)std::min(gpk_cdiv(n, 256), 64)", "min(ceil(n / 256), 64) column blocks, columns strided",
                  near=[(C, "GEMM_CASES", (2, 16384, 0, 1.0, 0.0, 0, False, "c", 0))],
                  far=[(C, "GEMM_CASES", (2, 16385, 0, 2.0, -0.5, 0, False, "ld", 0))]),
            clamp("for (int i0 = 0; i0 < m; i0 += 65535)", "at most 65535 rows per launch, a host loop over the first row",
                  near=[(C, "GEMM_CASES", (65535, 3, 0, 2.0, -0.5, 0, False, "c", 0))],
                  far=[(C, "GEMM_CASES", (65536, 3, 0, 1.0, 0.0, 0, False, "c", 0))]),
            clamp("(unsigned)std::min(m - i0, 65535), (unsigned)nbatch);", "blockIdx.z over the batch (refused above 65535)",
                  near=[(C, "GEMM_CASES", (9, 11, 0, 2.0, -0.5, 0, False, "c", 0))],
                  far=[(C, "GEMM_CASES", (9, 300, 0, 2.0, -0.5, 0, False, "c", 3))])),
    # ---- sync.hip: single blocks
    exact("sync.hip", "noop_kernel", "hipLaunchKernelGGL(noop_kernel, dim3(1), dim3(64)"),
    exact("sync.hip", "wait_flag_kernel", "hipLaunchKernelGGL(wait_flag_kernel, dim3(1), dim3(64)"),
    exact("sync.hip", "set_flag_kernel", "hipLaunchKernelGGL(set_flag_kernel, dim3(1), dim3(1)"),
    exact("sync.hip", "probe_wait_kernel", "hipLaunchKernelGGL(probe_wait_kernel, dim3(1), dim3(1)"),
    exact("sync.hip", "probe_set_kernel", "hipLaunchKernelGGL(probe_set_kernel, dim3(1), dim3(1)"),
    exact("sync.hip", "publish_host_kernel", "hipLaunchKernelGGL(publish_host_kernel, dim3(1), dim3(64)"),
    # ---- bench_kernels.hip: rate probes of bench.py, not primitives -- nothing to hold to a reference
    exact("bench_kernels.hip", "mfma_f64_rate_kernel", "hipLaunchKernelGGL(mfma_f64_rate_kernel, dim3(blocks), dim3(512)"),
    strided("bench_kernels.hip", "stream_store_kernel",
            clamp("hipLaunchKernelGGL(stream_store_kernel, dim3(256 * 8), dim3(256)", "a fixed grid of 2048 blocks, elements strided",
                  uncovered="a store-bandwidth probe of the benchmark: it writes one constant, and no result is read back")),
    # ---- rowops.hip
    exact("rowops.hip", "diag_add_kernel", "hipLaunchKernelGGL(diag_add_kernel, dim3((n + 255) / 256), dim3(256)"),
    strided("rowops.hip", "set_identity_kernel",
            clamp("dim3 grid((unsigned)gpk_cdiv(n, 256), (unsigned)n, (unsigned)(batch > 0 ? batch : 1));", "no clamp: ceil(n / 256) column blocks",
                  uncovered="the grid covers the row at every n, so the column loop makes one trip: it has no far side")),
    strided("rowops.hip", "zero_upper_kernel",
            clamp("if (gx > 16) gx = 16;", "min(ceil(n / 256), 16) column blocks, columns strided",
                  near=[("test_gpu_thresholds", None, '@pytest.mark.parametrize("n", [4095, 4096, 4097])')],
                  far=[("test_gpu_thresholds", None, '@pytest.mark.parametrize("n", [4095, 4096, 4097])')])),
    exact("rowops.hip", "transpose_kernel", "dim3 grid((unsigned)gpk_cdiv(cols, 32), (unsigned)gpk_cdiv(rows, 32),\n"),
    exact("rowops.hip", "row_stats_kernel<4>", "const dim3 grid((unsigned)gpk_cdiv(rows, 4));"),
    exact("rowops.hip", "row_stats_sep_kernel", "hipLaunchKernelGGL(row_stats_sep_kernel, dim3((unsigned)gpk_cdiv(rows, 4), (unsigned)P), dim3(256)"),
    exact("rowops.hip", "row_dot_kernel", "hipLaunchKernelGGL(row_dot_kernel, dim3((unsigned)gpk_cdiv(rows, 4)), dim3(256)"),
    exact("rowops.hip", "transpose_shift_kernel", "dim3 grid((unsigned)gpk_cdiv(cols, 32), (unsigned)gpk_cdiv(rows, 32), 1);"),
    # ---- kernel matrices: one T x T tile per block
    exact("rbf.hip", "rbf_kernel<FAMILY, COMB>", "dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));"),
    exact("dot.hip", "dot_kernel<FAMILY, COMB>", "dim3 grid((unsigned)gpk_cdiv(a.n2, T), (unsigned)gpk_cdiv(a.n1, T));"),
    exact("dot.hip", "dot_diag_kernel<GPK_DOT_LINEAR>", "const dim3 grid((unsigned)gpk_cdiv(n, T));"),
    exact("dot.hip", "dot_diag_kernel<GPK_DOT_POLYNOMIAL>", "const dim3 grid((unsigned)gpk_cdiv(n, T));"),
    exact("dot.hip", "dot_adjoint_tail_kernel", "hipLaunchKernelGGL(dot_adjoint_tail_kernel, dim3(1), dim3(DT_THREADS)"),
    # ---- the factorisation: one block per problem of the batch; the in-group solves walk their slivers under a plan
    planned("leaf.hip", "leaf_kernel<true>", "dim3 grid((unsigned)(batch > 0 ? batch : 1));", "tests/test_potrf_plan.py"),
    planned("leaf.hip", "leaf2_kernel", "dim3 grid((unsigned)(batch > 0 ? batch : 1));", "tests/test_potrf_plan.py"),
    planned("group_solve.hip", "group_solve2_kernel", "const dim3 grid(c.wgs, (unsigned)batch);", "tests/test_gpu_potrf_layouts.py"),
    planned("group_solve.hip", "group_solve_kernel", "const dim3 grid(c.wgs, (unsigned)batch);", "tests/test_gpu_potrf_layouts.py"),
    # ---- varexp.hip
    strided("varexp.hip", "varexp_kernel<false>",
            clamp("const int nb = nblocks_for((long)m.rows * m.P);", "one block per 1024 elements (four trips), at most 1024 blocks",
                  near=[(C, "VAREXP_CASES", (257, 5, False, True, "off"))], far=[(C, "VAREXP_CASES", (270000, 4, False, False, "c"))])),
    strided("varexp.hip", "varexp_kernel<true>",
            clamp("nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);\n  hipLaunchKernelGGL(varexp_kernel<true>",
                  "min(ceil(rows P / 256), 1024) blocks, elements strided",
                  near=[(C, "SVGP_CASES", (16, 131072, 2, 2, False, True, "c"))], far=[(C, "SVGP_CASES", (16, 131073, 2, 2, False, True, "c"))]),
            clamp("for (int i = threadIdx.x; i < (int)gridDim.x; i += RB)", "the last ticket's block sums gridDim.x partials, 256 per trip",
                  near=[(C, "SVGP_CASES", (129, 257, 3, 5, False, True, "c"))],
                  far=[(C, "SVGP_CASES", (16, 65537, 2, 1, False, True, "c")), ("test_gpu_step_tail", None, "(16, 65537, 2, 1)])")])),
    strided("varexp.hip", "mixed_varexp_kernel",
            clamp("return (int)(nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb));", "four wave passes per block, at most 1024 blocks",
                  near=[("test_gpu_lcm", "MIXED_CASES", (300, 16, 1, "per", True, False, "c"))],
                  far=[("test_gpu_lcm", "MIXED_CASES", (16391, 16, 16, "per", True, True, "c"))])),
    strided("varexp.hip", "plan.kernel",   # hipLaunchKernel through LikPlan::kernel
            clamp("nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);\n  void* kargs[] = {&a};",
                  "four wave passes per block, at most 1024 blocks",
                  near=[("test_gpu_likelihoods", "KERNEL_CASES", (257, 1, False, "ld")), ("test_gpu_multiclass", "KERNEL_CASES", (257, 2, False, "ld"))],
                  far=[("test_gpu_likelihoods", "[BIG_CASE]", (70001, 1, False, "c")), ("test_gpu_multiclass", "[BIG_CASE]", (4200, 16, False, "c"))]),
            covers=("lik_varexp_kernel", "lik_multiclass_kernel")),
    # ---- periodic.hip
    exact("periodic.hip", "periodic_warp_kernel", "const long blocks = ((long)n * d + 255) / 256;"),
    exact("periodic.hip", "periodic_moment_rows_kernel", "hipLaunchKernelGGL(periodic_moment_rows_kernel, dim3((unsigned)gpk_cdiv(n2, 256)), dim3(256)"),
    exact("periodic.hip", "periodic_adjoint_tail_kernel", "hipLaunchKernelGGL(periodic_adjoint_tail_kernel, dim3(1), dim3(PT_THREADS)"),
    # ---- train_glue.hip
    exact("train_glue.hip", "moment_rows_kernel", "hipLaunchKernelGGL(moment_rows_kernel, dim3((unsigned)gpk_cdiv(n2, 256)), dim3(256)"),
    exact("train_glue.hip", "adjoint_tail_kernel", "hipLaunchKernelGGL(adjoint_tail_kernel, dim3(1), dim3(AT_THREADS)"),
    strided("train_glue.hip", "adam_kernel",
            clamp("nb < 4096 ? nb : 4096", "min(ceil(n / 256), 4096) blocks, elements strided",
                  near=[(C, 'CASE_TABLES["adam_step_"]', (1048576, False))],
                  far=[(C, 'CASE_TABLES["adam_step_"]', (1048577, True)), (C, 'CASE_TABLES["adam_step_"]', (2097153 + 257, False))])),
    exact("train_glue.hip", "symmetrize_kernel", "hipLaunchKernelGGL(symmetrize_kernel, dim3(nb, nb), dim3(256)"),
    strided("train_glue.hip", "lowrank_axpy_kernel",
            clamp("(unsigned)(m < 2048 ? m : 2048)", "gridDim.y = min(m, 2048), rows strided",
                  near=[(C, 'CASE_TABLES["lowrank_axpy"]', (2048, 130, 16, "c"))],
                  far=[(C, 'CASE_TABLES["lowrank_axpy"]', (2049, 63, 5, "off")), (C, 'CASE_TABLES["lowrank_axpy"]', (4097, 66, 16, "c"))])),
]


# ------------------------------------------------------------------------------------------------ the scans
def _sources(csrc=CSRC):
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(csrc, "*.hip")))}


def _first_argument(text, start):
    """the first argument of the call whose opening parenthesis is at text[start - 1], without a wrapping pair of parentheses or a
    leading cast to a pointer"""
    depth, i = 0, start
    while depth or text[i] not in ",)":
        depth += text[i] in "(<"
        depth -= text[i] in ")>"
        i += 1
    arg = " ".join(text[start:i].split())
    arg = re.sub(r"^\((?:const )?void ?\*\)", "", arg)
    return arg[1:-1] if arg.startswith("(") and arg.endswith(")") else arg


def launch_sites(sources):
    """{(file, kernel name as written at the site)} over hipLaunchKernelGGL( and hipLaunchKernel("""
    return {(f, _first_argument(text, m.end())) for f, text in sources.items() for m in re.finditer(r"\bhipLaunchKernel(?:GGL)?\(", text)}


def kernel_bodies(sources):
    """{(file, kernel): text from its __global__ line to the next one (or the end of the file)}"""
    out = {}
    for f, text in sources.items():
        starts = [m.start() for m in re.finditer(r"__global__", text)]
        for a, b in zip(starts, starts[1:] + [len(text)]):
            name = re.match(r"__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)", text[a:b])
            assert name, (f, text[a:a + 80])
            out[(f, name.group(1))] = text[a:b]
    return out


def _names(row):
    """the kernels a row stands for, without template arguments"""
    return (row["kernel"].split("<")[0],) + tuple(row.get("covers", ()))


def problems(rows, sources):
    """Every disagreement between the table and the sources, as text (empty: the inventory holds)."""
    bad = []
    have, want = {(r["file"], r["kernel"]) for r in rows}, launch_sites(sources)
    bad += [f"launch without a row in LAUNCHES: {k}" for k in sorted(want - have)]
    bad += [f"row of LAUNCHES without a launch site: {k}" for k in sorted(have - want)]
    if len(have) != len(rows):
        bad.append("two rows for one launch")
    by_kernel = {(r["file"], n): r for r in rows for n in _names(r)}
    for (f, name), body in sorted(kernel_bodies(sources).items()):
        row = by_kernel.get((f, name))
        if row is None:
            bad.append(f"{f}: {name} is defined but no row launches or covers it")
        elif "gridDim" in body and row["kind"] == EXACT:
            bad.append(f"{f}: {name} mentions gridDim, so its row cannot be exact: it needs its clamp and cases on both sides of it")
    for r in rows:
        bad += [f"{r['file']}: {r['kernel']}: the launch expression {e!r} is gone: re-derive the row" for e in r["exprs"]
                if e not in sources.get(r["file"], "")]
    return bad


def _case_exists(ref):
    module, table, case = ref
    mod = importlib.import_module(module)
    if table is None:
        return case in open(mod.__file__).read()
    return case in eval(table, vars(mod))   # (the expression is a literal of LAUNCHES above)


# ------------------------------------------------------------------------------------------------ the guards
def test_inventory_matches_the_sources():
    """Launch sites == rows; no kernel that mentions gridDim is exact; every quoted launch expression still stands in its file."""
    bad = problems(LAUNCHES, _sources())
    assert not bad, "\n".join(bad)


def test_strided_rows_name_cases_on_both_sides():
    for r in LAUNCHES:
        if r["kind"] == PLANNED:
            assert os.path.exists(os.path.join(os.path.dirname(HERE), r["owner"])), r
        if r["kind"] != STRIDED:
            continue
        for c in r["clamps"]:
            if c["uncovered"]:
                assert not c["near"] and not c["far"], (r["kernel"], c["expr"])
                continue
            assert c["near"] and c["far"], f"{r['kernel']}: {c['value']}: a clamp needs a case on each side"
            gone = [ref for ref in c["near"] + c["far"] if not _case_exists(ref)]
            assert not gone, f"{r['kernel']}: {c['value']}: cases that are not in their table: {gone}"


def test_guard_sees_a_deleted_row_and_a_moved_clamp():
    """The guard's own failure modes, on copies: a row taken out, a clamp literal edited, a loop added to an exact kernel, a new launch."""
    sources = _sources()
    adam = next(r for r in LAUNCHES if r["kernel"] == "adam_kernel")
    assert any("launch without a row" in b and "adam_kernel" in b for b in problems([r for r in LAUNCHES if r is not adam], sources))
    moved = dict(sources, **{"train_glue.hip": sources["train_glue.hip"].replace("nb < 4096 ? nb : 4096", "nb < 8192 ? nb : 8192")})
    assert moved != sources
    assert any("adam_kernel" in b and "is gone" in b for b in problems(LAUNCHES, moved))
    looped = dict(sources, **{"rowops.hip": sources["rowops.hip"].replace("if (i < n) A[(long)i * lda + i] += v[i];",
                                                                           "for (; i < n; i += gridDim.x * 256) A[(long)i * lda + i] += v[i];")})
    assert looped != sources
    assert any("diag_add_kernel mentions gridDim" in b for b in problems(LAUNCHES, looped))
    added = dict(sources, **{"sync.hip": sources["sync.hip"] + "\nvoid f() { hipLaunchKernelGGL((new_kernel<2>), dim3(1), dim3(1), 0, 0); }\n"})
    assert any("launch without a row" in b and "new_kernel<2>" in b for b in problems(LAUNCHES, added))
