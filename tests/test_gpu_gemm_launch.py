"""Every launch variant of the GEMM, element by element, at its smallest shape.

Which kernel a GEMM call gets, and how it is launched, is decided by make_gemm_plan (gpflow_amd/csrc/gemm_plan.h).  Half of what the
plan can select is set only on internal GemmArgs -- max_wgs (capped persistent workgroups, the tail split into 64 x 64 quarters, the
exclusive-LDS request), tile_queue, tile64, small_loop, no_small, sig_ptr / wait_ptr, stat_* -- and so is out of reach of
ops.gemm_nt / ops.project.  tests/gemm_launch_run.hip links the library's object files and calls the hidden gpk_launch_gemm itself.

ONE table (CASES) holds, per row, the call words (tests/gemm_case_words.h), the plan fields the row is there for, and a comment
naming the branch.  A NEW LAUNCH VARIANT GETS ITS CASE HERE.  Two tiers share the table:

CPU tier (no device): tests/gemm_plan_dump.cpp must return exactly the pinned plan of every row -- a retuned threshold that moves a
row off its branch fails here, with the row named; the table must cover every variant the plan can produce; and the case tables of
tests/test_gpu_contract.py are pinned to the branches their comments claim.

GPU tier: one runner process per session runs all rows (never a second one: a failure fails every dependent test with the runner's
stderr).  Per row: the plan printed on the device machine equals the pin; the result is within the derived bound of a longdouble
reference; never-read regions are NaN and skipped regions come back bitwise; a second run is bit-identical; the hand-off words hold
what the kernel must leave there.

Left out of the table: b_tri_off, b_tri_rows and the C2 / sq_cols < n epilogue are set by no caller in csrc/; stagger_ticks only
delays a start and needs 1024 tiles.  The awaited word of the wait=1 row already holds the awaited value: the expiry of the bounded
wait is tests/test_gpu_handoff.py's."""
import itertools
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gemm_plan as tgp  # noqa: E402

dumper = tgp.dumper   # (the session fixture that builds tests/gemm_plan_dump.cpp with plain g++)

ROOT = tgp.ROOT
RUNNER = os.path.join(ROOT, "gpflow_amd", "csrc", "build", "gemm_launch_run")
U = 2.0 ** -53
LD = np.longdouble
NAN = float("nan")
SENTINEL = -777.0
FAST_LDS = tgp.FAST_LDS          # 73728
EXCL_LDS = 84 * 1024             # the exclusive request of a capped launch (CAP_EXCL_LDS_KB)
SMALL_LDS = lambda k: 144 * (k + 2) * 8   # noqa: E731   (16 + 128 rows of k + 2 doubles)
T128, T128x64, T64x128w, T64x128, T64, T32 = "128,128,2,2", "128,64,2,2", "64,128,1,4", "64,128,2,2", "64,64,4,1", "32,64,2,2"
PINNED = ("kernel", "tile", "epi", "pair", "queue", "sp", "compact", "total", "grid", "lds_bytes", "tile_snake", "tail_tiles",
          "tail_first1", "tail_grid_x", "queue_wgs")


def pin(kernel, total, grid, lds_bytes, tile=None, epi=0, pair=0, queue=0, sp=0, compact=0, snake=0, tail=(0, 0, 0), queue_wgs=0):
    """tail = (tail_tiles, tail_first1, tail_grid_x); grid = (x, y, z)"""
    return dict(kernel=kernel, tile=tile, epi=epi, pair=pair, queue=queue, sp=sp, compact=compact, total=total, grid=grid,
                lds_bytes=lds_bytes, tile_snake=snake, tail_tiles=tail[0], tail_first1=tail[1], tail_grid_x=tail[2], queue_wgs=queue_wgs)


def fast(total, grid, lds_bytes=FAST_LDS, **kw):
    return pin("fast", total, grid, lds_bytes, **kw)


def generic(tile, total, grid, **kw):
    bm, bn = (int(v) for v in tile.split(",")[:2])
    return pin("generic", total, grid, 2 * (bm + bn) * 18 * 8, tile=tile, **kw)


def small(k, grid):
    return pin("small", 0, grid, SMALL_LDS(k))


def pre64(total, grid, **kw):
    return pin("pre64", total, grid, 36864, **kw)


R = dict(m=700, n=450, k=144)                 # ragged edges on the fast tile: 6 x 4 tiles of 128 x 128
PROJ = dict(epi=1, b_tri=1)                   # a projection: alpha = 1, beta = 0, no C, B upper-triangular
# (call words, pinned plan).  epi 0 rows are alpha = -1, beta = 1 unless stated.
CASES = [
    # ---- capped walk and tail split (epi 0, fast tile)
    (dict(R, max_wgs=5), fast(24, (5, 1, 1), EXCL_LDS)),                       # 5 persistent workgroups walk 24 tiles; 24 % 5 = 4 > 60 % of 5: no tail; exclusive LDS
    (dict(R, max_wgs=7), fast(21, (7, 1, 1), EXCL_LDS, tail=(3, 22, 12))),     # three whole rounds + 3 tiles as 12 quarters (tail launch on the 64 x 64 tile)
    (dict(R, max_wgs=7, beta=0), fast(21, (7, 1, 1), EXCL_LDS, tail=(3, 22, 12))),   # the same with beta = 0: NaN C must not leak from either launch
    (dict(R, max_wgs=20), fast(20, (20, 1, 1), FAST_LDS, tail=(4, 21, 16))),   # ONE whole round: no walk, so no exclusive request; 4 tail tiles
    (dict(R, max_wgs=7, c_lower=1), fast(18, (7, 1, 1), EXCL_LDS, compact=1)),  # lower-only: compact numbering, capped walk, never a tail
    (dict(R, max_wgs=7, b_tri=1), fast(24, (7, 1, 1), EXCL_LDS)),              # triangular K under a cap: unpaired, no tail
    (dict(R, max_wgs=7, batch=2), fast(24, (7, 2, 1), FAST_LDS)),              # batched under a cap: walk over grid.y, no tail, no exclusive request
    (dict(m=64, n=129, k=256, max_wgs=1, sig=1), fast(2, (1, 1, 1), EXCL_LDS)),   # one workgroup, two tiles (partial column tile); entry signal of the fast kernel
    # ---- tile queue
    (dict(m=1024, n=1024, k=16, batch=9, tile_queue=1), fast(64, (512, 1, 1), queue=1, queue_wgs=512)),    # 576 (entry, tile) pairs over the batch
    (dict(m=2944, n=2944, k=16, tile_queue=1), fast(529, (512, 1, 1), queue=1, queue_wgs=512)),            # 529 tiles of one problem
    (dict(m=4000, n=4000, k=16, c_lower=1, tile_queue=1, stagger_first=224),
     fast(528, (448, 1, 1), queue=1, queue_wgs=448, compact=1)),                                           # the trailing update's form: compact, 2 x 224 workgroups
    # ---- tile64
    (dict(m=200, n=200, k=128, c_lower=1, tile64=1, no_small=1), pre64(10, (10, 1, 1), compact=1)),        # pre64, lower-only
    (dict(m=130, n=70, k=16, tile64=1, sig=1), pre64(6, (6, 1, 1))),                                       # pre64, dense, one slab, ragged edges; entry signal
    (dict(m=200, n=200, k=144, c_lower=1, tile64=1, no_small=1, sig=1), generic(T64, 10, (10, 1, 1), compact=1)),   # K > 128: generic 64 x 64, compact; entry signal
    (dict(m=200, n=200, k=128, c_lower=1, tile64=1, align=1), generic(T64, 10, (10, 1, 1), compact=1)),    # odd lda: generic 64 x 64 (scalar loads)
    # ---- the latency kernel walking row blocks
    (dict(m=8208, n=128, k=16, small_loop=1), small(16, (1, 512, 1))),         # 513 slivers on 512 workgroups (small_loop)
    (dict(m=256, n=256, k=32, max_wgs=5), small(32, (2, 3, 1))),               # capped: 3 rows of workgroups walk 16 row blocks
    (dict(m=1920, n=128, k=128, c_lower=1, max_wgs=16, sig=1, wait=1), small(128, (1, 16, 1))),   # the chain strip: 16 walkers; signal and (satisfied) wait
    (dict(m=300, n=130, k=128, c_lower=1), small(128, (2, 19, 1))),            # one row block per workgroup, partial column tile, lower-only
    (dict(m=8208, n=128, k=16), fast(65, (65, 1, 1))),                         # the small_loop product without the flag: fast tile
    (dict(m=768, n=512, k=128, no_small=1), fast(24, (24, 1, 1))),             # no_small: fast tile instead of the latency kernel
    # ---- paired triangular K, epi 0
    (dict(m=64, n=512, k=512, b_tri=1), fast(2, (2, 1, 1), pair=1)),           # kind 3, two pairs
    (dict(m=64, n=640, k=640, b_tri=2), fast(3, (3, 1, 1), pair=1)),           # kind 3, odd gx: the last workgroup unpaired; B lower
    (dict(m=64, n=512, k=512, b_tri=1, c_lower=1), fast(1, (1, 1, 1), compact=1)),   # lower-only: unpaired, compact, one tile
    # ---- projections (epi 1)
    (dict(PROJ, m=40, n=512, k=512), fast(4, (4, 1, 1), epi=1, snake=1)),      # kind 4: unpaired, heavy and light tile per CU
    (dict(PROJ, m=40, n=640, k=640), fast(3, (3, 1, 1), epi=1, pair=1)),       # kind 5: paired, odd gx
    (dict(PROJ, m=40, n=640, k=640, batch=2), fast(3, (3, 2, 1), epi=1, pair=1)),   # paired over grid.y
    (dict(PROJ, m=40, n=512, k=512, stats=1), fast(4, (4, 1, 1), epi=1, sp=1, snake=1)),   # row statistics ride along, kind 4
    (dict(PROJ, m=40, n=640, k=640, stats=1, batch=3), fast(3, (3, 3, 1), epi=1, pair=1, sp=1)),   # kind 5: three columns of stat_mv from one shared A
    (dict(PROJ, m=40, n=256, k=256), fast(2, (2, 1, 1), epi=1)),               # gx < 4: neither paired nor in the unpaired order
    (dict(PROJ, m=40, n=256, k=256, stats=1), fast(2, (2, 1, 1), epi=1, sp=1)),   # ... with the row statistics
    (dict(PROJ, m=520, n=512, k=512), generic(T32, 136, (136, 1, 1))),         # 32 x 64, fewer than 256 tiles: no snake
    (dict(PROJ, m=1040, n=512, k=512), generic(T32, 264, (512, 1, 1), snake=1)),   # 32 x 64, snake 1, grid padded from 264 to 512
    (dict(PROJ, m=1024, n=512, k=512, batch=2), generic(T32, 256, (256, 2, 1), snake=2)),   # 32 x 64, snake 2 (whole rounds, XCD-private rows)
    (dict(PROJ, m=1024, n=512, k=512), generic(T32, 256, (256, 1, 1))),        # 256 tiles of ONE problem: snake off
    (dict(PROJ, m=1300, n=512, k=512, batch=5), generic(T64, 168, (168, 5, 1))),   # pairs 110: the 64 x 64 few-rows tile
    (dict(PROJ, m=12700, n=128, k=128), generic(T64, 398, (512, 1, 1), snake=1)),   # 64 x 64 (pairs 100) under snake 1: 398 tiles on a grid of 512
    (dict(PROJ, m=8192, n=128, k=128, batch=2), generic(T64, 256, (256, 2, 1), snake=2)),   # 64 x 64 (pairs 128) under snake 2
    (dict(PROJ, m=300, n=129, k=129), generic(T64x128, 10, (10, 1, 1))),       # 64 x 128 2x2 (n = 129: 64-wide tiles would miss a slot); slots of 64, 64, 1, 0 columns
    (dict(PROJ, m=8200, n=129, k=129), generic(T64x128, 258, (512, 1, 1), snake=1)),   # 64 x 128 2x2 under snake 1
    (dict(PROJ, m=8192, n=129, k=129, batch=2), generic(T64x128, 256, (256, 2, 1), snake=2)),   # 64 x 128 2x2 under snake 2
    # ---- generic tiles of epi 0
    (dict(m=300, n=300, k=1024, c_lower=1), generic(T64x128w, 15, (15, 1, 1))),   # 64 x 128 1x4, NOT compact (bm != bn): 15 tiles enumerated, the kernel skips above the diagonal
    (dict(m=64, n=129, k=17), generic(T128, 2, (2, 1, 1))),                    # m <= 64, ragged K: the 128 x 128 generic tile
    (dict(m=65, n=64, k=144), generic(T128x64, 1, (1, 1, 1))),                 # n <= 64: the 128 x 64 tile
]


def words(call):
    return " ".join("%s=%s" % kv for kv in call.items())


IDS = [words(c) for c, _ in CASES]


def pinned(plan):
    p = dict(plan, grid=tgp.grid(plan))
    return {k: p.get(k) for k in PINNED}


# ================================================================================================ CPU tier
@pytest.fixture(scope="session")
def table_plans(dumper, tmp_path_factory):
    return tgp.plans(dumper, [c for c, _ in CASES], tmp_path_factory.mktemp("gemm_launch_plans"))


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_table_plan(table_plans, i):
    assert pinned(table_plans[i]) == CASES[i][1], IDS[i]


KERNELS = ("none", "small", "pre64", "generic", "fast", "unsupported")          # GemmKernel
TILES = (None, T128, T128x64, T64x128w, T64x128, T64, T32)                      # GemmTile (None: not the generic kernel)
FAST_CASES = (None,) + tuple(itertools.product((0, 1), (0, 1), (0, 1)))         # launch_plan's switch on (epi, pair, sp)


def variant(call, p):
    """(kernel, tile, (epi, pair, sp), queue, tail split, tile_snake, capped small-kernel walk)"""
    kernel = p["kernel"]
    walk = int(kernel == "small" and p["grid_y"] < -(-call["m"] // 16))
    return (kernel, p.get("tile") if kernel == "generic" else None, (p["epi"], p["pair"], p["sp"]) if kernel == "fast" else None,
            p["queue"], int(p["tail_tiles"] > 0), p["tile_snake"], walk)


def cannot_produce(v):
    """the reason make_gemm_plan never returns this combination, or None"""
    kernel, tile, fc, queue, tail, snake, walk = v
    if kernel in ("none", "unsupported"):
        return "nothing is launched"
    if (tile is not None) != (kernel == "generic"):
        return "a tile shape is the generic kernel's template argument and nobody else's"
    if (fc is not None) != (kernel == "fast"):
        return "(epi, pair, sp) are gemm_nt_fast's template arguments and nobody else's"
    if walk and kernel != "small":
        return "the walk over row blocks is gemm_plan_small's"
    if kernel == "fast" and fc[2] and not fc[0]:
        return "sp = (EPI == 1 && stat_sumsq): the row statistics ride on the squaring epilogue only"
    if queue and (kernel != "fast" or fc != (0, 0, 0)):
        return "queue is set in gemm_plan_fast behind the paired / unpaired returns, under EPI == 0"
    if tail and (kernel != "fast" or fc != (0, 0, 0) or queue):
        return "tail_tiles needs EPI == 0 and no b_tri (so no pair); the queue branch needs tail_tiles == 0"
    if snake and kernel in ("small", "pre64"):
        return "tile_snake is set on the few-rows projection branch (generic) and the unpaired projection (fast) only"
    if snake and kernel == "generic" and tile not in (T32, T64, T64x128):
        return "the few-rows projection branch, the only one to set tile_snake, picks 32 x 64, 64 x 64 or 64 x 128 2x2"
    if snake and kernel == "fast" and (snake == 2 or fc[0] != 1 or fc[1] != 0):
        return "gemm_plan_fast sets tile_snake = 1 and only on its unpaired projection (EPI 1, pair 0)"
    return None


def test_table_covers_every_variant(dumper, table_plans, tmp_path):
    everything = set(itertools.product(KERNELS, TILES, FAST_CASES, (0, 1), (0, 1), (0, 1, 2), (0, 1)))
    producible = {v for v in everything if cannot_produce(v) is None}
    have = {variant(c, p) for (c, _), p in zip(CASES, table_plans)}
    assert have <= producible, f"the table holds variants declared impossible: {sorted(map(str, have - producible))}"
    assert not producible - have, f"producible variants without a row in CASES: {sorted(map(str, producible - have))}"
    # the reasons above are claims about make_gemm_plan: no call of test_gemm_plan's sweep may contradict one
    calls = list(tgp.sweep_calls())
    for c, p in zip(calls, tgp.plans(dumper, calls, tmp_path)):
        v = variant(c, p)
        assert v[0] in ("none", "unsupported") or cannot_produce(v) is None, (c, v, cannot_produce(v))


def _contract_words(layout, k, m, batch=1):
    """align word of an operand layout of test_gpu_contract._on: rows are 16-byte aligned only for a contiguous operand with even k"""
    odd = (k % 2 == 1) or layout in ("ld", "col") or (batch > 1 and (m * k) % 2 == 1)
    return dict(align=2) if layout == "off" else dict(align=1) if odd else {}


def _gemm_case_call(case):
    m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
    if m == 0 or n == 0 or k == 0:
        return None   # (gpk_gemm_nt returns, or runs its own K = 0 kernel, before any plan is made)
    call = dict(m=m, n=n, k=k, alpha=alpha, beta=beta, **_contract_words(layout if batch == 0 else "c", k, m, abs(batch) or 1))
    if b_tri:
        call["b_tri"] = b_tri
    if c_lower:
        call["c_lower"] = 1
    if batch:
        call["batch"] = abs(batch)
    return call


def _project_case_call(case):
    rows, m, P, batched, layout = case
    if rows == 0:
        return None
    call = dict(PROJ, m=rows, n=m, k=m, **_contract_words(layout, m, rows, P if batched else 1))
    if P > 1:
        call["batch"] = P
    return call


# what the comment of every row of test_gpu_contract.GEMM_CASES / PROJECT_CASES claims, as plan fields
GEMM_CASE_PINS = {
    (1, 1, 1, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic", tile=T128x64),
    (33, 35, 15, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic"),
    (33, 35, 16, 1.0, 0.0, 0, False, "c", 0): dict(kernel="small", kind=1),
    (33, 35, 17, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic"),
    (63, 65, 64, 1.0, 0.0, 0, False, "c", 0): dict(kernel="small"),
    (64, 129, 256, 1.0, 0.0, 0, False, "c", 0): dict(kernel="fast", kind=2),
    (65, 64, 144, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic", tile=T128x64),
    (200, 257, 17, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic", tile=T64x128w),
    (700, 700, 144, 1.0, 0.0, 0, False, "c", 0): dict(kernel="fast", kind=2, total=36),
    (129, 255, 1024, 1.0, 0.0, 0, False, "c", 0): dict(kernel="generic", tile=T64x128w),
    (127, 128, 129, 0.0, 1.5, 0, False, "c", 0): dict(kernel="generic"),
    (128, 127, 48, 1.3, -0.7, 0, False, "c", 0): dict(kernel="small"),
    (256, 257, 160, -1.1, 0.9, 0, False, "c", 0): dict(kernel="generic", tile=T64x128w),
    (64, 257, 160, -1.1, 0.9, 0, False, "c", 0): dict(kernel="fast", kind=2, total=3),
    (255, 256, 256, 1.0, 0.0, 1, False, "c", 0): dict(kernel="generic", tile=T64x128w),
    (257, 300, 300, 1.0, 0.0, 2, False, "c", 0): dict(kernel="generic", tile=T64x128w),
    (300, 300, 64, 1.0, 0.0, 0, True, "c", 0): dict(kernel="small"),
    (257, 257, 256, 0.5, 0.25, 1, True, "c", 0): dict(kernel="generic", tile=T64x128w, compact=0),
    (65, 63, 33, 1.0, 0.0, 0, False, "ld", 0): dict(kernel="generic"),
    (129, 130, 64, 1.0, 0.0, 0, False, "off", 0): dict(kernel="generic"),
    (129, 256, 256, 1.0, 0.5, 0, False, "off", 0): dict(kernel="generic", tile=T64x128w),
    (64, 256, 256, 1.0, 0.5, 0, False, "off", 0): dict(kernel="generic", tile=T128),
    (100, 70, 48, 1.0, 0.0, 0, False, "col", 0): dict(kernel="generic"),
    (64, 80, 32, 1.0, 0.0, 0, False, "c", 3): dict(kernel="small", grid=(1, 4, 3)),
    (130, 140, 144, 1.0, 0.0, 0, False, "c", 2): dict(kernel="generic", grid=(6, 2, 1)),
    (64, 96, 32, 1.0, 0.0, 0, False, "c", -3): dict(kernel="small", grid=(1, 4, 3)),
}
PROJECT_CASE_PINS = {
    (1, 16, 1, False, "c"): dict(kernel="fast", epi=1),
    (40, 128, 2, False, "c"): dict(kernel="fast", epi=1, kind=4),
    (300, 129, 2, False, "ld"): dict(kernel="generic", tile=T64x128),
    (257, 128, 4, False, "c"): dict(kernel="generic", tile=T32),
    (1300, 512, 1, False, "c"): dict(kernel="generic", tile=T32, tile_snake=1, grid=(512, 1, 1)),
    (1300, 512, 5, False, "c"): dict(kernel="generic", tile=T64, tile_snake=0, grid=(168, 5, 1)),
    (65, 64, 3, True, "c"): dict(kernel="generic", tile=T64x128, grid=(2, 3, 1)),
    (129, 96, 2, False, "off"): dict(kernel="generic", tile=T32),
    (40, 96, 2, False, "off"): dict(kernel="generic", tile=T128),
}


# The k = 0 rows make no plan: gpk_gemm_nt launches gemm_nt_empty_k_kernel itself, i0 = 0, 65535, ... < m, each launch on a grid of
# (min(ceil(n / 256), 64), min(m - i0, 65535), batch) with a grid-stride loop over the columns (tests/test_launch_geometry.py holds the
# two expressions to the source).  What each row's comment claims about that geometry:
# (column blocks, trips of the column loop, launches, rows of the last launch, grid.z)
GEMM_EMPTY_K_PINS = {
    (9, 11, 0, 1.0, 0.0, 0, False, "c", 0): (1, 1, 1, 9, 1),
    (9, 11, 0, 2.0, -0.5, 0, False, "c", 0): (1, 1, 1, 9, 1),
    (130, 140, 0, 1.0, 0.0, 0, True, "c", 0): (1, 1, 1, 130, 1),
    (2, 16384, 0, 1.0, 0.0, 0, False, "c", 0): (64, 1, 1, 2, 1),
    (2, 16385, 0, 2.0, -0.5, 0, False, "ld", 0): (64, 2, 1, 2, 1),
    (65535, 3, 0, 2.0, -0.5, 0, False, "c", 0): (1, 1, 1, 65535, 1),
    (65536, 3, 0, 1.0, 0.0, 0, False, "c", 0): (1, 1, 2, 1, 1),
    (9, 300, 0, 2.0, -0.5, 0, False, "c", 3): (2, 1, 1, 9, 3),
}


def _empty_k_geometry(case):
    m, n, batch = case[0], case[1], abs(case[8]) or 1
    gx = min(-(-n // 256), 64)
    launches = -(-m // 65535)
    return gx, -(-n // (gx * 256)), launches, m - (launches - 1) * 65535, batch


def test_contract_tables_are_on_their_branches(dumper, tmp_path):
    """Every row of the public-path tables of test_gpu_contract.py that reaches make_gemm_plan has a pin here, and takes the branch
    its comment names; every k = 0 row has its launch geometry pinned."""
    import test_gpu_contract as contract
    empty_k = [c for c in contract.GEMM_CASES if c[2] == 0 and c[0] > 0 and c[1] > 0]
    assert not [c for c in empty_k if c not in GEMM_EMPTY_K_PINS], "k = 0 rows without a pinned launch geometry"
    assert not [c for c in GEMM_EMPTY_K_PINS if c not in empty_k], "pins of k = 0 rows that are gone"
    for c in empty_k:
        assert _empty_k_geometry(c) == GEMM_EMPTY_K_PINS[c], (c, _empty_k_geometry(c))
    rows = [("gemm_nt", case, _gemm_case_call(case), GEMM_CASE_PINS) for case in contract.GEMM_CASES]
    rows += [("project", case, _project_case_call(case), PROJECT_CASE_PINS) for case in contract.PROJECT_CASES]
    rows = [r for r in rows if r[2] is not None]
    missing = [(name, case) for name, case, _, pins in rows if case not in pins]
    assert not missing, f"rows without a pinned plan: {missing}"
    for (name, case, call, pins), p in zip(rows, tgp.plans(dumper, [r[2] for r in rows], tmp_path)):
        p["grid"] = tgp.grid(p)
        want = pins[case]
        assert {k: p.get(k) for k in want} == want, (name, case, words(call))
    for pins, table in ((GEMM_CASE_PINS, contract.GEMM_CASES), (PROJECT_CASE_PINS, contract.PROJECT_CASES)):
        assert not [c for c in pins if c not in table], "pins of rows that are gone"


# ================================================================================================ inputs and references
def _batch(call):
    return call.get("batch", 1)


def _coeffs(call):
    epi = call.get("epi", 0)
    return float(call.get("alpha", 1.0 if epi else -1.0)), float(call.get("beta", 0.0 if epi else 1.0))


def make_inputs(call):
    """A [m, k] (the batch shares it), B [batch, n, k] with its structure stored as zeros, Bdev = B with the K ranges that fake_ops
    declares never read -- per 128-column tile; the narrower tiles read a subset -- set to NaN, C0 [batch, m, n] (NaN for beta = 0:
    never read; the sentinel in the 128-tiles strictly above the diagonal of a lower-only call), V [k, batch] (stats=1)."""
    m, n, k, nb, b_tri = call["m"], call["n"], call["k"], _batch(call), call.get("b_tri", 0)
    rng = np.random.default_rng([m, n, k, b_tri])
    A = rng.normal(size=(m, k))
    B = np.stack([np.triu(X) if b_tri == 1 else np.tril(X) if b_tri == 2 else X for X in rng.normal(size=(nb, n, k))])
    Bdev = B.copy()
    for n0 in range(0, n, 128) if b_tri else ():
        if b_tri == 1:
            Bdev[:, n0:n0 + 128, :min(n0 & ~15, k)] = NAN
        else:
            Bdev[:, n0:n0 + 128, min(n0 + 128, k):] = NAN
    C0 = None
    if call.get("epi", 0) == 0:
        C0 = rng.normal(size=(nb, m, n)) if _coeffs(call)[1] != 0 else np.full((nb, m, n), NAN)
        if call.get("c_lower"):
            for m0 in range(0, m, 128):
                C0[:, m0:m0 + 128, m0 + 128:] = SENTINEL
    V = rng.normal(size=(k, nb)) if call.get("stats") else None
    return A, B, Bdev, C0, V


def _macs(call):
    return call["m"] * call["n"] * call["k"] * _batch(call)


# the three largest products take a fp64 BLAS reference (longdouble: more than a few seconds each); its own worst case
# (k + 2) u |A| |B|^T is then added to the bound
BLAS_REFERENCE = {words(c) for c in sorted((c for c, _ in CASES), key=_macs)[-3:]}
_products = {}   # (kept only for operands that more than one row uses)


def _operands_key(call):
    return (call["m"], call["n"], call["k"], call.get("b_tri", 0), _batch(call))


_SHARED = {k for k in map(_operands_key, (c for c, _ in CASES)) if [_operands_key(c) for c, _ in CASES].count(k) > 1}


def products(call, A, B):
    """(A B[z]^T, |A| |B[z]|^T, exact) per batch entry z, shared by the rows with the same operands.  exact: in longdouble, block by
    block over the non-zero K range of each 128 rows of B; else fp64 BLAS.  The products of absolute values only scale the bounds:
    they are formed in fp64 and scaled DOWN by their own worst relative error, so no bound is wider than with an exact sum."""
    key = _operands_key(call)
    exact = words(call) not in BLAS_REFERENCE
    if key in _products:
        return _products[key] + (exact,)
    if True:
        m, n, k, b_tri, nb = key
        absAB = np.stack([np.abs(A) @ np.abs(B[z]).T for z in range(nb)]) * (1.0 - 2 * (k + 2) * U)
        if exact:
            a = A.astype(LD)
            AB = np.zeros((nb, m, n), dtype=LD)
            for z, n0 in itertools.product(range(nb), range(0, n, 128)):
                k0, k1 = (min(n0, k) if b_tri == 1 else 0), (min(n0 + 128, k) if b_tri == 2 else k)
                AB[z, :, n0:n0 + 128] = a[:, k0:k1] @ B[z, n0:n0 + 128, k0:k1].astype(LD).T
        else:
            AB = np.stack([A @ B[z].T for z in range(nb)])
        if key in _SHARED:
            _products[key] = (AB, absAB)
    return AB, absAB, exact


def within(name, got, ref, bound):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    bad = ~(err <= bound)   # (a NaN in `got` is bad)
    if bad.any():
        i = int(np.argmax(bad.reshape(-1)))
        idx = np.unravel_index(i, bad.shape)
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries over the bound; first at {idx}: got {got[idx]!r} "
                             f"ref {float(ref[idx])!r} bound {float(np.broadcast_to(bound, bad.shape)[idx])!r}")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ================================================================================================ GPU tier
RUNNER_SECONDS_PER_CASE = 4      # upload, two launches, download, file i/o: well under this for the largest rows
RUNNER_SECONDS_STARTUP = 30      # device initialisation and the load of the code objects


def case_dir(base, i):
    return os.path.join(str(base), "case%03d" % i)


def write_operands(base):
    lines = []
    for i, (call, _) in enumerate(CASES):
        d = case_dir(base, i)
        os.makedirs(d)
        A, _, Bdev, C0, V = make_inputs(call)
        A.tofile(os.path.join(d, "A.bin"))
        Bdev.tofile(os.path.join(d, "B.bin"))
        if C0 is not None:
            C0.tofile(os.path.join(d, "C0.bin"))
        if V is not None:
            V.tofile(os.path.join(d, "V.bin"))
        lines.append(words(call) + " dir=" + d + "\n")
    listing = os.path.join(str(base), "cases.txt")
    with open(listing, "w") as f:
        f.writelines(lines)
    return listing


class Run:
    """what the ONE runner process of the session left: .error (None, or why every dependent test fails), .records (one dict per row),
    .seconds, .base (the directory of the operand and result files)"""

    def __init__(self, base):
        self.base, self.error, self.records, self.seconds = base, None, [], 0.0
        if not os.path.exists(RUNNER):
            self.error = f"{RUNNER} is not built: run __graft_entry__.build() (make -C gpflow_amd/csrc)"
            return
        listing = write_operands(base)
        limit = RUNNER_SECONDS_STARTUP + RUNNER_SECONDS_PER_CASE * len(CASES)
        t0 = time.time()
        try:
            done = subprocess.run([RUNNER, "@" + listing], capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired as e:
            self.error = f"the runner did not finish within {limit} s; nothing is launched again.\nstdout so far:\n{e.stdout}\nstderr:\n{e.stderr}"
            return
        self.seconds = time.time() - t0
        self.stdout = done.stdout
        if done.returncode != 0:
            self.error = f"the runner ended with status {done.returncode}; nothing is launched again.\nstderr:\n{done.stderr}\nlast output:\n{done.stdout[-2000:]}"
            return
        self.records = tgp._parse(done.stdout)
        if len(self.records) != len(CASES) + 1 or "total_ms" not in self.records[-1]:
            self.error = f"the runner printed {len(self.records)} records for {len(CASES)} cases"

    def record(self, i):
        if self.error:
            pytest.fail(self.error, pytrace=False)
        assert self.records[i]["case"] == i
        return self.records[i]

    def result(self, i, name, shape):
        return np.fromfile(os.path.join(case_dir(self.base, i), name + ".bin"), dtype=np.float64).reshape(shape)


@pytest.fixture(scope="session")
def run(gpu):
    with tempfile.TemporaryDirectory(prefix="gemm_launch_") as base:   # (about 1 GB of operands and results: gone with the session)
        yield Run(base)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_device_plan(run, i):
    """1. the plan made on the device machine, with real pointers (so real alignment facts), is the pinned one; and, 3., the padding of
    C is still NaN and A, B, V are bitwise what was uploaded"""
    rec = run.record(i)
    assert pinned(rec) == CASES[i][1], IDS[i]
    assert rec["pad_intact"] == 1, "the padding of C was written"
    assert rec["inputs_intact"] == 1, "A, B or V was modified"


def _check_c(call, got, A, B, C0):
    """2. |C^ - C| <= 2 (k + 2) u (|alpha| |A| |B|^T + |beta| |C0|) against the longdouble product; 3. regions: with c_lower the
    128-tiles strictly above the diagonal keep the sentinel bitwise, entries on or below the diagonal are computed, and the rest
    (above the diagonal inside a diagonal 128-tile: the narrower tiles skip more of it) is either untouched, bitwise, or computed.
    NaN in C0 (beta = 0) or in the never-read ranges of B would show as NaN here."""
    m, n, k = call["m"], call["n"], call["k"]
    alpha, beta = _coeffs(call)
    AB, absAB, exact = products(call, A, B)
    assert exact
    c0 = np.zeros_like(C0) if beta == 0 else C0
    ref = alpha * AB + beta * c0.astype(LD)
    bnd = 2 * (k + 2) * U * (abs(alpha) * absAB.astype(LD) + abs(beta) * np.abs(c0))
    if not call.get("c_lower"):
        return within("C", got, ref, bnd)
    rows, cols = np.arange(m)[:, None], np.arange(n)[None, :]
    strict = np.broadcast_to((cols & ~127) > (rows | 127), got.shape)
    lower = np.broadcast_to(cols <= rows, got.shape)
    assert same_bits(got[strict], C0[strict]), "a 128-tile strictly above the diagonal was written"
    untouched = ~lower & (got.view(np.uint64) == C0.view(np.uint64))
    skip = strict | untouched
    within("C (lower-only)", np.where(skip, 0, got), np.where(skip, 0, ref), np.where(skip, 0, bnd))


def _check_parts(call, part, A, B):
    """Slot partials part[z, s, r] = sum over the 64 columns j of slot s of y_rj^2, y = alpha A B[z]^T.  As test_project_contract
    bounds ssq, restricted to the slot: with e_j = 2 (k + 2) u |alpha| (|A| |B|^T)_j,
    |part^ - part| <= sum_j (2 |y_j| e_j + e_j^2) + 2 (c + 2) u sum_j y_j^2  for the c columns of the slot; a slot without columns is
    exactly 0 (part was NaN on entry: an unwritten slot shows).  Under the fp64 BLAS reference, y itself is off by up to
    f_j = (k + 2) u |alpha| (|A| |B|^T)_j: sum_j (2 |y_j| f_j + f_j^2) is added."""
    n, k = call["n"], call["k"]
    alpha, _ = _coeffs(call)
    AB, absAB, exact = products(call, A, B)
    y = alpha * AB.astype(LD)
    e = 2 * (k + 2) * U * abs(alpha) * absAB.astype(LD)
    for s in range(part.shape[1]):
        cols = slice(64 * s, min(64 * s + 64, n))
        ys, es = y[:, :, cols], e[:, :, cols]
        c = ys.shape[2]
        if c == 0:
            assert np.all(part[:, s] == 0.0) and not np.any(np.signbit(part[:, s])), f"slot {s} has no columns and is not exactly 0"
            continue
        ref = (ys * ys).sum(2)
        bnd = (2 * np.abs(ys) * es + es * es).sum(2) + 2 * (c + 2) * U * ref
        if not exact:
            bnd = bnd + (np.abs(ys) * es + es * es / 4).sum(2)   # (f = e / 2)
        within(f"part, slot {s}", part[:, s], ref, bnd)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_values_and_regions(run, i):
    run.record(i)
    call = CASES[i][0]
    m, n, k, nb = call["m"], call["n"], call["k"], _batch(call)
    A, B, _, C0, V = make_inputs(call)
    if call.get("epi", 0) == 0:
        return _check_c(call, run.result(i, "C_run1", (nb, m, n)), A, B, C0)
    _check_parts(call, run.result(i, "part_run1", (nb, 2 * -(-n // 128), m)), A, B)
    if call.get("stats"):
        # row statistics against the longdouble row sums:  (k + 2) u sum_k |a| |v|
        a, v = A.astype(LD), V.astype(LD)
        within("stat_sumsq", run.result(i, "sumsq_run1", (m,)), (a * a).sum(1), (k + 2) * U * (a * a).sum(1))
        within("stat_mv", run.result(i, "mv_run1", (m, nb)), a @ v, (k + 2) * U * (np.abs(a) @ np.abs(v)))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_second_run_is_bit_identical(run, i):
    """4. which workgroup takes which tile is dynamic under the tile queue; each tile's arithmetic is not"""
    run.record(i)
    call = CASES[i][0]
    names = ["C"] if call.get("epi", 0) == 0 else ["part"] + (["sumsq", "mv"] if call.get("stats") else [])
    for name in names:
        assert same_bits(run.result(i, name + "_run1", (-1,)), run.result(i, name + "_run2", (-1,))), name


HANDOFF = [i for i, (c, _) in enumerate(CASES) if c.get("sig") or c.get("wait")]


def test_handoff_rows_cover_every_kernel_family():
    assert {CASES[i][1]["kernel"] for i in HANDOFF if CASES[i][0].get("sig")} == {"small", "pre64", "generic", "fast"}
    assert any(CASES[i][0].get("wait") and CASES[i][1]["kernel"] == "small" for i in HANDOFF)


@pytest.mark.gpu
@pytest.mark.parametrize("i", HANDOFF, ids=[IDS[i] for i in HANDOFF])
def test_handoff_words(run, i):
    """5. the entry signal stored sig_val = 7; a wait on a word that already holds the awaited value did not expire (wait_info 0)"""
    rec, call = run.record(i), CASES[i][0]
    if call.get("sig"):
        assert rec["sig_word"] == 7
    if call.get("wait"):
        assert rec["wait_info"] == 0


# ================================================================================================ the record
def main(out):
    """python tests/test_gpu_gemm_launch.py FILE: runs the table once and writes the runner's wall time and per-case plans to FILE
    (profiles/gemm_launch_variants.txt)"""
    with tempfile.TemporaryDirectory() as base:
        r = Run(base)
        if r.error:
            sys.exit(r.error)
        with open(out, "w") as f:
            f.write("tests/gemm_launch_run.hip over the table of tests/test_gpu_gemm_launch.py, one process, two launches per case.\n")
            f.write(f"{len(CASES)} cases; runner wall time {r.seconds:.1f} s (inside the runner: {r.records[-1]['total_ms']} ms).\n\n")
            for (call, _), rec in zip(CASES, r.records):
                p = pinned(rec)
                f.write(f"{words(call)}\n    launch_ms {rec['launch_ms']}  " + " ".join(f"{k}={p[k]}" for k in PINNED if p[k]) + "\n")


if __name__ == "__main__":
    main(sys.argv[1])
