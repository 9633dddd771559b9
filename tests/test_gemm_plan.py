"""CPU: which kernel a GEMM call gets and how it is launched (gpflow_amd/csrc/gemm_plan.h, make_gemm_plan) is host arithmetic on the
GemmArgs, so it is tested here, without a device: tests/gemm_plan_dump.cpp prints the plan, built with plain g++ and WITHOUT the ROCm
include path (which is the check that the header needs no HIP header).  Pinned: the selections rounds 3 - 6 paid for, as the launcher
made them before the plan was split out of it (the two were compared launch by launch, profiles/gemm_plan_refactor.txt); swept: the
invariants every plan must satisfy."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KB = 1024
FAST_LDS = 2 * 256 * 18 * 8   # two buffers of (128 + 128) rows x (16 + 2) doubles


@pytest.fixture(scope="session")
def dumper(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_dump"
    # no -I at all, and no include path from the environment either: the ROCm headers are out of reach
    env = {k: v for k, v in os.environ.items() if k not in ("CPATH", "CPLUS_INCLUDE_PATH", "C_INCLUDE_PATH")}
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "gemm_plan_dump.cpp"), "-o", str(exe)],
                   check=True, env=env)
    return str(exe)


def _value(text):
    return int(text) if text.lstrip("-").isdigit() else text


def _parse(out):
    plans, cur = [], {}
    for line in out.splitlines():
        if line == "end":
            plans.append(cur)
            cur = {}
        else:
            key, val = line.split()
            cur[key] = _value(val)
    assert not cur
    return plans


def _words(call):
    return ["%s=%s" % kv for kv in call.items()]


def plan(dumper, **call):
    (p,) = _parse(subprocess.run([dumper] + _words(call), check=True, capture_output=True, text=True).stdout)
    return p


def plans(dumper, calls, tmp_path):
    """the plans of many calls from ONE run of the dumper"""
    listing = tmp_path / "calls.txt"
    listing.write_text("".join(" ".join(_words(c)) + "\n" for c in calls))
    out = _parse(subprocess.run([dumper, "@" + str(listing)], check=True, capture_output=True, text=True).stdout)
    assert len(out) == len(calls)
    return out


def grid(p):
    return (p["grid_x"], p["grid_y"], p["grid_z"])


CM = dict(epi=1, b_tri=1, m=8192, n=2048, k=2048)   # the projections of the benchmark's SVGP steps: M = 2048 ...
C3 = dict(epi=1, b_tri=1, m=8192, n=1024, k=1024)   # ... and M = 1024
SHARD = dict(epi=1, b_tri=1, m=1024, n=2048, k=2048)   # a rank's 1024-row shard of the strong-scaled step
REST = dict(m=1792, n=1792, k=128, c_lower=1, tile64=1, no_small=1)   # rest-update of a single-leaf panel beside capped bulk work
# (call, expected fields of the plan); epi 0 calls are alpha = -1, beta = 1 unless stated, operands aligned, batch 1
PINS = {
    "chain_strip": (dict(m=1920, n=128, k=128, c_lower=1),
                    dict(kernel="small", grid=(1, 120, 1), threads=512, lds_bytes=(16 + 128) * 130 * 8, kind=1)),
    "too_many_slivers": (dict(m=8320, n=128, k=128),
                         dict(kernel="fast", epi=0, pair=0, queue=0, grid=(65, 1, 1), lds_bytes=FAST_LDS, stagger_ticks=0, kind=2)),
    "small_loop": (dict(m=8320, n=128, k=128, small_loop=1), dict(kernel="small", grid=(1, 512, 1), kind=1)),
    "rest_pre64": (REST, dict(kernel="pre64", gx=28, gy=28, compact=1, total=406, grid=(406, 1, 1), lds_bytes=36864, kind=6)),
    "rest_odd_lda": (dict(REST, align=1), dict(kernel="generic", tile="64,64,4,1", compact=1, total=406, kind=6)),
    # 256 tiles on 224 workgroups: one whole round, so the exclusive-LDS request does NOT apply; 32 tiles of tail as 128 quarters
    "capped_one_round": (dict(m=8192, n=512, k=512, max_wgs=224),
                         dict(kernel="fast", epi=0, pair=0, grid=(224, 1, 1), total=224, lds_bytes=FAST_LDS, tail_tiles=32, tail_grid_x=128,
                              tail_first1=225, kind=2)),
    "capped_three_rounds": (dict(m=8192, n=1536, k=512, max_wgs=224),
                            dict(kernel="fast", epi=0, pair=0, grid=(224, 1, 1), total=672, lds_bytes=84 * KB, tail_tiles=96,
                                 tail_grid_x=384, tail_first1=673, kind=2)),
    "cm_projection": (CM, dict(kernel="fast", epi=1, pair=1, sp=0, total=512, grid=(512, 1, 1), pair_k_align=1, lds_bytes=FAST_LDS,
                               kind=5)),
    "cm_projection_stats": (dict(CM, stats=1), dict(kernel="fast", epi=1, pair=1, sp=1, total=512, grid=(512, 1, 1), kind=5)),
    "c3_projection": (C3, dict(kernel="fast", epi=1, pair=0, tile_snake=1, stagger_first=256, stagger_ticks=0, total=512,
                               grid=(512, 1, 1), kind=4)),
    "shard_projection": (SHARD, dict(kernel="generic", tile="32,64,2,2", total=1024, grid=(1024, 1, 1), tile_snake=2, lds_bytes=27648,
                                     kind=6)),
    "half_tile": (dict(m=2048, n=2048, k=2048, beta=0), dict(kernel="generic", tile="64,128,1,4", total=512, lds_bytes=55296, kind=6)),
    "ragged_k": (dict(m=1800, n=1800, k=17, beta=0), dict(kernel="generic", tile="128,128,2,2", total=225, lds_bytes=73728, kind=6)),
    "narrow_n": (dict(m=4096, n=64, k=256), dict(kernel="generic", tile="128,64,2,2", kind=6)),
    "staggered": (dict(m=16384, n=16384, k=512, beta=1),
                  dict(kernel="fast", epi=0, pair=0, queue=0, grid=(16384, 1, 1), stagger_first=256, stagger_ticks=2720, kind=2)),
    "tile_queue": (dict(m=15744, n=15744, k=640, c_lower=1, tile_queue=1, stagger_first=224),
                   dict(kernel="fast", epi=0, pair=0, queue=1, compact=1, total=123 * 124 // 2, grid=(448, 1, 1), queue_wgs=448,
                        queue_fetches=7626 + 448, stagger_ticks=0, lds_bytes=FAST_LDS, kind=2)),
    "cm_stats_offset": (dict(CM, stats=1, b_tri_off=16), dict(kernel="unsupported")),
    "c3_stats_offset": (dict(C3, stats=1, b_tri_off=16), dict(kernel="unsupported")),
    "shard_stats_offset": (dict(SHARD, stats=1, b_tri_off=16), dict(kernel="unsupported")),
}


@pytest.mark.parametrize("name", list(PINS))
def test_pinned_plans(dumper, name):
    call, want = PINS[name]
    p = plan(dumper, **call)
    p["grid"] = grid(p)
    assert {k: p.get(k) for k in want} == want


def test_predicates_follow_the_plan(dumper):
    """What gpk_gemm_takes_latency_kernel / gpk_gemm_fuses_row_stats answer is the plan's kernel: tile64 is tested before the latency
    kernel, statistics ride along on the fast tile only, and an under-filled projection cannot carry them."""
    assert plan(dumper, m=1920, n=128, k=128, c_lower=1, tile64=1)["kernel"] == "pre64"
    assert plan(dumper, m=1920, n=128, k=128, c_lower=1, no_small=1)["kernel"] != "small"
    assert plan(dumper, **dict(SHARD, stats=1))["kernel"] == "unsupported"
    assert plan(dumper, **dict(CM, stats=1, stat_P=2))["kernel"] == "unsupported"   # (stat_P must equal the batch)
    assert plan(dumper, **dict(CM, beta=1, align=1))["kernel"] == "unsupported"     # (only the fast tile preloads C for epi 1)
    assert plan(dumper, m=0, n=128, k=128)["kernel"] == "none"


def lower_tiles(m, n, bm, bn):
    """(row tile, column tile) pairs of an m x n output that a lower-only launch visits: the device skips a tile whose first column lies
    right of its last row (tile_decode and the kernels' `n0 > m0 + BM - 1`)"""
    gy, gx = -(-m // bm), -(-n // bn)
    return sum(1 for tm in range(gy) for tn in range(gx) if tn * bn <= tm * bm + bm - 1)


SWEEP_MN = [1, 63, 64, 65, 128, 129, 1024, 1800, 8192]
SWEEP_K = [16, 17, 128, 144, 512, 2048]


def sweep_calls():
    for m, n, k, align in itertools.product(SWEEP_MN, SWEEP_MN, SWEEP_K, (0, 1, 2)):
        shape = dict(m=m, n=n, k=k, align=align)
        for b_tri, c_lower, max_wgs, tile64, small_loop in itertools.product((0, 1), (0, 1), (0, 224), (0, 1), (0, 1)):
            yield dict(shape, epi=0, b_tri=b_tri, c_lower=c_lower, max_wgs=max_wgs, tile64=tile64, small_loop=small_loop)
        for b_tri, max_wgs, stats in itertools.product((0, 1), (0, 224), (0, 1)):
            yield dict(shape, epi=1, b_tri=b_tri, max_wgs=max_wgs, stats=stats)


def test_invariants_over_the_sweep(dumper, tmp_path):
    calls = list(sweep_calls())
    counted = {}
    for c, p in zip(calls, plans(dumper, calls, tmp_path)):
        tag = (c, p)
        kernel = p["kernel"]
        assert kernel != "none", tag
        if c.get("stats"):
            assert kernel == "unsupported" or (kernel == "fast" and p["sp"] == 1), tag   # never the generic kernel
        if kernel == "unsupported":
            assert c["epi"] == 1 and c.get("stats"), tag   # (beta = 0 throughout the epi 1 sweep)
            continue
        assert min(grid(p)) >= 1 and p["threads"] in (256, 512), tag
        assert 0 < p["lds_bytes"] <= 160 * KB, tag
        assert p["kind"] == {"small": 1, "pre64": 6, "generic": 6, "fast": 2 + 2 * p["epi"] + p["pair"]}[kernel], tag
        if kernel in ("fast", "pre64", "small"):
            assert c["align"] == 0 and c["k"] % 16 == 0, tag
        if kernel in ("pre64", "small"):
            assert c["k"] <= 128 and c["epi"] == 0, tag
        assert p["sp"] == 0 or (kernel == "fast" and p["epi"] == 1), tag
        assert p["queue"] == 0 or (kernel == "fast" and p["epi"] == 0), tag
        if kernel == "small":
            assert p["ldk"] == c["k"] + 2 and p["lds_bytes"] == 144 * p["ldk"] * 8, tag
            continue
        # the tile count, from the definition
        bm, bn = {"pre64": (64, 64), "fast": (128, 128)}.get(kernel) or tuple(int(v) for v in p["tile"].split(",")[:2])
        gy, gx = -(-c["m"] // bm), -(-c["n"] // bn)
        assert (p["gx"], p["gy"]) == (gx, gy), tag
        if p["compact"]:
            assert c["c_lower"] and bm == bn and p["pair"] == 0 and p["tail_tiles"] == 0, tag
            key = (c["m"], c["n"], bm)
            if key not in counted:
                counted[key] = lower_tiles(c["m"], c["n"], bm, bn)
            assert p["total"] == counted[key], tag
            if bm == 128:
                assert p["lower_tiles_128"] == counted[key], tag
        elif p["pair"]:
            assert p["total"] == (gx + 1) // 2 * gy, tag
        else:
            assert p["total"] + p["tail_tiles"] == gx * gy, tag   # main + tail tiles = all tiles
        # tail split
        if p["tail_tiles"]:
            assert kernel == "fast" and c["max_wgs"] > 0 and p["grid_x"] == c["max_wgs"], tag
            assert p["tail_grid_x"] == 4 * p["tail_tiles"] and p["tail_first1"] == p["total"] + 1, tag
        else:
            assert p["tail_grid_x"] == 0 and p["tail_first1"] == 0, tag
        # workgroups: one per tile (generic: rounded up to whole rounds of 256 under the snake order), or capped, or the queue's
        if kernel == "fast" and p["queue"]:
            assert p["grid_x"] == p["queue_wgs"] and p["queue_fetches"] == p["total"] * c.get("batch", 1) + p["queue_wgs"], tag
        elif kernel == "fast":
            assert p["grid_x"] == (min(p["total"], c["max_wgs"]) if c["max_wgs"] and not p["pair"] and not p["tile_snake"] else p["total"]), tag
        else:
            assert p["total"] <= p["grid_x"] < p["total"] + 256, tag
