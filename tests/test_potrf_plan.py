"""CPU: the schedule plan of the trapezoidal Cholesky (gpflow_amd/csrc/potrf_plan.h) is host arithmetic on (n, extra, batch, tri) and two
device facts, so it is tested here, without a device: tests/potrf_plan_dump.cpp prints the plan, built with plain g++ and WITHOUT the
ROCm include path (which is the check that the header needs no HIP header).  Pinned: the schedules of the benchmark's shapes, as the
scheduler decided them before the plan was split out of it (the two were compared call by call, profiles/potrf_plan_refactor.txt);
swept: the invariants every plan must satisfy."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NB = 128


@pytest.fixture(scope="session")
def dumper(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("potrf_plan") / "potrf_plan_dump"
    # no -I at all, and no include path from the environment either: the ROCm headers are out of reach
    env = {k: v for k, v in os.environ.items() if k not in ("CPATH", "CPLUS_INCLUDE_PATH", "C_INCLUDE_PATH")}
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", os.path.join(ROOT, "tests", "potrf_plan_dump.cpp"), "-o", str(exe)],
                   check=True, env=env)
    return str(exe)


def _value(text):
    return int(text) if text.lstrip("-").isdigit() else text


def plan(dumper, n, extra, batch=1, tri=0, bulk_cus=224, flags_usable=1, replan=0):
    """replan=1: with the extra-row groups planned again without the progressive first group (what gpk_potrf_core does when the operands
    rule it out)"""
    out = subprocess.run([dumper] + [str(v) for v in (n, extra, batch, tri, bulk_cus, flags_usable, replan)], check=True,
                         capture_output=True, text=True).stdout
    whole, panels = {}, []
    for line in out.splitlines():
        key, *rest = line.split()
        if key == "panel":
            panels.append({k: _value(v) for k, v in (item.split("=") for item in rest)})
        else:
            whole[key] = _value(rest[0])
    assert whole["npanels"] == len(panels)
    return whole, panels


def group_ends(panels):
    return [q["c1"] for q in panels if q["x_group_end"]]


def progressive_ends(panels):
    return [q["c1"] for q in panels if q["x_progressive_block"] >= 0]


def path(whole):
    if whole["single_leaf"]:
        return "single_leaf"
    words = (["large"] if whole["large"] else []) + (["ride"] if whole["ride"] else []) + (["X"] if whole["useX"] else []) + \
        (["tail_zone"] if whole["tail_zone"] else [])
    return " ".join(words)


R256 = list(range(256, 1792 + 1, 256)) + [1920, 2048]
# (n, extra, batch, tri): (wide panels, narrow-or-plain panels), path, stream of the extra rows, group ends, progressive blocks end at, rest_tiled
PINS = [
    ((100, 300, 1, 0), (0, 1), "single_leaf", "X", [100], [], 0),
    ((1024, 4, 1, 0), (0, 8), "ride", None, [], [], 0),
    ((640, 1000, 1, 0), (0, 5), "X", "X", [384, 640], [], 0),
    ((1024, 300, 1, 0), (0, 8), "X tail_zone", "X", [384, 768, 896, 1024], [], 0),
    ((1024, 8192, 1, 0), (0, 8), "X", "X", [384, 768, 1024], [128, 256, 384], 1),
    ((1024, 8192, 4, 0), (0, 8), "X", "X", [256, 512, 768, 1024], [], 0),
    ((1152, 777, 1, 0), (0, 9), "X tail_zone", "X", [256, 512, 768, 896, 1024, 1152], [], 0),
    ((2048, 1024, 1, 0), (0, 16), "X tail_zone", "X", R256, [], 0),
    ((2048, 4096, 1, 0), (0, 16), "X tail_zone", "X", R256, [], 1),
    ((2048, 8192, 1, 0), (0, 16), "X", "X", [512, 1024, 1536, 2048], [128, 256, 384, 512], 1),
    ((2048, 8192 + 1 + 2048, 1, 2048), (0, 16), "X", "X", [512, 1024, 1536, 2048], [128, 256, 384, 512], 1),
    ((4096, 1024, 1, 0), (0, 32), "large X", "B_masked", list(range(512, 4096 + 1, 512)), [], 0),
    ((5000, 1, 1, 0), (2, 30), "large ride", None, [], [], 0),
    ((16384, 1, 1, 0), (20, 28), "large ride", None, [], [], 0),
]


@pytest.mark.parametrize("shape,counts,want_path,xstream,ends,prog,tiled", PINS, ids=["n%d_x%d_b%d_t%d" % p[0] for p in PINS])
def test_pinned_schedules(dumper, shape, counts, want_path, xstream, ends, prog, tiled):
    n, extra, batch, tri = shape
    whole, panels = plan(dumper, n, extra, batch, tri)
    wide = sum(1 for q in panels if q["c1"] - q["c0"] > NB)
    assert (wide, len(panels) - wide) == counts
    assert path(whole) == want_path
    if xstream is not None:
        assert whole["X"] == xstream
    assert group_ends(panels) == ends
    assert progressive_ends(panels) == prog
    assert whole["progressive_candidate"] == (1 if prog else 0)
    assert whole["rest_tiled"] == tiled
    assert whole["nevents"] == 2 * len(panels) + 8


def test_pinned_large_cuts(dumper):
    """n = 5000: two 640-column panels, narrow ones from column 1280, the last 8 columns wide; n = 16384: narrow from 12800; n = 4096: all narrow,
    every narrow panel's rest-update on Bs and no panel whose extra-row group waits on the masked stream is a flag candidate."""
    _, p5000 = plan(dumper, 5000, 1)
    assert [q["c1"] - q["c0"] for q in p5000] == [640, 640] + [128] * 29 + [8]
    assert [q["narrow"] for q in p5000] == [0, 0] + [1] * 30 and p5000[2]["c0"] == 1280
    assert [q["rest_stream"] for q in p5000[:2]] == ["B_masked"] * 2 and all(q["rest_stream"] == "Bs" for q in p5000[2:])
    assert [q["rest_tile_queue"] for q in p5000] == [1, 1] + [0] * 30
    _, p16k = plan(dumper, 16384, 1)
    assert next(q["c0"] for q in p16k if q["narrow"]) == 12800
    _, p4096 = plan(dumper, 4096, 1024)
    assert all(q["narrow"] for q in p4096)
    assert [q["flag_candidate"] for q in p4096] == [0 if (q["x_group_end"] or q["c1"] == 4096) else 1 for q in p4096]


def test_flags_unusable_means_events_everywhere(dumper):
    whole, panels = plan(dumper, 2048, 8192, flags_usable=0)
    assert whole["use_flags"] == 0 and whole["rest_split_enabled"] == 0
    assert not any(q["flag_candidate"] or q["rest_flag"] or q["rest_split_candidate"] for q in panels)


SWEEP_N = [1, 127, 128, 129, 256, 640, 1024, 1152, 2048, 4095, 4096, 4097, 4736, 5000, 16384]
SWEEP_EXTRA = [0, 1, 256, 257, 1023, 1024, 2999, 3000, 6143, 6144, 8192]


def test_invariants_over_the_sweep(dumper):
    for n, extra, batch in itertools.product(SWEEP_N, SWEEP_EXTRA, [1, 4]):
        whole, panels = plan(dumper, n, extra, batch)
        tag = (n, extra, batch)
        # cuts: strictly increasing from 0 to n, every panel at most nbo wide, wide panels before narrow ones
        assert panels[0]["c0"] == 0 and panels[-1]["c1"] == n, tag
        for q, nxt in zip(panels, panels[1:]):
            assert q["c0"] < q["c1"] == nxt["c0"], tag
            assert q["c2"] == nxt["c1"], tag
        assert panels[-1]["c0"] < panels[-1]["c1"] and panels[-1]["c2"] == n and panels[-1]["c3"] == n, tag
        widths = [q["c1"] - q["c0"] for q in panels]
        assert max(widths) <= whole["nbo"], tag
        is_wide = [w > NB for w in widths]
        assert is_wide == sorted(is_wide, reverse=True), tag
        assert all(q["narrow"] == (1 if whole["large"] and q["c1"] - q["c0"] <= NB else 0) for q in panels), tag
        # extra-row groups
        ends = group_ends(panels)
        if whole["useX"]:
            assert ends == sorted(set(ends)) and ends[-1] == n, tag
            begins = [q["x_group_begin"] for q in panels if q["x_group_end"]]
            assert begins == [0] + ends[:-1], tag
        else:
            assert ends == [] and not whole["tail_zone"], tag
        blocks = [q["x_progressive_block"] for q in panels]
        k = sum(1 for b in blocks if b >= 0)
        assert blocks == list(range(k)) + [-1] * (len(panels) - k), tag
        assert k == 0 or whole["progressive_candidate"], tag
        if k:
            assert panels[k - 1]["c1"] == whole["prog_end"] and panels[k - 1]["x_group_end"], tag
        # hand-offs
        for q in panels:
            assert not (q["flag_candidate"] and q["c1"] - q["c0"] > NB), tag
            assert not (q["flag_candidate"] and q["x_group_end"] and whole["X"] == "B_masked"), tag
            assert not (q["rest_split_candidate"] and not q["flag_candidate"]), tag
            assert not (q["rest_flag"] and q["rest_stream"] == "B_masked"), tag
            assert q["rest_stream"] == ("Bs" if q["narrow"] else whole["B"]), tag
        assert 0 <= whole["late_panel"] < len(panels), tag
