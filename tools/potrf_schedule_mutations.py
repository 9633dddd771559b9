#!/usr/bin/env python3
"""Proof that tests/test_potrf_schedule.py sees what it is for: one mutation of the enqueue code at a time, on a scratch copy of
gpflow_amd/csrc, each run through the recorder and the checker.  Prints the table kept in profiles/potrf_schedule_check.txt.
CPU only (g++ and Python).    python tools/potrf_schedule_mutations.py [part of a mutation's name]
                              python tools/potrf_schedule_mutations.py --write-pins    rewrites tests/golden/potrf_schedule_*.txt from the
                                                                                     tree as it is (after a DELIBERATE schedule change)"""
import collections
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_potrf_schedule as T   # noqa: E402

# name, file, (old, new) replacements, runs [(entry, mode, shape)], checker model, expected assertion (None: nothing may change)
SHAPES_SMALL = [("potrf", m, dict(n=2048, extra=8192)) for m in T.ALL_MODES] + [("potrf", m, dict(n=1024, extra=300)) for m in T.ALL_MODES] + \
    [("svgp", m, dict(n=2048, rows=8192, P=1)) for m in T.ALL_MODES]
SHAPES_5000 = [("potrf", m, dict(n=5000, extra=1)) for m in T.ALL_MODES]
# where a flagged rest-update meets a panel that is not flagged, so that its event is recorded on demand: operands the latency kernel
# does not take, and the group ends of a large factorisation whose extra rows wait on the masked stream
SHAPES_EVR = [("potrf", m, dict(n=2048, extra=8192, layout="odd")) for m in T.ALL_MODES] + [("potrf", m, dict(n=4096, extra=1024)) for m in T.ALL_MODES]
SHAPES_OPEN = [(entry, m, shape) for entry, shape in T.OPEN_ITEM for m in T.ALL_MODES]
MUTATIONS = [
    ("drop the cap on the workgroups of a strip that waits in-kernel (the tree before the fix)", "potrf.hip",
     [("if (strip.wait_ptr && plan.bulk_cus > 0) {", "if (false) {")], SHAPES_OPEN + SHAPES_SMALL, {}, 7),
    ("drop the body of strip_waits_for_rest", "potrf.hip",
     [("  int strip_waits_for_rest(GemmArgs& strip) {\n", "  int strip_waits_for_rest(GemmArgs& strip) {\n    return 0;\n")], SHAPES_SMALL, {}, 1),
    ("drop wait_panel in enqueue_rest_update", "potrf.hip", [("  GPK_TRY(sync.wait_panel(Bp, p));\n", "")], SHAPES_SMALL, {}, 1),
    ("drop wait_panel in enqueue_extra_rows", "potrf.hip", [("GPK_TRY(sync.wait_panel(X, p));", "")], SHAPES_SMALL, {}, 1),
    ("drop order_rest_after_previous (n = 5000)", "potrf.hip", [("    GPK_TRY(sync.order_rest_after_previous(Bp));\n", "")], SHAPES_5000, {}, 1),
    ("make need_evr a no-op", "potrf.hip", [("  int need_evr() {\n", "  int need_evr() {\n    return 0;\n")], SHAPES_SMALL + SHAPES_5000 + SHAPES_EVR, {}, 1),
    ("drop the evJoinX pair in join", "potrf.hip",
     [("      GPK_HIP(hipEventRecord(evJoinX, X));\n      GPK_HIP(hipStreamWaitEvent(S, evJoinX, 0));\n", "")], SHAPES_SMALL, {}, 4),
    ("issue late_work on X instead of sync.last_bulk, join untouched", "potrf.hip",
     [("GPK_TRY(hooks.late_work(sync.last_bulk));", "GPK_TRY(hooks.late_work(X));")], SHAPES_SMALL, {}, None),
    ("issue late_work on the unused placeholder stream, join untouched", "potrf.hip",
     [("GPK_TRY(hooks.late_work(sync.last_bulk));", "GPK_TRY(hooks.late_work(aux->pad));")], SHAPES_SMALL, {}, 4),
    ("(model) a sig_ptr signal covers the kernel itself", None, [], SHAPES_SMALL + SHAPES_5000, {"lenient_entry": True}, None),
    ("rest_flag allowed on the masked stream; stream writes there modelled as unordered", "potrf_plan.h",
     [("q.rest_flag = pl.use_flags && p < kMaxFlagPanels && !masked;", "q.rest_flag = pl.use_flags && p < kMaxFlagPanels;")],
     [("potrf", "streamops", dict(n=5000, extra=1))], {"unordered_writes_on": ("masked",)}, 1),
    ("the shard's layout asks for 256 bytes less than it carves (V, the last piece, sticks out)", "drivers.hip",
     [("  w.V = c.take((size_t)m * P * sizeof(double));\n  w.total = c.used;", "  w.V = c.take((size_t)m * P * sizeof(double));\n  w.total = c.used - 256;")],
     [("svgp", m, dict(n=300, rows=333, P=3, whiten=0)) for m in T.ALL_MODES], {}, 8),
    ("drop the KL launches of the whitened shard (kl_white_kernel zeroes the tail's ticket)", "drivers.hip",
     [("  return kl_white_to_out(s, a, w);\n}", "  return 0;\n}")], [("svgp", m, dict(n=300, rows=333, P=3)) for m in T.ALL_MODES], {}, 9),
    ("(control) the unmodified tree under the same runs and models", None, [], SHAPES_SMALL + SHAPES_5000, {"unordered_writes_on": ("masked",)}, None),
    ("(control) the unmodified tree, operands and shapes with events recorded on demand", None, [], SHAPES_EVR, {}, None),
]


def write_pins():
    work = tempfile.mkdtemp(prefix="potrf_schedule_pins_")
    runners = {"product": T.build_runner(work), "exp": T.build_runner(work, experimental=True)}
    for name, (entry, shape) in sorted(T.HEADLINES.items()):
        path = os.path.join(T.PIN_DIR, "potrf_schedule_%s.txt" % name)
        seq = T.sequence(T.record(runners, entry, "gate", reps=2, **shape))
        with open(path, "w") as f:
            f.write("".join("%d %s\n" % p for p in seq))
        print("wrote %s (%d lines)" % (path, len(seq)))
    shutil.rmtree(work)
    return 0


def main():
    if sys.argv[1:] == ["--write-pins"]:
        return write_pins()
    work = tempfile.mkdtemp(prefix="potrf_schedule_mut_")
    ok = True
    for k, (name, fname, repl, runs, model, want) in enumerate(MUTATIONS):
        if len(sys.argv) > 1 and sys.argv[1] not in name:
            continue
        csrc = os.path.join(work, "m%d" % k, "csrc")
        shutil.copytree(T.CSRC, csrc)
        # (the copy sits two levels below `work` as csrc/ does below the repository, next to a copy of include/)
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(work, "include"), dirs_exist_ok=True)
        if fname:
            path = os.path.join(csrc, fname)
            text = open(path).read()
            for old, new in repl:
                assert old in text, (name, old)
                text = text.replace(old, new)
            open(path, "w").write(text)
        out = os.path.join(work, "m%d" % k)
        runners = {"product": T.build_runner(out, csrc), "exp": T.build_runner(out, csrc, experimental=True)}
        failed = collections.Counter()
        first = {}
        for entry, mode, shape in runs:
            for a, msg in T.check_log(T.record(runners, entry, mode, reps=2, **shape), **model):
                failed[a] += 1
                first.setdefault(a, "%s %s %s: %s" % (entry, shape, mode, msg))
        verdict = "nothing fails" if not failed else "fails " + ", ".join("assertion %d (%d messages)" % kv for kv in sorted(failed.items()))
        good = (want is None and not failed) or (want is not None and want in failed)
        ok = ok and good
        print("%-86s | expected %-12s | %s%s" % (name, "nothing" if want is None else "assertion %d" % want, verdict, "" if good else "   <-- NOT AS EXPECTED"))
        for a in sorted(first):
            print("      first of assertion %d: %s" % (a, first[a][:420]))
    shutil.rmtree(work)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
