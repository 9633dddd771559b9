"""CPU: HOW the factorisation hands work over between its streams, checked without a device.

tests/potrf_schedule_run.cpp compiles the unmodified gpflow_amd/csrc/potrf.hip and drivers.hip as plain C++ against a recording
stand-in for the HIP runtime (tests/hip_record) and prints what one entry point enqueues: every event record / wait, stream value
operation and kernel launch with its stream and the memory it reads and writes.  This file builds the happens-before relation of
such a log and asserts on it -- for every shape, hand-off mode and operand layout below, the workload's own sizes included.

Edges of the relation
  * stream order;
  * an event wait is ordered after the record of that event that was the most recent IN HOST ORDER when the wait was issued;
  * a flag word written on a kernel's ENTRY (GemmArgs::sig_ptr) carries everything enqueued before that kernel on its stream, not the
    kernel itself (modelled as a node of its own in front of the kernel);
  * a set-flag kernel or hipStreamWriteValue32 carries everything before it on its stream;
  * a gate kernel or hipStreamWaitValue32 orders everything behind it on its stream, an in-kernel wait (wait_ptr) that kernel and
    everything behind it;
  * a wait for (word, v) is satisfied by the signals on that word with (int)(value - v) >= 0.  It is bound to the satisfying
    signals of its own call (normally one; several: only what all of them carry is taken).  Signals of later calls are left out of
    the binding, which is sound because successive signals on one word are themselves asserted to be ordered.

Assertions (check_log): 1 no unordered conflict, 2 no lost hand-off, 3 no cycle, 4 the join is complete, 5 the status word is reset
before anything may store INT_MAX there, 6 no cycle when the streams are mapped to hardware queues, 7 the workgroups that wait
in-kernel leave compute units free, 8 the whole extent of every access (base + (batch - 1) stride + (rows - 1) ld + cols) lies inside
its buffer, 9 within one call every read of the caller's workspace is covered by writes of that call that happen-before it
(workspace_reads_are_written; include/gpk.h, the workspace contract -- necessary only: tests/test_gpu_workspace.py is the real check).

Assertion 6 is a MODEL and is stated as one: streams are mapped to hardware queues by the rule written in aux_create's comment
(potrf.hip: a pool of normal-priority queues, a new stream opens a queue while the pool is not full and then shares the queue with the
fewest streams, ties to the most recently opened; priority and CU-masked streams keep queues of their own), for pools of 2 and 4, and
each hardware queue is a FIFO in host enqueue order in which a packet starts after the packets ahead of it have completed.  That rule
rests on the comment; it was not measured for this test.  A cycle under it would mean a bounded wait that has to expire.

Assertion 7 is about resources, not order, and is a model too.  A kernel that waits in-kernel holds its compute units while it waits; a
workgroup that asks for more than half of a compute unit's LDS sits there alone (the strip's 150 KB of 160: nothing else fits).  If one
launch has as many such waiters as the chip has compute units, whatever must still run to satisfy the wait finds none, and the bounded
wait expires -- the status word at INT_MAX.  Asserted: such waiters of one launch number at most the compute units minus 32, the
reserve potrf.hip keeps free of bulk work anyway (RESERVED_CUS).  The unmodified tree failed this at exactly the shapes of the open
item of NEXT.md section 5 and at none of the benchmark's: test_open_item_shapes.

What the checker was seen to catch (one mutation of potrf.hip at a time): profiles/potrf_schedule_check.txt."""
import collections
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpflow_amd", "csrc")
NB = 128
RESERVED_CUS = 32       # potrf.hip, aux_create: the compute units outside the bulk stream's mask
MAX_FLAG_PANELS = 512   # potrf_plan.h, kMaxFlagPanels: F[p] = flags[p], R[p] = flags[512 + p]

STATS = collections.Counter()   # logs, launches, pairs (unordered pairs of launches in one buffer whose rectangles were compared)


# ---- building and running the recorder ------------------------------------------------------------------------------------------
def build_runner(out_dir, csrc=CSRC, experimental=False):
    """g++ only; `csrc` may be a mutated copy of gpflow_amd/csrc (profiles/potrf_schedule_check.txt)"""
    exe = os.path.join(str(out_dir), "potrf_schedule_run" + ("_exp" if experimental else ""))
    cmd = ["g++", "-std=c++17", "-O1", "-w", "-I", os.path.join(ROOT, "tests", "hip_record"), "-I", csrc,
           '-DPOTRF_SRC="%s"' % os.path.join(csrc, "potrf.hip"), '-DDRIVERS_SRC="%s"' % os.path.join(csrc, "drivers.hip")]
    if experimental:
        cmd.append("-DGPK_EXPERIMENTAL")
    subprocess.run(cmd + [os.path.join(ROOT, "tests", "potrf_schedule_run.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="session")
def runners(tmp_path_factory):
    if shutil.which("g++") is None:   # (a toolchain the CPU tier has: without it the whole check would vanish quietly)
        pytest.fail("no g++: the schedule check cannot be built")
    out = tmp_path_factory.mktemp("potrf_schedule")
    yield {"product": build_runner(out), "exp": build_runner(out, experimental=True)}
    print("\npotrf schedule check: %(logs)d logs checked (%(identical)d more were identical to one of them), %(launches)d launches, "
          "%(pairs)d unordered pairs of launches in one buffer compared" % {k: STATS[k] for k in ("logs", "identical", "launches", "pairs")})


# hand-off modes: (build, environment of the A/B build, answer of the concurrency probe)
MODES = {
    "gate": ("product", {}, 1),                          # flag words, gate / set-flag kernels (the product)
    "streamops": ("exp", {"GPK_GATE_KERNELS": "0"}, 1),  # flag words, hipStreamWaitValue32 / hipStreamWriteValue32
    "events": ("exp", {"GPK_CHAIN_FLAGS": "0"}, 1),      # events only
    "noconc": ("product", {}, 0),                        # flags_usable = 0: kernels of two streams were not seen running together
}


def record(runners, entry, mode="gate", env=None, **kw):
    build, mode_env, conc = MODES[mode]
    if env:
        build = "exp"
    e = {k: v for k, v in os.environ.items() if not k.startswith("GPK_")}
    e.update(mode_env)
    e.update(env or {})
    args = [runners[build], entry, "conc=%d" % conc] + ["%s=%s" % kv for kv in kw.items()]
    out = subprocess.run(args, check=True, capture_output=True, text=True, env=e).stdout
    log = Log(json.loads(line) for line in out.splitlines())
    log.text = out
    return log


class Log(list):
    text = None


# ---- the happens-before relation ---------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("i", "s", "kind", "name", "desc", "call", "acc", "info", "preds", "sigsrc", "wait", "sig", "ev", "host", "wgs", "lds")

    def __init__(self, i, s, kind, name, desc, call, host):
        self.i, self.s, self.kind, self.name, self.desc, self.call, self.host = i, s, kind, name, desc, call, host
        self.acc, self.info, self.preds, self.sigsrc, self.wait, self.sig, self.ev = [], "none", [], [], None, None, None
        self.wgs = self.lds = 0

    def __str__(self):
        return "%s%s on stream %d (call %d, op %d)" % (self.name, " [%s]" % self.desc if self.desc else "", self.s, self.call, self.host)


class Schedule:
    """The log of one run as a graph.  lenient_entry: a signal on a kernel's entry also covers the kernel itself (the model this
    checker does NOT use; kept to show that the strict one is in force).  unordered_writes_on: stream kinds on which a
    hipStreamWriteValue32 is not ordered behind the work queued before it (the behaviour once seen on the CU-masked stream)."""

    def __init__(self, log, lenient_entry=False, unordered_writes_on=()):
        self.bufs = [o for o in log if o["k"] == "buf"]
        self.stream_kind = {}
        self.nodes = []
        self.problems = []   # (assertion number, message)
        last_sync = max([i for i, o in enumerate(log) if o["k"] == "host_sync"], default=-1)
        # What is dropped below as "completed before the host went on" may only be the init-time self-check, which comes before the first
        # fork (the first event record on the caller's stream).  A host synchronisation behind it would make this checker discard real work.
        first_fork = next((i for i, o in enumerate(log) if o["k"] == "record" and o["s"] == 0), len(log))
        assert last_sync < first_fork, "the enqueue code synchronises with the host behind its fork (log line %d): the checker must learn about it" % last_sync
        self.device = next((o for o in log if o["k"] == "device"), {"cus": 256, "lds": 163840})
        tail = {}            # stream -> last node
        last_record = {}     # event -> record node
        signals = collections.defaultdict(list)   # word -> [(value, source node)]
        waits = []
        call = -1
        self.calls = []
        for host, o in enumerate(log):
            k = o["k"]
            if k == "stream":
                self.stream_kind[o["s"]] = o["kind"]
                continue
            if k == "call":
                call = o["i"]
                self.calls.append(call)
                continue
            if k in ("buf", "call_end", "host_sync", "stream_destroy", "device"):
                continue
            s = o["s"]
            if host < last_sync and s != 0:
                continue   # completed before the host went on: the init-time self-check of the stream layout, on the internal streams

            def add(kind, name, desc=""):
                n = Node(len(self.nodes), s, kind, name, desc, call, host)
                self.nodes.append(n)
                if s in tail:
                    n.preds.append(tail[s])
                tail[s] = n
                return n

            if k == "launch":
                src = None
                if "sig" in o and o.get("sig_on_entry") and not lenient_entry:
                    src = add("entry", o["name"] + ".entry", o["desc"])
                n = add("launch", o["name"], o["desc"])
                n.acc = o["acc"]
                n.info = o["info"]
                n.wgs, n.lds = o.get("wgs", 0), o.get("lds", 0)
                if o.get("wait_dropped"):
                    self.problems.append((2, "lost hand-off: %s was asked to wait in-kernel but its kernel does not honour wait_ptr" % n))
                if "sig" in o:
                    src = src or n
                    src.sig = tuple(o["sig"])
                    signals[o["sig"][0]].append((o["sig"][1], src))
                if "wait" in o:
                    n.wait = tuple(o["wait"])
                    waits.append(n)
            elif k == "write_value":
                prev = tail.get(s)
                n = add("write_value", "hipStreamWriteValue32")
                n.sig = tuple(o["sig"])
                if self.stream_kind.get(s) in unordered_writes_on:   # the write floats: nothing before it, the stream goes on without it
                    n.preds = []
                    if prev is not None:
                        tail[s] = prev
                signals[o["sig"][0]].append((o["sig"][1], n))
            elif k == "wait_value":
                n = add("wait_value", "hipStreamWaitValue32")
                n.wait = tuple(o["wait"])
                waits.append(n)
            elif k == "record":
                n = add("record", "hipEventRecord(%d)" % o["ev"])
                last_record[o["ev"]] = n
            elif k == "wait_event":
                n = add("wait_event", "hipStreamWaitEvent(%d)" % o["ev"])
                r = last_record.get(o["ev"])
                if r is None:
                    self.problems.append((2, "lost hand-off: %s waits for an event that was never recorded" % n))
                elif r.call != n.call:
                    self.problems.append((2, "lost hand-off: %s binds to %s, a record of an earlier call" % (n, r)))
                else:
                    n.preds.append(r)
            else:
                raise ValueError(k)
        self.signals = signals
        for n in waits:
            word, v = n.wait
            sat = [(val, src) for val, src in signals.get(word, []) if _i32(val - v) >= 0]
            stale = [src for _, src in sat if src.call < n.call]
            own = [src for _, src in sat if src.call == n.call]
            for src in stale:
                self.problems.append((2, "lost hand-off: the signal %s of an earlier call satisfies the wait of %s for %s" % (src, n, self.word(word))))
            if not own:
                self.problems.append((2, "lost hand-off: %s waits for %s >= %d and no signal of its call satisfies it%s" %
                                      (n, self.word(word), v, self.strip_hint(n, word))))
            n.sigsrc = own
        self._close()

    # -- names for messages
    def word(self, ptr):
        for b in self.bufs:
            if b["name"] == "hipMalloc" and b["base"] <= ptr < b["base"] + b["bytes"]:
                i = (ptr - b["base"]) // 4
                return "F[%d]" % i if i < MAX_FLAG_PANELS else "R[%d]" % (i - MAX_FLAG_PANELS)
        return "word %d" % ptr

    def strip_hint(self, n, word):
        w = self.word(word)
        if n.kind == "launch" and n.name.startswith("gemm") and w.startswith("R["):
            return " (the waiting kernel is strip %d, the look-ahead update behind panel %d)" % (int(w[2:-1]) + 1, int(w[2:-1]) + 1)
        return ""

    # -- transitive closure (assertion 3 on the way)
    def _order(self, extra_preds=None):
        nodes = self.nodes
        indeg = [0] * len(nodes)
        succ = [[] for _ in nodes]
        for n in nodes:
            ps = n.preds + n.sigsrc + (extra_preds[n.i] if extra_preds else [])
            indeg[n.i] = len(ps)
            for p in ps:
                succ[p.i].append(n.i)
        ready = [i for i, d in enumerate(indeg) if d == 0]
        order = []
        while ready:
            i = ready.pop()
            order.append(i)
            for j in succ[i]:
                indeg[j] -= 1
                if indeg[j] == 0:
                    ready.append(j)
        if len(order) == len(nodes):
            return order, None
        # name one cycle: walk predecessors inside the unsorted remainder
        left = {i for i, d in enumerate(indeg) if d > 0}
        i = min(left)
        seen = []
        while i not in seen:
            seen.append(i)
            n = nodes[i]
            i = next(p.i for p in n.preds + n.sigsrc + (extra_preds[n.i] if extra_preds else []) if p.i in left)
        cyc = seen[seen.index(i):]
        return None, " <- ".join(str(nodes[c]) for c in cyc)

    def _close(self):
        order, cyc = self._order()
        self.anc = None
        self.order = order
        if order is None:
            self.problems.append((3, "cycle in stream order plus signal -> wait edges: " + cyc))
            return
        anc = [0] * len(self.nodes)
        for i in order:
            n = self.nodes[i]
            a = 0
            for p in n.preds:
                a |= anc[p.i] | (1 << p.i)
            if n.sigsrc:
                c = -1
                for p in n.sigsrc:
                    c &= anc[p.i] | (1 << p.i)
                a |= c
            anc[i] = a
        desc = [0] * len(self.nodes)
        if all(len(n.sigsrc) <= 1 for n in self.nodes):
            for i in reversed(order):
                d = desc[i] | (1 << i)
                n = self.nodes[i]
                for p in n.preds + n.sigsrc:
                    desc[p.i] |= d
        else:   # (a wait bound to several signals is not an edge: transpose the ancestor sets)
            for i in order:
                bit = 1 << i
                a = anc[i]
                while a:
                    low = a & -a
                    desc[low.bit_length() - 1] |= bit
                    a ^= low
        self.anc, self.desc = anc, desc

    def before(self, a, b):
        return bool(self.anc[b.i] >> a.i & 1)

    # -- assertion 1
    def buffer_of(self, ptr):
        for b in self.bufs:
            if b["base"] - 16 <= ptr < b["base"] + b["bytes"] + 16:
                return b
        raise ValueError("access outside every buffer: %d" % ptr)

    def conflicts(self):
        per_buf = collections.defaultdict(lambda: ({}, {}))   # buffer base -> (writes, reads): node index -> [(rw, base, rows, cols, ld)]
        for n in self.nodes:
            for rw, base, rows, cols, ld, batch, stride in n.acc:
                b = self.buffer_of(base)
                for z in range(batch):
                    per_buf[b["base"]][rw == "R"].setdefault(n.i, []).append((rw, base + z * stride, rows, cols, ld))
        out = []
        none = []
        for bbase, (writes, reads) in per_buf.items():
            wmask = amask = 0
            for i in writes:
                wmask |= 1 << i
            for i in reads:
                amask |= 1 << i
            amask |= wmask
            for i in sorted(set(writes) | set(reads)):
                wi, ri = writes.get(i, none), reads.get(i, none)
                # a writer meets everybody, a reader the writers; each unordered pair once
                cand = (amask if wi else wmask) & ~self.anc[i] & ~self.desc[i] & ~((1 << (i + 1)) - 1)
                while cand:
                    low = cand & -cand
                    cand ^= low
                    j = low.bit_length() - 1
                    STATS["pairs"] += 1
                    wj = writes.get(j, none)
                    hit = _first_overlap(wi, wj) or _first_overlap(wi, reads.get(j, none)) or _first_overlap(ri, wj)
                    if hit:
                        out.append((self.nodes[i], self.nodes[j], bbase, hit))
        return out

    def describe_conflict(self, a, b, bbase, hit):
        buf = next(x for x in self.bufs if x["base"] == bbase)
        (rwa, basea, rowsa, colsa, lda), (rwb, baseb, rowsb, colsb, ldb) = hit

        def rect(base, rows, cols, ld):
            off = base - bbase
            r, c = (off // ld, off % ld // 8) if rows > 1 else (0, off // 8)
            txt = "rows [%d, %d) x columns [%d, %d)" % (r, r + rows, c, c + cols // 8)
            if rows > 1:
                txt += " (leaf blocks %d..%d)" % (c // NB, (c + cols // 8 - 1) // NB)
            return txt
        return ("unordered conflict in buffer '%s': %s %s %s while %s %s %s" %
                (buf["name"], a, "writes" if rwa == "W" else "reads", rect(basea, rowsa, colsa, lda), b, "writes" if rwb == "W" else "reads",
                 rect(baseb, rowsb, colsb, ldb)))

    # -- assertion 6
    def hardware_queue(self, pool):
        queues = {0: 0}          # stream -> queue; the caller's stream is the default stream on queue 0
        shared = [[0]]           # the pool: streams per normal-priority queue, in the order the queues were opened
        own = 1000
        for s in sorted(self.stream_kind):
            kind = self.stream_kind[s]
            if kind == "caller":
                continue
            if kind in ("priority", "masked"):
                queues[s] = own
                own += 1
            elif len(shared) < pool:
                shared.append([s])
                queues[s] = len(shared) - 1
            else:
                fewest = min(len(q) for q in shared)
                q = max(i for i, x in enumerate(shared) if len(x) == fewest)
                shared[q].append(s)
                queues[s] = q
        return queues

    def queue_cycle(self, pool):
        queues = self.hardware_queue(pool)
        extra = [[] for _ in self.nodes]
        last = {}
        for n in self.nodes:   # (host enqueue order)
            q = queues[n.s]
            if q in last and last[q].s != n.s:
                extra[n.i].append(last[q])
            last[q] = n
        order, cyc = self._order(extra)
        return cyc


def _i32(x):
    x &= 0xffffffff
    return x - (1 << 32) if x & 0x80000000 else x


def _rect_overlap(a, b):
    """(rw, base, rows, cols, ld), bytes.  Exact for two rectangles of one pitch and for anything against a single row; the bounding
    intervals otherwise (which can only report a conflict that is none)."""
    _, ba, ra, ca, la = a
    _, bb, rb, cb, lb = b
    if ra == 1 or rb == 1:
        if rb == 1:
            ba, ca, bb, rb, cb, lb = bb, cb, ba, ra, ca, la
        # the interval [ba, ba + ca) against rb rows [bb + r lb, bb + r lb + cb): the rows that end behind ba and start before its end
        lo = max(0, (ba - bb - cb) // lb + 1)
        hi = min(rb - 1, (ba + ca - 1 - bb) // lb)
        return lo <= hi
    if la != lb:
        return ba < bb + (rb - 1) * lb + cb and bb < ba + (ra - 1) * la + ca
    d = bb - ba
    dr, dc = d // la, d % la
    pieces = [(dr, dc, min(cb, la - dc))]
    if dc + cb > la:
        pieces.append((dr + 1, 0, dc + cb - la))
    for r0, c0, w in pieces:
        if r0 < ra and r0 + rb > 0 and c0 < ca and w > 0:
            return True
    return False


def _first_overlap(mine, theirs):
    for a in mine:
        for b in theirs:
            if _rect_overlap(a, b):
                return a, b
    return None


def test_rectangle_overlap_against_enumeration():
    """the overlap test of assertion 1 against the byte sets themselves: exact for one pitch and for single rows, never a missed
    overlap otherwise"""
    import random
    rnd = random.Random(7)

    def cells(base, rows, cols, ld):
        return {base + r * ld + c for r in range(rows) for c in range(cols)}
    for _ in range(4000):
        lda = rnd.choice([5, 6, 8])
        ldb = lda if rnd.random() < 0.7 else rnd.choice([5, 6, 8])
        a = ("W", rnd.randrange(0, 40), rnd.randrange(1, 5), rnd.randrange(1, lda + 1), lda)
        b = ("R", rnd.randrange(0, 40), rnd.randrange(1, 5), rnd.randrange(1, ldb + 1), ldb)
        truth = bool(cells(*a[1:]) & cells(*b[1:]))
        got = _rect_overlap(a, b)
        if lda == ldb or a[2] == 1 or b[2] == 1:
            assert got == truth, (a, b)
        else:
            assert got or not truth, (a, b)


def check_log(log, expect=None, pools=(2, 4), **model):
    """All nine assertions on one log; returns the list of (assertion, message) that failed.  expect: launch name -> how often it
    must appear in EVERY call (the hooks: each non-empty one ran exactly once)."""
    sch = Schedule(log, **model)
    STATS["logs"] += 1
    STATS["launches"] += sum(1 for n in sch.nodes if n.kind == "launch")
    problems = list(sch.problems)
    if sch.anc is None:
        return problems
    for a, b, bbase, hit in sch.conflicts():
        problems.append((1, sch.describe_conflict(a, b, bbase, hit)))
    # successive signals on one word are ordered (what the binding of the waits leaves out rests on this)
    for word, sigs in sch.signals.items():
        for (_, s0), (_, s1) in zip(sigs, sigs[1:]):
            if s0.call != s1.call and not sch.before(s0, s1):
                problems.append((2, "lost hand-off: the signals %s and %s on %s are not ordered" % (s0, s1, sch.word(word))))
    # 4: the join
    markers = {n.call: n for n in sch.nodes if n.name == "caller_next"}
    resets = {}
    for n in sch.nodes:
        if n.call < 0 or n.name == "caller_next" or n.kind not in ("launch", "entry", "write_value"):
            continue   # (work only: a stream that merely waited for the fork has nothing to join)
        m = markers.get(n.call)
        if m is None or not sch.before(n, m):
            problems.append((4, "the join is incomplete: %s is not ordered before the caller's next launch on its stream" % n))
        if n.info == "reset":
            resets[n.call] = n
    for c in sch.calls:
        names = collections.Counter(n.name for n in sch.nodes if n.call == c and n.kind == "launch")
        for name, count in (expect or {}).items():
            if names[name] != count:
                problems.append((4, "call %d: %d launches of %s, expected %d" % (c, names[name], name, count)))
    # 5: the status word
    for n in sch.nodes:
        if n.info in ("may", "rmw"):
            r = resets.get(n.call)
            if r is None or not sch.before(r, n):
                problems.append((5, "status word: %s may write it and is not ordered behind the reset by the leaf of column 0 (%s)" % (n, r)))
            nxt = resets.get(n.call + 1)
            if nxt is not None and not sch.before(n, nxt):
                problems.append((5, "status word: %s of call %d is not ordered before the reset of the next call" % (n, n.call)))
    # 7: waiters leave compute units free (a model)
    room = sch.device["cus"] - RESERVED_CUS
    for n in sch.nodes:
        if n.kind == "launch" and n.wait and 2 * n.lds > sch.device["lds"] and n.wgs > room:
            problems.append((7, "%s waits in-kernel for %s with %d workgroups of %d KB of LDS, one per compute unit: more than the %d compute "
                                "units that leave %d free for what it waits for" % (n, sch.word(n.wait[0]), n.wgs, n.lds // 1024, room, RESERVED_CUS)))
    # 6: hardware queues (a model)
    for pool in pools:
        cyc = sch.queue_cycle(pool)
        if cyc:
            problems.append((6, "hardware-queue model, pool of %d: a wait that cannot be satisfied: %s" % (pool, cyc)))
    # 8: the whole extent of every access lies inside its buffer (buffer_of only places the access's first byte)
    inside = True
    for n in sch.nodes:
        for rw, base, rows, cols, ld, batch, stride in n.acc:
            b = sch.buffer_of(base)
            end = base + (batch - 1) * stride + (rows - 1) * ld + cols
            if base < b["base"] or end > b["base"] + b["bytes"]:
                inside = False
                problems.append((8, "out of bounds: %s %s [%d, %d) of buffer '%s', which has %d bytes" %
                                 (n, "writes" if rw == "W" else "reads", base - b["base"], end - b["base"], b["name"], b["bytes"])))
    # 9: the workspace contract of include/gpk.h, point (a), in the recorded model
    if inside:
        problems.extend(workspace_reads_are_written(sch))
    return problems


def workspace_reads_are_written(sch):
    """Assertion 9.  Within one call, every byte of the caller's workspace (the buffer the runner names 'ws') that a launch reads was
    written by a launch of the SAME call that happens-before it, or earlier in the access list of the reading launch itself (a stub
    lists its accesses in the kernel's own order: varexp_tail writes its block partials and then reads them, but reads the ticket before
    it writes it).  What an earlier call or the caller left in the workspace never counts: its contents at entry do not matter.
    The launches of a call are walked in one topological order of the happens-before relation.  Where assertion 1 holds, every write
    that overlaps a read is ordered against it, so the writes met before the reader in that order are exactly the ones that
    happen-before it.
    This is NECESSARY, NOT SUFFICIENT: a stub's write set may be a superset of what its kernel touches (lower_only builds declare the
    whole rectangle, padding rows and columns are never listed), so a kernel that reads what nobody wrote can pass here.
    tests/test_gpu_workspace.py, which poisons the real workspace on the device, is the real check.  Granularity: 8-byte words."""
    import numpy as np
    ws = next((b for b in sch.bufs if b["name"] == "ws"), None)
    if ws is None:
        return []
    lo, hi = ws["base"], ws["base"] + ws["bytes"]
    written = np.zeros((ws["bytes"] + 7) // 8, dtype=np.bool_)

    def words(base, rows, cols, ld, batch, stride):
        for z in range(batch):
            off = base + z * stride - lo
            w0, w1 = off // 8, (off + cols + 7) // 8
            if rows == 1:
                yield written[w0:w1]
            else:
                assert ld % 8 == 0, "a pitch inside the workspace that is no multiple of 8 bytes"
                yield np.lib.stride_tricks.as_strided(written[w0:], shape=(rows, w1 - w0), strides=(ld // 8, 1))

    problems = []
    for c in sch.calls:
        written[:] = False
        for i in sch.order:
            n = sch.nodes[i]
            if n.call != c or n.kind != "launch" or n.name.startswith("caller_"):
                continue
            for rw, base, rows, cols, ld, batch, stride in n.acc:
                if not lo <= base < hi:
                    continue
                for z, v in enumerate(words(base, rows, cols, ld, batch, stride)):
                    if rw == "W":
                        v[...] = True
                    elif not v.all():
                        r, w = np.argwhere(~np.atleast_2d(v))[0]
                        at = base + z * stride + int(r) * ld + 8 * int(w) - lo
                        problems.append((9, "workspace read before it is written: %s reads byte %d of 'ws' (entry %d, row %d of an access of "
                                            "%d rows x %d bytes at offset %d), which no launch of call %d that happens-before it has written"
                                         % (n, at, z, int(r), rows, cols, base - lo, c)))
                        break
    return problems


_CLEAN = set()   # logs already found clean, by their text and what was asked of them: two modes often enqueue the same thing


def assert_clean(log, tag, **kw):
    key = (hash(log.text), repr(sorted(kw.items())))
    if key in _CLEAN:
        STATS["identical"] += 1
        return
    problems = check_log(log, **kw)
    if not problems:
        _CLEAN.add(key)
    assert not problems, "%s: %d problems, first: assertion %d: %s" % (tag, len(problems), problems[0][0], problems[0][1])


# ---- what is swept -----------------------------------------------------------------------------------------------------------------
from test_potrf_plan import PINS, SWEEP_EXTRA, SWEEP_N   # noqa: E402  (the plan's own lists)

ALL_MODES = list(MODES)
POTRF_LAYOUTS = ["a", "p8", "odd"]


def sequence(log):
    """(stream, launch name) of every launch and stream operation of the LAST call, in host order"""
    last = max(o["i"] for o in log if o["k"] == "call")
    out, on = [], False
    for o in log:
        if o["k"] == "call":
            on = o["i"] == last
        elif o["k"] == "call_end":
            on = False
        elif on and "s" in o and o["k"] != "stream":
            out.append((o["s"], o.get("name", o["k"])))
    return out


# Every (mode, layout) pair up to n = 1152; from n = 2048 on, where a log costs 0.05 - 0.4 s to check, every mode on the aligned layout
# and every layout in the product's mode.  From n = 4095 on the extra rows are thinned to one value per regime of the plan (none, riding
# along, solved beside the chain below and above the rest_tiled threshold, the workload's 8192) and the batch of four keeps the product's
# mode only.  The pinned and open-item shapes below are never thinned.
FULL_COMBOS = [(m, la) for m in ALL_MODES for la in POTRF_LAYOUTS]
THIN_COMBOS = [(m, "a") for m in ALL_MODES] + [("gate", la) for la in POTRF_LAYOUTS if la != "a"]
LARGE_EXTRA = [0, 1, 257, 3000, 8192]


def potrf_sweep_cases():
    for n in SWEEP_N:
        large = n >= 4095
        for extra, batch in itertools.product(LARGE_EXTRA if large else SWEEP_EXTRA, [1, 4]):
            if large and batch > 1:
                combos = [("gate", "a")] if n < 16384 or extra in (1, 8192) else []
            elif n == 16384:
                combos = [c for c in THIN_COMBOS if c != ("noconc", "a") and c != ("gate", "p8")] if extra != 3000 else []
            else:
                combos = FULL_COMBOS if n <= 1152 else THIN_COMBOS if n < 4095 else [c for c in THIN_COMBOS if c != ("gate", "p8")]
            for mode, layout in combos:
                yield n, extra, batch, mode, layout


def test_sweep_potrf(runners):
    """SWEEP_N x SWEEP_EXTRA x batch {1, 4} of the plan's test in the hand-off modes and operand layouts (thinned as said above)"""
    for n, extra, batch, mode, layout in potrf_sweep_cases():
        log = record(runners, "potrf", mode, n=n, extra=extra, batch=batch, layout=layout, reps=2)
        assert_clean(log, ("potrf", n, extra, batch, mode, layout))


def test_sweep_potrf_inv_and_trsm(runners):
    """tri = n rows for potrf_inv; the solves against a cached factor (one stream: nothing to hand over, conflicts only)"""
    for n in SWEEP_N:
        for mode in ALL_MODES:
            for layout in ("a", "p8"):
                if n >= 4095 and (mode, layout) not in (("gate", "a"), ("events", "a"), ("gate", "p8")):
                    continue
                for extra in (0, 300):
                    assert_clean(record(runners, "potrf_inv", mode, n=n, extra=extra, layout=layout, reps=2), ("potrf_inv", n, extra, mode, layout))
    for n, m, batch in itertools.product([100, 640, 1152, 2048], [1, 300, 1040], [1, 3]):
        for entry in ("trsm0", "trsm1"):
            for layout in POTRF_LAYOUTS:
                assert_clean(record(runners, entry, n=n, extra=m, batch=batch, layout=layout, reps=2), (entry, n, m, batch, layout))


def test_pinned_plan_shapes(runners):
    """every shape of the plan's PINS, through gpk_potrf (tri = 0) or gpk_potrf_inv (tri = n)"""
    for (n, extra, batch, tri), *_ in PINS:
        for mode, layout in THIN_COMBOS:
            if layout != "p8":
                if tri:
                    log = record(runners, "potrf_inv", mode, n=n, extra=extra - tri, layout=layout, reps=2)
                else:
                    log = record(runners, "potrf", mode, n=n, extra=extra, batch=batch, layout=layout, reps=2)
                assert_clean(log, (n, extra, batch, tri, mode, layout))


def test_potrf_layout_rows(runners):
    """every shape of POTRF_ROWS (tests/test_gpu_potrf_layouts.py, where the device holds them to LAPACK layout by layout): every mode
    in every operand layout of the recorder"""
    from test_gpu_potrf_layouts import POTRF_ROWS
    for row in POTRF_ROWS:
        for mode, layout in FULL_COMBOS:
            if row.identity:
                log = record(runners, "potrf_inv", mode, n=row.n, extra=row.extra, layout=layout, zero_upper=int(row.zero_upper), reps=2)
            else:
                log = record(runners, "potrf", mode, n=row.n, extra=row.extra, batch=row.batch, layout=layout, zero_upper=int(row.zero_upper), reps=2)
            assert_clean(log, (row.id, mode, layout))


# (M, rows, P): shapes around the leaf, group and tail-zone edges, the contract rows of tests/test_gpu_contract.py that run on the
# factorisation's own streams, and the benchmark's driver shapes
DRIVER_SHAPES = [(100, 300, 1), (129, 77, 2), (200, 300, 3), (640, 300, 1), (640, 1040, 2), (640, 1040, 3), (1024, 8192, 1), (1024, 8192, 4), (1152, 1040, 1), (2048, 1024, 1),
                 (2048, 4096, 1), (2048, 8192, 1), (2048, 8192, 4)]
WHITE = {"kernel_matrix.sym": 1, "kernel_matrix.cross": 1, "kl_white_stage1": 1}


def test_sweep_drivers(runners):
    """the four forms of the shard, the likelihood shard and the separate-kernel shard: the hooks put the Kuu build on the panel
    stream, the Kfu build on the extra-row stream, the KL term on the rest-update stream.  (The drivers lay their own workspace out:
    ld is a multiple of 8 and every piece 256-byte aligned, so there is one layout.)"""
    for (m, rows, P), mode in itertools.product(DRIVER_SHAPES, ALL_MODES):
        tag = (m, rows, P, mode)
        for whiten, q_diag in ((1, 0), (1, 1), (0, 0), (0, 1)):
            expect = dict(WHITE) if whiten else {"kernel_matrix.sym": 1, "kernel_matrix.cross": 1}
            log = record(runners, "svgp", mode, n=m, rows=rows, P=P, whiten=whiten, q_diag=q_diag, reps=2)
            assert_clean(log, ("svgp", whiten, q_diag) + tag, expect=expect)
        assert_clean(record(runners, "svgp_lik", mode, n=m, rows=rows, P=P, reps=2), ("svgp_lik",) + tag, expect=WHITE)
        assert_clean(record(runners, "svgp_sep", mode, n=m, rows=rows, P=P, reps=2), ("svgp_sep",) + tag,
                     expect={"kernel_matrix.sym": P, "kernel_matrix.cross": P, "kl_white_stage1": 1})
    for n, P in itertools.product([100, 1024, 4096, 4500, 16384], [1, 4]):
        for mode in ALL_MODES:
            assert_clean(record(runners, "gpr_lml", mode, n=n, P=P, reps=2), ("gpr_lml", n, P, mode), expect={"kernel_matrix.sym": 1})


# (M, rows): the shapes of tests/test_gpu_workspace.py, where the device runs on a poisoned workspace -- one leaf block with padding
# columns (M % 8 = 4) and padding rows (rows % 32 != 0); two leaf blocks with the extra rows riding through the panels; the side
# schedule with a fused group solve
WORKSPACE_SHAPES = [(100, 300), (130, 40), (300, 333)]


def test_sweep_drivers_workspace_shapes(runners):
    """assertions 8 and 9 (and the rest) where the workspace layouts have padding: every driver the runner has, P = 1 and 3, two calls
    on one workspace"""
    for (m, rows), P, mode in itertools.product(WORKSPACE_SHAPES, (1, 3), ALL_MODES):
        tag = (m, rows, P, mode)
        for whiten, q_diag in ((1, 0), (1, 1), (0, 0), (0, 1)):
            assert_clean(record(runners, "svgp", mode, n=m, rows=rows, P=P, whiten=whiten, q_diag=q_diag, reps=2), ("svgp", whiten, q_diag) + tag)
            assert_clean(record(runners, "svgp_lik", mode, n=m, rows=rows, P=P, whiten=whiten, q_diag=q_diag, reps=2),
                         ("svgp_lik", whiten, q_diag) + tag)
        assert_clean(record(runners, "svgp_sep", mode, n=m, rows=rows, P=P, reps=2), ("svgp_sep",) + tag)
        assert_clean(record(runners, "gpr_lml", mode, n=m, P=P, reps=2), ("gpr_lml",) + tag)


def test_workspace_assertions_catch_what_they_are_for(runners):
    """8 and 9 on a log that was tampered with: a workspace 256 bytes shorter than the driver's layout, and a whitened shard without
    its kl_white_stage1 launch (whose kernel zeroes the ticket of the one-launch tail)"""
    log = record(runners, "svgp", "gate", n=300, rows=333, P=3, reps=2)
    assert not check_log(log)
    short = Log(dict(o, bytes=o["bytes"] - 256) if o["k"] == "buf" and o["name"] == "ws" else o for o in log)
    assert {a for a, _ in check_log(short)} == {8}
    no_kl = Log(o for o in log if not (o["k"] == "launch" and o["name"] == "kl_white_stage1"))
    found = [msg for a, msg in check_log(no_kl) if a == 9]
    assert found and all("varexp_tail" in msg or "final" in msg for msg in found), found
    assert any("varexp_tail" in msg for msg in found), found


def test_unwhitened_full_prefilled_and_not(runners):
    """the un-whitened full form: P = 1 skips the prefilled triangular rows (tri_prefilled), P = 2 does not"""
    for (m, rows), P, mode in itertools.product([(640, 300), (1152, 1040), (2048, 8192)], [1, 2], ALL_MODES):
        log = record(runners, "svgp", mode, n=m, rows=rows, P=P, whiten=0, q_diag=0, reps=2)
        assert_clean(log, ("unwhitened full", m, rows, P, mode), expect={"kernel_matrix.sym": 1, "kernel_matrix.cross": 1, "transpose": 3})


OPEN_ITEM = [("svgp_sep", dict(n=2048, rows=8192, P=4)), ("gpr_lml", dict(n=4500, P=4)), ("potrf", dict(n=4736, extra=1))]


@pytest.mark.parametrize("entry,shape", OPEN_ITEM, ids=["sep_2048x8192_P4", "gpr_lml_4500_P4", "potrf_4736_x1"])
def test_open_item_shapes(runners, entry, shape):
    """NEXT.md section 5, the calls that came back with the status word at INT_MAX: no lost hand-off, no unordered conflict and no
    cycle (hardware-queue model included) in any mode; gpk_potrf also in the unaligned layouts.  Three back-to-back calls."""
    for mode in ALL_MODES:
        for layout in (POTRF_LAYOUTS if entry == "potrf" else ["a"]):
            kw = dict(shape, layout=layout) if entry == "potrf" else shape
            assert_clean(record(runners, entry, mode, reps=3, **kw), (entry, shape, mode, layout))


@pytest.mark.parametrize("entry,shape", OPEN_ITEM, ids=["sep_2048x8192_P4", "gpr_lml_4500_P4", "potrf_4736_x1"])
def test_waiting_strips_leave_compute_units_free(runners, entry, shape):
    """What the sweep found (assertion 7): at these shapes the strips that wait in-kernel for "rest-update done" had 448, 226 and 249
    workgroups of 146 KB of LDS -- one per compute unit, on the high-priority stream, of 256 -- so a rest-update that was late found
    no compute unit to run on and the bounded wait expired.  gpk_potrf_core now keeps the waiters of one launch within the compute
    units of the bulk stream's mask (224); they walk their row blocks.  The shapes must still HAVE waiting strips, or this says nothing."""
    sch = Schedule(record(runners, entry, "gate", reps=2, **shape))
    waiting = [n for n in sch.nodes if n.kind == "launch" and n.wait and n.name == "gemm.small"]
    assert waiting and all(n.lds > 80 * 1024 for n in waiting)
    assert max(n.wgs for n in waiting) <= 256 - RESERVED_CUS, max(waiting, key=lambda n: n.wgs)
    assert max(n.wgs for n in waiting) > 200   # (the cap is in force here, not merely unneeded)


def test_dropped_rest_flag_is_a_lost_handoff(runners):
    """CPU counterpart of tests/test_gpu_handoff.py: with GPK_FAULT_DROP_REST_FLAG=1 (A/B build) the word R[1] is never written, and
    assertion 2 must say so, naming R[1] and strip 2"""
    log = record(runners, "potrf", "gate", env={"GPK_FAULT_DROP_REST_FLAG": "1"}, n=1024, extra=300, reps=2)
    lost = [msg for a, msg in check_log(log) if a == 2]
    assert lost and all("R[1]" in msg and "strip 2" in msg for msg in lost), lost
    assert_clean(record(runners, "potrf", "gate", env={"GPK_FAULT_DROP_REST_FLAG": "-1"}, n=1024, extra=300, reps=2), "exp build, nothing dropped")


def test_entry_signal_model_is_the_strict_one(runners):
    """a signal on entry must not be taken to cover its own kernel: the schedule passes under either reading today, and the strict
    one is the one in force (an edge count shows the two models differ)"""
    log = record(runners, "potrf", "gate", n=2048, extra=8192, reps=2)
    strict, lenient = Schedule(log), Schedule(log, lenient_entry=True)
    assert any(n.kind == "entry" for n in strict.nodes) and not any(n.kind == "entry" for n in lenient.nodes)
    assert not check_log(log) and not check_log(log, lenient_entry=True)


# ---- pinned sequences ----------------------------------------------------------------------------------------------------------------
def _runs(seq):
    """run-length form: [(stream, name, count)], consecutive repeats folded"""
    out = []
    for s, name in seq:
        if out and out[-1][:2] == (s, name):
            out[-1] = (s, name, out[-1][2] + 1)
        else:
            out.append((s, name, 1))
    return out


PIN_DIR = os.path.join(ROOT, "tests", "golden")
HEADLINES = {
    "potrf_2048x8192": ("potrf", dict(n=2048, extra=8192, zero_upper=0)),
    "svgp_whitened_2048x8192": ("svgp", dict(n=2048, rows=8192, P=1)),
    "svgp_sep_2048x8192_P4": ("svgp_sep", dict(n=2048, rows=8192, P=4)),
    "gpr_lml_16384": ("gpr_lml", dict(n=16384, P=1)),
}


@pytest.mark.parametrize("name", sorted(HEADLINES))
def test_pinned_sequences(runners, name):
    """the (stream, launch name) sequence of the four headline calls (second call of two: the steady state), so that a change of the
    schedule shows up as a diff of tests/golden/potrf_schedule_<name>.txt.  Streams: 0 caller, 1 panel, 2 extra rows, 4 rest-updates,
    5 masked bulk."""
    entry, shape = HEADLINES[name]
    seq = sequence(record(runners, entry, "gate", reps=2, **shape))
    text = "".join("%d %s\n" % p for p in seq)
    path = os.path.join(PIN_DIR, "potrf_schedule_%s.txt" % name)
    with open(path) as f:
        want = f.read()
    if text != want:
        import difflib
        diff = "".join(itertools.islice(difflib.unified_diff(want.splitlines(True), text.splitlines(True), "pinned", "now"), 60))
        raise AssertionError("the schedule of %s changed:\n%s" % (name, diff))
