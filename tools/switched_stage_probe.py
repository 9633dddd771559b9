"""Cost of the switched variational-expectation stage beside the composition it replaces: rows = 65536, P = 1, T = 4,
[Gaussian, StudentT, Bernoulli, Poisson], every call with the gradients (dmu, dvar and the per-task parameter sums).

  switched_sorted / switched_round_robin   ONE ops.switched_varexp_sum call, the rows stacked task by task / task = row mod 4
  composed                                 what the stage replaces, from the primitives that existed before it: partition the rows by
                                           index_select (Y, fmean, s0, ssq), one ops.gaussian_varexp_sum plus three
                                           ops.likelihood_varexp_sum(want_grads=True), the Gaussian member's dmu / dvar / d/ds2 as
                                           elementwise glue, index_copy_ of dmu and dvar back into row order, the four sums added
                                           (the row partition -- the index lists -- is made once, outside the timed calls)

All of them in interleaved rounds of ONE process (same device, same clocks, same neighbours), the same warm-up, device events around
`--calls` calls, medians over `--rounds` rounds with min and max as the spread; the host clock around the same calls (enqueue only) is
printed beside the event time so that a host-bound figure shows as one.  The results of the three are compared first (out[0] within
1e-9 relative; dmu, dvar of the sorted and round-robin runs bit-identical after un-permuting).

Prints one JSON line.

    python tools/switched_stage_probe.py [--rounds 9] [--calls 50] [--rows 65536]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflow_amd import ops  # noqa: E402

MEMBERS = [("gaussian", (0.6,)), ("student_t", (0.8, 3.0)), ("bernoulli_probit", ()), ("poisson_exp", (0.7,))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rows", type=int, default=65536)
    args = ap.parse_args()
    dev = ops.device()
    rng = np.random.default_rng(0)
    rows, T = args.rows, len(MEMBERS)
    task = np.repeat(np.arange(T), rows // T)
    rows = task.size
    y = np.where(task == 2, (rng.uniform(size=rows) < 0.5).astype(np.float64),
                 np.where(task == 3, rng.poisson(3.0, size=rows).astype(np.float64), rng.normal(size=rows) * 1.5))
    F = rng.normal(size=(rows, 1)) * np.where(task == 3, 0.7, 1.5)[:, None]
    s0, ssq = rng.uniform(0, 0.5, size=rows), rng.uniform(0, 0.6, size=(1, rows))
    Y = np.stack([y, task.astype(np.float64)], axis=1)
    rr = np.argsort(np.arange(rows) % (rows // T) * T + task, kind="stable")      # the same rows, task = position mod 4
    assert (task[rr][:8] == np.arange(8) % T).all()
    t = ops.to_device

    def operands(order):
        return t(Y[order]), t(F[order]), t(s0[order]), t(np.ascontiguousarray(ssq[:, order]))
    sorted_ops, rr_ops = operands(np.arange(rows)), operands(rr)

    def switched(o):
        return ops.switched_varexp_sum(o[0], o[1], s0=o[2], ssq=o[3], knn=[1.2], members=MEMBERS, want_grads=True)

    # the composition, on the round-robin rows (sorted rows would make the partition a no-op)
    Yd, Fd, s0d, ssqd = rr_ops
    idx = [torch.nonzero(Yd[:, 1].long() == k).reshape(-1) for k in range(T)]

    def composed():
        dmu, dvar = torch.empty_like(Fd), torch.empty_like(Fd)
        total, grads = None, []
        for k, (name, par) in enumerate(MEMBERS):
            i = idx[k]
            Yk, Fk = Yd.index_select(0, i), Fd.index_select(0, i)
            s0k, ssqk = s0d.index_select(0, i), ssqd.index_select(1, i)
            if name == "gaussian":
                s2 = par[0]
                out, fv = ops.gaussian_varexp_sum(Yk[:, :1], Fk, s0=s0k, ssq=ssqk, knn=[1.2], noise_variance=s2, want_fvar=True)
                dy = Yk[:, :1] - Fk
                dm, dv = dy / s2, torch.full_like(Fk, -0.5 / s2)
                grads.append((-0.5 / s2 + 0.5 * (dy * dy + fv) / (s2 * s2)).sum().reshape(1))
                ve = out[0:1]
            else:
                out, _, dm, dv, _ = ops.likelihood_varexp_sum(Yk[:, :1], Fk, s0=s0k, ssq=ssqk, knn=[1.2], lik=name, params=par,
                                                              want_grads=True)
                ve = out[0:1]
                grads.append(out[1:2])
            dmu.index_copy_(0, i, dm)
            dvar.index_copy_(0, i, dv)
            total = ve if total is None else total + ve
        return torch.cat([total] + grads), None, dmu, dvar, None

    fns = {"switched_sorted": lambda: switched(sorted_ops), "switched_round_robin": lambda: switched(rr_ops), "composed": composed}

    # the three compute the same thing
    res = {k: [None if r is None else r.cpu().numpy() for r in fn()] for k, fn in fns.items()}
    a, b, c = res["switched_sorted"], res["switched_round_robin"], res["composed"]
    inv = np.argsort(rr)
    same_bits = all(np.array_equal(a[i].view(np.uint64), b[i][inv].view(np.uint64)) for i in (2, 3))
    agree = float(np.max(np.abs(b[0] - c[0]) / np.maximum(1.0, np.abs(c[0]))))
    agree_el = float(max(np.abs(b[2] - c[2]).max(), np.abs(b[3] - c[3]).max()))

    def timed(fn, n):
        """(device ms per call by events, host ms per call spent enqueueing)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        h0 = time.perf_counter()
        for _ in range(n):
            fn()
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n, (h1 - h0) / n * 1e3

    rec = {"rows": rows, "P": 1, "members": [m for m, _ in MEMBERS], "rounds": args.rounds, "calls_per_round": args.calls,
           "device": str(dev), "sorted_vs_round_robin_elements_bit_identical": bool(same_bits),
           "switched_vs_composed_out_max_rel": agree, "switched_vs_composed_dmu_dvar_max_abs": agree_el}
    for fn in fns.values():          # warm-up: code objects, allocator, clocks
        timed(fn, max(10, args.calls // 2))
    got = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            got[name].append(timed(fn, args.calls))
    for name, v in got.items():
        ev, host = np.array(v).T
        rec[name] = {"median_us": round(float(np.median(ev) * 1e3), 2), "min_us": round(float(ev.min() * 1e3), 2),
                     "max_us": round(float(ev.max() * 1e3), 2), "host_enqueue_median_us": round(float(np.median(host) * 1e3), 2)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
