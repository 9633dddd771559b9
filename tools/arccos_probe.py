"""Times of the ArcCosine builder and adjoint stage beside the Polynomial(degree=3) builder and its `ds` pass at one shape, in one
process on one device: device events around `reps` back-to-back launches, the sides alternating over `rounds` rounds, the median and
the spread per side, and the rate of the output write (n1 n2 8 bytes; the stage also reads Kbar) that bounds them.

    python tools/arccos_probe.py [--n 8192] [--d 8] [--reps 20] [--rounds 5]

Needs the device; there is no CPU path.  DESIGN §6 "ArcCosine kernel" records what it printed.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from gpflow_amd import ops
    dev = ops.device()
    rng = np.random.default_rng(1)
    X1, X2 = ops.to_device(rng.uniform(-1, 1, size=(a.n, a.d))), ops.to_device(rng.uniform(-1, 1, size=(a.n, a.d)))
    out = torch.empty((a.n, a.n), dtype=torch.float64, device=dev)
    Kbar = ops.to_device(rng.normal(size=(a.n, a.n)))
    parts = ops.arccos_adjoint_parts(a.n, a.n, dev)
    poly = dict(family="Polynomial", variance=1.3, offset=0.3, degree=3)
    sides = {"Polynomial(3) build": lambda: ops.dot_kernel_matrix(X1, X2, out=out, **poly),
             "Polynomial(3) ds pass": lambda: ops.dot_kernel_matrix_combine(X1, X2, Kbar, op="ds", out=out, **poly)}
    for order in (0, 1, 2):
        kw = dict(order=order, variance=0.8, weight_variances=1.3, bias_variance=0.7)
        sides[f"ArcCosine({order}) build"] = lambda kw=kw: ops.arccos_kernel_matrix(X1, X2, out=out, **kw)
        sides[f"ArcCosine({order}) adjoint stage"] = lambda kw=kw: ops.arccos_adjoint_stage(X1, X2, Kbar, parts, out=out, **kw)
    times = {name: [] for name in sides}
    for name, f in sides.items():      # warm-up: code objects, the LDS attribute
        f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    wr = a.n * a.n * 8
    print(f"n1 = n2 = {a.n}, d = {a.d}, {a.reps} launches per window, {a.rounds} rounds, microseconds per launch")
    for name, ts in times.items():
        med = statistics.median(ts)
        traffic = wr * (2 if ("stage" in name or "ds" in name) else 1)
        print(f"{name:32s} median {med:9.1f}  min {min(ts):9.1f}  max {max(ts):9.1f}   {traffic / med / 1e6:7.2f} TB/s of its {traffic >> 20} MB")


if __name__ == "__main__":
    main()
