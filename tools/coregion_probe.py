"""Times of the Coregion builder, its `mul` fold and its whole adjoint at P = 3 and P = 64 beside the Linear builder and fold at d = 1
(the same global writes and no more reads) at one shape, in one process on one device: device events around `reps` back-to-back
launches, the sides alternating over `rounds` rounds, the median and the spread per side, and the rate of the traffic that bounds
them (the build writes n1 n2 8 bytes; the fold reads and writes them; the adjoint reads Kbar once).  The adjoint's first contraction is
timed in both orientations: Kbar E2^T with the small transpose it then needs (taken by gradients.coregion_kernel_adjoint) and E2 Kbar^T.

    python tools/coregion_probe.py [--n 8192] [--reps 20] [--rounds 5]

Needs the device; there is no CPU path.  DESIGN §6 "Coregion kernel" records what it printed.
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    from gpflow_amd import gradients, ops
    from gpflow_amd.leaf import CoregionLeaf
    dev = ops.device()
    rng = np.random.default_rng(1)
    n = a.n
    out = torch.empty((n, n), dtype=torch.float64, device=dev)
    Kbar = ops.to_device(rng.normal(size=(n, n)))
    X1, X2 = ops.to_device(rng.uniform(-1, 1, size=(n, 1))), ops.to_device(rng.uniform(-1, 1, size=(n, 1)))
    lin = dict(family="Linear", variance=0.8)
    sides = {"Linear(d=1) build": (lambda: ops.dot_kernel_matrix(X1, X2, out=out, **lin), 1),
             "Linear(d=1) mul fold": (lambda: ops.dot_kernel_matrix_combine(X1, X2, out, op="mul", out=out, **lin), 2)}
    for P in (3, 64):
        R = 2 if P == 3 else 64
        leaf = CoregionLeaf(0.1 + 0.5 * rng.normal(size=(P, R)), rng.uniform(0.5, 1.5, size=P))
        L1 = ops.to_device(rng.integers(0, P, size=(n, 1)).astype(np.float64))
        L2 = ops.to_device(rng.integers(0, P, size=(n, 1)).astype(np.float64))
        kw = leaf.keywords()

        def other_orientation(leaf=leaf, L1=L1, L2=L2, P=P):
            E1, E2 = ops.coregion_onehot_rows(L1, P), ops.coregion_onehot_rows(L2, P)
            Tt = gradients.splitk_gemm_nt(E2, Kbar)                      # [P, n1]
            return ops.coregion_adjoint_tail(ops.gemm_nt(E1, Tt), W=leaf.W)
        sides[f"Coregion(P={P}) build"] = (lambda L1=L1, L2=L2, kw=kw: ops.coregion_kernel_matrix(L1, L2, out=out, **kw), 1)
        sides[f"Coregion(P={P}) mul fold"] = (lambda L1=L1, L2=L2, kw=kw: ops.coregion_kernel_matrix_combine(L1, L2, out, op="mul", out=out, **kw), 2)
        sides[f"Coregion(P={P}) adjoint"] = (lambda leaf=leaf, L1=L1, L2=L2: gradients.coregion_kernel_adjoint(leaf, L1, L2, Kbar, symmetric=False), 1)
        sides[f"Coregion(P={P}) adjoint, E2 Kbar^T"] = (other_orientation, 1)
    times = {name: [] for name in sides}
    out.fill_(1.0)
    for name, (f, _) in sides.items():      # warm-up: code objects, the LDS attribute, the cached B
        f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (f, _) in sides.items():
            out.fill_(1.0)                  # (the folds multiply in place: keep the values finite over the window)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    unit = n * n * 8
    print(f"n1 = n2 = {n}, {a.reps} launches per window, {a.rounds} rounds, microseconds per call")
    for name, ts in times.items():
        med = statistics.median(ts)
        traffic = unit * sides[name][1]
        print(f"{name:36s} median {med:9.1f}  min {min(ts):9.1f}  max {max(ts):9.1f}   {traffic / med / 1e6:7.2f} TB/s of its {traffic >> 20} MB")


if __name__ == "__main__":
    main()
