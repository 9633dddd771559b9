"""Times of the ChangePoints tile kernels beside the torch compositions they replace, at one shape, in one process on one device:
device events around `reps` back-to-back calls, the sides alternating over `rounds` rounds, the median and the spread per side, and
the rate of the traffic that bounds the two kernels (fold op 1: Ki and acc read, out written -- 3 passes; the stage: Kbar and Ki read,
G written -- 3 passes and the partials).

  (a) gpk_changepoint_fold op 1           against  out += (a[:, None] * Ki) * b[None, :]          (three torch calls)
  (b) one gpk_changepoint_adjoint_stage   against  G = (Kbar * a[:, None]) * b[None, :];  E = Kbar * Ki;  E @ b;  a @ E
  (c) ChangePoints.K of T members whole   against  Sum of the same members (the floor: the members built and added in place)
  and the tail (two launches) once per argument, after T stage calls.

    python tools/changepoints_probe.py [--n 8192] [--members 3] [--reps 20] [--rounds 5]

Needs the device; there is no CPU path.  DESIGN §6 "ChangePoints kernel" records what it printed.
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
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import gpflow_amd as gpflow
    from gpflow_amd import ops
    K = gpflow.kernels
    dev = ops.device()
    rng = np.random.default_rng(1)
    n, T = a.n, a.members
    X1, X2 = ops.to_device(rng.uniform(-1, 1, size=(n, 3))), ops.to_device(rng.uniform(-1, 1, size=(n, 3)))
    loc, st = np.linspace(-0.5, 0.5, T - 1), np.full(T - 1, 4.0)
    A, B = ops.changepoint_weights(X1[:, 0], locations=loc, steepness=st), ops.changepoint_weights(X2[:, 0], locations=loc, steepness=st)
    Ki, Kbar = ops.to_device(rng.normal(size=(n, n))), ops.to_device(rng.normal(size=(n, n)))
    out, G = torch.zeros((n, n), dtype=torch.float64, device=dev), torch.empty((n, n), dtype=torch.float64, device=dev)
    parts = ops.changepoint_adjoint_parts(T, n, n, dev)
    members = [K.SquaredExponential(lengthscales=0.3 + 0.2 * i) for i in range(T)]
    cp, plain = K.ChangePoints(members, loc, st), K.Sum(members)
    a0, b0 = A[1], B[1]

    def torch_fold():
        t = Ki * a0[:, None]
        t *= b0[None, :]
        out.add_(t)

    def torch_stage():
        g = Kbar * a0[:, None]
        g *= b0[None, :]
        e = Kbar * Ki
        return g, e @ b0, a0 @ e

    def tails():
        kw = dict(locations=loc, steepness=st, parts=parts)
        ops.changepoint_adjoint_tail(X1[:, 0], n_other=n, columns=False, **kw)
        ops.changepoint_adjoint_tail(X2[:, 0], n_other=n, columns=True, **kw)
    sides = {
        "(a) changepoint_fold op 1": (lambda: ops.changepoint_fold(a0, b0, Ki, out, out=out), 3),
        "(a) torch: mul, mul, add": (torch_fold, None),
        "(b) changepoint_adjoint_stage": (lambda: ops.changepoint_adjoint_stage(a0, b0, Kbar, Ki, parts[1], out=G), 3),
        "(b) torch: mul, mul, mul, 2 matvec": (torch_stage, None),
        f"(c) ChangePoints.K, {T} members": (lambda: cp.K_into(X1, X2, out), None),
        f"(c) Sum.K, {T} members": (lambda: plain.K_into(X1, X2, out), None),
        "tail, both arguments": (tails, None),
    }
    for i in range(T):
        ops.changepoint_adjoint_stage(A[i], B[i], Kbar, Ki, parts[i], out=G)
    times = {name: [] for name in sides}
    for name, (f, _) in sides.items():      # warm-up: code objects, the allocator's blocks
        f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, (f, _) in sides.items():
            out.zero_()                     # (the folds add in place: keep the values finite over the window)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    unit = n * n * 8
    print(f"n1 = n2 = {n}, T = {T}, {a.reps} calls per window, {a.rounds} rounds, microseconds per call")
    for name, ts in times.items():
        med = statistics.median(ts)
        passes = sides[name][1]
        rate = "" if passes is None else f"   {unit * passes / med / 1e6:7.2f} TB/s of its {unit * passes >> 20} MB"
        print(f"{name:38s} median {med:9.1f}  min {min(ts):9.1f}  max {max(ts):9.1f}{rate}")


if __name__ == "__main__":
    main()
