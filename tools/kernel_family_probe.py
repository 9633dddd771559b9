"""Builder time of every kernel family: `ops.kernel_matrix` for all eight families in ONE process (same device, same clocks, same
neighbours), SquaredExponential the yardstick of the same run.

  --shape sym     K(X, X), 16384 x 16384, d = 8  (the mirror-tile build: lower tiles computed, written twice)
  --shape cross   K(X, Z), 8192 x 2048, d = 8

Rounds alternate over the families (family 0 .. 7, then again), every family warmed up first, each timed call bracketed by device
events.  Prints one JSON line: per family the median / min / max of the calls in microseconds and the ratio of its median to the
SquaredExponential's; `repeat_SquaredExponential` is the yardstick measured a second time at the end of the same process -- the
spread to read a difference against.  For the kernels' own times put the process under `rocprofv3 --kernel-trace --stats` in a run
of its own (one shape per run: every family is its own instantiation rbf_kernel<FAMILY, 0>, so the per-kernel statistics are the
per-family times).

    python tools/kernel_family_probe.py --shape sym [--rounds 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflow_amd import ops  # noqa: E402

FAMILIES = ["SquaredExponential", "Matern12", "Matern32", "Matern52", "Exponential", "RationalQuadratic", "White", "Constant"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["sym", "cross"], default="sym")
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    d = 8
    n1, n2 = (16384, None) if args.shape == "sym" else (8192, 2048)
    X1 = ops.to_device(rng.normal(size=(n1, d)))
    X2 = None if n2 is None else ops.to_device(rng.normal(size=(n2, d)))
    out = torch.empty((n1, n1 if n2 is None else n2), dtype=torch.float64, device=X1.device)
    ls = float(np.sqrt(d))

    def build(family):
        return ops.kernel_matrix(X1, X2, variance=1.3, lengthscales=ls, family=family, out=out,
                                 alpha=1.0 if family == "RationalQuadratic" else None)

    def timed(family):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        build(family)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3

    for family in FAMILIES:
        for _ in range(3):
            build(family)
    torch.cuda.synchronize()
    times = {f: [] for f in FAMILIES}
    for _ in range(args.rounds):
        for family in FAMILIES:
            times[family].append(timed(family))
    repeat = [timed("SquaredExponential") for _ in range(args.rounds)]
    stat = lambda v: {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}  # noqa: E731
    res = {"shape": args.shape, "n1": n1, "n2": n2 if n2 is not None else n1, "d": d, "rounds": args.rounds,
           "bytes_written": int(out.numel()) * 8}
    se = float(np.median(times["SquaredExponential"]))
    for family in FAMILIES:
        res[family] = dict(stat(times[family]), ratio_to_se=float(np.median(times[family])) / se)
    res["repeat_SquaredExponential"] = stat(repeat)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
