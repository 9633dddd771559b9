"""Cost of the MultiClass (RobustMax) likelihood stage beside the Bernoulli one, and of the fused shard with it.  Device events
around back-to-back calls, interleaved rounds of ONE process (same device, same clocks, same neighbours):

  * stage: ops.likelihood_varexp_sum on 8192 rows x 10 latents -- "multiclass_robustmax" (C = 10, one label column) and
    "bernoulli_probit" (P = 10 label columns).  Both evaluate 8192 x 10 x 20 erfc / exp nodes.  A call is the stage-1 kernel and
    the two one-block final sums, plus the wrapper's host work; the host clock around the same calls (enqueue only) is printed
    beside the event time so that a host-bound figure shows as one.
  * step: ops.svgp_elbo_shard_lik at M = 1024, B = 8192, D = 8, C = 10, diagonal q_sqrt, whitened, with either likelihood.

Prints one JSON line: median and min per call of each.

    python tools/multiclass_stage_probe.py [--rounds 7] [--calls 200] [--steps 60]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=60)
    args = ap.parse_args()
    device = ops.device()
    rng = np.random.default_rng(0)
    rows, C, M, D = 8192, 10, 1024, 8
    t = ops.to_device
    F, s0, ssq = t(rng.normal(size=(rows, C)) * 1.5), t(rng.uniform(0, 0.5, size=rows)), t(rng.uniform(0, 0.6, size=(C, rows)))
    Ymc = t(rng.integers(0, C, size=(rows, 1)).astype(np.float64))
    Ybe = t((rng.uniform(size=(rows, C)) < 0.5).astype(np.float64))
    stage = {
        "multiclass_robustmax": lambda: ops.likelihood_varexp_sum(Ymc, F, s0=s0, ssq=ssq, knn=[1.2], lik="multiclass_robustmax",
                                                                  params=(1e-3,)),
        "bernoulli_probit": lambda: ops.likelihood_varexp_sum(Ybe, F, s0=s0, ssq=ssq, knn=[1.2], lik="bernoulli_probit"),
    }
    X = t(rng.normal(size=(rows, D)))
    Z = t(X[:M].cpu().numpy() + 0.05 * rng.normal(size=(M, D)))
    q_mu, q_sqrt = t(0.4 * rng.normal(size=(M, C))), t(rng.uniform(0.3, 0.9, size=(M, C)))
    ws = ops.svgp_elbo_workspace(M, rows, D, C, True, True)
    out = torch.empty(2, dtype=torch.float64, device=device)
    info = torch.zeros(1, dtype=torch.int32, device=device)

    def shard(lik, par, Y):
        return lambda: ops.svgp_elbo_shard_lik(Z, X, Y, q_mu, q_sqrt, variance=1.3, lengthscales=float(np.sqrt(D)), lik=lik, params=par,
                                               jitter=1e-6, ws=ws, out=out, info=info)
    step = {"multiclass_robustmax": shard("multiclass_robustmax", (1e-3,), Ymc), "bernoulli_probit": shard("bernoulli_probit", (), Ybe)}

    def timed(fn, n):
        """(device ms per call by events, host ms per call spent enqueueing)"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        h0 = time.perf_counter()
        for _ in range(n):
            fn()
        h1 = time.perf_counter()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n, (h1 - h0) / n * 1e3

    rec = {"rows": rows, "latents": C, "m": M, "d": D, "rounds": args.rounds}
    for label, fns, n in (("stage", stage, args.calls), ("step", step, args.steps)):
        for fn in fns.values():          # warm-up: code objects, workspaces, clocks
            timed(fn, max(10, n // 4))
        got = {name: [] for name in fns}
        for _ in range(args.rounds):
            for name, fn in fns.items():
                got[name].append(timed(fn, n))
        for name, v in got.items():
            ev, host = np.array(v).T
            rec[f"{label}_{name}"] = {"median_us": float(np.median(ev) * 1e3), "min_us": float(ev.min() * 1e3),
                                      "host_enqueue_median_us": float(np.median(host) * 1e3), "calls_per_round": n}
    assert int(info.cpu()[0]) == 0 and bool(torch.isfinite(out).all())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
