"""Cost of the variational-expectation stage of the Exponential / Gamma / Beta / Ordinal likelihood codes beside Bernoulli and
Poisson: ops.likelihood_varexp_sum at 8192 rows x 1 latent and 8192 x 16, all six codes in interleaved rounds of ONE process (same
device, same clocks, same neighbours).  A call is the stage-1 kernel and the two one-block final sums plus the wrapper's host work;
the host clock around the same calls (enqueue only) is printed beside the event time so that a host-bound figure shows as one.  For
the stage-1 KERNEL times run this file under `rocprofv3 --kernel-trace --stats` (the instantiations of lik_varexp_kernel carry the
code in their names: <1> Bernoulli, <2> Poisson, <8> Exponential, <9> Gamma, <10> Beta, <11> Ordinal).

Prints one JSON line: median and min per call of each (code, P).

    python tools/likelihood_zoo_stage_probe.py [--rounds 7] [--calls 100]
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
    ap.add_argument("--calls", type=int, default=100)
    args = ap.parse_args()
    ops.device()
    rng = np.random.default_rng(0)
    rows = 8192
    t = ops.to_device
    edges = (-1.1, -0.3, 0.2, 0.9, 1.7)
    liks = {"bernoulli_probit": ((), lambda s: (rng.uniform(size=s) < 0.5).astype(np.float64), 1.5),
            "poisson_exp": ((1.0,), lambda s: rng.poisson(3.0, size=s).astype(np.float64), 0.7),
            "exponential_exp": ((), lambda s: rng.exponential(size=s), 0.7),
            "gamma_exp": ((1.7,), lambda s: rng.gamma(2.0, size=s), 0.7),
            "beta_probit": ((2.5,), lambda s: rng.beta(2, 3, size=s), 1.5),
            "ordinal": ((0.6, 5.0) + edges, lambda s: rng.integers(0, 6, size=s).astype(np.float64), 1.5)}
    fns = {}
    for P in (1, 16):
        s0, ssq = t(rng.uniform(0, 0.5, size=rows)), t(rng.uniform(0, 0.6, size=(P, rows)))
        for name, (par, labels, spread) in liks.items():
            Y, F = t(labels((rows, P))), t(rng.normal(size=(rows, P)) * spread)
            fns[f"{name}_P{P}"] = (lambda Y=Y, F=F, s0=s0, ssq=ssq, name=name, par=par:
                                   ops.likelihood_varexp_sum(Y, F, s0=s0, ssq=ssq, knn=[1.2], lik=name, params=par))

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

    rec = {"rows": rows, "rounds": args.rounds, "calls_per_round": args.calls}
    for fn in fns.values():          # warm-up: code objects, workspaces, clocks
        assert bool(torch.isfinite(fn()[0]).all())
        timed(fn, max(10, args.calls // 4))
    got = {name: [] for name in fns}
    for _ in range(args.rounds):
        for name, fn in fns.items():
            got[name].append(timed(fn, args.calls))
    for name, v in got.items():
        ev, host = np.array(v).T
        rec[name] = {"median_us": round(float(np.median(ev) * 1e3), 2), "min_us": round(float(ev.min() * 1e3), 2),
                     "host_enqueue_median_us": round(float(np.median(host) * 1e3), 2)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
