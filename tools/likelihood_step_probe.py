"""Step cost of a non-Gaussian likelihood: the Cm ELBO step (M 2048, 8192 rows, D 8; bench.py's shapes, inputs and mailbox
protocol) with the Bernoulli quadrature stage beside the same step with the Gaussian stage, in interleaved rounds of ONE process
(same device, same clocks, same neighbours).  The likelihood stage is the only difference between the two.  Prints one JSON line:
median and min ms per step of either, and their ratio.

    python tools/likelihood_step_probe.py [--rounds 12] [--steps 40] [--lik bernoulli_probit|poisson_exp|student_t]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (make_inputs, WORKLOADS: the benchmark's own data)
from gpflow_amd import ops  # noqa: E402

PARAMS = {"bernoulli_probit": (), "poisson_exp": (1.0,), "student_t": (1.0, 3.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--lik", default="bernoulli_probit", choices=sorted(PARAMS))
    args = ap.parse_args()
    device = ops.device()
    warm = torch.eye(256, dtype=torch.float64, device=device)
    ops.potrf_(warm, 256)          # the library places its streams first (bench.py)
    torch.cuda.synchronize()
    n_data, m_ind, d_in, rows, _, seed = bench.WORKLOADS["cm"]
    X, Y, Z, q_mu, q_sqrt, ls = bench.make_inputs(n_data, m_ind, d_in, seed, device)
    Ylab = (Y > 0).to(torch.float64) if args.lik == "bernoulli_probit" else Y.abs().round() if args.lik == "poisson_exp" else Y
    ws = ops.svgp_elbo_workspace(m_ind, rows, d_in, 1, False)
    out = torch.empty(2, dtype=torch.float64, device=device)
    info = torch.zeros(1, dtype=torch.int32, device=device)
    mailbox = ops.HostMailbox(2)
    n_batches = n_data // rows

    def gaussian(s):
        lo = (s % n_batches) * rows
        ops.svgp_elbo_shard(Z, X[lo:lo + rows], Y[lo:lo + rows], q_mu, q_sqrt, variance=1.0, lengthscales=ls, noise_variance=0.1,
                            jitter=1e-6, ws=ws, out=out, info=info)

    def quadrature(s):
        lo = (s % n_batches) * rows
        ops.svgp_elbo_shard_lik(Z, X[lo:lo + rows], Ylab[lo:lo + rows], q_mu, q_sqrt, variance=1.0, lengthscales=ls, lik=args.lik,
                                params=PARAMS[args.lik], jitter=1e-6, ws=ws, out=out, info=info)

    def timed(fn, base):
        t0 = time.perf_counter()
        for s in range(args.steps):
            fn(base + s)
            mailbox.post(out, info)
            vals, inf = mailbox.wait()
            assert inf == 0 and np.isfinite(vals).all(), (inf, vals)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for fn in (gaussian, quadrature):
        timed(fn, 0)
    ms = {"gaussian": [], args.lik: []}
    for r in range(args.rounds):
        for name, fn in (("gaussian", gaussian), (args.lik, quadrature)):
            ms[name].append(timed(fn, r * args.steps))
    rec = {"workload": "cm", "rounds": args.rounds, "steps_per_round": args.steps}
    for name, v in ms.items():
        rec[name] = {"median_ms": float(np.median(v)), "min_ms": float(np.min(v))}
    rec["ratio_median"] = rec[args.lik]["median_ms"] / rec["gaussian"]["median_ms"]
    rec["ratio_min"] = rec[args.lik]["min_ms"] / rec["gaussian"]["min_ms"]
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
