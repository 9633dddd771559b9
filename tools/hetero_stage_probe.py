"""Cost of the heteroskedastic two-latent stage (ops.hetero_varexp_sum, value and seeds) beside what it replaces, rows = 65536:

  exp       against the composed torch expression of the closed form (value, dmu, dvar as elementwise torch on the device)
  softplus  against the reference's 20 x 20 = 400-node Gauss-Hermite grid written in torch (the value alone: the grid has no seeds)

and one SVGP.elbo at the benchmark's shape (M = 2048, 8192 rows, d = 8) with this likelihood (two latents, composed path) against
Gaussian (one latent, fused shard): what the stage and the second latent add to a step.

All in interleaved rounds of ONE process, the same warm-up, device events around `--calls` calls, medians over `--rounds` rounds with
min and max as the spread; the host clock around the same calls (enqueue only) beside the event time.  Prints one JSON line.

    python tools/hetero_stage_probe.py [--rounds 9] [--calls 50] [--rows 65536]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpflow_amd as gp  # noqa: E402
from gpflow_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rows", type=int, default=65536)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    n, t = args.rows, ops.to_device
    F = t(np.stack([rng.normal(size=n), rng.uniform(-2, 2, size=n)], 1))
    Y = t(rng.normal(size=(n, 1)) * 1.5)
    s0, ssq = t(rng.uniform(0, 0.5, size=n)), t(rng.uniform(0, 0.6, size=(2, n)))
    x, w = ops.gauss_hermite(20)
    gx, gw = t(x), t(w / np.sqrt(np.pi))

    def stage(link):
        return ops.hetero_varexp_sum(Y, F, s0=s0, ssq=ssq, knn=[1.2], link=link, want_grads=True)

    def moments():
        fv = (1.2 - s0[None, :] + ssq).t()
        return Y[:, 0], F[:, 0], fv[:, 0], F[:, 1], fv[:, 1]

    def composed_exp():
        y, m1, v1, m2, v2 = moments()
        dy = y - m1
        a, e2 = dy * dy + v1, torch.exp(2 * v2 - 2 * m2)
        ve = -0.5 * math.log(2 * math.pi) - m2 - 0.5 * a * e2
        return ve.sum().reshape(1), None, torch.stack([dy * e2, a * e2 - 1], 1), torch.stack([-0.5 * e2, -a * e2], 1), None

    def grid_softplus():
        y, m1, v1, m2, v2 = moments()
        f = m1[:, None, None] + torch.sqrt(2 * v1)[:, None, None] * gx[None, :, None]
        s = torch.nn.functional.softplus(m2[:, None, None] + torch.sqrt(2 * v2)[:, None, None] * gx[None, None, :])
        lp = -0.5 * math.log(2 * math.pi) - torch.log(s) - 0.5 * ((y[:, None, None] - f) / s) ** 2
        return ((lp * gw[None, :, None] * gw[None, None, :]).sum((1, 2))).sum().reshape(1),

    B, M, d = 8192, 2048, 8
    X, Z = rng.uniform(-1, 1, size=(B, d)), rng.uniform(-1, 1, size=(M, d))
    Yb = np.sin(X[:, :1]) + 0.3 * rng.normal(size=(B, 1))
    models = {"svgp_elbo_gaussian": gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=np.ones(d)), gp.likelihoods.Gaussian(0.1),
                                                   Z.copy(), num_data=10 ** 6)}
    for link in ("exp", "softplus"):
        models[f"svgp_elbo_hetero_{link}"] = gp.models.SVGP(gp.kernels.SquaredExponential(lengthscales=np.ones(d)),
                                                            gp.likelihoods.HeteroskedasticTFPConditional(scale_transform=link),
                                                            Z.copy(), num_data=10 ** 6)
    data = (t(X), t(Yb))
    fns = {"stage_exp": lambda: stage("exp"), "composed_exp": composed_exp, "stage_softplus": lambda: stage("softplus"),
           "grid400_softplus": grid_softplus, **{k: (lambda m=m: m.elbo(data)) for k, m in models.items()}}

    a, c, b, g = (fns[k]() for k in ("stage_exp", "composed_exp", "stage_softplus", "grid400_softplus"))
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max().clamp(min=1.0))  # noqa: E731
    rec = {"rows": n, "rounds": args.rounds, "calls_per_round": args.calls, "device": str(ops.device()),
           "exp_stage_vs_composed_max_rel": max(rel(a[0], c[0]), rel(a[2], c[2]), rel(a[3], c[3])),
           "softplus_stage_vs_grid_rel": rel(b[0], g[0]), "svgp_shape": {"M": M, "rows": B, "d": d}}

    def timed(fn, k):
        """(device ms per call by events, host ms per call spent enqueueing)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        h0 = time.perf_counter()
        for _ in range(k):
            fn()
        h1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / k, (h1 - h0) / k * 1e3

    calls = {k: (args.calls if k.startswith(("stage", "composed", "grid")) else max(5, args.calls // 5)) for k in fns}
    for k, fn in fns.items():          # warm-up: code objects, allocator, clocks
        timed(fn, max(5, calls[k] // 2))
    got = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            got[k].append(timed(fn, calls[k]))
    for k, v in got.items():
        ev, host = np.array(v).T
        rec[k] = {"median_us": round(float(np.median(ev) * 1e3), 2), "min_us": round(float(ev.min() * 1e3), 2),
                  "max_us": round(float(ev.max() * 1e3), 2), "host_enqueue_median_us": round(float(np.median(host) * 1e3), 2)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
