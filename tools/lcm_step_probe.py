"""Cost of one ELBO step of a LinearCoregionalization SVGP, and of its mixing stage.  Alternating rounds of ONE process (same device,
same clocks, same neighbours), every shape warmed up, every timed window ended by a device synchronise:

  (a) ops.svgp_elbo_shard_lcm        M = 1024, 8192 rows, d = 8, L = 4 latents mixed into P = 8 outputs (one C-ABI call)
  (b) the composed elbo_terms of the same model (predict_f + Gaussian variational expectations + KL from the host mirror)
  (c) ops.svgp_elbo_shard_sep at P = 4 -- config C5's separate shard, the floor: (a) is (c) with the mixing stage as its tail
  stage: ops.mixed_gaussian_varexp_sum alone on 8192 rows (the stage-1 kernel, two one-block final sums, the dW combine)

Prints one JSON line: median / min / max per call of each over the rounds, and `repeat_*` -- the same measurement taken a second
time in the same process -- as the spread to read a difference against.  With --kernel-only N the process only runs N fused steps
and N stage calls: the run to put under `rocprofv3 --kernel-trace --stats` for the kernel's own time (mixed_varexp_kernel).
The bytes the stage-1 kernel has to move, from the shapes: rows (L gmean + L s0 + L ssq + P Y) doubles in; with every optional
output rows (2 P + L) doubles out (`stage_bytes_*`).

    python tools/lcm_step_probe.py [--rounds 5] [--steps 200] [--calls 400] [--kernel-only 0]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpflow_amd as gpflow  # noqa: E402
from gpflow_amd import ops  # noqa: E402

FAMILIES = ["SquaredExponential", "Matern32", "Matern52", "SquaredExponential"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=400)
    ap.add_argument("--kernel-only", type=int, default=0)
    args = ap.parse_args()
    device = ops.device()
    rng = np.random.default_rng(0)
    M, rows, D, L, P = 1024, 8192, 8, 4, 8
    t = ops.to_device
    Xh = rng.normal(size=(rows, D))
    Zh = Xh[:M] + 0.05 * rng.normal(size=(M, D))
    Wh = rng.normal(size=(P, L)) / np.sqrt(L)
    Yh = rng.normal(size=(rows, P))
    qmh = 0.3 * rng.normal(size=(M, L))
    qsh = np.stack([np.tril(0.02 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(L)])
    X, Z, Y, q_mu, q_sqrt = t(Xh), t(Zh), t(Yh), t(qmh), t(qsh)
    var, ls = [1.0 + 0.1 * l for l in range(L)], [float(np.sqrt(D)) * (1.0 + 0.1 * l) for l in range(L)]
    kw = dict(variances=var, lengthscales=ls, families=FAMILIES, noise_variance=0.2, jitter=1e-6, mean_const=0.1)
    out = torch.empty(2, dtype=torch.float64, device=device)
    info = torch.zeros(L, dtype=torch.int32, device=device)
    ws_lcm, ws_sep = ops.svgp_elbo_lcm_workspace(M, rows, D, L, P), ops.svgp_elbo_sep_workspace(M, rows, D, L)
    Y4 = Y[:, :L].contiguous()

    def fused():
        return ops.svgp_elbo_shard_lcm(Z, X, Y, q_mu, q_sqrt, Wh, ws=ws_lcm, out=out, info=info, **kw)

    def separate():
        return ops.svgp_elbo_shard_sep(Z, X, Y4, q_mu, q_sqrt, ws=ws_sep, out=out, info=info, **kw)

    K = gpflow.kernels
    kern = K.LinearCoregionalization([getattr(K, f)(variance=v, lengthscales=l) for f, v, l in zip(FAMILIES, var, ls)], Wh)
    iv = gpflow.inducing_variables.SharedIndependentInducingVariables(gpflow.inducing_variables.InducingPoints(Zh))
    model = gpflow.models.SVGP(kern, gpflow.likelihoods.Gaussian(0.2), iv, q_mu=qmh, q_sqrt=qsh, num_latent_gps=L,
                               mean_function=gpflow.mean_functions.Constant(0.1))
    assert model._fused_lcm_config() is not None
    f_model = model.elbo_terms((X, Y)).cpu().numpy()
    model._fused_lcm_config = lambda: None

    def composed():
        return model.elbo_terms((X, Y))

    gm, s0, ssq = t(rng.normal(size=(rows, L))), t(rng.uniform(0, 0.5, size=(L, rows))), t(rng.uniform(0, 0.3, size=(L, rows)))

    def stage():
        return ops.mixed_gaussian_varexp_sum(Y, gm, Wh, s0=s0, ssq=ssq, knn=var, noise_variance=0.2, mean_const=0.1, s0_per_latent=True,
                                             want_moments=True, want_grads=True)

    def stage_bare():
        return ops.mixed_gaussian_varexp_sum(Y, gm, Wh, s0=s0, ssq=ssq, knn=var, noise_variance=0.2, mean_const=0.1, s0_per_latent=True)

    if args.kernel_only:
        for fn in (fused, stage, stage_bare):
            for _ in range(args.kernel_only):
                fn()
        torch.cuda.synchronize()
        print(json.dumps({"kernel_only": args.kernel_only}))
        return

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n * 1e3      # us per call

    # (the three forms compute the same thing where they overlap: checked before anything is timed)
    f_fused = fused()[0].cpu().numpy().copy()
    f_comp = composed().cpu().numpy()
    assert np.allclose(f_fused, f_comp, rtol=1e-9) and np.allclose(f_fused, f_model, rtol=0, atol=0), (f_fused, f_comp, f_model)
    rec = {"m": M, "rows": rows, "d": D, "L": L, "P": P, "rounds": args.rounds, "steps": args.steps, "calls": args.calls,
           "stage_bytes_in": rows * (3 * L + P) * 8, "stage_bytes_out_all": rows * (2 * P + L) * 8}
    steps = {"a_fused_lcm": fused, "b_composed_lcm": composed, "c_separate_P4": separate}
    stages = {"stage_all_outputs": stage, "stage_out_only": stage_bare}
    for fns, n in ((steps, args.steps), (stages, args.calls)):
        for fn in fns.values():
            timed(fn, max(20, n // 4))
        for tag in ("", "repeat_"):
            got = {name: [] for name in fns}
            for _ in range(args.rounds):
                for name, fn in fns.items():
                    got[name].append(timed(fn, n))
            for name, v in got.items():
                rec[tag + name] = {"median_us": float(np.median(v)), "min_us": float(np.min(v)), "max_us": float(np.max(v))}
    assert int(info.abs().sum().cpu()) == 0 and bool(torch.isfinite(out).all())
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
