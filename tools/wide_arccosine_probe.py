"""Timings for DESIGN 6 "Wide ArcCosine" (profiles/wide_arccosine.txt): builder, adjoint stage, whole adjoint, tail and contraction at
8192 x 8192, d = 64 (the narrow path) / 128 / 784, orders 0 / 2, against the composed torch-on-device form (matmul plus elementwise
ops, autograd for the adjoint) and the wide SquaredExponential builder.  One process, device events around 5 calls, every shape warmed,
the sides alternating, median (min, max) of 7 windows.  Needs the device; prints one JSON line per shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from gpflow_amd import gradients, ops  # noqa: E402
from gpflow_amd.leaf import ArcLeaf  # noqa: E402

N = 8192
V, B = 0.8, 0.7
out = {}


def timed(fns, reps=5, windows=7):
    for f in fns.values():
        f()
        f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    for _ in range(windows):
        for k, f in fns.items():   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                f()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b) / reps)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in res.items()}


def torch_k(order, A, Bm, w):
    p, q = (A * A * w).sum(1) + B, (Bm * Bm * w).sum(1) + B
    c = ((A * w) @ Bm.T + B) / (torch.sqrt(p)[:, None] * torch.sqrt(q)[None, :])
    th = torch.acos(1e-15 + (1 - 2e-15) * c)
    pt = np.pi - th
    if order == 0:
        return V / np.pi * pt
    sn, cs = torch.sin(th), torch.cos(th)
    return V / np.pi * (3.0 * sn * cs + pt * (1.0 + 2.0 * cs * cs)) * p[:, None] * q[None, :]


for d in (64, 128, 784):
    rng = np.random.default_rng(d)
    A, Bm = ops.to_device(rng.normal(size=(N, d))), ops.to_device(rng.normal(size=(N, d)))
    Kbar = ops.to_device(rng.normal(size=(N, N)))
    w = 1.3 / d
    for order in (0, 2):
        kw = dict(order=order, variance=V, weight_variances=w, bias_variance=B)
        Kout, Gout = torch.empty((N, N), dtype=torch.float64, device=A.device), torch.empty((N, N), dtype=torch.float64, device=A.device)
        parts = ops.arccos_adjoint_parts(N, N, A.device)
        leaf = ArcLeaf(order, V, w, B)
        fns = {"builder": lambda: ops.arccos_kernel_matrix(A, Bm, out=Kout, **kw),
               "stage": lambda: ops.arccos_adjoint_stage(A, Bm, Kbar, parts, out=Gout, **kw),
               "adjoint": lambda: gradients.arccos_kernel_adjoint(leaf, A, Bm, Kbar, symmetric=False),
               "torch_builder": lambda: torch_k(order, A, Bm, w)}
        if d > 64:
            fns["se_builder"] = lambda: ops.kernel_matrix(A, Bm, variance=V, lengthscales=0.9 * np.sqrt(d), out=Kout)

        def torch_adj():
            Al = A.detach().clone().requires_grad_(True)
            wl = torch.tensor(w, dtype=torch.float64, device=A.device, requires_grad=True)
            (Kbar * torch_k(order, Al, Bm, wl)).sum().backward()
        fns["torch_adjoint"] = torch_adj
        r = timed(fns)
        if order == 2:   # the tail alone, on the stage's parts
            Vt = ops.moment_rows(Bm)[:1 + d] if d > 64 else ops.moment_rows(Bm)
            R = gradients.splitk_gemm_nt(Gout, Vt)
            r.update(timed({"tail": lambda: ops.arccos_adjoint_tail(R, A, Bm, parts, weight_variances=w),
                            "contraction": lambda: gradients.splitk_gemm_nt(Gout, Vt)}))
        rel = float((ops.arccos_kernel_matrix(A, Bm, **kw) - torch_k(order, A, Bm, w)).abs().max() / torch_k(order, A, Bm, w).abs().max())
        out[f"d{d}_order{order}"] = dict(ms=r, builder_vs_torch_maxrel=rel)
        print(d, order, json.dumps(out[f"d{d}_order{order}"]), flush=True)

if len(sys.argv) > 1:   # python tools/wide_arccosine_probe.py [results.json], from the repository root
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
