"""Timings for DESIGN 6 "Multiscale" (profiles/multiscale.txt): the Kfu builder at 8192 x 2048, d = 8 and d = 64, the Kuu builder at
M = 2048 and the whole Kfu adjoint (op "mul" + contraction + tail) and Kuu adjoint, against the composed torch-on-device form of the same
quantity (the [N, M, D] broadcast; autograd for the adjoints).  The composed form runs on a slice of ROWS_T rows of X and its time is scaled
by N / ROWS_T (the [N, M, D] temporaries of autograd at d = 64 are the reason).  One process, device events around 5 calls, every
shape warmed, the sides alternating, median (min, max) of 7 windows.  Needs the device; prints one JSON line per shape."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from gpflow_amd import ops  # noqa: E402

N, M, V = 8192, 2048, 1.7
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


def torch_kfu(X, Z, S, ls):
    r = 1 / (ls + S)
    return V * torch.prod(ls * r, -1)[None] * torch.exp(-0.5 * (((X[:, None, :] - Z[None]) * r[None]) ** 2).sum(-1))


def torch_kuu(Z, S, ls):
    a = (ls + S) ** 2
    q = 1 / (a[:, None] + a[None] - ls ** 2)
    return V * torch.sqrt(torch.prod(ls ** 2 * q, -1)) * torch.exp(-0.5 * ((Z[:, None, :] - Z[None]) ** 2 * q).sum(-1))


for d, rows_t in ((8, 8192), (64, 1024)):
    rng = np.random.default_rng(d)
    X, Z = ops.to_device(rng.normal(size=(N, d))), ops.to_device(rng.normal(size=(M, d)))
    S = ops.to_device(rng.uniform(0.05, 1.5, size=(M, d)))
    ls = 1.3 * np.sqrt(d)
    kw = dict(variance=V, lengthscales=ls)
    Kbar, Kub = ops.to_device(rng.normal(size=(N, M))), ops.to_device(rng.normal(size=(M, M)))
    Kout, Uout = torch.empty((N, M), dtype=torch.float64, device=X.device), torch.empty((M, M), dtype=torch.float64, device=X.device)
    parts = ops.multiscale_adjoint_parts(M, d, X.device)
    Xt, Kbt, Mt = X[:rows_t], Kbar[:rows_t], min(M, rows_t)   # the composed side's slice (Kuu: Mt x Mt, scaled by (M / Mt)^2)

    def torch_kfu_adj():
        Zl, Sl = Z.detach().clone().requires_grad_(True), S.detach().clone().requires_grad_(True)
        ll = torch.tensor(ls, dtype=torch.float64, device=X.device, requires_grad=True)
        (Kbt * torch_kfu(Xt, Zl, Sl, ll)).sum().backward()

    def torch_kuu_adj():
        Zl, Sl = Z[:Mt].detach().clone().requires_grad_(True), S[:Mt].detach().clone().requires_grad_(True)
        ll = torch.tensor(ls, dtype=torch.float64, device=X.device, requires_grad=True)
        (Kub[:Mt, :Mt] * torch_kuu(Zl, Sl, ll)).sum().backward()
    r = timed({"kfu": lambda: ops.multiscale_kfu(X, Z, S, out=Kout, **kw),
               "kuu": lambda: ops.multiscale_kuu(Z, S, out=Uout, **kw),
               "kfu_adjoint": lambda: ops.multiscale_kfu_adjoint(X, Z, S, Kbar, **kw),
               "kuu_adjoint": lambda: ops.multiscale_kuu_adjoint(Z, S, Kub, parts=parts, **kw),
               "se_builder": lambda: ops.kernel_matrix(X, Z, out=Kout, **kw),
               "torch_kfu_slice": lambda: torch_kfu(Xt, Z, S, ls), "torch_kuu_slice": lambda: torch_kuu(Z[:Mt], S[:Mt], ls),
               "torch_kfu_adjoint_slice": torch_kfu_adj, "torch_kuu_adjoint_slice": torch_kuu_adj})
    scale = {"torch_kfu_slice": N / rows_t, "torch_kfu_adjoint_slice": N / rows_t, "torch_kuu_slice": (M / Mt) ** 2,
             "torch_kuu_adjoint_slice": (M / Mt) ** 2}
    ref = torch_kfu(Xt, Z, S, ls)
    rel = float((ops.multiscale_kfu(Xt, Z, S, **kw) - ref).abs().max() / ref.abs().max())
    out[f"d{d}"] = dict(ms=r, composed_scale=scale, kfu_write_GBps=N * M * 8 / r["kfu"][0] / 1e6,
                        kfu_valu_Gflops=N * M * (3 * d) / r["kfu"][0] / 1e6, kfu_vs_torch_maxrel=rel)
    print(d, json.dumps(out[f"d{d}"]), flush=True)

if len(sys.argv) > 1:   # python tools/multiscale_probe.py [results.json], from the repository root
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
