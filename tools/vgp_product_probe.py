"""A/B of ops.tril_product (ssq only) against the composed route of existing primitives (transpose + gemm_nt(a_tri=2, b_tri=1) +
row_stats), and whole VGP.elbo() / objective_and_grad() call times: the numbers of DESIGN 6 "VGP".  Untraced, the two sides alternating
in one process, device events around each call; medians and spread as JSON lines.  Rates are against the N^3 / 3 * R flops of the
triangular product.

    python tools/vgp_product_probe.py [ab | model | all]
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpflow_amd as gp  # noqa: E402
from gpflow_amd import ops  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    v = np.sort(np.asarray(v))
    return dict(median_ms=float(np.median(v)), min_ms=float(v[0]), p10_ms=float(v[len(v) // 10]), p90_ms=float(v[(9 * len(v)) // 10]),
                max_ms=float(v[-1]), calls=len(v))


def ab(N, R, calls=24, warm=4):
    rng = np.random.default_rng(N + R)
    X = ops.to_device(rng.uniform(-2, 2, size=(N, 2)))
    K = ops.kernel_matrix(X, None, variance=1.3, lengthscales=0.7, diag_add=1e-3)
    _, info = ops.potrf_(K, N, zero_upper=True)
    ops.check_info(info)
    L = K
    S = torch.tril(0.05 * torch.randn((R, N, N), dtype=torch.float64, device=L.device)) + 0.6 * torch.eye(N, dtype=torch.float64, device=L.device)
    S += torch.triu(torch.full((N, N), 0.37, dtype=torch.float64, device=L.device), 1)    # junk above the diagonal
    parts = ops.tril_product_parts(N, R)

    def fused():
        return ops.tril_product(L, S, parts=parts)[0]

    def composed():
        ST = ops.transpose(S, mode=1)                                   # tril(S_r)^T
        W = ops.gemm_nt(L, ST, a_tri=2, b_tri=1)                        # the whole [R, N, N] product
        W3 = W if W.dim() == 3 else W.unsqueeze(0)
        return torch.stack([ops.row_stats(W3[r])[0] for r in range(R)])
    tf, tc = [], []
    for i in range(warm + calls):
        for side in ((fused, tf), (composed, tc)) if i % 2 == 0 else ((composed, tc), (fused, tf)):
            ms, out = timed(side[0])
            if i >= warm:
                side[1].append(ms)
    a, b = fused(), composed()
    rel = float(((a - b).abs() / b.abs()).max())
    flops = N ** 3 / 3.0 * R
    sf, sc = stats(tf), stats(tc)
    print(json.dumps(dict(what="tril_product_ab", N=N, R=R, fused=sf, composed=sc, ratio_composed_over_fused=sc["median_ms"] / sf["median_ms"],
                          fused_tflops=flops / sf["median_ms"] / 1e9, composed_tflops=flops / sc["median_ms"] / 1e9,
                          max_rel_diff=rel, temporary_bytes_saved=int(2 * R * N * N * 8), parts_bytes=int(parts.numel() * 8))), flush=True)


def model(N, R, calls=7, warm=2):
    rng = np.random.default_rng(7 * N + R)
    X = rng.uniform(-2, 2, size=(N, 2))
    Y = (np.sin(X.sum(1, keepdims=True) + np.arange(R)[None]) + 0.3 * rng.normal(size=(N, R)) > 0).astype(np.float64)
    m = gp.models.VGP((X, Y), gp.kernels.SquaredExponential(variance=1.3, lengthscales=0.7), gp.likelihoods.Bernoulli())
    m.q_mu.assign(0.1 * rng.normal(size=(N, R)))
    te, tg = [], []
    for i in range(warm + calls):
        t0 = time.perf_counter()
        v = float(m.elbo())
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        F, g = m.objective_and_grad()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            te.append(1e3 * (t1 - t0))
            tg.append(1e3 * (t2 - t1))
    print(json.dumps(dict(what="vgp_model", N=N, R=R, likelihood="Bernoulli", elbo=stats(te), objective_and_grad=stats(tg), elbo_value=v,
                          grad_value=F)), flush=True)


if __name__ == "__main__":
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    if which in ("ab", "all"):
        for N, R in ((4096, 1), (4096, 4), (512, 1), (1024, 1), (2048, 1), (8192, 1)):
            ab(N, R)
    if which in ("model", "all"):
        for N, R in ((4096, 1), (4096, 4)):
            model(N, R)
