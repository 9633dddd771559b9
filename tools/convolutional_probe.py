"""Times of the Convolutional kernel's four device entry points (ops.conv_kfu, conv_kdiag, conv_kfu_adjoint, conv_kdiag_adjoint) beside
the COMPOSED form of the same quantities at the convolutional-GP notebook's shape: 28 x 28 x 1 images, 5 x 5 patches (P = 576),
M = 1000 inducing patches, a minibatch of N images.  The composed form materialises every patch with torch's `unfold` ([N P, 25]),
builds the [N P, M] base-kernel matrix with the stationary builder (ops.kernel_matrix) and takes the weighted sum over p; for K_diag
it builds, per image, the [P, P] matrix of its patches and takes the doubly weighted sum.  The composed adjoint of Kfu is the
stationary adjoint over the [M, N P] seed (gradients.stationary_kernel_adjoint) behind the broadcast of G; K_diag's has no composed
form short of N matrices of [P, P] and is timed alone.  One process, one device: device events around `reps` back-to-back calls, the
sides alternating over `rounds` rounds, median and spread per side.

    python tools/convolutional_probe.py [--n 256] [--m 1000] [--reps 5] [--rounds 7]

Needs the device; there is no CPU path.  DESIGN section 6 "Convolutional kernel" records what it printed.
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
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    from gpflow_amd import gradients, ops
    from gpflow_amd.leaf import Leaf
    dev = ops.device()
    rng = np.random.default_rng(1)
    H = W = 28
    h = w = 5
    geo = (H, W, 1, h, w)
    P, plen, N, M = ops.conv_num_patches(geo), h * w, a.n, a.m
    ls, v = 0.8 * np.sqrt(plen), 1.7
    wts = rng.uniform(0.5, 1.5, size=P)
    kw = dict(geometry=geo, weights=wts, variance=v, lengthscales=ls)
    X, Z = ops.to_device(rng.uniform(size=(N, H * W))), ops.to_device(rng.uniform(size=(M, plen)))
    G, c = ops.to_device(rng.normal(size=(N, M))), ops.to_device(rng.normal(size=N))
    wd = ops.to_device(wts)
    leaf = Leaf("SquaredExponential", v, ls)
    gradients.ls_device(ls, plen, dev)

    def unfold():
        return torch.nn.functional.unfold(X.view(N, 1, H, W), (h, w)).transpose(1, 2).reshape(N * P, plen).contiguous()

    def composed_kfu():
        K = ops.kernel_matrix(unfold(), Z, variance=v, lengthscales=ls)              # [N P, M]
        return torch.einsum("npm,p->nm", K.view(N, P, M), wd) / P

    def composed_kdiag():
        Xp = unfold().view(N, P, plen)
        out = torch.empty(N, dtype=torch.float64, device=dev)
        buf = torch.empty((P, P), dtype=torch.float64, device=dev)
        for n in range(N):
            ops.kernel_matrix(Xp[n], None, out=buf, variance=v, lengthscales=ls)
            out[n] = wd @ (buf @ wd) / (P * P)
        return out

    def composed_kfu_adjoint():
        Kbar = (G.t()[:, :, None] * (wd / P)[None, None, :]).reshape(M, N * P).contiguous()   # dF/dK(Z, patches)
        return gradients.stationary_kernel_adjoint(leaf, Z, unfold(), Kbar, symmetric=False)

    sides = {"conv_kfu": lambda: ops.conv_kfu(X, Z, **kw), "composed Kfu": composed_kfu,
             "conv_kdiag": lambda: ops.conv_kdiag(X, **kw), "composed K_diag": composed_kdiag,
             "conv_kfu_adjoint": lambda: ops.conv_kfu_adjoint(X, Z, G, **kw), "composed Kfu adjoint (no d/dweights)": composed_kfu_adjoint,
             "conv_kdiag_adjoint": lambda: ops.conv_kdiag_adjoint(X, c, **kw)}
    got, ref = ops.conv_kfu(X, Z, **kw), composed_kfu()
    print(f"Kfu, conv against composed: max |difference| {float((got - ref).abs().max()):.2e} at max |Kfu| {float(ref.abs().max()):.2e}")
    times = {name: [] for name in sides}
    for f in sides.values():      # warm-up: code objects, the LDS attribute, the cached weights
        f()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.reps)
    print(f"28 x 28 x 1, 5 x 5 patches (P = {P}), N = {N}, M = {M}: {a.reps} calls per window, {a.rounds} rounds, microseconds per call")
    for name, ts in times.items():
        print(f"{name:40s} median {statistics.median(ts):10.1f}  min {min(ts):10.1f}  max {max(ts):10.1f}")
    evals = {"conv_kfu": N * M * P, "conv_kdiag": N * P * (P + 1) // 2, "conv_kfu_adjoint": N * M * P, "conv_kdiag_adjoint": N * P * P}
    for name, n_exp in evals.items():
        print(f"{name:40s} {n_exp / statistics.median(times[name]) / 1e3:8.2f} G base-kernel evaluations / s")


if __name__ == "__main__":
    main()
