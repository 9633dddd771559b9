"""Times of the wide stationary builder (gpflow_amd/csrc/wide/wide_stationary.hip) beside (a) `ops.gemm_nt` alone on the same (n1, n2, d)
-- a GEMM with no scaling, norms or epilogue: the ceiling -- and (b) the composed torch expansion on the device, what a user could do
before; then `gradients.stationary_kernel_adjoint` beside torch autograd over the same expansion, and the adjoint's pieces one by one.
One process, one device: device events around `reps` back-to-back calls (as many as fill --window-ms), the sides alternating over
--rounds rounds, median [min, max] per side.  TFLOP/s counts 2 n1 n2 d whatever the symmetry.

    python tools/wide_inputs_probe.py [--rounds 5] [--window-ms 200]

Needs the device; there is no CPU path.  DESIGN §6 "Wide inputs" and profiles/wide_inputs.txt record what it printed.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpflow_amd import gradients, ops  # noqa: E402
from gpflow_amd.leaf import Leaf  # noqa: E402

ARGS = None


def say(*a):
    print(" ".join(str(x) for x in a), flush=True)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_kernel(family, X1, X2, ls, variance):
    a, b = X1 / ls, X2 / ls
    r2 = (-2.0 * (a @ b.t())) + ((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :])
    if family == "SquaredExponential":
        return variance * torch.exp(-0.5 * r2)
    r = torch.sqrt(torch.clamp(r2, min=1e-36))
    s5 = 5.0 ** 0.5
    return variance * (1.0 + s5 * r + (5.0 / 3.0) * r * r) * torch.exp(-s5 * r)


def compare(sides):
    reps = {}
    for k, fn in sides.items():   # warm-up of every side, and as many calls per window as fill it
        fn()
        reps[k] = max(4, min(4000, int(ARGS.window_ms / max(timed(fn, 2), 1e-3))))
    torch.cuda.synchronize()
    t = {k: [] for k in sides}
    for _ in range(ARGS.rounds):
        for k, fn in sides.items():
            t[k].append(timed(fn, reps[k]))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in t.items()}


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=200.0)
    ARGS = ap.parse_args()
    dev = ops.device()
    say("device", torch.cuda.get_device_name(0), "compute units", torch.cuda.get_device_properties(0).multi_processor_count)
    g = torch.Generator(device="cpu").manual_seed(0)
    for (n1, n2, sym) in ((8192, 8192, True), (8192, 8192, False), (8192, 1024, False)):
        for d in (128, 784):
            X1 = torch.randn((n1, d), generator=g, dtype=torch.float64).to(dev)
            X2 = X1 if sym else torch.randn((n2, d), generator=g, dtype=torch.float64).to(dev)
            ls = 0.9 * d ** 0.5
            out = torch.empty((n1, n2), dtype=torch.float64, device=dev)
            C = torch.empty((n1, n2), dtype=torch.float64, device=dev)
            for family in ("SquaredExponential", "Matern52"):
                sides = {
                    "wide": lambda: ops.kernel_matrix(X1, None if sym else X2, variance=1.3, lengthscales=ls, family=family, out=out),
                    "gemm": lambda: ops.gemm_nt(X1, X2, C=C),
                    "torch": lambda: torch_kernel(family, X1, X2, ls, 1.3),
                }
                r = compare(sides)
                ref = torch_kernel(family, X1, X2, ls, 1.3)
                err = float((sides["wide"]() - ref).abs().max())
                flop = 2.0 * n1 * n2 * d
                say(f"build n1={n1} n2={n2} sym={int(sym)} d={d} {family}: " +
                    "  ".join(f"{k} {m:.3f} ms [{lo:.3f}, {hi:.3f}]" for k, (m, lo, hi) in r.items()) +
                    f"  wide {flop / r['wide'][0] / 1e9:.1f} TFLOP/s  fraction of gemm {r['gemm'][0] / r['wide'][0]:.2f}"
                    f"  torch / wide {r['torch'][0] / r['wide'][0]:.2f}  max |wide - torch| {err:.2e}")
                del ref
            del out, C
            torch.cuda.empty_cache()
    # the adjoint at 8192 x 1024, d = 784, against torch autograd over the same expansion
    n1, n2, d = 8192, 1024, 784
    A = torch.randn((n1, d), generator=g, dtype=torch.float64).to(dev)
    B = torch.randn((n2, d), generator=g, dtype=torch.float64).to(dev)
    Kbar = torch.randn((n1, n2), generator=g, dtype=torch.float64).to(dev)
    for family in ("SquaredExponential", "Matern52"):
        ls = np.full(d, 0.9 * d ** 0.5)
        leaf = Leaf(family, 1.3, ls)

        def autograd():
            a = A.clone().requires_grad_(True)
            l = torch.tensor(ls, device=dev, requires_grad=True)
            v = torch.tensor(1.3, dtype=torch.float64, device=dev, requires_grad=True)
            (torch_kernel(family, a, B, l, v) * Kbar).sum().backward()
            return v.grad, l.grad, a.grad
        sides = {"adjoint": lambda: gradients.stationary_kernel_adjoint(leaf, A, B, Kbar, symmetric=False), "torch": autograd}
        r = compare(sides)
        got, ref = sides["adjoint"](), autograd()
        err = max(float((g_ - r_.reshape(g_.shape)).abs().max() / r_.abs().max()) for g_, r_ in zip(got, ref))
        say(f"adjoint n1={n1} n2={n2} d={d} {family}: " + "  ".join(f"{k} {m:.3f} ms [{lo:.3f}, {hi:.3f}]" for k, (m, lo, hi) in r.items()) +
            f"  torch / adjoint {r['torch'][0] / r['adjoint'][0]:.2f}  max relative difference {err:.2e}")
    # where the adjoint's time goes: its pieces at the same shape (SquaredExponential: one combine pass, the contraction, the tail)
    kw = Leaf("SquaredExponential", 1.3, ls).keywords()
    G = ops.kernel_matrix_hadamard(A, B, Kbar, **kw)
    Vt = ops.moment_rows(B)
    R = gradients.splitk_gemm_nt(G, Vt)
    lsd = ops.ls_device(ls, d, dev)
    pieces = {"combine pass (wide)": lambda: ops.kernel_matrix_hadamard(A, B, Kbar, out=G, **kw), "moment_rows": lambda: ops.moment_rows(B),
              "contraction G [1, B, B^2]": lambda: gradients.splitk_gemm_nt(G, Vt),
              "stationary_adjoint_tail": lambda: ops.stationary_adjoint_tail(R, A, lsd, variance=1.3, symmetric=False)}
    say("adjoint pieces: " + "  ".join(f"{k} {m:.3f} ms [{lo:.3f}, {hi:.3f}]" for k, (m, lo, hi) in compare(pieces).items()))


if __name__ == "__main__":
    main()
