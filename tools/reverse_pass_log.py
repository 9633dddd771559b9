"""What the reverse pass ISSUES, and what it returns, for a tree of this repository -- no device needed.

    python tools/reverse_pass_log.py dump  <tree> <out.pkl>     run the matrix below on <tree>'s gpflow_amd/gradients.py
    python tools/reverse_pass_log.py compare <a.pkl> <b.pkl>    compare two dumps case by case

`gradients.ops` is tests/fake_ops.py + tests/fake_likelihood_ops.py (of the SAME tree) behind a logging proxy: one line per outermost
`ops.*` call (name, shape and strides of every tensor argument, every scalar argument); a TorchDispatchMode adds one line per aten op
issued OUTSIDE an `ops.*` call (the torch glue).  Each case runs twice and the second run is kept (`ls_device` caches).  Kept per
case: the log and the bytes of F, every gradient and info.  Written for the refactor recorded in profiles/reverse_pass_refactor.txt.
"""
import itertools
import pickle
import sys
import types

import numpy as np


def _desc(a):
    import torch
    if isinstance(a, torch.Tensor):
        return ("T", tuple(a.shape), tuple(a.stride()), str(a.dtype))
    if isinstance(a, np.ndarray):
        return ("np", a.shape, a.tobytes().hex())
    if isinstance(a, (list, tuple)):
        return tuple(_desc(x) for x in a)
    if isinstance(a, (int, float, str, bool, type(None), np.floating, np.integer)):
        return repr(a)
    return type(a).__name__


def load(tree):
    sys.path[:0] = [tree, tree + "/tests"]
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    import fake_likelihood_ops
    import fake_ops
    from gpflow_amd import gradients
    log, depth = [], [0]

    def wrap(name, fn):
        def call(*args, **kw):
            if depth[0] == 0:
                log.append(("ops." + name, tuple(_desc(a) for a in args), tuple((k, _desc(v)) for k, v in sorted(kw.items()))))
            depth[0] += 1
            try:
                return fn(*args, **kw)
            finally:
                depth[0] -= 1
        return call

    proxy = types.SimpleNamespace()
    for mod in (fake_ops, fake_likelihood_ops):
        for name in dir(mod):
            v = getattr(mod, name)
            if name.startswith("_") or isinstance(v, types.ModuleType):
                continue
            setattr(proxy, name, wrap(name, v) if callable(v) else v)
    gradients.ops = proxy

    class Glue(TorchDispatchMode):
        def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
            if depth[0] == 0:
                log.append((str(func), tuple(_desc(a) for a in args), tuple((k, _desc(v)) for k, v in sorted((kwargs or {}).items()))))
            return func(*args, **(kwargs or {}))

    return torch, gradients, log, Glue


def kernels(g, D=3):
    ard = np.sqrt(D) * (0.8 + 0.05 * np.arange(D))
    se, m32, m52 = ("SquaredExponential", 1.3, ard), ("Matern32", 0.7, np.array(1.3)), ("Matern52", 0.9, np.array(0.8))
    return {
        "se_ard": lambda: dict(variance=1.3, lengthscales=ard),
        "m32_iso": lambda: dict(variance=0.7, lengthscales=1.3, family="Matern32"),
        "sum2": lambda: dict(kernel_spec=g.KernelSpec([se, m32], "add")),
        "prod2_cols": lambda: dict(kernel_spec=g.KernelSpec([("SquaredExponential", 1.3, ard[:2]), m32], "mul", [[0, 1], [2]])),
        "nested": lambda: dict(kernel_spec=g.KernelSpec([se, m32, m52], ("mul", [("add", [0, 1]), 2]))),
    }


def cases(torch, g):
    """(name, function, args, kwargs-maker) for the whole matrix at M = 64, B = 200, D = 3 and the benchmark form at M = 256, B = 512"""
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    out = []

    def data(M, B, D, P, lik="scalar"):
        rng = np.random.default_rng(7)
        X = rng.normal(size=(B, D))
        Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(B, P))
        if lik == "bernoulli_probit":
            Y = (Y > 0).astype(np.float64)
        if lik == "poisson_exp":
            Y = np.floor(np.exp(Y))
        Z = rng.normal(size=(M, D))
        q_mu = 0.3 * rng.normal(size=(M, P))
        q_full = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(P)])
        q_diag = 0.4 + 0.2 * np.abs(rng.normal(size=(M, P)))
        rows = 0.2 + 0.1 * np.abs(X[:, 0])
        return X, Y, Z, q_mu, q_full, q_diag, rows

    liks = {"bernoulli_probit": (), "poisson_exp": (1.5,), "student_t": (0.7, 4.0)}
    kn = kernels(g)
    for qf, lik, (kname, kmk), P in itertools.product(("full", "diag"), ("scalar", "rows", *liks), kn.items(), (1, 2)):
        if lik in liks and kname not in ("se_ard", "m32_iso"):
            continue   # (refused by SVGP.elbo_and_grad: a quadrature likelihood needs one stationary kernel)
        X, Y, Z, q_mu, q_full, q_diag, rows = data(64, 200, 3, P, lik)
        kw = dict(jitter=1e-6, scale=5.0, mean_const=0.1, kl_weight=0.5)
        kw["noise_variance"] = t(rows) if lik == "rows" else 0.2
        if lik in liks:
            kw["likelihood"] = (lik, liks[lik])
        out.append((f"white/{qf}/{lik}/{kname}/P{P}", "svgp_elbo_and_grad",
                    (Z, X, Y, q_mu, q_full if qf == "full" else q_diag), kw, kmk))
    for qf, lik, (kname, kmk) in itertools.product(("full", "diag"), ("scalar", "rows"), kn.items()):
        X, Y, Z, q_mu, q_full, q_diag, rows = data(64, 200, 3, 2)
        kw = dict(jitter=1e-6, scale=5.0, mean_const=0.1, kl_weight=0.5, noise_variance=t(rows) if lik == "rows" else 0.2)
        out.append((f"unwhite/{qf}/{lik}/{kname}", "svgp_elbo_and_grad_unwhitened", (Z, X, Y, q_mu, q_full if qf == "full" else q_diag), kw, kmk))
    for lik, (kname, kmk) in itertools.product(("scalar", "rows"), kn.items()):
        X, Y, Z, q_mu, q_full, q_diag, rows = data(64, 200, 3, 2)
        nv = t(rows) if lik == "rows" else 0.2
        out.append((f"sgpr/{lik}/{kname}", "sgpr_elbo_and_grad", (Z, X, Y), dict(jitter=1e-6, mean_const=0.1, noise_variance=nv), kmk))
        out.append((f"gpr/{lik}/{kname}", "gpr_lml_and_grad", (X, Y), dict(mean_const=0.1, noise_variance=nv), kmk))
    # the smallest shape where splitk_gemm_nt splits (K = 512: two chunks of 256), benchmark form
    X, Y, Z, q_mu, q_full, q_diag, rows = data(256, 512, 3, 2)
    out.append(("white/full/scalar/se_ard/M256", "svgp_elbo_and_grad", (Z, X, Y, q_mu, q_full),
                dict(jitter=1e-6, scale=5.0, mean_const=0.1, noise_variance=0.2), kn["se_ard"]))
    return [(n, f, tuple(t(a) for a in args), kw, kmk) for n, f, args, kw, kmk in out]


def dump(tree, path):
    torch, g, log, Glue = load(tree)
    res = {}
    for chunks, min_n in ((1, 1024), (4, 64)):
        g.TRI_PRODUCT_CHUNKS, g.TRI_PRODUCT_MIN_N = chunks, min_n
        for name, fn, args, kw, kmk in cases(torch, g):
            for _ in range(2):
                del log[:]
                with Glue():
                    F, grads, info = getattr(g, fn)(*args, **kw, **kmk())
            vals = {"F": F, "info": info}
            for k, v in grads.items():
                for i, vi in enumerate(v if isinstance(v, list) else [v]):
                    vals[f"{k}[{i}]" if isinstance(v, list) else k] = vi
            res[f"chunks{chunks}/{name}"] = (list(log), {k: (tuple(v.shape), v.detach().contiguous().numpy().tobytes()) for k, v in vals.items()})
    with open(path, "wb") as f:
        pickle.dump(res, f)
    n_ops = sum(1 for e in res["chunks1/white/full/scalar/se_ard/P2"][0] if e[0].startswith("ops."))
    print(len(res), "cases; benchmark form (M = 64, P = 2):", n_ops, "ops.* calls,",
          len(res["chunks1/white/full/scalar/se_ard/P2"][0]) - n_ops, "aten ops")
    print([e[0][4:] for e in res["chunks1/white/full/scalar/se_ard/P2"][0] if e[0].startswith("ops.")])


def compare(pa, pb):
    """per case: are the logs identical / the same lines in another order / different lines, and are the returned bytes identical"""
    a, b = pickle.load(open(pa, "rb")), pickle.load(open(pb, "rb"))
    assert a.keys() == b.keys()
    kinds, same_bytes = {}, 0
    for name in a:
        (la, va), (lb, vb) = a[name], b[name]
        sub = lambda l, ops_: [e for e in l if e[0].startswith("ops.") == ops_]  # noqa: E731
        if la == lb:
            kind = "identical log"
        elif sorted(map(repr, la)) == sorted(map(repr, lb)):
            kind = "same lines, torch glue in another order" if sub(la, True) == sub(lb, True) else "same lines, ops.* calls in another order"
        else:
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            kind = "different lines (ops.* calls %s)" % ("identical" if sub(la, True) == sub(lb, True) else "differ")
            print(f"LOG   {name}: {len(la)} -> {len(lb)} lines ({len(sub(la, True))} -> {len(sub(lb, True))} ops.* calls), first difference at "
                  f"{first}: {la[first][0] if first < len(la) else None} | {lb[first][0] if first < len(lb) else None}")
        kinds.setdefault(kind, []).append(name)
        assert va.keys() == vb.keys(), (name, va.keys(), vb.keys())
        devs = {}
        for k in va:
            assert va[k][0] == vb[k][0], (name, k, "shape")
            if va[k][1] != vb[k][1]:
                dt = np.float64 if k != "info" else np.uint8
                x, y = np.frombuffer(va[k][1], dtype=dt), np.frombuffer(vb[k][1], dtype=dt)
                devs[k] = float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300))
        if devs:
            print(f"BYTES {name}: " + ", ".join(f"{k} {d:.2e} of its largest entry" for k, d in devs.items()))
        else:
            same_bytes += 1
    print(f"{len(a)} cases: {same_bytes} return identical bytes (F, every gradient, info)")
    for kind, names in kinds.items():
        print(f"  {len(names):4d} {kind}")
        for n in names:
            print("         " + n)


if __name__ == "__main__":
    {"dump": dump, "compare": compare}[sys.argv[1]](*sys.argv[2:])
