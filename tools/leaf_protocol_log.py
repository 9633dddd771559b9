"""What a KernelSpec of every kind of leaf ISSUES and RETURNS, for a tree of this repository -- the comparison recorded in
profiles/leaf_protocol_refactor.txt.

    python tools/leaf_protocol_log.py dump <tree> <out.pkl> [device]    the spec matrix below on <tree>
    python tools/leaf_protocol_log.py abi <tree> <out.pkl>              what the twelve builder wrappers of `ops` hand the C ABI, and raise
    python tools/leaf_protocol_log.py compare <a.pkl> <b.pkl>           two dumps, case by case: log lines and returned bytes
    PYTHONPATH=tools LEAF_PROTOCOL_LOG=<out.pkl> python -m pytest -p leaf_protocol_log tests/test_*_emulated.py
                                                                        as a pytest plugin: the log of every emulated test, per test id

`dump` without `device`: `gradients.ops` is the emulation of the SAME tree (tests/emulation.py's modules and the fake_* modules of
the ArcCosine, Coregion, ChangePoints and VGP tests) behind the logging proxy of tools/reverse_pass_log.py: one line per outermost
`ops.*` call -- name, shapes and strides of the tensors, every scalar and keyword, the bytes of NumPy arguments -- and one per aten op of
the glue.  With `device` nothing is patched or logged and the real library runs; kept per case either way: the bytes of everything returned.
The matrix: every member kind (stationary, RationalQuadratic, static, periodic, Linear ARD, Polynomial, ArcCosine ARD and not, Coregion)
alone, all in a Sum, in a Product of Sums with per-member `cols`, and under a ChangePoints node; n1 = 65, n2 = 63, three real columns
and one of P = 3 labels, one NaN planted in a row of X1; `build` (X2 given and None, with diag_add), every leaf's own builder with
`lower_only` both ways, `kdiag_rows`, `diag_adjoint`, `adjoint` (symmetric and not) and the nodes' gradients.

As a plugin it wraps what `emulation.primitives` returns, so the `gp` fixture of every *_emulated.py installs logging functions: the
models' elbo_and_grad / objective_and_grad on the problems those tests use are logged as the tests run them.
"""
import os
import pickle
import sys
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reverse_pass_log import _desc, _logger  # noqa: E402


def specs(g):
    """name -> KernelSpec over inputs of four columns (0 .. 2 real, 3 the label)"""
    from gpflow_amd.leaf import ArcLeaf, CoregionLeaf, DotLeaf, Leaf
    real, label = [0, 1, 2], [3]
    rng = np.random.default_rng(3)
    leaves = {"se": (Leaf("SquaredExponential", 1.3, [0.9, 1.4, 1.1]), real, None),
              "rq": (Leaf("RationalQuadratic", 0.9, 1.2, alpha=0.7), [0, 2], None),
              "white": (Leaf("White", 0.3), real, None),
              "per": (Leaf("SquaredExponential", 1.1, [1.2, 1.2, 1.8, 1.8]), [0, 1], [1.5, 3.0]),
              "lin": (DotLeaf("Linear", [0.5, 2.0, 1.25]), real, None),
              "poly": (DotLeaf("Polynomial", 0.7, offset=0.3, degree=2), [1, 2], None),
              "arc": (ArcLeaf(1, 0.9, [0.6, 1.1, 0.8], 0.4), real, None),
              "arc0": (ArcLeaf(0, 1.2, 0.7, 0.5), [0, 1], None),
              "cor": (CoregionLeaf(0.4 * rng.normal(size=(3, 2)), [0.5, 1.0, 1.5]), label, None)}
    names = list(leaves)

    def spec(members, tree, nodes=None):
        lf, cols, per = zip(*(leaves[m] for m in members))
        return g.KernelSpec(lf, tree, cols=cols, periods=per, nodes=nodes)
    out = {f"alone/{m}": (lambda m=m: spec([m], None)) for m in names}
    out["sum"] = lambda: spec(names, "add")
    out["product_of_sums"] = lambda: spec(names, ("mul", [("add", [0, 4, 6]), ("add", [1, 2, 8]), ("add", [3, 5, 7])]))
    out["changepoints"] = lambda: spec(names, ("cp", [("add", [0, 4, 3]), ("mul", [6, 8]), ("add", [1, 2, 5, 7])], 0),
                                       [g.ChangePointsNode([0.4, -0.3], [2.0, 3.0], switch_dim=1)])
    out["sum_over_changepoints"] = lambda: spec(["se", "lin", "cor", "arc"], ("add", [("cp", [0, ("mul", [1, 2])], 0), 3]),
                                                [g.ChangePointsNode([0.1], 2.5, switch_dim=0)])
    return out


def dump(tree, path, device=None):
    sys.path[:0] = [tree, tree + "/tests"]
    import torch
    from gpflow_amd import gradients as g
    from gpflow_amd import ops
    log = []
    if device is None:
        from torch.utils._python_dispatch import TorchDispatchMode
        import emulation
        import fake_arccosine_ops
        import fake_changepoints_ops
        import fake_coregion_ops
        import fake_vgp_ops
        log, depth, wrap = _logger()
        fakes = emulation.primitives(emulation.MODULES + (fake_coregion_ops, fake_vgp_ops, fake_arccosine_ops, fake_changepoints_ops))
        public = {k: v for k, v in vars(ops).items() if not k.startswith("_")}      # (the constants; a primitive without an emulation fails loudly)
        ops = g.ops = types.SimpleNamespace(**{**public, **{name: wrap(name, fn) for name, fn in fakes.items()}})

        class Glue(TorchDispatchMode):
            def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
                if depth[0] == 0:
                    log.append((str(func), tuple(_desc(a) for a in args), tuple((k, _desc(v)) for k, v in sorted((kwargs or {}).items()))))
                return func(*args, **(kwargs or {}))
    else:
        import contextlib
        Glue = contextlib.nullcontext
    rng = np.random.default_rng(5)
    n1, n2, P = 65, 63, 3
    X1 = np.concatenate([rng.normal(size=(n1, 3)), rng.integers(0, P, size=(n1, 1)).astype(np.float64)], axis=1)
    X2 = np.concatenate([rng.normal(size=(n2, 3)), rng.integers(0, P, size=(n2, 1)).astype(np.float64)], axis=1)
    X1[17, 1] = np.nan
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), device=device or "cpu")  # noqa: E731
    X1, X2 = t(X1), t(X2)
    Ks = rng.normal(size=(n1, n1))
    Ks, Kr, bar = t(Ks + Ks.T), t(rng.normal(size=(n1, n2))), t(rng.normal(size=n1))
    res = {}
    for name, make in specs(g).items():
        del log[:]
        vals = {}

        def keep(key, v):
            for i, vi in enumerate(v if isinstance(v, (list, tuple)) else [v]):
                vals[f"{key}[{i}]"] = torch.zeros(0) if vi is None else vi.detach().clone()
        with Glue():
            spec = make().warm(X1.device, X1.shape[1])
            keep("build/X2", spec.build(X1, X2))
            keep("build/sym", spec.build(X1, None, None, 0.25))
            for i, m in enumerate(spec.parts):
                for lower in (False, True):
                    keep(f"leaf{i}/lower_only={lower}", getattr(ops, m.leaf.builders[0] if hasattr(m.leaf, "builders") else m.matrix)(
                        m.view(X1), None, diag_add=0.5, lower_only=lower, **m.leaf.keywords()))
            keep("kdiag_rows", spec.kdiag_rows(X1))
            dv, dl = spec.diag_adjoint(X1, bar)
            keep("diag_adjoint/dv", dv), keep("diag_adjoint/dl", dl)
            for tag, (A, Bm, Kbar, sym) in {"sym": (X1, X1, Ks, True), "pair": (X1, X2, Kr, False)}.items():
                dv, dl, Ab = spec.adjoint(A, Bm, Kbar, sym)
                keep(f"adjoint/{tag}/dv", dv), keep(f"adjoint/{tag}/dl", dl), keep(f"adjoint/{tag}/Abar", Ab)
            for k, nd in enumerate(spec._changepoint_grads().get("changepoints", [])):
                keep(f"node{k}/locations", nd["locations"]), keep(f"node{k}/steepness", nd["steepness"])
        res[name] = (list(log), {k: (tuple(v.shape), v.contiguous().cpu().numpy().tobytes()) for k, v in vals.items()})
    with open(path, "wb") as f:
        pickle.dump(res, f)
    print(len(res), "spec cases,", sum(len(l) for l, _ in res.values()), "log lines,", sum(len(v) for _, v in res.values()), "returned tensors")


def compare(pa, pb):
    """case by case: the logs line for line, the returned tensors byte for byte (NaN positions with them)"""
    a, b = pickle.load(open(pa, "rb")), pickle.load(open(pb, "rb"))
    print("cases:", len(a), len(b), "same ids" if a.keys() == b.keys() else f"ids differ: {sorted(set(a) ^ set(b))[:10]}")
    logs = tensors = bad = 0
    for name in sorted(set(a) & set(b)):
        (la, va), (lb, vb) = a[name], b[name]
        logs += len(la)
        if la != lb:
            first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print(f"LOG   {name}: {len(la)} -> {len(lb)} lines, first difference at {first}: "
                  f"{la[first] if first < len(la) else None} | {lb[first] if first < len(lb) else None}")
            bad += 1
        if va.keys() != vb.keys():
            print(f"KEYS  {name}: {sorted(set(va) ^ set(vb))}")
            bad += 1
        for k in sorted(set(va) & set(vb)):
            tensors += 1
            if va[k] != vb[k]:
                print(f"BYTES {name}: {k}")
                bad += 1
    print(f"{logs} log lines, {tensors} returned tensors compared: {bad} differences")
    return bad


def abi(tree, path):
    """what the twelve kernel-matrix and row-diagonal wrappers of <tree>'s `ops` hand the C ABI -- entry point and every argument, a
    pointer as the name of the tensor it points into -- and what they raise for an input with one fault, on CPU tensors: the library
    is a recorder that returns 0, and `ops._chk` is restated without the test for a device tensor"""
    sys.path[:0] = [tree]
    import ctypes
    import torch
    from gpflow_amd import _lib, ops
    calls, names = [], {}

    def show(a):
        if isinstance(a, ctypes.Array):
            return list(a)
        if isinstance(a, int) and not isinstance(a, bool) and a > 2 ** 32:
            return "&" + names.get(a, "table")
        return repr(a)

    class Recorder:
        def __getattr__(self, entry):
            return lambda *args: calls.append((entry, tuple(show(a) for a in args))) or 0

    def chk(t, name, ndim=None):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch tensor, got {type(t)}")
        if t.dtype != torch.float64:
            raise _lib.GpkError(f"{name}: dtype must be float64 (got {t.dtype})")
        if ndim is not None and t.dim() != ndim:
            raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    _lib.load, _lib.check, ops._chk, ops._stream = Recorder, (lambda rc, what: calls.append(("check", what))), chk, (lambda: 0)
    rng = np.random.default_rng(1)
    T = lambda *shape: torch.tensor(rng.normal(size=shape))  # noqa: E731
    E = lambda *shape: torch.empty(*shape, dtype=torch.float64)  # noqa: E731
    n1, n2, d = 5, 4, 3
    leaves = {"": dict(variance=1.3, lengthscales=[0.9, 1.4, 1.1]), "dot_": dict(family="Polynomial", variance=[0.5, 2.0, 1.2], offset=0.3, degree=2),
              "arccos_": dict(order=1, variance=0.9, weight_variances=[0.6, 1.1, 0.8], bias_variance=0.4),
              "coregion_": dict(W=0.1 * np.arange(6.0).reshape(3, 2), kappa=[0.5, 1.0, 1.5])}
    bad_leaf = {"": [dict(family="Nope"), dict(lengthscales=[1.0, 2.0]), dict(alpha=0.5), dict(family="RationalQuadratic")],
                "dot_": [dict(family="Nope"), dict(variance=[1.0, 2.0]), dict(degree=2.5), dict(family="Linear")],
                "arccos_": [dict(order=3), dict(weight_variances=[1.0, 2.0]), dict(weight_variances=np.ones((2, 2)))],
                "coregion_": [dict(kappa=[1.0, 2.0]), dict(W=np.ones(3))]}
    res = {}

    def run(key, fn, *args, **kw):
        del calls[:]
        names.clear()
        names.update({a.data_ptr(): f"arg{i}" for i, a in enumerate(args) if isinstance(a, torch.Tensor)})
        names.update({v.data_ptr(): k for k, v in kw.items() if isinstance(v, torch.Tensor)})
        try:
            out = fn(*args, **kw)
            end = ("returned", tuple(out.shape), "out" if any(out is v for v in kw.values()) else "new")
        except Exception as e:  # noqa: BLE001  (the type and the text are what is compared)
            end = ("raised", type(e).__name__, str(e))
        res[key] = (list(calls), {repr(end): ((), b"")})
    for prefix, kw in leaves.items():
        w = 1 if prefix == "coregion_" else d
        X1, X2, G, Gs, g = T(n1, w), T(n2, w), T(n1, n2), T(n1, n1), T(n1)
        matrix, combine, diag = (getattr(ops, prefix + f) for f in ("kernel_matrix", "kernel_matrix_combine", "kernel_diag")) if prefix else \
            (ops.kernel_matrix, ops.kernel_matrix_combine, None)
        pair = {"matrix": (matrix, (), {}), "combine": (combine, (G,), dict(op="mul"))}
        if not prefix:
            pair["hadamard"] = (ops.kernel_matrix_hadamard, (G,), {})
        for which, (fn, more, okw) in pair.items():
            k = f"{prefix}{which}"
            sym = which != "hadamard"
            run(k + "/pair", fn, X1, X2, *more, **okw, **kw)
            run(k + "/pair/out", fn, X1, X2, *more, out=E(n1, 8)[:, :n2], **okw, **kw)
            if sym:
                run(k + "/sym", fn, X1, None, *((Gs,) if more else ()), diag_add=0.25, **okw, **kw)
                for op in ("add", "dr2", "dalpha", "ds", "dp", "k", "nope") if more else ():
                    run(k + f"/op={op}", fn, X1, None, Gs, **dict(okw, op=op), **kw)
            if which == "matrix":
                run(k + "/lower_only", fn, X1, None, lower_only=True, **kw)
            run(k + "/no rows", fn, X1[:0], X2, *((G[:0],) if more else ()), **okw, **kw)
            run(k + "/no columns", fn, X1, X2[:0], *((G[:, :0],) if more else ()), **okw, **kw)
            for tag, b in enumerate(bad_leaf[prefix]):
                run(k + f"/bad leaf {tag}", fn, X1, X2, *more, **okw, **dict(kw, **b))
                run(k + f"/bad leaf {tag}, no rows", fn, X1[:0], X2, *((G[:0],) if more else ()), **okw, **dict(kw, **b))
            faults = {"X1 an array": (X1.numpy(), X2), "X1 float32": (X1.float(), X2), "X1 [n]": (X1[:, 0], X2), "X2 [n]": (X1, X2[:, 0]),
                      "X2 narrower": (X1, T(n2, w + 1)), "X1 transposed": (T(w + 1, n1).T[:, :w + 1][:, :w] if w > 1 else T(2, n1).T[:, :1], X2),
                      "too wide": (T(n1, 65), T(n2, 65)), "two columns": (T(n1, 2), T(n2, 2))}
            for tag, (a, b) in faults.items():
                run(k + "/" + tag, fn, a, b, *more, **okw, **kw)
            if more:
                run(k + "/G of another shape", fn, X1, X2, G[:, :3], **okw, **kw)
                run(k + "/G transposed", fn, X1, X2, T(n2, n1).T, **okw, **kw)
            run(k + "/out [n]", fn, X1, X2, *more, out=E(n1), **okw, **kw)
            run(k + "/out transposed", fn, X1, X2, *more, out=E(n2, n1).T, **okw, **kw)
        if diag is None:
            continue
        k = prefix + "diag"
        run(k + "/k", diag, X1, **kw)
        run(k + "/k/out", diag, X1, out=E(n1), **kw)
        for op in ("mul", "add", "ds", "dp", "dr2", "nope"):
            run(k + f"/op={op}", diag, X1, g, op=op, out=g, **kw)
        run(k + "/no rows", diag, X1[:0], **kw)
        for tag, b in enumerate(bad_leaf[prefix]):
            run(k + f"/bad leaf {tag}", diag, X1, **dict(kw, **b))
            run(k + f"/bad leaf {tag}, no rows", diag, X1[:0], **dict(kw, **b))
        faults = {"X an array": ((X1.numpy(),), {}), "X [n]": ((X1[:, 0],), {}), "too wide": ((T(n1, 65),), {}), "two columns": ((T(n1, 2),), {}),
                  "g without an op": ((X1, g), {}), "op without g": ((X1,), dict(op="mul")), "g too long": ((X1, T(n1 + 1)), dict(op="mul")),
                  "g strided": ((X1, T(n1, 2)[:, 0]), dict(op="mul")), "g [n, 1]": ((X1, T(n1, 1)), dict(op="mul")),
                  "out too long": ((X1,), dict(out=E(n1 + 1))), "out strided": ((X1,), dict(out=E(n1, 2)[:, 0])),
                  "out float32": ((X1,), dict(out=torch.empty(n1, dtype=torch.float32)))}
        for tag, (args, okw) in faults.items():
            run(k + "/" + tag, diag, *args, **okw, **kw)
    with open(path, "wb") as f:
        pickle.dump(res, f)
    print(len(res), "wrapper cases:", sum(1 for _, v in res.values() if "raised" in next(iter(v))), "raise,", sum(len(l) for l, _ in res.values()), "recorded calls")


# ---- as a pytest plugin: the log of every emulated test
_TESTS, _LOG = {}, []


def pytest_configure(config):
    sys.path.insert(0, os.path.join(str(config.rootpath), "tests"))
    import emulation
    log, depth, wrap = _logger()
    plain = emulation.primitives
    emulation.primitives = lambda *a, **kw: {name: wrap(name, fn) for name, fn in plain(*a, **kw).items()}
    _LOG.append(log)


def pytest_runtest_setup(item):
    del _LOG[0][:]


def pytest_runtest_logreport(report):
    if report.when == "call":
        _TESTS[report.nodeid] = (list(_LOG[0]), {"outcome:" + report.outcome: ((), b"")})


def pytest_sessionfinish(session):
    if os.environ.get("LEAF_PROTOCOL_LOG"):
        with open(os.environ["LEAF_PROTOCOL_LOG"], "wb") as f:
            pickle.dump(_TESTS, f)


if __name__ == "__main__":
    sys.exit({"dump": dump, "abi": abi, "compare": compare}[sys.argv[1]](*sys.argv[2:]) or 0)
