"""What the reverse pass ISSUES, and what it returns, for a tree of this repository -- no device needed.

    python tools/reverse_pass_log.py dump  <tree> <out.pkl>     run the matrix below on <tree>'s gpflow_amd/gradients.py
    python tools/reverse_pass_log.py dump-models <tree> <out.pkl> [device]
                                                                the MODEL layer of <tree> (`model_cases`): what SVGP.elbo_and_grad, GPR /
                                                                SGPR.objective_and_grad, SVGPTrainer and NaturalGradient issue and return
    python tools/reverse_pass_log.py compare <a.pkl> <b.pkl>    compare two dumps case by case

`gradients.ops` is the whole emulation of the SAME tree (`primitives()` of its tests/emulation.py: every name of every tests/fake_*.py,
each defined once) behind a logging proxy: one line per outermost
`ops.*` call (name, shape and strides of every tensor argument, every scalar argument); a TorchDispatchMode adds one line per aten op
issued OUTSIDE an `ops.*` call (the torch glue).  Each case runs twice and the second run is kept (`ls_device` caches).  Kept per
case: the log and the bytes of F, every gradient and info; a refusal is kept as its exception type and message (a spec without a
constant diagonal under a quadrature likelihood or in sgpr_elbo_and_grad).  Written for the refactor recorded in
profiles/reverse_pass_refactor.txt.

`dump-models` patches every `gpflow_amd.ops` name the emulation defines (the same `primitives()`, what `emulation.install` patches
in the tests) behind the same logging wrapper -- or, with `device`, patches nothing and logs nothing: the same matrix on the real library.
A tree from before tests/emulation.py existed is dumped with ITS OWN copy of this tool (profiles/emulation_refactor.txt).  Kept per
case: the `ops.*` log, the returned value, every gradient under a key that carries its position in the returned dict and the
position of its Parameter in `model.parameters`; for the trainer F, every `u` / `dev` entry after two steps and the names of `host` in
order (in the key); for a fused forward call (kind "value") the returned value alone.  A refusal is kept as its exception type and message.  The model functions run twice on one model: `<case>` is the second run
(Parameter.device_value caches warm), `<case>#cold` the first.  Written for the refactor recorded in profiles/model_layer_refactor.txt;
the RationalQuadratic / Exponential / White / Constant leaves and the LinearCoregionalization models were added for the one recorded
in profiles/kernel_leaf_refactor.txt; the Periodic and dot-product (Linear, Polynomial) leaves and their trees for the one recorded in
profiles/kernel_members_refactor.txt.
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


def _logger():
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
    return log, depth, wrap


def load(tree):
    sys.path[:0] = [tree, tree + "/tests"]
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    import emulation
    from gpflow_amd import gradients
    log, depth, wrap = _logger()
    gradients.ops = types.SimpleNamespace(**{name: wrap(name, fn) for name, fn in emulation.primitives().items()})

    class Glue(TorchDispatchMode):
        def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
            if depth[0] == 0:
                log.append((str(func), tuple(_desc(a) for a in args), tuple((k, _desc(v)) for k, v in sorted((kwargs or {}).items()))))
            return func(*args, **(kwargs or {}))

    return torch, gradients, log, Glue


def kernels(g, D=3):
    from gpflow_amd.leaf import DotLeaf, Leaf
    ard = np.sqrt(D) * (0.8 + 0.05 * np.arange(D))
    lin, lin_ard = DotLeaf("Linear", 0.8), DotLeaf("Linear", [0.5, 2.0, 1.25])
    poly2, poly1 = DotLeaf("Polynomial", 0.7, offset=0.3, degree=2), DotLeaf("Polynomial", [0.4, 0.9, 0.6], offset=0.5, degree=1)
    # a periodic member's leaf is in the device form: lengthscales 2 l over the warped columns, an ARD one repeated pairwise
    per_se = Leaf("SquaredExponential", 1.3, 2 * 0.9)
    per_se_ard = Leaf("SquaredExponential", 1.3, [1.2, 1.2, 1.8, 1.8, 2.6, 2.6])
    per_rq = Leaf("RationalQuadratic", 0.9, [1.0, 1.0, 4.0, 4.0], alpha=0.7)
    se, m32, m52 = ("SquaredExponential", 1.3, ard), ("Matern32", 0.7, np.array(1.3)), ("Matern52", 0.9, np.array(0.8))
    return {
        "se_ard": lambda: dict(variance=1.3, lengthscales=ard),
        "m32_iso": lambda: dict(variance=0.7, lengthscales=1.3, family="Matern32"),
        "sum2": lambda: dict(kernel_spec=g.KernelSpec([se, m32], "add")),
        "prod2_cols": lambda: dict(kernel_spec=g.KernelSpec([("SquaredExponential", 1.3, ard[:2]), m32], "mul", [[0, 1], [2]])),
        "nested": lambda: dict(kernel_spec=g.KernelSpec([se, m32, m52], ("mul", [("add", [0, 1]), 2]))),
        # the families with an extra hyperparameter or without lengthscales: by keywords, and as members
        "rq_iso": lambda: dict(variance=0.9, lengthscales=1.1, family="RationalQuadratic", alpha=0.7),
        "rq_ard": lambda: dict(variance=0.9, lengthscales=ard, family="RationalQuadratic", alpha=1.7),
        "exp_iso": lambda: dict(variance=1.1, lengthscales=1.4, family="Exponential"),
        "const_rq_white": lambda: dict(kernel_spec=g.KernelSpec([("Constant", 2.0, 1.0), ("RationalQuadratic", 0.5, ard, 0.7),
                                                                 ("White", 0.1, 1.0, None)], "add")),
        "prod_static": lambda: dict(kernel_spec=g.KernelSpec([se, ("Constant", 2.0, 1.0)], "mul")),
        "nested_rq_cols": lambda: dict(kernel_spec=g.KernelSpec([se, ("RationalQuadratic", 0.6, np.array(1.2), 1.3), m52],
                                                                ("mul", [("add", [0, 1]), 2]), [None, [0, 2], None])),
        # dot-product leaves (a diagonal that depends on the row), periodic members (warped inputs, a period gradient), and their trees
        "lin_iso": lambda: dict(kernel_spec=g.KernelSpec([lin])),
        "lin_ard": lambda: dict(kernel_spec=g.KernelSpec([lin_ard])),
        "poly2": lambda: dict(kernel_spec=g.KernelSpec([poly2])),
        "poly1_ard": lambda: dict(kernel_spec=g.KernelSpec([poly1])),
        "per_se": lambda: dict(kernel_spec=g.KernelSpec([per_se], periods=[1.5])),
        "per_rq_cols": lambda: dict(kernel_spec=g.KernelSpec([per_rq], cols=[[0, 2]], periods=[[1.5, 3.0]])),
        "sum_lin_se": lambda: dict(kernel_spec=g.KernelSpec([lin_ard, se], "add")),
        "prod_m32_poly": lambda: dict(kernel_spec=g.KernelSpec([m32, poly2], "mul")),
        "three_level": lambda: dict(kernel_spec=g.KernelSpec(
            [lin_ard, per_se_ard, poly2, Leaf("White", 0.3), Leaf("RationalQuadratic", 0.6, 0.5, alpha=0.7)],
            ("add", [("mul", [("add", [0, 1]), ("add", [2, 3])]), 4]), [None, None, None, None, [0, 2]],
            [None, [2.5, 3.0, 3.5], None, None, None])),
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
        if lik in liks and kname not in ("se_ard", "m32_iso", "rq_iso", "lin_ard", "per_se", "sum_lin_se"):
            continue   # (refused by SVGP.elbo_and_grad: a quadrature likelihood needs one stationary kernel; here a row diagonal is refused)
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
            try:
                for _ in range(2):
                    del log[:]
                    with Glue():
                        F, grads, info = getattr(g, fn)(*args, **kw, **kmk())
            except (NotImplementedError, ValueError) as e:
                res[f"chunks{chunks}/{name}"] = (list(log), {f"refused:{type(e).__name__}:{e}": ((), b"")})
                continue
            vals = {"F": F, "info": info}
            for k, v in grads.items():
                for i, vi in enumerate(v if isinstance(v, list) else [v]):   # (None: a member without that entry, kept as an empty one)
                    vals[(f"{k}[{i}]" if isinstance(v, list) else k) + ("=None" if vi is None else "")] = torch.zeros(0) if vi is None else vi
            res[f"chunks{chunks}/{name}"] = (list(log), {k: (tuple(v.shape), v.detach().contiguous().numpy().tobytes()) for k, v in vals.items()})
    with open(path, "wb") as f:
        pickle.dump(res, f)
    n_ops = sum(1 for e in res["chunks1/white/full/scalar/se_ard/P2"][0] if e[0].startswith("ops."))
    print(len(res), "cases; benchmark form (M = 64, P = 2):", n_ops, "ops.* calls,",
          len(res["chunks1/white/full/scalar/se_ard/P2"][0]) - n_ops, "aten ops")
    print([e[0][4:] for e in res["chunks1/white/full/scalar/se_ard/P2"][0] if e[0].startswith("ops.")])
    refused = [n for n, (_, v) in res.items() if any(k.startswith("refused:") for k in v)]
    print(len(refused), "refusals:", sorted({next(iter(res[n][1])) for n in refused}))


def model_cases(gp):
    """[(name, kind, make)] of the model-layer matrix at M = 20, N = 64, D = 3.  kind "grad": make() -> (model, function returning
    (value, {Parameter: gradient})); "trainer": make() -> (model, trainer kwargs, data); "natgrad": make() -> (model, data)."""
    K, L, IV, F = gp.kernels, gp.likelihoods, gp.inducing_variables, gp.functions
    M, N, D = 20, 64, 3
    rng = np.random.default_rng(11)
    X, Z = rng.normal(size=(N, D)), rng.normal(size=(M, D))
    Y2 = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(N, 2))
    q_mu = 0.3 * rng.normal(size=(M, 3))
    q_full = np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(3)])
    q_diag = 0.4 + 0.2 * np.abs(rng.normal(size=(M, 3)))
    se = lambda **kw: K.SquaredExponential(variance=1.3, lengthscales=0.9, **kw)  # noqa: E731
    m32 = lambda **kw: K.Matern32(variance=0.7, lengthscales=1.3, **kw)  # noqa: E731
    pts = lambda dz=0.0: IV.InducingPoints(Z + dz)  # noqa: E731

    def shared_sum():
        k0 = se()
        return k0 + k0
    plain = {"se": se, "m32_active": lambda: m32(active_dims=[0, 2]), "sum_shared": shared_sum,
             "nested": lambda: (se() + m32(active_dims=[1])) * K.Matern52(variance=0.9, lengthscales=0.8)}
    multi = {"shared": lambda: (K.SharedIndependent(se(), 2), IV.SharedIndependentInducingVariables(pts())),
             "sep_shared_z": lambda: (K.SeparateIndependent([se(), m32()]), IV.SharedIndependentInducingVariables(pts())),
             "sep_separate_z": lambda: (K.SeparateIndependent([se(), m32()]),
                                        IV.SeparateIndependentInducingVariables([pts(), pts(0.1)]))}
    noise = {"const": lambda: L.Gaussian(0.2),
             "het": lambda: L.Gaussian(scale=F.Linear(A=np.array([[-0.1], [0.05], [0.02]]), b=np.array([0.6])))}

    def svgp(kname, lik, *, whiten=True, diag=False, mean=None, P=None, num_data=5 * N):
        k, iv = multi[kname]() if kname in multi else (plain[kname](), Z.copy())
        P = (2 if kname in multi else 1) if P is None else P
        return gp.models.SVGP(k, lik, iv, q_mu=q_mu[:, :P].copy(), q_sqrt=(q_diag[:, :P] if diag else q_full[:P]).copy(), q_diag=diag,
                              whiten=whiten, num_latent_gps=P, num_data=num_data, mean_function=mean)

    def svgp_over(k, iv, lik, P):
        return gp.models.SVGP(k, lik, iv, q_mu=q_mu[:, :P].copy(), q_sqrt=q_full[:P].copy(), num_latent_gps=P, num_data=5 * N)
    shared_pts = lambda: IV.SharedIndependentInducingVariables(pts())  # noqa: E731
    # SeparateIndependent at its edges: a member that is a Sum (refused), ONE member (still "separate": kvar_ / kls_ names, one output
    # column per member), the same InducingPoints object twice in a SeparateIndependentInducingVariables (refused by the trainer)
    sep_edge = {"sep_sum_member": lambda lik=None: svgp_over(K.SeparateIndependent([se() + m32(), se()]), shared_pts(), lik or L.Gaussian(0.2), 2),
                "sep_one_member": lambda lik=None: svgp_over(K.SeparateIndependent([se()]), shared_pts(), lik or L.Gaussian(0.2), 1)}

    def same_points_twice():
        p0 = pts()
        return svgp_over(K.SeparateIndependent([se(), m32()]), IV.SeparateIndependentInducingVariables([p0, p0]), L.Gaussian(0.2), 2)

    def elbo_case(mk, Y):
        def make():
            m = mk()
            return m, lambda: m.elbo_and_grad((X, Y))
        return make
    out = []
    for wh, diag, kname, nz in itertools.product((True, False), (False, True), (*plain, *multi), noise):
        out.append((f"svgp/{'white' if wh else 'unwhite'}/{'diag' if diag else 'full'}/{kname}/{nz}", "grad",
                    elbo_case(lambda wh=wh, diag=diag, kname=kname, nz=nz: svgp(kname, noise[nz](), whiten=wh, diag=diag),
                              Y2[:, :2 if kname in multi else 1])))
    liks = {"bernoulli": (L.Bernoulli, 1, (Y2[:, :1] > 0).astype(np.float64)), "poisson": (L.Poisson, 1, np.floor(np.exp(Y2[:, :1]))),
            "student_t": (L.StudentT, 1, Y2[:, :1]), "multiclass3": (lambda: L.MultiClass(3), 3, rng.integers(0, 3, size=(N, 1)).astype(np.float64))}
    for (lname, (mk, P, Yl)), diag in itertools.product(liks.items(), (False, True)):
        out.append((f"svgp/quadrature/{lname}/{'diag' if diag else 'full'}", "grad",
                    elbo_case(lambda mk=mk, P=P, diag=diag: svgp("se", mk(), diag=diag, P=P), Yl)))
    # quadrature likelihoods outside their narrower scope (refused)
    for tag, kw, kname in (("unwhite", dict(whiten=False), "se"), ("active", {}, "m32_active"), ("sum", {}, "sum_shared")):
        out.append((f"svgp/quadrature/bernoulli/{tag}", "grad",
                    elbo_case(lambda kw=kw, kname=kname: svgp(kname, L.Bernoulli(), **kw), liks["bernoulli"][2])))

    def frozen_ls():
        m = svgp("se", L.Gaussian(0.2))
        gp.set_trainable(m.kernel.lengthscales, False)
        return m

    def with_prior(m):
        m.kernel.variance.prior = gp.priors.LogNormal(0.1, 0.8)
        return m
    extra = {"constant_mean": lambda: svgp("se", L.Gaussian(0.2), mean=gp.mean_functions.Constant(0.25)),
             "constant_mean_sum": lambda: svgp("sum_shared", L.Gaussian(0.2), mean=gp.mean_functions.Constant(0.25)),
             "frozen_lengthscale": frozen_ls, "variance_prior": lambda: with_prior(svgp("se", L.Gaussian(0.2))),
             "no_num_data": lambda: svgp("se", L.Gaussian(0.2), num_data=None),
             "linear_mean": lambda: svgp("se", L.Gaussian(0.2), mean=gp.mean_functions.Linear(A=np.ones((D, 1)), b=np.zeros(1))),
             "odd_member": lambda: gp.models.SVGP(se() + K.SeparateIndependent([se()]), L.Gaussian(0.2), Z.copy()),
             "shared_sum": lambda: gp.models.SVGP(K.SharedIndependent(shared_sum(), 1), L.Gaussian(0.2),
                                                  IV.SharedIndependentInducingVariables(pts()), num_latent_gps=1),
             "separate_over_points": lambda: gp.models.SVGP(K.SeparateIndependent([se()]), L.Gaussian(0.2), Z.copy())}
    for name, mk in extra.items():
        out.append((f"svgp/extra/{name}", "grad", elbo_case(mk, Y2[:, :1])))
    out.append(("svgp/extra/sep_sum_member", "grad", elbo_case(sep_edge["sep_sum_member"], Y2[:, :2])))
    out.append(("svgp/extra/sep_one_member", "grad", elbo_case(sep_edge["sep_one_member"], Y2[:, :1])))
    out.append(("svgp/extra/sep_one_member_het", "grad", elbo_case(lambda: sep_edge["sep_one_member"](noise["het"]()), Y2[:, :1])))
    out.append(("svgp/extra/sep_same_points_twice", "grad", elbo_case(same_points_twice, Y2[:, :2])))
    for cls, (kname, nz) in itertools.product(("gpr", "sgpr"), itertools.product(plain, noise)):
        def make(cls=cls, kname=kname, nz=nz):
            m = gp.models.GPR((X, Y2), plain[kname](), likelihood=noise[nz]()) if cls == "gpr" else \
                gp.models.SGPR((X, Y2), plain[kname](), Z.copy(), likelihood=noise[nz]())
            return m, m.objective_and_grad
        out.append((f"{cls}/{kname}/{nz}", "grad", make))
    for cls in ("gpr", "sgpr"):
        def make(cls=cls):
            m = gp.models.GPR((X, Y2), se(), mean_function=gp.mean_functions.Constant(0.25), noise_variance=0.2) if cls == "gpr" else \
                gp.models.SGPR((X, Y2), se(), Z.copy(), mean_function=gp.mean_functions.Constant(0.25), noise_variance=0.2)
            return m, m.objective_and_grad
        out.append((f"{cls}/constant_mean", "grad", make))
        def linear_mean(cls=cls):
            mf = gp.mean_functions.Linear(A=np.ones((D, 2)), b=np.zeros(2))
            m = gp.models.GPR((X, Y2), se(), mean_function=mf) if cls == "gpr" else gp.models.SGPR((X, Y2), se(), Z.copy(), mean_function=mf)
            return m, m.objective_and_grad
        out.append((f"{cls}/linear_mean", "grad", linear_mean))

        def noise_scale(cls=cls):   # (a constant noise that is not a `variance` Parameter; the SGPR says so after its _config)
            m = gp.models.GPR((X, Y2), se(), likelihood=L.Gaussian(scale=0.4)) if cls == "gpr" else \
                gp.models.SGPR((X, Y2), se(), Z.copy(), likelihood=L.Gaussian(scale=0.4))
            return m, m.objective_and_grad
        out.append((f"{cls}/noise_scale", "grad", noise_scale))
    trainers = {"single": (lambda: svgp("se", L.Gaussian(0.2), mean=gp.mean_functions.Constant(0.25)), {}),
                "unwhite_single": (lambda: svgp("se", L.Gaussian(0.2), whiten=False), {}),
                "diag_active": (lambda: svgp("m32_active", L.Gaussian(0.2), diag=True), {}),
                "sum_shared": (lambda: svgp("sum_shared", L.Gaussian(0.2)), {}),
                "nested": (lambda: svgp("nested", L.Gaussian(0.2), whiten=False), {}),
                "shared": (lambda: svgp("shared", L.Gaussian(0.2)), {}),
                "sep_shared_z": (lambda: svgp("sep_shared_z", L.Gaussian(0.2)), {}),
                "het": (lambda: svgp("se", noise["het"]()), {}),
                "het_sep": (lambda: svgp("sep_shared_z", noise["het"]()), {}),
                "het_nested": (lambda: svgp("nested", noise["het"]()), {}),
                "natgrad": (lambda: svgp("se", L.Gaussian(0.2)), dict(natgrad_gamma=0.5)),
                "variance_prior": (lambda: with_prior(svgp("se", L.Gaussian(0.2))), {}),
                "sep_one_member": (sep_edge["sep_one_member"], {}),
                # refused
                "sep_one_member_two_columns": (sep_edge["sep_one_member"], {}),     # (by step: ValueError)
                "sep_sum_member": (sep_edge["sep_sum_member"], {}),
                "sep_same_points_twice": (same_points_twice, {}),
                "sep_separate_z": (lambda: svgp("sep_separate_z", L.Gaussian(0.2)), {}),
                "diag_natgrad": (lambda: svgp("se", L.Gaussian(0.2), diag=True), dict(natgrad_gamma=0.5)),
                "bernoulli": (lambda: svgp("se", L.Bernoulli()), {}),
                "linear_mean": (extra["linear_mean"], {})}
    for name, (mk, kw) in trainers.items():
        P = 2 if name in ("shared", "sep_shared_z", "het_sep", "sep_separate_z", "sep_one_member_two_columns", "sep_sum_member",
                          "sep_same_points_twice") else 1
        out.append((f"trainer/{name}", "trainer", lambda mk=mk, kw=kw, P=P: (mk(), dict(learning_rate=1e-2, **kw), (X, Y2[:, :P]))))
    nat = {"accepted": lambda: svgp("se", L.Gaussian(0.2)), "accepted_unwhite_shared": lambda: svgp("shared", L.Gaussian(0.2), whiten=False),
           "active": lambda: svgp("m32_active", L.Gaussian(0.2)), "diag": lambda: svgp("se", L.Gaussian(0.2), diag=True),
           "het": lambda: svgp("se", noise["het"]()), "sum": lambda: svgp("sum_shared", L.Gaussian(0.2)),
           "separate": lambda: svgp("sep_shared_z", L.Gaussian(0.2)), "bernoulli": lambda: svgp("se", L.Bernoulli())}
    for name, mk in nat.items():
        P = 2 if name in ("accepted_unwhite_shared", "separate") else 1
        out.append((f"natgrad/{name}", "natgrad", lambda mk=mk, P=P: (mk(), (X, Y2[:, :P]))))
    # ---- leaves with an extra hyperparameter (RationalQuadratic) or without lengthscales (White, Constant), and LinearCoregionalization
    rq = lambda **kw: K.RationalQuadratic(variance=1.1, lengthscales=0.9, alpha=0.7, **kw)  # noqa: E731
    leaves = {"rq": rq, "rq_ard_active": lambda: K.RationalQuadratic(variance=1.1, lengthscales=[0.9, 1.2], alpha=1.7, active_dims=[0, 2]),
              "se_white": lambda: se() + K.White(0.3), "const_times_rq": lambda: K.Constant(2.0) * rq()}

    def model_over(cls, k, lik=None, P=1):
        lik = lik or L.Gaussian(0.2)
        if cls == "svgp":
            return svgp_over(k, Z.copy(), lik, P)
        return gp.models.GPR((X, Y2), k, likelihood=lik) if cls == "gpr" else gp.models.SGPR((X, Y2), k, Z.copy(), likelihood=lik)
    for cls, (kname, mk) in itertools.product(("svgp", "gpr", "sgpr"), leaves.items()):
        def make(cls=cls, mk=mk):
            m = model_over(cls, mk())
            return m, (lambda: m.elbo_and_grad((X, Y2[:, :1]))) if cls == "svgp" else m.objective_and_grad
        out.append((f"leaf/{cls}/{kname}", "grad", make))

    def value_case(mk, fn):
        def make():
            m = mk()
            return m, lambda: fn(m)
        return make
    sep = lambda members: svgp_over(K.SeparateIndependent(members), shared_pts(), L.Gaussian(0.2), len(members))  # noqa: E731
    forward = {"svgp/rq": (lambda: model_over("svgp", rq()), lambda m: m.elbo((X, Y2[:, :1]))),
               "svgp/white": (lambda: model_over("svgp", K.White(0.3)), lambda m: m.elbo((X, Y2[:, :1]))),
               "svgp/constant_bernoulli": (lambda: model_over("svgp", K.Constant(2.0), L.Bernoulli()), lambda m: m.elbo((X, liks["bernoulli"][2]))),
               "svgp/rq_bernoulli": (lambda: model_over("svgp", rq(), L.Bernoulli()), lambda m: m.elbo((X, liks["bernoulli"][2]))),
               "gpr/rq": (lambda: model_over("gpr", rq()), lambda m: m.log_marginal_likelihood()),
               "gpr/constant": (lambda: model_over("gpr", K.Constant(2.0)), lambda m: m.log_marginal_likelihood()),
               "sep/se_exponential_ard": (lambda: sep([se(), K.Exponential(variance=0.8, lengthscales=[1.1, 0.7, 1.3])]), lambda m: m.elbo((X, Y2))),
               "sep/se_white": (lambda: sep([se(), K.White(0.3)]), lambda m: m.elbo((X, Y2))),
               "sep/rq_member": (lambda: sep([se(), rq()]), lambda m: m.elbo((X, Y2)))}                 # (refused: no slot for alpha)
    for name, (mk, fn) in forward.items():
        out.append((f"forward/{name}", "value", value_case(mk, fn)))
    Wmix = 0.5 * rng.normal(size=(2, 3))

    def lcm(members=None, separate_z=False):
        ks = members or [se(), m32(), K.Matern52(variance=0.8, lengthscales=[1.1, 0.7, 1.3])]   # (the fused shard's emulation: fake_ops' families)
        iv = IV.SeparateIndependentInducingVariables([pts(0.1 * i) for i in range(3)]) if separate_z else shared_pts()
        return svgp_over(K.LinearCoregionalization(ks, Wmix.copy()), iv, L.Gaussian(0.2), 3)
    out.append(("lcm/elbo", "value", value_case(lcm, lambda m: m.elbo((X, Y2)))))
    out.append(("lcm/elbo_separate_z", "value", value_case(lambda: lcm(separate_z=True), lambda m: m.elbo((X, Y2)))))
    out.append(("lcm/elbo_rq_member", "value", value_case(lambda: lcm([se(), rq(), m32()]), lambda m: m.elbo((X, Y2)))))   # (refused)
    out.append(("lcm/elbo_and_grad", "grad", elbo_case(lcm, Y2)))
    out.append(("lcm/elbo_and_grad_rq_white", "grad", elbo_case(lambda: lcm([se(), rq(), K.White(0.3)], separate_z=True), Y2)))
    for name, mk in (("rq", rq), ("se_white", leaves["se_white"]), ("constant", lambda: K.Constant(2.0))):                 # (refused)
        out.append((f"trainer/leaf_{name}", "trainer", lambda mk=mk: (model_over("svgp", mk()), dict(learning_rate=1e-2), (X, Y2[:, :1]))))
    # ---- dot-product leaves (Linear, Polynomial: K(x, x) depends on the row), Periodic (warped inputs, a period), and trees of them
    lin = lambda **kw: K.Linear(variance=0.8, **kw)  # noqa: E731
    lin_ard = lambda: K.Linear(variance=[0.5, 2.0, 1.25])  # noqa: E731
    poly2 = lambda: K.Polynomial(2, variance=0.7, offset=0.3)  # noqa: E731
    per_se = lambda: K.Periodic(se(), period=1.5)  # noqa: E731

    def three_level():
        per = K.Periodic(K.SquaredExponential(variance=1.3, lengthscales=[0.6, 0.9, 1.3]), period=[2.5, 3.0, 3.5])
        return (lin_ard() + per) * (poly2() + K.White(variance=0.3)) + K.RationalQuadratic(variance=0.6, lengthscales=0.5, alpha=0.7,
                                                                                             active_dims=[0, 2])
    members = {"lin_iso": lin, "lin_ard": lin_ard, "poly2": poly2,
               "poly1_ard_active": lambda: K.Polynomial(1, variance=[0.4, 0.9], offset=0.5, active_dims=[2, 0]),
               "per_se": per_se,
               "per_rq_cols": lambda: K.Periodic(K.RationalQuadratic(variance=1.1, lengthscales=[0.9, 1.2], alpha=1.7, active_dims=[0, 2]),
                                                 period=[1.5, 3.0]),
               "sum_lin_se": lambda: lin_ard() + se(), "prod_m32_poly": lambda: m32() * poly2(), "three_level": three_level}
    for (kname, mk), wh, diag in itertools.product(members.items(), (True, False), (False, True)):
        def make(mk=mk, wh=wh, diag=diag):
            m = gp.models.SVGP(mk(), L.Gaussian(0.2), Z.copy(), q_mu=q_mu[:, :1].copy(), q_sqrt=(q_diag[:, :1] if diag else q_full[:1]).copy(),
                               q_diag=diag, whiten=wh, num_latent_gps=1, num_data=5 * N)
            return m, lambda: m.elbo_and_grad((X, Y2[:, :1]))
        out.append((f"member/svgp/{'white' if wh else 'unwhite'}/{'diag' if diag else 'full'}/{kname}", "grad", make))
    for cls, (kname, mk) in itertools.product(("gpr", "sgpr"), members.items()):     # (SGPR refuses a row diagonal)
        def make(cls=cls, mk=mk):
            m = model_over(cls, mk())
            return m, m.objective_and_grad
        out.append((f"member/{cls}/{kname}", "grad", make))
    # refused: a row diagonal outside the plain routes, a Periodic member in the trainer
    for kname in ("lin_iso", "sum_lin_se"):
        out.append((f"member/quadrature/{kname}", "grad",
                    elbo_case(lambda kname=kname: model_over("svgp", members[kname](), L.Bernoulli()), liks["bernoulli"][2])))
        out.append((f"natgrad/member_{kname}", "natgrad", lambda kname=kname: (model_over("svgp", members[kname]()), (X, Y2[:, :1]))))
    for kname in ("per_se", "three_level", "lin_iso"):
        out.append((f"trainer/member_{kname}", "trainer",
                    lambda kname=kname: (model_over("svgp", members[kname]()), dict(learning_rate=1e-2), (X, Y2[:, :1]))))
    out.append(("member/sep_dot", "grad", elbo_case(lambda: sep([se(), lin()]), Y2)))
    out.append(("member/sep_per", "grad", elbo_case(lambda: sep([se(), per_se()]), Y2)))
    out.append(("member/lcm_dot", "grad", elbo_case(lambda: lcm([se(), poly2(), m32()]), Y2)))
    out.append(("member/lcm_sum_dot", "grad", elbo_case(lambda: lcm([se(), lin() + se(), m32()]), Y2)))
    return out


def dump_models(tree, path, device=None):
    sys.path[:0] = [tree, tree + "/tests"]
    import torch
    import gpflow_amd as gp
    from gpflow_amd import ops, training
    log, depth, wrap = _logger()
    if device is None:
        import emulation
        for name, fn in emulation.primitives().items():
            if hasattr(ops, name):
                setattr(ops, name, wrap(name, fn))
    arr = lambda v: np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64))  # noqa: E731
    pack = lambda vals: {k: (tuple(arr(v).shape), arr(v).tobytes()) for k, v in vals.items()}  # noqa: E731
    res = {}
    for name, kind, make in model_cases(gp):
        del log[:]
        try:
            if kind == "grad":
                model, fn = make()
                pos = {id(p): i for i, p in enumerate(model.parameters)}
                for run in ("#cold", ""):
                    del log[:]
                    value, grads = fn()
                    vals = {"F": value}
                    for j, (p, g) in enumerate(grads.items()):
                        vals[f"grad{j:02d}:parameter{pos[id(p)]}"] = g
                    res[name + run] = (list(log), pack(vals))
                continue
            if kind == "value":
                model, fn = make()
                for run in ("#cold", ""):
                    del log[:]
                    vals = {"F": fn()}
                    res[name + run] = (list(log), pack(vals))
                continue
            if kind == "trainer":
                model, kw, data = make()
                tr = training.SVGPTrainer(model, **kw)
                for _ in range(2):
                    Fv = tr.step(data)
                vals = {"F": Fv, "host_names=" + ",".join(tr.host): np.zeros(0)}
                vals.update({f"u:{n}": v for n, v in tr.u.items()})
                vals.update({f"dev:{n}": v for n, v in tr.dev.items()})
            else:
                model, data = make()
                gp.optimizers.NaturalGradient(1.0).minimize(model, data)
                vals = {"q_mu": model.q_mu.numpy(), "q_sqrt": model.q_sqrt.numpy()}
            res[name] = (list(log), pack(vals))
        except (NotImplementedError, ValueError) as e:
            res[name] = (list(log), {f"refused:{type(e).__name__}:{e}": ((), b"")})
    with open(path, "wb") as f:
        pickle.dump(res, f)
    refused = [n for n, (_, v) in res.items() if any(k.startswith("refused:") for k in v)]
    print(len(res), "entries;", len(refused), "refusals:")
    for n in refused:
        print("   ", n, next(iter(res[n][1]))[:60], "after", len(res[n][0]), "ops.* calls")


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
    {"dump": dump, "dump-models": dump_models, "compare": compare}[sys.argv[1]](*sys.argv[2:])
