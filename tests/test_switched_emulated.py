"""CPU: the switched likelihood's host layer (likelihoods.SwitchedLikelihood, the VGP and SVGP routes, the reverse pass's likelihood
stage) driven by the model-level test bodies of tests/test_gpu_switched.py with the device primitives replaced by their NumPy
emulation -- tests/emulation.py's modules, tests/fake_switched_ops.py and the Coregion / VGP modules, installed here.  What this does
NOT test is the HIP kernel: that is what tests/test_gpu_switched.py does under `-m gpu`.  The CPU-only checks of the feature (the
launch inventory of gpflow_amd/csrc/switched, the exports, the refusals, the gradient names) follow; they need no device.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import emulation
import fake_coregion_ops
import fake_switched_ops
import fake_vgp_ops
import test_gpu_switched as T
import test_launch_geometry as G
from gpflow_amd.likelihoods import SwitchedLikelihood  # noqa: F401  (the feature: without it nothing in this file can pass)

MODULES = emulation.MODULES + (fake_switched_ops, fake_coregion_ops, fake_vgp_ops)


@pytest.fixture
def gp(monkeypatch):
    import gpflow_amd
    from gpflow_amd import ops
    for name, fn in emulation.primitives(MODULES).items():
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, fn)
    return gpflow_amd


# the model-level bodies; the primitive's own tests (bounds, bits, planted bytes, scratch) are the device tier's
for _n in ("test_vgp_recipe_elbo_and_grad_against_autograd", "test_vgp_predict_log_density_and_the_refused_predictions",
           "test_scipy_lowers_the_objective_and_moves_each_tasks_parameter", "test_svgp_elbo_and_grad_against_autograd",
           "test_svgp_elbo_with_the_coregion_product_runs_forward_only"):
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
SWITCHED_CSRC = os.path.join(G.CSRC, "switched")
GPU = "test_gpu_switched"
# one row per launch site of gpflow_amd/csrc/switched/*.hip (tests/test_launch_geometry.py inventories csrc/*.hip and keeps its own table)
SWITCHED_LAUNCHES = [
    G.strided("switched_varexp.hip", "switched_varexp_kernel<true>",
              G.clamp("nb = nb < 1 ? 1 : (nb > GPK_REDUCE_MAXPART ? GPK_REDUCE_MAXPART : nb);\n  return (int)nb;",
                      "four wave passes of floor(16 / P) rows per block, at most 1024 blocks",
                      near=[(GPU, "CASES", (257, 1, 4, "sorted", False, "ld"))],
                      far=[(GPU, "[BIG_CASE]", (70001, 1, 3, "random", False, "c"))])),
    G.strided("switched_varexp.hip", "switched_varexp_kernel<false>",
              G.clamp("if (heavy) hipLaunchKernelGGL(switched_varexp_kernel<true>",
                      "the instantiation is chosen by whether the table holds Beta or Poisson; the grid is the same",
                      near=[(GPU, "CASES", (257, 1, 4, "sorted", False, "ld"))],
                      far=[(GPU, "[BIG_CASE]", (70001, 1, 3, "random", False, "c"))])),
    G.exact("switched_varexp.hip", "switched_tail_kernel", "hipLaunchKernelGGL(switched_tail_kernel, dim3(1), dim3(RB)"),   # one block, loops inside itself
]


def test_launch_inventory_of_the_switched_directory():
    """launch sites == rows, the one kernel that mentions gridDim is strided with cases on both sides, every quoted launch expression
    stands; a row taken out is seen; the inventory of csrc/*.hip is unchanged by the new directory"""
    sources = G._sources(SWITCHED_CSRC)
    assert sorted(sources) == ["switched_varexp.hip"]
    assert G.problems(SWITCHED_LAUNCHES, sources) == []
    for row in SWITCHED_LAUNCHES:
        bad = G.problems([r for r in SWITCHED_LAUNCHES if r is not row], sources)
        assert any("launch without a row" in b and row["kernel"] in b for b in bad), (row["kernel"], bad)
        for c in row.get("clamps", ()):
            assert c["near"] and c["far"] and all(G._case_exists(ref) for ref in c["near"] + c["far"]), row["kernel"]
    assert {k for _, k in G.kernel_bodies(sources)} == {"switched_varexp_kernel", "switched_tail_kernel"}
    text = sources["switched_varexp.hip"]
    assert "atomic" not in text.replace("No floating-point atomics", "") and "getenv" not in text
    assert G.problems(G.LAUNCHES, G._sources()) == []          # (the sub-directory is not part of that inventory)


def test_exports_header_and_tables():
    import gpflow_amd as gpflow
    from gpflow_amd import _lib, ops
    import fake_likelihood_ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    new = {"gpk_switched_varexp_sum", "gpk_switched_varexp_blocks"}
    assert new <= declared and declared == set(_lib.EXPORTED_SYMBOLS) and all(hasattr(lib, n) for n in declared)
    # a typed scratch operand: neither a (void* ws, size_t ws_bytes) pair nor a *_workspace_bytes function
    assert _lib._SIGS["gpk_switched_varexp_sum"][1][-2:] != [_lib.c_void_p, _lib.c_size_t]
    assert f"{len(declared)} functions" in open(os.path.join(root, "README.md")).read()
    assert ops.SWITCHED_MEMBERS == {"gaussian": 0, **{k: ops.LIKELIHOOD_CODES[k] for k in fake_switched_ops._MEMBERS[1:]}}
    assert set(fake_likelihood_ops.LIKELIHOODS) == set(ops.LIKELIHOOD_CODES) and 0 not in ops.LIKELIHOOD_CODES.values()
    assert {"switched_varexp_sum"} == set(emulation.primitives(emulation.MODULES + (fake_switched_ops,))) - set(emulation.primitives())
    assert issubclass(gpflow.likelihoods.SwitchedLikelihood, gpflow.likelihoods.Likelihood)
    assert not issubclass(gpflow.likelihoods.SwitchedLikelihood, gpflow.likelihoods.ScalarLikelihood)


def test_the_library_judges_the_table_on_the_host():
    """gpk_switched_varexp_sum with rows = 0, no device operand and a HOST buffer as `out`: every refusal of the sizes and of the table
    is answered before anything is enqueued, so the statuses can be read without a device -- GPK_E_ARG (-1) for T, P, ylab and a
    member's bad parameter, GPK_E_UNSUPPORTED (-3) for codes 4, 5 and 11 -- and the buffer keeps its planted bytes; a NULL `out` is
    GPK_E_ARG whatever the table (the versions with device buffers run on the device tier)"""
    from gpflow_amd import _lib
    lib = _lib.load()
    knn = (ctypes.c_double * 1)(1.0)
    plant = 0x7FF8DEADBEEF1234
    host_out = (ctypes.c_uint64 * 18)(*[plant] * 18)

    def answer(T_, codes, params, P=1, ylab=1, out=None):
        return lib.gpk_switched_varexp_sum(None, T_, (ctypes.c_int * max(len(codes), 1))(*codes),
                                           (ctypes.c_double * max(len(params), 1))(*params), None, 2, ylab, None, 0, P, None, 0, None,
                                           knn, 0, 0.0, None, None, None, None, out, None)
    out = ctypes.addressof(host_out)
    table = [(0, [], [], 1, 1, -1), (17, [1] * 17, [0.0] * 34, 1, 1, -1), (1, [1], [0, 0], 17, 17, -1), (1, [1], [0, 0], 2, 1, -1),
             (1, [4], [0.5, 0], 1, 1, -3), (1, [5], [0, 0], 1, 1, -3), (1, [11], [1, 1], 1, 1, -3), (2, [1, 6], [0, 0, 0, 0], 1, 1, -3)]
    table += [(2, [1, code], [0.0, 0.0] + par, 1, 1, -1) for code, par in ((0, [0.0, 0.0]), (0, [-1.0, 0.0]), (0, [float("nan"), 0.0]),
                                                                          (2, [0.0, 0.0]), (3, [-1.0, 3.0]), (3, [1.0, 0.0]),
                                                                          (9, [0.0, 0.0]), (10, [-2.0, 0.0]))]
    for T_, codes, params, P, ylab, status in table:
        assert answer(T_, codes, params, P, ylab, out) == status, (T_, codes, params)
        assert list(host_out) == [plant] * 18, (T_, codes, params)
    assert answer(1, [1], [0, 0]) == -1 and answer(1, [4], [0.5, 0]) == -1          # out is NULL: GPK_E_ARG comes first
    assert lib.gpk_switched_varexp_blocks(257, 1) == 5 and lib.gpk_switched_varexp_blocks(70001, 1) == 1024
    assert lib.gpk_switched_varexp_blocks(0, 1) == 1 and lib.gpk_switched_varexp_blocks(33, 16) == 9
    assert lib.gpk_switched_varexp_blocks(10, 17) == 1 and lib.gpk_switched_varexp_blocks(130, 5) == 11


def test_construction_refusals_and_num_latent_gps(gp):
    Ls, K = gp.likelihoods, gp.kernels
    het = Ls.Gaussian(variance=gp.functions.Linear(A=np.ones((1, 1)), b=np.ones(1)))
    for member, word in ((Ls.Ordinal([0.0]), "edge table"), (Ls.MultiClass(3), "couples"), (het, "Function"),
                         (Ls.Gaussian(scale=0.5), "scale="), (Ls.SwitchedLikelihood([Ls.Gaussian()]), "itself switched")):
        with pytest.raises(NotImplementedError) as e:
            Ls.SwitchedLikelihood([Ls.Gaussian(), member])
        assert type(member).__name__ in str(e.value) and word in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        Ls.SwitchedLikelihood([])
    with pytest.raises(ValueError):
        Ls.SwitchedLikelihood([Ls.Gaussian() for _ in range(17)])
    lik = Ls.SwitchedLikelihood([Ls.StudentT(scale=0.7, df=4.0), Ls.Gaussian(0.3), Ls.Poisson(), Ls.Gamma(shape=1.5)])
    assert lik.device_members() == (("student_t", (0.7, 4.0)), ("gaussian", (0.3,)), ("poisson_exp", (1.0,)), ("gamma_exp", (1.5,)))
    assert lik.device_grad_params() == [lik.likelihoods[0].scale, lik.likelihoods[1].variance, None, lik.likelihoods[3].shape]
    assert len(lik.trainable_parameters) == 3
    Y3 = np.zeros((5, 3))
    assert gp.models.GPModel.calc_num_latent_gps_from_data((None, Y3), K.SquaredExponential(), lik) == 2
    assert gp.models.VGP.calc_num_latent_gps_from_data((None, Y3), K.SquaredExponential(), lik) == 2
    assert gp.models.GPModel.calc_num_latent_gps_from_data((None, Y3), K.SquaredExponential(), Ls.Gaussian()) == 3
    for method, args in (("predict_mean_and_var", (None, None, None)), ("conditional_mean", (None, None)), ("conditional_variance", (None, None))):
        with pytest.raises(NotImplementedError):
            getattr(lik, method)(*args)
    with pytest.raises(NotImplementedError):     # more than 16 latents: refused when the VGP is built
        gp.models.VGP((np.zeros((3, 1)), np.zeros((3, 18))), K.SquaredExponential(), lik)


def test_variational_expectations_and_log_prob_pick_the_rows_member(gp):
    """the per-row values against the members' own methods on the rows of each task; an invalid label gives NaN"""
    Ls = gp.likelihoods
    members = [Ls.StudentT(scale=0.7, df=4.0), Ls.Gaussian(0.3), Ls.Bernoulli()]
    lik = Ls.SwitchedLikelihood(members)
    rng = np.random.default_rng(3)
    N, P = 30, 2
    task = np.arange(N) % 3
    Yv = np.where((task == 2)[:, None], (rng.uniform(size=(N, P)) < 0.5).astype(np.float64), rng.normal(size=(N, P)))
    Y = np.concatenate([Yv, task[:, None] + 0.25], axis=1)
    Y[7, -1] = np.nan
    Fmu, Fvar = rng.normal(size=(N, P)), rng.uniform(0.2, 0.9, size=(N, P))
    t = gp.ops.to_device
    for method in ("variational_expectations", "predict_log_density"):
        got = T._np(getattr(lik, method)(None, t(Fmu), t(Fvar), t(Y)))
        for k, mem in enumerate(members):
            sel = (task == k) & (np.arange(N) != 7)
            ref = T._np(getattr(mem, method)(None, t(Fmu[sel]), t(Fvar[sel]), t(Yv[sel])))
            np.testing.assert_allclose(got[sel], ref, rtol=1e-13, atol=1e-13, err_msg=f"{method} {k}")
        assert np.isnan(got[7]) and np.isfinite(np.delete(got, 7)).all()
    got = T._np(lik.log_prob(None, t(Fmu), t(Y)))
    for k, mem in enumerate(members):
        sel = (task == k) & (np.arange(N) != 7)
        np.testing.assert_allclose(got[sel], T._np(mem.log_prob(None, t(Fmu[sel]), t(Yv[sel]))), rtol=1e-13, atol=1e-13)
    assert np.isnan(got[7])
    with pytest.raises(ValueError):
        lik.variational_expectations(None, t(Fmu), t(Fvar), t(Yv))      # no label column


def test_gradient_names_and_the_one_stage_call(gp, monkeypatch):
    """gradients.vgp_elbo_and_grad / svgp_elbo_and_grad with likelihood = ("switched", members) through a logging proxy: ONE
    switched_varexp_sum call and no likelihood_varexp_sum, gradients named likelihood_<t> for every task; any other likelihood name
    issues the likelihood_varexp_sum call it issued before; the SVGP site multiplies the parameter gradients by `scale`"""
    import torch
    from gpflow_amd import gradients
    calls = []
    prims = emulation.primitives(MODULES)
    monkeypatch.setattr(gradients, "ops", types.SimpleNamespace(**{n: (lambda n_, f: lambda *a, **kw: (calls.append(n_), f(*a, **kw))[1])(n, fn)
                                                                   for n, fn in prims.items()}))
    table = T.MODEL_TABLES["studentt-gaussian"]
    X, Y, q_mu, q_sqrt = T._recipe_data(table, 40, 3)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    spec = gradients.KernelSpec.single(1.3, 0.9)
    F, g, _ = gradients.vgp_elbo_and_grad(t(X[:, :1]), t(Y), t(q_mu), t(q_sqrt), kernel_spec=spec, jitter=1e-6, likelihood=("switched", table))
    assert calls.count("switched_varexp_sum") == 1 and "likelihood_varexp_sum" not in calls
    assert {"likelihood_0", "likelihood_1"} <= set(g) and not [n for n in g if n.startswith("likelihood_") and n[11:] not in "01"]
    calls.clear()
    _, g1, _ = gradients.vgp_elbo_and_grad(t(X[:, :1]), t(Y[:, :1]), t(q_mu), t(q_sqrt), kernel_spec=spec, jitter=1e-6,
                                           likelihood=("student_t", (0.7, 4.0)))
    assert calls.count("likelihood_varexp_sum") == 1 and "switched_varexp_sum" not in calls and "likelihood_scale" in g1
    Zx = X[::4, :1].copy()
    args = (t(Zx), t(X[:, :1]), t(Y), t(q_mu[:10]), t(q_sqrt[:, :10, :10]))
    kw = dict(variance=1.3, lengthscales=0.9, noise_variance=None, jitter=1e-6, likelihood=("switched", table))
    _, ga, _ = gradients.svgp_elbo_and_grad(*args, scale=1.0, kl_weight=0.0, **kw)
    _, gb, _ = gradients.svgp_elbo_and_grad(*args, scale=2.5, kl_weight=0.0, **kw)
    for name in ("likelihood_0", "likelihood_1"):
        np.testing.assert_allclose(gb[name].numpy(), 2.5 * ga[name].numpy(), rtol=1e-14)


def test_every_refusal_comes_before_the_device_and_the_fused_shard_is_never_called(gp, monkeypatch):
    """SVGP with a switched likelihood: the fused entry points are never called (elbo runs composed); the reverse pass refuses a
    row-diagonal member, the un-whitened model, SeparateIndependent / LinearCoregionalization, natural gradients and the trainer --
    each with NotImplementedError and not one call into gpflow_amd.ops"""
    ops, K, Ls = gp.ops, gp.kernels, gp.likelihoods
    table = T.MODEL_TABLES["studentt-gaussian"]
    X2, Y, Zx, q_mu, q_sqrt = T._svgp_problem(table, 8, 20, 5, False)
    X = X2[:, :1].copy()
    lik = lambda: Ls.SwitchedLikelihood(T._member_objects(gp, table))  # noqa: E731
    calls = []
    for name in dir(ops):
        fn = getattr(ops, name)
        if not name.startswith("_") and callable(fn) and not isinstance(fn, type):
            monkeypatch.setattr(ops, name, (lambda n, f: lambda *a, **kw: (calls.append(n), f(*a, **kw))[1])(name, fn))
    m = gp.models.SVGP(K.SquaredExponential(), lik(), Zx.copy(), q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), num_data=100)
    assert np.isfinite(float(m.elbo((X, Y))))
    m.elbo_and_grad((X, Y))
    assert "switched_varexp_sum" in calls and not [c for c in calls if c.startswith("svgp_elbo_shard")]
    calls.clear()
    Zf = np.concatenate([Zx, np.zeros((8, 1))], axis=1)
    iv = gp.inducing_variables
    shared = iv.SharedIndependentInducingVariables(iv.InducingPoints(Zx.copy()))
    refused = [
        gp.models.SVGP(T._recipe_kernel(gp), lik(), Zf.copy(), q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy()),              # row-diagonal member
        gp.models.SVGP(K.Linear() + K.SquaredExponential(), lik(), Zx.copy(), q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy()),
        gp.models.SVGP(K.SquaredExponential(), lik(), Zx.copy(), q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), whiten=False),   # un-whitened
        gp.models.SVGP(K.SeparateIndependent([K.SquaredExponential()]), lik(), shared, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy()),
        gp.models.SVGP(K.LinearCoregionalization([K.SquaredExponential()], W=np.ones((1, 1))), lik(), shared, q_mu=q_mu.copy(),
                       q_sqrt=q_sqrt.copy()),
    ]
    for model in refused:
        data = (X2, Y) if model is refused[0] else (X, Y)
        with pytest.raises(NotImplementedError):
            model.elbo_and_grad(data)
    with pytest.raises(NotImplementedError):
        gp.optimizers.NaturalGradient(gamma=0.1).minimize(m, (X, Y))
    with pytest.raises(NotImplementedError):
        gp.training.SVGPTrainer(m)
    assert calls == [], calls
