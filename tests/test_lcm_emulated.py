"""CPU: the LinearCoregionalization layer (kernel class, mixing, posterior, SVGP routing, reverse pass) driven by the test bodies of
tests/test_gpu_lcm.py with the device primitives replaced by their NumPy emulation (tests/emulation.py: every
tests/fake_*.py) -- exactly as tests/test_multiclass_emulated.py drives
tests/test_gpu_multiclass.py.  What this does NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The
CPU-only checks of the feature (constructors, the posterior table, what the library answers before it touches a device, the call
log of the reverse pass, the build) are at the end; they need no device.
"""
import ctypes
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import emulation
import test_gpu_lcm as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
def _members(K, n=3):
    return [K.SquaredExponential(variance=1.0 + 0.1 * i, lengthscales=0.8 + 0.2 * i) for i in range(n)]


def test_lcm_constructors_shapes_and_wrong_width():
    """The kernel class as the reference has it; W of the wrong width, q_mu of the wrong width and Y of the wrong width are
    ValueErrors at elbo (no device here: anything that reached one would raise something else)."""
    import gpflow_amd as gpflow
    K, IV = gpflow.kernels, gpflow.inducing_variables
    assert "LinearCoregionalization" in K.__all__
    W = np.arange(12.0).reshape(4, 3)
    k = K.LinearCoregionalization(_members(K), W)
    assert isinstance(k, K.MultioutputKernel) and isinstance(k.W, gpflow.Parameter) and k.W.shape == (4, 3)
    assert k.num_latent_gps == 3 and k.latent_kernels == tuple(k.kernels) and k.name == "LinearCoregionalization"
    assert np.array_equal(k.W.unconstrained_variable, W) and k.W in k.trainable_parameters        # no transform
    assert np.array_equal(k.mixing_host(), W)
    Z = np.random.default_rng(0).normal(size=(5, 2))
    iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Z))
    data = (np.zeros((4, 2)), np.ones((4, 4)))
    lik = gpflow.likelihoods.Gaussian(0.1)
    wrong_W = gpflow.models.SVGP(K.LinearCoregionalization(_members(K), np.ones((4, 2))), lik, iv, num_latent_gps=3)
    for fn in (wrong_W.elbo, wrong_W.elbo_terms):
        with pytest.raises(ValueError, match=r"\[P, L\]"):
            fn(data)
    wrong_q = gpflow.models.SVGP(k, lik, iv, num_latent_gps=4)
    with pytest.raises(ValueError, match="LATENT"):
        wrong_q.elbo(data)
    assert gpflow.models.SVGP(k, lik, iv, num_latent_gps=3).q_mu.shape == (5, 3)


def test_lcm_posterior_class_table():
    import gpflow_amd as gpflow
    K, IV, Pz = gpflow.kernels, gpflow.inducing_variables, gpflow.posteriors
    k = K.LinearCoregionalization(_members(K), np.ones((4, 3)))
    pts = IV.InducingPoints(np.zeros((5, 2)))
    assert Pz.get_posterior_class(k, IV.SharedIndependentInducingVariables(pts)) is Pz.LinearCoregionalizationPosterior
    assert Pz.get_posterior_class(k, IV.SeparateIndependentInducingVariables([pts] * 3)) is Pz.LinearCoregionalizationPosterior
    assert issubclass(Pz.LinearCoregionalizationPosterior, Pz.IndependentPosteriorMultiOutput)
    with pytest.raises(NotImplementedError, match="FullyCorrelated"):
        Pz.get_posterior_class(k, pts)
    # the rows that were there keep their classes
    assert Pz.get_posterior_class(K.SeparateIndependent(_members(K)), IV.SharedIndependentInducingVariables(pts)) \
        is Pz.IndependentPosteriorMultiOutput
    assert Pz.get_posterior_class(K.SquaredExponential(), pts) is Pz.IndependentPosteriorSingleOutput


def test_mix_latent_gp_forms():
    """the four covariance forms of conditionals.mix_latent_gp against explicit loops, with a leading batch dimension"""
    from gpflow_amd.conditionals import mix_latent_gp
    rng = np.random.default_rng(2)
    B, N, L, P = 2, 5, 3, 4
    W, gm = rng.normal(size=(P, L)), rng.normal(size=(B, N, L))
    gv, gc = rng.uniform(0.1, 1, size=(B, N, L)), rng.normal(size=(B, L, N, N))
    t = torch.from_numpy
    for fc, foc, g_var, shape in ((False, False, gv, (B, N, P)), (False, True, gv, (B, N, P, P)), (True, False, gc, (B, P, N, N)),
                                  (True, True, gc, (B, N, P, N, P))):
        mu, var = mix_latent_gp(t(W), t(gm), t(g_var), fc, foc)
        assert tuple(var.shape) == shape
        np.testing.assert_allclose(mu.numpy(), gm @ W.T, atol=1e-14)
        ref = np.zeros(shape)
        for l in range(L):
            for p in range(P):
                for q in range(P):
                    if fc and foc:
                        ref[:, :, p, :, q] += W[p, l] * W[q, l] * gc[:, l]
                    elif fc and p == q:
                        ref[:, p] += W[p, l] ** 2 * gc[:, l]
                    elif foc and not fc:
                        ref[:, :, p, q] += W[p, l] * W[q, l] * gv[:, :, l]
                    elif not fc and not foc and p == q:
                        ref[:, :, p] += W[p, l] ** 2 * gv[:, :, l]
        np.testing.assert_allclose(var.numpy(), ref, atol=1e-13)


def test_library_answers_for_the_lcm_entry_points_before_the_device():
    """gpk_mixed_gaussian_varexp_sum and gpk_svgp_elbo_shard_lcm with rows = 0 and host buffers in the pointer slots they check
    first: GPK_E_ARG (-1) for L or P outside [1, 16], a NULL W / knn / out and a noise variance that is not > 0; GPK_E_WORKSPACE (-2)
    for a short workspace; nothing written.  The workspace queries are monotone in rows and in L."""
    from gpflow_amd import _lib
    assert {"gpk_mixed_varexp_workspace_bytes", "gpk_mixed_gaussian_varexp_sum", "gpk_svgp_elbo_lcm_workspace_bytes",
            "gpk_svgp_elbo_shard_lcm"} <= set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    W, knn, out = _lib.host_doubles([0.5] * 289), _lib.host_doubles([1.0]), _lib.host_doubles([7.0, 7.0])
    nws = int(lib.gpk_mixed_varexp_workspace_bytes(0, 16, 16))
    ws = (ctypes.c_double * (nws // 8 + 1))()
    addr = lambda a: ctypes.cast(a, ctypes.c_void_p).value   # noqa: E731

    def call(L, P, s2, w=W, k=knn, o=out, n=nws):
        return lib.gpk_mixed_gaussian_varexp_sum(None, None, 1, None, 0, L, P, w, None, 0, None, k, 0, s2, 0.0, None, None, None, None,
                                                 None if o is None else addr(o), addr(ws), n)
    for L, P, s2 in ((0, 2, 0.3), (17, 2, 0.3), (2, 0, 0.3), (2, 17, 0.3), (2, 3, 0.0), (2, 3, -0.1), (2, 3, float("nan"))):
        assert call(L, P, s2) == -1, (L, P, s2)
    assert call(2, 3, 0.3, w=None) == -1 and call(2, 3, 0.3, k=None) == -1 and call(2, 3, 0.3, o=None) == -1
    assert call(2, 3, 0.3, n=int(lib.gpk_mixed_varexp_workspace_bytes(0, 2, 3)) - 8) == -2 and call(2, 3, 0.3, n=0) == -2
    assert list(out) == [7.0, 7.0]
    # the fused shard: the mixing stage's arguments are checked before the workspace and before anything is launched
    one, fam = _lib.host_doubles([1.0] * 16), (ctypes.c_int * 16)()

    def shard(L, P, s2, w=W, n=0):
        return lib.gpk_svgp_elbo_shard_lcm(None, fam, addr(ws), 8, 2, 0, None, None, 0, 2, max(P, 1), 2, L, P, w, one, 0, one, s2, 1e-6,
                                           0.0, addr(ws), addr(ws), addr(out), addr(ws), addr(ws), n)
    for L, P, s2 in ((0, 2, 0.3), (17, 2, 0.3), (2, 0, 0.3), (2, 17, 0.3), (2, 3, 0.0)):
        assert shard(L, P, s2) == -1, (L, P, s2)
    assert shard(2, 3, 0.3, w=None) == -1
    assert shard(2, 3, 0.3) == -2                                   # valid arguments, no workspace
    assert list(out) == [7.0, 7.0]
    q = lib.gpk_mixed_varexp_workspace_bytes
    assert all(q(r1, L, 5) <= q(r2, L, 5) for L in (1, 4, 16) for r1, r2 in ((0, 1), (1, 67), (67, 4096), (4096, 100000)))
    assert all(q(r, L, 5) < q(r, L + 1, 5) for r in (0, 67, 100000) for L in range(1, 16))
    q = lib.gpk_svgp_elbo_lcm_workspace_bytes
    assert all(q(64, r1, 2, L, 5) <= q(64, r2, 2, L, 5) for L in (1, 4, 16) for r1, r2 in ((0, 1), (1, 67), (67, 4096)))
    assert all(q(64, r, 2, L, 5) < q(64, r, 2, L + 1, 5) for r in (0, 67, 4096) for L in range(1, 16))
    assert q(64, 67, 2, 3, 5) == lib.gpk_svgp_elbo_sep_workspace_bytes(64, 67, 2, 3)   # the layout of the L latents


def test_lcm_reverse_pass_call_log(monkeypatch):
    """The ordered outermost `ops.*` calls of gradients.svgp_elbo_and_grad_lcm: L per-latent forwards, exactly ONE
    mixed_gaussian_varexp_sum, one KL, then L copies of the per-latent backward list -- the lists that
    svgp_elbo_and_grad itself issues around its Gaussian stage on a one-latent problem (the benchmark form, whose list
    test_gradients_cpu.test_benchmark_form_issues_a_fixed_list_of_primitive_calls pins)."""
    from gpflow_amd import gradients
    calls, depth = [], [0]

    def logged(name, fn):
        def call(*a, **kw):
            if depth[0] == 0:
                calls.append(name)
            depth[0] += 1
            try:
                return fn(*a, **kw)
            finally:
                depth[0] -= 1
        return call
    monkeypatch.setattr(gradients, "ops", types.SimpleNamespace(**{n: logged(n, fn) for n, fn in emulation.primitives().items()}))
    rng = np.random.default_rng(4)
    M, B, D, L, P = 24, 50, 2, 3, 4
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    Z, X, Y = t(rng.normal(size=(M, D))), t(rng.normal(size=(B, D))), t(rng.normal(size=(B, P)))
    q_mu = t(0.3 * rng.normal(size=(M, L)))
    q_sqrt = t(np.stack([np.tril(0.05 * rng.normal(size=(M, M))) + 0.6 * np.eye(M) for _ in range(L)]))
    specs = [gradients.KernelSpec.single(1.0 + 0.1 * l, 0.9 + 0.1 * l) for l in range(L)]
    gradients.svgp_elbo_and_grad_lcm([Z] * L, [X] * L, Y, q_mu, q_sqrt, rng.normal(size=(P, L)), kernel_specs=specs, noise_variance=0.2,
                                     jitter=1e-6, scale=4.0, mean_const=0.1)
    lcm_calls = list(calls)
    # the per-latent lists, from the pass they were factored out of: svgp_elbo_and_grad on a one-latent problem
    del calls[:]
    gradients.svgp_elbo_and_grad(Z, X, Y[:, :1].contiguous(), q_mu[:, :1].contiguous(), q_sqrt[:1].contiguous(), variance=1.0,
                                 lengthscales=0.9, noise_variance=0.2, jitter=1e-6, scale=4.0, mean_const=0.1)
    i = calls.index("gaussian_varexp_sum")
    assert calls[i + 1] == "gauss_kl_white" and calls.count("gaussian_varexp_sum") == 1
    forward, backward = calls[:i], calls[i + 2:]
    assert forward[:3] == ["kernel_matrix", "kernel_matrix", "potrf_"] and backward[0] == "lowrank_axpy" and len(backward) > 20
    assert lcm_calls.count("mixed_gaussian_varexp_sum") == 1 and lcm_calls.count("gaussian_varexp_sum") == 0
    assert lcm_calls == forward * L + ["mixed_gaussian_varexp_sum", "gauss_kl_white"] + backward * L, lcm_calls


def test_feature_sources_compile_without_warnings(tmp_path):
    """The two translation units the feature touches compile with the Makefile's own command lines (`make -n -B`, the object files
    redirected to a scratch directory so that the loaded library is left alone) and without a single warning."""
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpflow_amd", "csrc")
    objs = ["build/varexp.o", "build/drivers.o"]
    plan = subprocess.run(["make", "-C", src, "-n", "-B"] + objs, capture_output=True, text=True, check=True).stdout
    cmds = [ln for ln in plan.splitlines() if " -c " in ln and ln.rstrip().endswith(tuple(objs))]
    assert len(cmds) == 2, plan
    for cmd, obj in zip(cmds, objs):
        r = subprocess.run(cmd.replace("-o " + obj, "-o " + str(tmp_path / os.path.basename(obj))), shell=True, cwd=src,
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        assert "warning" not in (r.stdout + r.stderr), (r.stdout + r.stderr)[-2000:]
