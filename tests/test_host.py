"""CPU: host-side logic of the GPflow surface (parameters, transforms, config, argument checking, error
behaviour) and the C-ABI library itself (loads, exports every symbol include/gpk.h declares).  No
compute calls: there is no GPU here and gpflow_amd has no CPU path."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def built_lib():
    from gpflow_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def test_library_exports_every_declared_symbol(built_lib):
    header = open(os.path.join(ROOT, "include", "gpk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", header))
    assert len(declared) >= 25
    from gpflow_amd import _lib
    for name in declared:
        assert hasattr(built_lib, name), f"libgpk.so lacks {name} declared in include/gpk.h"
    # and the ctypes table binds exactly the declared interface
    assert set(_lib.EXPORTED_SYMBOLS) == declared
    assert built_lib.gpk_version().decode().startswith("gpk")
    assert built_lib.gpk_invd_elems(300, 2) == 2 * 3 * 128 * 128
    assert built_lib.gpk_svgp_elbo_workspace_bytes(2048, 8192, 8, 1, 0, 1) > (2048 + 8192) * 2048 * 8
    # the separate-kernel driver keeps one trapezoid PER latent (config C5: 4 x (1024 + 8192) x 1024 doubles) + its tails
    sep = built_lib.gpk_svgp_elbo_sep_workspace_bytes(1024, 8192, 8, 4)
    assert 4 * (1024 + 8192) * 1024 * 8 < sep < 2 * 4 * (1024 + 8192) * 1024 * 8
    # argument errors are reported before anything touches a device (GPK_E_ARG = -1)
    assert built_lib.gpk_svgp_elbo_shard_sep(None, None, None, 1024, 8, 0, None, None, 8192, 8, 4, 8, 4, None, 1, None, 0.1, None, 1e-6,
                                             0.0, None, None, None, None, None, 0) == -1
    # an un-whitened diagonal q_sqrt keeps P + m more trapezoid rows and the second-solve buffer; the whitened one neither
    assert built_lib.gpk_svgp_elbo_workspace_bytes(2048, 8192, 8, 1, 1, 0) > built_lib.gpk_svgp_elbo_workspace_bytes(2048, 8192, 8, 1, 1, 1) \
        + 8192 * 2048 * 8
    # the single-launch step kernel of round 4 reserves nothing in the product library (its regions doubled this figure)
    assert built_lib.gpk_svgp_elbo_workspace_bytes(2048, 8192, 8, 1, 0, 1) < 1.45 * (2048 + 8192 + 2048) * 2048 * 8


def test_header_is_plain_c_and_a_c_client_links(built_lib, tmp_path):
    """The drop-in boundary is a C ABI: include/gpk.h must compile as C99 (and C++), and a C client that references
    every declared entry point must link against libgpk.so (no C++ types or mangled names leak through)."""
    import shutil
    import subprocess
    from gpflow_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    hdr = os.path.join(ROOT, "include", "gpk.h")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", hdr], check=True)
    subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-x", "c++", hdr], check=True)
    names = sorted(_lib.EXPORTED_SYMBOLS)
    src = tmp_path / "client.c"
    src.write_text('#include "gpk.h"\n#include <stdio.h>\nint main(void) {\n  const void* f[] = {' +
                   ", ".join(f"(const void*){n}" for n in names) +
                   '};\n  printf("%s %d\\n", gpk_version(), (int)(sizeof f / sizeof f[0]));\n  return f[0] == 0;\n}\n')
    exe = tmp_path / "client"
    libdir = os.path.dirname(_lib.lib_path())
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
                    "-l:" + os.path.basename(_lib.lib_path()), "-Wl,-rpath," + libdir], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("gpk") and out.split()[-1] == str(len(names))


def test_missing_extension_fails_loudly(monkeypatch, tmp_path):
    from gpflow_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "_LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()


def test_no_gpu_means_error_not_fallback(built_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import gpflow_amd as gpflow
    from gpflow_amd._lib import GpkError
    m_kernel = gpflow.kernels.RBF()
    with pytest.raises(GpkError, match="no CPU path"):
        m_kernel(np.zeros((3, 1)))
    from gpflow_amd import ops
    with pytest.raises(GpkError):
        ops.kernel_matrix(torch.zeros(3, 1, dtype=torch.float64), None, variance=1.0, lengthscales=1.0)


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under gpflow_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gpflow_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f
                assert "gp_oracle" not in src, f


def test_parameter_transforms():
    from gpflow_amd.base import Parameter, positive, triangular
    from oracle import gp_oracle as orc
    p = Parameter(2.5, transform=positive())
    np.testing.assert_allclose(p.numpy(), 2.5)
    np.testing.assert_allclose(p.unconstrained_variable, orc.softplus_inverse(2.5))
    p.assign(0.3)
    np.testing.assert_allclose(p.numpy(), 0.3, rtol=1e-15)
    q = Parameter(1.0, transform=positive(lower=1e-6))
    np.testing.assert_allclose(q.unconstrained_variable, orc.positive_inverse(1.0, 1e-6))
    # tests/gpflow/test_base.py:30-37: a value at/below the lower bound is rejected
    with pytest.raises(ValueError, match="incompatible with this parameter's transform"):
        Parameter(0.0, transform=positive(lower=1e-6))
    with pytest.raises(ValueError):
        q.assign(-1.0)
    L = np.tril(np.arange(1.0, 10.0).reshape(3, 3))[None]
    t = Parameter(L + np.triu(np.ones((1, 3, 3)), 1), transform=triangular())  # upper part dropped
    np.testing.assert_array_equal(t.numpy(), L)
    np.testing.assert_array_equal(t.unconstrained_variable, orc.fill_triangular_inverse(L))
    e = Parameter(2.0, transform=positive(base="exp"))
    np.testing.assert_allclose(e.unconstrained_variable, np.log(2.0))
    pp = Parameter(p)
    assert pp.transform is p.transform and pp.trainable


def test_config():
    from gpflow_amd import config
    assert config.default_float() is np.float64
    assert config.default_jitter() == 1e-6
    assert config.default_likelihood_positive_minimum() == 1e-6
    assert config.default_positive_bijector() == "softplus"
    with config.as_context():
        config.set_default_jitter(1e-3)
        assert config.default_jitter() == 1e-3
    assert config.default_jitter() == 1e-6
    with pytest.raises(TypeError):
        config.set_default_float(np.float32)
    with pytest.raises(ValueError):
        config.set_default_positive_bijector("nope")
    with pytest.raises(ValueError):
        config.set_default_jitter(-1.0)


def test_model_construction_and_module_traversal():
    import gpflow_amd as gpflow
    k = gpflow.kernels.SquaredExponential(variance=2.0, lengthscales=[1.0, 3.0])
    assert k.ard and gpflow.kernels.RBF is gpflow.kernels.SquaredExponential
    with pytest.raises(TypeError, match="Unknown keyword argument"):
        gpflow.kernels.SquaredExponential(foo=1)
    with pytest.raises(ValueError, match="does not match size of ard parameter"):
        gpflow.kernels.RBF(lengthscales=[1.0, 2.0], active_dims=[0, 1, 2])
    lik = gpflow.likelihoods.Gaussian(0.5)
    assert lik.noise_variance() == pytest.approx(0.5)
    assert gpflow.likelihoods.Gaussian(scale=2.0).noise_variance() == pytest.approx(4.0)
    with pytest.raises(AssertionError):
        gpflow.likelihoods.Gaussian(1.0, scale=1.0)
    with pytest.raises(ValueError):
        gpflow.likelihoods.Gaussian(1e-7)  # below the 1e-6 lower bound
    Z = np.random.default_rng(0).normal(size=(4, 2))
    m = gpflow.models.SVGP(k, lik, Z, num_latent_gps=3)
    assert m.q_mu.shape == (4, 3) and m.q_sqrt.shape == (3, 4, 4)
    np.testing.assert_array_equal(m.q_sqrt.numpy()[1], np.eye(4))
    md = gpflow.models.SVGP(k, lik, Z, num_latent_gps=2, q_diag=True)
    assert md.q_sqrt.shape == (4, 2)
    m2 = gpflow.models.SVGP(k, lik, gpflow.inducing_variables.InducingPoints(Z), q_mu=np.zeros((4, 5)),
                            q_sqrt=np.stack([np.eye(4)] * 5))
    assert m2.num_latent_gps == 5
    names = set(gpflow.utilities.parameter_dict(m).keys())
    assert {".kernel.variance", ".kernel.lengthscales", ".likelihood.variance", ".inducing_variable.Z", ".q_mu",
            ".q_sqrt"} <= names
    assert len(m.trainable_parameters) == 6
    gpflow.set_trainable(m.kernel, False)
    assert len(m.trainable_parameters) == 4
    vals = gpflow.utilities.read_values(m)
    gpflow.utilities.multiple_assign(m, {".kernel.variance": 3.0})
    assert float(m.kernel.variance.numpy()) == pytest.approx(3.0) and vals[".kernel.variance"] == pytest.approx(2.0)
    cls = gpflow.posteriors.get_posterior_class
    iv = gpflow.inducing_variables.InducingPoints(Z)
    assert cls(k, iv) is gpflow.posteriors.IndependentPosteriorSingleOutput
    shared = gpflow.kernels.SharedIndependent(k, 3)
    siv = gpflow.inducing_variables.SharedIndependentInducingVariables(iv)
    assert cls(shared, siv) is gpflow.posteriors.IndependentPosteriorMultiOutput
    with pytest.raises(NotImplementedError):
        cls(shared, iv)
    assert gpflow.posteriors._validate_precompute_cache_type("Tensor") is gpflow.posteriors.PrecomputeCacheType.TENSOR
    assert gpflow.posteriors._validate_precompute_cache_type(None) is gpflow.posteriors.PrecomputeCacheType.NOCACHE
    with pytest.raises(ValueError):
        gpflow.posteriors._validate_precompute_cache_type(3)


def test_shard_bounds():
    from gpflow_amd.distributed import shard_bounds
    for n in (0, 1, 7, 8192, 8193):
        for w in (1, 2, 3, 8):
            spans = [shard_bounds(n, w, r) for r in range(w)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [hi - lo for lo, hi in spans]
            assert max(sizes) - min(sizes) <= 1
    with pytest.raises(ValueError):
        shard_bounds(10, 2, 2)


# ---------------------------------------------------------------- host logic of the rows added for SURVEY 8f
def test_bijector_forward_grad_matches_finite_differences():
    from gpflow_amd.base import Chain, Exp, Identity, Shift, Softplus, positive
    x = np.array([-4.0, -0.3, 0.0, 0.7, 6.0])
    h = 1e-6
    for b in (Identity(), Softplus(), Exp(), Shift(0.5), Chain([Shift(1e-3), Softplus()]), positive(lower=1e-6),
              positive(base="exp")):
        fd = (b.forward(x + h) - b.forward(x - h)) / (2 * h)
        np.testing.assert_allclose(b.forward_grad(x), fd, rtol=1e-6, atol=1e-9, err_msg=b.name)
    from gpflow_amd.base import FillTriangular
    with pytest.raises(NotImplementedError):
        FillTriangular().forward_grad(np.zeros(3))


def test_gradient_entry_points_refuse_unsupported_models_before_touching_the_device():
    """The reverse pass covers the SVGP (whitened or not) / GPR / SGPR with ONE SquaredExponential or Matern kernel and a
    Gaussian likelihood; everything else must say so (NotImplementedError), not silently compute something else."""
    import gpflow_amd as gpflow
    from gpflow_amd import training
    Z = np.random.default_rng(0).normal(size=(5, 2))
    lik = gpflow.likelihoods.Gaussian(0.1)
    summed = gpflow.models.SVGP(gpflow.kernels.Matern32() + gpflow.kernels.SquaredExponential(), lik, Z)
    qdiag = gpflow.models.SVGP(gpflow.kernels.SquaredExponential(), lik, Z, q_diag=True)
    sliced = gpflow.models.SVGP(gpflow.kernels.SquaredExponential(active_dims=[0]), lik, Z)
    data = (np.zeros((4, 2)), np.zeros((4, 1)))
    with pytest.raises(NotImplementedError):      # natural gradients need the full q_sqrt (optimizers/natgrad.py)
        training.SVGPTrainer(qdiag, natgrad_gamma=0.1)
    for m in (summed, qdiag, sliced):
        with pytest.raises(NotImplementedError):
            gpflow.optimizers.NaturalGradient(1.0).minimize(m, data)
    # (round 3: SVGP.elbo_and_grad itself covers q_diag, active_dims and the Matern families; round 4: Sum / Product of
    #  stationary kernels; round 5: members with their own active_dims, combinations under the un-whitened SVGP and SGPR --
    #  a diagonal q_sqrt under a combination, a heteroskedastic likelihood under either SVGP -- tests/test_gpu_gradients.py.
    #  and under the device-resident trainer, nested combinations.  Still out in the reverse pass: combinations holding something other
    #  than SquaredExponential / Matern members)
    odd = gpflow.models.SVGP(gpflow.kernels.Matern32() + gpflow.kernels.SeparateIndependent([gpflow.kernels.SquaredExponential()]), lik, Z)
    with pytest.raises(NotImplementedError):
        odd.elbo_and_grad(data)
    with pytest.raises(NotImplementedError):
        gpflow.optimizers.Scipy().minimize(object())


def test_adam_state_matches_tf_keras_rule():
    from gpflow_amd.training import _Adam
    opt = _Adam(1e-2, 0.9, 0.999, 1e-7)
    p = np.array([1.0, -2.0]); m = np.zeros(2); v = np.zeros(2)
    for t, g in enumerate([np.array([0.3, -0.1]), np.array([0.2, 0.4]), np.array([-0.5, 0.1])], start=1):
        opt.t = t
        p_new = opt.update_host("p", p, g)
        m = 0.9 * m + 0.1 * g; v = 0.999 * v + 0.001 * g * g
        lr_t = 1e-2 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        np.testing.assert_allclose(p_new, p - lr_t * m / (np.sqrt(v) + 1e-7), rtol=1e-14)
        p = p_new


def test_bench_spawns_its_own_ranks():
    """`python bench.py --gpus 2` without a launcher starts two ranks itself and rank 0 prints ONE JSON line with n_gpus = 2
    (the launch / barrier / MAX-over-ranks protocol, exercised on CPU through --dry-launch: gloo, no device work)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dry-launch", "--steps", "4", "--warmup", "1",
                        "--workload", "c4-strong"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["steps"] == 4 and rec["warmup"] == 1 and rec["scaling"] == "strong"
    assert rec["dry_launch"] is True and rec["allreduce_check"] is True


def test_bench_rejects_a_run_without_timed_steps():
    """`ms_per_step` is the wall-clock of the timed region over --steps: a run with no timed step is refused up front."""
    import subprocess
    import sys
    for extra in (["--steps", "0"], ["--steps", "2", "--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--full", "--dump-outputs", "unused"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--steps must be >= 1" in r.stderr, r.stderr[-2000:]
        assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert not os.path.exists(os.path.join(ROOT, "unused")) and not os.path.exists("unused")


def test_bench_refuses_fewer_devices_than_ranks():
    """Without enough devices a multi-rank bench must fail loudly, not run a silent 1-GPU job."""
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("node has two devices")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2"], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode != 0
    assert "needs 2 HIP devices" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_gaussian_rewraps_a_parameter_with_the_lower_bound_transform():
    """prepare_parameter_or_function (utilities/parameter_or_function.py:27-39) wraps ANY non-Function value -- a Parameter too --
    in Parameter(value, transform=positive(lower_bound)): a variance handed in with an identity transform must not be able to
    leave the bound, and prior / trainable carry over (base.py:155-161)."""
    import numpy as np
    import gpflow_amd as gpflow
    from gpflow_amd.base import Parameter
    raw = Parameter(0.3, trainable=False)                      # identity transform
    lik = gpflow.likelihoods.Gaussian(variance=raw)
    assert lik.variance is not raw and lik.variance.trainable is False
    assert abs(float(lik.variance.numpy()) - 0.3) < 1e-15
    lik.variance.assign_unconstrained(np.array(-50.0))        # far below anything an optimiser would reach
    assert float(lik.variance.numpy()) > lik.variance_lower_bound * (1 - 1e-12)


def test_check_info_names_a_timed_out_handoff():
    """include/gpk.h "info": INT_MAX is a timed-out internal hand-off, not a pivot column."""
    import torch
    from gpflow_amd import _lib, ops
    with pytest.raises(_lib.GpkError, match="hand-off timed out"):
        ops.check_info(torch.tensor([2 ** 31 - 1], dtype=torch.int32))
    with pytest.raises(_lib.GpkError, match="non-positive pivot at column 4"):
        ops.check_info(torch.tensor([5], dtype=torch.int32))


# ---------------------------------------------------------------- models/reverse.py: what the gradient entry points share
def test_to_unconstrained_chain_rule_sums_and_order():
    from gpflow_amd.base import Parameter, positive, triangular
    from gpflow_amd.models.reverse import to_unconstrained
    a, b = Parameter(np.array([0.7, 1.9]), transform=positive()), Parameter(np.array(2.0))
    frozen = Parameter(np.array(1.5), transform=positive(), trainable=False)
    M, P = 3, 2
    tri = Parameter(np.stack([np.tril(np.arange(1.0, 10.0).reshape(M, M))] * P), transform=triangular())
    ga1, ga2, gtri = np.array([0.5, -2.0]), np.array([4.0, 8.0]), np.arange(100.0, 100.0 + P * M * M).reshape(P, M, M)
    out = to_unconstrained([(b, np.array(3.0)), (a, ga1), (frozen, np.array(9.0)), (tri, gtri), (a, ga2)])
    assert list(out) == [b, a, tri]                                      # first occurrence, pair order; the frozen one is absent
    u = a.unconstrained_variable
    np.testing.assert_array_equal(out[a], ga1 * a.transform.forward_grad(u) + ga2 * a.transform.forward_grad(u))   # the sum, in pair order
    assert out[b] == 3.0 and np.shape(out[b]) == np.shape(b.unconstrained_variable)   # identity transform: forward_grad = 1
    # fill-triangular: an index map onto the lower-triangular entries -- the junk above the diagonal is dropped, nothing is scaled
    low = tri.transform.inverse(np.tril(gtri))
    np.testing.assert_array_equal(out[tri], low.reshape(tri.unconstrained_variable.shape))
    assert out[tri].size == P * M * (M + 1) // 2 and sorted(np.ravel(out[tri])) == sorted(gtri[:, np.tril_indices(M)[0], np.tril_indices(M)[1]].ravel())


def test_covariance_route_normalises_both_packings_of_the_kernel_gradients():
    """KernelSpec.pack returns "variance" [1] + "lengthscales" a tensor for one member, "variance" [n] + a list for several: the route
    pairs both with the members' Parameters, in member order; a Parameter shared by two members then collects the sum."""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd.models.reverse import CovarianceRoute, to_unconstrained
    K = gpflow.kernels
    one = K.Matern32(variance=0.7, lengthscales=[1.3, 0.8], active_dims=[0, 2])
    r1 = CovarianceRoute(one, 3)
    assert r1.spec.n == 1 and r1.spec.cols == [None] and r1.members == [(one.variance, one.lengthscales)]
    g1 = {"variance": torch.tensor([2.0]), "lengthscales": torch.tensor([3.0, 4.0])}
    assert r1.spec.pack([g1["variance"]], [g1["lengthscales"]])[1] is g1["lengthscales"]
    pairs = r1.kernel_pairs(g1)
    assert [p for p, _ in pairs] == [one.variance, one.lengthscales]
    np.testing.assert_array_equal(pairs[0][1], [2.0]); np.testing.assert_array_equal(pairs[1][1], [3.0, 4.0])
    k0, k2 = K.SquaredExponential(variance=1.3, lengthscales=0.9), K.Matern52(variance=0.9, lengthscales=0.8)
    k1 = K.Matern32(variance=0.7, lengthscales=1.1, active_dims=[1])
    k1.variance = k0.variance                                            # one Parameter, two members
    r3 = CovarianceRoute((k0 + k1) * k2, 3)
    assert r3.spec.n == 3 and r3.spec.tree == ("mul", [("add", [0, 1]), 2]) and r3.members[1][0] is k0.variance
    dvs, dls = [torch.tensor([1.0]), torch.tensor([10.0]), torch.tensor([100.0])], [torch.tensor([5.0]), torch.tensor([6.0]), torch.tensor([7.0])]
    g3 = dict(zip(("variance", "lengthscales"), r3.spec.pack(dvs, dls)))
    assert g3["variance"].shape == (3,) and isinstance(g3["lengthscales"], list)
    pairs = r3.kernel_pairs(g3)
    assert [p for p, _ in pairs] == [k0.variance, k0.lengthscales, k0.variance, k1.lengthscales, k2.variance, k2.lengthscales]
    assert [float(np.ravel(v)[0]) for _, v in pairs] == [1.0, 5.0, 10.0, 6.0, 100.0, 7.0]
    out = to_unconstrained(pairs)
    assert list(out) == [k0.variance, k0.lengthscales, k1.lengthscales, k2.variance, k2.lengthscales]
    u = k0.variance.unconstrained_variable
    np.testing.assert_array_equal(out[k0.variance], 1.0 * k0.variance.transform.forward_grad(u) + 10.0 * k0.variance.transform.forward_grad(u))
    # the device form the trainer takes: one [1] and one flat tensor per member
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in r3.member_grads(g3)] == [((1,), (1,))] * 3
    assert [(tuple(a.shape), tuple(b.shape)) for a, b in r1.member_grads(g1)] == [((1,), (2,))]
    with pytest.raises(NotImplementedError):
        CovarianceRoute(K.SharedIndependent(k2, 2), 3)


def test_every_gradient_entry_point_refuses_before_the_device(monkeypatch):
    """Every (entry point, model) pair that tools/reverse_pass_log.py's model matrix records as refused: the same exception type, and
    `ops.to_device` is never reached.  (GPR / SGPR hold their data on the device: it is 'uploaded' to the CPU while they are built.  One
    more refusal of that matrix is not here: the SGPR with a constant noise that is no `variance` Parameter says so after its `_config`,
    which has fetched Z by then -- tests/test_gpu_sgpr.py.)"""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd import ops, training
    K, L, IV, MF = gpflow.kernels, gpflow.likelihoods, gpflow.inducing_variables, gpflow.mean_functions
    rng = np.random.default_rng(0)
    N, M, D = 6, 4, 3
    X, Z, Y = rng.normal(size=(N, D)), rng.normal(size=(M, D)), rng.normal(size=(N, 2))
    se, m32 = lambda **kw: K.SquaredExponential(**kw), lambda **kw: K.Matern32(**kw)  # noqa: E731
    gauss = lambda: L.Gaussian(0.2)  # noqa: E731
    het = lambda: L.Gaussian(scale=gpflow.functions.Linear(A=np.array([[-0.1], [0.05], [0.02]]), b=np.array([0.6])))  # noqa: E731
    shared_z = lambda: IV.SharedIndependentInducingVariables(IV.InducingPoints(Z.copy()))  # noqa: E731
    separate_z = lambda: IV.SeparateIndependentInducingVariables([IV.InducingPoints(Z.copy()), IV.InducingPoints(Z + 0.1)])  # noqa: E731
    sep = lambda: K.SeparateIndependent([se(), m32()])  # noqa: E731

    def same_z_twice():   # (one InducingPoints object for both latents is still not the SHARED inducing variable the trainer asks for)
        p0 = IV.InducingPoints(Z.copy())
        return IV.SeparateIndependentInducingVariables([p0, p0])
    linear = lambda q: MF.Linear(A=np.ones((D, q)), b=np.zeros(q))  # noqa: E731

    def svgp(k, lik, iv=None, P=1, **kw):
        return gpflow.models.SVGP(k, lik, Z.copy() if iv is None else iv, num_latent_gps=P, **kw)

    def k_sum():
        k0 = se()
        return k0 + k0
    elbo = lambda m, P=1: (lambda: m.elbo_and_grad((X, Y[:, :P])))  # noqa: E731
    trainer = lambda m, **kw: (lambda: training.SVGPTrainer(m, **kw))  # noqa: E731
    natgrad = lambda m, P=1: (lambda: gpflow.optimizers.NaturalGradient(1.0).minimize(m, (X, Y[:, :P])))  # noqa: E731
    table = [(elbo(svgp(sep(), lik(), iv(), P=2, q_diag=True, whiten=wh), 2), NotImplementedError)
             for wh in (True, False) for iv in (shared_z, separate_z) for lik in (gauss, het)]
    table += [(elbo(svgp(se(), L.Bernoulli(), whiten=False)), NotImplementedError),
              (elbo(svgp(m32(active_dims=[0, 2]), L.Bernoulli())), NotImplementedError),
              (elbo(svgp(k_sum(), L.Bernoulli())), NotImplementedError),
              (elbo(svgp(se(), L.MultiClass(3), P=2)), ValueError),
              (elbo(svgp(se(), gauss(), mean_function=linear(1))), NotImplementedError),
              (elbo(svgp(se() + K.SeparateIndependent([se()]), gauss())), NotImplementedError),
              (elbo(svgp(K.SharedIndependent(k_sum(), 1), gauss(), shared_z())), NotImplementedError),
              (elbo(svgp(K.SeparateIndependent([se()]), gauss())), NotImplementedError),
              (elbo(svgp(K.SeparateIndependent([se() + m32(), se()]), gauss(), shared_z(), P=2), 2), NotImplementedError),
              (trainer(svgp(K.SeparateIndependent([se() + m32(), se()]), gauss(), shared_z(), P=2)), NotImplementedError),
              (trainer(svgp(sep(), gauss(), same_z_twice(), P=2)), NotImplementedError),
              (trainer(svgp(sep(), gauss(), separate_z(), P=2)), NotImplementedError),
              (trainer(svgp(se(), gauss(), q_diag=True), natgrad_gamma=0.5), NotImplementedError),
              (trainer(svgp(se(), L.Bernoulli())), NotImplementedError),
              (trainer(svgp(se(), gauss(), mean_function=linear(1))), NotImplementedError),
              (natgrad(svgp(m32(active_dims=[0, 2]), gauss())), NotImplementedError),
              (natgrad(svgp(se(), gauss(), q_diag=True)), NotImplementedError),
              (natgrad(svgp(se(), het())), NotImplementedError),
              (natgrad(svgp(k_sum(), gauss())), NotImplementedError),
              (natgrad(svgp(sep(), gauss(), shared_z(), P=2), 2), NotImplementedError),
              (natgrad(svgp(se(), L.Bernoulli())), NotImplementedError)]
    monkeypatch.setattr(ops, "to_device", lambda x, dtype=torch.float64: torch.as_tensor(np.asarray(x), dtype=dtype))
    table += [(gpflow.models.GPR((X, Y), se(), mean_function=linear(2)).objective_and_grad, NotImplementedError),
              (gpflow.models.GPR((X, Y), se(), likelihood=L.Gaussian(scale=0.4)).objective_and_grad, NotImplementedError),
              (gpflow.models.SGPR((X, Y), se(), Z.copy(), mean_function=linear(2)).objective_and_grad, NotImplementedError)]

    def reached(*a, **kw):
        pytest.fail("ops.to_device was reached before the refusal")
    monkeypatch.setattr(ops, "to_device", reached)
    for i, (call, exc) in enumerate(table):
        with pytest.raises(exc) as e:
            call()
        assert e.type is exc, (i, e.type)


def test_trainer_treats_one_separate_kernel_as_separate(monkeypatch):
    """SeparateIndependent decides the trainer's naming and its column check, not the number of members: one member still reads
    kvar_ / kls_ entries (Adam's state is keyed by them) and still wants one output column per member."""
    import torch
    import gpflow_amd as gpflow
    from gpflow_amd import ops, training
    K, IV = gpflow.kernels, gpflow.inducing_variables
    rng = np.random.default_rng(1)
    X, Z, Y = rng.normal(size=(6, 3)), rng.normal(size=(4, 3)), rng.normal(size=(6, 2))
    monkeypatch.setattr(ops, "to_device", lambda x, dtype=torch.float64: torch.as_tensor(np.asarray(x), dtype=dtype))
    m = gpflow.models.SVGP(K.SeparateIndependent([K.SquaredExponential()]), gpflow.likelihoods.Gaussian(0.2),
                           IV.SharedIndependentInducingVariables(IV.InducingPoints(Z)), num_latent_gps=1)
    tr = training.SVGPTrainer(m)
    assert list(tr.host) == ["kvar_0", "kls_1", "noise_variance"]
    with pytest.raises(ValueError, match="1 separate kernels need 1 output columns"):
        tr.step((X, Y))
