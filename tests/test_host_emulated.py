"""CPU: the WHOLE host layer (models, posteriors, conditionals, KL, covariances, kernels, likelihoods) driven end to
end against the oracle with the device primitives replaced by their CPU emulation (tests/emulation.py; tests/fake_ops.py
reproduces each kernel's read / write contract).  The test bodies are the GPU parity tests of tests/test_gpu_models.py
themselves -- imported here without that module's `gpu` mark and given an emulated `gp` fixture -- so the routing,
shapes, transposes, broadcasting and error behaviour of the Python mirror are exercised in the `-m "not gpu"` tier too.
What this does NOT test is the HIP kernels: that is what the same bodies do under `-m gpu`.
"""
import pytest

import emulation
import test_gpu_models as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


@pytest.fixture
def gpu(gp):
    """The next-row GPU tests (gradients, trainer, SGPR, natural gradient) ask for the `gpu` fixture: under emulation it
    is the patched primitive layer and a CPU device."""
    import torch
    return torch.device("cpu")


_names = [n for n in dir(T) if n.startswith("test_")]
for _n in _names:
    globals()[_n] = getattr(T, _n)
import test_gpu_gradients as TG  # noqa: E402
import test_gpu_reference_golden as TR  # noqa: E402  (values computed by the reference's own source)
import test_gpu_sgpr as TS  # noqa: E402

for _mod, _pre in ((TG, "grad"), (TS, "sgpr"), (TR, "refgolden")):
    for _n in [n for n in dir(_mod) if n.startswith("test_")]:
        globals()[f"test_{_pre}_{_n[5:]}"] = getattr(_mod, _n)
del _n, _mod, _pre


# ------------------------------------------------------------------------------------------------ the emulation itself
def test_every_emulated_name_is_defined_in_one_module():
    """emulation.primitives() refuses a public name that two modules define; the modules as they are pass, and every primitive
    comes from the module that defines it"""
    import types
    found = emulation.primitives()
    assert all(fn.__module__ in {m.__name__ for m in emulation.MODULES} for fn in found.values())
    assert {"kernel_matrix", "svgp_elbo_shard", "likelihood_varexp_sum", "svgp_elbo_shard_lik", "svgp_elbo_shard_lcm", "periodic_warp",
            "dot_kernel_matrix"} <= set(found) and "torch" not in found and "gauss_hermite" in found
    twice = types.ModuleType("fake_twice_ops")
    twice.kernel_matrix = lambda: None
    twice.kernel_matrix.__module__ = twice.__name__
    with pytest.raises(RuntimeError, match="kernel_matrix is defined in fake_ops and in fake_twice_ops"):
        emulation.primitives(emulation.MODULES + (twice,))


def test_the_likelihood_table_has_a_row_per_code():
    import fake_likelihood_ops
    import fake_ops
    from gpflow_amd import ops
    assert set(fake_likelihood_ops.LIKELIHOODS) == set(ops.LIKELIHOOD_CODES)
    assert fake_ops.KERNEL_FAMILIES == ops.KERNEL_FAMILIES
