"""CPU: the full variational GP (the primitive's contract, the reverse pass, models.VGP on every route) driven by the test bodies of
tests/test_gpu_vgp.py with the device primitives replaced by their NumPy emulation -- tests/emulation.py's modules and
tests/fake_vgp_ops.py, installed here -- as tests/test_dot_kernels_emulated.py drives tests/test_gpu_dot_kernels.py.  What this does
NOT test is the HIP kernel: that is what the same bodies do under `-m gpu`.  The CPU-only checks of the feature (the launch inventory
of gpflow_amd/csrc/vgp, the exports, the launch list of the reverse pass) are at the end; they need no device.
"""
import os
import re
import types

import numpy as np
import pytest

import emulation
import fake_vgp_ops
import test_gpu_vgp as T
import test_launch_geometry as G

MODULES = emulation.MODULES + (fake_vgp_ops,)


@pytest.fixture
def gp(monkeypatch):
    import gpflow_amd
    from gpflow_amd import ops
    for name, fn in emulation.primitives(MODULES).items():
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, fn)
    return gpflow_amd


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n


# ------------------------------------------------------------------------------------------------ CPU-only checks
VGP_CSRC = os.path.join(G.CSRC, "vgp")
# one row per launch site of gpflow_amd/csrc/vgp/*.hip (tests/test_launch_geometry.py inventories csrc/*.hip and keeps its own table)
VGP_LAUNCHES = [
    # one workgroup per (tile, latent), the tiles decoded from blockIdx.x alone: the grid is the whole geometry
    G.exact("tril_product.hip", "tril_product_kernel", "hipLaunchKernelGGL(tril_product_kernel, dim3((unsigned)tiles), dim3(256)"),
    G.exact("tril_product.hip", "tril_rowsum_kernel", "hipLaunchKernelGGL(tril_rowsum_kernel, dim3((unsigned)blocks), dim3(256)"),
]


def test_launch_inventory_of_the_vgp_directory():
    """launch sites == rows, no kernel mentions gridDim, every quoted launch expression stands; a row taken out is seen"""
    sources = G._sources(VGP_CSRC)
    assert sorted(sources) == ["tril_product.hip"]
    assert G.problems(VGP_LAUNCHES, sources) == []
    for row in VGP_LAUNCHES:
        bad = G.problems([r for r in VGP_LAUNCHES if r is not row], sources)
        assert any("launch without a row" in b and row["kernel"] in b for b in bad), (row["kernel"], bad)
    assert {k for _, k in G.kernel_bodies(sources)} == {"tril_product_kernel", "tril_rowsum_kernel"}
    assert "gridDim" not in sources["tril_product.hip"]
    assert G.problems(G.LAUNCHES, G._sources()) == []          # (the sub-directory is not part of that inventory)


def test_exports_header_and_class():
    import gpflow_amd as gpflow
    from gpflow_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "gpk.h")).read()
    declared = set(re.findall(r"\b(gpk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    lib = _lib.load()
    assert {"gpk_tril_product", "gpk_tril_product_tiles"} <= declared and declared == set(_lib.EXPORTED_SYMBOLS) \
        and all(hasattr(lib, n) for n in declared)
    assert int(re.search(r"#define GPK_TRIL_TILE (\d+)", text).group(1)) == ops.TRIL_TILE == fake_vgp_ops.TRIL_TILE == T.T
    assert "VGP" in gpflow.models.__all__ and issubclass(gpflow.models.VGP, gpflow.models.GPModel)
    assert {"tril_product", "tril_product_parts"} <= set(emulation.primitives(MODULES)) - set(emulation.primitives())
    readme = open(os.path.join(root, "README.md")).read()
    assert f"{len(declared)} functions" in readme


def test_the_reverse_pass_issues_two_products_and_no_composed_form(monkeypatch):
    """gradients.vgp_elbo_and_grad through a logging proxy: tril_product twice (row sums, then the stored seed), one factorisation,
    one variational-expectation stage called with knn = 0 and s0 = None, one KL, and no projection / N x N product of the composed
    route in front of the likelihood"""
    import torch
    from gpflow_amd import gradients
    calls, seen = [], {}

    def logged(name, fn):
        def call(*a, **kw):
            calls.append(name)
            if name.endswith("varexp_sum"):
                seen.update(knn=kw["knn"], s0=kw["s0"])
            return fn(*a, **kw)
        return call
    monkeypatch.setattr(gradients, "ops", types.SimpleNamespace(**{n: logged(n, fn) for n, fn in emulation.primitives(MODULES).items()}))
    X, Y, q_mu, q_sqrt = T._data("bernoulli_probit", 40, 2, 2, 3)
    t = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))  # noqa: E731
    gradients.vgp_elbo_and_grad(t(X), t(Y), t(q_mu), t(q_sqrt), kernel_spec=gradients.KernelSpec.single(1.3, 0.9), jitter=1e-6,
                                likelihood=("bernoulli_probit", ()))
    assert calls.count("tril_product") == 2 and calls.count("potrf_") == 1 and calls.count("gauss_kl_white") == 1
    assert calls.count("likelihood_varexp_sum") == 1 and list(seen["knn"]) == [0.0] and seen["s0"] is None
    assert not [c for c in calls if c in ("project", "project_stats")]
    assert calls.index("tril_product") < calls.index("likelihood_varexp_sum") < len(calls) - 1 - calls[::-1].index("tril_product")
