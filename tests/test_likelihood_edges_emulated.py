"""CPU: the test bodies of tests/test_gpu_likelihood_edges.py -- the likelihood stages at extreme arguments -- with the device
primitives replaced by their NumPy emulation (tests/emulation.py), following tests/test_likelihood_zoo_emulated.py.  What this does
NOT test is the HIP kernels: that is what the same bodies do under `-m gpu`.  What it does test is that the references, their bounds
and the underflow floor hold for a plain fp64 evaluation of the contract, so that a failure on the device is the device's.
"""
import pytest

import emulation
import test_gpu_likelihood_edges as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n
