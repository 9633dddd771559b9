"""CPU: the test bodies of tests/test_gpu_wide_inputs.py with the device primitives replaced by their NumPy emulation, as
tests/test_kernel_families_emulated.py drives tests/test_gpu_kernel_families.py.  The emulation never had a width limit: what this
holds is the ROUTING of wide leaves on the CPU tier -- the model layer past the fused drivers, the reverse pass, the refusals and
what the library answers before it touches a device -- not the HIP kernel; that is what the same bodies do under `-m gpu`.
"""
import pytest

import emulation
import test_gpu_wide_inputs as T


@pytest.fixture
def gp(monkeypatch):
    return emulation.install(monkeypatch)


for _n in [n for n in dir(T) if n.startswith("test_")]:
    globals()[_n] = getattr(T, _n)
del _n
