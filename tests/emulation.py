"""The CPU emulation of `gpflow_amd.ops` as ONE set of primitives -- TEST INFRASTRUCTURE ONLY.

`MODULES` are the modules that hold it; each public function is an emulated primitive of the module that DEFINES it (a name a module
merely imports is not its own), and no name is defined twice, so there is no order among them.  `install(monkeypatch)` is the `gp`
fixture of every tests/*_emulated.py; `primitives()` is what a logging proxy in the place of `gradients.ops` is built from
(tools/reverse_pass_log.py, the call-log tests).  A new primitive goes into the module of its kind, or into a new module listed here.
"""
import types

import fake_dot_ops
import fake_lcm_ops
import fake_likelihood_ops
import fake_ops
import fake_periodic_ops

MODULES = (fake_ops, fake_likelihood_ops, fake_periodic_ops, fake_lcm_ops, fake_dot_ops)


def primitives(modules=MODULES):
    """name -> function over all of `modules`; a name that two of them define is an error"""
    found = {}
    for mod in modules:
        for name, fn in vars(mod).items():
            if name.startswith("_") or not isinstance(fn, types.FunctionType) or fn.__module__ != mod.__name__:
                continue
            if name in found:
                raise RuntimeError(f"{name} is defined in {found[name].__module__} and in {mod.__name__}")
            found[name] = fn
    return found


def install(monkeypatch):
    """every `gpflow_amd.ops` name the emulation defines replaced by it for the duration of a test; returns the package"""
    import gpflow_amd
    from gpflow_amd import ops
    for name, fn in primitives().items():
        if hasattr(ops, name):
            monkeypatch.setattr(ops, name, fn)
    return gpflow_amd
