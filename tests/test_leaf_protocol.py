"""CPU: the protocol every kind of kernel leaf answers (gpflow_amd/leaf.py, the comment block at its top), held for one instance of
each of the four value types -- ARD and not where the type has both -- and the three kernel predicates of kernels/base.py, pairwise
exclusive over one kernel of every class in gpflow_amd.kernels.  No device and no library call: `builders` is checked against the
signatures of the `ops` functions it names, which are not called.
"""
import inspect

import numpy as np
import pytest

import gpflow_amd.kernels as K
from gpflow_amd import ops
from gpflow_amd.kernels.base import has_row_diagonal_leaf, is_arc_leaf, is_coregion_leaf, is_device_leaf, is_dot_leaf
from gpflow_amd.leaf import ArcLeaf, CoregionLeaf, DotLeaf, Leaf

D = 3
LEAVES = {
    "se_iso": Leaf("SquaredExponential", 1.3, 0.9),
    "se_ard": Leaf("SquaredExponential", 1.3, [0.9, 1.4, 1.1]),
    "rq_ard": Leaf("RationalQuadratic", 0.9, [0.9, 1.4, 1.1], alpha=0.7),
    "white": Leaf("White", 0.3),
    "linear_iso": DotLeaf("Linear", 0.8),
    "linear_ard": DotLeaf("Linear", [0.5, 2.0, 1.25]),
    "polynomial_ard": DotLeaf("Polynomial", [0.4, 0.9, 0.6], offset=0.5, degree=2),
    "arc_iso": ArcLeaf(1, 0.9, 0.7, 0.4),
    "arc_ard": ArcLeaf(2, 0.9, [0.6, 1.1, 0.8], 0.4),
    "coregion": CoregionLeaf(0.1 * np.arange(6.0).reshape(3, 2), [0.5, 1.0, 1.5]),
}


def _values(leaf):
    """the leaf's own values in `parameters` order (every one of them is a keyword of its builders)"""
    return [leaf.keywords()[name] for name in leaf.parameters]


def _same(a, b):
    ka, kb = a.keywords(), b.keywords()
    return type(a) is type(b) and a.family == b.family and ka.keys() == kb.keys() and all(np.array_equal(ka[k], kb[k]) for k in ka)


@pytest.mark.parametrize("name", LEAVES)
def test_gradient_layout_agrees_with_the_values(name):
    """`parameters` names the variance slot, then the pieces of the shape gradient in the order `split_shape` cuts them; `n_variance` and
    `n_shape` are the sizes of the leaf's own values"""
    leaf = LEAVES[name]
    values = dict(zip(leaf.parameters, _values(leaf)))
    assert isinstance(leaf.family, str) and len(values) == len(leaf.parameters) >= 1
    assert leaf.n_variance == np.size(values[leaf.parameters[0]])
    g = np.arange(leaf.n_shape, dtype=np.float64)
    pieces = leaf.split_shape(g)
    assert [k for k in pieces if k != "lengthscales" or "lengthscales" in values] == list(leaf.parameters[1:])
    assert "lengthscales" in pieces and (pieces["lengthscales"].size == 0 or "lengthscales" in values)   # (the members' convention)
    assert np.array_equal(np.concatenate([np.ravel(p) for p in pieces.values()]), g)      # a partition of the gradient, in order
    assert leaf.n_shape == sum(np.size(values[k]) for k in leaf.parameters[1:])
    for k in leaf.parameters[1:]:
        assert pieces[k].size == np.size(values[k]), k
    assert isinstance(leaf.is_plain, bool) and leaf.is_plain == (name in ("se_iso", "se_ard"))


@pytest.mark.parametrize("name", LEAVES)
def test_replace_with_its_own_values_gives_an_equal_leaf(name):
    leaf = LEAVES[name]
    again = leaf.replace(_values(leaf))
    assert _same(leaf, again) and again is not leaf
    doubled = leaf.replace([2.0 * np.asarray(v) for v in _values(leaf)])
    assert not _same(leaf, doubled) and doubled.family == leaf.family and doubled.n_shape == leaf.n_shape
    assert all(np.array_equal(np.asarray(d), 2.0 * np.asarray(v)) for d, v in zip(_values(doubled), _values(leaf)))
    for const in ("degree", "order"):      # the constants of a leaf go with it
        assert getattr(doubled, const, None) == getattr(leaf, const, None)


@pytest.mark.parametrize("name", LEAVES)
def test_builders_name_ops_functions_that_take_the_keywords(name):
    leaf = LEAVES[name]
    matrix, combine, diag = leaf.builders
    assert (diag is None) == leaf.constant_diagonal == isinstance(leaf, Leaf)      # the constant diagonal: a Leaf, and only it
    for fn_name, operands in ((matrix, ("X1", "X2")), (combine, ("X1", "X2", "G")), (diag, ("X",))):
        if fn_name is None:
            continue
        fn = getattr(ops, fn_name)
        assert inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not fn_name.startswith("_")
        bound = inspect.signature(fn).bind_partial(*operands, **leaf.keywords())      # TypeError for a keyword the function does not take
        assert list(bound.arguments)[:len(operands)] == list(operands)
        assert "out" in inspect.signature(fn).parameters and ("op" in inspect.signature(fn).parameters) == (fn_name != matrix)


@pytest.mark.parametrize("name", LEAVES)
def test_abi_is_the_code_then_the_host_form(name):
    leaf = LEAVES[name]
    if isinstance(leaf, CoregionLeaf):      # no host-only form: its table lives on the device, `ops` resolves it
        assert not hasattr(leaf, "abi") and not hasattr(leaf, "host")
        return
    code, host, ard, *rest = leaf.abi(D)
    assert code == (leaf.order if isinstance(leaf, ArcLeaf) else leaf.code) and ard == int(name.endswith("_ard"))
    assert list(host) == list(leaf.host(D)[0]) and ard == leaf.host(D)[1]
    assert rest == {Leaf: lambda: [leaf.variance], DotLeaf: lambda: [leaf.offset, leaf.degree],
                    ArcLeaf: lambda: [leaf.variance, leaf.bias_variance]}[type(leaf)]()
    if ard:
        with pytest.raises(ValueError, match="entries"):
            leaf.abi(D + 1)


def _one_of_every_class():
    se = lambda: K.SquaredExponential(variance=1.3, lengthscales=0.9)  # noqa: E731
    made = {"Sum": K.Sum([se(), K.Linear()]), "Product": K.Product([se(), K.ArcCosine()]), "Combination": K.Combination([se(), se()]),
            "Periodic": K.Periodic(se()), "Coregion": K.Coregion(3, 2, active_dims=[1]),
            "ChangePoints": K.ChangePoints([se(), K.Linear()], locations=[0.5]), "SharedIndependent": K.SharedIndependent(se(), 2),
            "SeparateIndependent": K.SeparateIndependent([se(), K.Linear()]),
            "LinearCoregionalization": K.LinearCoregionalization([se(), se()], np.ones((2, 2)))}
    for name in K.__all__:
        cls = getattr(K, name)
        if name not in made and not inspect.isabstract(cls) and cls not in (K.Stationary, K.IsotropicStationary, K.Static, K.MultioutputKernel):
            made[name] = cls()
    return made


def test_the_kernel_predicates_are_pairwise_exclusive():
    made = _one_of_every_class()
    assert {type(k) for k in made.values()} >= {getattr(K, n) for n in K.__all__ if not inspect.isabstract(getattr(K, n))} \
        - {K.Stationary, K.IsotropicStationary, K.Static, K.MultioutputKernel}
    kinds = {}
    for name, k in made.items():
        answers = [is_dot_leaf(k), is_arc_leaf(k), is_coregion_leaf(k)]
        assert sum(answers) <= 1 and has_row_diagonal_leaf(k) == any(answers), name
        assert not (any(answers) and is_device_leaf(k)), name
        kinds[name] = ("dot", "arc", "coregion")[answers.index(True)] if any(answers) else None
    assert {n: v for n, v in kinds.items() if v} == {"Linear": "dot", "Polynomial": "dot", "ArcCosine": "arc", "Coregion": "coregion"}
    for name, kind in kinds.items():      # the kernel's leaf is of the kind the predicate says, and only a Leaf has the constant diagonal
        if kind:
            assert type(made[name].leaf()) is {"dot": DotLeaf, "arc": ArcLeaf, "coregion": CoregionLeaf}[kind]
            assert made[name].leaf().constant_diagonal is False
    assert is_device_leaf(made["SquaredExponential"]) and made["SquaredExponential"].leaf().constant_diagonal is True
