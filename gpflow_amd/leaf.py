"""What a device-built kernel leaf consists of, written once: the table of families and the value type `Leaf`.

A leaf is one kernel that `gpk_kernel_matrix` builds from host hyperparameters.  Its pieces travel in one order everywhere -- as the
Parameters of the kernel class, as the `ls_host` array of the C-ABI, as a shape gradient of the reverse pass:

    variance, lengthscales (a family with a distance), then the family's extras in the order of its table row

`ops` (the C-ABI form), `kernels` (the classes answer `leaf()`) and `gradients.KernelSpec` (its members are leaves) import this
module; it imports none of them.  A new family is a row of FAMILIES; a new extra hyperparameter is a name in that row.
"""
from __future__ import annotations

import collections
from typing import NamedTuple, Tuple

import numpy as np

from . import _lib


class Family(NamedTuple):
    name: str
    code: int              # GPK_KERN_* of include/gpk.h
    has_distance: bool     # False: a static family -- the inputs are never read, no lengthscale or input gradient
    extras: Tuple[str, ...] = ()   # extra hyperparameters, in the order they follow the lengthscales in `ls_host`

    @property
    def parameters(self) -> Tuple[str, ...]:
        """names of a leaf's hyperparameters (and of its kernel class's Parameters) in their one order"""
        return ("variance",) + (("lengthscales",) if self.has_distance else ()) + self.extras


FAMILIES = (Family("SquaredExponential", 0, True), Family("Matern12", 1, True), Family("Matern32", 2, True),
            Family("Matern52", 3, True), Family("Exponential", 4, True), Family("RationalQuadratic", 5, True, ("alpha",)),
            Family("White", 6, False), Family("Constant", 7, False))
BY_NAME = {f.name: f for f in FAMILIES}
_EXTRA_OWNER = {x: f.name for f in FAMILIES for x in f.extras}
_DUMMY_LENGTHSCALE = np.asarray(1.0, dtype=np.float64)   # what a static leaf hands the builders: never read


class Leaf(collections.namedtuple("_LeafFields", "row variance lengthscales extras")):
    """One leaf's host values, immutable: `row` (its Family; `family` is the name), `variance`, `lengthscales` (0-d isotropic or
    [D]; a static family's is the dummy 1.0 the builders never read) and `extras`, the family's extra hyperparameters in the row's
    order.  Made from keywords -- Leaf(family, variance, lengthscales, alpha=...) -- or, `of` / `replace`, from values in Parameter
    order."""
    __slots__ = ()

    def __new__(cls, family: str, variance, lengthscales=None, **extras):
        row = BY_NAME[family]
        for name, value in extras.items():
            if value is not None and name not in row.extras:
                raise ValueError(f"{name} belongs to the {_EXTRA_OWNER[name]!r} family, not to {family!r}")
        values = ()
        if row.extras:
            for name in row.extras:
                if extras.get(name) is None:
                    raise ValueError(f"family {family!r} needs {name}")
            values = tuple(float(extras[name]) for name in row.extras)
        return tuple.__new__(cls, (row, float(variance), _DUMMY_LENGTHSCALE if lengthscales is None
                                   else np.asarray(lengthscales, dtype=np.float64), values))

    @classmethod
    def of(cls, family: str, values) -> "Leaf":
        """from the values in Parameter order (Family.parameters)"""
        return cls(family, **dict(zip(BY_NAME[family].parameters, values)))

    def replace(self, values) -> "Leaf":
        """the same family with other values, given in Parameter order"""
        return Leaf.of(self.family, values)

    @property
    def family(self) -> str:
        return self.row.name

    @property
    def code(self) -> int:
        return self.row.code

    @property
    def is_static(self) -> bool:
        return not self.row.has_distance

    @property
    def is_plain(self) -> bool:
        """(variance, lengthscales) and nothing else: what the packed covariance tail and the trainer's device step keep"""
        return self.row.has_distance and not self.row.extras

    @property
    def n_lengthscales(self) -> int:
        """lengthscale entries (0 = static, 1 = isotropic, D = ARD)"""
        return int(self.lengthscales.size) if self.row.has_distance else 0

    @property
    def n_shape(self) -> int:
        """entries of the shape gradient: the lengthscales, then the extras"""
        return self.n_lengthscales + len(self.extras)

    def keywords(self) -> dict:
        """as the `ops` builders take a leaf: variance=, lengthscales=, family=, and an extra's keyword only where the family has one"""
        return dict(variance=self.variance, lengthscales=self.lengthscales, family=self.family, **dict(zip(self.row.extras, self.extras)))

    def host(self, d: int):
        """(host array, ard) of the C-ABI: the lengthscales, then the extras (include/gpk.h, next to the family codes)"""
        ls = np.atleast_1d(self.lengthscales)
        ard = ls.size > 1
        if ard and ls.size != d:
            raise ValueError(f"lengthscales has {ls.size} entries, input dimension is {d}")
        return _lib.host_doubles(ls.tolist() + list(self.extras)), int(ard)

    def split_shape(self, g) -> dict:
        """a shape gradient, laid out like `host`, as {"lengthscales": ..., <extra>: [1], ...}"""
        if not self.extras:
            return {"lengthscales": g}
        cuts = [self.n_lengthscales + j for j in range(len(self.extras))] + [None]   # (the extras partition what follows the lengthscales)
        return {"lengthscales": g[:cuts[0]], **{name: g[cuts[j]:cuts[j + 1]] for j, name in enumerate(self.row.extras)}}


def latent_keywords(leaves, d: int) -> dict:
    """variances=, lengthscales=, families= as the per-latent shards (ops.svgp_elbo_shard_sep / _lcm) take one leaf per latent:
    lengthscales [n] (all isotropic) or [n, d]"""
    if any(leaf.extras for leaf in leaves):
        raise NotImplementedError("SeparateIndependent / LinearCoregionalization with a RationalQuadratic member: the fused per-latent "
                                  "shard strides its lengthscales by latent and has no slot for alpha (include/gpk.h)")
    ls = [np.atleast_1d(leaf.lengthscales) for leaf in leaves]
    if any(l.size > 1 for l in ls):   # mixed isotropic / ARD members: every row spelled out
        ls = np.stack([np.broadcast_to(l, (d,)) for l in ls])
    else:
        ls = np.concatenate(ls)
    return dict(variances=[leaf.variance for leaf in leaves], lengthscales=ls, families=[leaf.family for leaf in leaves])
