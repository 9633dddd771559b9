"""What a device-built kernel leaf consists of, written once: the tables of families and the four value types of a leaf.

A leaf is one kernel that the device builds from host hyperparameters.  There are four kinds, one immutable value type each:

    Leaf          a row of FAMILIES (stationary, static; a Periodic kernel's base), built by `gpk_kernel_matrix`; K(x, x) = variance
    DotLeaf       a row of DOT_FAMILIES (Linear, Polynomial), built by the `gpk_dot_*` entry points
    ArcLeaf       ArcCosine of order 0, 1 or 2, built by the `gpk_arccos_*` entry points
    CoregionLeaf  Coregion over one column of task labels, built by the `gpk_coregion_*` entry points

THE PROTOCOL.  Every kind answers the same names with the same meaning; `ops` (the C-ABI form), `kernels` (the classes answer
`leaf()`) and `gradients.KernelSpec` (its members are leaves) ask nothing else of a leaf, and none of them asks which kind it is:

    family              the name of the leaf's family
    parameters          the names of its hyperparameters (and of its kernel class's Parameters) in the ONE order they travel in: as
                        the values `replace` takes, as the gradients of the reverse pass (the variance slot, then the shape gradient)
    n_variance          entries of the gradient slot a KernelSpec calls "variance": 1; D for an ARD DotLeaf; P (d/dkappa) for Coregion
    n_shape             entries of the shape gradient, everything after that slot
    split_shape(g)      a shape gradient as {"lengthscales": ..., <name>: ..., ...} ("lengthscales" empty where the kind has none)
    keywords()          the leaf as the keywords of its `ops` builders
    replace(values)     the same family (and constants: degree, order) with other values, given in `parameters` order
    is_plain            (variance, lengthscales) and nothing else: what the packed covariance tail and the trainer's device step keep
    constant_diagonal   K(x, x) is one host value, the variance (Leaf); False: it depends on the row and the kind has a diag builder
    builders            the names of the kind's `ops` functions: (matrix, combine, row diagonal or None)
    abi(d)              what stands between the operands and `diag_add` in the kind's C entry points for inputs of d columns, the
                        code that goes in front of the operands first: (code, *host(d), variance) for a Leaf -- `host` is the
                        lengthscales, then the family's extras in the order of its table row --, (code, w, ard, offset, degree) for a
                        DotLeaf, (order, w, ard, variance, bias) for an ArcLeaf.  A CoregionLeaf has no host-only form -- its table
                        B = W W^T + diag(kappa) lives on the device -- and so no `abi`: it keeps W / kappa, and `ops` resolves B.

This module imports none of its users.  A new family is a row of FAMILIES or DOT_FAMILIES, a new extra hyperparameter a name in that
row; a new KIND is one more value type here that answers the protocol (then: three thin `ops` wrappers, a kernel class on
kernels.base.RowDiagonalLeaf, a member class in `gradients`).
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
    n_variance, constant_diagonal = 1, True
    builders = ("kernel_matrix", "kernel_matrix_combine", None)

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
    def parameters(self) -> Tuple[str, ...]:
        return self.row.parameters

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
        ls = self.lengthscales if self.lengthscales.ndim else self.lengthscales.reshape(1)
        ard = ls.size > 1
        if ard and ls.size != d:
            raise ValueError(f"lengthscales has {ls.size} entries, input dimension is {d}")
        return _lib.host_doubles(ls.tolist() + list(self.extras)), int(ard)

    def abi(self, d: int) -> tuple:
        return (self.code, *self.host(d), self.variance)

    def split_shape(self, g) -> dict:
        """a shape gradient, laid out like `host`, as {"lengthscales": ..., <extra>: [1], ...}"""
        if not self.extras:
            return {"lengthscales": g}
        cuts = [self.n_lengthscales + j for j in range(len(self.extras))] + [None]   # (the extras partition what follows the lengthscales)
        return {"lengthscales": g[:cuts[0]], **{name: g[cuts[j]:cuts[j + 1]] for j, name in enumerate(self.row.extras)}}


class DotFamily(NamedTuple):
    name: str
    code: int                          # GPK_DOT_* of include/gpk.h: NOT a GPK_KERN_* code, the stationary builders do not take it
    extras: Tuple[str, ...] = ()       # hyperparameters with a gradient beyond the variance, in the order of the shape gradient

    @property
    def parameters(self) -> Tuple[str, ...]:
        return ("variance",) + self.extras


DOT_FAMILIES = (DotFamily("Linear", 0), DotFamily("Polynomial", 1, ("offset",)))
DOT_BY_NAME = {f.name: f for f in DOT_FAMILIES}
DOT_MAX_DEGREE = 16                    # GPK_DOT_MAX_DEGREE


class DotLeaf(collections.namedtuple("_DotLeafFields", "row variance offset degree")):
    """One dot-product leaf's host values (gpflow/kernels/linears.py), immutable: k = s for "Linear", (s + offset)^degree for
    "Polynomial", s = sum_j variance_j x_j x'_j.  `variance` is 0-d (one weight) or [D] (ARD); `offset` a float; `degree` an int in
    [1, DOT_MAX_DEGREE], a constant of the leaf without a gradient.  Its diagonal K(x, x) depends on the row: it is no row of FAMILIES,
    gpk_kernel_matrix and the fused drivers do not take it -- the gpk_dot_* entry points do (ops.dot_kernel_matrix, ...)."""
    __slots__ = ()
    is_plain = constant_diagonal = False
    builders = ("dot_kernel_matrix", "dot_kernel_matrix_combine", "dot_kernel_diag")

    def __new__(cls, family: str, variance, offset=None, degree=None):
        if family not in DOT_BY_NAME:
            raise ValueError(f"{family!r} is not a dot-product family: {sorted(DOT_BY_NAME)}")
        row = DOT_BY_NAME[family]
        variance = np.asarray(variance, dtype=np.float64)
        if variance.ndim > 1:
            raise ValueError(f"variance of shape {variance.shape}: one weight, or one per active input column")
        if row.name == "Linear":
            if offset is not None or degree is not None:
                raise ValueError("offset and degree belong to the 'Polynomial' family, not to 'Linear'")
            return tuple.__new__(cls, (row, variance, 0.0, 1))
        if offset is None or degree is None:
            raise ValueError("family 'Polynomial' needs offset and degree")
        return tuple.__new__(cls, (row, variance, float(offset), check_degree(degree)))

    @classmethod
    def of(cls, family: str, values, degree=None) -> "DotLeaf":
        """from the values in Parameter order (DotFamily.parameters) and the constant degree"""
        return cls(family, **dict(zip(DOT_BY_NAME[family].parameters, values)), **({} if degree is None else {"degree": degree}))

    def replace(self, values) -> "DotLeaf":
        return DotLeaf.of(self.family, values, degree=self.degree if self.row.extras else None)

    @property
    def family(self) -> str:
        return self.row.name

    @property
    def parameters(self) -> Tuple[str, ...]:
        return self.row.parameters

    @property
    def code(self) -> int:
        return self.row.code

    @property
    def ard(self) -> bool:
        return self.variance.ndim == 1

    @property
    def n_variance(self) -> int:
        """entries of the variance gradient: 1, or D for an ARD variance"""
        return int(self.variance.size) if self.ard else 1

    @property
    def n_shape(self) -> int:
        """entries of the shape gradient: [d/doffset] for the Polynomial, none for Linear"""
        return len(self.row.extras)

    def keywords(self) -> dict:
        """as the `ops.dot_*` builders take a leaf: family=, variance=, and offset= / degree= only where the family has them"""
        return dict(family=self.family, variance=self.variance, **(dict(offset=self.offset, degree=self.degree) if self.row.extras else {}))

    def host(self, d: int):
        """(host array of the weights, ard) of the C-ABI"""
        w = self.variance if self.variance.ndim else self.variance.reshape(1)
        if self.ard and w.size != d:
            raise ValueError(f"variance has {w.size} entries, input dimension is {d}")
        return _lib.host_doubles(w.tolist()), int(self.ard)

    def abi(self, d: int) -> tuple:
        return (self.code, *self.host(d), float(self.offset), int(self.degree))

    def split_shape(self, g) -> dict:
        """a shape gradient as {"lengthscales": empty, "offset": [1]}: no lengthscales, by the static members' convention"""
        return {"lengthscales": g[:0], **{name: g[j:j + 1] for j, name in enumerate(self.row.extras)}}


ARC_ORDERS = (0, 1, 2)
ARC_PARAMETERS = ("variance", "weight_variances", "bias_variance")


def check_order(order) -> int:
    """the ArcCosine's order as an int; ValueError unless it is 0, 1 or 2 (gpflow/kernels/misc.py: `implemented_orders`)"""
    if isinstance(order, bool) or not isinstance(order, (int, float, np.integer, np.floating)) or order not in ARC_ORDERS:
        raise ValueError(f"ArcCosine(order={order!r}): requested kernel order is not implemented, it is one of {ARC_ORDERS}")
    return int(order)


class ArcLeaf(collections.namedtuple("_ArcLeafFields", "order variance weight_variances bias_variance")):
    """One ArcCosine leaf's host values (gpflow/kernels/misc.py), immutable: `order` 0, 1 or 2, a constant of the leaf without a
    gradient; `variance` a float; `weight_variances` 0-d (one weight) or [D] (ARD); `bias_variance` a float.  Its diagonal K(x, x)
    depends on the row and each element needs both row norms and an acos: it is no row of FAMILIES and none of DOT_FAMILIES -- the
    gpk_arccos_* entry points take it (ops.arccos_kernel_matrix, ...)."""
    __slots__ = ()
    is_plain = constant_diagonal = False
    family, parameters, n_variance = "ArcCosine", ARC_PARAMETERS, 1
    builders = ("arccos_kernel_matrix", "arccos_kernel_matrix_combine", "arccos_kernel_diag")

    def __new__(cls, order, variance, weight_variances=1.0, bias_variance=1.0):
        w = np.asarray(weight_variances, dtype=np.float64)
        if w.ndim > 1:
            raise ValueError(f"weight_variances of shape {w.shape}: one weight, or one per active input column")
        return tuple.__new__(cls, (check_order(order), float(variance), w, float(bias_variance)))

    @classmethod
    def of(cls, order, values) -> "ArcLeaf":
        """from the values in Parameter order (ARC_PARAMETERS) and the constant order"""
        return cls(order, **dict(zip(ARC_PARAMETERS, values)))

    def replace(self, values) -> "ArcLeaf":
        return ArcLeaf.of(self.order, values)

    @property
    def ard(self) -> bool:
        return self.weight_variances.ndim == 1

    @property
    def n_weights(self) -> int:
        """entries of the weight gradient: 1, or D for ARD weights"""
        return int(self.weight_variances.size) if self.ard else 1

    @property
    def n_shape(self) -> int:
        """entries of the shape gradient: d/dweight_variances, then d/dbias_variance"""
        return self.n_weights + 1

    def keywords(self) -> dict:
        """as the `ops.arccos_*` builders take a leaf"""
        return dict(order=self.order, variance=self.variance, weight_variances=self.weight_variances, bias_variance=self.bias_variance)

    def host(self, d: int):
        """(host array of the weights, ard) of the C-ABI"""
        w = self.weight_variances if self.weight_variances.ndim else self.weight_variances.reshape(1)
        if self.ard and w.size != d:
            raise ValueError(f"weight_variances has {w.size} entries, input dimension is {d}")
        return _lib.host_doubles(w.tolist()), int(self.ard)

    def abi(self, d: int) -> tuple:
        return (self.order, *self.host(d), self.variance, self.bias_variance)

    def split_shape(self, g) -> dict:
        """a shape gradient as {"lengthscales": empty, "weight_variances": [1 or D], "bias_variance": [1]}"""
        nw = self.n_weights
        return {"lengthscales": g[:0], "weight_variances": g[:nw], "bias_variance": g[nw:nw + 1]}


COREGION_MAX_OUTPUTS = 64             # GPK_COREGION_MAX_OUTPUTS
COREGION_MAX_RANK = 64                # GPK_COREGION_MAX_RANK
COREGION_PARAMETERS = ("kappa", "W")  # in the order of the gradients: the "variance" slot holds d/dkappa, the shape gradient d/dW


def check_coregion_sizes(output_dim, rank) -> tuple:
    """(output_dim, rank) as ints; ValueError unless both are integral, output_dim in 1 ... COREGION_MAX_OUTPUTS and rank in
    1 ... COREGION_MAX_RANK"""
    for name, v, top in (("output_dim", output_dim, COREGION_MAX_OUTPUTS), ("rank", rank, COREGION_MAX_RANK)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= top:
            raise ValueError(f"Coregion({name}={v!r}): an integer in 1 ... {top}")
    return int(output_dim), int(rank)


class CoregionLeaf(collections.namedtuple("_CoregionLeafFields", "W kappa")):
    """One Coregion leaf's host values (gpflow/kernels/misc.py `Coregion`), immutable: `W` [P, R] unconstrained, `kappa` [P] positive;
    B = W W^T + diag(kappa), K(x, y) = B[l(x), l(y)] over ONE column of task labels.  Its diagonal depends on the row; it is no row of
    FAMILIES and none of DOT_FAMILIES -- the gpk_coregion_* entry points take it (ops.coregion_kernel_matrix, ...).  In the gradient
    layout of a KernelSpec the slot called "variance" holds d/dkappa [P] (as the ARD variance of a DotLeaf has D entries) and the shape
    gradient is d/dW flattened row-major [P R]."""
    __slots__ = ()
    is_plain = constant_diagonal = False
    family, parameters = "Coregion", COREGION_PARAMETERS
    builders = ("coregion_kernel_matrix", "coregion_kernel_matrix_combine", "coregion_kernel_diag")

    def __new__(cls, W, kappa):
        W, kappa = np.array(W, dtype=np.float64), np.array(kappa, dtype=np.float64)
        if W.ndim != 2 or kappa.ndim != 1 or kappa.shape[0] != W.shape[0]:
            raise ValueError(f"W of shape {W.shape} and kappa of shape {kappa.shape}: W is [output_dim, rank], kappa [output_dim]")
        check_coregion_sizes(*W.shape)
        W.setflags(write=False)
        kappa.setflags(write=False)
        return tuple.__new__(cls, (W, kappa))

    @classmethod
    def of(cls, values) -> "CoregionLeaf":
        """from the values in gradient order (COREGION_PARAMETERS: kappa, then W)"""
        return cls(**dict(zip(COREGION_PARAMETERS, values)))

    def replace(self, values) -> "CoregionLeaf":
        return CoregionLeaf.of(values)

    @property
    def n_outputs(self) -> int:
        return int(self.W.shape[0])

    @property
    def rank(self) -> int:
        return int(self.W.shape[1])

    @property
    def n_variance(self) -> int:
        """entries of the gradient slot the spec calls "variance": d/dkappa [P]"""
        return self.n_outputs

    @property
    def n_shape(self) -> int:
        """entries of the shape gradient: d/dW flattened row-major"""
        return self.n_outputs * self.rank

    def keywords(self) -> dict:
        """as the `ops.coregion_*` builders take a leaf"""
        return dict(W=self.W, kappa=self.kappa)

    def split_shape(self, g) -> dict:
        """a shape gradient as {"lengthscales": empty, "W": [P R]}"""
        return {"lengthscales": g[:0], "W": g}


def check_degree(degree) -> int:
    """the Polynomial's degree as an int; NotImplementedError unless it is integral and in [1, DOT_MAX_DEGREE]"""
    try:
        ok = isinstance(degree, (int, float, np.integer, np.floating)) and float(degree) == int(degree) and 1 <= int(degree) <= DOT_MAX_DEGREE
    except (ValueError, OverflowError):   # (int(nan), int(inf))
        ok = False
    if not ok:
        raise NotImplementedError(f"Polynomial(degree={degree!r}): an integral degree 1 ... {DOT_MAX_DEGREE}: the power is a product, not pow")
    return int(degree)


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
