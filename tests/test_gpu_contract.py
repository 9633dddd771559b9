"""Contract tests: every `gpflow_amd.ops` primitive that `tests/fake_ops.py` emulates is held, on the device, to the contract
the emulator states -- and both are held to a higher-precision reference of the same operation.

Each case runs the device call and the `fake_ops` call on the same NumPy inputs and checks, for both:
  1. the error against a reference evaluated in np.longdouble (or math.fsum), under a bound derived from the operation
     (u = 2^-53; the bound is written next to each check, not tuned to pass);
  2. regions: what the emulator declares never read is NaN on input, what it declares left alone comes back bitwise;
  3. inputs of non-underscore functions are bitwise unchanged;
  4. a second identical device call is bit-identical (no floating-point atomics in the library);
  5. inputs outside the contract are refused on both sides.
Every case carries a comment naming the boundary or branch it targets; for GEMM_CASES and PROJECT_CASES the branch is pinned, on the
CPU, by tests/test_gpu_gemm_launch.py (test_contract_tables_are_on_their_branches): a row added here gets its pin there.  The rows on
the two sides of a grid clamp, a gridDim-stride loop or a count-selected instantiation are named, per launch, by LAUNCHES in
tests/test_launch_geometry.py, whose CPU guard fails when such a row leaves its table.  The
CPU-tier guard at the end fails when a primitive shared by `fake_ops` and `ops` has no case table here.
"""
import contextlib
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_ops  # noqa: E402

U = 2.0 ** -53
LD = np.longdouble
NAN = float("nan")

# what a case table covers: one entry per primitive shared by fake_ops and ops (the selection rule of
# test_distributed_gloo.py, which swaps exactly these in); plumbing that computes nothing is listed with the reason
NOT_PRIMITIVES = {
    "device": "returns the torch device",
    "to_device": "host-to-device copy (torch)",
    "invd_alloc": "allocates the block-inverse buffer the solves fill",
    "svgp_elbo_workspace": "allocates workspace",
    "svgp_elbo_sep_workspace": "allocates workspace",
}
CASE_TABLES = {}   # primitive name -> the case list that covers it (filled below, next to each table)


def shared_primitives():
    from gpflow_amd import ops
    return sorted(name for name in dir(fake_ops) if not name.startswith("_") and callable(getattr(fake_ops, name))
                  and hasattr(ops, name) and name not in ("torch", "np", "sla"))


@contextlib.contextmanager
def _emulated():
    """gpflow_amd.ops with the shared primitives swapped for fake_ops (test_distributed_gloo.py's rule), restored after."""
    from gpflow_amd import ops
    saved = {name: getattr(ops, name) for name in shared_primitives()}
    try:
        for name in saved:
            setattr(ops, name, getattr(fake_ops, name))
        yield
    finally:
        for name, f in saved.items():
            setattr(ops, name, f)


# ------------------------------------------------------------------------------------------------ helpers
def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _on(x, layout="c", dev="cuda", base=False):
    """NumPy -> fp64 tensor on `dev` in one of the operand layouts the kernels distinguish:
    c: fresh contiguous tensor (a zero-row one has no storage: data_ptr() == 0);
    view0: a zero-row VIEW into live storage (non-null pointer);
    ld: row-major view with an odd leading dimension;
    off: storage starting one element in -- 8-byte but not 16-byte aligned;
    col: a column slice (odd start, ld = cols + 2), as active_dims produces;
    pad: the first cols columns of a wider buffer whose leading dimension is even (the smallest even value >= cols + 2): base and
         every row 16-byte aligned, as in c, but ld != cols;
    bpad / bodd (3-D input only; any other layout of a 3-D input is c): contiguous entries carved from one 1-D buffer at batch stride
         rows * cols + 2 (even) / rows * cols + 1 (odd: every second entry is 8-byte aligned only);
    bld (3-D input only): every entry a row-major view with the odd leading dimension of ld, entries rows * ld apart.
    Padding around a view is NaN, inside the allocation.  base=True: returns (view, allocation), for _outside_view."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 3 and layout == "bld":
        b, r, c = x.shape
        buf = torch.full((b, r, c + 1 if (c + 1) % 2 else c + 2), NAN, dtype=torch.float64, device=dev)
        v = buf[:, :, :c]
        v.copy_(torch.from_numpy(x))
        return (v, buf) if base else v
    if x.ndim == 3 and layout in ("bpad", "bodd"):
        b, r, c = x.shape
        stride = r * c + (2 if layout == "bpad" else 1)
        buf = torch.full((b * stride,), NAN, dtype=torch.float64, device=dev)
        v = torch.as_strided(buf, (b, r, c), (stride, c, 1))
        v.copy_(torch.from_numpy(x))
        return (v, buf) if base else v
    if layout == "c" or x.ndim != 2:
        v = torch.tensor(x, dtype=torch.float64, device=dev)
        return (v, v) if base else v
    r, c = x.shape
    if layout == "view0":
        assert r == 0
        buf = torch.full((2, max(c, 1)), NAN, dtype=torch.float64, device=dev)
        return (buf[:0, :c], buf) if base else buf[:0, :c]
    if layout == "ld":
        ld = c + 1 if (c + 1) % 2 else c + 2
        buf = torch.full((r, ld), NAN, dtype=torch.float64, device=dev)
        v = buf[:, :c]
    elif layout == "pad":
        buf = torch.full((r, c + 2 + c % 2), NAN, dtype=torch.float64, device=dev)
        v = buf[:, :c]
    elif layout == "off":
        buf = torch.full((r * c + 1,), NAN, dtype=torch.float64, device=dev)
        v = buf[1:].view(r, c)
    elif layout == "col":
        buf = torch.full((r, c + 2), NAN, dtype=torch.float64, device=dev)
        v = buf[:, 1:1 + c]
    else:
        raise KeyError(layout)
    v.copy_(torch.from_numpy(x))
    return (v, buf) if base else v


def _outside_view(v, buf):
    """The elements of the allocation `buf` that are not part of its view `v` (from v's offset and strides), as a NumPy array."""
    off = (v.data_ptr() - buf.data_ptr()) // 8 if v.numel() else 0
    idx = np.full((), off, dtype=np.int64)
    for size, stride in zip(v.shape, v.stride()):
        idx = idx[..., None] + np.arange(size, dtype=np.int64) * stride
    inside = np.zeros(buf.numel(), dtype=bool)
    inside[idx.reshape(-1)] = True
    return _np(buf).reshape(-1)[~inside]


def _padding_untouched(v, buf):
    """every element of the allocation outside the view is bitwise the NaN _on filled it with"""
    return bool(np.all(_bits(_outside_view(v, buf)) == _bits(np.array([NAN]))[0]))


def _impls():
    from gpflow_amd import ops
    return (("device", ops, "cuda"), ("fake_ops", fake_ops, "cpu"))


def _within(name, got, ref, bound):
    got, ref, bound = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref)
    bad = ~(err <= bound)
    if bad.any():
        i = int(np.argmax(bad.reshape(-1)))
        b = np.broadcast_to(bound, err.shape).reshape(-1)[i]
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.size} entries over the bound; first at flat index {i}: "
                             f"got {got.reshape(-1)[i]!r} ref {float(ref.reshape(-1)[i])!r} bound {float(b)!r}")


def _check_unchanged(name, tensors, arrays):
    for t, a in zip(tensors, arrays):
        assert _same_bits(_np(t), a), f"{name}: an input was modified"


# ------------------------------------------------------------------------------------------------ GEMM
def _gemm_ref(A, B, C0, alpha, beta, batched):
    A3 = A if A.ndim == 3 else A[None]
    B3 = B if B.ndim == 3 else B[None]
    nb = max(A3.shape[0], B3.shape[0])
    out, bnd = [], []
    for z in range(nb):
        a = A3[z if A3.shape[0] > 1 else 0].astype(LD)
        b = B3[z if B3.shape[0] > 1 else 0].astype(LD)
        k = a.shape[1]
        c0 = (C0[z] if batched else C0).astype(LD)
        c0z = np.where(np.isnan(c0), 0, c0) if beta == 0 else c0
        out.append(alpha * (a @ b.T) + beta * c0z)
        # |C^ - C*| <= 2 (k + 2) u (|alpha| |A| |B|^T + |beta| |C|)
        bnd.append(2 * (k + 2) * U * (abs(alpha) * (np.abs(a) @ np.abs(b).T) + abs(beta) * np.abs(c0z)))
    return (np.stack(out), np.stack(bnd)) if batched else (out[0], bnd[0])


def _tri(rng, rows, cols, kind):
    X = rng.normal(size=(rows, cols))
    return np.triu(X) if kind == 1 else np.tril(X) if kind == 2 else X


# (m, n, k, alpha, beta, b_tri, c_lower, layout, batch) -- batch: 0 plain 2-D, b > 0 batched, -b: A batched, B broadcast
GEMM_CASES = [
    (1, 1, 1, 1.0, 0.0, 0, False, "c", 0),          # sizes 1: one partial tile, generic kernel (K % 16 != 0)
    (0, 5, 16, 1.0, 0.0, 0, False, "c", 0),         # m = 0: nothing to write, null A / C accepted
    (7, 0, 16, 1.0, 0.0, 0, False, "c", 0),         # n = 0: null B / C accepted
    (9, 11, 0, 1.0, 0.0, 0, False, "c", 0),         # k = 0, fresh empty operands (null A / B): C = 0, NaN C not read
    (9, 11, 0, 2.0, -0.5, 0, False, "c", 0),        # k = 0 with beta != 0: C = beta C
    (130, 140, 0, 1.0, 0.0, 0, True, "c", 0),       # k = 0 with c_lower: the tile above the diagonal keeps its sentinel
    # gemm_nt_empty_k_kernel's launch: min(ceil(n / 256), 64) column blocks with a grid-stride loop, at most 65535 rows per launch
    # with a host loop over the first row, blockIdx.z over the batch (tests/test_launch_geometry.py: LAUNCHES)
    (2, 16384, 0, 1.0, 0.0, 0, False, "c", 0),      # k = 0, 64 column blocks, exactly the clamp: no second trip; NaN C not read
    (2, 16385, 0, 2.0, -0.5, 0, False, "ld", 0),    # k = 0, one column past the clamp: thread 0 of block 0 loops; beta C, odd ld
    (65535, 3, 0, 2.0, -0.5, 0, False, "c", 0),     # k = 0, 65535 rows: one launch, grid.y at its limit; beta C
    (65536, 3, 0, 1.0, 0.0, 0, False, "c", 0),      # k = 0, 65536 rows: a second launch of one row (row0 = 65535); NaN C not read
    (9, 300, 0, 2.0, -0.5, 0, False, "c", 3),       # k = 0, batch 3 (3-D operands without a last dimension are accepted): blockIdx.z
    (33, 35, 15, 1.0, 0.0, 0, False, "c", 0),       # K slab - 1: generic kernel
    (33, 35, 16, 1.0, 0.0, 0, False, "c", 0),       # one whole K slab: small latency kernel (kind 1)
    (33, 35, 17, 1.0, 0.0, 0, False, "c", 0),       # K slab + 1: generic kernel, partial slab
    (63, 65, 64, 1.0, 0.0, 0, False, "c", 0),       # wave / 64-tile edges, small kernel
    (64, 129, 256, 1.0, 0.0, 0, False, "c", 0),     # m <= 64, n > 64, K % 16 == 0, K > 128: fast tile (kind 2)
    (65, 64, 144, 1.0, 0.0, 0, False, "c", 0),      # n <= 64 off the fast path: 128 x 64 generic branch
    (200, 257, 17, 1.0, 0.0, 0, False, "c", 0),     # tiles128 < 192, m > 64, K odd: 64 x 128 generic branch
    (700, 700, 144, 1.0, 0.0, 0, False, "c", 0),    # 36 tiles >= 24, K > 128: fast tile (kind 2)
    (129, 255, 1024, 1.0, 0.0, 0, False, "c", 0),   # K >= 1024, few tiles: half-tile long-K branch (64 x 128)
    (127, 128, 129, 0.0, 1.5, 0, False, "c", 0),    # alpha = 0, beta != 0: off fast / small, generic kernel
    (128, 127, 48, 1.3, -0.7, 0, False, "c", 0),    # beta != 0 in the small kernel's (beta / alpha) C prologue
    (256, 257, 160, -1.1, 0.9, 0, False, "c", 0),   # beta != 0, partial column tile; 6 tiles < 24 and m > 64: the 64 x 128 generic tile
    (64, 257, 160, -1.1, 0.9, 0, False, "c", 0),    # m <= 64: beta != 0 in the FAST tile's C preload, partial column tile
    (255, 256, 256, 1.0, 0.0, 1, False, "c", 0),    # b_tri = 1 (B upper): K range from n0 & ~15, B[:, < n0] is NaN
    (257, 300, 300, 1.0, 0.0, 2, False, "c", 0),    # b_tri = 2 (B lower): K range ends at n0 + 128, the rest is NaN
    (300, 300, 64, 1.0, 0.0, 0, True, "c", 0),      # c_lower: tiles above the diagonal keep their sentinel
    (257, 257, 256, 0.5, 0.25, 1, True, "c", 0),    # c_lower with b_tri and beta != 0
    (65, 63, 33, 1.0, 0.0, 0, False, "ld", 0),      # odd leading dimensions: generic kernel
    (129, 130, 64, 1.0, 0.0, 0, False, "off", 0),   # 8- but not 16-byte aligned pointers: off the small path
    (129, 256, 256, 1.0, 0.5, 0, False, "off", 0),  # misaligned, beta != 0, on the 64 x 128 generic tile (4 tiles: generic when aligned too)
    (64, 256, 256, 1.0, 0.5, 0, False, "off", 0),   # m <= 64, misaligned: off the fast path onto the 128 x 128 generic tile, beta != 0
    (100, 70, 48, 1.0, 0.0, 0, False, "col", 0),    # column slices
    (64, 80, 32, 1.0, 0.0, 0, False, "c", 3),       # batch > 1: small kernel over the batch
    (130, 140, 144, 1.0, 0.0, 0, False, "c", 2),    # batch > 1, generic tiles over grid.y
    (64, 96, 32, 1.0, 0.0, 0, False, "c", -3),      # broadcast B (batch stride 0)
]
CASE_TABLES["gemm_nt"] = GEMM_CASES


def _gemm_inputs(case, seed=0):
    m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
    rng = np.random.default_rng(seed + m * 7 + n * 3 + k)
    if batch > 0:
        A, B = rng.normal(size=(batch, m, k)), rng.normal(size=(batch, n, k))
    elif batch < 0:
        A, B = rng.normal(size=(-batch, m, k)), rng.normal(size=(n, k))
    else:
        A, B = rng.normal(size=(m, k)), _tri(rng, n, k, b_tri)
    cshape = (abs(batch), m, n) if batch else (m, n)
    C0 = rng.normal(size=cshape) if beta != 0 else np.full(cshape, NAN)   # beta = 0: C must not be read
    Bdev = B.copy()
    if b_tri and n and k:    # poison the K ranges fake_ops declares never read
        for n0 in range(0, n, 128):
            if b_tri == 1:
                Bdev[n0:n0 + 128, :min(n0 & ~15, k)] = NAN
            else:
                Bdev[n0:n0 + 128, min(n0 + 128, k):] = NAN
    if c_lower:   # tiles strictly above the diagonal: a sentinel that must come back bitwise
        for m0 in range(0, m, 128):
            for n0 in range(0, n, 128):
                if n0 > m0 + 127:
                    C0[..., m0:m0 + 128, n0:n0 + 128] = -777.0
    return A, B, Bdev, C0


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEMM_CASES, ids=[str(c) for c in GEMM_CASES])
def test_gemm_nt_contract(gpu, case):
    m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
    A, B, Bdev, C0 = _gemm_inputs(case)
    ref, bnd = _gemm_ref(A, B, C0, alpha, beta, batch != 0)
    skipped = (C0 == -777.0) if c_lower else np.zeros(C0.shape, dtype=bool)
    for who, impl, dev in _impls():
        lay = layout if batch == 0 else "c"
        tA, tB, (tC, bufC) = _on(A, lay, dev), _on(Bdev, lay, dev), _on(C0, lay, dev, base=True)
        got = _np(impl.gemm_nt(tA, tB, alpha=alpha, beta=beta, C=tC, b_tri=b_tri, c_lower=c_lower))
        _within(f"gemm_nt {who}", np.where(skipped, 0, got), np.where(skipped, 0, ref), np.where(skipped, 0, bnd))
        assert _same_bits(got[skipped], C0[skipped]), f"gemm_nt {who}: a skipped c_lower tile was written"
        if k == 0:   # no product: exact zeros, or the one rounding of beta C -- NumPy's bits
            assert _same_bits(got[~skipped], (beta * C0 if beta != 0 else np.zeros(C0.shape))[~skipped]), f"gemm_nt {who}: k = 0"
        assert _padding_untouched(tC, bufC), f"gemm_nt {who}: wrote outside the view of C"
        _check_unchanged(f"gemm_nt {who}", (tA, tB), (A, Bdev))
        if who == "device":   # determinism: the same call again is bit-identical
            tC2 = _on(C0, lay, dev)
            impl.gemm_nt(tA, tB, alpha=alpha, beta=beta, C=tC2, b_tri=b_tri, c_lower=c_lower)
            assert _same_bits(_np(tC2), got), "gemm_nt: a second call differs"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["c", "view0"])
def test_gemm_nt_zero_k_fresh_result(gpu, layout):
    """k = 0 without C (a rank without rows contracting over them: functions.Linear.backward): exact zeros, from a fresh empty
    operand (null pointer) and from an empty view alike."""
    for who, impl, dev in _impls():
        if layout == "c":
            A, B = _on(np.zeros((3, 0)), "c", dev), _on(np.zeros((2, 0)), "c", dev)
        else:
            A, B = _on(np.zeros((0, 3)), "view0", dev).t(), _on(np.zeros((0, 2)), "view0", dev).t()
        assert _same_bits(_np(impl.gemm_nt(A, B)), np.zeros((3, 2))), who


def test_fake_gemm_k_split_structure():
    """fake_ops refuses a K-split product whose b_tri hint is false of the concatenated B (the device would skip real entries)."""
    rng = np.random.default_rng(3)
    k = 32
    split = lambda X: torch.from_numpy(X).reshape(64, 2, k).permute(1, 0, 2).contiguous()  # noqa: E731
    A = split(np.triu(rng.normal(size=(64, 2 * k))))
    fake_ops.gemm_nt(A, split(np.triu(rng.normal(size=(64, 2 * k)))), b_tri=1, k_split=True)
    with pytest.raises(AssertionError):
        fake_ops.gemm_nt(A, split(rng.normal(size=(64, 2 * k))), b_tri=1, k_split=True)


GEMM_BAD = [
    dict(b_tri=3),                        # b_tri = 3 is not a structure
    dict(a_tri=3),                        # nor is a_tri = 3
]


@pytest.mark.gpu
@pytest.mark.parametrize("kw", GEMM_BAD, ids=str)
def test_gemm_nt_refusals(gpu, kw):
    from gpflow_amd import _lib, ops
    rng = np.random.default_rng(1)
    A, B = rng.normal(size=(32, 32)), rng.normal(size=(32, 32))
    with pytest.raises(_lib.GpkError):
        ops.gemm_nt(_on(A), _on(B), **kw)
    with pytest.raises(AssertionError):
        fake_ops.gemm_nt(_on(A, dev="cpu"), _on(B, dev="cpu"), **kw)
    with pytest.raises(ValueError):     # mismatched inner dimensions, both sides
        ops.gemm_nt(_on(A), _on(B[:, :31]))
    with pytest.raises(AssertionError):
        fake_ops.gemm_nt(_on(A, dev="cpu"), _on(B[:, :31], dev="cpu"))


# ------------------------------------------------------------------------------------------------ kernel matrices
def _kfun(family, r2, variance, op="k"):
    r2 = np.asarray(r2, dtype=LD)
    s3, s5 = np.sqrt(LD(3)), np.sqrt(LD(5))
    if family == "SquaredExponential":
        return variance * np.exp(-r2 / 2)      # (-2 dk/dr2 = k as well)
    if op == "dr2":
        ok = r2 > 1e-36
        r = np.sqrt(np.where(ok, r2, 1))
        f = {"Matern12": lambda: variance * np.exp(-r) / r, "Matern32": lambda: 3 * variance * np.exp(-s3 * r),
             "Matern52": lambda: LD(5) / 3 * variance * (1 + s5 * r) * np.exp(-s5 * r)}[family]()
        return np.where(ok, f, 0)
    r = np.sqrt(np.maximum(r2, LD(1e-36)))
    if family == "Matern12":
        return variance * np.exp(-r)
    if family == "Matern32":
        return variance * (1 + s3 * r) * np.exp(-s3 * r)
    return variance * (1 + s5 * r + LD(5) / 3 * r * r) * np.exp(-s5 * r)


def _kref(family, X1, X2, variance, ls, op="k"):
    """Reference K by the same expansion formula in longdouble, and its bound.  k is monotone in r2, so the interval
    k(r2 -+ delta), delta = (d + 4) u (|a|^2 + |b|^2) (the expansion's rounding plus the scaling by 1 / ls), bounds what a
    correctly evaluated fp64 expansion can give -- |dk/dr2| (d + 3) u (|a|^2 + |b|^2) to first order, and the right thing
    where sqrt(r2) is not differentiable; + 8 u |k| for exp / sqrt / the products (a few ulp each)."""
    d = X1.shape[1]
    lsv = np.broadcast_to(np.asarray(ls, dtype=LD), (d,))
    a, b = X1.astype(LD) / lsv, X2.astype(LD) / lsv
    na, nb = (a * a).sum(1)[:, None], (b * b).sum(1)[None, :]
    r2 = -2 * (a @ b.T) + na + nb
    delta = (d + 4) * U * (na + nb)
    k = _kfun(family, r2, variance, op)
    klo, khi = _kfun(family, np.maximum(r2 - delta, 0), variance, op), _kfun(family, r2 + delta, variance, op)
    bnd = np.maximum(np.abs(klo - k), np.abs(khi - k)) + 8 * U * np.abs(k) + LD(1e-300)
    zero_ok = (r2 - delta <= 1e-36) if op == "dr2" and family != "SquaredExponential" else np.zeros(r2.shape, dtype=bool)
    return k, bnd, zero_ok   # zero_ok: the dr2 clamp may legitimately switch to 0 there


def _kdata(rng, n, d, kind):
    X = rng.normal(size=(n, d))
    if kind == "dup" and n > 1:          # near-duplicate rows: r2 ~ 0, the Matern 1e-36 clamp and the dr2 zero
        X[1::2] = X[0::2][: n // 2] + 1e-9 * rng.normal(size=(n // 2, d))
    if kind == "far":                    # far from the origin: the expansion cancels |a|^2 + |b|^2 - 2 a.b
        X = X + 300.0
    return X


# (family, n1, n2 (None: symmetric), d, ard, data, layout, lower_only, diag_add)
KM_CASES = [
    ("SquaredExponential", 1, 1, 1, False, "normal", "c", False, 0.0),       # sizes 1
    ("SquaredExponential", 0, 5, 2, False, "normal", "c", False, 0.0),       # n1 = 0, fresh empty X1 (null)
    ("Matern12", 5, 0, 2, False, "normal", "c", False, 0.0),                 # n2 = 0, fresh empty X2 (null)
    ("Matern32", 63, 65, 3, True, "normal", "c", False, 0.0),                # tile edges 63 / 65, ARD
    ("Matern52", 127, 129, 16, True, "normal", "ld", False, 0.0),            # tile edges, odd leading dimensions
    ("SquaredExponential", 255, 257, 8, False, "far", "off", False, 0.0),    # offset data, misaligned pointers
    ("Matern12", 64, 64, 2, False, "dup", "c", False, 0.0),                  # near-duplicate rows at the clamp
    ("Matern52", 130, None, 4, False, "dup", "c", False, 0.1),               # symmetric + diag_add, near duplicates
    ("SquaredExponential", 257, None, 5, True, "normal", "c", True, 0.3),    # lower_only: unwritten upper tiles keep their value
    ("Matern32", 100, 70, 64, False, "normal", "col", False, 0.0),           # d = 64 (the maximum), column slices
]
CASE_TABLES["kernel_matrix"] = KM_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", KM_CASES, ids=[str(c) for c in KM_CASES])
def test_kernel_matrix_contract(gpu, case):
    family, n1, n2, d, ard, data, layout, lower_only, diag_add = case
    rng = np.random.default_rng(n1 + 3 * d)
    X1 = _kdata(rng, n1, d, data)
    X2 = None if n2 is None else _kdata(rng, n2, d, data)
    ls = (0.6 + 0.05 * np.arange(d)) if ard else 0.9 * np.sqrt(d)
    k, bnd, _ = _kref(family, X1, X1 if X2 is None else X2, 1.7, ls)
    if X2 is None:
        k = k + diag_add * np.eye(n1, dtype=LD)
        bnd = bnd + U * np.abs(k)
    for who, impl, dev in _impls():
        t1 = _on(X1, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        out = _on(np.full(k.shape, -555.0), "c", dev) if lower_only else None
        K = _np(impl.kernel_matrix(t1, t2, variance=1.7, lengthscales=ls, family=family, diag_add=diag_add,
                                   lower_only=lower_only, out=out))
        if lower_only:   # only the lower triangle is defined; above it: the untouched sentinel / NaN, or a correct value
            low = np.tril(np.ones(k.shape, dtype=bool))
            _within(f"kernel_matrix {who}", np.where(low, K, 0), np.where(low, k, 0), np.where(low, bnd, 0))
            up = ~low & ~np.isnan(K) & (K != -555.0)
            _within(f"kernel_matrix {who} upper", K[up], k[up], bnd[up])
        else:
            _within(f"kernel_matrix {who}", K, k, bnd)
        _check_unchanged(f"kernel_matrix {who}", [t1] + ([t2] if t2 is not None else []), [X1] + ([X2] if X2 is not None else []))


# (op, family, n1, n2 (None: X2 = X1), d, data, layout)
KC_CASES = [
    ("mul", "SquaredExponential", 1, 1, 1, "normal", "c"),     # sizes 1
    ("mul", "Matern32", 0, 4, 2, "normal", "c"),               # zero rows, fresh empty operands
    ("add", "Matern52", 65, 63, 3, "normal", "ld"),            # op add, tile edges, odd ld
    ("add", "Matern12", 129, None, 2, "normal", "c"),          # symmetric: diag_add on the combined diagonal
    ("dr2", "Matern12", 64, 64, 2, "dup", "c"),                # dr2 at near duplicates: the clamp zero
    ("dr2", "Matern52", 130, None, 3, "normal", "off"),        # dr2 symmetric: exact zeros on the diagonal, misaligned
    ("dr2", "SquaredExponential", 257, 255, 8, "far", "col"),  # dr2 = k for SE, far data, column slices
    ("mul", "Matern52", 129, 65, 3, "normal", "c"),            # mul with X2 given: the hadamard entry point as well
]
CASE_TABLES["kernel_matrix_combine"] = KC_CASES
CASE_TABLES["kernel_matrix_hadamard"] = KC_CASES   # (op "mul" with X2 given: checked against the same reference)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KC_CASES, ids=[str(c) for c in KC_CASES])
def test_kernel_matrix_combine_contract(gpu, case):
    op, family, n1, n2, d, data, layout = case
    rng = np.random.default_rng(17 + n1 + d)
    X1 = _kdata(rng, n1, d, data)
    X2 = None if n2 is None else _kdata(rng, n2, d, data)
    G = rng.normal(size=(n1, n1 if n2 is None else n2))
    ls, diag = 0.8 * np.sqrt(d), (0.2 if n2 is None else 0.0)
    k, bnd, zero_ok = _kref(family, X1, X1 if X2 is None else X2, 1.3, ls, "dr2" if op == "dr2" else "k")
    g = G.astype(LD)
    if op == "dr2":
        ref, rb = k * g, bnd * np.abs(g) + U * np.abs(k * g)
        if X2 is None:
            np.fill_diagonal(ref, 0)
            np.fill_diagonal(rb, 0)
    else:
        ref = k * g if op == "mul" else k + g
        rb = (bnd * np.abs(g) if op == "mul" else bnd) + 2 * U * np.abs(ref)
        if X2 is None:
            ref = ref + diag * np.eye(n1, dtype=LD)
            rb = rb + U * np.abs(ref)
    for who, impl, dev in _impls():
        t1, tG = _on(X1, layout, dev), _on(G, layout, dev)
        t2 = None if X2 is None else _on(X2, layout, dev)
        R = _np(impl.kernel_matrix_combine(t1, t2, tG, op=op, variance=1.3, lengthscales=ls, family=family, diag_add=diag))
        if op == "dr2" and X2 is None:
            assert np.all(np.diagonal(R) == 0), f"dr2 {who}: diagonal not exactly zero"
        Rc = np.where(zero_ok & (R == 0), ref.astype(np.float64), R)
        _within(f"kernel_matrix_combine {who}", Rc, ref, rb)
        _check_unchanged(f"kernel_matrix_combine {who}", [t1, tG], [X1, G])
        if op == "mul" and X2 is not None:
            H = _np(impl.kernel_matrix_hadamard(t1, t2, tG, variance=1.3, lengthscales=ls, family=family))
            _within(f"kernel_matrix_hadamard {who}", H, ref, rb)


# ------------------------------------------------------------------------------------------------ Cholesky and solves
def _spd(rng, n, extra=0):
    X = rng.normal(size=(n, 3))
    d2 = ((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)
    K = 1.3 * np.exp(-0.25 * d2) + 0.5 * np.eye(n)
    return K, rng.normal(size=(extra, n))


def _chol_checks(who, T, K, E, n, zero_upper, up_in):
    """normwise backward errors with c = 4:  |K - L L^T|_F <= 4 (n + 1) u |K|_F  and  |E - X L^T|_F <= 4 (n + 1) u |X|_F |L|_F"""
    L = np.tril(T[:n]).astype(LD)
    assert np.linalg.norm((K - L @ L.T).astype(np.float64)) <= 4 * (n + 1) * U * np.linalg.norm(K), f"potrf {who}: |K - LL^T|"
    if E.shape[0]:
        X = T[n:].astype(LD)
        r = np.linalg.norm((E - X @ L.T).astype(np.float64))
        assert r <= 4 * (n + 1) * U * np.linalg.norm(T[n:]) * np.linalg.norm(np.tril(T[:n])), f"potrf {who}: |E - X L^T|"
    up = np.triu(np.ones((n, n), dtype=bool), 1)
    if zero_upper:
        assert np.all(T[:n][up] == 0), f"potrf {who}: zero_upper"
    else:   # the strict upper triangle is left as is (it was NaN: also never read)
        assert _same_bits(T[:n][up], up_in[up]), f"potrf {who}: upper triangle written"


# (n, extra rows, zero_upper, batch)
POTRF_CASES = [
    (1, 0, False, 0),       # size 1
    (15, 3, True, 0),       # K slab - 1
    (16, 1, False, 0),      # K slab
    (17, 0, False, 0),      # K slab + 1
    (64, 65, True, 0),      # wave-wide panel
    (127, 0, False, 0),     # leaf - 1 (single-leaf path)
    (128, 129, False, 0),   # the leaf exactly, extra rows over a tile edge
    (129, 1, True, 0),      # leaf + 1: the first blocked factorisation (internal streams)
    (257, 0, False, 0),     # reduction-block edge, three panels
    (513, 513, True, 0),    # 512-column group + 1, extra-row stream
    (130, 7, False, 3),     # batched (SeparateIndependent), batch stride
    (384, 300, False, 2),   # batched with an extra-row stream (256-column groups)
]
CASE_TABLES["potrf_"] = POTRF_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", POTRF_CASES, ids=[str(c) for c in POTRF_CASES])
def test_potrf_contract(gpu, case):
    n, extra, zero_upper, batch = case
    rng = np.random.default_rng(n + extra)
    probs = [_spd(rng, n, extra) for _ in range(max(batch, 1))]
    Ts = []
    for K, E in probs:
        T = np.vstack([K, E])
        T[:n][np.triu_indices(n, 1)] = NAN     # never read
        Ts.append(T)
    T0 = np.stack(Ts) if batch else Ts[0]
    for who, impl, dev in _impls():
        tT = _on(T0, "c", dev)
        _, info = impl.potrf_(tT, n, zero_upper=zero_upper)
        assert np.all(_np(info) == 0), (who, _np(info))
        got = _np(tT)
        for b, (K, E) in enumerate(probs):
            _chol_checks(who, got[b] if batch else got, K, E, n, zero_upper, (T0[b] if batch else T0)[:n])
        if who == "device":
            tT2 = _on(T0, "c", dev)
            impl.potrf_(tT2, n, zero_upper=zero_upper)
            assert _same_bits(_np(tT2), got), "potrf_: a second call differs"


CASE_TABLES["check_info"] = [(40, 17), (200, 150)]   # (n, bad column): a pivot inside the leaf, one past the first leaf


@pytest.mark.gpu
@pytest.mark.parametrize("n,bad", CASE_TABLES["check_info"])
def test_potrf_info(gpu, n, bad):
    """LAPACK info = j + 1 of the first non-positive pivot on both sides, and check_info raises GpkError on both."""
    from gpflow_amd import _lib
    rng = np.random.default_rng(n)
    K, _ = _spd(rng, n)
    K[bad, bad] = -1.0
    infos = []
    for who, impl, dev in _impls():
        _, info = impl.potrf_(_on(K, "c", dev), n)
        infos.append(int(_np(info)[0]))
        with pytest.raises(_lib.GpkError):
            impl.check_info(info)
    assert infos[0] == infos[1] == bad + 1, infos


# (n, rows of B, layout of B)
SOLVE_CASES = [
    (1, 3, "c"),        # size 1
    (17, 0, "c"),       # zero right-hand sides
    (128, 65, "ld"),    # one diagonal block exactly, odd ldb
    (129, 130, "off"),  # block edge + 1, misaligned B
    (300, 64, "c"),     # three blocks
]
for _name in ("trtri_blocks", "transpose_factor", "trsm_"):
    CASE_TABLES[_name] = SOLVE_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", SOLVE_CASES, ids=[str(c) for c in SOLVE_CASES])
def test_solves_contract(gpu, case):
    """trtri_blocks -> trsm_(trans 0): B L^-T;  transpose_factor -> trsm_(trans 1): B L^-1.  transpose_factor's LT is bitwise
    tril(L)^T (the upper triangle of L is NaN: never read).  |B - X L^T|_F <= 4 (n + 1) u |X|_F |L|_F."""
    n, rows, layout = case
    rng = np.random.default_rng(n + rows)
    K, B = _spd(rng, n, rows)
    L = np.linalg.cholesky(K)
    Lp = L.copy()
    Lp[np.triu_indices(n, 1)] = NAN
    for who, impl, dev in _impls():
        tL = _on(Lp, "c", dev)
        invd = impl.trtri_blocks(tL)
        LT, invdT = impl.transpose_factor(tL, invd)
        assert _same_bits(_np(LT), L.T), f"transpose_factor {who}"
        for trans in (0, 1):
            tB = _on(B, layout, dev)
            impl.trsm_(tB, tL if trans == 0 else LT, invd if trans == 0 else invdT, trans=trans)
            X = _np(tB).astype(LD)
            res = B - (X @ L.T.astype(LD) if trans == 0 else X @ L.astype(LD))
            assert np.linalg.norm(res.astype(np.float64)) <= 4 * (n + 1) * U * np.linalg.norm(_np(tB)) * np.linalg.norm(L), (who, trans)
        _check_unchanged(f"solves {who}", [tL], [Lp])


# ------------------------------------------------------------------------------------------------ exact operations
# (rows, cols, mode, batch, layout)
TRANSPOSE_CASES = [
    (0, 5, 0, 0, "c"),        # zero rows, fresh (null)
    (1, 1, 1, 0, "c"),        # size 1, lower mode
    (31, 33, 0, 0, "ld"),     # 32-wide transpose tile edges, odd ld
    (65, 64, 1, 0, "off"),    # mode 1 keeps the lower triangle; misaligned
    (64, 129, 2, 0, "col"),   # mode 2 keeps the upper triangle; column slice
    (17, 16, 1, 4, "c"),      # batched (q_sqrt [P, m, m] -> LqT)
]
CASE_TABLES["transpose"] = TRANSPOSE_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=[str(c) for c in TRANSPOSE_CASES])
def test_transpose_contract(gpu, case):
    rows, cols, mode, batch, layout = case
    rng = np.random.default_rng(rows + cols)
    X = rng.normal(size=(batch, rows, cols) if batch else (rows, cols))
    if mode:     # the discarded triangle is never read
        keep = np.tril(np.ones((rows, cols), dtype=bool)) if mode == 1 else np.triu(np.ones((rows, cols), dtype=bool))
        Xin, ref = np.where(keep, X, NAN), np.where(keep, X, 0.0)
    else:
        Xin, ref = X, X
    ref = np.swapaxes(ref, -1, -2)
    for who, impl, dev in _impls():
        t = _on(Xin, layout, dev)
        assert _same_bits(_np(impl.transpose(t, mode=mode)), ref), f"transpose {who}"
        _check_unchanged(f"transpose {who}", [t], [Xin])


CASE_TABLES["symmetrize_"] = [(1, "c"), (33, "ld"), (129, "off")]   # size 1; 32-tile edge, odd ld; misaligned


@pytest.mark.gpu
@pytest.mark.parametrize("n,layout", CASE_TABLES["symmetrize_"])
def test_symmetrize_contract(gpu, n, layout):
    """(S + S^T) / 2 is one add and one exact halving: bitwise, and exactly symmetric."""
    S = np.random.default_rng(n).normal(size=(n, n))
    ref = 0.5 * (S + S.T)
    for who, impl, dev in _impls():
        t = _on(S, layout, dev)
        impl.symmetrize_(t)
        assert _same_bits(_np(t), ref), who


CASE_TABLES["diag_add_"] = [(1, 1, "c"), (65, 64, "ld"), (64, 130, "off"), (300, 300, "col")]
# size 1; non-square both ways with odd ld / misaligned; column slice


@pytest.mark.gpu
@pytest.mark.parametrize("r,c,layout", CASE_TABLES["diag_add_"])
def test_diag_add_contract(gpu, r, c, layout):
    """A[i, i] += v[i]: one correctly rounded add per diagonal entry, nothing else touched -- bitwise."""
    rng = np.random.default_rng(r + c)
    A, v = rng.normal(size=(r, c)), rng.normal(size=min(r, c))
    ref = A.copy()
    ref[np.diag_indices(min(r, c))] += v
    for who, impl, dev in _impls():
        t = _on(A, layout, dev)
        impl.diag_add_(t, _on(v, "c", dev))
        assert _same_bits(_np(t), ref), who


# ------------------------------------------------------------------------------------------------ reductions
def _sum_bound(terms, n, per_term_ulps=0):
    """2 (n + 2) u sum|terms|, + a few ulp per term where log / exp enter"""
    s = float(np.abs(np.asarray(terms, dtype=np.float64)).sum()) if np.size(terms) else 0.0
    return (2 * (n + 2) + per_term_ulps) * U * s


# (rows, m, P, layout of At)
ROW_STATS_CASES = [
    (0, 16, 1, "c"),      # zero rows, fresh (null At)
    (0, 16, 2, "view0"),  # zero rows as a view
    (1, 1, 1, "c"),       # sizes 1
    (63, 65, 4, "ld"),    # one chunk of 4 latents exactly; odd ld
    (64, 128, 5, "off"),  # P = 5: a second chunk of 4; misaligned
    (257, 255, 16, "c"),  # P = 16, the fused-driver maximum; reduction-block edge
    (129, 17, 1, "col"),  # column slice
]
CASE_TABLES["row_stats"] = ROW_STATS_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", ROW_STATS_CASES, ids=[str(c) for c in ROW_STATS_CASES])
def test_row_stats_contract(gpu, case):
    rows, m, P, layout = case
    rng = np.random.default_rng(rows + m + P)
    At, V, W = rng.normal(size=(rows, m)), rng.normal(size=(m, P)), rng.normal(size=(m, P))
    a = At.astype(LD)
    ss, mv, wsq = (a * a).sum(1), a @ V.astype(LD), ((a * a) @ (W.astype(LD) ** 2)).T
    bss = 2 * (m + 2) * U * ss
    bmv = 2 * (m + 2) * U * (np.abs(a) @ np.abs(V.astype(LD)))
    bw = 2 * (m + 4) * U * wsq
    for who, impl, dev in _impls():
        tA, tV, tW = _on(At, layout, dev), _on(V, "c", dev), _on(W, "c", dev)
        s, v, w = impl.row_stats(tA, V=tV, W=tW)
        _within(f"row_stats sumsq {who}", _np(s), ss, bss)
        _within(f"row_stats mv {who}", _np(v), mv, bmv)
        _within(f"row_stats wsq {who}", _np(w), wsq, bw)
        _check_unchanged(f"row_stats {who}", [tA, tV, tW], [At, V, W])


CASE_TABLES["row_dot"] = [(0, 3, "c"), (0, 3, "view0"), (1, 1, "c"), (255, 256, "ld"), (257, 513, "off"), (64, 65, "col")]
# zero rows fresh / view; size 1; reduction-block edges with odd ld; misaligned, 512-column edge; column slice


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols,layout", CASE_TABLES["row_dot"])
def test_row_dot_contract(gpu, rows, cols, layout):
    rng = np.random.default_rng(rows * 3 + cols)
    A, B = rng.normal(size=(rows, cols)), rng.normal(size=(rows, cols))
    ref = (A.astype(LD) * B.astype(LD)).sum(1)
    bnd = 2 * (cols + 2) * U * np.abs(A.astype(LD) * B).sum(1)
    for who, impl, dev in _impls():
        tA, tB = _on(A, layout, dev), _on(B, layout, dev)
        r1 = _np(impl.row_dot(tA, tB))
        _within(f"row_dot {who}", r1, ref, bnd)
        _check_unchanged(f"row_dot {who}", [tA, tB], [A, B])
        if who == "device":
            assert _same_bits(_np(impl.row_dot(tA, tB)), r1)


# (rows, cols, upper_only, layout)
SUMSQ_CASES = [
    (0, 4, False, "c"),          # zero rows, fresh
    (1, 1, True, "c"),           # size 1
    (255, 257, True, "ld"),      # reduction-block edges; upper_only
    (1025, 64, False, "off"),    # more rows than MAXPART stage-1 blocks
    (300, 100, False, "col"),    # column slice
]
CASE_TABLES["sumsq"] = SUMSQ_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", SUMSQ_CASES, ids=[str(c) for c in SUMSQ_CASES])
def test_sumsq_contract(gpu, case):
    rows, cols, upper, layout = case
    A = np.random.default_rng(rows + cols).normal(size=(rows, cols))
    terms = (np.triu(A) if upper else A) ** 2
    ref = math.fsum(terms.reshape(-1))
    for who, impl, dev in _impls():
        t = _on(A, layout, dev)
        r = float(_np(impl.sumsq(t, upper_only=upper))[0])
        assert abs(r - ref) <= _sum_bound(terms, terms.size, 2), (who, r, ref)
        _check_unchanged(f"sumsq {who}", [t], [A])
        if who == "device":
            assert float(_np(impl.sumsq(t, upper_only=upper))[0]) == r


CASE_TABLES["sum_log_diag"] = [(1, 0), (129, 0), (257, 3)]   # size 1; tile edge; batched


@pytest.mark.gpu
@pytest.mark.parametrize("n,batch", CASE_TABLES["sum_log_diag"])
def test_sum_log_diag_contract(gpu, n, batch):
    from gpflow_amd import _lib, ops
    rng = np.random.default_rng(n)
    L = rng.normal(size=(max(batch, 1), n, n))
    L[:, np.arange(n), np.arange(n)] = np.exp(rng.normal(size=(max(batch, 1), n)))
    Lin = L if batch else L[0]
    logs = [np.log(np.diagonal(Lb)) for Lb in L]
    for who, impl, dev in _impls():
        r = _np(impl.sum_log_diag(_on(Lin, "c", dev)))
        for b, lg in enumerate(logs):   # summation bound + 2 ulp per log (relative to the log's magnitude, or 1)
            assert abs(r[b] - math.fsum(lg)) <= _sum_bound(lg, n) + 2 * U * np.maximum(np.abs(lg), 1).sum(), (who, b)
    with pytest.raises(_lib.GpkError):   # n = 0 is refused on both sides
        ops.sum_log_diag(_on(np.zeros((0, 0))))
    with pytest.raises(AssertionError):
        fake_ops.sum_log_diag(torch.zeros((0, 0), dtype=torch.float64))


# (rows, P, per-latent s0 / knn, noise per row, layout of Y)
VAREXP_CASES = [
    (0, 1, False, False, "c"),         # zero rows, fresh (null Y / fmean): 0
    (0, 2, True, True, "view0"),       # zero rows as views
    (1, 1, False, False, "c"),         # size 1
    (255, 4, True, False, "ld"),       # reduction-block edge; odd ld of Y
    (257, 5, False, True, "off"),      # P = 5; per-row noise; misaligned Y
    (512, 16, True, True, "col"),      # P = 16 (maximum); column slice
    (270000, 4, False, False, "c"),    # > 1024 x 1024 elements: stage 1 capped at MAXPART blocks
]
CASE_TABLES["gaussian_varexp_sum"] = VAREXP_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", VAREXP_CASES, ids=[str(c) for c in VAREXP_CASES])
def test_gaussian_varexp_sum_contract(gpu, case):
    rows, P, per, het, layout = case
    rng = np.random.default_rng(rows + P)
    Y, F = rng.normal(size=(rows, P)), rng.normal(size=(rows, P))
    s0 = rng.uniform(0, 0.5, size=(P, rows) if per else (rows,))
    ssq = rng.uniform(0, 0.3, size=(P, rows))
    knn = list(1.0 + 0.1 * np.arange(P)) if per else [1.2]
    nv = rng.uniform(0.1, 0.5, size=rows) if het else 0.3
    s0c = (s0.T if per else s0[:, None]).astype(LD)
    fv = np.asarray(knn, dtype=LD)[None, :] - s0c + ssq.T.astype(LD)
    nvl = np.asarray(nv, dtype=LD)[:, None] if het else LD(nv)
    terms = -0.5 * np.log(2 * np.pi * LD(1)) - 0.5 * np.log(nvl) - 0.5 * ((Y.astype(LD) - F - 0.1) ** 2 + fv) / nvl
    terms = np.broadcast_to(terms, (rows, P))
    ref = float(terms.sum())
    bnd = _sum_bound(terms.astype(np.float64), terms.size, 12)
    for who, impl, dev in _impls():
        tY, tF, ts0, tss = _on(Y, layout, dev), _on(F, "c", dev), _on(s0, "c", dev), _on(ssq, "c", dev)
        nvt = _on(nv, "c", dev) if het else nv
        out, fvar = impl.gaussian_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, noise_variance=nvt, mean_const=0.1,
                                             s0_per_latent=per, want_fvar=True)
        r = float(_np(out)[0])
        assert abs(r - ref) <= bnd, (who, r, ref, bnd)
        _within(f"fvar {who}", _np(fvar), fv, 2 * U * (np.abs(fv) + np.abs(s0c) + ssq.T) + LD(1e-300))
        _check_unchanged(f"varexp {who}", [tY, tF, ts0, tss], [Y, F, s0, ssq])
        if who == "device":
            r2 = impl.gaussian_varexp_sum(tY, tF, s0=ts0, ssq=tss, knn=knn, noise_variance=nvt, mean_const=0.1, s0_per_latent=per)[0]
            assert float(_np(r2)[0]) == r, "gaussian_varexp_sum: a second call differs"


@pytest.mark.gpu
def test_gaussian_varexp_sum_refuses_17_latents(gpu):
    """P = 17 is outside the contract (at most 16 latents): refused on both sides."""
    from gpflow_amd import _lib, ops
    Y = np.zeros((3, 17))
    with pytest.raises(_lib.GpkError):
        ops.gaussian_varexp_sum(_on(Y), _on(Y), s0=None, ssq=None, knn=[1.0], noise_variance=0.1)
    with pytest.raises(AssertionError):
        fake_ops.gaussian_varexp_sum(_on(Y, dev="cpu"), _on(Y, dev="cpu"), s0=None, ssq=None, knn=[1.0], noise_variance=0.1)


# (m, P, q_diag)
KL_CASES = [(1, 1, False), (17, 5, True), (129, 4, False), (1100, 1, True), (1100, 1, False)]
# size 1; P = 5 diagonal; a tile edge over 4 latents; more rows than MAXPART stage-1 blocks;
# kl_white_kernel's grid is one block per 1024 elements, clamped to MAXPART = 1024 blocks: a full q_sqrt of 1100 x 1100 asks for 1182
# (the diagonal form counts M P elements: its 1100 rows are two blocks), so the grid-stride loop runs past its usual four trips
CASE_TABLES["gauss_kl_white"] = KL_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("m,P,q_diag", KL_CASES)
def test_gauss_kl_white_contract(gpu, m, P, q_diag):
    rng = np.random.default_rng(m + P)
    q_mu = rng.normal(size=(m, P))
    if q_diag:
        qs = np.exp(0.3 * rng.normal(size=(m, P)))
        terms = np.concatenate([(q_mu ** 2).ravel(), -np.log(qs ** 2).ravel(), (qs ** 2).ravel()])
    else:
        qs = np.tril(0.1 * rng.normal(size=(P, m, m)))
        qs[:, np.arange(m), np.arange(m)] = np.exp(0.3 * rng.normal(size=(P, m)))
        d = np.diagonal(qs, axis1=1, axis2=2)
        terms = np.concatenate([(q_mu ** 2).ravel(), -np.log(d ** 2).ravel(), (qs ** 2).ravel()])
    ref = 0.5 * (math.fsum(terms) - m * P)
    for who, impl, dev in _impls():
        r = float(_np(impl.gauss_kl_white(_on(q_mu, "c", dev), _on(qs, "c", dev)))[0])
        assert abs(r - ref) <= 0.5 * _sum_bound(terms, terms.size, 4) + 4 * U * (abs(ref) + m * P), (who, r, ref)


# (nparts, m, n, alpha, lower, diag_scale, layout)
COMBINE_CASES = [
    (1, 1, 1, 1.0, False, 1.0, "c"),          # sizes 1, one part
    (2, 0, 5, 1.0, False, 1.0, "c"),          # zero rows, fresh
    (1, 65, 63, -0.5, False, 1.0, "ld"),      # tile edges, alpha, odd ld (one part: a 2-D view)
    (4, 130, 130, 1.0, True, 0.5, "c"),       # lower: NaN above the diagonal is never read; Phi's diagonal 0.5
    (5, 257, 300, 2.0, True, 1.0, "c"),       # nparts 5, lower, non-square
    (1, 129, 64, 1.0, True, 0.5, "off"),      # one part, misaligned, lower
    (2, 65537, 3, 1.0, False, 1.0, "c"),      # more than 65535 rows: grid.y capped, the kernel loops over rows
]
# combine_parts_kernel<NP> is picked by the count: 8, 16 (splitk_gemm_nt's 8 chunks) and 32 (the [M, 17] product at K = 8192) have an
# instantiation of their own, 33 takes the run-time loop of NP = 0.  Per count: (130, 66) contiguous -- the 16-byte loads, all NP
# issued before the first add; (65, 63) with an odd leading dimension and part stride -- the element loop inside the same
# instantiation; lower with NaN above the diagonal -- never read, zeros written, Phi's diagonal 0.5
for _np_count in (8, 16, 32, 33):
    COMBINE_CASES += [(_np_count, 130, 66, -0.5, False, 1.0, "c"), (_np_count, 65, 63, 2.0, False, 1.0, "ld"),
                      (_np_count, 130, 130, 1.0, True, 0.5, "c")]
CASE_TABLES["combine_parts"] = COMBINE_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", COMBINE_CASES, ids=[str(c) for c in COMBINE_CASES])
def test_combine_parts_contract(gpu, case):
    npart, m, n, alpha, lower, dscale, layout = case
    rng = np.random.default_rng(npart + m + n)
    parts = rng.normal(size=(npart, m, n))
    pin = parts.copy()
    keep = np.tril(np.ones((m, n), dtype=bool))
    if lower:
        pin[:, ~keep] = NAN
    ref = alpha * parts.astype(LD).sum(0)
    bnd = (npart + 1) * U * abs(alpha) * np.abs(parts).sum(0)
    if lower:
        ref = np.where(keep, ref, 0)
        ref[np.diag_indices(min(m, n))] *= dscale
        bnd = np.where(keep, bnd, 0)
    src = pin if npart > 1 else pin[0]
    for who, impl, dev in _impls():
        tp, buf = _on(src, layout if npart == 1 else {"ld": "bld"}.get(layout, "c"), dev, base=True)
        R = _np(impl.combine_parts(tp, alpha=alpha, lower=lower, diag_scale=dscale))
        _within(f"combine_parts {who}", R, ref, bnd)
        if lower:
            assert np.all(R[~keep] == 0), who
        _check_unchanged(f"combine_parts {who}", [tp], [src])
        assert _padding_untouched(tp, buf), f"combine_parts {who}: wrote outside the view of parts"
        if who == "device":   # determinism: the same call again is bit-identical
            assert _same_bits(_np(impl.combine_parts(tp, alpha=alpha, lower=lower, diag_scale=dscale)), R), "combine_parts: a second call differs"


# ------------------------------------------------------------------------------------------------ projection
# (rows, m, P, batched At, layout of At)
PROJECT_CASES = [
    (0, 16, 1, False, "c"),       # zero rows, fresh
    (1, 16, 1, False, "c"),       # one row
    (40, 128, 2, False, "c"),     # rows <= 64, m % 16 == 0, aligned: fast tile with the squaring epilogue (kind 4 / 5)
    (300, 129, 2, False, "ld"),   # few rows, m odd: 64 x 128 few-rows branch (64-wide tiles would miss a partial slot)
    (257, 128, 4, False, "c"),    # few rows, pairs < 100, whole 64-column slots: the 32 x 64 few-rows branch
    (1300, 512, 1, False, "c"),   # pairs 22 < 100: the 32 x 64 few-rows tile under the snake order (328 tiles on a grid of 512)
    (1300, 512, 5, False, "c"),   # pairs 110 (100 .. 199): the 64 x 64 few-rows branch
    (65, 64, 3, True, "c"),       # batched At [P, rows, m] (SeparateIndependent)
    (129, 96, 2, False, "off"),   # misaligned At on the 32 x 64 few-rows tile (scalar loads)
    (40, 96, 2, False, "off"),    # rows <= 64, misaligned At: off the fast path onto the 128 x 128 generic tile, squaring epilogue
]
CASE_TABLES["project"] = PROJECT_CASES


def _project_inputs(case):
    rows, m, P, batched, layout = case
    rng = np.random.default_rng(rows + m + P)
    At = rng.normal(size=(P, rows, m) if batched else (rows, m))
    Lq = np.tril(rng.normal(size=(P, m, m)))
    return At, Lq, np.ascontiguousarray(np.swapaxes(Lq, 1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("case", PROJECT_CASES, ids=[str(c) for c in PROJECT_CASES])
def test_project_contract(gpu, case):
    """ssq[p, b] = sum_j y_j^2, y = At Lq_p; with e_j = 2 (m + 2) u (|At| |Lq_p|)_j:
    |ssq^ - ssq| <= sum_j (2 |y_j| e_j + e_j^2) + 2 (m + 2) u sum_j y_j^2."""
    rows, m, P, batched, layout = case
    At, Lq, LqT = _project_inputs(case)
    ref, bnd = [], []
    for p in range(P):
        a = (At[p] if batched else At).astype(LD)
        y = a @ Lq[p].astype(LD)
        e = 2 * (m + 2) * U * (np.abs(a) @ np.abs(Lq[p]))
        ref.append((y * y).sum(1))
        bnd.append((2 * np.abs(y) * e + e * e).sum(1) + 2 * (m + 2) * U * (y * y).sum(1))
    ref, bnd = np.stack(ref), np.stack(bnd)
    for who, impl, dev in _impls():
        tA = _on(At, layout, dev)
        r = _np(impl.project(tA, _on(LqT, "c", dev)))
        _within(f"project {who}", r, ref, bnd)
        _check_unchanged(f"project {who}", [tA], [At])


# ------------------------------------------------------------------------------------------------ dispatch coverage
@pytest.mark.gpu
def test_gemm_dispatch_coverage(gpu):
    """The GEMM and projection tables reach every kernel of launch_select: kind 1 gemm_nt_small, kind 2 gemm_nt_fast<0,false>,
    kind 6 gemm_nt_kernel (128 x 64: n <= 64; 64 x 128: the half-tile long-K case and tiles128 < 192; 128 x 128: the 1800-row
    K = 17 product below; the few-rows projection tiles), and the projection's fast tile, kind 4 or 5."""
    import ctypes as C
    from gpflow_amd import _lib, ops
    lib = _lib.load()
    lib.gpk_profile_gemm_enable(1)
    try:
        for case in GEMM_CASES:
            m, n, k, alpha, beta, b_tri, c_lower, layout, batch = case
            A, B, Bdev, C0 = _gemm_inputs(case)
            lay = layout if batch == 0 else "c"
            ops.gemm_nt(_on(A, lay), _on(Bdev, lay), alpha=alpha, beta=beta, C=_on(C0, lay), b_tri=b_tri, c_lower=c_lower)
        rng = np.random.default_rng(0)
        X = _on(rng.normal(size=(1800, 17)))
        ops.gemm_nt(X, X)                       # tiles128 = 225 >= 192, K odd: the 128 x 128 generic tile
        for case in PROJECT_CASES:
            At, _, LqT = _project_inputs(case)
            ops.project(_on(At, case[4]), _on(LqT))
        torch.cuda.synchronize()
        launches = {}
        for kind in range(1, 7):
            ms, cnt, fl = C.c_double(), C.c_long(), C.c_double()
            assert lib.gpk_profile_gemm_collect_kind(kind, 0.0, C.byref(ms), C.byref(cnt), C.byref(fl)) == 0
            launches[kind] = cnt.value
    finally:
        lib.gpk_profile_gemm_enable(0)
        lib.gpk_profile_gemm_collect(None, None, None)   # drops the records
    print("GEMM launches per kind:", launches)
    assert launches[1] > 0 and launches[2] > 0 and launches[6] > 0, launches
    assert launches[4] + launches[5] > 0, launches


# ------------------------------------------------------------------------------------------------ fused drivers
def _svgp_inputs(rng, M, rows, d, P, q_diag):
    Z, X = rng.normal(size=(M, d)), rng.normal(size=(rows, d))
    Y = rng.normal(size=(rows, P))
    q_mu = 0.3 * rng.normal(size=(M, P))
    if q_diag:
        qs = np.exp(0.2 * rng.normal(size=(M, P)))
    else:
        qs = np.tril(0.05 * rng.normal(size=(P, M, M))) + 0.6 * np.eye(M)[None]
    return Z, X, Y, q_mu, qs


def _fused_bound(n, value, scale, cond=1.0):
    """Fused drivers against each other: both are the result of an exactly factored Kuu + dK with |dK|_F <= 4 (n + 1) u |Kuu|_F
    (the potrf bound above), propagated to first order through terms of total size `scale`: the relative change of a solve is
    at most cond times the relative backward error -- cond = kappa(Kuu) where Kuu^-1 enters (un-whitened), kappa(L) =
    sqrt(kappa(Kuu)) where L^-1 does (whitened) -- sqrt(n) for the norm change, times 2 for the two sides; + the summation bound."""
    return 2 * 4 * (n + 1) * U * scale * cond * max(1.0, math.sqrt(n)) + 2 * (n + 2) * U * abs(value)


def _kappa(Z, family, variance, ls, jitter):
    from oracle import gp_oracle as orc
    return float(np.linalg.cond(orc.stationary_K(family, Z, variance=variance, lengthscales=ls) + jitter * np.eye(Z.shape[0])))


# (M, rows, d, P, q_diag, whiten, rows layout)
SVGP_CASES = [
    (16, 0, 2, 1, False, True, "c"),        # zero rows, fresh (null Xb / Yb): [0, KL]
    (16, 0, 2, 2, True, True, "view0"),     # zero rows as views, diagonal q_sqrt
    (17, 1, 3, 1, False, True, "c"),        # one row; M = 17 (slab + 1)
    (129, 257, 3, 5, False, True, "c"),     # whitened full q_sqrt, P = 5; leaf + 1, reduction-block edge
    (64, 130, 2, 4, True, True, "ld"),      # whitened diagonal q_sqrt; odd ld of the rows
    (65, 200, 2, 2, False, False, "c"),     # un-whitened full q_sqrt (the one trapezoid)
    (64, 100, 2, 3, True, False, "off"),    # un-whitened diagonal q_sqrt (identity rows -> Lm^-T); misaligned rows
    (16, 0, 2, 2, False, False, "c"),       # un-whitened, zero rows
    # schedule classes that only tests/test_potrf_schedule.py (CPU, no numbers) saw: the un-whitened full form at sizes where the
    # factorisation runs on its own streams.  d = 8 keeps kappa(Kuu), and with it the derived bound, meaningful.
    (640, 300, 8, 1, False, False, "c"),    # P = 1: the prefilled triangular rows (tril(q_sqrt)^T) skipped across two extra-row groups
    (1152, 1040, 8, 1, False, False, "c"),  # ... across three groups and in the tail zone (shrinking groups at the end)
    (640, 300, 8, 2, False, False, "off"),  # P = 2: the same form without the skip; misaligned rows
    # varexp_kernel<true>, the one-launch tail of the whitened Gaussian shard: min(ceil(rows P / 256), 1024) blocks with a grid-stride
    # loop over the elements; the block that draws the last ticket sums gridDim.x block partials with a loop i += 256
    (16, 65537, 2, 1, False, True, "c"),    # 257 blocks: the ticket holder's loop takes a second trip, of one partial
    (16, 131072, 2, 2, False, True, "c"),   # rows P = 262144, exactly 1024 blocks: one element per thread, four trips of the ticket sum
    (16, 131073, 2, 2, False, True, "c"),   # rows P = 262146: two threads take a second element trip; P = 2, so b = e / P matters
    # kl_unwhite_diag_kernel: min(M, 1024) blocks, the inducing points strided by gridDim.x, a block_sum (shared scratch) per trip
    (1024, 64, 8, 2, True, False, "c"),     # un-whitened diagonal q_sqrt at exactly the clamp: one trip per block
    (1100, 64, 8, 2, True, False, "c"),     # 76 blocks take a second trip and reuse the scratch of block_sum
]
CASE_TABLES["svgp_elbo_shard"] = SVGP_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("case", SVGP_CASES, ids=[str(c) for c in SVGP_CASES])
def test_svgp_elbo_shard_contract(gpu, case):
    M, rows, d, P, q_diag, whiten, layout = case
    rng = np.random.default_rng(M + rows + P)
    Z, X, Y, q_mu, qs = _svgp_inputs(rng, M, rows, d, P, q_diag)
    kw = dict(variance=1.1, lengthscales=0.9, noise_variance=0.2, jitter=1e-6, mean_const=0.05)
    res = {}
    for who, impl, dev in _impls():
        (tX, bX), (tY, bY) = _on(X, layout, dev, base=True), _on(Y, layout, dev, base=True)
        args = (_on(Z, "c", dev), tX, tY, _on(q_mu, "c", dev), _on(qs, "c", dev))
        out, info = impl.svgp_elbo_shard(*args, whiten=whiten, **kw)
        assert int(_np(info)[0]) == 0
        res[who] = _np(out)
        _check_unchanged(f"svgp_elbo_shard {who}", [tX, tY], [X, Y])
        assert _padding_untouched(tX, bX) and _padding_untouched(tY, bY), f"svgp_elbo_shard {who}: wrote outside a view"
        if who == "device":   # determinism: the same call again (a fresh workspace) is bit-identical
            assert _same_bits(_np(impl.svgp_elbo_shard(*args, whiten=whiten, **kw)[0]), res[who]), "svgp_elbo_shard: a second call differs"
    dv, fv = res["device"], res["fake_ops"]
    if rows == 0:
        assert dv[0] == 0.0 and fv[0] == 0.0, (dv, fv)
    kap = _kappa(Z, "SquaredExponential", 1.1, 0.9, 1e-6)
    cond = math.sqrt(kap) if whiten else kap
    bounds = (_fused_bound(M, fv[0], abs(fv[0]) + 10 * rows * P, cond), _fused_bound(M, fv[1], abs(fv[1]) + 10 * M * P, cond))
    if rows:
        print(f"svgp_elbo_shard {case}: |device - fake_ops| / bound = {abs(dv[0] - fv[0]) / bounds[0]:.3e} (out[0]), "
              f"{abs(dv[1] - fv[1]) / bounds[1]:.3e} (out[1]); kappa(Kuu) = {kap:.3e}")
    assert abs(dv[0] - fv[0]) <= bounds[0], (dv, fv)
    assert abs(dv[1] - fv[1]) <= bounds[1], (dv, fv)
    if whiten:   # the whitened KL does not involve Kuu: the reduction bound alone
        kl = float(fake_ops.gauss_kl_white(torch.from_numpy(q_mu), torch.from_numpy(qs))[0])
        assert abs(dv[1] - kl) <= (2 * (M * M * P + 2) + 4) * U * (abs(kl) + M * M * P), (dv[1], kl)


CASE_TABLES["svgp_elbo_shard_sep"] = [(16, 0, 2, "c"), (16, 0, 3, "view0"), (65, 130, 2, "c"), (129, 64, 4, "ld"),
                                      (640, 1040, 2, "c"), (640, 1040, 3, "ld")]
# zero rows fresh / view; leaf edges with P = 2 / 4 and an odd ld
# M = 640 (input dimension SEP_D_LARGE, so that kappa(Kuu) keeps the derived bound meaningful): the batched factorisation on its own
# streams -- two extra-row column groups of 256 and a ragged third (128), each through the fused batched in-group solve (rows >= 1024;
# the driver lays the trapezoids out itself, with an even ld and batch stride whatever the layout of the minibatch rows, so the odd-ld
# row takes that solve too and differs in how Xb / Yb are read); late work (tril(q_sqrt)^T, the KL term) on the rest-update stream
SEP_D_LARGE = 8


@pytest.mark.gpu
@pytest.mark.parametrize("M,rows,P,layout", CASE_TABLES["svgp_elbo_shard_sep"])
def test_svgp_elbo_shard_sep_contract(gpu, M, rows, P, layout):
    rng = np.random.default_rng(M + rows)
    Z, X, Y, q_mu, qs = _svgp_inputs(rng, M, rows, SEP_D_LARGE if M >= 640 else 2, P, False)
    kw = dict(variances=list(1.0 + 0.1 * np.arange(P)), lengthscales=list(0.8 + 0.1 * np.arange(P)),
              families=["SquaredExponential", "Matern32", "Matern52", "Matern12"][:P], noise_variance=0.3, jitter=1e-6)
    res = {}
    for who, impl, dev in _impls():
        out, info = impl.svgp_elbo_shard_sep(_on(Z, "c", dev), _on(X, layout, dev), _on(Y, layout, dev), _on(q_mu, "c", dev),
                                             _on(qs, "c", dev), **kw)
        assert np.all(_np(info) == 0)
        res[who] = _np(out)
    dv, fv = res["device"], res["fake_ops"]
    if rows == 0:
        assert dv[0] == 0.0 and fv[0] == 0.0, (dv, fv)
    cond = max(math.sqrt(_kappa(Z, f, v, l, 1e-6)) for f, v, l in zip(kw["families"], kw["variances"], kw["lengthscales"]))
    assert abs(dv[0] - fv[0]) <= _fused_bound(M, fv[0], abs(fv[0]) + 10 * rows * P, cond), (dv, fv)
    kl = float(fake_ops.gauss_kl_white(torch.from_numpy(q_mu), torch.from_numpy(qs))[0])
    assert abs(dv[1] - kl) <= (2 * (M * M * P + 2) + 4) * U * (abs(kl) + M * M * P), (dv[1], kl)


# (n, P, family, per-row noise)
GPR_CASES = [(1, 1, "SquaredExponential", False), (17, 2, "Matern12", True), (129, 1, "Matern52", False),
             (513, 3, "Matern32", True)]
# size 1; slab + 1 with per-row noise; leaf + 1; 512-column group + 1
CASE_TABLES["gpr_lml"] = GPR_CASES


@pytest.mark.gpu
@pytest.mark.parametrize("n,P,family,het", GPR_CASES)
def test_gpr_lml_contract(gpu, n, P, family, het):
    """|d lml| <= 1/2 |dK|_2 (sum_p |alpha_p|^2 + P tr K^-1) for |dK|_F <= 4 (n + 1) u |K|_F, doubled to cover the fp64
    reference's own error, + the summation bound."""
    from oracle import gp_oracle as orc
    rng = np.random.default_rng(n + P)
    X, Y = rng.normal(size=(n, 2)), rng.normal(size=(n, P))
    nv = rng.uniform(0.1, 0.3, size=n) if het else 0.2
    K = orc.stationary_K(family, X, variance=1.2, lengthscales=0.8) + np.diag(np.broadcast_to(nv, (n,)))
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(K, Y - 0.1)
    ref = float(-0.5 * ((Y - 0.1) * alpha).sum() - 0.5 * n * P * np.log(2 * np.pi) - P * np.log(np.diag(L)).sum())
    dK = 4 * (n + 1) * U * np.linalg.norm(K)
    bnd = 2 * 0.5 * dK * ((alpha ** 2).sum() + P * np.trace(np.linalg.inv(K))) + 2 * (n + 2) * U * (abs(ref) + 2 * n * P)
    for who, impl, dev in _impls():
        out, info = impl.gpr_lml(_on(X, "c", dev), _on(Y, "c", dev), variance=1.2, lengthscales=0.8,
                                 noise_variance=_on(nv, "c", dev) if het else nv, mean_const=0.1, family=family)
        assert int(_np(info)[0]) == 0
        assert abs(float(_np(out)[0]) - ref) <= bnd, (who, float(_np(out)[0]), ref, bnd)


# ------------------------------------------------------------------------------------------------ reverse-pass glue
CASE_TABLES["moment_rows"] = [(0, 2, "c"), (1, 1, "c"), (257, 3, "ld"), (64, 8, "off")]   # zero / one row; odd ld; misaligned


@pytest.mark.gpu
@pytest.mark.parametrize("n2,d,layout", CASE_TABLES["moment_rows"])
def test_moment_rows_contract(gpu, n2, d, layout):
    """[1; B^T; (B^T)^2]: exact except the square (one correctly rounded product) -- bitwise."""
    B = np.random.default_rng(n2 + d).normal(size=(n2, d))
    ref = np.concatenate([np.ones((1, n2)), B.T, B.T * B.T], 0)
    for who, impl, dev in _impls():
        t = _on(B, layout, dev)
        assert _same_bits(_np(impl.moment_rows(t)), ref), who
        _check_unchanged(f"moment_rows {who}", [t], [B])


CASE_TABLES["stationary_adjoint_tail"] = [(1, 1, True), (257, 3, False), (300, 8, True)]   # size 1; block edge; D = 8


@pytest.mark.gpu
@pytest.mark.parametrize("n1,d,sym", CASE_TABLES["stationary_adjoint_tail"])
def test_stationary_adjoint_tail_contract(gpu, n1, d, sym):
    rng = np.random.default_rng(n1 + d)
    R, A, ls = rng.normal(size=(n1, 1 + 2 * d)), rng.normal(size=(n1, d)), 0.5 + rng.uniform(size=d)
    r, a, l = R.astype(LD), A.astype(LD), ls.astype(LD)
    T = r[:, 1:1 + d] - a * r[:, :1]
    if sym:
        Abar = 2 * T / (l * l)
        dls = -(a * Abar).sum(0) / l
    else:
        Abar = T / (l * l)
        dls = (r[:, 1 + d:] - a * (r[:, 1:1 + d] + T)).sum(0) / l ** 3
    dvar = r[:, 0].sum() / LD(1.4)
    mag = np.abs(r[:, 1:1 + d]) + np.abs(a * r[:, :1])       # |T| before cancellation
    for who, impl, dev in _impls():
        sv, sl, Ab = impl.stationary_adjoint_tail(_on(R, "c", dev), _on(A, "c", dev), _on(ls, "c", dev), variance=1.4,
                                                  symmetric=sym)
        _within(f"adjoint Abar {who}", _np(Ab), Abar, 6 * U * mag / (l * l) * (2 if sym else 1))
        _within(f"adjoint dvar {who}", _np(sv), np.array([dvar]), np.array([(2 * (n1 + 2) + 2) * U * np.abs(r[:, 0]).sum() / 1.4]))
        terms = np.abs(a) * (np.abs(r[:, 1 + d:]) + 3 * mag) if not sym else 2 * np.abs(a) * mag
        _within(f"adjoint dls {who}", _np(sl), dls, (2 * (n1 + 2) + 10) * U * terms.sum(0) / (l ** 3) + LD(1e-300))


CASE_TABLES["adam_step_"] = [
    (1, False), (257, True), (5000, False),   # size 1; maximise; several blocks
    # adam_kernel's grid is clamped to 4096 blocks of 256 threads, then a grid-stride loop (q_sqrt at M = 2048 is 4 194 304 elements)
    (1048576, False),      # 4096 x 256, exactly the clamp: every thread one trip
    (1048577, True),       # one element past it: thread 0 of block 0 takes a second trip; maximise
    (2097153 + 257, False),   # every thread a second trip, 258 of them a third; the last block of the last trip partial
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,maxi", CASE_TABLES["adam_step_"])
def test_adam_step_contract(gpu, n, maxi):
    """A handful of correctly rounded operations per element: a few ulp of each term of the longdouble update.  (One flat
    contiguous variable each: the three that are written sit one element inside a NaN-filled allocation, which must stay NaN on
    both sides.)"""
    rng = np.random.default_rng(n)
    p, g, m, v = rng.normal(size=n), rng.normal(size=n), rng.normal(size=n), rng.uniform(0.1, 1, size=n)
    b1, b2, eps, step = 0.9, 0.999, 1e-7, 0.01
    gg = (-g if maxi else g).astype(LD)
    mr = b1 * m.astype(LD) + (1 - LD(b1)) * gg
    vr = b2 * v.astype(LD) + (1 - LD(b2)) * gg * gg
    upd = step * mr / (np.sqrt(vr) + eps)
    pr = p - upd

    def inside(x, dev):   # x as the elements 1 .. n of a NaN-filled allocation of n + 2
        buf = torch.full((n + 2,), NAN, dtype=torch.float64, device=dev)
        buf[1:n + 1].copy_(torch.from_numpy(x))
        return buf[1:n + 1], buf

    for who, impl, dev in _impls():
        def run():
            (tp, bp), (tm, bm), (tv, bv), tg = inside(p, dev), inside(m, dev), inside(v, dev), _on(g, "c", dev)
            impl.adam_step_(tp, tg, tm, tv, beta1=b1, beta2=b2, epsilon=eps, step=step, maximise=maxi)
            for t, b in ((tp, bp), (tm, bm), (tv, bv)):
                assert _padding_untouched(t, b), f"adam {who}: wrote outside the variable"
            _check_unchanged(f"adam {who}", [tg], [g])
            return _np(tp), _np(tm), _np(tv)
        gp, gm, gv = run()
        _within(f"adam m {who}", gm, mr, 4 * U * (np.abs(m) + np.abs(g)))
        _within(f"adam v {who}", gv, vr, 4 * U * (v + g * g))
        _within(f"adam p {who}", gp, pr, 2 * U * np.abs(p) + 8 * U * (np.abs(upd) + step * (np.abs(m) + np.abs(g)) / np.sqrt(vr)))
        if who == "device":   # determinism: the same update again, from the same state, is bit-identical
            assert all(_same_bits(a, b) for a, b in zip(run(), (gp, gm, gv))), "adam: a second call differs"


CASE_TABLES["lowrank_axpy"] = [
    (1, 1, 1, "c"), (65, 130, 16, "ld"), (300, 63, 5, "off"),   # size 1; k = 16 maximum; misaligned
    # lowrank_axpy_kernel's gridDim.y is clamped to 2048, the rows strided by it (8192 rows in the reverse pass of the training step)
    (2048, 130, 16, "c"),     # exactly the clamp: one row per block; aligned, even n: the 16-byte path; k = 16
    (2049, 63, 5, "off"),     # one row past it: blockIdx.y = 0 takes a second trip; odd n, misaligned: the element path; k = 5
    (4097, 66, 16, "c"),      # every blockIdx.y a second trip, the first a third; the 16-byte path in the strided rows
]


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k,layout", CASE_TABLES["lowrank_axpy"])
def test_lowrank_axpy_contract(gpu, m, n, k, layout):
    from gpflow_amd import ops
    rng = np.random.default_rng(m + n + k)
    X, Uu, V = rng.normal(size=(m, n)), rng.normal(size=(m, k)), rng.normal(size=(n, k))
    ref = -0.7 * X.astype(LD) + Uu.astype(LD) @ V.T.astype(LD)
    bnd = 2 * (k + 3) * U * (0.7 * np.abs(X) + np.abs(Uu) @ np.abs(V).T)
    for who, impl, dev in _impls():
        (tX, bX), (tU, bU), (tV, bV) = (_on(x, layout, dev, base=True) for x in (X, Uu, V))
        got = _np(impl.lowrank_axpy(-0.7, tX, tU, tV))
        _within(f"lowrank_axpy {who}", got, ref, bnd)
        _check_unchanged(f"lowrank_axpy {who}", [tX, tU, tV], [X, Uu, V])
        assert all(_padding_untouched(t, b) for t, b in ((tX, bX), (tU, bU), (tV, bV))), f"lowrank_axpy {who}: wrote outside a view"
        if who == "device":   # determinism: the same call again is bit-identical
            assert _same_bits(_np(impl.lowrank_axpy(-0.7, tX, tU, tV)), got), "lowrank_axpy: a second call differs"
    with pytest.raises(ValueError):       # k = 17 is refused on both sides
        ops.lowrank_axpy(1.0, _on(X), _on(np.zeros((m, 17))), _on(np.zeros((n, 17))))
    with pytest.raises(AssertionError):
        fake_ops.lowrank_axpy(1.0, torch.from_numpy(X), torch.zeros((m, 17), dtype=torch.float64), torch.zeros((n, 17), dtype=torch.float64))


# ------------------------------------------------------------------------------------------------ model level: empty shards
@pytest.mark.gpu
@pytest.mark.parametrize("fn", ["Linear", "Polynomial"])
def test_noise_param_grads_zero_rows(gpu, fn):
    """Gaussian(variance=Function) on a rank without rows: the backward contracts over zero rows (gemm_nt with k = 0) and
    returns zero gradients of the parameters' shapes instead of raising before the all-reduce."""
    import gpflow_amd as gpflow
    f = gpflow.functions.Linear(A=np.array([[0.2], [0.1]]), b=np.array([0.5])) if fn == "Linear" \
        else gpflow.functions.Polynomial(2, input_dim=2, w=[0.5, 0.1, 0.0, 0.2, 0.0, 0.0])
    lik = gpflow.likelihoods.Gaussian(variance=f)
    grads = lik.noise_param_grads(np.zeros((0, 2)), torch.zeros(0, dtype=torch.float64, device="cuda"))
    assert len(grads) > 0
    for param, g in grads:
        assert tuple(g.shape) == tuple(np.shape(param.numpy())), (tuple(g.shape), np.shape(param.numpy()))
        assert torch.count_nonzero(g).item() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("whiten", [True, False])
def test_svgp_elbo_terms_zero_rows(gpu, whiten):
    """SVGP.elbo_terms on an empty NumPy shard (a fresh zero-row tensor through ops.to_device) returns [0, KL], equal to the
    emulator's result for the same shard."""
    import gpflow_amd as gpflow
    from gpflow_amd import config
    rng = np.random.default_rng(5)
    Z = rng.normal(size=(20, 2))
    q_mu = 0.2 * rng.normal(size=(20, 1))
    q_sqrt = (np.tril(0.05 * rng.normal(size=(20, 20))) + 0.7 * np.eye(20))[None]
    m = gpflow.models.SVGP(gpflow.kernels.SquaredExponential(lengthscales=0.8), gpflow.likelihoods.Gaussian(0.2), Z, q_mu=q_mu,
                           q_sqrt=q_sqrt, whiten=whiten, num_data=100)
    out = _np(m.elbo_terms((np.zeros((0, 2)), np.zeros((0, 1)))))
    emu, _ = fake_ops.svgp_elbo_shard(torch.from_numpy(Z), torch.zeros((0, 2), dtype=torch.float64),
                                      torch.zeros((0, 1), dtype=torch.float64), torch.from_numpy(q_mu), torch.from_numpy(q_sqrt),
                                      variance=1.0, lengthscales=0.8, noise_variance=0.2, jitter=config.default_jitter(),
                                      whiten=whiten)
    emu = _np(emu)
    assert out[0] == 0.0 and emu[0] == 0.0, (out, emu)
    assert abs(out[1] - emu[1]) <= _fused_bound(20, emu[1], abs(emu[1]) + 200), (out, emu)


@pytest.mark.gpu
def test_sgpr_shard_statistics_zero_rows(gpu):
    """sgpr.shard_statistics over an empty shard matches the emulator: the factor of Kuu and all-zero statistics."""
    from gpflow_amd.models import sgpr
    rng = np.random.default_rng(9)
    Z = rng.normal(size=(12, 2))
    kw = dict(jitter=1e-6, mean_const=0.1, variance=1.1, lengthscales=0.9)
    L, _, packed = sgpr.shard_statistics(_on(Z), _on(np.zeros((0, 2))), _on(np.zeros((0, 1))), **kw)
    with _emulated():
        Le, _, packed_e = sgpr.shard_statistics(_on(Z, dev="cpu"), _on(np.zeros((0, 2)), dev="cpu"),
                                                _on(np.zeros((0, 1)), dev="cpu"), **kw)
    assert _same_bits(_np(packed), _np(packed_e)) and not np.any(_np(packed))
    K = _np(Le) @ _np(Le).T
    _chol_checks("device", _np(L), K, np.zeros((0, 12)), 12, True, None)


# ------------------------------------------------------------------------------------------------ CPU-tier guard
def test_every_shared_primitive_has_a_case_table():
    """A primitive shared by fake_ops and ops without a case table here fails this test: a primitive added later has to
    bring its contract cases (or be listed in NOT_PRIMITIVES with the reason it computes nothing)."""
    shared = shared_primitives()
    missing = [n for n in shared if n not in CASE_TABLES and n not in NOT_PRIMITIVES]
    assert not missing, f"shared primitives without a contract case table: {missing}"
    stale = [n for n in list(CASE_TABLES) + list(NOT_PRIMITIVES) if n not in shared]
    assert not stale, f"case tables for names that are no longer shared primitives: {stale}"
    assert all(len(t) > 0 for t in CASE_TABLES.values())
