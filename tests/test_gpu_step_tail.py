"""The tail of the fused SVGP step: row statistics out of the projection GEMM (gpk_project_stats, GemmArgs::stat_*) and the
one-launch reduction behind it (varexp_kernel<true>: slot partials -> variational expectations -> scalar, last block by ticket).

Which kernel a shape takes (gemm.hip, launch_select / launch_fast), with pairs = ceil(ceil(m / 128) / 2) * ceil(rows / 128) * P:
  rows <= 64, or pairs >= 200     the 128 x 128 fast tile -- the statistics come out of the GEMM (P <= 4);
      pairs > 256                 paired column tiles (the headline's walk), 200 <= pairs <= 256: unpaired "snake" walk;
  everything else                 small generic tiles, or P > 4: the statistics come from gpk_row_stats as before.
The issue's shapes are all here; the three large ones are added because none of the issue's reaches the paired walk.

Bound of test 1, derived and not tuned.  A sum of n terms in ANY order, with or without FMA, has |err| <= (n - 1) u sum |term|
+ O(u^2), u = 2^-53 (Higham, Accuracy and Stability, section 4.2).  For s0 (terms a^2) and fmean (terms a v) the device sum and
the NumPy reference each stay within m u sum |term|, so their difference is within 2 m u sum |term|; the test allows 4.  For
ssq[p, b] = sum_j y_j^2, y_j = sum_k A[b, k] Lq_p[k, j]:  |y_j| <= S_j = sum_k |A[b, k]| |Lq_p[k, j]|, the computed y_j is off by at most
m u S_j, so y_j^2 by 2 m u S_j^2, and the outer sum adds m u sum_j y_j^2 <= m u sum_j S_j^2: 3 m u sum_j S_j^2 per side where the
test allows 4 m u sum_j S_j^2 for the difference -- that is below the worst case of the two sides together, and holds because
rounding errors of random data grow like sqrt(m), not m; test_bound_holds_for_permuted_numpy_sums checks exactly that on the CPU.
"""
import numpy as np
import pytest

from oracle import gp_oracle as orc  # noqa: E402  (test-side checker only)

U = 2.0 ** -53

# (rows, m, P)
ISSUE_SHAPES = [(200, 256, 1),      # partial last row tile, several column tiles
                (384, 512, 4),      # P at the in-kernel limit
                (384, 512, 5),      # gpk_row_stats fallback
                (64, 128, 1),       # at most 64 rows
                (130, 80, 3)]       # K not a multiple of 128; small generic tiles
LARGE_SHAPES = [(16507, 512, 1),    # 258 pairs: the paired walk, one latent (the headline's form), partial last row tile
                (16507, 512, 3),    # paired walk, three batch entries: each forms its own latent's column of fmean
                (3837, 512, 4)]     # 240 pairs: unpaired snake walk on the fast tile, P at the limit


def _t(x):
    from gpflow_amd import ops
    return ops.to_device(x)


_CASES = {}


def _stats_case(rows, m, P):
    """inputs, float64 NumPy references and the per-entry bounds of one shape (computed once, never modified)"""
    key = (rows, m, P)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * P + m + rows)
        A = rng.normal(size=(rows, m))
        Lq = np.stack([np.tril(0.3 * rng.normal(size=(m, m))) + 0.5 * np.eye(m) for _ in range(P)])
        V = rng.normal(size=(m, P))
        aA = np.abs(A)
        ref = dict(s0=(A * A).sum(1), fmean=A @ V, ssq=np.stack([((A @ Lq[p]) ** 2).sum(1) for p in range(P)]))
        bound = dict(s0=4 * m * U * (A * A).sum(1), fmean=4 * m * U * (aA @ np.abs(V)),
                     ssq=np.stack([4 * m * U * ((aA @ np.abs(Lq[p])) ** 2).sum(1) for p in range(P)]))
        for v in list(ref.values()) + list(bound.values()) + [A, Lq, V]:
            v.setflags(write=False)
        _CASES[key] = (A, Lq, V, ref, bound)
    return _CASES[key]


def _check(tag, got, ref, bound):
    for name in ("s0", "fmean", "ssq"):
        err = np.abs(got[name] - ref[name])
        worst = float(np.max(err / bound[name]))
        print(f"{tag} {name}: max |err| / bound = {worst:.3e}")
        assert np.all(err <= bound[name]), f"{tag} {name}: max |err| / bound = {worst:.3e}"


@pytest.mark.parametrize("rows,m,P", ISSUE_SHAPES)
def test_bound_holds_for_permuted_numpy_sums(rows, m, P):
    """CPU: the same three sums taken by NumPy with the K (and, for ssq, the column) index permuted stay inside the bound."""
    A, Lq, V, ref, bound = _stats_case(rows, m, P)
    perm = np.random.default_rng(7).permutation(m)
    Ap = np.ascontiguousarray(A[:, perm])
    got = dict(s0=(Ap * Ap).sum(1), fmean=Ap @ V[perm],
               ssq=np.stack([((Ap @ Lq[p][perm][:, perm[::-1]]) ** 2).sum(1) for p in range(P)]))
    _check(f"numpy permuted ({rows}, {m}, {P})", got, ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("rows,m,P", ISSUE_SHAPES + LARGE_SHAPES)
def test_fused_statistics_against_numpy(gpu, rows, m, P):
    """1. s0, fmean and ssq of the driver-level fused call against float64 NumPy, entry by entry; twice: identical bits."""
    from gpflow_amd import ops
    A, Lq, V, ref, bound = _stats_case(rows, m, P)
    tA, tL, tV = _t(A), _t(np.ascontiguousarray(np.transpose(Lq, (0, 2, 1)))), _t(V)
    s0, fmean, ssq = ops.project_stats(tA, tL, tV)
    got = dict(s0=s0.cpu().numpy(), fmean=fmean.cpu().numpy(), ssq=ssq.cpu().numpy())
    _check(f"({rows}, {m}, {P})", got, ref, bound)
    again = ops.project_stats(tA, tL, tV)
    for name, t in zip(("s0", "fmean", "ssq"), again):
        assert np.array_equal(t.cpu().numpy().view(np.int64), got[name].view(np.int64)), f"{name}: two calls differ"
    # the projection alone is the same GEMM with or without the statistics riding along
    assert np.array_equal(ops.project(tA, tL).cpu().numpy().view(np.int64), got["ssq"].view(np.int64))


# shapes of test_shard_against_oracle that take one noise variance per row (varexp_kernel's noise_rows branch) instead of a constant
PER_ROW_NOISE = {(16, 65537, 2, 1)}


def _shard_inputs(m, rows, d, P, seed=13):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(rows, d))
    Y = np.sin(X.sum(1, keepdims=True)) + 0.1 * rng.normal(size=(rows, P))
    Z = rng.normal(size=(m, d))
    q_mu = 0.1 * rng.normal(size=(m, P))
    q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(m, m))) + 0.5 * np.eye(m) for _ in range(P)])
    kw = dict(variance=1.1, lengthscales=np.sqrt(d) * (0.8 + 0.05 * np.arange(d)), noise_variance=0.1)
    return X, Y, Z, q_mu, q_sqrt, kw


def _shard(X, Y, Z, q_mu, q_sqrt, kw, ws=None):
    from gpflow_amd import ops
    out, info = ops.svgp_elbo_shard(_t(Z), _t(X), _t(Y), _t(q_mu), _t(q_sqrt), jitter=1e-6, ws=ws, **kw)
    return out.cpu().numpy(), info.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("m,rows,d,P", [(256, 300, 3, 1), (256, 300, 3, 2),   # side schedule, one-launch tail
                                        (256, 200, 3, 1),                      # the extra rows ride through the panels
                                        (256, 64, 3, 1),                       # statistics out of the GEMM (unpaired fast tile)
                                        (512, 16507, 3, 1),                    # side schedule AND the paired walk with statistics
                                        (16, 65537, 2, 1)])                    # 257 tail blocks (PER_ROW_NOISE): the ticket sum's second trip
def test_shard_against_oracle(gpu, m, rows, d, P):
    """2. Both terms of the whitened shard against the oracle at rtol = 1e-9, the tolerance of the model-level ELBO comparisons
    (tests/test_gpu_models.py:284; the shard tests of tests/test_gpu_primitives.py:425 use the same for out[0])."""
    X, Y, Z, q_mu, q_sqrt, kw = _shard_inputs(m, rows, d, P)
    if (m, rows, d, P) in PER_ROW_NOISE:
        kw["noise_variance"] = np.random.default_rng(rows).uniform(0.05, 0.2, size=rows)
    out, info = _shard(X, Y, Z, q_mu, q_sqrt, kw)
    assert np.all(info == 0), info
    s_ref, kl_ref = orc.svgp_elbo_terms(X, Y, Z, q_mu, q_sqrt, whiten=True, **kw)
    print(f"({m}, {rows}, {d}, {P}): rel err out[0] {abs(out[0] - s_ref) / abs(s_ref):.3e}, out[1] {abs(out[1] - kl_ref) / abs(kl_ref):.3e}")
    np.testing.assert_allclose(out[0], s_ref, rtol=1e-9)
    np.testing.assert_allclose(out[1], kl_ref, rtol=1e-9)
    np.testing.assert_allclose(out[0] - out[1], orc.svgp_elbo(X, Y, Z, q_mu, q_sqrt, **kw), rtol=1e-9)


@pytest.mark.gpu
@pytest.mark.parametrize("q_diag", [False, True], ids=["full", "qdiag"])
def test_ticket_and_workspace_reuse(gpu, q_diag):
    """3. One workspace from torch.empty, filled with 0xFF bytes (the ticket word starts at -1, not 0): three calls in a row,
    then a smaller shape carved from the same buffer.  Each result equals a call on a fresh workspace bit for bit."""
    import torch
    from gpflow_amd import ops
    big = _shard_inputs(256, 300, 3, 2)
    small = _shard_inputs(192, 150, 3, 2, seed=14)
    if q_diag:
        big = big[:4] + (np.abs(big[3]) + 0.3,) + big[5:]
        small = small[:4] + (np.abs(small[3]) + 0.3,) + small[5:]
    nbytes = int(ops._lib.load().gpk_svgp_elbo_workspace_bytes(256, 300, 3, 2, int(q_diag), 1))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=ops.device())
    ws.view(torch.uint8).fill_(0xFF)
    fresh_big = _shard(*big, ws=torch.zeros_like(ws))
    fresh_small = _shard(*small, ws=torch.zeros_like(ws))
    assert np.all(np.isfinite(fresh_big[0])) and np.all(fresh_big[1] == 0)
    runs = [_shard(*big, ws=ws) for _ in range(3)]
    for i, (out, info) in enumerate(runs):
        assert np.all(info == 0)
        assert np.array_equal(out.view(np.int64), fresh_big[0].view(np.int64)), f"call {i} on the reused workspace: {out!r} vs {fresh_big[0]!r}"
    out, info = _shard(*small, ws=ws)
    assert np.all(info == 0)
    assert np.array_equal(out.view(np.int64), fresh_small[0].view(np.int64)), f"smaller shape on the reused workspace: {out!r} vs {fresh_small[0]!r}"


@pytest.mark.gpu
def test_ticket_and_workspace_reuse_past_the_block_clamp(gpu):
    """3b. The same at rows P = 262146 (tests/test_gpu_contract.py: SVGP_CASES), where the tail's grid is clamped to 1024 blocks and
    its elements are strided: the ticket stands at 1024 after a call, and kl_white_kernel of the next call must zero it -- else no
    block draws the last ticket and out[0] is never written.  The workspace starts with 0xFF bytes; out is NaN before every call;
    each result equals the call on a fresh workspace bit for bit."""
    import torch
    from gpflow_amd import ops
    m, rows, d, P = 16, 131073, 2, 2
    X, Y, Z, q_mu, q_sqrt, kw = _shard_inputs(m, rows, d, P)
    tensors = [_t(x) for x in (Z, X, Y, q_mu, q_sqrt)]
    nbytes = int(ops._lib.load().gpk_svgp_elbo_workspace_bytes(m, rows, d, P, 0, 1))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=ops.device())
    ws.view(torch.uint8).fill_(0xFF)

    def call(w):
        out = torch.full((2,), float("nan"), dtype=torch.float64, device=ops.device())
        _, info = ops.svgp_elbo_shard(*tensors, jitter=1e-6, ws=w, out=out, **kw)
        assert np.all(info.cpu().numpy() == 0)
        return out.cpu().numpy()
    fresh = call(torch.zeros_like(ws))
    assert np.all(np.isfinite(fresh)), fresh
    for i in range(2):
        out = call(ws)
        assert np.array_equal(out.view(np.int64), fresh.view(np.int64)), f"call {i} on the reused workspace: {out!r} vs {fresh!r}"


@pytest.mark.gpu
@pytest.mark.parametrize("m,rows", [(256, 300), (256, 64)], ids=["row_stats_kernel", "stats_in_gemm"])
def test_nonfinite_rows(gpu, m, rows):
    """4. A NaN in one row of Xb -- an inner row, the last row, a row of the last partial 128-row tile: out[0] is NaN, the
    whitened KL keeps its bits and info stays 0 (the rule of tests/test_gpu_nonfinite.py for this driver)."""
    X, Y, Z, q_mu, q_sqrt, kw = _shard_inputs(m, rows, 3, 1)
    clean, info0 = _shard(X, Y, Z, q_mu, q_sqrt, kw)
    assert np.all(np.isfinite(clean)) and np.all(info0 == 0)
    for r in sorted({7, rows - 1, (rows - 1) // 128 * 128 + 3}):
        Xn = X.copy()
        Xn[r, 1] = np.nan
        out, info = _shard(Xn, Y, Z, q_mu, q_sqrt, kw)
        assert np.isnan(out[0]), f"NaN in row {r} was swallowed: {out!r}"
        assert out[1:].view(np.int64) == clean[1:].view(np.int64), (r, out, clean)
        assert np.all(info == 0), (r, info)
