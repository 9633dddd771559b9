"""GPU tests of the LinearCoregionalization feature: the mixing kernel behind `ops.mixed_gaussian_varexp_sum`, the fused shard
`ops.svgp_elbo_shard_lcm`, `kernels.LinearCoregionalization`, `conditionals.mix_latent_gp`, `LinearCoregionalizationPosterior`,
`SVGP.elbo` / `predict_f` and the reverse pass `SVGP.elbo_and_grad` of the model.

The same bodies run in the CPU tier against the NumPy emulation (tests/test_lcm_emulated.py imports them without this module's
`gpu` mark and gives them an emulated `gp` fixture: tests/emulation.py, with tests/fake_lcm_ops.py for the primitives here).

References.  The primitive: its contract (include/gpk.h) restated in np.longdouble (`_mixed_reference`), every bound derived next
to its check with u = 2^-53.  The fused shard: the emulation, within test_gpu_contract._fused_bound.  The model: per-latent
oracle/gp_oracle.py (`svgp_predict_f`, `gauss_kl`) mixed in NumPy.  Gradients: a torch-CPU fp64 autograd restatement of the same
ELBO (`_torch_elbo_lcm`).
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle as orc  # noqa: E402  (checker only)
from oracle import gp_oracle_grad as orcg  # noqa: E402  (checker only)
import fake_lcm_ops  # noqa: E402
import fake_ops  # noqa: E402
from test_gpu_contract import LD, U, _bits, _fused_bound, _kappa, _np, _on, _sum_bound, _svgp_inputs, _within  # noqa: E402
from test_gpu_likelihoods import _refused  # noqa: E402

LOG2PI = np.log(2 * np.pi * LD(1))


@pytest.fixture(scope="module")
def gp(gpu):
    import gpflow_amd
    return gpflow_amd


def _dev(gp):
    """where `gp.ops` keeps its tensors: the HIP device, or the CPU under the emulation"""
    return str(gp.ops.device())


# ------------------------------------------------------------------------------------------------ 1. the primitive
def _mixed_reference(Y, gm, W, s0, ssq, knn, s2, c, s0_per):
    """include/gpk.h, gpk_mixed_gaussian_varexp_sum, in longdouble, and bounds on the fp64 error of every output (first order in u;
    the inputs are fp64 numbers, so the operands themselves are exact):
      gvar = knn - s0 + ssq, two roundings:              egv = 3 u (|knn| + |s0| + |ssq|)
      f = sum_l W_pl gm_bl + c: an L-term dot of exact operands plus one addition:
                                                         ef = (L + 3) u (sum_l |W_pl gm_bl| + |c|)
      fvar = sum_l W_pl^2 gvar_bl: the square, the product and the L-term sum, and the operand error through W^2:
                                                         efv = (L + 3) u sum_l |W_pl^2 gvar_bl| + sum_l W_pl^2 egv_bl
      dy = Y - f:                                        edy = ef + u (|Y| + |f|)
      dgmu = (sum_p W_pl dy_bp) / s2: a P-term dot, the division, the operand error through |W|:
                                                         (P + 5) u sum_p |W_pl dy_bp| / s2 + sum_p |W_pl| edy_bp / s2
      q = dy^2 + fvar:                                   eq = 2 |dy| edy + efv + 3 u (dy^2 + |fvar|)
      VE = c0 - q / (2 s2), c0 with a log at 3 ulp:      eve = eq / (2 s2) + 8 u (|c0| + |q| / (2 s2))
      d/ds2 = -1 / (2 s2) + q / (2 s2^2):                ed2 = eq / (2 s2^2) + 8 u (1 / (2 s2) + |q| / (2 s2^2))
      out[0], out[1]: the terms' errors and the summation of n = rows P terms -- two stages of pairwise-and-sequential partial sums,
        never worse than the sequential 2 (n + 2) u sum |term| that test_gaussian_varexp_sum_contract allows (_sum_bound)
      dW = (sum_b dy_bp gm_bl - W_pl gvar_bl) / s2: per row  |gm| edy + |W| egv + 3 u (|dy gm| + |W gvar|), the sum over the rows
        2 (rows + 2) u sum_b (|dy gm| + |W gvar|), the division 2 u |dW|."""
    rows, L = gm.shape
    P = W.shape[0]
    Yl, gml, Wl = Y.astype(LD), gm.astype(LD), W.astype(LD)
    knn_l = np.broadcast_to(np.atleast_1d(np.asarray(knn, dtype=LD)), (L,))
    gv = np.tile(knn_l[None, :], (rows, 1))
    mag = np.abs(gv)
    if s0 is not None:
        s0c = (s0.T if s0_per else s0[:, None]).astype(LD)
        gv, mag = gv - s0c, mag + np.abs(s0c)
    if ssq is not None:
        gv, mag = gv + ssq.T.astype(LD), mag + np.abs(ssq.T.astype(LD))
    egv = 3 * U * mag
    s2, c = LD(s2), LD(c)
    f, af = np.zeros((rows, P), dtype=LD), np.zeros((rows, P), dtype=LD)
    fv, afv, pfv = (np.zeros((rows, P), dtype=LD) for _ in range(3))
    for l in range(L):
        t = Wl[None, :, l] * gml[:, l:l + 1]
        f, af = f + t, af + np.abs(t)
        t = Wl[None, :, l] ** 2 * gv[:, l:l + 1]
        fv, afv, pfv = fv + t, afv + np.abs(t), pfv + Wl[None, :, l] ** 2 * egv[:, l:l + 1]
    f = f + c
    ef = (L + 3) * U * (af + abs(c))
    efv = (L + 3) * U * afv + pfv
    dy = Yl - f
    edy = ef + U * (np.abs(Yl) + np.abs(f))
    dg, adg, pdg = (np.zeros((rows, L), dtype=LD) for _ in range(3))
    for p in range(P):
        t = Wl[None, p, :] * dy[:, p:p + 1]
        dg, adg, pdg = dg + t, adg + np.abs(t), pdg + np.abs(Wl[None, p, :]) * edy[:, p:p + 1]
    dg = dg / s2
    edg = ((P + 5) * U * adg + pdg) / s2
    q = dy * dy + fv
    eq = 2 * np.abs(dy) * edy + efv + 3 * U * (dy * dy + np.abs(fv))
    c0 = -LOG2PI / 2 - np.log(s2) / 2
    ve = c0 - q / (2 * s2)
    eve = eq / (2 * s2) + 8 * U * (abs(c0) + np.abs(q) / (2 * s2))
    d2 = -1 / (2 * s2) + q / (2 * s2 * s2)
    ed2 = eq / (2 * s2 * s2) + 8 * U * (1 / (2 * s2) + np.abs(q) / (2 * s2 * s2))
    n = rows * P
    out = np.array([ve.sum(), d2.sum()], dtype=LD) if rows else np.zeros(2, dtype=LD)
    eout = np.array([float(eve.sum()) + _sum_bound(ve.astype(np.float64), n), float(ed2.sum()) + _sum_bound(d2.astype(np.float64), n)])
    dW, edW = np.zeros((P, L), dtype=LD), np.zeros((P, L), dtype=LD)
    for l in range(L):
        a, b_ = dy * gml[:, l:l + 1], Wl[None, :, l] * gv[:, l:l + 1]                       # [rows, P]
        m_ = np.abs(a) + np.abs(b_)
        dW[:, l] = (a - b_).sum(0)
        edW[:, l] = (np.abs(gml[:, l:l + 1]) * edy + np.abs(Wl[None, :, l]) * egv[:, l:l + 1] + 3 * U * m_).sum(0) \
            + 2 * (rows + 2) * U * m_.sum(0)
    dW = dW / s2
    edW = edW / s2 + 2 * U * np.abs(dW)
    return dict(out=out, eout=eout, f=f, ef=ef + LD(1e-300), fv=fv, efv=efv + LD(1e-300), dg=dg, edg=edg + LD(1e-300), dW=dW,
                edW=edW + LD(1e-300), gv=gv, ve_terms=ve)


# (rows, L, P, s0: "per" latent | "shared" | None, ssq given, knn per latent, layout of Y)
MIXED_CASES = [
    (0, 2, 3, "per", True, True, "c"),          # zero rows: out = [0, 0], dW = 0
    (1, 1, 1, "shared", True, False, "c"),      # one row, one latent, one output
    (5, 16, 16, "per", True, True, "ld"),       # the widest group: four rows per wave pass, the last pass one row
    (67, 3, 5, "shared", True, True, "ld"),     # L < P: 12 rows per pass and four idle lanes; rows no multiple of 12; Y with ld > P
    (67, 5, 2, None, False, False, "c"),        # L > P; s0 and ssq NULL; one knn
    (67, 3, 5, "per", False, True, "c"),        # ssq NULL alone
    (300, 16, 1, "per", True, False, "c"),      # one output reads 16 latents; 75 passes = 19 blocks
    # the launcher gives a block four wave passes and at most 1024 blocks: with 16 lanes per row a pass is four rows, so from
    # 4 * 4 * 1024 = 16384 rows on the grid-stride loop runs a second time -- here for the last two passes
    (16391, 16, 16, "per", True, True, "c"),
]


def _mixed_inputs(case):
    rows, L, P, s0m, has_ssq, per_knn, _ = case
    rng = np.random.default_rng(1000 * rows + 16 * L + P)
    Y, gm = rng.normal(size=(rows, P)), rng.normal(size=(rows, L))
    W = rng.normal(size=(P, L)) / math.sqrt(L)
    s0 = None if s0m is None else rng.uniform(0, 0.5, size=(L, rows) if s0m == "per" else (rows,))
    ssq = rng.uniform(0, 0.3, size=(L, rows)) if has_ssq else None
    knn = list(1.0 + 0.1 * np.arange(L)) if per_knn else [1.2]
    return Y, gm, W, s0, ssq, knn


@pytest.mark.parametrize("case", MIXED_CASES, ids=[str(c) for c in MIXED_CASES])
def test_mixed_gaussian_varexp_sum_contract(gp, case):
    ops, dev = gp.ops, _dev(gp)
    rows, L, P, s0m, _, _, layout = case
    Y, gm, W, s0, ssq, knn = _mixed_inputs(case)
    ref = _mixed_reference(Y, gm, W, s0, ssq, knn, 0.3, 0.1, s0m == "per")
    tY, tg = _on(Y, layout, dev), _on(gm, "c", dev)
    ts0, tss = (None if s0 is None else _on(s0, "c", dev)), (None if ssq is None else _on(ssq, "c", dev))
    kw = dict(s0=ts0, ssq=tss, knn=knn, noise_variance=0.3, mean_const=0.1, s0_per_latent=s0m == "per")
    out, fm, fv, dg, dW = ops.mixed_gaussian_varexp_sum(tY, tg, W, want_moments=True, want_grads=True, **kw)
    o = _np(out)
    print("mixed", case, "out", o, "ref", ref["out"].astype(np.float64), "bound", ref["eout"])
    for i in range(2):
        assert abs(LD(o[i]) - ref["out"][i]) <= ref["eout"][i], (i, o, ref["out"], ref["eout"])
    _within("fmean", _np(fm), ref["f"], ref["ef"])
    _within("fvar", _np(fv), ref["fv"], ref["efv"])
    _within("dgmu", _np(dg), ref["dg"], ref["edg"])
    _within("dW", _np(dW), ref["dW"], ref["edW"])
    if rows == 0:
        assert o[0] == 0.0 and o[1] == 0.0 and np.all(_np(dW) == 0.0)
    assert np.array_equal(_bits(_np(tY)), _bits(Y)) and np.array_equal(_bits(_np(tg)), _bits(gm)), "an input was modified"
    # a second call gives the same bits; so does a call without the optional outputs
    again = ops.mixed_gaussian_varexp_sum(tY, tg, W, want_moments=True, want_grads=True, **kw)
    for a, b_ in zip((out, fm, fv, dg, dW), again):
        assert np.array_equal(_bits(_np(a)), _bits(_np(b_))), "a second call differs"
    bare = ops.mixed_gaussian_varexp_sum(tY, tg, W, **kw)
    assert all(t is None for t in bare[1:]) and np.array_equal(_bits(_np(bare[0])), _bits(o))
    half = ops.mixed_gaussian_varexp_sum(tY, tg, W, want_grads=True, **kw)
    assert half[1] is None and np.array_equal(_bits(_np(half[4])), _bits(_np(dW)))


@pytest.mark.parametrize("rows,P", [(67, 5), (300, 16)])
def test_mixed_stage_with_identity_weights_is_the_gaussian_stage(gp, rows, P):
    """W = I, L = P: out[0] against ops.gaussian_varexp_sum on the same moments, within the two stages' bounds added (this stage's
    from _mixed_reference, the other's from test_gaussian_varexp_sum_contract: _sum_bound(terms, n, 12)).  mean_const = 0.1 on both
    sides: after an identity mixing it is where the Gaussian stage adds it."""
    ops, dev = gp.ops, _dev(gp)
    Y, gm, _, s0, ssq, knn = _mixed_inputs((rows, P, P, "per", True, True, "c"))
    ref = _mixed_reference(Y, gm, np.eye(P), s0, ssq, knn, 0.3, 0.1, True)
    tY, tg, ts0, tss = (_on(a, "c", dev) for a in (Y, gm, s0, ssq))
    mixed = ops.mixed_gaussian_varexp_sum(tY, tg, np.eye(P), s0=ts0, ssq=tss, knn=knn, noise_variance=0.3, mean_const=0.1,
                                          s0_per_latent=True)[0]
    plain = ops.gaussian_varexp_sum(tY, tg, s0=ts0, ssq=tss, knn=knn, noise_variance=0.3, mean_const=0.1, s0_per_latent=True)[0]
    bound = ref["eout"][0] + _sum_bound(ref["ve_terms"].astype(np.float64), rows * P, 12)
    assert abs(float(_np(mixed)[0]) - float(_np(plain)[0])) <= bound, (_np(mixed), _np(plain), bound)


# ------------------------------------------------------------------------------------------------ 2. refusals, non-finite inputs
def test_mixed_stage_refusals(gp):
    """L = 17, P = 0, noise_variance = 0 (and NaN) and a short workspace: the library's codes, with `out` untouched; nothing is
    launched by a refused call, so the same body runs on host buffers under the emulation.  Then the same through the wrappers."""
    from gpflow_amd import _lib
    ops, dev = gp.ops, _dev(gp)
    lib = _lib.load()
    rows = 3
    buf = lambda *shape, fill=0.0: torch.full(shape, fill, dtype=torch.float64, device=dev)   # noqa: E731
    Y, gm, out = buf(rows, 16), buf(rows, 16), buf(2, fill=7.0)
    nws = int(lib.gpk_mixed_varexp_workspace_bytes(rows, 16, 16))
    ws = buf(nws // 8 + 1)
    Wh, knn = _lib.host_doubles([0.5] * 17 * 17), _lib.host_doubles([1.0])

    def call(L, P, s2, nbytes=nws, W=Wh, k=knn, o=out):
        return lib.gpk_mixed_gaussian_varexp_sum(None, Y.data_ptr(), 16, gm.data_ptr(), rows, L, P, W, None, 0, None, k, 0, s2, 0.0,
                                                 None, None, None, None, None if o is None else o.data_ptr(), ws.data_ptr(), nbytes)
    for L, P, s2 in ((17, 2, 0.3), (0, 2, 0.3), (2, 0, 0.3), (2, 17, 0.3), (2, 3, 0.0), (2, 3, -1.0), (2, 3, float("nan"))):
        assert call(L, P, s2) == -1, (L, P, s2)                      # GPK_E_ARG
    assert call(2, 3, 0.3, W=None) == -1 and call(2, 3, 0.3, k=None) == -1 and call(2, 3, 0.3, o=None) == -1
    assert call(16, 16, 0.3, nbytes=nws - 8) == -2                   # GPK_E_WORKSPACE
    assert call(2, 3, 0.3, nbytes=0) == -2
    assert _np(out).tolist() == [7.0, 7.0]                           # refused: nothing written
    z = lambda *s: ops.to_device(np.zeros(s))                        # noqa: E731
    good = ops.mixed_gaussian_varexp_sum(z(3, 3), z(3, 2), np.ones((3, 2)), s0=None, ssq=None, knn=[1.0], noise_variance=0.3)
    assert np.isfinite(_np(good[0])).all()
    for L, P, s2 in ((17, 2, 0.3), (2, 17, 0.3), (2, 3, 0.0)):
        with pytest.raises(_refused()):
            ops.mixed_gaussian_varexp_sum(z(3, P), z(3, L), np.ones((P, L)), s0=None, ssq=None, knn=[1.0], noise_variance=s2)
    with pytest.raises(_refused()):                                  # W of the wrong width
        ops.mixed_gaussian_varexp_sum(z(3, 3), z(3, 2), np.ones((3, 3)), s0=None, ssq=None, knn=[1.0], noise_variance=0.3)
    Z = ops.to_device(np.random.default_rng(0).normal(size=(5, 2)))
    skw = dict(variances=[1.0, 1.0], lengthscales=[1.0, 1.0], families=["SquaredExponential"] * 2, jitter=1e-6)
    for Wbad, s2 in ((np.ones((3, 3)), 0.3), (np.ones((17, 2)), 0.3), (np.ones((3, 2)), 0.0)):
        with pytest.raises(_refused()):
            ops.svgp_elbo_shard_lcm(Z, Z, z(5, Wbad.shape[0]), z(5, 2), ops.to_device(np.stack([np.eye(5)] * 2)), Wbad,
                                    noise_variance=s2, **skw)


@pytest.mark.parametrize("where", ["gmean", "ssq", "Y"])
def test_mixed_stage_nonfinite_inputs(gp, where):
    """One NaN at row 17 -- gmean[17, 1], ssq[1, 17] (so gvar[17, 1]) or Y[17, 2] -- of a 41-row problem with L = 3, P = 4: out is NaN;
    of row 17's outputs exactly those that read it are NaN (gmean: fmean and dgmu; gvar: fvar; Y: dgmu), the others keep their bits;
    every other row of every per-row output keeps its bits.  dW: a NaN residual (gmean, Y) reaches the rows p it belongs to -- all of
    them for gmean, row 2 for Y -- and a NaN variance the column of its latent."""
    ops, dev = gp.ops, _dev(gp)
    rows, L, P, b = 41, 3, 4, 17
    Y, gm, W, s0, ssq, knn = _mixed_inputs((rows, L, P, "per", True, True, "c"))

    def run(Y, gm, ssq):
        r = ops.mixed_gaussian_varexp_sum(_on(Y, "c", dev), _on(gm, "c", dev), W, s0=_on(s0, "c", dev), ssq=_on(ssq, "c", dev), knn=knn,
                                          noise_variance=0.3, s0_per_latent=True, want_moments=True, want_grads=True)
        return [_np(t) for t in r]
    clean = run(Y, gm, ssq)
    assert all(np.isfinite(a).all() for a in clean)
    Y2, g2, q2 = Y.copy(), gm.copy(), ssq.copy()
    if where == "gmean":
        g2[b, 1] = np.nan
    elif where == "ssq":
        q2[1, b] = np.nan
    else:
        Y2[b, 2] = np.nan
    out, fm, fv, dg, dW = run(Y2, g2, q2)
    assert np.isnan(out).all()
    keep = np.ones(rows, dtype=bool); keep[b] = False
    hit = {"gmean": (True, False, True), "ssq": (False, True, False), "Y": (False, False, True)}[where]
    for name, got, ref, nan_row in zip(("fmean", "fvar", "dgmu"), (fm, fv, dg), clean[1:4], hit):
        assert np.array_equal(_bits(got[keep]), _bits(ref[keep])), name
        if nan_row:
            assert np.isnan(got[b]).all(), name
        else:
            assert np.array_equal(_bits(got[b]), _bits(ref[b])), name
    nan_dW = np.zeros((P, L), dtype=bool)
    if where == "gmean":
        nan_dW[:] = True
    elif where == "ssq":
        nan_dW[:, 1] = True
    else:
        nan_dW[2, :] = True
    assert np.array_equal(np.isnan(dW), nan_dW), dW
    assert np.array_equal(_bits(dW[~nan_dW]), _bits(clean[4][~nan_dW]))


# ------------------------------------------------------------------------------------------------ 3. the fused shard
LCM_FAMILIES = ["SquaredExponential", "Matern32", "Matern52", "Matern12"]
# (M, rows, L, P, layout of the minibatch, one Z per latent, ARD)
LCM_SHARD_CASES = [
    (16, 0, 2, 3, "c", False, False),       # zero rows: [0, KL]
    (65, 130, 2, 4, "c", True, False),      # leaf + 1; one set of inducing points per latent
    (129, 64, 3, 2, "ld", False, True),     # odd ld of the minibatch rows; L > P; ARD members
    (200, 300, 3, 5, "c", True, True),      # rows > 256: the side schedule (late work on the rest-update stream)
]


def _lcm_shard_inputs(case):
    M, rows, L, P, _, sepz, ard = case
    d = 8 if M >= 200 else 2      # (kappa(Kuu), and with it the derived bound, stays meaningful: test_svgp_elbo_shard_sep_contract)
    rng = np.random.default_rng(M + rows + 7 * L)
    Z, X, _, q_mu, qs = _svgp_inputs(rng, M, rows, d, L, False)
    Y = rng.normal(size=(rows, P))
    W = rng.normal(size=(P, L)) / math.sqrt(L)      # rows of W of norm ~1: the outputs' moments are of the latents' size
    if sepz:
        Z = np.stack([Z + 0.05 * l for l in range(L)])
    ls = 0.8 + 0.1 * np.arange(L)
    if ard:
        ls = ls[:, None] * (1.0 + 0.15 * np.arange(d))[None, :]
    kw = dict(variances=list(1.0 + 0.1 * np.arange(L)), lengthscales=ls, families=LCM_FAMILIES[:L], noise_variance=0.3, jitter=1e-6,
              mean_const=0.05)
    return Z, X, Y, q_mu, qs, W, kw


def _lcm_cond(Z, kw):
    L = len(kw["families"])
    return max(math.sqrt(_kappa(Z if Z.ndim == 2 else Z[l], kw["families"][l], kw["variances"][l], kw["lengthscales"][l], 1e-6))
               for l in range(L))


@pytest.mark.parametrize("case", LCM_SHARD_CASES, ids=[str(c) for c in LCM_SHARD_CASES])
def test_svgp_elbo_shard_lcm_contract(gp, case):
    """The fused shard against its emulation (fake_lcm_ops on fake_ops' per-latent chain) within _fused_bound, as
    test_svgp_elbo_shard_sep_contract holds the separate shard; the KL to that test's reduction bound."""
    ops, dev = gp.ops, _dev(gp)
    M, rows, L, P, layout, _, _ = case
    Z, X, Y, q_mu, qs, W, kw = _lcm_shard_inputs(case)
    tX, tY = _on(X, layout, dev), _on(Y, layout, dev)
    out, info = ops.svgp_elbo_shard_lcm(_on(Z, "c", dev), tX, tY, _on(q_mu, "c", dev), _on(qs, "c", dev), W, **kw)
    assert np.all(_np(info) == 0) and _np(info).shape == (L,)
    assert np.array_equal(_bits(_np(tX)), _bits(X)) and np.array_equal(_bits(_np(tY)), _bits(Y)), "an input was modified"
    fo, finfo = fake_lcm_ops.svgp_elbo_shard_lcm(*(torch.from_numpy(np.ascontiguousarray(a)) for a in (Z, X, Y, q_mu, qs)), W, **kw)
    dv, fv = _np(out), _np(fo)
    print("lcm shard", case, "device", dv, "emulation", fv)
    if rows == 0:
        assert dv[0] == 0.0 and fv[0] == 0.0, (dv, fv)
    assert abs(dv[0] - fv[0]) <= _fused_bound(M, fv[0], abs(fv[0]) + 10 * rows * P, _lcm_cond(Z, kw)), (dv, fv)
    kl = float(fake_ops.gauss_kl_white(torch.from_numpy(q_mu), torch.from_numpy(qs))[0])
    assert abs(dv[1] - kl) <= (2 * (M * M * L + 2) + 4) * U * (abs(kl) + M * M * L), (dv[1], kl)


def test_lcm_shard_with_identity_weights_is_the_separate_shard(gp):
    """W = I, L = P = 3: the same numbers as ops.svgp_elbo_shard_sep, within twice the bound (each side once)."""
    ops, dev = gp.ops, _dev(gp)
    case = (65, 130, 3, 3, "c", True, False)
    Z, X, Y, q_mu, qs, _, kw = _lcm_shard_inputs(case)
    t = [_on(a, "c", dev) for a in (Z, X, Y, q_mu, qs)]
    lcm = _np(ops.svgp_elbo_shard_lcm(*t, np.eye(3), **kw)[0])
    sep = _np(ops.svgp_elbo_shard_sep(*t, **kw)[0])
    assert abs(lcm[0] - sep[0]) <= 2 * _fused_bound(65, sep[0], abs(sep[0]) + 10 * 130 * 3, _lcm_cond(Z, kw)), (lcm, sep)
    assert lcm[1] == sep[1], (lcm, sep)      # (the same KL launches on the same operands)


# ------------------------------------------------------------------------------------------------ 4. the model
M_, N_, L_, P_, D_ = 24, 50, 3, 4, 2
MEMBERS = [("SquaredExponential", 1.1, np.array([0.9, 1.4])), ("Matern32", 0.8, 1.3), ("SquaredExponential", 1.3, 1.7)]
NOISE, MEAN = 0.2, 0.3


def _model_problem(whiten=True, q_diag=False, sepz=False, seed=11):
    """X, Y, per-latent Z, q_mu [M, L], q_sqrt, W.  whiten=False: the same q(u) expressed un-whitened (test_gpu_likelihoods._svgp_problem)"""
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(N_, D_))
    Z = X[:M_] + 0.05 * rng.normal(size=(M_, D_))
    Zs = [Z + 0.02 * l for l in range(L_)] if sepz else [Z] * L_
    q_mu = 0.4 * rng.normal(size=(M_, L_))
    if q_diag:
        q_sqrt = rng.uniform(0.3, 0.9, size=(M_, L_))
    else:
        q_sqrt = np.stack([np.tril(0.05 * rng.normal(size=(M_, M_))) + 0.6 * np.eye(M_) for _ in range(L_)])
    if not whiten:
        q_mu, q_sqrt = q_mu.copy(), q_sqrt.copy()
        for l, (fam, v, ls) in enumerate(MEMBERS):
            Kmm = orc.Kuu(Zs[l], variance=v, lengthscales=ls, jitter=orc.DEFAULT_JITTER, kernel=fam)
            Lm = np.linalg.cholesky(Kmm)
            q_mu[:, l] = Lm @ q_mu[:, l]
            if q_diag:
                q_sqrt[:, l] = q_sqrt[:, l] / np.sqrt(np.diag(np.linalg.inv(Kmm)))
            else:
                q_sqrt[l] = Lm @ q_sqrt[l]
    W = rng.normal(size=(P_, L_)) / math.sqrt(L_)
    Y = np.sin(X.sum(1, keepdims=True)) + 0.3 * rng.normal(size=(N_, P_))
    return X, Y, Zs, q_mu, q_sqrt, W


def _build(gp, Zs, q_mu, q_sqrt, W, *, sepz=False, whiten=True, likelihood=None, num_data=1000, mean=MEAN):
    K, IV = gp.kernels, gp.inducing_variables
    kern = K.LinearCoregionalization([getattr(K, fam)(variance=v, lengthscales=ls) for fam, v, ls in MEMBERS], W.copy())
    if sepz:
        iv = IV.SeparateIndependentInducingVariables([IV.InducingPoints(z.copy()) for z in Zs])
    else:
        iv = IV.SharedIndependentInducingVariables(IV.InducingPoints(Zs[0].copy()))
    lik = gp.likelihoods.Gaussian(NOISE) if likelihood is None else likelihood
    return gp.models.SVGP(kern, lik, iv, q_mu=q_mu.copy(), q_sqrt=q_sqrt.copy(), num_latent_gps=L_, whiten=whiten, num_data=num_data,
                          q_diag=q_sqrt.ndim == 2,                          mean_function=gp.mean_functions.Constant(mean))


def _latent_moments(Xnew, Zs, q_mu, q_sqrt, whiten, full_cov):
    """per-latent oracle q(g): means [N, L]; variances [N, L] or, full_cov, [L, N, N]; the KL summed over the latents"""
    mus, vs, kl = [], [], 0.0
    for l, (fam, v, ls) in enumerate(MEMBERS):
        qs = q_sqrt[:, l:l + 1] if q_sqrt.ndim == 2 else q_sqrt[l:l + 1]
        mu, var = orc.svgp_predict_f(Xnew, Zs[l], q_mu[:, l:l + 1], qs, variance=v, lengthscales=ls, whiten=whiten, full_cov=full_cov,
                                     kernel=fam)
        mus.append(mu[:, 0])
        vs.append(var[0] if full_cov else var[:, 0])
        K = None if whiten else orc.Kuu(Zs[l], variance=v, lengthscales=ls, jitter=orc.DEFAULT_JITTER, kernel=fam)
        kl += float(orc.gauss_kl(q_mu[:, l:l + 1], qs, K))
    return np.stack(mus, 1), (np.stack(vs, 0) if full_cov else np.stack(vs, 1)), kl


def _bernoulli_ve(Y, f, fv):
    """sum of the 20-node Gauss-Hermite variational expectations of the probit Bernoulli (likelihoods/scalar_discrete.py) in NumPy"""
    import scipy.special as sps
    x, w = np.polynomial.hermite.hermgauss(20)
    F = f[..., None] + np.sqrt(2.0 * fv)[..., None] * x
    p = 0.5 * (1.0 + sps.erf(F / np.sqrt(2.0))) * (1 - 2e-3) + 1e-3
    return float((np.log(np.where(Y[..., None] == 1.0, p, 1.0 - p)) * w / np.sqrt(np.pi)).sum())


@pytest.mark.parametrize("form", ["fused", "fused-separate-Z", "unwhitened", "q_diag", "bernoulli"])
def test_lcm_model_elbo(gp, form):
    """SVGP.elbo of the model against per-latent oracle moments mixed in NumPy, 1e-8 relative: the fused shard (shared and per-latent
    inducing points), and the composed path for the un-whitened model, a diagonal q_sqrt and a Bernoulli likelihood on the mixed moments."""
    whiten, q_diag, sepz = form != "unwhitened", form == "q_diag", form == "fused-separate-Z"
    X, Y, Zs, q_mu, q_sqrt, W = _model_problem(whiten, q_diag, sepz)
    lik = None
    if form == "bernoulli":
        Y = (Y > 0).astype(np.float64)
        lik = gp.likelihoods.Bernoulli()
    m = _build(gp, Zs, q_mu, q_sqrt, W, sepz=sepz, whiten=whiten, likelihood=lik)
    assert (m._fused_lcm_config() is not None) == form.startswith("fused")
    gmu, gvar, kl = _latent_moments(X, Zs, q_mu, q_sqrt, whiten, False)
    f, fv = gmu @ W.T + MEAN, gvar @ (W ** 2).T
    if form == "bernoulli":
        ve = _bernoulli_ve(Y, f, fv)
    else:
        ve = float((-0.5 * np.log(2 * np.pi * NOISE) - 0.5 * ((Y - f) ** 2 + fv) / NOISE).sum())
    ref = ve * (1000 / N_) - kl
    got = float(m.elbo((X, Y)))
    print("lcm elbo", form, got, ref)
    np.testing.assert_allclose(got, ref, rtol=1e-8)
    if form.startswith("fused"):        # ... and the fused shard against the composed path of the same model
        m._fused_lcm_config = lambda: None
        np.testing.assert_allclose(float(m.elbo((X, Y))), got, rtol=1e-10)


@pytest.mark.parametrize("sepz", [False, True])
def test_lcm_predict_f_all_covariance_forms(gp, sepz):
    """predict_f in the four covariance forms, fused and from the precompute cache, against mixed oracle moments, to the 1e-9 absolute
    tests/test_gpu_models.py holds SeparateIndependent to; predict_y, predict_log_density and predict_f_samples run on them."""
    X, Y, Zs, q_mu, q_sqrt, W = _model_problem(sepz=sepz)
    m = _build(gp, Zs, q_mu, q_sqrt, W, sepz=sepz)
    Xnew = np.random.default_rng(5).normal(size=(7, D_))
    gmu, gvar, _ = _latent_moments(Xnew, Zs, q_mu, q_sqrt, True, False)
    _, gcov, _ = _latent_moments(Xnew, Zs, q_mu, q_sqrt, True, True)
    refs = {(False, False): gvar @ (W ** 2).T, (False, True): np.einsum("nl,pl,ql->npq", gvar, W, W),
            (True, False): np.einsum("lnm,pl->pnm", gcov, W ** 2), (True, True): np.einsum("lnm,pl,ql->npmq", gcov, W, W)}
    post = m.posterior()
    for (fc, foc), ref in refs.items():
        for who, fn in (("fused", m.predict_f), ("cache", post.predict_f)):
            mu, var = fn(Xnew, full_cov=fc, full_output_cov=foc)
            np.testing.assert_allclose(_np(mu), gmu @ W.T + MEAN, rtol=0, atol=1e-9, err_msg=f"{who} mean {fc} {foc}")
            assert _np(var).shape == ref.shape, (who, fc, foc)
            np.testing.assert_allclose(_np(var), ref, rtol=0, atol=1e-9, err_msg=f"{who} {fc} {foc}")
    ym, yv = m.predict_y(Xnew)
    np.testing.assert_allclose(_np(ym), gmu @ W.T + MEAN, atol=1e-9)
    np.testing.assert_allclose(_np(yv), refs[(False, False)] + NOISE, atol=1e-9)
    ld = _np(m.predict_log_density((Xnew, Y[:7])))
    ref_ld = -0.5 * np.log(2 * np.pi * _np(yv)) - 0.5 * (Y[:7] - _np(ym)) ** 2 / _np(yv)
    np.testing.assert_allclose(ld.reshape(-1), ref_ld.sum(-1) if ld.ndim == 1 else ref_ld.reshape(-1), rtol=1e-9, atol=1e-9)
    assert tuple(m.predict_f_samples(Xnew, 5).shape) == (5, 7, P_)
    assert tuple(m.predict_f_samples(Xnew, 5, full_cov=False).shape) == (5, 7, P_)


def test_lcm_kernel_matrices(gp):
    """K / K_diag in both output-covariance forms against einsum over the members' matrices; K(X)[n, :, n, :] == K_diag(X)[n]."""
    rng = np.random.default_rng(3)
    X, X2, W = rng.normal(size=(9, D_)), rng.normal(size=(6, D_)), rng.normal(size=(P_, L_))
    K = gp.kernels
    kern = K.LinearCoregionalization([getattr(K, fam)(variance=v, lengthscales=ls) for fam, v, ls in MEMBERS], W)
    assert isinstance(kern, K.MultioutputKernel) and kern.num_latent_gps == L_ and len(kern.latent_kernels) == L_
    assert kern.W.transform.forward(np.array([-2.0]))[0] == -2.0          # no transform
    Kg = lambda A, B: np.stack([orc.stationary_K(fam, A, B, variance=v, lengthscales=ls) for fam, v, ls in MEMBERS])   # noqa: E731
    t = gp.ops.to_device
    np.testing.assert_allclose(_np(kern.Kgg(t(X), t(X2))), Kg(X, X2), atol=1e-13)
    for A, B in ((X, X2), (X, None)):
        np.testing.assert_allclose(_np(kern(A, B, full_cov=True, full_output_cov=True)), np.einsum("lnm,kl,ql->nkmq", Kg(A, B), W, W),
                                   atol=1e-12)
        np.testing.assert_allclose(_np(kern(A, B, full_cov=True, full_output_cov=False)), np.einsum("lnm,kl,kl->knm", Kg(A, B), W, W),
                                   atol=1e-12)
    kd = np.array([v for _, v, _ in MEMBERS])[None, :].repeat(9, 0)
    np.testing.assert_allclose(_np(kern(X, full_cov=False, full_output_cov=True)), np.einsum("nl,kl,ql->nkq", kd, W, W), atol=1e-13)
    np.testing.assert_allclose(_np(kern(X, full_cov=False, full_output_cov=False)), kd @ (W ** 2).T, atol=1e-13)
    full, diag = _np(kern(X, full_cov=True, full_output_cov=True)), _np(kern(X, full_cov=False, full_output_cov=True))
    np.testing.assert_allclose(np.stack([full[n, :, n, :] for n in range(9)]), diag, atol=1e-12)


# ------------------------------------------------------------------------------------------------ 5. gradients
def _torch_elbo_lcm(X, Y, Zs, q_mu, q_sqrt, W, variances, lss, noise, mean, num_data):
    """the whitened ELBO of the model on torch fp64 tensors (conditionals/util.py:84-169 per latent, mix_latent_gp, Gaussian
    variational expectations, the whitened KL over the L latents)"""
    M = q_mu.shape[0]
    gmu, gvar = [], []
    for l, (fam, _, _) in enumerate(MEMBERS):
        kf = lambda A, B: orcg._rbf(A, B, variances[l], lss[l], fam)   # noqa: E731
        Lm = torch.linalg.cholesky(kf(Zs[l], Zs[l]) + 1e-6 * torch.eye(M, dtype=torch.float64))
        A = torch.linalg.solve_triangular(Lm, kf(Zs[l], X), upper=False)
        LTA = torch.tril(q_sqrt[l]).T @ A
        gmu.append(A.T @ q_mu[:, l])
        gvar.append(variances[l] - (A * A).sum(0) + (LTA * LTA).sum(0))
    gmu, gvar = torch.stack(gmu, 1), torch.stack(gvar, 1)
    f, fv = gmu @ W.T + mean, gvar @ (W * W).T
    ve = -0.5 * math.log(2 * math.pi) - 0.5 * torch.log(noise) - 0.5 * ((Y - f) ** 2 + fv) / noise
    Lq = torch.tril(q_sqrt)
    kl = 0.5 * ((q_mu * q_mu).sum() - M * q_mu.shape[1] - torch.log(torch.diagonal(Lq, dim1=1, dim2=2) ** 2).sum() + (Lq * Lq).sum())
    return ve.sum() * (num_data / X.shape[0]) - kl


@pytest.mark.parametrize("sepz", [False, True])
def test_lcm_elbo_and_grad_vs_autograd(gp, sepz):
    """SVGP.elbo_and_grad of the model (one Matern32 member, one ARD member) against torch autograd on the same ELBO: the value to 1e-9
    relative, every gradient to 1e-8 max(1, |ref|_max) -- what test_active_dims_and_separate_independent_model_gradients holds the
    per-latent pass to; a parameter's gradient w.r.t. its unconstrained value through its transform.  Then three central differences
    on W at 1e-5, and one ascent step raises the ELBO."""
    X, Y, Zs, q_mu, q_sqrt, W = _model_problem(sepz=sepz, seed=13)
    m = _build(gp, Zs, q_mu, q_sqrt, W, sepz=sepz, num_data=2000)
    v, g = m.elbo_and_grad((X, Y))
    t = lambda a, r=True: torch.tensor(np.asarray(a, dtype=np.float64), dtype=torch.float64, requires_grad=r)   # noqa: E731
    tZ = [t(z) for z in Zs] if sepz else [t(Zs[0])] * L_
    tq, ts, tW = t(q_mu), t(q_sqrt), t(W)
    tv, tl = [t(mv) for _, mv, _ in MEMBERS], [t(np.atleast_1d(ls)) for _, _, ls in MEMBERS]
    tn, tm = t(NOISE), t(MEAN)
    F = _torch_elbo_lcm(t(X, False), t(Y, False), tZ, tq, ts, tW, tv, tl, tn, tm, 2000)
    F.backward()
    rv = float(F.detach())
    print("lcm grad value", v, rv, "device elbo", float(m.elbo((X, Y))))
    assert abs(v - rv) <= 1e-9 * abs(rv), (v, rv)
    assert abs(v - float(m.elbo((X, Y)))) <= 1e-9 * abs(v)

    def check(name, par, ref):
        ref = np.asarray(ref.detach().numpy() if torch.is_tensor(ref) else ref, dtype=np.float64)
        u = par.unconstrained_variable
        tri = par.transform.inverse(ref).reshape(u.shape) if type(par.transform).__name__ == "FillTriangular" else \
            ref.reshape(u.shape) * par.transform.forward_grad(u)
        got = np.asarray(g[par], dtype=np.float64)
        err = np.abs(got - tri).max()
        print("lcm grad", name, "max err", err, "ref max", np.abs(tri).max())
        assert err <= 1e-8 * max(1.0, np.abs(tri).max()), (name, err)
    for l, kk in enumerate(m.kernel.kernels):
        check(f"variance[{l}]", kk.variance, tv[l].grad)
        check(f"lengthscales[{l}]", kk.lengthscales, tl[l].grad)
    if sepz:
        for l, iv in enumerate(m.inducing_variable.inducing_variable_list):
            check(f"Z[{l}]", iv.Z, tZ[l].grad)
    else:
        check("Z", m.inducing_variable.inducing_variable.Z, tZ[0].grad)
    check("q_mu", m.q_mu, tq.grad)
    check("q_sqrt", m.q_sqrt, torch.tril(ts.grad))
    check("W", m.kernel.W, tW.grad)
    check("noise", m.likelihood.variance, tn.grad)
    check("mean", m.mean_function.c, tm.grad)
    assert set(g) == set(m.trainable_parameters)
    # central differences on three entries of W (the model's own forward): 1e-5 relative to the gradient's size
    gW = np.asarray(g[m.kernel.W]).reshape(P_, L_)
    for (p, l) in ((0, 0), (2, 1), (3, 2)):
        h = 1e-5
        vals = []
        for s in (+1, -1):
            W2 = W.copy(); W2[p, l] += s * h
            m.kernel.W.assign(W2)
            vals.append(float(m.elbo((X, Y))))
        m.kernel.W.assign(W)
        fd = (vals[0] - vals[1]) / (2 * h)
        assert abs(fd - gW[p, l]) <= 1e-5 * max(1.0, np.abs(gW).max()), (p, l, fd, gW[p, l])
    # one step of plain ascent along the gradient (unconstrained variables) raises the ELBO
    before = float(m.elbo((X, Y)))
    gn = math.sqrt(sum(float((np.asarray(a) ** 2).sum()) for a in g.values()))
    for par, a in g.items():
        par.assign_unconstrained(par.unconstrained_variable + (1e-3 / gn) * np.asarray(a).reshape(par.unconstrained_variable.shape))
    after = float(m.elbo((X, Y)))
    assert after > before, (before, after)


def test_lcm_reverse_pass_refusals(gp):
    """Outside the reverse pass of the mixing stage, NotImplementedError names the limit -- before anything touches a device: the
    un-whitened model, a diagonal q_sqrt, a heteroskedastic or a quadrature likelihood under elbo_and_grad; the device-resident trainer;
    natural gradients."""
    from gpflow_amd import optimizers, training
    X, Y, Zs, q_mu, q_sqrt, W = _model_problem()
    data = (X, Y)
    with pytest.raises(NotImplementedError, match="un-whitened"):
        _build(gp, Zs, q_mu, q_sqrt, W, whiten=False).elbo_and_grad(data)
    qd = np.full((M_, L_), 0.5)
    with pytest.raises(NotImplementedError, match="diagonal q_sqrt"):
        _build(gp, Zs, q_mu, qd, W).elbo_and_grad(data)
    het = gp.likelihoods.Gaussian(scale=gp.functions.Linear(A=np.array([[-0.3], [0.05]]), b=np.array([0.6])))
    with pytest.raises(NotImplementedError, match="heteroskedastic"):
        _build(gp, Zs, q_mu, q_sqrt, W, likelihood=het).elbo_and_grad(data)
    with pytest.raises(NotImplementedError, match="non-Gaussian"):
        _build(gp, Zs, q_mu, q_sqrt, W, likelihood=gp.likelihoods.Bernoulli()).elbo_and_grad(data)
    ok = _build(gp, Zs, q_mu, q_sqrt, W)
    with pytest.raises(NotImplementedError, match="trainer"):
        training.SVGPTrainer(ok)
    with pytest.raises(NotImplementedError, match="natural gradients"):
        optimizers.NaturalGradient(gamma=0.1).minimize(ok, data)
