"""float64 restatement of the weight rule of regional guidance (include/cvar_region.h), shared by tests/test_region_host.py and
tests/test_gpu_region.py.  Nothing here is taken from the library: the maps are read as python floats (fp32 values are exact in float64), every mean
over a bin is math.fsum - the correctly rounded sum - divided by the bin size, and the result is left in float64 so that the caller decides how to
compare it with an fp32 table."""
import math

import numpy as np


def bins(pn, S):
    """cell index -> (r0, r1, c0, c1): latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns"""
    edge = [(i * S // pn, -((-(i + 1) * S) // pn)) for i in range(pn)]
    return [(r0, r1, c0, c1) for (r0, r1) in edge for (c0, c1) in edge]


def coef_ref(regions, strength, cfg, pns, mf):
    """regions (B, K, S, S) fp32, strength (B, S, S) fp32 or None, cfg (B, K) float64 -> (coef (B, L, 4) float64, pure (B, L) bool) with
    L = sum mf pn^2 in the token order of generation (the halves of a scale read the same maps, so their order changes no value).
    pure: one label holds all the weight of every cell of the token's bin"""
    w = np.asarray(regions, dtype=np.float32).astype(np.float64)
    g = None if strength is None else np.asarray(strength, dtype=np.float32).astype(np.float64)
    cf = np.asarray(cfg, dtype=np.float64)
    B, K, S = w.shape[0], w.shape[1], w.shape[-1]
    n_scales = len(pns)
    tot = w[:, 0].copy()
    for k in range(1, K):
        tot = tot + w[:, k]                                      # w_0 + ... + w_{K-1} in index order
    nrm = (w / tot[:, None]).tolist()
    gl = None if g is None else g.tolist()
    coef = np.zeros((B, mf * sum(p * p for p in pns), 4))
    pure = np.zeros(coef.shape[:2], dtype=bool)
    o = 0
    for si, pn in enumerate(pns):
        ratio = si / (n_scales - 1)
        for cell, (r0, r1, c0, c1) in enumerate(bins(pn, S)):
            n = (r1 - r0) * (c1 - c0)
            for b in range(B):
                gbar = 1.0 if gl is None else math.fsum(gl[b][r][c] for r in range(r0, r1) for c in range(c0, c1)) / n
                row, neg, is_pure = [0.0] * 4, 0.0, False
                for k in range(K):
                    vals = [nrm[b][k][r][c] for r in range(r0, r1) for c in range(c0, c1)]
                    wbar = math.fsum(vals) / n
                    is_pure = is_pure or all(v == 1.0 for v in vals)
                    t = (float(cf[b, k]) * gbar) * ratio
                    row[k] = wbar * (1 + t)
                    neg += wbar * t
                row[K] = -neg
                for h in range(mf):
                    coef[b, o + h * pn * pn + cell] = row
                    pure[b, o + h * pn * pn + cell] = is_pure
        o += mf * pn * pn
    return coef, pure


def ulps(got32, ref64):
    """|got - ref| in units of the fp32 spacing at fp32(ref): 0.5 is the final rounding alone"""
    got32 = np.asarray(got32, dtype=np.float32)
    r32 = np.asarray(ref64).astype(np.float32)
    return np.abs(got32.astype(np.float64) - ref64) / np.spacing(np.abs(r32)).astype(np.float64)


def region_maps(B, K, S, seed):
    """(B, K, S, S) fp32 maps: row 0 random weights with whole patches of zeros (labels absent in places), row 1 a binary split into K vertical
    bands (pure bins), further rows smooth random weights.  Every latent cell keeps a positive sum."""
    rng = np.random.default_rng(seed)
    w = rng.random((B, K, S, S), dtype=np.float32) + np.float32(0.05)
    for k in range(1, K):
        w[0, k, (k * 3) % S:(k * 3) % S + S // 3, :S // 2] = 0.0          # label k absent from a patch; label 0 stays everywhere
    if B > 1:
        band = np.minimum(np.arange(S) * K // S, K - 1)
        w[1] = (band[None, None, :] == np.arange(K)[:, None, None]).astype(np.float32) * np.ones((1, S, 1), dtype=np.float32)
    return w
