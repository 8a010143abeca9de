"""Shared by tests/test_wide_host.py (CPU) and tests/test_gpu_wide_kernels.py: the cases of the wide adaLN kernels (include/cvar_wide.h, 2048 < C <=
CVAR_WIDE_CMAX), their operands, and a numpy model of the kernels' fp32 arithmetic in the wide layout.  The float64 oracle, the float32 yardstick, the
bound and the input families are oracle/norm_ref.py's (imported, not edited); its case tables stop at C = 2048, so the cases are generated here.

Layout of a wide row (csrc/ops.hip, ln_modulate_kernel at NV = 9 .. 12): NV = ceil(C / 256) float4 vectors per lane, vector i of lane L covers the columns
(64 i + L) 4 .. + 3; only the LAST vector can be partly populated (C % 256 != 0) and its dead lanes hold zeros.  Sums: per lane over the vectors in order,
inside a vector (e0 + e1) + (e2 + e3) for the mean and element by element for the squares; then one xor-shuffle tree (32, 16, 8, 4, 2, 1) over the 64 lanes."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import norm_ref as N

F32 = np.float32
CMAX = 3072                                     # CVAR_WIDE_CMAX; tests/test_wide_host.py holds it to the header and to _lib.WIDE_CMAX
WIDE_C = (2052, 2304, 2500, 2560, CMAX)         # nv9t (one live lane in the ninth vector), nv9, nv10t (tail in the tenth vector), nv10, nv12
WIDE_M = ((9, 3), (5, 1), (1, 1))               # (M, rows_per): four rows per block -> more than one block with a partial one, a partial block, one row
# (C, M, rows_per, family)
CASES = {i + 1: c for i, c in enumerate(
    [(C, M, rp, 'unit') for C in WIDE_C for M, rp in WIDE_M] +
    [(2304, 9, 3, fam) for fam in N.LN_FAMILIES[1:]] +
    [(2500, 9, 3, 'small_var'), (2500, 9, 3, 'const_row'), (CMAX, 9, 3, 'outlier'), (2816, 5, 3, 'unit')])}          # 2816: nv11


def name(n):
    C, M, rp, fam = CASES[n]
    return f'{n}-C{C}-nv{(C + 255) // 256}{"t" if C % 256 else ""}-M{M}x{rp}-{fam}'


def inputs(n):
    """-> x (M, C), scale, shift (groups, C) fp32; the seed is 1000 + the case number (norm_ref's own cases use 1 ..)"""
    C, M, rp, fam = CASES[n]
    g = torch.Generator().manual_seed(1000 + n)
    x = N._ln_x(g, M, C, fam).float()
    G = (M + rp - 1) // rp
    return x, 0.4 * torch.randn(G, C, generator=g), 0.4 * torch.randn(G, C, generator=g)


_REFS = {}


def refs(n):
    """-> x, s, b, float64 oracle, float32 yardstick y; computed once per process"""
    if n not in _REFS:
        C, M, rp, fam = CASES[n]
        x, s, b = inputs(n)
        _REFS[n] = (x, s, b, N.ln_forward(x, s, b, rp), N.ln_forward(x, s, b, rp, dtype=np.float32).y)
    return _REFS[n]


# ------------------------------------------------------------------------------------------------ the model
FAULTS = N.LN_FWD_FAULTS            # restated for the wide layout below: the tail is the LAST of nine to twelve vectors, NV 256 is 2304 .. 3072


def _tree(a):
    for o in (32, 16, 8, 4, 2, 1):
        a = a + a[:, np.arange(64) ^ o]
    return a[:, 0]


def forward_model(x, s, b, rows_per, eps=N.EPS, fault=None):
    x, s, b = (np.asarray(t, F32) for t in (x, s, b))
    M, C = x.shape
    nv = (C + 255) // 256
    assert 9 <= nv <= 12, 'the wide instantiations'
    tail = C % 256 != 0
    v = np.zeros((M, nv * 256), F32)
    v[:, :C] = x
    v = v.reshape(M, nv, 64, 4)
    live = (np.arange(nv * 256) < C).reshape(1, nv, 64, 4)
    vm = v.copy()
    if fault == 'tail_out_of_mean' and tail:
        vm[:, nv - 1] = 0
    a = np.zeros((M, 64), F32)
    for i in range(nv):
        a = a + ((vm[:, i, :, 0] + vm[:, i, :, 1]) + (vm[:, i, :, 2] + vm[:, i, :, 3]))
    denom = F32(nv * 256 if fault == 'div_nv256' else C)
    mean = _tree(a) / denom
    d = np.where(live, v - mean[:, None, None, None], F32(0)).astype(F32)
    dq = d.copy()
    if fault == 'tail_out_of_var' and tail:
        dq[:, nv - 1] = 0
    q = np.zeros((M, 64), F32)
    for i in range(nv):
        for e in range(4):
            q = q + dq[:, i, :, e] * dq[:, i, :, e]
    var = _tree(q) / denom
    rstd = (F32(1) / np.sqrt(var + F32(0 if fault == 'no_eps' else eps))).astype(F32)
    g = np.arange(M) // rows_per
    if fault == 'group_off_by_one' and s.shape[0] > 1:
        g = np.minimum((np.arange(M) + 1) // rows_per, s.shape[0] - 1)
    d = d.reshape(M, -1)[:, :C]
    return NS(y=(d * rstd[:, None]) * (F32(1) + s[g]) + b[g], mean=mean, rstd=rstd)
