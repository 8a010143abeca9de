"""ORACLE (test infrastructure only - never imported by the product path).

Normalisation kernels: float64 oracles, float32 yardsticks, case tables, per-element bounds and numpy models of the kernels' arithmetic
for cvar_ln_modulate, cvar_ln_modulate_bwd, cvar_gated_grad, cvar_groupnorm_silu and cvar_groupnorm_silu_partials.
tests/test_norm_oracle_host.py (CPU) pins the oracles to torch in float64, shows that the models stay inside the bounds and that planted faults
do not; tests/test_gpu_norm_oracle.py holds the kernels to the same bounds on the same operands.

Every oracle takes the operands AS STORED (bf16 operands are converted exactly) and one function serves both precisions: `dtype=np.float64` is the
oracle, `dtype=np.float32` the yardstick (two-pass mean / variance, numpy's summation).

Bounds (u = 2^-24; per element, from float64 quantities and the float32 yardstick only - never from what a kernel returned):
  LN forward, row m      E_m = max( max_c |y32 - y64| , 2^-23 ( max_c |y64| + rstd max_c |x| max_c |1 + s| ) );  4 E_m  (+ 2^-8 |y64_c| for bf16 output)
  LN backward dx, row m  4 max( max_c |dx32 - dx64| , 2^-23 ( max |dx_in| + rstd max |g| (1 + max |xhat|^2) + rstd^2 max |x| max |g| ) )
  dscale, dshift, dgate  per sequence r: 4 max( max_c |v32 - v64| , 2^-23 max_c sum_t |term| ); dscale's floor times 1 + max_t (rstd max |x|)
  GroupNorm output       2^-20 ( K_g (|x a| + |mean_g a|) + |b_c| ): the kernel applies x a + d with rounded a = rstd w, d = b - mean a; as
                         fma(x, a, d) its first-order worst case is 2^-21 of that sum at K_g = 1 (the separate product adds 2^-24 |x a|).  K_g = max(1, sum (x - pivot)^2 / sum (x - mean_g)^2) is the
                         conditioning of statistics accumulated in fp32 around the pivots (channel's first pixel, or the tile pivots).
                         SiLU: times 1.1 (the bound on |silu'|) plus SILU_REL |y|;  bf16 output: + 2^-8 |y64|.
  df                     2^-22 |df64| (two roundings)  (+ 2^-8 |df64| for bf16)
SILU_REL: fp32 kernel 2^-22 (__expf, one addition, the IEEE quotient, ~4 u).  bf16 kernel: y * v_rcp_f32(1 + v_exp_f32(-log2e y)); both instructions
are documented to 1 ulp (2^-23 relative), plus the roundings of the argument product, the addition and the final product (2^-24 each; the
argument's rounding moves silu by y^2 sig (1 - sig) 2^-24 <= 2^-24 |y|-ish, inside the same term) - 2^-21 relative covers them.
The margin 4 is the house margin of tests/test_gpu_attn_train_oracle.py.
"""
from __future__ import annotations

from types import SimpleNamespace as NS

import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = 1e-6
SILU_REL = {'f32': 2.0 ** -22, 'bf16': 2.0 ** -21}


def as_np(t, dtype=F64):
    """stored values -> numpy of `dtype` (bf16 / fp32 -> float64 is exact)"""
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t).astype(dtype)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def ratio_of(err, bound):
    """max over the elements of |error| / bound; 0 / 0 (an element that must be exact and is) counts as 0"""
    err, bound = np.broadcast_arrays(np.abs(err), bound)
    r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    return float(r.max())


# ================================================================================================ LayerNorm + modulation
def _groups(M, rows_per, nrows):
    return np.zeros(M, dtype=np.int64) if nrows == 1 else np.arange(M) // rows_per


def ln_forward(x, s, b, rows_per, eps=EPS, dtype=F64):
    """y = xhat (1 + s) + b with xhat = (x - mean) rstd, biased variance; s, b: (groups, C) rows, row m uses m // rows_per (one row: all)"""
    x, s, b = as_np(x, dtype), as_np(s, dtype), as_np(b, dtype)
    M, C = x.shape
    mean = x.mean(1, dtype=dtype, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, dtype=dtype, keepdims=True)
    rstd = (1 / np.sqrt(var + dtype(eps))).astype(dtype)
    xhat = d * rstd
    g = _groups(M, rows_per, s.shape[0])
    return NS(y=xhat * (1 + s[g]) + b[g], mean=mean[:, 0], rstd=rstd[:, 0], xhat=xhat)


def ln_backward(x, dy, s, dx_in, R, l, eps=EPS, dtype=F64):
    """dx = dx_in + rstd (g - mean(g) - xhat mean(g xhat)), g = dy (1 + s);  dscale[r] = sum_t dy xhat,  dshift[r] = sum_t dy"""
    f = ln_forward(x, s, np.zeros_like(as_np(s)), l, eps, dtype)
    dy, s = as_np(dy, dtype), as_np(s, dtype)
    C = dy.shape[1]
    g = dy * (1 + s[_groups(R * l, l, s.shape[0])])
    mg = g.mean(1, dtype=dtype, keepdims=True)
    mgx = (g * f.xhat).mean(1, dtype=dtype, keepdims=True)
    dx0 = f.rstd[:, None] * (g - mg - f.xhat * mgx)
    dx = dx0 if dx_in is None else as_np(dx_in, dtype) + dx0
    return NS(dx=dx, dx0=dx0, dscale=(dy * f.xhat).reshape(R, l, C).sum(1, dtype=dtype), dshift=dy.reshape(R, l, C).sum(1, dtype=dtype),
              mean=f.mean, rstd=f.rstd, xhat=f.xhat, g=g)


def gated_grad(dx, f, gate, rowscale, R, l, dtype=F64):
    """df = dx gate rowscale;  dgate[r] = rowscale[r] sum_t dx f"""
    dx, f, gate = as_np(dx, dtype), as_np(f, dtype), as_np(gate, dtype)
    C = dx.shape[1]
    rs = np.ones(R, dtype) if rowscale is None else as_np(rowscale, dtype)
    g = (gate * rs[:, None])[np.arange(R * l) // l]
    return NS(df=dx * g, dgate=rs[:, None] * (dx * f).reshape(R, l, C).sum(1, dtype=dtype))


# ---- bounds
def ln_fwd_bound(ex, y32, x, s, rows_per, out_bf16):
    x, s = as_np(x), as_np(s)
    s1 = np.abs(1 + s).max(1)[_groups(x.shape[0], rows_per, s.shape[0])]
    E = np.maximum(np.abs(y32 - ex.y).max(1), 2.0 ** -23 * (np.abs(ex.y).max(1) + ex.rstd * np.abs(x).max(1) * s1))
    return NS(E=E, bound=4 * E[:, None] + (2.0 ** -8 * np.abs(ex.y) if out_bf16 else 0.0))


def ln_bwd_dx_bound(ex, dx32, x, dx_in):
    x = as_np(x)
    gm = np.abs(ex.g).max(1)
    din = 0.0 if dx_in is None else np.abs(as_np(dx_in)).max(1)
    floor = 2.0 ** -23 * (din + ex.rstd * gm * (1 + (ex.xhat ** 2).max(1)) + ex.rstd ** 2 * np.abs(x).max(1) * gm)
    yard = np.abs(dx32 - (ex.dx if dx_in is not None else ex.dx0)).max(1)
    return NS(yard=yard, floor=floor, bound=(4 * np.maximum(yard, floor))[:, None] * np.ones((1, x.shape[1])))


def colsum_bound(v64, v32, abs_terms, R, l, factor=None):
    """per sequence r: 4 max( max_c |v32 - v64| , 2^-23 max_c sum_t |term| (x factor_r) ), the same for every channel of the sequence"""
    C = v64.shape[1]
    floor = 2.0 ** -23 * abs_terms.reshape(R, l, C).sum(1).max(1)
    if factor is not None:
        floor = floor * factor
    yard = np.abs(v32 - v64).max(1)
    return NS(yard=yard, floor=floor, bound=(4 * np.maximum(yard, floor))[:, None] * np.ones((1, C)))


def dscale_factor(ex, x, R, l):
    return 1 + (ex.rstd * np.abs(as_np(x)).max(1)).reshape(R, l).max(1)


def df_bound(df64, bf16):
    return (2.0 ** -22 + (2.0 ** -8 if bf16 else 0.0)) * np.abs(df64)


# ---- numpy models of the kernels' fp32 arithmetic (summation orders as in csrc/ops.hip, csrc/train.hip)
_XOR = [np.arange(64) ^ o for o in (32, 16, 8, 4, 2, 1)]


def _wave_sum(a):
    for idx in _XOR:
        a = a + a[:, idx]
    return a[:, 0]


def _lanes(v, C):
    """(M, C) fp32 -> (M, NV, 64, 4) as the row kernels hold a row: vector i of lane L covers columns (i 64 + L) 4 .. + 3, zero past C"""
    M, nv = v.shape[0], (C + 255) // 256
    p = np.zeros((M, nv * 256), F32)
    p[:, :C] = v
    return p.reshape(M, nv, 64, 4)


def _lane_sum(v, C):
    """scalar accumulation per lane over the vectors and elements, then the shuffle tree"""
    t = _lanes(v.astype(F32), C)
    a = np.zeros((t.shape[0], 64), F32)
    for i in range(t.shape[1]):
        for e in range(4):
            a = a + t[:, i, :, e]
    return _wave_sum(a)


def _row_stats_model(x, C, eps, fault=None):
    v = _lanes(as_np(x, F32), C)
    M, nv = v.shape[0], v.shape[1]
    tail = C % 256 != 0
    live = (np.arange(nv * 256) < C).reshape(1, nv, 64, 4)
    vm = v.copy()
    if fault == 'tail_out_of_mean' and tail:
        vm[:, nv - 1] = 0
    a = np.zeros((M, 64), F32)
    for i in range(nv):
        a = a + ((vm[:, i, :, 0] + vm[:, i, :, 1]) + (vm[:, i, :, 2] + vm[:, i, :, 3]))
    denom = F32(nv * 256 if fault == 'div_nv256' else C)
    mean = _wave_sum(a) / denom
    d = np.where(live, v - mean[:, None, None, None], F32(0)).astype(F32)
    dq = d.copy()
    if fault == 'tail_out_of_var' and tail:
        dq[:, nv - 1] = 0
    q = np.zeros((M, 64), F32)
    for i in range(nv):
        for e in range(4):
            q = q + dq[:, i, :, e] * dq[:, i, :, e]
    var = _wave_sum(q) / denom
    rstd = (F32(1) / np.sqrt(var + F32(0 if fault == 'no_eps' else eps))).astype(F32)
    return mean, rstd, d.reshape(M, -1)[:, :C]


LN_FWD_FAULTS = ('tail_out_of_mean', 'tail_out_of_var', 'div_nv256', 'no_eps', 'group_off_by_one')


def ln_forward_model(x, s, b, rows_per, eps=EPS, fault=None):
    """ln_modulate_kernel: lane-strided sums + shuffle tree, (d rstd) (1 + s) + b in fp32"""
    s, b = as_np(s, F32), as_np(b, F32)
    M, C = x.shape
    mean, rstd, d = _row_stats_model(x, C, eps, fault)
    g = _groups(M, rows_per, s.shape[0])
    if fault == 'group_off_by_one' and s.shape[0] > 1:
        g = np.minimum((np.arange(M) + 1) // rows_per, s.shape[0] - 1)
    return NS(y=(d * rstd[:, None]) * (F32(1) + s[g]) + b[g], mean=mean, rstd=rstd)


def red_segments(R, l, target):
    return max(1, min(64, (target + R - 1) // max(R, 1), (l + 3) // 4))


RED_S, RED_TARGET, GG_TARGET = 8, 512, 256


def ln_stats_floats(M):
    """floats of the row-statistics area at the head of the training workspace (whole 16-byte vectors)"""
    return (2 * M + 3) & ~3


def _segmented_colsum(term, R, l, nseg, waves, fault=None):
    """sum over t of term (R l, C) per sequence: nseg row segments, inside a segment `waves` interleaved sequential accumulators folded in order,
    segments added in order - the order of ln_bwd_fused_kernel (waves = 4) and of the column kernels (waves = 1)"""
    C = term.shape[1]
    seg = (l + nseg - 1) // nseg
    K = (seg + waves - 1) // waves
    p = np.zeros((R, nseg * seg, C), F32)
    p[:, :l] = term.reshape(R, l, C)
    p = p.reshape(R, nseg, seg, C)
    if fault == 'drop_segment':
        p[:, min(1, nseg - 1)] = 0
    q = np.zeros((R, nseg, K * waves, C), F32)
    q[:, :, :seg] = p
    q = q.reshape(R, nseg, K, waves, C)
    acc = np.zeros((R, nseg, waves, C), F32)
    for k in range(K):
        acc = acc + q[:, :, k]
    if fault == 'last_row_twice':
        acc[:, 0, 0] = acc[:, 0, 0] + p[:, 0, min(seg, l) - 1]
    a = acc[:, :, 0]
    for w in range(1, waves):
        a = a + acc[:, :, w]
    out = np.zeros((R, C), F32)
    for sidx in range(nseg):
        out = out + a[:, sidx]
    return out


LN_BWD_FAULTS = ('drop_mgx', 'drop_segment', 'last_row_twice')


def ln_backward_model(x, dy, s, dx_in, R, l, eps=EPS, nseg=None, waves=4, fault=None):
    s, dy = as_np(s, F32), as_np(dy, F32)
    M, C = dy.shape
    nseg = nseg or red_segments(R, l, RED_TARGET)
    mean, rstd, d = _row_stats_model(x, C, eps)
    xhat = d * rstd[:, None]
    g = dy * (F32(1) + s[_groups(M, l, s.shape[0])])
    mg = _lane_sum(g, C) / F32(C)
    mgx = _lane_sum(g * xhat, C) / F32(C) if fault != 'drop_mgx' else np.zeros(M, F32)
    dx = rstd[:, None] * (g - mg[:, None] - xhat * mgx[:, None])
    if dx_in is not None:
        dx = as_np(dx_in, F32) + dx
    return NS(dx=dx, dscale=_segmented_colsum(dy * xhat, R, l, nseg, waves, fault), dshift=_segmented_colsum(dy, R, l, nseg, waves, fault),
              mean=mean, rstd=rstd)


def gated_grad_model(dx, f, gate, rowscale, R, l, nseg=None):
    dx, f, gate = as_np(dx, F32), as_np(f, F32), as_np(gate, F32)
    rs = np.ones(R, F32) if rowscale is None else as_np(rowscale, F32)
    nseg = nseg or red_segments(R, l, GG_TARGET)
    g = (gate * rs[:, None])[np.arange(R * l) // l]
    return NS(df=dx * g, dgate=_segmented_colsum(dx * f, R, l, nseg, 1) * rs[:, None])


# ---- cases.  Seeds are the case numbers; the GPU test and the host test build identical operands from these tables.
def ln_instance(C):
    """name of the NV / TAIL instantiation of ln_modulate_kernel, ln_bwd_row_vec_kernel and ln_bwd_fused_kernel that serves C"""
    return f'nv{(C + 255) // 256}' + ('t' if C % 256 else '')


LN_INSTANCES = tuple(f'nv{n}{t}' for n in range(1, 9) for t in ('', 't'))
#        nv1t nv1t nv1 nv2t nv2  nv3t nv3  nv4t  nv4   nv5t  nv5   nv6t  nv6   nv7t  nv7   nv8t  nv8      (260, 516, 1028: one live lane in the last vector)
LN_C = (4, 252, 256, 260, 512, 516, 768, 1000, 1024, 1028, 1280, 1500, 1536, 1540, 1792, 1920, 2048)
LN_FAMILIES = ('unit', 'small_var', 'large_mean', 'const_row', 'outlier')
CONST_ROW_VALUES = (1.5, -2.25, 0.1, 1000.3)        # C x 1.5 and C x 2.25 are exact in fp32 for every C here: the mean is exact and y must be exactly b


def _ln_x(g, M, C, family):
    n = _randn(g, M, C)
    if family == 'unit':
        return 1.7 * n + 0.3
    if family == 'small_var':
        return 0.5 + 1e-3 * n
    if family == 'large_mean':
        return 300.0 + 2.0 * n
    if family == 'const_row':
        return torch.tensor([CONST_ROW_VALUES[m % 4] for m in range(M)]).view(M, 1).expand(M, C).contiguous()
    if family == 'outlier':
        x = 1.7 * n + 0.3
        for m in range(M):
            x[m, (7 * m + 3) % C] = 1e4
        return x
    raise KeyError(family)


def _table(rows):
    return {i + 1: r for i, r in enumerate(rows)}


# (C, M, rows_per, family, one adaLN row for all (ld_ada = 0))
LN_FWD_CASES = _table(
    [(C, 7, 3, 'unit', False) for C in LN_C] +
    [(C, M, rp, 'unit', False) for C in (260, 1536) for M, rp in ((1, 1), (5, 1), (21, 7))] +
    [(C, 21, 7, fam, False) for C in (1000, 1536) for fam in LN_FAMILIES[1:]] +
    [(1000, 21, 7, 'unit', False), (768, 5, 2, 'unit', True)])
LN_BWD_ILL = ('small_var',)           # dx: rstd = 1000; the floor's rstd^2 max |x| max |g| is 2^-23 rstd |x| = 6e-5 of |dx| ~ rstd |g|
LN_FWD_ILL = ('const_row',)          # rstd = eps^-1/2 = 1000 amplifies the rounding of the mean: the bound is large against |b| by construction


def ln_fwd_name(n):
    C, M, rp, fam, ld0 = LN_FWD_CASES[n]
    return f'{n}-C{C}-{ln_instance(C)}-M{M}x{rp}-{fam}' + ('-ld0' if ld0 else '')


def ln_fwd_inputs(n):
    """-> x (M, C), scale, shift (groups, C) fp32"""
    C, M, rp, fam, ld0 = LN_FWD_CASES[n]
    g = torch.Generator().manual_seed(n)
    x = _ln_x(g, M, C, fam).float()
    G = 1 if ld0 else (M + rp - 1) // rp
    return x, 0.4 * _randn(g, G, C), 0.4 * _randn(g, G, C)


# (C, R, l, dtype of dy, path, family).  path: what the dispatch of cvar_ln_modulate_bwd takes for these operands -
#   fused       ln_bwd_fused_kernel (bf16 dy, C % 4 == 0, C <= 2048, everything 16-byte aligned); writes no row statistics
#   vec+col     ln_bwd_row_vec_kernel + ln_bwd_col_kernel: fp32 dy, or bf16 with the workspace 8 bytes off a 16-byte boundary
#   row+colvec  ln_bwd_row_kernel + ln_bwd_col_vec_kernel: bf16, C > 2048
#   row+col     ln_bwd_row_kernel + ln_bwd_col_kernel: C % 4 != 0, C > 2048 in fp32 or with the workspace 8 bytes off
LN_BWD_SEGS = ((1, 1), (5, 3), (2, 5), (2, 37), (2, 680), (300, 8), (9, 64))
LN_BWD_CASES = _table(
    [(C, 2, 6, 'bf16', 'fused', 'unit') for C in LN_C] +
    [(C, R, l, 'bf16', 'fused', 'unit') for C in (260, 1536) for R, l in LN_BWD_SEGS] +
    [(C, 2, 37, 'bf16', 'vec+col', 'unit') for C in (260, 1536)] +
    [(130, 2, 37, 'bf16', 'row+col', 'unit'), (130, 2, 37, 'f32', 'row+col', 'unit'),
     (2304, 2, 37, 'bf16', 'row+colvec', 'unit'), (2304, 2, 37, 'f32', 'row+col', 'unit')] +
    [(C, R, l, 'f32', 'vec+col', 'unit') for C in (128, 1000, 2048) for R, l in ((2, 37), (1, 9))] +
    [(1536, 2, 37, 'bf16', 'fused', fam) for fam in ('small_var', 'large_mean')] +
    [(1000, 2, 37, 'f32', 'vec+col', fam) for fam in ('small_var', 'large_mean')] +
    # equal segment counts (red_segments(2, 30) = 8 = RED_S): ln_bwd_col_vec_kernel and ln_bwd_col_kernel promise the same bits
    [(2304, 2, 30, 'bf16', 'row+colvec', 'unit'), (2304, 2, 30, 'bf16', 'row+col', 'unit')])


def ln_bwd_name(n):
    C, R, l, dt, path, fam = LN_BWD_CASES[n]
    return f'{n}-C{C}-{ln_instance(C) if C <= 2048 and C % 4 == 0 else "scalar"}-R{R}xl{l}-{dt}-{path}-{fam}'


def ln_bwd_segments(n):
    """row segments the column sums of case n are cut into (what the partial area of the workspace must show)"""
    C, R, l, dt, path, fam = LN_BWD_CASES[n]
    return red_segments(R, l, RED_TARGET) if path in ('fused', 'row+colvec') else RED_S


def ln_bwd_inputs(n):
    """-> x (M, C) fp32, dy (M, C) stored dtype, scale (R, C), dx_in (M, C)"""
    C, R, l, dt, path, fam = LN_BWD_CASES[n]
    g = torch.Generator().manual_seed(n)
    x = _ln_x(g, R * l, C, fam).float()
    dy = _randn(g, R * l, C).to(torch.bfloat16 if dt == 'bf16' else torch.float32)
    return x, dy, 0.4 * _randn(g, R, C), _randn(g, R * l, C)


# (C, R, l, dtype of f / df, form).  vec: gated_grad_vec_kernel; scalar: gated_grad_kernel (C % 4 != 0, fp32, or df one element off)
GG_CASES = _table(
    [(C, R, l, 'bf16', 'vec') for C in (4, 192, 516, 1536) for R, l in ((1, 1), (3, 50), (2, 680), (300, 8))] +
    [(130, 3, 50, 'bf16', 'scalar'), (192, 3, 50, 'bf16', 'scalar_df_off'), (192, 3, 50, 'f32', 'scalar'), (130, 2, 37, 'f32', 'scalar')])


def gg_name(n):
    C, R, l, dt, form = GG_CASES[n]
    return f'{n}-C{C}-R{R}xl{l}-{dt}-{form}'


def gg_segments(n):
    C, R, l, dt, form = GG_CASES[n]
    return red_segments(R, l, GG_TARGET) if form == 'vec' else RED_S


def gg_inputs(n):
    """-> dx (M, C) fp32, f (M, C) stored dtype, gate (R, C), rowscale (R,) or None (odd cases; even ones carry zeros)"""
    C, R, l, dt, form = GG_CASES[n]
    g = torch.Generator().manual_seed(n)
    dx, f = _randn(g, R * l, C), _randn(g, R * l, C).to(torch.bfloat16 if dt == 'bf16' else torch.float32)
    rs = None if n % 2 else torch.tensor([(1.0, 0.0, 1.25)[r % 3] for r in range(R)])
    return dx, f, 0.4 * _randn(g, R, C) + 1, rs


# ================================================================================================ GroupNorm (+ SiLU) over NHWC
def gn_pix_per_block(HW):
    return 512 if HW >= 16384 else (128 if HW >= 1024 else 32)


def groupnorm(x, w, b, G, eps=EPS, silu=False, dtype=F64):
    """x (B, HW, C) as stored -> y, and per (image, group) mean, rstd, per channel a = rstd w, d = b - mean a (y = x a + d)"""
    x, w, b = as_np(x, dtype), as_np(w, dtype), as_np(b, dtype)
    B, HW, C = x.shape
    xg = x.reshape(B, HW, G, C // G)
    mean = xg.mean((1, 3), dtype=dtype)
    dev = xg - mean[:, None, :, None]
    ss = (dev * dev).sum((1, 3), dtype=dtype)
    rstd = (1 / np.sqrt(ss / dtype(HW * (C // G)) + dtype(eps))).astype(dtype)
    a = np.repeat(rstd, C // G, 1) * w
    d = b - np.repeat(mean, C // G, 1) * a
    lin = x * a[:, None] + d[:, None]
    y = lin / (1 + np.exp(-lin)) if silu else lin
    return NS(y=y.astype(dtype), lin=lin, mean=mean, rstd=rstd, a=a, d=d, ss=ss)


def gn_conditioning(x, ex, G, piv):
    """K_g (B, G).  piv: (B, C) one pivot per channel, or (B, tiles, C) one per tile and channel"""
    x = as_np(x)
    B, HW, C = x.shape
    if piv.ndim == 2:
        piv = piv[:, None]
    T = piv.shape[1]
    num = ((x.reshape(B, T, HW // T, C) - piv[:, :, None]) ** 2).sum((1, 2)).reshape(B, G, C // G).sum(2)
    with np.errstate(divide='ignore', invalid='ignore'):
        k = np.where(ex.ss > 0, num / ex.ss, np.where(num > 0, np.inf, 1.0))
    return np.maximum(1.0, k)


def gn_bound(x, ex, b, G, K, silu, kernel, rounding=True):
    """kernel: 'f32' | 'bf16' (element type of x and of the output); rounding=False: without the term of the bf16 output rounding"""
    x, b = as_np(x), as_np(b)
    C = x.shape[2]
    Kc = np.repeat(K, C // G, 1)[:, None]
    ma = (np.repeat(ex.mean, C // G, 1) * ex.a)[:, None]
    bound = 2.0 ** -20 * (Kc * (np.abs(x * ex.a[:, None]) + np.abs(ma)) + np.abs(b))
    if silu:
        bound = 1.1 * bound + SILU_REL[kernel] * np.abs(ex.y)
    if kernel == 'bf16' and rounding:
        bound = bound + 2.0 ** -8 * np.abs(ex.y)
    return bound


def tile_partials(x, tiles, poor=False):
    """the conv epilogue's GroupNorm partials of a stored x (B, HW, C): (sum (x - piv_t), sum (x - piv_t)^2, piv_t) per (image, tile, channel)
    from float64 sums rounded to fp32, layout [b][tile][C][3].  piv_t: the tile's first pixel; poor: 8 away from it (any fp32 value is a valid pivot)"""
    x = as_np(x)
    B, HW, C = x.shape
    xt = x.reshape(B, tiles, HW // tiles, C)
    piv = (xt[:, :, 0] + (8.0 if poor else 0.0)).astype(F32).astype(F64)
    dv = xt - piv[:, :, None]
    return np.stack([dv.sum(2), (dv * dv).sum(2), piv], -1).astype(F32)


GN_FAULTS = ('raw_sums', 'drop_last_chunk', 'skip_second_trip', 'ignore_tile_pivots')


def _gn_apply_model(x, mean, ss, n, w, b, G, eps, silu):
    C = x.shape[2]
    rstd = (1.0 / np.sqrt(np.maximum(ss / n, 0.0) + F64(F32(eps)))).astype(F32)
    a = (np.repeat(rstd, C // G, 1) * as_np(w, F32)).astype(F32)
    d = (as_np(b, F32) - np.repeat(mean.astype(F32), C // G, 1) * a).astype(F32)
    y = x * a[:, None] + d[:, None]                 # product and sum rounded separately (the library is built without contraction)
    if silu:
        y = (y / (F32(1) + np.exp(-y).astype(F32))).astype(F32)
    return NS(y=y, a=a, d=d, rstd=rstd)


def groupnorm_model(x, w, b, G, eps=EPS, silu=False, vec=4, fault=None):
    """gn_stats_kernel in its own order (a chunk's pixels strided over PL = 256 / (C / vec) lanes, each lane's fp32 sums of x - pivot sequential, the
    lanes added in order; vec = 4 fp32 / 8 bf16 elements per 16-byte vector), gn_finalize_kernel (double), gn_apply_kernel (x a + d, fp32 SiLU) before
    the output's rounding"""
    x = as_np(x, F32)
    B, HW, C = x.shape
    cpg = C // G
    ppb = gn_pix_per_block(HW)
    nchunk = (HW + ppb - 1) // ppb
    PL = 256 // (C // vec)
    K = (ppb + PL - 1) // PL
    piv = np.zeros((B, C), F32) if fault == 'raw_sums' else x[:, 0].copy()
    p = np.broadcast_to(piv[:, None], (B, nchunk * ppb, C)).copy()
    p[:, :HW] = x
    q = np.broadcast_to(piv[:, None, None], (B, nchunk, K * PL, C)).copy()
    q[:, :, :ppb] = p.reshape(B, nchunk, ppb, C)
    q = q.reshape(B, nchunk, K, PL, C)
    s, qq = np.zeros((B, nchunk, PL, C), F32), np.zeros((B, nchunk, PL, C), F32)
    for k in range(K):
        f = q[:, :, k] - piv[:, None, None]
        s, qq = s + f, qq + f * f
    if PL > 64 and PL % 4 == 0:             # four interleaved sums of the lanes
        s, qq = (t.reshape(B, nchunk, PL // 4, 4, C) for t in (s, qq))
    S, Q = np.zeros_like(s[:, :, 0]), np.zeros_like(s[:, :, 0])
    for k in range(s.shape[2]):
        S, Q = S + s[:, :, k], Q + qq[:, :, k]
    if PL > 64 and PL % 4 == 0:
        S, Q = ((t[:, :, 0] + t[:, :, 1]) + (t[:, :, 2] + t[:, :, 3]) for t in (S, Q))
    if fault == 'drop_last_chunk' and nchunk > 1:
        S[:, -1], Q[:, -1] = 0, 0
    S, Q, pv = S.astype(F64), Q.astype(F64), piv.astype(F64)
    trip = (np.arange(C) % cpg < 64) if fault == 'skip_second_trip' else np.ones(C, bool)       # the cc += 64 loops over the pivot terms stop after one trip
    n = float(HW * cpg)
    grp = lambda t: t.reshape(B, G, cpg).sum(2)
    mean = grp(S.sum(1) + HW * pv * trip) / n
    dm = pv - np.repeat(mean, cpg, 1)
    ss = grp(Q.sum(1) + 2.0 * dm * S.sum(1) + HW * dm * dm * trip)
    return _gn_apply_model(x, mean, ss, n, w, b, G, eps, silu)


def groupnorm_tiles_model(x, part, w, b, G, eps=EPS, silu=False, fault=None):
    """gn_finalize_tiles_kernel (double, every tile around its own pivot) + gn_apply_kernel<bf16>"""
    x = as_np(x, F32)
    B, HW, C = x.shape
    cpg, T = C // G, part.shape[1]
    npx = HW // T
    S, Q, pv = (part[..., i].astype(F64) for i in range(3))
    if fault == 'ignore_tile_pivots':
        pv = np.broadcast_to(pv[:, :1], pv.shape)
    n = float(HW * cpg)
    grp = lambda t: t.reshape(B, G, cpg).sum(2)
    mean = grp((npx * pv + S).sum(1)) / n
    dm = pv - np.repeat(mean, cpg, 1)[:, None]
    ss = grp((Q + 2.0 * dm * S + npx * dm * dm).sum(1))
    return _gn_apply_model(x, mean, ss, n, w, b, G, eps, silu)


GN_SHAPES = ((8, 1), (8, 8), (32, 32), (160, 32), (256, 2), (640, 32), (1024, 32), (2048, 32))      # (C, groups); 1024: fp32 only, 2048: bf16 only (C / VEC = 256)
GN_HW = (1, 31, 96, 1000, 1024, 1030, 16384, 16424)
GN_FAMILIES = ('unit', 'large_mean', 'group_means', 'outlier_pivot')
GN_B = 2
# (C, groups, HW, family): every shape at HW = 96 and 1030, every HW at C = 32, the families at (160, 32) and (256, 2) with HW = 1030
GN_CASES = _table(
    [(C, G, HW, 'unit') for C, G in GN_SHAPES for HW in (96, 1030)] +
    [(32, 32, HW, 'unit') for HW in GN_HW if HW not in (96, 1030)] +
    [(C, G, 1030, fam) for C, G in ((160, 32), (256, 2)) for fam in GN_FAMILIES[1:]] +
    [(8, 8, 96, 'large_mean'), (8, 1, 31, 'unit'), (8, 8, 1, 'unit')])
GN_ILL = ('large_mean', 'outlier_pivot')       # |mean a| >> |y| (large mean), K_g ~ 100 (outlier pivot): bounds that are large against |y| by construction


def gn_dtypes(n):
    C = GN_CASES[n][0]
    return ('f32',) if C == 1024 else (('bf16',) if C == 2048 else ('f32', 'bf16'))


def gn_name(n):
    C, G, HW, fam = GN_CASES[n]
    return f'{n}-C{C}-G{G}-HW{HW}-{fam}'


def _gn_x(g, B, HW, C, G, family):
    n = _randn(g, B, HW, C)
    if family == 'unit':
        return 1.5 * n + 0.7
    if family == 'large_mean':
        return (300.0 + 50.0 * _randn(g, B, 1, C)) + 0.05 * n
    if family == 'group_means':
        return n + 3.0 * (torch.arange(C) % (C // G)).float().view(1, 1, C) / max(1, C // G - 1) * 4
    if family == 'outlier_pivot':
        x = 1.5 * n + 0.7
        x[:, 0] = 0.7 + 15.0
        return x
    raise KeyError(family)


def gn_inputs(n, dtype):
    """-> x (B, HW, C) in the stored dtype ('f32' | 'bf16'), weight, bias (C,) fp32"""
    C, G, HW, fam = GN_CASES[n]
    g = torch.Generator().manual_seed(n)
    x = _gn_x(g, GN_B, HW, C, G, fam).to(torch.bfloat16 if dtype == 'bf16' else torch.float32)
    return x, 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C)


# (C, groups, tiles, pixels per tile, family, poor pivots) - bf16 only
GN_TILE_CASES = _table(
    [(C, G, t, p, 'unit', poor) for (C, G, t, p) in ((160, 32, 1, 96), (160, 32, 4, 256), (256, 2, 96, 8), (32, 32, 64, 256)) for poor in (False, True)] +
    [(160, 32, 4, 256, 'large_mean', False), (160, 32, 4, 256, 'group_means', False)])


def gn_tile_name(n):
    C, G, t, p, fam, poor = GN_TILE_CASES[n]
    return f'{n}-C{C}-G{G}-{t}x{p}-{fam}' + ('-poor' if poor else '')


def gn_tile_inputs(n):
    C, G, t, p, fam, poor = GN_TILE_CASES[n]
    g = torch.Generator().manual_seed(n)
    x = _gn_x(g, GN_B, t * p, C, G, fam).to(torch.bfloat16)
    return x, 1 + 0.1 * _randn(g, C), 0.1 * _randn(g, C), tile_partials(x, t, poor)
