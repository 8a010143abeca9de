"""ORACLE (test infrastructure only - never imported by the product path).

The tail of the training step: float64 oracles, float32 yardsticks, numpy models of the kernels' arithmetic, per-element bounds and the case tables
for cvar_ce_fwd_bwd, cvar_adamw, cvar_adamw_multi, cvar_sumsq, cvar_sumsq_multi, cvar_clip_coef, cvar_colsum, cvar_rowsum, cvar_wordembed_grad,
cvar_scatter_add_rows, cvar_silu_bwd, cvar_gelu, cvar_gelu_bwd and cvar_gate_residual (csrc/train.hip, rowsum_kernel in csrc/ops.hip).
tests/test_train_kernels_oracle_host.py (CPU) pins the oracles to torch in float64, shows that the models stay at <= 0.5 of every bound and that
planted faults do not; tests/test_gpu_train_kernels_oracle.py holds the kernels to the same bounds on the same operands.

Conventions.  Operands are taken AS STORED (bf16 / fp32 -> float64 is exact).  Scalar parameters are taken as the C ABI receives them: lr, betas,
eps, wd, gscale, pre_scale, max_norm are rounded to float32 first and then used in float64.  The AdamW bias corrections are float64 powers of
those float32 betas, as torch.optim.AdamW forms them.  One function serves both precisions: dtype=np.float64 is the oracle, dtype=np.float32 the
yardstick (the same formula in float32, numpy's summation).  Bounds use float64 quantities and the yardstick only, never what a kernel or a model
returned.  u = 2^-24 (half an ulp of fp32, the relative error of one correctly rounded operation; the library is built with -ffp-contract=off,
so every product and sum below is rounded on its own, `/` and sqrtf are correctly rounded).  TINY = 2^-126: a result below the smallest normal
number may be flushed.  Every bound carries the house margin 4 (tests/test_gpu_attn_train_oracle.py, oracle/norm_ref.py); a bf16 output adds
2^-8 |ref|, the worst case of its rounding.

Instruction precision, from documentation only:  __expf(a) = v_exp_f32(a log2 e): (2 |a| + 4) u relative - |a| u for the rounding of the argument
where it is a difference, |a| u for the product by log2 e, 4 u for the instruction (1 ulp) and one more ulp of allowance (oracle/sample_ref.py);
logf: 1 ulp = 2 u relative; v_rcp_f32 1 ulp (not used by these kernels: they divide).

AdamW (adamw_kernel, adamw_multi_kernel; per element, in the kernel's order)
    gs = gscale gdev          1 rounding            g' = g gs                 1        (g': 2 u relative)
    pd = p (1 - lr wd)        3 roundings: lr wd, 1 - ., the product                  -> <= 3 u |p|
    m' = b1 m + (1 - b1) g'   b1 m: 1; 1 - b1: 1; its product with g': 1 (+ 2 of g'); the sum: 1      -> <= 5 u T,  T = |b1 m| + |(1 - b1) g'|
    v' = b2 v + (1 - b2) g' g'   b2 v: 1; 1 - b2: 1; two products: 2 (+ 2 x 2 of g'); the sum: 1     -> <= 8 u v'   (every term is positive)
    den = sqrt(v') / bc2s + eps   half of v' (4), sqrtf 1, bc2s (rounded once from double) 1, `/` 1, the sum 1     -> <= 8 u den
    upd = (lr / bc1) m' / den     bc1 1, `/` 1, the product 1, `/` 1, den 8, m' 5 T / |m'|   -> <= 17 u A,  A = (lr / bc1) T / den >= |upd|
    p' = pd - upd             1 rounding            -> u |p'|
  m and v are held to their aligned worst cases: 4 x 5 u T and 4 x 8 u v'.  For p the aligned worst case u (|p'| + 3 |p| + 17 A) is NOT what is asserted:
  it needs all seventeen roundings of the update at their half ulp with one sign, and at 4 x 17 u A the bound could not see what this test exists for
  (float32 powf bias corrections at beta2 = 0.999 are 10 - 30 u of the sum below; eps on the wrong side of the correction is of the same order at
  late steps).  The bound asserted is the house unit of oracle/norm_ref.py, 2^-23 of the magnitudes that are rounded, times the margin:
      |p_kernel - p'| <= 8 u (|p'| + |p| + A)
  i.e. two aligned half-ulps on each of the three magnitudes, times 4.  Independent roundings of the seventeen give an rms of (17 / 3)^1/2 u = 2.4 u on A;
  the CPU model (every case, every element) has to stay at <= 0.5 of the bound, i.e. <= 4 u, which is what makes the cases fair.

Cross-entropy (ce_kernel: 256 lanes stride over the row, wave tree, four wave partials)
    e_v = __expf(l_v - max): relative eps_v <= (2 |l_v - max| + 4) u (+ TINY absolute: a flushed result)
    se = sum e_v: ceil(V / 256) sequential additions per lane, 6 tree levels, 2 additions of the wave partials: depth D, <= D u se on top of the terms'
    own errors:  R = sum_v e_v eps_v / se + D u + V TINY / se   is the relative error of se
    loss = (logf(se) + max) - l_tg:   R (d log) + 2 u |log se| (logf) + u |log se + max| + u |loss|   <= R + u (4 |log se| + 2 |max| + |l_tg|)
        asserted: 4 (R + u (4 |log se| + 2 |max| + |l_tg|))   (absolute: loss cancels to ~0 where the target's probability is near 1)
    dlogits_v = (e_v (1 / se) - [v = tg]) (w gscale):  p_v relative eps_v + R + 2 u (the quotient 1 / se and the product), the difference 1, w gscale 1,
        the last product 1:   4 |w gscale| (p_v (eps_v + R + 2 u) + 3 u |p_v - [v = tg]|) + 2 TINY (1 + |w gscale|)       (+ 2^-8 |ref| in bf16)
        - absolute at the target, where p - 1 cancels.

Reductions (colsum, rowsum, wordembed_grad, scatter_add_rows): out = sum of terms, accumulated in fp32 in a fixed order of depth gamma (additions that
    one term can pass through: sequential within a segment / slice / lane, then across them, then the accumulate).  Every addition rounds a partial
    sum that is at most sum |term| in size:  floor = gamma u sum |term|  per output; cancellation is priced by sum |term|, not by |ref|.
    asserted: 4 max(floor, |yardstick - oracle|).  wordembed's dW accumulates by fmaf (one rounding per token), its terms are the products.

sumsq, sumsq_multi, clip_coef (double precision): x^2 of an fp32 x is exact in double.  A partial passes ceil(n / 65536) + 8 additions; asserted
    4 (adds) 2^-53 partial.  clip_coef: ceil(count / 256) + 8 additions, sqrt, product by pre_scale (+ the sum with 1e-6 and `/`): 4 (adds + 4) 2^-53
    relative, plus the one float32 rounding u of each of the two outputs.

GELU / SiLU (c = 0.044715, k2 = 2 (2 / pi)^1/2, u2 = k2 (t + c t^3), e = __expf(-u2), sg = 1 / (1 + e))
    u2: three products and a sum inside, the product by k2, the two float32 constants: <= 7 u |u2|;  e: (2 |u2| + 4) u + 7 u |u2| = (9 |u2| + 4) u =: r_e
    gelu = t / (1 + e): the sum and `/`:  |y| ((1 - sg) r_e + 2 u)     - relative to |y| itself; in the negative tail (1 - sg) r_e ~ 9 |u2| u is all of it
    E_sg = sg ((1 - sg) r_e + 2 u);  q = 1 - sg: E_q = E_sg + u q  (absolute: q cancels where sg -> 1);  P = 1 + 3 c t^2: E_P = 4 u P
    gelu' = sg + t sg q k2 P:  E_2 = |term2| 5 u + |term2| E_sg / sg + |t sg k2 P| E_q + |term2| E_P / P;   E = E_sg + E_2 + u |gelu'|
    gelu_bwd = dh gelu':  |dh| (E + u |gelu'|) - relative to the magnitude of the TERMS: gelu' crosses zero near t = -0.75 and the bound does not
    silu' = sg (1 + x q), e = __expf(-x), r_e = (2 |x| + 4) u:  E_xq = |x| E_q + u |x q|;  r = 1 + x q: E_r = E_xq + u |r|;  E_s = |r| E_sg + sg E_r + u |s|
    silu_bwd = ds s: |ds| (E_s + u |s|)     (r crosses zero near x = -1.28)
    Every one of these adds TINY (1 + the factor a flushed sg is multiplied by); gelu also |t| 2^-128: e overflows float32 just below 2^128 and
    t / inf = 0 then misses a quotient of up to |t| 2^-128, which is a normal number for |t| > 4.  All times 4.

gate_residual: x + (g rs) f: two products and the sum: 4 u (2 |g rs f| + |x'|).
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from .norm_ref import _wave_sum, as_np, ratio_of  # noqa: F401  (ratio_of: re-exported for the tests)

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
MARGIN = 4.0
BF16_HALF_ULP = 2.0 ** -8


def f32(x):
    """a scalar as the C ABI receives it"""
    return float(F32(x))


def bf16_round(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).double().numpy()


def _table(rows):
    return {i + 1: r for i, r in enumerate(rows)}


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _store(t, dt):
    return t.to(torch.bfloat16 if dt == 'bf16' else torch.float32)


# ================================================================================================ AdamW
ADAM_K_P, ADAM_K_M, ADAM_K_V = 8.0, 20.0, 32.0
ADAM_FAULTS = ('eps_inside', 'bc2_for_sqrt', 'decay_after', 'unscaled_moment', 'powf')


def adam_corrections(b1, b2, step, mode='double'):
    """(bc1, sqrt(bc2)) as float32.  double: float64 powers of the float32 betas, rounded once (the library);  powf: the float32 form it replaced"""
    if mode == 'double':
        return F32(1.0 - f32(b1) ** step), F32(math.sqrt(1.0 - f32(b2) ** step))
    return F32(1) - np.power(F32(b1), F32(step)), np.sqrt(F32(1) - np.power(F32(b2), F32(step)))


def adamw(p, g, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, gdev=None, dtype=F64):
    """one torch.optim.AdamW step on g' = g gscale gdev -> p, m, v and the magnitudes the bounds are stated in"""
    p, g, m, v = (as_np(t, dtype) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = (dtype(f32(t)) for t in (lr, b1, b2, eps, wd))
    gs = dtype(f32(gscale)) * dtype(1.0 if gdev is None else f32(gdev))
    bc1, bc2 = dtype(1.0 - f32(b1) ** step), dtype(1.0 - f32(b2) ** step)
    gr = g * gs
    T = np.abs(b1 * m) + np.abs((1 - b1) * gr)
    mn = b1 * m + (1 - b1) * gr
    vn = b2 * v + (1 - b2) * gr * gr
    den = np.sqrt(vn) / np.sqrt(bc2) + eps
    A = (lr / bc1) * T / den
    pn = p * (1 - lr * wd) - (lr / bc1) * mn / den
    return NS(p=pn, m=mn, v=vn, A=A, T=T, p_bound=ADAM_K_P * U * (np.abs(pn) + np.abs(p) + A), m_bound=ADAM_K_M * U * T, v_bound=ADAM_K_V * U * vn)


def adamw_model(p, g, m, v, step, lr, b1, b2, eps, wd, gscale=1.0, gdev=None, fault=None):
    """adamw_kernel in float32, operation by operation"""
    p, g, m, v = (as_np(t, F32) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = (F32(t) for t in (lr, b1, b2, eps, wd))
    one = F32(1)
    bc1, bc2s = adam_corrections(b1, b2, step, 'powf' if fault == 'powf' else 'double')
    gs = F32(gscale) * (one if gdev is None else F32(gdev))
    gr = g * gs
    gm = g if fault == 'unscaled_moment' else gr
    decay = one - lr * wd
    mv = b1 * m + (one - b1) * gm
    vv = b2 * v + (one - b2) * gr * gr
    if fault == 'eps_inside':
        den = (np.sqrt(vv) + eps) / bc2s
    elif fault == 'bc2_for_sqrt':
        den = np.sqrt(vv) / (bc2s * bc2s) + eps
    else:
        den = np.sqrt(vv) / bc2s + eps
    upd = (lr / bc1) * mv / den
    pv = (p - upd) * decay if fault == 'decay_after' else p * decay - upd
    return NS(p=pv.astype(F32), m=mv.astype(F32), v=vv.astype(F32))


ADAM_N = (1, 255, 257, 10007, 4096 * 256 + 257)          # 4096 x 256 threads: the last size makes the grid-stride loop iterate
ADAM_STEPS = (1, 2, 7, 1000, 100000)
ADAM_BETAS = ((0.9, 0.95), (0.9, 0.999))
ADAM_EPS = 1e-8
# (n, step, betas, wd, lr, gdev, gscale): every step x betas at n = 10007 (wd and the device scale alternate), every n at step 7, lr = 0
ADAM_CASES = _table(
    [(10007, s, bt, (0.0, 0.05)[(i + j) % 2], 3e-3, (None, 0.5)[i % 2], (1.0, 0.25)[i % 2]) for i, s in enumerate(ADAM_STEPS) for j, bt in enumerate(ADAM_BETAS)] +
    [(n, 7, bt, 0.05, 3e-3, 0.5, 0.25) for n in ADAM_N if n != 10007 for bt in ADAM_BETAS] +
    [(10007, 7, (0.9, 0.999), 0.05, 0.0, None, 0.5), (257, 2, (0.9, 0.999), 0.0, 1e-4, 0.75, 3.0)])


def adam_name(n):
    N, step, bt, wd, lr, gdev, gs = ADAM_CASES[n]
    return f'{n}-n{N}-step{step}-b2_{bt[1]}-wd{wd}-lr{lr}-' + ('gdev' if gdev is not None else 'nodev')


def adam_values(N, step, seed):
    """p, g, m, v (fp32) in four interleaved value blocks (element i is in block (i + seed) % 4):
    0  p = 0: the update meets a single rounding        1  |p| ~ 1, moments of a run in progress
    2  gradients of the size of eps (1e-9 .. 1e-7): eps decides the quotient        3  p = g = m = v = 0: every output exactly 0
    step 1 starts from m = v = 0"""
    g_ = torch.Generator().manual_seed(7919 * seed + N % 1000)
    blk = (torch.arange(N) + seed) % 4
    p, g = _randn(g_, N), _randn(g_, N)
    m, v = 0.1 * _randn(g_, N), 0.01 * _randn(g_, N).abs()
    small = 10.0 ** (-9 + 2 * torch.rand(N, generator=g_))
    g = torch.where(blk == 2, g.sign() * small, g)
    m = torch.where(blk == 2, m * small * 10, m)
    v = torch.where(blk == 2, small * small * (0.5 + v * 100), v)
    p = torch.where((blk == 0) | (blk == 3), torch.zeros(()), p)
    z = blk == 3
    g, m, v = (torch.where(z, torch.zeros(()), t) for t in (g, m, v))
    if step == 1:
        m, v = torch.zeros(N), torch.zeros(N)
    return p, g, m, v, blk.numpy()


def adam_inputs(n):
    N, step = ADAM_CASES[n][:2]
    return adam_values(N, step, n)


def adam_args(n):
    """keyword arguments of adamw / adamw_model for case n"""
    N, step, bt, wd, lr, gdev, gs = ADAM_CASES[n]
    return dict(step=step, lr=lr, b1=bt[0], b2=bt[1], eps=ADAM_EPS, wd=wd, gscale=gs, gdev=gdev)


# multi-tensor tables: (sizes, group of each tensor, lr by group, wd by group, tensors with a bf16 copy)
ADAM_MULTI = {
    'six': ((1, 7, 32768, 32769, 70001, 300), (0, 1, 2, 0, 1, 2), (3e-3, 1e-3, 5e-4), (0.05, 0.0, 0.1), (2, 4)),       # 128 x 256 threads: 32769 and 70001 iterate
    'eight_groups': ((300,) * 8, tuple(range(8)), tuple(1e-3 * (k + 1) for k in range(8)), tuple(0.02 * k for k in range(8)), (1, 6)),
}
ADAM_MULTI_ARGS = dict(step=7, b1=0.9, b2=0.999, eps=ADAM_EPS, gscale=0.25, gdev=0.5)


def adam_multi_inputs(name):
    sizes = ADAM_MULTI[name][0]
    return [adam_values(N, 7, 100 + 10 * i + len(sizes))[:4] for i, N in enumerate(sizes)]


# ================================================================================================ sumsq / clip_coef
def _sumsq_layout(x):
    """x^2 (exact in double) as (K, 256 blocks, 256 threads): element i belongs to block (i // 256) % 256, thread i % 256, trip i // 65536"""
    x = as_np(x)
    K = max(1, -(-x.size // 65536))
    sq = np.zeros(K * 65536)
    sq[:x.size] = x * x
    return sq.reshape(K, 256, 256)


def sumsq(x):
    """-> the 256 partials (extended-precision sums of exact squares), their bound, the number of additions"""
    sq = _sumsq_layout(x)
    part = sq.astype(np.longdouble).sum((0, 2)).astype(F64)
    adds = sq.shape[0] + 8
    return NS(partial=part, bound=MARGIN * adds * 2.0 ** -53 * part, adds=adds)


def _tree256(a):
    """(.., 256) thread values -> block value: shuffle tree per wave, then (w0 + w1) + (w2 + w3)"""
    w = [_wave_sum(a[..., 64 * k:64 * k + 64].reshape(-1, 64)).reshape(a.shape[:-1]) for k in range(4)]
    return (w[0] + w[1]) + (w[2] + w[3])


def sumsq_model(x):
    sq = _sumsq_layout(x)
    a = np.zeros(sq.shape[1:])
    for k in range(sq.shape[0]):
        a = a + sq[k]
    return _tree256(a)


SUMSQ_CASES = _table([(1, 'unit'), (255, 'unit'), (255, 'wide'), (65536, 'unit'), (65537, 'unit'), (200003, 'unit'), (200003, 'wide')])


def sumsq_inputs(n):
    N, fam = SUMSQ_CASES[n]
    g = torch.Generator().manual_seed(300 + n)
    x = _randn(g, N)
    if fam == 'wide':       # magnitudes 1e-25 .. 1e25: the squares leave float32 on both sides
        x = x.sign() * 10.0 ** (-25 + 50 * torch.rand(N, generator=g))
    return x.float()


CLIP_FAULTS = ('no_1e6', 'pre_scale_inside')


def _clip_bound_rel(count):
    return MARGIN * (-(-count // 256) + 8 + 4) * 2.0 ** -53 + U


def clip_coef(partials, count, pre_scale, max_norm):
    """-> norm = pre_scale sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)) (1 for max_norm <= 0) in float64, and their bounds"""
    total = float(as_np(partials)[:count].astype(np.longdouble).sum())
    ps, mn = f32(pre_scale), f32(max_norm)
    nrm = math.sqrt(total) * ps
    raw = mn / (nrm + 1e-6) if mn > 0 else 2.0
    rel = _clip_bound_rel(count)
    # a quotient that is clearly above 1 is clamped: the coefficient is then exactly 1
    return NS(norm=nrm, coef=min(1.0, raw), norm_bound=rel * nrm, coef_bound=0.0 if raw > 1 + 1e-9 else rel * min(1.0, raw))


def clip_coef_model(partials, count, pre_scale, max_norm, fault=None):
    """clip_coef_kernel: 256 lanes stride over the partials in double, shuffle tree, (w0 + w1) + (w2 + w3); the two outputs rounded to float32"""
    K = -(-count // 256)
    pad = np.zeros(K * 256)
    pad[:count] = as_np(partials)[:count]
    a = np.zeros(256)
    for k in range(K):
        a = a + pad[k * 256:(k + 1) * 256]
    total = float(_tree256(a[None])[0])
    ps, mn = f32(pre_scale), f32(max_norm)
    nrm = math.sqrt(total * ps) if fault == 'pre_scale_inside' else math.sqrt(total) * ps
    coef = min(1.0, mn / (nrm + (0.0 if fault == 'no_1e6' else 1e-6))) if mn > 0 else 1.0
    return NS(norm=float(F32(nrm)), coef=float(F32(coef)), norm64=nrm, coef64=coef)


CLIP_COUNTS = (1, 255, 256, 257, 6 * 256)
# (count, pre_scale, max_norm, kind).  kind: size of the partials - mid (norm a few times max_norm), below (norm < max_norm: the coefficient is exactly 1),
# huge (norm >> max_norm), zero (norm = 0)
CLIP_CASES = _table([(c, ps, mn, kind) for i, c in enumerate(CLIP_COUNTS) for j, ps in enumerate((1.0, 0.5, 0.125)) for mn in (0.0, -1.0, 2.0)
                     for kind in (('mid', 'below', 'huge', 'zero')[(i + j) % 4],)] +
                    [(c, 1.0, 2.0, kind) for c in (257, 1536) for kind in ('mid', 'below', 'huge', 'zero')])


def clip_inputs(n):
    c, ps, mn, kind = CLIP_CASES[n]
    g = torch.Generator().manual_seed(500 + n)
    scale = {'mid': 40.0 / c, 'below': 1e-4 / c, 'huge': 1e12 / c, 'zero': 0.0}[kind]
    return (torch.rand(c, generator=g, dtype=torch.float64) + 0.5) * scale


# ================================================================================================ cross-entropy
CE_FAULTS = ('inv_before_last_partial', 'onehot_unweighted')
CE_V = (2, 63, 255, 256, 257, 4096, 4099)
CE_FAMILIES = ('normal', 'spread200', 'offset1e4', 'equal', 'dominant', 'neginf8')
CE_WEIGHTS = ('none', 'zero', 'mixed')
CE_M = 5
# (V, family, weight kind, gscale): every V x family; the weight kind and gscale go round
CE_CASES = _table([(V, fam, CE_WEIGHTS[(i + j) % 3], (1.0, 1.0 / 37)[(i + j) % 2]) for i, V in enumerate(CE_V) for j, fam in enumerate(CE_FAMILIES)])


def ce_name(n):
    V, fam, wk, gs = CE_CASES[n]
    return f'{n}-V{V}-{fam}-w_{wk}-gs{gs:.3f}'


def ce_inputs(n):
    """-> logits (5, V) fp32, target (5,) int32 at 0, V - 1, the arg-max, the arg-min and one more, weight (5,) or None, gscale"""
    V, fam, wk, gs = CE_CASES[n]
    g = torch.Generator().manual_seed(700 + n)
    M = CE_M
    z = _randn(g, M, V)
    if fam == 'normal':
        lg = 3.0 * z
    elif fam == 'spread200':
        lg = 200.0 * torch.rand(M, V, generator=g) - 100.0
    elif fam == 'offset1e4':
        lg = 1e4 + z
    elif fam == 'equal':
        lg = torch.full((M, V), 0.75)
    elif fam == 'dominant':
        lg = z.clone()
        for m in range(M):
            lg[m, (7 * m + 3) % V] = 40.0
    else:
        lg = torch.full((M, V), float('-inf'))
        for m in range(M):
            keep = torch.randperm(V, generator=g)[:min(8, V)]
            lg[m, keep] = 3.0 * z[m, keep]
    lg = lg.float()
    tgt = torch.tensor([0, V - 1, int(lg[2].argmax()), int(lg[3].argmin()), (3 * n + 1) % V], dtype=torch.int32)
    w = {'none': None, 'zero': torch.zeros(M), 'mixed': torch.tensor([1.0, 0.0, 0.37, 2.5, 0.0])}[wk]
    return lg, tgt, w, gs


def _ce_depth(V):
    return -(-V // 256) + 8


def ce(logits, target, weight, gscale, dtype=F64):
    """loss_tok = logsumexp - l_tg, dlogits = (softmax - onehot) w gscale, and the bounds (float64 only)"""
    l = as_np(logits, dtype)
    M, V = l.shape
    tg = as_np(target, np.int64)
    w = (np.ones(M, dtype) if weight is None else as_np(weight, dtype)) * dtype(f32(gscale))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        mx = l.max(1, keepdims=True)
        d = l - mx
        e = np.exp(d)
        se = e.sum(1, dtype=dtype, keepdims=True)
        lse = np.log(se) + mx
        ltg = l[np.arange(M), tg]
        loss = lse[:, 0] - ltg
        p = e / se
        hot = np.zeros((M, V), dtype)
        hot[np.arange(M), tg] = 1
        dl = (p - hot) * w[:, None]
        out = NS(loss=loss, dlogits=dl, p=p)
        if dtype is F64:
            eps_v = np.where(np.isfinite(d), (2 * np.abs(d) + 4) * U, 0.0)
            R = (e * eps_v).sum(1, keepdims=True) / se + _ce_depth(V) * U + V * TINY / se
            fin = np.where(np.isfinite(ltg), np.abs(ltg), 0.0)
            out.loss_bound = MARGIN * (R[:, 0] + U * (4 * np.abs(np.log(se[:, 0])) + 2 * np.abs(mx[:, 0]) + fin))
            aw = np.abs(w)[:, None]
            out.dl_bound = MARGIN * aw * (p * (eps_v + R + 2 * U) + 3 * U * np.abs(p - hot)) + 2 * TINY * (1 + aw)
            out.R = R[:, 0]
    return out


def ce_model(logits, target, weight, gscale, fault=None):
    """ce_kernel in float32: lane v % 256 accumulates its elements in order, shuffle tree per wave, (w0 + w1) + (w2 + w3); lanes past V add 0"""
    l = as_np(logits, F32)
    M, V = l.shape
    tg = as_np(target, np.int64)
    K = -(-V // 256)
    pad = np.full((M, K * 256), -np.inf, F32)
    pad[:, :V] = l
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        mx = pad.max(1, keepdims=True)
        e = np.exp(pad - mx).astype(F32)
        a = np.zeros((M, 256), F32)
        for k in range(K):
            a = a + e[:, k * 256:(k + 1) * 256]
        w4 = [_wave_sum(a[:, 64 * k:64 * k + 64]) for k in range(4)]
        se = (w4[0] + w4[1]) + (w4[2] + w4[3])
        ltg = l[np.arange(M), tg]
        loss = (np.log(se).astype(F32) + mx[:, 0]) - ltg
        w = (np.ones(M, F32) if weight is None else as_np(weight, F32)) * F32(gscale)
        inv = F32(1) / ((w4[0] + w4[1]) + w4[2] if fault == 'inv_before_last_partial' else se)
        pr = e[:, :V] * inv[:, None]
        hot = np.zeros((M, V), F32)
        hot[np.arange(M), tg] = 1
        dl = pr * w[:, None] - hot if fault == 'onehot_unweighted' else (pr - hot) * w[:, None]
    return NS(loss=loss.astype(F32), dlogits=dl.astype(F32))


def abs_err(got, ref):
    """|got - ref| where equal infinities (a target on a -inf logit has an infinite loss) count as 0 and NaN as infinite"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    with np.errstate(invalid='ignore'):
        e = np.where(got == ref, 0.0, np.abs(got - ref))
    return np.where(np.isnan(e), np.inf, e)


# ================================================================================================ reductions
def reduction_bound(ref, yard, abs_terms, gamma):
    floor = gamma * U * abs_terms
    yd = np.abs(yard - ref)
    return NS(floor=floor, yard=yd, bound=MARGIN * np.maximum(floor, yd))


# ---- colsum
def colsum_segments(M):
    nseg = min(64, max(1, M // 64))
    return nseg, -(-M // nseg)


def colsum(A, out0=None, dtype=F64):
    """out[n] = (out0[n] +) sum_m A[m, n]"""
    A = as_np(A, dtype)
    s = A.sum(0, dtype=dtype)
    return s if out0 is None else as_np(out0, dtype) + s


def colsum_model(A, out0=None, fault=None):
    """colsum_kernel / colsum_vec_kernel (the same order per column) + colsum_finalize_kernel"""
    A = as_np(A, F32)
    M, N = A.shape
    nseg, seg = colsum_segments(M)
    part = np.zeros((nseg, N), F32)
    for s in range(nseg):
        m0, m1 = s * seg, min(M, s * seg + seg)
        if fault == 'drop_last_row':
            m1 -= 1
        for m in range(m0, m1):
            part[s] = part[s] + A[m]
    a = np.zeros(N, F32)
    for s in range(nseg):
        a = a + part[s]
    return a if out0 is None else as_np(out0, F32) + a


def colsum_bound(A, out0, ref, yard):
    M = A.shape[0]
    nseg, seg = colsum_segments(M)
    terms = np.abs(as_np(A)).sum(0) + (0.0 if out0 is None else np.abs(as_np(out0)))
    return reduction_bound(ref, yard, terms, seg + nseg + (out0 is not None))


COLSUM_M = (1, 63, 64, 65, 127, 128, 4095, 4097)
# (form, M, N, family).  f32: colsum_kernel<float>; vec: colsum_vec_kernel; off: the same bf16 values one element off a 16-byte boundary (odd a_off) and
# odd: N % 8 != 0 - both colsum_kernel<bf16>.  lda = N + 24 (+ 1 for odd N in bf16 keeps nothing aligned on purpose), accumulate on the even cases
COLSUM_CASES = _table([(form, M, N, ('unit', 'offset')[(i + j) % 2]) for i, M in enumerate(COLSUM_M) for j, (form, N) in enumerate((('f32', 200), ('vec', 264), ('off', 264)))] +
                      [('f32', 127, 1, 'unit'), ('odd', 127, 1, 'unit'), ('f32', 127, 8, 'offset'), ('vec', 127, 8, 'unit'), ('f32', 4097, 520, 'unit'),
                       ('vec', 4097, 520, 'offset'), ('odd', 4097, 203, 'offset'), ('vec', 128, 200, 'unit')])


def colsum_name(n):
    form, M, N, fam = COLSUM_CASES[n]
    return f'{n}-{form}-M{M}-N{N}-{fam}'


def colsum_layout(n):
    """-> lda, a_off, out_off, accumulate"""
    form, M, N, fam = COLSUM_CASES[n]
    return N + 24, 9 if form == 'off' else 8, 5, n % 2 == 0


def colsum_inputs(n):
    """-> A (M, N) in the stored dtype, out0 (N,) fp32.  'off' cases carry the values of the 'vec' case before them"""
    form, M, N, fam = COLSUM_CASES[n]
    g = torch.Generator().manual_seed(900 + (n - 1 if form == 'off' else n))
    A = _randn(g, M, N)
    if fam == 'offset':
        A = 1e4 + A
    return _store(A, 'f32' if form == 'f32' else 'bf16'), _randn(g, N)


# ---- rowsum
def rowsum(A, out0=None, dtype=F64):
    A = as_np(A, dtype)
    s = A.sum(1, dtype=dtype)
    return s if out0 is None else as_np(out0, dtype) + s


def rowsum_model(A, vec, out0=None):
    """rowsum_kernel: lane L adds the `vec` elements of the 16-byte vectors L, L + 64, .. in order, then the tail elements, then the shuffle tree"""
    A = as_np(A, F32)
    R, n = A.shape
    nv = n // vec
    a = np.zeros((R, 64), F32)
    for i0 in range(0, nv, 64):
        blk = np.zeros((R, 64, vec), F32)
        k = min(64, nv - i0)
        blk[:, :k] = A[:, i0 * vec:(i0 + k) * vec].reshape(R, k, vec)
        for e in range(vec):
            a = a + blk[:, :, e]
    for j0 in range(nv * vec, n, 64):
        t = np.zeros((R, 64), F32)
        k = min(64, n - j0)
        t[:, :k] = A[:, j0:j0 + k]
        a = a + t
    s = _wave_sum(a)
    return s if out0 is None else as_np(out0, F32) + s


def rowsum_bound(A, vec, out0, ref, yard):
    n = A.shape[1]
    nv = n // vec
    gamma = -(-nv // 64) * vec + -(-(n - nv * vec) // 64) + 6 + (out0 is not None)
    return reduction_bound(ref, yard, np.abs(as_np(A)).sum(1) + (0.0 if out0 is None else np.abs(as_np(out0))), gamma)


ROWSUM_NCOLS = (1, 3, 4, 7, 8, 255, 256, 257, 1000, 4097)
ROWSUM_CASES = _table([(dt, (1, 3, 4, 5)[(i + j) % 4], nc) for j, dt in enumerate(('f32', 'bf16')) for i, nc in enumerate(ROWSUM_NCOLS)])


def rowsum_inputs(n):
    dt, R, nc = ROWSUM_CASES[n]
    g = torch.Generator().manual_seed(1100 + n)
    return _store(_randn(g, R, nc) + (0.5 if n % 3 == 0 else 0.0), dt), _randn(g, R)


def rowsum_lda(n):
    dt, R, nc = ROWSUM_CASES[n]
    q = 4 if dt == 'f32' else 8
    return (nc + 8 + q - 1) // q * q


# ---- wordembed_grad
def wordembed_slices(ntok):
    nslice = 32 if ntok >= 32768 else (16 if ntok >= 4096 else (4 if ntok >= 256 else 1))
    return nslice, -(-ntok // nslice)


def _we_rows(B, n, rows, skip):
    t = np.arange(B * n)
    return (t // n) * rows + skip + t % n


def wordembed(dx, tok, B, n, rows, skip, dtype=F64):
    """dW[c][j] = sum_t dX[row(t)][c] tok[t][j], db[c] = sum_t dX[row(t)][c] over the B n word-embedded rows; and sum |term| of both"""
    X = as_np(dx, dtype)[_we_rows(B, n, rows, skip)]
    tk = as_np(tok, dtype)
    out = NS(dW=(X.T @ tk).astype(dtype), db=X.sum(0, dtype=dtype))
    if dtype is F64:
        out.abs_W, out.abs_b = np.abs(X).T @ np.abs(tk), np.abs(X).sum(0)
    return out


def wordembed_model(dx, tok, B, n, rows, skip, fault=None):
    """wordembed_grad_kernel (fmaf over the slice's tokens in order; the bias by plain additions) + wordembed_grad_reduce_kernel (slices in order)"""
    ntok = B * n
    nslice, per = wordembed_slices(ntok)
    t = np.arange(ntok)
    row = _we_rows(B, n, rows, skip)
    if fault == 'no_skip_after_first_sample':          # the row pointer of a slice forgets `skip` once it has crossed into its next sample
        first = (t // per * per) // n
        row = np.where(t // n > first, row - skip, row)
    X = np.zeros((nslice * per, dx.shape[1]), F32)
    X[:ntok] = as_np(dx, F32)[row]
    tk = np.zeros((nslice * per, 32), F32)
    tk[:ntok] = as_np(tok, F32)
    X, tk = X.reshape(nslice, per, -1), tk.reshape(nslice, per, 32)
    acc = np.zeros((nslice, X.shape[2], 32), F32)
    accb = np.zeros((nslice, X.shape[2]), F32)
    for k in range(per):
        acc = (X[:, k, :, None].astype(F64) * tk[:, k, None, :].astype(F64) + acc).astype(F32)       # fmaf: the product is exact in double
        accb = accb + X[:, k]
    W, b = acc[0], accb[0]
    for s in range(1, nslice):
        W, b = W + acc[s], b + accb[s]
    return NS(dW=W, db=b)


# (B, n per sample, skip, C): tokens 255 | 256 (1 | 4 slices), 4095 | 4096 (4 | 16), 32767 | 32768 (16 | 32); a slice holds more than one sample or ends inside one
WE_CASES = _table([(3, 85, 2, 64), (8, 32, 0, 192), (5, 819, 2, 192), (32, 128, 0, 64), (31, 1057, 2, 64), (128, 256, 2, 192)])


def we_name(n):
    B, npr, skip, C = WE_CASES[n]
    return f'{n}-B{B}xn{npr}-tok{B * npr}-skip{skip}-C{C}'


def we_layout(n):
    """-> rows per sample (> skip + n), ldx (> C)"""
    B, npr, skip, C = WE_CASES[n]
    return skip + npr + 1, C + 4


def we_inputs(n):
    """-> dx (B rows, C) fp32 (rows outside the word-embedded ones included: the test makes them NaN on the device), tok (B n, 32)"""
    B, npr, skip, C = WE_CASES[n]
    g = torch.Generator().manual_seed(1300 + n)
    return _randn(g, B * we_layout(n)[0], C), _randn(g, B * npr, 32)


def we_bounds(n, ex, y32):
    B, npr, skip, C = WE_CASES[n]
    nslice, per = wordembed_slices(B * npr)
    return reduction_bound(ex.dW, y32.dW, ex.abs_W, per + nslice), reduction_bound(ex.db, y32.db, ex.abs_b, per + nslice)


# ---- scatter_add_rows
SCATTER_IDX = (3, 1, 3, 0, 3, 5, 5, 1, 3)
SCATTER_ROWS = 7
SCATTER_C = (1, 255, 257)


def scatter_inputs(C):
    g = torch.Generator().manual_seed(1500 + C)
    return _randn(g, len(SCATTER_IDX), C), _randn(g, SCATTER_ROWS, C)


def scatter_add(src, dst0, idx=SCATTER_IDX, dtype=F64):
    out = as_np(dst0, dtype).copy()
    s = as_np(src, dtype)
    for i, r in enumerate(idx):         # in order, one addition each: this IS the kernel's order in float32
        out[r] = out[r] + s[i]
    return out


def scatter_bound(src, dst0, ref, yard, idx=SCATTER_IDX):
    terms, hits = np.abs(as_np(dst0)).copy(), np.zeros(dst0.shape[0])
    for i, r in enumerate(idx):
        terms[r] += np.abs(as_np(src)[i])
        hits[r] += 1
    return reduction_bound(ref, yard, terms, hits[:, None])


# ================================================================================================ GELU / SiLU / gate_residual
GELU_C, GELU_C3 = 0.044715, 0.134145
GELU_K2 = 2.0 * math.sqrt(2.0 / math.pi)
ACT_SPECIALS = (20.0, -20.0, 88.0, -88.0, 0.0, -0.0, 1e-30, -0.7524614, -1.2784645)
ACT_FAULTS = ('gelu_c3', 'silu_no_one')
GELU_EDGE, SILU_EDGE = 8192 * 256, 2048 * 256             # threads of the largest grid: three elements more make the grid-stride loop iterate
ACT_N = (1, 257)


def act_inputs(n, dt, seed=0):
    """-> a (n,) in the stored dtype: the specials, then a dense sweep of [-12, 12]; upstream gradient (n,)"""
    k = len(ACT_SPECIALS)
    a = torch.tensor([-0.75]) if n == 1 else torch.cat([torch.tensor(ACT_SPECIALS), torch.linspace(-12, 12, n - k)])
    g = torch.Generator().manual_seed(1700 + seed + n % 1000)
    return _store(a.float(), dt), _store(_randn(g, n), dt)


def _sig_parts(u2, r_e):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        e = np.exp(-u2)
        sg = 1.0 / (1.0 + e)
        q = e / (1.0 + e)              # 1 - sg without its cancellation
    q = np.where(np.isfinite(e), q, 1.0)
    E_sg = sg * (q * r_e + 2 * U)
    return sg, q, E_sg, E_sg + U * q


def gelu(a, dh=None, dtype=F64, c3=GELU_C3):
    """gelu(tanh form) = a sigmoid(2 u), its derivative, dh gelu' and the bounds of all three"""
    t = as_np(a, dtype)
    if dtype is F32:
        k2, c, c3 = F32(GELU_K2), F32(GELU_C), F32(c3)
        with np.errstate(over='ignore', under='ignore'):
            sg = F32(1) / (F32(1) + np.exp(-(k2 * (t + c * t * t * t))))
            gp = sg + t * sg * (F32(1) - sg) * k2 * (F32(1) + c3 * t * t)
        return NS(y=t * sg, grad=gp, dy=None if dh is None else as_np(dh, F32) * gp)
    u2 = GELU_K2 * (t + GELU_C * t ** 3)
    r_e = (9 * np.abs(u2) + 4) * U
    sg, q, E_sg, E_q = _sig_parts(u2, r_e)
    y = t * sg
    P = 1 + c3 * t * t
    t2 = t * sg * q * GELU_K2 * P
    gp = sg + t2
    fac = np.abs(t * GELU_K2 * P)
    E_gp = E_sg + np.abs(t2) * 9 * U + fac * (q * E_sg + sg * E_q) + U * np.abs(gp)
    out = NS(y=y, grad=gp, y_bound=MARGIN * (np.abs(y) * (q * r_e + 2 * U) + TINY + np.abs(t) * 2.0 ** -128))
    if dh is not None:
        d = as_np(dh)
        out.dy = d * gp
        out.dy_bound = MARGIN * (np.abs(d) * (E_gp + U * np.abs(gp)) + TINY * (1 + np.abs(d) * (1 + fac)))
    return out


def gelu_model(a, dh=None, fault=None):
    return gelu(a, dh, dtype=F32, c3=GELU_C if fault == 'gelu_c3' else GELU_C3)


def silu_bwd(x, ds, dtype=F64, fault=None):
    """ds silu'(x), silu'(x) = sg (1 + x (1 - sg))"""
    x, ds = as_np(x, dtype), as_np(ds, dtype)
    if dtype is F32:
        with np.errstate(over='ignore', under='ignore'):
            sg = F32(1) / (F32(1) + np.exp(-x))
        r = x * (F32(1) - sg) if fault == 'silu_no_one' else F32(1) + x * (F32(1) - sg)
        return NS(dx=ds * (sg * r))
    r_e = (2 * np.abs(x) + 4) * U
    sg, q, E_sg, E_q = _sig_parts(x, r_e)
    xq = x * q
    r = 1 + xq
    s = sg * r
    E_r = np.abs(x) * E_q + U * np.abs(xq) + U * np.abs(r)
    E_s = np.abs(r) * E_sg + sg * E_r + U * np.abs(s)
    return NS(dx=ds * s, grad=s, bound=MARGIN * (np.abs(ds) * (E_s + U * np.abs(s)) + TINY * (1 + np.abs(ds) * (1 + np.abs(x)))))


def silu_bwd_model(x, ds, fault=None):
    return silu_bwd(x, ds, dtype=F32, fault=fault)


def gate_residual(x, f, gate, rowscale, gate_rows, dtype=F64):
    """x + (gate[m // gate_rows] rowscale[m // gate_rows]) f, and its bound 4 u (2 |g rs f| + |x'|)"""
    x, f, gate = as_np(x, dtype), as_np(f, dtype), as_np(gate, dtype)
    r = np.arange(x.shape[0]) // gate_rows
    g = gate[r] if rowscale is None else gate[r] * as_np(rowscale, dtype)[r, None]
    y = x + g * f
    return NS(y=y, bound=MARGIN * U * (2 * np.abs(g * f) + np.abs(y)) if dtype is F64 else None)


# (dtype of f, rowscale given, gate_rows, C, M): the last shape passes 8192 x 256 float4 groups (the grid-stride loop iterates)
GR_CASES = _table([(dt, rs, gr, C, 21) for dt in ('f32', 'bf16') for rs in (False, True) for gr in (1, 7) for C in (4, 132)] +
                  [('bf16', True, 7, 132, 63553)])


def gr_name(n):
    dt, rs, gr, C, M = GR_CASES[n]
    return f'{n}-{dt}-' + ('rs-' if rs else 'nors-') + f'rows{gr}-C{C}-M{M}'


def gr_inputs(n):
    """-> x (M, C), f (M, C) stored dtype, gate (R, C), rowscale (R,) or None"""
    dt, rs, gr, C, M = GR_CASES[n]
    g = torch.Generator().manual_seed(1900 + n)
    R = -(-M // gr)
    return _randn(g, M, C), _store(_randn(g, M, C), dt), 0.4 * _randn(g, R, C) + 1, (torch.tensor([(1.0, 0.0, 1.25)[r % 3] for r in range(R)]) if rs else None)
