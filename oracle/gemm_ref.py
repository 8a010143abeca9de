"""ORACLE (test infrastructure only - never imported by the product path; numpy only, nothing from the library).

cvar_gemm (csrc/gemm.hip, gemm_skinny.hip, gemm_params.h), plain GEMM, per element against float64:

    C[row(m), n] = cast( residual + gate[m // gate_rows] * gate_scale[m // gate_rows] * act( alpha * sum_k A[m,k] W[n,k] + bias[n] ) )

reference(case)  float64 value of everything one call writes: C (as [batch][M][N - split_n]; rows(case) maps m to the remapped row), C_split, pre_act
bound(case)      per-element bound of |kernel - reference|, by forward error analysis along the same chain (below)
model(case)      the kernels' arithmetic in numpy float32, in their operation order, with optional planted faults (tests/test_gemm_oracle_host.py)
CASES            the case table both tests share: operands, flags, seed and the route (kernel + epilogue implementation) a case is meant to reach

Conventions.  Operands are taken AS STORED (bf16 / fp32 -> float64 is exact); alpha and split_alpha as the C ABI receives them (float32).  u = 2^-24,
the relative error of one correctly rounded fp32 operation (the library is built with -ffp-contract=off: every product and sum rounds on its own).
The product term and the function terms (GELU, GELU') are worst cases of many roundings that cannot all align; they carry no margin.  A single
epilogue rounding (alpha, bias, split_alpha, gate, residual) is priced at one ulp, 2 u (|value| + E) with E the bound carried so far - the house unit
2^-23 of oracle/norm_ref.py: where one of them is all that separates an output from float64 (a gate near 0 in front of the residual add) a correct
kernel's error reaches u |value| itself, and the host test asks that a correct model stays at half the bound.

Product.  s = sum_k A W in float64, S = sum_k |A| |W|.
  bf16 operands: every product is exact in fp32.  v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16 update an accumulator once per 16 k (32 k); the sum inside
      the instruction is treated as tests/x3_ref.depth treats it (the term test_split_product_through_gemm_against_float64 holds the kernels to
      on hardware): one rounding per update, K / 16 of them, plus up to 16 for the sum inside an instruction; the split-K reduction adds at most
      16 slices, the weight-streaming kernel 8 wave partials:                                        depth = ceil(K / 16) + 16 + 16 + 8
  fp32 operands: v_mfma_f32_32x32x2f32 - the product and the add each round (a fused form rounds less):  depth = 2 K + 16   (16 split-K slices)
  every rounding is <= u of a partial sum, itself <= (1 + 2^-7) S:         E_acc = depth u (1 + 2^-7) S
Epilogue, in the kernels' order (each line: propagated bound + own roundings)
  x = alpha s          |alpha| E_acc + 2 u |x|               (one product; alpha = 1 multiplies exactly but is priced all the same)
  x += bias            E + 2 u |x|
  pre_act = x          stored in the operand dtype: E (+ the store term)
  x *= split_alpha     |split_alpha| E + 2 u |x|             (split columns only; 0 is read as 1)
  gelu(x)              1.13 E + |y| ((1 - sg) r_e + 5 u) + TINY:  |gelu'| <= 1.13 everywhere (its maximum is 1.129 at t = 1.46), so the incoming bound
                       passes through the function at that Lipschitz constant.  Own terms cover both forms: gelu_tanh_f  t / (1 + __expf(-u2)) and
                       gelu_tanh_fast  t * v_rcp_f32(1 + v_exp_f32(arg)).  u2 = k2 (t + c t^3) resp. arg = t (c1 + c3 t^2): <= 7 roundings, constants
                       included -> 7 u |u2| on the exponent; __expf / v_exp_f32: (2 |u2| + 4) u (argument scaling, 1 ulp, 1 ulp allowance:
                       oracle/train_kernels_ref.py) -> r_e = (9 |u2| + 4) u relative on e, which reaches y through (1 - sg); the sum 1 + e (u), the
                       division (u) or v_rcp_f32 (1 ulp = 2 u) and the product (u): <= 5 u |y|.
  x *= gelu'(aux)      aux is a stored operand (exact).  E_gp as derived in oracle/train_kernels_ref.py (gelu_tanh_grad: __expf, one division):
                       E_sg = sg ((1 - sg) r_e + 2 u), E_q = E_sg + u q, gelu' = sg + t2, t2 = t sg q k2 (1 + 3 c t^2):
                       E_gp = E_sg + 9 u |t2| + |t k2 P| (q E_sg + sg E_q) + u |gelu'|;   product: |gelu'| E + (|x| + E) E_gp + 2 u |x gelu'|
  x *= g gs            g gs rounds once where gate_scale is given (E_G = u |g gs|):  |G| E + (|x| + E) E_G + 2 u |x G|
  x += residual        E + 2 u |x|
  store                fp32: exact.  bf16 (C, C_split, pre_act): round to nearest even, half an ulp of the binade of |value| + E:
                       + 2^-9 * 2^(floor(log2(|value| + E)) + 1).  (The first form of this term, 2^-9 |value|, miscounted the rounding: bf16 keeps 8
                       significant bits, so an ulp is 2^-7 of the binade's LOWER end and half of it reaches 2^-8 |value| there - 1 + 2^-8 is a tie
                       that goes to 1.  2^-9 holds relative to the binade's upper end, which is how the term is written now; it is never more than
                       2^-8 |value| and equals 2^-9 |value| at the top of a binade.)
A bf16 output's store term is the worst case of its rounding, so ratios of bf16 tensors sit near 1 by construction; the host test therefore holds the
model BEFORE that rounding to 0.5 of the bound without the term and the rounded model to the whole bound (as test_train_kernels_oracle_host.py does).
"""
from __future__ import annotations

import math
from types import SimpleNamespace as NS

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
TINY = 2.0 ** -126
BF16_STORE = 2.0 ** -9
ACT_NONE, ACT_GELU, ACT_GELU_GRAD = 0, 1, 2
GELU_C, GELU_C3 = 0.044715, 0.134145
GELU_K2 = 2.0 * math.sqrt(2.0 / math.pi)
GELU_LIP = 1.13


# ================================================================================================ number formats
def bf16_bits(x):
    """fp32 -> the 16 bits of bf16(x), round to nearest even, in uint32 arithmetic (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)


def bf16_value(bits16):
    return (np.asarray(bits16, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def bf16_round(x):
    return bf16_value(bf16_bits(x))


def bf16_trunc(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return (u & np.uint32(0xFFFF0000)).view(F32)


def bf16_half_ulp(mag):
    """half an ulp of bf16 in the binade of `mag` (float64, > 0): 2^-9 of the binade's upper end"""
    mag = np.maximum(np.asarray(mag, F64), TINY)
    return BF16_STORE * np.exp2(np.floor(np.log2(mag)) + 1)


def stored(x, dt):
    """values as a tensor of dtype `dt` holds them, as float32"""
    x = np.asarray(x, dtype=F32)
    return bf16_round(x) if dt == 'bf16' else x


def abs_err(got, ref):
    """|got - ref|; NaN (in either, unless both are NaN: an element nobody owns) counts as infinite"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    with np.errstate(invalid='ignore'):
        e = np.where(got == ref, 0.0, np.abs(got - ref))
    e = np.where(np.isnan(got) & np.isnan(ref), 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


def ratio_of(err, bound):
    """max over the elements of error / bound; 0 / 0 (an element that must be exact and is) counts as 0"""
    err, bound = np.broadcast_arrays(np.abs(err), np.nan_to_num(np.asarray(bound, F64), nan=0.0))
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    return float(r.max()) if r.size else 0.0


def outside_share(err, bound):
    err, bound = np.broadcast_arrays(np.abs(err), np.nan_to_num(np.asarray(bound, F64), nan=0.0))
    return float(np.mean(err > bound)) if err.size else 0.0


# ================================================================================================ cases
_DEFAULTS = dict(dt='bf16', out=None, seed=0, lda=0, ldc=0, tile_cfg=0, small_m=False, split_k=False, alpha=1.0, bias=True, bias_mis=False, act=ACT_NONE,
                 pre_act=False, gate_rows=0, ldg=0, gate_off=-1, gate_scale=False, res=None, inplace=False, ldr=0, remap=None, split_n=0, ld_split=0,
                 split_alpha=1.0, batch=1, stride_c_odd=False, ln=False, scales=False)


def _case(name, route, impl, M, N, K, **kw):
    bad = set(kw) - set(_DEFAULTS)
    assert not bad, bad
    c = NS(name=name, route=route, impl=impl, M=M, N=N, K=K, **{**_DEFAULTS, **kw})
    c.out = c.out or c.dt
    c.Nc = N - c.split_n
    c.ldc = c.ldc or c.Nc
    c.lda = c.lda or K
    if c.gate_rows:
        c.ldg = c.ldg or 3 * N
        c.gate_off = N if c.gate_off < 0 else c.gate_off
        assert c.gate_off + N <= c.ldg
    if c.res:
        c.ldr = c.ldr or N
        if c.inplace:
            assert c.res == c.out and c.ldr == c.ldc and not c.remap
    if c.split_n:
        c.ld_split = c.ld_split or c.split_n
    return c


def groups(c):
    return -(-c.M // c.gate_rows) if c.gate_rows else 0


def rows(c):
    """output row of m (cvar_gemm_desc.remap_l / remap_L / remap_off)"""
    m = np.arange(c.M)
    if not c.remap:
        return m
    l, L, off = c.remap
    return (m // l) * L + off + m % l


def c_rows(c):
    """rows of the C buffer of one batch slice"""
    if not c.remap:
        return c.M
    l, L, off = c.remap
    return -(-c.M // l) * L


def operands(c):
    """the stored operand values of a case (float32 arrays that hold bf16-exact values where the tensor is bf16)"""
    rng = np.random.default_rng(7700 + 13 * c.seed + c.M + 3 * c.N + 5 * c.K)
    M, N, K, B = c.M, c.N, c.K, c.batch
    a = rng.standard_normal((B, M, K))
    w = rng.standard_normal((N, K)) / math.sqrt(K)
    if c.scales:        # tests/x3_ref.operands: one power of two per k, 2^-6 ... 2^6, on either side
        a = a * np.exp2(rng.integers(-6, 7, size=(1, 1, K)))
        w = w * np.exp2(rng.integers(-6, 7, size=(1, K)))
    o = NS(A=stored(a, c.dt), W=stored(w, c.dt))
    o.bias = (0.5 * rng.standard_normal(N)).astype(F32) if c.bias else None
    o.gate = o.gate_scale = o.res = o.aux = None
    if c.gate_rows:
        o.gate = (0.5 + 0.2 * rng.standard_normal((groups(c), c.ldg))).astype(F32)
        if c.gate_scale:
            o.gate_scale = np.asarray([(1.25, 0.0, 1.0, 0.8)[r % 4] for r in range(groups(c))], dtype=F32)
    if c.res:
        o.res = stored(1.0 + 0.5 * rng.standard_normal((B, M, N)), c.res)
    if c.act == ACT_GELU_GRAD:
        o.aux = stored(rng.standard_normal((B, M, N)), c.out)
    if c.ln:
        o.ln_eps = 1e-6
    return o


# ================================================================================================ float64 reference and bound
def depth(c):
    return -(-c.K // 16) + 16 + 16 + 8 if c.dt == 'bf16' else 2 * c.K + 16


def _sig_parts(u2, r_e):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        e = np.exp(-u2)
        sg = 1.0 / (1.0 + e)
        q = e / (1.0 + e)
    q = np.where(np.isfinite(e), q, 1.0)
    E_sg = sg * (q * r_e + 2 * U)
    return sg, q, E_sg, E_sg + U * q


def _gelu64(t):
    u2 = GELU_K2 * (t + GELU_C * t ** 3)
    r_e = (9 * np.abs(u2) + 4) * U
    sg, q, _, _ = _sig_parts(u2, r_e)
    y = t * sg
    return y, np.abs(y) * (q * r_e + 5 * U) + TINY


def _gelu_grad64(t):
    u2 = GELU_K2 * (t + GELU_C * t ** 3)
    r_e = (9 * np.abs(u2) + 4) * U
    sg, q, E_sg, E_q = _sig_parts(u2, r_e)
    P = 1 + GELU_C3 * t * t
    t2 = t * sg * q * GELU_K2 * P
    gp = sg + t2
    fac = np.abs(t * GELU_K2 * P)
    return gp, E_sg + np.abs(t2) * 9 * U + fac * (q * E_sg + sg * E_q) + U * np.abs(gp) + TINY * (1 + fac)


_EVAL = {}


def evaluate(c):
    """-> NS(C, C_bound, Cs, Cs_bound, pre, pre_bound) and the same bounds without the bf16 store term (*_raw_bound); cached per case"""
    if c.name in _EVAL:
        return _EVAL[c.name]
    o = operands(c)
    A, W = o.A.astype(F64), o.W.astype(F64)
    s = A @ W.T
    S = np.abs(A) @ np.abs(W).T
    E = depth(c) * U * (1 + 2.0 ** -7) * S

    def rnd(val, E):
        return E + 2 * U * (np.abs(val) + E)

    def store(val, E, dt):
        return E + bf16_half_ulp(np.abs(val) + E) if dt == 'bf16' else E

    alpha = float(F32(c.alpha))
    x = alpha * s
    E = rnd(x, abs(alpha) * E)
    if c.bias:
        x = x + o.bias.astype(F64)
        E = rnd(x, E)
    r = NS(pre=None, pre_bound=None, pre_raw_bound=None, Cs=None, Cs_bound=None, Cs_raw_bound=None)
    if c.pre_act:
        r.pre, r.pre_raw_bound, r.pre_bound = x, E, store(x, E, c.dt)
    if c.split_n and c.split_alpha not in (0.0, 1.0):
        sa = float(F32(c.split_alpha))
        xs = x[..., :c.split_n] * sa
        Es = rnd(xs, abs(sa) * E[..., :c.split_n])
        x = np.concatenate([xs, x[..., c.split_n:]], axis=-1)
        E = np.concatenate([Es, E[..., c.split_n:]], axis=-1)
    if c.act == ACT_GELU:
        y, own = _gelu64(x)
        x, E = y, GELU_LIP * E + own
    elif c.act == ACT_GELU_GRAD:
        gp, E_gp = _gelu_grad64(o.aux.astype(F64))
        y = x * gp
        E = np.abs(gp) * E + (np.abs(x) + E) * E_gp
        x, E = y, rnd(y, E)
    if c.gate_rows:
        gi = np.arange(c.M) // c.gate_rows
        G = o.gate[gi, c.gate_off:c.gate_off + c.N].astype(F64)
        E_G = 0.0
        if c.gate_scale:
            G = G * o.gate_scale[gi].astype(F64)[:, None]
            E_G = U * np.abs(G)
        y = x * G
        E = np.abs(G) * E + (np.abs(x) + E) * E_G
        x, E = y, rnd(y, E)
    if c.res:
        x = x + o.res.astype(F64)
        E = rnd(x, E)
    if c.split_n:
        r.Cs, r.Cs_raw_bound, r.Cs_bound = x[0, :, :c.split_n], E[0, :, :c.split_n], store(x, E, c.out)[0, :, :c.split_n]
        x, E = x[..., c.split_n:], E[..., c.split_n:]
    r.C, r.C_raw_bound, r.C_bound = x, E, store(x, E, c.out)
    _EVAL[c.name] = r
    return r


def reference(c):
    r = evaluate(c)
    return NS(C=r.C, Cs=r.Cs, pre=r.pre)


def bound(c):
    r = evaluate(c)
    return NS(C=r.C_bound, Cs=r.Cs_bound, pre=r.pre_bound)


def image(c, vals, rows_=None):
    """[batch][M][Nc] values -> the C buffer [batch][c_rows][ldc] with NaN wherever the call owns nothing"""
    rr = rows(c) if rows_ is None else rows_
    n_rows = c_rows(c)
    img = np.full((c.batch, n_rows + 1, c.ldc), np.nan)        # one spare row: a planted row fault may step past the arena
    img[:, rr, :c.Nc] = vals
    return img[:, :n_rows], img[:, n_rows:]


# ================================================================================================ float32 model of the kernels' arithmetic
FAULTS = ('drop_last_k', 'drop_last_chunk', 'gate_row', 'no_gate_scale', 'bias_after_act', 'alpha_after_bias', 'res_other_dtype', 'no_split_alpha',
          'remap_off', 'pre_after_act', 'bf16_trunc', 'gelu_c3')


def uses(c, fault):
    """does the case exercise what the fault breaks"""
    return {
        'drop_last_k': True,
        'drop_last_chunk': c.K % (64 if c.dt == 'bf16' else 32) != 0,
        'gate_row': c.gate_rows > 0 and groups(c) > 1,
        'no_gate_scale': c.gate_scale,
        'bias_after_act': c.bias and c.act != ACT_NONE,
        'alpha_after_bias': c.bias and c.alpha != 1.0,
        'res_other_dtype': c.res is not None,
        'no_split_alpha': c.split_n > 0 and c.split_alpha not in (0.0, 1.0),
        'remap_off': c.remap is not None,
        'pre_after_act': c.pre_act,
        'bf16_trunc': c.out == 'bf16' or (c.pre_act and c.dt == 'bf16'),
        'gelu_c3': c.act == ACT_GELU_GRAD,
    }[fault]


def _accumulate(c, o, fault):
    """fp32 accumulation in the kernels' granularity: bf16 - one accumulator update per 16 k of exact products; fp32 - a rounded product and a
    rounded add per k (v_mfma_f32_32x32x2f32)"""
    K = c.K
    if fault == 'drop_last_k':
        K -= 1
    elif fault == 'drop_last_chunk':
        K -= 8 if c.dt == 'bf16' else 4
    acc = np.zeros((c.batch, c.M, c.N), dtype=F32)
    if c.dt == 'bf16':
        A, W = o.A.astype(F64), o.W.astype(F64)
        for k0 in range(0, K, 16):
            k1 = min(K, k0 + 16)
            acc = acc + (A[..., k0:k1] @ W[:, k0:k1].T).astype(F32)
    else:
        for k in range(K):
            acc = acc + o.A[..., k, None] * o.W[None, None, :, k]
    return acc


def _gelu32(t, fast):
    with np.errstate(over='ignore', under='ignore'):
        if fast:
            c1 = F32(-2.0) * F32(0.7978845608028654) * F32(1.4426950408889634)
            c3 = c1 * F32(GELU_C)
            return t * (F32(1) / (F32(1) + np.exp2(t * (c1 + c3 * (t * t)))))
        k2 = F32(2.0) * F32(0.7978845608028654)
        return t / (F32(1) + np.exp(-(k2 * (t + F32(GELU_C) * t * t * t))))


def _gelu_grad32(t, c3):
    with np.errstate(over='ignore', under='ignore'):
        k2 = F32(2.0) * F32(0.7978845608028654)
        sg = F32(1) / (F32(1) + np.exp(-(k2 * (t + F32(GELU_C) * t * t * t))))
        return sg + t * sg * (F32(1) - sg) * k2 * (F32(1) + F32(c3) * t * t)


def _reinterpret(res, c):
    """the residual buffer read in the other dtype at the same element index"""
    B, M, N = res.shape
    buf = np.zeros((B, M, c.ldr), dtype=F32)
    buf[..., :N] = res
    idx = (np.arange(B)[:, None, None] * (M * c.ldr) + np.arange(M)[None, :, None] * c.ldr + np.arange(N)[None, None, :])
    if c.res == 'f32':
        halves = buf.reshape(-1).view(np.uint16)
        return bf16_value(halves[idx])
    words = bf16_bits(buf.reshape(-1))
    words = words[:words.size // 2 * 2].view(np.uint32).view(F32)
    return words[idx % words.size]


def model(c, fault=None, acc=None):
    """-> NS(C, Cs, pre: as stored; C_raw, Cs_raw, pre_raw: before the store's rounding; rows)"""
    o = operands(c)
    with np.errstate(invalid='ignore', over='ignore'):
        return _model(c, o, fault, _accumulate(c, o, fault) if acc is None else acc)


def _model(c, o, fault, acc):
    alpha = F32(c.alpha)
    bias = o.bias if c.bias else None
    if fault == 'alpha_after_bias' and bias is not None:
        x = (acc + bias) * alpha
    else:
        x = acc * alpha
        if bias is not None and fault != 'bias_after_act':
            x = x + bias
    r = NS(pre=None, pre_raw=None, Cs=None, Cs_raw=None)
    rnd = bf16_trunc if fault == 'bf16_trunc' else bf16_round

    def store(v, dt):
        return rnd(v) if dt == 'bf16' else v

    pre = x
    if c.split_n and c.split_alpha not in (0.0, 1.0) and fault != 'no_split_alpha':
        x = x.copy()
        x[..., :c.split_n] *= F32(c.split_alpha)
    if c.act == ACT_GELU:
        x = _gelu32(x, fast=c.dt == 'bf16')
    elif c.act == ACT_GELU_GRAD:
        x = x * _gelu_grad32(o.aux, GELU_C if fault == 'gelu_c3' else GELU_C3)
    if fault == 'bias_after_act' and bias is not None:
        x = x + bias
    if fault == 'pre_after_act' and c.act != ACT_NONE:
        pre = x
    if c.gate_rows:
        gi = np.arange(c.M) // c.gate_rows
        if fault == 'gate_row':
            gi = np.minimum((np.arange(c.M) + 1) // c.gate_rows, groups(c) - 1)
        G = o.gate[gi, c.gate_off:c.gate_off + c.N]
        if c.gate_scale and fault != 'no_gate_scale':
            G = G * o.gate_scale[gi][:, None]
        x = x * G
    if c.res:
        x = x + (_reinterpret(o.res, c) if fault == 'res_other_dtype' else o.res)
    if fault == 'pre_after_act' and c.act == ACT_NONE:
        pre = x
    if c.pre_act:
        r.pre_raw, r.pre = pre, store(pre, c.dt)
    if c.split_n:
        r.Cs_raw, r.Cs = x[0, :, :c.split_n], store(x[0, :, :c.split_n], c.out)
        x = x[..., c.split_n:]
    r.C_raw, r.C = x, store(x, c.out)
    r.rows = rows(c) + (1 if fault == 'remap_off' else 0)
    return r


# ================================================================================================ the case table
# route: the kernel a case is meant to launch (tests/test_gpu_gemm_oracle.py lists the kernel names); impl: the epilogue implementation
SPEC, RPF, VEC, SCALAR, QUAD_SK, QUAD_ST, ROWFIN = 'spec', 'rpf', 'vector', 'scalar', 'quad-splitk', 'quad-stream', 'rowfin'
GATE = dict(res='f32', inplace=True, out='f32')                   # x += gate * f, the proj / fc2 form


def _build():
    t = []

    def add(name, route, impl, M, N, K, **kw):
        t.append(_case(name, route, impl, M, N, K, seed=len(t), **kw))

    big = dict(M=2085, N=256)
    # ---- bf16 tiles: every shape with the DMA-fast loop (K % 64 == 0) and the any-K loop (K % 8 == 0 only)
    for K in (128, 72):
        add(f't64-K{K}', '64x128', VEC, 37, 256, K, alpha=0.37, lda=K + 8)
    for K in (128, 200):
        add(f't128w8-K{K}', '128x128 w8', VEC, 300, 256, K, alpha=0.37, out='f32')
        add(f't128w4-K{K}', '128x128 w4', VEC, 300, 256, K, tile_cfg=26)
        add(f't128s3-K{K + 64}', '128x128 s3', VEC, 300, 256, K + 64, tile_cfg=13, alpha=0.37, bias=False)
        add(f't128s4-K{K + 128}', '128x128 s4', VEC, 300, 256, K + 128, tile_cfg=14, out='f32')
        add(f't256w8-K{K}', '256x256 w8', SPEC, K=K, tile_cfg=2, alpha=0.37, lda=K + 8, **big)
        add(f't256w4-K{K}', '256x256 w4', SPEC, K=K, tile_cfg=3, out='f32', **big)
        add(f't256x192-K{K}', '256x192', SPEC, 2085, 384, K, tile_cfg=27, alpha=0.37, bias=False)
        add(f't128x160-K{K}', '128x160', SPEC, 4100, 320, K, out='f32')
    add('t256x192-N200', '256x192', SPEC, 2085, 200, 72, tile_cfg=27, alpha=0.37)
    add('t256w8-scales', '256x256 w8', SPEC, K=256, tile_cfg=2, scales=True, out='f32', **big)
    # ---- specialised variants of the large tiles
    add('spec-gelu-bf16', '256x256 w8', SPEC, K=128, tile_cfg=2, act=ACT_GELU, **big)
    add('spec-gelu-pre-160', '128x160', SPEC, 4100, 320, 72, act=ACT_GELU, pre_act=True)
    add('spec-gelu-192', '256x192', SPEC, 2085, 384, 128, tile_cfg=27, act=ACT_GELU, alpha=0.37)
    add('spec-grad-bf16', '256x256 w8', SPEC, K=128, tile_cfg=2, act=ACT_GELU_GRAD, **big)
    add('spec-grad-192', '256x192', SPEC, 2085, 384, 72, tile_cfg=27, act=ACT_GELU_GRAD)
    add('rpf-gate100', '256x256 w8', RPF, K=128, tile_cfg=2, gate_rows=100, **GATE, **big)
    add('spec-gate3-reg', '256x256 w8', SPEC, K=128, tile_cfg=28, gate_rows=3, alpha=0.37, **GATE, **big)
    add('spec-gate1-w4', '256x256 w4', SPEC, K=72, tile_cfg=3, gate_rows=1, **GATE, **big)
    add('spec-gatescale', '256x256 w8', SPEC, K=128, tile_cfg=28, gate_rows=100, gate_scale=True, **GATE, **big)
    add('spec-pre-gate', '256x256 w8', SPEC, K=128, tile_cfg=2, gate_rows=3, pre_act=True, **GATE, **big)
    add('spec-gate-N200', '256x192', SPEC, 2085, 200, 128, tile_cfg=27, gate_rows=100, **GATE)
    add('spec-gate-160', '128x160', SPEC, 4100, 320, 128, gate_rows=100, gate_scale=True, **GATE)
    add('spec-remap', '256x256 w8', SPEC, K=128, tile_cfg=2, remap=(695, 700, 3), **big)
    add('spec-remap-split', '256x256 w8', SPEC, K=128, tile_cfg=2, remap=(695, 700, 3), split_n=64, split_alpha=0.18, ldc=200, ld_split=72, **big)
    add('spec-remap-split-160', '128x160', SPEC, 4100, 320, 72, remap=(1025, 1030, 2), split_n=160, split_alpha=0.18)
    # ---- generic vector form on the large tiles (combinations without a specialised variant)
    add('vec-gelu-f32-256', '256x256 w8', VEC, K=128, tile_cfg=2, act=ACT_GELU, out='f32', **big)
    add('vec-grad-f32-256', '256x256 w4', VEC, K=72, tile_cfg=3, act=ACT_GELU_GRAD, out='f32', **big)
    add('vec-resbf16-256', '256x256 w8', VEC, K=128, tile_cfg=2, res='bf16', ldr=264, alpha=0.37, **big)
    add('vec-remap-split-f32-256', '256x256 w8', VEC, K=128, tile_cfg=2, remap=(695, 700, 3), split_n=64, split_alpha=0.18, out='f32', **big)
    add('vec-batch3-256', '256x256 w8', VEC, K=128, tile_cfg=2, batch=3, res='bf16', **big)
    add('vec-gate-bf16out-192', '256x192', VEC, 2085, 384, 128, tile_cfg=27, gate_rows=3, gate_scale=True, res='bf16', inplace=True)
    # ---- generic vector form on the small tiles
    add('vec-alpha-nobias', '64x128', VEC, 37, 256, 128, alpha=0.37, bias=False, out='f32')
    add('vec-gelu-bf16', '128x128 w8', VEC, 300, 256, 128, act=ACT_GELU)
    add('vec-gelu-f32', '64x128', VEC, 37, 256, 72, act=ACT_GELU, out='f32', alpha=0.37)
    add('vec-pre-gelu', '128x128 w8', VEC, 300, 256, 200, act=ACT_GELU, pre_act=True, ldc=264)
    add('vec-pre-gate', '64x128', VEC, 37, 256, 128, gate_rows=3, pre_act=True, **GATE)
    add('vec-grad-small', '128x128 w8', VEC, 300, 256, 128, act=ACT_GELU_GRAD, alpha=0.37)
    add('vec-grad-t64-f32', '64x128', VEC, 37, 256, 128, act=ACT_GELU_GRAD, out='f32')
    add('vec-gate1', '128x128 w8', VEC, 300, 256, 128, gate_rows=1, **GATE)
    add('vec-gate3', '128x128 w4', VEC, 300, 256, 128, tile_cfg=26, gate_rows=3, **GATE)
    add('vec-gate100', '128x128 w8', VEC, 300, 256, 72, gate_rows=100, gate_scale=True, **GATE)
    add('vec-gate3-t64', '64x128', VEC, 37, 256, 128, gate_rows=3, gate_scale=True, alpha=0.37, **GATE)
    add('vec-res-f32-oop', '128x128 w8', VEC, 300, 256, 128, res='f32', ldr=264, out='f32')
    add('vec-res-bf16-inplace', '128x128 s3', VEC, 300, 256, 192, tile_cfg=13, res='bf16', inplace=True, ldr=264, ldc=264)
    add('vec-res-bf16-oop-f32out', '64x128', VEC, 37, 256, 128, res='bf16', ldr=264, out='f32')
    add('vec-remap', '128x128 w8', VEC, 300, 256, 128, remap=(100, 104, 3))
    add('vec-remap-split-bf16', '128x128 w8', VEC, 300, 256, 128, remap=(100, 104, 3), split_n=64, split_alpha=0.18, ldc=200)
    add('vec-remap-split-f32', '64x128', VEC, 36, 256, 72, remap=(12, 20, 5), split_n=128, split_alpha=0.18, out='f32')
    add('vec-batch3', '64x128', VEC, 37, 256, 128, batch=3, res='f32', out='f32', alpha=0.37)
    add('vec-scales', '128x128 w8', VEC, 300, 256, 200, scales=True, out='f32')
    # ---- generic scalar form: N % 8, ldc % 8, a bias one float past a 16-byte boundary, ldg % 4
    add('scalar-N100', '128x128 w8', SCALAR, 300, 100, 128, gate_rows=3, alpha=0.37, **GATE)
    add('scalar-N100-gelu', '64x128', SCALAR, 37, 100, 72, act=ACT_GELU, pre_act=True)
    add('scalar-ldc', '128x128 w8', SCALAR, 300, 256, 128, ldc=260, act=ACT_GELU, pre_act=True)
    add('scalar-ldc-grad-256', '256x256 w8', SCALAR, K=128, tile_cfg=2, ldc=260, act=ACT_GELU_GRAD, out='f32', **big)
    add('scalar-bias-split', '128x128 w8', SCALAR, 300, 256, 128, bias_mis=True, remap=(100, 104, 3), split_n=64, split_alpha=0.18, ldc=200)
    add('scalar-bias-split-256', '256x256 w8', SCALAR, K=128, tile_cfg=2, bias_mis=True, remap=(695, 700, 3), split_n=64, split_alpha=0.18, out='f32', **big)
    add('scalar-stride-split', '64x128', SCALAR, 36, 256, 128, stride_c_odd=True, remap=(12, 20, 5), split_n=128, split_alpha=0.18)
    add('scalar-ldg', '128x128 w8', SCALAR, 300, 256, 128, gate_rows=100, ldg=3 * 256 + 2, gate_scale=True, res='bf16', out='f32')
    # ---- split-K slices + the element-wise finish (gemm_epilogue_quad)
    for M in (36, 300):
        for K in (512, 1536):
            add(f'splitk-M{M}-K{K}', 'split-K', QUAD_SK, M, 256, K, split_k=True, alpha=0.37, out='f32' if K == 512 else 'bf16')
    add('splitk-long', 'split-K long', QUAD_SK, 1152, 1536, 1536, split_k=True)
    add('splitk-gelu-bf16', 'split-K', QUAD_SK, 36, 256, 512, split_k=True, act=ACT_GELU)
    add('splitk-gelu-pre-f32', 'split-K', QUAD_SK, 300, 256, 512, split_k=True, act=ACT_GELU, pre_act=True, out='f32')
    add('splitk-grad', 'split-K', QUAD_SK, 36, 256, 512, split_k=True, act=ACT_GELU_GRAD, alpha=0.37)
    add('splitk-gate3', 'split-K', QUAD_SK, 300, 256, 512, split_k=True, gate_rows=3, gate_scale=True, **GATE)
    add('splitk-pre-gate', 'split-K', QUAD_SK, 36, 256, 512, split_k=True, gate_rows=1, pre_act=True, **GATE)
    add('splitk-resbf16', 'split-K', QUAD_SK, 300, 256, 512, split_k=True, res='bf16', ldr=264)
    add('splitk-remap', 'split-K', QUAD_SK, 300, 256, 512, split_k=True, remap=(100, 104, 3))
    add('splitk-remap-split', 'split-K', QUAD_SK, 300, 256, 512, split_k=True, remap=(100, 104, 3), split_n=64, split_alpha=0.18, ldc=200)
    add('splitk-remap-split-f32', 'split-K', QUAD_SK, 36, 256, 1536, split_k=True, remap=(12, 20, 5), split_n=128, split_alpha=0.18, out='f32')
    # ---- the weight-streaming kernel (small_m), one case per (mt, nt) plan, + slices, + two row groups
    add('stream-1x1', 'stream 1x1', QUAD_ST, 4, 64, 64, small_m=True, split_k=True, alpha=0.37)
    add('stream-2x1', 'stream 2x1', QUAD_ST, 24, 64, 96, small_m=True, split_k=True, act=ACT_GELU)
    add('stream-4x1', 'stream 4x1', QUAD_ST, 40, 64, 64, small_m=True, split_k=True, gate_rows=3, gate_scale=True, **GATE)
    add('stream-4x2', 'stream 4x2', QUAD_ST, 40, 4096, 64, small_m=True, split_k=True, alpha=0.37, out='f32')
    add('stream-remap-split', 'stream 4x1', QUAD_ST, 36, 64, 128, small_m=True, split_k=True, remap=(12, 20, 5), split_n=32, split_alpha=0.18, ldc=40)
    add('stream-gelu-f32', 'stream 1x1', QUAD_ST, 4, 64, 64, small_m=True, split_k=True, act=ACT_GELU, out='f32', alpha=0.37, bias=False)
    add('stream-resbf16', 'stream 2x1', QUAD_ST, 24, 64, 96, small_m=True, split_k=True, res='bf16', ldr=72, gate_rows=100)
    add('stream-sliced', 'stream sliced', QUAD_SK, 40, 64, 4096, small_m=True, split_k=True, alpha=0.37)
    add('stream-two-groups', 'stream 4x1 gy2', QUAD_ST, 100, 64, 64, small_m=True, split_k=True, gate_rows=3, **GATE)
    # ---- the row-finishing reduction (ln=): gate + fp32 residual in place
    add('rowfin-stream-N192', 'rowfin stream', ROWFIN, 16, 192, 1024, small_m=True, split_k=True, ln=True, gate_rows=8, gate_off=192, ldg=6 * 192, **GATE)
    add('rowfin-tile-N192', 'rowfin tiles', ROWFIN, 300, 192, 1536, split_k=True, ln=True, gate_rows=150, gate_off=192, ldg=6 * 192, alpha=0.37, **GATE)
    add('rowfin-tile-N320', 'rowfin tiles', ROWFIN, 300, 320, 1536, split_k=True, ln=True, gate_rows=150, gate_off=320, ldg=6 * 320, gate_scale=True, **GATE)
    add('rowfin-tile-N512', 'rowfin tiles', ROWFIN, 36, 512, 512, split_k=True, ln=True, gate_rows=18, gate_off=512, ldg=6 * 512, bias=False, **GATE)
    # ---- fp32 operands (parity mode): generic epilogue only
    for K in (64, 36):
        add(f'f32-t64-K{K}', 'f32 64x128', VEC, 37, 256, K, dt='f32', alpha=0.37)
        add(f'f32-t128-K{K}', 'f32 128x128', VEC, 300, 256, K, dt='f32', lda=K + 4)
        add(f'f32-t160-K{K}', 'f32 128x160', VEC, 4100, 320, K, dt='f32', alpha=0.37, bias=False)
        add(f'f32-t256-K{K}', 'f32 256x256', VEC, K=K, tile_cfg=2, dt='f32', **big)
    add('f32-splitk', 'f32 split-K', QUAD_SK, 36, 256, 256, dt='f32', split_k=True, alpha=0.37)
    add('f32-scales', 'f32 128x128', VEC, 300, 256, 64, dt='f32', scales=True)
    add('f32-gelu-pre', 'f32 128x128', VEC, 300, 256, 64, dt='f32', act=ACT_GELU, pre_act=True)
    add('f32-grad', 'f32 64x128', VEC, 37, 256, 36, dt='f32', act=ACT_GELU_GRAD, alpha=0.37)
    add('f32-gate', 'f32 256x256', VEC, K=64, tile_cfg=2, dt='f32', gate_rows=100, gate_scale=True, **GATE, **big)
    add('f32-remap-split', 'f32 128x128', VEC, 300, 256, 64, dt='f32', remap=(100, 104, 3), split_n=64, split_alpha=0.18)
    add('f32-scalar-N100', 'f32 128x128', SCALAR, 300, 100, 36, dt='f32', res='f32', alpha=0.37)
    add('f32-splitk-grad', 'f32 split-K', QUAD_SK, 300, 256, 256, dt='f32', split_k=True, act=ACT_GELU_GRAD)
    names = [c.name for c in t]
    assert len(set(names)) == len(names)
    return {c.name: c for c in t}


CASES = _build()
