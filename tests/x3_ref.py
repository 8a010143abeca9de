"""Host restatement of the split-bf16 ("bf16x3") contract of gemm_precision='bf16x3' (include/cvar_serve.h) in numpy's uint32 / float32
arithmetic - nothing here is taken from the library - and the error bound of a split product, term by term.

A value x is carried as hi = bf16(x), lo = bf16(x - hi) (round to nearest even; x - hi is exact in fp32).  An activation row is [hi | lo | hi], a
weight row [w_hi | w_hi | w_lo], and one bf16 GEMM over the 3 K columns sums a_hi w_hi + a_lo w_hi + a_hi w_lo in fp32.

The bound of one output  y = sum_k a_k w_k  (+ epilogue), with S = sum_k |a_k| |w_k| taken in float64:
  representation   |a - (a_hi + a_lo)| <= 2^-17 |a| and the same for w              ->  2 * 2^-17 S   (the cross term 2^-34 S rides in the slack below)
  dropped product  |a_lo w_lo| <= 2^-16 |a w|   (the issue's figure; |a_lo| <= 2^-9 |a| makes it 2^-18, so the 2^-34 above is covered)   ->  2^-16 S
  accumulation     every product of two bf16 values is exact in fp32.  The tile kernels add them in v_mfma_f32_32x32x16_bf16 / 16x16x32_bf16 steps: an
                   output's chain is one accumulator update per 16 (at least) of its 3 K columns, each update rounding once to fp32 - treated here as up to
                   16 roundings for the sum inside the instruction - plus at most 16 K slices summed by the split-K reduction and 8 wave partials of the
                   weight-streaming kernel.  Every rounding is <= 2^-24 of a partial sum, itself <= (1 + 2^-7) S:
                   depth(K) = 3 K / 16 + 16 + 16 + 8 roundings                          ->  depth(K) * 2^-24 * (1 + 2^-7) S
  epilogue         bias add, GELU, gate multiply and residual add round once each to fp32 (GELU: v_exp_f32 / v_rcp_f32 at ~1 ulp each, 4 ulp taken)
                   ->  2^-24 * (|y + b| + ...) per step, see product_bound's `epilogue` argument.
"""
import numpy as np

U24 = 2.0 ** -24


def bf16_bits(x):
    """fp32 -> the 16 bits of bf16(x), round to nearest even, in uint32 arithmetic (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16).astype(np.uint16)


def bf16_value(bits16):
    return (np.asarray(bits16, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    """fp32 -> bf16(x) as an fp32 value"""
    return bf16_value(bf16_bits(x))


def split(x):
    """x -> (hi, lo) as fp32 values: hi = bf16(x), lo = bf16(x - hi) with the subtraction in fp32 (exact)"""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_round(x)
    lo = bf16_round((x - hi).astype(np.float32))
    return hi, lo


def activation_rows(x):
    """[M][C] fp32 -> [M][3 C] bf16 bit patterns [hi | lo | hi]"""
    hi, lo = split(x)
    return np.concatenate([bf16_bits(hi), bf16_bits(lo), bf16_bits(hi)], axis=-1)


def weight_rows(w):
    """[N][K] fp32 -> [N][3 K] bf16 bit patterns [w_hi | w_hi | w_lo]"""
    hi, lo = split(w)
    return np.concatenate([bf16_bits(hi), bf16_bits(hi), bf16_bits(lo)], axis=-1)


def split_product_model(a, w):
    """the arithmetic of the mode in numpy: the three-segment rows contracted with fp32 products and fp32 accumulation (numpy's own order: any fp32
    order of the 3 K exact products is covered by the accumulation term of the bound)"""
    A = bf16_value(activation_rows(a))
    W = bf16_value(weight_rows(w))
    return A @ W.T


def depth(K):
    return 3 * K // 16 + 16 + 16 + 8


def product_bound(a, w, epilogue=0.0):
    """per-output bound of |split product - float64 a w^T| for fp32 a [M][K], w [N][K]; `epilogue`: float64 [M][N] of the epilogue's rounding terms"""
    S = np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T
    K = a.shape[1]
    rel = 2 * 2.0 ** -17 + 2.0 ** -16 + depth(K) * U24 * (1 + 2.0 ** -7)
    return rel * S + epilogue


def operands(M, N, K, seed):
    """gaussian operands whose columns carry scales 2^-6 ... 2^6 (one power of two per k, the inverse on the other side for half of them so the products
    span the range too)"""
    rng = np.random.default_rng(seed)
    sa = np.exp2(rng.integers(-6, 7, size=(1, K))).astype(np.float32)
    sw = np.exp2(rng.integers(-6, 7, size=(1, K))).astype(np.float32)
    a = (rng.standard_normal((M, K)).astype(np.float32) * sa).astype(np.float32)
    w = (rng.standard_normal((N, K)).astype(np.float32) * sw).astype(np.float32)
    return a, w


def gelu_tanh(t):
    t = np.asarray(t, dtype=np.float64)
    return 0.5 * t * (1.0 + np.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))
