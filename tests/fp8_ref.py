"""Host restatement of the e4m3 contract of gemm_precision='fp8' (include/cvar_serve.h) in numpy - nothing here is taken from the library -
and the error bound of an e4m3 product, term by term.

OCP e4m3 (e4m3fn): 1 sign, 4 exponent (bias 7), 3 mantissa bits; no infinities, S.1111.111 is NaN, the largest finite value is 448 = 1.75 * 2^8, the
subnormals are m / 8 * 2^-6 (the smallest 2^-9).

A row x[0..K) is carried as bytes q_k = e4m3_rne(x_k * 2^-k) and one scale 2^k, k the smallest integer with amax <= 448 * 2^k clamped to [-60, 120], read off
the exponent and mantissa fields of amax.  A zero row gets k = -60 and zero bytes; a row with a NaN or an Inf gets scale 1 and every byte 0x7F; bytes
[K, ldq) are zero.

The product is acc = sum_k q_a q_w, one v_mfma_scale_f32_16x16x128_f8f6f4 per 128 k into an fp32 accumulator; the epilogue sees (acc * a_scale) * w_scale -
exact, both factors are powers of two.

The bound of one output against float64 on the SAME quantised operands, with S = sum_k |q_a q_w| * a_scale * w_scale in float64:
  accumulation   the candidate of the issue was an fp32 chain: one accumulator update per 128 k, each rounding once, plus the sum inside the instruction
                 taken as 3 roundings per 32-element block and 40 for the tree - candidate_depth(K) = K / 32 + 40 roundings of 2^-24 (1 + 2^-7) S.
                 The MI355X does NOT sum that way.  Measured with exact data (tools/fp8_mfma_probe.py): inside the instruction the products of a group of 8
                 consecutive k are aligned to the group's largest product and what lies some 2^-9 ... 2^-16 below it is cut off (one product 2^16 with
                 seven products 1.0 in its group gives 2^16 exactly, the other 120 products 1.0 of the instruction arrive), and the group sums are added
                 with truncation, not rounding.  Operands inside a few binades are summed exactly (random codes of four binades: every output exact up to
                 K = 6144); operands drawn over all 127 magnitudes - eighteen binades, which no quantised row of the model has - lose up to
                 HW_DEPTH_MEASURED = 2566 units of 2^-24 (1 + 2^-7) S (worst output of the three asserted cases, at K = 128; 1228 at K = 384, 650 at
                 K = 1536: the loss is per group, so it falls against S as K grows).  By the issue's rule for that outcome the constant is TWICE the
                 measured worst case, for every K:
                 depth(K) = 2 * 2566 = 5132                ->  depth(K) * 2^-24 * (1 + 2^-7) S
  epilogue       alpha, bias add, gate multiply, residual add and split_alpha round once each to fp32; GELU, see gelu_bound; a bf16 output rounds once
                 more, by at most half a step = 2^-8 of its value.  The tests add these per case.
"""
import numpy as np

U24 = 2.0 ** -24
E4M3_MAX = 448.0


# ------------------------------------------------------------------------------------------------ e4m3
def decode_table():
    """float64 [256]: the value of every e4m3 byte (NaN for 0x7F / 0xFF)"""
    b = np.arange(256)
    e, m = (b >> 3) & 15, b & 7
    v = np.where(e == 0, m / 8.0 * 2.0 ** -6, (1 + m / 8.0) * np.exp2(e - 7.0))
    v = np.where((b & 0x7F) == 0x7F, np.nan, v)
    return np.where(b >> 7, -v, v)


DECODE = decode_table()
_POS = DECODE[:0x7F]                      # the 127 finite non-negative values, ascending: value -> code by search


def decode(q):
    return DECODE[np.asarray(q, dtype=np.uint8)]


def encode_rne(x):
    """fp32 / float64 values with |x| <= 448 (or NaN / Inf -> 0x7F) -> e4m3 bytes, round to nearest, ties to even; the sign of a negative value survives
    a rounding to zero (0x80)"""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(x)
    bad = ~np.isfinite(x)
    a = np.where(bad, 0.0, a)
    assert (a <= E4M3_MAX).all(), 'encode_rne is stated for |x| <= 448: the row scale guarantees it'
    _, ex = np.frexp(a)                                   # a = f * 2^ex, 0.5 <= f < 1: the binade of a is ex - 1
    step = np.exp2(np.maximum(ex - 1, -6) - 3.0)          # spacing of the e4m3 grid in that binade (subnormals share the spacing of 2^-6)
    r = np.rint(a / step) * step                          # a / step is exact (a power of two); rint is ties-to-even; n = 16 is the next binade's m = 0
    code = np.searchsorted(_POS, r).astype(np.uint8)
    assert np.array_equal(_POS[code], r)
    code = code | (np.signbit(x).astype(np.uint8) << 7)
    return np.where(bad, np.uint8(0x7F), code).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ bf16 (for the rows the kernels take)
def bf16_round(x):
    """fp32 -> bf16(x) as an fp32 value, round to nearest even in uint32 arithmetic (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (((u + (((u >> 16) & 1) + np.uint32(0x7FFF))) >> 16) << 16).astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------------------------------------ the row rule
def row_exponent(amax):
    """k of a finite amax >= 0 (fp32), from its bit fields: amax = (1 + m / 2^23) 2^(e - 127) <= 1.75 * 2^(8 + k)  <=>  k >= e - 135 (m <= 0x600000) or
    e - 134 (above); zero and subnormals (e == 0) fall below the clamp"""
    bits = np.asarray(amax, dtype=np.float32).view(np.uint32).astype(np.int64)
    e, m = bits >> 23, bits & 0x7FFFFF
    k = e - 135 + (m > 0x600000)
    return np.where(e == 0, -60, np.clip(k, -60, 120)).astype(np.int64)


def ldq_of(K):
    return (K + 127) // 128 * 128


def quant_rows(x, ldq=None):
    """x [M][K] (fp32 values; bf16 rows are passed as their fp32 values) -> (bytes uint8 [M][ldq], scale fp32 [M])"""
    x = np.asarray(x, dtype=np.float32)
    M, K = x.shape
    ldq = ldq_of(K) if ldq is None else ldq
    assert ldq % 128 == 0 and ldq >= K
    bad = ~np.isfinite(x).all(axis=1)
    amax = np.where(bad, np.float32(0), np.abs(np.where(np.isfinite(x), x, 0)).max(axis=1)).astype(np.float32)
    k = row_exponent(amax)
    inv = np.exp2(-k.astype(np.float64)).astype(np.float32)          # 2^-k: a normal fp32 for every k in [-60, 120]
    with np.errstate(invalid='ignore', over='ignore'):
        scaled = (x * inv[:, None]).astype(np.float32)               # exact, or below the fp32 normals (then it rounds to zero either way)
    q = np.zeros((M, ldq), dtype=np.uint8)
    q[:, :K] = encode_rne(np.where(bad[:, None], np.float32(np.nan), scaled))
    scale = np.where(bad, 1.0, np.exp2(k.astype(np.float64))).astype(np.float32)
    return q, scale


def dequant(q, scale, K):
    """float64 values the bytes stand for"""
    return decode(q[:, :K]) * np.asarray(scale, dtype=np.float64)[:, None]


# ------------------------------------------------------------------------------------------------ the product
HW_DEPTH_MEASURED = 2566          # MI355X, worst output of the three asserted cases of tests/test_gpu_fp8_kernels.py, in units of 2^-24 (1 + 2^-7) S


def candidate_depth(K):
    """the fp32-chain figure the bound started from (exceeded by the hardware: see above)"""
    return K // 32 + 40


def depth(K):
    return 2 * HW_DEPTH_MEASURED


def product_ref(qa, sa, qw, sw):
    """float64 [M][N]: sum_k q_a q_w * a_scale * w_scale on the decoded bytes (all K columns of the byte rows; pad bytes are zeros)"""
    return (decode(qa) * np.asarray(sa, np.float64)[:, None]) @ (decode(qw) * np.asarray(sw, np.float64)[:, None]).T


def product_bound(qa, sa, qw, sw, depth_const=None):
    """per-output bound of |fp32-accumulated product - product_ref|"""
    K = qa.shape[1]
    S = (np.abs(decode(qa)) * np.asarray(sa, np.float64)[:, None]) @ (np.abs(decode(qw)) * np.asarray(sw, np.float64)[:, None]).T
    return (depth(K) if depth_const is None else depth_const) * U24 * (1 + 2.0 ** -7) * S


def gelu_tanh(t):
    t = np.asarray(t, dtype=np.float64)
    return 0.5 * t * (1.0 + np.tanh(0.7978845608028654 * (t + 0.044715 * t ** 3)))


def gelu_bound(t, err_in):
    """|fp32 gelu(t~) - gelu(t)| for |t~ - t| <= err_in.  The library evaluates t * sigmoid(u), u = 2 sqrt(2 / pi) (t + 0.044715 t^3), as t / (1 + exp(-u)):
    the input error passes through |gelu'| <= 1.13; u carries 5 roundings and exp one more ulp or two (6 * 2^-24 |u| on exp's argument, i.e. on the result
    |t| sigma (1 - sigma) |u| of it); the sum 1 + e, the division and exp's own value error are taken as 6 * 2^-24 of the result"""
    t = np.asarray(t, dtype=np.float64)
    u = 2 * 0.7978845608028654 * (t + 0.044715 * t ** 3)
    sg = 1.0 / (1.0 + np.exp(-u))
    return 1.13 * err_in + U24 * (6 * np.abs(t * sg) + 6 * np.abs(t * u) * sg * (1 - sg))


def random_e4m3(shape, rng, amax_code=0x7E):
    """uniformly drawn finite e4m3 bytes (both signs, subnormals and zeros included)"""
    mag = rng.integers(0, amax_code + 1, size=shape).astype(np.uint8)
    return (mag | (rng.integers(0, 2, size=shape).astype(np.uint8) << 7)).astype(np.uint8)
