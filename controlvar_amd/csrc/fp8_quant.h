// Row quantisation to OCP e4m3 with one power-of-two scale per row (gemm_precision='fp8'; the contract is stated in include/cvar_serve.h).
// Shared by the row pass (gemm_fp8.hip: cvar_quant_rows_fp8) and the adaLN store (ops.hip: cvar_ln_modulate_fp8): one text, the same bits.
#pragma once
#include "cvar_common.h"

__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, 64));
    return v;
}

// |x| as its bit pattern: the order of the patterns is the order of the values, and Inf / NaN (>= 0x7f800000) sort above every finite
// value, so one unsigned maximum gives the row's amax AND tells whether the row is broken.
__device__ __forceinline__ unsigned fp8_abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// k = the smallest integer with amax <= 448 * 2^k = 1.75 * 2^(8 + k), clamped to [-60, 120]; from the exponent and mantissa fields of amax.
// amax = (1 + m / 2^23) * 2^(e - 127): k = e - 135 when the mantissa is <= 1.75 (m <= 0x600000), e - 134 otherwise.  Zero and subnormals
// (e == 0) fall below the clamp.  The largest finite fp32 gives exactly 120.
__device__ __forceinline__ int fp8_row_exp(unsigned amax_bits) {
    const int e = (int)(amax_bits >> 23), m = (int)(amax_bits & 0x7fffffu);
    const int k = e - 135 + (m > 0x600000 ? 1 : 0);
    return e == 0 ? -60 : min(max(k, -60), 120);
}
__device__ __forceinline__ float fp8_pow2(int k) { return __uint_as_float((unsigned)(k + 127) << 23); }    // -126 <= k <= 127

// four values, already multiplied by 2^-k (|v| <= 448), to four e4m3 bytes: v_cvt_pk_fp8_f32 rounds to nearest even
__device__ __forceinline__ unsigned fp8_pack4(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (unsigned)w;
}

// The way back (kv_precision='fp8', include/cvar_kvcache.h): eight e4m3 bytes (w0 = elements 0..3, w1 = 4..7) times a power-of-two scale, as
// eight bf16 values.  An e4m3 value has 3 mantissa bits and bf16 has 7, so value * 2^k IS a bf16 value: the fp32 product is exact and its upper
// 16 bits are the result - no rounding anywhere (v_perm_b32 picks the two upper halves).  0x7F / 0xFF (NaN) stay NaN.
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16(int w0, int w1, float scale) {
    const f32x2_t f[4] = {__builtin_amdgcn_cvt_pk_f32_fp8(w0, false), __builtin_amdgcn_cvt_pk_f32_fp8(w0, true),
                          __builtin_amdgcn_cvt_pk_f32_fp8(w1, false), __builtin_amdgcn_cvt_pk_f32_fp8(w1, true)};
    // The pair times (scale, scale) as ONE vector multiply.  Written as two scalar multiplies, the compiler paired the K and the V scale of a thread in one
    // register pair and built each product pair from two v_pk_mul_f32 with crossed op_sel; the G = 2 attention instantiations then gave wrong upper halves
    // (odd elements of V) on the MI355X, differently from run to run.  This form compiles to one broadcast v_pk_mul_f32 per pair.
    const f32x2_t s2 = {scale, scale};
    unsigned u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2_t p = f[i] * s2;                    // one packed multiply per pair
        u[i] = __builtin_amdgcn_perm(__float_as_uint(p[1]), __float_as_uint(p[0]), 0x07060302u);
    }
    const u32x4_t v = {u[0], u[1], u[2], u[3]};
    return __builtin_bit_cast(bf16x8_t, v);
}
