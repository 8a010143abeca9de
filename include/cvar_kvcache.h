/* cvar_kvcache.h - the e4m3 K/V cache of generation (kv_precision='fp8'); same rules as cvar.h: plain pointers + sizes + stream, no
 * allocation, asynchronous, negative `cvar_status` on error.  The functions live in the same libcvar_hip.so.
 *
 * Format (one layer of the arena):
 *   kv8      [R][Lmax][2C] bytes, OCP e4m3 (e4m3fn), C = 64 H: per token the H key heads, then the H value heads, 64 bytes each;
 *   kv_scale [R][Lmax][2H] fp32: per token H scales of the key heads, then H of the value heads; every scale is a power of two.
 *   That is 2C + 8H = 2C * 17/16 bytes per token against the 4C of the bf16 arena: 17/32.
 * Quantisation unit: ONE 64-element head vector of one token, keys and values separately, by the row rule of gemm_precision='fp8' (cvar_serve.h)
 * with K = 64:  k = the smallest integer with amax <= 448 * 2^k, clamped to [-60, 120], read off the bit fields of amax; scale = 2^k;
 * byte = e4m3_rne(x * 2^-k).  A zero vector gives k = -60 and zero bytes.  A vector with a NaN or an Inf gives scale 1 and every byte 0x7F (NaN).
 * The cached value is byte * scale.  An e4m3 value has 3 mantissa bits, bf16 has 7: byte * scale is exactly a bf16 value, so attention over this
 * arena computes, bit for bit, what cvar_attention_prescaled computes over a bf16 arena that holds byte * scale.
 * Adding these entry points changed no signature of cvar.h, cvar_serve.h or cvar_accum.h: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_KVCACHE_H
#define CVAR_KVCACHE_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Quantise the k|v rows of one pass into the arena rows of one layer.  kv: bf16 [R * l][2C], row r * l + t = token t of sequence r (what the qkv GEMM
 * writes with ldc = 2C and no row remap).  Writes the 2C bytes and the 2H scales of the arena rows (r, q_off + t), t < l, and nothing else: other
 * positions and their scale entries keep what they held.  All offsets are 64-bit.  kv 16-byte aligned, kv8 8-byte aligned.
 * CVAR_EINVAL: a NULL pointer, a size <= 0, q_off < 0 or q_off + l > Lmax, a misaligned pointer. */
int cvar_kv_append_fp8(const void* kv, void* kv8, float* kv_scale, int R, int H, int Lmax, int q_off, int l, void* stream);

/* cvar_attention_prescaled (cvar.h) over the e4m3 arena of one layer: the same queries (bf16 [R][l][C], carrying scale * log2(e)), levels, holes,
 * out (bf16 [R * l][C]) and optional lse, the same launch rule, the same arithmetic from the first LDS read of a tile on; the tiles are dequantised
 * (exactly) while they are staged.  Rows at and behind the last visible key are never read as values: whatever they hold does not reach the output.
 * CVAR_EUNSUPPORTED, without a write, where cvar_attention_prescaled returns it (a hole that hides all of keys [0, 64) from a level; a grid beyond 2^31).
 * kv8 16-byte aligned. */
int cvar_attention_kv8(const void* kv8, const float* kv_scale, const void* q, int R, int H, int Lmax, int q_off, int l,
                       const int* lvl_end_host, int n_lvl, const int* hole_host, void* out, float* lse, void* stream);

#ifdef __cplusplus
}
#endif
#endif
