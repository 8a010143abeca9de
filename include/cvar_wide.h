/* cvar_wide.h - the adaLN row kernels for models wider than 2048 channels; same rules as cvar.h: plain pointers + sizes + stream, no
 * allocation, asynchronous, negative `cvar_status` on error.  The functions live in the same libcvar_hip.so.
 *
 * cvar_ln_modulate, cvar_ln_modulate_split3 and cvar_ln_modulate_fp8 keep one row in one wave's registers and stop at C = 2048 (eight 16-byte vectors
 * per lane).  Each entry point here takes its namesake's arguments and serves C % 4 == 0, C <= CVAR_WIDE_CMAX:
 *   - C <= 2048: it launches the very kernel its namesake launches - the same bits, the same cost; a caller needs one function whatever the width;
 *   - 2048 < C <= CVAR_WIDE_CMAX: the same kernel text with nine to twelve vectors per lane.  The arithmetic, its order and the stores are the
 *     namesake's: y = ((x - mean) * rstd) * (1 + scale) + shift in fp32, mean and variance over exactly C elements (lane-strided sums, one xor-shuffle
 *     tree each), rstd = rsqrt(var + eps), modulation row = row / rows_per, 16-byte loads (a row's loads of x issued back to back), vector stores only.
 * The mutual contracts hold at every width, bit for bit:
 *   cvar_ln_modulate_split3_wide == cvar_split3(cvar_ln_modulate_wide(..., CVAR_F32));
 *   cvar_ln_modulate_fp8_wide    == cvar_quant_rows_fp8(the bf16 rows of cvar_ln_modulate_wide(..., CVAR_BF16)), bytes [C, ldq) zero, one
 *                                   power-of-two scale per row (the row rule of cvar_serve.h).
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        a NULL pointer, M <= 0 or rows_per <= 0;
 *   CVAR_EUNSUPPORTED (-2)  C > CVAR_WIDE_CMAX, C % 4, ld_ada % 4, an unknown out_dtype; split3 / fp8: x, scale or shift not 16-byte aligned, out not
 *                           8-byte (split3) or q not 16-byte (fp8) aligned; fp8: ldq % 128 or ldq < C.
 * Adding these entry points changed no signature of cvar.h, cvar_serve.h, cvar_accum.h or cvar_kvcache.h: cvar_abi_version() and cvar_serve_version()
 * stay where they were.
 */
#ifndef CVAR_WIDE_H
#define CVAR_WIDE_H

#include "cvar.h"

/* the widest row: twelve 16-byte vectors per lane of a 64-lane wave (embed_dim 3072 = depth 48 at 64 channels per head) */
#define CVAR_WIDE_CMAX 3072

#ifdef __cplusplus
extern "C" {
#endif

int cvar_ln_modulate_wide(const float* x, const float* scale, const float* shift, int64_t ld_ada, int rows_per,
                          void* out, int out_dtype, int M, int C, float eps, void* stream);

int cvar_ln_modulate_split3_wide(const float* x, const float* scale, const float* shift, int64_t ld_ada, int rows_per,
                                 void* out_bf16 /* [M][3 C] */, int M, int C, float eps, void* stream);

int cvar_ln_modulate_fp8_wide(const float* x, const float* scale, const float* shift, int64_t ld_ada, int rows_per,
                              void* q /* [M][ldq] */, int64_t ldq, float* q_scale /* [M] */, int M, int C, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
