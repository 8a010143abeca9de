/* cvar_accum.h - accumulating forms of the gradient producers of cvar.h (gradient accumulation over micro-batches); same rules as
 * cvar.h: plain pointers + sizes + stream, no allocation, asynchronous, negative `cvar_status` on error.
 *
 * The functions live in the same libcvar_hip.so.  Every one is its cvar.h namesake with one more argument, `accumulate`, in front of the stream:
 *   accumulate == 0: exactly the namesake - the same kernels, the same bits;
 *   accumulate != 0: every output element becomes fp32(old + plain), where `plain` is what the namesake writes for the same operands and `old` is
 *                    what the element held before the call: ONE IEEE add per element, performed last (after the fixed-order sum over token slices,
 *                    after the scale).  A window of micro-batches therefore holds, bit for bit, the sum in micro-batch order of what the plain
 *                    calls produce.  Nothing else is read-modify-written: elements the namesake leaves alone stay untouched, the split partials
 *                    go to the workspace as before and no slice ever reads the output.
 * cvar_colsum and cvar_rowsum of cvar.h already take such a flag with the same meaning.
 * Adding these entry points changed no signature of cvar.h or cvar_serve.h: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_ACCUM_H
#define CVAR_ACCUM_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cvar_gemm_tn: C[n][k] (and colsum_a[n], if given) (+)= sum_t A[t][n] B[t][k].  One slice: the accumulator epilogue loads the 128-byte row segments
 * it is about to store; token split (ws given, >= 24 K steps per slice): the reduction adds the old C after the last slice.  The second half of a
 * half-filled last column tile is neither loaded nor stored.  Both tile heights take the flag. */
int cvar_gemm_tn_acc(const void* A, int64_t lda, const void* B, int64_t ldb, float* C, int64_t ldc, int T, int Nn, int Kk,
                     float* ws, int64_t ws_bytes, float* colsum_a, int accumulate, void* stream);

/* cvar_lora_wgrad: out[n * os_n + j * os_j] (+)= scale * sum_m drop(Y)[m,n] Z[m,j], j < r (the finishing pass adds the old value last). */
int cvar_lora_wgrad_acc(const void* Y, int64_t ldy, const void* Z, int64_t ldz, int M, int N, int r, int dtype, float scale, float p, uint64_t seed,
                        uint32_t tag, float* ws, int64_t ws_floats, float* out, int64_t os_n, int64_t os_j, int accumulate, void* stream);

/* cvar_wordembed_grad: dW[c][j], db[c] (+)= ... (the slice reduction adds the old value last). */
int cvar_wordembed_grad_acc(const float* dx, int64_t ldx, int rows_per_sample, int skip, const float* tok, int n_per_sample, int B, int C, int Cvae,
                            float* dW, float* db, float* ws, int accumulate, void* stream);

/* y[i] = fp32(y[i] + x[i]), i < n; x and y must not overlap, both 4-byte aligned.  For gradients that cannot take the flag at their producer: entries
 * derived from other entries of the gradient buffer (they must be derived from THIS micro-batch's values, not from the window's sum) and the
 * cvar_gemm fallbacks are computed into a staging buffer exactly as in a plain step, then added here. */
int cvar_add_inplace(float* y, const float* x, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
