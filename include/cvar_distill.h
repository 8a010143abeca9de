/* cvar_distill.h - the soft-target (distillation) loss beside cvar_ce_fwd_bwd (guidance distillation); same rules as cvar.h: plain
 * pointers + sizes + stream, no allocation, asynchronous, negative `cvar_status` on error.  The function lives in the same libcvar_hip.so.
 *
 * cvar_kd_fwd_bwd: one 256-thread workgroup per token row m of the student logits [M][V] fp32 (row stride V) and the teacher logits [M][ldt] fp32
 * (first V columns used, ldt >= V), 64-bit row offsets, vector stores only, no atomics; a row's results depend on that row's inputs alone (not on M,
 * not on the row's place in the batch).  The teacher is given as logits, not probabilities: the kernel normalises it itself.
 *
 * Per row, in fp32, one rounding per operation, no contraction, x the student row and z the teacher row:
 *   1. mx = max_v x_v, se = sum_v __expf(x_v - mx): the loops, the wave tree and the (w0 + w1) + (w2 + w3) of cvar_ce_fwd_bwd;  lse_x = logf(se) + mx
 *   2. mz, sz, lse_z over z with the same text
 *   3. p_v = __expf(x_v - mx) * (1 / se),  q_v = __expf(z_v - mz) * (1 / sz)
 *   4. kl = sum_v q_v * ((z_v - lse_z) - (x_v - lse_x)): per thread in the loop's order (v = t, t + 256, ...), then the same wave tree and the
 *      same four-wave combination
 *   5. loss_tok[m] = kl                                       KL(teacher || student) of the row
 *   6. dlogits[m, v] = (p_v - q_v) * g,  g = (weight ? weight[m] : 1.0f) * gscale, as cvar_ce_fwd_bwd forms it
 * Outputs: loss_tok [M] is required; dlogits ([M][V], out_dtype CVAR_F32 or CVAR_BF16 as cvar_ce_fwd_bwd takes it) is optional (NULL = not written).
 * Identities, bit for bit in both output dtypes:
 *   (a) a teacher row equal to the student row (same values, separate buffers): loss_tok == 0 and every dlogits element compares equal to 0;
 *   (b) a teacher row that is 0 at column t and -200 elsewhere: q is exactly one-hot (__expf underflows to 0), and loss_tok and dlogits are those
 *       of cvar_ce_fwd_bwd(target = t, weight, gscale).
 * Out of contract: non-finite inputs; |x| or |z| so large that lse overflows.
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        NULL logits, teacher or loss_tok; M <= 0; V <= 1; ldt < V;
 *   CVAR_EUNSUPPORTED (-2)  an unknown out_dtype.
 * Adding this entry point changed no signature of the other headers: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_DISTILL_H
#define CVAR_DISTILL_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

int cvar_kd_fwd_bwd(const float* logits, const float* teacher, int ldt, const float* weight, float gscale, float* loss_tok, void* dlogits,
                    int out_dtype, int64_t M, int V, void* stream);

#ifdef __cplusplus
}
#endif
#endif
