/* cvar_policy.h - the clipped policy-gradient loss beside cvar_ce_fwd_bwd (policy-gradient fine-tuning on token ids); same rules as
 * cvar.h: plain pointers + sizes + stream, no allocation, asynchronous, negative `cvar_status` on error.  The function lives in the same libcvar_hip.so.
 *
 * cvar_pg_fwd_bwd: one 256-thread workgroup per token row m of logits [M][V] fp32 (row stride V), 64-bit indexing, vector stores only, no atomics; a
 * row's results depend on that row's inputs alone (not on M, not on the row's place in the batch).
 *
 * Per row: target[m] (int32 in [0, V)), adv[m] (fp32, signed), weight[m] (or NULL = 1), old_lp[m] (or NULL = ratio exactly 1.0f), ref_lp[m] (or NULL =
 * no KL term).  Scalars: clip_lo, clip_hi >= 0 (they may differ), kl_coef >= 0, gscale.  In fp32, one rounding per operation, no contraction:
 *   1. mx = max_v x_v, se = sum_v __expf(x_v - mx), p_v = __expf(x_v - mx) * (1 / se): the loops and the reduction order of cvar_ce_fwd_bwd;
 *   2. lp = -((logf(se) + mx) - x_t);                       logprob[m]: bit for bit the negative of cvar_ce_fwd_bwd's loss_tok[m]
 *   3. r  = expf(lp - old_lp[m]) (accurate expf), or 1.0f;  ratio[m]
 *   4. s1 = r * a,  s2 = min(max(r, 1 - clip_lo), 1 + clip_hi) * a,  active = (s1 <= s2) - a tie is active;  clipped[m] = !active
 *      obj = min(s1, s2); with old_lp NULL - r is the constant 1 and min(s1, s2) the constant a - obj = a * lp, the score-function surrogate with the
 *      same gradient, so that the reported loss still says something and identity (a) below covers loss_tok;
 *   5. d  = ref_lp[m] - lp,  k = (expf(d) - d) - 1 (the k3 estimator of KL(policy || reference)), or 0;  kl[m]
 *   6. loss_tok[m] = -obj + kl_coef * k
 *   7. c  = (active ? s1 : 0) - kl_coef * (1 - expf(d))     = -d loss / d lp   (the second term is 0 without ref_lp)
 *   8. coef[m] = c * w;  g = coef[m] * gscale
 *   9. dlogits[m, v] = (p_v - onehot_v) * g                 = d loss / d x_v
 * Outputs: loss_tok [M] is required; logprob, ratio, kl, coef (fp32 [M]), clipped (int32 [M], 0 or 1) and dlogits ([M][V], out_dtype CVAR_F32 or
 * CVAR_BF16 as cvar_ce_fwd_bwd takes it) are each optional (NULL = not written).
 * Identities, bit for bit in both output dtypes:
 *   (a) adv == 1, old_lp == ref_lp == NULL: loss_tok and dlogits are those of cvar_ce_fwd_bwd(weight, gscale);
 *   (b) any adv, old_lp == ref_lp == NULL: dlogits are those of cvar_ce_fwd_bwd with the weight fp32(adv * weight);
 *   (c) always: dlogits are those of cvar_ce_fwd_bwd with the weight coef and the same gscale.
 * Out of contract: |lp - old_lp| or |ref_lp - lp| above 80 (expf leaves the normal range), NaN inputs, targets outside [0, V) (the row is read at the
 * target's column unchecked).
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        NULL logits, target, adv or loss_tok; M <= 0; V <= 1; clip_lo, clip_hi or kl_coef negative (or NaN);
 *   CVAR_EUNSUPPORTED (-2)  an unknown out_dtype.
 * Adding this entry point changed no signature of the other headers: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_POLICY_H
#define CVAR_POLICY_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

int cvar_pg_fwd_bwd(const float* logits, const int32_t* target, const float* adv, const float* weight, const float* old_lp, const float* ref_lp,
                    float clip_lo, float clip_hi, float kl_coef, float gscale, float* loss_tok, float* logprob, float* ratio, float* kl,
                    int32_t* clipped, float* coef, void* dlogits, int out_dtype, int64_t M, int V, void* stream);

#ifdef __cplusplus
}
#endif
#endif
