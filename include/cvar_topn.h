/* cvar_topn.h - the N most likely codes of the CFG-combined distribution beside cvar_score_rows, and the sparse soft-target loss
 * beside cvar_kd_fwd_bwd; same rules as cvar.h: plain pointers + sizes + stream, no allocation, asynchronous, negative `cvar_status`
 * on error.  Both functions live in the same libcvar_hip.so.
 *
 * cvar_score_topn: one 256-thread workgroup per token (b, t), as cvar_score_rows.  logits [nrep*B][l][ldv] fp32 (ldv 0 = V), coef [B][4] fp32 (the
 * sampler's table of this stage), nrep 1..4, V <= 4096, N 1..64, ldo the row stride of the outputs in tokens (0 = l).
 *   top_id      [B][ldo][N] int32     top_id[b, t, i] is the one code whose cvar_score_rows rank is i: combined value descending, then id ascending;
 *                                     values compare as floats (-0.0 ties with +0.0)
 *   top_logprob [B][ldo][N] fp32      bit for bit the logprob cvar_score_rows writes for target = top_id[b, t, i]: the same combine, the same row
 *                                     maximum m (the value of rank 0) and the same S = sum_e expf(x_e - m), summed in that kernel's order (thread tid
 *                                     owns e = tid + 256 j and adds in increasing j, a 64-lane xor tree, the wave partials 0..3 in order)
 *   tail_logprob [B][ldo] fp32        logf(S_tail) - logf(S), S_tail the sum of expf(x_e - m) over the codes NOT among the N in the same fixed
 *                                     order; -inf when that sum is 0.  Optional (NULL = not written)
 * i >= V: id -1, logprob -inf.  One of top_id / top_logprob may be NULL.  Row b of a call equals the B = 1 call on that row, bit for bit; no atomics.
 * Out of contract: NaN logits or weights.
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        NULL logits or coef; top_id and top_logprob both NULL; B <= 0; l <= 0; V < 1; 0 < ldo < l; 0 < ldv < V;
 *   CVAR_EUNSUPPORTED (-2)  nrep outside 1..4; V > 4096; N outside 1..64.
 *
 * cvar_kd_topn_fwd_bwd: one 256-thread workgroup per token row m of the student logits [M][V] fp32 (row stride V), 64-bit row offsets, vector stores
 * only, no atomics; a row's results depend on that row's inputs alone.  The teacher is sparse: t_id [M][N] int32 (an entry < 0 or >= V is unused;
 * duplicate ids are out of contract), t_lp [M][N] fp32 the teacher's log-probabilities of those codes, t_tail [M] fp32 the log of the teacher's mass
 * on every other code (NULL or -inf: no tail mass).
 *
 * Per row, in fp32, one rounding per operation, no contraction, x the student row:
 *   1. mx, se, lse_x = logf(se) + mx and p_v = __expf(x_v - mx) * (1 / se) exactly as cvar_kd_fwd_bwd forms them
 *   2. q_j = __expf(t_lp_j);  r = t_tail finite ? __expf(t_tail) : 0
 *   3. p_tail = sum of p_v over the v no slot lists: the loop, the wave tree and the (w0 + w1) + (w2 + w3) of se
 *   4. loss_tok[m] = sum_j q_j * (t_lp_j - (x_id_j - lse_x)) + (r > 0 ? r * (t_tail - logf(p_tail)) : 0): slot j on lane j of one wave (unused
 *      slots carry 0), its xor tree, the tail term added last.  This is KL(teacher || student) over the N + 1 cells {id_0}, .., {id_N-1}, {the rest}
 *   5. dlogits[m, v] = (p_v - q_j) * g where slot j lists v, (p_v * f) * g elsewhere;  f is exactly 1 when r == 0 and 1 - r / p_tail otherwise;
 *      g = (weight ? weight[m] : 1.0f) * gscale, as cvar_ce_fwd_bwd forms it
 * Outputs: loss_tok [M] is required; dlogits ([M][V], out_dtype CVAR_F32 or CVAR_BF16) is optional (NULL = not written).
 * Identity, bit for bit in both output dtypes: N = 1, t_lp = 0, no tail gives cvar_ce_fwd_bwd(target = t_id)'s loss_tok and dlogits.
 * Out of contract: non-finite logits; r > 0 with p_tail == 0.
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        NULL logits, t_id, t_lp or loss_tok; M <= 0; V <= 1;
 *   CVAR_EUNSUPPORTED (-2)  an unknown out_dtype; N outside 1..64; V > 32768 (the slot table of a row lives in LDS).
 * Adding these entry points changed no signature of the other headers: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_TOPN_H
#define CVAR_TOPN_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

int cvar_score_topn(const float* logits, int B, int nrep, int l, int V, const float* coef, int N, int32_t* top_id, float* top_logprob,
                    float* tail_logprob, int ldo, int ldv, void* stream);

int cvar_kd_topn_fwd_bwd(const float* logits, const int32_t* t_id, const float* t_lp, const float* t_tail, int N, const float* weight, float gscale,
                         float* loss_tok, void* dlogits, int out_dtype, int64_t M, int V, void* stream);

#ifdef __cplusplus
}
#endif
#endif
