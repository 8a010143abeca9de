/* cvar_region.h - regional guidance: several class labels per sample, weighed per token by latent-resolution region maps; same rules
 * as cvar.h: plain pointers + sizes + stream, no allocation, asynchronous, negative `cvar_status` on error.  The functions live in the same
 * libcvar_hip.so.
 *
 * A sample carries K labels (1 <= K <= 3): its transformer rows are [label_0 ; ... ; label_{K-1} ; unconditional], nrep = K + 1 <= 4, the sampler's
 * four weight slots.  The combine stays ((c0 l0 + c1 l1) + c2 l2) + c3 l3 with separately rounded products; what is new is that the four weights
 * are read per TOKEN from a table that one launch derives from the maps.
 *
 * cvar_region_coef_table: one wave per token, one launch for all scales.
 *   regions    [B][K][S][S] fp32  non-negative weights at latent resolution, S = patch_nums[nstage - 1]; every latent cell has a positive sum over k;
 *   strength   [B][S][S]    fp32  >= 0, multiplies the guidance scale per latent cell; NULL = 1;
 *   cfg        [B][K]       fp64  DEVICE table of the guidance scales;
 *   patch_nums HOST array of the nstage scale sizes (1 <= pn <= S, the last one == S; nstage 2..16);
 *   coef       [B][L][4]    fp32  L = sum mask_factor * pn^2, in the token order of generation: per scale the halves in mask_first order, the order of
 *                                 cvar_edit_force_table.  Both halves of a sample read the same maps, so mask_first changes no value; it is taken so
 *                                 that the two table calls of one request read alike.  16-byte aligned.
 * The token of scale si, cell (i, j) of the pn x pn map covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns (the
 * bins of cvar_edit_force_table).  All in float64, from the fp32 maps:
 *   n_k(c)  = w_k(c) / (w_0(c) + ... + w_{K-1}(c))        per latent cell c of the bin, the sum in index order
 *   wbar_k  = mean of n_k over the bin,   gbar = mean of strength over the bin (1 without strength)
 *   ratio   = si / (nstage - 1)
 *   t_k     = (cfg[b][k] * gbar) * ratio
 *   coef_k  = wbar_k * (1 + t_k)                           k < K
 *   coef_K  = -(wbar_0 * t_0 + ... )                       summed in index order
 *   slots above K are 0.
 * Each value is rounded to fp32 once.  No product is contracted.  The means are sums in a fixed order (lane q of 64 adds the cells q, q + 64, ... of
 * the bin in row-major order, a xor-shuffle tree follows) divided by the bin size: the same inputs give the same bits on every run, and every entry
 * lies within 1 fp32 ulp of the exactly summed float64 value.  A bin in which one label holds all the weight and the others none is exact.
 * With K = 1 and no strength the table holds [1 + t, -t, 0, 0] with t = cfg * ratio in float64: bit for bit the per-request table of
 * cvar_cfg_sample_rows.  No atomics, no LDS, vector stores only, 64-bit indexing.
 * Out of contract (the host checks the maps): negative or non-finite weights, a latent cell whose weights sum to 0 (its 0 / 0 shows as a NaN).
 * Refusals, all before any launch and without a write:
 *   CVAR_EINVAL (-1)        K outside 1..3; NULL regions, cfg, patch_nums or coef; B <= 0; S <= 0; nstage outside 2..16 (ratio needs two scales);
 *                           a pn outside 1..S, or the last one != S;
 *   CVAR_EUNSUPPORTED (-2)  mask_factor not 1 or 2; S > 1024; coef not 16-byte aligned; B * L >= 2^25.
 *
 * cvar_cfg_sample_map: cvar_cfg_sample_rows (include/cvar_serve.h) with the combine weights read per token.  coef points at THIS stage's slice of
 * the table, row stride ldc TOKENS (>= l): token (b, t) reads the four floats at coef + (b * ldc + t) * 4.  forced / ldf: cvar_cfg_sample_edit's
 * pair with its meaning - token (b, t) with forced[b * ldf + t] >= 0 gets that id in all n_draw rows, kept = 0, margin = +inf, no combined row, and
 * none of its logits is read; forced == NULL forces nothing (ldf is then not read).  Every other token is, bit for bit in idx_out, combined, margin
 * and kept, what cvar_cfg_sample_rows gives that token with its four weights as the row's: one sampler text serves all forms, and the draw stays
 * keyed by (seed[b], stage, d, t).  top_k / top_p / seed stay per batch row.  Refusals: as cvar_cfg_sample_rows (expo and soft_out must be NULL:
 * CVAR_EUNSUPPORTED), and CVAR_EINVAL on ldc < l or on forced != NULL with ldf < l.
 *
 * cvar_score_map: cvar_score_rows (include/cvar_serve.h) with the same per-token weights (coef, ldc as above), so that a regional generation
 * reports token log-probabilities; outputs, order of evaluation and refusals are cvar_score_rows', plus CVAR_EINVAL on ldc < l.
 *
 * Adding these entry points changed no signature of the other headers: cvar_abi_version() and cvar_serve_version() stay where they were.
 */
#ifndef CVAR_REGION_H
#define CVAR_REGION_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

int cvar_region_coef_table(const float* regions, const float* strength, const double* cfg, const int* patch_nums, int nstage, int B, int K, int S,
                           int mask_first, int mask_factor, float* coef, void* stream);

int cvar_cfg_sample_map(const float* logits, int B, int nrep, int l, int V, const float* coef, int ldc, const int32_t* top_k, const float* top_p,
                        const int64_t* seed, int stage, int n_draw, int32_t* idx_out, float* combined, float* margin, int32_t* kept, int ldv,
                        const float* expo, float* soft_out, const int32_t* forced, int ldf, void* stream);

int cvar_score_map(const float* logits, int B, int nrep, int l, int V, const float* coef, int ldc, const int32_t* target, int ldt, float* combined,
                   float* logprob, float* entropy, int32_t* rank, int32_t* argmax, int ldo, int ldv, void* stream);

#ifdef __cplusplus
}
#endif
#endif
