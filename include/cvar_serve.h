/* cvar_serve.h - entry points with no counterpart in the reference; same rules as cvar.h: plain pointers + sizes + stream,
 * no allocation, asynchronous, negative `cvar_status` on error.
 *
 * The functions live in the same libcvar_hip.so as those of cvar.h.  They are versioned on their own: cvar_serve_version() bumps on
 * any signature change in THIS header, cvar_abi_version() stays the version of cvar.h.  Adding an entry point changes no signature and
 * leaves the version alone: cvar_edit_force_table, cvar_cfg_sample_edit, cvar_lora_down_rows,
 * cvar_score_rows, cvar_ln_modulate_split3, cvar_quant_rows_fp8, cvar_ln_modulate_fp8 and cvar_gemm_fp8 joined at version 1.
 */
#ifndef CVAR_SERVE_H
#define CVAR_SERVE_H

#include "cvar.h"

#ifdef __cplusplus
extern "C" {
#endif

int cvar_serve_version(void);               /* 1 */

/* ---------------------------------------------------------------------------------------------
 * CFG combine + sampling with one parameter set per batch row (a row = one request of a serving batch).
 * As cvar_cfg_sample, with its scalar coef_host / top_k / top_p / seed / seed_dev replaced by DEVICE tables indexed by the batch row b:
 *   coef  [B][4] fp32   combine weights of THIS stage (entries >= nrep are not used), added up as ((c0 l0 + c1 l1) + c2 l2) + c3 l3 with
 *                       separately rounded products.  The caller rounds them to fp32 on the host; the kernel never derives them from a
 *                       guidance scale (a contracted 1 + cfg * ratio would change bits);
 *   top_k [B]    int32  <= 0 or >= V: no top-k filter; 1: greedy - argmax, lowest index on ties, kept = 1, the same id in all n_draw
 *                       rows - inside the same launch, for that row only;
 *   top_p [B]    fp32   <= 0: no nucleus filter;
 *   seed  [B]    uint64 stored as its int64 bit pattern.
 * The draw of row b, draw row d, token t is keyed by (seed[b], stage, d, t): the key cvar_cfg_sample forms at B = 1.  Row b of one call
 * therefore equals - idx_out (all n_draw rows), combined, margin and kept, bit for bit - the call
 *   cvar_cfg_sample(logits of row b, B = 1, ..., coef[b], top_k[b], top_p[b], seed[b], seed_dev = NULL, ...)
 * and does not depend on the slot b or on the other rows.
 * logits [nrep*B][l][ldv], idx_out [n_draw*B][l], the optional combined [B][l][V] / margin [B][l] / kept [B][l] and ldv: as there.
 * nrep 1..4, n_draw 1..4, V <= 4096 (CVAR_EUNSUPPORTED otherwise); a NULL table is CVAR_EINVAL.  The values IN the tables are not
 * checked (they are on the device): the caller keeps top_k <= V as it does for the scalar call.
 * expo, soft_out: the caller-drawn noise and the more_smooth output of cvar_cfg_sample have no per-row form; both must be NULL,
 * anything else returns CVAR_EUNSUPPORTED (never a silent fallback to the counter draw or to hard ids). */
int cvar_cfg_sample_rows(const float* logits, int B, int nrep, int l, int V,
                         const float* coef /* [B][4] */, const int32_t* top_k /* [B] */, const float* top_p /* [B] */, const int64_t* seed /* [B] */,
                         int stage, int n_draw, int32_t* idx_out, float* combined, float* margin, int32_t* kept, int ldv,
                         const float* expo /* must be NULL */, float* soft_out /* must be NULL */, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Region-constrained generation: keep the source's tokens where a latent-resolution mask says "keep", sample the others.
 *
 * cvar_edit_force_table: one launch turns the keep masks of a batch into the forced-token table of every scale.
 *   keep_ctrl / keep_img [B][S][S] uint8 (non-zero = keep the source there), each may be NULL (nothing of that half is kept);
 *   src_ctrl / src_img   [B][sum pn^2] int32, the half's multi-scale ids, scale after scale (required where the half's mask is given);
 *   patch_nums           HOST array of the nstage scale sizes (1 <= pn <= S, the last one == S; nstage 1..16);
 *   forced               [B][L] int32, L = sum mask_factor * pn^2, in the token order of generation: per scale the two halves, control first
 *                        when mask_first != 0 and image first otherwise (mask_factor == 1: the image half only; keep_ctrl must be NULL).
 * Cell (i, j) of scale pn covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns - the bins of area
 * interpolation, with which the quantizer forms that token.  The cell is kept iff 2 * (kept latent cells in the bin) > bin size: a strict
 * majority in integers, an exact half stays free; at the last scale the rule is the mask itself.
 * forced = the source id of that scale and cell where kept, -1 where free.  The ids are copied, not checked. */
int cvar_edit_force_table(const uint8_t* keep_ctrl, const uint8_t* keep_img, const int32_t* src_ctrl, const int32_t* src_img,
                          const int* patch_nums /* host, [nstage] */, int nstage, int B, int S, int mask_first, int mask_factor,
                          int32_t* forced /* [B][L] */, void* stream);

/* cvar_cfg_sample_edit: cvar_cfg_sample_rows with per-token forcing.  forced points at THIS stage's slice of the table, row stride ldf
 * (>= l): token (b, t) reads forced[b * ldf + t].
 *   >= 0: that id goes to all n_draw rows of idx_out, kept = 0, margin = +inf, its combined row is NOT written, and no logit of the token
 *         is read (they may hold anything, NaN included);
 *   <  0: the token is what cvar_cfg_sample_rows gives on the same inputs - idx_out, combined, margin and kept, bit for bit.
 * forced == NULL or ldf < l is CVAR_EINVAL; every other argument is checked as cvar_cfg_sample_rows checks it. */
int cvar_cfg_sample_edit(const float* logits, int B, int nrep, int l, int V,
                         const float* coef /* [B][4] */, const int32_t* top_k /* [B] */, const float* top_p /* [B] */, const int64_t* seed /* [B] */,
                         int stage, int n_draw, int32_t* idx_out, float* combined, float* margin, int32_t* kept, int ldv,
                         const float* expo /* must be NULL */, float* soft_out /* must be NULL */,
                         const int32_t* forced, int ldf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-request LoRA adapters: the per-row form of cvar_lora_down for inference (no dropout).  Joined at version 1.
 * The M = R * l rows of x are R sequences of l rows; row m belongs to sequence m / l and uses the adapter slot[m / l].
 *   x      [M][ldx]            compute dtype (CVAR_BF16 / CVAR_F32), K columns read;
 *   A_bank [n_slots][16][lda]  compute dtype, the down matrices of the bank; rows >= an adapter's rank are zero;
 *   scale  [n_slots] fp32      DEVICE table, alpha / r of every slot;
 *   slot   [R]       int32     DEVICE table; -1: no adapter.  The values are not checked (they are on the device): the caller keeps
 *                              them in [-1, n_slots);
 *   xa     [M][ldxa]           the K-augmented operand: the kernel owns the kpad columns [K, K + kpad) of every row;
 *   kpad                       a multiple of 16, >= 16 * n_slots (CVAR_EINVAL otherwise);
 *   x_copy [M][ld_copy]        optional: receives x bit for bit in the same pass (usually xa itself with ld_copy = ldxa).  NULL where the
 *                              producer already wrote the wide buffer through its ldc (then x == xa, ldx == ldxa is allowed: the
 *                              kernel reads columns < K and writes columns >= K only).
 * Columns K + 16 slot .. K + 16 slot + 15 of row m hold scale[slot] * x[m] A_slot^T; EVERY other one of the kpad columns is written as
 * zero (the buffers of a generation pass are uninitialised, and a NaN there would reach the GEMM); a slot = -1 row gets kpad zeros.
 * Nothing outside [K, K + kpad) and the copy is touched.
 * Row m with slot s equals, bit for bit, what cvar_lora_down(p = 0, r = 16, scale = scale[s]) writes for that row with A_bank[s]: both
 * kernels run one reduction body.  One block serves one (sequence, 16-row chunk), so it stages the A slabs of one adapter only.
 * n_slots 1..8, R >= 1, l >= 1, a NULL table: CVAR_EINVAL; K, ldx, lda, ldxa (>= K + kpad) and the pointers are checked as
 * cvar_lora_down checks them (CVAR_EUNSUPPORTED). */
int cvar_lora_down_rows(const void* x, int64_t ldx, const void* A_bank, int64_t lda, const float* scale /* [n_slots] */,
                        const int32_t* slot /* [R] */, int n_slots, int R, int l, void* xa, int64_t ldxa, int kpad,
                        void* x_copy, int64_t ld_copy, int K, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Token log-probabilities: score a GIVEN id per token under the CFG-combined distribution the sampler draws from.  Joined at version 1.
 * One workgroup per token (b, t), in the shape of cvar_cfg_sample_rows, and with its inputs:
 *   logits [nrep*B][l][ldv] fp32, B, nrep 1..4, l, V <= 4096, ldv (0: V; otherwise >= V);
 *   coef   [B][4] fp32   the device table of THIS stage - the very table the sampler reads;
 *   target [B][ldt] int32, ldt >= l: token (b, t) reads target[b * ldt + t] (a column slice of a wider table will do).
 * Outputs, each optional (all five NULL: CVAR_EINVAL), x = the combined row of the token, t_id = its target.  The four per-token outputs
 * share the row stride ldo (0: l; otherwise >= l): token (b, t) is written at b * ldo + t, so one scale's columns of [B][L] buffers will do.
 *   combined [B][l][V] fp32  ((c0 l0 + c1 l1) + c2 l2) + c3 l3 with separately rounded products: the sampler's `combined`, bit for bit (one text);
 *   logprob  [B][l]    fp32  (x_t - m) - logf(S), m = the row maximum, S = sum_e expf(x_e - m) (accurate expf / logf, no fast-math);
 *   entropy  [B][l]    fp32  logf(S) - (sum_e expf(x_e - m) (x_e - m)) / S; terms with expf(...) == 0 are skipped, so a -inf logit carries
 *                            zero mass and produces no NaN;
 *   rank     [B][l]    int32 the number of codes e with x_e > x_t, or x_e == x_t and e < t_id: rank 0 is exactly the greedy kernel's id
 *                            (the lowest index on ties);
 *   argmax   [B][l]    int32 the id cvar_cfg_sample gives that token at top_k = 1.
 * The distribution is the UNFILTERED combined one: a top-k / top-p kept set is not renormalised over.
 * target < 0: the token has no target - logprob = 0 and rank = -1; entropy, argmax and combined are written as usual.
 * The order of evaluation is fixed and independent of B and of the slot b: thread tid of 256 owns elements tid + 256 j, j = 0..15, and adds
 * them in increasing j; a 64-lane xor-shuffle tree follows; the four wave partials are added in order 0..3.  No atomics: row b of a call
 * equals the B = 1 call on that row, bit for bit.
 * Out of contract: target values >= V (the caller checks its ids; the kernel reads nothing for them and treats them as "no target"),
 * NaN logits, and rows whose maximum is not finite.
 * nrep outside 1..4 or V > 4096: CVAR_EUNSUPPORTED; a NULL logits / coef / target, ldt < l, 0 < ldo < l, V < 1, 0 < ldv < V: CVAR_EINVAL. */
int cvar_score_rows(const float* logits, int B, int nrep, int l, int V, const float* coef /* [B][4] */,
                    const int32_t* target /* [B][ldt] */, int ldt, float* combined, float* logprob, float* entropy,
                    int32_t* rank, int32_t* argmax, int ldo, int ldv, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Split-bf16 transformer mode (`gemm_precision='bf16x3'` of an fp32 model).  Joined at version 1.
 * The contract of the mode, stated once:
 *   - a value x is carried as hi = bf16(x), lo = bf16(x - hi) (round to nearest even; x - hi is exact in fp32), so it is used to
 *     |x - hi - lo| <= 2^-17 |x|;
 *   - a product a w is taken as a_hi w_hi + a_lo w_hi + a_hi w_lo: the only dropped term is a_lo w_lo <= 2^-16 |a w|;
 *   - the three products are three K segments of ONE bf16 cvar_gemm over K' = 3 K with an fp32 output: activation rows
 *     [hi(K) | lo(K) | hi(K)] (lda = 3 K: what cvar_split3 and this entry point write), weight rows [w_hi(K) | w_hi(K) | w_lo(K)] (ldw = 3 K),
 *     accumulated in fp32 in the K order of whichever bf16 kernel cvar_gemm picks for the call (segment 0 first, then 1, then 2 inside a K slice);
 *   - everything else of the model - residual stream, adaLN table, K/V arena, attention, sampler, quantizer - is the fp32 mode's.
 * cvar_ln_modulate_split3 is cvar_ln_modulate with that store: y = LN(x[m]) * (1 + scale) + shift in cvar_ln_modulate's fp32 arithmetic and order
 * (one wave per row, the row in registers), then out[m] = [hi(y) | lo(y) | hi(y)], out [M][3 C] bf16.  Bit for bit
 * cvar_split3(cvar_ln_modulate(..., CVAR_F32)) in one pass: the fp32 row is never written.
 * Arguments and refusals as cvar_ln_modulate (C % 4 == 0, C <= 2048, ld_ada % 4 == 0; NULL pointers, M <= 0 or rows_per <= 0: CVAR_EINVAL);
 * x, scale and shift 16-byte aligned, out 8-byte aligned.  A refused call writes nothing. */
int cvar_ln_modulate_split3(const float* x, const float* scale, const float* shift, int64_t ld_ada, int rows_per,
                            void* out_bf16 /* [M][3 C] */, int M, int C, float eps, void* stream);

/* ---------------------------------------------------------------------------------------------
 * e4m3 linear layers (`gemm_precision='fp8'` of a bf16 model).  Joined at version 1.
 * The mode is the bf16 mode in everything except the qkv, proj, fc1 and fc2 GEMMs of every block: those take OCP e4m3 (e4m3fn) operands with one
 * power-of-two scale per row and accumulate in fp32; their epilogues are cvar_gemm's.  The contract, stated once:
 *
 * Quantising a row x[0..K) (fp32 or bf16 values):
 *   - amax = max |x_k|;
 *   - k = the smallest integer with amax <= 448 * 2^k, clamped to [-60, 120], read off the exponent and mantissa fields of amax
 *     (448 = 1.75 * 2^8: k = e - 8 for a mantissa <= 1.75, e - 7 above; no logarithm is taken);
 *   - scale = 2^k as fp32;
 *   - q_k = e4m3_rne(x_k * 2^-k): the product is exact (a result below the fp32 normal range rounds to zero either way), nothing exceeds 448,
 *     so nothing saturates; the one rounding is the conversion, to nearest, ties to even;
 *   - an all-zero row gets k = -60 and zero bytes (an entry -0.0 keeps its sign, here and in any row: its byte is 0x80, the e4m3 -0; so does a negative
 *     value that rounds to zero - the product does not tell the two zeros apart);
 *   - a row that holds a NaN or an Inf gets scale = 1 and every byte 0x7F (NaN): a broken activation shows instead of hiding;
 *   - bytes [K, ldq) of a row are zero, ldq = K rounded up to 128 (or any larger multiple of 128).
 * Product: acc[m,n] = sum_k q_a[m,k] q_w[n,k] into an fp32 accumulator, K ascending in blocks of 128 - one v_mfma_scale_f32_16x16x128_f8f6f4 per
 * block - and no K slices in any plan: the bits of a row do not depend on M, the tile or the batch.  The hardware block scales of the MFMA are the
 * constant 1.0 (e8m0 0x7F); MX block scales are not used.  Inside a block the sum is the instruction's, and how the instruction sums is NOT part of
 * this contract.  What the tests hold the call to: exact results for integer-valued operands whose partial sums stay below 2^24, and the bound of
 * tests/fp8_ref.py otherwise.  An observation, not a promise (tools/fp8_mfma_probe.py reproduces it with exact data, DESIGN.md 4i records one run on
 * an MI355X): products far below the largest of their group of 8 consecutive k - from 2^-14 of it on - did not reach the sum, and group sums were
 * truncated, not rounded, into the accumulator; operands inside a few binades were summed exactly.
 * The value the epilogue sees is (acc * a_scale[m]) * w_scale[n], in that order (both factors are powers of two); bias, alpha, split_alpha,
 * GELU, gate, residual, row remap, column split and the output cast follow as cvar_gemm does them.
 *
 * cvar_quant_rows_fp8: the row pass, one wave per row.  x [M][ldx] of x_dtype (CVAR_BF16 / CVAR_F32), K columns read; q [M][ldq] bytes, scale [M] fp32.
 * ldq % 128 == 0, ldq >= K, ldx >= K, q 4-byte aligned (CVAR_EUNSUPPORTED otherwise); NULL pointers, M <= 0 or K <= 0: CVAR_EINVAL.  A refused call
 * writes nothing.  With fp32 input it also quantises the weight stacks when a model packs them. */
int cvar_quant_rows_fp8(const void* x, int x_dtype, int64_t ldx, int64_t M, int K, void* q, int64_t ldq, float* scale, void* stream);

/* cvar_ln_modulate with the e4m3 store: y = LN(x[m]) * (1 + scale) + shift in cvar_ln_modulate's fp32 arithmetic and order, rounded to bf16, and that
 * row quantised as above - bit for bit cvar_quant_rows_fp8(the bf16 rows of cvar_ln_modulate(..., CVAR_BF16)) in one pass (the row is in registers,
 * its amax is one wave reduction).  Arguments and refusals as cvar_ln_modulate_split3; q [M][ldq] bytes (ldq % 128 == 0, ldq >= C - any such ldq: the
 * bytes [C, ldq) of every row are written as zeros - 16-byte aligned),
 * q_scale [M] fp32.  A refused call writes nothing. */
int cvar_ln_modulate_fp8(const float* x, const float* scale, const float* shift, int64_t ld_ada, int rows_per,
                         void* q /* [M][ldq] */, int64_t ldq, float* q_scale /* [M] */, int M, int C, float eps, void* stream);

/* cvar_gemm on e4m3 operands.  d->A [M][lda] and d->W [N][ldw] are e4m3 bytes, lda / ldw in bytes; d->dtype is not read.  a_scale [M], w_scale [N] fp32.
 * Needs K % 128 == 0, lda and ldw multiples of 16 and >= K, A and W 16-byte aligned.  Honoured: bias, alpha, act NONE / GELU_TANH, gate (+ gate_rows), residual
 * (fp32 in place included), row remap + column split + split_alpha, bf16 or fp32 C; any M and N.
 * Fast path of the epilogue (16-byte accesses of whole row segments; every other call takes the element-wise form: the same bits, and the d24 B = 512
 * step 1.4x as long when the model's calls took it): N, ldc, ldr, ldg, split_n and ld_split multiples of 4; w_scale, bias, gate and an fp32 C / C_split / residual 16-byte
 * aligned, a bf16 C / C_split / residual 8-byte aligned.  conv, batch > 1, ws, ln_out, gn_part, pre_act, aux,
 * gate_scale and GELU_GRAD return CVAR_EUNSUPPORTED before any write; tile_cfg, stagger and group_m are not read (no plan changes a bit).
 * One 256x256 tile (eight waves) for M >= 1024, a 128x128 tile (four waves) below; tails of any size. */
int cvar_gemm_fp8(const cvar_gemm_desc* d, const float* a_scale, const float* w_scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif
