"""ORACLE (test infrastructure only - never imported by the product path).

Level-masked attention (include/cvar.h cvar_attention / cvar_attention_bwd) and the cos-attention pre-pass
(cvar_cos_qk_norm / cvar_cos_qk_norm_bwd) restated in plain torch float64 on the host, in three layers:

* the contract: ``visibility`` builds the [l][l] mask from (lvl_end, holes) with nothing shared with the kernels' level tables;
* the exact answer: ``attention_fwd_bwd_f64`` / ``cos_qk_norm_fwd_bwd_f64`` run torch.autograd in float64 on the operands as given;
* the rounding yardstick: ``attention_fwd_emulated`` / ``attention_bwd_emulated`` / ``cos_qk_norm_bwd_emulated`` repeat the same
  mathematics with the STORAGE POINTS of the bf16 kernels (what is rounded to bf16 or fp32, and where) and everything else in
  float64.  Their distance from the exact answer is what bf16 costs; a kernel that is several times further away has a
  different problem.

``row_error`` is the metric both are read in: per token row of one head, so that one wrong row cannot hide behind the largest
element of a whole tensor.

The cached (inference) forward - a K/V arena, this call's queries at positions [q_off, q_off + l), optionally prescaled by
scale * log2 e - has the same three layers: ``visibility_cached``, ``attention_cached_f64``, ``attention_cached_emulated``, read in
``row_error_fwd`` (the same metric with its floor taken per sample), on the cases of ``FWD_CASES`` / ``fwd_case_inputs``.

Layouts are the kernels': qkv [R][l][3*H*64] (q | k | v thirds, head-major inside a third), out / dout [R*l][H*64], lse [R][H][l];
cached form: q [R][l][H*64], kv [R][L][2*H*64] (k | v halves).
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

F64 = torch.float64
LN100 = math.log(100.0)


def bf16(t: torch.Tensor) -> torch.Tensor:
    """round to bf16 (nearest even), keep float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def f32(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(F64)


def visibility(l: int, lvl_end: Optional[Sequence[int]] = None, holes: Optional[Sequence[Tuple[int, int]]] = None) -> torch.Tensor:
    """bool [l][l]: row = query position, column = key position.  A query at position p of level k (the first level whose end lies
    above p; positions behind the last end belong to the last level) sees keys [0, lvl_end[k]) minus [hole_lo[k], hole_hi[k]);
    no levels: every query sees [0, l)."""
    vis = torch.zeros(l, l, dtype=torch.bool)
    if not lvl_end:
        vis[:] = True
        return vis
    for p in range(l):
        k = len(lvl_end) - 1
        for i, e in enumerate(lvl_end):
            if p < e:
                k = i
                break
        vis[p, :min(lvl_end[k], l)] = True
        if holes and holes[k][1] > holes[k][0]:
            vis[p, holes[k][0]:holes[k][1]] = False
    return vis


def split_heads(qkv: torch.Tensor):
    """[R][l][3*H*64] -> q, k, v as float64 [R][H][l][64]"""
    R, l, C3 = qkv.shape
    H = C3 // 192
    x = qkv.to(F64).view(R, l, 3, H, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def rows_to_heads(t: torch.Tensor, R: int) -> torch.Tensor:
    """[R*l][H*64] -> float64 [R][H][l][64]"""
    H = t.shape[-1] // 64
    return t.to(F64).view(R, -1, H, 64).permute(0, 2, 1, 3)


def heads_to_rows(t: torch.Tensor) -> torch.Tensor:
    """[R][H][l][64] -> [R*l][H*64]"""
    R, H, l, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(R * l, H * 64)


def merge_heads(dq: torch.Tensor, dk: torch.Tensor, dv: torch.Tensor) -> torch.Tensor:
    """three [R][H][l][64] -> [R][l][3*H*64]"""
    R, H, l, _ = dq.shape
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(R, l, 3 * H * 64)


class AttnF64(NamedTuple):
    out: torch.Tensor        # [R*l][H*64]
    lse: torch.Tensor        # [R][H][l]
    dqkv: torch.Tensor       # [R][l][3*H*64]


def attention_fwd_bwd_f64(qkv: torch.Tensor, dout: torch.Tensor, scale: float, vis: torch.Tensor) -> AttnF64:
    """softmax(q k^T * scale, over the visible keys) v and its gradients by torch.autograd, float64, from the operands as given"""
    R = qkv.shape[0]
    x = qkv.detach().to(F64).clone().requires_grad_(True)
    q, k, v = split_heads(x)
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, -math.inf)
    o = heads_to_rows(torch.softmax(s, -1) @ v)
    o.backward(dout.to(F64))
    return AttnF64(o.detach(), torch.logsumexp(s, -1).detach(), x.grad)


def visibility_cached(q_off: int, l: int, lvl_end: Optional[Sequence[int]] = None,
                      holes: Optional[Sequence[Tuple[int, int]]] = None) -> torch.Tensor:
    """bool [l][q_off + l]: rows q_off .. q_off + l - 1 of visibility(q_off + l, ...) - the queries of one cached call against the arena"""
    return visibility(q_off + l, lvl_end, holes)[q_off:q_off + l]


def drop_last_visible_key(vis: torch.Tensor) -> torch.Tensor:
    """the deliberately wrong mask of the sensitivity tests: every query loses the last key it sees"""
    last = vis.shape[1] - 1 - vis.flip(1).to(torch.int8).argmax(1)
    wrong = vis.clone()
    wrong[torch.arange(vis.shape[0]), last] = False
    return wrong


def q_heads(q: torch.Tensor) -> torch.Tensor:
    """[R][l][H*64] -> float64 [R][H][l][64]"""
    R, l, C = q.shape
    return q.to(F64).view(R, l, C // 64, 64).permute(0, 2, 1, 3)


def split_kv(kv: torch.Tensor):
    """[R][L][2*H*64] -> k, v as float64 [R][H][L][64]"""
    R, L, C2 = kv.shape
    x = kv.to(F64).reshape(R, L, 2, C2 // 128, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1]


def attention_cached_f64(q: torch.Tensor, kv: torch.Tensor, s_mul: float, vis: torch.Tensor):
    """softmax(q k^T * s_mul, over the visible keys) v in float64 from the operands as given: (out [R*l][H*64], lse [R][H][l]).
    q [R][l][H*64]: the call's queries; kv [R][L][2*H*64]: the arena, of which the vis.shape[1] = q_off + l first rows are read.
    Prescaled queries (q' = q * scale * log2 e): s_mul = ln 2, the scores q' . k live in the log2 domain; otherwise s_mul = scale."""
    k, v = split_kv(kv[:, :vis.shape[1]])
    s = (q_heads(q) @ k.transpose(-1, -2) * s_mul).masked_fill(~vis, -math.inf)
    return heads_to_rows(torch.softmax(s, -1) @ v), torch.logsumexp(s, -1)


def attention_bwd_formula(qkv, dout, out, lse, scale: float, vis, dtype=F64, drop_last_key: bool = False) -> torch.Tensor:
    """the textbook backward written out, no autograd:  P = exp(S scale - lse), D = rowsum(dO . O), dV = P^T dO, dS = P (dP - D),
    dQ = dS K scale, dK = dS^T Q scale - every step in ``dtype`` (float64: the second opinion on the autograd oracle; float32:
    the yardstick of the fp32 kernels).  drop_last_key: the deliberately wrong variant of the sensitivity test."""
    R = qkv.shape[0]
    q, k, v = (t.to(dtype) for t in split_heads(qkv))
    do, o = rows_to_heads(dout, R).to(dtype), rows_to_heads(out, R).to(dtype)
    vis = vis.clone()
    if drop_last_key:
        vis[:, -1] = False
    p = torch.exp(q @ k.transpose(-1, -2) * scale - lse.to(dtype)[..., None]) * vis.to(dtype)
    d = (do * o).sum(-1, keepdim=True)
    dv = p.transpose(-1, -2) @ do
    ds = p * (do @ v.transpose(-1, -2) - d)
    return merge_heads(ds @ k * scale, ds.transpose(-1, -2) @ q * scale, dv)


def attention_cached_emulated(q: torch.Tensor, kv: torch.Tensor, s_mul: float, vis: torch.Tensor):
    """forward with the bf16 kernels' storage points: the unnormalised P = exp(s - max) is computed in fp32 and rounded to bf16
    before P V, the row sum is taken from the fp32 P, out is rounded to bf16.  lse is returned twice - from the fp32 row sum
    (what the kernels store, formed in the exp2 domain as they form it) and from the row sum of the bf16-rounded P (what normalises a product of bf16 operands) - as
    (out [R*l][H*64], lse_fp32sum [R][H][l], lse_bf16sum [R][H][l]).
    q [R][l][H*64], kv [R][L][2*H*64], vis [l][<= L]; scores are q . k * s_mul (prescaled queries: s_mul = ln 2).
    The prescaled kernels shift by a LAZY maximum rounded to bf16 instead of the exact one (their P reaches 2^(2 + |m~|/64)); that
    needs no emulation of its own: softmax is invariant under the shift, and the bf16 rounding of P is relative, so P 2^d rounds
    with the same relative error as P (one difference stays inside the test's factor: the dominant P of a near one-hot row is 1 here
    and exact, 2^(s - m~) there and rounded - up to 2^-9 of such a row)."""
    qh, (k, v) = q_heads(q), split_kv(kv[:, :vis.shape[1]])
    s = (qh @ k.transpose(-1, -2) * s_mul).masked_fill(~vis, -math.inf)
    m = f32(s.max(-1, keepdim=True).values)
    p = torch.exp((s - m).to(torch.float32)).to(F64)                # fp32 P, masked keys exactly 0
    p_b = bf16(p)
    rowsum = f32(p.sum(-1, keepdim=True))
    out = bf16(heads_to_rows(p_b @ v / rowsum))
    # the MFMA kernels keep the maximum in the exp2 domain: m2 = max(s) * (scale * log2 e), lse = (m2 + log2(row sum)) * ln 2, each step fp32
    raw_max = (qh @ k.transpose(-1, -2)).masked_fill(~vis, -math.inf).max(-1, keepdim=True).values.to(torch.float32)
    c2 = torch.tensor(s_mul, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    lse_a = ((raw_max * c2 + torch.log2(rowsum.to(torch.float32))) * torch.tensor(0.6931471805599453, dtype=torch.float32)).to(F64)[..., 0]
    lse_b = f32(m + torch.log(p_b.sum(-1, keepdim=True)))[..., 0]
    return out, lse_a, lse_b


def attention_fwd_emulated(qkv: torch.Tensor, scale: float, vis: torch.Tensor):
    """attention_cached_emulated on the packed training layout (q_off = 0, queries = the arena's own q third)"""
    C = qkv.shape[-1] // 3
    return attention_cached_emulated(qkv[..., :C], qkv[..., C:], scale, vis)


def attention_bwd_emulated(qkv, dout, out, lse, scale: float, vis) -> torch.Tensor:
    """backward with the storage points of the MFMA kernels (csrc/attn.hip attn_bwd_*_mfma_kernel): O arrives in bf16 and
    D = rowsum(dO . O) is formed from it, lse is an fp32 value, P = exp(S scale - lse) is an fp32 value, P and dS = P (dP - D) are
    rounded to bf16 before the second products, dQ / dK / dV are rounded to bf16.  Sums and products: float64.
    out / lse: the exact float64 forward results (this function does the rounding)."""
    R = qkv.shape[0]
    q, k, v = split_heads(qkv)
    do, o = rows_to_heads(dout, R), bf16(rows_to_heads(out, R))
    d = (do * o).sum(-1, keepdim=True)
    p = torch.exp((q @ k.transpose(-1, -2) * scale - f32(lse)[..., None]).to(torch.float32)).to(F64) * vis.to(F64)
    ds_b = bf16(p * (do @ v.transpose(-1, -2) - d))
    p_b = bf16(p)
    return bf16(merge_heads(ds_b @ k * scale, ds_b.transpose(-1, -2) @ q * scale, p_b.transpose(-1, -2) @ do))


def row_error(got: torch.Tensor, ref: torch.Tensor, dout: torch.Tensor) -> float:
    """max over token rows of one head (64 channels) of |got - ref|_2 / (|ref|_2 + tau), tau = 5e-2 * RMS of the reference's row
    norms + 1e-4 * RMS row norm of dO (the absolute floor keeps a reference that is exactly zero - l = 1: dQ = dK = 0 - defined).
    got / ref: any shape whose last dimension is a multiple of 64 (pass one third of dqkv at a time)."""
    g, r = got.to(F64).reshape(-1, 64), ref.to(F64).reshape(-1, 64)
    rn = r.norm(dim=-1)
    tau = 5e-2 * rn.pow(2).mean().sqrt() + 1e-4 * dout.to(F64).reshape(-1, 64).norm(dim=-1).pow(2).mean().sqrt()
    return float(((g - r).norm(dim=-1) / (rn + tau)).max())


def row_error_fwd(got: torch.Tensor, ref: torch.Tensor, R: int):
    """row_error for a forward output [R*l][H*64] whose samples live in different regimes: max over the (token, head) rows of 64
    channels of |got - ref|_2 / (|ref|_2 + tau_r), tau_r = 5e-2 * RMS row norm of the reference over sample r ALONE (a floor taken
    over all samples would let the large ones hide the near-uniform one).  Returns (maximum, [value of sample r])."""
    g, r = got.to(F64).reshape(R, -1, 64), ref.to(F64).reshape(R, -1, 64)
    rn = r.norm(dim=-1)
    tau = 5e-2 * rn.pow(2).mean(-1, keepdim=True).sqrt()
    per = ((g - r).norm(dim=-1) / (rn + tau)).amax(-1)
    per = torch.where(torch.isnan(per), torch.full_like(per, math.inf), per)        # a NaN row is an infinite error, never a passing one
    return float(per.max()), [float(x) for x in per]


def thirds(dqkv: torch.Tensor):
    """[R][l][3*H*64] -> {'dQ', 'dK', 'dV'} views [R][l][H*64]"""
    C = dqkv.shape[-1] // 3
    return {'dQ': dqkv[..., :C], 'dK': dqkv[..., C:2 * C], 'dV': dqkv[..., 2 * C:]}


# ------------------------------------------------------------------------------------------------ cos-attention pre-pass
class CosNorm(NamedTuple):
    qn: torch.Tensor         # [N][H][64]  normalize(q) * exp(min(s, ln 100))
    kn: torch.Tensor         # [N][H][64]  normalize(k)
    norms: torch.Tensor      # [N][H][2]   |q|, |k|
    dq: torch.Tensor         # [N][H][64]
    dk: torch.Tensor
    dsm_tok: torch.Tensor    # [N][H]      d loss / d scale_mul[h] contributed by each token


def cos_qk_norm_fwd_bwd(q, k, scale_mul, gq, gk, dtype=F64) -> CosNorm:
    """autograd through  F.normalize(q) * exp(clamp_max(s, ln 100))  and  F.normalize(k)  (basic_var.py:99-104) in ``dtype``.
    q, k, gq, gk: [N][H][64] raw rows and the gradients w.r.t. the two outputs; scale_mul [H].  The temperature is expanded
    per token before the graph is built, so its gradient comes back per (token, head)."""
    q, k = q.detach().to(dtype).clone().requires_grad_(True), k.detach().to(dtype).clone().requires_grad_(True)
    N, H, _ = q.shape
    s = scale_mul.detach().to(torch.float32).to(dtype).view(1, H).expand(N, H).clone().requires_grad_(True)
    qn = F.normalize(q, dim=-1) * s.clamp_max(torch.tensor(LN100, dtype=torch.float32).to(dtype)).exp()[..., None]
    kn = F.normalize(k, dim=-1)
    torch.autograd.backward([qn, kn], [gq.to(dtype), gk.to(dtype)])
    norms = torch.stack([q.detach().norm(dim=-1), k.detach().norm(dim=-1)], -1)
    return CosNorm(qn.detach(), kn.detach(), norms, q.grad, k.grad, s.grad)


def cos_qk_norm_fwd_bwd_f64(q, k, scale_mul, gq, gk) -> CosNorm:
    return cos_qk_norm_fwd_bwd(q, k, scale_mul, gq, gk, F64)


def cos_qk_norm_bwd_emulated(q, k, scale_mul, gq, gk):
    """the backward kernel's view of the same function in bf16 mode: it reads back the bf16-ROUNDED normalised rows the forward
    left in the arena (q_hat * sm, k_hat), the fp32 norms and bf16 gradients, and writes bf16; the arithmetic in between is float64:
      x_t = x_hat / sm (q) or x_hat (k);  g' = g sm (q) or g (k);  dx = (g' - x_t (x_t . g')) / |x|;  dsm = (g . x_t) sm  below or at the clamp.
    Returns (dq, dk, dsm_tok)."""
    q, k, gq, gk = q.to(F64), k.to(F64), gq.to(F64), gk.to(F64)
    s32 = scale_mul.to(torch.float32)
    sm = s32.to(F64).clamp_max(float(torch.tensor(LN100, dtype=torch.float32))).exp().view(1, -1, 1)
    nq, nk = f32(q.norm(dim=-1, keepdim=True)), f32(k.norm(dim=-1, keepdim=True))
    qh, kh = bf16(q / nq * sm), bf16(k / nk)
    xt, gp = qh / sm, gq * sm
    dq = bf16((gp - xt * (xt * gp).sum(-1, keepdim=True)) / nq)
    dk = bf16((gk - kh * (kh * gk).sum(-1, keepdim=True)) / nk)
    passes = (s32 <= torch.tensor(LN100, dtype=torch.float32)).to(F64).view(1, -1)
    dsm = f32((gq * xt).sum(-1) * sm[..., 0] * passes)
    return dq, dk, dsm


def temperature_error(got: torch.Tensor, ref: torch.Tensor, gq: torch.Tensor, scale_mul: torch.Tensor) -> float:
    """max over (token, head) of |got - ref| / (|g|_2 sm): the per-token temperature gradient is g . x_t sm with |x_t| = 1"""
    sm = scale_mul.to(torch.float32).to(F64).clamp_max(LN100).exp().view(1, -1)
    return float(((got.to(F64) - ref.to(F64)).abs() / (gq.to(F64).norm(dim=-1) * sm)).max())


# ------------------------------------------------------------------------------------------------ the shared case table
def _case9():
    ends = [7, 14, 45, 76, 140, 204, 333, 462]
    begins = [0] + ends[:-1]
    return ends, [(begins[i - 1], ends[i - 1]) if i % 2 else (0, 0) for i in range(len(ends))]


# number -> (R, H, l, Lmax, lvl_end, holes); tests/test_attn_oracle_host.py holds the yardstick condition on every one of them.
# 11 came out of tools/fuzz_attn_bwd.py: rows whose first key tiles are hidden completely (the forward's running maximum had no finite start)
CASES = {
    1: (2, 2, 1, 1, None, None),                                            # one query, one key
    2: (2, 1, 33, 33, None, None),                                          # one lane into the second wave; n_lvl == 0
    3: (1, 2, 129, 160, None, None),                                        # one query / key in the second workgroup; l < Lmax
    4: (1, 2, 200, 200, [200], None),                                       # n_lvl == 1
    5: (2, 2, 182, 182, [2, 10, 28, 60, 110, 182], None),                   # the training pyramid of patch sizes 1..6
    6: (2, 3, 257, 257, [31, 32, 33, 97, 128, 129, 191, 257], None),        # ends at +-1 around 32 / 64 / 128, one-token levels
    7: (1, 1, 96, 96, list(range(3, 97, 3)), None),                         # 32 levels
    8: (1, 2, 384, 384, [64, 128, 256, 384], None),                         # boundaries on tile edges
    9: (1, 2, 462, 462) + _case9(),                                         # holes: mid-tile start, exactly 64 keys, two tiles
    10: (1, 2, 300, 300, [7, 100, 300], [(0, 0), (0, 0), (0, 7)]),          # a hole far in front of its level
    11: (1, 2, 200, 200, [130, 200], [(0, 0), (0, 130)]),                   # a hole that hides two whole key tiles from key 0 on
}
AMP, SCALE = 1.0, 0.125


def case_inputs(n: int, amp: float = AMP):
    """(qkv [R][l][3*H*64], dout [R*l][H*64]) of case n: randn * amp and randn from a generator seeded by the case number,
    rounded to bf16, returned as float32"""
    R, H, l = CASES[n][:3]
    g = torch.Generator().manual_seed(n)
    qkv = (torch.randn(R, l, 3 * H * 64, generator=g) * amp).to(torch.bfloat16).float()
    dout = torch.randn(R * l, H * 64, generator=g).to(torch.bfloat16).float()
    return qkv, dout


# ------------------------------------------------------------------------------------------------ the cached (inference) forward
# number -> (R, H, Lmax, q_off, l, lvl_end, holes): the smallest shapes at which each piece of the inference kernels' logic is still
# exercised; tests/test_attn_fwd_oracle_host.py holds the yardstick and the sensitivity condition on every one of them.
FWD_CASES = {
    1: (4, 1, 2, 0, 2, None, None),                                         # first scale: two queries, two keys
    2: (4, 2, 28, 10, 18, None, None),                                      # one partial tile, one partial wave
    3: (4, 2, 110, 60, 50, None, None),                                     # ragged second tile, waves 2-3 idle
    4: (4, 3, 400, 110, 72, None, None),                                    # 12 pairs (plain block-id mapping); Lmax far behind q_off + l
    5: (4, 1, 128, 64, 64, None, None),                                     # key count on a tile edge
    6: (4, 2, 310, 182, 128, None, None),                                   # exactly one query block
    7: (4, 2, 510, 310, 200, None, None),                                   # two query blocks, 8 pairs (XCD-grouped mapping)
    8: (4, 2, 1360, 848, 512, None, None),                                  # last scale of the 256^2 pyramid: 4 query blocks, 22 tiles
    9: (4, 2, 300, 0, 300, [2, 10, 28, 60, 110, 182, 300], None),           # teacher-forced forward through the inference kernel
    10: (4, 2, 120, 40, 80, [20, 40, 80, 120], [(0, 0), (0, 0), (20, 40), (40, 80)]),   # indep + separate_decoding, cached form
    11: (1, 1, 4480, 2432, 2048, None, None),                               # S = 32 last scale: 16 query blocks, 70 tiles; regime 1
    12: (8, 64, 256, 56, 200, None, None),                                  # 512 workgroups of 256 queries: the 64-query kernel
    13: (4, 2, 510, 310, 200, None, None),                                  # cos-attention regime: unit-norm q, k at the temperature clamp
}
FWD_SCALE, FWD_SCALE_SHARP = 0.125, 1.0
FWD_SHARP_CASES = (2, 3, 7, 9, 10)          # also run at scale 1.0: near one-hot rows, sample 3's first-tile shift is below -128
COS_CASE, COS_Q_NORMS = 13, (100.0, 30.0, 5.0, 100.0)
# every (case, scale) the tests run: 1-12 at 0.125, the sharp cases again at 1.0, the cos-attention case at its own scale 1
FWD_RUNS = [(n, FWD_SCALE) for n in range(1, 13)] + [(n, FWD_SCALE_SHARP) for n in FWD_SHARP_CASES] + [(COS_CASE, 1.0)]
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453


def fwd_case_inputs(n: int, scale: float):
    """(kv [R][Lmax][2*H*64], q [R][l][H*64], q' = bf16(bf16(q) * scale * log2 e)) of case n from a generator seeded by the case
    number, rounded to bf16, returned as float32.  The regime of sample r is r % 4 (R >= 4; a single sample is regime 1):
      0  plain randn;
      1  the K row of key (q_off + l - 1) // 2 times 12: the running maximum jumps late;
      2  q * 0.05: near-uniform attention;
      3  q = 3 |q|, k = -|k|: every score far below zero, the first tile moves the shift DOWN.
    COS_CASE: unit-norm keys, unit-norm queries times COS_Q_NORMS[r] (cos-attention at its temperature clamp; scale 1)."""
    R, H, Lmax, q_off, l, _, _ = FWD_CASES[n]
    C = H * 64
    g = torch.Generator().manual_seed(n)
    kv = torch.randn(R, Lmax, 2 * C, generator=g)
    q = torch.randn(R, l, C, generator=g)
    if n == COS_CASE:
        kv[..., :C] = F.normalize(kv[..., :C].reshape(R, Lmax, H, 64), dim=-1).reshape(R, Lmax, C)
        q = F.normalize(q.view(R, l, H, 64), dim=-1).reshape(R, l, C) * torch.tensor(COS_Q_NORMS).view(R, 1, 1)
    else:
        for r in range(R):
            regime = r % 4 if R >= 4 else 1
            if regime == 1:
                kv[r, (q_off + l - 1) // 2, :C] *= 12.0
            elif regime == 2:
                q[r] *= 0.05
            elif regime == 3:
                q[r] = q[r].abs() * 3.0
                kv[r, :, :C] = -kv[r, :, :C].abs()
    kv, q = kv.to(torch.bfloat16).float(), q.to(torch.bfloat16).float()
    return kv, q, (q * (scale * LOG2E)).to(torch.bfloat16).float()
