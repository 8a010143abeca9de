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

Layouts are the kernels': qkv [R][l][3*H*64] (q | k | v thirds, head-major inside a third), out / dout [R*l][H*64], lse [R][H][l].
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


def attention_fwd_emulated(qkv: torch.Tensor, scale: float, vis: torch.Tensor):
    """forward with the bf16 kernels' storage points: the unnormalised P = exp(s - max) is computed in fp32 and rounded to bf16
    before P V, the row sum is taken from the fp32 P, out is rounded to bf16.  lse is returned twice - from the fp32 row sum
    (what the kernels store, formed in the exp2 domain as they form it) and from the row sum of the bf16-rounded P (what normalises a product of bf16 operands) - as
    (out [R*l][H*64], lse_fp32sum [R][H][l], lse_bf16sum [R][H][l])."""
    q, k, v = split_heads(qkv)
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, -math.inf)
    m = f32(s.max(-1, keepdim=True).values)
    p = torch.exp((s - m).to(torch.float32)).to(F64)                # fp32 P, masked keys exactly 0
    p_b = bf16(p)
    rowsum = f32(p.sum(-1, keepdim=True))
    out = bf16(heads_to_rows(p_b @ v / rowsum))
    # the MFMA kernels keep the maximum in the exp2 domain: m2 = max(s) * (scale * log2 e), lse = (m2 + log2(row sum)) * ln 2, each step fp32
    raw_max = (q @ k.transpose(-1, -2)).masked_fill(~vis, -math.inf).max(-1, keepdim=True).values.to(torch.float32)
    c2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    lse_a = ((raw_max * c2 + torch.log2(rowsum.to(torch.float32))) * torch.tensor(0.6931471805599453, dtype=torch.float32)).to(F64)[..., 0]
    lse_b = f32(m + torch.log(p_b.sum(-1, keepdim=True)))[..., 0]
    return out, lse_a, lse_b


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
