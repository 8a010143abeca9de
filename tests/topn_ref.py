"""Shared by tests/test_topn_host.py (CPU), tests/test_gpu_score_topn.py and tests/test_gpu_kd_topn_kernel.py: the contracts of cvar_score_topn and
cvar_kd_topn_fwd_bwd (include/cvar_topn.h) restated in float64 numpy on the fp32 inputs as stored, numpy-float32 models of the kernels'
order of operations, the bounds, and the inputs of the kernel sweeps.

Bounds (u = 2^-24, one rounding per operation, -ffp-contract=off; the house margin 4 is applied once, at the end; nothing here is measured on a kernel).

cvar_score_topn.  The ids are exact (an order of fp32 values) and top_logprob is cvar_score_rows' value bit for bit, so only tail_logprob has a bound.
x_e is the fp32 combined logit (the combine is exact to restate: separately rounded products, added in order), m its maximum, d_e = x_e - m:
    ex_e = expf(x_e - m)               relative eps_e = (|d_e| + 2) u    (the difference's rounding moves the exponent by u |d_e|; accurate expf, 1 ulp <= 2 u)
    S = sum_e ex_e                     relative R_S = sum_e ex_e eps_e / S + D u + V TINY / S,   D = ceil(V / 256) + 9  (lane, 6-level tree, 3 wave adds)
    S_tail over the unlisted e         relative R_T likewise over its own terms
    tail = logf(S_tail) - logf(S)      R_T + R_S + 2 u (|log S_tail| + |log S|) + u |tail|      (d log, logf 1 ulp each, the difference) - ABSOLUTE
    S_tail == 0 (every code listed, or the rest at -inf): -inf exactly.  The TINY term is an element's absolute error where expf leaves the normal range: a
    tail whose whole mass is below MARGIN V TINY may come out as 0, and tail_logprob as -inf.

cvar_kd_topn_fwd_bwd.  R_x is T.ce's relative error of se; eps_v = (2 |d_v| + 4) u is its bound of __expf(d_v), d_v = x_v - mx (distill_ref's terms).
    lse_x = logf(se) + mx              e_lx = R_x + 2 u |log se| + u |lse_x|
    b_j = x_id_j - lse_x               e_lx + u |b_j|
    t_j = t_lp_j - b_j                 E_t = e_lx + u (|b_j| + |t_j|)
    q_j = __expf(t_lp_j)               relative rq_j = (2 |t_lp_j| + 4) u
    term_j = q_j t_j                   q_j (rq_j |t_j| + E_t) + u |q_j t_j| + TINY
    listed = sum_j term_j              one wave's tree, depth 6: sum_j of the terms' bounds + 6 u sum_j |term_j|
    p_v = __expf(d_v) (1 / se)         relative rp_v = eps_v + R_x + 2 u
    p_tail = sum_unlisted p_v          absolute E_pt = sum_unlisted p_v rp_v + D u p_tail, D = ceil(V / 256) + 8;  relative R_pt = E_pt / p_tail
    r = __expf(t_tail)                 relative rr = (2 |t_tail| + 4) u
    s = t_tail - logf(p_tail)          E_s = R_pt + 2 u |log p_tail| + u |s|
    tail term = r s                    r (rr |s| + E_s) + u |r s|
    loss = listed + tail term          the sum of the two bounds + u |loss|     - ABSOLUTE: the loss cancels to zero where the student has learnt the teacher
    g = w gscale                       u |g|
    dlogits_v, listed: (p_v - q_j) g   |g| (p_v rp_v + q_j rq_j + u |p_v - q_j|) + 2 u |dl_v| + 4 TINY (1 + |g|)
    f = 1 - r / p_tail                 E_f = (r / p_tail) (rr + R_pt + u) + u |f|;   exactly 1 (E_f = 0) when r == 0
    dlogits_v, unlisted: (p_v f) g     |g| (p_v (rp_v |f| + E_f) + u |p_v f|) + 2 u |dl_v| + 4 TINY (1 + |g|)
                                       (+ 2^-8 |ref| in bf16)"""
from types import SimpleNamespace as NS

import numpy as np
import torch

import distill_ref as D
from oracle import train_kernels_ref as T
from oracle.norm_ref import _wave_sum

F32, F64 = np.float32, np.float64
U, TINY, MARGIN = T.U, T.TINY, T.MARGIN
GSCALE = D.GSCALE
NMAX = 64


# ================================================================================================ cvar_score_topn
def combine32(logits, coef, B, nrep):
    """combine_logits in numpy float32: ((c0 l0 + c1 l1) + c2 l2) + c3 l3 with separately rounded products -> (B, l, V) float32, the kernel's bits"""
    x = T.as_np(logits, F32)
    x = x.reshape(nrep, B, *x.shape[1:])
    c = T.as_np(coef, F32)
    with np.errstate(invalid='ignore', over='ignore'):
        v = (c[:, 0, None, None] * x[0]).astype(F32)
        for r in range(1, nrep):
            v = (v + (c[:, r, None, None] * x[r]).astype(F32)).astype(F32)
    return v


def rank_order(comb):
    """cvar_score_rows' rank order per row: value descending (floats compared as floats), id ascending -> (..., V) ids"""
    x = np.asarray(comb, F64)
    ids = np.broadcast_to(np.arange(x.shape[-1]), x.shape)
    return np.lexsort((ids, -x), axis=-1)


def _score_depth(V):
    return -(-V // 256) + 9


def score_reference(comb, N):
    """the contract in float64 on the fp32 combined logits (B, l, V) -> ids (B, l, N) (-1 past V), logprob (B, l, N) (-inf past V), tail (B, l) and
    tail_bound"""
    x = np.asarray(comb, F64)
    V = x.shape[-1]
    order = rank_order(x)
    n = min(N, V)
    ids = np.full(x.shape[:-1] + (N,), -1, np.int64)
    ids[..., :n] = order[..., :n]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        m = x.max(-1, keepdims=True)
        d = x - m
        ex = np.exp(d)
        S = ex.sum(-1)
        lp = np.full(x.shape[:-1] + (N,), -np.inf)
        lp[..., :n] = np.take_along_axis(d, order[..., :n], -1) - np.log(S)[..., None]
        listed = np.zeros(x.shape, bool)
        np.put_along_axis(listed, order[..., :n], True, -1)
        ext = np.where(listed, 0.0, ex)
        St = ext.sum(-1)
        tail = np.log(St) - np.log(S)
        eps = np.where(np.isfinite(d), (np.abs(d) + 2) * U, 0.0)
        Dp = _score_depth(V)
        R_S = (ex * eps).sum(-1) / S + Dp * U + V * TINY / S
        R_T = (ext * eps).sum(-1) / np.maximum(St, 1e-300) + Dp * U + V * TINY / np.maximum(St, 1e-300)
        fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
        bound = MARGIN * (R_T + R_S + 2 * U * (fin(np.log(St)) + fin(np.log(S))) + U * fin(tail))
        bound = np.where(St > 0, bound, 0.0)
    return NS(ids=ids, logprob=lp, tail=tail, tail_bound=bound, S=S, S_tail=St, tail_may_vanish=St <= MARGIN * V * TINY)


def _seq_lanes_sum(v):
    """(R, 256 K) per-element values -> score_token's block sum: lane e % 256 accumulates in order, shuffle tree per wave, ((w0 + w1) + w2) + w3"""
    a = np.zeros((v.shape[0], 256), F32)
    for k in range(v.shape[1] // 256):
        a = a + v[:, k * 256:(k + 1) * 256]
    w4 = [_wave_sum(a[:, 64 * k:64 * k + 64]) for k in range(4)]
    return (((w4[0] + w4[1]) + w4[2]) + w4[3]).astype(F32)


def score_model(comb, N):
    """the kernel's sums in numpy float32 (np.exp / np.log in float32 stand for expf / logf) -> logprob (R, N), tail (R,) on rows (R, V)"""
    x = np.asarray(comb, F32)
    x = x.reshape(-1, x.shape[-1])
    R, V = x.shape
    K = -(-V // 256)
    order = rank_order(x)
    n = min(N, V)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        m = x.max(1, keepdims=True)
        ex = np.zeros((R, K * 256), F32)
        ex[:, :V] = np.exp((x - m).astype(F32)).astype(F32)
        S = _seq_lanes_sum(ex)
        np.put_along_axis(ex, order[:, :n], F32(0), 1)
        St = _seq_lanes_sum(ex)
        logS = np.log(S).astype(F32)
        lp = np.full((R, N), -np.inf, F32)
        lp[:, :n] = ((np.take_along_axis(x, order[:, :n], 1) - m).astype(F32) - logS[:, None]).astype(F32)
        tail = np.where(St > 0, (np.log(St).astype(F32) - logS).astype(F32), F32(-np.inf))
    return NS(logprob=lp, tail=tail.astype(F32))


# ================================================================================================ cvar_kd_topn_fwd_bwd
KD_MS, KD_VS, KD_NS = (1, 5, 37), (4096, 1000, 257, 65), (1, 8, 64)


def sparse_from_dense(z, N, tail=True, drop=0, shuffle_seed=None):
    """a dense teacher (M, V) of logits -> the sparse teacher cvar_score_topn would give for it, in float64 then stored as fp32: ids (M, N) int32 (-1 past
    V), lp (M, N) fp32, tail (M,) fp32 (the log of the unlisted mass; None with tail=False).  drop: that many of the listed slots are marked unused (-1:
    their mass is simply not taught).  shuffle_seed: the slots are permuted - the contract does not ask for an order."""
    z = T.as_np(z, F64)
    M, V = z.shape
    ref = score_reference(z.astype(F32), N)
    ids, lp = ref.ids.copy(), ref.logprob.copy()
    g = np.random.default_rng(0 if shuffle_seed is None else shuffle_seed)
    for m in range(M):
        live = np.flatnonzero(ids[m] >= 0)
        if drop and live.size > drop:
            ids[m, g.choice(live, drop, replace=False)] = -1
        if shuffle_seed is not None:
            perm = g.permutation(N)
            ids[m], lp[m] = ids[m, perm], lp[m, perm]
    lp = np.where(ids >= 0, lp, 0.0)
    t = torch.from_numpy(ref.tail.astype(F32)) if tail else None
    return NS(ids=torch.from_numpy(ids.astype(np.int32)), lp=torch.from_numpy(lp.astype(F32)), tail=t)


def kd_inputs(M, V, N, seed=0, tail=True, drop=0):
    """-> NS of torch tensors: D.inputs' student logits, teacher and weight (logits to +-30, the nearly-learnt row 1, the edge row 2), and the sparse
    teacher of that dense one (slots shuffled)"""
    x = D.inputs(M, V, seed=seed + 17 * N)
    x.logits = x.logits.clamp(-D.RANGE, D.RANGE)
    sp = sparse_from_dense(x.teacher, N, tail=tail, drop=drop, shuffle_seed=1000 * M + V + N + seed)
    return NS(logits=x.logits, dense=x.teacher, weight=x.weight, ids=sp.ids, lp=sp.lp, tail=sp.tail)


def _listed(ids, V):
    """(M, N) ids -> slot (M, V): the slot that lists v, -1 for none"""
    M, N = ids.shape
    slot = np.full((M, V), -1, np.int64)
    for j in range(N):
        rows = np.flatnonzero((ids[:, j] >= 0) & (ids[:, j] < V))
        slot[rows, ids[rows, j]] = j
    return slot


def kd_reference(logits, ids, lp, tail=None, weight=None, gscale=1.0, bf16=False):
    """the contract in float64 on the stored fp32 inputs (gscale as the C ABI receives it) and the bounds of the module's header"""
    x = T.as_np(logits, F64)
    M, V = x.shape
    ids = T.as_np(ids, np.int64)
    N = ids.shape[1]
    tlp = T.as_np(lp, F64)
    tt = np.full(M, -np.inf) if tail is None else T.as_np(tail, F64)
    w = np.ones(M) if weight is None else T.as_np(weight, F64)
    g = w * T.f32(gscale)
    sx = D._softmax_parts(x)
    p = sx.p
    slot = _listed(ids, V)
    used = (ids >= 0) & (ids < V)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        q = np.where(used, np.exp(tlp), 0.0)
        has_tail = np.isfinite(tt)
        r = np.where(has_tail, np.exp(np.where(has_tail, tt, 0.0)), 0.0)
        safe = np.where(used, ids, 0)
        b = np.take_along_axis(x, safe, 1) - sx.lse[:, None]
        t = np.where(used, tlp - b, 0.0)
        term = q * t
        unl = slot < 0
        pt = np.where(unl, p, 0.0).sum(1)
        logpt = np.where(r > 0, np.log(np.where(r > 0, pt, 1.0)), 0.0)
        s = np.where(r > 0, np.where(has_tail, tt, 0.0) - logpt, 0.0)
        tail_term = r * s
        loss = term.sum(1) + tail_term
        f = np.where(r > 0, 1.0 - r / np.where(r > 0, pt, 1.0), 1.0)
        qv = np.where(unl, 0.0, np.take_along_axis(q, np.maximum(slot, 0), 1))
        dl = np.where(unl, p * f[:, None], p - qv) * g[:, None]
        # ---- bounds
        e_lx = sx.R + 2 * U * np.abs(sx.logse) + U * np.abs(sx.lse)
        E_t = e_lx[:, None] + U * (np.abs(b) + np.abs(t))
        rq = (2 * np.abs(tlp) + 4) * U
        term_b = np.where(used, q * (rq * np.abs(t) + E_t) + U * np.abs(term) + TINY, 0.0)
        listed_b = term_b.sum(1) + 6 * U * np.abs(term).sum(1)
        rp = sx.eps + sx.R[:, None] + 2 * U
        Dp = -(-V // 256) + 8
        E_pt = np.where(unl, p * rp, 0.0).sum(1) + Dp * U * pt
        R_pt = np.where(r > 0, E_pt / np.where(r > 0, pt, 1.0), 0.0)
        rr = np.where(has_tail, (2 * np.abs(np.where(has_tail, tt, 0.0)) + 4) * U, 0.0)
        E_s = R_pt + 2 * U * np.abs(logpt) + U * np.abs(s)
        tail_b = np.where(r > 0, r * (rr * np.abs(s) + E_s) + U * np.abs(tail_term), 0.0)
        loss_bound = MARGIN * (listed_b + tail_b + np.where(r > 0, U * np.abs(loss), 0.0))
        ag = np.abs(g)[:, None]
        rqv = np.where(unl, 0.0, np.take_along_axis(rq, np.maximum(slot, 0), 1))
        E_f = np.where(r > 0, (r / np.where(r > 0, pt, 1.0)) * (rr + R_pt + U) + U * np.abs(f), 0.0)
        inner = np.where(unl, p * (rp * np.abs(f)[:, None] + E_f[:, None]) + U * np.abs(p * f[:, None]), p * rp + qv * rqv + U * np.abs(p - qv))
        dl_bound = MARGIN * (ag * inner + 2 * U * np.abs(dl)) + 4 * TINY * (1 + ag)
        if bf16:
            dl_bound = dl_bound + T.BF16_HALF_ULP * np.abs(dl)
    return NS(loss=loss, dlogits=dl, p=p, q=q, r=r, p_tail=pt, f=f, slot=slot, loss_bound=loss_bound, dl_bound=dl_bound)


KD_FAULTS = ('renormalised_q', 'tail_dropped', 'f_on_listed')


def kd_model(logits, ids, lp, tail=None, weight=None, gscale=1.0, fault=None):
    """kd_topn_kernel in numpy float32, operation by operation (np.exp / np.log in float32 stand for __expf / logf).  fault: a planted mistake the bounds
    must see - 'renormalised_q' (the listed q_j divided by their sum, as if the teacher had no tail), 'tail_dropped' (no tail term in the loss and f = 1),
    'f_on_listed' (the listed columns' p_v scaled by f too)"""
    x = T.as_np(logits, F32)
    M, V = x.shape
    ids = T.as_np(ids, np.int64)
    tlp = T.as_np(lp, F32)
    tt = np.full(M, -np.inf, F32) if tail is None else T.as_np(tail, F32)
    slot = _listed(ids, V)
    used = (ids >= 0) & (ids < V)
    unl = slot < 0
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        mx, ex, se = D._row_pass(x)
        lse_x = np.log(se).astype(F32) + mx[:, 0]
        inv = F32(1) / se
        p = (ex[:, :V] * inv[:, None]).astype(F32)
        q = np.where(used, np.exp(tlp).astype(F32), F32(0)).astype(F32)
        if fault == 'renormalised_q':
            q = (q / q.sum(1, keepdims=True)).astype(F32)
        has_tail = np.isfinite(tt)
        r = np.where(has_tail, np.exp(np.where(has_tail, tt, F32(0))).astype(F32), F32(0)).astype(F32)
        safe = np.where(used, ids, 0)
        b = (np.take_along_axis(x, safe, 1) - lse_x[:, None]).astype(F32)
        term = np.zeros((M, 64), F32)
        term[:, :ids.shape[1]] = np.where(used, q * (tlp - b).astype(F32), F32(0))
        listed = _wave_sum(term)
        pu = np.zeros_like(ex)
        pu[:, :V] = np.where(unl, p, F32(0))
        pt = D._lanes_sum(pu)
        live = r > 0
        pts = np.where(live, pt, F32(1))
        tts = np.where(has_tail, tt, F32(0))
        f = np.where(live, F32(1) - (r / pts).astype(F32), F32(1)).astype(F32)
        tail_term = (r * (tts - np.log(pts).astype(F32)).astype(F32)).astype(F32)
        if fault == 'tail_dropped':
            f = np.ones(M, F32)
            live = np.zeros(M, bool)
        loss = np.where(live, listed + tail_term, listed).astype(F32)
        g = ((np.ones(M, F32) if weight is None else T.as_np(weight, F32)) * F32(gscale)).astype(F32)
        qv = np.where(unl, F32(0), np.take_along_axis(q, np.maximum(slot, 0), 1)).astype(F32)
        pl = (p * f[:, None]).astype(F32) if fault == 'f_on_listed' else p
        dl = np.where(unl, (p * f[:, None]).astype(F32), (pl - qv).astype(F32)) * g[:, None]
    return NS(loss=loss.astype(F32), dlogits=dl.astype(F32))


def kd_fractions(got_loss, got_dl, ref):
    """-> (largest |loss error| / bound, largest |dlogits error| / bound or None)"""
    fl = T.ratio_of(T.abs_err(got_loss, ref.loss), ref.loss_bound)
    return fl, (T.ratio_of(T.abs_err(got_dl, ref.dlogits), ref.dl_bound) if got_dl is not None else None)


def dense_kl(z, x):
    """KL(softmax z || softmax x) per row in float64: the loss the dense teacher gives"""
    z, x = T.as_np(z, F64), T.as_np(x, F64)
    lq = z - (np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)) + z.max(1, keepdims=True))
    lpx = x - (np.log(np.exp(x - x.max(1, keepdims=True)).sum(1, keepdims=True)) + x.max(1, keepdims=True))
    return (np.exp(lq) * (lq - lpx)).sum(1)
