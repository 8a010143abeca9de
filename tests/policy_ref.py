"""Shared by tests/test_policy_host.py (CPU) and tests/test_gpu_policy_kernel.py: the contract of cvar_pg_fwd_bwd (include/cvar_policy.h)
restated in float64 numpy on the fp32 inputs as stored, a numpy-float32 model of the kernel's order of operations, the per-row bounds, and the inputs of
the kernel sweep.  The softmax part is oracle/train_kernels_ref.py's cross-entropy (T.ce, T.ce_model and its bound R): the kernel's first two passes are
ce_kernel's.

Bounds (u = 2^-24, one rounding per operation, -ffp-contract=off; the house margin 4 is applied once, at the end; nothing here is measured on a kernel).
    lp = -((logf(se) + mx) - x_t)      e_lp = T.ce's loss bound / 4 = R + u (4 |log se| + 2 |mx| + |x_t|)              (the negation is exact)
    r  = expf(lp - old)                the difference: e_a = e_lp + u |lp - old|; accurate expf: 1 ulp = 2 u   ->  E_r = r (e_a + 2 u) + TINY
    s1 = r a                           E_s1 = |a| (E_r + u r)
    s2 = clamp(r, 1 - lo, 1 + hi) a    the edges are rounded once (u (1 + clip)); clamp is 1-Lipschitz: E_s2 = |a| (max(E_r, 2 u) + u clamp)
    obj = min(s1, s2)                  E_obj = max(E_s1, E_s2);      without old_lp obj = a lp: E_obj = |a| e_lp + u |a lp|
    d = ref - lp, e = expf(d)          e_d = e_lp + u |d|;  E_e = e (e_d + 2 u) + TINY
    k = (e - d) - 1                    E_k = E_e + e_d + u |e - d| + u |k|            (absolute: k cancels to ~0 near d = 0)
    loss = -obj + kc k                 E_obj + kc (E_k + u |k|) + u |loss|
    c = (active ? s1 : 0) - kc (1 - e) [active] E_s1 + kc (E_e + 2 u |1 - e|) + u |c|
    coef = c w                         |w| (E_c + u |c|)
    g = coef gscale                    E_g = |gscale| (E_coef + u |coef|)
    dlogits_v = (p_v - [v = t]) g      |g| (p_v (eps_v + R + 2 u) + u |p_v - hot|) + |p_v - hot| E_g + u |dl|    (+ 2^-8 |ref| in bf16)
The clip decision.  In exact arithmetic and in the kernel alike, a > 0 is active iff r <= 1 + hi, a < 0 iff r >= 1 - lo, a = 0 always: inside the window
clamp(r) IS r, so s1 and s2 are the same product - a tie, active - whatever the rounding; fp32 multiplication is monotonic, so a row is decided wrongly only
if the computed r lies on the other side of the edge that matters than the exact one.  The rows whose decision the bound leaves open are therefore those
with a != 0 and |r - edge| <= 4 E_r (E_r with its margin) - for rows outside the window this is the issue's |s1 - s2| <= 4 x bound divided by |a|; the
inputs keep every ratio far from both edges, and open_rows() of the reference alone must stay under 1 % (asserted on the CPU)."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import train_kernels_ref as T

F32, F64 = np.float32, np.float64
U, TINY, MARGIN = T.U, T.TINY, T.MARGIN
CLIP = (0.2, 0.3)                      # asymmetric: the window is [0.8, 1.3]
KL_COEFS = (0.0, 0.05)
GSCALE = 1.0 / 37
MS, VS = (1, 5, 37), (4104, 4096, 1000, 257, 2)
RATIOS = (0.5, 0.7, 0.95, 1.0, 1.05, 1.2, 1.6, 2.0)       # placed ratios: below, inside and above [0.8, 1.3], none within 0.1 of an edge


def inputs(M, V, seed=0):
    """-> NS of torch tensors: logits (M, V) fp32 (row m of standard deviation 0.5 .. 20), target, adv (both signs and zero), weight (with zeros),
    old_lp (placed at the RATIOS, cycling against the sign of adv so that both signs see every zone), ref_lp (within 1 of lp)"""
    g = torch.Generator().manual_seed(9000 + 131 * M + V + seed)
    std = torch.tensor(np.geomspace(0.5, 20.0, M) if M > 1 else [3.0], dtype=torch.float32)
    logits = (torch.randn(M, V, generator=g) * std[:, None]).float()
    target = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    if M >= 5:
        target[0], target[1], target[2] = 0, V - 1, int(logits[2].argmax())
    sign = torch.tensor([(1.0, -1.0, 0.0)[(m + seed) % 3] for m in range(M)])
    adv = (sign * (0.25 + 2 * torch.rand(M, generator=g))).float()
    weight = torch.tensor([(1.0, 0.0, 0.37, 2.5)[(m // 3 + 1) % 4] for m in range(M)], dtype=torch.float32)
    lp = -T.ce(logits, target, None, 1.0).loss
    ratio = np.array([RATIOS[(m // 3 + seed) % len(RATIOS)] for m in range(M)])
    old_lp = torch.from_numpy((lp - np.log(ratio)).astype(F32))
    ref_lp = torch.from_numpy((lp + (2 * torch.rand(M, generator=g).double().numpy() - 1)).astype(F32))
    return NS(logits=logits, target=target, adv=adv, weight=weight, old_lp=old_lp, ref_lp=ref_lp)


def _np(t, dtype):
    return None if t is None else T.as_np(t, dtype)


def reference(logits, target, adv, weight=None, old_lp=None, ref_lp=None, clip=CLIP, kl_coef=0.0, gscale=1.0, bf16=False):
    """the contract in float64 on the stored fp32 inputs (scalars as the C ABI receives them) and the per-row bounds of the module's header"""
    ce = T.ce(logits, target, None, 1.0)
    l = T.as_np(logits, F64)
    M, V = l.shape
    tg = T.as_np(target, np.int64)
    a = _np(adv, F64)
    w = np.ones(M) if weight is None else _np(weight, F64)
    lo, hi, kc, gs = 1.0 - T.f32(clip[0]), 1.0 + T.f32(clip[1]), T.f32(kl_coef), T.f32(gscale)
    lp = -ce.loss
    e_lp = ce.loss_bound / MARGIN
    if old_lp is not None:
        da = lp - _np(old_lp, F64)
        r = np.exp(da)
        E_r = r * (e_lp + U * np.abs(da) + 2 * U) + TINY
    else:
        r, E_r = np.ones(M), np.zeros(M)
    cl = np.minimum(np.maximum(r, lo), hi)
    s1, s2 = r * a, cl * a
    active = s1 <= s2
    E_s1 = np.abs(a) * (E_r + U * r) if old_lp is not None else np.zeros(M)             # 1.0f * a is exact
    E_s2 = np.abs(a) * (np.maximum(E_r, 2 * U) + U * cl)
    if old_lp is not None:
        obj, E_obj = np.minimum(s1, s2), np.maximum(E_s1, E_s2)
    else:
        obj, E_obj = a * lp, np.abs(a) * e_lp + U * np.abs(a * lp)
    if ref_lp is not None:
        d = _np(ref_lp, F64) - lp
        e = np.exp(d)
        e_d = e_lp + U * np.abs(d)
        E_e = e * (e_d + 2 * U) + TINY
        k, dk = (e - d) - 1, 1 - e
        E_k = E_e + e_d + U * np.abs(e - d) + U * np.abs(k)
    else:
        k, dk, E_e, E_k = np.zeros(M), np.zeros(M), np.zeros(M), np.zeros(M)
    loss = -obj + kc * k
    c = np.where(active, s1, 0.0) - kc * dk
    E_c = np.where(active, E_s1, 0.0) + kc * (E_e + 2 * U * np.abs(dk)) + U * np.abs(c)
    coef = c * w
    E_coef = np.abs(w) * (E_c + U * np.abs(c))
    g = coef * gs
    E_g = abs(gs) * (E_coef + U * np.abs(coef))
    hot = np.zeros((M, V))
    hot[np.arange(M), tg] = 1
    ph = ce.p - hot
    dl = ph * g[:, None]
    eps_v = (2 * np.abs(l - l.max(1, keepdims=True)) + 4) * U
    dl_bound = MARGIN * (np.abs(g)[:, None] * (ce.p * (eps_v + ce.R[:, None] + 2 * U) + U * np.abs(ph)) + np.abs(ph) * E_g[:, None] + U * np.abs(dl)) \
        + 2 * TINY * (1 + np.abs(g)[:, None])
    if bf16:
        dl_bound = dl_bound + T.BF16_HALF_ULP * np.abs(dl)
    out = NS(logprob=lp, ratio=r, clipped=(~active).astype(np.int32), kl=k, loss=loss, coef=coef, dlogits=dl, s1=s1, s2=s2,
             logprob_bound=ce.loss_bound, ratio_bound=MARGIN * E_r, kl_bound=MARGIN * E_k + TINY,
             loss_bound=MARGIN * (E_obj + kc * (E_k + U * np.abs(k)) + U * np.abs(loss)) + TINY, coef_bound=MARGIN * E_coef + TINY, dl_bound=dl_bound)
    edge = np.where(a > 0, hi, lo)
    out.open = (a != 0) & (np.abs(r - edge) <= 4 * out.ratio_bound + 4 * U * edge) if old_lp is not None else np.zeros(M, bool)
    return out


def open_rows(ref):
    """rows whose clip decision the bound leaves open (the module's header)"""
    return ref.open


def model(logits, target, adv, weight=None, old_lp=None, ref_lp=None, clip=CLIP, kl_coef=0.0, gscale=1.0):
    """pg_kernel in numpy float32, operation by operation: ce_kernel's model for lp and the gradient pass, then the scalars of the contract"""
    M = T.as_np(logits, F32).shape[0]
    lp = -T.ce_model(logits, target, None, 1.0).loss
    a = _np(adv, F32)
    w = np.ones(M, F32) if weight is None else _np(weight, F32)
    lo, hi, kc = F32(1) - F32(clip[0]), F32(1) + F32(clip[1]), F32(kl_coef)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        r = np.exp((lp - _np(old_lp, F32)).astype(F32)).astype(F32) if old_lp is not None else np.ones(M, F32)
        s1 = r * a
        s2 = np.minimum(np.maximum(r, lo), hi) * a
        active = s1 <= s2
        k, dk = np.zeros(M, F32), np.zeros(M, F32)
        if ref_lp is not None:
            d = _np(ref_lp, F32) - lp
            e = np.exp(d).astype(F32)
            k, dk = (e - d) - F32(1), F32(1) - e
        c = np.where(active, s1, F32(0)) - kc * dk
        coef = (c * w).astype(F32)
        obj = np.minimum(s1, s2) if old_lp is not None else a * lp
        loss = -obj + kc * k
    dl = T.ce_model(logits, target, coef, gscale).dlogits               # identity (c): the gradient pass is ce_kernel's with the weight coef
    return NS(logprob=lp.astype(F32), ratio=r.astype(F32), clipped=(~active).astype(np.int32), kl=k.astype(F32), loss=loss.astype(F32), coef=coef,
              dlogits=dl)


def combos():
    """(weight, old_lp, ref_lp given?, kl_coef): every NULL pattern; a row of KL_COEFS per pattern with a reference, alternating without"""
    out = []
    for i in range(8):
        wg, og, rg = bool(i & 1), bool(i & 2), bool(i & 4)
        out += [(wg, og, rg, kc) for kc in (KL_COEFS if rg else (KL_COEFS[i & 1],))]
    return out


def pick(x, wg, og, rg):
    return dict(weight=x.weight if wg else None, old_lp=x.old_lp if og else None, ref_lp=x.ref_lp if rg else None)


FIELDS = (('logprob', 'logprob'), ('ratio', 'ratio'), ('kl', 'kl'), ('loss', 'loss'), ('coef', 'coef'))      # (output, bound stem) of the per-row outputs


def fraction(got, ref, name, bound):
    return T.ratio_of(T.abs_err(got, getattr(ref, name)), getattr(ref, bound))
