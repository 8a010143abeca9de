"""Shared by tests/test_distill_host.py (CPU) and tests/test_gpu_distill_kernel.py: the contract of cvar_kd_fwd_bwd (include/cvar_distill.h)
restated in float64 numpy on the fp32 inputs as stored, a numpy-float32 model of the kernel's order of operations, the per-row and per-element bounds, and
the inputs of the kernel sweep.  Both softmax parts are oracle/train_kernels_ref.py's cross-entropy (T.ce and its bound R, T.ce_model's loops): the kernel's
passes over the student row x and over the teacher row z are ce_kernel's.

Bounds (u = 2^-24, one rounding per operation, -ffp-contract=off; the house margin 4 is applied once, at the end; nothing here is measured on a kernel).
R_x, R_z are T.ce's relative error of se and sz; eps_v = (2 |d_v| + 4) u is its bound of __expf(d_v), d_v = x_v - mx or z_v - mz.
    lse_x = logf(se) + mx              e_lx = R_x + 2 u |log se| + u |lse_x|             (d log, logf 1 ulp, the sum);   e_lz likewise
    a_v = z_v - lse_z, b_v = x_v - lse_x    e_lz + u |a_v|,  e_lx + u |b_v|
    t_v = a_v - b_v                    E_t = e_lz + e_lx + u (|a_v| + |b_v| + |t_v|)
    q_v = __expf(z_v - mz) (1 / sz)    relative rq_v = eps_v + R_z + 2 u  (the quotient and the product);   p_v: rp_v = eps_v + R_x + 2 u
    term_v = q_v t_v                   q_v (rq_v |t_v| + E_t) + u |q_v t_v| + TINY
    kl = sum_v term_v                  depth D = ceil(V / 256) + 8 (lane, wave tree, four partials):  sum_v of the terms' bounds + D u sum_v |q_v t_v|
        - ABSOLUTE: kl cancels to zero at teacher = student, where every t_v is 0 while |a_v|, |b_v| are not; the bound prices the cancellation by
        |a_v| + |b_v| and by sum |q_v t_v|, never by |kl|.
    g = w gscale                       u |g|
    dlogits_v = (p_v - q_v) g          |g| (p_v rp_v + q_v rq_v + u |p_v - q_v|) + 2 u |dl_v|   (g's rounding and the product)  + 4 TINY (1 + |g|)
                                       (+ 2^-8 |ref| in bf16)   - absolute as well: p - q cancels where the student has learnt the teacher."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import train_kernels_ref as T
from oracle.norm_ref import _wave_sum

F32, F64 = np.float32, np.float64
U, TINY, MARGIN = T.U, T.TINY, T.MARGIN
GSCALE = 1.0 / 37
MS, VS = (1, 5, 37), (4096, 4104, 1000, 257, 2)
LDT_PAD = 8
RANGE = 30.0                            # teacher logits reach +-30, as guided logits at cfg = 4 do


def inputs(M, V, seed=0):
    """-> NS of torch tensors: logits (M, V) fp32 (row m of standard deviation 0.5 .. 20), teacher (M, V) fp32 (row m from near-uniform, standard deviation
    0.02, to sharply peaked, 12, clamped to +-RANGE, in the opposite order of the student's spread; with M >= 5 row 1 is the student's own row plus noise
    of 1e-3 - the nearly-learnt case, where kl and p - q cancel), weight (with zeros)"""
    g = torch.Generator().manual_seed(7000 + 131 * M + V + seed)
    std = torch.tensor(np.geomspace(0.5, 20.0, M) if M > 1 else [3.0], dtype=torch.float32)
    logits = (torch.randn(M, V, generator=g) * std[:, None]).float()
    tstd = torch.tensor(np.geomspace(12.0, 0.02, M) if M > 1 else [4.0], dtype=torch.float32)
    teacher = (torch.randn(M, V, generator=g) * tstd[:, None]).clamp(-RANGE, RANGE).float()
    if M >= 5:
        teacher[1] = logits[1] + 1e-3 * torch.randn(V, generator=g)
        teacher[2, int(teacher[2].argmax())] = RANGE                # a row at the edge of the range
        teacher[2, int(teacher[2].argmin())] = -RANGE
    weight = torch.tensor([(1.0, 0.0, 0.37, 2.5)[(m // 3 + 1) % 4] for m in range(M)], dtype=torch.float32)
    return NS(logits=logits, teacher=teacher, weight=weight)


def onehot_teacher(target, V):
    """identity (b): 0 at the target's column and -200 elsewhere"""
    z = torch.full((target.numel(), V), -200.0)
    z[torch.arange(target.numel()), target.long()] = 0.0
    return z


def _softmax_parts(l):
    """T.ce on a row block, without a target: p, lse, R, eps_v, mx (float64)"""
    M, V = l.shape
    ce = T.ce(torch.from_numpy(l.astype(F32)), torch.zeros(M, dtype=torch.int32), None, 1.0)
    mx = l.max(1, keepdims=True)
    d = l - mx
    se = np.exp(d).sum(1, keepdims=True)
    return NS(p=ce.p, lse=(np.log(se) + mx)[:, 0], logse=np.log(se)[:, 0], R=ce.R, eps=(2 * np.abs(d) + 4) * U)


def reference(logits, teacher, weight=None, gscale=1.0, bf16=False):
    """the contract in float64 on the stored fp32 inputs (gscale as the C ABI receives it) and the bounds of the module's header"""
    x, z = T.as_np(logits, F64), T.as_np(teacher, F64)
    M, V = x.shape
    w = np.ones(M) if weight is None else T.as_np(weight, F64)
    g = w * T.f32(gscale)
    sx, sz = _softmax_parts(x), _softmax_parts(z)
    e_lx = sx.R + 2 * U * np.abs(sx.logse) + U * np.abs(sx.lse)
    e_lz = sz.R + 2 * U * np.abs(sz.logse) + U * np.abs(sz.lse)
    a, b = z - sz.lse[:, None], x - sx.lse[:, None]
    t = a - b
    E_t = (e_lz + e_lx)[:, None] + U * (np.abs(a) + np.abs(b) + np.abs(t))
    rq, rp = sz.eps + sz.R[:, None] + 2 * U, sx.eps + sx.R[:, None] + 2 * U
    q, p = sz.p, sx.p
    term = q * t
    kl = term.sum(1)
    D = -(-V // 256) + 8
    kl_bound = MARGIN * ((q * (rq * np.abs(t) + E_t) + U * np.abs(term) + TINY).sum(1) + D * U * np.abs(term).sum(1))
    dl = (p - q) * g[:, None]
    ag = np.abs(g)[:, None]
    dl_bound = MARGIN * (ag * (p * rp + q * rq + U * np.abs(p - q)) + 2 * U * np.abs(dl)) + 4 * TINY * (1 + ag)
    if bf16:
        dl_bound = dl_bound + T.BF16_HALF_ULP * np.abs(dl)
    return NS(loss=kl, dlogits=dl, p=p, q=q, loss_bound=kl_bound, dl_bound=dl_bound)


def _row_pass(l):
    """ce_kernel's first two passes in float32 -> (mx (M, 1), e padded (M, 256 K), se (M,))"""
    M, V = l.shape
    K = -(-V // 256)
    pad = np.full((M, K * 256), -np.inf, F32)
    pad[:, :V] = l
    mx = pad.max(1, keepdims=True)
    e = np.exp(pad - mx).astype(F32)
    return mx, e, _lanes_sum(e)


def _lanes_sum(v):
    """(M, 256 K) per-element values -> the block sum: lane v % 256 accumulates in order, shuffle tree per wave, (w0 + w1) + (w2 + w3)"""
    a = np.zeros((v.shape[0], 256), F32)
    for k in range(v.shape[1] // 256):
        a = a + v[:, k * 256:(k + 1) * 256]
    w4 = [_wave_sum(a[:, 64 * k:64 * k + 64]) for k in range(4)]
    return ((w4[0] + w4[1]) + (w4[2] + w4[3])).astype(F32)


def model(logits, teacher, weight=None, gscale=1.0, fault=None):
    """kd_kernel in numpy float32, operation by operation (np.exp / np.log in float32 stand for __expf / logf).  fault: a planted mistake the bounds must
    see - 'p_for_q' (the KL weighted by the student's probabilities), 'unnormalised_teacher' (z_v in the place of z_v - lse_z), 'q_unscaled' (the gradient's
    q_v without 1 / sz)"""
    x, z = T.as_np(logits, F32), T.as_np(teacher, F32)
    M, V = x.shape
    with np.errstate(invalid='ignore', divide='ignore', over='ignore', under='ignore'):
        mx, ex, se = _row_pass(x)
        mz, ez, sz = _row_pass(z)
        lse_x = np.log(se).astype(F32) + mx[:, 0]
        lse_z = np.log(sz).astype(F32) + mz[:, 0]
        inv, invz = F32(1) / se, F32(1) / sz
        p = ex[:, :V] * inv[:, None]
        q = ez[:, :V] * invz[:, None]
        a = z if fault == 'unnormalised_teacher' else z - lse_z[:, None]
        term = np.zeros_like(ex)
        term[:, :V] = (p if fault == 'p_for_q' else q) * (a - (x - lse_x[:, None]))
        kl = _lanes_sum(term)
        g = (np.ones(M, F32) if weight is None else T.as_np(weight, F32)) * F32(gscale)
        dl = (p - (ez[:, :V] if fault == 'q_unscaled' else q)) * g[:, None]
    return NS(loss=kl.astype(F32), dlogits=dl.astype(F32))


FAULTS = ('p_for_q', 'unnormalised_teacher', 'q_unscaled')


def fractions(got_loss, got_dl, ref):
    """-> (largest |loss error| / bound, largest |dlogits error| / bound or None)"""
    fl = T.ratio_of(T.abs_err(got_loss, ref.loss), ref.loss_bound)
    return fl, (T.ratio_of(T.abs_err(got_dl, ref.dlogits), ref.dl_bound) if got_dl is not None else None)
