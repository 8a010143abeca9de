#!/usr/bin/env python3
"""Randomised sweep of the LoRA adapter kernels (csrc/lora.hip) against float64 references built from the host copy of the dropout mask
(oracle/lora_ref.py): cvar_lora_down (x_copy, the in-place [x | u] form), cvar_lora_dx (both dtype pairs, fused GELU'), cvar_lora_wgrad
(plain and transposed outputs, output offsets) - random shapes, strides, offsets, ranks, dropout rates and seeds, every operand inside a
NaN arena whose bytes outside the declared outputs must stay unchanged.  usage: fuzz_lora.py [n_cases] [seed]"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from controlvar_amd import ops
from oracle import lora_ref, var_ref

dev = torch.device('cuda:0')
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
U = 2.0 ** -24
PAD = 64
NAN = float('nan')


def arena(rows, ld, dtype):
    buf = torch.full((2 * PAD + rows * ld,), NAN, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + rows * ld].view(rows, ld)


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def factor(M, K, p, seed, tag):
    if p == 0:
        return torch.ones(M, K, dtype=torch.float64, device=dev)
    keep = torch.from_numpy(lora_ref.keep_mask(M, K, p, seed, tag)).to(dev)
    return torch.where(keep, lora_ref.inv_keep(p), 0.0).to(torch.float64)


def outside_unchanged(buf, before, window):
    """every element of buf outside `window` (a view into it) keeps its bits"""
    a, b = buf.clone(), before.clone()
    off = window.storage_offset() - buf.storage_offset()
    rows, cols = window.shape
    ld = window.stride(0)
    for t in (a, b):
        t.as_strided((rows, cols), (ld, 1), off).zero_()
    return torch.equal(bits(a), bits(b))


bad = 0
for case in range(n_cases):
    g = torch.Generator().manual_seed(case)
    kind = case % 3
    dtype = rng.choice([torch.float32, torch.bfloat16])
    M = rng.choice([1, 2, 15, 16, 17, 63, 64, 65, 1003, 2720, 10880, 43520])
    K = 8 * rng.randint(1, 800) if rng.random() < 0.6 else rng.choice([8, 504, 512, 520, 1000, 1536, 4096, 6144])
    if M * K > 6e7:
        M = rng.choice([1003, 2720])
    r = rng.choice([1, 2, 5, 8, 15, 16, 16])
    p = rng.choice([0.0, 0.0, 0.05, 0.3, 0.5, 0.9])
    scale = rng.choice([1.0, 2.0, 32.0 / r])
    seed, tag = rng.choice([0, 7, 2 ** 32 + 3, 2 ** 63 + 1, -9, rng.getrandbits(64)]), rng.randint(0, 99)
    f = factor(M, K, p, seed, tag) if kind < 2 else None
    if kind == 0:                                   # u = s drop(x) A^T: separate output, or u inside the [x | u | pad] row of x itself
        inplace = rng.random() < 0.3
        rp = rng.choice([16, 32, 64])
        ldx = K + (rp if inplace else 8 * rng.randint(0, 3))
        xb, x = arena(M, ldx, dtype)
        x[:, :K] = (torch.randn(M, K, generator=g) * rng.choice([0.3, 1.0, 4.0])).to(dtype).to(dev)
        ab, A = arena(r, K + 8 * rng.randint(0, 2), dtype)
        A[:, :K] = ((torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5).to(dtype).to(dev)
        a0 = ab.clone()
        if inplace:
            x[:, K:] = 0
            x0 = xb.clone()
            ops.lora_down(x, A, x, M=M, K=K, r=r, scale=scale, p=p, seed=seed, tag=tag, ldx=ldx, lda=A.stride(0), ldu=ldx, u_off=K)
            ub, before, u = xb, x0, x[:, K:K + r]
            xc_ok = True
        else:
            x0 = xb.clone()
            ldu = r + rng.randint(0, 9)
            ub, uw = arena(M, ldu, dtype)
            before = ub.clone()
            cb, xc = arena(M, K, dtype) if p > 0 else (None, None)
            ops.lora_down(x, A, uw, M=M, K=K, r=r, scale=scale, p=p, seed=seed, tag=tag, ldx=ldx, lda=A.stride(0), ldu=ldu, x_copy=xc)
            u = uw[:, :r]
            xc_ok = xc is None or (torch.equal(bits(xc), bits(x[:, :K].contiguous())) and bool(torch.isnan(cb[:PAD]).all())
                                   and bool(torch.isnan(cb[PAD + M * K:]).all()))
            xc_ok = xc_ok and torch.equal(bits(xb), bits(x0))
        ref = scale * (x[:, :K].double() * f) @ A[:, :K].double().t()
        S = scale * (x[:, :K].double().abs() * f) @ A[:, :K].double().abs().t()
        bound = (K + 2) * U * S + (ref.abs() * 2.0 ** -8 if dtype == torch.bfloat16 else 0)        # fp32 dot of K terms (+ one bf16 rounding)
        err = ((u.double() - ref).abs() - bound).max().item()
        fence = outside_unchanged(ub, before, u) and torch.equal(bits(ab), bits(a0)) and xc_ok
        ok = err <= 1e-30 and fence
        desc = dict(kind='down', M=M, K=K, r=r, dtype=str(dtype), p=p, inplace=inplace, fence=fence)
    elif kind == 1:                                 # dx = (dx + s drop'(du A)) * gelu'(aux), in place
        dxt = torch.float32 if dtype == torch.float32 else rng.choice([torch.float32, torch.bfloat16])
        lddx, lddu = K + 8 * rng.randint(0, 2), rng.choice([16, 24, 32])
        db, dx = arena(M, lddx, dxt)
        dx[:, :K] = torch.randn(M, K, generator=g).to(dxt).to(dev)
        ub, du = arena(M, lddu, dtype)              # du columns >= r stay NaN
        du[:, :r] = torch.randn(M, r, generator=g).to(dtype).to(dev)
        ab, A = arena(r, K, dtype)
        A[:, :] = (torch.randn(r, K, generator=g) / 4).to(dtype).to(dev)
        use_aux = rng.random() < 0.5
        if use_aux:
            xb, aux = arena(M, K, dtype)
            aux[:] = (torch.randn(M, K, generator=g) * 2).to(dtype).to(dev)
        else:
            aux = None
        before, u0 = db.clone(), ub.clone()
        dx0 = dx[:, :K].double()
        ops.lora_dx(dx, du, A, M=M, K=K, r=r, scale=scale, p=p, seed=seed, tag=tag, lddx=lddx, lddu=lddu, aux=aux)
        pre = dx0 + scale * f * (du[:, :r].double() @ A.double())
        S = dx0.abs() + scale * f * (du[:, :r].double().abs() @ A.double().abs())
        if use_aux:
            t = aux.double().requires_grad_(True)
            var_ref.gelu_tanh(t).sum().backward()
            gp = t.grad
        else:
            gp = torch.ones_like(pre)
        ref = pre * gp
        bound = (r + 4) * U * S * gp.abs() + (1e-5 * pre.abs() if use_aux else 0)      # fp32 (+ gelu' with a fast exp)
        if dxt == torch.bfloat16:
            bound = bound + ref.abs() * 2.0 ** -8
        err = ((dx[:, :K].double() - ref).abs() - bound).max().item()
        fence = outside_unchanged(db, before, dx[:, :K]) and torch.equal(bits(ub), bits(u0))
        ok = err <= 1e-30 and fence
        desc = dict(kind='dx', M=M, K=K, r=r, dtype=str(dtype), dx=str(dxt), p=p, aux=use_aux, fence=fence)
    else:                                           # G[n, j] = s sum_m drop(Y)[m, n] Z[m, j]
        N = K if rng.random() < 0.5 else 2 * rng.randint(1, 4700)
        if M * N > 6e7:
            M = 1003
        f = factor(M, N, p, seed, tag)
        ldy, ldz = N + 2 * rng.randint(0, 4), r + rng.randint(0, 20)
        yb, Y = arena(M, ldy, dtype)
        Y[:, :N] = torch.randn(M, N, generator=g).to(dtype).to(dev)
        zb, Z = arena(M, ldz, dtype)
        Z[:, :r] = torch.randn(M, r, generator=g).to(dtype).to(dev)
        nws = ops.lora_wgrad_ws_floats(M, N)
        wsb = torch.full((nws + 64,), NAN, device=dev)
        off = rng.randint(0, 40)
        tr = rng.random() < 0.5
        os_n, os_j = (1, N) if tr else (r + rng.randint(0, 3), 1)
        size = (r - 1) * os_j + (N - 1) * os_n + 1
        ob = torch.full((off + size + 64,), NAN, device=dev)
        ops.lora_wgrad(Y, Z, ob, wsb[:nws], M=M, N=N, r=r, scale=scale, p=p, seed=seed, tag=tag, ldy=ldy, ldz=ldz, out_off=off, os_n=os_n, os_j=os_j)
        Yf = Y[:, :N].double() * f
        ref = scale * Yf.t() @ Z[:, :r].double()
        S = scale * Yf.abs().t() @ Z[:, :r].double().abs()
        idx = off + torch.arange(N, device=dev)[:, None] * os_n + torch.arange(r, device=dev)[None, :] * os_j
        got = ob[idx].double()
        err = ((got - ref).abs() - (M + 8) * U * S).max().item()
        rest = torch.ones_like(ob, dtype=torch.bool)
        rest[idx] = False
        fence = bool(torch.isnan(ob[rest]).all()) and bool(torch.isnan(wsb[nws:]).all())
        ok = err <= 1e-30 and fence
        desc = dict(kind='wgrad', M=M, N=N, r=r, dtype=str(dtype), p=p, tr=tr, off=off, fence=fence)
    if not ok:
        bad += 1
        print('FAIL', case, desc, 'excess over bound', err)
torch.cuda.synchronize()
print(f'{n_cases - bad}/{n_cases} cases ok')
sys.exit(1 if bad else 0)
