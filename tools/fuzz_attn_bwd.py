#!/usr/bin/env python3
"""Randomised sweep of the MFMA attention backward (dq and dk/dv kernels) against the exact row-wise backward of the same
library: random rows / heads / block-causal level structures (ragged level lengths), qkv, o, do and dqkv embedded in
NaN-filled buffers so that a read or write outside a tensor shows up.  About a third of the cases split every level in halves
and make the second half blind to the first (the `indep` holes tools/fuzz_attn.py draws for the forward); about a fifth run with
l < Lmax, the arena rows behind l NaN in qkv and in dqkv, where they must stay NaN.

This is a SAME-LIBRARY comparison: both sides share vis_of, first_query_of and the level tables, so an error in those moves
both and the sweep stays green.  It finds what the two implementations do differently (tiles, masks, fences) over many
structures; the independent judge is tests/test_gpu_attn_train_oracle.py (float64 oracle, per-row metric).
usage: fuzz_attn_bwd.py [n_cases] [seed]"""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from controlvar_amd import ops

dev = torch.device('cuda:0'); T = torch.bfloat16
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
PAD = 4096


def arena(shape, fill=None, gen=None, amp=1.0):
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), float('nan'), device=dev, dtype=T)
    v = buf[PAD:PAD + n].view(*shape)
    if gen is not None:
        v.copy_((torch.randn(*shape, generator=gen) * amp).to(T))
    elif fill is not None:
        v.fill_(fill)
    return buf, v


bad = n_holes = n_short = 0
for case in range(n_cases):
    R, H = rng.choice([1, 2, 3]), rng.choice([1, 2, 4, 12])
    nl = rng.randint(1, 10)
    ends, acc = [], 0
    for _ in range(nl):
        acc += rng.choice([1, 2, 7, 8, 18, 50, 64, 72, 128, 200, 338, 512]); ends.append(acc)
    if acc > 1400:
        ends = [e for e in ends if e <= 1400] or [1400]
        acc = ends[-1]
    L = acc
    holes = None
    if rng.random() < 0.34:                               # indep form: halves of every level, the second half blind to the first
        lv, hl, b0 = [], [], 0
        for e in ends:
            half = (e - b0) // 2
            if half:
                lv += [b0 + half, e]; hl += [(0, 0), (b0, b0 + half)]
            else:
                lv.append(e); hl.append((0, 0))
            b0 = e
        ends, holes = lv, hl
        n_holes += 1
    Lmax = L + rng.choice([1, 5, 64, 131]) if rng.random() < 0.2 else L
    n_short += Lmax > L
    C3 = 3 * H * 64
    g = torch.Generator().manual_seed(case)
    amp = rng.choice([0.3, 1.0, 2.0])
    scale = rng.choice([0.125, 0.03125, 0.5])
    qb, qkv = arena((R, Lmax, C3))
    qkv[:, :L].copy_((torch.randn(R, L, C3, generator=g) * amp).to(T))          # rows [L, Lmax) stay NaN
    _, do = arena((R * L, H * 64), gen=g, amp=1.0)
    ob, out = arena((R * L, H * 64), fill=0.0)
    lse = torch.empty(R, H, L, device=dev, dtype=torch.float32)
    ops.attention(qkv, out, R, H, Lmax, 0, L, scale, ends, lse=lse, holes=holes)
    ws = torch.empty(R * H * L + 64, device=dev)
    b1, d1 = arena((R, Lmax, C3))
    b2, d2 = arena((R, Lmax, C3))
    d1[:, :L] = 0; d2[:, :L] = 0
    ops.attention_bwd(qkv, out, do, lse, d1, ws, R, H, Lmax, L, scale, ends, holes=holes)
    ops.attention_bwd(qkv, out, do, lse, d2, ws, R, H, Lmax, L, scale, ends, rowwise=True, holes=holes)
    a, b = d1[:, :L].float(), d2[:, :L].float()
    fin = torch.isfinite(a).all() and torch.isfinite(b).all()
    pads_ok = all(torch.isnan(x[:PAD]).all() and torch.isnan(x[-PAD:]).all() for x in (b1, b2, ob, qb))
    pads_ok = pads_ok and torch.isnan(d1[:, L:]).all() and torch.isnan(d2[:, L:]).all()
    ref = max(1.0, b.abs().max().item())
    err = (a - b).abs().max().item() / ref if fin else float('nan')
    ok = fin and pads_ok and err < 3e-2
    if not ok:
        bad += 1
        print('FAIL', case, dict(R=R, H=H, L=L, Lmax=Lmax, ends=ends, holes=holes, scale=scale, amp=amp), 'err', err, 'finite', bool(fin), 'pads intact', bool(pads_ok), flush=True)
print(f'{n_holes} cases with holes, {n_short} with l < Lmax')
print(f'{n_cases - bad}/{n_cases} cases ok')
sys.exit(1 if bad else 0)
