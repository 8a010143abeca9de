"""cvar_ln_modulate_wide, cvar_ln_modulate_split3_wide and cvar_ln_modulate_fp8_wide on MI355X (include/cvar_wide.h).

Rows of 2048 < C <= CVAR_WIDE_CMAX against the float64 oracle of oracle/norm_ref.py at its bound (tests/test_wide_host.py shows on the CPU that a model of
the wide layout sits at <= 0.21 of it - asserted there at <= 0.5 - and that planted faults overshoot it >= 100 x - asserted at >= 10 x): C = 2052 (one live lane in the ninth vector), 2304 (d36), 2500 (a tail in
the tenth vector), 2560 (d40), 2816 and CMAX; M = 1, 5, 9 at four rows per block; rows_per 1 and 3; the adaLN table wider than its rows, read at a column
offset.  The split and the e4m3 store are held bit for bit to the two-call forms their narrow namesakes promise; at C <= 2048 the wide entry points are held
to the bits of the old ones.  Every operand and output lies between NaN pads, and a refused call leaves its output NaN."""
import math

import numpy as np
import pytest
import torch

import wide_ref as W
from conftest import record
from oracle import norm_ref as N

pytestmark = pytest.mark.gpu

from controlvar_amd import _lib, ops  # noqa: E402
from controlvar_amd._lib import CvarError  # noqa: E402

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
TD = {'f32': F32, 'bf16': BF16}
PAD = 4096


def fenced(shape, dtype, dev, value=None, shift=0):
    """(buffer, view): a tensor of `shape` between two NaN pads (0xFF bytes for uint8) of >= PAD elements, `shift` elements off the pad's end"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD + shift,), 0xFF if dtype == U8 else float('nan'), device=dev, dtype=dtype)
    view = buf[PAD + shift:PAD + shift + n].view(*shape)
    if value is not None:
        view.copy_(torch.as_tensor(value).to(dtype))
    return buf, view


def untouched(t):
    return bool((t == 0xFF).all()) if t.dtype == U8 else bool(torch.isnan(t).all())


def pads_intact(*pairs):
    for buf, view in pairs:
        lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        if not (untouched(buf[:lo]) and untouched(buf[lo + view.numel():])):
            return False
    return True


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32, U8: torch.uint8}[t.dtype])


def ada_table(s, b, dev):
    """(pair, scale_off, shift_off, ld): the adaLN rows [4 unused | scale (C) | 4 unused | shift (C) | 4 unused] - ld_ada > 2 C, both read at a column offset"""
    G, C = s.shape
    z = torch.full((G, 4), float('nan'))
    return fenced((G, 2 * C + 12), F32, dev, torch.cat([z, s, z, b, z], 1)), 4, C + 8, 2 * C + 12


def operands(n, dev):
    C, M, rp, fam = W.CASES[n]
    x, s, b, ex, y32 = W.refs(n)
    return fenced((M, C), F32, dev, x), ada_table(s, b, dev)


# ================================================================================================ against the float64 oracle
@pytest.mark.parametrize('out_dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('n', list(W.CASES), ids=W.name)
def test_wide_rows_against_the_oracle(gpu_device, n, out_dtype):
    """4 E_m per row (+ half a bf16 ulp): norm_ref.ln_fwd_bound, ratio <= 1; a constant row whose fp32 mean is exact gives exactly the shift"""
    C, M, rp, fam = W.CASES[n]
    x, s, b, ex, y32 = W.refs(n)
    xp, (ap, sc, sh, ld) = operands(n, gpu_device)
    op = fenced((M, C), TD[out_dtype], gpu_device)
    ops.ln_modulate_wide(xp[1], ap[1], sc, sh, ld, rp, op[1], M, C, N.EPS)
    assert pads_intact(xp, ap, op)
    bd = N.ln_fwd_bound(ex, y32, x, s, rp, out_dtype == 'bf16')
    got = op[1].detach().cpu().double().numpy()
    err = np.abs(got - ex.y)
    ratio = N.ratio_of(np.where(np.isfinite(err), err, np.inf), bd.bound * np.ones_like(ex.y))
    print(f'[wide] ln_modulate_wide {W.name(n)} {out_dtype}: kernel {float(np.nanmax(err)):.3e}  yardstick {float(bd.E.max()):.3e}  ratio {ratio:.3f}')
    record(f'ln_modulate_wide {W.name(n)} {out_dtype}', kind='norm_oracle', tensor='y', kernel=float(np.nanmax(err)), yardstick=float(bd.E.max()),
           bound=float(np.max(bd.bound)), ratio=ratio, op='ln_modulate_wide', dtype=out_dtype, case=n)
    if fam == 'const_row':
        for m in range(M):
            if m % 4 < 2:            # 1.5 C and 2.25 C are exact in fp32 for these C, so is the mean: xhat = 0 and y = b
                want = b[m // rp].to(TD[out_dtype]).to(gpu_device)
                assert torch.equal(bits(op[1][m]), bits(want)), f'constant row {m} (x = {N.CONST_ROW_VALUES[m % 4]}) must give exactly the shift'
    assert ratio <= 1.0, (W.name(n), out_dtype, ratio)


# ================================================================================================ the mutual contracts of the three stores
@pytest.mark.parametrize('n', list(W.CASES), ids=W.name)
def test_split3_wide_equals_split3_of_the_fp32_rows(gpu_device, n):
    C, M, rp, fam = W.CASES[n]
    xp, (ap, sc, sh, ld) = operands(n, gpu_device)
    y = torch.empty(M, C, device=gpu_device, dtype=F32)
    ops.ln_modulate_wide(xp[1], ap[1], sc, sh, ld, rp, y, M, C, N.EPS)
    want = torch.empty(M, 3 * C, device=gpu_device, dtype=BF16)
    ops.split3(y, want, M, C)
    op = fenced((M, 3 * C), BF16, gpu_device)
    ops.ln_modulate_split3_wide(xp[1], ap[1], sc, sh, ld, rp, op[1], M, C, N.EPS)
    assert pads_intact(xp, ap, op)
    assert torch.equal(bits(op[1]), bits(want))


@pytest.mark.parametrize('wider', [0, 256], ids=['ldq-min', 'ldq+256'])
@pytest.mark.parametrize('n', list(W.CASES), ids=W.name)
def test_fp8_wide_equals_quant_rows_of_the_bf16_rows(gpu_device, n, wider):
    """bytes, scales and the pad bytes [C, ldq), for ldq = C rounded up to 128 and for a wider one"""
    C, M, rp, fam = W.CASES[n]
    ldq = ops.fp8_ldq(C) + wider
    xp, (ap, sc, sh, ld) = operands(n, gpu_device)
    y = torch.empty(M, C, device=gpu_device, dtype=BF16)
    ops.ln_modulate_wide(xp[1], ap[1], sc, sh, ld, rp, y, M, C, N.EPS)
    wq, wscale = torch.full((M, ldq), 0xFF, device=gpu_device, dtype=U8), torch.empty(M, device=gpu_device, dtype=F32)
    ops.quant_rows_fp8(y, wq, wscale, M=M, K=C, ldq=ldq)
    qp, sp = fenced((M, ldq), U8, gpu_device), fenced((M,), F32, gpu_device)
    ops.ln_modulate_fp8_wide(xp[1], ap[1], sc, sh, ld, rp, qp[1], sp[1], M, C, N.EPS, ldq=ldq)
    assert pads_intact(xp, ap, qp, sp)
    assert torch.equal(qp[1], wq) and torch.equal(bits(sp[1]), bits(wscale))
    assert not bool(qp[1][:, C:].any()), 'pad bytes [C, ldq) are zero'
    lg = torch.log2(sp[1])
    assert torch.equal(lg, lg.round()), 'one power-of-two scale per row'


# ================================================================================================ C <= 2048: the bits of the old entry points
def _call(fn, x, ada, sc, sh, ld, rp, *rest):
    base = ada.data_ptr()
    return fn(x.data_ptr(), base + 4 * sc, base + 4 * sh, ld, rp, *rest, ops._stream())


@pytest.mark.parametrize('C', [128, 1000, 2048])
def test_narrow_rows_through_the_wide_entry_points_give_the_old_bits(gpu_device, C):
    lib, M, rp, dev = _lib.load(), 9, 3, gpu_device
    g = torch.Generator().manual_seed(C)
    x = N._ln_x(g, M, C, 'unit').float()
    s, b = 0.4 * torch.randn(3, C, generator=g), 0.4 * torch.randn(3, C, generator=g)
    xp, (ap, sc, sh, ld) = fenced((M, C), F32, dev, x), ada_table(s, b, dev)
    for dtype in (F32, BF16):
        old, new = torch.empty(M, C, device=dev, dtype=dtype), fenced((M, C), dtype, dev)
        ops.ln_modulate(xp[1], ap[1], sc, sh, ld, rp, old, M, C, N.EPS)
        assert _call(lib.cvar_ln_modulate_wide, xp[1], ap[1], sc, sh, ld, rp, new[1].data_ptr(), ops.dt(new[1]), M, C, N.EPS) == 0
        assert pads_intact(new) and torch.equal(bits(new[1]), bits(old))
    old, new = torch.empty(M, 3 * C, device=dev, dtype=BF16), fenced((M, 3 * C), BF16, dev)
    ops.ln_modulate_split3(xp[1], ap[1], sc, sh, ld, rp, old, M, C, N.EPS)
    assert _call(lib.cvar_ln_modulate_split3_wide, xp[1], ap[1], sc, sh, ld, rp, new[1].data_ptr(), M, C, N.EPS) == 0
    assert pads_intact(new) and torch.equal(bits(new[1]), bits(old))
    ldq = ops.fp8_ldq(C)
    oq, oscale = torch.empty(M, ldq, device=dev, dtype=U8), torch.empty(M, device=dev, dtype=F32)
    ops.ln_modulate_fp8(xp[1], ap[1], sc, sh, ld, rp, oq, oscale, M, C, N.EPS, ldq=ldq)
    nq, ns = fenced((M, ldq), U8, dev), fenced((M,), F32, dev)
    assert _call(lib.cvar_ln_modulate_fp8_wide, xp[1], ap[1], sc, sh, ld, rp, nq[1].data_ptr(), ldq, ns[1].data_ptr(), M, C, N.EPS) == 0
    assert pads_intact(nq, ns, xp, ap) and torch.equal(nq[1], oq) and torch.equal(bits(ns[1]), bits(oscale))


# ================================================================================================ refusals
def test_wide_entry_points_refuse_without_writing(gpu_device):
    """C > CMAX, C % 4, ld_ada % 4 and (split3 / fp8) a pointer 4 bytes off are CVAR_EUNSUPPORTED (-2) before any launch: fences and outputs stay NaN"""
    dev = gpu_device
    # (C, ld_ada, elements x is shifted by)
    for C, ld, xs in ((W.CMAX + 4, 2 * W.CMAX + 8, 0), (2306, 4612, 0), (2304, 4610, 0), (2304, 4608, 1)):
        M = 3
        xp, ap = fenced((M, C), F32, dev, torch.ones(M, C), shift=xs), fenced((M, ld), F32, dev, torch.zeros(M, ld))
        ldq = ops.fp8_ldq(C)
        o32, o16, o3 = fenced((M, C), F32, dev), fenced((M, C), BF16, dev), fenced((M, 3 * C), BF16, dev)
        q, qs = fenced((M, ldq), U8, dev), fenced((M,), F32, dev)
        calls = [lambda: ops.ln_modulate_split3_wide(xp[1], ap[1], 0, C, ld, 1, o3[1], M, C, N.EPS),
                 lambda: ops.ln_modulate_fp8_wide(xp[1], ap[1], 0, C, ld, 1, q[1], qs[1], M, C, N.EPS, ldq=ldq)]
        if not xs:                   # cvar_ln_modulate_wide keeps its namesake's contract: no alignment refusal of its own
            calls += [lambda: ops.ln_modulate_wide(xp[1], ap[1], 0, C, ld, 1, o32[1], M, C, N.EPS), lambda: ops.ln_modulate_wide(xp[1], ap[1], 0, C, ld, 1, o16[1], M, C, N.EPS)]
        for call in calls:
            with pytest.raises(CvarError, match=r'\(-2\)'):
                call()
        torch.cuda.synchronize()
        assert all(untouched(p[0]) for p in (o32, o16, o3, q, qs)) and pads_intact(xp, ap), (C, ld, xs)
    # a misaligned output of the split3 form (4 bytes off) and of the e4m3 form (8 bytes off)
    C, M, ld = 2304, 3, 4608
    xp, ap = fenced((M, C), F32, dev, torch.ones(M, C)), fenced((M, ld), F32, dev, torch.zeros(M, ld))
    o3, q, qs = fenced((M, 3 * C), BF16, dev, shift=2), fenced((M, C), U8, dev, shift=8), fenced((M,), F32, dev)
    with pytest.raises(CvarError, match=r'\(-2\)'):
        ops.ln_modulate_split3_wide(xp[1], ap[1], 0, C, ld, 1, o3[1], M, C, N.EPS)
    with pytest.raises(CvarError, match=r'\(-2\)'):
        ops.ln_modulate_fp8_wide(xp[1], ap[1], 0, C, ld, 1, q[1], qs[1], M, C, N.EPS, ldq=C)
    torch.cuda.synchronize()
    assert all(untouched(p[0]) for p in (o3, q, qs))
