"""The kernel-level promises of gemm_precision='fp8' on MI355X (include/cvar_serve.h), against the numpy restatement tests/fp8_ref.py.

cvar_quant_rows_fp8: bytes and scales bit for bit against the oracle - K = 128 (one K tile), 1000 (a pad), 1536, 6144, one block and more than one
(M = 1 / 5 / 9 at four rows per block), bf16 and fp32 input, ldx > K, rows whose scales span 2^-20 ... 2^20, a zero row, a NaN row, zero pad bytes,
NaN fences around q and scale untouched.
cvar_ln_modulate_fp8 is DEFINED as cvar_quant_rows_fp8(the bf16 rows of cvar_ln_modulate): every case compares its bits with that two-pass form taken on
the device AND with the oracle applied to the device's bf16 rows.
cvar_gemm_fp8: integer operands in [-8, 8] (exact in e4m3; every partial sum below 2^24) must give the float64 product exactly, with asymmetric A and W -
that establishes the operand and accumulator lane maps and the K order; then random e4m3 bytes against float64 at the bound fp8_ref derives, with the
epilogue's roundings added per case.  The observed / bound ratios are printed and recorded.  Every refusal is checked without a write."""
import numpy as np
import pytest
import torch

import fp8_ref as F
from conftest import record

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402
from controlvar_amd._lib import ACT_GELU_TANH, CvarError  # noqa: E402

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8
EPS = 1e-6
PAD = 4096
U24 = 2.0 ** -24


def fenced(shape, dtype, dev, value=None, fill=None):
    """a view inside a buffer with fences on both sides: NaN for float types, 0xA5 for bytes"""
    n = int(np.prod(shape))
    fill = (0xA5 if dtype == U8 else float('nan')) if fill is None else fill
    buf = torch.full((n + 2 * PAD,), fill, device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(torch.as_tensor(value).to(dtype))
    return buf, view


def pads_intact(*pairs):
    for buf, view in pairs:
        lo, hi = buf[:PAD], buf[PAD + view.numel():]
        ok = (bool((lo == 0xA5).all()) and bool((hi == 0xA5).all())) if buf.dtype == U8 else (bool(torch.isnan(lo).all()) and bool(torch.isnan(hi).all()))
        if not ok:
            return False
    return True


# ================================================================================================ quant_rows_fp8
def quant_input(M, K, ldx, seed):
    rng = np.random.default_rng(seed)
    x = np.full((M, ldx), np.nan, dtype=np.float32)                         # columns >= K are never read: NaN there must not show
    x[:, :K] = rng.standard_normal((M, K)) * np.exp2(rng.integers(-20, 21, (M, 1)))
    x[:, :K] *= np.exp2(rng.integers(-6, 1, (M, K)))                        # several binades inside a row: subnormal e4m3 codes and zeros occur
    if M >= 5:
        x[1, :K] = 0                                                        # a zero row ...
        x[1, K // 3] = -0.0                                                 # ... with a -0.0: k = -60 all the same, and that byte is 0x80
        x[3, K // 2] = np.nan                                               # a NaN row
        x[4, :K] = 448.0 * 2.0 ** -3                                        # amax exactly on a scale edge
    if M >= 9:
        x[6, K - 1] = -np.inf
        x[7, :K] = np.nextafter(np.float32(448.0 * 2.0 ** 5), np.float32(np.inf))       # one ulp above an edge
    return x


@pytest.mark.parametrize('dtype', [F32, BF16])
@pytest.mark.parametrize('M', [1, 5, 9])
@pytest.mark.parametrize('K', [128, 1000, 1536, 6144])
def test_quant_rows_bit_for_bit(gpu_device, K, M, dtype):
    dev = gpu_device
    ldx = K + 8
    x = quant_input(M, K, ldx, 100 * K + 10 * M + (dtype == BF16))
    xt = torch.from_numpy(x).to(dtype)
    xv = xt.float().numpy()[:, :K]                                           # the values the kernel sees
    ldq = F.ldq_of(K)
    xp, qp, sp = fenced((M, ldx), dtype, dev, xt), fenced((M, ldq), U8, dev), fenced((M,), F32, dev)
    ops.quant_rows_fp8(xp[1], qp[1], sp[1], M=M, K=K, ldx=ldx, ldq=ldq)
    torch.cuda.synchronize()
    assert pads_intact(xp, qp, sp)
    wq, ws = F.quant_rows(xv, ldq)
    gq, gs = qp[1].cpu().numpy(), sp[1].cpu().numpy()
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (gs, ws)
    assert not gq[:, K:].any()
    if M >= 5:
        assert gs[1] == np.float32(2.0 ** -60) and gq[1, K // 3] == 0x80 and int(np.count_nonzero(gq[1])) == 1
    bad = np.argwhere(gq != wq)
    assert bad.size == 0, (bad[:5], gq[tuple(bad[0])], wq[tuple(bad[0])], xv[tuple(bad[0])] if bad[0][1] < K else None)


def test_quant_rows_wider_ldq_and_offsets(gpu_device):
    """a layer's slice of a stacked buffer: byte offset, scale offset, ldq wider than K rounded up"""
    dev = gpu_device
    M, K, ldq = 6, 200, 384
    x = quant_input(M, K, K, 7)
    q, s = fenced((3 * M, ldq), U8, dev), fenced((3 * M,), F32, dev)
    ops.quant_rows_fp8(torch.from_numpy(x).to(dev), q[1], s[1], M=M, K=K, ldq=ldq, q_off=M * ldq, s_off=M)
    torch.cuda.synchronize()
    assert pads_intact(q, s)
    wq, ws = F.quant_rows(x, ldq)
    assert np.array_equal(q[1][M:2 * M].cpu().numpy(), wq) and np.array_equal(s[1][M:2 * M].cpu().numpy(), ws)
    assert bool((q[1][:M] == 0xA5).all()) and bool((q[1][2 * M:] == 0xA5).all()) and bool(torch.isnan(s[1][:M]).all()) and bool(torch.isnan(s[1][2 * M:]).all())


# ================================================================================================ ln_modulate_fp8
def ln_inputs(C, M, rp, seed):
    g = torch.Generator().manual_seed(seed)
    G = (M + rp - 1) // rp
    x = torch.randn(M, C, generator=g) * 3 + torch.randn(M, 1, generator=g)
    x *= torch.exp2(torch.randint(-20, 21, (M, 1), generator=g).float())       # the residual stream's scale does not reach the row (LN), the table's does
    x[0, 0] = 1e4 * x[0, 1].abs()                                              # one outlier: the row statistics matter
    ld = 6 * C + 8                                                             # a wider ld_ada: scale at column 2 C + 4, shift at 4 C + 8
    ada = torch.randn(G, ld, generator=g) * 0.5
    ada *= torch.exp2(torch.randint(-10, 11, (G, 1), generator=g).float())     # rows whose outputs span many scales
    return x, ada, ld


@pytest.mark.parametrize('rp', [1, 3])
@pytest.mark.parametrize('M', [1, 5, 9])
@pytest.mark.parametrize('C,wide', [(128, 0), (128, 384), (1000, 0), (1000, 512), (1536, 0), (1920, 0), (2048, 0), (2048, 128)])
def test_ln_modulate_fp8_equals_quant_of_ln_modulate(gpu_device, C, wide, M, rp):
    """wide: ldq beyond C rounded up to 128 by that many bytes (the 0xA5 the buffers start with must be gone from every pad byte: [C, ldq) is zeros)"""
    dev = gpu_device
    x, ada, ld = ln_inputs(C, M, rp, 1000 * C + 10 * M + rp)
    if M >= 5:
        x[2] = 0                                                               # LN of a zero row: the row is the shift
        x[3, 5] = float('nan')                                                 # a broken activation shows as 0x7F bytes
    ldq = F.ldq_of(C) + wide
    xp, ap = fenced((M, C), F32, dev, x), fenced(tuple(ada.shape), F32, dev, ada)
    yp = fenced((M, C), BF16, dev)
    q2, s2 = fenced((M, ldq), U8, dev), fenced((M,), F32, dev)
    q1, s1 = fenced((M, ldq), U8, dev), fenced((M,), F32, dev)
    so, sh = 2 * C + 4, 4 * C + 8
    ops.ln_modulate(xp[1], ap[1], so, sh, ld, rp, yp[1], M, C, EPS)
    ops.quant_rows_fp8(yp[1], q2[1], s2[1], M=M, K=C, ldq=ldq)
    ops.ln_modulate_fp8(xp[1], ap[1], so, sh, ld, rp, q1[1], s1[1], M, C, EPS, ldq=ldq)
    torch.cuda.synchronize()
    assert pads_intact(xp, ap, yp, q1, s1, q2, s2)
    assert torch.equal(q1[1], q2[1]) and torch.equal(s1[1].view(torch.int32), s2[1].view(torch.int32))
    assert not bool(q1[1][:, C:].any())
    wq, ws = F.quant_rows(yp[1].float().cpu().numpy(), ldq)
    assert np.array_equal(q1[1].cpu().numpy(), wq) and np.array_equal(s1[1].cpu().numpy().view(np.uint32), ws.view(np.uint32))
    if M >= 5:
        assert bool((q1[1][3, :C] == 0x7F).all()) and float(s1[1][3]) == 1.0 and not bool(q1[1][3, C:].any())


# ================================================================================================ gemm_fp8
def run_gemm(dev, qa, sa, qw, sw, M, N, K, out_dtype=F32, **kw):
    """the call on fenced buffers; returns (C as float64 numpy, the fenced pairs)"""
    ap, wp = fenced(qa.shape, U8, dev, torch.from_numpy(qa)), fenced(qw.shape, U8, dev, torch.from_numpy(qw))
    sap, swp = fenced(sa.shape, F32, dev, torch.from_numpy(sa)), fenced(sw.shape, F32, dev, torch.from_numpy(sw))
    cp = fenced((M, N), out_dtype, dev)
    ops.gemm_fp8(ap[1], sap[1], wp[1], swp[1], cp[1], M=M, N=N, K=K, lda=qa.shape[1], ldw=qw.shape[1], **kw)
    torch.cuda.synchronize()
    assert pads_intact(ap, wp, sap, swp, cp)
    return cp[1].double().cpu().numpy()


def integer_operands(M, N, K, seed):
    """integers in [-8, 8] with no symmetry between A and W or between rows and columns: A carries its row index, W its column index, in a few entries"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (M, K)).astype(np.float64)
    w = rng.integers(-8, 9, (N, K)).astype(np.float64)
    a[:, 0] = np.arange(M) % 9
    w[:, 1] = -(np.arange(N) % 8)
    a[:, K - 1] = (np.arange(M) // 9) % 9 - 4
    w[:, K - 2] = (np.arange(N) // 8) % 9 - 4
    return a, w


@pytest.mark.parametrize('scaled', [False, True])
@pytest.mark.parametrize('M,N,K', [(5, 256, 128), (300, 200, 384), (257, 264, 1536), (512, 256, 6144), (1100, 520, 256), (70, 203, 128)])
def test_gemm_fp8_exact_on_integers(gpu_device, M, N, K, scaled):
    """(1100, 520, 256): the 256x256 tile with row and column tails; the rest run the 128x128 tile; (70, 203, 128): an N that is no multiple of 4 - the
    element-wise epilogue instead of the 16-byte one"""
    a, w = integer_operands(M, N, K, M + N + K)
    qa, qw = F.encode_rne(a), F.encode_rne(w)
    assert np.array_equal(F.decode(qa), a) and np.array_equal(F.decode(qw), w)
    rng = np.random.default_rng(K)
    sa = np.exp2(rng.integers(-6, 7, M)).astype(np.float32) if scaled else np.ones(M, np.float32)
    sw = np.exp2(rng.integers(-6, 7, N)).astype(np.float32) if scaled else np.ones(N, np.float32)
    assert 64 * K < 2 ** 24
    got = run_gemm(gpu_device, qa, sa, qw, sw, M, N, K)
    want = (a @ w.T) * sa.astype(np.float64)[:, None] * sw.astype(np.float64)[None, :]
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8], got[tuple(bad[0])], want[tuple(bad[0])])


def check_bound(name, got, ref, bound):
    ratio = np.abs(got - ref) / bound
    worst = float(ratio.max())
    print(f'[fp8] {name}: worst observed / bound = {worst:.4f} (mean {float(ratio.mean()):.4f})')
    record('fp8_gemm_bound_' + name, kind='ratio', worst=worst, mean=float(ratio.mean()))
    at = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert worst <= 1.0, (name, worst, at, got[at], ref[at], bound[at])


@pytest.mark.parametrize('N', [200, 203])
def test_gemm_fp8_gate_residual_in_place(gpu_device, N):
    """N = 200: the 16-byte epilogue; N = 203: the element-wise one (N % 4 != 0) with bias, gate and residual.  At N = 200 the same call with a bias pointer
    that is only 4-byte aligned takes the element-wise form and must give the same bits."""
    dev = gpu_device
    M, K, l = 300, 384, 50
    rng = np.random.default_rng(11)
    qa, qw = F.random_e4m3((M, K), rng), F.random_e4m3((N, K), rng)
    sa, sw = np.exp2(rng.integers(-12, -5, M)).astype(np.float32), np.exp2(rng.integers(-12, -5, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    G, ldg, goff = M // l, 3 * N + 4, N + 4
    gate = rng.standard_normal((G, ldg)).astype(np.float32)
    x0 = rng.standard_normal((M, N)).astype(np.float32)
    ap, wp = fenced(qa.shape, U8, dev, torch.from_numpy(qa)), fenced(qw.shape, U8, dev, torch.from_numpy(qw))
    sap, swp = fenced((M,), F32, dev, torch.from_numpy(sa)), fenced((N,), F32, dev, torch.from_numpy(sw))
    xp = fenced((M, N), F32, dev, torch.from_numpy(x0))
    gate_d = torch.from_numpy(gate).to(dev)
    ops.gemm_fp8(ap[1], sap[1], wp[1], swp[1], xp[1], M=M, N=N, K=K, bias=torch.from_numpy(bias).to(dev), gate=gate_d, gate_off=goff,
                 ldg=ldg, gate_rows=l, residual=xp[1])
    torch.cuda.synchronize()
    assert pads_intact(ap, wp, sap, swp, xp)
    got = xp[1].double().cpu().numpy()
    if N % 4 == 0:
        x2 = fenced((M, N), F32, dev, torch.from_numpy(x0))
        b_off = torch.zeros(N + 1, device=dev)
        b_off[1:] = torch.from_numpy(bias).to(dev)
        assert b_off[1:].data_ptr() % 16 == 4
        ops.gemm_fp8(ap[1], sap[1], wp[1], swp[1], x2[1], M=M, N=N, K=K, bias=b_off[1:], gate=gate_d, gate_off=goff, ldg=ldg, gate_rows=l, residual=x2[1])
        torch.cuda.synchronize()
        assert pads_intact(x2) and torch.equal(x2[1].view(torch.int32), xp[1].view(torch.int32))
    p = F.product_ref(qa, sa, qw, sw)
    g = gate[np.arange(M) // l, goff:goff + N].astype(np.float64)
    f = p + bias
    ref = x0 + g * f
    pb = F.product_bound(qa, sa, qw, sw)
    # bias add, gate multiply, residual add: one fp32 rounding each, on values bounded by the exact ones plus the error so far
    e1 = pb + U24 * (np.abs(f) + pb)
    e2 = np.abs(g) * e1 + U24 * (np.abs(g * f) + np.abs(g) * e1)
    bound = e2 + U24 * (np.abs(ref) + e2)
    check_bound(f'gate_residual_300x{N}x384', got, ref, bound)


@pytest.mark.parametrize('M,N,K', [(2085, 512, 1536), (130, 203, 256)])
def test_gemm_fp8_gelu_bf16_out(gpu_device, M, N, K):
    """(130, 203, 256): the element-wise epilogue (N % 4 != 0) with bias, GELU and the bf16 store"""
    rng = np.random.default_rng(12)
    qa, qw = F.random_e4m3((M, K), rng), F.random_e4m3((N, K), rng)
    sa, sw = np.exp2(rng.integers(-14, -9, M)).astype(np.float32), np.exp2(rng.integers(-14, -9, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    got = run_gemm(gpu_device, qa, sa, qw, sw, M, N, K, out_dtype=BF16, bias=torch.from_numpy(bias).to(gpu_device), act=ACT_GELU_TANH)
    t = F.product_ref(qa, sa, qw, sw) + bias
    pb = F.product_bound(qa, sa, qw, sw)
    e1 = pb + U24 * (np.abs(t) + pb)
    ref = F.gelu_tanh(t)
    e2 = F.gelu_bound(t, e1)
    bound = e2 + 2.0 ** -8 * (np.abs(ref) + e2) + 2.0 ** -134               # the bf16 store: half a step, i.e. 2^-8 of the binade's base at most; subnormal outputs on the bf16 grid
    assert M < 2000 or (float(np.abs(t).max()) > 3 and float(np.abs(t).min()) < 1e-2)      # the large case reaches both tails of the GELU and its middle
    check_bound(f'gelu_bf16_{M}x{N}x{K}', got, ref, bound)


def test_gemm_fp8_qkv_form(gpu_device):
    """remap + column split + split_alpha, the second layer of a stacked weight (byte offset) and of its scales.  The same call with the scale table moved by
    one element (w_scale only 4-byte aligned) takes the element-wise epilogue through remap and split and must give the same bits."""
    dev = gpu_device
    R, l, Lmax, C, q_off = 4, 9, 30, 128, 14
    M, N, K = R * l, 3 * C, C
    rng = np.random.default_rng(13)
    qa, qw = F.random_e4m3((M, K), rng), F.random_e4m3((2 * N, K), rng)
    sa, sw = np.exp2(rng.integers(-12, -5, M)).astype(np.float32), np.exp2(rng.integers(-12, -5, 2 * N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    alpha_q = 0.08838834764831845 * 1.4426950408889634
    ap, wp = fenced(qa.shape, U8, dev, torch.from_numpy(qa)), fenced(qw.shape, U8, dev, torch.from_numpy(qw))
    sap, swp = fenced((M,), F32, dev, torch.from_numpy(sa)), fenced((2 * N,), F32, dev, torch.from_numpy(sw))
    arena, qs = fenced((2, R, Lmax, 2 * C), BF16, dev), fenced((M, C), BF16, dev)
    stride = R * Lmax * 2 * C
    ops.gemm_fp8(ap[1], sap[1], wp[1], swp[1], arena[1], M=M, N=N, K=K, w_off=N * K, ws_off=N, bias=torch.from_numpy(bias).to(dev), c_off=stride, ldc=2 * C,
                 remap=(l, Lmax, q_off), split=(qs[1], C, C), split_alpha=alpha_q)
    torch.cuda.synchronize()
    assert pads_intact(ap, wp, sap, swp, arena, qs)
    sw1 = fenced((2 * N + 1,), F32, dev, torch.from_numpy(np.concatenate([[np.float32(3.0)], sw])))
    arena1, qs1 = fenced((2, R, Lmax, 2 * C), BF16, dev), fenced((M, C), BF16, dev)
    ops.gemm_fp8(ap[1], sap[1], wp[1], sw1[1], arena1[1], M=M, N=N, K=K, w_off=N * K, ws_off=N + 1, bias=torch.from_numpy(bias).to(dev), c_off=stride, ldc=2 * C,
                 remap=(l, Lmax, q_off), split=(qs1[1], C, C), split_alpha=alpha_q)
    torch.cuda.synchronize()
    assert pads_intact(sw1, arena1, qs1)
    assert torch.equal(qs1[1].view(torch.int16), qs[1].view(torch.int16)) and torch.equal(arena1[1].view(torch.int16), arena[1].view(torch.int16))
    f = F.product_ref(qa, sa, qw[N:], sw[N:]) + bias
    pb = F.product_bound(qa, sa, qw[N:], sw[N:])
    e1 = pb + U24 * (np.abs(f) + pb)
    aq = float(np.float32(alpha_q))
    ref_q = f[:, :C] * aq
    eq = aq * e1[:, :C] + U24 * (np.abs(ref_q) + aq * e1[:, :C])
    bq = eq + 2.0 ** -8 * (np.abs(ref_q) + eq)
    check_bound('qkv_q', qs[1].double().cpu().numpy(), ref_q, bq)
    ar = arena[1].float().cpu().numpy()
    assert np.isnan(ar[0]).all()                                              # layer 0 of the arena is not this call's
    got_kv = ar[1][:, q_off:q_off + l].reshape(M, 2 * C).astype(np.float64)
    bkv = e1[:, C:] + 2.0 ** -8 * (np.abs(f[:, C:]) + e1[:, C:])
    check_bound('qkv_kv', got_kv, f[:, C:], bkv)
    rest = np.ones(Lmax, bool)
    rest[q_off:q_off + l] = False
    assert np.isnan(ar[1][:, rest]).all()                                     # rows of other scales untouched


def test_gemm_fp8_rows_do_not_depend_on_m_or_the_tile(gpu_device):
    """the same activation rows inside M = 40 (128x128 tile) and M = 1100 (256x256 tile): the same bits"""
    N, K = 520, 768
    rng = np.random.default_rng(14)
    qa, qw = F.random_e4m3((1100, K), rng), F.random_e4m3((N, K), rng)
    sa, sw = np.exp2(rng.integers(-8, 0, 1100)).astype(np.float32), np.exp2(rng.integers(-8, 0, N)).astype(np.float32)
    big = run_gemm(gpu_device, qa, sa, qw, sw, 1100, N, K)
    small = run_gemm(gpu_device, qa[700:740].copy(), sa[700:740].copy(), qw, sw, 40, N, K)
    assert np.array_equal(big[700:740], small)


def test_gemm_fp8_refusals_write_nothing(gpu_device):
    dev = gpu_device
    M, N, K = 8, 16, 128
    a, w = torch.zeros(M, K + 16, device=dev, dtype=U8), torch.zeros(N, K + 16, device=dev, dtype=U8)
    sa, sw = torch.ones(M, device=dev), torch.ones(N, device=dev)
    cp = fenced((M, N), F32, dev)
    other = torch.zeros(M, N, device=dev)

    def refused(status_word, hook=None, **kw):
        args = dict(M=M, N=N, K=K, lda=K + 16, ldw=K + 16)
        args.update(kw)
        with pytest.raises(CvarError, match=status_word):
            ops.gemm_fp8(a, sa, w, sw, cp[1], desc_hook=hook, **args)

    def setter(**fields):
        def hook(d):
            for k, v in fields.items():
                setattr(d, k, v)
        return hook

    p = other.data_ptr()
    for fields in (dict(conv=1), dict(batch=2), dict(ws=p, ws_bytes=other.numel() * 4), dict(ln_out=p), dict(gn_part=p), dict(pre_act=p), dict(aux=p), dict(act=2),
                   dict(gate_scale=p)):
        refused('unsupported', setter(**fields))
    refused('unsupported', K=96)
    refused('unsupported', lda=K + 8)
    refused('unsupported', ldw=K + 8)
    refused('unsupported', lda=64)                                            # lda < K
    refused('invalid', a_off=8)                                               # A not 16-byte aligned
    refused('invalid', setter(split_n=N, C_split=p, ld_split=N))              # split_n >= N
    refused('unsupported', setter(split_n=8, C_split=p, ld_split=8))          # a column split without a row remap
    refused('invalid', gate=other, gate_rows=0, ldg=N)
    with pytest.raises(TypeError):
        ops.gemm_fp8(a.view(torch.int8), sa, w, sw, cp[1], M=M, N=N, K=K)
    # the row passes
    q, s = fenced((M, 128), U8, dev), fenced((M,), F32, dev)
    x = torch.zeros(M, 200, device=dev)
    with pytest.raises(CvarError, match='unsupported'):
        ops.quant_rows_fp8(x, q[1], s[1], M=M, K=128, ldx=200, ldq=64)
    with pytest.raises(CvarError, match='unsupported'):
        ops.quant_rows_fp8(x, q[1], s[1], M=M, K=200, ldx=200, ldq=128)
    with pytest.raises(CvarError, match='unsupported'):
        ops.ln_modulate_fp8(x, x, 0, 0, 200, 1, q[1], s[1], M, 128, EPS, ldq=64)
    with pytest.raises(CvarError, match='unsupported'):
        ops.ln_modulate_fp8(x, x, 0, 2, 200, 1, q[1], s[1], M, 128, EPS, ldq=128)          # scale pointer off 16-byte alignment
    torch.cuda.synchronize()
    assert pads_intact(cp, q, s) and bool(torch.isnan(cp[1]).all()) and bool((q[1] == 0xA5).all()) and bool(torch.isnan(s[1]).all())
