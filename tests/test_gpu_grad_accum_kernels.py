"""The accumulating forms of the gradient producers (include/cvar_accum.h) on MI355X.

The contract is exact: with the flag set every output element is fp32(old + plain), `plain` being what the non-accumulating call writes for the
same operands - one IEEE add, performed last.  So every check here is torch.equal against `old + plain` formed by torch from the plain call's
own output; no tolerance.  Operands are random, `old` is a random non-zero fp32 tensor and every output region sits between NaN fences."""
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float('nan')


def _fenced(n_inner, lead, tail, dev):
    buf = torch.full((lead + n_inner + tail,), NAN, device=dev)
    return buf, buf[lead:lead + n_inner]


# ------------------------------------------------------------------------------------------------------------------ cvar_gemm_tn_acc
# T = 40: one K step and a zero-filled partial one, one slice.  T = 2720 without the workspace: 85 K steps in ONE slice (the accumulator epilogue
# loads C).  T = 2720 with it: >= 24 K steps per slice -> three slices for these one- and two-tile problems (the reduction adds C last).
# (Nn, Kk): (128, 128) the 128-row tile with a half-filled last column tile; (256, 384) the 256-row tile, a full column tile and a half-filled
# one; (512, 128) two 256-row tiles
@pytest.mark.parametrize('T,use_ws', [(40, True), (2720, False), (2720, True)])
@pytest.mark.parametrize('Nn,Kk', [(128, 128), (256, 384), (512, 128)])
def test_gemm_tn_accumulating_is_old_plus_plain(gpu_device, T, use_ws, Nn, Kk):
    from controlvar_amd import ops
    g = torch.Generator().manual_seed(T + Nn + Kk)
    A = torch.randn(T, Nn, generator=g).to(torch.bfloat16).to(gpu_device)
    B = torch.randn(T, Kk, generator=g).to(torch.bfloat16).to(gpu_device)
    ldc, c_off, cs_off = Kk + 8, 24, 36                   # ldc > Kk: eight fence columns behind every row; the window starts inside the buffer
    old = (torch.randn(Nn, Kk, generator=g) * 3 + 0.5).to(gpu_device)
    old_cs = (torch.randn(Nn, generator=g) * 3 + 0.5).to(gpu_device)
    assert (old != 0).all() and (old_cs != 0).all()

    def buffers():
        buf = torch.full((c_off + Nn * ldc + 64,), NAN, device=gpu_device)
        cs = torch.full((cs_off + Nn + 64,), NAN, device=gpu_device)
        return buf, cs

    def window(buf):
        return buf[c_off:c_off + Nn * ldc].view(Nn, ldc)[:, :Kk]

    def fences_intact(buf, cs):
        m = torch.ones_like(buf, dtype=torch.bool)
        window(m).fill_(False)
        return bool(torch.isnan(buf[m]).all()) and bool(torch.isnan(cs[:cs_off]).all()) and bool(torch.isnan(cs[cs_off + Nn:]).all())

    def run(buf, cs, accumulate):
        ops.gemm_tn(A, B, buf, T=T, Nn=Nn, Kk=Kk, ldc=ldc, c_off=c_off, colsum=cs, colsum_off=cs_off, accumulate=accumulate, use_ws=use_ws)

    pbuf, pcs = buffers()
    run(pbuf, pcs, False)
    plain, plain_cs = window(pbuf).clone(), pcs[cs_off:cs_off + Nn].clone()
    assert torch.isfinite(plain).all() and torch.isfinite(plain_cs).all() and fences_intact(pbuf, pcs)

    buf, cs = buffers()
    window(buf).copy_(old); cs[cs_off:cs_off + Nn] = old_cs
    run(buf, cs, True)
    assert torch.equal(window(buf), old + plain)
    assert torch.equal(cs[cs_off:cs_off + Nn], old_cs + plain_cs)
    assert fences_intact(buf, cs)
    run(buf, cs, True)                                    # a third micro-batch: (old + plain) + plain, in that order
    assert torch.equal(window(buf), (old + plain) + plain)
    assert torch.equal(cs[cs_off:cs_off + Nn], (old_cs + plain_cs) + plain_cs)
    run(buf, cs, False)                                   # the flag leaves no state behind
    assert torch.equal(window(buf), plain) and torch.equal(cs[cs_off:cs_off + Nn], plain_cs)
    assert fences_intact(buf, cs)

    nbuf, ncs = buffers()                                 # without the column sums
    window(nbuf).copy_(old)
    ops.gemm_tn(A, B, nbuf, T=T, Nn=Nn, Kk=Kk, ldc=ldc, c_off=c_off, accumulate=True, use_ws=use_ws)
    assert torch.equal(window(nbuf), old + plain) and fences_intact(nbuf, ncs)


def test_gemm_tn_accumulating_entry_point_with_the_flag_off_is_the_plain_call(gpu_device):
    """cvar_gemm_tn_acc(accumulate = 0) overwrites, bit for bit as cvar_gemm_tn"""
    from controlvar_amd import _lib, ops
    T, Nn, Kk = 2720, 256, 384
    g = torch.Generator().manual_seed(1)
    A = torch.randn(T, Nn, generator=g).to(torch.bfloat16).to(gpu_device)
    B = torch.randn(T, Kk, generator=g).to(torch.bfloat16).to(gpu_device)
    plain = torch.empty(Nn, Kk, device=gpu_device)
    ops.gemm_tn(A, B, plain, T=T, Nn=Nn, Kk=Kk)
    out = torch.randn(Nn, Kk, generator=g).to(gpu_device)
    ws = ops.ensure_splitk_workspace(gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().cvar_gemm_tn_acc(A.data_ptr(), Nn, B.data_ptr(), Kk, out.data_ptr(), Kk, T, Nn, Kk, ws.data_ptr(), ws.numel(), None, 0, st), 'acc')
    assert torch.equal(out, plain)


# ------------------------------------------------------------------------------------------------------------------ cvar_lora_wgrad_acc
@pytest.mark.parametrize('M', [1360, 2720])
@pytest.mark.parametrize('form', ['dB', 'dA'])
def test_lora_wgrad_accumulating_is_old_plus_plain(gpu_device, M, form):
    """both output stride forms of the engine: dB = dY^T u as an [N][r] matrix, dA = s du^T drop(x) as [r][N] (os_n = 1, os_j = N) with dropout on"""
    from controlvar_amd import ops
    N, r = 512, 16
    g = torch.Generator().manual_seed(M + len(form))
    Y = torch.randn(M, N, generator=g).to(torch.bfloat16).to(gpu_device)
    Z = torch.randn(M, 16, generator=g).to(torch.bfloat16).to(gpu_device)
    kw = dict(M=M, N=N, r=r) if form == 'dB' else dict(M=M, N=N, r=r, scale=0.5, p=0.1, seed=7, tag=3, os_n=1, os_j=N)
    ws = torch.empty(ops.lora_wgrad_ws_floats(M, N), device=gpu_device)
    lead = 20
    old = (torch.randn(N * r, generator=g) * 2 + 0.25).to(gpu_device)
    pbuf, pwin = _fenced(N * r, lead, 40, gpu_device)
    ops.lora_wgrad(Y, Z, pbuf, ws, out_off=lead, **kw)
    plain = pwin.clone()
    assert torch.isfinite(plain).all() and plain.abs().max() > 0
    buf, win = _fenced(N * r, lead, 40, gpu_device)
    win.copy_(old)
    ops.lora_wgrad(Y, Z, buf, ws, out_off=lead, accumulate=True, **kw)
    assert torch.equal(win, old + plain)
    assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + N * r:]).all()
    ops.lora_wgrad(Y, Z, buf, ws, out_off=lead, **kw)
    assert torch.equal(win, plain)


# ------------------------------------------------------------------------------------------------------------------ cvar_wordembed_grad_acc
@pytest.mark.parametrize('B,n,rows,skip,C', [(3, 50, 52, 2, 128),           # one token slice
                                             (4, 100, 102, 2, 192)])        # four slices, summed in order, the old value last
def test_wordembed_grad_accumulating_is_old_plus_plain(gpu_device, B, n, rows, skip, C):
    from controlvar_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + n)
    dx = torch.randn(B, rows, C, generator=g)
    dx[:, :skip] = NAN
    dx = dx.to(gpu_device).view(B * rows, C)
    tok = torch.randn(B * n, 32, generator=g).to(gpu_device)
    lead, inner = 8, C * 33
    old = (torch.randn(inner, generator=g) + 0.125).to(gpu_device)
    pbuf, pwin = _fenced(inner, lead, 16, gpu_device)
    ops.wordembed_grad(dx, C, rows, skip, tok, n, B, C, 32, pbuf, lead, lead + C * 32)
    plain = pwin.clone()
    assert torch.isfinite(plain).all()
    buf, win = _fenced(inner, lead, 16, gpu_device)
    win.copy_(old)
    ops.wordembed_grad(dx, C, rows, skip, tok, n, B, C, 32, buf, lead, lead + C * 32, accumulate=True)
    assert torch.equal(win, old + plain)
    assert torch.isnan(buf[:lead]).all() and torch.isnan(buf[lead + inner:]).all()
    ops.wordembed_grad(dx, C, rows, skip, tok, n, B, C, 32, buf, lead, lead + C * 32)
    assert torch.equal(win, plain)


# ------------------------------------------------------------------------------------------------------------------ cvar_add_inplace
@pytest.mark.parametrize('n,y_off,x_off', [(1, 8, 8), (1027, 8, 12),          # 16-byte aligned: vector body + a scalar tail
                                           (1027, 9, 8), (5, 8, 3),           # either side off the 16-byte grid: the scalar form
                                           (4 * 256 * 4096 + 4 * 700 + 2, 8, 8)])  # more vectors than one pass of the largest grid holds: the stride loop
def test_add_inplace(gpu_device, n, y_off, x_off):
    from controlvar_amd import ops
    g = torch.Generator().manual_seed(n)
    old = torch.randn(n, generator=g).to(gpu_device)
    inc = torch.randn(n, generator=g).to(gpu_device)
    ybuf = torch.full((y_off + n + 32,), NAN, device=gpu_device)
    xbuf = torch.full((x_off + n + 32,), NAN, device=gpu_device)
    ybuf[y_off:y_off + n] = old; xbuf[x_off:x_off + n] = inc
    ops.add_inplace(ybuf, xbuf, n, y_off=y_off, x_off=x_off)
    assert torch.equal(ybuf[y_off:y_off + n], old + inc)
    assert torch.equal(xbuf[x_off:x_off + n], inc)
    assert torch.isnan(ybuf[:y_off]).all() and torch.isnan(ybuf[y_off + n:]).all()
    with pytest.raises(ValueError):
        ops.add_inplace(ybuf, xbuf, n + 64, y_off=y_off, x_off=x_off)        # past the end of the tensors: refused on the host
