"""The two kernel-level promises of gemm_precision='bf16x3' on MI355X (include/cvar_serve.h).

cvar_ln_modulate_split3 is DEFINED as cvar_split3(cvar_ln_modulate(..., fp32 out)) in one pass: every case compares the bits of the two, between NaN
fences, over every NV / TAIL instantiation family the model widths reach (C = 128: NV 1, 1000: NV 4 with a tail, 1536: NV 6, 1920: NV 8 with a tail,
2048: NV 8), one and several row groups per modulation row, one block and more than one (M = 1 / 5 / 9 at four rows per block).

The split product through ops.gemm - activation rows [hi | lo | hi], weight rows [w_hi | w_hi | w_lo], one bf16 GEMM over 3 K, fp32 output - is held
against a float64 matmul of the fp32 operands at the bound tests/x3_ref.py derives term by term (representation 2 * 2^-17, dropped product 2^-16, fp32
accumulation at the tile kernels' depth, all times sum |a| |w|, plus the epilogue's roundings).  The same call on plain bf16 operands must land outside
that bound: the test tells the modes apart."""
import numpy as np
import pytest
import torch

import x3_ref as X
from conftest import record

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402
from controlvar_amd._lib import ACT_GELU_TANH, CvarError  # noqa: E402
from controlvar_amd import _lib  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
EPS = 1e-6
PAD = 4096


def fenced(shape, dtype, dev, value=None):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float('nan'), device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(torch.as_tensor(value).to(dtype))
    return buf, view


def pads_intact(*pairs):
    for buf, view in pairs:
        if not (bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[PAD + view.numel():]).all())):
            return False
    return True


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


# ================================================================================================ ln_modulate_split3
def ln_inputs(C, M, rp, seed):
    g = torch.Generator().manual_seed(seed)
    G = (M + rp - 1) // rp
    x = torch.randn(M, C, generator=g) * 3 + torch.randn(M, 1, generator=g)
    x[0, 0] = 1e4                                            # one outlier: the row statistics matter
    ld = 6 * C + 8                                           # a non-trivial ld_ada: scale at column 2 C + 4, shift at 4 C + 8 of a wider table
    ada = torch.randn(G, ld, generator=g) * 0.5
    return x, ada, ld


@pytest.mark.parametrize('rp', [1, 3])
@pytest.mark.parametrize('M', [1, 5, 9])
@pytest.mark.parametrize('C', [128, 1000, 1536, 1920, 2048])
def test_ln_modulate_split3_equals_split3_of_ln_modulate(gpu_device, C, M, rp):
    dev = gpu_device
    x, ada, ld = ln_inputs(C, M, rp, 1000 * C + 10 * M + rp)
    xp, ap = fenced((M, C), F32, dev, x), fenced(tuple(ada.shape), F32, dev, ada)
    yp, sp, op = fenced((M, C), F32, dev), fenced((M, 3 * C), BF16, dev), fenced((M, 3 * C), BF16, dev)
    so, sh = 2 * C + 4, 4 * C + 8
    ops.ln_modulate(xp[1], ap[1], so, sh, ld, rp, yp[1], M, C, EPS)
    ops.split3(yp[1], sp[1], M, C)
    ops.ln_modulate_split3(xp[1], ap[1], so, sh, ld, rp, op[1], M, C, EPS)
    torch.cuda.synchronize()
    assert pads_intact(xp, ap, yp, sp, op)
    assert not bool(torch.isnan(op[1].float()).any())
    assert torch.equal(bits(op[1]), bits(sp[1]))
    # and the two-pass form is what the host restatement says it is: [hi | lo | hi] of the fp32 row
    want = torch.from_numpy(X.activation_rows(yp[1].cpu().numpy()).view(np.int16))
    assert torch.equal(bits(op[1]).cpu(), want)


def test_the_torch_op_gives_the_same_rows(gpu_device):
    """torch.ops.cvar.ln_modulate_split3 (broadcast modulation rows, any leading shape) against the pointer-level call"""
    import controlvar_amd
    ns = controlvar_amd.register_torch_ops()
    C, R, l = 1000, 3, 5
    x, ada, ld = ln_inputs(C, R * l, l, 17)
    x, ada = x.to(gpu_device), ada.to(gpu_device)
    so, sh = 2 * C + 4, 4 * C + 8
    want = torch.empty(R * l, 3 * C, device=gpu_device, dtype=BF16)
    ops.ln_modulate_split3(x, ada, so, sh, ld, l, want, R * l, C, EPS)
    got = ns.ln_modulate_split3(x.view(R, l, C), ada[:, so:so + C], ada[:, sh:sh + C], l, EPS)
    assert got.shape == (R, l, 3 * C) and torch.equal(bits(got.reshape(R * l, 3 * C)), bits(want))


def test_ln_modulate_split3_constant_rows_give_the_split_of_the_shift(gpu_device):
    """a constant row whose fp32 mean is exact normalises to 0: y = shift, so the output is exactly the split of the shift"""
    dev = gpu_device
    for C in (128, 1000, 2048):
        M, rp = 6, 2
        x = torch.tensor([1.5, 2.25, -4.0, 0.0, 8.0, -0.5]).reshape(M, 1).repeat(1, C)
        g = torch.Generator().manual_seed(C)
        ada = torch.randn(3, 2 * C, generator=g)
        xp, ap, op = fenced((M, C), F32, dev, x), fenced((3, 2 * C), F32, dev, ada), fenced((M, 3 * C), BF16, dev)
        ops.ln_modulate_split3(xp[1], ap[1], 0, C, 2 * C, rp, op[1], M, C, EPS)
        torch.cuda.synchronize()
        assert pads_intact(xp, ap, op)
        want = X.activation_rows(ada[:, C:].numpy())
        got = bits(op[1]).cpu().numpy().view(np.uint16)
        for m in range(M):
            assert np.array_equal(got[m], want[m // rp]), (C, m)


def test_ln_modulate_split3_refuses_without_writing(gpu_device):
    """C % 4, C > 2048 and ld_ada % 4 are CVAR_EUNSUPPORTED (-2), a NULL pointer CVAR_EINVAL (-1), before any launch"""
    dev = gpu_device
    for C, ld in ((130, 260), (2052, 4104), (128, 258)):
        xp, ap, op = fenced((3, C), F32, dev, torch.ones(3, C)), fenced((3, ld), F32, dev, torch.zeros(3, ld)), fenced((3, 3 * C), BF16, dev)
        with pytest.raises(CvarError, match=r'\(-2\)'):
            ops.ln_modulate_split3(xp[1], ap[1], 0, C, ld, 1, op[1], 3, C, EPS)
        torch.cuda.synchronize()
        assert bool(torch.isnan(op[0]).all())
    C = 128
    xp, ap, op = fenced((3, C), F32, dev, torch.ones(3, C)), fenced((3, 2 * C), F32, dev, torch.zeros(3, 2 * C)), fenced((3, 3 * C), BF16, dev)
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    ptrs = [xp[1].data_ptr(), ap[1].data_ptr(), ap[1].data_ptr() + 4 * C, op[1].data_ptr()]
    for null in range(4):
        a = list(ptrs)
        a[null] = None
        assert lib.cvar_ln_modulate_split3(a[0], a[1], a[2], 2 * C, 1, a[3], 3, C, EPS, st) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(op[0]).all())


# ================================================================================================ the split product through ops.gemm
CASES = {
    'skinny_plain': dict(shape=(5, 256, 128), epi='plain'),
    'odd_gate_residual': dict(shape=(300, 200, 96), epi='gate'),
    'tiles_gelu': dict(shape=(2085, 512, 1536), epi='gelu'),
    'long_k': dict(shape=(512, 256, 6144), epi='plain'),
}
_REF = {}


def case_data(name):
    """operands, the float64 reference and the bound of one case, computed once"""
    if name in _REF:
        return _REF[name]
    M, N, K = CASES[name]['shape']
    epi = CASES[name]['epi']
    a, w = X.operands(M, N, K, seed=sum(map(ord, name)))
    rng = np.random.default_rng(7)
    bias = rng.standard_normal(N).astype(np.float32) if epi != 'plain' else None
    l = 100
    gate = (rng.standard_normal(((M + l - 1) // l, N)) * 0.5).astype(np.float32) if epi == 'gate' else None
    res = (rng.standard_normal((M, N)) * 4).astype(np.float32) if epi == 'gate' else None
    y = a.astype(np.float64) @ w.astype(np.float64).T
    U = X.U24
    if epi == 'plain':
        ref, ep = y, 0.0
    elif epi == 'gate':
        t = y + bias
        ref = t * np.repeat(gate, l, axis=0)[:M] + res
        g = np.abs(np.repeat(gate, l, axis=0)[:M].astype(np.float64))
        # the product error passes through the gate: scale the product bound by |gate| (done below); roundings: bias add, gate multiply, residual add
        ep = U * (np.abs(t) * g + np.abs(t) * g + np.abs(ref))
    else:
        t = y + bias
        ref = X.gelu_tanh(t)
        # |gelu'| <= 1.13: the product error and the bias-add rounding (U |t|) pass through it.  The GELU itself is t * sigma(z), z = 1.5958 (t + 0.044715 t^3):
        # z carries 4 roundings, and sigma(1 - sigma) |z| <= 0.23, so sigma moves by <= 0.92 U from them, 0.25 U from the 1-ulp exponential and 2 U sigma from
        # the add and the reciprocal / quotient - under 4 U in all, times |t|; the last multiply rounds the result once (8 U |result| taken)
        ep = 1.13 * U * np.abs(t) + 4 * U * np.abs(t) + 8 * U * np.abs(ref)
    bd = X.product_bound(a, w)
    if epi == 'gate':
        bd = bd * g
    if epi == 'gelu':
        bd = bd * 1.13
    # the numpy model of the arithmetic (the product alone: the epilogue is float64 on the host) against the product's own bound
    model_ratio = float((np.abs(X.split_product_model(a, w).astype(np.float64) - y) / X.product_bound(a, w)).max())
    _REF[name] = dict(a=a, w=w, bias=bias, gate=gate, res=res, l=l, ref=ref, bound=bd + ep, model_ratio=model_ratio)
    return _REF[name]


def run_gemm(dev, d, name, A, W, K_call, **kw):
    M, N, K = CASES[name]['shape']
    epi = CASES[name]['epi']
    out = torch.empty(M, N, device=dev, dtype=F32)
    args = dict(M=M, N=N, K=K_call, **kw)
    if d['bias'] is not None:
        args['bias'] = torch.from_numpy(d['bias']).to(dev)
    if epi == 'gate':
        out.copy_(torch.from_numpy(d['res']))
        args.update(gate=torch.from_numpy(d['gate']).to(dev), ldg=N, gate_rows=d['l'], residual=out)
    if epi == 'gelu':
        args['act'] = ACT_GELU_TANH
    ops.gemm(A, W, out, **args)
    torch.cuda.synchronize()
    return out.cpu().double().numpy()


@pytest.mark.parametrize('small_m', [False, True], ids=['tiles', 'small_m_plans'])
@pytest.mark.parametrize('name', list(CASES))
def test_split_product_through_gemm_against_float64(gpu_device, name, small_m):
    dev = gpu_device
    d = case_data(name)
    M, N, K = CASES[name]['shape']
    a, w = torch.from_numpy(d['a']).to(dev), torch.from_numpy(d['w']).to(dev)
    A3 = torch.empty(M, 3 * K, device=dev, dtype=BF16)
    ops.split3(a, A3, M, K)
    W3 = torch.from_numpy(X.weight_rows(d['w']).view(np.int16)).to(dev).view(BF16)
    got = run_gemm(dev, d, name, A3, W3, 3 * K, small_m=small_m, split_k=small_m)
    ratio = float((np.abs(got - d['ref']) / d['bound']).max())
    model_ratio = d['model_ratio']
    plain = run_gemm(dev, d, name, a.to(BF16), w.to(BF16), K, small_m=small_m, split_k=small_m)
    plain_ratio = float((np.abs(plain - d['ref']) / d['bound']).max())
    print(f'[x3] gemm {name} small_m={small_m}: split {ratio:.3f}  numpy model {model_ratio:.3f}  plain bf16 {plain_ratio:.1f}  (of the bound)')
    record(f'x3 gemm {name}', kind='x3_gemm', small_m=bool(small_m), ratio=ratio, model_ratio=model_ratio, plain_bf16_ratio=plain_ratio)
    assert np.isfinite(got).all()
    assert ratio <= 1.0
    assert model_ratio <= 1.0
    assert plain_ratio > 1.0
