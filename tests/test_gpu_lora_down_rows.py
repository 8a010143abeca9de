"""cvar_lora_down_rows (csrc/lora.hip, include/cvar_serve.h): the per-row form of cvar_lora_down that per-request adapters run.

With R sequences of l rows, row m uses slot[m // l].  Every case lives between NaN fences in NaN-prefilled buffers and checks
* the slot's 16 columns: bit for bit what ops.lora_down(p = 0, r = 16, scale[s]) writes for that row's sequence alone with A_bank[s], and
  within the rounding bound of tests/test_gpu_lora_kernels.py::test_down_random_values_with_rounding_bounds of a float64 product;
* every other owned column: exactly +0, rows of slot -1 entirely;
* the copy: x bit for bit; everything else - fences, columns behind the owned ones, columns < K of a call without x_copy: unchanged.
The shapes are the smallest at which the kernel takes another path: l below / at / above the 16-row chunk and many chunks, K below one
512-column slab, not a multiple of 64 lanes x 8, two slabs and eight, 1 / 3 / 8 slots, kpad tight and rounded up to the 128-byte step."""
import pytest
import torch

from controlvar_amd import ops
from controlvar_amd._lib import CvarError

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
U = 2.0 ** -24                      # fp32 unit roundoff
R = 5
RANKS = (16, 5, 1)
PAD = 64


def bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def arena(rows, ld, dtype, dev):
    buf = torch.full((2 * PAD + rows * ld,), float('nan'), dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + rows * ld].view(rows, ld)


def slots_of(n):
    """-1, a repeated slot and the last slot"""
    return [n - 1, -1, 0, n - 1, n // 2]


def bank(n, K, dtype, dev, gen, integer=False):
    """(A_bank (n, 16, K) with rows >= the rank zero, scale (n,) fp32 = 32 / r)"""
    A = torch.zeros(n, 16, K)
    for k in range(n):
        r = RANKS[k % 3]
        A[k, :r] = torch.randint(-2, 3, (r, K), generator=gen).float() if integer else (torch.rand(r, K, generator=gen) * 2 - 1) / K ** 0.5
    scale = torch.tensor([2.0 if integer else 32.0 / RANKS[k % 3] for k in range(n)], dtype=F32)
    return A.to(dtype).to(dev), scale.to(dev)


def kpads(n, dtype):
    rp = 128 // (2 if dtype == BF16 else 4)
    return sorted({16 * n, -(-16 * n // rp) * rp})


def run_case(dev, dtype, l, K, n, kpad, gen, integer=False):
    M = R * l
    slots = slots_of(n)
    A, scale = bank(n, K, dtype, dev, gen, integer)
    slot = torch.tensor(slots, dtype=torch.int32, device=dev)
    ldx, ldxa = K + 8, K + kpad + 8
    xb, x = arena(M, ldx, dtype, dev)
    x[:, :K] = (torch.randint(-2, 3, (M, K), generator=gen).float() if integer else torch.randn(M, K, generator=gen)).to(dtype).to(dev)
    x0 = xb.clone()
    # reference: every sequence alone through cvar_lora_down with its own adapter (r = 16: the bank's zero rows give zero columns)
    want = torch.zeros(M, kpad, dtype=dtype, device=dev)
    for s, k in enumerate(slots):
        if k < 0:
            continue
        u = torch.full((l, 16), float('nan'), dtype=dtype, device=dev)
        ops.lora_down(x[s * l:(s + 1) * l], A[k], u, M=l, K=K, r=16, scale=float(scale[k]), ldx=ldx)
        want[s * l:(s + 1) * l, 16 * k:16 * k + 16] = u
    # float64 product and its rounding bound
    xd = x[:, :K].double()
    for s, k in enumerate(slots):
        if k < 0:
            continue
        rows = slice(s * l, (s + 1) * l)
        sc = float(scale[k])
        ref = sc * xd[rows] @ A[k].double().t()
        got = want[rows, 16 * k:16 * k + 16].double()
        if integer:
            assert (ref.abs() < 2 ** 24).all()
            assert torch.equal(got, ref.to(F32).to(dtype).double()), (l, K, n, k)
        else:
            bound = (K + 2) * U * sc * xd[rows].abs() @ A[k].double().abs().t()
            if dtype == BF16:
                bound = bound + ref.abs() * 2.0 ** -8
            assert ((got - ref).abs() <= bound + 1e-30).all(), (l, K, n, k, float((got - ref).abs().max()))
    # form 1: a separate x, the copy goes into the wide buffer
    ab, xa = arena(M, ldxa, dtype, dev)
    ops.lora_down_rows(x, A, scale, slot, xa, R=R, l=l, K=K, kpad=kpad, ldx=ldx, ldxa=ldxa, x_copy=xa, ld_copy=ldxa)
    expect = torch.full_like(ab, float('nan'))
    ev = expect[PAD:PAD + M * ldxa].view(M, ldxa)
    ev[:, :K] = x[:, :K]
    ev[:, K:K + kpad] = want
    assert same_bits(ab, expect), (l, K, n, kpad, 'copy form')            # values, +0 elsewhere, the copy, fences and the 8 columns behind
    assert same_bits(xb, x0)
    # form 2: the producer wrote the wide buffer itself (fc2): in place, no copy, columns < K untouched
    ab2, xa2 = arena(M, ldxa, dtype, dev)
    xa2[:, :K] = x[:, :K]
    expect2 = ab2.clone()
    expect2[PAD:PAD + M * ldxa].view(M, ldxa)[:, K:K + kpad] = want
    ops.lora_down_rows(xa2, A, scale, slot, xa2, R=R, l=l, K=K, kpad=kpad, ldx=ldxa, ldxa=ldxa)
    assert same_bits(ab2, expect2), (l, K, n, kpad, 'in-place form')


@pytest.mark.parametrize('dtype', [BF16, F32])
@pytest.mark.parametrize('K', [128, 320, 1024, 4096])
@pytest.mark.parametrize('l', [1, 3, 16, 17, 200])
def test_rows_equal_lora_down_of_their_own_adapter(gpu_device, l, K, dtype):
    gen = torch.Generator().manual_seed(1000 * l + K)
    for n in (1, 3, 8):
        for kpad in kpads(n, dtype):
            run_case(gpu_device, dtype, l, K, n, kpad, gen)


@pytest.mark.parametrize('dtype', [BF16, F32])
def test_integer_data_is_exact(gpu_device, dtype):
    """inputs in [-2, 2] and scale 2 keep every partial sum an integer below 2^24: the result is the float64 product, rounded once"""
    gen = torch.Generator().manual_seed(5)
    run_case(gpu_device, dtype, 17, 1024, 3, 64, gen, integer=True)


def test_rejected_arguments_leave_the_device_usable(gpu_device):
    dev = gpu_device
    gen = torch.Generator().manual_seed(9)
    l, K, n, kpad = 3, 128, 3, 48
    A, scale = bank(n, K, BF16, dev, gen)
    slot = torch.tensor(slots_of(n), dtype=torch.int32, device=dev)
    x = torch.randn(R * l, K, generator=gen).to(BF16).to(dev)
    xa = torch.full((R * l, K + kpad), float('nan'), dtype=BF16, device=dev)

    def call(x=x, A=A, scale=scale, slot=slot, xa=xa, **kw):
        args = dict(R=R, l=l, K=K, kpad=kpad)
        args.update(kw)
        ops.lora_down_rows(x, A, scale, slot, xa, **args)

    A9, scale9 = bank(9, K, BF16, dev, gen)
    for bad in (dict(A=A9, scale=scale9), dict(l=0), dict(R=0, slot=slot[:0]), dict(kpad=40), dict(kpad=32), dict(scale=None), dict(slot=None)):
        with pytest.raises(CvarError, match='invalid'):
            call(**bad)
    for bad in (dict(K=124), dict(ldxa=K + kpad - 8), dict(ldx=K - 8), dict(ldx=K + 4), dict(x=x.view(-1)[1:]), dict(x_copy=xa, ld_copy=K - 8)):
        with pytest.raises(CvarError, match='unsupported'):
            call(**bad)
    with pytest.raises(TypeError, match='share a dtype'):
        call(A=A.float())
    with pytest.raises(ValueError, match='slot'):
        call(slot=slot.long())
    with pytest.raises(ValueError, match='scale'):
        call(scale=scale[:2])
    torch.cuda.synchronize()
    assert bool(torch.isnan(xa).all())                  # no refused call launched anything
    call()
    torch.cuda.synchronize()
    assert not bool(torch.isnan(xa[:, K:]).any()) and bool(torch.isnan(xa[:, :K]).all())         # no x_copy: the owned columns only
