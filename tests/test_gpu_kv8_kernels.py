"""The two kernels of kv_precision='fp8' on MI355X (include/cvar_kvcache.h).

Append (cvar_kv_append_fp8): bytes and scales equal the numpy restatement of the per-head rule (tests/test_kv8_host.py: quant_heads, built on tests/fp8_ref.py)
bit for bit, and nothing but the rows (r, q_off + t) of the arena and of the scale table changes.

Attention (cvar_attention_kv8): an e4m3 byte times a power-of-two scale IS a bf16 value (test_kv8_host.py checks every code and every exponent), so the kernel
must give, bit for bit, what cvar_attention_prescaled gives on a bf16 arena that holds byte * scale - output and lse, torch.equal.  The issue's six cases use
R = 2, H = 3.  The launch rule (launch_attn_mfma / attn_two_groups in csrc/attn.hip) takes two query groups per wave, G = 2, only where
l >= 192, the last 256-query block misses fewer than 64 queries AND cdiv(l, 256) * H * R >= 512 - which R * H = 6 never reaches, and l = 338 never does at any
R.  The cases below therefore keep the issue's six shapes as stated (they run G = 1) and add shapes that DO reach G = 2: l = 256 at 516 and 512 (row, head)
pairs (the second a multiple of 8: the XCD mapping of the block ids), a ragged G = 2 block (l = 200: 56 queries short) and the hole case at l = 720.

Large offsets: one layer of the arena at H = 24, Lmax = 1360, R = 1032 is 4.3e9 bytes; the sequences that hold byte 2^31 and byte 2^32 (514 and 1028), the first
and the last must come out of append + attention exactly as they do from a four-sequence arena that holds only them."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import fp8_ref as R8  # noqa: E402
from controlvar_amd import ops  # noqa: E402
from controlvar_amd._lib import CvarError  # noqa: E402
from test_kv8_host import quant_heads  # noqa: E402

F32, BF16, U8 = torch.float32, torch.bfloat16, torch.uint8


def bits(x):
    return x.view(torch.int32) if x.dtype == F32 else x.view(torch.int16) if x.dtype == BF16 else x


# ================================================================================================ append
def append_rows(R, l, H, seed):
    """bf16 k|v rows [R*l][2H][64] as fp32 values: magnitudes 2^-20 .. 2^20 per head vector, and the special vectors in front"""
    rng = np.random.default_rng(seed)
    n = R * l * 2 * H
    e = (np.arange(n) * 7 + seed) % 41 - 20
    x = R8.bf16_round((rng.standard_normal((n, 64)) * np.exp2(e)[:, None]).astype(np.float32))
    small = R8.bf16_round((rng.uniform(-200, 200, size=(3, 64)) * 8.0).astype(np.float32))     # |.| <= 1600 < 446 * 8
    special = [np.zeros(64, np.float32), x[1].copy(), x[2].copy()]
    special[1][17] = np.nan
    special[2][63] = -np.inf
    for j, top in enumerate((448.0 * 8, 446.0 * 8, 450.0 * 8)):          # exactly 448 * 2^3, one bf16 ulp (2 * 2^3) below and above
        v = small[j].copy()
        v[(5 * j + 3) % 64] = -top if j == 1 else top
        special.append(v)
    for j, v in enumerate(special):
        if j < n:
            x[j] = v
    return x.reshape(R * l, 2 * H, 64)


@pytest.mark.parametrize('q_off', [0, 30, 511])
@pytest.mark.parametrize('l', [1, 5, 169])
@pytest.mark.parametrize('H', [1, 3, 24])
def test_append_matches_the_numpy_rule_and_touches_nothing_else(gpu_device, H, l, q_off):
    R, Lmax = 3, q_off + l + 3
    x = append_rows(R, l, H, seed=H * 1000 + l * 10 + q_off)
    q_ref, s_ref = quant_heads(x)
    if R * l * 2 * H >= 6:
        assert s_ref.reshape(-1)[0] == np.float32(2.0 ** -60) and s_ref.reshape(-1)[1] == 1.0 and (q_ref.reshape(-1, 64)[2] == 0x7F).all()
        assert list(s_ref.reshape(-1)[3:6]) == [8.0, 8.0, 16.0]           # 448 * 2^3 and one ulp below stay at k = 3, one ulp above moves to k = 4
    want_q = np.full((R, Lmax, 2 * H * 64), 0xA5, np.uint8)
    want_s = np.full((R, Lmax, 2 * H), np.nan, np.float32)
    want_q[:, q_off:q_off + l] = q_ref.reshape(R, l, 2 * H * 64)
    want_s[:, q_off:q_off + l] = s_ref.reshape(R, l, 2 * H)
    # two layers, the second one written: the layer offset rides in the pointer
    kv8 = torch.full((2, R, Lmax, 2 * H * 64), 0xA5, device=gpu_device, dtype=U8)
    ksc = torch.full((2, R, Lmax, 2 * H), float('nan'), device=gpu_device, dtype=F32)
    nan_bits = bits(ksc[0]).clone()
    kv = torch.from_numpy(x.reshape(R * l, 2 * H * 64)).to(gpu_device).to(BF16)
    ops.kv_append_fp8(kv, kv8, ksc, R, H, Lmax, q_off, l, kv8_off=kv8[0].numel(), scale_off=ksc[0].numel())
    torch.cuda.synchronize()
    assert bool((kv8[0] == 0xA5).all()) and torch.equal(bits(ksc[0]), nan_bits)
    got_q, got_s = kv8[1].cpu().numpy(), ksc[1].cpu().numpy()
    assert np.array_equal(got_q, want_q)
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))


# ================================================================================================ attention identity
_DEC = {}


def dequant(kv8, ksc, H):
    """the bf16 arena that holds byte * scale (exact): [R][L][2H*64]"""
    dev = kv8.device
    if dev not in _DEC:
        _DEC[dev] = torch.tensor(R8.DECODE, dtype=F32, device=dev)
    R, L, _ = kv8.shape
    v = _DEC[dev][kv8.long()].view(R, L, 2 * H, 64) * ksc.unsqueeze(-1)
    out = v.to(BF16)
    live = torch.isfinite(v)
    assert torch.equal(out.float()[live], v[live])                         # the conversion did not round
    return out.view(R, L, 2 * H * 64)


def random_arena(R, Lmax, H, kv_end, dev, seed):
    """random finite e4m3 codes of both signs with scales 2^-6 .. 2^6 in rows [0, kv_end); rows behind hold 0x7F bytes and NaN scales"""
    g = torch.Generator(device=dev).manual_seed(seed)
    mag = torch.randint(0, 0x7F, (R, Lmax, 2 * H * 64), device=dev, generator=g, dtype=torch.int16)
    sign = torch.randint(0, 2, (R, Lmax, 2 * H * 64), device=dev, generator=g, dtype=torch.int16)
    kv8 = (mag | (sign << 7)).to(U8)
    ksc = torch.exp2(torch.randint(-6, 7, (R, Lmax, 2 * H), device=dev, generator=g).float())
    kv8[:, kv_end:] = 0x7F
    ksc[:, kv_end:] = float('nan')
    return kv8, ksc, g


def identity_case(dev, R, H, l, q_off, lvl_end=None, holes=None, seed=0):
    kv_end = q_off + l
    Lmax = kv_end + 5
    kv8, ksc, g = random_arena(R, Lmax, H, kv_end, dev, seed)
    ref = dequant(kv8, ksc, H)
    k_rms = float(ref[:, :kv_end, :H * 64].float().pow(2).mean().sqrt())
    q = (torch.randn(R * l, H * 64, device=dev, generator=g) * (3.0 / (8.0 * k_rms))).to(BF16)      # scores of a few units: a softmax over many keys
    out = [torch.full((R * l, H * 64), float('nan'), device=dev, dtype=BF16) for _ in range(2)]
    lse = [torch.full((R, H, l), float('nan'), device=dev, dtype=F32) for _ in range(2)]
    ops.attention_kv8(kv8, ksc, q, out[0], R, H, Lmax, q_off, l, lvl_end, holes=holes, lse=lse[0])
    ops.attention(ref, out[1], R, H, Lmax, q_off, l, 1.0, lvl_end, holes=holes, q=q, prescaled=True, lse=lse[1])
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[1].float()).all()) and bool(torch.isfinite(lse[1]).all())         # the poisoned rows did not reach the bf16 kernel either
    assert torch.equal(bits(out[0]), bits(out[1]))
    assert torch.equal(bits(lse[0]), bits(lse[1]))


LEVELS = [1, 5, 14, 30, 55, 91, 155, 255, 424, 680]                      # the block-causal levels of a 680-token sequence
HOLE_LEVELS, HOLES = [100, 300, 680], [(0, 0), (40, 100), (150, 300)]
HOLE_LEVELS_G2, HOLES_G2 = [100, 300, 720], [(0, 0), (40, 100), (150, 300)]

IDENTITY_CASES = {
    # the issue's table (R = 2, H = 3: G = 1 by the launch rule)
    '1_one_key': dict(R=2, H=3, l=1, q_off=0),
    '2_partial_last_tile': dict(R=2, H=3, l=100, q_off=155),
    '3_l256_680_keys': dict(R=2, H=3, l=256, q_off=424),
    '4_l338_ragged_last_block': dict(R=2, H=3, l=338, q_off=1022),
    '5_level_masked': dict(R=2, H=3, l=680, q_off=0, lvl_end=LEVELS),
    '6_indep_hole_g1': dict(R=2, H=3, l=680, q_off=0, lvl_end=HOLE_LEVELS, holes=HOLES),
    # shapes that reach G = 2 (cdiv(l, 256) * H * R >= 512)
    '3_l256_g2_516_pairs': dict(R=86, H=6, l=256, q_off=424),
    '3_l256_g2_512_pairs_xcd_map': dict(R=64, H=8, l=256, q_off=424),
    '4_l200_g2_ragged_block': dict(R=86, H=6, l=200, q_off=55),
    '5_level_masked_g2': dict(R=29, H=6, l=720, q_off=0, lvl_end=LEVELS[:-1] + [720]),
    '6_indep_hole_g2': dict(R=29, H=6, l=720, q_off=0, lvl_end=HOLE_LEVELS_G2, holes=HOLES_G2),
}


@pytest.mark.parametrize('name', list(IDENTITY_CASES))
def test_attention_over_the_e4m3_arena_equals_the_bf16_kernel_on_the_dequantised_arena(gpu_device, name):
    identity_case(gpu_device, seed=len(name), **IDENTITY_CASES[name])


def test_a_hole_over_the_first_tile_is_refused_without_a_write(gpu_device):
    R, H, l, Lmax = 2, 3, 256, 256
    kv8, ksc, g = random_arena(R, Lmax, H, Lmax, gpu_device, 3)
    q = torch.randn(R * l, H * 64, device=gpu_device, generator=g).to(BF16)
    out = torch.full((R * l, H * 64), float('nan'), device=gpu_device, dtype=BF16)
    lse = torch.full((R, H, l), float('nan'), device=gpu_device, dtype=F32)
    with pytest.raises(CvarError, match='cvar_attention_kv8'):
        ops.attention_kv8(kv8, ksc, q, out, R, H, Lmax, 0, l, [128, 256], holes=[(0, 0), (0, 64)], lse=lse)
    with pytest.raises(CvarError, match='cvar_attention_prescaled'):                                  # ... where the bf16 entry point refuses it
        ops.attention(dequant(kv8, ksc, H), out, R, H, Lmax, 0, l, 1.0, [128, 256], holes=[(0, 0), (0, 64)], q=q, prescaled=True, lse=lse)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all()) and bool(torch.isnan(lse).all())


# ================================================================================================ large offsets
def test_append_and_attention_past_2_31_and_2_32_bytes(gpu_device):
    """peak memory: the 4.3 GB arena, its 0.27 GB scale table and the generator's int16 temporaries of 1.1 GB each (129 sequences at a time): below 9 GB"""
    H, Lmax, R = 24, 1360, 1032
    C2 = 2 * H * 64
    seq_bytes = Lmax * C2
    picks = [0, (1 << 31) // seq_bytes, (1 << 32) // seq_bytes, R - 1]
    assert picks == [0, 514, 1028, 1031] and R * seq_bytes > (1 << 32)
    for p, b in ((picks[1], 1 << 31), (picks[2], 1 << 32)):
        assert p * seq_bytes < b < (p + 1) * seq_bytes                                             # the sequence straddles the boundary
    dev = gpu_device
    g = torch.Generator(device=dev).manual_seed(77)
    kv8 = torch.empty(R, Lmax, C2, device=dev, dtype=U8)
    for r0 in range(0, R, 129):                                                                     # data made on the device, chunk by chunk
        n = min(129, R - r0)
        mag = torch.randint(0, 0x7F, (n, Lmax, C2), device=dev, generator=g, dtype=torch.int16)
        kv8[r0:r0 + n] = (mag | (torch.randint(0, 2, (n, Lmax, C2), device=dev, generator=g, dtype=torch.int16) << 7)).to(U8)
        del mag
    ksc = torch.exp2(torch.randint(-6, 7, (R, Lmax, 2 * H), device=dev, generator=g).float())
    kv = (torch.randn(R, C2, device=dev, generator=g) * 40.0).to(BF16)                              # the k|v rows of the pass: l = 1
    q = (torch.randn(R, H * 64, device=dev, generator=g) * 2e-4).to(BF16)
    q_off, l = Lmax - 1, 1
    idx = torch.tensor(picks, device=dev)
    small8, smalls = kv8[idx].clone(), ksc[idx].clone()                                             # the four sequences BEFORE the append
    before8 = small8.clone()
    out, lse = torch.full((R, H * 64), float('nan'), device=dev, dtype=BF16), torch.full((R, H, 1), float('nan'), device=dev, dtype=F32)
    ops.kv_append_fp8(kv, kv8, ksc, R, H, Lmax, q_off, l)
    ops.attention_kv8(kv8, ksc, q, out, R, H, Lmax, q_off, l, lse=lse)
    outs, lses = torch.full((4, H * 64), float('nan'), device=dev, dtype=BF16), torch.full((4, H, 1), float('nan'), device=dev, dtype=F32)
    ops.kv_append_fp8(kv[idx].contiguous(), small8, smalls, 4, H, Lmax, q_off, l)
    ops.attention_kv8(small8, smalls, q[idx].contiguous(), outs, 4, H, Lmax, q_off, l, lse=lses)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    assert torch.equal(kv8[idx], small8) and torch.equal(bits(ksc[idx]), bits(smalls))
    assert torch.equal(bits(out[idx]), bits(outs)) and torch.equal(bits(lse[idx]), bits(lses))
    # only the appended row moved
    assert torch.equal(small8[:, :q_off], before8[:, :q_off]) and not torch.equal(small8[:, q_off], before8[:, q_off])
