"""gemm_precision='bf16x3' on the host (no GPU): the split contract restated in numpy (tests/x3_ref.py), the weight pack of a depth-2 model, the keyword
through both factories, the refusals - each raised before any device work, so a CPU model shows them - and the pack dropped when the attribute flips."""
import numpy as np
import pytest
import torch

import x3_ref as X
from controlvar_amd import lora, models

F32, BF16 = torch.float32, torch.bfloat16
C, DEPTH, HID = 128, 2, 512


def make(gp='bf16x3', control=True, dtype=F32, **kw):
    vae = models.build_vae(ch=32, compute_dtype=dtype)
    if control:
        return models.build_control_var(vae, depth=DEPTH, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, gemm_precision=gp, **kw)
    return models.build_var(vae, depth=DEPTH, compute_dtype=dtype, gemm_precision=gp, **kw)


# ------------------------------------------------------------------------------------------------ the split, restated
BF16_MAX = np.float32(3.3895313892515355e38)           # largest finite bf16


def split_cases():
    rng = np.random.default_rng(0)
    normal = (rng.standard_normal(4096) * np.exp2(rng.integers(-20, 21, 4096))).astype(np.float32)
    # lo a bf16 subnormal: |x - hi| < 2^-126, i.e. |x| around 2^-118 and below (still a normal fp32 / bf16 hi)
    sublo = (rng.uniform(1, 2, 512) * np.exp2(rng.integers(-125, -117, 512)) * rng.choice([-1, 1], 512)).astype(np.float32)
    edge = np.array([0.0, -0.0, BF16_MAX, -BF16_MAX, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9, 1.0 + 3 * 2.0 ** -9], dtype=np.float32)
    return {'normal': normal, 'lo_subnormal': sublo, 'edges': edge}


@pytest.mark.parametrize('name', ['normal', 'lo_subnormal', 'edges'])
def test_hi_plus_lo_reconstructs_the_value(name):
    x = split_cases()[name]
    hi, lo = X.split(x)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    # hi and lo are bf16 values: their low 16 bits are zero
    assert not (hi.view(np.uint32) & 0xFFFF).any() and not (lo.view(np.uint32) & 0xFFFF).any()
    err = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64))
    # 2^-17 |x|; a subnormal lo is rounded to the bf16 subnormal grid (spacing 2^-133): half a step on top
    bound = 2.0 ** -17 * np.abs(x.astype(np.float64)) + (2.0 ** -134 if name == 'lo_subnormal' else 0.0)
    assert (err <= bound).all(), float((err / np.maximum(bound, 1e-300)).max())
    if name == 'lo_subnormal':
        sub = (lo != 0) & (np.abs(lo) < 2.0 ** -126)
        assert sub.sum() > 100                     # the case is what its name says
    if name == 'edges':
        assert hi[0] == 0 and lo[0] == 0 and not np.signbit(hi[0]) and np.signbit(hi[1]) and lo[1] == 0      # +-0 stay +-0, lo = 0
        assert hi[2] == BF16_MAX and lo[2] == 0 and hi[3] == -BF16_MAX and lo[3] == 0
        assert hi[6] == 1.0 and lo[6] == np.float32(2.0 ** -8)          # a tie of the first rounding goes to even; lo carries the rest exactly
        assert hi[8] == np.float32(1.0 + 2.0 ** -7) and lo[8] == np.float32(-(2.0 ** -9))


def test_three_segment_product_against_float64():
    rng = np.random.default_rng(1)
    a = (rng.standard_normal(20000) * np.exp2(rng.integers(-6, 7, 20000))).astype(np.float32)
    w = (rng.standard_normal(20000) * np.exp2(rng.integers(-6, 7, 20000))).astype(np.float32)
    ah, al = (v.astype(np.float64) for v in X.split(a))
    wh, wl = (v.astype(np.float64) for v in X.split(w))
    got = ah * wh + al * wh + ah * wl
    aw = np.abs(a.astype(np.float64) * w.astype(np.float64))
    # dropped term 2^-16 |a w| plus the representation terms 2 * 2^-17 |a w| (+ their product)
    assert (np.abs(got - a.astype(np.float64) * w.astype(np.float64)) <= (2.0 ** -16 + 2 * 2.0 ** -17 + 2.0 ** -34) * aw).all()
    # and the rows of the GEMM form hold exactly those three products
    A, W = X.bf16_value(X.activation_rows(a[None, :64])), X.bf16_value(X.weight_rows(w[None, :64]))
    assert np.array_equal(A[0, :64] * W[0, :64] + A[0, 64:128] * W[0, 64:128] + A[0, 128:] * W[0, 128:],
                          (ah[:64] * wh[:64]).astype(np.float32) + (al[:64] * wh[:64]).astype(np.float32) + (ah[:64] * wl[:64]).astype(np.float32))


def test_numpy_model_of_the_gemm_stays_inside_the_bound_and_plain_bf16_does_not():
    for (M, N, K), seed in (((5, 256, 128), 0), ((300, 200, 96), 1), ((64, 128, 1536), 2)):
        a, w = X.operands(M, N, K, seed)
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        bd = X.product_bound(a, w)
        assert (np.abs(X.split_product_model(a, w) - ref) <= bd).all()
        plain = X.bf16_round(a) @ X.bf16_round(w).T
        assert (np.abs(plain - ref) > bd).any()


# ------------------------------------------------------------------------------------------------ the weight pack
def test_weight_pack_of_a_depth2_model():
    m = make()
    P = m._build_pack(None, (), None, host=True)
    sd = m.state_dict()
    n_ada = DEPTH * 6 * C + 2 * C
    want = {'w_qkv_x3': (DEPTH, 3 * C, 3 * C), 'w_proj_x3': (DEPTH, C, 3 * C), 'w_fc1_x3': (DEPTH, HID, 3 * C), 'w_fc2_x3': (DEPTH, C, 3 * HID),
            'w_ada_x3': (n_ada, 3 * C), 'w_head_x3': (4096, 3 * C)}
    for key, shape in want.items():
        assert tuple(P[key].shape) == shape and P[key].dtype == BF16 and P[key].is_contiguous(), key
    assert P['hid'] == HID and P['n_ada'] == n_ada
    # the fp32 matrices are not held beside the split ones: they are built when forward() / training first ask
    assert all(k not in P for k in ('w_qkv', 'w_proj', 'w_fc1', 'w_fc2', 'w_ada', 'w_head'))
    srcs = {'w_qkv_x3': 'attn.mat_qkv.weight', 'w_proj_x3': 'attn.proj.weight', 'w_fc1_x3': 'ffn.fc1.weight', 'w_fc2_x3': 'ffn.fc2.weight'}
    for key, name in srcs.items():
        K = want[key][2] // 3
        flat = P[key].reshape(-1).view(torch.int16)
        for i in range(DEPTH):
            W = sd[f'blocks.{i}.{name}'].detach().float().numpy()
            rows = X.weight_rows(W)
            # layer i starts at w_off = i * N * 3K elements (units of 3 K per row)
            off = i * W.shape[0] * 3 * K
            got = flat[off:off + W.shape[0] * 3 * K].view(W.shape[0], 3 * K).numpy().view(np.uint16)
            assert np.array_equal(got, rows), (key, i)
            assert np.array_equal(got[:, :K], got[:, K:2 * K])                                         # segments 0 and 1: w_hi twice
            hi = X.bf16_value(got[:, :K])
            assert np.array_equal(got[:, 2 * K:], X.bf16_bits((W - hi).astype(np.float32)))            # segment 2: bf16(W - hi)
    ada = torch.cat([sd[f'blocks.{i}.ada_lin.1.weight'] for i in range(DEPTH)] + [sd['head_nm.ada_lin.1.weight']]).detach().float().numpy()
    assert np.array_equal(P['w_ada_x3'].view(torch.int16).numpy().view(np.uint16), X.weight_rows(ada))
    assert np.array_equal(P['w_head_x3'].view(torch.int16).numpy().view(np.uint16), X.weight_rows(sd['head.weight'].detach().float().numpy()))
    # first use builds the fp32 copy, as an fp32 model's pack holds it
    P0 = make(gp=None)._build_pack(None, (), None, host=True)
    assert torch.equal(P['w_fc1'], P0['w_fc1']) and P['w_fc1'].dtype == F32 and 'w_qkv' not in P
    assert not any(k.endswith('_x3') for k in P0)


@pytest.mark.parametrize('control', [True, False])
def test_keyword_reaches_the_model_through_the_factories(control):
    m = make(control=control)
    assert m.gemm_precision == 'bf16x3' and isinstance(m, models.ControlVAR if control else models.VAR)
    assert make(gp=None, control=control).gemm_precision is None
    with pytest.raises(ValueError, match='gemm_precision must be one of'):
        make(gp='bf16x2', control=control)


@pytest.mark.parametrize('control', [True, False])
def test_a_bf16_model_refuses_the_mode_in_words(control):
    with pytest.raises(ValueError, match=r"needs a compute_dtype=torch\.float32 model"):
        make(control=control, dtype=BF16)
    m = make(gp=None, control=control, dtype=BF16)
    with pytest.raises(ValueError, match=r"needs a compute_dtype=torch\.float32 model"):
        m.gemm_precision = 'bf16x3'
    assert m.gemm_precision is None


def _adapter(m, r=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    sd = {}
    for t in lora.target_names(m):
        out_f, in_f = mods[t]._parameters['weight'].shape
        sd[f'{t}.lora_A.default.weight'] = torch.randn(r, in_f, generator=g) / in_f ** 0.5
        sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * 0.2
    return sd


def test_the_adapter_bank_is_refused_in_words():
    m = make()
    with pytest.raises(NotImplementedError, match='adapter bank .* is not offered'):
        lora.attach_adapters(m, [_adapter(m)])
    assert not lora.has_adapters(m)
    with pytest.raises(NotImplementedError, match='adapter bank .* is not offered'):
        m.autoregressive_infer_cfg(2, torch.tensor([1, 2]), cond_type=torch.tensor([0, 1]), g_seed=[0, 1], adapter=[0, -1])
    with pytest.raises(NotImplementedError, match='adapter bank .* is not offered'):
        m.graphed_generator(2, per_request=True, adapters=True)
    # a model that has a bank refuses the switch, and keeps its mode
    m0 = make(gp=None)
    lora.attach_adapters(m0, [_adapter(m0)])
    with pytest.raises(NotImplementedError, match='adapter bank .* is not offered'):
        m0.gemm_precision = 'bf16x3'
    assert m0.gemm_precision is None and lora.has_adapters(m0)


def test_flipping_the_attribute_on_a_built_model_drops_the_pack_and_the_arena():
    m = make(gp=None)
    for new in ('bf16x3', None):
        m._packed, m._packed_base, m._arena = m._build_pack(None, (), None, host=True), object(), {0: ('key', torch.zeros(1))}
        old = m._packed
        m.gemm_precision = m.gemm_precision            # same value: nothing is dropped
        assert m._packed is old and m._arena is not None
        m.gemm_precision = new
        assert m._packed is None and m._packed_base is None and m._arena is None and m.gemm_precision == new
    with pytest.raises(ValueError):
        m.gemm_precision = 'fp16x2'
    assert m.gemm_precision is None


def test_the_torch_op_is_registered_with_a_fake_kernel():
    import controlvar_amd
    ns = controlvar_amd.register_torch_ops()
    from controlvar_amd import torch_ops
    assert 'ln_modulate_split3' in torch_ops.OPS and ns.ln_modulate_split3.default._schema.name == 'cvar::ln_modulate_split3'
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        y = ns.ln_modulate_split3(torch.empty(2, 3, 64, device='cuda'), torch.empty(2, 64, device='cuda'), torch.empty(2, 64, device='cuda'), 3, 1e-6)
        assert y.shape == (2, 3, 192) and y.dtype == BF16
    with pytest.raises(RuntimeError, match='no CPU'):
        ns.ln_modulate_split3(torch.randn(6, 64), torch.randn(2, 64), torch.randn(2, 64), 3, 1e-6)
