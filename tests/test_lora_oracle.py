"""The LoRA oracle (oracle/lora_ref.py and the lora hook of oracle.var_ref / oracle.train_ref), CPU only: the host copy of the dropout
keep mask (threshold, scale, statistics, independent streams), and the adapter term against merged weights W + s B A in float64."""
import numpy as np
import pytest
import torch

from controlvar_amd import lora, models
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VarConfig
from oracle import lora_ref, train_ref, var_ref


# ---------------------------------------------------------------------------------------------------------------- the host mask
def test_threshold_and_scale_follow_the_float32_p():
    assert lora_ref.thresh(0.0) == 0
    assert lora_ref.thresh(0.5) == 2 ** 31 and lora_ref.thresh(0.75) == 3 * 2 ** 30
    # 0.3 is not a float32: the threshold is taken from float32(0.3) = 0.30000001192..., not from the double 0.3
    assert lora_ref.thresh(0.3) == int(float(np.float32(0.3)) * 2 ** 32) == 1288490240
    assert int(0.3 * 2 ** 32) == 1288490188
    assert lora_ref.thresh(1 - 1e-9) == 2 ** 32 - 1                 # float32(p) rounds to 1.0: clamped, nothing is kept
    assert lora_ref.inv_keep(0.0) == 1.0 and lora_ref.inv_keep(0.5) == 2.0 and lora_ref.inv_keep(0.75) == 4.0
    assert lora_ref.inv_keep(0.3) == float(np.float32(1.0) / np.float32(0.7)) != 1.0 / 0.7
    f = lora_ref.drop_factor(64, 64, 0.3, 5, 2)
    assert set(f.unique().tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.7))}
    assert torch.equal(lora_ref.drop_factor(3, 8, 0.0, 5, 2), torch.ones(3, 8, dtype=torch.float64))


def test_hash_wraps_modulo_2_32():
    # lora_mix restated with Python ints: the numpy uint32 products must wrap, not widen
    def mix(h):
        h ^= h >> 16; h = (h * 0x7feb352d) & 0xffffffff
        h ^= h >> 15; h = (h * 0x846ca68b) & 0xffffffff
        return h ^ (h >> 16)
    xs = [0, 1, 0x9e3779b9, 0xffffffff, 123456789]
    assert [int(v) for v in lora_ref.mix(np.array(xs, dtype=np.uint32))] == [mix(x) for x in xs]
    seed, tag = 0x123456789abcdef0, 97
    h = mix((seed & 0xffffffff) ^ 0x9e3779b9)
    h = mix(h ^ (seed >> 32))
    k = mix(h ^ ((tag * 0x85ebca6b + 0x632be5ab) & 0xffffffff))
    assert int(lora_ref.key(seed, tag)) == k
    assert int(lora_ref.key(seed - 2 ** 64, tag)) == k                  # a negative Python int names the same uint64 seed
    row, col = 40000, 6000
    rk = mix(k ^ ((row * 0xc2b2ae35) & 0xffffffff))
    bit = mix((rk + col * 0x9e3779b9) & 0xffffffff) >= lora_ref.thresh(0.3)
    assert bool(lora_ref.keep_mask(row + 1, col + 1, 0.3, seed, tag)[row, col]) == bit


@pytest.mark.parametrize('p', [0.05, 0.3, 0.5])
def test_keep_fraction(p):
    m = lora_ref.keep_mask(1024, 1024, p, 11, 0)
    assert abs(m.mean() - (1 - p)) < 3e-3                               # 1M Bernoulli draws: sd <= 5e-4
    rows, cols = m.mean(1), m.mean(0)
    assert abs(rows.std() - np.sqrt(p * (1 - p) / 1024)) < 0.25 * np.sqrt(p * (1 - p) / 1024)       # no row or column structure
    assert abs(cols.std() - np.sqrt(p * (1 - p) / 1024)) < 0.25 * np.sqrt(p * (1 - p) / 1024)


def test_streams_of_different_seeds_and_tags_are_independent():
    p = 0.3
    m0 = lora_ref.keep_mask(512, 512, p, 11, 0)
    chance = (1 - p) ** 2 + p ** 2
    for seed, tag in ((11, 1), (11, 4), (11, 99), (12, 0), (11 + 2 ** 32, 0), (-11, 0)):
        other = lora_ref.keep_mask(512, 512, p, seed, tag)
        assert abs((other == m0).mean() - chance) < 6e-3, (seed, tag)     # agreement by chance only (sd 9e-4)
    # shifted rows / columns of one stream are not copies of each other either
    assert abs((m0[1:] == m0[:-1]).mean() - chance) < 6e-3
    assert abs((m0[:, 1:] == m0[:, :-1]).mean() - chance) < 6e-3
    assert np.array_equal(m0, lora_ref.keep_mask(512, 512, p, 11, 0))


def test_target_tags():
    assert lora_ref.target_tag('blocks.0.attn.proj', 2) == 0
    assert lora_ref.target_tag('blocks.3.ffn.fc1', 24) == 13
    assert lora_ref.target_tag('blocks.23.ffn.fc2', 24) == 94
    assert lora_ref.target_tag('blocks.23.ada_lin.1', 24) == 95
    assert lora_ref.target_tag('head_nm.ada_lin.1', 24) == 99
    with pytest.raises(KeyError):
        lora_ref.target_tag('blocks.0.attn.mat_qkv', 24)


# ---------------------------------------------------------------------------------------------------------------- the adapter term
def lora_model(control, r, b_seed=3):
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    if control:
        m = models.ControlVAR(vae, depth=2, embed_dim=128, num_heads=2, mask_factor=2, multi_cond=True, patch_nums=PN,
                              compute_dtype=torch.float32, cond_drop_rate=0.0, init_seed=0)
        cfg = VarConfig(depth=2)
    else:
        m = models.VAR(vae, depth=2, embed_dim=128, num_heads=2, patch_nums=PN, compute_dtype=torch.float32, cond_drop_rate=0.0, init_seed=0)
        cfg = VarConfig(depth=2, mask_factor=1, control=False, multi_cond=False)
    lora.add_lora(m, r=r, seed=1)
    g = torch.Generator().manual_seed(b_seed)
    with torch.no_grad():
        for _, (_, B) in lora.adapters(m).items():
            B.copy_(torch.randn(B.shape, generator=g) * 0.05)
    return m, cfg


def f64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


def batch(cfg, seed=5):
    B, L, fl = 2, cfg.pyramid.L, cfg.pyramid.first_l
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L - fl, 32, generator=gen, dtype=torch.float64)
    tg = torch.randint(0, 4096, (B, L), generator=gen)
    return x, tg, torch.tensor([5, 999]), torch.tensor([1, 3])


@pytest.mark.parametrize('control,r', [(True, 16), (True, 5), (False, 5)])
def test_hook_at_p0_matches_merged_weights_in_float64(control, r):
    m, cfg = lora_model(control, r)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    s = m._lora['scale']
    assert s == 32 / r
    base = f64({k: v for k, v in sd.items() if '.lora_' not in k})
    merged = dict(base)
    for t in m._lora['targets']:
        A, B = sd[f'{t}.lora_A.default.weight'].double(), sd[f'{t}.lora_B.default.weight'].double()
        merged[f'{t}.weight'] = base[f'{t}.weight'] + s * B @ A
    # lora.merged_state folds the same W + s B A (in fp32)
    ms = lora.merged_state(sd, m._lora)
    assert set(ms) == set(merged)
    for t in m._lora['targets']:
        assert (ms[f'{t}.weight'].double() - merged[f'{t}.weight']).abs().max() < 1e-6
    x, tg, cls, ty = batch(cfg)
    ty = ty if cfg.control else None
    hook = lora_ref.LoraTerm(lora.adapters(m), s, p=0.0, dtype=torch.float64)
    with torch.no_grad():
        lg_hook = var_ref.forward_logits(base, cfg, cls, x, ty, lora=hook)
        lg_merged = var_ref.forward_logits(merged, cfg, cls, x, ty)
    assert lg_hook.dtype == torch.float64
    assert (lg_hook - lg_merged).abs().max() < 1e-10 * lg_merged.abs().max()
    # adapter gradients by autograd through the hook == the chain rule through W_eff = W + s B A
    loss_h, _, g_hook = train_ref.loss_and_grads(base, cfg, cls, x, ty, tg, lora=hook)
    loss_m, _, g_merged = train_ref.loss_and_grads(merged, cfg, cls, x, ty, tg)
    assert abs(loss_h.item() - loss_m.item()) < 1e-12
    assert set(g_hook) == {n for n, p in m.named_parameters() if p.requires_grad}
    for t in m._lora['targets']:
        dW = g_merged[f'{t}.weight']
        A, B = hook.A[t].detach(), hook.B[t].detach()
        for name, want in ((f'{t}.lora_B.default.weight', s * dW @ A.t()), (f'{t}.lora_A.default.weight', s * B.t() @ dW)):
            got = g_hook[name]
            assert got.shape == want.shape
            assert (got - want).abs().max() < 1e-10 * max(1e-6, want.abs().max().item()), name
    # a second call starts from fresh gradients (no accumulation across calls)
    _, _, g2 = train_ref.loss_and_grads(base, cfg, cls, x, ty, tg, lora=hook)
    assert all(torch.equal(g2[k], g_hook[k]) for k in g_hook)


def test_hook_applies_the_mask_of_each_target_at_the_engine_rows():
    m, cfg = lora_model(True, 5)
    ad = lora.adapters(m)
    s, p, seed = m._lora['scale'], 0.3, 2 ** 40 + 7
    hook = lora_ref.LoraTerm(ad, s, p=p, seed=seed, dtype=torch.float64)
    g = torch.Generator().manual_seed(0)
    B, L, C = 2, 7, cfg.C
    depth = cfg.depth
    for name, rows, K in (('blocks.1.attn.proj', B * L, C), ('blocks.1.ffn.fc1', B * L, C), ('blocks.1.ffn.fc2', B * L, 4 * C),
                          ('blocks.0.ada_lin.1', B, C), ('head_nm.ada_lin.1', B, C)):
        x = torch.randn(rows, K, generator=g, dtype=torch.float64)
        tag = {'blocks.1.attn.proj': 4, 'blocks.1.ffn.fc1': 5, 'blocks.1.ffn.fc2': 6, 'blocks.0.ada_lin.1': 3, 'head_nm.ada_lin.1': 4 * depth + 3}[name]
        A, Bw = ad[name][0].detach().double(), ad[name][1].detach().double()
        keep = torch.from_numpy(lora_ref.keep_mask(rows, K, p, seed, tag)).double() * lora_ref.inv_keep(p)
        want = s * ((x * keep) @ A.t()) @ Bw.t()
        xin = x.view(B, L, K) if rows == B * L else x                          # block rows b * L + l, adaLN rows b
        got = hook(name, xin).reshape(rows, -1)
        assert (got - want).abs().max() < 1e-12 * want.abs().max(), name
        other = s * ((x * torch.from_numpy(lora_ref.keep_mask(rows, K, p, seed, tag ^ 1)).double() * lora_ref.inv_keep(p)) @ A.t()) @ Bw.t()
        assert (got - other).abs().max() > 1e-3 * want.abs().max(), name        # the tag is not interchangeable
