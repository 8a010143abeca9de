"""LoRA host side (controlvar_amd/lora.py): targets, initialisation, trainable count, state-dict layouts, merge, checkpoint loading.
CPU only: nothing here packs weights or launches a kernel."""
import math

import pytest
import torch

from controlvar_amd import checkpoint as ckpt
from controlvar_amd import lora, models
from controlvar_amd import train as T


def build(depth=2, control=True, **kw):
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    if control:
        return models.build_control_var(vae, depth=depth, mask_type='interleave_append', multi_cond=True, compute_dtype=torch.float32, **kw)
    return models.build_var(vae, depth=depth, compute_dtype=torch.float32, **kw)


def rule_targets(depth):
    """the reference's rule spelled out: proj / fc1 / fc2 / ada_lin.1 of every block, then head_nm.ada_lin.1 (attn.mat_qkv excluded)"""
    out = []
    for i in range(depth):
        out += [f'blocks.{i}.attn.proj', f'blocks.{i}.ffn.fc1', f'blocks.{i}.ffn.fc2', f'blocks.{i}.ada_lin.1']
    return out + ['head_nm.ada_lin.1']


@pytest.mark.parametrize('control', [True, False])
def test_targets_follow_the_reference_rule(control):
    m = build(control=control)
    assert lora.add_lora(m) == rule_targets(2)
    assert all(not lora.is_target(n) for n in ('blocks.0.attn.mat_qkv', 'blocks.0.attn.proj_drop', 'blocks.0.ffn', 'head'))


def test_d24_targets_and_trainable_count():
    m = build(depth=24)
    assert lora.add_lora(m) == rule_targets(24)
    C = 1536
    tr, total = lora.trainable_parameters(m)
    assert tr == 24 * 16 * 19 * C + 16 * 3 * C == 11_280_384
    assert total == sum(p.numel() for p in m.parameters())


def test_initialisation_and_freezing():
    m = build()
    lora.add_lora(m, seed=4)
    assert m._lora['scale'] == 2.0 and m._lora['r'] == 16 and m._lora['dropout'] == 0.05
    for t, (A, B) in lora.adapters(m).items():
        fan_in = A.shape[1]
        assert A.shape[0] == 16 and B.shape[1] == 16 and torch.count_nonzero(B) == 0
        assert A.abs().max() <= 1 / math.sqrt(fan_in)
        assert abs(A.std().item() - 1 / math.sqrt(3 * fan_in)) < 0.1 / math.sqrt(3 * fan_in)        # U(-b, b): std b / sqrt(3)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert frozen and all('.lora_' not in n for n in frozen)
    assert all('.lora_' in n for n, p in m.named_parameters() if p.requires_grad)
    m2 = build()
    lora.add_lora(m2, seed=4)
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))             # seeded


def test_unsupported_variants_raise():
    with pytest.raises(NotImplementedError, match='shared_aln'):
        lora.add_lora(build(shared_aln=True))
    with pytest.raises(NotImplementedError, match='SABlock'):
        lora.add_lora(build(aln=-1))
    with pytest.raises(NotImplementedError):
        lora.add_lora(build(), r=32)


def _randomise(m, seed=0):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, (A, B) in lora.adapters(m).items():
            B.copy_(torch.randn(B.shape, generator=g))
            A.copy_(torch.randn(A.shape, generator=g))


def test_state_dict_layouts_round_trip():
    m = build()
    plain = set(m.state_dict())
    targets = lora.add_lora(m)
    _randomise(m)
    peft = lora.lora_state_dict(m, 'peft')
    want = set()
    for k in plain:
        t = next((t for t in targets if k.startswith(t + '.')), None)
        want.add('base_model.model.' + (k if t is None else t + '.base_layer' + k[len(t):]))
    for t in targets:
        want |= {f'base_model.model.{t}.lora_A.default.weight', f'base_model.model.{t}.lora_B.default.weight'}
    assert set(peft) == want
    adapter = lora.lora_state_dict(m, 'adapter')
    assert set(adapter) == {f'base_model.model.{t}.lora_{ab}.weight' for t in targets for ab in 'AB'}
    for src in (peft, adapter, {'module.' + k: v for k, v in peft.items()}, {'module.' + k: v for k, v in adapter.items()}):
        m2 = build()
        lora.add_lora(m2, seed=9)
        lora.load_lora(m2, src)
        assert all(torch.equal(v, m.state_dict()[k]) for k, v in m2.state_dict().items())
    # through the checkpoint reader with the DDP prefix, and a strict load of the peft layout
    m3 = build()
    lora.add_lora(m3, seed=9)
    ckpt.load_weights(m3, {'model_state_dict': {'module.' + k: v for k, v in peft.items()}})
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in m3.state_dict().items())


def test_merge_folds_the_adapters_into_a_plain_model():
    m = build()
    plain = set(m.state_dict())
    lora.add_lora(m)
    _randomise(m)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    lora.merge_lora(m)
    sd = m.state_dict()
    assert set(sd) == plain
    for t in rule_targets(2):
        A, B = before[f'{t}.lora_A.default.weight'], before[f'{t}.lora_B.default.weight']
        assert torch.allclose(sd[f'{t}.weight'], before[f'{t}.weight'] + 2 * B @ A, atol=1e-5)
    assert torch.equal(sd['blocks.0.attn.mat_qkv.weight'], before['blocks.0.attn.mat_qkv.weight'])
    assert all(p.requires_grad for p in m.parameters())
    fresh = build()
    fresh.load_state_dict(sd, strict=True)


def test_adapter_free_models_keep_their_keys_and_the_param_filter():
    m = build()
    keys = list(m.state_dict())
    assert not any('lora' in k for k in keys)
    names, _, groups = T.filter_params(m)
    assert len(names) == len(list(m.parameters())) and len(groups) == 2
    lora.add_lora(m)
    with pytest.raises(AssertionError, match='frozen parameter'):
        T.filter_params(m)                                             # the reference's assert stays
    names, params, groups = lora.param_groups(m)
    assert set(names) == {n for n, p in m.named_parameters() if p.requires_grad}
    assert len(groups) == 1 and groups[0]['wd_sc'] == 1.0           # 2-D adapter weights: the decayed group 'D'
