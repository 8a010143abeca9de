"""ControlVAR.graphed_conditional_generator, host side: what it refuses, and that it refuses before any device work.
CPU only: the models live on the CPU, so a refusal that came after the first device allocation would surface as a CUDA error instead."""
import pytest
import torch

from controlvar_amd import models


def build(depth=2, control=True, mask_type='interleave_append', **kw):
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    if control:
        return models.build_control_var(vae, depth=depth, mask_type=mask_type, multi_cond=True, compute_dtype=torch.float32, **kw)
    return models.build_var(vae, depth=depth, compute_dtype=torch.float32, **kw)


def test_plain_var_raises_as_its_conditional_infer_cfg_does():
    m = build(control=False)
    with pytest.raises(NotImplementedError, match='plain VAR has no conditional_infer_cfg') as a:
        m.conditional_infer_cfg(2, None)
    with pytest.raises(NotImplementedError, match='plain VAR has no conditional_infer_cfg') as b:
        m.graphed_conditional_generator(2, given='control')
    assert str(a.value) == str(b.value)


def test_mask_factor_one_is_refused():
    m = build(mask_type='replace')
    with pytest.raises(NotImplementedError, match=r'needs mask_factor == 2 \(control_var.py:333\)'):
        m.graphed_conditional_generator(2, given='control')


def test_torch_sampler_is_refused_in_graphed_generators_words():
    m = build(sampler='torch')
    with pytest.raises(NotImplementedError, match=r"captures the counter sampler only: sampler='torch' draws its noise with torch on model.rng") as e:
        m.graphed_conditional_generator(2, given='image')
    assert "set model.sampler = 'counter' to capture, or call conditional_infer_cfg" in str(e.value)
    with pytest.raises(NotImplementedError, match="captures the counter sampler only"):
        m.graphed_generator(2)


def test_separator_models_are_refused():
    m = build(separator=True)
    with pytest.raises(NotImplementedError, match='separator: conditional_infer_cfg ignores the special tokens'):
        m.graphed_conditional_generator(2, given='control')


@pytest.mark.parametrize('kw,msg', [(dict(given='mask'), "given='mask': one of control / image"),
                                    (dict(given='control', source='file'), "source='file': one of ids / pixels"),
                                    (dict(given='image', decode='image'), "decode='image': one of both / generated")])
def test_unknown_choices_are_refused(kw, msg):
    with pytest.raises(ValueError, match=msg):
        build().graphed_conditional_generator(2, **kw)


@pytest.mark.parametrize('cfg', [1.5, (1.5,), (1.5, 1.5), (1.0, 2.0, 3.0, 4.0), []])
def test_cfg_must_be_three_numbers(cfg):
    with pytest.raises(ValueError, match='cfg: three guidance scales'):
        build().graphed_conditional_generator(2, given='control', cfg=cfg)


def test_top_k_beyond_the_vocabulary_raises_as_the_eager_call():
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        build().graphed_conditional_generator(2, given='control', top_k=5000)
