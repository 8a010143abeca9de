"""LoRA fine-tuning (the ``--lora`` option of train_control_var.py:337-353 / train_control_var_hpu.py:449-470 / train_var_hpu.py:306-330).

The reference wraps the transformer with peft (``LoraConfig(r=16, lora_alpha=32, lora_dropout=0.05, bias="none")``) on the modules
its name rule selects; here the adapters are plain parameters of the model under peft's key names, and the training engine runs the
rank-r branch through the HIP kernels of csrc/lora.hip (DESIGN.md "LoRA").  A target computes

    y = x W^T + b + s * (drop(x) A^T) B^T,    s = alpha / r,  A (r, in) ~ U(-1/sqrt(in), 1/sqrt(in)),  B (out, r) = 0

Only A and B train; every other parameter is frozen.  In eval() the adapters are merged into the packed GEMM weights, so inference
runs exactly the adapter-free kernels.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Any, Dict, List, Mapping, Tuple, Union

import torch
from torch import nn

PEFT_PREFIX = 'base_model.model.'
ADAPTER = 'default'                     # peft's adapter name
MAX_RANK = 16                           # rank the GPU kernels hold in registers (csrc/lora.hip LORA_R)


def is_target(name: str) -> bool:
    """the reference's target rule over named_modules() (train_control_var_hpu.py:449-470, train_var_hpu.py:306-330)"""
    return ('attn.' in name and 'attn.proj_drop' not in name and 'attn.mat_qkv' not in name) or 'ffn.fc' in name or 'ada_lin.1' in name


def _linear_like(m: nn.Module) -> bool:
    w = m._parameters.get('weight')
    return w is not None and w.ndim == 2


def target_names(model) -> List[str]:
    """names of the modules add_lora wraps, in named_modules() order"""
    return [n for n, m in model.named_modules() if n and '.lora_' not in n and is_target(n) and _linear_like(m)]


def has_lora(model) -> bool:
    return getattr(model, '_lora', None) is not None


def _check_supported(model):
    cfg = getattr(model, 'cfg', None)
    if cfg is None or not hasattr(model, '_pack'):
        raise TypeError('add_lora expects a controlvar_amd ControlVAR / VAR model')
    if cfg.shared_aln:
        raise NotImplementedError("LoRA with shared_aln: 'shared_ada_lin.1' matches the target rule and peft's wrapper breaks on SharedAdaLin's "
                                  'reshaped output (basic_var.py:204-205); no shipped config uses shared_aln')
    if cfg.sa_block:
        raise NotImplementedError('LoRA with aln < 0 (SABlock): the block has no ada_lin to adapt; no shipped config uses it')


def add_lora(model, r: int = 16, alpha: float = 32, dropout: float = 0.05, seed: int = 0) -> List[str]:
    """Register ``<target>.lora_A.default.weight`` (r, in) and ``<target>.lora_B.default.weight`` (out, r) on every target and freeze every
    other parameter (peft's get_peft_model with the reference's LoraConfig).  A is drawn from U(-1/sqrt(in), 1/sqrt(in)) -
    kaiming_uniform_(a=sqrt(5)) - with a generator seeded by ``seed``; B starts at zero.  Returns the target names."""
    _check_supported(model)
    if has_lora(model):
        raise RuntimeError('the model already has LoRA adapters (one adapter per model)')
    if not 1 <= r <= MAX_RANK:
        raise NotImplementedError(f'LoRA rank {r}: the GPU kernels take 1 <= r <= {MAX_RANK}')
    if not 0.0 <= dropout < 1.0:
        raise ValueError(f'lora dropout {dropout} outside [0, 1)')
    from .models import _Tree
    names = target_names(model)
    mods = dict(model.named_modules())
    g = torch.Generator().manual_seed(int(seed))
    for p in model.parameters():
        p.requires_grad_(False)
    for n in names:
        m = mods[n]
        w = m._parameters['weight']
        out_f, in_f = w.shape
        bound = 1.0 / math.sqrt(in_f)
        A = (torch.rand(r, in_f, generator=g, dtype=torch.float64) * 2 - 1).mul_(bound).float()
        B = torch.zeros(out_f, r)
        for kind, t in (('lora_A', A), ('lora_B', B)):
            holder = _Tree()
            holder.add_module(ADAPTER, _Tree())
            holder._modules[ADAPTER].register_parameter('weight', nn.Parameter(t.to(device=w.device, dtype=w.dtype), requires_grad=True))
            m.add_module(kind, holder)
    model._lora = dict(r=int(r), alpha=float(alpha), dropout=float(dropout), scale=float(alpha) / int(r), targets=list(names))
    _invalidate(model)
    return names


def _invalidate(model):
    model._packed = None
    model._packed_base = None
    if getattr(model, '_train_engine', None) is not None:
        model._train_engine = None


def adapters(model) -> "OrderedDict[str, Tuple[torch.Tensor, torch.Tensor]]":
    """target name -> (A, B) parameters"""
    mods = dict(model.named_modules())
    return OrderedDict((n, (mods[n].lora_A._modules[ADAPTER].weight, mods[n].lora_B._modules[ADAPTER].weight)) for n in model._lora['targets'])


def merged_state(sd: Mapping[str, torch.Tensor], lora: Mapping[str, Any]) -> Dict[str, torch.Tensor]:
    """state dict with W + s B A folded in fp32 and the adapter keys removed (the key set of an adapter-free model)"""
    s = lora['scale']
    out = {k: v for k, v in sd.items() if '.lora_' not in k}
    for t in lora['targets']:
        A = sd[f'{t}.lora_A.{ADAPTER}.weight'].float()
        B = sd[f'{t}.lora_B.{ADAPTER}.weight'].float()
        W = sd[f'{t}.weight']
        out[f'{t}.weight'] = (W.float() + s * (B @ A)).to(W.dtype)
    return out


@torch.no_grad()
def merge_lora(model):
    """fold W += s B A (fp32) into every target, remove the adapters and unfreeze the model: the result has exactly the key set of a
    model that never had adapters (its state dict loads strict=True into a fresh one)"""
    if not has_lora(model):
        raise RuntimeError('the model has no LoRA adapters')
    s = model._lora['scale']
    mods = dict(model.named_modules())
    for t, (A, B) in adapters(model).items():
        W = mods[t]._parameters['weight']
        W.add_((B.float() @ A.float()).mul_(s).to(W.dtype))
        del mods[t]._modules['lora_A'], mods[t]._modules['lora_B']
    for p in model.parameters():
        p.requires_grad_(p.is_floating_point())
    model._lora = None
    _invalidate(model)
    return model


def _target_of(key: str, targets) -> Union[str, None]:
    for t in targets:
        if key.startswith(t + '.'):
            return t
    return None


def lora_state_dict(model, layout: str = 'peft') -> "OrderedDict[str, torch.Tensor]":
    """'peft': what the reference's ``model.state_dict()`` holds after get_peft_model - every key under ``base_model.model.``, each target
    split into ``.base_layer.weight`` / ``.base_layer.bias`` / ``.lora_A.default.weight`` / ``.lora_B.default.weight``.
    'adapter': the adapter tensors only, as peft writes an adapter file (``base_model.model.<target>.lora_A.weight``, no adapter name)."""
    if not has_lora(model):
        raise RuntimeError('the model has no LoRA adapters')
    targets = model._lora['targets']
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in model.state_dict().items():
        t = _target_of(k, targets)
        if layout == 'adapter':
            if t is not None and '.lora_' in k:
                out[PEFT_PREFIX + k.replace(f'.{ADAPTER}.', '.')] = v
        elif layout == 'peft':
            if t is not None and '.lora_' not in k:
                k = t + '.base_layer' + k[len(t):]
            out[PEFT_PREFIX + k] = v
        else:
            raise ValueError(f"layout {layout!r}: 'peft' or 'adapter'")
    return out


def to_module_layout(sd: Mapping[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """peft / adapter-file / DDP key names -> this package's keys (``<target>.weight``, ``<target>.lora_A.default.weight``)"""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for k, v in sd.items():
        if k.startswith('module.'):
            k = k[len('module.'):]
        if k.startswith(PEFT_PREFIX):
            k = k[len(PEFT_PREFIX):]
        k = k.replace('.base_layer.', '.')
        for kind in ('lora_A', 'lora_B'):
            if k.endswith(f'.{kind}.weight'):
                k = k[:-len('weight')] + f'{ADAPTER}.weight'
        out[k] = v
    return out


def load_lora(model, src) -> None:
    """load a LoRA state: the 'peft' layout (whole model, strict), an adapter file ('adapter' layout: adapter tensors only), or this package's
    own state dict - each with or without the DDP ``module.`` prefix; ``src`` is a path or a mapping"""
    if not has_lora(model):
        raise RuntimeError('the model has no LoRA adapters: call add_lora first')
    obj = torch.load(os.fspath(src), map_location='cpu') if isinstance(src, (str, os.PathLike)) else src
    if 'model_state_dict' in obj:
        obj = obj['model_state_dict']
    sd = to_module_layout(obj)
    if all('.lora_' in k for k in sd):
        own = dict(model.named_parameters())
        want = {k for k in own if '.lora_' in k}
        if set(sd) != want:
            raise KeyError(f'adapter state: missing {sorted(want - set(sd))[:4]}, unexpected {sorted(set(sd) - want)[:4]}')
        with torch.no_grad():
            for k, v in sd.items():
                if tuple(v.shape) != tuple(own[k].shape):
                    raise ValueError(f'{k}: shape {tuple(v.shape)} != {tuple(own[k].shape)}')
                own[k].copy_(v)
        _invalidate(model)
    else:
        model.load_state_dict(sd, strict=True)


def trainable_parameters(model) -> Tuple[int, int]:
    """(trainable, total) parameter counts (peft's print_trainable_parameters)"""
    tr = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return tr, sum(p.numel() for p in model.parameters())


def param_groups(model, nowd_keys=None):
    """names, params, groups of the trainable parameters (train.filter_params with trainable_only=True): the adapter weights are 2-D
    ``weight``s, so they land in the decayed group 'D'"""
    from .train import NOWD_KEYS, filter_params
    return filter_params(model, NOWD_KEYS if nowd_keys is None else nowd_keys, trainable_only=True)
