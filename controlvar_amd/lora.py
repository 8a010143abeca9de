"""LoRA fine-tuning (the ``--lora`` option of train_control_var.py:337-353 / train_control_var_hpu.py:449-470 / train_var_hpu.py:306-330).

The reference wraps the transformer with peft (``LoraConfig(r=16, lora_alpha=32, lora_dropout=0.05, bias="none")``) on the modules
its name rule selects; here the adapters are plain parameters of the model under peft's key names, and the training engine runs the
rank-r branch through the HIP kernels of csrc/lora.hip (DESIGN.md "LoRA").  A target computes

    y = x W^T + b + s * (drop(x) A^T) B^T,    s = alpha / r,  A (r, in) ~ U(-1/sqrt(in), 1/sqrt(in)),  B (out, r) = 0

Only A and B train; every other parameter is frozen.  In eval() the adapters are merged into the packed GEMM weights, so inference
runs exactly the adapter-free kernels.

attach_adapters (an addition of this library) is the serving form: a bank of up to 8 adapters beside the unchanged base
weights, one of which every request of a generation batch picks with ``adapter=``.
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
    if getattr(model, '_adapter_bank', None) is not None:
        raise RuntimeError('the model has an adapter bank (attach_adapters): a bank and add_lora on one model are mutually exclusive (detach_adapters first)')
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


# ---- adapter bank: several adapters on one model, chosen per request (an addition of this library) ---------------------
MAX_ADAPTERS = 8                        # slots of one bank (cvar_lora_down_rows: n_slots 1..8)
BANK_KINDS = (('proj', 'attn.proj'), ('fc1', 'ffn.fc1'), ('fc2', 'ffn.fc2'))


def has_adapters(model) -> bool:
    return getattr(model, '_adapter_bank', None) is not None


def _adapter_tensors(src, targets) -> "OrderedDict[str, Tuple[torch.Tensor, torch.Tensor]]":
    """one adapter state (a path or a mapping in any layout load_lora reads) -> target name -> (A (r, in), B (out, r)) in fp32 on the host;
    the base weights of a whole-model layout are not read"""
    obj = torch.load(os.fspath(src), map_location='cpu') if isinstance(src, (str, os.PathLike)) else src
    if 'model_state_dict' in obj:
        obj = obj['model_state_dict']
    sd = {k: v for k, v in to_module_layout(obj).items() if '.lora_' in k}
    want = {f'{t}.lora_{ab}.{ADAPTER}.weight' for t in targets for ab in 'AB'}
    if set(sd) != want:
        raise KeyError(f'adapter state: missing {sorted(want - set(sd))[:4]}, unexpected {sorted(set(sd) - want)[:4]}')
    return OrderedDict((t, (sd[f'{t}.lora_A.{ADAPTER}.weight'].detach().float().cpu(), sd[f'{t}.lora_B.{ADAPTER}.weight'].detach().float().cpu()))
                       for t in targets)


def attach_adapters(model, sources, alpha=32) -> List[str]:
    """Attach a bank of 1..8 LoRA adapters to an adapter-free model, for generation with ``adapter=`` (one adapter id per request of a
    batch; -1 = the base model).  sources: adapter states, each a path or mapping in a layout load_lora reads; their ranks may differ
    (1..16).  alpha: one value or one per adapter; scale = alpha / r.  The bank is no set of parameters: state_dict() is unchanged, and
    calls without ``adapter=`` run exactly the adapter-free launches.  Returns the target names."""
    _check_supported(model)
    if has_lora(model):
        raise RuntimeError('the model has add_lora adapters: a bank and add_lora on one model are mutually exclusive (merge_lora first)')
    if getattr(model, 'gemm_precision', None) is not None:
        from .models import _no_bank_message
        raise NotImplementedError(_no_bank_message(model.gemm_precision))
    sources = list(sources)
    if not 1 <= len(sources) <= MAX_ADAPTERS:
        raise NotImplementedError(f'{len(sources)} adapters: a bank holds 1 .. {MAX_ADAPTERS}')
    alphas = [float(alpha)] * len(sources) if isinstance(alpha, (int, float)) else [float(a) for a in alpha]
    if len(alphas) != len(sources):
        raise ValueError(f'alpha: one value or {len(sources)} values (one per adapter) expected, got {len(alphas)}')
    names = target_names(model)
    mods = dict(model.named_modules())
    adapters_, ranks = [], []
    for k, src in enumerate(sources):
        ad = _adapter_tensors(src, names)
        r = int(next(iter(ad.values()))[0].shape[0])
        if not 1 <= r <= MAX_RANK:
            raise NotImplementedError(f'LoRA rank {r}: the GPU kernels take 1 <= r <= {MAX_RANK}')
        for t, (A, B) in ad.items():
            out_f, in_f = mods[t]._parameters['weight'].shape
            for ab, v, want in (('A', A, (r, in_f)), ('B', B, (out_f, r))):
                if tuple(v.shape) != want:
                    raise ValueError(f'{t}.lora_{ab}.{ADAPTER}.weight: shape {tuple(v.shape)} != {want}')
        adapters_.append(ad)
        ranks.append(r)
    model._adapter_bank = dict(n=len(sources), ranks=ranks, alphas=alphas, scales=[a / r for a, r in zip(alphas, ranks)], targets=list(names),
                               adapters=adapters_, pack=None)
    return names


def detach_adapters(model):
    if not has_adapters(model):
        raise RuntimeError('the model has no adapter bank')
    model._adapter_bank = None
    return model


def bank_kx(n: int, dtype: torch.dtype, groups: int = 1) -> int:
    """columns behind K of an augmented operand: 16 per (slot, group), rounded up to the 128-byte step of train.py (rp)"""
    rp = 128 // torch.tensor([], dtype=dtype).element_size()
    return -(-16 * n * groups // rp) * rp


def pack_bank(bank, P: Mapping[str, Any], C: int, depth: int, dtype: torch.dtype) -> Dict[str, Any]:
    """The device operands of a bank over the packed base weights P (w_proj / w_fc1 / w_fc2 (depth, out, in), w_ada (n_ada, C)), in `dtype`:
       A[kind]   (depth, n, 16, k_in), kind 'ada': (depth + 1, n, 16, C) - rows >= the adapter's rank are zero;
       W[kind]   (depth, out, k_in + kx) = [W | B_0 | ... | B_{n-1} | 0], adapter k in columns k_in + 16 k .. + r_k;
       W['ada']  (n_ada, C + kx_ada) = [W_ada | blockdiag]: target t (block t, then head_nm), slot k in columns C + 16 (t n + k), rows of target t;
       scale     (n,) fp32 = alpha / r."""
    n, dev = bank['n'], P['w_proj'].device
    kx, kxa = bank_kx(n, dtype), bank_kx(n, dtype, depth + 1)
    A, W = {}, {}
    for kind, name in BANK_KINDS:
        w = P['w_' + kind]
        _, n_out, k_in = w.shape
        A[kind] = torch.zeros(depth, n, 16, k_in, device=dev, dtype=dtype)
        W[kind] = torch.zeros(depth, n_out, k_in + kx, device=dev, dtype=dtype)
        W[kind][:, :, :k_in] = w
        for k, (ad, r) in enumerate(zip(bank['adapters'], bank['ranks'])):
            for i in range(depth):
                a, b = ad[f'blocks.{i}.{name}']
                A[kind][i, k, :r] = a.to(device=dev, dtype=dtype)
                W[kind][i, :, k_in + 16 * k:k_in + 16 * k + r] = b.to(device=dev, dtype=dtype)
    tn = [f'blocks.{t}.ada_lin.1' for t in range(depth)] + ['head_nm.ada_lin.1']
    n_ada = P['w_ada'].shape[0]
    A['ada'] = torch.zeros(depth + 1, n, 16, C, device=dev, dtype=dtype)
    W['ada'] = torch.zeros(n_ada, C + kxa, device=dev, dtype=dtype)
    W['ada'][:, :C] = P['w_ada']
    for k, (ad, r) in enumerate(zip(bank['adapters'], bank['ranks'])):
        for t, name in enumerate(tn):
            a, b = ad[name]
            A['ada'][t, k, :r] = a.to(device=dev, dtype=dtype)
            c0 = C + 16 * (t * n + k)
            W['ada'][t * 6 * C:t * 6 * C + b.shape[0], c0:c0 + r] = b.to(device=dev, dtype=dtype)
    return dict(n=n, kx=kx, kxa=kxa, A=A, W=W, scale=torch.tensor(bank['scales'], dtype=torch.float32, device=dev))


def bank_pack(model) -> Dict[str, Any]:
    """pack_bank of the model's bank, built once per base pack"""
    bank = model._adapter_bank
    P = model._pack()
    if bank['pack'] is None or bank['pack'][0] is not P:
        bank['pack'] = (P, pack_bank(bank, P, model.cfg.C, model.cfg.depth, model.compute_dtype))
    return bank['pack'][1]


def adapter_ids(adapter, B: int, n: int):
    """``adapter=`` of a generation call -> (B,) int32 numpy array: one int (broadcast) or a length-B sequence / tensor of ints in [-1, n)"""
    import numpy as np
    a = adapter.detach().cpu().numpy() if torch.is_tensor(adapter) else np.asarray(adapter)
    if a.dtype == object or a.dtype.kind not in 'iu':
        raise ValueError(f'adapter: integers expected, got {a.dtype}')
    if a.ndim == 0:
        a = np.broadcast_to(a, (B,))
    if a.shape != (B,):
        raise ValueError(f'adapter: one integer or shape ({B},) (one per batch row) expected, got {a.shape}')
    if (a < -1).any() or (a >= n).any():
        raise ValueError(f'adapter: id out of range - {n} adapter(s) attached, ids -1 (the base model) .. {n - 1} expected, got {sorted(set(a.tolist()))}')
    return np.ascontiguousarray(a.astype(np.int32))


def sequence_slots(ids, nrep: int):
    """request ids (B,) -> the slot of every sequence of the batch (nrep * B,): the CFG rows are laid out branch-major ([cond ; uncond],
    row = branch * B + b), and every branch of a request uses the request's adapter"""
    import numpy as np
    return np.tile(np.asarray(ids, dtype=np.int32), nrep)


def merged_adapter_state(sd: Mapping[str, torch.Tensor], bank, k: int) -> Dict[str, torch.Tensor]:
    """state dict of the base model with adapter k of the bank folded in (W + s B A in fp32): what merge_lora gives for that adapter alone"""
    out = dict(sd)
    s = bank['scales'][k]
    for t, (A, B) in bank['adapters'][k].items():
        W = sd[f'{t}.weight']
        out[f'{t}.weight'] = (W.float() + s * (B.to(W.device) @ A.to(W.device))).to(W.dtype)
    return out


def trainable_parameters(model) -> Tuple[int, int]:
    """(trainable, total) parameter counts (peft's print_trainable_parameters)"""
    tr = sum(p.numel() for p in model.parameters() if p.requires_grad)
    return tr, sum(p.numel() for p in model.parameters())


def param_groups(model, nowd_keys=None):
    """names, params, groups of the trainable parameters (train.filter_params with trainable_only=True): the adapter weights are 2-D
    ``weight``s, so they land in the decayed group 'D'"""
    from .train import NOWD_KEYS, filter_params
    return filter_params(model, NOWD_KEYS if nowd_keys is None else nowd_keys, trainable_only=True)
