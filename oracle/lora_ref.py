"""ORACLE (test infrastructure only - never imported by the product path).

LoRA adapter branch (controlvar_amd/lora.py, csrc/lora.hip) restated on the host:

* the dropout keep mask of (seed, tag, row, column), written in numpy uint32 arithmetic from the hash of csrc/lora.hip
  (lora_mix, lora_key, lora_row_key, lora_keep) - an independent copy, so a change of the device hash changes what the
  tests expect instead of moving the tests' source of truth along with it;
* LoraTerm, the adapter term s * (drop(x) A^T) B^T that the functional oracle (oracle.var_ref) adds inside each target
  linear when it is handed one, with the engine's mask addressing.
"""
from __future__ import annotations

import re
from typing import Dict, Mapping, Tuple

import numpy as np
import torch

_U32 = np.uint32
KINDS = ('proj', 'fc1', 'fc2', 'ada')            # tag = 4 * layer + kind index; head_nm.ada_lin.1 is layer `depth`


def mix(h):
    """lora_mix: the 32-bit finaliser (every product wraps modulo 2^32)"""
    h = np.asarray(h, dtype=_U32)
    with np.errstate(over='ignore'):
        h = h ^ (h >> _U32(16))
        h = h * _U32(0x7feb352d)
        h = h ^ (h >> _U32(15))
        h = h * _U32(0x846ca68b)
        h = h ^ (h >> _U32(16))
    return h


def key(seed: int, tag: int) -> np.uint32:
    """lora_key: low 32 bits of the uint64 seed, then the high 32 bits, then the tag"""
    seed = int(seed) & (2 ** 64 - 1)
    tag = int(tag) & 0xffffffff
    h = mix(_U32(seed & 0xffffffff) ^ _U32(0x9e3779b9))
    h = mix(h ^ _U32(seed >> 32))
    with np.errstate(over='ignore'):
        t = np.asarray(tag, dtype=_U32) * _U32(0x85ebca6b) + _U32(0x632be5ab)
    return mix(h ^ t)


def row_keys(k, rows) -> np.ndarray:
    """lora_row_key for every row index in `rows`"""
    with np.errstate(over='ignore'):
        return mix(_U32(k) ^ (np.asarray(rows, dtype=np.int64).astype(_U32) * _U32(0xc2b2ae35)))


def thresh(p: float) -> int:
    """min(trunc(double(float32(p)) * 2^32), 2^32 - 1): the float32 cast of p is part of the definition"""
    t = float(np.float32(p)) * 4294967296.0
    return 0xffffffff if t >= 4294967295.0 else int(t)


def inv_keep(p: float) -> float:
    """the factor a kept element is multiplied by: 1.0f / (1.0f - p) in fp32 (1 when p == 0)"""
    p32 = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p32)) if p32 > 0 else 1.0


def keep_mask(M: int, K: int, p: float, seed: int, tag: int) -> np.ndarray:
    """(M, K) bool: element (m, k) of target `tag` is kept (lora_keep(lora_row_key(key, m), k, thresh))"""
    rk = row_keys(key(seed, tag), np.arange(M))
    cols = np.arange(K, dtype=np.int64).astype(_U32)
    with np.errstate(over='ignore'):
        h = mix(rk[:, None] + cols[None, :] * _U32(0x9e3779b9))
    return h >= _U32(thresh(p))


def drop_factor(M: int, K: int, p: float, seed: int, tag: int) -> torch.Tensor:
    """(M, K) float64 factor of inverted dropout: inv_keep(p) where kept, 0 where dropped (all ones at p == 0)"""
    if np.float32(p) <= 0:
        return torch.ones(M, K, dtype=torch.float64)
    return torch.from_numpy(np.where(keep_mask(M, K, p, seed, tag), inv_keep(p), 0.0))


def target_tag(name: str, depth: int) -> int:
    """the engine's tag of a target name (controlvar_amd/train.py TrainEngine._tag)"""
    if name == 'head_nm.ada_lin.1':
        return 4 * depth + 3
    m = re.fullmatch(r'blocks\.(\d+)\.(attn\.proj|ffn\.fc1|ffn\.fc2|ada_lin\.1)', name)
    if m is None:
        raise KeyError(f'not a LoRA target: {name}')
    kind = {'attn.proj': 'proj', 'ffn.fc1': 'fc1', 'ffn.fc2': 'fc2', 'ada_lin.1': 'ada'}[m.group(2)]
    return 4 * int(m.group(1)) + KINDS.index(kind)


class LoraTerm:
    """hook(name, x) -> s * (drop(x) A^T) B^T of target `name`, shaped like x with the last dimension N.

    x is the target linear's input as the oracle holds it: (B, L, K) for a block target (mask row b * L + l) or (B, K) for an
    adaLN generator (mask row b).  A and B are fresh leaf tensors (requires_grad) of the given dtype, so a backward through
    the oracle leaves the adapter gradients on them: `grads()` returns them under peft's key names."""

    def __init__(self, adapters: Mapping[str, Tuple[torch.Tensor, torch.Tensor]], scale: float, p: float = 0.0, seed: int = 0,
                 dtype: torch.dtype = torch.float32):
        self.scale, self.p, self.seed = float(scale), float(p), int(seed)
        self.depth = sum(1 for t in adapters if t.endswith('attn.proj'))
        self.A = {t: A.detach().cpu().to(dtype).clone().requires_grad_(True) for t, (A, _) in adapters.items()}
        self.B = {t: B.detach().cpu().to(dtype).clone().requires_grad_(True) for t, (_, B) in adapters.items()}

    def params(self) -> Dict[str, torch.Tensor]:
        out = {}
        for t in self.A:
            out[f'{t}.lora_A.default.weight'] = self.A[t]
            out[f'{t}.lora_B.default.weight'] = self.B[t]
        return out

    def grads(self) -> Dict[str, torch.Tensor]:
        return {k: v.grad for k, v in self.params().items()}

    def __call__(self, name: str, x: torch.Tensor) -> torch.Tensor:
        A, B = self.A[name], self.B[name]
        K = x.shape[-1]
        rows = x.reshape(-1, K)
        if self.p > 0:
            rows = rows * drop_factor(rows.shape[0], K, self.p, self.seed, target_tag(name, self.depth)).to(rows.dtype)
        u = self.scale * (rows @ A.to(rows.dtype).t())
        return (u @ B.to(rows.dtype).t()).reshape(*x.shape[:-1], B.shape[0])
