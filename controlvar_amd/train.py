"""Host-side training logic of the hot path.

* lr_wd_annealing / filter_params: restated from utils/lr_control.py:10-101 (per-step LR / weight-decay schedule and
  the decay / no-decay parameter split of train_control_var_hpu.py:609-615);
* Trainer: the step of train_control_var_hpu.py:157-250 over the HIP kernels (tokenise -> interleave -> teacher-forced
  forward -> fused cross-entropy -> hand-written backward -> gradient all-reduce -> clip -> fused AdamW).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

NOWD_KEYS = ('cls_token', 'start_token', 'task_token', 'cfg_uncond', 'pos_embed', 'pos_1LC', 'pos_start', 'start_pos', 'lvl_embed',
             'gamma', 'beta', 'ada_gss', 'moe_bias', 'scale_mul')          # train_control_var_hpu.py:609-615


def lr_wd_factors(sche_type: str, peak_lr: float, wd: float, wd_end: float, cur_it: int, wp_it: float, max_it: int,
                  wp0: float = 0.005, wpe: float = 0.001) -> Tuple[float, float]:
    """(lr, weight_decay) of iteration cur_it  (utils/lr_control.py:10-48)."""
    wp_it = round(wp_it)
    if cur_it < wp_it:
        cur = wp0 + (1 - wp0) * cur_it / wp_it
    else:
        pasd = (cur_it - wp_it) / (max_it - 1 - wp_it)
        rest = 1 - pasd
        if sche_type == 'cos':
            cur = wpe + (1 - wpe) * (0.5 + 0.5 * math.cos(math.pi * pasd))
        elif sche_type == 'lin':
            T = 0.15
            cur = 1 if pasd < T else wpe + (1 - wpe) * rest / (1 - T)
        elif sche_type == 'lin0':
            T = 0.05
            cur = 1 if pasd < T else wpe + (1 - wpe) * rest / (1 - T)
        elif sche_type == 'lin00':
            cur = wpe + (1 - wpe) * rest
        elif sche_type.startswith('lin'):
            T = float(sche_type[3:])
            max_rest = 1 - T
            wpe_mid = (1 + (wpe + (1 - wpe) * max_rest)) / 2
            cur = 1 + (wpe_mid - 1) * pasd / T if pasd < T else wpe + (wpe_mid - wpe) * rest / max_rest
        elif sche_type == 'exp':
            T = 0.15
            cur = 1 if pasd < T else math.exp((pasd - T) / (1 - T) * math.log(wpe))
        else:
            raise NotImplementedError(f'unknown sche_type {sche_type}')
    lr = cur * peak_lr
    pasd = cur_it / (max_it - 1)
    cur_wd = wd_end + (wd - wd_end) * (0.5 + 0.5 * math.cos(math.pi * pasd))
    return lr, cur_wd


def lr_wd_annealing(sche_type: str, optimizer, peak_lr, wd, wd_end, cur_it, wp_it, max_it, wp0=0.005, wpe=0.001):
    """Drop-in of utils/lr_control.py:10-64 for anything with torch-style ``param_groups`` (returns min/max lr, min/max wd)."""
    lr, cur_wd = lr_wd_factors(sche_type, peak_lr, wd, wd_end, cur_it, wp_it, max_it, wp0, wpe)
    inf = 1e6
    min_lr, max_lr, min_wd, max_wd = inf, -1, inf, -1
    for g in optimizer.param_groups:
        g['lr'] = lr * g.get('lr_sc', 1)
        max_lr, min_lr = max(max_lr, g['lr']), min(min_lr, g['lr'])
        g['weight_decay'] = cur_wd * g.get('wd_sc', 1)
        max_wd = max(max_wd, g['weight_decay'])
        if g['weight_decay'] > 0:
            min_wd = min(min_wd, g['weight_decay'])
    if min_lr == inf:
        min_lr = -1
    if min_wd == inf:
        min_wd = -1
    return min_lr, max_lr, min_wd, max_wd


def decays(name: str, ndim: int, nowd_keys: Iterable[str] = NOWD_KEYS) -> bool:
    """True if the parameter is weight-decayed (utils/lr_control.py:84-87)."""
    return not (ndim == 1 or name.endswith('bias') or any(k in name for k in nowd_keys))


def filter_params(model, nowd_keys: Iterable[str] = NOWD_KEYS, trainable_only: bool = False):
    """names, params, [group 'D' (wd_sc 1), group 'ND' (wd_sc 0)] in first-seen order (utils/lr_control.py:67-101).
    trainable_only=True (LoRA, controlvar_amd/lora.py): frozen parameters are skipped instead of failing the reference's assert."""
    groups: Dict[str, dict] = {}
    names, paras = [], []
    for name, p in model.named_parameters():
        name = name.replace('_fsdp_wrapped_module.', '')
        if not p.requires_grad:
            if trainable_only:
                continue
            raise AssertionError(f'frozen parameter {name}')
        names.append(name)
        paras.append(p)
        gname = 'D' if decays(name, p.ndim, nowd_keys) else 'ND'
        groups.setdefault(gname, {'params': [], 'wd_sc': 1.0 if gname == 'D' else 0.0, 'lr_sc': 1.0})['params'].append(p)
    return names, paras, list(groups.values())


class AccumWindow:
    """Bookkeeping of gradient accumulation, accelerate's semantics (`accelerator.accumulate`, train.py:105 / train_var.py:112 /
    train_control_var.py:130 of the reference): a window is n consecutive micro-batches, each with its own loss; the optimizer sees
    (1 / n) * sum_k grad(loss_k) - micro-batches are NOT sample-weighted - and steps once, in the call that closes the window.
    Plain Python (no device work): Trainer.step asks `begin()` what this call is and reports back with `end()`."""

    def __init__(self, n: int = 1):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f'grad_accum must be an integer >= 1 (micro-batches per optimizer step), got {n!r}')
        self.n = n
        self.micro = 0              # index of the next micro-batch inside its window
        self.it = 0                 # optimizer steps taken = closed windows (what the lr / wd schedule counts, as accelerator.sync_gradients does)

    def begin(self) -> Tuple[int, bool, bool]:
        """-> (micro, accumulate, sync) of the call that starts now: the first micro-batch of a window overwrites the gradient
        buffers, the later ones add to them; the last one reduces, steps the optimizer and closes the window"""
        return self.micro, self.micro > 0, self.micro == self.n - 1

    def end(self) -> bool:
        """the call is done; -> whether it closed a window (it then counted one optimizer step)"""
        if self.micro == self.n - 1:
            self.micro = 0
            self.it += 1
            return True
        self.micro += 1
        return False

    @staticmethod
    def grad_scale(world: int, n: int) -> float:
        """the gradient buffers hold the SUM over the window's micro-batches and, after the all-reduce, over the ranks: the mean over both
        is folded into the optimizer's gradient scale (clip coefficient and AdamW alike)"""
        return 1.0 / (world * n)


# =====================================================================================
# Training engine (GPU): forward with saved activations, hand-written backward, fused optimizer
# =====================================================================================
import torch  # noqa: E402

from . import ops  # noqa: E402
from ._lib import ACT_GELU_GRAD, ACT_GELU_TANH, ACT_NONE  # noqa: E402
from .spec import attention_levels  # noqa: E402


def _pad8(n: int) -> int:
    return (n + 7) // 8 * 8


@dataclass
class PolicyLoss:
    """The clipped policy-gradient loss of a training step on token ids (cvar_pg_fwd_bwd, include/cvar_policy.h), in the place of
    the cross-entropy: per token, with lp its log-probability under the model being trained,
        ratio = exp(lp - old_logprob),  loss = -min(ratio * A, clamp(ratio, 1 - clip[0], 1 + clip[1]) * A) + kl_coef * k3(ref_logprob - lp).
    advantages   (B,) - one per sample, broadcast over its tokens - or (B, L), signed;
    old_logprob  (B, L) log-probabilities of the policy the tokens were drawn from (Trainer.token_logprobs); None: the ratio is exactly 1
                 and nothing clips - REINFORCE with the advantage as the token weight;
    ref_logprob  (B, L) log-probabilities of the frozen reference policy of the KL term; None: no KL term (kl_coef must then be 0);
    clip         (below, above) >= 0, or one number for both.
    (B, L) tensors are in the token order of the training labels: per scale the two halves, control first when mask_first (TokenScores).
    Everything is checked on the host when the object is built and, against the batch, by rows()."""
    advantages: torch.Tensor
    old_logprob: Optional[torch.Tensor] = None
    ref_logprob: Optional[torch.Tensor] = None
    clip: Tuple[float, float] = (0.2, 0.2)
    kl_coef: float = 0.0

    def __post_init__(self):
        clip = self.clip
        if isinstance(clip, (int, float)) and not isinstance(clip, bool):
            clip = (clip, clip)
        if (not isinstance(clip, (tuple, list)) or len(clip) != 2
                or not all(isinstance(c, (int, float)) and not isinstance(c, bool) and math.isfinite(c) and c >= 0 for c in clip)):
            raise ValueError(f'clip={self.clip!r}: two finite numbers >= 0 (below, above), or one for both')
        self.clip = (float(clip[0]), float(clip[1]))
        k = self.kl_coef
        if isinstance(k, bool) or not isinstance(k, (int, float)) or not math.isfinite(k) or k < 0:
            raise ValueError(f'kl_coef={k!r}: a finite number >= 0')
        self.kl_coef = float(k)
        if self.kl_coef > 0 and self.ref_logprob is None:
            raise ValueError('kl_coef > 0 needs ref_logprob: the KL term is taken against a reference policy (Trainer.token_logprobs before the first update)')
        for name in ('advantages', 'old_logprob', 'ref_logprob'):
            t = getattr(self, name)
            if t is None and name != 'advantages':
                continue
            if not torch.is_tensor(t) or not t.is_floating_point():
                raise ValueError(f'{name}: expected a floating-point tensor, got {type(t).__name__ if not torch.is_tensor(t) else t.dtype}')
            if t.dim() not in ((1, 2) if name == 'advantages' else (2,)):
                raise ValueError(f'{name}: expected {"(B,) or (B, L)" if name == "advantages" else "(B, L)"}, got {tuple(t.shape)}')

    def check(self, B: int, L: int):
        """the shapes against a batch of B samples of L tokens (host only)"""
        for name in ('advantages', 'old_logprob', 'ref_logprob'):
            t = getattr(self, name)
            ok = ((B,), (B, L)) if name == 'advantages' else ((B, L),)
            if t is not None and tuple(t.shape) not in ok:
                raise ValueError(f'{name}: expected shape {" or ".join(str(o) for o in ok)}, got {tuple(t.shape)}')

    def rows(self, B: int, L: int, device=None):
        """-> (advantages, old_logprob or None, ref_logprob or None), each (B * L,) fp32 contiguous on `device`, advantages broadcast"""
        self.check(B, L)
        out = []
        for name in ('advantages', 'old_logprob', 'ref_logprob'):
            t = getattr(self, name)
            if t is None:
                out.append(None)
                continue
            t = t.to(device=device, dtype=torch.float32)
            if t.dim() == 1:
                t = t[:, None].expand(B, L)
            out.append(t.contiguous().view(-1))
        return tuple(out)


_NO_SEPARATOR = ('training on token ids: separator models are not offered (their label row carries special tokens between the '
                 'halves, which the (B, L) token layout does not hold)')


@dataclass
class DistillLoss:
    """The soft-target loss of a training step on token ids (cvar_kd_fwd_bwd, include/cvar_distill.h), in the place of the
    cross-entropy: per token KL(softmax(teacher logits) || model), with gradient (p - q) * weight * gscale in the model's logits.
    logits   (B, L, V) fp32 on the device: the teacher's logits of every token - for guidance distillation the guided combination
             sum_k coef_k * logits_k a generation call returns as DistillTargets.logits - V == cfg.vocab;
    weights  (B, L) token weights, or None = 1; they take ignore_mask's place (loss normalisation included), so the two exclude each other.
    Both are in the token order of the training labels: per scale the two halves, control first when mask_first (TokenScores).
    A student is trained with cond_drop_rate = 0: it learns the guided distribution of the condition it is given, and a dropped condition
    would pair the teacher's guided row with an unconditional student row.
    The types are checked on the host when the object is built, the shapes against the batch by check()."""
    logits: torch.Tensor
    weights: Optional[torch.Tensor] = None

    def __post_init__(self):
        t = self.logits
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f'logits: expected a float32 tensor, got {type(t).__name__ if not torch.is_tensor(t) else t.dtype}')
        if t.dim() != 3:
            raise ValueError(f'logits: expected (B, L, V), got {tuple(t.shape)}')
        w = self.weights
        if w is not None:
            if not torch.is_tensor(w) or w.dtype not in (torch.bool, torch.float32, torch.float64, torch.bfloat16, torch.float16):
                raise ValueError(f'weights: expected a floating-point or bool tensor, got {type(w).__name__ if not torch.is_tensor(w) else w.dtype}')
            if w.dim() != 2:
                raise ValueError(f'weights: expected (B, L), got {tuple(w.shape)}')

    def check(self, B: int, L: int, V: int, device=None):
        """the shapes (and the device) against a batch of B samples of L tokens over V classes (host only)"""
        if tuple(self.logits.shape) != (B, L, V):
            raise ValueError(f'logits: expected shape {(B, L, V)}, got {tuple(self.logits.shape)}')
        if device is not None and self.logits.device.type != torch.device(device).type:
            raise ValueError(f'logits: expected on {device}, got {self.logits.device} (teacher logits are not copied between devices)')
        if self.weights is not None and tuple(self.weights.shape) != (B, L):
            raise ValueError(f'weights: expected shape {(B, L)}, got {tuple(self.weights.shape)}')


@dataclass
class SparseDistillLoss:
    """The sparse form of DistillLoss (cvar_kd_topn_fwd_bwd, include/cvar_topn.h): the teacher of every token as its N most likely
    codes, their log-probabilities and the log of the mass of all the other codes - what TokenScores carries under top_logprobs=N, and 63 times
    smaller than the dense logits at N = 32.  The loss per token is KL(teacher || model) over the N + 1 cells {id_0}, .., {id_N-1}, {the rest}.
    top_ids       (B, L, N) int32 on the device, 1 <= N <= 64; an entry < 0 is unused, the others are distinct per token and < cfg.vocab
    top_logprobs  (B, L, N) fp32
    tail_logprob  (B, L) fp32 or None: None or -inf = no tail mass
    weights       (B, L) token weights, or None = 1; they take ignore_mask's place, as DistillLoss.weights do.
    All in the token order of the training labels (TokenScores).  The types are checked on the host when the object is built, the shapes
    against the batch by check(); distinct ids are the caller's contract (cvar_score_topn's output has them)."""
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor
    tail_logprob: Optional[torch.Tensor] = None
    weights: Optional[torch.Tensor] = None

    def __post_init__(self):
        for name, t, dtype, dim, shape in (('top_ids', self.top_ids, torch.int32, 3, '(B, L, N)'), ('top_logprobs', self.top_logprobs, torch.float32, 3, '(B, L, N)'),
                                           ('tail_logprob', self.tail_logprob, torch.float32, 2, '(B, L)')):
            if t is None and name == 'tail_logprob':
                continue
            if not torch.is_tensor(t) or t.dtype != dtype:
                raise ValueError(f'{name}: expected {"an" if dtype == torch.int32 else "a"} {str(dtype)[6:]} tensor, got '
                                 f'{type(t).__name__ if not torch.is_tensor(t) else t.dtype}')
            if t.dim() != dim:
                raise ValueError(f'{name}: expected {shape}, got {tuple(t.shape)}')
        if tuple(self.top_ids.shape) != tuple(self.top_logprobs.shape):
            raise ValueError(f'top_ids and top_logprobs: one shape (B, L, N), got {tuple(self.top_ids.shape)} and {tuple(self.top_logprobs.shape)}')
        if not 1 <= self.top_ids.shape[2] <= 64:
            raise ValueError(f'top_ids: N = {self.top_ids.shape[2]} listed codes per token, 1 to 64 are offered')
        w = self.weights
        if w is not None:
            if not torch.is_tensor(w) or w.dtype not in (torch.bool, torch.float32, torch.float64, torch.bfloat16, torch.float16):
                raise ValueError(f'weights: expected a floating-point or bool tensor, got {type(w).__name__ if not torch.is_tensor(w) else w.dtype}')
            if w.dim() != 2:
                raise ValueError(f'weights: expected (B, L), got {tuple(w.shape)}')

    @property
    def N(self) -> int:
        return int(self.top_ids.shape[2])

    def check(self, B: int, L: int, V: int, device=None):
        """the shapes (and the device) against a batch of B samples of L tokens over V classes (host only; the ids' range is the kernel's
        contract: an id >= V counts as unused)"""
        if tuple(self.top_ids.shape[:2]) != (B, L):
            raise ValueError(f'top_ids: expected shape {(B, L, self.N)}, got {tuple(self.top_ids.shape)}')
        if self.tail_logprob is not None and tuple(self.tail_logprob.shape) != (B, L):
            raise ValueError(f'tail_logprob: expected shape {(B, L)}, got {tuple(self.tail_logprob.shape)}')
        if device is not None:
            for name, t in (('top_ids', self.top_ids), ('top_logprobs', self.top_logprobs), ('tail_logprob', self.tail_logprob)):
                if t is not None and t.device.type != torch.device(device).type:
                    raise ValueError(f'{name}: expected on {device}, got {t.device} (teacher targets are not copied between devices)')
        if self.weights is not None and tuple(self.weights.shape) != (B, L):
            raise ValueError(f'weights: expected shape {(B, L)}, got {tuple(self.weights.shape)}')


_DISTILL_FORMS = (DistillLoss, SparseDistillLoss)


def _ln_rows(C: int):
    """the adaLN forward of rows of C channels: above 2048 the entry point of include/cvar_wide.h; narrow models call ops.ln_modulate exactly as before"""
    return ops.ln_modulate_wide if C > 2048 else ops.ln_modulate


_MODS = dict(qkv='attn.mat_qkv', proj='attn.proj', fc1='ffn.fc1', fc2='ffn.fc2')          # linear of a block -> its module name in the state dict


class TrainEngine:
    """Teacher-forced forward + backward of ControlVAR / VAR over the HIP kernels (control_var.py:568-651 under autograd).

    Activations of every block are kept in HBM (288 GB: no recomputation).  Weight gradients are produced by the same
    MFMA GEMM as the forward on transposed operands (activations are transposed into zero-padded [N][Mpad] buffers),
    accumulated in fp32 into per-layer contiguous slabs so that each layer's slab can be all-reduced as soon as its
    backward is done (bucket = layer, overlapped with the rest of the backward on a side stream).

    One walk serves the full model and a LoRA model (controlvar_amd/lora.py).  The walk owns the order of a block - adaLN, qkv,
    cos-norm, attention, proj, adaLN, fc1, fc2 forward; gated_grad, the four data-gradient GEMMs, the three ln_modulate_bwd,
    attention_bwd, cos_qk_norm_bwd and reducer.ready(i) backward - with every epilogue and offset written once.  A mode supplies
    * its set of buffers in `_setup`, with `Xin`: linear -> (saved input (depth, M, ld), row stride ld; 0 = dense rows), where the forward
      leaves the operand of a linear and the backward finds it again;
    * the forward leaf that launches a linear (`ops.gemm` on the packed weight; `_lora_linear`);
    * the backward leaf that follows a data-gradient GEMM (`_full_grads_of`: the weight and bias gradient; `_lora_grads_of`: du, the
      branch's share of dx, dB, dA);
    * its generator tail (`_ada_grads_full`, then `_embedding_grads`; `_ada_grads_lora`) and its gradient layout in `_setup_grads`:
      `grad_views`, state_dict key -> (buffer, offset, shape), which `grads()` turns into views.
    What only the full model has is said where it happens: GELU' fused into fc2's data-gradient GEMM, the parameter gradients of qkv
    and head, colsum(DSM), the embedding tail.

    Gradient accumulation: ``forward_backward(..., accumulate=True)`` adds this micro-batch's gradient to what
    ``grads()`` holds - every element becomes fp32(old + plain), `plain` being the bits the non-accumulating call produces - so a
    window of micro-batches leaves their sum in micro-batch order.  The gradient buffers are allocated once per engine and do not
    depend on the batch size: the micro-batches of a window may differ in size.
    """

    def __init__(self, var, drop_path: bool = True, reducer=None):
        self.var = var
        self.cfg = cfg = var.cfg
        self.drop_path = drop_path
        self.reducer = reducer
        self._B = None
        self._wt_gen = -1
        self._lora = None
        self._grads_key = None          # what the gradient buffers were allocated for: 'full' or ('lora', id of the LoRA state)
        self._staging = {}              # accumulating backward: fp32 staging buffers by name (_stage)
        # the dimensions every method needs; those of a batch (M, Mp, Bp) and of a LoRA state (r, rp, Kx, kc, kh) are set by _setup
        self.C, self.depth, self.V, self.L = cfg.C, cfg.depth, cfg.head_ld, cfg.pyramid.L      # head columns incl. separator labels, padded to 8 (spec.VarConfig.head_ld)
        self.hid = round(cfg.C * cfg.mlp_ratio)
        self.ah = cfg.depth * 6 * cfg.C                                                        # the head's rows of the adaLN generator
        self.n_ada = self.ah + 2 * cfg.C
        self.ncode = len(cfg.pyramid.code_positions()) - cfg.pyramid.first_l                   # teacher-forcing tokens per sample (separators excluded)
        self.lvl_end, self.holes = attention_levels(cfg)
        self.scale, self.eps = float(cfg.attn_scale), cfg.norm_eps

    # ---------------------------------------------------------------- buffers
    def _setup(self, B: int):
        """the buffers of batch size B: what both modes have, and in its place the mode's own set.  LoRA: the base weights are
        frozen, so nothing of their weight gradients exists (TA / TB, the slabs); the operand of each adapted linear is kept K-augmented,
        [x | u | 0] with u = s drop(x) A^T and zero padding up to a 128-byte row step."""
        cfg, var = self.cfg, self.var
        lora = getattr(var, '_lora', None)
        if lora is None and self._lora is not None:                   # the adapters were merged away: back to the full path
            self._lora, self._B = None, None
        key = B if lora is None else (B, id(lora))
        if self._B == key:
            return
        dev, T = var.device, var.compute_dtype
        C, depth, V, L, hid, n_ada = self.C, self.depth, self.V, self.L, self.hid, self.n_ada
        M = B * L
        self.M, self.Mp, self.Bp = M, _pad8(M), _pad8(B)
        self.Xin = {}                                                 # the old plan's references go with its buffers
        f32 = dict(device=dev, dtype=torch.float32)
        tT = dict(device=dev, dtype=T)
        if lora is not None:
            rp = 128 // torch.tensor([], dtype=T).element_size()      # augmented K step: keeps cvar_gemm on its K-multiple-of-128-bytes path
            self._lora, self.r, self.rp = lora, lora['r'], rp
            self.Kx = -(-(depth + 1) * 16 // rp) * rp                 # [cs | u_0 ... u_depth] columns beyond C
            self.kc, self.kh = kc, kh = C + rp, hid + rp
        # saved activations
        self.Xs = torch.empty(depth + 1, M, C, **f32)
        self.X1s = torch.empty(depth, M, C, **f32)
        self.U = torch.empty(depth, M, C, **tT); self.O = torch.empty(depth, M, C, **tT)
        self.F1 = torch.empty(depth, M, C, **tT)
        if lora is None:
            self.U2 = torch.empty(depth, M, C, **tT)
        else:                                                         # fc1's input is kept in its augmented buffer: one (M, C) scratch serves every layer
            self.U2 = torch.empty(M, C, **tT).expand(depth, M, C)
        self.F2 = torch.empty(depth, M, C, **tT)
        if lora is None:
            self.A = torch.empty(depth, M, hid, **tT); self.Hh = torch.empty(depth, M, hid, **tT)
            self.Xin = dict(qkv=(self.U, 0), proj=(self.O, 0), fc1=(self.U2, 0), fc2=(self.Hh, 0))
        else:
            Oa = torch.zeros(depth, M, kc, **tT)                      # [o | u_proj | 0]
            U2a = torch.zeros(depth, M, kc, **tT)                     # [u2 | u_fc1 | 0]
            self.Hh = torch.zeros(depth, M, kh, **tT)                 # [gelu(a) | u_fc2 | 0]
            self.A = torch.empty(depth, M, kh, **tT)                  # fc1 pre-activation (row stride of the fc1 output)
            self.csa = torch.zeros(B, C + self.Kx, **tT)
            self.Xin = dict(proj=(Oa, kc), fc1=(U2a, kc), fc2=(self.Hh, kh), ada=(self.csa[None], C + self.Kx))
        self.arena = torch.empty(depth, B, L, 3 * C, **tT)
        self.LSE = torch.empty(depth, B, cfg.H, L, **f32)
        self.NORMS = torch.empty(depth, B, L, cfg.H, 2, **f32) if cfg.uses_cos_attn else None
        self.DSM = torch.empty(M, cfg.H, **f32) if cfg.uses_cos_attn else None
        self.UH = torch.empty(M, C, **tT)
        self.logits = torch.empty(M, V, **f32)
        self.loss_tok = torch.empty(M, **f32)
        # backward work buffers
        self.dlogits = torch.empty(M, V, **tT)
        self.dX = torch.empty(M, C, **f32)
        self.DF = torch.empty(M, C, **tT); self.DU = torch.empty(M, C, **tT)
        self.DH = torch.empty(M, hid, **tT)
        self.DQKV = torch.empty(B, L, 3 * C, **tT)
        if lora is None:
            nmax = max(hid, 3 * C, V)
            self.TA = torch.zeros(nmax * self.Mp, **tT)               # zero padding columns stay zero
            self.TB = torch.zeros(nmax * self.Mp, **tT)
            self.TA32 = torch.zeros(C * _pad8(B * self.ncode), **f32)
            self.TB32 = torch.zeros(cfg.cvae * _pad8(B * self.ncode), **f32)
        else:
            self.DUr = torch.empty(M, 16, **tT)
            self.DUa = torch.empty(B, 16, **tT)
        self.dada = torch.zeros(B, n_ada, **f32)
        self.ws = torch.empty(max(ops.train_ws_floats(M, B, C), 64 * max(hid, 3 * C, V, n_ada), L * C, B * cfg.H * L,
                                  6 * C * C if cfg.shared_aln else 0) + 16, **f32)
        if lora is not None:
            self.lws = torch.empty(max(ops.lora_wgrad_ws_floats(M, hid), ops.lora_wgrad_ws_floats(M, C), ops.lora_wgrad_ws_floats(B, 6 * C)), **f32)
            self._aug = None
        self._setup_grads(lora)
        self._B = key
        self._transposed_weights()

    def _setup_grads(self, lora=None):
        """gradient buffers and their layout: once per engine (full model) or per adapter state (LoRA), whatever the batch size (a window of
        micro-batches accumulates into them).  The layout is declared here alone: `grad_views`, state_dict key -> (buffer, offset, shape)."""
        key = 'full' if lora is None else ('lora', id(lora))
        if self._grads_key == key:
            return
        cfg = self.cfg
        C, depth, V, L, hid, n_ada, ah, H = self.C, self.depth, self.V, self.L, self.hid, self.n_ada, self.ah, cfg.H
        f32 = dict(device=self.var.device, dtype=torch.float32)
        views = {}
        if lora is None:
            # gradient slabs: [layer][w_qkv | w_proj | w_fc1 | w_fc2 | b_qkv | b_proj | b_fc1 | b_fc2 | scale_mul]
            self.slab_off, o = {}, 0
            for name, n in (('w_qkv', 3 * C * C), ('w_proj', C * C), ('w_fc1', hid * C), ('w_fc2', C * hid), ('b_qkv', 3 * C), ('b_proj', C),
                            ('b_fc1', hid), ('b_fc2', C), ('scale_mul', _pad8(H))):
                self.slab_off[name] = o
                o += n
            self.slab = o
            self.G_layers = torch.zeros(depth, self.slab, **f32)
            self.G_ada = torch.zeros(n_ada * C + n_ada, **f32)                       # [w_ada | b_ada]: 6C rows of each per block, then the head's 2C
            # (key in the block, slab entry, offset in it, shape); the k-bias third of b_qkv has no key (zero_k_bias is a buffer)
            layer = [(_MODS['qkv'] + '.weight', 'w_qkv', 0, (3 * C, C)), (_MODS['proj'] + '.weight', 'w_proj', 0, (C, C)),
                     (_MODS['fc1'] + '.weight', 'w_fc1', 0, (hid, C)), (_MODS['fc2'] + '.weight', 'w_fc2', 0, (C, hid)),
                     ('attn.q_bias', 'b_qkv', 0, (C,)), ('attn.v_bias', 'b_qkv', 2 * C, (C,)), (_MODS['proj'] + '.bias', 'b_proj', 0, (C,)),
                     (_MODS['fc1'] + '.bias', 'b_fc1', 0, (hid,)), (_MODS['fc2'] + '.bias', 'b_fc2', 0, (C,))]
            if cfg.uses_cos_attn:
                layer.append(('attn.scale_mul_1H11', 'scale_mul', 0, (1, H, 1, 1)))
            Gl, Ga, ba = self.G_layers.view(-1), self.G_ada, n_ada * C
            for i in range(depth):
                p = f'blocks.{i}.'
                for k, name, o, shape in layer:
                    views[p + k] = (Gl, i * self.slab + self.slab_off[name] + o, shape)
                if cfg.sa_block:        # constants in the folded bias (models._pack): [gamma1, gamma2, w1 - 1, w2 - 1, b1, b2]
                    for j, k in enumerate(('gamma1', 'gamma2', 'norm1.weight', 'norm2.weight', 'norm1.bias', 'norm2.bias')):
                        if j >= 2 or cfg.layer_scale >= 0:
                            views[p + k] = (Ga, ba + (i * 6 + j) * C, (C,))
                elif cfg.shared_aln:    # folded bias_i = shared bias + ada_gss_i (models._pack): d ada_gss_i = d bias_i
                    views[p + 'ada_gss'] = (Ga, ba + i * 6 * C, (1, 1, 6, C))
                else:
                    views[p + 'ada_lin.1.weight'] = (Ga, i * 6 * C * C, (6 * C, C))
                    views[p + 'ada_lin.1.bias'] = (Ga, ba + i * 6 * C, (6 * C,))
            if cfg.sa_block:            # head = Sequential(LayerNorm, Linear) (control_var.py:205-207)
                views['head.0.weight'], views['head.0.bias'] = (Ga, ba + ah, (C,)), (Ga, ba + ah + C, (C,))
            else:
                views['head_nm.ada_lin.1.weight'], views['head_nm.ada_lin.1.bias'] = (Ga, ah * C, (2 * C, C)), (Ga, ba + ah, (2 * C,))
            # (region, its size, key or None, shape); the head's rows beyond head_out (padding of head_ld) have no key
            hd, py, Vo = 'head.1.' if cfg.sa_block else 'head.', cfg.pyramid, cfg.head_out
            nl, fl, nc = len(cfg.patch_nums), py.first_l, cfg.num_classes + 1
            misc = [('w_head', V * C, hd + 'weight', (Vo, C)), ('b_head', V, hd + 'bias', (Vo,)), ('w_we', C * cfg.cvae, 'word_embed.weight', (C, cfg.cvae)),
                    ('b_we', C, 'word_embed.bias', (C,)), ('pos', L * C, 'pos_1LC', (1, L, C)), ('lvl', nl * C, 'lvl_embed.weight', (nl, C)),
                    ('pos_start', fl * C, 'pos_start', (1, fl, C)), ('class_emb', nc * C, 'class_emb.weight', (nc, C)),
                    ('cond_embed', 5 * C, 'cond_embed.weight' if cfg.mask_factor == 2 else None, (5, C))]
            if cfg.shared_aln:      # the shared generator's gradient = sum over blocks of the per-block (folded) ones
                misc += [('w_shared', 6 * C * C, 'shared_ada_lin.1.weight', (6 * C, C)), ('b_shared', 6 * C, 'shared_ada_lin.1.bias', (6 * C,))]
            if cfg.type_pos:
                misc += [('type', cfg.mask_factor * C, 'type_embed.weight', (cfg.mask_factor, C))]
            if cfg.separator:
                misc += [('special', cfg.n_special * C, 'special_embed.weight', (cfg.n_special, C))]
            self.misc_off, o = {}, 0
            for name, n, _, _ in misc:
                self.misc_off[name] = (o, n)
                o += n
            self.G_misc = torch.zeros(o, **f32)
            views.update({k: (self.G_misc, self.misc_off[name][0], shape) for name, _, k, shape in misc if k is not None})
            self.buckets = [self.G_layers[i] for i in range(depth)] + [self.G_ada, self.G_misc]
        else:
            # adapter gradient slabs: one per layer [proj A, B | fc1 A, B | fc2 A, B], then every ada_lin adapter (the all-reduce buckets)
            r = lora['r']
            dims = dict(proj=(C, C), fc1=(C, hid), fc2=(hid, C))
            groups = [[(f'blocks.{i}.{_MODS[kind]}', *dims[kind]) for kind in ('proj', 'fc1', 'fc2')] for i in range(depth)]
            groups.append([(f'blocks.{t}.ada_lin.1', C, 6 * C) for t in range(depth)] + [('head_nm.ada_lin.1', C, 2 * C)])
            self.lora_off, o, starts = {}, 0, []
            for group in groups:
                starts.append(o)
                for name, k_in, n_out in group:
                    for ab, shape in (('A', (r, k_in)), ('B', (n_out, r))):
                        self.lora_off[f'{name}.lora_{ab}.default.weight'] = (o, shape[0] * shape[1], shape)
                        o += shape[0] * shape[1]
            if set(self.lora_off) != {n for n, p in self.var.named_parameters() if p.requires_grad}:
                raise RuntimeError('LoRA: the trainable parameters are not exactly the adapters of add_lora')
            self.G_lora = torch.zeros(o, **f32)
            self.buckets = [self.G_lora[a:b] for a, b in zip(starts, starts[1:] + [o])]
            views = {k: (self.G_lora, o, shape) for k, (o, _, shape) in self.lora_off.items()}
        self.grad_views = views
        self._staging = {}
        self._grads_key = key

    def _stage(self, name: str, n: int) -> torch.Tensor:
        """fp32 staging buffer of an accumulating backward (allocated on first use, kept): what cannot take the accumulate flag at its producer
        is computed here exactly as in a plain step and then added into the accumulator by ops.add_inplace"""
        t = self._staging.get(name)
        if t is None or t.numel() < n:
            t = self._staging[name] = torch.zeros(n, device=self.var.device, dtype=torch.float32)
        return t

    def _transposed_weights(self):
        """W^T copies for the data-gradient GEMMs (refreshed after every optimizer step).  LoRA: of the frozen base weights."""
        P = self.var._pack(base=True)
        C, depth, V, hid, n_ada = self.C, self.depth, self.V, self.hid, self.n_ada
        mk = lambda *s: torch.empty(*s, device=self.var.device, dtype=self.var.compute_dtype)
        self.WT = dict(qkv=mk(depth, C, 3 * C), proj=mk(depth, C, C), fc1=mk(depth, C, hid), fc2=mk(depth, hid, C), head=mk(C, V), ada=mk(C, n_ada))
        ops.transpose(P['w_qkv'], self.WT['qkv'], depth, 3 * C, C, C)
        ops.transpose(P['w_proj'], self.WT['proj'], depth, C, C, C)
        ops.transpose(P['w_fc1'], self.WT['fc1'], depth, hid, C, C)
        ops.transpose(P['w_fc2'], self.WT['fc2'], depth, C, hid, hid)
        ops.transpose(P['w_head'], self.WT['head'], 1, V, C, C)
        ops.transpose(P['w_ada'], self.WT['ada'], 1, n_ada, C, C)
        self._wt_gen = self._pack_gen()

    def _pack_gen(self):
        return self.var._pack_base_gen if getattr(self.var, '_lora', None) is not None else self.var._pack_gen

    def grads(self) -> Dict[str, torch.Tensor]:
        """state_dict key -> gradient view (fp32); a LoRA model: the adapter keys only"""
        return {k: buf[o:o + math.prod(shape)].view(shape) for k, (buf, o, shape) in self.grad_views.items()}

    # ---------------------------------------------------------------- forward + backward
    @torch.no_grad()
    def forward_backward(self, label_B: torch.Tensor, x_wo_first: torch.Tensor, cond_type: Optional[torch.Tensor], targets: torch.Tensor,
                         ignore_mask: Optional[torch.Tensor] = None, drop_seed: Optional[int] = None, mask_first: bool = True,
                         accumulate: bool = False, policy: Optional[PolicyLoss] = None, distill=None):
        """-> (loss scalar tensor, per-token loss (B*L,)); gradients land in self.grads(): overwritten, or with accumulate=True added to what
        it holds - fp32(old + this micro-batch's plain gradient) per element, whatever the batch size of the earlier calls.  The loss and its
        1 / M scale are this micro-batch's own; the 1 / N of a window of N belongs to the optimizer's gradient scale (FusedAdamW.step).
        policy: the clipped policy-gradient loss in the place of the cross-entropy (PolicyLoss) - one other loss launch on the
        same logits and dlogits, nothing else; the per-token logprob, ratio, clipped, kl and coef stay on the engine as self.policy_out.
        distill: the soft-target loss in the place of the cross-entropy (DistillLoss) - likewise one other loss launch; `targets`
        is not read, distill.weights stands where ignore_mask stands, and the returned per-token loss is the token's KL(teacher || model).
        A SparseDistillLoss (the teacher's N most likely codes and its tail mass) dispatches to cvar_kd_topn_fwd_bwd in the same place."""
        if policy is not None:
            policy.check(x_wo_first.shape[0], self.L)                 # refused before any device work
        if distill is not None:                                      # likewise
            if policy is not None:
                raise ValueError('distill and policy: a step has one loss - the soft-target loss or the policy-gradient loss')
            if not isinstance(distill, _DISTILL_FORMS):
                raise TypeError(f'distill: a DistillLoss or a SparseDistillLoss, got {type(distill).__name__}')
            if distill.weights is not None and ignore_mask is not None:
                raise ValueError('distill.weights and ignore_mask: the weights take the place of ignore_mask - fold the two into one and pass it as weights')
            if self.cfg.separator:
                raise NotImplementedError(_NO_SEPARATOR)
            if self.cfg.vocab != self.V:
                raise NotImplementedError(f'distill: the head is {self.V} columns wide for a vocabulary of {self.cfg.vocab}; teacher logits are (B, L, vocab)')
            distill.check(x_wo_first.shape[0], self.L, self.cfg.vocab, self.var.device)
            if distill.weights is not None:
                ignore_mask = distill.weights
        self.forward_train(label_B, x_wo_first, cond_type, drop_seed, mask_first)
        dev = self.var.device
        M, V = self.M, self.V
        tg = targets.to(device=dev, dtype=torch.int32).contiguous().view(-1)
        if ignore_mask is not None:                                  # train_control_var_hpu.py:233-237
            w = ignore_mask.to(device=dev, dtype=torch.float32).contiguous().view(-1)
            gscale = 1.0 / (M * (float(w.mean()) + 1e-6))
        else:
            w, gscale = None, 1.0 / M
        if isinstance(distill, SparseDistillLoss):
            ops.kd_topn_fwd_bwd(self.logits, distill.top_ids.contiguous(), distill.top_logprobs.contiguous(),
                                None if distill.tail_logprob is None else distill.tail_logprob.contiguous(), distill.N, w, gscale, self.loss_tok,
                                self.dlogits, M, V)
        elif distill is not None:
            ops.kd_fwd_bwd(self.logits, distill.logits.contiguous(), V, w, gscale, self.loss_tok, self.dlogits, M, V)
        elif policy is None:
            ops.ce_fwd_bwd(self.logits, tg, w, gscale, self.loss_tok, self.dlogits, M, V)
        else:
            adv, old, ref = policy.rows(self._saved['B'], self.L, dev)
            po = self.policy_out = dict(logprob=torch.empty(M, device=dev), ratio=torch.empty(M, device=dev), kl=torch.empty(M, device=dev),
                                        coef=torch.empty(M, device=dev), clipped=torch.empty(M, device=dev, dtype=torch.int32))
            ops.pg_fwd_bwd(self.logits, tg, adv, w, old, ref, policy.clip[0], policy.clip[1], policy.kl_coef, gscale, self.loss_tok, M, V,
                           dlogits=self.dlogits, **po)
        loss = (self.loss_tok * w).mean() / (w.mean() + 1e-6) if w is not None else self.loss_tok.mean()
        self.backward(accumulate=accumulate)
        return loss, self.loss_tok

    @torch.no_grad()
    def forward_train(self, label_B: torch.Tensor, x_wo_first: torch.Tensor, cond_type: Optional[torch.Tensor], drop_seed: Optional[int] = None,
                      mask_first: bool = True):
        """teacher-forced forward that keeps every block's activations; returns logits (B*L, V) fp32"""
        cfg, var = self.cfg, self.var
        P = var._pack(check=True, base=True)
        C, depth, V, L, hid, n_ada, ah, H, eps = self.C, self.depth, self.V, self.L, self.hid, self.n_ada, self.ah, cfg.H, self.eps
        dev, T = var.device, var.compute_dtype
        B = x_wo_first.shape[0]
        self._setup(B)
        if self._wt_gen != self._pack_gen():       # the W^T copies follow the packed weights (any optimizer, manual edits, resume)
            self._transposed_weights()
        lo, M = self._lora, self.M
        from .models import _check_index_range
        _check_index_range(label_B, 0, cfg.num_classes, 'label_B')
        labels = label_B.to(dev)
        types = cond_type.to(dev) if (cond_type is not None and cfg.mask_factor == 2) else None
        if types is not None:
            _check_index_range(types, 0, 4, 'cond_type')
        if cfg.cond_drop_rate > 0:                                  # control_var.py:578,584: every forward(), train or eval
            labels = torch.where(torch.rand(B, device=dev) < cfg.cond_drop_rate, cfg.num_classes, labels)
            if types is not None:
                types = torch.where(torch.rand(B, device=dev) < cfg.cond_drop_rate, 4, types)
        labels = labels.to(torch.int32).contiguous()
        types = types.to(torch.int32).contiguous() if types is not None else None
        # DropPath row scales (helpers.py:39-46): per sample, per block, per branch
        dp1 = dp2 = None
        rate = cfg.drop_path_rate                                     # constructor argument; the factories pass 0.1 * depth / 24 (models/__init__.py:15,40)
        if self.drop_path and var.training and rate > 0:
            g = torch.Generator(device=dev)
            g.manual_seed(drop_seed if drop_seed is not None else int(torch.empty((), dtype=torch.int64).random_().item()))
            dpr = torch.linspace(0, rate, depth, device=dev).view(depth, 1)
            keep = 1 - dpr
            dp1 = (torch.rand(depth, B, device=dev, generator=g) < keep).float() / keep
            dp2 = (torch.rand(depth, B, device=dev, generator=g) < keep).float() / keep
        if lo is None:          # the leaf that launches an adapted linear (proj, fc1, fc2, the adaLN generator): the GEMM on the packed weight
            linear = lambda kind, i, x, out, M, N, K, **epi: ops.gemm(x, P['w_' + kind], out, M=M, N=N, K=K, w_off=i * N * K, **epi)
        else:                   # adapter dropout: active in train() only; drop_seed seeds it too
            self._lp = lo['dropout'] if var.training else 0.0
            self._lseed = drop_seed if drop_seed is not None else int(torch.empty((), dtype=torch.int64).random_().item())
            self._lora_pack()
            linear = self._lora_linear
        # ---- forward
        x0 = self.Xs[0]
        cond = torch.empty(B, C, device=dev, dtype=torch.float32)
        mask_first = self._mask_first = bool(mask_first) or cfg.mask_factor != 2
        table = P['lvl_pos_fwd'] if mask_first else P['lvl_pos_fwd_']
        var._first_tokens(P, labels, types, x0, cond, B, L, table, mask_first)
        tok = x_wo_first.to(device=dev, dtype=torch.float32).contiguous()
        if tok.shape[1] != self.ncode:
            raise AssertionError(f'teacher-forcing input has {tok.shape[1]} tokens, expected {self.ncode}')
        var._embed_teacher_forced(P, tok, x0, B, table, mask_first)
        cs = torch.empty(B, C, device=dev, dtype=T)
        ops.silu_cast(cond, cs)
        ada = torch.empty(B, n_ada, device=dev, dtype=torch.float32)
        linear('ada', 0, cs, ada, B, n_ada, C, bias=P['b_ada'])
        ln = _ln_rows(C)
        ldh = self.Xin['fc2'][1]                                      # fc1 writes fc2's operand in place: with fc2's row stride
        for i in range(depth):
            a0 = i * 6 * C
            x, x1 = self.Xs[i], self.X1s[i]
            ln(x, ada, a0 + 2 * C, a0 + 4 * C, n_ada, L, self.U[i], M, C, eps)
            ops.gemm(self.U[i], P['w_qkv'], self.arena[i], M=M, N=3 * C, K=C, w_off=i * 3 * C * C, bias=P['b_qkv'][i])
            if cfg.uses_cos_attn:
                ops.cos_qk_norm(self.arena[i], B, H, L, 0, L, P['scale_mul'], sm_off=i * H, norms=self.NORMS[i])
            ops.attention(self.arena[i], self.O[i], B, H, L, 0, L, self.scale, self.lvl_end, lse=self.LSE[i], holes=self.holes)
            # x1 = x + (gamma1 * keep1) * proj(o): gate / DropPath scale / residual in the GEMM epilogue; the branch output the backward
            # needs (d gamma1 = sum dx * f) is stored next to it
            linear('proj', i, self.O[i], x1, M, C, C, bias=P['b_proj'][i], gate=ada, ldg=n_ada, gate_rows=L, gate_off=a0,
                   gate_scale=dp1[i].contiguous() if dp1 is not None else None, residual=x, pre_act=self.F1[i])
            ln(x1, ada, a0 + 3 * C, a0 + 5 * C, n_ada, L, self.U2[i], M, C, eps)
            # fc1 with the GELU in its epilogue; the pre-activation the backward needs is stored alongside (no separate gelu pass)
            linear('fc1', i, self.U2[i], self.Hh[i], M, hid, C, ldc=ldh, bias=P['b_fc1'][i], act=ACT_GELU_TANH, pre_act=self.A[i])
            linear('fc2', i, self.Hh[i], self.Xs[i + 1], M, C, hid, bias=P['b_fc2'][i], gate=ada, ldg=n_ada, gate_rows=L, gate_off=a0 + C,
                   gate_scale=dp2[i].contiguous() if dp2 is not None else None, residual=x1, pre_act=self.F2[i])
        ln(self.Xs[depth], ada, ah, ah + C, n_ada, L, self.UH, M, C, eps)
        ops.gemm(self.UH, P['w_head'], self.logits, M=M, N=V, K=C, bias=P['b_head'])
        self._saved = dict(ada=ada, cs=cs, cond=cond, labels=labels, types=types, tok=tok, dp1=dp1, dp2=dp2, B=B)
        return self.logits

    def backward(self, accumulate: bool = False):
        """backward from self.dlogits (compute dtype, (B*L, V)) through head, blocks, adaLN generator and - full model - embeddings.
        accumulate: every gradient element becomes fp32(old + plain).  The weight-gradient GEMMs, bias sums, the adapter gradients and
        the word-embedding gradient add at their producer; the adaLN generator's gradient and the small embedding gradients - several of
        which are DERIVED from other entries of the gradient buffer - are computed on staging copies exactly as in a plain step and then
        added.  A LoRA model: data gradients through the frozen base plus the adapter gradients into self.G_lora."""
        cfg = self.cfg
        acc = bool(accumulate)
        full = self._lora is None
        grads_of = self._full_grads_of if full else self._lora_grads_of       # the leaf behind the data-gradient GEMM of a linear
        ready = self.reducer.ready if self.reducer is not None else (lambda idx: None)
        P = self.var._pack(base=True)
        C, depth, V, L, M, hid, n_ada, ah, H, eps, ws = self.C, self.depth, self.V, self.L, self.M, self.hid, self.n_ada, self.ah, cfg.H, self.eps, self.ws
        ada, dp1, dp2, B = (self._saved[k] for k in ('ada', 'dp1', 'dp2', 'B'))
        # ---- head
        self.dada.zero_()
        ops.gemm(self.dlogits, self.WT['head'], self.DU, M=M, N=C, K=V)
        if full:                        # head and qkv carry no adapter: they have a parameter gradient in the full model only
            mo = self.misc_off
            self._wgrad(self.dlogits, V, self.UH, C, self.G_misc, mo['w_head'][0], mo['b_head'][0], acc)
        ops.ln_modulate_bwd(self.Xs[depth], self.DU, ada, ah, n_ada, L, None, self.dX, self.dada, ah, ah + C, n_ada, M, C, eps, ws)
        # ---- blocks
        for i in reversed(range(depth)):
            a0 = i * 6 * C
            # FFN branch.  Full model: dH = (dF W2) * gelu'(A) in one GEMM; LoRA: cvar_lora_dx applies GELU' after adding the branch's share
            gelu = dict(act=ACT_GELU_GRAD, aux=self.A[i]) if full else {}
            ops.gated_grad(self.dX, self.F2[i], ada, a0 + C, n_ada, dp2[i].contiguous() if dp2 is not None else None, self.DF, self.dada, a0 + C, n_ada, B, L, C, ws)
            ops.gemm(self.DF, self.WT['fc2'], self.DH, M=M, N=hid, K=C, w_off=i * hid * C, **gelu)
            grads_of(i, 'fc2', self.DF, C, hid, acc)
            ops.gemm(self.DH, self.WT['fc1'], self.DU, M=M, N=C, K=hid, w_off=i * C * hid)
            grads_of(i, 'fc1', self.DH, hid, C, acc)
            ops.ln_modulate_bwd(self.X1s[i], self.DU, ada, a0 + 3 * C, n_ada, L, self.dX, self.dX, self.dada, a0 + 3 * C, a0 + 5 * C, n_ada, M, C, eps, ws)
            # attention branch
            ops.gated_grad(self.dX, self.F1[i], ada, a0, n_ada, dp1[i].contiguous() if dp1 is not None else None, self.DF, self.dada, a0, n_ada, B, L, C, ws)
            ops.gemm(self.DF, self.WT['proj'], self.DU, M=M, N=C, K=C, w_off=i * C * C)
            grads_of(i, 'proj', self.DF, C, C, acc)
            ops.attention_bwd(self.arena[i], self.O[i], self.DU, self.LSE[i], self.DQKV, ws, B, H, L, L, self.scale, self.lvl_end, holes=self.holes)
            if cfg.uses_cos_attn:           # normalisation + learned temperature of basic_var.py:99-104 (a parameter of the base: frozen under LoRA)
                ops.cos_qk_norm_bwd(self.arena[i], self.DQKV, B, H, L, L, P['scale_mul'], self.NORMS[i], self.DSM, sm_off=i * H)
                if full:
                    ops.colsum(self.DSM, H, self.G_layers, M, H, ws, accumulate=acc, out_off=i * self.slab + self.slab_off['scale_mul'])
            ops.gemm(self.DQKV, self.WT['qkv'], self.DU, M=M, N=C, K=3 * C, w_off=i * C * 3 * C)
            if full:
                grads_of(i, 'qkv', self.DQKV, 3 * C, C, acc)      # the k-bias third is unused (zero_k_bias is a buffer)
            ops.ln_modulate_bwd(self.Xs[i], self.DU, ada, a0 + 2 * C, n_ada, L, self.dX, self.dX, self.dada, a0 + 2 * C, a0 + 4 * C, n_ada, M, C, eps, ws)
            ready(i)
        # ---- adaLN parameter generator, then - full model - the embeddings (dX now holds d loss / d x0)
        if full:
            dcond, Gm = self._ada_grads_full(acc)
            ready(depth)
            self._embedding_grads(dcond, Gm, acc)
            ready(depth + 1)
        else:
            self._ada_grads_lora(acc)
            ready(depth)

    # ---------------------------------------------------------------- full model: weight gradients, generator and embedding tail
    def _full_grads_of(self, i, kind, dY, n_out, k_in, acc):
        """weight and bias gradient of linear `kind` of block i into its layer's slab"""
        go, so = i * self.slab, self.slab_off
        self._wgrad(dY, n_out, self.Xin[kind][0][i], k_in, self.G_layers, go + so['w_' + kind], go + so['b_' + kind], acc)

    @torch.no_grad()
    def _wgrad(self, dY, n_out: int, X, k_in: int, G, w_off: int, b_off=None, acc: bool = False):
        """dW[n_out, k_in] = dY^T X into the fp32 gradient slab (+ the bias gradient = column sums of dY).  bf16 mode: `cvar_gemm_tn` reads both
        token-major operands in place (LDS transpose-read) - no transposed copies; shapes it does not take (a dimension that is not a
        multiple of its tile, the fp32 parity mode) go through two HBM transposes + `cvar_gemm` as in round 1.  acc: add to what G holds -
        `cvar_gemm_tn_acc`; the fallback computes into a staging buffer and adds it (cvar_gemm's kernels have no accumulating form)."""
        M, Mp = self.M, self.Mp
        if (dY.dtype == torch.bfloat16 and X.dtype == torch.bfloat16 and n_out % 128 == 0 and k_in % 128 == 0
                and 2 * M * max(n_out, k_in) < 2 ** 31 - 1):
            # the bias gradient (column sums of dY) rides on the same pass: ones-operand MFMAs on the dY fragments (round 3; a separate colsum pass before)
            ops.gemm_tn(dY, X, G, T=M, Nn=n_out, Kk=k_in, c_off=w_off, colsum=G if b_off is not None else None, colsum_off=b_off or 0, accumulate=acc)
            return
        ops.transpose(dY, self.TA, 1, M, n_out, n_out, ld_out=Mp)
        ops.transpose(X, self.TB, 1, M, k_in, k_in, ld_out=Mp)
        if acc:
            S = self._stage('wgrad', n_out * k_in)
            ops.gemm(self.TA, self.TB, S, M=n_out, N=k_in, K=Mp)
            ops.add_inplace(G, S, n_out * k_in, y_off=w_off)
        else:
            ops.gemm(self.TA, self.TB, G, M=n_out, N=k_in, K=Mp, c_off=w_off)
        if b_off is not None:
            ops.rowsum(self.TA, Mp, G, n_out, M, accumulate=acc, out_off=b_off)

    def _ada_grads_full(self, acc):
        """gradient of the adaLN parameter generator (one GEMM for all blocks + head) -> (d cond, Gm: where this micro-batch's G_misc values go).
        accumulating: they go to staging copies (Ga, Gm) - what is derived from them must be derived from them, not from the window's sum"""
        cfg, dev, T = self.cfg, self.var.device, self.var.compute_dtype
        C, depth, n_ada, Bp, ws, mo = self.C, self.depth, self.n_ada, self.Bp, self.ws, self.misc_off
        cs, cond, B = (self._saved[k] for k in ('cs', 'cond', 'B'))
        dada_T = self.dada.to(T)
        dsilu = torch.empty(B, C, device=dev, dtype=torch.float32)
        ops.gemm(dada_T, self.WT['ada'], dsilu, M=B, N=C, K=n_ada)
        tA = torch.zeros(n_ada, Bp, device=dev, dtype=T)
        tB = torch.zeros(C, Bp, device=dev, dtype=T)
        ops.transpose(dada_T, tA, 1, B, n_ada, n_ada, ld_out=Bp)
        ops.transpose(cs, tB, 1, B, C, C, ld_out=Bp)
        Ga = self._stage('ada', self.G_ada.numel()) if acc else self.G_ada
        Gm = self._stage('misc', self.G_misc.numel()) if acc else self.G_misc
        ops.gemm(tA, tB, Ga, M=n_ada, N=C, K=Bp)
        ops.colsum(self.dada, n_ada, Ga, B, n_ada, ws, out_off=n_ada * C)
        if cfg.shared_aln:          # rows = blocks: column sums over the depth axis of the folded per-block gradients
            ops.colsum(Ga, 6 * C * C, Gm, depth, 6 * C * C, ws, out_off=mo['w_shared'][0])
            ops.colsum(Ga, 6 * C, Gm, depth, 6 * C, ws, a_off=n_ada * C, out_off=mo['b_shared'][0])
        if acc:
            ops.add_inplace(self.G_ada, Ga, self.G_ada.numel())
        dcond = torch.empty(B, C, device=dev, dtype=torch.float32)
        ops.silu_bwd(cond, dsilu, dcond)
        return dcond, Gm

    def _embedding_grads(self, dcond, Gm, acc):
        """the small embedding gradients from self.dX = d loss / d x0 and d cond.  Several are DERIVED from other entries of the gradient buffer
        (lvl / type from pos, pos_start a copy, class_emb / cond_embed zeroed and scattered into): all of it is computed in Gm - self.G_misc,
        or its staging copy when accumulating, which is then added"""
        cfg, dev = self.cfg, self.var.device
        py, C, L, ws, mo = cfg.pyramid, self.C, self.L, self.ws, self.misc_off
        fl = py.first_l
        labels, types, tok, B = (self._saved[k] for k in ('labels', 'types', 'tok', 'B'))
        ops.colsum(self.dX, L * C, Gm, B, L * C, ws, out_off=mo['pos'][0])
        for k, (b0, e0) in enumerate(zip(py.begin, py.end)):
            ops.colsum(Gm, C, Gm, e0 - b0, C, ws, a_off=mo['pos'][0] + b0 * C, out_off=mo['lvl'][0] + k * C)
        if cfg.type_pos:            # type_1L: first (control) half of every scale has id 1, the image half id 0 (control_var.py:103-108)
            for k, (b0, e0) in enumerate(zip(py.begin, py.end)):
                half = (e0 - b0) // 2
                for tid, r0 in (((1, b0), (0, b0 + half)) if self._mask_first else ((0, b0), (1, b0 + half))):
                    ops.colsum(Gm, C, Gm, half, C, ws, accumulate=(k > 0), a_off=mo['pos'][0] + r0 * C, out_off=mo['type'][0] + tid * C)
        Gm[mo['pos_start'][0]:mo['pos_start'][0] + fl * C].copy_(Gm[mo['pos'][0]:mo['pos'][0] + fl * C])
        Mt = B * self.ncode
        Mtp = _pad8(Mt)
        if cfg.separator:           # code rows are interleaved with the separator rows: gather them; the separators' gradient is the batch sum of their rows
            code = torch.from_numpy(py.code_positions()[fl:]).to(dev)
            dXw = self.dX.view(B, L, C)[:, code].contiguous()               # (B, ncode, C)
            we_staged = self._word_embed_grads(tok, B, self.ncode + fl, fl, C, Mt, Mtp, Gm, acc, src=dXw, src_has_first=False)
            mapping = cfg.special_mapping(self._mask_first)
            for j, pos in enumerate(int(q) for q in py.special_positions()):
                ops.colsum(self.dX, L * C, Gm, B, C, ws, a_off=pos * C, out_off=mo['special'][0] + mapping[j] * C)
        else:
            we_staged = self._word_embed_grads(tok, B, L, fl, C, Mt, Mtp, Gm, acc)
        cls_o, cnd_o = mo['class_emb'][0], mo['cond_embed'][0]
        Gm[cls_o:cls_o + mo['class_emb'][1]].zero_()
        Gm[cnd_o:cnd_o + mo['cond_embed'][1]].zero_()
        g_class = Gm[cls_o:cls_o + mo['class_emb'][1]]
        sos_row = (fl - 1) if self._mask_first else 0                 # position of the class token; image first: [sos, cond_token]
        ops.scatter_add_rows(self.dX, L * C, labels, g_class, B, C, src_off=sos_row * C)
        ops.scatter_add_rows(dcond, C, labels, g_class, B, C)
        if cfg.mask_factor == 2:
            ops.scatter_add_rows(self.dX, L * C, types, Gm[cnd_o:cnd_o + mo['cond_embed'][1]], B, C, src_off=(1 - sos_row) * C)
        if acc:         # misc layout: [w_head | b_head | w_we | b_we | pos ... ]: the head added at its GEMM, word_embed at its kernel unless it took the slow path
            o0 = mo['w_we'][0] if we_staged else mo['pos'][0]
            ops.add_inplace(self.G_misc, Gm, self.G_misc.numel() - o0, y_off=o0, x_off=o0)

    def _word_embed_grads(self, tok, B, L, fl, C, Mt, Mtp, Gm, acc=False, src=None, src_has_first=True):
        """src: gradient rows of the word-embedded tokens - self.dX with L rows per sample of which the first fl are skipped, or a compact
        (B, L - fl, C) gather of them (separator models).  Gm: where the plain values go (self.G_misc, or its staging copy when acc); the
        one-pass kernel adds into self.G_misc itself when acc.  -> True if the values were left in the staging copy for the caller to add"""
        cfg = self.cfg
        mo = self.misc_off
        src = self.dX if src is None else src
        rows = L if src_has_first else L - fl
        skip = fl if src_has_first else 0
        if cfg.cvae == 32 and C % 64 == 0 and tok.dtype == torch.float32 and src.dtype == torch.float32:
            # one pass over the token-major tensors (round 3): dW and db together, no transposes, no per-sample launches
            ops.wordembed_grad(src, C, rows, skip, tok, L - fl, B, C, cfg.cvae, self.G_misc if acc else Gm, mo['w_we'][0], mo['b_we'][0], accumulate=acc)
            return False
        for b in range(B):      # gradient rows of sample b -> columns [b*(L-fl), (b+1)*(L-fl)) of TA32 ([C][Mtp])
            ops.transpose(src, self.TA32[b * (L - fl):], 1, L - fl, C, C, in_off=(b * rows + skip) * C, ld_out=Mtp)
        ops.transpose(tok, self.TB32, 1, Mt, cfg.cvae, cfg.cvae, ld_out=Mtp)
        ops.gemm(self.TA32, self.TB32, Gm, M=C, N=cfg.cvae, K=Mtp, c_off=mo['w_we'][0])
        for b in range(B):
            ops.colsum(src, C, Gm, L - fl, C, self.ws, accumulate=(b > 0), a_off=(b * rows + skip) * C, out_off=mo['b_we'][0])
        return acc

    # ---------------------------------------------------------------- LoRA (controlvar_amd/lora.py; DESIGN.md "LoRA")
    # The base weights are frozen: their gradients are neither computed nor stored.  Each target's rank-r branch enters the base
    # GEMM - and so its fused epilogue (bias, gate, DropPath scale, residual, GELU, pre_act) - by K-augmentation: the operand [x | u]
    # (u = s drop(x) A^T from cvar_lora_down, zero padding up to a 128-byte row step) against the packed weight [W | B | 0].  The
    # backward runs the base data-gradient GEMM, then cvar_lora_down for du = dY B, cvar_lora_dx for the branch's share of dx, and
    # cvar_lora_wgrad for dB = dY^T u and dA = s du^T drop(x).  Targets: tag 4 i + (0 proj, 1 fc1, 2 fc2, 3 ada_lin), head_nm 4 depth + 3.
    def _lora_pack(self):
        """operands of the adapter branch in the compute dtype: A (16 rows, zero beyond r), B^T (16 rows) per target, and the K-augmented
        GEMM weights [W | B | 0] (base part copied once per base pack, the B columns at every forward)"""
        from .lora import adapters
        var = self.var
        P = var._pack(base=True)
        T, dev = var.compute_dtype, var.device
        C, depth, hid, n_ada, r, rp = self.C, self.depth, self.hid, self.n_ada, self.r, self.rp
        ad = adapters(var)
        if self._aug is None or self._aug[0] is not P:
            W = {}
            for kind, (n_out, k_in) in (('proj', (C, C)), ('fc1', (hid, C)), ('fc2', (C, hid))):
                w = torch.zeros(depth, n_out, k_in + rp, device=dev, dtype=T)
                w[:, :, :k_in] = P['w_' + kind]
                W[kind] = w
            w = torch.zeros(n_ada, C + self.Kx, device=dev, dtype=T)
            w[:, :C] = P['w_ada']
            W['ada'] = w
            self._aug = (P, W)
        W = self._aug[1]
        self.Wa = W
        self.LA, self.LBT = {}, {}
        for kind, (n_out, k_in) in (('proj', (C, C)), ('fc1', (hid, C)), ('fc2', (C, hid))):
            As = torch.stack([ad[f'blocks.{i}.{_MODS[kind]}'][0] for i in range(depth)])          # (depth, r, k_in)
            Bs = torch.stack([ad[f'blocks.{i}.{_MODS[kind]}'][1] for i in range(depth)])          # (depth, n_out, r)
            self.LA[kind] = torch.zeros(depth, 16, k_in, device=dev, dtype=T)
            self.LA[kind][:, :r] = As
            self.LBT[kind] = torch.zeros(depth, 16, n_out, device=dev, dtype=T)
            self.LBT[kind][:, :r] = Bs.transpose(1, 2)
            W[kind][:, :, k_in:k_in + r] = Bs
        tn = [f'blocks.{t}.ada_lin.1' for t in range(depth)] + ['head_nm.ada_lin.1']
        self.LA['ada'] = torch.zeros(depth + 1, 16, C, device=dev, dtype=T)
        self.LA['ada'][:, :r] = torch.stack([ad[n][0] for n in tn])
        self.LBT['ada'] = torch.zeros(depth + 1, 16, 6 * C, device=dev, dtype=T)
        for t, n in enumerate(tn):
            Bt = ad[n][1]
            self.LBT['ada'][t, :r, :Bt.shape[0]] = Bt.t()
            W['ada'][t * 6 * C:t * 6 * C + Bt.shape[0], C + 16 * t:C + 16 * t + r] = Bt

    def _tag(self, i: int, kind: str) -> int:
        return 4 * i + ('proj', 'fc1', 'fc2', 'ada').index(kind)

    def _lora_linear(self, kind, i, x, out, M, N, K, **epi):
        """forward leaf: u = s drop(x) A^T of every adapter that feeds this GEMM into the augmented operand [x | u | 0] (x copied in the same
        pass), then the GEMM on [W | B | 0].  The generator's depth + 1 adapters share one operand, 16 columns each; fc2 finds x already in
        its augmented buffer, where fc1 wrote it"""
        lo = self._lora
        xa, ld = self.Xin[kind]
        xa, there = xa[i], kind == 'fc2'
        for j, t in enumerate(range(self.depth + 1) if kind == 'ada' else (i,)):
            ops.lora_down(x, self.LA[kind][t], xa, M=M, K=K, r=self.r, scale=lo['scale'], p=self._lp, seed=self._lseed, tag=self._tag(t, kind),
                          ldx=ld if there else 0, ldu=ld, u_off=K + 16 * j, x_copy=None if there or j else xa, ld_copy=0 if there else ld)
        ops.gemm(xa, self.Wa[kind], out, M=M, N=N, K=ld, lda=ld, ldw=ld, w_off=i * N * ld, **epi)

    def _lora_grads_of(self, i, kind, dY, n_out, k_in, acc):
        """backward leaf: du = dY B; dx (self.DU / self.DH, in place) += branch share (fc2: * gelu'(A)); dB = dY^T u; dA = s du^T drop(x).
        x: the augmented saved input [x | u] of the linear, u at column k_in"""
        lo, M, r = self._lora, self.M, self.r
        s, p, seed, tag = lo['scale'], self._lp, self._lseed, self._tag(i, kind)
        x, ldx = self.Xin[kind]
        x, G = x[i], self.G_lora
        oA = self.lora_off[f'blocks.{i}.{_MODS[kind]}.lora_A.default.weight'][0]
        oB = self.lora_off[f'blocks.{i}.{_MODS[kind]}.lora_B.default.weight'][0]
        fc2 = kind == 'fc2'
        ops.lora_down(dY, self.LBT[kind][i], self.DUr, M=M, K=n_out, r=r, scale=1.0, ldu=16)
        ops.lora_dx(self.DH if fc2 else self.DU, self.DUr, self.LA[kind][i], M=M, K=k_in, r=r, scale=s, p=p, seed=seed, tag=tag, lddu=16,
                    aux=self.A[i] if fc2 else None, ldaux=ldx if fc2 else 0)
        ops.lora_wgrad(dY, x, G, self.lws, M=M, N=n_out, r=r, ldz=ldx, z_off=k_in, out_off=oB, accumulate=acc)
        ops.lora_wgrad(x, self.DUr, G, self.lws, M=M, N=k_in, r=r, scale=s, p=p, seed=seed, tag=tag, ldy=ldx, ldz=16, out_off=oA, os_n=1, os_j=k_in,
                       accumulate=acc)

    def _ada_grads_lora(self, acc):
        """adaLN generator adapters: dY = d ada (B rows), u_t in the columns of [cs | u_0 ... u_depth]"""
        lo, C, depth, n_ada, r = self._lora, self.C, self.depth, self.n_ada, self.r
        s, p, seed, B = lo['scale'], self._lp, self._lseed, self._saved['B']
        dada_T = self.dada.to(self.var.compute_dtype)
        ld = C + self.Kx
        for t in range(depth + 1):
            n_out = 6 * C if t < depth else 2 * C
            name = f'blocks.{t}.ada_lin.1' if t < depth else 'head_nm.ada_lin.1'
            oA = self.lora_off[f'{name}.lora_A.default.weight'][0]
            oB = self.lora_off[f'{name}.lora_B.default.weight'][0]
            ops.lora_down(dada_T, self.LBT['ada'][t], self.DUa, M=B, K=n_out, r=r, scale=1.0, ldx=n_ada, x_off=t * 6 * C, lda=6 * C, ldu=16)
            ops.lora_wgrad(dada_T, self.csa, self.G_lora, self.lws, M=B, N=n_out, r=r, ldy=n_ada, y_off=t * 6 * C, ldz=ld, z_off=C + 16 * t, out_off=oB,
                           accumulate=acc)
            ops.lora_wgrad(self.csa, self.DUa, self.G_lora, self.lws, M=B, N=C, r=r, scale=s, p=p, seed=seed, tag=self._tag(t, 'ada'), ldy=ld, ldz=16,
                           out_off=oA, os_n=1, os_j=C, accumulate=acc)


class BucketReducer:
    """Gradient all-reduce of the data-parallel step (replaces DDP's bucketed all-reduce, train_control_var_hpu.py:604, and
    dist.py:100-116): one SUM all-reduce per bucket (bucket = one transformer layer's gradient slab, then the adaLN
    generator, then head + embeddings), launched on a side stream the moment the backward has finished that bucket, so that
    RCCL traffic over xGMI overlaps the remaining backward.  The 1/world mean is folded into the optimizer's gradient scale."""

    def __init__(self, buckets: Sequence[torch.Tensor], group=None, force: bool = False):
        """force=True issues the collectives even in a one-rank group (SUM over one rank = identity): the real slabs then travel the
        whole path - side stream, RCCL call, event hand-back - on a single GPU, which is how the path is tested without a node."""
        import torch.distributed as dist
        self.dist = dist
        self.buckets = list(buckets)
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.active = self.world > 1 or (force and dist.is_initialized())
        self.cuda = len(self.buckets) > 0 and self.buckets[0].is_cuda
        self.stream = torch.cuda.Stream() if (self.cuda and self.active) else None
        self.handles: List = []
        self.launched: List[int] = []
        self.bytes_sent = 0

    def ready(self, idx: int):
        self.launched.append(idx)
        if not self.active:
            return
        self.bytes_sent += self.buckets[idx].numel() * self.buckets[idx].element_size()
        b = self.buckets[idx]
        if self.cuda:
            ev = torch.cuda.Event()
            ev.record()
            with torch.cuda.stream(self.stream):
                self.stream.wait_event(ev)
                self.handles.append(self.dist.all_reduce(b, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))
        else:
            self.handles.append(self.dist.all_reduce(b, op=self.dist.ReduceOp.SUM, group=self.group, async_op=True))

    def wait(self):
        for h in self.handles:
            h.wait()
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)
        self.handles.clear()
        done, self.launched = self.launched, []
        return done


class FusedAdamW:
    """torch.optim.AdamW(betas=(0.9, 0.95)) over the model's parameters (train_control_var_hpu.py:631-633) with the
    decay / no-decay groups of filter_params, gradient-norm clipping (:244-245) and the all-reduce mean folded into one
    fused kernel per tensor.  `param_groups` is torch-shaped so that lr_wd_annealing() drives it unchanged."""

    def __init__(self, var, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.0, nowd_keys=NOWD_KEYS):
        self.var = var
        self.betas, self.eps = betas, eps
        self.lora = getattr(var, '_lora', None) is not None        # LoRA: the adapters only (the frozen base has no state and no step)
        self.named = [(n, p) for n, p in var.named_parameters() if p.requires_grad or not self.lora]
        self.state = {n: (torch.zeros_like(p.data), torch.zeros_like(p.data)) for n, p in self.named}
        groups: Dict[str, dict] = {}                             # first-seen order, as filter_params (utils/lr_control.py:67-101)
        for n, p in self.named:
            d = decays(n, p.ndim, nowd_keys)
            groups.setdefault('D' if d else 'ND', dict(names=[], lr=lr, weight_decay=weight_decay if d else 0.0,
                                                       wd_sc=1.0 if d else 0.0, lr_sc=1.0))['names'].append(n)
        self.param_groups = list(groups.values())
        self.steps = 0
        self._partial = None
        self._out2 = None
        self._table = None
        self._table_sig = None
        self.fuse_copies = True                                  # False: rebuild every packed copy from the fp32 parameters after a step

    @torch.no_grad()
    def step(self, grads: Dict[str, torch.Tensor], max_norm: float = 0.0, world: int = 1, accum: int = 1) -> torch.Tensor:
        """returns a device tensor [grad_norm (of the averaged gradient), clip coefficient].  `grads` holds the sum over `world` ranks and over
        the `accum` micro-batches of a window: the gradient scale is 1 / (world * accum)"""
        dev = self.named[0][1].device
        n = len(self.named)
        if self._partial is None:
            self._partial = torch.zeros(n * 256, device=dev, dtype=torch.float64)
            self._out2 = torch.ones(2, device=dev, dtype=torch.float32)
        # one launch over a device table of (param, grad, m, v) instead of 2 x ~830 per-tensor launches; the table is rebuilt
        # only when a buffer moved (new batch geometry -> new gradient slabs, .to(), load_state_dict)
        group_of = {name: gi for gi, g in enumerate(self.param_groups) for name in g['names']}
        # bf16 compute: the update kernel also writes the rounded value of every weight MATRIX into its slot of the stacked GEMM-ready
        # copies (models.VAR._matrix_copies), so the step does not re-read the fp32 masters to rebuild them (stack + cast were 3.4 ms)
        copies, fresh = (self.var._matrix_copies() if self.fuse_copies and hasattr(self.var, '_matrix_copies') and not self.lora
                         else ({}, ()))
        if not set(copies) <= {name for name, _ in self.named}:
            copies, fresh = {}, ()
        sig = (tuple(p.data_ptr() for _, p in self.named) + tuple(grads[name].data_ptr() for name, _ in self.named) +
               tuple(c.data_ptr() for c in copies.values()))
        if self._table is None or self._table_sig != sig:
            entries = [(p.data, grads[name], self.state[name][0], self.state[name][1], group_of[name], copies.get(name)) for name, p in self.named]
            self._table = ops.adam_table(entries, dev)
            self._table_sig = sig
        ops.sumsq_multi(self._table, n, self._partial)
        gscale = AccumWindow.grad_scale(world, accum)
        ops.clip_coef(self._partial, n * 256, gscale, float(max_norm), self._out2)
        self.steps += 1
        coef = self._out2[1:]
        ops.adamw_multi(self._table, n, [float(g['lr']) for g in self.param_groups], [float(g['weight_decay']) for g in self.param_groups],
                        self.betas[0], self.betas[1], self.eps, self.steps, coef, gscale)
        if fresh:
            self.var._pack(fresh=fresh)                          # the matrices are current; biases / tables are rebuilt from the parameters
        else:
            self.var._packed = None                              # GEMM-ready copies are refreshed lazily (LoRA: re-merged with the new adapters)
        return self._out2

    # ---- wire format of torch.optim.AdamW.state_dict() (what train_control_var_hpu.py:420-447 saves and resumes)
    def state_dict(self) -> Dict[str, object]:
        state, groups, at = {}, [], 0
        for g in self.param_groups:
            idx = list(range(at, at + len(g['names'])))
            at += len(idx)
            if self.steps > 0:
                for i, name in zip(idx, g['names']):
                    m, v = self.state[name]
                    state[i] = {'step': torch.tensor(float(self.steps)), 'exp_avg': m, 'exp_avg_sq': v}
            groups.append({'lr': g['lr'], 'betas': tuple(self.betas), 'eps': self.eps, 'weight_decay': g['weight_decay'], 'amsgrad': False,
                           'maximize': False, 'foreach': None, 'capturable': False, 'differentiable': False, 'fused': None,
                           'decoupled_weight_decay': True, 'wd_sc': g['wd_sc'], 'lr_sc': g['lr_sc'], 'params': idx})
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, sd: Dict[str, object]) -> None:
        groups = sd['param_groups']
        if len(groups) != len(self.param_groups) or any(len(a['params']) != len(b['names']) for a, b in zip(groups, self.param_groups)):
            raise ValueError('loaded state dict has a different number / size of parameter groups')     # torch's own check
        steps = set()
        for saved, g in zip(groups, self.param_groups):
            for k in ('lr', 'weight_decay', 'wd_sc', 'lr_sc'):
                if k in saved:
                    g[k] = saved[k]
            if 'betas' in saved:
                self.betas = tuple(saved['betas'])
            self.eps = saved.get('eps', self.eps)
            for i, name in zip(saved['params'], g['names']):
                st = sd['state'].get(i)
                m, v = self.state[name]
                if st is None:
                    m.zero_(); v.zero_()
                    continue
                if tuple(st['exp_avg'].shape) != tuple(m.shape):
                    raise ValueError(f'optimizer state for {name}: shape {tuple(st["exp_avg"].shape)} != {tuple(m.shape)}')
                m.copy_(st['exp_avg']); v.copy_(st['exp_avg_sq'])
                steps.add(int(float(st['step'])))
        if len(steps) > 1:
            raise ValueError(f'per-parameter step counts differ ({sorted(steps)}); the fused optimizer keeps one')
        self.steps = steps.pop() if steps else 0


class Trainer:
    """One process per GPU; the step of train_control_var_hpu.py:130-255 (minus its logging and its own accumulation quirk: it steps the
    optimizer every batch and zeroes the gradients every N-th).

    grad_accum=N accumulates gradients over windows of N calls of step() with the semantics of `accelerator.accumulate` (train.py:105,
    train_var.py:112, train_control_var.py:130): step() is called once per micro-batch, as the reference's loop body is; calls 1 .. N-1 of a
    window run tokenizer, forward and backward only, call N also all-reduces, clips, steps AdamW with the mean of the N micro-batch gradients
    (micro-batches weigh the same whatever their size) and advances `it`.  The lr / wd schedule counts optimizer steps.  N = 1 is the plain
    step.  See AccumWindow and DESIGN.md 8c."""

    def __init__(self, var, vae, peak_lr: float, weight_decay: float, weight_decay_end: Optional[float] = None, sche: str = 'lin0',
                 warmup_it: float = 0, max_it: int = 1000, clip: float = 2.0, wp0: float = 0.005, wpe: float = 0.01, drop_path: bool = True,
                 train_mode: Optional[bool] = None, force_reducer: bool = False, grad_accum: int = 1):
        """train_mode: True puts the model in train() (DropPath active, as the reference's loop runs it, train_control_var_hpu.py:136),
        False in eval(); None leaves the mode as the caller set it."""
        import torch.distributed as dist
        self.window = AccumWindow(grad_accum)           # refuses N < 1 before anything is built
        self.grad_accum = grad_accum
        self._loss_sum = None
        self.var, self.vae = var, vae
        if train_mode is not None:
            var.train(train_mode)
        self.engine = TrainEngine(var, drop_path=drop_path)
        self.opt = FusedAdamW(var, lr=peak_lr, weight_decay=weight_decay)
        self.sched = dict(sche=sche, peak_lr=peak_lr, wd=weight_decay, wd_end=weight_decay if weight_decay_end is None else weight_decay_end,
                          wp_it=warmup_it, max_it=max_it, wp0=wp0, wpe=wpe)
        self.clip = clip
        self.world = dist.get_world_size() if dist.is_initialized() else 1
        self.force_reducer = force_reducer
        self.comm = True                        # False: skip the gradient exchange (bench.py measures the exposed communication time with it)
        self.comm_group = None                  # process group of the gradient exchange (None = default); see set_comm_group
        self._reducer_for = None

    @property
    def it(self) -> int:
        """optimizer steps taken (the iteration the lr / wd schedule is evaluated at)"""
        return self.window.it

    @it.setter
    def it(self, value: int):
        self.window.it = int(value)

    def set_comm_group(self, group):
        """run the gradient all-reduce in `group` from the next step on (launcher.channel_groups: one group per RCCL channel cap)"""
        self.comm_group = group
        self._reducer_for = None

    @torch.no_grad()
    def tokenize(self, images: torch.Tensor, masks: torch.Tensor, mask_first: bool = True):
        """frozen tokenizer + 'interleave_append' (mask first unless bidirectional drew image first): train_control_var_hpu.py:157-204"""
        # one tokenizer pass over [masks ; images] (the reference makes two calls, :160-176): the ten-scale residual quantiser is one latency-bound
        # launch of ~2.7 ms whatever the batch, and the conv stack sees twice the tiles.  Every image is encoded and quantised on its own and no kernel of the
        # tokenizer sums in a batch-dependent order, so the ids equal the two-call form's exactly in both precision modes
        # (tests/test_gpu_train.py::test_tokenize_one_pass_equals_the_two_call_form)
        B = masks.shape[0]
        return self._inputs_of(self.vae.img_to_idxBl(torch.cat((masks, images), dim=0)), B, mask_first)

    @torch.no_grad()
    def _inputs_of(self, both: List[torch.Tensor], B: int, mask_first: bool = True):
        """the ids of a batch -> (teacher-forcing input x, labels): per scale (2 B, pn^2) ids, the control halves of the B samples above their
        image halves - what the one-pass tokenizer returns and what step_tokens stacks - or, for a plain VAR, (B, pn^2)"""
        hboth = self.vae.idxBl_to_h(both)
        if self.var.cfg.mask_factor != 2:
            return torch.cat(hboth, dim=1), torch.cat(both, dim=1)
        mi, ii = [t[:B] for t in both], [t[B:] for t in both]
        mh, ih = [t[:B] for t in hboth], [t[B:] for t in hboth]
        if not mask_first:
            mi, ii, mh, ih = ii, mi, ih, mh
        x = torch.cat([torch.cat((a, b), 1) for a, b in zip(mh, ih)], dim=1)
        cfg = self.var.cfg
        if cfg.separator:           # train_control_var_hpu.py:214-224: the label of a separator is V + its special_embed row
            mapping = cfg.special_mapping(mask_first)
            parts = [mi[0], ii[0]]
            for k in range(1, len(mi)):
                for h, ids in enumerate((mi[k], ii[k])):
                    parts += [ids, ids.new_full((ids.shape[0], 1), cfg.vocab + mapping[2 * (k - 1) + h])]
            labels = torch.cat(parts, dim=1)
        else:
            labels = torch.cat([torch.cat((a, b), 1) for a, b in zip(mi, ii)], dim=1)
        return x, labels

    @torch.no_grad()
    def step(self, images, masks, cls, types, ignore_mask=None, drop_seed=None, mask_first: Optional[bool] = None) -> Dict[str, object]:
        """mask_first=None draws the order as the reference does (image first with probability 1/2 when the model is bidirectional,
        python `random`, train_control_var_hpu.py:192-199); pass the matching ``ignore_mask`` / ``ignore_mask_`` (:234).  It is drawn per
        call, as the reference draws it per batch; ``drop_seed`` is per call too.

        One call = one micro-batch.  The returned dict carries ``micro`` (index inside the window) and ``synced`` (this call closed the window
        and stepped the optimizer).  A call that does not sync returns its micro-batch loss and ``grad_norm`` / ``clip_coef`` None; the one
        that does returns the last micro-batch's ``loss`` next to ``window_loss``, the mean of the window's micro-batch losses."""
        if mask_first is None:
            import random
            mask_first = not (getattr(self.var, 'bidirectional', False) and random.random() < 0.5)
        return self._micro_batch(lambda: self.tokenize(images, masks, mask_first), cls, types, ignore_mask, drop_seed, mask_first)

    def _micro_batch(self, inputs, cls, types, ignore_mask, drop_seed, mask_first: bool, policy: Optional[PolicyLoss] = None,
                     distill: Optional[DistillLoss] = None) -> Dict[str, object]:
        """one micro-batch of the window on the (x, labels) that inputs() returns: schedule, forward + backward, and - when it closes the window -
        all-reduce, clipping, AdamW.  The body of step() and of step_tokens()"""
        micro, accumulate, sync = self.window.begin()
        s = self.sched
        _, max_lr, _, max_wd = lr_wd_annealing(s['sche'], self.opt, s['peak_lr'], s['wd'], s['wd_end'], self.it, s['wp_it'], s['max_it'], wp0=s['wp0'], wpe=s['wpe'])
        x, labels = inputs()
        self.engine._setup(x.shape[0])
        if (self.world > 1 or self.force_reducer) and self.comm and sync:         # the all-reduce rides on the backward that closes the window
            if self._reducer_for is not self.engine.buckets:
                self._reducer = BucketReducer(self.engine.buckets, group=self.comm_group, force=self.force_reducer)
                self._reducer_for = self.engine.buckets
            self.engine.reducer = self._reducer
        else:
            self.engine.reducer = None
        loss, _ = self.engine.forward_backward(cls, x, types, labels, ignore_mask, drop_seed, mask_first, accumulate=accumulate, policy=policy, distill=distill)
        extra = self._policy_report(x.shape[0], ignore_mask) if policy is not None else {}
        n = self.window.n
        if n > 1:
            self._loss_sum = loss if micro == 0 else self._loss_sum + loss
        if not sync:
            self.window.end()
            return dict(loss=loss, grad_norm=None, clip_coef=None, lr=max_lr, wd=max_wd, mask_first=mask_first, synced=False, micro=micro, **extra)
        if self.engine.reducer is not None:
            self.engine.reducer.wait()
        norm_coef = self.opt.step(self.engine.grads(), self.clip, self.world, n)
        if self.engine._lora is None:                # LoRA: the base weights (and their W^T copies) do not move
            self.engine._transposed_weights()
        self.window.end()
        window_loss = self._loss_sum / n if n > 1 else loss
        return dict(loss=loss, window_loss=window_loss, grad_norm=norm_coef[0], clip_coef=norm_coef[1], lr=max_lr, wd=max_wd, mask_first=mask_first,
                    synced=True, micro=micro, **extra)

    # ---------------------------------------------------------------- training on token ids
    def _policy_report(self, B: int, ignore_mask) -> Dict[str, object]:
        """what a policy step adds to the returned dict: means over the tokens that count (weight != 0; all of them without ignore_mask) as
        device scalars, and the (B, L) log-probabilities the step saw"""
        po = self.engine.policy_out
        if ignore_mask is None:
            mean = lambda t: t.float().mean()
        else:
            live = (ignore_mask.to(device=po['ratio'].device).reshape(-1) != 0).float()
            mean = lambda t: (t.float() * live).sum() / live.sum().clamp(min=1.0)
        return dict(mean_ratio=mean(po['ratio']), clip_frac=mean(po['clipped']), mean_kl=mean(po['kl']), token_logprob=po['logprob'].view(B, -1))

    def _check_tokens(self, ids_img, ids_ctrl, cls, types, mask_first: Optional[bool]):
        """the host side of step_tokens / token_logprobs, before any device work -> (per scale the stacked ids _inputs_of takes, B, mask_first)"""
        from .models import _check_index_range, _flat_ids
        cfg = self.var.cfg
        if cfg.separator:
            raise NotImplementedError(_NO_SEPARATOR)
        bidir = bool(getattr(self.var, 'bidirectional', False))
        if mask_first is None:
            if bidir:
                raise ValueError('mask_first: a bidirectional model lays either half first - say which order these ids are in (step() draws it, '
                                 'given ids have one)')
            mask_first = True
        if not mask_first and not bidir:
            raise ValueError('mask_first=False: only a bidirectional model lays the image half first')
        if not torch.is_tensor(cls) or cls.dim() != 1 or cls.is_floating_point():
            raise ValueError(f'cls: expected integer class labels of shape (B,), got {tuple(cls.shape) if torch.is_tensor(cls) else type(cls).__name__}')
        B, pns, mf = cls.shape[0], cfg.pyramid.patch_nums, cfg.mask_factor
        _check_index_range(cls, 0, cfg.num_classes, 'cls')
        if mf == 2 and types is not None:
            if not torch.is_tensor(types) or tuple(types.shape) != (B,) or types.is_floating_point():
                raise ValueError(f'types: expected integer control types of shape ({B},)')
            _check_index_range(types, 0, 4, 'types')
        img = _flat_ids('ids_img', ids_img, B, pns, cfg.vocab)
        if mf == 2:
            if ids_ctrl is None:
                raise ValueError('ids_ctrl: a ControlVAR sample is its control half and its image half - pass both')
            ctrl = _flat_ids('ids_ctrl', ids_ctrl, B, pns, cfg.vocab)
            flat = torch.cat((ctrl.to(self.var.device), img.to(self.var.device)), dim=0).long()
        else:
            if ids_ctrl is not None:
                raise ValueError('ids_ctrl: a plain VAR has the image half only')
            flat = img.to(self.var.device).long()
        both, o = [], 0
        for pn in pns:
            both.append(flat[:, o:o + pn * pn])
            o += pn * pn
        return both, B, mask_first

    @torch.no_grad()
    def step_tokens(self, ids_img, ids_ctrl, cls, types, *, ignore_mask=None, policy: Optional[PolicyLoss] = None, drop_seed=None,
                    mask_first: Optional[bool] = None, distill=None) -> Dict[str, object]:
        """step() on token ids instead of pixels: one micro-batch with step()'s window, schedule, all-reduce, clipping and return dict, without
        the tokenizer.  ids_img / ids_ctrl: each half's multi-scale ids in the forms score_infer_cfg takes - the list of (B, pn^2) tensors
        vae.img_to_idxBl returns or one (B, sum pn^2) tensor - so a sampled sequence or a pre-tokenised dataset trains as it is; ids_ctrl=None
        for a plain VAR.  On the ids of tokenize() the step equals step() on the pixels bit for bit.
        policy: a PolicyLoss replaces the cross-entropy by the clipped policy-gradient loss; the dict then also carries mean_ratio, clip_frac,
        mean_kl (device scalars over the tokens that count) and token_logprob (B, L) in TokenScores' token order.
        distill: a DistillLoss replaces the cross-entropy by KL(teacher || model) on the teacher logits it carries; the ids
        are then the model's inputs only, `loss` is the weighted mean KL, distill.weights stands where ignore_mask stands (not both) and
        policy is excluded.  DistillTargets.loss() of a generation call with distill_targets=True is such an object; the student is trained
        with cond_drop_rate = 0.  A SparseDistillLoss (SparseDistillTargets.loss() of distill_topn=N, TokenScores.sparse_loss() of
        top_logprobs=N) takes the same place with the teacher's N most likely codes and its tail mass.
        Shapes and the id range are checked on the host before any device work.  Separator models are refused; a bidirectional model needs
        mask_first said (True: these ids go control first)."""
        both, B, mask_first = self._check_tokens(ids_img, ids_ctrl, cls, types, mask_first)
        if policy is not None:
            if not isinstance(policy, PolicyLoss):
                raise TypeError(f'policy: a PolicyLoss, got {type(policy).__name__}')
            policy.check(B, self.var.cfg.pyramid.L)
        if distill is not None:
            if policy is not None:
                raise ValueError('distill and policy: a step has one loss - the soft-target loss or the policy-gradient loss')
            if not isinstance(distill, _DISTILL_FORMS):
                raise TypeError(f'distill: a DistillLoss or a SparseDistillLoss, got {type(distill).__name__}')
            if distill.weights is not None and ignore_mask is not None:
                raise ValueError('distill.weights and ignore_mask: the weights take the place of ignore_mask - fold the two into one and pass it as weights')
            if self.var.cfg.vocab != self.var.cfg.head_ld:
                raise NotImplementedError(f'distill: the head is {self.var.cfg.head_ld} columns wide for a vocabulary of {self.var.cfg.vocab}; teacher logits are (B, L, vocab)')
            distill.check(B, self.var.cfg.pyramid.L, self.var.cfg.vocab, self.var.device)
        if ignore_mask is not None and ignore_mask.numel() != B * self.var.cfg.pyramid.L:
            raise ValueError(f'ignore_mask: expected {B} x {self.var.cfg.pyramid.L} token weights, got {tuple(ignore_mask.shape)}')
        return self._micro_batch(lambda: self._inputs_of(both, B, mask_first), cls, types, ignore_mask, drop_seed, mask_first, policy, distill)

    @torch.no_grad()
    def token_logprobs(self, ids_img, ids_ctrl, cls, types, *, drop_seed=None, mask_first: Optional[bool] = None) -> torch.Tensor:
        """-> (B, L) fp32: the log-probability of every given token under the model as the TRAINING forward sees it (the model's current mode,
        DropPath and adapter dropout drawn from drop_seed), in TokenScores' token order - the producer of PolicyLoss.old_logprob /
        ref_logprob.  The forward is forward_train and the log-probability the negated per-token loss of a loss-only cvar_ce_fwd_bwd, so with
        unchanged parameters and the same drop_seed a following policy step sees ratio == 1.0f in every token (a model with cond_drop_rate > 0
        draws its condition dropout per forward, outside drop_seed).  No backward runs, no gradient buffer is written, the accumulation window
        and `it` stay where they are.  mask_first=None: True, except that a bidirectional model must say it.  Refusals as step_tokens."""
        both, B, mask_first = self._check_tokens(ids_img, ids_ctrl, cls, types, mask_first)
        x, labels = self._inputs_of(both, B, mask_first)
        eng = self.engine
        eng.forward_train(cls, x, types, drop_seed, mask_first)
        tg = labels.to(device=self.var.device, dtype=torch.int32).contiguous().view(-1)
        ops.ce_fwd_bwd(eng.logits, tg, None, 1.0, eng.loss_tok, None, eng.M, eng.V)
        return (-eng.loss_tok).view(B, -1)


class _TeacherForcedFn(torch.autograd.Function):
    """Autograd bridge so that the reference's own training code (`logits = var(...)`; `loss.backward()`,
    train_control_var_hpu.py:207-241) works unchanged: forward keeps the activations inside the engine, backward runs the
    hand-written kernels and hands one gradient per parameter back to autograd."""

    @staticmethod
    def forward(ctx, engine, label_B, x, cond_type, mask_first, *params):
        logits = engine.forward_train(label_B, x, cond_type, None, mask_first)
        ctx.engine = engine
        B = x.shape[0]
        return logits.view(B, -1, logits.shape[-1])[:, :, :engine.cfg.head_out].clone()       # head_ld padding columns are not part of the API

    @staticmethod
    def backward(ctx, dlogits):
        eng = ctx.engine
        if eng.cfg.head_ld != eng.cfg.head_out:
            eng.dlogits.zero_()
        eng.dlogits[:, :eng.cfg.head_out].copy_(dlogits.reshape(eng.M, -1))
        eng.backward()
        g = eng.grads()
        return (None, None, None, None, None) + tuple(g[n].clone() if n in g else None for n, _ in eng.var.named_parameters())


def teacher_forced_with_grad(var, label_B, x, cond_type, mask_first: bool = True):
    eng = getattr(var, '_train_engine', None)
    if eng is None:
        eng = var._train_engine = TrainEngine(var, drop_path=True)
    return _TeacherForcedFn.apply(eng, label_B, x, cond_type, mask_first, *[p for _, p in var.named_parameters()])
