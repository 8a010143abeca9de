"""Host-side mirror of the reference's model API (models/__init__.py, models/vqvae.py,
models/var.py, models/control_var.py) over the HIP kernels of libcvar_hip.so.

Same class names, constructor keywords, method names / argument meaning and state_dict keys
as the reference, so a checkpoint (or a caller such as train_control_var_hpu.py:157-176,288,
322,332) works unchanged; the computation is organised MI355X-first instead of nn.Module-per-op:
weights are packed once into GEMM-ready device buffers, the KV cache is a preallocated arena
written by the QKV GEMM's epilogue, adaLN parameters are computed once per generation, and every
scale step runs as a short sequence of fused kernels.  There is no CPU / eager fallback.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn as nn

from . import ops
from . import _lib
from ._lib import CvarError
from ._lib import ACT_GELU_TANH
from .pyramid import packed_tables
from .spec import DEFAULT_PATCH_NUMS, VaeConfig, check_latent_size, VarConfig, attention_levels, vae_state_shapes, var_state_shapes
from .synth import synth_vae_state, synth_var_state


class _Tree(nn.Module):
    """plain container so that dotted state_dict keys map onto nested attributes"""


def _register_tree(root: nn.Module, shapes, values: Dict[str, torch.Tensor], requires_grad: bool):
    for key, (shape, kind) in shapes.items():
        parts = key.split('.')
        m = root
        for p in parts[:-1]:
            if p not in m._modules:
                m.add_module(p, _Tree())
            m = m._modules[p]
        t = values[key]
        assert tuple(t.shape) == tuple(shape), key
        if kind == 'param':
            m.register_parameter(parts[-1], nn.Parameter(t, requires_grad=requires_grad and t.is_floating_point()))
        else:
            m.register_buffer(parts[-1], t)


def _tensor_sig(module: nn.Module):
    """identity + in-place-version stamp of every parameter and buffer: changes when a tensor is replaced (load_state_dict(assign),
    .data swaps, .to()) or written in place through autograd-visible ops (torch.optim steps, p.mul_(), p.copy_())"""
    return tuple((t.data_ptr(), t._version) for t in list(module.parameters(recurse=True)) + list(module.buffers(recurse=True)))


def _check_index_range(t: torch.Tensor, lo: int, hi: int, what: str):
    """nn.Embedding raises on an out-of-range index (the reference's failure mode); the gather kernels read unchecked, so ids are
    validated here: for free on host tensors, with one tiny reduction + read-back on device tensors (outside any graph capture)."""
    if t.numel() == 0:
        return
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    mn, mx = (int(v) for v in torch.stack((t.min(), t.max())).tolist())
    if mn < lo or mx > hi:
        raise IndexError(f'{what}: index out of range (got [{mn}, {mx}], valid [{lo}, {hi}])')


def _compute_dtype(d) -> torch.dtype:
    if isinstance(d, torch.dtype):
        return d
    return {'bf16': torch.bfloat16, 'bfloat16': torch.bfloat16, 'fp32': torch.float32, 'f32': torch.float32, 'float32': torch.float32}[d]


# =====================================================================================
# VQVAE
# =====================================================================================
class VQVAE(nn.Module):
    """Multi-scale VQVAE tokenizer (reference: models/vqvae.py:16-109).

    compute_dtype: torch.bfloat16 (throughput mode: bf16 NHWC activations, fp32 accumulate) or
    torch.float32 (parity mode: exact-f32 MFMA).  The quantizer itself always runs in fp32.
    """

    def __init__(self, vocab_size=4096, z_channels=32, ch=128, dropout=0.0, beta=0.25, using_znorm=False, quant_conv_ks=3,
                 quant_resi=0.5, share_quant_resi=4, default_qresi_counts=0, v_patch_nums=DEFAULT_PATCH_NUMS, test_mode=True,
                 compute_dtype=torch.bfloat16, init_seed: int = 0, decode_chunk: Optional[int] = None, encoder_precision: Optional[str] = None):
        """v_patch_nums fixes the latent size S = v_patch_nums[-1] and with it the image size 16 S: DEFAULT_PATCH_NUMS (S = 16, 256 x 256 images) or
        PATCH_NUMS_512 (S = 32, 512 x 512); any other S raises NotImplementedError (the quantizer kernels are built for these two).
        encoder_precision (bf16 compute only; None = 'bf16'): arithmetic of the ENCODER conv stack in front of the exact quantizer -
        'bf16' (throughput), 'bf16x3' (split-bf16: every operand as hi + lo bf16, three MFMA products per multiply, fp32 accumulate and fp32 activations:
        ~2^-16 relative error per product, ids agree with the reference's fp32 encoder far beyond plain bf16 at about a third of its encoder rate) or 'fp32'
        (the parity mode's exact-f32 MFMA for the encoder only).  The decoder keeps compute_dtype either way."""
        super().__init__()
        check_latent_size(tuple(v_patch_nums)[-1])
        if using_znorm or quant_conv_ks != 3 or abs(quant_resi - 0.5) > 1e-9 or share_quant_resi != 4 or dropout != 0.0:
            raise NotImplementedError('only the shipped VQVAE configuration (vqvae.py:18-27 defaults, share_quant_resi=4) is built')
        self.cfg = VaeConfig(vocab=vocab_size, z_channels=z_channels, ch=ch, share_quant_resi=share_quant_resi,
                             patch_nums=tuple(v_patch_nums))
        self.test_mode = test_mode
        self.V = self.vocab_size = vocab_size
        self.Cvae = z_channels
        self.downsample = 2 ** (len(self.cfg.ch_mult) - 1)
        self.compute_dtype = _compute_dtype(compute_dtype)
        ep = encoder_precision or ('bf16' if self.compute_dtype == torch.bfloat16 else 'fp32')
        if ep not in ('bf16', 'bf16x3', 'fp32') or (self.compute_dtype == torch.float32 and ep != 'fp32'):
            raise ValueError(f'encoder_precision={encoder_precision!r}: one of bf16 / bf16x3 / fp32 (an fp32 model encodes in fp32)')
        self.encoder_precision = ep
        # images per decoder pass (an image's bits do not depend on it).  128 since round 5: VQVAE round trip 1 355 -> 1 373-1 379 images/s, headline +0.4 % at the
        # same 226 GB peak (64 / 128 / 256: 201.5 / 202.3 / 202.0 images/s on one box).  A 512 x 512 image has 4 x the pixels at every decoder level, so 4 x the
        # activation bytes per image (the widest tensors, (B, 512 * 512, 160) bf16, are 84 MB each against 21 MB) and its 1 024 x 1 024 attention scores add
        # 4 MB fp32 + 2 MB bf16 per image and block: 32 images per pass keep the 256 x 256 pass's footprint.
        self.decode_chunk = decode_chunk if decode_chunk is not None else (128 if self.cfg.patch_nums[-1] <= 16 else 32)
        _register_tree(self, vae_state_shapes(self.cfg), synth_vae_state(self.cfg, init_seed), requires_grad=not test_mode)
        self._packed = None
        if test_mode:
            self.eval()

    # ---- nn.Module plumbing
    def load_state_dict(self, state_dict: Dict[str, Any], strict=True, assign=False):
        key = 'quantize.ema_vocab_hit_SV'
        if key in state_dict and state_dict[key].shape[0] != self.quantize.ema_vocab_hit_SV.shape[0]:
            state_dict = dict(state_dict)
            state_dict[key] = self.quantize.ema_vocab_hit_SV          # vqvae.py:106-108
        self._packed = None
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.quant_conv.weight.device

    # ---- weight packing (one-time layout work, not on the timed path)
    def _state_sig(self):
        return _tensor_sig(self)

    def _pack(self, check: bool = False):
        """GEMM-ready device copies of the weights.  check=True (public entry points): rebuild them when any parameter / buffer
        was replaced or modified in place since they were made (optimizer steps, manual edits, .data swaps)."""
        if self._packed is not None and (not check or self._packed_sig == self._state_sig()):
            return self._packed
        dev, T = self.device, self.compute_dtype
        if dev.type != 'cuda':
            raise RuntimeError('controlvar_amd.VQVAE computes on the GPU only; call .to("cuda") first')
        kch = 8 if T == torch.bfloat16 else 4
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        P: Dict[str, Any] = {'conv': {}, 'norm': {}}
        for k, v in sd.items():
            if k.endswith('.weight') and v.dim() == 4 and not k.startswith('quantize.'):
                name = k[:-len('.weight')]
                fp32_only = name in ('quant_conv', 'post_quant_conv')        # quantizer side stays fp32
                Tw = torch.float32 if fp32_only else T
                kc = 4 if fp32_only else kch
                cout, cin, ks, _ = v.shape
                if ks == 3:
                    cin_p = (cin + kc - 1) // kc * kc
                    w = torch.zeros(cout, 3, 3, cin_p, device=dev, dtype=torch.float32)
                    w[..., :cin] = v.permute(0, 2, 3, 1)
                    w = w.reshape(cout, 9 * cin_p)
                else:
                    cin_p = cin
                    w = v.reshape(cout, cin)
                P['conv'][name] = dict(w=w.to(Tw).contiguous(), b=sd[name + '.bias'].float().contiguous(), cin=cin_p, cout=cout, ks=ks)
                if name.startswith('encoder.') and T == torch.bfloat16 and self.encoder_precision != 'bf16':
                    P.setdefault('enc', {})[name] = self._pack_encoder_conv(v, sd[name + '.bias'], dev)
            elif '.norm' in k and k.endswith('.weight'):
                name = k[:-len('.weight')]
                P['norm'][name] = (v.float().contiguous(), sd[name + '.bias'].float().contiguous())
        P['E'] = sd['quantize.embedding.weight'].float().contiguous()
        nphi = self.cfg.share_quant_resi
        pw = torch.stack([sd[f'quantize.quant_resi.qresi_ls.{k}.weight'] for k in range(nphi)])      # (k, co, ci, 3, 3)
        P['phi_w'] = pw.permute(0, 2, 3, 4, 1).reshape(nphi, self.Cvae, 9, self.Cvae).float().contiguous()   # [k][ci][tap][co]
        P['phi_b'] = torch.stack([sd[f'quantize.quant_resi.qresi_ls.{k}.bias'] for k in range(nphi)]).float().contiguous()
        # Phi as ONE conv for the generic conv path (low-resolution reconstructions): h (1 - r) + (conv(h) + b) r = conv'(h) + b r with the
        # identity folded into the centre tap, W' = r W + (1 - r) I  (quant.py:263-270)
        r = float(self.cfg.quant_resi)
        pf = pw.float() * r                                                                       # (k, co, ci, 3, 3)
        pf[:, torch.arange(self.Cvae), torch.arange(self.Cvae), 1, 1] += 1.0 - r
        P['phi_fold_w'] = pf.permute(0, 1, 3, 4, 2).reshape(nphi, self.Cvae, 9 * self.Cvae).contiguous()   # [k][co][tap][ci]
        P['phi_fold_b'] = (P['phi_b'] * r).contiguous()
        up, down, offs = packed_tables(self.cfg.patch_nums)
        P['up'] = torch.from_numpy(up).to(dev)
        P['down'] = torch.from_numpy(down).to(dev)
        P['tab_off'] = [int(o) for o in offs]
        P['phi_map'] = self.cfg.phi_map
        self._packed = P
        self._packed_sig = self._state_sig()
        return P

    def _pack_encoder_conv(self, v, bias, dev):
        """encoder weights of the non-default encoder precisions: 'fp32' = the parity mode's packing; 'bf16x3' = per tap [w_hi | w_hi | w_lo] over 3 x cin channels
        (the weight side of the split product, include/cvar.h cvar_split3)"""
        cout, cin, ks, _ = v.shape
        cin_p = (cin + 3) // 4 * 4
        w = torch.zeros(cout, ks, ks, cin_p, device=dev, dtype=torch.float32)
        w[..., :cin] = v.permute(0, 2, 3, 1).float()
        b = bias.float().contiguous()
        if self.encoder_precision == 'fp32':
            return dict(w=w.reshape(cout, ks * ks * cin_p).contiguous(), b=b, cin=cin_p, cout=cout, ks=ks)
        hi = w.to(torch.bfloat16)
        lo = (w - hi.float()).to(torch.bfloat16)
        cin3 = (3 * cin_p + 7) // 8 * 8                                       # bf16 K moves 16-byte chunks
        w3 = torch.zeros(cout, ks, ks, cin3, device=dev, dtype=torch.bfloat16)
        w3[..., :cin_p], w3[..., cin_p:2 * cin_p], w3[..., 2 * cin_p:3 * cin_p] = hi, hi, lo
        return dict(w=w3.reshape(cout, ks * ks * cin3).contiguous(), b=b, cin=cin_p, cin3=cin3, cout=cout, ks=ks)

    # ---- conv-stack building blocks (NHWC activations of compute dtype)
    # GroupNorm statistics from the producing conv's epilogue (round 5): a 3x3 conv that the LDS-halo kernel takes writes per-tile partial sums of its
    # output next to it; the GroupNorm that reads that tensor then skips its statistics pass (7 % of a VQVAE round trip).  The partials ride on the
    # tensor object (``_gn_part``): whoever consumes the tensor without a GroupNorm simply ignores them.  Class-level switch for A/B runs and tests.
    GN_FROM_CONV = True

    # The encoder of a bf16 model in its higher precisions (encoder_precision 'fp32' / 'bf16x3') is the same layer walk over other conv and GroupNorm leaves: fp32 NHWC
    # activations throughout; 'fp32' = the parity mode's exact-f32 MFMA, 'bf16x3' = every conv input split into [hi | lo | hi] bf16 rows (by the GroupNorm that feeds it,
    # or by cvar_split3) and contracted with [w_hi | w_hi | w_lo] rows on the bf16 tiles.  The 16 x 16 attention blocks (0.1 % of the encoder's flops) then run q k^T and
    # p v on the exact-f32 MFMA, as every fp32 tensor does.  _conv and _gn pick the leaf by the layer's name; everything outside 'encoder.' is native.
    def _encoder_leaf(self, name: str) -> Optional[str]:
        """'fp32' / 'bf16x3' when layer `name` runs in the encoder's own precision, None for the native leaf (compute dtype)"""
        if name.startswith('encoder.') and self.compute_dtype == torch.bfloat16 and self.encoder_precision != 'bf16':
            return self.encoder_precision
        return None

    def _conv(self, x, name, B, Hin, Win, *, stride=1, up=0, residual=None, out_dtype=None):
        leaf = self._encoder_leaf(name)
        c = self._pack()['conv' if leaf is None else 'enc'][name]
        T, cin = c['w'].dtype, c['cin']
        if leaf == 'bf16x3':
            cin = c['cin3']
            if x.dtype != torch.bfloat16:           # not split by the GroupNorm in front (split rows are the only bf16 tensors of this stream)
                xs = torch.empty(B * Hin * Win, cin, device=x.device, dtype=torch.bfloat16)
                x = ops.split3(x, xs, B * Hin * Win, c['cin'], cin)
        out_dtype = out_dtype or (T if leaf is None else torch.float32)
        if c['ks'] == 1:
            M = B * Hin * Win
            out = torch.empty(M, c['cout'], device=x.device, dtype=out_dtype)
            # never split along K: with the tile kernels alone a row's sum order does not depend on M, so an image decodes / encodes to the same bits in any batch
            ops.gemm(x, c['w'], out, M=M, N=c['cout'], K=cin, bias=c['b'], residual=residual, split_k=False)
            return out, Hin, Win
        Hout = Hin * 2 if up else (Hin // 2 if stride == 2 else Hin)
        Wout = Win * 2 if up else (Win // 2 if stride == 2 else Win)
        M = B * Hout * Wout
        out = torch.empty(M, c['cout'], device=x.device, dtype=out_dtype)
        geo = ops.conv_gn_partials(T, stride, cin, c['cout'], Hin, Win, Hout, Wout) if (leaf is None and self.GN_FROM_CONV and out.dtype == T) else None
        part = torch.empty(B, geo[0], c['cout'], 3, device=x.device, dtype=torch.float32) if geo else None
        cv = dict(Hin=Hin, Win=Win, Cin=cin, Hout=Hout, Wout=Wout, stride=stride, up=up)
        try:
            ops.gemm(x, c['w'], out, M=M, N=c['cout'], K=9 * cin, bias=c['b'], residual=residual, conv=cv, gn_part=part)
        except CvarError as e:
            # conv_gn_partials() decides by shape alone; the kernel that emits the partials also needs 16-byte aligned bias / output / residual and dense
            # strides (a state dict assigned from a flat buffer can hand over a 4-byte aligned bias).  Such a call is unsupported WITH partials, not
            # without: run it on the implicit-GEMM tiles and let the GroupNorm that follows make its own statistics pass.
            if part is None or 'unsupported' not in str(e).lower():
                raise
            geo, part = None, None
            ops.gemm(x, c['w'], out, M=M, N=c['cout'], K=9 * cin, bias=c['b'], residual=residual, conv=cv)
        if geo:
            out._gn_part = (part, geo[0], geo[1])
        return out, Hout, Wout

    def _hp_conv(self, x, name, B, Hin, Win, **kw):
        """one encoder conv in the encoder's own precision: the name under which tests/test_gpu_encoder_precision.py calls that leaf of _conv"""
        if self._encoder_leaf(name) is None:
            raise ValueError(f'{name}: not a layer that runs in an encoder precision of its own')
        return self._conv(x, name, B, Hin, Win, **kw)

    def _gn(self, x, name, B, HW, C, silu=True):
        w, b = self._pack()['norm'][name]
        ws = torch.empty(ops.groupnorm_ws_bytes(B, HW, C), device=x.device, dtype=torch.uint8)
        if self._encoder_leaf(name) == 'bf16x3':        # GroupNorm(+SiLU) of the fp32 stream -> split rows, the next conv's operand
            out = torch.empty(B * HW, 3 * C, device=x.device, dtype=torch.bfloat16)
            return ops.groupnorm_silu_split3(x, w, b, out, B, HW, C, self.cfg.gn_groups, self.cfg.gn_eps, silu, ws)
        out = torch.empty_like(x)
        gp = getattr(x, '_gn_part', None)
        if gp is not None and gp[0].shape[0] == B and gp[0].shape[2] == C and gp[1] * gp[2] == HW:
            return ops.groupnorm_silu_partials(x, w, b, out, B, HW, C, self.cfg.gn_groups, self.cfg.gn_eps, silu, gp[0], gp[1], gp[2], ws)
        return ops.groupnorm_silu(x, w, b, out, B, HW, C, self.cfg.gn_groups, self.cfg.gn_eps, silu, ws)

    def _resblock(self, x, name, B, H, W, cin, cout):
        h = self._gn(x, name + '.norm1', B, H * W, cin)
        h, _, _ = self._conv(h, name + '.conv1', B, H, W)
        h = self._gn(h, name + '.norm2', B, H * W, cout)
        if cin != cout:
            x, _, _ = self._conv(x, name + '.nin_shortcut', B, H, W)
        h, _, _ = self._conv(h, name + '.conv2', B, H, W, residual=x)
        return h

    def _attnblock(self, x, name, B, HW, C):
        T = x.dtype
        n = self._gn(x, name + '.norm', B, HW, C, silu=False)
        qkv, _, _ = self._conv(n, name + '.qkv', B, HW, 1)                     # (B*HW, 3C): q | k | v
        kch = 16 // x.element_size()
        HWp = -(-HW // kch) * kch               # the GEMM's K dimension moves 16-byte chunks: pad the key axis of P and V^T with zeros
        vT = torch.empty(B, C, HW, device=x.device, dtype=T) if HWp == HW else torch.zeros(B, C, HWp, device=x.device, dtype=T)
        ops.transpose(qkv, vT, B, HW, C, 3 * C, in_off=2 * C, ld_out=HWp)
        s = torch.empty(B, HW, HW, device=x.device, dtype=torch.float32)
        ops.gemm(qkv, qkv, s, M=HW, N=HW, K=C, lda=3 * C, ldw=3 * C, w_off=C, alpha=float(int(C) ** -0.5), batch=B,
                 strideA=HW * 3 * C, strideW=HW * 3 * C, strideC=HW * HW)
        p = torch.empty(B, HW, HW, device=x.device, dtype=T)
        ops.softmax_rows(s, p, B * HW, HW)
        if HWp != HW:                           # latent sizes other than 16x16 / 32x32 (low-resolution reconstructions, vqvae.py:97-104 same_shape=False)
            pp = torch.zeros(B, HW, HWp, device=x.device, dtype=T)
            pp[:, :, :HW] = p
            p = pp
        o = torch.empty(B * HW, C, device=x.device, dtype=T)
        ops.gemm(p, vT, o, M=HW, N=C, K=HWp, batch=B, strideA=HW * HWp, strideW=C * HWp, strideC=HW * C)
        y, _, _ = self._conv(o, name + '.proj_out', B, HW, 1, residual=x)
        return y

    # ---- encoder / decoder
    def _encode_f(self, img: torch.Tensor) -> torch.Tensor:
        """quant_conv(encoder(img)) -> f (B, Cvae, S, S) fp32, S = H / 16 (16 for 256 x 256 images, 32 for 512 x 512) (vqvae.py:74; vae_modules.py:144-160)."""
        P = self._pack()
        B, _, H, W = img.shape
        cfg = self.cfg
        leaf = self._encoder_leaf('encoder.conv_in')
        cin_p = P['conv' if leaf is None else 'enc']['encoder.conv_in']['cin']
        x = torch.empty(B * H * W, cin_p, device=img.device, dtype=self.compute_dtype if leaf is None else torch.float32)
        ops.nchw_to_nhwc(img.contiguous().float(), x, B, 3, H * W, cin_p)
        h, H, W = self._conv(x, 'encoder.conv_in', B, H, W)
        nlev = len(cfg.ch_mult)
        cur = cfg.ch
        for lv in range(nlev):
            cout = cfg.ch * cfg.ch_mult[lv]
            for b in range(cfg.num_res_blocks):
                h = self._resblock(h, f'encoder.down.{lv}.block.{b}', B, H, W, cur, cout)
                cur = cout
                if lv == nlev - 1:
                    h = self._attnblock(h, f'encoder.down.{lv}.attn.{b}', B, H * W, cur)
            if lv != nlev - 1:
                h, H, W = self._conv(h, f'encoder.down.{lv}.downsample.conv', B, H, W, stride=2)
        h = self._resblock(h, 'encoder.mid.block_1', B, H, W, cur, cur)
        h = self._attnblock(h, 'encoder.mid.attn_1', B, H * W, cur)
        h = self._resblock(h, 'encoder.mid.block_2', B, H, W, cur, cur)
        h = self._gn(h, 'encoder.norm_out', B, H * W, cur)
        z, _, _ = self._conv(h, 'encoder.conv_out', B, H, W, out_dtype=torch.float32)      # (B*HW, Cvae) fp32 NHWC
        f, _, _ = self._conv(z, 'quant_conv', B, H, W)                                      # fp32 weights
        out = torch.empty(B, self.Cvae, H, W, device=img.device, dtype=torch.float32)
        ops.nhwc_to_nchw(f, self.Cvae, out, B, self.Cvae, H * W)
        return out

    def _decode(self, f_hat: torch.Tensor, lo=-1.0, hi=1.0, mul=1.0, add=0.0) -> torch.Tensor:
        """decoder(post_quant_conv(f_hat)).clamp(lo,hi)*mul+add (vqvae.py:88-89; vae_modules.py:210-225)."""
        P = self._pack()
        outs = []
        for s in range(0, f_hat.shape[0], self.decode_chunk):
            outs.append(self._decode_chunk(f_hat[s:s + self.decode_chunk].contiguous(), lo, hi, mul, add))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)

    def _decode_chunk(self, f_hat, lo, hi, mul, add):
        cfg = self.cfg
        T = self.compute_dtype
        B, Cv, H, W = f_hat.shape
        x = torch.empty(B * H * W, Cv, device=f_hat.device, dtype=torch.float32)
        ops.nchw_to_nhwc(f_hat.float(), x, B, Cv, H * W, Cv)
        z, _, _ = self._conv(x, 'post_quant_conv', B, H, W, out_dtype=T)                   # fp32 conv, output in compute dtype
        nlev = len(cfg.ch_mult)
        cur = cfg.ch * cfg.ch_mult[-1]
        h, _, _ = self._conv(z, 'decoder.conv_in', B, H, W)
        h = self._resblock(h, 'decoder.mid.block_1', B, H, W, cur, cur)
        h = self._attnblock(h, 'decoder.mid.attn_1', B, H * W, cur)
        h = self._resblock(h, 'decoder.mid.block_2', B, H, W, cur, cur)
        for lv in reversed(range(nlev)):
            cout = cfg.ch * cfg.ch_mult[lv]
            for b in range(cfg.num_res_blocks + 1):
                h = self._resblock(h, f'decoder.up.{lv}.block.{b}', B, H, W, cur, cout)
                cur = cout
                if lv == nlev - 1:
                    h = self._attnblock(h, f'decoder.up.{lv}.attn.{b}', B, H * W, cur)
            if lv != 0:
                h, H, W = self._conv(h, f'decoder.up.{lv}.upsample.conv', B, H, W, up=1)
        h = self._gn(h, 'decoder.norm_out', B, H * W, cur)
        y, _, _ = self._conv(h, 'decoder.conv_out', B, H, W, out_dtype=torch.float32)      # (B*HW, 3) fp32
        out = torch.empty(B, 3, H, W, device=f_hat.device, dtype=torch.float32)
        ops.nhwc_to_nchw(y, 3, out, B, 3, H * W, lo, hi, mul, add)
        return out

    # ---- quantizer helpers
    def _split(self, flat: torch.Tensor, mf: int = 1) -> List[torch.Tensor]:
        outs, o = [], 0
        for pn in self.cfg.patch_nums:
            n = mf * pn * pn
            outs.append(flat[:, o:o + n])
            o += n
        return outs

    def _scale_tables(self, v_patch_nums):
        """operator tables + phi map of a caller-chosen scale list (vqvae.py:73-75 passes v_patch_nums through to
        f_to_idxBl_or_fhat, quant.py:184-215, which accepts any list ending at the latent size; phi by the nearest-tick rule :282-290)"""
        P = self._pack()
        pns = tuple(int(p[0] if isinstance(p, (tuple, list)) else p) for p in v_patch_nums)
        if any(isinstance(p, (tuple, list)) and p[0] != p[1] for p in v_patch_nums):
            raise NotImplementedError('non-square scales (ph != pw) are not built')
        if pns == tuple(self.cfg.patch_nums):
            return pns, P['up'], P['down'], P['phi_map']
        if pns[-1] != self.cfg.patch_nums[-1]:
            raise AssertionError(f'patch_hws[-1]={pns[-1]} != latent size {self.cfg.patch_nums[-1]}')          # quant.py:193
        check_latent_size(pns[-1])                       # a guard only: the constructor has checked the size the line above compares with
        if len(pns) > 16:
            raise NotImplementedError('at most 16 scales')
        cache = P.setdefault('alt_tables', {})
        if pns not in cache:
            from .spec import phi_index_map
            up, down, _ = packed_tables(pns)
            cache[pns] = (torch.from_numpy(up).to(self.device), torch.from_numpy(down).to(self.device), phi_index_map(len(pns), self.cfg.share_quant_resi))
        up, down, pm = cache[pns]
        return pns, up, down, pm

    def _ms_encode(self, f: torch.Tensor, want_fhat=False, want_margin=False, v_patch_nums=None):
        P = self._pack()
        B = f.shape[0]
        pns, up, down, phi_map = self._scale_tables(v_patch_nums) if v_patch_nums is not None else (self.cfg.patch_nums, P['up'], P['down'], P['phi_map'])
        Ltot = sum(p * p for p in pns)
        idx = torch.empty(B, Ltot, device=f.device, dtype=torch.int32)
        fh = torch.empty_like(f) if want_fhat else None
        mg = torch.empty(B, Ltot, device=f.device, dtype=torch.float32) if want_margin else None
        ops.ms_encode(f.contiguous(), P['E'], self.V, P['phi_w'], P['phi_b'], phi_map, list(pns), up, down, idx, fh, mg,
                      B, pns[-1], self.Cvae)
        return idx, fh, mg

    def _next_input(self, si: int, idx: torch.Tensor, f_hat: torch.Tensor, nb: int, nmaps: int, want_tok: bool, soft: Optional[torch.Tensor] = None,
                    pn_next: Optional[int] = None):
        """one scale step for all (nb, nmaps) maps: f_hat updated in place, returns tokens of the next scale or None.
        soft: (nb, nmaps*pn*pn, Cvae) embeddings used INSTEAD of E[idx] (more_smooth, control_var.py:511-515) - they are handed to the
        kernel as a one-off codebook addressed by the identity index.  pn_next: pool the updated map to this size instead of the next
        scale's (the control pass of separate_decoding feeds area(f_hat -> the SAME scale), control_var.py:467-468)."""
        P = self._pack()
        pns = self.cfg.patch_nums
        pn = pns[si]
        last = si == len(pns) - 1
        explicit = pn_next is not None
        if not explicit:
            pn_next = pns[si + 1] if not last else pn
        codebook = P['E']
        if soft is not None:
            codebook = soft.reshape(-1, self.Cvae).float().contiguous()
            idx = torch.arange(codebook.shape[0], device=f_hat.device, dtype=torch.int32).view(nb, -1)
        make_tok = want_tok and (explicit or not last)
        tok = torch.empty(nb, nmaps * pn_next * pn_next, self.Cvae, device=f_hat.device, dtype=torch.float32) if make_tok else None
        down_off = P['tab_off'][pns.index(pn_next)] if make_tok else 0
        ops.ms_next_input(idx, codebook, P['phi_w'], P['phi_b'], P['up'], P['down'], f_hat, tok, nb, nmaps, pn, pn_next, pns[-1], self.Cvae,
                          P['phi_map'][si], P['tab_off'][si], down_off)
        return tok

    # ---- public API (same names / meaning as models/vqvae.py)
    @torch.no_grad()
    def img_to_idxBl(self, inp_img_no_grad: torch.Tensor, v_patch_nums=None) -> List[torch.Tensor]:
        """vqvae.py:73-75 -> list of (B, pn*pn) int64 ids, coarse to fine"""
        self._pack(check=True)
        idx, _, _ = self._ms_encode(self._encode_f(inp_img_no_grad), v_patch_nums=v_patch_nums)
        pns = self._scale_tables(v_patch_nums)[0] if v_patch_nums is not None else self.cfg.patch_nums
        outs, o = [], 0
        for pn in pns:
            outs.append(idx[:, o:o + pn * pn].long())
            o += pn * pn
        return outs

    @torch.no_grad()
    def idxBl_to_h(self, gt_ms_idx_Bl: List[torch.Tensor]) -> List[torch.Tensor]:
        """vqvae.py:77-78 / quant.py:217-240 -> teacher-forcing inputs, list of (B, pn_{k+1}^2, Cvae) fp32"""
        self._pack(check=True)
        B = gt_ms_idx_Bl[0].shape[0]
        dev = gt_ms_idx_Bl[0].device
        S = self.cfg.patch_nums[-1]
        f_hat = torch.zeros(B, 1, self.Cvae, S, S, device=dev, dtype=torch.float32)
        outs = []
        for si in range(len(self.cfg.patch_nums) - 1):
            outs.append(self._next_input(si, gt_ms_idx_Bl[si].to(torch.int32).contiguous(), f_hat, B, 1, True))
        return outs

    def _idx_to_fhat(self, ms_idx_Bl: List[torch.Tensor]) -> torch.Tensor:
        B = ms_idx_Bl[0].shape[0]
        S = self.cfg.patch_nums[-1]
        f_hat = torch.zeros(B, 1, self.Cvae, S, S, device=ms_idx_Bl[0].device, dtype=torch.float32)
        for si in range(len(self.cfg.patch_nums)):
            self._next_input(si, ms_idx_Bl[si].to(torch.int32).contiguous(), f_hat, B, 1, False)
        return f_hat[:, 0]

    @torch.no_grad()
    def fhat_to_img(self, f_hat: torch.Tensor) -> torch.Tensor:
        """vqvae.py:88-89"""
        self._pack(check=True)
        return self._decode(f_hat)

    @torch.no_grad()
    def idxBl_to_img(self, ms_idx_Bl: List[torch.Tensor], same_shape: bool = True, last_one: bool = False):
        """vqvae.py:97-104; same_shape=False decodes every scale at its own resolution (images of 16 pn x 16 pn)"""
        self._pack(check=True)
        if not same_shape:                                   # every scale at its own resolution (quant.py:171-180)
            rows = [self._embed(idx) for idx in ms_idx_Bl]
            fh = self._lowres_fhats(rows, ms_idx_Bl[0].shape[0], last_one)
            return self._decode(fh) if last_one else [self._decode(f) for f in fh]
        if last_one:
            return self._decode(self._idx_to_fhat(ms_idx_Bl))
        B = ms_idx_Bl[0].shape[0]
        S = self.cfg.patch_nums[-1]
        f_hat = torch.zeros(B, 1, self.Cvae, S, S, device=ms_idx_Bl[0].device, dtype=torch.float32)
        outs = []
        for si in range(len(self.cfg.patch_nums)):
            self._next_input(si, ms_idx_Bl[si].to(torch.int32).contiguous(), f_hat, B, 1, False)
            outs.append(self._decode(f_hat[:, 0]))
        return outs

    def _embed(self, idx_Bl: torch.Tensor) -> torch.Tensor:
        """quantize.embedding(idx) -> (B * l, Cvae) fp32 rows (vqvae.py:103)"""
        P = self._pack()
        _check_index_range(idx_Bl, 0, self.V - 1, 'token ids')           # inclusive bounds: id == V raises like nn.Embedding's IndexError
        out = torch.empty(idx_Bl.numel(), self.Cvae, device=idx_Bl.device, dtype=torch.float32)
        return ops.embed_rows(idx_Bl.to(torch.int32).contiguous(), P['E'], out)

    def _lowres_fhats(self, ms_rows: List[torch.Tensor], B: int, last_one: bool):
        """embed_to_fhat(all_to_max_scale=False) (quant.py:171-180): f_hat starts at the first scale's size, is bicubic-resized to every next
        scale's size and receives phi_k(h_k) computed at THAT resolution.  ms_rows: per scale (B * pn * pn, Cvae) fp32 NHWC rows.
        Returns (B, Cvae, pn, pn) fp32 maps - the last one, or one per scale."""
        from .pyramid import bicubic_matrix
        P = self._pack()
        pns, C, dev = self.cfg.patch_nums, self.Cvae, ms_rows[0].device
        if len(ms_rows) != len(pns):
            raise ValueError(f'expected {len(pns)} scales, got {len(ms_rows)}')
        mats = P.setdefault('lowres_mats', {})
        f, prev, outs = None, None, []
        for si, pn in enumerate(pns):
            n = B * pn * pn
            h = ms_rows[si].reshape(n, C).float().contiguous()
            base = torch.zeros(n, C, device=dev, dtype=torch.float32)
            if f is not None:
                if (prev, pn) not in mats:
                    mats[(prev, pn)] = torch.from_numpy(bicubic_matrix(prev, pn).astype('float32')).to(dev)
                m = mats[(prev, pn)]
                ops.resample_sep(f, m, m, base, B, prev, prev, pn, pn, C)
            k = P['phi_map'][si]
            f = torch.empty(n, C, device=dev, dtype=torch.float32)
            ops.gemm(h, P['phi_fold_w'], f, M=n, N=C, K=9 * C, w_off=k * C * 9 * C, bias=P['phi_fold_b'][k], residual=base,
                     conv=dict(Hin=pn, Win=pn, Cin=C, Hout=pn, Wout=pn))
            prev = pn
            if not last_one or si == len(pns) - 1:
                o = torch.empty(B, C, pn, pn, device=dev, dtype=torch.float32)
                ops.nhwc_to_nchw(f, C, o, B, C, pn * pn)
                outs.append(o)
        return outs[-1] if last_one else outs

    @torch.no_grad()
    def embed_to_fhat(self, ms_h_BChw: List[torch.Tensor], all_to_max_scale: bool = True, last_one: bool = False):
        """quant.py:156-182: multi-scale embeddings (B, Cvae, pn, pn) -> f_hat (the last, or after every scale)"""
        self._pack(check=True)
        B = ms_h_BChw[0].shape[0]
        rows = [h.float().permute(0, 2, 3, 1).reshape(B * h.shape[2] * h.shape[3], self.Cvae).contiguous() for h in ms_h_BChw]
        if not all_to_max_scale:
            return self._lowres_fhats(rows, B, last_one)
        S = self.cfg.patch_nums[-1]
        f_hat = torch.zeros(B, 1, self.Cvae, S, S, device=rows[0].device, dtype=torch.float32)
        outs = []
        for si in range(len(self.cfg.patch_nums)):
            self._next_input(si, None, f_hat, B, 1, False, soft=rows[si].view(B, -1, self.Cvae))
            if not last_one:
                outs.append(f_hat[:, 0].clone())
        return f_hat[:, 0] if last_one else outs

    @torch.no_grad()
    def embed_to_img(self, ms_h_BChw: List[torch.Tensor], all_to_max_scale: bool, last_one: bool = False):
        """vqvae.py:91-95"""
        fh = self.embed_to_fhat(ms_h_BChw, all_to_max_scale=all_to_max_scale, last_one=last_one)
        return self._decode(fh) if last_one else [self._decode(f) for f in fh]

    @torch.no_grad()
    def img_to_recon(self, x, v_patch_nums=None, last_one=False):
        """vqvae.py:80-86"""
        self._pack(check=True)
        idx, fh, _ = self._ms_encode(self._encode_f(x), want_fhat=True, v_patch_nums=v_patch_nums)
        if last_one:
            return self._decode(fh, lo=-3.0e38, hi=3.0e38)
        return self._recon_all(idx, v_patch_nums)

    def _recon_all(self, idx, v_patch_nums=None):
        """decode f_hat after every scale (quant.py:184-215 with to_fhat=True) - for the constructor's scale list or a caller-chosen one"""
        P = self._pack()
        pns, up, down, phi_map = self._scale_tables(v_patch_nums) if v_patch_nums is not None else (self.cfg.patch_nums, P['up'], P['down'], P['phi_map'])
        B = idx.shape[0]
        S = pns[-1]
        f_hat = torch.zeros(B, 1, self.Cvae, S, S, device=idx.device, dtype=torch.float32)
        outs, o, tab = [], 0, 0
        for si, pn in enumerate(pns):
            ids = idx[:, o:o + pn * pn].contiguous()
            ops.ms_next_input(ids, P['E'], P['phi_w'], P['phi_b'], up, down, f_hat, None, B, 1, pn, pn, S, self.Cvae, phi_map[si], tab, 0)
            outs.append(self._decode(f_hat[:, 0], lo=-3.0e38, hi=3.0e38))
            o += pn * pn
            tab += S * pn
        return outs

    def forward(self, *a, **k):
        raise NotImplementedError('VQVAE training (vqvae.py:56-59, losses/) is out of scope: the tokenizer is frozen on the hot path')


# =====================================================================================
# ControlVAR / VAR
# =====================================================================================
FUSE_LN_BELOW = 4097       # passes with fewer rows ask proj / fc2 for the next op's adaLN (see _blocks_and_head); 2048 -> 4097: B = 8 63.0 -> 62.3 ms, B = 16 106.7 -> 106.0


SAMPLERS = ('counter', 'torch')


def torch_draw_schedule(cfg: VarConfig, B: int, *, label_B_none: bool, cond_type_none: bool, four_way: bool, more_smooth: bool
                        ) -> List[Tuple[str, Tuple[int, ...]]]:
    """Every call one generation of the reference makes on its generator, in its order, as (kind, shape) - sampler='torch' makes the same
    calls, so the generator's state after a call equals the reference's:
      ('labels', (B,))        label_B=None: multinomial(selecting_idx (1, num_classes), B, replacement=True)     control_var.py:248,377; var.py:164
      ('cond_type', (B,))     autoregressive_infer_cfg of a multi_cond model, cond_type=None, B != 4: multinomial((1, 4) uniform, B, True)
                              (control_var.py:392; the conditional form takes cond_type as given and draws none)
      ('expo', (rows*l, V))   each sampling call: torch.multinomial's Exp(1) noise (its one-sample path), rows = B, or 4B after the
                              conditional form's .repeat (control_var.py:306); l counts separator positions                helpers.py:19
      ('gumbel', (rows, l, V))  more_smooth, after each sample (also at top_k == 1): exponential_ of gumbel_softmax_with_rng    helpers.py:26
    The two-pass branch (separate_decoding without indep, control_var.py:428-485) samples the control half, then the image half, per scale."""
    py = cfg.pyramid
    out: List[Tuple[str, Tuple[int, ...]]] = []
    if label_B_none:
        out.append(('labels', (B,)))
    if cfg.mask_factor == 2 and not four_way and cond_type_none and B != 4:
        out.append(('cond_type', (B,)))
    if cfg.separate_decoding and not cfg.indep and not four_way:
        passes = [(B, pn * pn) for pn in py.patch_nums for _ in (0, 1)]
    else:
        passes = [(4 * B if four_way else B, l) for l in py.l]
    for rows, l in passes:
        out.append(('expo', (rows * l, cfg.vocab)))
        if more_smooth:
            out.append(('gumbel', (rows, l, cfg.vocab)))
    return out


def torch_draw(kind: str, shape: Tuple[int, ...], generator: Optional[torch.Generator], device, num_classes: int) -> torch.Tensor:
    """One entry of torch_draw_schedule, drawn as the reference draws it (generator None: the device's default generator)"""
    if kind in ('labels', 'cond_type'):
        n = num_classes if kind == 'labels' else 4
        probs = torch.full((1, n), fill_value=1 / n, dtype=torch.float32, device=device)
        return torch.multinomial(probs, num_samples=shape[0], replacement=True, generator=generator).reshape(shape[0])
    e = torch.empty(shape, dtype=torch.float32, device=device).exponential_(generator=generator)
    if kind == 'expo':
        return e
    if kind == 'gumbel':
        return -e.log()
    raise ValueError(f'unknown draw kind {kind!r}')


def _check_generator_device(gdev: torch.device, dev: torch.device):
    """sampler='torch' draws on the model's device or on the CPU (then copies the noise over)"""
    def norm(d):
        d = torch.device(d)
        return torch.device(d.type, torch.cuda.current_device()) if d.type == 'cuda' and d.index is None else d
    if norm(gdev).type != 'cpu' and norm(gdev) != norm(dev):
        raise ValueError(f"model.rng is a generator on {gdev}: sampler='torch' needs one on the model's device ({dev}) or on the CPU")


class _TorchDraws:
    """Hands out the draws of a torch_draw_schedule in order, on the model's device; a request out of order is a bug and raises."""

    def __init__(self, schedule, generator, gdev, dev, num_classes):
        self.schedule, self.generator, self.gdev, self.dev, self.num_classes = schedule, generator, gdev, dev, num_classes
        self.pos = 0

    def next_kind(self) -> Optional[str]:
        return self.schedule[self.pos][0] if self.pos < len(self.schedule) else None

    def take(self, kind: str, shape: Tuple[int, ...]) -> torch.Tensor:
        want = self.schedule[self.pos] if self.pos < len(self.schedule) else None
        if want != (kind, tuple(shape)):
            raise RuntimeError(f'torch sampler: draw {self.pos} is {(kind, tuple(shape))}, the schedule has {want}')
        self.pos += 1
        return torch_draw(kind, tuple(shape), self.generator, self.gdev, self.num_classes).to(self.dev).contiguous()

    def finish(self):
        if self.pos != len(self.schedule):
            raise RuntimeError(f'torch sampler: {len(self.schedule) - self.pos} scheduled draws were not taken')


# ---- per-request sampling parameters (an addition of this library; include/cvar_serve.h) ---------------------------------------
def _host_array(v) -> np.ndarray:
    """a sampling parameter as a host array; a device tensor is read back (this synchronises with the device)"""
    if torch.is_tensor(v):
        return v.detach().cpu().numpy()
    if isinstance(v, (list, tuple)) and any(torch.is_tensor(x) for x in v):
        v = [_host_array(x) for x in v]
    return np.asarray(v)


def _per_request(cfg, top_k, top_p, g_seed, four_way: bool) -> bool:
    """does any of the sampling parameters come per batch row?  A scalar (python / numpy number, 0-d array or tensor; g_seed also None) is
    the reference's one-value-per-call form, and so is ONE triple of guidance scales for the four-branch cfg; everything else is per row"""
    if _host_array(cfg).ndim == (2 if four_way else 1):
        return True
    return any(v is not None and _host_array(v).ndim != 0 for v in (top_k, top_p, g_seed))


class _RequestTable:
    """The per-row sampling parameters of one batch in ONE contiguous host buffer - seeds int64 [B] | top_k int32 [B] | top_p fp32 [B] |
    combine weights fp32 [nstage][B][4] - so that one host-to-device copy refreshes all of them (before a graph replay).
    n_seq > 0 (per-request adapters): the adapter slot of every sequence, int32 [n_seq], rides behind them in the same buffer."""

    def __init__(self, B: int, nstage: int, n_seq: int = 0):
        self.B, self.nstage, self.n_seq = B, nstage, n_seq
        self.host = torch.zeros(self.nbytes(B, nstage) + 4 * n_seq, dtype=torch.uint8)
        self.seed, self.top_k, self.top_p, self.coef = self.views(self.host)
        self.slot = self.slot_view(self.host)

    @staticmethod
    def nbytes(B: int, nstage: int) -> int:
        return 8 * B + 4 * B + 4 * B + 16 * nstage * B

    def slot_view(self, buf: torch.Tensor):
        """(n_seq,) int32 view of the adapter slots in `buf` (None without them)"""
        return buf[self.nbytes(self.B, self.nstage):].view(torch.int32) if self.n_seq else None

    def views(self, buf: torch.Tensor):
        """(seed (B,) int64, top_k (B,) int32, top_p (B,) fp32, coef (nstage, B, 4) fp32) views of `buf`, the host buffer or a device copy of it"""
        B = self.B
        return (buf[:8 * B].view(torch.int64), buf[8 * B:12 * B].view(torch.int32), buf[12 * B:16 * B].view(torch.float32),
                buf[16 * B:self.nbytes(B, self.nstage)].view(torch.float32).view(self.nstage, B, 4))


def _request_table(B: int, cfg, top_k, top_p, g_seed, four_way: bool, vocab: int, nstage: int, slots=None) -> _RequestTable:
    """Normalise per-request sampling parameters.  cfg / top_k / top_p / g_seed: each a scalar (broadcast to the B rows) or a length-B
    sequence, numpy array or tensor (a device tensor is read back, which synchronises); the four-branch cfg is one triple or (B, 3).
    g_seed=None draws one host seed per row, as the scalar path draws its one; seeds are taken modulo 2^64.  The combine weights of every
    stage come from the very expressions of _generate_core, in python doubles, rounded to fp32 once: bit-identical to what the scalar
    call hands to cvar_cfg_sample.  Raises before anything is written anywhere: ValueError on a wrong length or shape, RuntimeError on
    top_k > vocabulary (as the scalar call).  slots (per-request adapters): the validated slot of every sequence (lora.sequence_slots)."""
    def rows(name, v, width=None):
        a = _host_array(v)
        if a.dtype == object or a.dtype.kind not in 'iuf':
            raise ValueError(f'{name}: numbers expected, got {a.dtype}')
        scalar_ndim = 0 if width is None else 1
        want = (B,) if width is None else (B, width)
        if a.ndim == scalar_ndim and (width is None or a.shape == (width,)):
            a = np.broadcast_to(a, want)
        if a.shape != want:
            raise ValueError(f'{name}: a scalar or shape {want} (one per batch row) expected, got {a.shape}' if width is None else
                             f'{name}: one triple of guidance scales or shape {want} expected, got {a.shape}')
        return a

    cfg_r = rows('cfg', cfg, 3 if four_way else None).astype(np.float64) if cfg is not None else None      # None: no guidance rows, the weights are [1]
    k_r = rows('top_k', top_k)
    if k_r.dtype.kind == 'f':
        if not np.all(k_r == np.round(k_r)):
            raise ValueError('top_k: integers expected')
    k_r = k_r.astype(np.int64)
    if (k_r > vocab).any():                              # as _generate (helpers.py:8-10: torch.topk raises on k > V)
        raise RuntimeError(f'selected index k out of range (top_k={int(k_r.max())} > vocabulary {vocab})')
    p_r = rows('top_p', top_p).astype(np.float32)
    if g_seed is None:
        seeds = [int(s) for s in torch.empty(B, dtype=torch.int64).random_().tolist()]
    else:
        # python integers, not a numpy array: seeds are arbitrary-size integers taken modulo 2^64 (int(g_seed) & (2^64 - 1) in the scalar call)
        seeds = _host_array(g_seed).tolist() if torch.is_tensor(g_seed) or isinstance(g_seed, np.ndarray) else g_seed
        seeds = list(seeds) if isinstance(seeds, (list, tuple)) else [seeds] * B
        if len(seeds) != B or not all(isinstance(s, (int, np.integer)) and not isinstance(s, bool) for s in seeds):
            raise ValueError(f'g_seed: one integer or {B} integers (one per batch row) expected')
        seeds = [int(s) for s in seeds]
    tab = _RequestTable(B, nstage, 0 if slots is None else len(slots))
    if slots is not None:
        tab.slot.copy_(torch.from_numpy(np.ascontiguousarray(slots, dtype=np.int32)))
    tab.seed.copy_(torch.from_numpy(np.array([s & (2 ** 64 - 1) for s in seeds], dtype=np.uint64).view(np.int64)))
    tab.top_k.copy_(torch.from_numpy(np.maximum(k_r, -1).astype(np.int32)))          # <= 0: no filter (every negative value means the same)
    tab.top_p.copy_(torch.from_numpy(np.ascontiguousarray(p_r)))
    coef = np.zeros((nstage, B, 4), dtype=np.float32)
    for si in range(nstage):
        ratio = si / (nstage - 1)
        for b in range(B):
            if cfg_r is None:
                coef[si, b, 0] = 1.0
            elif four_way:
                t1, t2, t3 = [c * ratio for c in cfg_r[b].tolist()]
                coef[si, b] = [1 + t1, t2 - t1, t3 - t2, -t3]
            else:
                t = float(cfg_r[b]) * ratio
                coef[si, b, :2] = [1 + t, -t]
    tab.coef.copy_(torch.from_numpy(coef))
    return tab


def _refuse_request_keywords(g_seed, request: dict):
    """run() of a graph captured with per_request=False: cfg / top_k / top_p are baked into its launches, and its one seed is a scalar"""
    if request:
        raise TypeError(f'run() got {", ".join(sorted(request))}: this graph was captured with per_request=False, which bakes cfg, top_k and top_p into its '
                        'launches - capture it with per_request=True to pass them per call and per row')
    if g_seed is not None and _host_array(g_seed).ndim != 0:
        raise ValueError('g_seed: one integer - this graph was captured with per_request=False; capture it with per_request=True for one seed per row')


# ---- token log-probabilities (an addition of this library; include/cvar_serve.h: cvar_score_rows) ---------------------------------
class TokenScores:
    """Per-token scores of a generation (``logprobs=True``) or of given tokens (``score_infer_cfg``), all (B, L) with L = sum mask_factor pn^2
    in the token order of generation: per scale the two halves, control first when mask_first and image first otherwise.
      logprob  fp32   log-probability of the token's id under the CFG-combined distribution of its row - the UNFILTERED one: a top-k /
                      top-p kept set is not renormalised over (a token outside the kept set of another request still has its finite score)
      entropy  fp32   entropy of that distribution
      rank     int32  the number of codes ahead of the id (0 = the greedy id, lowest index on ties)
      argmax   int32  the greedy id
      sampled  bool   False where the token was teacher-forced or kept by an edit; those tokens are scored too (the head computes their
                      logits anyway)
    and, under ``top_logprobs=N`` (None without it; include/cvar_topn.h: cvar_score_topn, one more launch per scale):
      top_ids       (B, L, N) int32  the N most likely codes of that distribution in rank order (top_ids[..., rank] is the token's id where
                                     rank < N, top_ids[..., 0] is argmax); -1 past the vocabulary
      top_logprobs  (B, L, N) fp32   their log-probabilities, the bits `logprob` holds for that code; -inf past the vocabulary
      tail_logprob  (B, L) fp32      the log of the mass of all the other codes; -inf when there is none"""

    def __init__(self, logprob, entropy, rank, argmax, patch_nums, mask_factor: int, mask_first: bool, sampled=None, forced=None, top_ids=None,
                 top_logprobs=None, tail_logprob=None):
        self.logprob, self.entropy, self.rank, self.argmax = logprob, entropy, rank, argmax
        self.top_ids, self.top_logprobs, self.tail_logprob = top_ids, top_logprobs, tail_logprob
        self.patch_nums, self.mask_factor, self.mask_first = tuple(int(p) for p in patch_nums), int(mask_factor), bool(mask_first)
        self._sampled, self._forced = sampled, forced          # a (B, L) / (L,) bool pattern, or the forced-token table (>= 0: not sampled)

    @property
    def sampled(self) -> torch.Tensor:
        """evaluated on first use, so that a generation issues nothing for it"""
        if self._sampled is None or self._sampled.dim() == 1:
            if self._forced is not None:
                s = self._forced < 0
            else:
                col = torch.ones(self.logprob.shape[1], dtype=torch.bool) if self._sampled is None else self._sampled
                s = col.to(self.logprob.device)[None].expand(self.logprob.shape[0], -1).contiguous()
            self._sampled, self._forced = s, None
        return self._sampled

    def _bounds(self):
        b, out = 0, []
        for pn in self.patch_nums:
            out.append((b, b + self.mask_factor * pn * pn))
            b = out[-1][1]
        return out

    def half_mask(self, half: Optional[str]) -> torch.Tensor:
        """(L,) bool on the host: the tokens of 'control' / 'image' (None: all) in this object's half order"""
        if half not in (None, 'control', 'image'):
            raise ValueError(f"half={half!r}: None, 'control' or 'image'")
        L = self._bounds()[-1][1]
        if half is None or (self.mask_factor == 1 and half == 'image'):
            return torch.ones(L, dtype=torch.bool)
        if self.mask_factor == 1:
            raise ValueError("half='control': a plain VAR has the image half only")
        m = torch.zeros(L, dtype=torch.bool)
        first = (half == 'control') == self.mask_first
        for (b, e), pn in zip(self._bounds(), self.patch_nums):
            m[b:b + pn * pn] = first
            m[b + pn * pn:e] = not first
        return m

    def per_scale(self):
        """one TokenScores per scale, its fields the (B, mask_factor pn^2) column views of this one's"""
        s = self.sampled
        cut = lambda t, b, e: None if t is None else t[:, b:e]
        return [TokenScores(self.logprob[:, b:e], self.entropy[:, b:e], self.rank[:, b:e], self.argmax[:, b:e], (pn,), self.mask_factor, self.mask_first,
                            sampled=s[:, b:e], top_ids=cut(self.top_ids, b, e), top_logprobs=cut(self.top_logprobs, b, e),
                            tail_logprob=cut(self.tail_logprob, b, e)) for (b, e), pn in zip(self._bounds(), self.patch_nums)]

    def _without_alternatives(self) -> 'TokenScores':
        """these scores with the three top-N fields left out (the other fields shared, `sampled` as evaluated so far)"""
        return TokenScores(self.logprob, self.entropy, self.rank, self.argmax, self.patch_nums, self.mask_factor, self.mask_first, sampled=self._sampled,
                           forced=self._forced)

    def sparse_loss(self, weights=None):
        """the SparseDistillLoss of a training step along these tokens: the N most likely codes and the tail mass as the teacher -
        with score_infer_cfg(..., top_logprobs=N) a sparse guided teacher along DATASET tokens.  weights: (B, L) token weights or None"""
        if self.top_ids is None:
            raise ValueError('sparse_loss: these scores hold no alternatives - ask for them with top_logprobs=N')
        from .train import SparseDistillLoss
        return SparseDistillLoss(self.top_ids, self.top_logprobs, self.tail_logprob, weights=weights)

    def total(self, half: Optional[str] = None, sampled_only: bool = False) -> torch.Tensor:
        """(B,) float64: the sum of the log-probabilities over all tokens, or over one half ('control' / 'image'); sampled_only leaves out
        the teacher-forced and the kept ones.  With score_infer_cfg(given=g), total(half=<the other half>) is log p(other | g)."""
        m = self.half_mask(half).to(self.logprob.device)[None]
        if sampled_only:
            m = m & self.sampled
        lp = self.logprob.double()
        return torch.where(m, lp, torch.zeros((), dtype=lp.dtype, device=lp.device)).sum(dim=1)


class DistillTargets(NamedTuple):
    """What a generation call returns beside its images under ``distill_targets=True`` (guidance distillation): the sample the
    teacher drew and the guided distribution it drew every token from, in the forms Trainer.step_tokens takes -
        trainer.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=t.loss(), mask_first=t.mask_first)
      ids_img, ids_ctrl  (B, sum pn^2) int32: the ids the first branch continued with, i.e. after the teacher-forcing overwrites of
                         conditional_infer_cfg (last_trace['idx'] holds the draw before them); ids_ctrl is None for a plain VAR
      logits             (B, L, V) fp32: the sampler's combined logits sum_k coef_k logits_k of every scale in token order, bit for bit
                         what trace=True records
      sampled            (B, L) bool, as TokenScores.sampled: False where the token was teacher-forced
      mask_first         the order of the halves in `logits` / `sampled` (control first)"""
    ids_img: torch.Tensor
    ids_ctrl: Optional[torch.Tensor]
    logits: torch.Tensor
    sampled: torch.Tensor
    mask_first: bool

    def loss(self):
        """the DistillLoss of a training step on this batch: the guided logits as soft targets, the teacher-forced tokens weighted 0"""
        from .train import DistillLoss
        return DistillLoss(self.logits, weights=self.sampled)


class SparseDistillTargets(NamedTuple):
    """What a generation call returns beside its images under ``distill_topn=N``: DistillTargets with the guided distribution of
    every token as its N most likely codes and the mass of the rest - N x 8 + 4 bytes per token instead of 4 V, never materialised as (B, L, V) -
        trainer.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=t.loss(), mask_first=t.mask_first)
      ids_img, ids_ctrl  as DistillTargets'
      top_ids, top_logprobs, tail_logprob   (B, L, N) int32, (B, L, N) fp32, (B, L) fp32: TokenScores' fields of the same names
      sampled, mask_first                   as DistillTargets'"""
    ids_img: torch.Tensor
    ids_ctrl: Optional[torch.Tensor]
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor
    tail_logprob: torch.Tensor
    sampled: torch.Tensor
    mask_first: bool

    def loss(self):
        """the SparseDistillLoss of a training step on this batch, the teacher-forced tokens weighted 0"""
        from .train import SparseDistillLoss
        return SparseDistillLoss(self.top_ids, self.top_logprobs, self.tail_logprob, weights=self.sampled)


TOPN_MAX = 64                                        # cvar_score_topn's N (include/cvar_topn.h)


def _top_n(what: str, n, logprobs: bool = True) -> Optional[int]:
    """top_logprobs= / distill_topn= -> N, or None when it is not given; refused in words on the host"""
    if n is None:
        return None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= TOPN_MAX:
        raise ValueError(f'{what}={n!r}: an integer from 1 to {TOPN_MAX} (the number of most likely codes reported per token)')
    if not logprobs:
        raise ValueError(f'{what}={n!r} needs logprobs=True: the alternatives are fields of the TokenScores that logprobs=True returns')
    return int(n)


_NO_REGION_TOPN = ('{}: top_logprobs is not offered under regional guidance - the alternatives are ranked under ONE weight row per request, and a form that '
                   'reads the per-token weight map is not built; score the sample with logprobs=True alone')


def _topn_buffers(B: int, L: int, N: int, dev):
    """(top_ids, top_logprobs, tail_logprob) device buffers (B, L, N) / (B, L) that the top-N launch of every scale writes its columns of"""
    return (torch.empty(B, L, N, device=dev, dtype=torch.int32), torch.empty(B, L, N, device=dev, dtype=torch.float32),
            torch.empty(B, L, device=dev, dtype=torch.float32))


def _score_buffers(B: int, L: int, dev):
    """(logprob, entropy, rank, argmax) device buffers (B, L) that the score launch of every scale writes its columns of"""
    return (torch.empty(B, L, device=dev, dtype=torch.float32), torch.empty(B, L, device=dev, dtype=torch.float32),
            torch.empty(B, L, device=dev, dtype=torch.int32), torch.empty(B, L, device=dev, dtype=torch.int32))


def _flat_ids(name: str, ids, B: int, pns, vocab: int, range_name: Optional[str] = None) -> torch.Tensor:
    """one half's multi-scale ids as every entry point takes them - the list of (B, pn^2) tensors img_to_idxBl returns or one (B, sum pn^2)
    tensor -, checked on the host -> flat integer ids (B, sum pn^2) on the device they came on"""
    Lsrc = sum(pn * pn for pn in pns)
    if isinstance(ids, (list, tuple)):
        want = [(B, pn * pn) for pn in pns]
        if not all(torch.is_tensor(t) for t in ids) or [tuple(t.shape) for t in ids] != want:
            raise ValueError(f'{name}: expected {len(pns)} id tensors of shapes {want} (what img_to_idxBl returns)')
        if any(t.is_floating_point() or t.dtype == torch.bool for t in ids):
            raise ValueError(f'{name}: expected integer ids')
        ids = torch.cat([t.to(ids[0].device) for t in ids], dim=1)
    if not torch.is_tensor(ids) or tuple(ids.shape) != (B, Lsrc) or ids.is_floating_point() or ids.dtype == torch.bool:
        raise ValueError(f'{name}: expected integer ids of shape ({B}, {Lsrc}) or a list of (B, pn * pn) tensors, got '
                         f'{tuple(ids.shape) if torch.is_tensor(ids) else type(ids).__name__}')
    _check_index_range(ids, 0, vocab - 1, range_name or name)
    return ids


def _pixels(name: str, px, want) -> torch.Tensor:
    """one half given as pixels, checked on the host"""
    if not torch.is_tensor(px) or tuple(px.shape) != tuple(want) or not px.is_floating_point():
        raise ValueError(f'{name}: expected pixels of shape {tuple(want)} (floating point, in [-1, 1]), got '
                         f'{tuple(px.shape) if torch.is_tensor(px) else type(px).__name__}')
    return px


# ---- region-constrained generation (an addition of this library; include/cvar_serve.h) --------------------------------------------
def edit_keep_cells(keep: torch.Tensor, pn: int) -> torch.Tensor:
    """The cell rule of region-constrained generation on the host: keep (B, S, S) bool at latent resolution -> (B, pn * pn) bool, which tokens
    of scale pn are forced to the source.  Cell (i, j) covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns -
    the bins of F.interpolate(mode='area'), with which the quantizer forms that token (quant.py:199,238) - and is kept iff
    2 * (kept latent cells in the bin) > bin size: a strict majority in integers, an exact half stays free.  cvar_edit_force_table is the
    device form of this function."""
    k = keep.detach().cpu().to(torch.int64)
    B, S = k.shape[0], k.shape[-1]
    out = torch.empty(B, pn, pn, dtype=torch.bool)
    for i in range(pn):
        r0, r1 = i * S // pn, -((-(i + 1) * S) // pn)
        for j in range(pn):
            c0, c1 = j * S // pn, -((-(j + 1) * S) // pn)
            out[:, i, j] = 2 * k[:, r0:r1, c0:c1].sum(dim=(1, 2)) > (r1 - r0) * (c1 - c0)
    return out.view(B, pn * pn)


def _edit_half(half: str, src, keep, B: int, pns, vocab: int, pixels: bool = False):
    """one half (img / ctrl) of an edit request, checked on the host -> (source or None, keep mask (B, S, S) uint8 or None).  The source is
    returned as flat integer ids (B, sum pn^2) - or, with pixels=True, as the (B, 3, 16 S, 16 S) pixels it was given as -, on the device it
    came on.  keep: True keeps the whole half, None nothing.  A mask without a source is a ValueError; a source without a mask is unused."""
    S = pns[-1]
    if keep is None:
        mask = None
    elif keep is True:
        mask = torch.ones(B, S, S, dtype=torch.uint8)
    elif torch.is_tensor(keep) and keep.dtype == torch.bool and tuple(keep.shape) == (B, S, S):
        mask = keep.to(torch.uint8)
    else:
        raise ValueError(f'keep_{half}: True, None or a bool tensor of shape ({B}, {S}, {S}) (latent resolution, True = keep the source) expected, got '
                         f'{(str(keep.dtype)[6:] + " " + str(tuple(keep.shape))) if torch.is_tensor(keep) else repr(keep)[:40]}')
    if src is None:
        if mask is not None:
            raise ValueError(f'keep_{half} is given without src_{half}: there is nothing to keep')
        return None, None
    if pixels:
        return _pixels(f'src_{half}', src, (B, 3, 16 * S, 16 * S)), mask
    return _flat_ids(f'src_{half}', src, B, pns, vocab), mask


# ---- regional guidance (an addition of this library; include/cvar_region.h) ------------------------------------------------
REGION_MAX_LABELS = 3          # K conditional rows + the unconditional one fill the sampler's four weight slots


def region_coef_reference(regions, strength, cfg, patch_nums, mask_factor: int) -> np.ndarray:
    """The weight rule of regional guidance on the host, in float64: regions (B, K, S, S) fp32, strength (B, S, S) fp32 or None, cfg (B, K) ->
    (B, L, 4) fp32, L = sum mask_factor pn^2 in the token order of generation (both halves of a scale read the same maps, so the order of the
    halves changes no value).  Per latent cell c: n_k(c) = w_k(c) / sum_k w_k(c); per token, over its area-pooling bin (edit_keep_cells' bins):
    wbar_k = mean n_k, gbar = mean strength; t_k = (cfg_k gbar) si / (n - 1); weights wbar_k (1 + t_k) for the K labels, -(sum_k wbar_k t_k)
    for the unconditional row, 0 above - each rounded to fp32 once.  With K = 1 and no strength this is _request_table's [1 + t, -t] bit for
    bit.  cvar_region_coef_table is the device form of this function (it sums the means in another order: within 1 fp32 ulp)."""
    w = np.asarray(regions, dtype=np.float32).astype(np.float64)
    g = None if strength is None else np.asarray(strength, dtype=np.float32).astype(np.float64)
    cf = np.asarray(cfg, dtype=np.float64)
    B, K, S = w.shape[0], w.shape[1], w.shape[-1]
    pns = [int(p) for p in patch_nums]
    nrm = w / w.sum(axis=1, keepdims=True)
    out = np.zeros((B, mask_factor * sum(p * p for p in pns), 4), dtype=np.float32)
    o = 0
    for si, pn in enumerate(pns):
        ratio = si / (len(pns) - 1)
        for i in range(pn):
            r0, r1 = i * S // pn, -((-(i + 1) * S) // pn)
            for j in range(pn):
                c0, c1 = j * S // pn, -((-(j + 1) * S) // pn)
                n = (r1 - r0) * (c1 - c0)
                for b in range(B):
                    gbar = 1.0 if g is None else float(g[b, r0:r1, c0:c1].sum()) / n
                    neg, row = 0.0, [0.0] * 4
                    for k in range(K):
                        wbar = float(nrm[b, k, r0:r1, c0:c1].sum()) / n
                        t = (float(cf[b, k]) * gbar) * ratio
                        row[k] = wbar * (1 + t)
                        neg += wbar * t
                    row[K] = -neg
                    for h in range(mask_factor):
                        out[b, o + h * pn * pn + i * pn + j] = row
        o += mask_factor * pn * pn
    return out


def _region_request(B: int, labels, regions, cfg, strength, S: int, num_classes: int):
    """one regional request, checked on the host before anything is written -> (labels (B, K) int64, regions (B, K, S, S) fp32, strength
    (B, S, S) fp32 or None, cfg (B, K) float64), host tensors / arrays"""
    lab = torch.as_tensor(_host_array(labels))
    if lab.dim() != 2 or lab.shape[0] != B or lab.is_floating_point() or lab.dtype == torch.bool:
        raise ValueError(f'labels: integer class labels of shape ({B}, K) expected (K labels per sample), got '
                         f'{str(lab.dtype)[6:]} {tuple(lab.shape)}')
    K = int(lab.shape[1])
    if not 1 <= K <= REGION_MAX_LABELS:
        raise ValueError(f'labels: K = {K} labels per sample - 1 to {REGION_MAX_LABELS} are offered (K conditional rows and the unconditional one '
                         "fill the sampler's four weight slots)")
    _check_index_range(lab, 0, num_classes, 'labels')
    if not torch.is_tensor(regions) or tuple(regions.shape) != (B, K, S, S) or not regions.is_floating_point():
        raise ValueError(f'regions: a floating-point tensor of shape ({B}, {K}, {S}, {S}) (one non-negative weight map per label at latent resolution) '
                         f'expected, got {(str(regions.dtype)[6:] + " " + str(tuple(regions.shape))) if torch.is_tensor(regions) else type(regions).__name__}')
    reg = regions.detach().to(device='cpu', dtype=torch.float32).contiguous()
    if not torch.isfinite(reg).all() or (reg < 0).any():
        raise ValueError('regions: finite, non-negative weights expected')
    if (reg.double().sum(dim=1) <= 0).any():
        raise ValueError('regions: a latent cell whose weights sum to 0 belongs to no label - give every cell a positive weight for at least one label')
    st = None
    if strength is not None:
        if not torch.is_tensor(strength) or tuple(strength.shape) != (B, S, S) or not strength.is_floating_point():
            raise ValueError(f'strength: None or a floating-point tensor of shape ({B}, {S}, {S}) expected, got '
                             f'{(str(strength.dtype)[6:] + " " + str(tuple(strength.shape))) if torch.is_tensor(strength) else type(strength).__name__}')
        st = strength.detach().to(device='cpu', dtype=torch.float32).contiguous()
        if not torch.isfinite(st).all() or (st < 0).any():
            raise ValueError('strength: finite, non-negative factors expected')
    c = _host_array(cfg)
    if c.dtype == object or c.dtype.kind not in 'iuf':
        raise ValueError(f'cfg: numbers expected, got {c.dtype}')
    c = c.astype(np.float64)
    if c.ndim == 1 and c.shape == (B,):
        c = c[:, None]
    if c.ndim != 0 and c.shape not in ((B, 1), (B, K)):
        raise ValueError(f'cfg: a scalar, shape ({B},) (one per batch row) or ({B}, {K}) (one per row and label) expected, got {c.shape}')
    c = np.array(np.broadcast_to(c, (B, K)))                          # a copy: contiguous and writable
    if not np.isfinite(c).all():
        raise ValueError('cfg: finite guidance scales expected')
    return lab.to(torch.int64), reg, st, c


class _ScalarDraw(NamedTuple):
    """how the scale loops draw a scale on the scalar path: one cfg (a triple on the four-branch path), top_k, top_p and seed for the batch.
    seed_dev: the seed as a device scalar (graphs).  draws (sampler='torch'): the noise of each sampling call comes from the caller's
    torch generator (_TorchDraws).  gumbel (tests): the per-pass noise of more_smooth, injected instead of drawn."""
    cfg: Any
    top_k: int
    top_p: float
    seed: int
    seed_dev: Optional[torch.Tensor] = None
    more_smooth: bool = False
    gumbel: Any = None
    draws: Any = None


class _RowDraw(NamedTuple):
    """... and in per-request mode: rows, the device views (seed, top_k, top_p, coef [nstage][B][4]) of a _RequestTable; the sampling call of
    every scale is then the per-row one.
    forced (region-constrained generation): device (B, L) int32, the source id of every kept token and -1 elsewhere (ops.edit_force_table);
    the sampling launch of every scale then writes the kept ids itself (ops.cfg_sample_edit)
    ad (per-request adapters): (lora.bank_pack, device slot (R,) int32) handed to _ada and _blocks_and_head
    score (token log-probabilities): device (logprob, entropy, rank, argmax) buffers (B, L); every scale then issues ONE more launch
    (ops.score_rows) behind the sampling launch and the overwrites by force_idx / c_mask / c_img / the edit table: it scores the ids of rows
    0 .. B-1 - the sample f_hat[:B] returns - under this scale's combine weights rows[3][si] and writes this scale's columns
    sample=False (score_infer_cfg; with score and force_idx, (n_draw B, l) int32 device ids per scale): no sampling launch at all - the score
    launch is the only consumer of the logits, and the last scale's ids feed nothing
    coef_map (regional guidance): device (B, L, 4) fp32, the combine weights of every token (ops.region_coef_table); the sampling and the score
    launch of every scale then read their columns of it instead of rows[3][si] (ops.cfg_sample_map / ops.score_map), the sample's nrep = K + 1
    rows are [label_0 ; ... ; label_{K-1} ; unconditional], and ONE id row is drawn and fed to all of them
    topn (top_logprobs=N, with score): device (top_ids, top_logprobs, tail_logprob) buffers (B, L, N) / (B, L, N) / (B, L); every scale then
    issues ops.score_topn next to its ops.score_rows, with that launch's logits, weights and strides"""
    rows: Any
    forced: Optional[torch.Tensor] = None
    ad: Any = None
    score: Any = None
    sample: bool = True
    coef_map: Optional[torch.Tensor] = None
    topn: Any = None


GEMM_PRECISIONS = (None, 'bf16x3', 'fp8')
KV_PRECISIONS = (None, 'fp8')
_X3_NO_BANK = ("gemm_precision='bf16x3': the per-request adapter bank (attach_adapters / adapter=) is not offered - its K-augmented operands [W | B_0 ...] do not "
               "compose with the three K segments of the split product; merge one adapter with add_lora, or run the bank on gemm_precision=None")


_KV8_NO_X3 = ("kv_precision='fp8' is not offered under gemm_precision='bf16x3': the split-bf16 mode exists for exactness (fp32 arena, exact row-wise attention) "
              "and an e4m3 K/V cache would undo it; run it on a compute_dtype=torch.bfloat16 model with gemm_precision None or 'fp8'")
_FP8_NO_BANK = ("gemm_precision='fp8': the per-request adapter bank (attach_adapters / adapter=) is not offered - its K-augmented bf16 operands [W | B_0 ...] have no "
                "e4m3 form in this mode; merge one adapter with add_lora, or run the bank on gemm_precision=None")


_NO_UNGUIDED = ('{}: cfg=None (generation without guidance rows) is not offered here - it is built for autoregressive_infer_cfg, conditional_infer_cfg '
                'and their graphed generators; pass cfg=0.0 for the unguided distribution on the guided rows')


def _no_bank_message(precision) -> str:
    return _FP8_NO_BANK if precision == 'fp8' else _X3_NO_BANK


def _split_weight_rows(w: torch.Tensor) -> torch.Tensor:
    """fp32 [..., N, K] -> bf16 [..., N, 3 K] rows [w_hi | w_hi | w_lo], hi = bf16(w), lo = bf16(w - hi): the weight side of the split product
    (activation rows are [hi | lo | hi]: cvar_split3 / cvar_ln_modulate_split3)"""
    w = w.float()
    hi = w.to(torch.bfloat16)
    lo = (w - hi.float()).to(torch.bfloat16)
    return torch.cat((hi, hi, lo), dim=-1).contiguous()


def kv8_arena_shapes(depth: int, R: int, Lmax: int, H: int):
    """kv_precision='fp8' (include/cvar_kvcache.h): shapes of the e4m3 byte arena [depth][R][Lmax][2C] and of its fp32 scale table [depth][R][Lmax][2H] -
    2C + 8H = 136 H bytes per token and layer against the 256 H of the bf16 arena: 17/32"""
    return (depth, R, Lmax, 2 * H * 64), (depth, R, Lmax, 2 * H)


class KV8Arena(NamedTuple):
    """the e4m3 K/V arena of one stream: q = the bytes (uint8), scale = one power-of-two fp32 per (layer, sequence, token, k or v head)"""
    q: torch.Tensor
    scale: torch.Tensor

    @property
    def nbytes(self) -> int:
        return self.q.numel() + 4 * self.scale.numel()


class _Pack(dict):
    """the packed copies; `lazy` holds makers of entries that are built on first use (the fp32 matrices of a gemm_precision='bf16x3' model: only
    forward() and training read them)"""

    def __init__(self):
        super().__init__()
        self.lazy: Dict[str, Any] = {}

    def __missing__(self, key):
        if key not in self.lazy:
            raise KeyError(key)
        v = self[key] = self.lazy.pop(key)()
        return v


class ControlVAR(nn.Module):
    """Joint (control, image) next-scale transformer (reference: models/control_var.py:23-689).

    Built: aln=1 (AdaLNSABlock), multi_cond as given, and of the non-default variants ``shared_aln``
    and ``type_pos`` for inference, forward and training (both fold into tables at pack time, no extra kernel).
    ``aln < 0`` (SABlock: affine LayerNorms + layer scale, basic_var.py:128-176) is likewise folded into the adaLN layout.
    ``bidirectional`` (image-first order, mask_first=False) swaps the first two tokens and the type ids.
    ``separate_decoding`` (control half of a scale decoded before its image half; with ``indep`` the halves are blind to each other):
    masks as (level end, hole) tables of the attention kernels, the two-pass inference branch, and the mask applied at inference for
    ``indep``.  ``indep`` defaults to True as upstream's class does (a no-op without separate_decoding); the factory passes False.
    ``more_smooth`` = Gumbel-softmax soft code embeddings.  ``separator`` (+18 special tokens, head V + 18, special_embed): upstream
    indexes special_embed with V + k and raises IndexError everywhere (control_var.py:549,606); built with the evidently intended
    index k for forward() / training and the joint inference branch - including upstream's placement quirks there (:507-509,538).
    Width: ``embed_dim`` up to CVAR_WIDE_CMAX = 3072 at 64 channels per head (depth 48 by the factories' ``64 * depth``; d36 = 2304, d40 = 2560), in
    every mode.  Above 2048 the adaLN rows come from the kernels of include/cvar_wide.h as a launch of their own at every pass size;
    a wider model raises ValueError.
    """
    _control = True

    def __init__(self, vae_local: VQVAE, num_classes=1000, norm_eps=1e-6, aln=1, aln_gamma_init=1e-3, shared_aln=False,
                 cond_drop_rate=0.1, depth=16, embed_dim=1024, num_heads=16, mlp_ratio=4., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., layer_scale=-1., tau=4, cos_attn=False, patch_nums=DEFAULT_PATCH_NUMS,
                 flash_if_available=True, fused_if_available=True, mask_factor=2, bidirectional=False, separate_decoding=False,
                 separator=False, type_pos=False, indep=True, multi_cond=False,
                 compute_dtype=None, init_seed: int = 0, deterministic_plan: bool = False, sampler: str = 'counter', gemm_precision: Optional[str] = None,
                 kv_precision: Optional[str] = None):
        """gemm_precision (an addition of this library; fp32 models only; also settable: ``model.gemm_precision = 'bf16x3'``): None = the linear layers run
        in compute_dtype; 'bf16x3' = the fp32 model with its six GEMM families (ada, qkv, proj, fc1, fc2, head) taken as split-bf16 products on the bf16
        matrix pipe - operands carried as hi + lo in bf16, three products per multiply as three K segments of one bf16 GEMM, fp32 accumulation and fp32
        outputs (include/cvar_serve.h).  Everything else - residual stream, adaLN, K/V arena, attention, sampler, quantizer, VQVAE - is the
        fp32 mode's, through the same kernels.  Inference only: forward() and training on such a model run the fp32 path.
        'fp8' (bf16 models only) = the bf16 model with the qkv, proj, fc1 and fc2 GEMMs of every block on OCP e4m3 operands with one power-of-two scale per
        row, fp32 accumulation and the bf16 mode's epilogues (include/cvar_serve.h); the head, the adaLN table, the residual stream, the K/V arena,
        attention, sampler, quantizer and VQVAE are the bf16 mode's, through the same kernels.  Inference only: forward() and training run the bf16 path.

        kv_precision (an addition of this library; bf16 models with gemm_precision None or 'fp8'; also settable: ``model.kv_precision = 'fp8'``): None = the
        K/V arena of generation holds compute_dtype values; 'fp8' = it holds OCP e4m3 bytes with one power-of-two fp32 scale per (token, k or v head) - 17/32
        of the bf16 arena (include/cvar_kvcache.h).  The qkv GEMM then writes the k|v rows of a pass to a scratch, cvar_kv_append_fp8 quantises
        them into the arena and the attention kernel dequantises (exactly) while it stages its tiles; everything else is the mode's own.  Generation only:
        forward() and training keep the bf16 arena.

        deterministic_plan (an addition of this library): every transformer GEMM runs on the unsliced tile kernels whatever its row count - no small-M weight-streaming
        kernel, no K slices - so the fp32 summation order of a row does not depend on how many rows ride beside it, and one (label, condition, g_seed) in batch row 0 gives
        the same logits and tokens BIT FOR BIT at any batch size (default False: the small-M plans are 2.0x / 1.24x / 1.05x faster at B = 1 / 8 / 32 and move bf16 logits by ~5e-3 of
        max|logit| between batch sizes; tests/test_gpu_configs.py).  Can also be flipped on a built model: ``model.deterministic_plan = True``.

        sampler (an addition of this library; also settable: ``model.sampler = 'torch'``) picks where a sampled draw (top_k != 1) comes from:
          'counter' (default): the library's own counter-based generator keyed by (g_seed, scale, row) - no host work, capturable by
                     graphed_generator, a sample's draw independent of the batch it rides in;
          'torch':   the reference's generator calls (torch_draw_schedule): torch.multinomial's Exp(1) noise and more_smooth's Gumbel noise are
                     drawn with torch on ``model.rng`` (reseeded by g_seed; g_seed=None: the device's default generator) and the HIP
                     sampler races argmax(p / q) on them - the same tokens as the reference given the same logits and generator state.
                     As upstream, a sample's draw then depends on the batch it rides in (deterministic_plan's batch independence covers
                     the logits and greedy ids only); graphed_generator refuses this mode."""
        super().__init__()
        self.deterministic_plan = bool(deterministic_plan)
        self.sampler = sampler
        self._rng: Optional[torch.Generator] = None
        self._rng_assigned = False
        if separator and not (self._control and mask_factor == 2):
            raise NotImplementedError('separator needs the joint (control, image) sequence')
        if separator and len(patch_nums) != 10:
            raise NotImplementedError('separator: upstream hard-codes 18 special tokens (control_var.py:543)')
        if separate_decoding and not (self._control and mask_factor == 2):
            raise NotImplementedError('separate_decoding needs the joint (control, image) sequence')
        if bidirectional and not (self._control and mask_factor == 2):
            raise NotImplementedError('bidirectional needs the joint (control, image) sequence')
        sa_block = aln < 0                                           # control_var.py:41: using_aln = aln >= 0
        if type_pos and not (self._control and mask_factor == 2):
            raise NotImplementedError('type_pos needs the joint (control, image) sequence: upstream builds type_1L with 2*sum(pn^2) entries')
        if self._control and mask_factor == 2 and not multi_cond:
            raise NotImplementedError('mask_factor=2 requires multi_cond=True (every shipped config)')
        if embed_dim // num_heads != 64:
            raise NotImplementedError('head_dim must be 64')
        self.cfg = VarConfig(depth=depth, mask_factor=mask_factor, multi_cond=bool(multi_cond) and self._control and mask_factor == 2,
                             control=self._control, patch_nums=tuple(patch_nums), vocab=vae_local.vocab_size, cvae=vae_local.Cvae,
                             num_classes=num_classes, embed_dim=embed_dim, num_heads=num_heads, norm_eps=norm_eps, tau=float(tau),
                             cos_attn=bool(cos_attn), mlp_ratio=mlp_ratio, cond_drop_rate=cond_drop_rate, drop_path_rate=float(drop_path_rate),
                             shared_aln=bool(shared_aln) and not sa_block, type_pos=bool(type_pos), sa_block=sa_block,
                             layer_scale=float(layer_scale) if sa_block else -1.0, bidirectional=bool(bidirectional),
                             separate_decoding=bool(separate_decoding), indep=bool(indep) and self._control and mask_factor == 2,
                             separator=bool(separator))
        self.separate_decoding, self.indep, self.separator, self.type_pos = self.cfg.separate_decoding, bool(indep), self.cfg.separator, self.cfg.type_pos
        cfg = self.cfg
        self.bidirectional = cfg.bidirectional
        self.Cvae, self.V = cfg.cvae, cfg.vocab
        self.depth, self.C, self.D, self.num_heads = depth, cfg.C, cfg.C, cfg.H
        if cfg.C > _lib.WIDE_CMAX:
            # surfaced here instead of as CVAR_EUNSUPPORTED from inside a kernel call: the adaLN kernels keep a row of the residual stream in one wave's
            # registers (cvar_ln_modulate up to 2048, include/cvar_wide.h up to CVAR_WIDE_CMAX = depth <= 48 at 64 channels per head)
            raise ValueError(f'embed_dim {cfg.C} > CVAR_WIDE_CMAX = {_lib.WIDE_CMAX}: the adaLN kernels of controlvar_amd hold one row per wave '
                             f'(depth <= {_lib.WIDE_CMAX // 64})')
        self.patch_nums, self.mask_factor, self.multi_cond = tuple(patch_nums), mask_factor, cfg.multi_cond
        py = cfg.pyramid
        self.L, self.first_l = py.L, py.first_l
        self.begin_ends = list(zip(py.begin, py.end))
        self.num_stages_minus_1 = len(patch_nums) - 1
        self.num_classes = num_classes
        self.cond_drop_rate = cond_drop_rate
        self.prog_si = -1
        self.vae_proxy: Tuple[VQVAE] = (vae_local,)                  # tuple proxy: not a submodule (control_var.py:72-73)
        self.vae_quant_proxy = (vae_local.quantize,)
        self.compute_dtype = _compute_dtype(compute_dtype) if compute_dtype is not None else vae_local.compute_dtype
        _register_tree(self, var_state_shapes(cfg), synth_var_state(cfg, init_seed), requires_grad=True)
        self._packed = None
        self._arena = None
        self._gemm_precision = None
        self._kv_precision = None
        self.gemm_precision = gemm_precision
        self.kv_precision = kv_precision
        self.last_trace: Optional[dict] = None

    # ---- plumbing
    def load_state_dict(self, state_dict, strict=True, assign=False):
        self._packed = None
        if getattr(self, '_lora', None) is not None:        # LoRA model: peft's key layout loads too (controlvar_amd/lora.py)
            from .lora import to_module_layout
            self._packed_base = None
            state_dict = to_module_layout(state_dict)
        return super().load_state_dict(state_dict, strict=strict, assign=assign)

    def _apply(self, fn, *a, **k):
        self._packed = None
        self._packed_base = None
        self._arena = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.pos_1LC.device

    @property
    def sampler(self) -> str:
        return self._sampler

    @sampler.setter
    def sampler(self, value: str):
        if value not in SAMPLERS:
            raise ValueError(f'sampler must be one of {SAMPLERS}, got {value!r}')
        self._sampler = value

    @property
    def gemm_precision(self) -> Optional[str]:
        return self._gemm_precision

    @gemm_precision.setter
    def gemm_precision(self, value: Optional[str]):
        if value not in GEMM_PRECISIONS:
            raise ValueError(f'gemm_precision must be one of {GEMM_PRECISIONS}, got {value!r}')
        if value == 'fp8' and self.compute_dtype != torch.bfloat16:
            raise ValueError(f"gemm_precision='fp8' needs a compute_dtype=torch.bfloat16 model: it is the bf16 model with e4m3 qkv / proj / fc1 / fc2 layers, "
                             f"and this model computes in {self.compute_dtype} (build it with compute_dtype=torch.bfloat16)")
        if value == 'bf16x3' and self.compute_dtype != torch.float32:
            raise ValueError(f"gemm_precision={value!r} needs a compute_dtype=torch.float32 model: it is the fp32 model with split-bf16 linear layers, "
                             f"and this model computes in {self.compute_dtype} (build it with compute_dtype=torch.float32)")
        if value is not None and getattr(self, '_adapter_bank', None) is not None:
            raise NotImplementedError(_no_bank_message(value))
        if value == 'bf16x3' and getattr(self, '_kv_precision', None) is not None:
            raise ValueError(_KV8_NO_X3)
        if value != self._gemm_precision:       # the packed matrices and the arena key belong to the mode
            self._packed = None
            self._packed_base = None
            self._arena = None
        self._gemm_precision = value

    @property
    def kv_precision(self) -> Optional[str]:
        return self._kv_precision

    @kv_precision.setter
    def kv_precision(self, value: Optional[str]):
        if value not in KV_PRECISIONS:
            raise ValueError(f'kv_precision must be one of {KV_PRECISIONS}, got {value!r}')
        if value is not None and self._gemm_precision == 'bf16x3':
            raise ValueError(_KV8_NO_X3)
        if value is not None and self.compute_dtype != torch.bfloat16:
            raise ValueError(f"kv_precision={value!r} needs a compute_dtype=torch.bfloat16 model: the e4m3 K/V cache trades precision for memory, and this model "
                             f"computes in {self.compute_dtype}, a mode that exists for exactness (build it with compute_dtype=torch.bfloat16)")
        if value != self._kv_precision:         # the arena belongs to the mode; the packed matrices do not
            self._arena = None
        self._kv_precision = value

    @property
    def rng(self) -> torch.Generator:
        """The generator of sampler='torch' (control_var.py:68), created on the model's device when first used.  A generator assigned by the
        user stays as given; a CPU one is allowed (the noise is drawn on the CPU and copied over: CPU recordings, small batches)."""
        if self._rng is None or (not self._rng_assigned and self._rng.device != self.device):
            self._rng = torch.Generator(device=self.device)
        return self._rng

    @rng.setter
    def rng(self, generator: torch.Generator):
        if not isinstance(generator, torch.Generator):
            raise TypeError(f'model.rng must be a torch.Generator, got {type(generator).__name__}')
        self._rng, self._rng_assigned = generator, True

    def _state_sig(self):
        return _tensor_sig(self)

    def _matrix_copies(self) -> Tuple[Dict[str, torch.Tensor], Tuple[str, ...]]:
        """(state_dict key -> the contiguous slice of the packed copies that holds exactly this weight matrix, the packed keys those
        slices cover completely).  The fused optimizer writes the rounded update straight into the slices (cvar_adam_tensor.w16)
        and then calls _pack(fresh=keys); bf16 compute only (the fp32 form keeps no separate rounding)."""
        P, cfg = self._pack(), self.cfg
        C, depth = cfg.C, cfg.depth
        if self.compute_dtype != torch.bfloat16:
            return {}, ()
        out: Dict[str, torch.Tensor] = {}
        keys = ['w_qkv', 'w_proj', 'w_fc1', 'w_fc2', 'w_head']
        for i in range(depth):
            for key, name in (('w_qkv', 'attn.mat_qkv.weight'), ('w_proj', 'attn.proj.weight'), ('w_fc1', 'ffn.fc1.weight'), ('w_fc2', 'ffn.fc2.weight')):
                out[f'blocks.{i}.{name}'] = P[key][i]
        if not cfg.sa_block and not cfg.shared_aln:       # the other two forms derive w_ada (zeros / one shared matrix per block)
            for i in range(depth):
                out[f'blocks.{i}.ada_lin.1.weight'] = P['w_ada'][i * 6 * C:(i + 1) * 6 * C]
            out['head_nm.ada_lin.1.weight'] = P['w_ada'][depth * 6 * C:]
            keys.append('w_ada')
        hw = 'head.1.weight' if cfg.sa_block else 'head.weight'
        out[hw] = P['w_head'][:cfg.head_out]
        return out, tuple(keys)

    def _pack(self, check: bool = False, fresh: Sequence[str] = (), base: bool = False):
        """GEMM-ready device copies of the weights (stacked per kind, compute dtype).  check=True (every public entry point and
        the training engine's forward): rebuild when any parameter changed since - torch.optim steps through the autograd bridge,
        manual in-place edits, .data swaps (the copies used to go stale on that path).
        fresh: keys of the current copies that are already up to date (the fused optimizer updated them in its own pass) - those tensors
        are kept, everything else is rebuilt from the parameters.
        LoRA model (controlvar_amd/lora.py): the copies hold W + s B A (inference runs the adapter-free kernels; the signature covers the
        adapters); base=True returns the copies of the frozen base weights instead - what the training engine runs (the dropout of the
        adapter branch makes the merged form wrong there).  Without adapters ``base`` changes nothing."""
        lora = getattr(self, '_lora', None)
        if base and lora is not None:
            return self._pack_lora_base()
        if not fresh and self._packed is not None and (not check or self._packed_sig == self._state_sig()):
            return self._packed
        old = self._packed if fresh else None
        if fresh and old is None:
            raise RuntimeError('_pack(fresh=...) without packed copies to keep')
        P = self._build_pack(old, fresh, lora)
        self._packed = P
        self._packed_sig = self._state_sig()
        self._pack_gen = getattr(self, '_pack_gen', 0) + 1          # consumers of derived copies (TrainEngine.WT) compare this
        return P

    def _base_sig(self):
        return tuple((t.data_ptr(), t._version) for n, t in list(self.named_parameters()) + list(self.named_buffers()) if '.lora_' not in n)

    def _pack_lora_base(self):
        """packed copies of the frozen base weights of a LoRA model (rebuilt only when a base tensor changes)"""
        if getattr(self, '_packed_base', None) is not None and self._packed_base_sig == self._base_sig():
            return self._packed_base
        self._packed_base = self._build_pack(None, (), None)
        self._packed_base_sig = self._base_sig()
        self._pack_base_gen = getattr(self, '_pack_base_gen', 0) + 1
        return self._packed_base

    def _build_pack(self, old, fresh: Sequence[str], lora, host: bool = False):
        """host=True: build the copies where the parameters are, CPU included (the layout tests; nothing on the CPU computes with them)"""
        dev, T, cfg = self.device, self.compute_dtype, self.cfg
        if not host:
            if dev.type != 'cuda':
                raise RuntimeError('controlvar_amd models compute on the GPU only; call .to("cuda") first')
            ops.ensure_splitk_workspace(dev)
        sd = {k: v.detach() for k, v in self.state_dict().items()}
        if getattr(self, '_lora', None) is not None:
            from .lora import merged_state
            sd = merged_state(sd, self._lora) if lora is not None else {k: v for k, v in sd.items() if '.lora_' not in k}
        C, depth = cfg.C, cfg.depth
        P: Dict[str, Any] = _Pack()
        blk = lambda i, s: sd[f'blocks.{i}.{s}']
        x3 = self.gemm_precision == 'bf16x3'
        f8 = self.gemm_precision == 'fp8'
        F8_KEYS = ('w_qkv', 'w_proj', 'w_fc1', 'w_fc2')

        def quant_stack(w):
            """fp32 [depth][N][K] -> (e4m3 bytes [depth * N][ldq], fp32 row scales [depth * N]) through the library's row pass: torch converts nothing"""
            w = w.float().contiguous()
            rows, K = w.shape[0] * w.shape[1], w.shape[2]
            ldq = ops.fp8_ldq(K)
            q = torch.empty(rows, ldq, device=w.device, dtype=torch.uint8)
            sc = torch.empty(rows, device=w.device, dtype=torch.float32)
            ops.quant_rows_fp8(w, q, sc, M=rows, K=K, ldq=ldq)
            return q, sc

        def matrix(key, make):
            """one stacked weight matrix, GEMM-ready: in compute dtype, or (gemm_precision='bf16x3') as split rows [w_hi | w_hi | w_lo] under key + '_x3' - the
            fp32 copy is then built only when forward() / training ask for it (both copies of every matrix are never held from the start)"""
            if f8 and key in F8_KEYS:
                # gemm_precision='fp8': e4m3 rows + one power-of-two scale per row from the fp32 parameters (a merged LoRA is folded in `sd` already);
                # the bf16 copy is built only when forward() / training ask for it
                if host:
                    raise RuntimeError("gemm_precision='fp8': the e4m3 weight stacks are made by the device row pass (no host packing)")
                P[key + '_f8'], P['s_' + key[2:]] = quant_stack(make())
                if key in fresh:
                    P[key] = old[key]
                else:
                    P.lazy[key] = lambda: make().to(T).contiguous()
            elif key in fresh:
                P[key] = old[key]
            elif x3:
                P[key + '_x3'] = _split_weight_rows(make())
                P.lazy[key] = lambda: make().to(T).contiguous()
            else:
                P[key] = make().to(T).contiguous()

        stack = lambda name: (lambda: torch.stack([blk(i, name) for i in range(depth)]))
        matrix('w_qkv', stack('attn.mat_qkv.weight'))
        P['b_qkv'] = torch.stack([torch.cat((blk(i, 'attn.q_bias'), torch.zeros_like(blk(i, 'attn.q_bias')), blk(i, 'attn.v_bias')))
                                  for i in range(depth)]).float().contiguous()
        matrix('w_proj', stack('attn.proj.weight'))
        P['b_proj'] = torch.stack([blk(i, 'attn.proj.bias') for i in range(depth)]).float().contiguous()
        matrix('w_fc1', stack('ffn.fc1.weight'))
        P['hid'] = blk(0, 'ffn.fc1.weight').shape[0]
        P['b_fc1'] = torch.stack([blk(i, 'ffn.fc1.bias') for i in range(depth)]).float().contiguous()
        matrix('w_fc2', stack('ffn.fc2.weight'))
        P['b_fc2'] = torch.stack([blk(i, 'ffn.fc2.bias') for i in range(depth)]).float().contiguous()
        # every ada_lin of the model in ONE weight: rows [i*6C,(i+1)*6C) = block i, last 2C rows = head_nm
        head_w, head_b = ('head.1.weight', 'head.1.bias') if cfg.sa_block else ('head.weight', 'head.bias')
        if cfg.sa_block:
            # SABlock (basic_var.py:128-160) in the adaLN layout: LayerNorm(x) * w + b == LN0(x) * (1 + (w - 1)) + b and the
            # residual gates are the layer-scale gammas (or 1).  The generator weight is zero, its bias holds the constants,
            # so every kernel (and the backward: d bias = column sum of d ada) is shared with the adaLN form.
            one = torch.ones(C, device=dev)
            gam = (lambda i, k: blk(i, k)) if cfg.layer_scale >= 0 else (lambda i, k: one)
            b_blk = [torch.cat([gam(i, 'gamma1'), gam(i, 'gamma2'), blk(i, 'norm1.weight') - 1, blk(i, 'norm2.weight') - 1,
                                blk(i, 'norm1.bias'), blk(i, 'norm2.bias')]) for i in range(depth)]
            make_ada = lambda: torch.zeros(depth * 6 * C + 2 * C, C, device=dev)
            b_all = torch.cat(b_blk + [sd['head.0.weight'] - 1, sd['head.0.bias']])
        elif cfg.shared_aln:
            # (ada_gss + SharedAdaLin(cond)) of block i (basic_var.py:204-205) == a Linear whose weight is the shared one and whose
            # bias is shared bias + ada_gss_i: replicate the weight per block so the one-GEMM layout below serves both forms
            w_blk = [sd['shared_ada_lin.1.weight']] * depth
            b_blk = [sd['shared_ada_lin.1.bias'] + blk(i, 'ada_gss').reshape(-1) for i in range(depth)]
        else:
            w_blk = [blk(i, 'ada_lin.1.weight') for i in range(depth)]
            b_blk = [blk(i, 'ada_lin.1.bias') for i in range(depth)]
        if not cfg.sa_block:
            make_ada = lambda: torch.cat(w_blk + [sd['head_nm.ada_lin.1.weight']])
            b_all = torch.cat(b_blk + [sd['head_nm.ada_lin.1.bias']])
        matrix('w_ada', make_ada)
        P['b_ada'] = b_all.float().contiguous()
        P['n_ada'] = depth * 6 * C + 2 * C
        hw, hb = sd[head_w], sd[head_b].float()
        make_head = lambda: hw
        if cfg.head_ld != hw.shape[0]:               # separator: V + 18 = 4114 columns -> padded to 4120 (zero weight, -1e30 bias: softmax weight exactly 0)
            make_head = lambda: torch.cat((hw, hw.new_zeros(cfg.head_ld - hw.shape[0], hw.shape[1])))
            hb = torch.cat((hb, hb.new_full((cfg.head_ld - hb.shape[0],), -1e30)))
        matrix('w_head', make_head)
        P['b_head'] = hb.contiguous()
        P['special'] = sd['special_embed.weight'].float().contiguous() if cfg.separator else None
        P['sp_rows'] = {}
        P['w_we'] = sd['word_embed.weight'].float().contiguous()
        P['b_we'] = sd['word_embed.bias'].float().contiguous()
        P['lvl_pos'] = (sd['lvl_embed.weight'][sd['lvl_1L'][0]] + sd['pos_1LC'][0]).float().contiguous()      # (L, C)
        # type_pos (control_var.py:99-117): upstream adds type_embed[type_1L] to every row in forward() (:622-624), to the
        # rows of scales >= 1 in autoregressive_infer_cfg (:423-424,482-483) and nowhere in conditional_infer_cfg
        # the '_' tables are the image-first order (mask_first=False, bidirectional): type ids from type_1L_ (:424,624)
        P['lvl_pos_fwd'] = P['lvl_pos_gen'] = P['lvl_pos_fwd_'] = P['lvl_pos_gen_'] = P['lvl_pos']
        if cfg.type_pos:
            for suf, buf in (('', 'type_1L'), ('_', 'type_1L_')):
                ty = sd['type_embed.weight'][sd[buf][0]].float()
                P['lvl_pos_fwd' + suf] = (P['lvl_pos'] + ty).contiguous()
                P['lvl_pos_gen' + suf] = P['lvl_pos_fwd' + suf].clone()
                P['lvl_pos_gen' + suf][:cfg.pyramid.first_l] = P['lvl_pos'][:cfg.pyramid.first_l]
        P['pos_start'] = sd['pos_start'][0].float().contiguous()
        P['pos_start_sw'] = P['pos_start'].flip(0).contiguous()
        P['class_emb'] = sd['class_emb.weight'].float().contiguous()
        P['cond_embed'] = sd['cond_embed.weight'].float().contiguous() if 'cond_embed.weight' in sd else None
        if cfg.uses_cos_attn:
            P['scale_mul'] = torch.stack([blk(i, 'attn.scale_mul_1H11').reshape(-1) for i in range(depth)]).float().contiguous()
        return P

    def _first_tokens(self, P, labels, types, x, cond, R: int, x_rows: int, table, mask_first: bool = True):
        """first-scale tokens [cond_token, sos] (+ pos_start + table rows); image first (mask_first=False, control_var.py:404-407,
        587) is [sos, cond_token]: the kernel runs with the two position rows exchanged, then the two token rows are exchanged."""
        py, C = self.cfg.pyramid, self.cfg.C
        if mask_first or py.first_l != 2:
            ops.first_tokens(P['class_emb'], P['cond_embed'], labels, types, P['pos_start'], table, x, cond, R, py.first_l, C, x_rows)
            return
        ops.first_tokens(P['class_emb'], P['cond_embed'], labels, types, P['pos_start_sw'], table[:2].flip(0).contiguous(), x, cond, R,
                         py.first_l, C, x_rows)
        xv = x[:R * x_rows].view(R, x_rows, C)
        xv[:, :2] = xv[:, :2].flip(1)

    def _special_rows(self, table, positions, rows):
        """(len(positions), C): special_embed[rows] + table[positions] - the separator tokens as they enter the residual stream"""
        P = self._pack()
        key = (table.data_ptr(), tuple(positions), tuple(rows))
        if key not in P['sp_rows']:
            P['sp_rows'][key] = (P['special'][list(rows)] + table[list(positions)]).contiguous()
        return P['sp_rows'][key]

    def _embed_teacher_forced(self, P, tok, x, B: int, table, mask_first: bool):
        """word_embed of the teacher-forcing tokens into the rows of x behind the first scale (+ level / position / type rows).  With
        separators the code tokens of every half go to their own row range and the special rows are copied in between
        (control_var.py:603-620, special_embed indexed by the label offset without V)."""
        cfg = self.cfg
        py, C = cfg.pyramid, cfg.C
        if not cfg.separator:
            ops.word_embed(tok, P['w_we'], P['b_we'], table, x, B, 1, py.L - py.first_l, cfg.cvae, C, py.L, py.first_l, lvl_off=py.first_l)
            return
        mapping = cfg.special_mapping(mask_first)
        xv = x[:B * py.L].view(B, py.L, C)
        cur = 0
        for k in range(1, len(py.patch_nums)):
            n = py.patch_nums[k] ** 2
            for h in range(2):
                row0 = py.begin[k] + h * (n + 1)
                ops.word_embed(tok[:, cur:cur + n].contiguous(), P['w_we'], P['b_we'], table, x, B, 1, n, cfg.cvae, C, py.L, row0, lvl_off=row0)
                cur += n
        pos = [int(p) for p in py.special_positions()]
        xv[:, pos] = self._special_rows(table, pos, [mapping[i] for i in range(len(pos))])

    def _get_arena(self, R: int, Lmax: int, kv_precision: Optional[str] = None):
        """KV arena [depth][R][Lmax][2C] (k | v halves; the queries of a scale are dead after its attention and live in a per-call scratch,
        like the reference's cache of k and v only, basic_var.py:108-111) of the calling stream (generations running concurrently on
        different streams must not share it).  kv_precision='fp8' (generation passes the model's; forward() does not): a KV8Arena - the e4m3
        bytes and their scale table (include/cvar_kvcache.h)"""
        sid = torch.cuda.current_stream(self.device).cuda_stream
        key = (R, Lmax, self.compute_dtype, self.gemm_precision, kv_precision)
        if self._arena is None:
            self._arena = {}
        ent = self._arena.get(sid)
        if ent is None or ent[0] != key:
            if kv_precision == 'fp8':
                sq, ss = kv8_arena_shapes(self.cfg.depth, R, Lmax, self.cfg.H)
                buf = KV8Arena(torch.empty(sq, device=self.device, dtype=torch.uint8), torch.empty(ss, device=self.device, dtype=torch.float32))
            else:
                buf = torch.empty(self.cfg.depth, R, Lmax, 2 * self.cfg.C, device=self.device, dtype=self.compute_dtype)
            ent = self._arena[sid] = (key, buf)
        return ent[1]

    # ---- one pass of all blocks + head over l new tokens per sequence
    def _pass_mode(self, ad, x3: Optional[bool]) -> Optional[str]:
        """the operand form of a pass's linear layers: None (compute dtype), 'bf16x3' or 'fp8'.  x3: None = the model's gemm_precision decides; False = the
        compute-dtype form whatever the mode (forward(): the fp32 / bf16 matrices are then built on first use).  The adapter bank exists in the compute-dtype
        form only: refused here, before anything is allocated or launched."""
        mode = self.gemm_precision if x3 is None else ('bf16x3' if x3 else None)
        if mode is not None and ad is not None:
            raise NotImplementedError(_no_bank_message(mode))
        return mode

    def _blocks_and_head(self, x, ada, R: int, l: int, q_off: int, Lmax: int, arena, lvl_end=None, holes=None, ad=None, x3: Optional[bool] = None):
        """x: (R*l, C) fp32 residual stream (updated in place).  Returns logits (R*l, V) fp32.  x3: see _pass_mode.
        ONE walk for every mode.  The walk owns the offsets into the ada row, the qkv launch (q | k | v in one GEMM: the q columns land in a scratch, the k | v rows
        straight in their arena slots through the row remap), the arena / e4m3-arena branch with cos-norm and attention, the gate + residual epilogues of proj and
        fc2, and the head.  A mode is three leaves over its own scratch, chosen once per pass:
          norm(sc, sh, head)       writes the adaLN rows that qkv / fc1 / the head read and returns them as a GEMM operand
          feed(name, i, a)         turns the attention output (proj), the adaLN rows (fc1, adapter bank only) or the GELU output (fc2) into that layer's operand;
                                   called for the layers the mode names in `fed`, the others read `a` as it is
          linear(layer, i, a, out) one of qkv / proj / fc1 / fc2 / head of block i, epilogue keywords passed through; `layer` is the mode's entry of `layers`
                                   (weight, N, K as the call takes them), resolved before the loop
        compute dtype: cvar_ln_modulate, cvar_gemm on w_*; below FUSE_LN_BELOW rows proj / fc2 also write the adaLN rows of the op that follows (ln=).  With ad
            (per-request adapters: (lora.bank_pack, slot (R,) int32 on the device)) proj / fc1 / fc2 run over the K-augmented weights [W | B_0 .. B_{n-1} | 0] and
            feed is ops.lora_down_rows: it widens the operand by each row's own s x A^T.  Without it the launches are exactly the adapter-free ones.
        'bf16x3': every GEMM is ONE bf16 cvar_gemm over K' = 3 K, activation rows [hi | lo | hi] against weight rows [w_hi | w_hi | w_lo], fp32 output.  The adaLN rows
            leave cvar_ln_modulate_split3 split; the attention and GELU outputs are fp32 round trips through cvar_split3 (the next lever).
        'fp8': qkv / proj / fc1 / fc2 are cvar_gemm_fp8 on e4m3 operands (include/cvar_serve.h).  The adaLN rows leave cvar_ln_modulate_fp8 quantised; the attention and
            GELU outputs are bf16 round trips through cvar_quant_rows_fp8.  The head is the bf16 mode's: cvar_ln_modulate and cvar_gemm.  No plan
            slices K: deterministic_plan changes nothing in the four e4m3 GEMMs.
        ln_out of the GEMM makes bf16 / fp32 rows only, so under 'bf16x3' and 'fp8' adaLN is its own launch at every M.  The arena, the query scratch and the attention
        and GELU outputs hold compute_dtype in every mode ('bf16x3' is an fp32 model, 'fp8' a bf16 one)."""
        mode = self._pass_mode(ad, x3)
        P, cfg = self._pack(), self.cfg
        C, H, T, hid, n_ada, eps = cfg.C, cfg.H, self.compute_dtype, P['hid'], P['n_ada'], cfg.norm_eps
        M, dev = R * l, x.device
        bf = torch.bfloat16
        buf = lambda cols, dtype: torch.empty(M, cols, device=dev, dtype=dtype)
        sm = not self.deterministic_plan      # small-M plans (weight-streaming kernel, K slices): the summation order then depends on M; off = tile kernels only, unsliced
        NK = dict(qkv=(3 * C, C), proj=(C, C), fc1=(hid, C), fc2=(C, hid), head=(cfg.head_ld, C))          # (N, K) of every linear layer
        kx = 0 if ad is None else ad[0]['kx']                         # the bank's columns: proj / fc1 / fc2 operands and weights are wider by them
        # Every mode allocates its scratch first: o = attention output, hbuf = GELU output, qs = queries of this pass (R, l, C), all in T; the rest are the mode's
        # operands.  (The order of these allocations is part of the pass: the caching allocator reuses freed blocks by it, and torch.cuda.max_memory_allocated()
        # counts whole blocks - the peak that tests/test_gpu_block_pass_launches.py holds a fresh process to follows from it.)
        fc1_out, fuse_ln, fed = {}, False, ()           # fed: the layers whose operand feed() has to make
        # adaLN rows wider than 2048: the entry points of include/cvar_wide.h; narrow models call ops exactly as before
        ln_rows, ln_rows3, ln_rows8 = ((ops.ln_modulate_wide, ops.ln_modulate_split3_wide, ops.ln_modulate_fp8_wide) if C > 2048 else
                                       (ops.ln_modulate, ops.ln_modulate_split3, ops.ln_modulate_fp8))
        if mode is None:
            u = buf(C, T)                                             # adaLN rows: operand of qkv / fc1 / head
            o = buf(C, T)
            wide = {}
            if ad is not None:
                wide['proj'] = buf(C + kx, T)                         # [o | u_proj of the row's slot, zeros elsewhere]
                wide['fc1'] = buf(C + kx, T)                          # [adaLN output | u_fc1]
            hbuf = buf(hid + kx, T)                                   # adapters: [gelu | u_fc2], fc1 writes it through ldc
            qs = buf(C, T)
            W = {n: P['w_' + n] for n in NK}
            ld = dict(qkv=C, proj=C + kx, fc1=C + kx, fc2=hid + kx, head=C)          # K = lda = ldw of every call
            fc1_out = dict(ldc=hid + kx)
            # Small passes (early scales, small batches): proj / fc2 also produce the adaLN input of the op that follows (cvar_gemm_desc.ln_out) - their split-K
            # reduction finishes rows, so LayerNorm + modulation ride in that launch instead of a cvar_ln_modulate of their own (same bits).  Large passes keep the
            # separate launch: their GEMMs finish tiles, not rows.  So do all passes of a model wider than 2048: ln_out stops there (include/cvar.h), and the
            # separate launch is the wide kernel of include/cvar_wide.h.
            fuse_ln = M < FUSE_LN_BELOW and C <= 2048

            def norm(sc, sh, head=False):
                ln_rows(x, ada, sc, sh, n_ada, l, u, M, C, eps)
                return u

            def linear(layer, i, a, out, **epi):
                w, N, K = layer
                ops.gemm(a, w, out, M=M, N=N, K=K, w_off=i * N * K, small_m=sm, split_k=sm, **epi)

            if ad is not None:
                BK, slot = ad
                fed = ('proj', 'fc1', 'fc2')
                W.update((n, BK['W'][n]) for n in ('proj', 'fc1', 'fc2'))

                def feed(name, i, a):
                    K, kw = NK[name][1], ld[name]
                    if name == 'fc2':                                     # fc1 wrote the wide buffer itself: no copy
                        ops.lora_down_rows(a, BK['A'][name][i], BK['scale'], slot, a, R=R, l=l, K=K, kpad=kx, ldx=kw, ldxa=kw)
                        return a
                    xa = wide[name]
                    ops.lora_down_rows(a, BK['A'][name][i], BK['scale'], slot, xa, R=R, l=l, K=K, kpad=kx, ldxa=kw, x_copy=xa, ld_copy=kw)
                    return xa
            layers = {n: (W[n], NK[n][0], ld[n]) for n in NK}
        elif mode == 'bf16x3':
            u3 = buf(3 * C, bf)                                       # split adaLN rows: operand of qkv / fc1 / head
            o = buf(C, T)
            wide = dict(proj=buf(3 * C, bf))
            hbuf = buf(hid, T)
            wide['fc2'] = buf(3 * hid, bf)
            qs = buf(C, T)

            def norm(sc, sh, head=False):
                ln_rows3(x, ada, sc, sh, n_ada, l, u3, M, C, eps)
                return u3

            fed = ('proj', 'fc2')
            layers = {n: (P['w_' + n + '_x3'], NK[n][0], 3 * NK[n][1]) for n in NK}

            def feed(name, i, a):
                return ops.split3(a, wide[name], M, NK[name][1])

            def linear(layer, i, a, out, **epi):
                w, N, K = layer
                ops.gemm(a, w, out, M=M, N=N, K=K, w_off=i * N * K, small_m=sm, split_k=sm, **epi)
        else:
            ldq = {C: ops.fp8_ldq(C), hid: ops.fp8_ldq(hid)}              # row bytes of an e4m3 operand of C / hid columns
            rows8 = lambda K: (buf(ldq[K], torch.uint8), torch.empty(M, device=dev, dtype=torch.float32))          # e4m3 bytes + one scale per row
            u8 = rows8(C)                                             # quantised adaLN rows: operand of qkv / fc1
            o = buf(C, T)
            wide = dict(proj=rows8(C))
            hbuf = buf(hid, T)
            wide['fc2'] = rows8(hid)
            qs = buf(C, T)
            ub = buf(C, T)                                            # the head's adaLN rows
            fed = ('proj', 'fc2')
            layers = {n: (P['w_' + n + '_f8'], P['s_' + n], NK[n][0], ldq[NK[n][1]]) for n in ('qkv', 'proj', 'fc1', 'fc2')}
            layers['head'] = (P['w_head'], None, *NK['head'])                 # no e4m3 form: the bf16 GEMM

            def norm(sc, sh, head=False):
                if head:
                    ln_rows(x, ada, sc, sh, n_ada, l, ub, M, C, eps)
                    return ub
                ln_rows8(x, ada, sc, sh, n_ada, l, *u8, M, C, eps, ldq=ldq[C])
                return u8

            def feed(name, i, a):
                K = NK[name][1]
                ops.quant_rows_fp8(a, *wide[name], M=M, K=K, ldq=ldq[K])
                return wide[name]

            def linear(layer, i, a, out, ln=None, **epi):
                assert ln is None                                     # cvar_gemm_fp8 has no ln_out: fuse_ln stays off in this mode
                w, ws, N, K = layer
                if ws is None:
                    ops.gemm(a, w, out, M=M, N=N, K=K, small_m=sm, split_k=sm, **epi)
                    return
                ops.gemm_fp8(*a, w, ws, out, M=M, N=N, K=K, lda=K, ldw=K, w_off=i * N * K, ws_off=i * N, **epi)

        arena_stride = R * Lmax * 2 * C
        kv8 = isinstance(arena, KV8Arena)                           # kv_precision='fp8': k | v rows go to a scratch of the pass and from there, quantised, into the arena
        kvs = buf(2 * C, T) if kv8 else None
        # bf16 arena: the queries carry softmax scale * log2(e) from the producing epilogue (one rounding of q * c; the attention kernel then
        # spends no multiply per score - cvar_attention_prescaled).  fp32 arena: the exact row-wise kernel, unscaled queries.
        LOG2E = 1.4426950408889634
        pre = T == bf
        q_alpha = (float(cfg.attn_scale) * LOG2E) if (pre and not cfg.uses_cos_attn) else 1.0
        qkv_epi = dict(ldc=2 * C, split=(qs, C, C), split_alpha=q_alpha)
        ah = cfg.depth * 6 * C
        qkv, proj, fc1, fc2 = layers['qkv'], layers['proj'], layers['fc1'], layers['fc2']
        feed_proj, feed_fc1, feed_fc2 = 'proj' in fed, 'fc1' in fed, 'fc2' in fed
        u = norm(2 * C, 4 * C)
        for i in range(cfg.depth):
            a0 = i * 6 * C
            if kv8:
                # (the q split of cvar_gemm rides on its row-remap epilogue: the scratch is addressed as an arena of its own, Lmax = l, q_off = 0 - the identity)
                linear(qkv, i, u, kvs, bias=P['b_qkv'][i], remap=(l, l, 0), **qkv_epi)
                self._kv8_append_and_attend(i, arena, kvs, qs, o, R, l, q_off, Lmax, lvl_end, holes)
            else:
                linear(qkv, i, u, arena, bias=P['b_qkv'][i], c_off=i * arena_stride, remap=(l, Lmax, q_off), **qkv_epi)
                if cfg.uses_cos_attn:
                    ops.cos_qk_norm(arena, R, H, Lmax, q_off, l, P['scale_mul'], qkv_off=i * arena_stride, sm_off=i * H, q=qs, q_mul=LOG2E if pre else 1.0)
                ops.attention(arena, o, R, H, Lmax, q_off, l, float(cfg.attn_scale), lvl_end, qkv_off=i * arena_stride, holes=holes, q=qs, prescaled=pre)
            sc, sh = a0 + 3 * C, a0 + 5 * C
            linear(proj, i, feed('proj', i, o) if feed_proj else o, x, bias=P['b_proj'][i], gate=ada, gate_off=a0, ldg=n_ada, gate_rows=l, residual=x,
                   ln=(u, ada, sc, sh, n_ada, l, eps) if fuse_ln else None)
            if not fuse_ln:
                u = norm(sc, sh)
            linear(fc1, i, feed('fc1', i, u) if feed_fc1 else u, hbuf, bias=P['b_fc1'][i], act=ACT_GELU_TANH, **fc1_out)
            # the row finished by fc2 is the input of the next block's first adaLN (or of the head's)
            last = i + 1 == cfg.depth
            sc, sh = (ah, ah + C) if last else (a0 + 8 * C, a0 + 10 * C)
            linear(fc2, i, feed('fc2', i, hbuf) if feed_fc2 else hbuf, x, bias=P['b_fc2'][i], gate=ada, gate_off=a0 + C, ldg=n_ada, gate_rows=l, residual=x,
                   ln=(u, ada, sc, sh, n_ada, l, eps) if fuse_ln else None)
            if not fuse_ln:
                u = norm(sc, sh, head=last)
        logits = torch.empty(M, cfg.head_ld, device=dev, dtype=torch.float32)
        linear(layers['head'], 0, u, logits, bias=P['b_head'])
        return logits

    def _ada(self, cond: torch.Tensor, R: int, ad=None, x3: Optional[bool] = None):
        """the ada rows (R, n_ada) fp32 of every block and the head from one GEMM on SiLU(cond); the operand form follows _pass_mode ('fp8' keeps the bf16 one)"""
        x3 = self._pass_mode(ad, x3) == 'bf16x3'
        P, C, dev = self._pack(), self.cfg.C, cond.device
        cs = torch.empty(R, C, device=dev, dtype=self.compute_dtype)
        ops.silu_cast(cond, cs)
        if x3:
            cs3 = torch.empty(R, 3 * C, device=dev, dtype=torch.bfloat16)
            ops.split3(cs, cs3, R, C)
        ada = torch.empty(R, P['n_ada'], device=dev, dtype=torch.float32)
        sm = not self.deterministic_plan
        out = dict(M=R, N=P['n_ada'], bias=P['b_ada'], small_m=sm, split_k=sm)
        if x3:
            ops.gemm(cs3, P['w_ada_x3'], ada, K=3 * C, **out)
        elif ad is None:
            ops.gemm(cs, P['w_ada'], ada, K=C, **out)
        else:
            # per-request adapters: the operand [cs | one 16-column group per (ada target, slot)] is widened once per generation - one skinny
            # launch per target, each owning its 16 n columns (the last one also the padding) - against [W_ada | blockdiag]
            BK, slot = ad
            n, nt = BK['n'], self.cfg.depth + 1
            ld = C + BK['kxa']
            csa = torch.empty(R, ld, device=dev, dtype=self.compute_dtype)
            for t in range(nt):
                ops.lora_down_rows(cs, BK['A']['ada'][t], BK['scale'], slot, csa, R=R, l=1, K=C, kpad=16 * n if t + 1 < nt else BK['kxa'] - 16 * n * t,
                                   ldxa=ld, xa_off=16 * n * t, x_copy=csa if t == 0 else None, ld_copy=ld)
            ops.gemm(csa, BK['W']['ada'], ada, K=ld, lda=ld, ldw=ld, **out)
        return ada

    def _kv8_append_and_attend(self, i: int, arena: 'KV8Arena', kvs, qs, o, R: int, l: int, q_off: int, Lmax: int, lvl_end, holes):
        """kv_precision='fp8', layer i, behind the qkv GEMM that wrote this pass's k | v rows to the scratch kvs [R*l][2C] and its prescaled queries to qs:
        cos-norm on the scratch (a [R][l][2C] arena of its own: Lmax = l, q_off = 0), cvar_kv_append_fp8 into the arena rows (r, q_off + t), attention over the
        e4m3 arena (include/cvar_kvcache.h)"""
        cfg = self.cfg
        H = cfg.H
        a_off, s_off = i * R * Lmax * 2 * cfg.C, i * R * Lmax * 2 * H
        if cfg.uses_cos_attn:
            ops.cos_qk_norm(kvs, R, H, l, 0, l, self._pack()['scale_mul'], sm_off=i * H, q=qs, q_mul=1.4426950408889634)
        ops.kv_append_fp8(kvs, arena.q, arena.scale, R, H, Lmax, q_off, l, kv8_off=a_off, scale_off=s_off)
        ops.attention_kv8(arena.q, arena.scale, qs, o, R, H, Lmax, q_off, l, lvl_end, holes=holes, kv8_off=a_off, scale_off=s_off)

    def _as_labels(self, B, label_B, seed):
        dev = self.device
        if label_B is None:
            g = torch.Generator(device='cpu').manual_seed(seed)
            label_B = torch.randint(0, self.num_classes, (B,), generator=g)
        elif isinstance(label_B, int):
            label_B = torch.full((B,), self.num_classes if label_B < 0 else label_B)
        _check_index_range(label_B, 0, self.num_classes, 'label_B')
        return label_B.to(device=dev, dtype=torch.int32)

    def _as_types(self, B, cond_type, seed, allow_none=True):
        dev = self.device
        if cond_type is None:
            if B == 4:
                cond_type = torch.tensor([0, 1, 2, 3])                      # control_var.py:387-389
            else:
                g = torch.Generator(device='cpu').manual_seed(seed + 1)
                cond_type = torch.randint(0, 4, (B,), generator=g)
        elif isinstance(cond_type, int):
            assert 0 < cond_type <= 3                                      # control_var.py:395
            cond_type = torch.full((B,), cond_type)
        _check_index_range(cond_type, 0, 4, 'cond_type')
        return cond_type.to(device=dev, dtype=torch.int32)

    @torch.no_grad()
    def _prepare_rows(self, B, label_B, cond_type, four_way, seed, nrep: Optional[int] = None, K: int = 0):
        """labels / condition types of all CFG rows: [cond ; uncond] or the 4-branch layout (control_var.py:252-263,381-400); nrep == 1
        (cfg=None): the conditional rows alone.  K > 0 (regional guidance): label_B is (B, K) and the rows are [label_0 ; ... ; label_{K-1} ;
        uncond], each block B rows, the sample's condition type on the K conditional blocks and 4 on the last"""
        cfg = self.cfg
        labels = self._as_labels(B, label_B, seed)
        if K:
            labels = labels.t().reshape(-1)                              # (B, K) -> [label_0 rows ; ... ; label_{K-1} rows]
        empty = torch.full((B,), self.num_classes, device=labels.device, dtype=labels.dtype)
        nrep = (K + 1 if K else self._guidance_rows(four_way)) if nrep is None else nrep
        labels_all = torch.cat([labels] + [empty] * (1 if K else nrep - 1)).contiguous()
        types_all = None
        if cfg.mask_factor == 2:
            types = self._as_types(B, cond_type, seed)
            e4 = torch.full_like(types, 4)
            types_all = (torch.cat([types] * K + [e4]) if K else types if nrep == 1 else torch.cat([types, types, e4, e4]) if four_way
                         else torch.cat([types, e4])).contiguous()
        return labels_all, types_all

    @staticmethod
    def _guidance_rows(four_way: bool, unguided: bool = False) -> int:
        """nrep, the transformer rows per sample: [cond ; uncond] on the joint call, the four branches on the conditional call (four_way, which
        also says: control laid first, the given half teacher-forced, one cfg triple), one row without guidance (cfg=None)"""
        return 1 if unguided else 4 if four_way else 2

    def _check_unguided(self, four_way: bool, adapter=None, what: str = 'cfg=None'):
        """what generation without guidance rows does not offer, said on the host before any device work"""
        if self.sampler == 'torch':
            raise NotImplementedError(f"{what}: sampler='torch' is not offered (it reproduces the reference's generator calls, and the reference has no "
                                      "call without guidance rows); set model.sampler = 'counter'")
        if self.cfg.separate_decoding and not self.cfg.indep and not four_way:
            raise NotImplementedError(f'{what}: the two-pass separate_decoding branch (control_var.py:428-485) is not offered')
        if self.cfg.separator:
            raise NotImplementedError(f'{what}: separator models are not offered (their scale loop lays two guidance rows per sample)')
        if adapter is not None or getattr(self, '_adapter_bank', None) is not None:
            raise NotImplementedError(f'{what}: per-request adapters (adapter= / a model with an adapter bank) are not offered without guidance rows - '
                                      'the bank operands and slots are laid out for [cond ; uncond]; merge one adapter with add_lora, or detach the bank')

    @torch.no_grad()
    def _generate(self, B, label_B, g_seed, cfg_scale, top_k, top_p, more_smooth, cond_type, four_way, c_mask, c_img,
                  force_idx=None, trace: bool = False, gumbel=None, adapter=None, logprobs: bool = False, targets: Optional[dict] = None,
                  topn: Optional[int] = None):
        """-> f_hat, or (f_hat, TokenScores) with logprobs=True.  cfg_scale=None: generation without guidance rows (nrep == 1).
        targets (distill_targets=True): the dict _generate_core fills; the call then traces (last_trace holds the combined logits) - unless
        the dict says 'topn' (distill_topn=N): the sparse targets come from the score buffers, and nothing (B, L, V) is kept.
        topn (top_logprobs=N / distill_topn=N, with logprobs): the N most likely codes beside every score"""
        if cfg_scale is None:
            self._check_unguided(four_way, adapter)
        if targets is not None:
            self._check_distill_targets(four_way, more_smooth)
            trace = trace or 'topn' not in targets
        nrep = self._guidance_rows(four_way, cfg_scale is None)
        # adapter= and logprobs=True select the per-request path, as a per-row cfg does
        if adapter is not None or logprobs or _per_request(cfg_scale, top_k, top_p, g_seed, four_way):
            return self._generate_rows(B, label_B, g_seed, cfg_scale, top_k, top_p, more_smooth, cond_type, four_way, c_mask, c_img, force_idx, trace,
                                       adapter=adapter, logprobs=logprobs, targets=targets, topn=topn)
        if four_way and cfg_scale is not None:
            cfg_scale = tuple(cfg_scale)
        if top_k > self.cfg.vocab:                     # helpers.py:8-10: torch.topk raises on k > V; top_k <= 0 means no top-k filter
            raise RuntimeError(f'selected index k out of range (top_k={top_k} > vocabulary {self.cfg.vocab})')
        draws = None
        if self.sampler == 'torch':
            # the reference's generator calls, in its order (torch_draw_schedule); g_seed=None: the device's default generator, as rng=None upstream
            gen, gdev = None, self.device
            if g_seed is not None:
                gen = self.rng
                _check_generator_device(gen.device, self.device)
                gen.manual_seed(int(g_seed))
                gdev = gen.device
            draws = _TorchDraws(torch_draw_schedule(self.cfg, B, label_B_none=label_B is None, cond_type_none=cond_type is None, four_way=four_way,
                                                    more_smooth=bool(more_smooth)), gen, gdev, self.device, self.num_classes)
            if draws.next_kind() == 'labels':
                label_B = draws.take('labels', (B,))
            if draws.next_kind() == 'cond_type':
                cond_type = draws.take('cond_type', (B,))
            seed = int(g_seed) if g_seed is not None else 0          # the counter generator's key: unused by the race
        else:
            seed = int(g_seed) if g_seed is not None else int(torch.empty((), dtype=torch.int64).random_().item())
        self._pack(check=True); self.vae_proxy[0]._pack(check=True)
        for name, ids in (('c_mask', c_mask), ('c_img', c_img), ('_force_idx', force_idx)):
            if ids is not None:
                _check_index_range(torch.cat([t.reshape(-1) for t in ids]), 0, self.cfg.vocab - 1, name)
        labels_all, types_all = self._prepare_rows(B, label_B, cond_type, four_way, seed, nrep)
        mask_first = self._draw_order(four_way)
        if self.cfg.separator and (four_way or more_smooth or (self.cfg.separate_decoding and not self.cfg.indep)):
            raise NotImplementedError('separator: conditional_infer_cfg ignores the special tokens (control_var.py:270-330), the two-pass branch fails with a '
                                      'shape error (:481) and more_smooth slices the soft embeddings at shifted positions upstream; only forward(), training '
                                      'and the joint autoregressive_infer_cfg branch are built')
        how = _ScalarDraw(cfg_scale, top_k, top_p, seed, more_smooth=bool(more_smooth), gumbel=gumbel, draws=draws)
        if self.cfg.separate_decoding and not self.cfg.indep and not four_way:              # control_var.py:428-485
            f_hat = self._generate_two_pass(B, labels_all, types_all, how, force_idx, trace, mask_first)
        else:
            f_hat = self._generate_core(B, labels_all, types_all, four_way, how, c_mask, c_img, force_idx, trace, mask_first, nrep=nrep, targets=targets)
        if draws is not None:
            draws.finish()
        return f_hat

    def _draw_order(self, four_way: bool) -> bool:
        """mask_first of one call: is the control half laid first?"""
        if self.cfg.mask_factor != 2 or four_way:
            return True
        # control_var.py:403: python's global `random`, drawn on every call (before the `or`), exactly as upstream -
        # random.seed(k) before the call reproduces the reference's choice of order
        import random
        return True if (random.random() < 0.5 or not self.bidirectional) else False

    def _check_per_request(self, label_B, cond_type, four_way, more_smooth=False):
        """what per-request mode does not offer, said on the host before any device work"""
        self._check_per_request_mode(four_way, more_smooth)
        if label_B is None or (self.cfg.mask_factor == 2 and cond_type is None):
            raise ValueError('per-request sampling parameters: label_B' + (' and cond_type' if self.cfg.mask_factor == 2 else '') + ' must be given per row - '
                             'None draws them from the one batch seed of the scalar path, which a batch of requests does not have')

    def _check_per_request_mode(self, four_way, more_smooth=False):
        """... the part that does not depend on the request"""
        if more_smooth:
            raise NotImplementedError('per-request sampling parameters: more_smooth is not offered (the soft-embedding kernel has no per-row form); pass '
                                      'scalar cfg / top_k / top_p / g_seed, or more_smooth=False')
        if self.sampler == 'torch':
            raise NotImplementedError("per-request sampling parameters: sampler='torch' is not offered (its noise comes from ONE generator stream in "
                                      "batch order, so a row's draw depends on its slot); set model.sampler = 'counter'")
        if self.cfg.separate_decoding and not self.cfg.indep and not four_way:
            raise NotImplementedError('per-request sampling parameters: the two-pass separate_decoding branch (control_var.py:428-485) is not offered; '
                                      'pass scalar cfg / top_k / top_p / g_seed')

    @torch.no_grad()
    def _adapter_slots(self, adapter, B: int, nrep: int):
        """``adapter=`` -> the slot of every sequence (host int32, nrep * B), or None when it is not given; refuses on the host"""
        if adapter is None:
            return None
        if self.gemm_precision is not None:
            raise NotImplementedError(_no_bank_message(self.gemm_precision))
        from . import lora
        if not lora.has_adapters(self):
            raise RuntimeError('adapter=: no bank attached - call controlvar_amd.lora.attach_adapters(model, sources) first')
        return lora.sequence_slots(lora.adapter_ids(adapter, B, self._adapter_bank['n']), nrep)

    @torch.no_grad()
    def _generate_rows(self, B, label_B, g_seed, cfg_scale, top_k, top_p, more_smooth, cond_type, four_way, c_mask, c_img, force_idx=None, trace: bool = False,
                       adapter=None, logprobs: bool = False, targets: Optional[dict] = None, topn: Optional[int] = None):
        """per-request mode (an addition of this library): any of cfg / top_k / top_p / g_seed given per batch row.  Row b produces exactly
        what the scalar call produces at B = 1 with (label_b, cond_type_b, cfg_b, top_k_b, top_p_b, g_seed = seed_b): combined logits, kept-set
        size, margin, ids and image - bit for bit under deterministic_plan=True (the sampler always is; the plan makes the logits independent
        of the batch).  A bidirectional model still draws ONE (control, image) order per call from python's `random`, as the scalar path.
        logprobs=True: one score launch per scale behind the sampling launch and the teacher-forcing overwrites; returns (f_hat, TokenScores)."""
        self._check_per_request(label_B, cond_type, four_way, more_smooth)
        if logprobs:
            self._check_logprobs()
        nrep = self._guidance_rows(four_way, cfg_scale is None)
        slots = self._adapter_slots(adapter, B, nrep)
        table = _request_table(B, cfg_scale, top_k, top_p, g_seed, four_way, self.cfg.vocab, len(self.cfg.pyramid.patch_nums), slots=slots)
        f_hat, scores = self._run_rows(B, label_B, cond_type, four_way, table, c_mask=c_mask, c_img=c_img, force_idx=force_idx, trace=trace,
                                       logprobs=logprobs, sampled=self._sampled_pattern(four_way, c_mask, c_img, force_idx), nrep=nrep, targets=targets,
                                       topn=topn)
        return (f_hat, scores) if logprobs else f_hat

    def _row_state(self, B: int, table: _RequestTable, logprobs: bool, forced=None, sample: bool = True, coef_map=None, topn: Optional[int] = None):
        """the device state of one batch of requests -> (the table's device buffer, the _RowDraw over it).  The request table and the
        adapter slots are one upload; a graph builds this once and refreshes the buffer."""
        tab_dev = table.host.to(self.device)
        ad = None
        if table.n_seq:
            from . import lora
            ad = (lora.bank_pack(self), table.slot_view(tab_dev))
        return tab_dev, _RowDraw(table.views(tab_dev), forced, ad, _score_buffers(B, self.cfg.pyramid.L, self.device) if logprobs else None, sample, coef_map,
                                 _topn_buffers(B, self.cfg.pyramid.L, topn, self.device) if logprobs and topn else None)

    @torch.no_grad()
    def _run_rows(self, B, label_B, cond_type, four_way, table: _RequestTable, *, c_mask=None, c_img=None, force_idx=None, trace: bool = False,
                  logprobs: bool = False, sampled=None, mask_first: Optional[bool] = None, edit=None, score_halves=None, nrep: Optional[int] = None, targets: Optional[dict] = None,
                  region=None, topn: Optional[int] = None):
        """the per-request runner behind _generate_rows, edit_infer_cfg and score_infer_cfg: the validated table and the entry point's own extras
        -> (f_hat, TokenScores or None).  mask_first=None draws the (control, image) order (one per call, as the scalar path).
        edit: the host halves (src_ctrl, keep_ctrl, src_img, keep_img) of _edit_half - the forced-token table is built for the drawn order.
        score_halves: the flat ids of the halves in token order, checked by _flat_ids - teacher-forced along, scored, nothing sampled.
        region: the host (regions, strength, cfg) of _region_request - label_B is then (B, K), nrep = K + 1, and the weight table is built here."""
        self._pack(check=True); self.vae_proxy[0]._pack(check=True)
        for name, ids in (('c_mask', c_mask), ('c_img', c_img), ('_force_idx', force_idx)):
            if ids is not None:
                _check_index_range(torch.cat([t.reshape(-1) for t in ids]), 0, self.cfg.vocab - 1, name)
        K = 0 if region is None else int(region[0].shape[1])
        labels_all, types_all = self._prepare_rows(B, label_B, cond_type, four_way, 0, nrep, K=K)
        if mask_first is None:
            mask_first = self._draw_order(four_way)
        if self.cfg.separator and four_way:
            raise NotImplementedError('separator: conditional_infer_cfg ignores the special tokens (control_var.py:270-330); only forward(), training '
                                      'and the joint autoregressive_infer_cfg branch are built')
        dev, forced = self.device, None
        if edit is not None:
            forced = self._edit_table(B, *[None if t is None else t.to(device=dev, dtype=dt).contiguous()
                                           for t, dt in zip(edit, (torch.int32, torch.uint8, torch.int32, torch.uint8))], mask_first)
        if score_halves is not None:
            halves = [h.to(device=dev, dtype=torch.int32) for h in score_halves]
            force_idx, o = [], 0
            for pn in self.cfg.pyramid.patch_nums:
                ids = torch.cat([h[:, o:o + pn * pn] for h in halves], dim=1)
                force_idx.append((ids.repeat(4, 1) if four_way else ids).contiguous())
                o += pn * pn
        coef_map = None
        if region is not None:
            coef_map = self._region_table(B, K, *[None if t is None else torch.as_tensor(t).to(dev) for t in region], mask_first)
        _, how = self._row_state(B, table, logprobs or score_halves is not None, forced, sample=score_halves is None, coef_map=coef_map, topn=topn)
        f_hat = self._generate_core(B, labels_all, types_all, four_way, how, c_mask, c_img, force_idx, trace, mask_first, nrep=nrep, targets=targets)
        if trace and forced is not None:
            self.last_trace['forced'] = forced
        if trace and coef_map is not None:
            self.last_trace['coef'] = coef_map
        return f_hat, (self._token_scores(how.score, mask_first, sampled, forced, how.topn) if how.score is not None else None)

    def _check_logprobs(self):
        """what logprobs=True / score_infer_cfg do not offer beyond _check_per_request's list, said on the host before any device work"""
        if self.cfg.separator:
            raise NotImplementedError('token log-probabilities: separator models are not offered (their scales carry special tokens between the halves, '
                                      'which the (B, L) score layout does not hold)')

    def _token_scores(self, score, mask_first: bool, sampled=None, forced=None, topn=None) -> TokenScores:
        top = dict(zip(('top_ids', 'top_logprobs', 'tail_logprob'), topn)) if topn is not None else {}
        return TokenScores(*score, self.cfg.pyramid.patch_nums, self.cfg.mask_factor, mask_first, sampled=sampled, forced=forced, **top)

    def _sampled_pattern(self, four_way: bool, c_mask, c_img, force_idx) -> Optional[torch.Tensor]:
        """(L,) bool on the host: which tokens of a generation are sampled (None: all).  The four-branch path lays control first."""
        if force_idx is not None:
            return torch.zeros(self.cfg.pyramid.L, dtype=torch.bool)
        if not four_way or (c_mask is None and c_img is None):
            return None
        col, b = torch.ones(self.cfg.pyramid.L, dtype=torch.bool), 0
        for pn in self.cfg.pyramid.patch_nums:
            n = pn * pn
            if c_mask is not None:
                col[b:b + n] = False
            if c_img is not None:
                col[b + n:b + 2 * n] = False
            b += 2 * n
        return col

    def _check_distill_targets(self, four_way: bool, more_smooth=False):
        """what distill_targets=True does not offer, said on the host before any device work"""
        if more_smooth:
            raise NotImplementedError('distill_targets: more_smooth is not offered (the next scale is then fed soft embeddings, not the ids a student '
                                      'could be teacher-forced along)')
        if self.cfg.separator:
            raise NotImplementedError('distill_targets: separator models are not offered (their scales carry special tokens between the halves, which '
                                      'the (B, L) token layout does not hold)')
        if self.bidirectional:
            raise NotImplementedError('distill_targets: bidirectional models are not offered (they draw the order of the halves per call)')
        if self.cfg.separate_decoding and not self.cfg.indep and not four_way:
            raise NotImplementedError('distill_targets: the two-pass separate_decoding branch (control_var.py:428-485) is not offered')

    def _distill_targets(self, targets: dict, B: int, sampled, scores: Optional[TokenScores] = None):
        """the filled dict of _generate_core and the trace of the same call -> DistillTargets; with the dict's 'topn' (distill_topn=N) the
        top-N fields of the same call's scores -> SparseDistillTargets"""
        mf, pns, L = self.cfg.mask_factor, self.cfg.pyramid.patch_nums, self.cfg.pyramid.L
        ids, mask_first = targets['ids'], targets['mask_first']
        first = torch.cat([i[:, :pn * pn] for i, pn in zip(ids, pns)], dim=1).contiguous()
        second = torch.cat([i[:, pn * pn:] for i, pn in zip(ids, pns)], dim=1).contiguous() if mf == 2 else None
        ids_img, ids_ctrl = (first, None) if mf == 1 else (second, first) if mask_first else (first, second)
        col = torch.ones(L, dtype=torch.bool) if sampled is None else sampled
        col = col.to(self.device)[None].expand(B, -1).contiguous()
        if 'topn' in targets:
            return SparseDistillTargets(ids_img, ids_ctrl, scores.top_ids, scores.top_logprobs, scores.tail_logprob, col, mask_first)
        return DistillTargets(ids_img, ids_ctrl, torch.cat(self.last_trace['logits'], dim=1), col, mask_first)

    def _draw_scale(self, how, logits, B: int, nrep: int, l: int, si: int, ratio: float, ldv: int, cols, tr, force_idx):
        """draw the ids of one scale (sampling call si, at `ratio` of the way through the scales) from its logits, as `how` says (_ScalarDraw /
        _RowDraw) -> (idx (n_draw B, l) int32, the soft embeddings of more_smooth or None).  cols: this scale's columns of the (B, L) tables.
        tr: the trace to append to.  force_idx (tests, score_infer_cfg) replaces the drawn ids."""
        cfg, dev = self.cfg, logits.device
        mapped = isinstance(how, _RowDraw) and how.coef_map is not None  # regional guidance: nrep = K + 1 rows share ONE drawn id row
        n_draw = 4 if nrep == 4 and not mapped else 1
        idx = torch.empty(n_draw * B, l, device=dev, dtype=torch.int32)
        comb = torch.empty(B, l, cfg.vocab, device=dev, dtype=torch.float32) if tr is not None else None
        mg = torch.empty(B, l, device=dev, dtype=torch.float32) if tr is not None else None
        soft = None
        if isinstance(how, _RowDraw):
            seed, top_k, top_p, coef = how.rows                          # _request_table built the weights with the expressions below
            if not how.sample:
                pass                                                     # nothing is drawn: the ids are force_idx's, taken below
            elif mapped:
                ops.cfg_sample_map(logits, B, nrep, l, cfg.vocab, how.coef_map[:, cols], top_k, top_p, seed, si, n_draw, idx,
                                   None if how.forced is None else how.forced[:, cols], comb, mg, ldv=ldv)
                if tr is not None:                                       # the head's rows beside their combination (the tests of locality read both)
                    tr.setdefault('rows', []).append(logits.view(nrep * B, l, ldv)[:, :, :cfg.vocab].clone())
            elif how.forced is not None:
                ops.cfg_sample_edit(logits, B, nrep, l, cfg.vocab, coef[si], top_k, top_p, seed, si, n_draw, idx, how.forced[:, cols], comb, mg, ldv=ldv)
            else:
                ops.cfg_sample_rows(logits, B, nrep, l, cfg.vocab, coef[si], top_k, top_p, seed, si, n_draw, idx, comb, mg, ldv=ldv)
        else:
            if nrep == 4:
                t1, t2, t3 = [c * ratio for c in how.cfg]
                coef = [1 + t1, t2 - t1, t3 - t2, -t3]
            elif nrep == 2:
                t = how.cfg * ratio
                coef = [1 + t, -t]
            else:
                coef = [1.0]                                             # no guidance rows: the combined logits are the row's own
            expo, g_si = self._torch_noise(how.draws, n_draw * B, l, how.more_smooth)
            smooth = {}
            if how.more_smooth and how.top_k != 1:
                if how.gumbel is not None:
                    g_si = how.gumbel[si].to(device=dev, dtype=torch.float32).contiguous()      # greedy: the in-place masked softmax is one-hot, i.e. exactly E[idx] (control_var.py:511-515)
                soft = torch.empty(n_draw * B, l, cfg.cvae, device=dev, dtype=torch.float32)
                smooth = dict(codebook=self.vae_proxy[0]._pack()['E'], smooth_mul=1.0 + ratio, smooth_tau=max(0.27 * (1 - ratio * 0.95), 0.005),
                              gumbel=g_si, soft_out=soft)
            ops.cfg_sample(logits, B, nrep, l, cfg.vocab, coef, how.top_k, how.top_p, how.seed, si, n_draw, idx, comb, mg, seed_dev=how.seed_dev,
                           ldv=ldv, expo=expo, **smooth)
        if tr is not None:
            tr['idx'].append(idx.clone()); tr['margin'].append(mg); tr['logits'].append(comb)
        if force_idx is not None:
            idx = force_idx[si].to(device=dev, dtype=torch.int32).contiguous()
        return idx, soft

    @torch.no_grad()
    def _generate_core(self, B, labels_all, types_all, four_way, how, c_mask=None, c_img=None, force_idx=None, trace: bool = False,
                       mask_first: bool = True, nrep: Optional[int] = None, targets: Optional[dict] = None):
        """the 10-scale loop on device-resident inputs only (capturable in a HIP graph: no host sync, static shapes).
        how: a _ScalarDraw, or a _RowDraw (per-request mode) with what rides on it - the forced-token table, the adapters, the score buffers.
        nrep: the transformer rows per sample (_guidance_rows; None: 4 or 2 by four_way) - 1 runs R = B rows through every pass and the arena.
        targets (distill_targets): a dict that receives 'ids', per scale the ids the first branch continues with (B, l), after the overwrites,
        and 'mask_first', the order they are laid in."""
        row = isinstance(how, _RowDraw)
        if row and not how.sample and (how.score is None or force_idx is None or trace):
            raise ValueError('score_only: score buffers and force_idx are required')
        if row and how.forced is not None and (how.rows is None or four_way):
            raise ValueError('forced: the per-request joint path only (rows given, two branches)')
        if row and how.topn is not None and (how.score is None or how.coef_map is not None):
            raise ValueError('topn: beside the score launch of the per-request table only (score buffers given, no weight map)')
        ad, score = (how.ad, how.score) if row else (None, None)
        cfg, P = self.cfg, self._pack()
        vae: VQVAE = self.vae_proxy[0]
        py, mf, C = cfg.pyramid, cfg.mask_factor, cfg.C
        dev = self.device
        nrep = self._guidance_rows(four_way) if nrep is None else nrep
        R = nrep * B
        n_draw = nrep if four_way else 1                                 # the conditional call draws (and continues) every branch on its own ids
        nb = n_draw * B
        x = torch.empty(R * py.l[-1], C, device=dev, dtype=torch.float32)
        cond = torch.empty(R, C, device=dev, dtype=torch.float32)
        self._first_tokens(P, labels_all, types_all, x, cond, R, py.first_l, P['lvl_pos'], mask_first)
        gen_table = P['lvl_pos'] if four_way else (P['lvl_pos_gen'] if mask_first else P['lvl_pos_gen_'])
        ada = self._ada(cond, R, ad)
        arena = self._get_arena(R, py.L, self.kv_precision)
        S = py.patch_nums[-1]
        f_hat = torch.zeros(nb, mf, cfg.cvae, S, S, device=dev, dtype=torch.float32)
        tr = {'idx': [], 'margin': [], 'logits': []} if trace else None
        if targets is not None:
            targets.update(ids=[], mask_first=mask_first)
        nstage = len(py.patch_nums)
        # `indep` models hand the rows of the training mask to every inference pass (control_var.py:283,497); those rows hide something
        # only under separate_decoding (otherwise every cached key is visible anyway)
        inf_lvl, inf_holes = attention_levels(cfg) if (cfg.indep and cfg.separate_decoding) else (None, None)
        for si, pn in enumerate(py.patch_nums):
            l = py.l[si]
            ratio = si / (nstage - 1)
            logits = self._blocks_and_head(x[:R * l], ada, R, l, py.begin[si], py.L, arena, lvl_end=inf_lvl, holes=inf_holes, ad=ad)
            cols = slice(py.begin[si], py.end[si])
            idx, soft = self._draw_scale(how, logits, B, nrep, l, si, ratio, cfg.head_ld, cols, tr, force_idx)
            if four_way:                                                 # teacher forcing (control_var.py:309-324)
                nf = 3 if nrep == 4 else 1                               # the branches that see the given half: three of four, or the one there is
                if c_mask is not None:
                    idx[:nf * B, :pn * pn] = c_mask[si].to(device=dev, dtype=torch.int32).repeat(nf, 1)
                if c_img is not None:
                    idx[:nf * B, pn * pn:] = c_img[si].to(device=dev, dtype=torch.int32).repeat(nf, 1)
            if targets is not None:
                targets['ids'].append(idx[:B].clone())
            if score is not None and how.coef_map is not None:
                ops.score_map(logits, B, nrep, l, cfg.vocab, how.coef_map[:, cols], idx[:B], None, score[0][:, cols], score[1][:, cols], score[2][:, cols],
                              score[3][:, cols], ldv=cfg.head_ld)
            elif score is not None:
                ops.score_rows(logits, B, nrep, l, cfg.vocab, how.rows[3][si], idx[:B], None, score[0][:, cols], score[1][:, cols], score[2][:, cols],
                               score[3][:, cols], ldv=cfg.head_ld)
                if how.topn is not None:
                    ops.score_topn(logits, B, nrep, l, cfg.vocab, how.rows[3][si], int(how.topn[0].shape[2]), how.topn[0][:, cols], how.topn[1][:, cols],
                                   how.topn[2][:, cols], ldv=cfg.head_ld)
                if not how.sample and si == nstage - 1:
                    break
            if cfg.separator and py.sp(si):
                # control_var.py:507-509: the ids drawn at the separator positions are dropped from the THIRD scale on; at the second scale
                # upstream keeps all 10 ids and slices [:pn^2] / [-pn^2:], so the image half becomes ids 6..9 - replicated literally
                n = pn * pn
                idx = (torch.cat((idx[:, :n], idx[:, n + 1:2 * n + 1]), dim=1) if si > 1 else torch.cat((idx[:, :n], idx[:, -n:]), dim=1)).contiguous()
            tok = vae._next_input(si, idx, f_hat, nb, mf, True, soft=soft)
            if si != nstage - 1 and cfg.separator:
                # control_var.py:536-552: upstream stacks the two next-scale maps along H and splits the stack at row `pn` (the CURRENT
                # scale's size) before putting a separator behind each part: the first one lands behind pn * pn' tokens
                ln, pn2 = py.l[si + 1], py.patch_nums[si + 1]
                cut, nrep_x = pn * pn2, 2
                ops.word_embed(tok[:, :cut].contiguous(), P['w_we'], P['b_we'], gen_table, x, nb, nrep_x, cut, cfg.cvae, C, ln, 0, lvl_off=py.end[si])
                ops.word_embed(tok[:, cut:].contiguous(), P['w_we'], P['b_we'], gen_table, x, nb, nrep_x, 2 * pn2 * pn2 - cut, cfg.cvae, C, ln, cut + 1,
                               lvl_off=py.end[si] + cut + 1)
                mapping = cfg.special_mapping(mask_first)
                x[:R * ln].view(R, ln, C)[:, [cut, ln - 1]] = self._special_rows(gen_table, [py.end[si] + cut, py.end[si] + ln - 1], [mapping[2 * si], mapping[2 * si + 1]])
            elif si != nstage - 1:
                ln = py.l[si + 1]
                ops.word_embed(tok, P['w_we'], P['b_we'], gen_table, x, nb, nrep // n_draw, ln,
                               cfg.cvae, C, ln, 0, lvl_off=py.end[si])
        if trace:
            tr['f_hat'] = f_hat[:B].clone()
            self.last_trace = tr
        return f_hat[:B]

    @torch.no_grad()
    def _generate_two_pass(self, B, labels_all, types_all, how: _ScalarDraw, force_idx, trace, mask_first):
        """separate_decoding without indep (control_var.py:428-485): 2 x 10 passes over the same KV arena - per scale first the control
        tokens, then the image tokens, which see their scale's control tokens through the cache (attn_bias=None upstream).  The inputs
        cross over as upstream's do: the image pass of scale k is fed the CONTROL f_hat pooled to pn_k (:467-468), the control pass of
        scale k+1 the IMAGE f_hat pooled to pn_{k+1} (:470)."""
        cfg, P = self.cfg, self._pack()
        if cfg.type_pos:
            raise NotImplementedError('type_pos + separate_decoding: upstream indexes patch_nums[si + 1] with si up to 18 (control_var.py:483) and raises')
        vae: VQVAE = self.vae_proxy[0]
        py, C, dev = cfg.pyramid, cfg.C, self.device
        pns = py.patch_nums
        R = 2 * B
        xf = torch.empty(R * 2, C, device=dev, dtype=torch.float32)
        cond = torch.empty(R, C, device=dev, dtype=torch.float32)
        self._first_tokens(P, labels_all, types_all, xf, cond, R, 2, P['lvl_pos'], mask_first)
        ada = self._ada(cond, R)
        arena = self._get_arena(R, py.L, self.kv_precision)
        S = pns[-1]
        f = [torch.zeros(B, 1, cfg.cvae, S, S, device=dev, dtype=torch.float32) for _ in range(2)]
        x = torch.empty(R * S * S, C, device=dev, dtype=torch.float32)
        tr = {'idx': [], 'margin': [], 'logits': []} if trace else None
        nstage, pos = len(pns), 0
        for si in range(2 * nstage):
            half, k = si % 2, si // 2
            pn = pns[k]
            l = pn * pn
            ratio = k / (nstage - 1)
            if si < 2:
                x[:R].copy_(xf.view(R, 2, C)[:, si])
            logits = self._blocks_and_head(x[:R * l], ada, R, l, pos, py.L, arena)
            pos += l
            idx, soft = self._draw_scale(how, logits, B, 2, l, si, ratio, 0, None, tr, force_idx)
            if si == 2 * nstage - 1:
                vae._next_input(k, idx, f[1], B, 1, False, soft=soft)
                break
            tok = vae._next_input(k, idx, f[half], B, 1, True, soft=soft, pn_next=pn if half == 0 else None)
            ln = tok.shape[1]
            ops.word_embed(tok, P['w_we'], P['b_we'], P['lvl_pos'], x, B, 2, ln, cfg.cvae, C, ln, 0, lvl_off=pos)
        f_hat = torch.cat(f, dim=1)
        if trace:
            tr['f_hat'] = f_hat.clone()
            self.last_trace = tr
        return f_hat

    def _torch_noise(self, draws: Optional[_TorchDraws], rows: int, l: int, more_smooth: bool):
        """sampler='torch': (Exp(1) noise of the id draw, Gumbel noise of more_smooth) of one sampling call, drawn in that order as
        helpers.py:19 then :26 draw them (the Gumbel noise also at top_k == 1, where it is dropped); (None, None) otherwise"""
        if draws is None:
            return None, None
        expo = draws.take('expo', (rows * l, self.cfg.vocab))
        g = draws.take('gumbel', (rows, l, self.cfg.vocab)) if more_smooth else None
        return expo, g

    @torch.no_grad()
    def _capture(self, body):
        """Capture ``body()`` (launches on device-resident static buffers only) in a HIP graph: (graph, body's result, owned buffers).
        The warm-up runs on a side stream whose K/V arena and split-K workspace are dropped before the capture; the ones the capture
        creates are taken out of the per-stream tables and returned as `owned`, to live and die with the graph."""
        dev = self.device
        self._pack(); self.vae_proxy[0]._pack()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # warm-up off the capture (module loads, attribute setup, arena)
            body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self._arena:                                     # the warm-up's K/V arena (arenas are per stream): the capture allocates its own
            self._arena.pop(side.cuda_stream, None)         # in the graph's pool, and two of them do not fit at large batches
        ops.release_splitk_workspace(dev, side.cuda_stream)  # ... and the warm-up stream's split-K workspace
        torch.cuda.empty_cache()
        ws_before, arena_before = ops.splitk_workspace_keys(), set(self._arena or ())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = body()
        # buffers created during the capture live in the GRAPH's memory pool and are baked into its launches: they belong to the graph, not
        # to the per-stream tables - a later stream that is handed the capture stream's (pooled, reused) handle must not inherit them
        owned = [ops.take_splitk_workspace(k) for k in ops.splitk_workspace_keys() - ws_before]
        owned += [self._arena.pop(k) for k in set(self._arena or ()) - arena_before]
        return graph, out, owned

    @torch.no_grad()
    def _graph_runner(self, B, four_way, labels_all, types_all, cfg, top_k, top_p, finish, *, per_request: bool, adapters: bool = False,
                      logprobs: bool = False, forced=None, teach=None, refresh=None, prologue=None, sampled=None, check_rows: bool = True,
                      K: int = 0, coef_map=None, topn: Optional[int] = None):
        """The graphed generators: capture prologue() (inside the graph, before the scale loop), the scale loop and finish() over the static
        label / type rows, and return replay(label_B, cond_type, given, g_seed, request) -> images, with .graph and .owned.
        The sampling state lives in a device seed scalar (scalar graphs: cfg, top_k, top_p are baked in and replay refuses every request
        keyword) or, per_request=True, in the device buffer of a static _RequestTable (request holds cfg / top_k / top_p / adapter; those
        given here are validated as the defaults).  refresh(given) validates the given half / the edit request and returns the copy into its
        static buffers.  check_rows (scalar graphs): label_B / cond_type tensors must have shape (B,).
        adapters=True: the adapter launches are captured over the attached bank, the slot of every sequence rides in the same static table,
        and request['adapter'] chooses (None: every row on the base model)
        logprobs=True: the score launch of every scale is captured too, the (B, L) score buffers are static outputs of the graph, and replay
        returns (images, TokenScores) - copies, as the images are.  sampled: the (L,) host pattern of the sampled tokens (None: all); an edit
        graph (forced, the forced-token table) reads it off that table instead
        K > 0 with coef_map (regional guidance): label_B is (B, K), the rows are _prepare_rows' K-label layout and the scale loop reads its combine
        weights from the static (B, L, 4) table that prologue() fills inside the graph
        topn (top_logprobs=N, with logprobs): the top-N launch of every scale is captured beside the score launch, its (B, L, N) / (B, L) buffers are
        static outputs too, and the TokenScores replay returns carries copies of them"""
        dev, vocab, nstage = self.device, self.cfg.vocab, len(self.cfg.pyramid.patch_nums)
        unguided = cfg is None                               # captured without guidance rows: labels_all / types_all hold B rows, and so does every replay
        nrep = K + 1 if K else self._guidance_rows(four_way, unguided)
        if per_request:
            slots0 = self._adapter_slots(-1, B, nrep) if adapters else None
            table0 = _request_table(B, cfg, top_k, top_p, 0, four_way, vocab, nstage, slots=slots0)     # also validates the defaults
            state, how = self._row_state(B, table0, logprobs, forced, coef_map=coef_map, topn=topn)
        else:
            state = torch.zeros(1, device=dev, dtype=torch.int64)
            how = _ScalarDraw(cfg, top_k, top_p, 0, seed_dev=state)

        def body():
            if prologue is not None:
                prologue()
            return finish(self._generate_core(B, labels_all, types_all, four_way, how, nrep=nrep, **(teach or {})))

        graph, out, owned = self._capture(body)

        def check_shapes(label_B, cond_type):
            for name, v, want in (('label_B', label_B, (B, K) if K else (B,)), ('cond_type', cond_type, (B,))):
                if torch.is_tensor(v) and tuple(v.shape) != want:
                    raise ValueError(f'{name}: expected shape {want}, got {tuple(v.shape)}')

        def replay(label_B, cond_type, given, g_seed, request):
            # everything that can refuse runs before the first static buffer is written
            if per_request:
                self._check_per_request(label_B, cond_type, four_way)
                if (request['cfg'] is None) != unguided:
                    raise ValueError('run() got cfg=None: this graph was captured with guidance rows - capture it with cfg=None' if not unguided else
                                     f'run() got cfg={request["cfg"]!r}: this graph was captured with cfg=None and holds no guidance rows to weigh')
                adapter = request['adapter']
                if adapter is not None and not adapters:
                    raise TypeError('run() got adapter=: this graph was captured without adapters=True, so it holds none of the adapter launches - '
                                    'capture it with adapters=True to choose an adapter per call and per row')
                slots = self._adapter_slots(-1 if adapter is None else adapter, B, nrep) if adapters else None
                check_shapes(label_B, cond_type)
                table = _request_table(B, request['cfg'], request['top_k'], request['top_p'], g_seed, four_way, vocab, nstage, slots=slots)
                la, ta = self._prepare_rows(B, label_B, cond_type, four_way, 0, nrep, K=K)
                copy_given = refresh(given) if refresh is not None else None
            else:
                _refuse_request_keywords(g_seed, request)
                if check_rows:
                    check_shapes(label_B, cond_type)
                copy_given = refresh(given) if refresh is not None else None
                seed = int(g_seed) if g_seed is not None else int(torch.empty((), dtype=torch.int64).random_().item())
                la, ta = self._prepare_rows(B, label_B, cond_type, four_way, seed, nrep)
            labels_all.copy_(la)
            if types_all is not None:
                types_all.copy_(ta)
            if copy_given is not None:
                copy_given()
            if per_request:
                state.copy_(table.host)                     # seeds, top_k, top_p, every stage's weights and the adapter slots: one host-to-device copy
            else:
                state.fill_(seed & (2 ** 62 - 1))
            graph.replay()
            if logprobs:
                return out.clone(), self._token_scores([t.clone() for t in how.score], True, sampled=sampled,
                                                       forced=forced.clone() if forced is not None else None,
                                                       topn=[t.clone() for t in how.topn] if how.topn is not None else None)
            return out.clone()

        replay.graph = graph
        replay.owned = owned + ([how.ad[0]] if per_request and how.ad is not None else [])      # dropped together with the graph when the runner goes away
        return replay

    def _finisher(self, decode: str, generated: int):
        """decode='both': what _decode_pair returns; 'generated': only map `generated` of f_hat, one decoder pass of B images"""
        if decode == 'both':
            return self._decode_pair
        return lambda f_hat: self.vae_proxy[0]._decode(f_hat[:, generated].contiguous(), lo=-1.0, hi=1.0, mul=0.5, add=0.5)

    def _check_graph_logprobs(self, per_request: bool, logprobs: bool, four_way: bool, top_logprobs=None) -> Optional[int]:
        """logprobs=True / top_logprobs=N of the graphed generators: refused in words before anything is captured -> N or None"""
        n = _top_n('top_logprobs', top_logprobs, logprobs)
        if not logprobs:
            return None
        if not per_request:
            raise ValueError('logprobs=True needs per_request=True: the score launch reads the combine weights of the per-request table')
        self._check_logprobs()
        self._check_per_request_mode(four_way)
        return n

    def _check_graph_adapters(self, per_request: bool, adapters: bool):
        if not adapters:
            return
        if not per_request:
            raise ValueError('adapters=True needs per_request=True: the adapter slots travel with the per-request table')
        if self.gemm_precision is not None:
            raise NotImplementedError(_no_bank_message(self.gemm_precision))
        if getattr(self, '_adapter_bank', None) is None:
            raise RuntimeError('adapters=True: no bank attached - call controlvar_amd.lora.attach_adapters(model, sources) first')

    @torch.no_grad()
    def graphed_generator(self, B: int, cfg=1.5, top_k: int = 0, top_p: float = 0.0, per_request: bool = False, adapters: bool = False,
                          logprobs: bool = False, top_logprobs: Optional[int] = None):
        """Capture one full `autoregressive_infer_cfg` (10 scales x depth blocks + both VQVAE decodes, ~2.5k launches) in a
        HIP graph and return ``run(label_B, cond_type=None, g_seed=None) -> images``.  Labels, condition types and the
        sampling seed live in static device buffers that are refreshed before each replay, so every call draws new samples.
        Removes the host launch cost that dominates small batches (the reference's loop is host-launched op by op).
        per_request=True captures the per-row sampler instead: cfg, top_k, top_p and the seed of every row live in one static table that
        one copy refreshes, and ``run(label_B, cond_type, g_seed=None, cfg=..., top_k=..., top_p=...)`` takes each as a scalar or per row
        (those given here are its defaults) - one graph serves every mix of guidance scales, greedy beside sampled.  Row b of a replay is
        what autoregressive_infer_cfg(B, ...) gives in per-request mode; everything is validated on the host before a buffer is touched.
        adapters=True (with per_request=True, on a model with an adapter bank): run also takes adapter=, one id per row or one int.
        logprobs=True (with per_request=True): the graph holds the score launches and the (B, L) score buffers, and run returns
        (images, TokenScores) as autoregressive_infer_cfg(logprobs=True) does.  top_logprobs=N (with logprobs=True): the top-N launches and their
        static buffers join the graph, and the TokenScores carry top_ids / top_logprobs / tail_logprob."""
        four_way = False
        if cfg is None:                                     # cfg=None: the captured loop runs B rows, as autoregressive_infer_cfg(cfg=None); run takes cfg=None only
            self._check_unguided(four_way, True if adapters else None, 'graphed_generator(cfg=None)')
        self._check_graph_adapters(per_request, adapters)
        topn = self._check_graph_logprobs(per_request, logprobs, four_way, top_logprobs)
        if self.sampler == 'torch':
            raise NotImplementedError("graphed_generator captures the counter sampler only: sampler='torch' draws its noise with torch on model.rng "
                                      "between the launches; set model.sampler = 'counter' to capture, or call autoregressive_infer_cfg")
        if self.bidirectional:
            raise NotImplementedError('the captured generator fixes the (control, image) order; bidirectional models draw it per call')
        lab0 = torch.zeros(B, dtype=torch.int64)
        ty0 = torch.zeros(B, dtype=torch.int64) if self.cfg.mask_factor == 2 else None
        labels_all, types_all = self._prepare_rows(B, lab0, ty0, four_way, 0, self._guidance_rows(four_way, cfg is None))
        inner = self._graph_runner(B, four_way, labels_all, types_all, cfg, top_k, top_p, self._decode_pair, per_request=per_request, adapters=adapters,
                                   logprobs=logprobs, check_rows=False, topn=topn)
        if per_request:
            def run(label_B, cond_type=None, g_seed=None, cfg=cfg, top_k=top_k, top_p=top_p, adapter=None):
                return inner(label_B, cond_type, None, g_seed, dict(cfg=cfg, top_k=top_k, top_p=top_p, adapter=adapter))
        else:
            def run(label_B, cond_type=None, g_seed=None, **request):
                return inner(label_B, cond_type, None, g_seed, request)
        run.graph, run.owned = inner.graph, inner.owned
        return run

    @torch.no_grad()
    def graphed_conditional_generator(self, B: int, given: str = 'control', cfg=(1.5, 1.5, 1.5), top_k: int = 0, top_p: float = 0.0,
                                      source: str = 'ids', decode: str = 'both', per_request: bool = False, adapters: bool = False, logprobs: bool = False,
                                      top_logprobs: Optional[int] = None):
        """Capture one full `conditional_infer_cfg` in a HIP graph - control in, image out (given='control': the control ids are teacher-forced
        as `c_mask=`, the image is generated) or image in, control out (given='image', `c_img=`) - and return
        ``run(label_B, cond_type, given_half, g_seed=None) -> images``.
        source='ids': run is handed the given half's ids, the reference's list of (B, pn^2) integer tensors or one (B, sum pn^2) tensor, on the
        CPU or the device.  source='pixels': run is handed (B, 3, 16 S, 16 S) pixels in [-1, 1] and the graph also holds the tokeniser (the
        calls of `vae.img_to_idxBl`, in the VQVAE's compute_dtype / encoder_precision); ``run.ids()`` returns the ids it produced.
        decode='both': (B, 3, 2 H, H) exactly as conditional_infer_cfg (control on top, RGB below); decode='generated': only the generated map,
        (B, 3, H, H), one decoder pass of B images instead of 2 B.
        Labels, condition types (their 4 B-row forms), the seed, the given ids (int32 (B, sum pn^2)) and the pixels live in static device
        buffers refreshed before each replay.  more_smooth is not offered under capture; bidirectional models are captured as they are (the
        four-branch path never draws the order).
        per_request=True: as graphed_generator's - ``run(label_B, cond_type, given_half, g_seed=None, cfg=..., top_k=..., top_p=...)`` with each of
        g_seed / cfg / top_k / top_p a scalar (cfg: one triple) or per row (cfg: (B, 3)); those given here are the defaults of run.
        logprobs=True (with per_request=True): run returns (images, TokenScores) as conditional_infer_cfg(logprobs=True) does; top_logprobs=N
        as graphed_generator's."""
        if self.mask_factor != 2:
            raise NotImplementedError('graphed_conditional_generator needs mask_factor == 2 (control_var.py:333)')
        if cfg is None:                                     # cfg=None: the captured loop runs B rows, as conditional_infer_cfg(cfg=None)
            self._check_unguided(True, True if adapters else None, 'graphed_conditional_generator(cfg=None)')
        self._check_graph_adapters(per_request, adapters)
        topn = self._check_graph_logprobs(per_request, logprobs, True, top_logprobs)
        if self.sampler == 'torch':
            raise NotImplementedError("graphed_conditional_generator captures the counter sampler only: sampler='torch' draws its noise with torch on "
                                      "model.rng between the launches; set model.sampler = 'counter' to capture, or call conditional_infer_cfg")
        if self.cfg.separator:
            raise NotImplementedError('separator: conditional_infer_cfg ignores the special tokens (control_var.py:270-330); only forward(), training '
                                      'and the joint autoregressive_infer_cfg branch are built')
        for name, val, ok in (('given', given, ('control', 'image')), ('source', source, ('ids', 'pixels')), ('decode', decode, ('both', 'generated'))):
            if val not in ok:
                raise ValueError(f'{name}={val!r}: one of {" / ".join(ok)}')
        if int(B) != B or B < 1:
            raise ValueError(f'B={B!r}: a positive batch size')
        if not per_request:                                 # per_request: _request_table checks the defaults, which may come per row
            if cfg is not None:
                try:
                    cfg = tuple(float(c) for c in cfg)
                except TypeError:
                    cfg = ()
                if len(cfg) != 3:
                    raise ValueError('cfg: three guidance scales (t1, t2, t3) as in conditional_infer_cfg')
            if top_k > self.cfg.vocab:                      # as _generate (helpers.py:8-10)
                raise RuntimeError(f'selected index k out of range (top_k={top_k} > vocabulary {self.cfg.vocab})')
        dev = self.device
        vae: VQVAE = self.vae_proxy[0]
        pns = self.cfg.pyramid.patch_nums
        Ltot, side_px = sum(pn * pn for pn in pns), 16 * pns[-1]
        labels_all, types_all = self._prepare_rows(B, torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64), True, 0,
                                                   self._guidance_rows(True, cfg is None))
        ids_buf = torch.zeros(B, Ltot, device=dev, dtype=torch.int32)
        pix_buf = torch.zeros(B, 3, side_px, side_px, device=dev, dtype=torch.float32) if source == 'pixels' else None
        ids_Bl = vae._split(ids_buf)                        # per-scale views of the static buffer: what _generate_core teacher-forces from
        arg = 'c_mask' if given == 'control' else 'c_img'

        def tokenise():
            if pix_buf is not None:
                ids_buf.copy_(vae._ms_encode(vae._encode_f(pix_buf))[0])

        def refresh(given_half):
            """the given half as run() takes it, checked on the host -> the copy into the static pixel / id buffer"""
            if pix_buf is not None:
                checked = _pixels('given_half', given_half, pix_buf.shape)
            else:
                checked = _flat_ids('given_half', given_half, B, pns, self.cfg.vocab, arg)
            return lambda: (pix_buf if pix_buf is not None else ids_buf).copy_(checked)

        inner = self._graph_runner(B, True, labels_all, types_all, cfg, top_k, top_p, self._finisher(decode, 1 if given == 'control' else 0),
                                   per_request=per_request, adapters=adapters, logprobs=logprobs, teach={arg: ids_Bl}, refresh=refresh, prologue=tokenise,
                                   sampled=self._sampled_pattern(True, *((ids_Bl, None) if given == 'control' else (None, ids_Bl)), None), topn=topn)
        if per_request:
            def run(label_B, cond_type, given_half, g_seed=None, cfg=cfg, top_k=top_k, top_p=top_p, adapter=None):
                return inner(label_B, cond_type, given_half, g_seed, dict(cfg=cfg, top_k=top_k, top_p=top_p, adapter=adapter))
        else:
            def run(label_B, cond_type, given_half, g_seed=None, **request):
                return inner(label_B, cond_type, given_half, g_seed, request)
        run.graph, run.owned = inner.graph, inner.owned
        run.ids = lambda: ids_buf.clone()                   # the given half's ids of the last replay ('pixels': what the graph's tokeniser produced)
        return run

    # ---- region-constrained generation
    def _check_edit(self, label_B, cond_type, more_smooth=False):
        """what edit_infer_cfg / graphed_edit_generator do not offer, said on the host before any device work"""
        self._check_per_request(label_B, cond_type, False, more_smooth)
        if self.cfg.separator:
            raise NotImplementedError('region-constrained generation: separator models are not offered (their scales carry special tokens between '
                                      'the halves, which the forced-token table does not lay out)')

    def _edit_table(self, B, src_ctrl, keep_ctrl, src_img, keep_img, mask_first, forced=None):
        """device halves (flat int32 ids, uint8 masks; None where a half keeps nothing) -> forced (B, L) int32, one launch"""
        cfg = self.cfg
        if forced is None:
            forced = torch.empty(B, cfg.pyramid.L, device=self.device, dtype=torch.int32)
        return ops.edit_force_table(keep_ctrl, keep_img, src_ctrl if keep_ctrl is not None else None, src_img if keep_img is not None else None,
                                    cfg.pyramid.patch_nums, B, mask_first, cfg.mask_factor, forced)

    @torch.no_grad()
    def edit_infer_cfg(self, B: int, label_B, cond_type, *, src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, g_seed=None, cfg=1.5,
                       top_k=0, top_p=0.0, trace: bool = False, more_smooth: bool = False, adapter=None, logprobs: bool = False,
                       top_logprobs: Optional[int] = None):
        """Region-constrained generation (an addition of this library): keep the source's tokens where a mask says "keep", sample the others in
        their context - in-painting, out-painting, editing under a control map (keep_ctrl=True, the image partly kept), or a consistent joint
        edit (the same region of both halves free).  Returns what autoregressive_infer_cfg returns.
        src_img / src_ctrl: the half's multi-scale ids, the list of (B, pn^2) tensors vae.img_to_idxBl returns (or one (B, sum pn^2) tensor).
        keep_img / keep_ctrl: (B, S, S) bool at latent resolution (S = patch_nums[-1]), True = keep the source; the python value True keeps the
        whole half, None nothing.  A token of scale pn is kept iff a strict majority of the latent cells in its area-pooling bin is
        (edit_keep_cells); at the last scale that is the mask itself.  Kept tokens carry the source id of their scale and cell and feed the
        next scale like sampled ones; every other token is sampled exactly as the per-request joint path samples it, so with nothing kept
        the result is autoregressive_infer_cfg's in per-request mode, bit for bit.
        g_seed / cfg / top_k / top_p: a scalar or one value per row, as in per-request mode (a scalar seed gives identical requests
        identical results).  label_B and cond_type are given per row.  trace=True leaves last_trace as _trace does, 'idx' holding the ids
        AFTER forcing, plus last_trace['forced'], the table.  more_smooth, sampler='torch', the two-pass separate_decoding branch and
        separator models are refused.  adapter: one adapter id per row or one int, as in autoregressive_infer_cfg (lora.attach_adapters).
        logprobs=True: returns (images, TokenScores) as autoregressive_infer_cfg does; `sampled` is False at the kept tokens, which are scored too.
        top_logprobs=N (with logprobs=True): as autoregressive_infer_cfg's."""
        topn = _top_n('top_logprobs', top_logprobs, logprobs)
        self._check_edit(label_B, cond_type, more_smooth)
        if cfg is None:
            raise NotImplementedError(_NO_UNGUIDED.format('edit_infer_cfg'))
        pns = self.cfg.pyramid.patch_nums
        s_ctrl, k_ctrl = _edit_half('ctrl', src_ctrl, keep_ctrl, B, pns, self.cfg.vocab) if self.cfg.mask_factor == 2 else (None, None)
        s_img, k_img = _edit_half('img', src_img, keep_img, B, pns, self.cfg.vocab)
        table = _request_table(B, cfg, top_k, top_p, g_seed, False, self.cfg.vocab, len(pns), slots=self._adapter_slots(adapter, B, 2))
        f_hat, scores = self._run_rows(B, label_B, cond_type, False, table, trace=trace, logprobs=logprobs, edit=(s_ctrl, k_ctrl, s_img, k_img), topn=topn)
        return self._images(f_hat, scores)

    # ---- token log-probabilities of given tokens
    @torch.no_grad()
    def score_infer_cfg(self, B: int, label_B, cond_type, *, ids_img, ids_ctrl=None, given: Optional[str] = None, cfg=0.0, adapter=None,
                        mask_first: bool = True, top_logprobs: Optional[int] = None) -> TokenScores:
        """The likelihood of GIVEN tokens (an addition of this library): teacher-force the whole sample along its ids and score every token
        under the distribution a generation would have drawn it from.  No sampling launch and no decoder pass is issued: per scale the
        transformer, the head and one score launch (cvar_score_rows), the only consumer of the logits.  Returns a TokenScores whose `sampled`
        is all False; the log-probabilities are those of the UNFILTERED CFG-combined distribution.
        ids_img / ids_ctrl: each half's multi-scale ids, the list of (B, pn^2) tensors vae.img_to_idxBl returns (or one (B, sum pn^2) tensor).
        given=None: the joint two-branch path of autoregressive_infer_cfg; total() is log p(control, image | label, type).
        given='control' | 'image': the four-branch path of conditional_infer_cfg (mask_factor 2 only), cfg three numbers (or (B, 3)); all four
        branch rows carry the given tokens, and total(half=<the other half>) is log p(other | given).
        cfg = 0 scores under the conditional model alone; a per-row cfg scores under what a generation with that guidance draws from.
        label_B and cond_type are given per row; adapter as in autoregressive_infer_cfg.  A bidirectional model takes the (control, image)
        order as mask_first= here instead of drawing it.  Id range and shapes are checked on the host before any device work; more_smooth has
        no meaning here, and sampler='torch', the two-pass separate_decoding branch and separator models are refused.
        top_logprobs=N: the scores also carry the N most likely codes of every token's distribution (cvar_score_topn, one more launch per
        scale) - with a guidance scale in cfg, sparse_loss() of the result is a sparse guided teacher along these given tokens."""
        topn = _top_n('top_logprobs', top_logprobs)
        if given not in (None, 'control', 'image'):
            raise ValueError(f"given={given!r}: None (the joint path), 'control' or 'image'")
        four_way, mf = given is not None, self.cfg.mask_factor
        if cfg is None:
            raise NotImplementedError(_NO_UNGUIDED.format('score_infer_cfg'))
        if four_way and mf != 2:
            raise NotImplementedError("score_infer_cfg(given=...) needs mask_factor == 2, as conditional_infer_cfg (control_var.py:333)")
        self._check_per_request(label_B, cond_type, four_way)
        self._check_logprobs()
        if not mask_first and (four_way or not self.bidirectional):
            raise ValueError('mask_first=False: only a bidirectional model on the joint path (given=None) lays the image half first')
        pns, vocab = self.cfg.pyramid.patch_nums, self.cfg.vocab
        img = _flat_ids('ids_img', ids_img, B, pns, vocab)
        if mf == 2:
            if ids_ctrl is None:
                raise ValueError('ids_ctrl: the control half is scored too (given= says which half conditions the other) - pass its ids')
            ctrl = _flat_ids('ids_ctrl', ids_ctrl, B, pns, vocab)
        elif ids_ctrl is not None:
            raise ValueError('ids_ctrl: a plain VAR has the image half only')
        if four_way and _host_array(cfg).ndim == 0:
            cfg = (cfg,) * 3
        nrep = 4 if four_way else 2
        table = _request_table(B, cfg, 0, 0.0, 0, four_way, vocab, len(pns), slots=self._adapter_slots(adapter, B, nrep))
        halves = [img] if mf == 1 else ([ctrl, img] if mask_first else [img, ctrl])
        return self._run_rows(B, label_B, cond_type, four_way, table, sampled=torch.zeros(self.cfg.pyramid.L, dtype=torch.bool), mask_first=mask_first,
                              score_halves=halves, topn=topn)[1]

    @torch.no_grad()
    def graphed_edit_generator(self, B: int, source: str = 'ids', cfg=1.5, top_k=0, top_p=0.0, decode: str = 'both', adapters: bool = False,
                               logprobs: bool = False, top_logprobs: Optional[int] = None):
        """Capture one full `edit_infer_cfg` in a HIP graph and return
        ``run(label_B, cond_type, *, src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, g_seed=None, cfg=..., top_k=..., top_p=...) -> images``.
        The keep masks (uint8, all zero = nothing kept), the sources and the request table live in static device buffers refreshed before each
        replay; the graph holds the forced-token table's launch and the per-request scale loop with the forcing sampler.
        source='ids': the sources are ids as edit_infer_cfg takes them.  source='pixels': they are (B, 3, 16 S, 16 S) pixels in [-1, 1] and the
        graph also holds the tokeniser of both halves (the calls of `vae.img_to_idxBl`); ``run.ids()`` returns the (control, image) ids it produced.
        A half whose source is not given keeps the buffer of the previous replay and a mask of zeros.
        decode='both': what edit_infer_cfg returns; decode='generated': the image map only, (B, 3, H, H), one decoder pass of B images.
        cfg / top_k / top_p given here are the defaults of run; each and g_seed is a scalar or per row.  Everything is validated on the host
        before the first static buffer is written: a refused run leaves the graph as it was.  Bidirectional models are refused as
        graphed_generator refuses them.  logprobs=True: run returns (images, TokenScores) as edit_infer_cfg(logprobs=True) does; top_logprobs=N
        as graphed_generator's."""
        return self._graphed_edit('graphed_edit_generator', B, source, cfg, top_k, top_p, decode, adapters, logprobs,
                                  topn=_top_n('top_logprobs', top_logprobs, logprobs))

    @torch.no_grad()
    def _graphed_edit(self, what: str, B: int, source: str, cfg, top_k, top_p, decode: str, adapters: bool, logprobs: bool, K: int = 0,
                      topn: Optional[int] = None):
        """the capture behind graphed_edit_generator and, with K > 0 labels per sample, graphed_region_generator: the latter adds the static region
        maps, strength, guidance scales and the (B, L, 4) weight table, whose launch joins the forced-token table's in the prologue"""
        if cfg is None:
            raise NotImplementedError(_NO_UNGUIDED.format(what))
        if self.sampler == 'torch':
            raise NotImplementedError(f"{what} captures the counter sampler only: sampler='torch' draws its noise with torch on model.rng "
                                      "between the launches; set model.sampler = 'counter' to capture")
        if self.bidirectional:
            raise NotImplementedError('the captured generator fixes the (control, image) order; bidirectional models draw it per call')
        self._check_graph_adapters(True, adapters)
        for name, val, ok in (('source', source, ('ids', 'pixels')), ('decode', decode, ('both', 'generated'))):
            if val not in ok:
                raise ValueError(f'{name}={val!r}: one of {" / ".join(ok)}')
        if int(B) != B or B < 1:
            raise ValueError(f'B={B!r}: a positive batch size')
        mf = self.cfg.mask_factor
        lab0 = torch.zeros(B, dtype=torch.int64)
        if K:
            self._check_region(lab0, lab0)
        else:
            self._check_edit(lab0, lab0)
        dev = self.device
        vae: VQVAE = self.vae_proxy[0]
        pns = self.cfg.pyramid.patch_nums
        S, Lsrc, pixels = pns[-1], sum(pn * pn for pn in pns), source == 'pixels'
        labels_all, types_all = self._prepare_rows(B, torch.zeros(B, K, dtype=torch.int64) if K else lab0, lab0 if mf == 2 else None, False, 0, K=K)
        halves = ('ctrl', 'img') if mf == 2 else ('img',)
        keep_buf = {h: torch.zeros(B, S, S, device=dev, dtype=torch.uint8) for h in halves}
        ids_buf = {h: torch.zeros(B, Lsrc, device=dev, dtype=torch.int32) for h in halves}
        pix_buf = {h: torch.zeros(B, 3, 16 * S, 16 * S, device=dev, dtype=torch.float32) for h in halves} if pixels else None
        forced = torch.full((B, self.cfg.pyramid.L), -1, device=dev, dtype=torch.int32)
        # regional guidance: uniform maps, strength 1 (a mean of ones is exactly 1: the bits of strength=None) and cfg 0 until the first replay
        reg_buf = (torch.ones(B, K, S, S, device=dev), torch.ones(B, S, S, device=dev), torch.zeros(B, K, device=dev, dtype=torch.float64)) if K else None
        coef_map = torch.zeros(B, self.cfg.pyramid.L, 4, device=dev) if K else None

        def prologue():
            if pixels:
                for h in halves:                            # each half as its own batch of B: the calls of img_to_idxBl
                    ids_buf[h].copy_(vae._ms_encode(vae._encode_f(pix_buf[h]))[0])
            self._edit_table(B, ids_buf.get('ctrl'), keep_buf.get('ctrl'), ids_buf['img'], keep_buf['img'], True, forced)
            if K:
                self._region_table(B, K, *reg_buf, True, coef_map)

        def refresh(request):
            checked = {h: _edit_half(h, request.get('src_' + h), request.get('keep_' + h), B, pns, self.cfg.vocab, pixels) for h in halves}
            region = _region_request(B, request['labels'], request['regions'], request['cfg'], request['strength'], S, self.num_classes)[1:] if K else ()

            def copy():
                for buf, v in zip(reg_buf or (), region):
                    if v is None:
                        buf.fill_(1.0)
                    else:
                        buf.copy_(torch.as_tensor(v))
                for h, (src, mask) in checked.items():
                    if src is not None:
                        (pix_buf if pixels else ids_buf)[h].copy_(src)
                    if mask is None:
                        keep_buf[h].zero_()
                    else:
                        keep_buf[h].copy_(mask)
            return copy

        inner = self._graph_runner(B, False, labels_all, types_all, 0.0 if K else cfg, top_k, top_p, self._finisher(decode, mf - 1), per_request=True,
                                   adapters=adapters, logprobs=logprobs, forced=forced, refresh=refresh, prologue=prologue, K=K, coef_map=coef_map, topn=topn)

        if K:
            # the guidance scales travel with the maps (cfg_buf); the request table's own weights are not read, so its cfg is a constant 0
            def run(labels, cond_type=None, *, regions, cfg=cfg, strength=None, src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, g_seed=None,
                    top_k=top_k, top_p=top_p, adapter=None):
                if mf == 1 and (src_ctrl is not None or keep_ctrl is not None):
                    raise ValueError('src_ctrl / keep_ctrl: a plain VAR has the image half only')
                labels = torch.as_tensor(_host_array(labels))
                if labels.dim() != 2:
                    raise ValueError(f'labels: shape ({B}, {K}) expected, got {tuple(labels.shape)}')
                return inner(labels, cond_type if mf == 2 else None,
                             dict(src_img=src_img, keep_img=keep_img, src_ctrl=src_ctrl, keep_ctrl=keep_ctrl, labels=labels, regions=regions, cfg=cfg,
                                  strength=strength), g_seed, dict(cfg=0.0, top_k=top_k, top_p=top_p, adapter=adapter))
            run.coef = lambda: coef_map.clone()                              # the weight table of the last replay
        elif mf == 2:
            def run(label_B, cond_type, *, src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, g_seed=None, cfg=cfg, top_k=top_k, top_p=top_p,
                    adapter=None):
                return inner(label_B, cond_type, dict(src_img=src_img, keep_img=keep_img, src_ctrl=src_ctrl, keep_ctrl=keep_ctrl), g_seed,
                             dict(cfg=cfg, top_k=top_k, top_p=top_p, adapter=adapter))
        else:
            def run(label_B, cond_type=None, *, src_img=None, keep_img=None, g_seed=None, cfg=cfg, top_k=top_k, top_p=top_p, adapter=None):
                return inner(label_B, None, dict(src_img=src_img, keep_img=keep_img), g_seed, dict(cfg=cfg, top_k=top_k, top_p=top_p, adapter=adapter))
        run.graph, run.owned = inner.graph, inner.owned
        run.ids = lambda: tuple(ids_buf[h].clone() for h in halves)          # the sources of the last replay ('pixels': what the tokeniser produced)
        run.forced = lambda: forced.clone()                                  # ... and its forced-token table
        return run

    # ---- regional guidance
    def _check_region(self, label_B, cond_type, more_smooth=False, given=None, cfg=0.0):
        """what region_infer_cfg / graphed_region_generator do not offer, said on the host before any device work"""
        if cfg is None:
            raise NotImplementedError(_NO_UNGUIDED.format('region_infer_cfg'))
        if given is not None:
            raise NotImplementedError('regional guidance: the four-branch conditional call (given=) is not offered - its four weight slots hold the '
                                      'branches of conditional_infer_cfg, which leaves none for a second label; keep the given half with src_ctrl / keep_ctrl=True')
        if more_smooth:
            raise NotImplementedError('regional guidance: more_smooth is not offered (the soft-embedding kernel has no per-token form); pass more_smooth=False')
        if self.cfg.separator:
            raise NotImplementedError('regional guidance: separator models are not offered (their scales carry special tokens between the halves, '
                                      'which the per-token weight table does not lay out)')
        if self.cfg.separate_decoding:
            raise NotImplementedError('regional guidance: separate_decoding models are not offered (the two-pass branch (control_var.py:428-485) has no '
                                      'per-token sampler, and the K-label rows are not laid out for the training mask of indep)')
        self._check_per_request(label_B, cond_type, False, more_smooth)

    def _region_table(self, B, K, regions, strength, cfg, mask_first, coef=None):
        """device maps (fp32), strength (fp32 or None) and guidance scales (float64 (B, K)) -> coef (B, L, 4) fp32, one launch"""
        if coef is None:
            coef = torch.empty(B, self.cfg.pyramid.L, 4, device=self.device, dtype=torch.float32)
        return ops.region_coef_table(regions, strength, cfg, self.cfg.pyramid.patch_nums, B, K, mask_first, self.cfg.mask_factor, coef)

    @torch.no_grad()
    def region_infer_cfg(self, B: int, labels, cond_type, *, regions, cfg=1.5, strength=None, top_k=0, top_p=0.0, g_seed=None,
                         src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, adapter=None, logprobs: bool = False, trace: bool = False,
                         more_smooth: bool = False, given: Optional[str] = None, top_logprobs: Optional[int] = None):
        """Regional guidance (an addition of this library): several class labels per sample, each weighing the guidance where its
        latent-resolution map says so - "class A on the left, class B on the right", "class X inside this box", "guide harder in this region".
        Returns what autoregressive_infer_cfg returns.
        labels: (B, K) class labels, 1 <= K <= 3.  The sample runs K conditional transformer rows and one unconditional row (nrep = K + 1), all fed
        the one drawn id row; cond_type is the sample's on the conditional rows.
        regions: (B, K, S, S) non-negative weights at latent resolution (S = patch_nums[-1]), normalised per latent cell over the labels; every cell
        needs a positive weight somewhere.  cfg: a scalar, (B,) or (B, K) guidance scales.  strength: None or (B, S, S) >= 0, a factor on the
        guidance scale per latent cell.  A token's four combine weights are region_coef_reference's: its bin's mean normalised weight w_k times
        (1 + t_k) per label, -(sum_k w_k t_k) on the unconditional row, t_k = cfg_k strength ratio.  Both halves of a ControlVAR sample use the
        same maps.  With K = 1, uniform maps and no strength the call is autoregressive_infer_cfg in per-request mode, bit for bit.
        top_k / top_p / g_seed: a scalar or one value per row.  src_* / keep_*: edit_infer_cfg's - kept tokens carry the source ids, the others are
        sampled under the regional weights.  adapter, logprobs, trace: as edit_infer_cfg's; trace also leaves last_trace['coef'], the (B, L, 4)
        weight table, and last_trace['rows'], per scale the head's (nrep B, l, V) rows behind the combined logits.
        more_smooth, given= (the four-branch call), cfg=None, sampler='torch', separator and separate_decoding models are refused; what the
        maps do to image quality has not been judged (no published checkpoint is loaded here) - the contract is the weights above.
        top_logprobs is refused: a top-N form that reads the per-token weight map is not built."""
        if top_logprobs is not None:
            raise NotImplementedError(_NO_REGION_TOPN.format('region_infer_cfg'))
        self._check_region(labels, cond_type, more_smooth, given, cfg)
        if logprobs:
            self._check_logprobs()
        pns, mf = self.cfg.pyramid.patch_nums, self.cfg.mask_factor
        lab, reg, st, c = _region_request(B, labels, regions, cfg, strength, pns[-1], self.num_classes)
        K = int(lab.shape[1])
        edit = None
        if any(v is not None for v in (src_img, keep_img, src_ctrl, keep_ctrl)):
            s_ctrl, k_ctrl = _edit_half('ctrl', src_ctrl, keep_ctrl, B, pns, self.cfg.vocab) if mf == 2 else (None, None)
            edit = (s_ctrl, k_ctrl, *_edit_half('img', src_img, keep_img, B, pns, self.cfg.vocab))
        # the request table carries seeds, top_k, top_p and the adapter slots; its own combine weights are not read (cfg 0: a constant)
        table = _request_table(B, 0.0, top_k, top_p, g_seed, False, self.cfg.vocab, len(pns), slots=self._adapter_slots(adapter, B, K + 1))
        f_hat, scores = self._run_rows(B, lab, cond_type, False, table, trace=trace, logprobs=logprobs, edit=edit, nrep=K + 1, region=(reg, st, c))
        return self._images(f_hat, scores)

    @torch.no_grad()
    def graphed_region_generator(self, B: int, K: int, source: str = 'ids', top_k=0, top_p=0.0, decode: str = 'both', adapters: bool = False,
                                 logprobs: bool = False, top_logprobs: Optional[int] = None):
        """Capture one full `region_infer_cfg` with K labels per sample in a HIP graph and return
        ``run(labels, cond_type, *, regions, cfg=1.5, strength=None, src_img=None, keep_img=None, src_ctrl=None, keep_ctrl=None, g_seed=None, top_k=...,
        top_p=..., adapter=None) -> images``.  Labels, maps, strength, guidance scales, keep masks, sources and the request table live in static
        device buffers refreshed before each replay; the graph holds the launches of the weight table and of the forced-token table, so new maps
        need no recapture.  source / decode / adapters / logprobs: graphed_edit_generator's.  Everything is validated on the host before the first
        static buffer is written.  ``run.coef()`` returns the (B, L, 4) weight table of the last replay.  Bidirectional models are refused, and so
        is top_logprobs (region_infer_cfg)."""
        if top_logprobs is not None:
            raise NotImplementedError(_NO_REGION_TOPN.format('graphed_region_generator'))
        if int(K) != K or not 1 <= K <= REGION_MAX_LABELS:
            raise ValueError(f'K={K!r}: 1 to {REGION_MAX_LABELS} labels per sample')
        return self._graphed_edit('graphed_region_generator', B, source, 1.5, top_k, top_p, decode, adapters, logprobs, K=int(K))

    def _images(self, f_hat: torch.Tensor, scores: Optional[TokenScores] = None):
        """what the public generation calls return: the decoded images, or (images, scores) under logprobs=True"""
        return self._decode_pair(f_hat) if scores is None else (self._decode_pair(f_hat), scores)

    def _distill_request(self, logprobs: bool, top_logprobs, distill_targets: bool, distill_topn):
        """the scoring keywords of a generation call, checked on the host -> (the targets dict or None, score?, the launch's N or None)"""
        n, dn = _top_n('top_logprobs', top_logprobs, logprobs), _top_n('distill_topn', distill_topn)
        if dn is not None and distill_targets:
            raise ValueError('distill_targets=True and distill_topn=N: one form of targets per call - the dense logits or their N most likely codes')
        if dn is not None and n is not None and n != dn:
            raise ValueError(f'top_logprobs={n} and distill_topn={dn}: one top-N launch per scale serves both - pass the same N')
        tg = {'topn': dn} if dn is not None else ({} if distill_targets else None)
        return tg, bool(logprobs) or dn is not None, (n if n is not None else dn)

    def _results(self, B: int, out, logprobs: bool, targets: Optional[dict], sampled, top_logprobs=None):
        """_generate's result -> what the public call returns: images, (images, scores), and the DistillTargets / SparseDistillTargets behind
        them when asked for.  distill_topn=N scores the call whether logprobs is said or not; the scores are returned only when it is, and
        carry the alternatives only under top_logprobs"""
        sparse = targets is not None and 'topn' in targets
        scores = out[1] if logprobs or sparse else None
        t = self._distill_targets(targets, B, sampled, scores) if targets is not None else None
        if sparse and top_logprobs is None:
            scores = scores._without_alternatives()
        images = self._images(out[0], scores) if logprobs else self._images(out[0] if sparse else out)
        if t is None:
            return images
        return (*images, t) if logprobs else (images, t)

    def _decode_pair(self, f_hat: torch.Tensor) -> torch.Tensor:
        vae: VQVAE = self.vae_proxy[0]
        B, mf = f_hat.shape[:2]
        if mf == 1:
            return vae._decode(f_hat[:, 0].contiguous(), lo=-1.0, hi=1.0, mul=0.5, add=0.5)
        # control and image maps go through the decoder as ONE batch (b-major: [b][map]): at small B every decoder launch is a handful of workgroups
        # and latency-bound, so two passes of B images cost twice one pass of 2 B (B = 1: 78 conv + 234 GroupNorm launches -> 39 + 117).  Per-image
        # results do not depend on the batch they ride in (tests/test_gpu_parity.py::test_batch_rows_are_independent...), so the pixels are unchanged.
        img = vae._decode(f_hat.reshape(B * mf, *f_hat.shape[2:]), lo=-1.0, hi=1.0, mul=0.5, add=0.5)
        H, W = img.shape[-2:]
        return img.view(B, mf, 3, H, W).permute(0, 2, 1, 3, 4).reshape(B, 3, mf * H, W)          # control on top, RGB below (control_var.py:563-565)

    # ---- public API
    @torch.no_grad()
    def autoregressive_infer_cfg(self, B: int, label_B, g_seed: Optional[int] = None, cfg=1.5, top_k=0, top_p=0.0,
                                 more_smooth=False, cond_type=None, _force_idx=None, _trace=False, _gumbel=None, adapter=None, logprobs: bool = False,
                                 distill_targets: bool = False, top_logprobs: Optional[int] = None, distill_topn: Optional[int] = None):
        """control_var.py:356-565: returns (B, 3, 2 H, H) in [0,1] with H = 16 patch_nums[-1] - (B, 3, 512, 256) for the default list, (B, 3, 1024, 512) for
        PATCH_NUMS_512 (control image on top, RGB below).
        more_smooth: Gumbel-softmax soft code embeddings (:511-515); `_gumbel` (tests) injects the per-pass noise instead of drawing it.
        adapter (an addition of this library, lora.attach_adapters): one adapter id per row, or one int; -1 = the base model.  Selects the
        per-request path, as a per-row cfg does.
        logprobs=True (an addition of this library): returns (images, scores), scores a TokenScores - log-probability, entropy and rank of every
        token of the returned sample and the greedy id beside it, (B, L) each, from one more launch per scale (cvar_score_rows).  The
        log-probabilities are those of the UNFILTERED CFG-combined distribution: the top-k / top-p kept set is not renormalised over.  Selects the
        per-request path as adapter= does (scalars are broadcast), so its refusals apply; ids and images are bit-identical with and without it.
        cfg=None (an addition of this library): generation WITHOUT guidance rows, for a guidance-distilled student - one transformer
        row and one K/V arena row per sample instead of two; under deterministic_plan=True it returns the bits of cfg=0.0, which computes the
        unconditional rows and weighs them by zero.  sampler='torch', the two-pass separate_decoding branch, separator models and adapters
        are refused.
        distill_targets=True (likewise): the call traces and additionally returns a DistillTargets as its last value - the ids and the guided
        logits of the sample, in the forms Trainer.step_tokens(distill=...) takes.  more_smooth, separator and bidirectional models are refused.
        top_logprobs=N (with logprobs=True; 1 <= N <= 64): the scores also carry top_ids / top_logprobs (B, L, N), the N most likely codes of every
        token's distribution in rank order with the bits `logprob` would hold for them, and tail_logprob (B, L), the log of the mass of all the
        others - one more launch per scale (cvar_score_topn) beside the score launch; ids, images and the other fields are unchanged.
        distill_topn=N: additionally returns a SparseDistillTargets as the last value - DistillTargets with the guided distribution in that
        sparse form, never materialised as (B, L, V); it follows distill_targets' refusals.  One difference to distill_targets=True: it selects the
        per-request path as logprobs=True does, so label_B (and cond_type) must be given, and a scalar g_seed is broadcast as that path broadcasts
        it - every row draws under the key the scalar call builds at B = 1, so from B = 2 on the ids are those of distill_targets=True called with
        g_seed=[s] * B, not those of its scalar-seed call."""
        tg, score, topn = self._distill_request(logprobs, top_logprobs, distill_targets, distill_topn)
        out = self._generate(B, label_B, g_seed, cfg, top_k, top_p, more_smooth, cond_type, False, None, None, _force_idx, _trace, _gumbel, adapter=adapter,
                             logprobs=score, targets=tg, topn=topn)
        return self._results(B, out, logprobs, tg, self._sampled_pattern(False, None, None, _force_idx), top_logprobs)

    @torch.no_grad()
    def conditional_infer_cfg(self, B: int, label_B, g_seed: Optional[int] = None, cfg=(1.5, 1.5, 1.5), top_k=0, top_p=0.0,
                              more_smooth=False, cond_type=None, c_mask=None, c_img=None, _force_idx=None, _trace=False, _gumbel=None,
                              adapter=None, logprobs: bool = False, distill_targets: bool = False, top_logprobs: Optional[int] = None,
                              distill_topn: Optional[int] = None):
        """control_var.py:223-354: 4-branch CFG with teacher forcing of the control (c_mask) or image (c_img) ids.
        logprobs=True: returns (images, TokenScores) as autoregressive_infer_cfg does (the unfiltered combined distribution of the four branches;
        tokens in control-first order); `sampled` is False along the teacher-forced half, which is scored too.
        cfg=None: generation without guidance rows, as autoregressive_infer_cfg's - one row per sample instead of four, the given half
        teacher-forced into it; the bits of cfg=(0, 0, 0) under deterministic_plan=True.
        distill_targets=True: additionally returns a DistillTargets; its ids are those the first branch continued with (the given half where it
        was forced), and `sampled` is False along that half.
        top_logprobs=N, distill_topn=N: as autoregressive_infer_cfg's, under the combined distribution of the four branches."""
        if self.mask_factor != 2:
            raise NotImplementedError('conditional_infer_cfg needs mask_factor == 2 (control_var.py:333)')
        tg, score, topn = self._distill_request(logprobs, top_logprobs, distill_targets, distill_topn)
        out = self._generate(B, label_B, g_seed, cfg, top_k, top_p, more_smooth, cond_type, True, c_mask, c_img, _force_idx, _trace, _gumbel, adapter=adapter,
                             logprobs=score, targets=tg, topn=topn)
        return self._results(B, out, logprobs, tg, self._sampled_pattern(True, c_mask, c_img, _force_idx), top_logprobs)

    def forward(self, label_B: torch.LongTensor, x_BLCv_wo_first_l: torch.Tensor, cond_type=None, mask_first=True) -> torch.Tensor:
        """control_var.py:568-651 teacher-forced logits (B, L, V) fp32.  Under autograd (grad mode on and trainable
        parameters) the call is differentiable - `loss.backward()` runs the hand-written backward kernels
        (controlvar_amd/train.py); otherwise it is the inference-only fast path.  Label / cond-type dropout (rate ``cond_drop_rate``,
        torch.rand) is applied on EVERY call, in train and eval mode alike, exactly as the reference's forward does
        (control_var.py:578,584); DropPath follows ``self.training`` (helpers.py:39-46)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            from .train import teacher_forced_with_grad
            return teacher_forced_with_grad(self, label_B, x_BLCv_wo_first_l, cond_type, bool(mask_first))
        with torch.no_grad():
            return self._forward_nograd(label_B, x_BLCv_wo_first_l, cond_type, mask_first)

    def _forward_nograd(self, label_B, x_BLCv_wo_first_l, cond_type=None, mask_first=True):
        cfg, P = self.cfg, self._pack(check=True)
        py, C = cfg.pyramid, cfg.C
        dev = self.device
        mask_first = bool(mask_first) or cfg.mask_factor != 2
        B = x_BLCv_wo_first_l.shape[0]
        _check_index_range(label_B, 0, self.num_classes, 'label_B')
        labels = label_B.to(dev)
        if cfg.cond_drop_rate > 0:                  # control_var.py:578,584: applied on every forward(), train or eval mode
            labels = torch.where(torch.rand(B, device=dev) < cfg.cond_drop_rate, self.num_classes, labels)
        types = None
        if cfg.mask_factor == 2:
            _check_index_range(cond_type, 0, 4, 'cond_type')
            types = cond_type.to(dev)
            if cfg.cond_drop_rate > 0:
                types = torch.where(torch.rand(B, device=dev) < cfg.cond_drop_rate, 4, types)
            types = types.to(torch.int32).contiguous()
        labels = labels.to(torch.int32).contiguous()
        x = torch.empty(B * py.L, C, device=dev, dtype=torch.float32)
        cond = torch.empty(B, C, device=dev, dtype=torch.float32)
        table = P['lvl_pos_fwd'] if mask_first else P['lvl_pos_fwd_']
        self._first_tokens(P, labels, types, x, cond, B, py.L, table, mask_first)
        tok = x_BLCv_wo_first_l.to(device=dev, dtype=torch.float32).contiguous()
        if tok.shape[1] != len(py.code_positions()) - py.first_l:
            raise AssertionError(f'teacher-forcing input has {tok.shape[1]} tokens, expected {len(py.code_positions()) - py.first_l}')       # control_var.py:617
        self._embed_teacher_forced(P, tok, x, B, table, mask_first)
        ada = self._ada(cond, B, x3=False)              # forward() is the compute-dtype path in every gemm_precision
        arena = self._get_arena(B, py.L)
        lvl_end, holes = attention_levels(cfg)
        logits = self._blocks_and_head(x, ada, B, py.L, 0, py.L, arena, lvl_end=lvl_end, holes=holes, x3=False)
        return logits.view(B, py.L, cfg.head_ld)[:, :, :cfg.head_out]


class VAR(ControlVAR):
    """Plain class-conditional VAR (reference: models/var.py:20-291): mask_factor 1, L = 680."""
    _control = False

    def __init__(self, vae_local: VQVAE, num_classes=1000, norm_eps=1e-6, aln=1, aln_gamma_init=1e-3, shared_aln=False,
                 cond_drop_rate=0.1, depth=16, embed_dim=1024, num_heads=16, mlp_ratio=4., drop_rate=0., attn_drop_rate=0.,
                 drop_path_rate=0., layer_scale=-1., tau=4, cos_attn=False, patch_nums=DEFAULT_PATCH_NUMS,
                 flash_if_available=True, fused_if_available=True, compute_dtype=None, init_seed: int = 0, deterministic_plan: bool = False,
                 sampler: str = 'counter', gemm_precision: Optional[str] = None, kv_precision: Optional[str] = None):
        super().__init__(vae_local, num_classes=num_classes, norm_eps=norm_eps, aln=aln, aln_gamma_init=aln_gamma_init,
                         shared_aln=shared_aln, cond_drop_rate=cond_drop_rate, depth=depth, embed_dim=embed_dim, num_heads=num_heads,
                         mlp_ratio=mlp_ratio, drop_rate=drop_rate, attn_drop_rate=attn_drop_rate, drop_path_rate=drop_path_rate,
                         layer_scale=layer_scale, tau=tau, cos_attn=cos_attn, patch_nums=patch_nums,
                         flash_if_available=flash_if_available, fused_if_available=fused_if_available, mask_factor=1,
                         multi_cond=False, compute_dtype=compute_dtype, init_seed=init_seed, deterministic_plan=deterministic_plan,
                         sampler=sampler, gemm_precision=gemm_precision, kv_precision=kv_precision)

    @torch.no_grad()
    def autoregressive_infer_cfg(self, B: int, label_B, g_seed: Optional[int] = None, cfg=1.5, top_k=0, top_p=0.0,
                                 more_smooth=False, _force_idx=None, _trace=False, adapter=None, logprobs: bool = False, distill_targets: bool = False,
                                 top_logprobs: Optional[int] = None, distill_topn: Optional[int] = None):
        """var.py:143-207: returns (B, 3, H, H) in [0,1], H = 16 patch_nums[-1] (256, or 512 with PATCH_NUMS_512).
        logprobs=True: (images, TokenScores), as ControlVAR.autoregressive_infer_cfg; cfg=None, distill_targets=True, top_logprobs=N and
        distill_topn=N likewise."""
        tg, score, topn = self._distill_request(logprobs, top_logprobs, distill_targets, distill_topn)
        out = self._generate(B, label_B, g_seed, cfg, top_k, top_p, more_smooth, None, False, None, None, _force_idx, _trace, adapter=adapter, logprobs=score,
                             targets=tg, topn=topn)
        return self._results(B, out, logprobs, tg, self._sampled_pattern(False, None, None, _force_idx), top_logprobs)

    @torch.no_grad()
    def edit_infer_cfg(self, B: int, label_B, *, src_img=None, keep_img=None, g_seed=None, cfg=1.5, top_k=0, top_p=0.0, trace: bool = False,
                       more_smooth: bool = False, adapter=None, logprobs: bool = False, top_logprobs: Optional[int] = None):
        """ControlVAR.edit_infer_cfg for the one half a plain VAR has: returns (B, 3, H, H) as autoregressive_infer_cfg"""
        return super().edit_infer_cfg(B, label_B, None, src_img=src_img, keep_img=keep_img, g_seed=g_seed, cfg=cfg, top_k=top_k, top_p=top_p, trace=trace,
                                      more_smooth=more_smooth, adapter=adapter, logprobs=logprobs, top_logprobs=top_logprobs)

    @torch.no_grad()
    def region_infer_cfg(self, B: int, labels, *, regions, cfg=1.5, strength=None, top_k=0, top_p=0.0, g_seed=None, src_img=None, keep_img=None,
                         adapter=None, logprobs: bool = False, trace: bool = False, more_smooth: bool = False, top_logprobs: Optional[int] = None):
        """ControlVAR.region_infer_cfg for the one half a plain VAR has: returns (B, 3, H, H) as autoregressive_infer_cfg"""
        return super().region_infer_cfg(B, labels, None, regions=regions, cfg=cfg, strength=strength, top_k=top_k, top_p=top_p, g_seed=g_seed,
                                        src_img=src_img, keep_img=keep_img, adapter=adapter, logprobs=logprobs, trace=trace, more_smooth=more_smooth,
                                        top_logprobs=top_logprobs)

    @torch.no_grad()
    def score_infer_cfg(self, B: int, label_B, *, ids_img, cfg=0.0, adapter=None, top_logprobs: Optional[int] = None) -> 'TokenScores':
        """ControlVAR.score_infer_cfg for the one half a plain VAR has"""
        return super().score_infer_cfg(B, label_B, None, ids_img=ids_img, cfg=cfg, adapter=adapter, top_logprobs=top_logprobs)

    def conditional_infer_cfg(self, *a, **k):
        raise NotImplementedError('plain VAR has no conditional_infer_cfg (var.py)')

    def graphed_conditional_generator(self, *a, **k):
        raise NotImplementedError('plain VAR has no conditional_infer_cfg (var.py)')

    def forward(self, label_B, x_BLCv_wo_first_l, cond_type=None, mask_first=True):
        return super().forward(label_B, x_BLCv_wo_first_l, None, True)


# =====================================================================================
# factories (models/__init__.py:6-45)
# =====================================================================================
def build_vae(vocab_size=4096, z_channels=32, ch=160, share_quant_resi=4, v_patch_nums=DEFAULT_PATCH_NUMS, test_mode=True, **kw) -> VQVAE:
    """The VQVAE every script builds (train_control_var_hpu.py:581-582)."""
    return VQVAE(vocab_size=vocab_size, z_channels=z_channels, ch=ch, test_mode=test_mode, share_quant_resi=share_quant_resi,
                 v_patch_nums=v_patch_nums, **kw)


def build_var(vae: VQVAE, depth: int, patch_nums=DEFAULT_PATCH_NUMS, aln=1, aln_gamma_init=1e-3, shared_aln=False, layer_scale=-1,
              tau=4, cos_attn=False, flash_if_available=True, fused_if_available=True, **kw) -> VAR:
    return VAR(vae_local=vae, patch_nums=patch_nums, depth=depth, embed_dim=depth * 64, num_heads=depth, drop_path_rate=0.1 * depth / 24,
               aln=aln, aln_gamma_init=aln_gamma_init, shared_aln=shared_aln, layer_scale=layer_scale, tau=tau, cos_attn=cos_attn,
               flash_if_available=flash_if_available, fused_if_available=fused_if_available, **kw)


def build_control_var(vae: VQVAE, depth: int, patch_nums=DEFAULT_PATCH_NUMS, aln=1, aln_gamma_init=1e-3, shared_aln=False, layer_scale=-1,
                      tau=4, cos_attn=False, flash_if_available=True, fused_if_available=True, mask_type='replace', cond_drop_rate=0.1,
                      bidirectional=False, separate_decoding=False, separator=False, type_pos=False, indep=False, multi_cond=False,
                      **kw) -> ControlVAR:
    if mask_type == 'replace':
        mask_factor = 1
    elif mask_type == 'interleave_append':
        mask_factor = 2
    else:
        raise NotImplementedError
    return ControlVAR(vae_local=vae, patch_nums=patch_nums, depth=depth, embed_dim=depth * 64, num_heads=depth,
                      drop_path_rate=0.1 * depth / 24, aln=aln, aln_gamma_init=aln_gamma_init, shared_aln=shared_aln,
                      layer_scale=layer_scale, tau=tau, cos_attn=cos_attn, cond_drop_rate=cond_drop_rate,
                      flash_if_available=flash_if_available, fused_if_available=fused_if_available, mask_factor=mask_factor,
                      bidirectional=bidirectional, separate_decoding=separate_decoding, separator=separator, type_pos=type_pos,
                      indep=indep, multi_cond=multi_cond, **kw)
