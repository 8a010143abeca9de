"""Tensor-facing wrappers over the C ABI (include/cvar.h).

torch is plumbing here: it owns device memory and the stream; every computation is a call
into libcvar_hip.so with raw pointers.  All functions are asynchronous on the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import ACT_GELU_TANH, ACT_NONE, CVAR_BF16, CVAR_F32, GemmDesc, check

_DT = {torch.float32: CVAR_F32, torch.bfloat16: CVAR_BF16}

# bench.py sets this to a list to collect (start_event, end_event, algorithmic_flops, shape tag) per GEMM launch
GEMM_PROFILE = None


def dt(t_or_dtype) -> int:
    d = t_or_dtype.dtype if isinstance(t_or_dtype, torch.Tensor) else t_or_dtype
    try:
        return _DT[d]
    except KeyError:
        raise TypeError(f'unsupported dtype {d}') from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.CvarError('controlvar_amd ops need device tensors (no CPU fallback)')
    return t.data_ptr()


_SPLITK_WS = {}
# per-call execution options of cvar_gemm (include/cvar.h): A/B measurement knobs, never needed for correctness
GEMM_TILE_CFG = 0          # 0 automatic, 1 128x128 only, 2 8-wave 256x256, 3 4-wave 256x256
GEMM_STAGGER = 0           # start-stagger window in shader cycles (0 = the library's default: off)
GEMM_GROUP_M = 0           # row tiles per scheduling group (0 = automatic)
SMALL_M_KERNEL = True      # False: small_m calls stay on the LDS-tiled kernels + split-K (A/B runs)


def ensure_splitk_workspace(device, nbytes: int = 256 << 20) -> torch.Tensor:
    """The split-K workspace ops.gemm hands to every cvar_gemm call on `device` issued from the current stream.  Caller-owned
    memory (the library keeps no state); one buffer per (device, stream), created on first use, so that GEMMs on different
    streams never share partial-sum storage and the split-K decision - hence the summation order - is the same on every stream
    (eager, side-stream warm-up, graph capture)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _SPLITK_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _SPLITK_WS[key] = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    return ws


def splitk_workspace_keys() -> set:
    """(device index, stream handle) keys of the live split-K workspaces"""
    return set(_SPLITK_WS)


def take_splitk_workspace(key) -> Optional[torch.Tensor]:
    """remove one workspace from the per-stream table and hand it to the caller (models.graphed_generator: a workspace allocated during a
    graph capture belongs to that graph)"""
    return _SPLITK_WS.pop(key, None)


def release_splitk_workspace(device=None, stream_handle: Optional[int] = None):
    """Drop split-K workspaces (256 MB each) so the caching allocator can reuse the memory: the one of (device, stream_handle), or - with
    stream_handle None - every workspace of the device except the current stream's.  Streams come from a pool and their handles are
    reused; call this when a side stream is retired."""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if stream_handle is not None:
        _SPLITK_WS.pop((idx, stream_handle), None)
        return
    cur = torch.cuda.current_stream(dev).cuda_stream
    for k in [k for k in _SPLITK_WS if k[0] == idx and k[1] != cur]:
        del _SPLITK_WS[k]


def gemm(A: torch.Tensor, W: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int, lda: int = 0, ldw: int = 0, ldc: int = 0,
         bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, alpha: float = 1.0,
         gate: Optional[torch.Tensor] = None, ldg: int = 0, gate_rows: int = 1, gate_off: int = 0,
         residual: Optional[torch.Tensor] = None, ldr: int = 0,
         remap: Optional[Sequence[int]] = None, batch: int = 1, strideA: int = 0, strideW: int = 0, strideC: int = 0, strideR: int = 0,
         conv: Optional[dict] = None, a_off: int = 0, w_off: int = 0, c_off: int = 0,
         pre_act: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None, gate_scale: Optional[torch.Tensor] = None,
         split: Optional[tuple] = None, split_alpha: float = 1.0, ln: Optional[tuple] = None, small_m: bool = False, split_k: bool = True,
         gn_part: Optional[torch.Tensor] = None):
    """C = epilogue(A @ W^T).  Offsets (*_off) are in elements of the respective tensor.
    gn_part (fp32 [B][tiles][N][3], conv only): GroupNorm partials of the output from the conv's epilogue (cvar_gemm_desc.gn_part, ABI 18; ask
    conv_gn_partials() whether the call can emit them - it fails loudly otherwise).
    ln = (out, ada, scale_off, shift_off, ld_ada, rows_per, eps): also write cast(LN(C[m]) * (1 + scale) + shift) of the finished rows to ``out`` -
    the ln_modulate of the op that follows (cvar_gemm_desc.ln_out, ABI 17; fused into the split-K reduction of small-M calls).
    split = (tensor, split_n, ld_split): result columns [0, split_n) go to ``tensor`` (rows not remapped), the rest to ``out`` at
    column n - split_n (cvar_gemm_desc.C_split; the qkv GEMM of inference: q beside a [R][Lmax][2C] K/V arena)."""
    d = GemmDesc()
    d.M, d.N, d.K, d.dtype = M, N, K, dt(A)
    if W.dtype != A.dtype:
        raise TypeError('A and W must share a dtype')
    d.A = _ptr(A) + a_off * A.element_size()
    d.W = _ptr(W) + w_off * W.element_size()
    d.lda, d.ldw = lda or K, ldw or K
    d.batch, d.strideA, d.strideW, d.strideC, d.strideR = batch, strideA, strideW, strideC, strideR
    if conv:
        d.conv = 1
        d.Hin, d.Win, d.Cin, d.Hout, d.Wout = conv['Hin'], conv['Win'], conv['Cin'], conv['Hout'], conv['Wout']
        d.stride, d.up = conv.get('stride', 1), conv.get('up', 0)
    d.alpha = alpha
    d.bias = _ptr(bias)
    d.act = act
    if gate is not None:
        d.gate = _ptr(gate) + gate_off * 4
        d.ldg, d.gate_rows = ldg, gate_rows
    if residual is not None:
        d.residual, d.res_dtype, d.ldr = _ptr(residual), dt(residual), ldr or N
    d.C = _ptr(out) + c_off * out.element_size()
    d.out_dtype, d.ldc = dt(out), ldc or N
    if remap is not None:
        d.remap_l, d.remap_L, d.remap_off = remap
    d.pre_act, d.aux, d.gate_scale = _ptr(pre_act), _ptr(aux), _ptr(gate_scale)
    if split is not None:
        st, d.split_n, d.ld_split = split
        if st.dtype != out.dtype:
            raise TypeError('split target and out must share a dtype')
        d.C_split = _ptr(st)
        d.split_alpha = float(split_alpha)
    if ln is not None:
        lo, ada, sc_off, sh_off, ld_ada, rows_per, eps = ln
        d.ln_out, d.ln_out_dtype = _ptr(lo), dt(lo)
        d.ln_scale, d.ln_shift = _ptr(ada) + 4 * sc_off, _ptr(ada) + 4 * sh_off
        d.ld_ln, d.ln_rows, d.ln_eps = ld_ada, rows_per, eps
    d.gn_part = _ptr(gn_part)
    ws = _SPLITK_WS.get((A.device.index, _stream()))
    if ws is None:
        ws = ensure_splitk_workspace(A.device)
    if split_k:
        d.ws, d.ws_bytes = ws.data_ptr(), ws.numel()
    d.tile_cfg, d.stagger, d.group_m = (12 if (small_m and GEMM_TILE_CFG == 0 and SMALL_M_KERNEL) else GEMM_TILE_CFG), GEMM_STAGGER, GEMM_GROUP_M
    if GEMM_PROFILE is None:
        check(_lib.load().cvar_gemm(C.byref(d), _stream()), 'cvar_gemm')
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_lib.load().cvar_gemm(C.byref(d), _stream()), 'cvar_gemm')
        e1.record()
        tag = ('conv' if conv else 'gemm', M, N, K, batch, 'gate' if gate is not None else ('res' if residual is not None else ('act' if act else ('remap' if remap is not None else 'plain'))), str(out.dtype)[6:])
        GEMM_PROFILE.append((e0, e1, 2.0 * M * N * K * batch, tag))
    return out


def gemm_tn(A: torch.Tensor, B: torch.Tensor, out: torch.Tensor, *, T: int, Nn: int, Kk: int, lda: int = 0, ldb: int = 0, ldc: int = 0, c_off: int = 0,
            colsum: Optional[torch.Tensor] = None, colsum_off: int = 0, accumulate: bool = False, use_ws: bool = True):
    """out[n, k] (fp32) = sum_t A[t, n] * B[t, k] - the weight gradient dW = dY^T X on token-major bf16 operands (cvar_gemm_tn).
    colsum (fp32, optional): colsum[colsum_off + n] = sum_t A[t, n] - the bias gradient - from the same pass.
    accumulate: out and colsum become fp32(old + plain) (cvar_gemm_tn_acc, include/cvar_accum.h); use_ws=False: no workspace, hence one token slice"""
    ws = _SPLITK_WS.get((A.device.index, _stream()))
    if ws is None:
        ws = ensure_splitk_workspace(A.device)
    cs = (_ptr(colsum) + 4 * colsum_off) if colsum is not None else None
    wp, wn = (ws.data_ptr(), ws.numel()) if use_ws else (None, 0)
    if accumulate:
        check(_lib.load().cvar_gemm_tn_acc(_ptr(A), lda or Nn, _ptr(B), ldb or Kk, _ptr(out) + 4 * c_off, ldc or Kk, T, Nn, Kk, wp, wn, cs, 1, _stream()),
              'cvar_gemm_tn_acc')
        return out
    check(_lib.load().cvar_gemm_tn(_ptr(A), lda or Nn, _ptr(B), ldb or Kk, _ptr(out) + 4 * c_off, ldc or Kk, T, Nn, Kk, wp, wn, cs, _stream()),
          'cvar_gemm_tn')
    return out


def ln_modulate(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                out: torch.Tensor, M: int, Cdim: int, eps: float):
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                       _ptr(out), dt(out), M, Cdim, eps, _stream()), 'cvar_ln_modulate')
    return out


def ln_modulate_split3(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                       out: torch.Tensor, M: int, Cdim: int, eps: float):
    """ln_modulate with the split store: bf16 out[M][3 C] = [hi | lo | hi] of the fp32 adaLN row, bit for bit split3(ln_modulate(fp32 out))
    (cvar_ln_modulate_split3, include/cvar_serve.h)"""
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate_split3(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                              _ptr(out), M, Cdim, eps, _stream()), 'cvar_ln_modulate_split3')
    return out


def fp8_ldq(K: int) -> int:
    """row stride in bytes of an e4m3 operand of K columns: K rounded up to the 128-byte K tile"""
    return (K + 127) // 128 * 128


def quant_rows_fp8(x: torch.Tensor, q: torch.Tensor, scale: torch.Tensor, *, M: int, K: int, ldx: int = 0, ldq: int = 0,
                   x_off: int = 0, q_off: int = 0, s_off: int = 0):
    """rows of x (bf16 / fp32) -> e4m3 bytes q[M][ldq] + one power-of-two fp32 scale per row (cvar_quant_rows_fp8, include/cvar_serve.h).
    x_off in elements of x, q_off in bytes, s_off in scales."""
    if q.dtype != torch.uint8 or scale.dtype != torch.float32:
        raise TypeError('q is uint8 (e4m3 bytes), scale is float32')
    check(_lib.load().cvar_quant_rows_fp8(_ptr(x) + x_off * x.element_size(), dt(x), ldx or K, M, K, _ptr(q) + q_off, ldq or fp8_ldq(K),
                                          _ptr(scale) + 4 * s_off, _stream()), 'cvar_quant_rows_fp8')
    return q, scale


def ln_modulate_fp8(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                    q: torch.Tensor, q_scale: torch.Tensor, M: int, Cdim: int, eps: float, ldq: int = 0):
    """ln_modulate with the e4m3 store: bit for bit quant_rows_fp8(ln_modulate(bf16 out)) (cvar_ln_modulate_fp8, include/cvar_serve.h)"""
    if q.dtype != torch.uint8 or q_scale.dtype != torch.float32:
        raise TypeError('q is uint8 (e4m3 bytes), q_scale is float32')
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate_fp8(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                           _ptr(q), ldq or fp8_ldq(Cdim), _ptr(q_scale), M, Cdim, eps, _stream()), 'cvar_ln_modulate_fp8')
    return q, q_scale


def ln_modulate_wide(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                     out: torch.Tensor, M: int, Cdim: int, eps: float):
    """ln_modulate for any C <= CVAR_WIDE_CMAX (cvar_ln_modulate_wide, include/cvar_wide.h): up to 2048 channels the kernels ln_modulate launches.
    The models call this form, and the two below, where embed_dim > 2048; ln_modulate itself keeps cvar_ln_modulate's contract and refusals."""
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate_wide(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                            _ptr(out), dt(out), M, Cdim, eps, _stream()), 'cvar_ln_modulate_wide')
    return out


def ln_modulate_split3_wide(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                            out: torch.Tensor, M: int, Cdim: int, eps: float):
    """ln_modulate_split3 for any C <= CVAR_WIDE_CMAX (cvar_ln_modulate_split3_wide, include/cvar_wide.h)"""
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate_split3_wide(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                                   _ptr(out), M, Cdim, eps, _stream()), 'cvar_ln_modulate_split3_wide')
    return out


def ln_modulate_fp8_wide(x: torch.Tensor, ada: torch.Tensor, scale_off: int, shift_off: int, ld_ada: int, rows_per: int,
                         q: torch.Tensor, q_scale: torch.Tensor, M: int, Cdim: int, eps: float, ldq: int = 0):
    """ln_modulate_fp8 for any C <= CVAR_WIDE_CMAX (cvar_ln_modulate_fp8_wide, include/cvar_wide.h)"""
    if q.dtype != torch.uint8 or q_scale.dtype != torch.float32:
        raise TypeError('q is uint8 (e4m3 bytes), q_scale is float32')
    base = _ptr(ada)
    check(_lib.load().cvar_ln_modulate_fp8_wide(_ptr(x), base + 4 * scale_off, base + 4 * shift_off, ld_ada, rows_per,
                                                _ptr(q), ldq or fp8_ldq(Cdim), _ptr(q_scale), M, Cdim, eps, _stream()), 'cvar_ln_modulate_fp8_wide')
    return q, q_scale


def gemm_fp8(A: torch.Tensor, a_scale: torch.Tensor, W: torch.Tensor, w_scale: torch.Tensor, out: torch.Tensor, *, M: int, N: int, K: int,
             lda: int = 0, ldw: int = 0, ldc: int = 0, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, alpha: float = 1.0,
             gate: Optional[torch.Tensor] = None, ldg: int = 0, gate_rows: int = 1, gate_off: int = 0,
             residual: Optional[torch.Tensor] = None, ldr: int = 0, remap: Optional[Sequence[int]] = None,
             a_off: int = 0, w_off: int = 0, c_off: int = 0, as_off: int = 0, ws_off: int = 0,
             split: Optional[tuple] = None, split_alpha: float = 1.0, desc_hook=None):
    """C = epilogue(((qA @ qW^T) * a_scale[m]) * w_scale[n]) on e4m3 operands (cvar_gemm_fp8, include/cvar_serve.h).  A [M][lda] and W [N][ldw] are
    uint8 tensors of e4m3 bytes; lda, ldw, a_off and w_off are in bytes, as_off / ws_off in scales, c_off in elements of out.
    desc_hook(d): last-minute edits of the descriptor (tests of the refusals)."""
    if A.dtype != torch.uint8 or W.dtype != torch.uint8:
        raise TypeError('A and W are uint8 tensors of e4m3 bytes')
    d = GemmDesc()
    d.M, d.N, d.K, d.dtype = M, N, K, CVAR_BF16
    d.A, d.W = _ptr(A) + a_off, _ptr(W) + w_off
    d.lda, d.ldw = lda or K, ldw or K
    d.batch = 1
    d.alpha, d.bias, d.act = alpha, _ptr(bias), act
    if gate is not None:
        d.gate = _ptr(gate) + gate_off * 4
        d.ldg, d.gate_rows = ldg, gate_rows
    if residual is not None:
        d.residual, d.res_dtype, d.ldr = _ptr(residual), dt(residual), ldr or N
    d.C = _ptr(out) + c_off * out.element_size()
    d.out_dtype, d.ldc = dt(out), ldc or N
    if remap is not None:
        d.remap_l, d.remap_L, d.remap_off = remap
    if split is not None:
        st, d.split_n, d.ld_split = split
        if st.dtype != out.dtype:
            raise TypeError('split target and out must share a dtype')
        d.C_split = _ptr(st)
        d.split_alpha = float(split_alpha)
    if desc_hook is not None:
        desc_hook(d)
    args = (C.byref(d), _ptr(a_scale) + 4 * as_off, _ptr(w_scale) + 4 * ws_off, _stream())
    if GEMM_PROFILE is None:
        check(_lib.load().cvar_gemm_fp8(*args), 'cvar_gemm_fp8')
    else:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        check(_lib.load().cvar_gemm_fp8(*args), 'cvar_gemm_fp8')
        e1.record()
        tag = ('gemm_fp8', M, N, K, 1, 'gate' if gate is not None else ('res' if residual is not None else ('act' if act else ('remap' if remap is not None else 'plain'))), str(out.dtype)[6:])
        GEMM_PROFILE.append((e0, e1, 2.0 * M * N * K, tag))
    return out


def silu_cast(x: torch.Tensor, out: torch.Tensor):
    check(_lib.load().cvar_silu_cast(_ptr(x), _ptr(out), dt(out), x.numel(), _stream()), 'cvar_silu_cast')
    return out


def _level_arrays(lvl_end, holes):
    """lvl_end: level ends; holes: optional [(lo, hi)] per level (keys the level's queries do not see) -> ctypes int arrays"""
    n = len(lvl_end) if lvl_end else 0
    arr = (C.c_int * max(n, 1))(*(lvl_end or [0]))
    harr = None
    if holes:
        if len(holes) != n:
            raise ValueError('one (lo, hi) hole per level')
        harr = (C.c_int * (2 * n))(*[int(v) for h in holes for v in h])
    return n, arr, harr


def attention(qkv: torch.Tensor, out: torch.Tensor, R: int, H: int, Lmax: int, q_off: int, l: int, scale: float,
              lvl_end: Optional[Sequence[int]] = None, qkv_off: int = 0, rowwise: bool = False, lse: Optional[torch.Tensor] = None,
              holes: Optional[Sequence[Sequence[int]]] = None, q: Optional[torch.Tensor] = None, prescaled: bool = False, v1: bool = False):
    """q=None: qkv is the packed arena [R][Lmax][3C]; q given: qkv is a K/V arena [R][Lmax][2C] and q holds the call's queries [R*l][C].
    prescaled: the query rows already carry scale * log2(e) (cvar_attention_prescaled; `scale` is then not used).  v1: the round-2 kernel."""
    n, arr, harr = _level_arrays(lvl_end, holes)
    if q is not None and (q.dtype != qkv.dtype or q.numel() < R * l * H * 64):
        raise ValueError('q must hold R*l rows of H*64 elements in the arena dtype')
    if prescaled:
        if rowwise or q is None:
            raise ValueError('prescaled queries: K/V-arena form of the MFMA kernel only')
        check(_lib.load().cvar_attention_prescaled(_ptr(qkv) + qkv_off * qkv.element_size(), _ptr(q), dt(qkv), R, H, Lmax, q_off, l,
                                                   arr, n, harr, _ptr(out), _ptr(lse), _stream()), 'cvar_attention_prescaled')
        return out
    fn = _lib.load().cvar_attention_rowwise if rowwise else (_lib.load().cvar_attention_v1 if v1 else _lib.load().cvar_attention)
    check(fn(_ptr(qkv) + qkv_off * qkv.element_size(), _ptr(q), dt(qkv), R, H, Lmax, q_off, l, scale,
                                     arr, n, harr, _ptr(out), _ptr(lse), _stream()), 'cvar_attention')
    return out


def _check_kv8(name: str, kv8: torch.Tensor, kv_scale: torch.Tensor, R: int, H: int, Lmax: int, kv8_off: int, scale_off: int):
    if kv8.dtype != torch.uint8 or kv_scale.dtype != torch.float32 or not kv8.is_contiguous() or not kv_scale.is_contiguous():
        raise ValueError(f'{name}: the arena is contiguous uint8 [.., R, Lmax, 2*H*64] with a contiguous float32 scale table [.., R, Lmax, 2*H]')
    if kv8_off < 0 or scale_off < 0 or kv8.numel() - kv8_off < R * Lmax * 2 * H * 64 or kv_scale.numel() - scale_off < R * Lmax * 2 * H:
        raise ValueError(f'{name}: the arena / scale table is smaller than R x Lmax x 2H head vectors behind the offset')


def kv_append_fp8(kv: torch.Tensor, kv8: torch.Tensor, kv_scale: torch.Tensor, R: int, H: int, Lmax: int, q_off: int, l: int,
                  kv8_off: int = 0, scale_off: int = 0):
    """cvar_kv_append_fp8 (include/cvar_kvcache.h): the bf16 k|v rows [R*l][2*H*64] of one pass -> e4m3 bytes and power-of-two scales of the
    arena rows (r, q_off + t) of one layer (kv8_off / scale_off: that layer's offset, in elements)."""
    if kv.dtype != torch.bfloat16 or not kv.is_contiguous() or kv.numel() < R * l * 2 * H * 64:
        raise ValueError('kv_append_fp8: kv must be contiguous bfloat16 with R*l rows of 2*H*64 elements')
    _check_kv8('kv_append_fp8', kv8, kv_scale, R, H, Lmax, kv8_off, scale_off)
    check(_lib.load().cvar_kv_append_fp8(_ptr(kv), _ptr(kv8) + kv8_off, _ptr(kv_scale) + 4 * scale_off, R, H, Lmax, q_off, l, _stream()),
          'cvar_kv_append_fp8')


def attention_kv8(kv8: torch.Tensor, kv_scale: torch.Tensor, q: torch.Tensor, out: torch.Tensor, R: int, H: int, Lmax: int, q_off: int, l: int,
                  lvl_end: Optional[Sequence[int]] = None, holes: Optional[Sequence[Sequence[int]]] = None, lse: Optional[torch.Tensor] = None,
                  kv8_off: int = 0, scale_off: int = 0):
    """cvar_attention_kv8 (include/cvar_kvcache.h): attention(..., prescaled=True) over the e4m3 arena of one layer"""
    n, arr, harr = _level_arrays(lvl_end, holes)
    if q.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or q.numel() < R * l * H * 64 or out.numel() < R * l * H * 64:
        raise ValueError('attention_kv8: q and out must hold R*l bfloat16 rows of H*64 elements')
    _check_kv8('attention_kv8', kv8, kv_scale, R, H, Lmax, kv8_off, scale_off)
    check(_lib.load().cvar_attention_kv8(_ptr(kv8) + kv8_off, _ptr(kv_scale) + 4 * scale_off, _ptr(q), R, H, Lmax, q_off, l, arr, n, harr,
                                         _ptr(out), _ptr(lse), _stream()), 'cvar_attention_kv8')
    return out


def attention_bwd(qkv, o, dout, lse, dqkv, ws, R, H, Lmax, l, scale, lvl_end=None, qkv_off: int = 0, rowwise: bool = False, holes=None):
    n, arr, harr = _level_arrays(lvl_end, holes)
    fn = _lib.load().cvar_attention_bwd_rowwise if rowwise else _lib.load().cvar_attention_bwd
    check(fn(_ptr(qkv) + qkv_off * qkv.element_size(), dt(qkv), _ptr(o), _ptr(dout), _ptr(lse), R, H, Lmax, 0, l, scale,
                                         arr, n, harr, _ptr(dqkv), _ptr(ws), _stream()), 'cvar_attention_bwd')
    return dqkv


def cos_qk_norm(qkv: torch.Tensor, R: int, H: int, Lmax: int, q_off: int, l: int, scale_mul: torch.Tensor,
                qkv_off: int = 0, sm_off: int = 0, norms: Optional[torch.Tensor] = None, q: Optional[torch.Tensor] = None, q_mul: float = 1.0):
    check(_lib.load().cvar_cos_qk_norm(_ptr(qkv) + qkv_off * qkv.element_size(), _ptr(q), dt(qkv), R, H, Lmax, q_off, l,
                                       _ptr(scale_mul) + 4 * sm_off, _ptr(norms), float(q_mul), _stream()), 'cvar_cos_qk_norm')


def cos_qk_norm_bwd(qkv, dqkv, R, H, Lmax, l, scale_mul, norms, dsm_tok, sm_off: int = 0):
    check(_lib.load().cvar_cos_qk_norm_bwd(_ptr(qkv), _ptr(dqkv), dt(qkv), R, H, Lmax, l, _ptr(scale_mul) + 4 * sm_off, _ptr(norms), _ptr(dsm_tok),
                                           _stream()), 'cvar_cos_qk_norm_bwd')


def cfg_sample(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: Sequence[float], top_k: int, top_p: float,
               seed: int, stage: int, n_draw: int, idx_out: torch.Tensor, combined: Optional[torch.Tensor] = None,
               margin: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None, seed_dev: Optional[torch.Tensor] = None,
               ldv: int = 0, codebook: Optional[torch.Tensor] = None, smooth_mul: float = 1.0, smooth_tau: float = 1.0,
               gumbel: Optional[torch.Tensor] = None, soft_out: Optional[torch.Tensor] = None, expo: Optional[torch.Tensor] = None):
    """expo: Exp(1) noise (n_draw*B, l, V) fp32 contiguous, drawn by the caller (``torch.empty(...).exponential_(generator=g)``); the draw is
    then torch.multinomial's on the same noise, argmax(softmax(masked) / expo) (include/cvar.h)"""
    if expo is not None and (expo.dtype != torch.float32 or not expo.is_contiguous() or expo.numel() != n_draw * B * l * V
                             or expo.device != logits.device):
        raise ValueError(f'cfg_sample: expo must be a contiguous float32 ({n_draw * B}, {l}, {V}) tensor on {logits.device}')
    arr = (C.c_float * 4)(*(list(coef) + [0.0] * (4 - len(coef))))
    check(_lib.load().cvar_cfg_sample(_ptr(logits), B, nrep, l, V, arr, top_k, float(top_p), int(seed) & (2 ** 64 - 1), _ptr(seed_dev), stage, n_draw,
                                      _ptr(idx_out), _ptr(combined), _ptr(margin), _ptr(kept), int(ldv), _ptr(codebook),
                                      codebook.shape[1] if codebook is not None else 0, float(smooth_mul), float(smooth_tau), _ptr(gumbel), _ptr(soft_out),
                                      _ptr(expo), _stream()), 'cvar_cfg_sample')
    return idx_out


def cfg_sample_rows(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                    seed: torch.Tensor, stage: int, n_draw: int, idx_out: torch.Tensor, combined: Optional[torch.Tensor] = None,
                    margin: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None, ldv: int = 0,
                    expo: Optional[torch.Tensor] = None, soft_out: Optional[torch.Tensor] = None):
    """cfg_sample with one parameter set per batch row (cvar_cfg_sample_rows, include/cvar_serve.h): coef (B, 4) float32 - this stage's
    combine weights, rounded on the host -, top_k (B,) int32, top_p (B,) float32, seed (B,) int64 (the uint64 seed's bit pattern), all
    contiguous on the device of `logits`.  Row b equals cfg_sample at B = 1 on that row's logits with coef[b], top_k[b], top_p[b] and
    seed[b], bit for bit.  expo / soft_out are refused by the library (CvarError): the per-row form draws from the counter generator only."""
    for name, t, dtype, shape in (('coef', coef, torch.float32, (B, 4)), ('top_k', top_k, torch.int32, (B,)), ('top_p', top_p, torch.float32, (B,)),
                                  ('seed', seed, torch.int64, (B,))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device):
            raise ValueError(f'cfg_sample_rows: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor on {logits.device}')
    check(_lib.load().cvar_cfg_sample_rows(_ptr(logits), B, nrep, l, V, _ptr(coef), _ptr(top_k), _ptr(top_p), _ptr(seed), stage, n_draw,
                                           _ptr(idx_out), _ptr(combined), _ptr(margin), _ptr(kept), int(ldv), _ptr(expo), _ptr(soft_out), _stream()),
          'cvar_cfg_sample_rows')
    return idx_out


def cfg_sample_edit(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                    seed: torch.Tensor, stage: int, n_draw: int, idx_out: torch.Tensor, forced: torch.Tensor, combined: Optional[torch.Tensor] = None,
                    margin: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None, ldv: int = 0,
                    expo: Optional[torch.Tensor] = None, soft_out: Optional[torch.Tensor] = None):
    """cfg_sample_rows with per-token forcing (cvar_cfg_sample_edit, include/cvar_serve.h).  forced: (B, l) int32 on the device of `logits`,
    unit stride along the tokens - this stage's columns of the forced-token table, a view of it will do (its row stride is handed on as ldf).
    A token with forced >= 0 gets that id in all n_draw rows, kept = 0, margin = +inf, no combined row, and none of its logits is read; every
    other token is what cfg_sample_rows gives, bit for bit."""
    for name, t, dtype, shape in (('coef', coef, torch.float32, (B, 4)), ('top_k', top_k, torch.int32, (B,)), ('top_p', top_p, torch.float32, (B,)),
                                  ('seed', seed, torch.int64, (B,))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device):
            raise ValueError(f'cfg_sample_edit: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor on {logits.device}')
    ldf = 0
    if forced is not None:
        if (not torch.is_tensor(forced) or forced.dtype != torch.int32 or tuple(forced.shape) != (B, l) or forced.stride(1) != 1
                or (B > 1 and forced.stride(0) < l) or forced.device != logits.device):
            raise ValueError(f'cfg_sample_edit: forced must be an int32 ({B}, {l}) tensor on {logits.device} with unit stride along the tokens')
        ldf = forced.stride(0) if B > 1 else max(forced.stride(0), l)
    check(_lib.load().cvar_cfg_sample_edit(_ptr(logits), B, nrep, l, V, _ptr(coef), _ptr(top_k), _ptr(top_p), _ptr(seed), stage, n_draw,
                                           _ptr(idx_out), _ptr(combined), _ptr(margin), _ptr(kept), int(ldv), _ptr(expo), _ptr(soft_out),
                                           _ptr(forced), int(ldf), _stream()),
          'cvar_cfg_sample_edit')
    return idx_out


def score_rows(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, target: torch.Tensor,
               combined: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None,
               rank: Optional[torch.Tensor] = None, argmax: Optional[torch.Tensor] = None, ldv: int = 0):
    """Score a given id per token under the CFG-combined distribution (cvar_score_rows, include/cvar_serve.h).  coef (B, 4) float32, the
    sampler's table of this stage; target: (B, l) int32 on the device of `logits`, unit stride along the tokens - a column slice of a wider
    table will do (its row stride is handed on as ldt); < 0: no target (logprob 0, rank -1).  Outputs, each optional but not all None:
    combined (B, l, V) float32 contiguous; logprob / entropy float32 and rank / argmax int32, each (B, l) with unit stride along the tokens
    and ONE row stride for the four (handed on as ldo): the columns of one scale in (B, L) buffers will do.
    The log-probabilities are those of the unfiltered combined distribution; a top-k / top-p kept set is not renormalised over."""
    dev = logits.device
    if coef is not None and (not torch.is_tensor(coef) or coef.dtype != torch.float32 or tuple(coef.shape) != (B, 4) or not coef.is_contiguous()
                             or coef.device != dev):
        raise ValueError(f'score_rows: coef must be a contiguous float32 {(B, 4)} tensor on {dev}')

    def row_stride(name, t, dtype):
        if (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (B, l) or t.stride(1) != 1 or (B > 1 and t.stride(0) < l) or t.device != dev):
            raise ValueError(f'score_rows: {name} must be {"an" if dtype == torch.int32 else "a"} {str(dtype)[6:]} ({B}, {l}) tensor on {dev} with unit stride '
                             'along the tokens')
        return t.stride(0) if B > 1 else max(t.stride(0), l)

    ldt = row_stride('target', target, torch.int32) if target is not None else 0
    if combined is not None and (not torch.is_tensor(combined) or combined.dtype != torch.float32 or tuple(combined.shape) != (B, l, V)
                                 or not combined.is_contiguous() or combined.device != dev):
        raise ValueError(f'score_rows: combined must be a contiguous float32 ({B}, {l}, {V}) tensor on {dev}')
    ldo = {row_stride(name, t, dtype) for name, t, dtype in (('logprob', logprob, torch.float32), ('entropy', entropy, torch.float32),
                                                             ('rank', rank, torch.int32), ('argmax', argmax, torch.int32)) if t is not None}
    if len(ldo) > 1:
        raise ValueError(f'score_rows: logprob / entropy / rank / argmax must share one row stride, got {sorted(ldo)}')
    check(_lib.load().cvar_score_rows(_ptr(logits), B, nrep, l, V, _ptr(coef), _ptr(target), int(ldt), _ptr(combined), _ptr(logprob), _ptr(entropy),
                                      _ptr(rank), _ptr(argmax), int(ldo.pop()) if ldo else 0, int(ldv), _stream()), 'cvar_score_rows')


def score_topn(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, N: int, top_id: Optional[torch.Tensor] = None,
               top_logprob: Optional[torch.Tensor] = None, tail_logprob: Optional[torch.Tensor] = None, ldv: int = 0):
    """The N most likely codes per token under the CFG-combined distribution (cvar_score_topn, include/cvar_topn.h), in cvar_score_rows' rank
    order, with the log-probabilities score_rows would report for them and the log of the mass of all the other codes.  logits / coef as
    score_rows takes them.  top_id int32 / top_logprob float32: (B, l, N) with unit stride along N and stride N along the tokens;
    tail_logprob float32 (B, l) with unit stride along the tokens; ONE row stride in tokens for the three (handed on as ldo): the columns of
    one scale in (B, L, N) / (B, L) buffers will do.  top_id and top_logprob are each optional, but not both None."""
    dev = logits.device
    if coef is not None and (not torch.is_tensor(coef) or coef.dtype != torch.float32 or tuple(coef.shape) != (B, 4) or not coef.is_contiguous()
                             or coef.device != dev):
        raise ValueError(f'score_topn: coef must be a contiguous float32 {(B, 4)} tensor on {dev}')
    if not isinstance(N, int) or isinstance(N, bool) or not 1 <= N <= _lib.TOPN_MAX:
        raise ValueError(f'score_topn: N must be an integer in 1..{_lib.TOPN_MAX}, got {N!r}')
    ldo = set()
    for name, t, dtype, shape in (('top_id', top_id, torch.int32, (B, l, N)), ('top_logprob', top_logprob, torch.float32, (B, l, N)),
                                  ('tail_logprob', tail_logprob, torch.float32, (B, l))):
        if t is None:
            continue
        per = N if len(shape) == 3 else 1
        if (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or t.stride(-1) != 1
                or (len(shape) == 3 and l > 1 and t.stride(1) != N) or (B > 1 and (t.stride(0) % per or t.stride(0) < l * per))):
            raise ValueError(f'score_topn: {name} must be a {str(dtype)[6:]} {shape} tensor on {dev}, dense along the tokens and the N entries')
        ldo.add(t.stride(0) // per if B > 1 and t.stride(0) % per == 0 else l)
    if len(ldo) > 1:
        raise ValueError(f'score_topn: top_id / top_logprob / tail_logprob must share one row stride in tokens, got {sorted(ldo)}')
    check(_lib.load().cvar_score_topn(_ptr(logits), B, nrep, l, V, _ptr(coef), N, _ptr(top_id), _ptr(top_logprob), _ptr(tail_logprob),
                                      int(ldo.pop()) if ldo else 0, int(ldv), _stream()), 'cvar_score_topn')


def edit_force_table(keep_ctrl: Optional[torch.Tensor], keep_img: Optional[torch.Tensor], src_ctrl: Optional[torch.Tensor],
                     src_img: Optional[torch.Tensor], patch_nums: Sequence[int], B: int, mask_first: bool, mask_factor: int, forced: torch.Tensor):
    """The forced-token table of every scale in one launch (cvar_edit_force_table, include/cvar_serve.h).  keep_*: (B, S, S) uint8 or None,
    src_*: (B, sum pn^2) int32 or None, forced: (B, mask_factor * sum pn^2) int32, all contiguous on one device; S = patch_nums[-1].
    forced = the source id where the cell rule keeps the token (a strict majority of its area-pooling bin is kept), -1 where it is free."""
    pns = [int(p) for p in patch_nums]
    S, Lsrc = pns[-1], sum(p * p for p in pns)
    for name, t, dtype, shape in (('keep_ctrl', keep_ctrl, torch.uint8, (B, S, S)), ('keep_img', keep_img, torch.uint8, (B, S, S)),
                                  ('src_ctrl', src_ctrl, torch.int32, (B, Lsrc)), ('src_img', src_img, torch.int32, (B, Lsrc)),
                                  ('forced', forced, torch.int32, (B, mask_factor * Lsrc))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                              or (forced is not None and t.device != forced.device)):
            raise ValueError(f'edit_force_table: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor' + (f' on {forced.device}' if forced is not None else ''))
    arr = (C.c_int * len(pns))(*pns)
    check(_lib.load().cvar_edit_force_table(_ptr(keep_ctrl), _ptr(keep_img), _ptr(src_ctrl), _ptr(src_img), arr, len(pns), B, S, int(bool(mask_first)),
                                            int(mask_factor), _ptr(forced), _stream()), 'cvar_edit_force_table')
    return forced


def region_coef_table(regions: torch.Tensor, strength: Optional[torch.Tensor], cfg: torch.Tensor, patch_nums: Sequence[int], B: int, K: int,
                      mask_first: bool, mask_factor: int, coef: torch.Tensor):
    """The per-token combine weights of every scale in one launch (cvar_region_coef_table, include/cvar_region.h).  regions (B, K, S, S) float32,
    strength (B, S, S) float32 or None, cfg (B, K) float64, coef (B, mask_factor * sum pn^2, 4) float32, all contiguous on one device;
    S = patch_nums[-1].  The values in the maps are not checked here (they are on the device): the caller validates them on the host."""
    pns = [int(p) for p in patch_nums]
    S, L = pns[-1], mask_factor * sum(p * p for p in pns)
    for name, t, dtype, shape in (('regions', regions, torch.float32, (B, K, S, S)), ('strength', strength, torch.float32, (B, S, S)),
                                  ('cfg', cfg, torch.float64, (B, K)), ('coef', coef, torch.float32, (B, L, 4))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous()
                              or (coef is not None and t.device != coef.device)):
            raise ValueError(f'region_coef_table: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor' + (f' on {coef.device}' if coef is not None else ''))
    arr = (C.c_int * len(pns))(*pns)
    check(_lib.load().cvar_region_coef_table(_ptr(regions), _ptr(strength), _ptr(cfg), arr, len(pns), B, K, S, int(bool(mask_first)), int(mask_factor),
                                             _ptr(coef), _stream()), 'cvar_region_coef_table')
    return coef


def _coef_slice(what: str, coef, B: int, l: int, dev) -> int:
    """this stage's slice (B, l, 4) of a (B, L, 4) weight table, a view of it will do -> its row stride in tokens (ldc)"""
    if (not torch.is_tensor(coef) or coef.dtype != torch.float32 or tuple(coef.shape) != (B, l, 4) or coef.stride(2) != 1 or coef.stride(1) != 4
            or coef.stride(0) % 4 != 0 or (B > 1 and coef.stride(0) < 4 * l) or coef.device != dev):
        raise ValueError(f'{what}: coef must be a float32 ({B}, {l}, 4) tensor on {dev}, dense along its last two dimensions')
    return coef.stride(0) // 4 if B > 1 else max(coef.stride(0) // 4, l)


def cfg_sample_map(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor,
                   seed: torch.Tensor, stage: int, n_draw: int, idx_out: torch.Tensor, forced: Optional[torch.Tensor] = None,
                   combined: Optional[torch.Tensor] = None, margin: Optional[torch.Tensor] = None, kept: Optional[torch.Tensor] = None, ldv: int = 0,
                   expo: Optional[torch.Tensor] = None, soft_out: Optional[torch.Tensor] = None):
    """cfg_sample_rows with the combine weights read per token (cvar_cfg_sample_map, include/cvar_region.h).  coef: (B, l, 4) float32 - this stage's
    columns of the (B, L, 4) table, a view of it will do (its row stride is handed on as ldc).  forced: as cfg_sample_edit takes it, or None (nothing
    is forced).  top_k / top_p / seed stay per batch row.  A token equals what cfg_sample_rows gives it with its four weights as the row's."""
    for name, t, dtype, shape in (('top_k', top_k, torch.int32, (B,)), ('top_p', top_p, torch.float32, (B,)), ('seed', seed, torch.int64, (B,))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != logits.device):
            raise ValueError(f'cfg_sample_map: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor on {logits.device}')
    ldc = _coef_slice('cfg_sample_map', coef, B, l, logits.device) if coef is not None else 0
    ldf = 0
    if forced is not None:
        if (not torch.is_tensor(forced) or forced.dtype != torch.int32 or tuple(forced.shape) != (B, l) or forced.stride(1) != 1
                or (B > 1 and forced.stride(0) < l) or forced.device != logits.device):
            raise ValueError(f'cfg_sample_map: forced must be an int32 ({B}, {l}) tensor on {logits.device} with unit stride along the tokens')
        ldf = forced.stride(0) if B > 1 else max(forced.stride(0), l)
    check(_lib.load().cvar_cfg_sample_map(_ptr(logits), B, nrep, l, V, _ptr(coef), int(ldc), _ptr(top_k), _ptr(top_p), _ptr(seed), stage, n_draw,
                                          _ptr(idx_out), _ptr(combined), _ptr(margin), _ptr(kept), int(ldv), _ptr(expo), _ptr(soft_out),
                                          _ptr(forced), int(ldf), _stream()), 'cvar_cfg_sample_map')
    return idx_out


def score_map(logits: torch.Tensor, B: int, nrep: int, l: int, V: int, coef: torch.Tensor, target: torch.Tensor,
              combined: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None,
              rank: Optional[torch.Tensor] = None, argmax: Optional[torch.Tensor] = None, ldv: int = 0):
    """score_rows with the combine weights read per token (cvar_score_map, include/cvar_region.h): coef as cfg_sample_map takes it, everything else
    as score_rows."""
    dev = logits.device
    ldc = _coef_slice('score_map', coef, B, l, dev) if coef is not None else 0

    def row_stride(name, t, dtype):
        if (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != (B, l) or t.stride(1) != 1 or (B > 1 and t.stride(0) < l) or t.device != dev):
            raise ValueError(f'score_map: {name} must be {"an" if dtype == torch.int32 else "a"} {str(dtype)[6:]} ({B}, {l}) tensor on {dev} with unit stride '
                             'along the tokens')
        return t.stride(0) if B > 1 else max(t.stride(0), l)

    ldt = row_stride('target', target, torch.int32) if target is not None else 0
    if combined is not None and (not torch.is_tensor(combined) or combined.dtype != torch.float32 or tuple(combined.shape) != (B, l, V)
                                 or not combined.is_contiguous() or combined.device != dev):
        raise ValueError(f'score_map: combined must be a contiguous float32 ({B}, {l}, {V}) tensor on {dev}')
    ldo = {row_stride(name, t, dtype) for name, t, dtype in (('logprob', logprob, torch.float32), ('entropy', entropy, torch.float32),
                                                             ('rank', rank, torch.int32), ('argmax', argmax, torch.int32)) if t is not None}
    if len(ldo) > 1:
        raise ValueError(f'score_map: logprob / entropy / rank / argmax must share one row stride, got {sorted(ldo)}')
    check(_lib.load().cvar_score_map(_ptr(logits), B, nrep, l, V, _ptr(coef), int(ldc), _ptr(target), int(ldt), _ptr(combined), _ptr(logprob),
                                     _ptr(entropy), _ptr(rank), _ptr(argmax), int(ldo.pop()) if ldo else 0, int(ldv), _stream()), 'cvar_score_map')


def ms_next_input(idx: torch.Tensor, codebook, phi_w, phi_b, up, down, f_hat, tok_out, nb, nmaps, pn, pn_next, S, Cvae,
                  phi_k: int, up_off: int, down_off: int):
    lib = _lib.load()
    pw = _ptr(phi_w) + 4 * phi_k * Cvae * 9 * Cvae
    pb = _ptr(phi_b) + 4 * phi_k * Cvae
    check(lib.cvar_ms_next_input(_ptr(idx), _ptr(codebook), pw, pb, _ptr(up) + 4 * up_off, _ptr(down) + 4 * down_off,
                                 _ptr(f_hat), _ptr(tok_out), nb, nmaps, pn, pn_next, S, Cvae, _stream()), 'cvar_ms_next_input')


def ms_encode(f, codebook, V, phi_w, phi_b, phi_map, patch_nums, up, down, idx_out, f_hat_out, margin_out, B, S, Cvae):
    n = len(patch_nums)
    pm = (C.c_int * n)(*phi_map)
    pn = (C.c_int * n)(*patch_nums)
    check(_lib.load().cvar_ms_encode(_ptr(f), _ptr(codebook), V, _ptr(phi_w), _ptr(phi_b), pm, pn, n, _ptr(up), _ptr(down),
                                     _ptr(idx_out), _ptr(f_hat_out), _ptr(margin_out), B, S, Cvae, _stream()), 'cvar_ms_encode')


def word_embed(tok, W, bias, lvl_pos, x, nb, nrep, l, Cvae, Cdim, x_rows, x_off, lvl_off: int = 0):
    check(_lib.load().cvar_word_embed(_ptr(tok), _ptr(W), _ptr(bias), _ptr(lvl_pos) + 4 * lvl_off * Cdim, _ptr(x), nb, nrep, l, Cvae, Cdim,
                                      x_rows, x_off, _stream()), 'cvar_word_embed')


def first_tokens(class_emb, cond_embed, labels, types, pos_start, lvl_pos, x, cond, R, first_l, Cdim, x_rows):
    check(_lib.load().cvar_first_tokens(_ptr(class_emb), _ptr(cond_embed), _ptr(labels), _ptr(types), _ptr(pos_start), _ptr(lvl_pos),
                                        _ptr(x), _ptr(cond), R, first_l, Cdim, x_rows, _stream()), 'cvar_first_tokens')


def groupnorm_ws_bytes(B, HW, Cdim) -> int:
    return int(_lib.load().cvar_groupnorm_ws_bytes(B, HW, Cdim))


def groupnorm_silu(x, weight, bias, out, B, HW, Cdim, groups, eps, silu, ws):
    check(_lib.load().cvar_groupnorm_silu(_ptr(x), dt(x), _ptr(weight), _ptr(bias), _ptr(out), B, HW, Cdim, groups, eps, int(silu),
                                          _ptr(ws), _stream()), 'cvar_groupnorm_silu')
    return out


def split3(x, out, M, Cdim, Cpad=0, ldx=0):
    """fp32 x[M][ldx] -> bf16 out[M][Cpad or 3 C] = [hi | lo | hi] (+ zero padding): the activation side of a split-bf16 product (cvar_split3, ABI 20)"""
    check(_lib.load().cvar_split3(_ptr(x), ldx or Cdim, _ptr(out), M, Cdim, Cpad or 3 * Cdim, _stream()), 'cvar_split3')
    return out


def groupnorm_silu_split3(x, weight, bias, out, B, HW, Cdim, groups, eps, silu, ws):
    check(_lib.load().cvar_groupnorm_silu_split3(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), B, HW, Cdim, groups, eps, int(silu), _ptr(ws), _stream()),
          'cvar_groupnorm_silu_split3')
    return out


def conv_gn_partials(dtype: torch.dtype, stride: int, Cin: int, Cout: int, Hin: int, Win: int, Hout: int, Wout: int):
    """(tiles_per_image, pixels_per_tile) when a 3x3 conv of this shape emits GroupNorm partials of its output (gemm(..., gn_part=...)), else None"""
    if GEMM_TILE_CFG not in (0, 6):
        return None
    nt, pp = C.c_int(0), C.c_int(0)
    if dtype not in _DT:
        return None
    ok = _lib.load().cvar_conv3x3_gn_partials(_DT[dtype], stride, Cin, Cout, Hin, Win, Hout, Wout, C.byref(nt), C.byref(pp))
    return (nt.value, pp.value) if ok else None


def groupnorm_silu_partials(x, weight, bias, out, B, HW, Cdim, groups, eps, silu, gn_part, tiles, tile_pixels, ws):
    check(_lib.load().cvar_groupnorm_silu_partials(_ptr(x), dt(x), _ptr(weight), _ptr(bias), _ptr(out), B, HW, Cdim, groups, eps, int(silu),
                                                   _ptr(gn_part), tiles, tile_pixels, _ptr(ws), _stream()), 'cvar_groupnorm_silu_partials')
    return out


def softmax_rows(s, p, rows, cols):
    check(_lib.load().cvar_softmax_rows(_ptr(s), _ptr(p), dt(p), rows, cols, _stream()), 'cvar_softmax_rows')
    return p


def transpose(inp, out, B, n, c, ld_in, in_off: int = 0, ld_out: int = 0):
    check(_lib.load().cvar_transpose(_ptr(inp) + in_off * inp.element_size(), _ptr(out), dt(inp), B, n, c, ld_in, ld_out or n, _stream()), 'cvar_transpose')
    return out


def nchw_to_nhwc(inp, out, B, Cdim, HW, Cpad):
    check(_lib.load().cvar_nchw_to_nhwc(_ptr(inp), _ptr(out), dt(out), B, Cdim, HW, Cpad, _stream()), 'cvar_nchw_to_nhwc')
    return out


def nhwc_to_nchw(inp, ld_in, out, B, Cdim, HW, lo=-3.0e38, hi=3.0e38, mul=1.0, add=0.0):
    check(_lib.load().cvar_nhwc_to_nchw(_ptr(inp), dt(inp), ld_in, _ptr(out), B, Cdim, HW, lo, hi, mul, add, _stream()), 'cvar_nhwc_to_nchw')
    return out


def embed_rows(idx: torch.Tensor, codebook: torch.Tensor, out: torch.Tensor):
    """out[n] = codebook[idx[n]] (int32 ids, fp32 rows)"""
    check(_lib.load().cvar_embed_rows(_ptr(idx), _ptr(codebook), codebook.shape[0], _ptr(out), idx.numel(), codebook.shape[1], _stream()), 'cvar_embed_rows')
    return out


def resample_sep(inp: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, out: torch.Tensor, B: int, h: int, w: int, H: int, W: int, Cdim: int):
    """NHWC fp32 separable resample with dense (H x h), (W x w) matrices"""
    check(_lib.load().cvar_resample_sep(_ptr(inp), _ptr(wy), _ptr(wx), _ptr(out), B, h, w, H, W, Cdim, _stream()), 'cvar_resample_sep')
    return out


# ------------------------------------------------------------------------------------------ training step
def gate_residual(x, f, gate, gate_off, ldg, gate_rows, rowscale, M, Cdim):
    check(_lib.load().cvar_gate_residual(_ptr(x), _ptr(f), dt(f), _ptr(gate) + 4 * gate_off, ldg, gate_rows, _ptr(rowscale), M, Cdim, _stream()), 'cvar_gate_residual')


def train_ws_floats(M: int, R: int, Cdim: int) -> int:
    """floats of workspace cvar_gated_grad / cvar_ln_modulate_bwd may use for M = R x l rows (cvar_train_ws_floats)"""
    return int(_lib.load().cvar_train_ws_floats(M, R, Cdim))


def gated_grad(dx, f, gate, gate_off, ldg, rowscale, df, dgate, dgate_off, ldo, R, l, Cdim, ws):
    check(_lib.load().cvar_gated_grad(_ptr(dx), _ptr(f), dt(f), _ptr(gate) + 4 * gate_off, ldg, _ptr(rowscale), _ptr(df), _ptr(dgate) + 4 * dgate_off, ldo,
                                      R, l, Cdim, _ptr(ws), ws.numel(), _stream()), 'cvar_gated_grad')


def gelu(a, h):
    check(_lib.load().cvar_gelu(_ptr(a), _ptr(h), dt(a), a.numel(), _stream()), 'cvar_gelu')
    return h


def gelu_bwd(a, dh):
    check(_lib.load().cvar_gelu_bwd(_ptr(a), _ptr(dh), dt(a), a.numel(), _stream()), 'cvar_gelu_bwd')
    return dh


def ln_modulate_bwd(x, dy, ada, scale_off, ld_ada, rows_per, dx_in, dx_out, dada, dscale_off, dshift_off, ldo, M, Cdim, eps, ws):
    check(_lib.load().cvar_ln_modulate_bwd(_ptr(x), _ptr(dy), dt(dy), _ptr(ada) + 4 * scale_off, ld_ada, rows_per, _ptr(dx_in), _ptr(dx_out),
                                           _ptr(dada) + 4 * dscale_off, _ptr(dada) + 4 * dshift_off, ldo, M, Cdim, eps, _ptr(ws), ws.numel(), _stream()), 'cvar_ln_modulate_bwd')


def colsum(A, lda, out, M, N, ws, accumulate=False, a_off: int = 0, out_off: int = 0):
    check(_lib.load().cvar_colsum(_ptr(A) + a_off * A.element_size(), dt(A), lda, _ptr(out) + 4 * out_off, M, N, int(accumulate), _ptr(ws), _stream()), 'cvar_colsum')


def wordembed_grad(dx, ldx: int, rows_per_sample: int, skip: int, tok, n_per_sample: int, B: int, Cdim: int, Cvae: int, out, w_off: int, b_off: int,
                   dx_off: int = 0, accumulate: bool = False):
    """dW (Cdim x Cvae at out[w_off:]) and db (out[b_off:]) of word_embed from the token-major fp32 tensors (cvar_wordembed_grad);
    accumulate: both become fp32(old + plain) (cvar_wordembed_grad_acc)"""
    lib = _lib.load()
    nb = lib.cvar_wordembed_grad_ws_bytes(B * n_per_sample, Cdim)
    ws = torch.empty(nb, device=dx.device, dtype=torch.uint8)
    if accumulate:
        check(lib.cvar_wordembed_grad_acc(_ptr(dx) + 4 * dx_off, ldx, rows_per_sample, skip, _ptr(tok), n_per_sample, B, Cdim, Cvae,
                                          _ptr(out) + 4 * w_off, _ptr(out) + 4 * b_off, _ptr(ws), 1, _stream()), 'cvar_wordembed_grad_acc')
        return
    check(lib.cvar_wordembed_grad(_ptr(dx) + 4 * dx_off, ldx, rows_per_sample, skip, _ptr(tok), n_per_sample, B, Cdim, Cvae,
                                  _ptr(out) + 4 * w_off, _ptr(out) + 4 * b_off, _ptr(ws), _stream()), 'cvar_wordembed_grad')


def add_inplace(y, x, n: int, y_off: int = 0, x_off: int = 0):
    """y[y_off + i] = fp32(y[y_off + i] + x[x_off + i]), i < n, both fp32 and not overlapping (cvar_add_inplace): a staging buffer into an accumulator"""
    if y.dtype != torch.float32 or x.dtype != torch.float32:
        raise TypeError('add_inplace: y and x are fp32')
    if n <= 0 or y_off < 0 or x_off < 0 or y_off + n > y.numel() or x_off + n > x.numel():
        raise ValueError(f'add_inplace: range of {n} at {y_off} / {x_off} outside tensors of {y.numel()} / {x.numel()} elements')
    check(_lib.load().cvar_add_inplace(_ptr(y) + 4 * y_off, _ptr(x) + 4 * x_off, n, _stream()), 'cvar_add_inplace')


def rowsum(A, lda, out, nrows, ncols, accumulate=False, out_off: int = 0):
    check(_lib.load().cvar_rowsum(_ptr(A), dt(A), lda, _ptr(out) + 4 * out_off, nrows, ncols, int(accumulate), _stream()), 'cvar_rowsum')


def ce_fwd_bwd(logits, target, weight, gscale, loss_tok, dlogits, M, V):
    check(_lib.load().cvar_ce_fwd_bwd(_ptr(logits), _ptr(target), _ptr(weight), float(gscale), _ptr(loss_tok), _ptr(dlogits),
                                      dt(dlogits) if dlogits is not None else CVAR_F32, M, V, _stream()), 'cvar_ce_fwd_bwd')


def pg_fwd_bwd(logits, target, adv, weight, old_lp, ref_lp, clip_lo, clip_hi, kl_coef, gscale, loss_tok, M, V, dlogits=None, logprob=None,
               ratio=None, kl=None, clipped=None, coef=None):
    """the clipped policy-gradient loss on the rows cvar_ce_fwd_bwd takes (cvar_pg_fwd_bwd, include/cvar_policy.h): weight / old_lp / ref_lp and
    every output but loss_tok may be None"""
    check(_lib.load().cvar_pg_fwd_bwd(_ptr(logits), _ptr(target), _ptr(adv), _ptr(weight), _ptr(old_lp), _ptr(ref_lp), float(clip_lo), float(clip_hi),
                                      float(kl_coef), float(gscale), _ptr(loss_tok), _ptr(logprob), _ptr(ratio), _ptr(kl), _ptr(clipped), _ptr(coef),
                                      _ptr(dlogits), dt(dlogits) if dlogits is not None else CVAR_F32, M, V, _stream()), 'cvar_pg_fwd_bwd')


def kd_fwd_bwd(logits, teacher, ldt, weight, gscale, loss_tok, dlogits, M, V):
    """the soft-target loss on the rows cvar_ce_fwd_bwd takes (cvar_kd_fwd_bwd, include/cvar_distill.h): teacher logits [M][ldt] fp32 in the place
    of the target ids; weight and dlogits may be None"""
    check(_lib.load().cvar_kd_fwd_bwd(_ptr(logits), _ptr(teacher), int(ldt), _ptr(weight), float(gscale), _ptr(loss_tok), _ptr(dlogits),
                                      dt(dlogits) if dlogits is not None else CVAR_F32, M, V, _stream()), 'cvar_kd_fwd_bwd')


def kd_topn_fwd_bwd(logits, t_id, t_lp, t_tail, N, weight, gscale, loss_tok, dlogits, M, V):
    """the sparse soft-target loss on the rows cvar_ce_fwd_bwd takes (cvar_kd_topn_fwd_bwd, include/cvar_topn.h): the teacher as N listed codes per
    row - t_id [M][N] int32 (< 0: unused), t_lp [M][N] fp32 - and the log of its mass on all the others, t_tail [M] fp32 (None: no tail mass);
    weight and dlogits may be None"""
    check(_lib.load().cvar_kd_topn_fwd_bwd(_ptr(logits), _ptr(t_id), _ptr(t_lp), _ptr(t_tail), int(N), _ptr(weight), float(gscale), _ptr(loss_tok),
                                           _ptr(dlogits), dt(dlogits) if dlogits is not None else CVAR_F32, M, V, _stream()), 'cvar_kd_topn_fwd_bwd')


def scatter_add_rows(src, ld_src, idx, dst, n, Cdim, src_off: int = 0):
    check(_lib.load().cvar_scatter_add_rows(_ptr(src) + 4 * src_off, ld_src, _ptr(idx), _ptr(dst), n, Cdim, _stream()), 'cvar_scatter_add_rows')


def silu_bwd(cond, dsilu, dcond):
    check(_lib.load().cvar_silu_bwd(_ptr(cond), _ptr(dsilu), _ptr(dcond), cond.numel(), _stream()), 'cvar_silu_bwd')


def adamw(p, g, m, v, lr, b1, b2, eps, wd, step, gscale_dev=None, gscale=1.0):
    check(_lib.load().cvar_adamw(_ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, b1, b2, eps, wd, step, _ptr(gscale_dev), gscale, _stream()), 'cvar_adamw')


def sumsq(x, partial, slot):
    check(_lib.load().cvar_sumsq(_ptr(x), x.numel(), _ptr(partial) + 8 * 256 * slot, _stream()), 'cvar_sumsq')


def adam_table(entries, device) -> torch.Tensor:
    """device table of cvar_adam_tensor {p, g, m, v, n, group, pad, w16} (7 x int64 per entry) for the multi-tensor optimizer calls;
    an entry is (p, g, m, v, group) or (p, g, m, v, group, w16) with w16 a contiguous bf16 tensor of p's size (or None)"""
    rows = []
    for (p, g, m, v, group, *rest) in entries:
        w16 = rest[0] if rest else None
        if w16 is not None and (w16.dtype != torch.bfloat16 or w16.numel() != p.numel() or not w16.is_contiguous()):
            raise ValueError('adam_table: the bf16 copy must be a contiguous bfloat16 tensor of the size of the parameter')
        rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), int(group) & 0xffffffff, w16.data_ptr() if w16 is not None else 0])
    return torch.tensor(rows, dtype=torch.int64).to(device)


def sumsq_multi(table: torch.Tensor, n: int, partial: torch.Tensor):
    check(_lib.load().cvar_sumsq_multi(_ptr(table), n, _ptr(partial), _stream()), 'cvar_sumsq_multi')


def adamw_multi(table: torch.Tensor, n: int, lrs: Sequence[float], wds: Sequence[float], b1, b2, eps, step, gscale_dev=None, gscale=1.0):
    la = (C.c_float * len(lrs))(*lrs)
    wa = (C.c_float * len(wds))(*wds)
    check(_lib.load().cvar_adamw_multi(_ptr(table), n, la, wa, len(lrs), b1, b2, eps, step, _ptr(gscale_dev), gscale, _stream()), 'cvar_adamw_multi')


def clip_coef(partial, count, pre_scale, max_norm, out2):
    check(_lib.load().cvar_clip_coef(_ptr(partial), count, pre_scale, max_norm, _ptr(out2), _stream()), 'cvar_clip_coef')


# ---- tokenizer input pipeline (preprocess.py)
def resample_u8(src: torch.Tensor, src_h: int, src_w: int, channels: int, axis: int, dst_extent: int, bounds: torch.Tensor,
                coeffs: torch.Tensor, ksize: int, dst: torch.Tensor):
    check(_lib.load().cvar_resample_u8(_ptr(src), src_h, src_w, channels, axis, dst_extent, _ptr(bounds), _ptr(coeffs), ksize, _ptr(dst),
                                       _stream()), 'cvar_resample_u8')
    return dst


def crop_flip_normalize(src: torch.Tensor, src_h: int, src_w: int, channels: int, top: int, left: int, out_h: int, out_w: int,
                        flip: bool, dst: torch.Tensor):
    check(_lib.load().cvar_crop_flip_normalize(_ptr(src), src_h, src_w, channels, top, left, out_h, out_w, int(flip), _ptr(dst),
                                               _stream()), 'cvar_crop_flip_normalize')
    return dst


def ignore_mask(cond: torch.Tensor, B: int, H: int, W: int, patch_nums: Sequence[int], first_masked_scale: int, image_first: int,
                out: torch.Tensor, L: int):
    arr = (C.c_int * len(patch_nums))(*patch_nums)
    check(_lib.load().cvar_ignore_mask(_ptr(cond), B, H, W, arr, len(patch_nums), first_masked_scale, image_first, _ptr(out), L,
                                       _stream()), 'cvar_ignore_mask')
    return out


def rle_paint(run_ends: torch.Tensor, ann_offsets: torch.Tensor, colours: torch.Tensor, n_ann: int, H: int, W: int, out: torch.Tensor):
    check(_lib.load().cvar_rle_paint(_ptr(run_ends), _ptr(ann_offsets), _ptr(colours), n_ann, H, W, _ptr(out), _stream()), 'cvar_rle_paint')
    return out


# ---- LoRA adapter branch (cvar_lora_*, ABI 21).  Offsets (*_off) in elements; the (seed, tag) pair names one target's dropout mask.
def lora_down(x, A, u, *, M: int, K: int, r: int, scale: float, p: float = 0.0, seed: int = 0, tag: int = 0, ldx: int = 0, lda: int = 0,
              ldu: int = 0, x_off: int = 0, u_off: int = 0, x_copy=None, ld_copy: int = 0):
    """u[m, :r] = scale * drop(x[m]) A^T (cvar_lora_down); x_copy receives x unchanged in the same pass"""
    if A.dtype != x.dtype or u.dtype != x.dtype:
        raise TypeError('lora_down: x, A and u must share a dtype')
    es = x.element_size()
    check(_lib.load().cvar_lora_down(_ptr(x) + x_off * es, ldx or K, _ptr(A), lda or K, _ptr(u) + u_off * es, ldu or r, _ptr(x_copy), ld_copy or K,
                                     M, K, r, dt(x), float(scale), float(p), int(seed) & (2 ** 64 - 1), int(tag) & 0xffffffff, _stream()),
          'cvar_lora_down')
    return u


def lora_down_rows(x, A_bank, scale, slot, xa, *, R: int, l: int, K: int, kpad: int, ldx: int = 0, ldxa: int = 0, x_copy=None, ld_copy: int = 0,
                   xa_off: int = 0):
    """per-row adapters (cvar_lora_down_rows, include/cvar_serve.h): row m of the R * l rows of x uses slot[m // l] (-1: none).  A_bank
    (n_slots, 16, lda >= K) in x's dtype, scale (n_slots,) float32 and slot (R,) int32 contiguous on x's device.  Columns
    [K, K + kpad) of xa (+ xa_off elements) receive scale[s] x A_s^T in the slot's 16-column group and zeros everywhere else; x_copy
    receives x unchanged"""
    if A_bank.dtype != x.dtype or xa.dtype != x.dtype or (x_copy is not None and x_copy.dtype != x.dtype):
        raise TypeError('lora_down_rows: x, A_bank, xa and x_copy must share a dtype')
    if A_bank.ndim != 3 or A_bank.shape[1] != 16 or A_bank.stride(2) != 1 or A_bank.stride(0) != 16 * A_bank.stride(1):
        raise ValueError('lora_down_rows: A_bank must be (n_slots, 16, k) with dense 16-row slots')
    n = A_bank.shape[0]
    for name, t, dtype, shape in (('scale', scale, torch.float32, (n,)), ('slot', slot, torch.int32, (R,))):
        if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device):
            raise ValueError(f'lora_down_rows: {name} must be a contiguous {str(dtype)[6:]} {shape} tensor on {x.device}')
    check(_lib.load().cvar_lora_down_rows(_ptr(x), ldx or K, _ptr(A_bank), A_bank.stride(1), _ptr(scale), _ptr(slot), n, R, l,
                                          _ptr(xa) + xa_off * xa.element_size() if xa is not None else None, ldxa or (K + kpad), kpad, _ptr(x_copy),
                                          ld_copy or K, K, dt(x), _stream()), 'cvar_lora_down_rows')
    return xa


def lora_dx(dx, du, A, *, M: int, K: int, r: int, scale: float, p: float = 0.0, seed: int = 0, tag: int = 0, lddx: int = 0, lddu: int = 0,
            lda: int = 0, du_off: int = 0, aux=None, ldaux: int = 0):
    """dx = (dx + scale * drop'(du A)) * gelu'(aux) in place (cvar_lora_dx); du rows are 16 wide (lddu >= 16, a multiple of 8)"""
    if A.dtype != du.dtype or (aux is not None and aux.dtype != du.dtype):
        raise TypeError('lora_dx: du, A and aux must share a dtype')
    check(_lib.load().cvar_lora_dx(_ptr(dx), lddx or K, dt(dx), _ptr(du) + du_off * du.element_size(), lddu or 16, _ptr(A), lda or K, _ptr(aux),
                                   ldaux or K, M, K, r, dt(du), float(scale), float(p), int(seed) & (2 ** 64 - 1), int(tag) & 0xffffffff, _stream()),
          'cvar_lora_dx')
    return dx


def lora_wgrad_ws_floats(M: int, N: int) -> int:
    return int(_lib.load().cvar_lora_wgrad_ws_floats(M, N))


def lora_wgrad(Y, Z, out, ws, *, M: int, N: int, r: int, scale: float = 1.0, p: float = 0.0, seed: int = 0, tag: int = 0, ldy: int = 0,
               ldz: int = 0, y_off: int = 0, z_off: int = 0, out_off: int = 0, os_n: int = 0, os_j: int = 1, accumulate: bool = False):
    """fp32 out[n * os_n + j * os_j] = scale * sum_m drop(Y)[m, n] Z[m, j] (cvar_lora_wgrad; os_n defaults to r: an [N][r] matrix);
    accumulate: out becomes fp32(old + plain) (cvar_lora_wgrad_acc)"""
    if Y.dtype != Z.dtype:
        raise TypeError('lora_wgrad: Y and Z must share a dtype')
    if out.dtype != torch.float32 or ws.dtype != torch.float32:
        raise TypeError('lora_wgrad: out and ws are fp32')
    es = Y.element_size()
    if accumulate:
        check(_lib.load().cvar_lora_wgrad_acc(_ptr(Y) + y_off * es, ldy or N, _ptr(Z) + z_off * es, ldz or r, M, N, r, dt(Y), float(scale), float(p),
                                              int(seed) & (2 ** 64 - 1), int(tag) & 0xffffffff, _ptr(ws), ws.numel(), _ptr(out) + 4 * out_off,
                                              os_n or r, os_j, 1, _stream()), 'cvar_lora_wgrad_acc')
        return out
    check(_lib.load().cvar_lora_wgrad(_ptr(Y) + y_off * es, ldy or N, _ptr(Z) + z_off * es, ldz or r, M, N, r, dt(Y), float(scale), float(p),
                                      int(seed) & (2 ** 64 - 1), int(tag) & 0xffffffff, _ptr(ws), ws.numel(), _ptr(out) + 4 * out_off,
                                      os_n or r, os_j, _stream()), 'cvar_lora_wgrad')
    return out


def lora_dropout_mask(M: int, K: int, p: float, seed: int, tag: int, device=None) -> torch.Tensor:
    """(M, K) fp32 keep mask (1 / 0) of one target - exactly the bits the cvar_lora_* calls apply with the same (p, seed, tag)"""
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    out = torch.empty(M, K, device=dev, dtype=torch.float32)
    check(_lib.load().cvar_lora_dropout_mask(_ptr(out), M, K, float(p), int(seed) & (2 ** 64 - 1), int(tag) & 0xffffffff, _stream()),
          'cvar_lora_dropout_mask')
    return out
