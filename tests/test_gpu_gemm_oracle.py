"""cvar_gemm on MI355X, plain GEMM: every kernel route and every epilogue implementation against the float64 oracle of oracle/gemm_ref.py, element by
element, at the bounds derived there (tests/test_gemm_oracle_host.py shows on the CPU that a float32 model of the kernels' arithmetic sits at <= 0.5
of them and that planted faults land outside).  Every call goes through controlvar_amd.ops.gemm.  Operands, outputs, bias, gate, gate_scale, residual,
aux, pre_act and C_split lie between NaN pads, inside NaN rows where a leading dimension exceeds the width; outputs are NaN before the call.  After it
every element the call owns is within its bound (a NaN fails), every element it does not own is still NaN (pads, columns beyond N, arena rows outside
the remap, rows >= M) and every input is unchanged bit for bit, except a residual that is updated in place.  Every comparison is recorded
(kind = 'gemm_oracle') and asserted at ratio <= 1.

Routes (oracle/gemm_ref.CASES names one per case; shapes are the smallest that reach it by launch_typed / cvar_gemm; K % 64 == 0 (fp32: % 32) runs the
DMA-fast K loop - template argument FAST below - and K % 8 == 0 (% 4) only the any-K loop).  Kernel names as a kernel trace of this module showed them
(one profiler run of its own, no counters; every case launched the kernel of its row, 132 launches for 111 cases); T = unsigned short (bf16) or float:
  64x128            M = 37 (36 with a remap), unsliced                      cvar_gemm_kernel<T, 64, 128, 1, 4, false, 2, FAST, false>
  128x128 w8        M = 300                                                 cvar_gemm_kernel<bf16, 128, 128, 2, 4, false, 2, FAST, false>
  128x128 w4        tile_cfg 26 (fp32 operands: always)                     cvar_gemm_kernel<T, 128, 128, 2, 2, false, 2, FAST, false>
  128x128 s3 / s4   tile_cfg 13 / 14                                        cvar_gemm_kernel<bf16, 128, 128, 2, 4, false, 3, ...> / <bf16, 128, 128, 2, 2, false, 4, ...>
  256x256 w8        M = 2085, N = 256, tile_cfg 2 (28: register RMW)        cvar_gemm_kernel<T, 256, 256, 2, 4, false, 2, FAST, false>
  256x256 w4        tile_cfg 3                                              cvar_gemm_kernel<bf16, 256, 256, 2, 2, false, 2, FAST, false>
  256x192           tile_cfg 27, N = 384 and N = 200 (partial column tile)  cvar_gemm_kernel<bf16, 256, 192, 4, 2, false, 2, FAST, false>
  128x160           M = 4100, N = 320                                       cvar_gemm_kernel<T, 128, 160, 4, 1, false, 2, FAST, false>
  split-K           workspace passed, M = 36 / 300, N = 256, K = 512 / 1536 (fp32: K = 256)    the 64x128 / 128x128 tile, FAST + cvar_splitk_epilogue_kernel
  split-K long      M = 1152, N = 1536, K = 1536                            cvar_gemm_kernel<bf16, 256, 256, 2, 2, false, 2, true, false> + cvar_splitk_epilogue_kernel
  stream mt x nt    small_m, M = 4 / 24 / 40 (N = 4096: nt = 2), M = 100: two row groups       cvar_gemm_skinny_kernel<mt, nt, false>
  stream sliced     small_m, M = 40, N = 64, K = 4096                       cvar_gemm_skinny_kernel<4, 1, true> + cvar_splitk_epilogue_kernel
  rowfin stream     ln=, small_m, M = 16, N = 192, K = 1024 (two slices)    cvar_gemm_skinny_kernel<1, 1, true> + cvar_splitk_rowfin_kernel<bf16, 1, true>
  rowfin tiles      ln=, M = 300, K = 1536, N = 192 / 320; M = 36, N = 512  128x128 / 64x128 tile + cvar_splitk_rowfin_kernel<bf16, 1, true> / <bf16, 2, true> / <bf16, 2, false>
Epilogue implementations (a branch inside the kernel, invisible to a trace; the mutants below show that the named one ran): spec - the compile-time variants
of the 128x160 / 256x192 / 256x256 bf16 tiles; rpf - their LDS-prefetched read-modify-write (tile_cfg 2, full tiles; the 37-row tile of the same launch runs
the register form); vector / scalar - the generic forms (scalar: N = 100, ldc = N + 4, a bias one float past a 16-byte boundary, ldg % 4 != 0, and a batch
stride off the 8-element grid); quad - gemm_epilogue_quad behind split-K and in the streaming kernel; rowfin - cvar_splitk_rowfin_kernel (x is checked
here, the modulated rows by test_gemm_with_the_adaln_of_the_next_op_is_bit_identical_to_two_calls).

Largest error / bound measured on MI355X per route, implementation and written tensor.  bf16 tensors sit near 1 by construction: their store term is the
worst case of the rounding itself (half an ulp of the value's binade; see oracle/gemm_ref.py for why 2^-9 |value| would refuse a correct rounding).
  64x128          vector       C bf16 0.998  C f32 0.311  C_split f32 0.029  pre_act bf16 0.997
  128x128 w8      vector       C bf16 0.998  C f32 0.318  C_split bf16 0.996  pre_act bf16 0.996
  128x128 w4      vector       C bf16 0.997  C f32 0.317          128x128 s3  vector  C bf16 0.996          128x128 s4  vector  C f32 0.027
  256x256 w8      spec         C bf16 0.999  C f32 0.458  C_split bf16 0.998  pre_act bf16 0.998          rpf  C f32 0.333
  256x256 w4      spec         C f32 0.422          256x192  spec  C bf16 0.999  C f32 0.434
  128x160         spec         C bf16 0.998  C f32 0.411  C_split bf16 0.998  pre_act bf16 0.999
  256x256 w8      vector       C bf16 0.999  C f32 0.034  C_split f32 0.032          256x256 w4  vector  C f32 0.130          256x192  vector  C bf16 0.9998
  128x128 w8      scalar       C bf16 0.997  C f32 0.394  C_split bf16 0.996  pre_act bf16 0.997
  64x128          scalar       C bf16 0.995  C_split bf16 0.996  pre_act bf16 0.997          256x256 w8  scalar  C f32 0.093  C_split f32 0.033
  split-K         quad         C bf16 0.995  C f32 0.284  C_split bf16 0.994  C_split f32 0.004  pre_act bf16 0.992          split-K long  C bf16 0.987
  stream          quad         1x1 C bf16 0.994, f32 0.030   2x1 C bf16 0.997   4x1 C bf16 0.988, f32 0.079, C_split bf16 0.996   4x2 C f32 0.046
                               sliced C bf16 0.932   two row groups C f32 0.150
  rowfin          stream producer C f32 0.055   tile producer C f32 0.078
  fp32 operands   64x128 0.082   128x128 C 0.058, C_split 0.028, pre_act 0.031, scalar 0.045   128x160 0.059   256x256 0.441   split-K 0.075
  (fp32 outputs near 0.4: gate + residual cases, where a gate near 0 leaves the residual add's rounding as the whole error)

The bug this module was written around: the scalar generic epilogue dropped split_alpha.  On the library built from the commit before the fix the cases
scalar-bias-split, scalar-bias-split-256 and scalar-stride-split fail (C_split off by the factor 0.18) and the other 108 pass; with the fix all 111 pass.
Both observed on MI355X.
Kernel mutants (arithmetic only, one build each, never committed).  All six fail this module; beside it, tests/test_gpu_kernels.py and tools/fuzz_gemm.py 60 3:
  split_alpha dropped in gemm_epilogue_quad        here: splitk-remap-split, splitk-remap-split-f32, stream-remap-split      test_gpu_kernels: seen   fuzz: missed
  the RPF gate fetched for row m + 16              here: rpf-gate100                                                         test_gpu_kernels: seen   fuzz: missed
  gate_scale dropped in the specialised variant    here: spec-gatescale, spec-gate-160                                       test_gpu_kernels: missed fuzz: missed
  pre_act stored after GELU, generic vector form   here: vec-pre-gelu                                                        test_gpu_kernels: missed fuzz: missed
  the last 8-wide K chunk skipped, any-K loop      here: 21 cases (every K % 64 != 0 bf16 tile case)                         test_gpu_kernels: seen   fuzz: seen
  the row finish adding the bias after the gate    here: rowfin-stream-N192, rowfin-tile-N192, rowfin-tile-N320              test_gpu_kernels: seen   fuzz: missed
  (rowfin-tile-N512 has no bias and cannot see the last one.)
"""
import math

import numpy as np
import pytest
import torch

from conftest import record
from oracle import gemm_ref as G

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
TD = {'f32': F32, 'bf16': BF16}
PAD = 4096
NAN = float('nan')


def fenced(n, dtype, dev, lead=0):
    """(buffer, view): `n` NaN elements between two NaN pads; lead: elements the view starts past the 16-byte aligned end of the first pad"""
    buf = torch.full((n + lead + 2 * PAD,), NAN, device=dev, dtype=dtype)
    return buf, buf[PAD + lead:PAD + lead + n]


def put_rows(view, vals, ld, dtype):
    """vals [..., rows, cols] -> rows of leading dimension ld in the flat view; the columns beyond stay NaN"""
    v = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32)).reshape(-1, vals.shape[-1])
    host = torch.full((v.shape[0], ld), NAN, dtype=dtype)
    host[:, :v.shape[1]] = v.to(dtype)
    view.copy_(host.reshape(-1))


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32}[t.dtype]).cpu()


def pads_nan(buf, view):
    lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    return bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())


def host64(view, *shape):
    return view.detach().cpu().double().numpy().reshape(*shape)


def padded(vals, ld):
    """[..., rows, cols] float64 -> [..., rows, ld] with NaN in the columns nobody owns"""
    out = np.full(vals.shape[:-1] + (ld,), np.nan)
    out[..., :vals.shape[-1]] = vals
    return out


def run_case(c, dev):
    """-> {tensor: memory image as float64} of everything the call may write, after checking pads and inputs"""
    o = G.operands(c)
    dt, odt = TD[c.dt], TD[c.out]
    B, M, N, K = c.batch, c.M, c.N, c.K
    n_rows = G.c_rows(c)
    inputs, outputs = {}, {}

    def new_input(name, n, dtype, lead=0):
        inputs[name] = fenced(n, dtype, dev, lead)
        return inputs[name][1]

    put_rows(new_input('A', B * M * c.lda, dt), o.A, c.lda, dt)
    put_rows(new_input('W', N * K, dt), o.W, K, dt)
    kw = dict(M=M, N=N, K=K, lda=c.lda, ldc=c.ldc, alpha=c.alpha, act=c.act, batch=B, split_k=c.split_k, small_m=c.small_m)
    if c.bias:
        kw['bias'] = new_input('bias', N, F32, lead=1 if c.bias_mis else 0)
        kw['bias'].copy_(torch.from_numpy(o.bias))
        assert kw['bias'].data_ptr() % 16 == (4 if c.bias_mis else 0)
    if c.gate_rows:
        table = o.gate.copy()
        if not c.ln:                                   # only the gate's own columns of the wider table hold numbers
            table[:, :c.gate_off] = np.nan
            table[:, c.gate_off + N:] = np.nan
        gate = new_input('gate', table.size, F32)
        gate.copy_(torch.from_numpy(table).reshape(-1))
        kw.update(gate=gate, gate_off=c.gate_off, ldg=c.ldg, gate_rows=c.gate_rows)
        if c.gate_scale:
            kw['gate_scale'] = new_input('gate_scale', G.groups(c), F32)
            kw['gate_scale'].copy_(torch.from_numpy(o.gate_scale))
    outputs['C'] = fenced(B * n_rows * c.ldc, odt, dev)
    if c.res:
        if c.inplace:
            put_rows(outputs['C'][1], o.res, c.ldr, odt)
            kw.update(residual=outputs['C'][1], ldr=c.ldr)
        else:
            put_rows(new_input('residual', B * M * c.ldr, TD[c.res]), o.res, c.ldr, TD[c.res])
            kw.update(residual=inputs['residual'][1], ldr=c.ldr)
    if c.act == G.ACT_GELU_GRAD:
        put_rows(new_input('aux', B * M * c.ldc, odt), o.aux, c.ldc, odt)
        kw['aux'] = inputs['aux'][1]
    if c.pre_act:
        outputs['pre_act'] = fenced(B * M * c.ldc, dt, dev)
        kw['pre_act'] = outputs['pre_act'][1]
    if c.remap:
        kw['remap'] = c.remap
    if c.split_n:
        outputs['C_split'] = fenced(M * c.ld_split, odt, dev)
        kw.update(split=(outputs['C_split'][1], c.split_n, c.ld_split), split_alpha=c.split_alpha)
    if c.ln:
        outputs['ln_out'] = fenced(M * N, BF16, dev)
        kw['ln'] = (outputs['ln_out'][1], inputs['gate'][1], 3 * N, 5 * N, c.ldg, c.gate_rows, o.ln_eps)
    if B > 1:
        kw.update(strideA=M * c.lda, strideW=0, strideC=n_rows * c.ldc, strideR=M * c.ldr)
    if c.stride_c_odd:
        kw['strideC'] = 4
    before = {k: bits(buf) for k, (buf, _) in inputs.items()}
    ops.ensure_splitk_workspace(dev)
    old = ops.GEMM_TILE_CFG
    ops.GEMM_TILE_CFG = c.tile_cfg
    try:
        ops.gemm(inputs['A'][1], inputs['W'][1], outputs['C'][1], **kw)
        torch.cuda.synchronize()
    finally:
        ops.GEMM_TILE_CFG = old
    for k, (buf, _) in inputs.items():
        assert torch.equal(bits(buf), before[k]), f'{c.name}: {k} (or its pads) was written'
    for k, pair in outputs.items():
        assert pads_nan(*pair), f'{c.name}: the pads of {k} were written'
    got = {'C': host64(outputs['C'][1], B, n_rows, c.ldc)}
    if c.split_n:
        got['C_split'] = host64(outputs['C_split'][1], M, c.ld_split)
    if c.pre_act:
        got['pre_act'] = host64(outputs['pre_act'][1], B, M, c.ldc)
    if c.ln:
        assert not bool(torch.isnan(outputs['ln_out'][1].float()).any()), f'{c.name}: modulated rows missing'
    return got


def expected(c):
    """{tensor: (reference image, bound image)}: NaN where the call owns nothing"""
    ev = G.evaluate(c)
    exp = {'C': (G.image(c, ev.C)[0], G.image(c, ev.C_bound)[0])}
    if c.split_n:
        exp['C_split'] = (padded(ev.Cs, c.ld_split), padded(ev.Cs_bound, c.ld_split))
    if c.pre_act:
        exp['pre_act'] = (padded(ev.pre, c.ldc), padded(ev.pre_bound, c.ldc))
    return exp


@pytest.mark.parametrize('name', list(G.CASES))
def test_gemm_elements(gpu_device, name):
    c = G.CASES[name]
    exp = expected(c)
    got = run_case(c, gpu_device)
    failures = []
    for tensor, (ref, bnd) in exp.items():
        g = got[tensor]
        assert g.shape == ref.shape, (name, tensor, g.shape, ref.shape)
        owned = ~np.isnan(ref)
        stray = int((~np.isnan(g) & ~owned).sum())              # written where the call owns nothing
        missing = int((np.isnan(g) & owned).sum())
        err = G.abs_err(g, ref)
        ratio = G.ratio_of(err[owned], bnd[owned])
        fin = err[owned][np.isfinite(err[owned])]
        worst = float(fin.max()) if fin.size else math.inf
        print(f'[gemm_oracle] {name:28s} {c.route:16s} {c.impl:12s} {tensor:8s} kernel {worst:.3e}  bound {float(np.nanmax(bnd)):.3e}  ratio {ratio:.3f}'
              f'  stray {stray}  missing {missing}')
        record(f'gemm {name} {tensor}', kind='gemm_oracle', case=name, route=c.route, impl=c.impl, tensor=tensor, out=(c.dt if tensor == 'pre_act' else c.out),
               kernel=worst if math.isfinite(worst) else None, bound=float(np.nanmax(bnd)), ratio=ratio if math.isfinite(ratio) else None, stray=stray, missing=missing)
        if not ratio <= 1.0 or stray or missing:
            failures.append((tensor, ratio, stray, missing))
    assert not failures, (name, c.route, c.impl, failures)
