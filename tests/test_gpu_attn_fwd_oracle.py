"""The inference attention forward (K/V arena + separate queries, q_off > 0, prescaled queries) on MI355X against the float64 oracle
of oracle/attn_ref.py (attention_cached_f64), in the per-(token, head)-row metric with a per-sample floor (attn_ref.row_error_fwd).

Paths: `prescaled` (cvar_attention_prescaled: the 128-query kernel, and the 64-query kernel where the dispatch rule picks it),
`mfma` (cvar_attention, bf16, unscaled queries), `rowwise_bf16`, `rowwise_f32` (the parity mode's kernel).  Cases: attn_ref.FWD_CASES,
1 - 12 at scale 0.125, 2 / 3 / 7 / 9 / 10 again at scale 1.0 (near one-hot rows; sample 3's first-tile shift is below -128), 13 (unit
norm keys, query norms 100 / 30 / 5 / 100) at scale 1.

Bounds - the factors of tests/test_gpu_attn_train_oracle.py.  bf16 kernels: 3 x max(bf16 emulation of the kernel's storage points,
1e-3); fp32 kernel: 4 x the same formula evaluated by torch in float32 on the CPU; lse: absolute, 3 x / 4 x its yardstick.  Both
yardsticks are distances from the float64 oracle, evaluated in the same test on the same operands, never taken from a kernel.
tests/test_attn_fwd_oracle_host.py holds what the bf16 bound rests on: the emulation is <= 5e-3 on every case, sample, scale and
query form (bound < 1.5e-2), and a forward that ignores every query's last visible key moves every sample of cases 2 - 12 by at
least two bounds (2.1e-2 .. 1.6 against bounds of 7e-3 .. 1e-2) while the whole-tensor metric of the older tests lets it through.

Measured on MI355X (gfx950) - row error of out and absolute error of lse against float64; yardstick = bf16 emulation (bf16 paths) or
torch float32 (rowwise_f32) on the same operands; ratio = kernel / yardstick, the bound is at ratio 3 (bf16, yardstick >= 1e-3) or 4 (fp32):
  case scale  path          out: kernel  yardstick ratio   lse: kernel  yardstick ratio
    1  0.125  prescaled     3.12e-03  1.80e-03   1.73   1.72e-06  6.87e-04   0.00
    1  0.125  mfma          1.78e-03  1.78e-03   1.00   2.42e-07  7.55e-04   0.00
    1  0.125  rowwise_bf16  1.78e-03  1.78e-03   1.00   7.11e-07  7.55e-04   0.00
    1  0.125  rowwise_f32   5.25e-07  5.16e-07   1.02   7.11e-07  1.95e-06   0.37
    2  0.125  prescaled     5.21e-03  2.52e-03   2.07   2.12e-06  9.49e-04   0.00
    2  0.125  mfma          2.59e-03  2.59e-03   1.00   2.62e-06  1.01e-03   0.00
    2  0.125  rowwise_bf16  2.59e-03  2.59e-03   1.00   3.46e-06  1.01e-03   0.00
    2  0.125  rowwise_f32   8.53e-07  8.63e-07   0.99   3.46e-06  3.46e-06   1.00
    3  0.125  prescaled     4.11e-03  2.86e-03   1.44   3.13e-06  7.92e-04   0.00
    3  0.125  mfma          2.83e-03  2.83e-03   1.00   2.57e-06  8.50e-04   0.00
    3  0.125  rowwise_bf16  2.83e-03  2.83e-03   1.00   2.57e-06  8.50e-04   0.00
    3  0.125  rowwise_f32   1.40e-06  1.29e-06   1.09   2.57e-06  2.57e-06   1.00
    4  0.125  prescaled     5.12e-03  2.76e-03   1.86   2.33e-06  7.89e-04   0.00
    4  0.125  mfma          2.82e-03  2.95e-03   0.96   3.34e-06  6.51e-04   0.01
    4  0.125  rowwise_bf16  2.82e-03  2.95e-03   0.96   2.64e-06  6.51e-04   0.00
    4  0.125  rowwise_f32   1.33e-06  1.35e-06   0.98   2.64e-06  2.64e-06   1.00
    5  0.125  prescaled     3.49e-03  2.71e-03   1.29   2.30e-06  6.99e-04   0.00
    5  0.125  mfma          2.81e-03  2.81e-03   1.00   1.92e-06  8.14e-04   0.00
    5  0.125  rowwise_bf16  2.81e-03  2.81e-03   1.00   1.92e-06  8.14e-04   0.00
    5  0.125  rowwise_f32   9.34e-07  9.74e-07   0.96   1.92e-06  1.92e-06   1.00
    6  0.125  prescaled     5.17e-03  2.87e-03   1.80   3.97e-06  6.83e-04   0.01
    6  0.125  mfma          2.67e-03  2.85e-03   0.94   2.93e-06  5.59e-04   0.01
    6  0.125  rowwise_bf16  2.67e-03  2.85e-03   0.94   2.29e-06  5.59e-04   0.00
    6  0.125  rowwise_f32   1.15e-06  1.14e-06   1.01   2.29e-06  2.31e-06   0.99
    7  0.125  prescaled     5.21e-03  2.90e-03   1.80   2.60e-06  5.21e-04   0.00
    7  0.125  mfma          3.22e-03  2.94e-03   1.10   3.53e-06  6.35e-04   0.01
    7  0.125  rowwise_bf16  3.22e-03  2.94e-03   1.10   2.39e-06  6.35e-04   0.00
    7  0.125  rowwise_f32   1.19e-06  1.16e-06   1.03   2.39e-06  2.89e-06   0.83
    8  0.125  prescaled     4.61e-03  2.99e-03   1.54   5.85e-06  3.81e-04   0.02
    8  0.125  mfma          2.93e-03  2.95e-03   0.99   7.28e-06  4.68e-04   0.02
    8  0.125  rowwise_bf16  2.93e-03  2.95e-03   0.99   3.34e-06  4.68e-04   0.01
    8  0.125  rowwise_f32   1.30e-06  1.44e-06   0.90   3.34e-06  3.34e-06   1.00
    9  0.125  prescaled     5.45e-03  2.92e-03   1.87   2.17e-06  1.03e-03   0.00
    9  0.125  mfma          2.92e-03  2.92e-03   1.00   3.20e-06  1.09e-03   0.00
    9  0.125  rowwise_bf16  2.92e-03  2.92e-03   1.00   2.86e-06  1.09e-03   0.00
    9  0.125  rowwise_f32   1.09e-06  1.18e-06   0.92   2.86e-06  2.86e-06   1.00
   10  0.125  prescaled     5.30e-03  2.74e-03   1.93   1.23e-06  8.52e-04   0.00
   10  0.125  mfma          3.35e-03  3.35e-03   1.00   2.22e-06  7.96e-04   0.00
   10  0.125  rowwise_bf16  3.35e-03  3.35e-03   1.00   2.24e-06  7.96e-04   0.00
   10  0.125  rowwise_f32   1.46e-06  1.32e-06   1.10   2.24e-06  2.24e-06   1.00
   11  0.125  prescaled     5.40e-03  2.38e-03   2.27   1.54e-05  1.44e-04   0.11
   11  0.125  rowwise_f32   1.64e-06  2.38e-06   0.69   3.00e-06  3.00e-06   1.00
   12  0.125  prescaled     5.90e-03  3.22e-03   1.83   5.27e-06  9.73e-04   0.01
    2  1      prescaled     4.94e-03  2.47e-03   2.00   1.75e-05  1.50e-03   0.01
    2  1      mfma          2.62e-03  2.62e-03   1.00   2.10e-05  1.42e-03   0.01
    2  1      rowwise_bf16  2.62e-03  2.62e-03   1.00   2.10e-05  1.42e-03   0.01
    2  1      rowwise_f32   6.44e-06  6.42e-06   1.00   2.10e-05  2.10e-05   1.00
    3  1      prescaled     5.81e-03  2.69e-03   2.16   2.50e-05  1.15e-03   0.02
    3  1      mfma          2.62e-03  2.74e-03   0.95   2.06e-05  1.22e-03   0.02
    3  1      rowwise_bf16  2.62e-03  2.74e-03   0.95   2.06e-05  1.22e-03   0.02
    3  1      rowwise_f32   6.19e-06  6.21e-06   1.00   2.06e-05  2.06e-05   1.00
    7  1      prescaled     5.02e-03  2.82e-03   1.78   1.52e-05  1.39e-03   0.01
    7  1      mfma          2.93e-03  2.92e-03   1.00   2.38e-05  1.29e-03   0.02
    7  1      rowwise_bf16  2.93e-03  2.92e-03   1.00   2.19e-05  1.29e-03   0.02
    7  1      rowwise_f32   6.90e-06  6.86e-06   1.01   2.19e-05  2.19e-05   1.00
    9  1      prescaled     5.66e-03  2.86e-03   1.98   1.72e-05  1.35e-03   0.01
    9  1      mfma          2.91e-03  3.07e-03   0.95   2.10e-05  1.39e-03   0.02
    9  1      rowwise_bf16  2.91e-03  3.07e-03   0.95   2.29e-05  1.39e-03   0.02
    9  1      rowwise_f32   1.43e-05  1.43e-05   1.00   2.29e-05  2.29e-05   1.00
   10  1      prescaled     4.86e-03  2.80e-03   1.73   1.39e-05  1.27e-03   0.01
   10  1      mfma          2.89e-03  2.89e-03   1.00   1.48e-05  1.17e-03   0.01
   10  1      rowwise_bf16  2.89e-03  2.89e-03   1.00   2.43e-05  1.17e-03   0.02
   10  1      rowwise_f32   6.38e-06  6.38e-06   1.00   2.43e-05  2.43e-05   1.00
   13  1      prescaled     5.47e-03  2.84e-03   1.93   6.36e-06  1.17e-03   0.01
   13  1      mfma          2.88e-03  2.84e-03   1.02   7.21e-06  1.25e-03   0.01
   13  1      rowwise_bf16  2.88e-03  2.84e-03   1.02   8.79e-06  1.25e-03   0.01
   13  1      rowwise_f32   4.28e-06  4.27e-06   1.00   8.79e-06  7.17e-06   1.23
The bf16 lse yardstick is the larger of the emulation's two lse variants - the row sum of the bf16-rounded P, ~1e-3 -; the kernels store the
fp32 row sum, hence their small ratios.  `prescaled` sits at 1.3 - 2.3 x the emulation in out where `mfma` sits at 1.0, most on the
spike sample (1) and on the near one-hot rows of scale 1: under the exact maximum the dominant P is 1 and rounds to itself, under the lazy
bf16 maximum it is 2^(s - m~) and takes a bf16 rounding of its own (<= 2^-9 of the whole row, which the fp32 row sum does not share).
Before the per-tile summation in attn_rowwise_kernel, rowwise_f32 measured on the spike sample: case 6 2.74e-06 (ratio 2.41), case 7 4.09e-06
(3.53), case 8 1.03e-05 (7.17, lse 1.11e-05 = 3.32), case 11 3.32e-05 (13.96, lse 3.40e-05 = 11.35): every P behind a late dominant key was
rounded away when it was added to a running sum near 1.
"""
import math

import pytest
import torch

from conftest import record
from oracle import attn_ref as A

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
PAD = 4096
# path -> (dtype, rowwise, prescaled, query form of the oracle)
PATHS = {'prescaled': (BF16, False, True, 'pre'), 'mfma': (BF16, False, False, 'raw'),
         'rowwise_bf16': (BF16, True, False, 'raw'), 'rowwise_f32': (F32, True, False, 'raw')}
ONLY = {11: ('prescaled', 'rowwise_f32'), 12: ('prescaled',)}
RUNS = [pytest.param(n, scale, path, id=f'case{n}-scale{scale:g}-{path}')
        for n, scale in A.FWD_RUNS for path in PATHS if path in ONLY.get(n, tuple(PATHS))]
_INPUTS, _REFS = {}, {}


def inputs(n, scale):
    if (n, scale) not in _INPUTS:
        _INPUTS.clear()                                 # one case at a time: case 12 holds 100 MB of fp32 operands
        _REFS.clear()
        R, H, Lmax, q_off, l, ends, holes = A.FWD_CASES[n]
        _INPUTS[n, scale] = A.fwd_case_inputs(n, scale) + (A.visibility_cached(q_off, l, ends, holes),)
    return _INPUTS[n, scale]


def refs(n, scale, form):
    """(case, scale, query form) -> query operand, float64 oracle and both yardsticks (bf16 emulation; float32 torch for the
    unscaled form), computed once for the paths that share them"""
    kv, q, qp, vis = inputs(n, scale)
    if (n, scale, form) not in _REFS:
        qq, s_mul = (qp, A.LN2) if form == 'pre' else (q, scale)
        out, lse = A.attention_cached_f64(qq, kv, s_mul, vis)
        out_e, lse_a, lse_b = A.attention_cached_emulated(qq, kv, s_mul, vis)
        yard = {BF16: dict(out=out_e, lse=max(float((lse_a - lse).abs().max()), float((lse_b - lse).abs().max())))}
        if form == 'raw':
            k, v = (t.float() for t in A.split_kv(kv[:, :vis.shape[1]]))
            s32 = (A.q_heads(q).float() @ k.transpose(-1, -2) * scale).masked_fill(~vis, -math.inf)
            yard[F32] = dict(out=A.heads_to_rows(torch.softmax(s32, -1) @ v), lse=float((torch.logsumexp(s32, -1).double() - lse).abs().max()))
        _REFS[n, scale, form] = (qq, out, lse, yard)
    return _REFS[n, scale, form]


def fenced(shape, dtype, dev, value=None):
    """(buffer, view): a tensor of `shape` between two NaN pads of PAD elements, itself NaN unless `value` is given"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), float('nan'), device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(value.to(dtype))
    return buf, view


def pads_intact(*bufs):
    return all(bool(torch.isnan(b[:PAD]).all()) and bool(torch.isnan(b[-PAD:]).all()) for b in bufs)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def worst_row(got, ref, R, H):
    """(sample, token, head) of the row row_error_fwd returns - what a failure names"""
    g, r = got.to(F64).reshape(R, -1, 64), ref.to(F64).reshape(R, -1, 64)
    rn = r.norm(dim=-1)
    e = (g - r).norm(dim=-1) / (rn + 5e-2 * rn.pow(2).mean(-1, keepdim=True).sqrt())
    i = int(torch.nan_to_num(e, nan=math.inf).flatten().argmax())
    return i // e.shape[1], (i % e.shape[1]) // H, i % H


@pytest.mark.parametrize('n,scale,path', RUNS)
def test_attention_cached_forward_rows(gpu_device, n, scale, path):
    """module docstring.  Every operand and output sits between NaN pads that must be intact afterwards, arena rows [q_off + l, Lmax)
    are NaN, out and lse are NaN before the call and finite in every element after it (a (query block, pair) the block-id mapping
    skipped would stay NaN); a second call is bit-identical.  Case 12: rows 0:2 of the R = 8 call (512 workgroups: the 64-query kernel)
    equal an R = 2 call (128 workgroups: the 128-query kernel) bit for bit, which carries the float64 bound over to that kernel."""
    dtype, rowwise, prescaled, form = PATHS[path]
    R, H, Lmax, q_off, l, ends, holes = A.FWD_CASES[n]
    C = H * 64
    kv = inputs(n, scale)[0]
    qq, ex_out, ex_lse, yard = refs(n, scale, form)
    y = yard[dtype]
    factor = 3 if dtype == BF16 else 4
    failures = []

    ab, arena = fenced((R, Lmax, 2 * C), dtype, gpu_device)
    arena[:, :q_off + l] = kv[:, :q_off + l].to(dtype).to(gpu_device)
    qb, qd = fenced((R * l, C), dtype, gpu_device, qq.view(R * l, C))
    assert torch.equal(qd.cpu().float(), qq.view(R * l, C)), 'the operands are bf16 values: the kernel sees what the oracle sees'

    def call(arena_, q_, R_):
        ob, out = fenced((R_ * l, C), dtype, gpu_device)
        lb, lse = fenced((R_, H, l), F32, gpu_device)
        ops.attention(arena_, out, R_, H, Lmax, q_off, l, scale, ends, rowwise=rowwise, lse=lse, holes=holes, q=q_, prescaled=prescaled)
        return ob, out, lb, lse

    ob, out, lb, lse = call(arena, qd, R)
    assert pads_intact(ab, qb, ob, lb)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()), 'every element of out and lse must be written, and finite'
    got, got_lse = out.cpu(), lse.cpu().double()
    # ---- rows of out
    err, per = A.row_error_fwd(got, ex_out, R)
    yerr, yper = A.row_error_fwd(y['out'], ex_out, R)
    limit = factor * max(yerr, 1e-3) if dtype == BF16 else factor * yerr
    what = f'case {n} scale {scale:g} {path}'
    print(f'[attn_fwd_rows] {what} out: kernel {err:.3e}  yardstick {yerr:.3e}  bound {limit:.3e}  ratio {err / yerr:.2f}  per sample '
          + ' '.join(f'{v:.2e}' for v in per))
    record(f'{what} out', kind='attn_fwd_rows', kernel=err, yardstick=yerr, bound=limit, per_sample=per, yardstick_per_sample=yper,
           case=n, scale=scale, path=path, tensor='out')
    if not err <= limit:
        failures.append(('out', err, limit, 'worst (sample, token, head)', worst_row(got, ex_out, R, H)))
    # ---- lse, absolute
    lse_per = [float(v) for v in (got_lse - ex_lse).abs().amax((1, 2))]
    lse_err, lse_limit = max(lse_per), factor * y['lse']
    print(f'[attn_fwd_rows] {what} lse (absolute): kernel {lse_err:.3e}  yardstick {y["lse"]:.3e}  bound {lse_limit:.3e}  ratio {lse_err / y["lse"]:.2f}')
    record(f'{what} lse (absolute)', kind='attn_fwd_rows', kernel=lse_err, yardstick=y['lse'], bound=lse_limit, per_sample=lse_per,
           case=n, scale=scale, path=path, tensor='lse')
    if not lse_err <= lse_limit:
        failures.append(('lse', lse_err, lse_limit))
    # ---- a second call: fixed summation order
    ob2, out2, lb2, lse2 = call(arena, qd, R)
    assert pads_intact(ab, qb, ob2, lb2)
    if not (torch.equal(bits(out2), bits(out)) and torch.equal(bits(lse2), bits(lse))):
        failures.append(('a second call is not bit-identical',))
    if n == 12:
        a2, q2 = arena[:2].contiguous(), qd[:2 * l].contiguous()
        ob3, out3, lb3, lse3 = call(a2, q2, 2)
        assert pads_intact(ob3, lb3) and bool(torch.isfinite(out3).all())
        if not (torch.equal(bits(out3), bits(out[:2 * l])) and torch.equal(bits(lse3), bits(lse[:2]))):
            failures.append(('the 64-query kernel (R = 8) and the 128-query kernel (R = 2) differ on rows 0:2',))
    assert not failures, failures
