"""cvar_ln_modulate, cvar_ln_modulate_bwd, cvar_gated_grad, cvar_groupnorm_silu and cvar_groupnorm_silu_partials on MI355X against the float64
oracles of oracle/norm_ref.py, element by element, at the bounds stated there (tests/test_norm_oracle_host.py shows on the CPU that models of
the kernels' arithmetic sit at <= 0.5 of them and that planted faults overshoot them >= 10 x).  The cases name every NV / TAIL instantiation
of the row kernels, the segment edges of the per-sequence reductions and the chunk / lane edges of the GroupNorm passes.

Every operand and output lies between NaN pads; outputs, the workspace and the untouched columns of dada / dgate are NaN before the call.
The workspace then shows which path ran: the one-pass LayerNorm backward leaves the row-statistics area NaN, the two-kernel form fills it with
(mean, rstd); the partial area holds exactly `segments` x R rows of finite sums.  Every comparison is recorded (kind = 'norm_oracle').

Largest error / bound measured on MI355X (a bf16 output sits at 0.99 by construction: the 2^-8 |y| term is the worst case of its rounding):
  ln_modulate              fp32 0.27 (one 1e4 outlier per row)   bf16 0.995
  ln_modulate_bwd  bf16    dx 0.056  dscale 0.080  dshift 0.069  (one-pass kernel);  saved mean 0.02, rstd 0.25 of 2^-21 (two-kernel forms)
  ln_modulate_bwd  fp32    dx 0.051  dscale 0.062  dshift 0.169;  saved mean 0.31, rstd 0.23
  gated_grad               df fp32 0.25, bf16 0.996;  dgate 0.25 (bf16), 0.14 (fp32)
  groupnorm_silu           fp32 0.36 (HW = 31), with SiLU 0.14;  K_g ~ 100: 0.023;  bf16 0.996
  groupnorm_silu_partials  bf16 0.996
Kernel mutants (arithmetic only, never committed) that these tests catch: the row tail left out of the mean, the variance divided by NV 256, eps
dropped in LayerNorm (only the small-variance rows show it; the earlier suite does not) and in GroupNorm, mean(g xhat) dropped and one segment's
partial zeroed in the one-pass backward, the cross term of the tile partials halved, one channel's dgate partial off by 1e-4 (the earlier suite
does not)."""
import math

import numpy as np
import pytest
import torch

from conftest import record
from oracle import norm_ref as N

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402
from controlvar_amd._lib import CvarError  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
TD = {'f32': F32, 'bf16': BF16}
PAD = 4096
_REFS = {}


def once(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def fenced(shape, dtype, dev, value=None, shift=0):
    """(buffer, view): a tensor of `shape` between two NaN pads of >= PAD elements, `shift` elements off the pad's end, NaN unless `value` is given"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD + shift,), float('nan'), device=dev, dtype=dtype)
    view = buf[PAD + shift:PAD + shift + n].view(*shape)
    if value is not None:
        view.copy_(torch.as_tensor(value).to(dtype))
    return buf, view


def pads_intact(*pairs):
    """every element of the buffers outside their views is still NaN"""
    for buf, view in pairs:
        lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        if not (bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())):
            return False
    return True


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def host(t):
    return t.detach().cpu().double().numpy()


class Checks:
    def __init__(self, what, **kw):
        self.what, self.kw, self.failures = what, kw, []

    def add(self, tensor, got, ref, bound, yardstick=0.0, **kw):
        """got within `bound` of `ref` element by element (NaN in got fails)"""
        err = np.abs(got - ref)
        ratio = N.ratio_of(np.where(np.isfinite(err), err, np.inf), bound)
        print(f'[norm_oracle] {self.what} {tensor}: kernel {float(np.nanmax(err)):.3e}  yardstick {float(np.max(yardstick)):.3e}  '
              f'bound {float(np.max(bound)):.3e}  ratio {ratio:.3f}')
        record(f'{self.what} {tensor}', kind='norm_oracle', tensor=tensor, kernel=float(np.nanmax(err)), yardstick=float(np.max(yardstick)),
               bound=float(np.max(bound)), ratio=ratio, **self.kw, **kw)
        if not ratio <= 1.0:
            self.failures.append((tensor, ratio))

    def done(self):
        assert not self.failures, (self.what, self.failures)


# ================================================================================================ ln_modulate
def ln_fwd_refs(n):
    def make():
        C, M, rp, fam, ld0 = N.LN_FWD_CASES[n]
        x, s, b = N.ln_fwd_inputs(n)
        return x, s, b, N.ln_forward(x, s, b, rp), N.ln_forward(x, s, b, rp, dtype=np.float32).y
    return once(('lnf', n), make)


@pytest.mark.parametrize('out_dtype', ['f32', 'bf16'])
@pytest.mark.parametrize('n', list(N.LN_FWD_CASES), ids=N.ln_fwd_name)
def test_ln_modulate_rows(gpu_device, n, out_dtype):
    """4 E_m per row (+ half a bf16 ulp); a constant row whose fp32 mean is exact must come out as exactly the shift"""
    C, M, rp, fam, ld0 = N.LN_FWD_CASES[n]
    x, s, b, ex, y32 = ln_fwd_refs(n)
    G = s.shape[0]
    xp, ap = fenced((M, C), F32, gpu_device, x), fenced((G, 2 * C), F32, gpu_device, torch.cat([s, b], 1))
    op = fenced((M, C), TD[out_dtype], gpu_device)
    ops.ln_modulate(xp[1], ap[1], 0, C, 0 if ld0 else 2 * C, rp, op[1], M, C, N.EPS)
    assert pads_intact(xp, ap, op)
    bd = N.ln_fwd_bound(ex, y32, x, s, rp, out_dtype == 'bf16')
    ck = Checks(f'ln_modulate {N.ln_fwd_name(n)} {out_dtype}', op='ln_modulate', dtype=out_dtype, case=n)
    ck.add('y', host(op[1]), ex.y, bd.bound * np.ones_like(ex.y), bd.E)
    if fam == 'const_row':
        for m in range(M):
            if m % 4 < 2:            # 1.5 C and 2.25 C are exact in fp32, so is the mean: xhat = 0 and y = b
                want = b[0 if ld0 else m // rp].to(TD[out_dtype]).to(gpu_device)
                assert torch.equal(bits(op[1][m]), bits(want)), f'constant row {m} (x = {N.CONST_ROW_VALUES[m % 4]}) must give exactly the shift'
    ck.done()


def test_ln_modulate_refuses_without_writing(gpu_device):
    """C % 4, C > 2048 and ld_ada % 4 are CVAR_EUNSUPPORTED (-2) before any launch"""
    for C, ld in ((130, 260), (2052, 4104), (128, 258)):
        xp, ap, op = fenced((3, C), F32, gpu_device, torch.ones(3, C)), fenced((3, ld), F32, gpu_device, torch.zeros(3, ld)), fenced((3, C), BF16, gpu_device)
        with pytest.raises(CvarError, match=r'\(-2\)'):
            ops.ln_modulate(xp[1], ap[1], 0, C, ld, 1, op[1], 3, C, N.EPS)
        torch.cuda.synchronize()
        assert bool(torch.isnan(op[0]).all())


# ================================================================================================ ln_modulate_bwd
def ln_bwd_refs(n):
    def make():
        C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
        x, dy, s, dx_in = N.ln_bwd_inputs(n)
        return x, dy, s, dx_in, N.ln_backward(x, dy, s, dx_in, R, l), N.ln_backward(x, dy, s, dx_in, R, l, dtype=np.float32)
    return once(('lnb', n), make)


def ws_shift(n):
    """floats the workspace is moved off its 16-byte boundary: 2 (8 bytes; the entry point accepts it, the vector forms of the column sums and the
    one-pass kernel decline) for the bf16 cases that name a scalar column kernel at a width the vector kernels would serve"""
    C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
    return 2 if dt == 'bf16' and path in ('vec+col', 'row+col') and C % 4 == 0 else 0


def run_ln_bwd(n, dev, mode='separate', operands=None):
    """-> dx, dada, ws (views) of case n (on the operands of case `operands`); mode: how dx_in is passed (separate | inplace | none)"""
    C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
    M = R * l
    x, dy, s, dx_in, ex, y32 = ln_bwd_refs(operands or n)
    ada = torch.full((R, 6 * C), float('nan'))
    ada[:, 2 * C:3 * C] = s
    xp, yp, ap = fenced((M, C), F32, dev, x), fenced((M, C), TD[dt], dev, dy), fenced((R, 6 * C), F32, dev, ada)
    dp = fenced((M, C), F32, dev, dx_in if mode == 'inplace' else None)
    ip = fenced((M, C), F32, dev, dx_in) if mode == 'separate' else None
    gp = fenced((R, 6 * C), F32, dev)
    wp = fenced((ops.train_ws_floats(M, R, C),), F32, dev, shift=ws_shift(n))
    src = {'separate': ip[1] if ip else None, 'inplace': dp[1], 'none': None}[mode]
    ops.ln_modulate_bwd(xp[1], yp[1], ap[1], 2 * C, 6 * C, l, src, dp[1], gp[1], 3 * C, 5 * C, 6 * C, M, C, N.EPS, wp[1])
    assert pads_intact(xp, yp, ap, dp, gp, wp) and (ip is None or pads_intact(ip))
    return dp[1], gp[1], wp[1]


@pytest.mark.parametrize('n', list(N.LN_BWD_CASES), ids=N.ln_bwd_name)
def test_ln_modulate_bwd_rows_sums_and_path(gpu_device, n):
    C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
    M = R * l
    x, dy, s, dx_in, ex, y32 = ln_bwd_refs(n)
    ck = Checks(f'ln_modulate_bwd {N.ln_bwd_name(n)}', op='ln_modulate_bwd', dtype=dt, case=n, path=path)
    dx, dada, ws = run_ln_bwd(n, gpu_device)
    # ---- which path ran: the workspace
    w = ws.cpu()
    sf, nseg = N.ln_stats_floats(M), N.ln_bwd_segments(n)
    stats, partial = w[:2 * M], w[sf:]
    assert bool(torch.isnan(w[2 * M:sf]).all())
    if path == 'fused':
        assert bool(torch.isnan(stats).all()), 'the one-pass kernel writes no row statistics: the call fell back to the two-kernel form'
    else:
        assert bool(torch.isfinite(stats).all()), 'the two-kernel form stores (mean, rstd) of every row: the one-pass kernel ran instead'
        st = stats.double().numpy().reshape(M, 2)
        ck.add('mean', st[:, 0], ex.mean, 2.0 ** -21 * np.abs(N.as_np(x)).max(1))
        ck.add('rstd', st[:, 1], ex.rstd, 2.0 ** -21 * ex.rstd)
    used = nseg * R * 2 * C
    assert bool(torch.isfinite(partial[:used]).all()) and bool(torch.isnan(partial[used:]).all()), f'expected {nseg} row segments of partial sums'
    # ---- values
    bx = N.ln_bwd_dx_bound(ex, y32.dx, x, dx_in)
    ck.add('dx', host(dx), ex.dx, bx.bound, bx.yard)
    dyn = N.as_np(dy)
    bs = N.colsum_bound(ex.dscale, y32.dscale, np.abs(dyn * ex.xhat), R, l, N.dscale_factor(ex, x, R, l))
    bh = N.colsum_bound(ex.dshift, y32.dshift, np.abs(dyn), R, l)
    g = dada.cpu()
    ck.add('dscale', host(g[:, 3 * C:4 * C]), ex.dscale, bs.bound, bs.yard)
    ck.add('dshift', host(g[:, 5 * C:]), ex.dshift, bh.bound, bh.yard)
    assert bool(torch.isnan(g[:, :3 * C]).all()) and bool(torch.isnan(g[:, 4 * C:5 * C]).all()), 'columns of dada outside d scale / d shift were written'
    # ---- dx_in in place: the same bits; no dx_in: the bare LayerNorm gradient
    acc, dada2, _ = run_ln_bwd(n, gpu_device, 'inplace')
    assert torch.equal(bits(acc), bits(dx)) and torch.equal(bits(dada2[:, 3 * C:4 * C]), bits(dada[:, 3 * C:4 * C]))
    dx0, _, _ = run_ln_bwd(n, gpu_device, 'none')
    b0 = N.ln_bwd_dx_bound(ex, y32.dx0, x, None)
    ck.add('dx without dx_in', host(dx0), ex.dx0, b0.bound, b0.yard)
    ck.done()


def test_ln_bwd_column_kernels_share_their_bits_at_equal_segments(gpu_device):
    """ln_bwd_col_vec_kernel promises ln_bwd_col_kernel's per-channel order: at C = 2304, (R, l) = (2, 30) both cut 8 segments (cases 48 / 49: the
    workspace 8 bytes off a 16-byte boundary sends the same call to the scalar column kernel), fed by the same row kernel"""
    a, b = (n for n, c in N.LN_BWD_CASES.items() if c[:3] == (2304, 2, 30))
    assert N.ln_bwd_segments(a) == N.ln_bwd_segments(b) == N.RED_S and ws_shift(a) == 0 and ws_shift(b) == 2
    C = 2304
    dx_a, dada_a, _ = run_ln_bwd(a, gpu_device)
    dx_b, dada_b, _ = run_ln_bwd(b, gpu_device, operands=a)
    assert torch.equal(bits(dx_a), bits(dx_b))
    assert torch.equal(bits(dada_a[:, 3 * C:4 * C]), bits(dada_b[:, 3 * C:4 * C])) and torch.equal(bits(dada_a[:, 5 * C:]), bits(dada_b[:, 5 * C:]))


# ================================================================================================ gated_grad
@pytest.mark.parametrize('n', list(N.GG_CASES), ids=N.gg_name)
def test_gated_grad_elements_sums_and_path(gpu_device, n):
    C, R, l, dt, form = N.GG_CASES[n]
    M = R * l
    dx, f, gate, rs = N.gg_inputs(n)
    ex, y32 = N.gated_grad(dx, f, gate, rs, R, l), N.gated_grad(dx, f, gate, rs, R, l, dtype=np.float32)
    xp, fp, gp = fenced((M, C), F32, gpu_device, dx), fenced((M, C), TD[dt], gpu_device, f), fenced((R, C), F32, gpu_device, gate)
    rp = fenced((R,), F32, gpu_device, rs) if rs is not None else None
    dfp = fenced((M, C), TD[dt], gpu_device, shift=1 if form == 'scalar_df_off' else 0)
    dgp, wp = fenced((R, 3 * C), F32, gpu_device), fenced((ops.train_ws_floats(M, R, C),), F32, gpu_device)
    ops.gated_grad(xp[1], fp[1], gp[1], 0, C, rp[1] if rp else None, dfp[1], dgp[1], 2 * C, 3 * C, R, l, C, wp[1])
    assert pads_intact(xp, fp, gp, dfp, dgp, wp) and (rp is None or pads_intact(rp))
    used = N.gg_segments(n) * R * C
    w = wp[1].cpu()
    assert bool(torch.isfinite(w[:used]).all()) and bool(torch.isnan(w[used:]).all()), f'expected {N.gg_segments(n)} row segments of partial sums'
    ck = Checks(f'gated_grad {N.gg_name(n)}', op='gated_grad', dtype=dt, case=n, path=form)
    ck.add('df', host(dfp[1]), ex.df, N.df_bound(ex.df, dt == 'bf16'))
    r = np.ones(R) if rs is None else N.as_np(rs)
    bg = N.colsum_bound(ex.dgate, y32.dgate, np.abs(N.as_np(dx) * N.as_np(f)) * np.repeat(r, l)[:, None], R, l)
    g = dgp[1].cpu()
    ck.add('dgate', host(g[:, 2 * C:]), ex.dgate, bg.bound, bg.yard)
    assert bool(torch.isnan(g[:, :2 * C]).all()), 'columns of dgate outside the gate were written'
    ck.done()


# ================================================================================================ GroupNorm
def gn_ws(B, HW, C, dev):
    return fenced((ops.groupnorm_ws_bytes(B, HW, C) // 4,), F32, dev)


@pytest.mark.parametrize('n,dtype', [(n, d) for n in N.GN_CASES for d in N.gn_dtypes(n)], ids=lambda v: N.gn_name(v) if isinstance(v, int) else v)
def test_groupnorm_silu_elements(gpu_device, n, dtype):
    """y = x a + d (and its SiLU) element by element at 2^-20 (K_g (|x a| + |mean a|) + |b|); K_g from the channels' first pixels"""
    C, G, HW, fam = N.GN_CASES[n]
    B = N.GN_B
    x, w, b = N.gn_inputs(n, dtype)
    xp, wp, bp = fenced((B * HW, C), TD[dtype], gpu_device, x.view(B * HW, C)), fenced((C,), F32, gpu_device, w), fenced((C,), F32, gpu_device, b)
    ck = Checks(f'groupnorm {N.gn_name(n)} {dtype}', op='groupnorm_silu', dtype=dtype, case=n)
    for silu in (False, True):
        ex = N.groupnorm(x, w, b, G, silu=silu)
        K = N.gn_conditioning(x, ex, G, N.as_np(x)[:, 0])
        op, sp = fenced((B * HW, C), TD[dtype], gpu_device), gn_ws(B, HW, C, gpu_device)
        ops.groupnorm_silu(xp[1], wp[1], bp[1], op[1], B, HW, C, G, N.EPS, silu, sp[1])
        assert pads_intact(xp, wp, bp, op, sp)
        ck.add('y silu' if silu else 'y', host(op[1]).reshape(B, HW, C), ex.y, N.gn_bound(x, ex, b, G, K, silu, dtype), K_g=float(K.max()), silu=silu)
    ck.done()


@pytest.mark.parametrize('n', list(N.GN_TILE_CASES), ids=N.gn_tile_name)
def test_groupnorm_from_tile_partials_elements(gpu_device, n):
    """gn_finalize_tiles_kernel on partials computed in float64 from the stored x and rounded to fp32 (first-pixel pivots, and pivots 8 away: K_g ~ 30)"""
    C, G, t, p, fam, poor = N.GN_TILE_CASES[n]
    B, HW = N.GN_B, t * p
    x, w, b, part = N.gn_tile_inputs(n)
    xp, wp, bp = fenced((B * HW, C), BF16, gpu_device, x.view(B * HW, C)), fenced((C,), F32, gpu_device, w), fenced((C,), F32, gpu_device, b)
    pp = fenced((B, t, C, 3), F32, gpu_device, torch.from_numpy(part))
    ck = Checks(f'groupnorm tiles {N.gn_tile_name(n)}', op='groupnorm_silu_partials', dtype='bf16', case=n)
    for silu in (False, True):
        ex = N.groupnorm(x, w, b, G, silu=silu)
        K = N.gn_conditioning(x, ex, G, part[..., 2].astype(np.float64))
        op, sp = fenced((B * HW, C), BF16, gpu_device), gn_ws(B, HW, C, gpu_device)
        ops.groupnorm_silu_partials(xp[1], wp[1], bp[1], op[1], B, HW, C, G, N.EPS, silu, pp[1], t, p, sp[1])
        assert pads_intact(xp, wp, bp, pp, op, sp)
        ck.add('y silu' if silu else 'y', host(op[1]).reshape(B, HW, C), ex.y, N.gn_bound(x, ex, b, G, K, silu, 'bf16'), K_g=float(K.max()), silu=silu)
    ck.done()


def test_groupnorm_partials_refuses_without_writing(gpu_device):
    """tiles x pixels != HW is CVAR_EINVAL (-1), fp32 is CVAR_EUNSUPPORTED (-2), both before any launch"""
    B, HW, C, G = 2, 96, 160, 32
    for dtype, tiles, px, code in ((BF16, 4, 25, r'\(-1\)'), (F32, 4, 24, r'\(-2\)')):
        xp, op = fenced((B * HW, C), dtype, gpu_device, torch.ones(B * HW, C)), fenced((B * HW, C), dtype, gpu_device)
        wb, pp, sp = torch.ones(C, device=gpu_device), fenced((B, tiles, C, 3), F32, gpu_device, torch.zeros(B, tiles, C, 3)), gn_ws(B, HW, C, gpu_device)
        with pytest.raises(CvarError, match=code):
            ops.groupnorm_silu_partials(xp[1], wb, wb, op[1], B, HW, C, G, N.EPS, True, pp[1], tiles, px, sp[1])
        torch.cuda.synchronize()
        assert bool(torch.isnan(op[0]).all()) and bool(torch.isnan(sp[0]).all())
