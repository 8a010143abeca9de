"""The tail of the training step on MI355X - cvar_ce_fwd_bwd, cvar_adamw, cvar_adamw_multi, cvar_sumsq, cvar_sumsq_multi, cvar_clip_coef, cvar_colsum,
cvar_rowsum, cvar_wordembed_grad, cvar_scatter_add_rows, cvar_silu_bwd, cvar_gelu, cvar_gelu_bwd, cvar_gate_residual - against the float64 oracles of
oracle/train_kernels_ref.py, element by element, at the bounds derived there (tests/test_train_kernels_oracle_host.py shows on the CPU that models
of the kernels' arithmetic sit at <= 0.5 of them and that planted faults land outside).  Every call goes through controlvar_amd.ops; operands,
outputs and workspaces lie between NaN pads and unowned elements are NaN before the call.  The multi-tensor forms must give the single-tensor
forms' bits, the vector column sum the scalar one's.  Every comparison is recorded (kind = 'train_oracle').

Largest error / bound measured on MI355X (bf16 outputs and clip_coef's two float32 outputs sit near 1 by construction: their rounding term is a worst case):
  adamw        p 0.33  m 0.10  v 0.08          adamw_multi  p 0.30  m 0.09  v 0.06
  ce_fwd_bwd   loss 0.13  dlogits fp32 0.15, bf16 0.993          sumsq partials 0.055          clip_coef  norm 0.75  coef 0.83
  colsum 0.068     rowsum fp32 0.026, bf16 0.013     wordembed_grad dW 0.005, db 0.003     scatter_add_rows 0.25
  gelu fp32 0.25, bf16 0.985     gelu_bwd fp32 0.16, bf16 0.995     silu_bwd 0.15     gate_residual 0.25
Kernel mutants (arithmetic only, never committed) - all eleven fail here; tests/test_gpu_train_kernels.py alone (the earlier kernel tests) sees six of them:
  eps inside the bias correction, adamw_multi's group index forced to 0, w16 written from the old p, clip_coef without its 1e-6: missed there
  (the first three are seen by whole training steps in tests/test_gpu_train.py, the last by nothing else);
  decay after the update, bc2_sqrt squared, CE 1 / se from three of the four wave partials, a colsum segment ending at m1 - 1, wordembed's row pointer
  without `skip` after a sample boundary, gelu' with 0.044715 for 0.134145, silu' without its 1 +: seen there too.
With the bias corrections formed in float32 again (1 - powf(beta, step)) the betas (0.9, 0.999) cases at steps 2 and 7 fail and every (0.9, 0.95) case passes."""
import math

import numpy as np
import pytest
import torch

from conftest import record
from oracle import train_kernels_ref as T

pytestmark = pytest.mark.gpu

from controlvar_amd import ops  # noqa: E402

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
TD = {'f32': F32, 'bf16': BF16}
PAD = 4096
NAN = float('nan')
_REFS = {}


def once(key, fn):
    if key not in _REFS:
        _REFS[key] = fn()
    return _REFS[key]


def fenced(shape, dtype, dev, value=None):
    """(buffer, view): a tensor of `shape` between two NaN pads of PAD elements, NaN unless `value` is given"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * PAD,), NAN, device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(torch.as_tensor(value).to(dtype))
    return buf, view


def pads_intact(*pairs):
    for buf, view in pairs:
        lo = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        if not (bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[lo + view.numel():]).all())):
            return False
    return True


def window(flat_len, dev, dtype, off, rows, ld, block):
    """a (rows, ld)-strided window at element `off` of a NaN buffer between NaN pads that holds `block` (rows, cols <= ld); everything else is NaN"""
    host_ = torch.full((flat_len,), NAN, dtype=dtype)
    host_[off:off + rows * ld].view(rows, ld)[:, :block.shape[1]] = block.to(dtype)
    return fenced((flat_len,), dtype, dev, host_)


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32, F64: torch.int64}[t.dtype])


def host(t):
    return t.detach().cpu().double().numpy()


class Checks:
    def __init__(self, what, **kw):
        self.what, self.kw, self.failures = what, kw, []

    def add(self, tensor, got, ref, bound, **kw):
        """got within `bound` of `ref` element by element (NaN in got fails; equal infinities agree)"""
        err = T.abs_err(got, ref)
        ratio = T.ratio_of(err, bound)
        fin = err[np.isfinite(err)]
        print(f'[train_oracle] {self.what} {tensor}: kernel {float(fin.max()) if fin.size else math.inf:.3e}  bound {float(np.max(bound)):.3e}  ratio {ratio:.3f}')
        record(f'{self.what} {tensor}', kind='train_oracle', tensor=tensor, kernel=float(fin.max()) if fin.size else None, bound=float(np.max(bound)),
               ratio=ratio, **self.kw, **kw)
        if not ratio <= 1.0:
            self.failures.append((tensor, ratio))

    def done(self):
        assert not self.failures, (self.what, self.failures)


# ================================================================================================ AdamW
def run_adamw(dev, p, g, m, v, step, lr, b1, b2, eps, wd, gscale, gdev):
    bufs = [fenced((p.numel(),), F32, dev, t) for t in (p, g, m, v)]
    gd = fenced((1,), F32, dev, torch.tensor([gdev])) if gdev is not None else None
    ops.adamw(bufs[0][1], bufs[1][1], bufs[2][1], bufs[3][1], lr, b1, b2, eps, wd, step, gd[1] if gd else None, gscale)
    assert pads_intact(*bufs) and (gd is None or pads_intact(gd))
    assert torch.equal(bits(bufs[1][1].cpu()), bits(g)), 'the gradient was written'
    return bufs[0][1], bufs[2][1], bufs[3][1]


@pytest.mark.parametrize('n', list(T.ADAM_CASES), ids=T.adam_name)
def test_adamw_elements(gpu_device, n):
    """p within 8 u (|p'| + |p| + A), m within 20 u (|b1 m| + |(1 - b1) g'|), v within 32 u v' of torch.optim.AdamW in float64"""
    N, step, bt, wd, lr, gdev, gs = T.ADAM_CASES[n]
    p, g, m, v, blk = T.adam_inputs(n)
    kw = T.adam_args(n)
    ex = T.adamw(p, g, m, v, **kw)
    pd, md, vd = run_adamw(gpu_device, p, g, m, v, **kw)
    ck = Checks(f'adamw {T.adam_name(n)}', op='adamw', case=n)
    ck.add('p', host(pd), ex.p, ex.p_bound)
    ck.add('m', host(md), ex.m, ex.m_bound)
    ck.add('v', host(vd), ex.v, ex.v_bound)
    if lr == 0:
        assert torch.equal(bits(pd.cpu()), bits(p)), 'lr = 0 must leave every bit of p alone'
        assert not torch.equal(md.cpu(), m) and not torch.equal(vd.cpu(), v), 'lr = 0 still updates the moments'
    z = torch.from_numpy(blk == 3)
    if bool(z.any()):
        assert all(bool((t.cpu()[z] == 0).all()) for t in (pd, md, vd)), 'p = g = m = v = 0 must give exactly 0'
    ck.done()


@pytest.mark.parametrize('name', list(T.ADAM_MULTI))
def test_adamw_multi_elements_bits_of_the_single_form_and_bf16_copy(gpu_device, name):
    sizes, groups, lrs, wds, with16 = T.ADAM_MULTI[name]
    vals = T.adam_multi_inputs(name)
    a = T.ADAM_MULTI_ARGS
    tot, off = sum(sizes), np.cumsum([0] + list(sizes))
    arenas = [fenced((tot,), F32, gpu_device, torch.cat([t[k] for t in vals])) for k in range(4)]          # p, g, m, v back to back
    n16 = sum(sizes[i] for i in with16)
    w16 = fenced((n16,), BF16, gpu_device)
    gd = fenced((1,), F32, gpu_device, torch.tensor([a['gdev']]))
    view = lambda k, i: arenas[k][1][off[i]:off[i + 1]]
    o16, entries, copies = 0, [], {}
    for i in range(len(sizes)):
        c = None
        if i in with16:
            c = copies[i] = w16[1][o16:o16 + sizes[i]]
            o16 += sizes[i]
        entries.append((view(0, i), view(1, i), view(2, i), view(3, i), groups[i], c))
    table = ops.adam_table(entries, gpu_device)
    ops.adamw_multi(table, len(sizes), list(lrs), list(wds), a['b1'], a['b2'], a['eps'], a['step'], gd[1], a['gscale'])
    assert pads_intact(*arenas, w16, gd), 'the guards around the arenas were written'
    assert torch.equal(bits(arenas[1][1].cpu()), bits(torch.cat([t[1] for t in vals])))
    ck = Checks(f'adamw_multi {name}', op='adamw_multi', case=name)
    for i, (p, g, m, v) in enumerate(vals):
        kw = dict(a, lr=lrs[groups[i]], wd=wds[groups[i]])
        ex = T.adamw(p, g, m, v, **kw)
        ck.add(f'p[{i}]', host(view(0, i)), ex.p, ex.p_bound, group=groups[i])
        ck.add(f'm[{i}]', host(view(2, i)), ex.m, ex.m_bound)
        ck.add(f'v[{i}]', host(view(3, i)), ex.v, ex.v_bound)
        ps, ms, vs = run_adamw(gpu_device, p, g, m, v, **kw)
        for k, single in ((0, ps), (2, ms), (3, vs)):
            assert torch.equal(bits(view(k, i)), bits(single)), f'tensor {i} (n = {sizes[i]}, group {groups[i]}): not the bits of cvar_adamw'
        if i in copies:
            assert torch.equal(bits(copies[i]), bits(view(0, i).to(BF16))), f'tensor {i}: the bf16 copy is not the nearest-even rounding of the new p'
    ck.done()


# ================================================================================================ sumsq / clip_coef
def test_sumsq_partials_slots_and_the_multi_form(gpu_device):
    ck = Checks('sumsq', op='sumsq')
    xs, singles = [], []
    for n, (N, fam) in T.SUMSQ_CASES.items():
        x = T.sumsq_inputs(n)
        ex = once(('sumsq', n), lambda: T.sumsq(x))
        xp, pp = fenced((N,), F32, gpu_device, x), fenced((3 * 256,), F64, gpu_device)
        ops.sumsq(xp[1], pp[1], 1)
        assert pads_intact(xp, pp)
        got = pp[1].cpu()
        assert bool(torch.isnan(got[:256]).all()) and bool(torch.isnan(got[512:]).all()), 'slots 0 and 2 were written'
        ck.add(f'partials n{N}-{fam}', got[256:512].numpy(), ex.partial, ex.bound, case=n)
        assert bool(torch.isfinite(got[256:512]).all())
        xs.append(xp)
        singles.append(pp[1][256:512].clone())
    table = ops.adam_table([(x[1], x[1], x[1], x[1], 0) for x in xs], gpu_device)
    mp = fenced((len(xs) * 256,), F64, gpu_device)
    ops.sumsq_multi(table, len(xs), mp[1])
    assert pads_intact(mp, *xs)
    for i, s in enumerate(singles):
        assert torch.equal(bits(mp[1][i * 256:(i + 1) * 256]), bits(s)), f'tensor {i}: cvar_sumsq_multi does not give the bits of cvar_sumsq'
    ck.done()


def test_clip_coef_norm_and_coefficient(gpu_device):
    ck = Checks('clip_coef', op='clip_coef')
    for n, (c, ps, mn, kind) in T.CLIP_CASES.items():
        part = T.clip_inputs(n)
        ex = T.clip_coef(part, c, ps, mn)
        pp, op = fenced((c,), F64, gpu_device, part), fenced((2,), F32, gpu_device)          # the NaN pad behind `count` partials poisons a read past them
        ops.clip_coef(pp[1], c, ps, mn, op[1])
        assert pads_intact(pp, op)
        got = host(op[1])
        ck.add(f'norm {n}', got[:1], np.array([ex.norm]), np.array([ex.norm_bound]), case=n)
        ck.add(f'coef {n}', got[1:], np.array([ex.coef]), np.array([ex.coef_bound]), case=n)
        if kind in ('below', 'zero') or mn <= 0:
            assert got[1] == 1.0, (n, T.CLIP_CASES[n], got)
        if kind == 'zero':
            assert got[0] == 0.0
        if kind == 'huge' and mn > 0:
            assert 0 < got[1] < 1e-4
    ck.done()


# ================================================================================================ cross-entropy
def run_ce(dev, lg, tgt, w, gs, out):
    """out: None (loss only) | 'f32' | 'bf16' -> loss (M,), dlogits (M, V) or None"""
    M, V = lg.shape
    lp, tg = fenced((M, V), F32, dev, lg), tgt.to(dev)
    wp = fenced((M,), F32, dev, w) if w is not None else None
    sp = fenced((M,), F32, dev)
    dp = fenced((M, V), TD[out], dev) if out else None
    ops.ce_fwd_bwd(lp[1], tg, wp[1] if wp else None, gs, sp[1], dp[1] if dp else None, M, V)
    assert pads_intact(lp, sp) and (wp is None or pads_intact(wp)) and (dp is None or pads_intact(dp))
    return sp[1], dp[1] if dp else None


@pytest.mark.parametrize('n', list(T.CE_CASES), ids=T.ce_name)
def test_ce_loss_and_gradient_elements(gpu_device, n):
    V, fam, wk, gs = T.CE_CASES[n]
    lg, tgt, w, gs = T.ce_inputs(n)
    ex = T.ce(lg, tgt, w, gs)
    ck = Checks(f'ce {T.ce_name(n)}', op='ce_fwd_bwd', case=n)
    loss0, _ = run_ce(gpu_device, lg, tgt, w, gs, None)
    ck.add('loss (dlogits NULL)', host(loss0), ex.loss, ex.loss_bound)
    for out in ('f32', 'bf16'):
        loss, dl = run_ce(gpu_device, lg, tgt, w, gs, out)
        assert torch.equal(bits(loss), bits(loss0)), 'the loss depends on the gradient output'
        bound = ex.dl_bound + (T.BF16_HALF_ULP * np.abs(ex.dlogits) if out == 'bf16' else 0.0)
        got = host(dl)
        ck.add(f'dlogits {out}', got, ex.dlogits, bound, dtype=out)
        assert np.isfinite(got).all()
        rowsum = np.abs(got.sum(1))
        assert (rowsum <= bound.sum(1)).all(), ('a gradient row does not sum to 0 within the sum of its bounds', rowsum, bound.sum(1))
        if wk == 'zero':
            assert (got == 0).all()
        if out == 'f32':
            m = n % T.CE_M          # one block per row: row m of the M = 5 call is its own M = 1 call
            l1, d1 = run_ce(gpu_device, lg[m:m + 1], tgt[m:m + 1], None if w is None else w[m:m + 1], gs, 'f32')
            assert torch.equal(bits(l1), bits(loss[m:m + 1])) and torch.equal(bits(d1), bits(dl[m:m + 1]))
    ck.done()


# ================================================================================================ colsum / rowsum
def run_colsum(dev, form, A, out0, n):
    """the call of case n on the values A in the layout of `form`; -> out (N,), the workspace view"""
    M, N = A.shape
    lda, a_off, out_off, acc = T.colsum_layout(n)
    a_off = {'off': 9}.get(form, 8)
    ap = window(a_off + M * lda, dev, A.dtype, a_off, M, lda, A)
    o0 = torch.full((N + out_off + 3,), NAN)
    if acc:
        o0[out_off:out_off + N] = out0
    op, wp = fenced((N + out_off + 3,), F32, dev, o0), fenced((64 * N,), F32, dev)
    ops.colsum(ap[1], lda, op[1], M, N, wp[1], accumulate=acc, a_off=a_off, out_off=out_off)
    assert pads_intact(ap, op, wp)
    o = op[1].cpu()
    assert bool(torch.isnan(o[:out_off]).all()) and bool(torch.isnan(o[out_off + N:]).all()), 'out was written outside its N elements'
    used = T.colsum_segments(M)[0] * N
    w = wp[1].cpu()
    assert bool(torch.isfinite(w[:used]).all()) and bool(torch.isnan(w[used:]).all()), f'expected {used // N} segments of partial sums'
    return op[1][out_off:out_off + N]


@pytest.mark.parametrize('n', list(T.COLSUM_CASES), ids=T.colsum_name)
def test_colsum_elements_and_vector_bits(gpu_device, n):
    form, M, N, fam = T.COLSUM_CASES[n]
    A, out0 = T.colsum_inputs(n)
    o = out0 if T.colsum_layout(n)[3] else None
    ref, yard = T.colsum(A, o), T.colsum(A, o, dtype=np.float32)
    bd = T.colsum_bound(A, o, ref, yard)
    got = run_colsum(gpu_device, form, A, out0, n)
    ck = Checks(f'colsum {T.colsum_name(n)}', op='colsum', case=n, path=form)
    ck.add('out', host(got), ref, bd.bound)
    if form == 'off':       # the same values 16-byte aligned go to colsum_vec_kernel, which promises colsum_kernel's per-column order
        vec = run_colsum(gpu_device, 'vec', A, out0, n)
        assert torch.equal(bits(vec), bits(got)), 'colsum_vec_kernel and colsum_kernel<bf16> differ'
    ck.done()


@pytest.mark.parametrize('n', list(T.ROWSUM_CASES), ids=lambda n: '{}-{}-{}x{}'.format(n, *T.ROWSUM_CASES[n]))
def test_rowsum_elements(gpu_device, n):
    dt, R, nc = T.ROWSUM_CASES[n]
    A, out0 = T.rowsum_inputs(n)
    acc, lda, out_off = n % 2 == 0, T.rowsum_lda(n), 3
    o = out0 if acc else None
    ref, yard = T.rowsum(A, o), T.rowsum(A, o, dtype=np.float32)
    bd = T.rowsum_bound(A, 4 if dt == 'f32' else 8, o, ref, yard)
    ap = window(R * lda, gpu_device, TD[dt], 0, R, lda, A)
    o0 = torch.full((R + out_off + 2,), NAN)
    if acc:
        o0[out_off:out_off + R] = out0
    op = fenced((R + out_off + 2,), F32, gpu_device, o0)
    ops.rowsum(ap[1], lda, op[1], R, nc, accumulate=acc, out_off=out_off)
    assert pads_intact(ap, op)
    got = op[1].cpu()
    assert bool(torch.isnan(got[:out_off]).all()) and bool(torch.isnan(got[out_off + R:]).all())
    ck = Checks(f'rowsum {n}-{dt}-{R}x{nc}', op='rowsum', case=n, dtype=dt)
    ck.add('out', host(got[out_off:out_off + R]), ref, bd.bound)
    ck.done()


# ================================================================================================ wordembed_grad / scatter_add_rows
@pytest.mark.parametrize('n', list(T.WE_CASES), ids=T.we_name)
def test_wordembed_grad_weight_and_bias(gpu_device, n):
    B, npr, skip, C = T.WE_CASES[n]
    rows, ldx = T.we_layout(n)
    dx, tok = T.we_inputs(n)
    ex, y32 = T.wordembed(dx, tok, B, npr, rows, skip), T.wordembed(dx, tok, B, npr, rows, skip, dtype=np.float32)
    bw, bb = T.we_bounds(n, ex, y32)
    live = dx.clone().view(B, rows, C)
    live[:, :skip] = NAN            # rows a sample does not word-embed: a wrong row map poisons the sums
    live[:, skip + npr:] = NAN
    xp = window(B * rows * ldx, gpu_device, F32, 0, B * rows, ldx, live.view(B * rows, C))
    tp = fenced((B * npr, 32), F32, gpu_device, tok)
    w_off, b_off = 8, 8 + C * 32 + 4
    op = fenced((b_off + C + 8,), F32, gpu_device)
    ops.wordembed_grad(xp[1], ldx, rows, skip, tp[1], npr, B, C, 32, op[1], w_off, b_off)
    assert pads_intact(xp, tp, op)
    o = op[1].cpu()
    assert bool(torch.isnan(o[:w_off]).all()) and bool(torch.isnan(o[w_off + C * 32:b_off]).all()) and bool(torch.isnan(o[b_off + C:]).all())
    ck = Checks(f'wordembed_grad {T.we_name(n)}', op='wordembed_grad', case=n)
    ck.add('dW', host(o[w_off:w_off + C * 32]).reshape(C, 32), ex.dW, bw.bound)
    ck.add('db', host(o[b_off:b_off + C]), ex.db, bb.bound)
    ck.done()


@pytest.mark.parametrize('C', T.SCATTER_C)
def test_scatter_add_rows_in_order_onto_a_live_destination(gpu_device, C):
    src, dst = T.scatter_inputs(C)
    ref, yard = T.scatter_add(src, dst), T.scatter_add(src, dst, dtype=np.float32)
    bd = T.scatter_bound(src, dst, ref, yard)
    n, ld, off = len(T.SCATTER_IDX), C + 3, 2
    sp = window(off + n * ld, gpu_device, F32, off, n, ld, src)
    dp = fenced((T.SCATTER_ROWS, C), F32, gpu_device, dst)
    ops.scatter_add_rows(sp[1], ld, torch.tensor(T.SCATTER_IDX, dtype=torch.int32, device=gpu_device), dp[1], n, C, src_off=off)
    assert pads_intact(sp, dp)
    ck = Checks(f'scatter_add_rows C{C}', op='scatter_add_rows', case=C)
    ck.add('dst', host(dp[1]), ref, bd.bound * np.ones_like(ref))
    untouched = [r for r in range(T.SCATTER_ROWS) if r not in T.SCATTER_IDX]
    assert torch.equal(bits(dp[1].cpu()[untouched]), bits(dst[untouched]))
    ck.done()


# ================================================================================================ GELU / SiLU / gate_residual
@pytest.mark.parametrize('dt', ['f32', 'bf16'])
@pytest.mark.parametrize('n', T.ACT_N + (T.GELU_EDGE + 3,))
def test_gelu_forward_and_backward_elements(gpu_device, n, dt):
    a, dh = T.act_inputs(n, dt)
    ex = T.gelu(a, dh)
    ap, hp, dp = fenced((n,), TD[dt], gpu_device, a), fenced((n,), TD[dt], gpu_device), fenced((n,), TD[dt], gpu_device, dh)
    ops.gelu(ap[1], hp[1])
    ops.gelu_bwd(ap[1], dp[1])
    assert pads_intact(ap, hp, dp) and torch.equal(bits(ap[1].cpu()), bits(a))
    y, dy = host(hp[1]), host(dp[1])
    assert np.isfinite(y).all() and np.isfinite(dy).all(), 'a saturated __expf must not reach the output as inf or NaN'
    r = T.BF16_HALF_ULP if dt == 'bf16' else 0.0
    ck = Checks(f'gelu n{n} {dt}', op='gelu', dtype=dt, case=n)
    ck.add('gelu', y, ex.y, ex.y_bound + r * np.abs(ex.y))
    ck.add('gelu_bwd', dy, ex.dy, ex.dy_bound + r * np.abs(ex.dy))
    ck.done()


@pytest.mark.parametrize('n', T.ACT_N + (T.SILU_EDGE + 3,))
def test_silu_bwd_elements(gpu_device, n):
    x, ds = T.act_inputs(n, 'f32', seed=5)
    ex = T.silu_bwd(x, ds)
    xp, sp, op = fenced((n,), F32, gpu_device, x), fenced((n,), F32, gpu_device, ds), fenced((n,), F32, gpu_device)
    ops.silu_bwd(xp[1], sp[1], op[1])
    assert pads_intact(xp, sp, op)
    got = host(op[1])
    assert np.isfinite(got).all()
    ck = Checks(f'silu_bwd n{n}', op='silu_bwd', case=n)
    ck.add('dcond', got, ex.dx, ex.bound)
    ck.done()


@pytest.mark.parametrize('n', list(T.GR_CASES), ids=T.gr_name)
def test_gate_residual_elements(gpu_device, n):
    dt, has_rs, gr, C, M = T.GR_CASES[n]
    x, f, gate, rs = T.gr_inputs(n)
    ex = T.gate_residual(x, f, gate, rs, gr)
    R, ldg, goff = gate.shape[0], C + 8, 4
    xp, fp = fenced((M, C), F32, gpu_device, x), fenced((M, C), TD[dt], gpu_device, f)
    gp = window(goff + R * ldg, gpu_device, F32, goff, R, ldg, gate)
    rp = fenced((R,), F32, gpu_device, rs) if has_rs else None
    ops.gate_residual(xp[1], fp[1], gp[1], goff, ldg, gr, rp[1] if rp else None, M, C)
    assert pads_intact(xp, fp, gp) and (rp is None or pads_intact(rp))
    ck = Checks(f'gate_residual {T.gr_name(n)}', op='gate_residual', dtype=dt, case=n)
    ck.add('x', host(xp[1]), ex.y, ex.bound)
    ck.done()
