"""The training attention (forward with lse, backward) and the cos-attention pre-pass with its backward on MI355X against the
float64 oracles of oracle/attn_ref.py, in the per-token-row metric (attn_ref.row_error).

Bounds.  bf16 kernels: 3 x max(bf16 emulation of the kernel's storage points, 1e-3), the emulation evaluated in the same test on
the same operands; fp32 kernels: 4 x the same formula evaluated by torch in float32 on the CPU.  Both yardsticks are distances
from the float64 oracle.  tests/test_attn_oracle_host.py holds the two facts the bf16 bound rests on: the emulation is <= 2e-2 on
every case below (so the bound is < 6e-2), and a backward that ignores the last key or has one level end off by one moves some
token row by 0.24 .. 2.8 of its norm.

Emulation values measured on the CPU (amp 1.0, scale 0.125, seed = case number; row error against float64):
  case   dQ        dK        dV        out       |lse error| (fp32 row sum / bf16-P row sum)
   1     0         0         0         0         6.0e-08 / 6.0e-08
   2     4.03e-03  3.33e-03  3.20e-03  2.75e-03  4.5e-07 / 8.3e-04
   3     3.84e-03  3.52e-03  3.57e-03  2.78e-03  5.6e-07 / 6.3e-04
   4     4.09e-03  3.42e-03  3.22e-03  2.94e-03  7.4e-07 / 4.9e-04
   5     1.34e-02  4.54e-03  3.40e-03  2.89e-03  7.5e-07 / 1.2e-03
   6     4.88e-03  3.98e-03  3.54e-03  3.24e-03  7.6e-07 / 9.2e-04
   7     7.56e-03  3.37e-03  3.02e-03  2.53e-03  3.8e-07 / 6.6e-04
   8     3.97e-03  3.81e-03  3.59e-03  3.15e-03  7.6e-07 / 7.0e-04
   9     1.67e-02  3.80e-03  3.51e-03  2.92e-03  8.2e-07 / 1.2e-03
  10     4.33e-03  3.83e-03  3.08e-03  2.86e-03  8.0e-07 / 8.9e-04
  11     3.69e-03  3.72e-03  3.34e-03  3.29e-03  5.6e-07 / 6.9e-04
Cases 1 - 10 are the edges of the kernels' tile and level logic; 11 hides the first two key tiles completely from the second level
(found by tools/fuzz_attn_bwd.py once it drew holes: the MFMA forward returned NaN for such rows).
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
TENSORS = ('dQ', 'dK', 'dV')
PATHS = {'mfma': (BF16, False), 'rowwise_bf16': (BF16, True), 'rowwise_f32': (F32, True)}
_REFS = {}


def refs(n):
    """case n -> operands, float64 oracle and both yardsticks (bf16 emulation, float32 torch), computed once for the three paths"""
    if n not in _REFS:
        R, H, l, Lmax, ends, holes = A.CASES[n]
        qkv, dout = A.case_inputs(n)
        vis = A.visibility(l, ends, holes)
        ex = A.attention_fwd_bwd_f64(qkv, dout, A.SCALE, vis)
        out_e, lse_a, lse_b = A.attention_fwd_emulated(qkv, A.SCALE, vis)
        q, k, v = (t.float() for t in A.split_heads(qkv))
        s32 = (q @ k.transpose(-1, -2) * A.SCALE).masked_fill(~vis, -math.inf)
        yard = {
            BF16: dict(bwd=A.attention_bwd_emulated(qkv, dout, ex.out, ex.lse, A.SCALE, vis), out=out_e,
                       lse=max(float((lse_a - ex.lse).abs().max()), float((lse_b - ex.lse).abs().max()))),
            F32: dict(bwd=A.attention_bwd_formula(qkv, dout, ex.out.float(), ex.lse.float(), A.SCALE, vis, dtype=F32),
                      out=A.heads_to_rows(torch.softmax(s32, -1) @ v), lse=float((torch.logsumexp(s32, -1).double() - ex.lse).abs().max())),
        }
        _REFS[n] = (qkv, dout, ex, yard)
    return _REFS[n]


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


def bound(dtype, yardstick):
    return 3 * max(yardstick, 1e-3) if dtype == BF16 else 4 * yardstick


def report(kind, what, kernel, yardstick, limit, **kw):
    print(f'[{kind}] {what}: kernel {kernel:.3e}  yardstick {yardstick:.3e}  bound {limit:.3e}  ratio {kernel / yardstick if yardstick else float("inf"):.2f}')
    record(what, kind=kind, kernel=kernel, yardstick=yardstick, bound=limit, **kw)


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('n', list(A.CASES))
def test_attention_forward_and_isolated_backward_rows(gpu_device, n, path):
    """module docstring; the backward is handed O and lse of the float64 oracle (rounded to the path's dtype / fp32), so its error is
    its own.  All operands sit between NaN pads, arena rows [l, Lmax) are NaN, dqkv is NaN before the call."""
    dtype, rowwise = PATHS[path]
    R, H, l, Lmax, ends, holes = A.CASES[n]
    C = H * 64
    qkv, dout, ex, yard = refs(n)
    y = yard[dtype]
    failures = []

    def check(what, kernel, yardstick, tensor):
        limit = bound(dtype, yardstick)
        report('attn_bwd_rows', f'case {n} {path} {what}', kernel, yardstick, limit, case=n, path=path, tensor=tensor)
        if not kernel <= limit:
            failures.append((what, kernel, limit))

    qb, arena = fenced((R, Lmax, 3 * C), dtype, gpu_device)
    arena[:, :l] = qkv.to(dtype).to(gpu_device)
    dob, dod = fenced((R * l, C), dtype, gpu_device, dout)
    # ---- forward of the same call
    ob, out = fenced((R * l, C), dtype, gpu_device)
    lb, lse = fenced((R, H, l), F32, gpu_device)
    ops.attention(arena, out, R, H, Lmax, 0, l, A.SCALE, ends, rowwise=rowwise, lse=lse, holes=holes)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()) and pads_intact(qb, ob, lb)
    check('out', A.row_error(out.cpu(), ex.out, dout), A.row_error(y['out'], ex.out, dout), 'out')
    lse_err = float((lse.cpu().double() - ex.lse).abs().max())
    lse_limit = (3 if dtype == BF16 else 4) * y['lse']
    report('attn_bwd_rows', f'case {n} {path} lse (absolute)', lse_err, y['lse'], lse_limit, case=n, path=path, tensor='lse')
    if not lse_err <= lse_limit:
        failures.append(('lse', lse_err, lse_limit))
    # ---- isolated backward
    o_b, o_in = fenced((R * l, C), dtype, gpu_device, ex.out)
    l_b, lse_in = fenced((R, H, l), F32, gpu_device, ex.lse)
    wb, ws = fenced((R * H * l,), F32, gpu_device)
    db, dqkv = fenced((R, Lmax, 3 * C), dtype, gpu_device)
    ops.attention_bwd(arena, o_in, dod, lse_in, dqkv, ws, R, H, Lmax, l, A.SCALE, ends, rowwise=rowwise, holes=holes)
    got = dqkv.cpu()
    assert bool(torch.isfinite(got[:, :l]).all()), 'rows < l must all be written'
    assert bool(torch.isnan(got[:, l:]).all()), 'rows [l, Lmax) must stay untouched'
    assert pads_intact(qb, dob, o_b, l_b, wb, db)
    for name in TENSORS:
        ref = A.thirds(ex.dqkv)[name]
        check(name, A.row_error(A.thirds(got[:, :l])[name], ref, dout), A.row_error(A.thirds(y['bwd'])[name], ref, dout), name)
    if n == 1:            # one key: P = 1; dV = dO to one bf16 ulp (fp32: P = exp of two fp32 ulps of |lse| < 4 at most)
        dv, do3 = A.thirds(got)['dV'].double().view(R * l, C), dout.double()
        assert bool(((dv - do3).abs() <= (2.0 ** -7 if dtype == BF16 else 2.0 ** -20) * do3.abs()).all())
    # ---- a second call: fixed summation order, no atomics
    db2, dqkv2 = fenced((R, Lmax, 3 * C), dtype, gpu_device)
    ops.attention_bwd(arena, o_in, dod, lse_in, dqkv2, ws, R, H, Lmax, l, A.SCALE, ends, rowwise=rowwise, holes=holes)
    assert torch.equal(bits(dqkv2), bits(dqkv)) and pads_intact(db2)
    if n == 4:            # n_lvl == 1 with the end at l is the unlevelled problem: bit for bit the same on the same operands
        db3, dqkv3 = fenced((R, Lmax, 3 * C), dtype, gpu_device)
        ops.attention_bwd(arena, o_in, dod, lse_in, dqkv3, ws, R, H, Lmax, l, A.SCALE, None, rowwise=rowwise)
        assert torch.equal(bits(dqkv3), bits(dqkv))
        out3, lse3 = torch.empty_like(out), torch.empty_like(lse)
        ops.attention(arena, out3, R, H, Lmax, 0, l, A.SCALE, None, rowwise=rowwise, lse=lse3)
        assert torch.equal(bits(out3), bits(out)) and torch.equal(bits(lse3), bits(lse))
    assert not failures, failures


def test_prescaled_attention_refuses_a_hole_over_the_whole_first_tile(gpu_device):
    """the prescaled inference kernels take their shift from the first key tile's maximum; a level that sees nothing of [0, 64) has none.
    No inference mask is like that, so the call is an error instead of a NaN - the same structure one key shorter is served."""
    from controlvar_amd._lib import CvarError
    R, H, l = 1, 2, 200
    g = torch.Generator().manual_seed(1)
    kv = torch.randn(R, l, 2 * H * 64, generator=g).to(BF16).to(gpu_device)
    q = torch.randn(R, l, H * 64, generator=g).mul(0.125 * 1.4426950408889634).to(BF16).to(gpu_device)
    out = torch.empty(R * l, H * 64, device=gpu_device, dtype=BF16)
    with pytest.raises(CvarError):
        ops.attention(kv, out, R, H, l, 0, l, 1.0, [130, 200], holes=[(0, 0), (0, 130)], q=q, prescaled=True)
    ops.attention(kv, out, R, H, l, 0, l, 1.0, [130, 200], holes=[(0, 0), (1, 130)], q=q, prescaled=True)
    ref = torch.empty_like(out)
    ops.attention(kv, ref, R, H, l, 0, l, 0.6931471805599453, [130, 200], holes=[(0, 0), (1, 130)], q=q, rowwise=True)
    assert bool(torch.isfinite(out).all()) and float((out.float() - ref.float()).abs().max()) < 3e-2 * float(ref.float().abs().max())


# ------------------------------------------------------------------------------------------------ cos-attention pre-pass
LN100_F32 = float(torch.tensor(A.LN100, dtype=F32))
SCALE_MUL = [0.2, 1.4, LN100_F32, 5.0, 3.0]          # below, below, exactly at, above the clamp (ln 100); fifth head below
SENTINEL = 7.5


def ragged_rows(R, l, H, seed):
    """raw q | k | v rows whose norms spread over a decade"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, l, 3, H, 64, generator=g) * torch.rand(R, l, 3, H, 1, generator=g).mul(2.3).sub(1.15).exp()
    return x.reshape(R, l, 3 * H * 64)


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('R,H,l', [(2, 4, 9), (3, 5, 7)])
def test_cos_qk_norm_norms_and_backward(gpu_device, dtype, R, H, l):
    """cvar_cos_qk_norm with `norms`, then cvar_cos_qk_norm_bwd on random gradients in an arena-layout dqkv, against float64 autograd
    through F.normalize(q) * exp(clamp_max(s, ln 100)) and F.normalize(k).  (3, 5, 7): R l H 2 = 210 items, the last workgroup of four
    waves is half filled.  dq / dk: row metric; temperature gradient per (token, head): |error| / (|g|_2 sm).  bf16: 3 x the bf16
    emulation, fp32: 4 x torch float32 autograd.  The head exactly at the clamp carries the reference's gradient (torch's clamp_max
    passes it at equality; a parameter clamped in place sits exactly there), the head above it exactly 0."""
    C = H * 64
    assert (R * l * H * 2) % 4 == (0 if (R, H, l) == (2, 4, 9) else 2)
    sm = torch.tensor(SCALE_MUL[:H], dtype=F32)
    raw = ragged_rows(R, l, H, 11).to(dtype)
    grad = torch.randn(R, l, 3 * C, generator=torch.Generator().manual_seed(12)).to(dtype)
    grad[..., 2 * C:] = SENTINEL
    qb, arena = fenced((R, l, 3 * C), dtype, gpu_device, raw)
    nb, norms = fenced((R, l, H, 2), F32, gpu_device)
    smd = sm.to(gpu_device)
    ops.cos_qk_norm(arena, R, H, l, 0, l, smd, norms=norms)
    to_heads = lambda t, i: t.double()[..., i * C:(i + 1) * C].reshape(R * l, H, 64)
    q, k, gq, gk = to_heads(raw, 0), to_heads(raw, 1), to_heads(grad, 0), to_heads(grad, 1)
    ex = A.cos_qk_norm_fwd_bwd_f64(q, k, sm, gq, gk)
    # saved norms: 64 squares and a six-level tree of sums (7 roundings of a positive sum, halved by the root) + the root itself
    rel = float(((norms.cpu().double().view(R * l, H, 2) - ex.norms).abs() / ex.norms).max())
    print(f'[cos_norm] {dtype} R{R} H{H} l{l}: norms relative error {rel:.2e}')
    assert rel <= 6 * 2.0 ** -24 and pads_intact(qb, nb)
    assert torch.equal(bits(arena[..., 2 * C:]), bits(raw[..., 2 * C:].to(gpu_device))), 'v rows are not touched by the forward'
    gb, dqkv = fenced((R, l, 3 * C), dtype, gpu_device, grad)
    tb, dsm_tok = fenced((R * l, H), F32, gpu_device)
    ops.cos_qk_norm_bwd(arena, dqkv, R, H, l, l, smd, norms, dsm_tok)
    got = dqkv.cpu()
    assert pads_intact(qb, nb, gb, tb) and bool((got[..., 2 * C:] == SENTINEL).all()), 'the v third must come back unchanged'
    if dtype == BF16:
        y_dq, y_dk, y_ds = A.cos_qk_norm_bwd_emulated(q, k, sm, gq, gk)
    else:
        y = A.cos_qk_norm_fwd_bwd(q, k, sm, gq, gk, F32)
        y_dq, y_dk, y_ds = y.dq, y.dk, y.dsm_tok
    factor = 3 if dtype == BF16 else 4
    failures = []
    for name, g_, ref, yard_t, grads in (('dq', to_heads(got, 0), ex.dq, y_dq, gq), ('dk', to_heads(got, 1), ex.dk, y_dk, gk)):
        e, ye = A.row_error(g_, ref, grads), A.row_error(yard_t, ref, grads)
        report('cos_norm_rows', f'cos_qk_norm_bwd {dtype} R{R} H{H} l{l} {name}', e, ye, factor * ye, tensor=name)
        if not e <= factor * ye:
            failures.append((name, e, factor * ye))
    ds = dsm_tok.cpu().double()
    e, ye = A.temperature_error(ds, ex.dsm_tok, gq, sm), A.temperature_error(y_ds, ex.dsm_tok, gq, sm)
    report('cos_norm_rows', f'cos_qk_norm_bwd {dtype} R{R} H{H} l{l} temperature', e, ye, factor * ye, tensor='dsm')
    if not e <= factor * ye:
        failures.append(('dsm', e, factor * ye))
    at, above = SCALE_MUL.index(LN100_F32), SCALE_MUL.index(5.0)
    assert float(ex.dsm_tok[:, at].abs().min()) > 0
    assert bool((ds[:, at] != 0).all()), 'the head exactly at the clamp must carry the gradient (clamp_max passes it at equality)'
    assert bool((ds[:, above] == 0).all()), 'the head above the clamp carries exactly 0'
    assert not failures, failures


def test_cos_norm_attention_chain_fp32(gpu_device):
    """cos_qk_norm -> attention (levels of case 5) -> attention_bwd -> cos_qk_norm_bwd in fp32 against float64 autograd through the
    whole chain, the temperature gradient summed per head included.  Yardstick: the same chain under torch float32 autograd on the
    CPU, bound 4 x (row metric).  The summed temperature gradient: |sum_t got - ref_h| / sum_t(|g_t| sm_h) is at most the largest
    per-token error in units of |g_t| sm_h, so it is held to 4 x the float32 chain's per-token figure."""
    R, H, l, _, ends, _ = A.CASES[5]
    C = H * 64
    scale = 1.0                                        # cos-attention runs at scale 1 (basic_var.py:66-71)
    sm = torch.tensor([0.2, 1.4], dtype=F32)
    raw = ragged_rows(R, l, H, 21)
    dout = torch.randn(R * l, C, generator=torch.Generator().manual_seed(22))
    vis = A.visibility(l, ends)

    def chain(dtype):
        x = raw.to(dtype).clone().requires_grad_(True)
        xs = x.view(R, l, 3, H, 64)
        s = sm.to(dtype).view(1, 1, H).expand(R, l, H).clone().requires_grad_(True)
        qn = torch.nn.functional.normalize(xs[:, :, 0], dim=-1) * s.clamp_max(LN100_F32).exp()[..., None]
        kn = torch.nn.functional.normalize(xs[:, :, 1], dim=-1)
        qn.retain_grad()
        sc = (qn.permute(0, 2, 1, 3) @ kn.permute(0, 2, 3, 1) * scale).masked_fill(~vis, -math.inf)
        o = (torch.softmax(sc, -1) @ xs[:, :, 2].permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(R * l, C)
        o.backward(dout.to(dtype))
        return x.grad.double(), s.grad.double().view(R * l, H), qn.grad.double().reshape(R * l, H, 64)

    ref, ref_s, gq = chain(F64)
    y32, y32_s, _ = chain(F32)
    arena = raw.to(gpu_device).clone()
    norms = torch.empty(R, l, H, 2, device=gpu_device)
    smd = sm.to(gpu_device)
    ops.cos_qk_norm(arena, R, H, l, 0, l, smd, norms=norms)
    out = torch.empty(R * l, C, device=gpu_device)
    lse = torch.empty(R, H, l, device=gpu_device)
    ops.attention(arena, out, R, H, l, 0, l, scale, ends, lse=lse)
    db, dqkv = fenced((R, l, 3 * C), F32, gpu_device)
    ws = torch.empty(R * H * l, device=gpu_device)
    ops.attention_bwd(arena, out, dout.to(gpu_device), lse, dqkv, ws, R, H, l, l, scale, ends)
    dsm_tok = torch.empty(R * l, H, device=gpu_device)
    ops.cos_qk_norm_bwd(arena, dqkv, R, H, l, l, smd, norms, dsm_tok)
    got = dqkv.cpu().double()
    assert bool(torch.isfinite(got).all()) and pads_intact(db)
    failures = []
    for name in TENSORS:
        e = A.row_error(A.thirds(got)[name], A.thirds(ref)[name], dout)
        ye = A.row_error(A.thirds(y32)[name], A.thirds(ref)[name], dout)
        report('cos_norm_rows', f'fp32 chain {name}', e, ye, 4 * ye, tensor=name)
        if not e <= 4 * ye:
            failures.append((name, e, 4 * ye))
    ye = A.temperature_error(y32_s, ref_s, gq, sm)
    units = (gq.norm(dim=-1) * sm.double().exp().view(1, H)).sum(0)
    e = float(((dsm_tok.cpu().double().sum(0) - ref_s.sum(0)).abs() / units).max())
    report('cos_norm_rows', 'fp32 chain temperature gradient summed per head', e, ye, 4 * ye, tensor='dsm_sum')
    if not e <= 4 * ye:
        failures.append(('dsm_sum', e, 4 * ye))
    assert not failures, failures
