"""cvar_kd_topn_fwd_bwd on MI355X (include/cvar_topn.h) against the float64 contract of tests/topn_ref.py, row by row and element by element,
at the bounds derived there from the order of operations (tests/test_topn_host.py shows on the CPU that a float32 model of that order sits inside them and
that planted faults do not; no bound is measured on the kernel).  Sweep: M 1 / 5 / 37 x V 4096 / 1000 / 257 / 65 x N 1 / 8 / 64 x dlogits fp32 / bf16 / NULL x
weight given / NULL x the tail finite / -inf / NULL, slots shuffled and some marked unused (-1); logits to +-30.  Every operand and output lies between NaN
fences.  Bit for bit: N = 1, t_lp = 0, no tail == ops.ce_fwd_bwd; a row of a batch == its own M = 1 call.  A teacher that cvar_score_topn takes from the
student's own logits gives a loss and a gradient inside the bounds of zero.  Every refusal returns its code and leaves poisoned outputs untouched."""
import numpy as np
import pytest
import torch

import topn_ref as R
from conftest import record

pytestmark = pytest.mark.gpu

from controlvar_amd import _lib, ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
PAD = 1024
NAN = float('nan')


def fenced(shape, dtype, dev, value=None):
    """(buffer, view): `shape` between two pads of NaN (-77 for ids); the view is filled likewise unless `value` is given"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), -77 if dtype == torch.int32 else NAN, device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(value.to(dtype))
    return buf, view


def untouched(buf):
    """the pads still hold NaN"""
    n = buf.numel()
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[n - PAD:]).all())


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32}[t.dtype])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def run(dev, logits, ids, lp, tail, M, V, weight=None, gscale=R.GSCALE, dl=F32):
    """one call between fences -> (loss_tok, dlogits or None), views on the device"""
    N = ids.shape[1]
    lg = fenced((M, V), F32, dev, logits[:M])
    ti = fenced((M, N), torch.int32, dev, ids[:M])
    tl = fenced((M, N), F32, dev, lp[:M])
    tt = fenced((M,), F32, dev, tail[:M]) if tail is not None else None
    w = fenced((M,), F32, dev, weight[:M]) if weight is not None else None
    loss = fenced((M,), F32, dev)
    d = fenced((M, V), dl, dev) if dl is not None else None
    ops.kd_topn_fwd_bwd(lg[1], ti[1], tl[1], tt[1] if tt else None, N, w[1] if w else None, gscale, loss[1], d[1] if d else None, M, V)
    torch.cuda.synchronize()
    assert untouched(loss[0]) and (d is None or untouched(d[0])), 'a fence was written'
    return loss[1], (d[1] if d else None)


# ------------------------------------------------------------------------------------------------ the sweep against the float64 contract
@pytest.mark.parametrize('N', R.KD_NS)
@pytest.mark.parametrize('V', R.KD_VS)
def test_rows_and_elements_against_the_contract(gpu_device, V, N):
    worst = {}
    for M in R.KD_MS:
        for tail_kind, drop in (('finite', 0), ('finite', 2), ('minus_inf', 0), ('none', 1)):
            x = R.kd_inputs(M, V, N, tail=True, drop=drop if N > 2 else 0)
            tail = {'finite': x.tail, 'minus_inf': torch.full_like(x.tail, float('-inf')), 'none': None}[tail_kind]
            if tail_kind == 'finite' and M >= 5:
                tail = tail.clone()
                tail[3] = float('-inf')                             # one row of a finite-tail batch without tail mass
            for w in (None, x.weight):
                ref = {b: R.kd_reference(x.logits, x.ids, x.lp, tail, w, R.GSCALE, bf16=b) for b in (False, True)}
                for dl in (F32, BF16, None):
                    loss, d = run(gpu_device, x.logits, x.ids, x.lp, tail, M, V, weight=w, dl=dl)
                    fl, fd = R.kd_fractions(loss.cpu().double().numpy(), None if d is None else d.float().cpu().double().numpy(), ref[dl is BF16])
                    worst['loss_tok'] = max(worst.get('loss_tok', 0.0), fl)
                    if d is not None:
                        key = 'dlogits ' + ('bf16' if dl is BF16 else 'fp32')
                        worst[key] = max(worst.get(key, 0.0), fd)
    print(f'\n[kd_topn_kernel] V={V} N={N}: kernel / bound  ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    record('kd_topn_kernel', V=V, N=N, **{k.replace(' ', '_'): v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('dl', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('V', [4096, 1000, 257, 65])
def test_one_hot_teacher_is_the_cross_entropy(gpu_device, V, dl):
    M = 37
    x = R.kd_inputs(M, V, 1)
    target = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(V), dtype=torch.int32)
    target[0], target[1] = 0, V - 1
    for w in (None, x.weight):
        ce_loss, ce_dl = torch.empty(M, device=gpu_device), torch.empty(M, V, device=gpu_device, dtype=dl)
        ops.ce_fwd_bwd(x.logits.to(gpu_device), target.to(gpu_device), w.to(gpu_device) if w is not None else None, R.GSCALE, ce_loss, ce_dl, M, V)
        for tail in (None, torch.full((M,), float('-inf'))):
            loss, d = run(gpu_device, x.logits, target[:, None], torch.zeros(M, 1), tail, M, V, weight=w, dl=dl)
            assert same(loss, ce_loss) and same(d, ce_dl), (V, dl, w is None, tail is None)
        # the same teacher in slot 5 of N = 8, the other slots unused
        ids8 = torch.full((M, 8), -1, dtype=torch.int32)
        ids8[:, 5] = target
        loss, d = run(gpu_device, x.logits, ids8, torch.zeros(M, 8), None, M, V, weight=w, dl=dl)
        assert same(loss, ce_loss) and same(d, ce_dl), (V, dl, 'slot 5')


def test_a_row_is_its_own_call(gpu_device):
    """row m of the M = 37 call == the M = 1 call on that row, whatever its place"""
    M, V, N = 37, 1000, 8
    x = R.kd_inputs(M, V, N)
    for dl in (F32, BF16):
        loss, d = run(gpu_device, x.logits, x.ids, x.lp, x.tail, M, V, weight=x.weight, dl=dl)
        for m in (0, 5, 36):
            l1, d1 = run(gpu_device, x.logits[m:m + 1], x.ids[m:m + 1], x.lp[m:m + 1], x.tail[m:m + 1], 1, V, weight=x.weight[m:m + 1], dl=dl)
            assert same(l1.view(-1), loss[m].view(-1)) and same(d1.view(-1), d[m].view(-1)), (m, dl)


def test_dlogits_null_writes_only_the_loss(gpu_device):
    M, V, N = 5, 257, 8
    x = R.kd_inputs(M, V, N)
    full = run(gpu_device, x.logits, x.ids, x.lp, x.tail, M, V, weight=x.weight)
    loss, d = run(gpu_device, x.logits, x.ids, x.lp, x.tail, M, V, weight=x.weight, dl=None)
    assert d is None and same(loss, full[0])


# ------------------------------------------------------------------------------------------------ the teacher cvar_score_topn gives
@pytest.mark.parametrize('V,N', [(4096, 32), (1000, 64), (257, 8), (65, 64)])
def test_a_teacher_taken_from_the_students_own_logits_is_learnt(gpu_device, V, N):
    """score_topn on the student's logits (nrep = 1, weight 1) -> ids, log-probabilities, tail; the loss and dlogits lie inside the bounds of zero"""
    dev, M = gpu_device, 37
    x = R.kd_inputs(M, V, N)
    lg = x.logits.to(dev)
    coef = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=dev)
    ids = torch.empty(1, M, N, dtype=torch.int32, device=dev)
    lp, tail = torch.empty(1, M, N, device=dev), torch.empty(1, M, device=dev)
    ops.score_topn(lg.view(1, M, V), 1, 1, M, V, coef, N, ids, lp, tail)
    ids, lp, tail = ids[0].cpu(), torch.where(ids[0] >= 0, lp[0], torch.zeros_like(lp[0])).cpu(), tail[0].cpu()
    worst = {}
    for dl in (F32, BF16):
        ref = R.kd_reference(x.logits, ids, lp, tail, x.weight, R.GSCALE, bf16=dl is BF16)
        loss, d = run(dev, x.logits, ids, lp, tail, M, V, weight=x.weight, dl=dl)
        zero_l, zero_d = np.abs(loss.cpu().double().numpy()) / ref.loss_bound, np.abs(d.float().cpu().double().numpy()) / ref.dl_bound
        worst[str(dl)[6:]] = (float(zero_l.max()), float(zero_d.max()))
    print(f'\n[kd_topn_kernel] own teacher V={V} N={N}: |loss| / bound, |dlogits| / bound  {worst}')
    assert all(a <= 1.0 and b <= 1.0 for a, b in worst.values()), worst


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_device_usable(gpu_device):
    M, V, N = 5, 257, 8
    x = R.kd_inputs(M, V, N)
    dev = gpu_device
    lg, ti, tl, tt = x.logits.to(dev), x.ids.to(dev), x.lp.to(dev), x.tail.to(dev)
    loss = torch.full((M,), NAN, device=dev)
    dlp = torch.full((M, V), NAN, device=dev)
    dl16 = torch.zeros(M, V, device=dev, dtype=torch.float16)
    call = lambda **kw: ops.kd_topn_fwd_bwd(kw.pop('logits', lg), kw.pop('ids', ti), kw.pop('lp', tl), tt, kw.pop('N', N), None, 1.0, kw.pop('loss', loss),
                                            kw.pop('dl', dlp), kw.pop('M', M), kw.pop('V', V))
    for bad in (dict(logits=None), dict(ids=None), dict(lp=None), dict(loss=None), dict(M=0), dict(V=1), dict(N=0), dict(N=65)):
        with pytest.raises(_lib.CvarError, match='cvar_kd_topn_fwd_bwd'):
            call(**bad)
    with pytest.raises(TypeError):
        call(dl=dl16)                                                       # ops refuses a dtype the ABI has no code for
    lib = _lib.load()
    raw = lambda N=N, dtype=0, V=V, ids=ti.data_ptr(): lib.cvar_kd_topn_fwd_bwd(lg.data_ptr(), ids, tl.data_ptr(), tt.data_ptr(), N, None, 1.0, loss.data_ptr(),
                                                                                 dlp.data_ptr(), dtype, M, V, None)
    assert raw(dtype=9) == -2 and raw(N=0) == -2 and raw(N=65) == -2 and raw(V=32769) == -2
    assert raw(ids=None) == -1 and raw(V=1) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dlp).all()) and not bool(dl16.any())      # refused before any write
    call()
    torch.cuda.synchronize()
    l2, d2 = run(dev, x.logits, x.ids, x.lp, x.tail, M, V, gscale=1.0)
    assert same(loss, l2) and same(dlp, d2)
