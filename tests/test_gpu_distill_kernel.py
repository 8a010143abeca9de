"""cvar_kd_fwd_bwd on MI355X (include/cvar_distill.h) against the float64 contract of tests/distill_ref.py, row by row and element by element,
at the bounds derived there from the order of operations (tests/test_distill_host.py shows on the CPU that a float32 model of that order sits inside them and
that planted faults do not; no bound is measured on the kernel).  Sweep: M 1 / 5 / 37 x V 4096 / 4104 / 1000 / 257 / 2 x dlogits fp32 / bf16 / NULL x weight
given / NULL x ldt = V / V + 8; teacher rows from near-uniform to sharply peaked, logits up to +-30.  Every operand and output lies between NaN fences, and
the teacher's padding columns (ldt > V) hold NaN: a read past column V poisons the row.  Bit for bit: identity (a) (teacher == student: all zero), identity
(b) (one-hot teacher == ops.ce_fwd_bwd), a row of a batch == its own M = 1 call.  Every refusal returns its code and leaves poisoned outputs untouched.

Largest error / bound measured on MI355X over the whole sweep (the test prints every figure under -s and records it):
  loss_tok 0.038   dlogits fp32 0.120, bf16 0.994 (its rounding term is a worst case)."""
import numpy as np
import pytest
import torch

import distill_ref as D
from conftest import record
from oracle import train_kernels_ref as T

pytestmark = pytest.mark.gpu

from controlvar_amd import _lib, ops  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
PAD = 1024
NAN = float('nan')


def fenced(shape, dtype, dev, value=None):
    """(buffer, view): `shape` between two NaN pads; the view is NaN too unless `value` is given"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), NAN, device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(value.to(dtype))
    return buf, view


def untouched(buf, written=True):
    """the pads (and, with written=False, the view) still hold NaN"""
    t = buf.clone()
    if written:
        t[PAD:t.numel() - PAD] = NAN
    return bool(torch.isnan(t).all())


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32}[t.dtype])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def run(dev, logits, teacher, M, V, weight=None, gscale=D.GSCALE, dl=F32, pad=0):
    """one call between fences -> (loss_tok, dlogits or None), views on the device; the teacher lies in an (M, V + pad) buffer whose padding is NaN"""
    lg = fenced((M, V), F32, dev, logits[:M])
    tb = fenced((M, V + pad), F32, dev)
    tb[1][:, :V] = teacher[:M].to(dev)
    w = fenced((M,), F32, dev, weight[:M]) if weight is not None else None
    loss = fenced((M,), F32, dev)
    d = fenced((M, V), dl, dev) if dl is not None else None
    ops.kd_fwd_bwd(lg[1], tb[1], V + pad, w[1] if w else None, gscale, loss[1], d[1] if d else None, M, V)
    torch.cuda.synchronize()
    assert untouched(loss[0]) and (d is None or untouched(d[0])), 'a fence was written'
    return loss[1], (d[1] if d else None)


def run_ce(dev, logits, target, M, V, weight, gscale, dl):
    loss, d = torch.empty(M, device=dev), torch.empty(M, V, device=dev, dtype=dl)
    ops.ce_fwd_bwd(logits[:M].to(dev), target[:M].to(dev), weight[:M].to(dev) if weight is not None else None, gscale, loss, d, M, V)
    return loss, d


@pytest.fixture(scope='module')
def cases():
    return {(M, V): D.inputs(M, V) for M in D.MS for V in D.VS}


# ------------------------------------------------------------------------------------------------ the sweep against the float64 contract
@pytest.mark.parametrize('V', D.VS)
def test_rows_and_elements_against_the_contract(gpu_device, cases, V):
    worst = {}
    for M in D.MS:
        x = cases[(M, V)]
        for w in (None, x.weight):
            ref = {False: D.reference(x.logits, x.teacher, w, D.GSCALE), True: D.reference(x.logits, x.teacher, w, D.GSCALE, bf16=True)}
            for dl in (F32, BF16, None):
                for pad in (0, D.LDT_PAD):
                    loss, d = run(gpu_device, x.logits, x.teacher, M, V, weight=w, dl=dl, pad=pad)
                    fl, fd = D.fractions(loss.cpu().double().numpy(), None if d is None else d.float().cpu().double().numpy(), ref[dl is BF16])
                    worst['loss_tok'] = max(worst.get('loss_tok', 0.0), fl)
                    if d is not None:
                        key = 'dlogits ' + ('bf16' if dl is BF16 else 'fp32')
                        worst[key] = max(worst.get(key, 0.0), fd)
    print(f'\n[distill_kernel] V={V}: kernel / bound  ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    record('distill_kernel', V=V, **{k.replace(' ', '_'): v for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('dl', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('V', [4096, 4104, 257, 2])
def test_identities(gpu_device, cases, V, dl):
    M = 37
    x = cases[(M, V)]
    target = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(V), dtype=torch.int32)
    target[0], target[1] = 0, V - 1
    hot = D.onehot_teacher(target, V)
    for w in (None, x.weight):
        for pad in (0, D.LDT_PAD):
            loss, d = run(gpu_device, x.logits, x.logits.clone(), M, V, weight=w, dl=dl, pad=pad)            # (a) teacher == student, separate buffers
            assert torch.equal(loss, torch.zeros_like(loss)) and torch.equal(d, torch.zeros_like(d))
            ce_loss, ce_dl = run_ce(gpu_device, x.logits, target, M, V, w, D.GSCALE, dl)                     # (b) one-hot teacher == the cross-entropy
            loss, d = run(gpu_device, x.logits, hot, M, V, weight=w, dl=dl, pad=pad)
            assert torch.equal(loss, ce_loss) and torch.equal(d, ce_dl)


def test_a_row_is_its_own_call(gpu_device, cases):
    """row m of the M = 37 call == the M = 1 call on that row, whatever its place"""
    M, V = 37, 4104
    x = cases[(M, V)]
    for dl in (F32, BF16):
        loss, d = run(gpu_device, x.logits, x.teacher, M, V, weight=x.weight, dl=dl, pad=D.LDT_PAD)
        for m in (0, 5, 36):
            l1, d1 = run(gpu_device, x.logits[m:m + 1], x.teacher[m:m + 1], 1, V, weight=x.weight[m:m + 1], dl=dl)
            assert same(l1.view(-1), loss[m].view(-1)) and same(d1.view(-1), d[m].view(-1)), (m, dl)


def test_refusals_leave_the_device_usable(gpu_device, cases):
    M, V = 5, 257
    x = cases[(M, V)]
    lg, tc = x.logits.to(gpu_device), x.teacher.to(gpu_device)
    loss = torch.full((M,), NAN, device=gpu_device)
    dlp = torch.full((M, V), NAN, device=gpu_device)
    dl16 = torch.zeros(M, V, device=gpu_device, dtype=torch.float16)
    call = lambda **kw: ops.kd_fwd_bwd(kw.pop('logits', lg), kw.pop('teacher', tc), kw.pop('ldt', V), None, 1.0, kw.pop('loss', loss), kw.pop('dl', dlp),
                                       kw.pop('M', M), kw.pop('V', V))
    for bad in (dict(logits=None), dict(teacher=None), dict(loss=None), dict(M=0), dict(V=1), dict(ldt=V - 1)):
        with pytest.raises(_lib.CvarError, match='cvar_kd_fwd_bwd'):
            call(**bad)
    with pytest.raises(TypeError):
        call(dl=dl16)                                                       # ops refuses a dtype the ABI has no code for
    lib = _lib.load()
    assert lib.cvar_kd_fwd_bwd(lg.data_ptr(), tc.data_ptr(), V, None, 1.0, loss.data_ptr(), dlp.data_ptr(), 9, M, V, None) == -2
    assert lib.cvar_kd_fwd_bwd(lg.data_ptr(), tc.data_ptr(), V - 1, None, 1.0, loss.data_ptr(), dlp.data_ptr(), 0, M, V, None) == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dlp).all()) and not bool(dl16.any())      # refused before any write
    call()
    torch.cuda.synchronize()
    l2, d2 = run(gpu_device, x.logits, x.teacher, M, V, gscale=1.0)
    assert same(loss, l2) and same(dlp, d2)
