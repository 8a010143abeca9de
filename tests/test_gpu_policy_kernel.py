"""cvar_pg_fwd_bwd on MI355X (include/cvar_policy.h) against the float64 contract of tests/policy_ref.py, row by row and element by element, at
the bounds derived there from the order of operations (tests/test_policy_host.py shows on the CPU that a float32 model of that order sits inside them and
that planted faults do not; no bound is measured on the kernel).  Sweep: M 1 / 5 / 37 x V 4104 / 4096 / 1000 / 257 / 2 x dlogits fp32 / bf16 / NULL x each
of weight, old_lp, ref_lp NULL or given, kl_coef 0 and 0.05, the asymmetric window [0.8, 1.3].  Every operand and output lies between NaN fences.  The clip
flags must be exact on every row the bound does not leave open (none with these inputs).  Bit for bit: identities (a), (b), (c) against ops.ce_fwd_bwd,
logprob == -loss_tok of the cross-entropy call, ties active, a row of a batch == its own M = 1 call, each output pointer alone.

Largest error / bound measured on MI355X over the whole sweep (the test prints every figure under -s):
  logprob 0.148   ratio 0.146   kl 0.039   loss_tok 0.123   coef 0.144   dlogits fp32 0.188, bf16 0.993 (its rounding term is a worst case)
  clip flags: 0 of 7740 rows left out of the comparison (cap 1 %)."""
import numpy as np
import pytest
import torch

import policy_ref as P
from oracle import train_kernels_ref as T

pytestmark = pytest.mark.gpu

from controlvar_amd import _lib, ops  # noqa: E402

F32, BF16, I32 = torch.float32, torch.bfloat16, torch.int32
PAD = 1024
NAN = float('nan')
OUTS = ('logprob', 'ratio', 'kl', 'clipped', 'coef')


def fenced(shape, dtype, dev, value=None):
    """(buffer, view): `shape` between two pads; floats are NaN (pads and, unless `value` is given, the view), int32 holds the pattern -7"""
    n = int(np.prod(shape))
    fill = NAN if dtype.is_floating_point else -7
    buf = torch.full((n + 2 * PAD,), fill, device=dev, dtype=dtype)
    view = buf[PAD:PAD + n].view(*shape)
    if value is not None:
        view.copy_(value.to(dtype))
    return buf, view


def untouched(buf, written=None):
    """the pads (and, with written=False, the view) still hold the fill"""
    t = buf.clone()
    if written is not False:
        t[PAD:t.numel() - PAD] = NAN if t.is_floating_point() else -7
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t == -7).all())


def bits(t):
    return t.contiguous().view({BF16: torch.int16, F32: torch.int32, I32: torch.int32}[t.dtype])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def run(dev, x, M, V, weight=None, old_lp=None, ref_lp=None, clip=P.CLIP, kl_coef=0.0, gscale=P.GSCALE, dl=F32, outs=OUTS, adv=None):
    """one call between fences -> dict of outputs (views on the device); asserts that nothing outside the asked outputs was written"""
    ins = {k: fenced(v.shape, v.dtype, dev, v) for k, v in dict(logits=x.logits[:M], target=x.target[:M], adv=x.adv[:M] if adv is None else adv).items()}
    opt = {k: fenced((M,), F32, dev, v[:M]) if v is not None else None for k, v in dict(weight=weight, old_lp=old_lp, ref_lp=ref_lp).items()}
    o = {k: fenced((M,), I32 if k == 'clipped' else F32, dev) for k in ('loss',) + OUTS}
    o['dlogits'] = fenced((M, V), dl, dev) if dl is not None else None
    given = lambda k: o[k][1] if k in outs else None
    ops.pg_fwd_bwd(ins['logits'][1], ins['target'][1], ins['adv'][1], *(opt[k][1] if opt[k] else None for k in ('weight', 'old_lp', 'ref_lp')),
                   clip[0], clip[1], kl_coef, gscale, o['loss'][1], M, V, dlogits=o['dlogits'][1] if o['dlogits'] else None,
                   **{k: given(k) for k in OUTS})
    torch.cuda.synchronize()
    for k, pair in o.items():
        if pair is not None:
            assert untouched(pair[0], written=(k in outs or k in ('loss', 'dlogits'))), f'{k}: fence or an output that was not asked for was written'
    return {k: pair[1] for k, pair in o.items() if pair is not None}


def run_ce(dev, x, M, V, weight, gscale, dl):
    lg, tg = x.logits[:M].to(dev), x.target[:M].to(dev)
    loss, d = torch.empty(M, device=dev), torch.empty(M, V, device=dev, dtype=dl)
    ops.ce_fwd_bwd(lg, tg, weight.to(dev) if weight is not None else None, gscale, loss, d, M, V)
    return loss, d


@pytest.fixture(scope='module')
def cases():
    return {(M, V): P.inputs(M, V) for M in P.MS for V in P.VS}


# ------------------------------------------------------------------------------------------------ the sweep against the float64 contract
@pytest.mark.parametrize('V', P.VS)
def test_rows_and_elements_against_the_contract(gpu_device, cases, V):
    worst, rows, left_out = {}, 0, 0
    for M in P.MS:
        x = cases[(M, V)]
        for wg, og, rg, kc in P.combos():
            kw = dict(P.pick(x, wg, og, rg), kl_coef=kc)
            ref = {False: P.reference(x.logits, x.target, x.adv, gscale=P.GSCALE, **kw)}
            ref[True] = P.reference(x.logits, x.target, x.adv, gscale=P.GSCALE, bf16=True, **kw)
            for dl in (F32, BF16, None):
                got = run(gpu_device, x, M, V, dl=dl, **kw)
                host = {k: v.float().cpu().double().numpy() if k != 'clipped' else v.cpu().numpy() for k, v in got.items()}
                r = ref[dl is BF16]
                for out, stem in P.FIELDS:
                    f = P.fraction(host[out], r, out, stem + '_bound')
                    worst[out] = max(worst.get(out, 0.0), f)
                if dl is not None:
                    key = 'dlogits ' + ('bf16' if dl is BF16 else 'fp32')
                    worst[key] = max(worst.get(key, 0.0), T.ratio_of(T.abs_err(host['dlogits'], r.dlogits), r.dl_bound))
                keep = ~P.open_rows(r)
                assert set(np.unique(host['clipped'])) <= {0, 1}
                assert np.array_equal(host['clipped'][keep], r.clipped[keep]), (M, V, wg, og, rg, kc)
                rows, left_out = rows + M, left_out + int((~keep).sum())
                if not og:
                    assert bool((got['ratio'] == 1.0).all())
                if not rg:
                    assert not bool(got['kl'].any())
    print(f'\n[policy_kernel] V={V}: kernel / bound  ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f'  (flags left out: {left_out} of {rows} rows)')
    assert all(v <= 1.0 for v in worst.values()), worst
    assert left_out <= 0.01 * rows


# ------------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize('dl', [F32, BF16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('V', [4104, 257, 2])
def test_identities_against_the_cross_entropy_kernel(gpu_device, cases, V, dl):
    M = 37
    x = cases[(M, V)]
    ones = torch.ones(M)
    for w in (None, x.weight):
        ce_loss, ce_dl = run_ce(gpu_device, x, M, V, w, P.GSCALE, dl)
        a = run(gpu_device, x, M, V, weight=w, dl=dl, adv=ones)                                          # (a)
        assert same(a['loss'], ce_loss) and same(a['dlogits'], ce_dl)
        assert same(a['logprob'], -ce_loss) and bool((a['ratio'] == 1.0).all()) and not bool(a['clipped'].any()) and not bool(a['kl'].any())
        b = run(gpu_device, x, M, V, weight=w, dl=dl)                                                    # (b)
        aw = x.adv if w is None else x.adv * w
        assert same(b['dlogits'], run_ce(gpu_device, x, M, V, aw, P.GSCALE, dl)[1])
        assert same(b['logprob'], -ce_loss) and same(b['coef'], aw.to(gpu_device))
        c = run(gpu_device, x, M, V, weight=w, old_lp=x.old_lp, ref_lp=x.ref_lp, kl_coef=0.05, dl=dl)     # (c): the general case through its own coef
        assert same(c['dlogits'], run_ce(gpu_device, x, M, V, c['coef'].cpu(), P.GSCALE, dl)[1])
        assert same(c['logprob'], -ce_loss) and bool(c['clipped'].any()) and not bool(c['clipped'].all())


def test_ties_are_active(gpu_device, cases):
    M, V = 37, 1000
    x = cases[(M, V)]
    t = run(gpu_device, x, M, V, clip=(0.0, 0.0))                                        # no old policy, a window of width zero
    assert not bool(t['clipped'].any()) and same(t['coef'], x.adv.to(gpu_device))
    lp = t['logprob'].cpu()
    u = run(gpu_device, x, M, V, old_lp=lp, ref_lp=lp, clip=(0.0, 0.0), kl_coef=0.05)    # the old policy and the reference ARE the policy
    assert bool((u['ratio'] == 1.0).all()) and not bool(u['clipped'].any()) and not bool(u['kl'].any()) and same(u['coef'], t['coef'])
    assert same(u['dlogits'], t['dlogits'])


def test_a_row_is_its_own_call(gpu_device, cases):
    """row m of the M = 37 call == the M = 1 call on that row, whatever its place"""
    M, V = 37, 4104
    x = cases[(M, V)]
    kw = dict(kl_coef=0.05, dl=BF16)
    full = run(gpu_device, x, M, V, weight=x.weight, old_lp=x.old_lp, ref_lp=x.ref_lp, **kw)
    for m in (0, 5, 36):
        one = P.NS(logits=x.logits[m:m + 1], target=x.target[m:m + 1], adv=x.adv[m:m + 1])
        got = run(gpu_device, one, 1, V, weight=x.weight[m:m + 1], old_lp=x.old_lp[m:m + 1], ref_lp=x.ref_lp[m:m + 1], **kw)
        for k, v in got.items():
            assert same(v.view(-1), full[k][m].view(-1)), (m, k)


def test_each_output_alone(gpu_device, cases):
    M, V = 5, 257
    x = cases[(M, V)]
    kw = dict(weight=x.weight, old_lp=x.old_lp, ref_lp=x.ref_lp, kl_coef=0.05)
    full = run(gpu_device, x, M, V, **kw)
    for k in OUTS:
        got = run(gpu_device, x, M, V, dl=None, outs=(k,), **kw)            # run() asserts that the other outputs kept their fill
        assert same(got[k], full[k]) and same(got['loss'], full['loss']), k
    none = run(gpu_device, x, M, V, dl=None, outs=(), **kw)
    assert same(none['loss'], full['loss'])


def test_refusals_leave_the_device_usable(gpu_device, cases):
    M, V = 5, 257
    x = cases[(M, V)]
    lg, tg, adv = x.logits.to(gpu_device), x.target.to(gpu_device), x.adv.to(gpu_device)
    loss = torch.full((M,), NAN, device=gpu_device)
    dl8 = torch.zeros(M, V, device=gpu_device, dtype=torch.float16)
    call = lambda **kw: ops.pg_fwd_bwd(kw.pop('logits', lg), kw.pop('target', tg), kw.pop('adv', adv), None, None, None, kw.pop('lo', 0.2), kw.pop('hi', 0.2),
                                       kw.pop('kc', 0.0), 1.0, kw.pop('loss', loss), kw.pop('M', M), kw.pop('V', V), **kw)
    for bad in (dict(logits=None), dict(target=None), dict(adv=None), dict(loss=None), dict(M=0), dict(V=1), dict(lo=-0.1), dict(hi=-0.1), dict(kc=-1.0)):
        with pytest.raises(_lib.CvarError, match='cvar_pg_fwd_bwd'):
            call(**bad)
    with pytest.raises(TypeError):
        call(dlogits=dl8)                                                   # ops refuses a dtype the ABI has no code for
    lib = _lib.load()
    assert lib.cvar_pg_fwd_bwd(lg.data_ptr(), tg.data_ptr(), adv.data_ptr(), None, None, None, 0.2, 0.2, 0.0, 1.0, loss.data_ptr(), None, None, None, None, None,
                               dl8.data_ptr(), 9, M, V, None) == -2
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and not bool(dl8.any())            # refused before any write
    call()
    torch.cuda.synchronize()
    assert same(loss, run(gpu_device, x, M, V, dl=None)['loss'])
