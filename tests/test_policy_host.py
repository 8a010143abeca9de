"""Policy-gradient fine-tuning on token ids, host side (no GPU; DESIGN.md 8d, include/cvar_policy.h): the sixth header against its ctypes table and the
library's exports, the refusals of cvar_pg_fwd_bwd (returned before any launch, so dummy pointers do), PolicyLoss and the argument checks of
Trainer.step_tokens / token_logprobs on a depth-2 model, and what tests/test_gpu_policy_kernel.py rests on (tests/policy_ref.py): the float32 model of
the kernel's order of operations sits inside the derived bounds of the float64 contract on every case of the sweep, identities (a), (b) and (c) and the
tie rule hold in the model, planted faults land outside, and the share of rows whose clip decision the bound leaves open stays under the 1 % cap."""
import os
import re

import numpy as np
import pytest
import torch

import policy_ref as P
from oracle import train_kernels_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'cvar_pg_fwd_bwd'


@pytest.fixture(scope='module')
def lib():
    from controlvar_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.load()


def _declarations(header):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(cvar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


# ------------------------------------------------------------------------------------------------ the ABI
def test_entry_point_is_declared_exported_and_bound(lib):
    from controlvar_amd import _lib, build, ops
    decl = _declarations('cvar_policy.h')
    assert list(decl) == [NAME] == list(_lib.POLICY_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.SERVE_SIGNATURES, _lib.ACCUM_SIGNATURES, _lib.KVCACHE_SIGNATURES, _lib.WIDE_SIGNATURES):
        assert NAME not in table
    ctype = lambda d: _lib.c_p if '*' in d else {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[re.sub(r'\s+', ' ', d).rsplit(' ', 1)[0]]
    res, argtypes = _lib.POLICY_SIGNATURES[NAME]
    assert res is _lib.c_i and argtypes == [ctype(d) for d in decl[NAME]]
    assert getattr(lib, NAME).argtypes == argtypes and getattr(lib, NAME).restype is res
    assert _lib.ABI_VERSION == 22 == lib.cvar_abi_version() and _lib.SERVE_VERSION == 1 == lib.cvar_serve_version()
    assert set(_declarations('cvar.h')) == set(_lib.SIGNATURES) and 'train.hip' in build.SOURCES and callable(ops.pg_fwd_bwd)


def _call(lib, logits=64, target=64, adv=64, loss=64, lo=0.2, hi=0.2, kc=0.0, dtype=0, M=3, V=8, dl=None):
    return lib.cvar_pg_fwd_bwd(logits, target, adv, None, None, None, lo, hi, kc, 1.0, loss, None, None, None, None, None, dl, dtype, M, V, None)


def test_the_library_refuses_without_a_launch(lib):
    """CVAR_EINVAL (-1): NULL logits / target / adv / loss_tok, M <= 0, V <= 1, a negative (or NaN) clip_lo / clip_hi / kl_coef; CVAR_EUNSUPPORTED (-2): an
    unknown out_dtype.  64 is a non-NULL address that is never dereferenced: every call returns on the host."""
    for k in ('logits', 'target', 'adv', 'loss'):
        assert _call(lib, **{k: None}) == -1, k
    for kw in (dict(M=0), dict(M=-2), dict(V=1), dict(V=0), dict(lo=-0.1), dict(hi=-1e-9), dict(kc=-0.5), dict(lo=float('nan')), dict(kc=float('nan'))):
        assert _call(lib, **kw) == -1, kw
    assert _call(lib, dtype=7) == -2 and _call(lib, dtype=-1, dl=64) == -2


# ------------------------------------------------------------------------------------------------ the model against the contract
def _cases():
    for M in P.MS:
        for V in P.VS:
            for wg, og, rg, kc in P.combos():
                yield M, V, wg, og, rg, kc


def test_the_model_sits_inside_the_bounds_and_the_cap_holds():
    worst = {}
    rows = open_ = 0
    for M, V, wg, og, rg, kc in _cases():
        x = P.inputs(M, V)
        kw = dict(P.pick(x, wg, og, rg), kl_coef=kc, gscale=P.GSCALE)
        ref, bref = P.reference(x.logits, x.target, x.adv, **kw), P.reference(x.logits, x.target, x.adv, bf16=True, **kw)
        mod = P.model(x.logits, x.target, x.adv, **kw)
        for out, stem in P.FIELDS:
            worst[out] = max(worst.get(out, 0.0), P.fraction(getattr(mod, out), ref, out, stem + '_bound'))
        worst['dlogits'] = max(worst.get('dlogits', 0.0), T.ratio_of(T.abs_err(mod.dlogits, ref.dlogits), ref.dl_bound))
        worst['dlogits bf16'] = max(worst.get('dlogits bf16', 0.0), T.ratio_of(T.abs_err(T.bf16_round(mod.dlogits), bref.dlogits), bref.dl_bound))
        keep = ~P.open_rows(ref)
        assert np.array_equal(mod.clipped[keep], ref.clipped[keep]), (M, V, wg, og, rg)
        if og:
            rows, open_ = rows + M, open_ + int(P.open_rows(ref).sum())
            if M == 37:                     # the placement reaches every zone for both signs
                below, above = ref.ratio < 0.8, ref.ratio > 1.3
                for sgn in (1, -1):
                    s = np.sign(T.as_np(x.adv)) == sgn
                    assert (s & below).any() and (s & above).any() and (s & ~below & ~above).any()
                assert ref.clipped.any() and not ref.clipped.all() and (T.as_np(x.adv) == 0).any() and (T.as_np(x.weight) == 0).any()
    print('\n[policy_host] model / bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    print(f'[policy_host] rows with an open clip decision: {open_} of {rows}')
    assert all(v <= 1.0 for v in worst.values()), worst
    assert open_ <= 0.01 * rows


def test_identities_and_the_tie_rule_in_the_model():
    x = P.inputs(37, 1000)
    ones = torch.ones(37)
    for w in (None, x.weight):
        ce = T.ce_model(x.logits, x.target, w, P.GSCALE)
        a = P.model(x.logits, x.target, ones, weight=w, gscale=P.GSCALE)
        assert np.array_equal(a.loss.view(np.int32), ce.loss.view(np.int32)) and np.array_equal(a.dlogits.view(np.int32), ce.dlogits.view(np.int32))   # (a)
        assert np.array_equal(a.logprob, -ce.loss)
        aw = x.adv if w is None else (x.adv * w).float()
        b = P.model(x.logits, x.target, x.adv, weight=w, gscale=P.GSCALE)
        assert np.array_equal(b.dlogits.view(np.int32), T.ce_model(x.logits, x.target, aw, P.GSCALE).dlogits.view(np.int32))                           # (b)
    # ties are active: no old policy and a window of width zero, and an old policy that IS the policy
    for kw in (dict(), dict(old_lp=torch.from_numpy(P.model(x.logits, x.target, x.adv).logprob))):
        t = P.model(x.logits, x.target, x.adv, clip=(0.0, 0.0), **kw)
        assert not t.clipped.any() and np.array_equal(t.ratio, np.ones(37, np.float32)) and np.array_equal(t.coef, T.as_np(x.adv, np.float32))
        assert not P.reference(x.logits, x.target, x.adv, clip=(0.0, 0.0)).clipped.any()
    # k3 at the reference itself is exactly 0, and so is its gradient term
    lp = torch.from_numpy(P.model(x.logits, x.target, x.adv).logprob)
    z = P.model(x.logits, x.target, x.adv, ref_lp=lp, kl_coef=0.05)
    assert not z.kl.any() and np.array_equal(z.coef, T.as_np(x.adv, np.float32))


def test_planted_faults_land_outside_the_bound():
    """what the GPU sweep must be able to see: the clip window mirrored, the KL gradient with the wrong sign, the inactive rows not zeroed"""
    x = P.inputs(37, 257)
    kw = dict(weight=x.weight, old_lp=x.old_lp, ref_lp=x.ref_lp, kl_coef=0.05, gscale=P.GSCALE)
    ref = P.reference(x.logits, x.target, x.adv, **kw)
    mirrored = P.model(x.logits, x.target, x.adv, **dict(kw, clip=(P.CLIP[1], P.CLIP[0])))
    assert (mirrored.clipped != ref.clipped)[~P.open_rows(ref)].any()
    flipped = P.reference(x.logits, x.target, x.adv, **dict(kw, kl_coef=0.0))
    flipped.coef = 2 * flipped.coef - ref.coef                       # c with + kl_coef (1 - e) in the place of -
    assert P.fraction(flipped.coef, ref, 'coef', 'coef_bound') >= 10
    a, w = T.as_np(x.adv), T.as_np(x.weight)
    unclipped = (ref.ratio * a - T.f32(0.05) * (1 - np.exp(T.as_np(x.ref_lp) - ref.logprob))) * w
    assert P.fraction(unclipped, ref, 'coef', 'coef_bound') >= 10


# ------------------------------------------------------------------------------------------------ PolicyLoss and the Trainer's argument checks
def test_policy_loss_checks_and_broadcasts():
    from controlvar_amd.train import PolicyLoss
    B, L = 3, 10
    adv = torch.tensor([1.0, -2.0, 0.0])
    p = PolicyLoss(adv, clip=0.1)
    assert p.clip == (0.1, 0.1) and p.kl_coef == 0.0
    a, o, r = p.rows(B, L)
    assert o is None and r is None and a.shape == (B * L,) and a.is_contiguous() and torch.equal(a.view(B, L), adv[:, None].expand(B, L))
    full = torch.arange(B * L, dtype=torch.float64).view(B, L)
    a, o, r = PolicyLoss(full, old_logprob=-full, ref_logprob=full.float(), clip=(0.2, 0.3), kl_coef=0.05).rows(B, L)
    assert a.dtype == o.dtype == r.dtype == torch.float32 and torch.equal(a, full.float().view(-1)) and torch.equal(o, -a) and torch.equal(r, a)
    for bad in (dict(clip=-0.1), dict(clip=(0.2, -0.1)), dict(clip=(0.2,)), dict(clip='0.2'), dict(clip=float('nan')), dict(kl_coef=-1.0),
                dict(kl_coef=float('inf')), dict(kl_coef=0.1), dict(old_logprob=adv), dict(ref_logprob=torch.zeros(B, L, dtype=torch.int64))):
        with pytest.raises(ValueError):
            PolicyLoss(adv, **bad)
    for bad in (torch.zeros(B, L, 1), torch.zeros((), dtype=torch.float32), torch.zeros(B, dtype=torch.int64), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            PolicyLoss(bad)
    for p in (PolicyLoss(torch.zeros(B + 1)), PolicyLoss(torch.zeros(B, L + 1)), PolicyLoss(adv, old_logprob=torch.zeros(B, L - 1)),
              PolicyLoss(adv, ref_logprob=torch.zeros(B + 1, L))):
        with pytest.raises(ValueError):
            p.rows(B, L)


def _trainer(**kw):
    from controlvar_amd import models, train as T_
    vae = models.build_vae(ch=32)
    if kw.pop('var', False):
        m = models.build_var(vae, depth=2, cond_drop_rate=0.0)
    else:
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, cond_drop_rate=0.0, **kw)
    return m, T_.Trainer(m, vae, peak_lr=1e-3, weight_decay=0.0, grad_accum=2)


def test_step_tokens_and_token_logprobs_refuse_on_the_host():
    """every refusal below is raised before any device work: the models live on the CPU, where a launch would raise CvarError instead"""
    from controlvar_amd.train import PolicyLoss
    m, tr = _trainer()
    pns, L, vocab = m.cfg.pyramid.patch_nums, m.cfg.pyramid.L, m.cfg.vocab
    n = sum(pn * pn for pn in pns)
    B = 2
    ids, cls, types = torch.zeros(B, n, dtype=torch.int64), torch.tensor([3, 7]), torch.tensor([0, 1])
    lists = [torch.zeros(B, pn * pn, dtype=torch.int64) for pn in pns]
    for call in (lambda **kw: tr.step_tokens(kw.pop('ids_img', ids), kw.pop('ids_ctrl', ids), kw.pop('cls', cls), kw.pop('types', types), **kw),
                 lambda **kw: tr.token_logprobs(kw.pop('ids_img', ids), kw.pop('ids_ctrl', ids), kw.pop('cls', cls), kw.pop('types', types), **kw)):
        for bad in (dict(ids_ctrl=None), dict(ids_img=ids[:, :-1]), dict(ids_img=ids.float()), dict(ids_img=lists[:-1]), dict(ids_ctrl=ids[:1]),
                    dict(cls=torch.tensor([3.0, 7.0])), dict(cls=torch.tensor(3)), dict(types=torch.tensor([0, 1, 2])), dict(mask_first=False)):
            with pytest.raises(ValueError):
                call(**bad)
        for bad in (dict(ids_img=ids + vocab), dict(ids_ctrl=ids - 1), dict(cls=torch.tensor([3, m.cfg.num_classes + 1])), dict(types=torch.tensor([0, 5]))):
            with pytest.raises((IndexError, ValueError)):
                call(**bad)
    with pytest.raises(ValueError, match='advantages'):
        tr.step_tokens(lists, lists, cls, types, policy=PolicyLoss(torch.zeros(B + 1)))
    with pytest.raises(ValueError, match='old_logprob'):
        tr.step_tokens(ids, ids, cls, types, policy=PolicyLoss(torch.zeros(B), old_logprob=torch.zeros(B, L + 2)))
    with pytest.raises(TypeError):
        tr.step_tokens(ids, ids, cls, types, policy=dict(advantages=torch.zeros(B)))
    with pytest.raises(ValueError, match='ignore_mask'):
        tr.step_tokens(ids, ids, cls, types, ignore_mask=torch.ones(B, L - 1))
    assert tr.window.micro == 0 and tr.it == 0                       # a refused call is no micro-batch
    # a plain VAR has no control half; separator and bidirectional models
    mv, trv = _trainer(var=True)
    with pytest.raises(ValueError, match='plain VAR'):
        trv.step_tokens(ids, ids, cls, None)
    ms, trs = _trainer(separator=True)
    for call in (trs.step_tokens, trs.token_logprobs):
        with pytest.raises(NotImplementedError, match='special tokens'):
            call(ids, ids, cls, types)
    mb, trb = _trainer(bidirectional=True)
    for call in (trb.step_tokens, trb.token_logprobs):
        with pytest.raises(ValueError, match='mask_first'):
            call(ids, ids, cls, types)


def test_the_engine_checks_the_policy_before_the_forward():
    from controlvar_amd.train import PolicyLoss
    m, tr = _trainer()
    L = m.cfg.pyramid.L
    x = torch.zeros(2, L - m.cfg.pyramid.first_l, 32)
    with pytest.raises(ValueError, match='advantages'):
        tr.engine.forward_backward(torch.tensor([3, 7]), x, torch.tensor([0, 1]), torch.zeros(2, L, dtype=torch.int64), policy=PolicyLoss(torch.zeros(3)))
