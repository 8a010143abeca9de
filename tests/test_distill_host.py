"""Guidance distillation, host side (no GPU; DESIGN.md 8e, include/cvar_distill.h): the seventh header against its ctypes table and the library's
exports, the refusals of cvar_kd_fwd_bwd (returned before any launch, so dummy pointers do), DistillLoss / DistillTargets and the argument checks of
Trainer.step_tokens(distill=...) and TrainEngine.forward_backward(distill=...) on a depth-2 model, the refusals of cfg=None and distill_targets=True that
need no device, and what tests/test_gpu_distill_kernel.py rests on (tests/distill_ref.py): the float32 model of the kernel's order of operations sits inside
the derived bounds of the float64 contract on every case of the sweep, identities (a) and (b) hold in the model bit for bit, planted faults land outside."""
import os
import re

import numpy as np
import pytest
import torch

import distill_ref as D
from oracle import train_kernels_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'cvar_kd_fwd_bwd'


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
    decl = _declarations('cvar_distill.h')
    assert list(decl) == [NAME] == list(_lib.DISTILL_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.SERVE_SIGNATURES, _lib.ACCUM_SIGNATURES, _lib.KVCACHE_SIGNATURES, _lib.WIDE_SIGNATURES, _lib.POLICY_SIGNATURES):
        assert NAME not in table
    ctype = lambda d: _lib.c_p if '*' in d else {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[re.sub(r'\s+', ' ', d).rsplit(' ', 1)[0]]
    res, argtypes = _lib.DISTILL_SIGNATURES[NAME]
    assert res is _lib.c_i and argtypes == [ctype(d) for d in decl[NAME]]
    assert getattr(lib, NAME).argtypes == argtypes and getattr(lib, NAME).restype is res
    assert _lib.ABI_VERSION == 22 == lib.cvar_abi_version() and _lib.SERVE_VERSION == 1 == lib.cvar_serve_version()
    assert set(_declarations('cvar.h')) == set(_lib.SIGNATURES) and 'train.hip' in build.SOURCES and callable(ops.kd_fwd_bwd)


def _call(lib, logits=64, teacher=64, ldt=8, loss=64, dtype=0, M=3, V=8, dl=None):
    return lib.cvar_kd_fwd_bwd(logits, teacher, ldt, None, 1.0, loss, dl, dtype, M, V, None)


def test_the_library_refuses_without_a_launch(lib):
    """CVAR_EINVAL (-1): NULL logits / teacher / loss_tok, M <= 0, V <= 1, ldt < V; CVAR_EUNSUPPORTED (-2): an unknown out_dtype.  64 is a non-NULL address
    that is never dereferenced: every call returns on the host."""
    for k in ('logits', 'teacher', 'loss'):
        assert _call(lib, **{k: None}) == -1, k
    for kw in (dict(M=0), dict(M=-2), dict(V=1), dict(V=0), dict(ldt=7), dict(ldt=0), dict(ldt=-8)):
        assert _call(lib, **kw) == -1, kw
    assert _call(lib, dtype=7) == -2 and _call(lib, dtype=-1, dl=64) == -2


# ------------------------------------------------------------------------------------------------ the model against the contract
def test_the_model_sits_inside_the_bounds():
    worst = {}
    for M in D.MS:
        for V in D.VS:
            x = D.inputs(M, V)
            assert float(x.teacher.abs().max()) <= D.RANGE
            if M == 37 and V >= 257:                 # the teacher rows span near-uniform to sharply peaked, and reach the edge of the range
                q = torch.softmax(x.teacher.double(), 1).max(1).values
                assert float(q.min()) < 2.0 / V and float(q.max()) > 0.5 and float(x.teacher.abs().max()) == D.RANGE
            for w in (None, x.weight):
                ref, bref = D.reference(x.logits, x.teacher, w, D.GSCALE), D.reference(x.logits, x.teacher, w, D.GSCALE, bf16=True)
                mod = D.model(x.logits, x.teacher, w, D.GSCALE)
                fl, fd = D.fractions(mod.loss, mod.dlogits, ref)
                fb = D.fractions(mod.loss, T.bf16_round(mod.dlogits), bref)[1]
                for k, v in (('loss_tok', fl), ('dlogits', fd), ('dlogits bf16', fb)):
                    worst[k] = max(worst.get(k, 0.0), v)
                assert (ref.loss >= -ref.loss_bound).all()                       # a KL divergence
    print('\n[distill_host] model / bound: ' + '  '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst


def test_identities_in_the_model():
    M, V = 37, 1000
    x = D.inputs(M, V)
    for w in (None, x.weight):
        a = D.model(x.logits, x.logits.clone(), w, D.GSCALE)                                        # (a) teacher == student
        assert not a.loss.any() and not a.dlogits.any()
        tg = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
        b = D.model(x.logits, D.onehot_teacher(tg, V), w, D.GSCALE)                                 # (b) one-hot teacher == the cross-entropy
        ce = T.ce_model(x.logits, tg, w, D.GSCALE)
        assert np.array_equal(b.loss.view(np.int32), ce.loss.view(np.int32)) and np.array_equal(b.dlogits, ce.dlogits)
    ref = D.reference(x.logits, x.logits.clone(), None, D.GSCALE)
    assert np.abs(ref.loss).max() == 0 and np.abs(ref.dlogits).max() == 0 and (ref.loss_bound > 0).all()


def test_planted_faults_land_outside_the_bound():
    x = D.inputs(37, 1000)
    ref = D.reference(x.logits, x.teacher, x.weight, D.GSCALE)
    for fault in D.FAULTS:
        mod = D.model(x.logits, x.teacher, x.weight, D.GSCALE, fault=fault)
        assert max(D.fractions(mod.loss, mod.dlogits, ref)) >= 10, fault


# ------------------------------------------------------------------------------------------------ DistillLoss, DistillTargets and the argument checks
def test_distill_loss_checks():
    from controlvar_amd.train import DistillLoss
    B, L, V = 2, 10, 16
    lg = torch.zeros(B, L, V)
    d = DistillLoss(lg, weights=torch.ones(B, L, dtype=torch.bool))
    d.check(B, L, V, 'cpu')
    DistillLoss(lg).check(B, L, V)
    for bad in (lg.double(), lg[0], lg.long(), [[0.0]], None):
        with pytest.raises(ValueError, match='logits'):
            DistillLoss(bad)
    for bad in (torch.ones(B, L, 1), torch.ones(B * L), torch.ones(B, L, dtype=torch.int64), [1.0]):
        with pytest.raises(ValueError, match='weights'):
            DistillLoss(lg, weights=bad)
    for args in ((B + 1, L, V), (B, L - 1, V), (B, L, V + 8)):
        with pytest.raises(ValueError, match='logits'):
            d.check(*args)
    with pytest.raises(ValueError, match='weights'):
        DistillLoss(lg, weights=torch.ones(B, L + 1)).check(B, L, V)


def test_distill_targets_hand_their_loss_over():
    from controlvar_amd.models import DistillTargets
    from controlvar_amd.train import DistillLoss
    B, L, V = 2, 10, 16
    lg, sampled = torch.zeros(B, L, V), torch.zeros(B, L, dtype=torch.bool)
    t = DistillTargets(torch.zeros(B, 5, dtype=torch.int32), torch.zeros(B, 5, dtype=torch.int32), lg, sampled, True)
    loss = t.loss()
    assert isinstance(loss, DistillLoss) and loss.logits is lg and loss.weights is sampled and t.mask_first is True


def _trainer(**kw):
    from controlvar_amd import models, train as T_
    vae = models.build_vae(ch=32)
    if kw.pop('var', False):
        m = models.build_var(vae, depth=2, cond_drop_rate=0.0)
    else:
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, cond_drop_rate=0.0, **kw)
    return m, T_.Trainer(m, vae, peak_lr=1e-3, weight_decay=0.0, grad_accum=2)


def test_step_tokens_refuses_on_the_host():
    """every refusal below is raised before any device work: the models live on the CPU, where a launch would raise CvarError instead"""
    from controlvar_amd.train import DistillLoss, PolicyLoss
    m, tr = _trainer()
    pns, L, V = m.cfg.pyramid.patch_nums, m.cfg.pyramid.L, m.cfg.vocab
    n = sum(pn * pn for pn in pns)
    B = 2
    ids, cls, types = torch.zeros(B, n, dtype=torch.int64), torch.tensor([3, 7]), torch.tensor([0, 1])
    good = DistillLoss(torch.zeros(B, L, V))
    with pytest.raises(ValueError, match='distill and policy'):
        tr.step_tokens(ids, ids, cls, types, distill=good, policy=PolicyLoss(torch.zeros(B)))
    with pytest.raises(ValueError, match='ignore_mask'):
        tr.step_tokens(ids, ids, cls, types, distill=DistillLoss(torch.zeros(B, L, V), weights=torch.ones(B, L)), ignore_mask=torch.ones(B, L))
    with pytest.raises(TypeError, match='DistillLoss'):
        tr.step_tokens(ids, ids, cls, types, distill=dict(logits=torch.zeros(B, L, V)))
    for bad in (torch.zeros(B + 1, L, V), torch.zeros(B, L - 1, V), torch.zeros(B, L, V + 8)):
        with pytest.raises(ValueError, match='logits'):
            tr.step_tokens(ids, ids, cls, types, distill=DistillLoss(bad))
    with pytest.raises(ValueError, match='weights'):
        tr.step_tokens(ids, ids, cls, types, distill=DistillLoss(torch.zeros(B, L, V), weights=torch.ones(B, L + 2)))
    with pytest.raises(ValueError):
        tr.step_tokens(ids[:, :-1], ids, cls, types, distill=good)               # the ids are still checked
    assert tr.window.micro == 0 and tr.it == 0                                   # a refused call is no micro-batch
    ms, trs = _trainer(separator=True)
    with pytest.raises(NotImplementedError, match='special tokens'):
        trs.step_tokens(ids, ids, cls, types, distill=good)


def test_the_engine_checks_the_distillation_before_the_forward():
    from controlvar_amd.train import DistillLoss, PolicyLoss
    m, tr = _trainer()
    L, V = m.cfg.pyramid.L, m.cfg.vocab
    x = torch.zeros(2, L - m.cfg.pyramid.first_l, 32)
    call = lambda **kw: tr.engine.forward_backward(torch.tensor([3, 7]), x, torch.tensor([0, 1]), torch.zeros(2, L, dtype=torch.int64), **kw)
    with pytest.raises(ValueError, match='logits'):
        call(distill=DistillLoss(torch.zeros(3, L, V)))
    with pytest.raises(ValueError, match='distill and policy'):
        call(distill=DistillLoss(torch.zeros(2, L, V)), policy=PolicyLoss(torch.zeros(2)))
    with pytest.raises(ValueError, match='ignore_mask'):
        call(distill=DistillLoss(torch.zeros(2, L, V), weights=torch.ones(2, L)), ignore_mask=torch.ones(2, L))
    ms, trs = _trainer(separator=True)
    with pytest.raises(NotImplementedError, match='special tokens'):
        trs.engine.forward_backward(torch.tensor([3, 7]), x, torch.tensor([0, 1]), torch.zeros(2, L, dtype=torch.int64), distill=DistillLoss(torch.zeros(2, L, V)))


# ------------------------------------------------------------------------------------------------ cfg=None and distill_targets: what is refused without a device
def test_unguided_generation_refuses_on_the_host():
    from controlvar_amd import models
    m, _ = _trainer()
    lab, ty = torch.tensor([3, 7]), torch.tensor([0, 1])
    pns = m.cfg.pyramid.patch_nums
    ids = torch.zeros(2, sum(pn * pn for pn in pns), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match='adapter'):
        m.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty, adapter=0)
    m._adapter_bank = dict(n=1)                                                  # a model with a bank attached
    for call in (lambda: m.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty),
                 lambda: m.conditional_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty, c_mask=[ids]),
                 lambda: m.graphed_generator(2, cfg=None), lambda: m.graphed_conditional_generator(2, cfg=None)):
        with pytest.raises(NotImplementedError, match='adapter'):
            call()
    m._adapter_bank = None
    m.sampler = 'torch'
    for call in (lambda: m.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty),
                 lambda: m.conditional_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty, c_mask=[ids]),
                 lambda: m.graphed_generator(2, cfg=None), lambda: m.graphed_conditional_generator(2, cfg=None)):
        with pytest.raises(NotImplementedError, match="sampler='torch'"):
            call()
    m.sampler = 'counter'
    with pytest.raises(NotImplementedError, match='edit_infer_cfg'):
        m.edit_infer_cfg(2, lab, ty, src_img=ids, keep_img=True, cfg=None)
    with pytest.raises(NotImplementedError, match='graphed_edit_generator'):
        m.graphed_edit_generator(2, cfg=None)
    with pytest.raises(NotImplementedError, match='score_infer_cfg'):
        m.score_infer_cfg(2, lab, ty, ids_img=ids, ids_ctrl=ids, cfg=None)
    ms, _ = _trainer(separator=True)
    with pytest.raises(NotImplementedError, match='separator'):
        ms.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty)
    with pytest.raises(NotImplementedError, match='separator'):
        ms.graphed_generator(2, cfg=None)
    m2, _ = _trainer(separate_decoding=True)
    with pytest.raises(NotImplementedError, match='two-pass'):
        m2.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None, cond_type=ty)
    mv, _ = _trainer(var=True)
    mv.sampler = 'torch'
    with pytest.raises(NotImplementedError, match="sampler='torch'"):
        mv.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=None)
    assert models.ControlVAR._guidance_rows(False) == 2 and models.ControlVAR._guidance_rows(True) == 4
    assert models.ControlVAR._guidance_rows(False, True) == 1 == models.ControlVAR._guidance_rows(True, True)


def test_the_request_table_without_guidance_weighs_the_one_row_by_one():
    from controlvar_amd.models import _request_table
    for four_way in (False, True):
        tab = _request_table(3, None, [0, 5, 1], 0.0, [1, 2, 3], four_way, 4096, 10)
        assert torch.equal(tab.coef[..., 0], torch.ones(10, 3)) and not tab.coef[..., 1:].any()
        assert tab.top_k.tolist() == [0, 5, 1] and tab.seed.tolist() == [1, 2, 3]


def test_distill_targets_refuse_on_the_host():
    m, _ = _trainer()
    lab, ty = torch.tensor([3, 7]), torch.tensor([0, 1])
    with pytest.raises(NotImplementedError, match='more_smooth'):
        m.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, more_smooth=True, distill_targets=True)
    with pytest.raises(NotImplementedError, match='more_smooth'):
        m.conditional_infer_cfg(2, lab, g_seed=0, cfg=(4, 4, 4), cond_type=ty, more_smooth=True, distill_targets=True)
    ms, _ = _trainer(separator=True)
    with pytest.raises(NotImplementedError, match='separator'):
        ms.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, distill_targets=True)
    mb, _ = _trainer(bidirectional=True)
    with pytest.raises(NotImplementedError, match='bidirectional'):
        mb.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, distill_targets=True)
    mv, _ = _trainer(var=True)
    with pytest.raises(NotImplementedError, match='more_smooth'):
        mv.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, more_smooth=True, distill_targets=True)
