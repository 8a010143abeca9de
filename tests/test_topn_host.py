"""Top-N alternatives and sparse distillation targets, host side (no GPU; DESIGN.md 4g / 8e, include/cvar_topn.h): the ninth header against its ctypes table
and the library's symbols; tests/topn_ref.py against a brute-force sort, float64 autograd and the dense KL; a numpy float32 model of each kernel's order of
operations inside half of the bounds and planted faults far outside them; SparseDistillLoss' validation and every host refusal on a CPU model."""
import os
import re

import numpy as np
import pytest
import torch

import topn_ref as R
from controlvar_amd import _lib
from oracle import train_kernels_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['cvar_score_topn', 'cvar_kd_topn_fwd_bwd']


def _declarations(header):
    text = open(os.path.join(ROOT, 'include', header)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {m.group(2): m.group(3) for m in re.finditer(r'\b(int|int64_t)\s+(cvar_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)}


# ------------------------------------------------------------------------------------------------ the header and its table
def test_header_table_and_library_agree():
    decl = _declarations('cvar_topn.h')
    assert list(decl) == NAMES == list(_lib.TOPN_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.SERVE_SIGNATURES, _lib.ACCUM_SIGNATURES, _lib.KVCACHE_SIGNATURES, _lib.WIDE_SIGNATURES, _lib.POLICY_SIGNATURES,
                  _lib.DISTILL_SIGNATURES, _lib.REGION_SIGNATURES):
        assert not set(NAMES) & set(table)
    for name in NAMES:
        res, argtypes = _lib.TOPN_SIGNATURES[name]
        params = [p.strip() for p in decl[name].split(',')]
        assert len(params) == len(argtypes), name
        for p, a in zip(params, argtypes):
            want = _lib.c_p if '*' in p else {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[p.split()[0]]
            assert a is want, (name, p)
    lib = _lib.load()
    for name in NAMES:
        assert getattr(lib, name).argtypes == _lib.TOPN_SIGNATURES[name][1]
    assert not set(NAMES) & (set(_declarations('cvar.h')) | set(_declarations('cvar_serve.h')))            # their symbol tables stay what they were


# ------------------------------------------------------------------------------------------------ cvar_score_topn's reference
def _rows(V, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((6, V)) * 5).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 4                                   # ties on a 0.25 grid
    x[2, g.permutation(V)[:V // 2]] = -np.inf
    x[3] = 0.5
    x[4] = np.where(g.random(V) < 0.3, np.where(g.random(V) < 0.5, 0.0, -0.0), -1.0).astype(np.float32)
    return x


@pytest.mark.parametrize('V', [4096, 300, 37, 2])
def test_the_reference_is_a_brute_force_sort(V):
    x = _rows(V, V)
    for N in (1, 5, 32, 64):
        ref = R.score_reference(x[None], N)
        for r in range(x.shape[0]):
            order = sorted(range(V), key=lambda e: (-float(x[r, e]), e))
            want = order[:N] + [-1] * max(0, N - V)
            assert ref.ids[0, r].tolist() == want, (V, N, r)
            xs = x[r].astype(np.float64)
            with np.errstate(divide='ignore'):
                lse = np.log(np.exp(xs - xs.max()).sum()) + xs.max()
                rest = [e for e in range(V) if e not in set(order[:N])]
                tail = np.log(np.exp(xs[rest] - lse).sum()) if rest else -np.inf
            for i, e in enumerate(want):
                assert (ref.logprob[0, r, i] == -np.inf) if e < 0 or x[r, e] == -np.inf else abs(ref.logprob[0, r, i] - (xs[e] - lse)) < 1e-12
            assert (ref.tail[0, r] == -np.inf) if tail == -np.inf else abs(ref.tail[0, r] - tail) < 1e-9 * max(1.0, abs(tail)), (V, N, r)


@pytest.mark.parametrize('V', [4096, 1000, 300, 37])
def test_the_float32_model_of_score_topn_sits_inside_half_the_tail_bound(V):
    x = _rows(V, V + 1)
    for N in (1, 5, 32, 64):
        ref, mod = R.score_reference(x, N), R.score_model(x, N)
        live = ref.S_tail > 0
        assert bool(np.isneginf(mod.tail[~live]).all())
        if live.any():
            frac = T.ratio_of(T.abs_err(mod.tail[live], ref.tail[live]), ref.tail_bound[live])
            assert frac <= 0.5, (V, N, frac)
        fin = np.isfinite(ref.logprob)
        assert np.array_equal(np.isneginf(mod.logprob), ~fin)
        assert float(np.abs(mod.logprob[fin] - ref.logprob[fin]).max()) < 1e-4


# ------------------------------------------------------------------------------------------------ cvar_kd_topn_fwd_bwd's reference
def _stated_loss(x, ids, lp, tail):
    """the stated loss in float64 torch on one row set: x (M, V) requires grad"""
    M, V = x.shape
    lsm = torch.log_softmax(x, 1)
    used = ids >= 0
    q = torch.where(used, lp.exp(), torch.zeros_like(lp))
    listed = (q * torch.where(used, lp - lsm.gather(1, ids.clamp(min=0)), torch.zeros_like(lp))).sum(1)
    mask = torch.ones(M, V, dtype=torch.bool)
    for j in range(ids.shape[1]):
        rows = torch.nonzero(used[:, j]).flatten()
        mask[rows, ids[rows, j]] = False
    pt = torch.where(mask, lsm.exp(), torch.zeros_like(lsm)).sum(1)
    fin = torch.isfinite(tail)
    t0 = torch.where(fin, tail, torch.zeros_like(tail))
    return listed + torch.where(fin, t0.exp() * (t0 - torch.log(torch.where(fin, pt, torch.ones_like(pt)))), torch.zeros_like(pt))


@pytest.mark.parametrize('V,N', [(257, 8), (65, 64), (1000, 1), (65, 8)])
def test_loss_and_stated_gradient_against_float64_autograd(V, N):
    """a teacher whose listed mass and tail mass add up to one: the stated dlogits is the gradient of the stated loss"""
    M = 5
    x = R.kd_inputs(M, V, N)
    ref = R.kd_reference(x.logits, x.ids, x.lp, x.tail)
    xs = x.logits.double().requires_grad_(True)
    loss = _stated_loss(xs, x.ids.long(), x.lp.double(), x.tail.double())
    loss.sum().backward()
    assert float((loss.detach() - torch.from_numpy(ref.loss)).abs().max()) < 1e-10
    mass = ref.q.sum(1) + ref.r
    assert float(np.abs(mass - 1).max()) < 1e-5                       # fp32-stored log-probabilities
    # the stated gradient is the exact one for a teacher of total mass one: the residual is (mass - 1) p_v
    resid = np.abs(xs.grad.numpy() - ref.dlogits) - np.abs(mass - 1)[:, None] * ref.p
    assert float(resid.max()) < 1e-10


@pytest.mark.parametrize('V', [257, 1000])
def test_the_coarsened_kl_never_exceeds_the_dense_kl(V):
    M = 37
    for N in (1, 8, 64):
        x = R.kd_inputs(M, V, N)
        ref = R.kd_reference(x.logits, x.ids, x.lp, x.tail)
        dense = R.dense_kl(x.dense, x.logits)
        assert bool((ref.loss <= dense + 1e-5 * (1 + np.abs(dense))).all()), (V, N)
        assert bool((ref.loss >= -1e-5).all())
    full = R.kd_inputs(M, 65, 64)                                    # all but one code listed: the coarsening is the identity
    ref = R.kd_reference(full.logits, full.ids, full.lp, full.tail)
    assert float(np.abs(ref.loss - R.dense_kl(full.dense, full.logits)).max()) < 1e-4


@pytest.mark.parametrize('V', R.KD_VS)
def test_the_float32_model_sits_inside_half_the_bounds_and_planted_faults_far_outside(V):
    worst = {}
    for N in R.KD_NS:
        for M in R.KD_MS:
            for tail_kind, drop in (('finite', 0), ('finite', 2), ('none', 0)):
                x = R.kd_inputs(M, V, N, drop=drop if N > 2 else 0)
                tail = x.tail if tail_kind == 'finite' else None
                for w in (None, x.weight):
                    ref = R.kd_reference(x.logits, x.ids, x.lp, tail, w, R.GSCALE)
                    mod = R.kd_model(x.logits, x.ids, x.lp, tail, w, R.GSCALE)
                    fl, fd = R.kd_fractions(mod.loss, mod.dlogits, ref)
                    worst['loss'], worst['dl'] = max(worst.get('loss', 0), fl), max(worst.get('dl', 0), fd)
    assert worst['loss'] <= 0.5 and worst['dl'] <= 0.5, worst
    # planted faults, on a teacher with real tail mass (N = 8 of a broad teacher) and unit weights
    x = R.kd_inputs(37, V, 8)
    ref = R.kd_reference(x.logits, x.ids, x.lp, x.tail, None, 1.0)
    for fault in R.KD_FAULTS:
        mod = R.kd_model(x.logits, x.ids, x.lp, x.tail, None, 1.0, fault=fault)
        fl, fd = R.kd_fractions(mod.loss, mod.dlogits, ref)
        assert max(fl, fd) >= 10.0, (fault, fl, fd)


def test_the_model_of_a_teacher_taken_from_the_students_own_logits_is_inside_the_bounds_of_zero():
    for V, N in ((4096, 32), (1000, 64), (257, 8), (65, 64)):
        x = R.kd_inputs(37, V, N)
        sm = R.score_model(x.logits.numpy(), N)
        ids = R.score_reference(x.logits.numpy(), N).ids
        lp = np.where(ids >= 0, sm.logprob, 0).astype(np.float32)
        ref = R.kd_reference(x.logits, ids, lp, sm.tail, x.weight, R.GSCALE)
        mod = R.kd_model(x.logits, ids, lp, sm.tail, x.weight, R.GSCALE)
        assert float((np.abs(mod.loss) / ref.loss_bound).max()) <= 1.0 and float((np.abs(mod.dlogits) / ref.dl_bound).max()) <= 1.0, (V, N)


# ------------------------------------------------------------------------------------------------ SparseDistillLoss and the host refusals (CPU models)
def _trainer(**kw):
    from controlvar_amd import models, train as T_
    vae = models.build_vae(ch=32)
    if kw.pop('var', False):
        m = models.build_var(vae, depth=2, cond_drop_rate=0.0)
    else:
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, cond_drop_rate=0.0, **kw)
    return m, T_.Trainer(m, vae, peak_lr=1e-3, weight_decay=0.0, grad_accum=2)


def test_sparse_distill_loss_validates_types_and_shapes():
    import controlvar_amd
    from controlvar_amd.train import DistillLoss, SparseDistillLoss
    assert controlvar_amd.SparseDistillLoss is SparseDistillLoss and controlvar_amd.TokenScores.sparse_loss and controlvar_amd.SparseDistillTargets
    B, L, N = 2, 7, 4
    ids, lp, tail = torch.zeros(B, L, N, dtype=torch.int32), torch.zeros(B, L, N), torch.zeros(B, L)
    good = SparseDistillLoss(ids, lp, tail, weights=torch.ones(B, L, dtype=torch.bool))
    assert good.N == N and not isinstance(good, DistillLoss)
    SparseDistillLoss(ids, lp).check(B, L, 4096)
    for bad, what in ((dict(top_ids=ids.long()), 'top_ids'), (dict(top_ids=None), 'top_ids'), (dict(top_logprobs=lp.double()), 'top_logprobs'),
                      (dict(top_logprobs=lp[..., :2]), 'one shape'), (dict(top_ids=ids[0], top_logprobs=lp[0]), 'top_ids'), (dict(tail_logprob=tail.half()), 'tail_logprob'),
                      (dict(tail_logprob=tail[0]), 'tail_logprob'), (dict(weights=torch.ones(B, L, dtype=torch.int64)), 'weights'), (dict(weights=torch.ones(L)), 'weights'),
                      (dict(top_ids=torch.zeros(B, L, 65, dtype=torch.int32), top_logprobs=torch.zeros(B, L, 65)), '1 to 64'),
                      (dict(top_ids=torch.zeros(B, L, 0, dtype=torch.int32), top_logprobs=torch.zeros(B, L, 0)), '1 to 64')):
        with pytest.raises(ValueError, match=what):
            SparseDistillLoss(**{**dict(top_ids=ids, top_logprobs=lp, tail_logprob=tail), **bad})
    for shape in ((B + 1, L), (B, L + 1)):
        with pytest.raises(ValueError, match='top_ids'):
            good.check(*shape, 4096)
    with pytest.raises(ValueError, match='tail_logprob'):
        SparseDistillLoss(ids, lp, torch.zeros(B, L + 1)).check(B, L, 4096)
    with pytest.raises(ValueError, match='weights'):
        SparseDistillLoss(ids, lp, tail, weights=torch.ones(B, L + 1)).check(B, L, 4096)


def test_step_tokens_and_the_engine_refuse_a_bad_sparse_teacher_on_the_host():
    """every refusal below is raised before any device work: the models live on the CPU, where a launch would raise CvarError instead"""
    from controlvar_amd.train import PolicyLoss, SparseDistillLoss
    m, tr = _trainer()
    pns, L = m.cfg.pyramid.patch_nums, m.cfg.pyramid.L
    n, B, N = sum(pn * pn for pn in pns), 2, 8
    ids, cls, types = torch.zeros(B, n, dtype=torch.int64), torch.tensor([3, 7]), torch.tensor([0, 1])
    make = lambda b=B, l=L, **kw: SparseDistillLoss(torch.zeros(b, l, N, dtype=torch.int32), torch.zeros(b, l, N), **kw)
    with pytest.raises(ValueError, match='distill and policy'):
        tr.step_tokens(ids, ids, cls, types, distill=make(), policy=PolicyLoss(torch.zeros(B)))
    with pytest.raises(ValueError, match='ignore_mask'):
        tr.step_tokens(ids, ids, cls, types, distill=make(weights=torch.ones(B, L)), ignore_mask=torch.ones(B, L))
    with pytest.raises(TypeError, match='SparseDistillLoss'):
        tr.step_tokens(ids, ids, cls, types, distill=(torch.zeros(B, L, N), torch.zeros(B, L, N)))
    for bad in (make(b=B + 1), make(l=L - 1)):
        with pytest.raises(ValueError, match='top_ids'):
            tr.step_tokens(ids, ids, cls, types, distill=bad)
    with pytest.raises(ValueError, match='tail_logprob'):
        tr.step_tokens(ids, ids, cls, types, distill=make(tail_logprob=torch.zeros(B, L + 2)))
    with pytest.raises(ValueError):
        tr.step_tokens(ids[:, :-1], ids, cls, types, distill=make())               # the ids are still checked
    assert tr.window.micro == 0 and tr.it == 0                                     # a refused call is no micro-batch
    x = torch.zeros(B, L - m.cfg.pyramid.first_l, 32)
    with pytest.raises(ValueError, match='top_ids'):
        tr.engine.forward_backward(cls, x, types, torch.zeros(B, L, dtype=torch.int64), distill=make(b=3))
    ms, trs = _trainer(separator=True)
    with pytest.raises(NotImplementedError, match='special tokens'):
        trs.step_tokens(ids, ids, cls, types, distill=make())


def test_top_logprobs_and_distill_topn_refuse_on_the_host():
    m, _ = _trainer()
    lab, ty = torch.tensor([3, 7]), torch.tensor([0, 1])
    pns = m.cfg.pyramid.patch_nums
    ids = torch.zeros(2, sum(pn * pn for pn in pns), dtype=torch.int64)
    calls = {
        'joint': lambda **kw: m.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, **kw),
        'conditional': lambda **kw: m.conditional_infer_cfg(2, lab, g_seed=0, cfg=(4, 4, 4), cond_type=ty, c_mask=[ids], **kw),
        'edit': lambda **kw: m.edit_infer_cfg(2, lab, ty, src_img=ids, keep_img=True, **kw),
        'graph': lambda **kw: m.graphed_generator(2, per_request=True, **kw),
        'graph conditional': lambda **kw: m.graphed_conditional_generator(2, per_request=True, **kw),
        'graph edit': lambda **kw: m.graphed_edit_generator(2, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match='needs logprobs=True'):
            call(top_logprobs=8)
        for n in (0, 65, -1, 2.0, True, '8'):
            with pytest.raises(ValueError, match='an integer from 1 to 64'):
                call(logprobs=True, top_logprobs=n)
    for n in (0, 65, True):
        with pytest.raises(ValueError, match='an integer from 1 to 64'):
            m.score_infer_cfg(2, lab, ty, ids_img=ids, ids_ctrl=ids, top_logprobs=n)
        for name in ('joint', 'conditional'):
            with pytest.raises(ValueError, match='distill_topn'):
                calls[name](distill_topn=n)
    with pytest.raises(ValueError, match='one form of targets'):
        calls['joint'](distill_targets=True, distill_topn=8)
    with pytest.raises(ValueError, match='pass the same N'):
        calls['joint'](logprobs=True, top_logprobs=4, distill_topn=8)
    # regional guidance: a map form is not built
    reg = torch.ones(2, 1, 16, 16)
    with pytest.raises(NotImplementedError, match='regional guidance'):
        m.region_infer_cfg(2, lab[:, None], ty, regions=reg, logprobs=True, top_logprobs=8)
    with pytest.raises(NotImplementedError, match='regional guidance'):
        m.graphed_region_generator(2, 1, logprobs=True, top_logprobs=8)
    # a graph needs the per-request table, as logprobs=True does
    with pytest.raises(ValueError, match='per_request=True'):
        m.graphed_generator(2, logprobs=True, top_logprobs=8)
    # everything logprobs and distill_targets refuse today
    with pytest.raises(NotImplementedError, match='more_smooth'):
        calls['joint'](logprobs=True, top_logprobs=8, more_smooth=True)
    with pytest.raises(NotImplementedError, match='more_smooth'):
        calls['joint'](distill_topn=8, more_smooth=True)
    with pytest.raises(ValueError, match='per row'):
        m.autoregressive_infer_cfg(2, None, g_seed=0, cfg=4.0, cond_type=ty, distill_topn=8)          # the per-request path: labels are given
    ms, _ = _trainer(separator=True)
    for kw in (dict(logprobs=True, top_logprobs=8), dict(distill_topn=8)):
        with pytest.raises(NotImplementedError, match='separator'):
            ms.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, **kw)
    with pytest.raises(NotImplementedError, match='separator'):
        ms.score_infer_cfg(2, lab, ty, ids_img=ids, ids_ctrl=ids, top_logprobs=8)
    mb, _ = _trainer(bidirectional=True)
    with pytest.raises(NotImplementedError, match='bidirectional'):
        mb.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, cond_type=ty, distill_topn=8)
    m.sampler = 'torch'
    with pytest.raises(NotImplementedError, match="sampler='torch'"):
        calls['joint'](logprobs=True, top_logprobs=8)
    m.sampler = 'counter'
    mv, _ = _trainer(var=True)
    with pytest.raises(ValueError, match='needs logprobs=True'):
        mv.autoregressive_infer_cfg(2, lab, g_seed=0, cfg=4.0, top_logprobs=8)
    with pytest.raises(ValueError, match='an integer from 1 to 64'):
        mv.score_infer_cfg(2, lab, ids_img=ids, top_logprobs=65)
    with pytest.raises(NotImplementedError, match='regional guidance'):
        mv.region_infer_cfg(2, lab[:, None], regions=reg, logprobs=True, top_logprobs=8)


def test_token_scores_carry_the_alternatives_as_defaulted_keywords():
    from controlvar_amd.models import SparseDistillTargets, TokenScores
    from controlvar_amd.train import SparseDistillLoss
    B, pns, N = 2, (1, 2), 4
    L = 2 * 5
    z, zi = torch.zeros(B, L), torch.zeros(B, L, dtype=torch.int32)
    old = TokenScores(z, z, zi, zi, pns, 2, True)
    assert old.top_ids is None and old.top_logprobs is None and old.tail_logprob is None
    assert all(s.top_ids is None for s in old.per_scale())
    with pytest.raises(ValueError, match='top_logprobs=N'):
        old.sparse_loss()
    ids = torch.arange(B * L * N, dtype=torch.int32).view(B, L, N)
    sc = TokenScores(z, z, zi, zi, pns, 2, True, top_ids=ids, top_logprobs=torch.zeros(B, L, N), tail_logprob=z)
    parts = sc.per_scale()
    assert [tuple(p.top_ids.shape) for p in parts] == [(B, 2, N), (B, 8, N)] and torch.equal(parts[1].top_ids, ids[:, 2:])
    assert tuple(parts[1].tail_logprob.shape) == (B, 8)
    w = torch.ones(B, L)
    loss = sc.sparse_loss(weights=w)
    assert isinstance(loss, SparseDistillLoss) and loss.top_ids is ids and loss.weights is w
    t = SparseDistillTargets(zi, zi, ids, torch.zeros(B, L, N), z, torch.ones(B, L, dtype=torch.bool), True)
    assert isinstance(t.loss(), SparseDistillLoss) and t.loss().weights is t.sampled
