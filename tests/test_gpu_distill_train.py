"""The distillation step and the teacher's targets on MI355X: TrainEngine.forward_backward(distill=...), Trainer.step_tokens(distill=...)
and distill_targets=True of the generation calls, on the depth-2 models of test_gpu_policy_train.py (tiny VQVAE, condition dropout off, B = 2).

Almost every statement is bitwise, torch.equal with no tolerance: the distillation step IS the supervised step with another loss launch - everything behind
dlogits is the same code on the same buffers - and the kernels are deterministic.  The one statement that is not (four updates lower the KL of the batch) is
an inequality with no bound to tune."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import ops, train as T  # noqa: E402
from controlvar_amd.train import DistillLoss  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
KW = dict(peak_lr=2e-3, weight_decay=0.05, sche='lin0', warmup_it=2, max_it=50, clip=2.0, drop_path=False)      # test_gpu_grad_accum.KW
CLS = [17, 403, 5, 999]
TYPES = [2, 0, 1, 3]
KINDS = [('joint', BF16), ('joint', F32), ('lora', BF16), ('lora', F32)]
_IDS = {}


def _models(kind, dtype, dev, **kw):
    from controlvar_amd import lora, models
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0, **kw).to(dev).eval()
    if kind == 'lora':
        lora.add_lora(m, r=16, dropout=0.0, seed=1)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for _, (_, Bm) in lora.adapters(m).items():      # B = 0 would make every dA zero and hide half of the gradients
                Bm.copy_(torch.randn(Bm.shape, generator=g) * 0.05)
    return vae, m


def _ids(vae, dev, dtype, B):
    """(ids_ctrl, ids_img) of a synthetic batch from the tokenizer: computed once per precision, shared, never changed"""
    key = (dtype, B)
    if key not in _IDS:
        from controlvar_amd.synth import synth_images
        images, masks = synth_images(4, 256, seed=6)[:B].to(dev), synth_images(4, 256, seed=7)[:B].to(dev)
        both = vae.img_to_idxBl(torch.cat((masks, images), dim=0))
        _IDS[key] = ([t[:B].clone() for t in both], [t[B:].clone() for t in both])
    return _IDS[key]


def _labels(B):
    return torch.tensor(CLS[:B]), torch.tensor(TYPES[:B])


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def _same(a, b, what=''):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _teacher_logits(B, L, V, dev, seed=0):
    """(B, L, V) fp32: rows from near-uniform to peaked"""
    g = torch.Generator().manual_seed(70 + seed)
    std = torch.logspace(-1.5, 0.9, B * L).view(B, L, 1)
    return (torch.randn(B, L, V, generator=g) * std).clamp(-30, 30).to(dev)


def _inputs(tr, ctrl, img, B):
    return tr._inputs_of([torch.cat((c, i), 0) for c, i in zip(ctrl, img)], B, True)


# ---------------------------------------------------------------------------------------------------------------- 1. only the loss kernel changed
@pytest.mark.parametrize('kind,dtype', KINDS)
def test_distill_step_is_the_walk_with_another_loss_launch(gpu_device, kind, dtype):
    B = 2
    cls, types = _labels(B)
    vae, m = _models(kind, dtype, gpu_device)
    tr = T.Trainer(m, vae, **KW)
    eng = tr.engine
    ctrl, img = _ids(vae, gpu_device, dtype, B)
    L, V = m.cfg.pyramid.L, m.cfg.vocab
    teacher = _teacher_logits(B, L, V, gpu_device)
    mask = (torch.rand(B, L, generator=torch.Generator().manual_seed(5)) < 0.8).float().to(gpu_device)
    x, labels = _inputs(tr, ctrl, img, B)
    loss, loss_tok = eng.forward_backward(cls, x, types, labels, distill=DistillLoss(teacher, weights=mask))
    grads, dlogits, loss_tok = _clone(eng.grads()), eng.dlogits.clone(), loss_tok.clone()
    assert bool((loss_tok > 0).all()) and bool(dlogits.any())
    # forward_train + the kernel on the engine's logits by hand + backward()
    eng.forward_train(cls, x, types, None, True)
    M = eng.M
    assert eng.V == V
    w = mask.view(-1)
    gscale = 1.0 / (M * (float(w.mean()) + 1e-6))
    lt, dl = torch.empty(M, device=gpu_device), torch.empty_like(dlogits)
    ops.kd_fwd_bwd(eng.logits, teacher, V, w, gscale, lt, dl, M, V)
    assert torch.equal(dl, dlogits) and torch.equal(lt, loss_tok)
    assert torch.equal(loss, (loss_tok * w).mean() / (w.mean() + 1e-6))
    eng.dlogits.copy_(dl)
    eng.backward()
    _same(eng.grads(), grads, 'grads')
    # without weights the loss is the plain mean and gscale 1 / M
    loss2, lt2 = eng.forward_backward(cls, x, types, labels, distill=DistillLoss(teacher))
    ops.kd_fwd_bwd(eng.logits, teacher, V, None, 1.0 / M, lt, dl, M, V)
    assert torch.equal(dl, eng.dlogits) and torch.equal(lt, lt2) and torch.equal(loss2, lt2.mean())


# ---------------------------------------------------------------------------------------------------------------- 2. one-hot teacher == supervised
@pytest.mark.parametrize('kind,dtype', KINDS)
def test_one_hot_teacher_step_is_the_supervised_step(gpu_device, kind, dtype):
    B = 2
    cls, types = _labels(B)
    out = []
    for distill in (False, True):
        vae, m = _models(kind, dtype, gpu_device)
        tr = T.Trainer(m, vae, **KW)
        ctrl, img = _ids(vae, gpu_device, dtype, B)
        L, V = m.cfg.pyramid.L, m.cfg.vocab
        labels = _inputs(tr, ctrl, img, B)[1].to(gpu_device).long()
        hot = torch.full((B, L, V), -200.0, device=gpu_device)
        hot.scatter_(2, labels.view(B, L, 1), 0.0)
        log = []
        for _ in range(2):
            o = tr.step_tokens(img, ctrl, cls, types, distill=DistillLoss(hot) if distill else None)
            log.append((o['loss'].clone(), o['grad_norm'].clone(), _clone(tr.engine.grads()), _clone(m.state_dict())))
        out.append(log)
    for a, b in zip(*out):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        _same(a[2], b[2], 'grads')
        _same(a[3], b[3], 'parameters')
    assert any(not torch.equal(out[0][0][3][k], out[0][1][3][k]) for k in out[0][0][3])                  # the steps did move the parameters


# ---------------------------------------------------------------------------------------------------------------- 3. the accumulation window
@pytest.mark.parametrize('kind,dtype', [('joint', BF16), ('lora', BF16), ('joint', F32)])
def test_window_of_distillation_micro_batches_holds_the_sum(gpu_device, kind, dtype):
    B = 2
    cls, types = _labels(B)
    vae, m = _models(kind, dtype, gpu_device)
    ctrl, img = _ids(vae, gpu_device, dtype, B)
    L, V = m.cfg.pyramid.L, m.cfg.vocab
    teacher = _teacher_logits(B, L, V, gpu_device, seed=1)
    w = (torch.rand(B, L, generator=torch.Generator().manual_seed(8)) < 0.7).float().to(gpu_device)
    one = lambda t, b: [s[b:b + 1] for s in t]
    # the plain gradients of the two micro-batches, on the untouched parameters
    tr0 = T.Trainer(m, vae, **KW)
    plain = []
    for b in range(B):
        x, labels = _inputs(tr0, one(ctrl, b), one(img, b), 1)
        tr0.engine.forward_backward(cls[b:b + 1], x, types[b:b + 1], labels, distill=DistillLoss(teacher[b:b + 1], weights=w[b:b + 1]))
        plain.append(_clone(tr0.engine.grads()))
    assert any(bool((plain[0][k] != plain[1][k]).any()) for k in plain[0])
    vae2, m2 = _models(kind, dtype, gpu_device)
    tr = T.Trainer(m2, vae2, grad_accum=2, **KW)
    for b in range(B):
        o = tr.step_tokens(one(img, b), one(ctrl, b), cls[b:b + 1], types[b:b + 1], distill=DistillLoss(teacher[b:b + 1], weights=w[b:b + 1]))
        assert o['micro'] == b and o['synced'] == (b == 1)
    _same(tr.engine.grads(), {k: plain[0][k] + plain[1][k] for k in plain[0]}, 'window')


# ---------------------------------------------------------------------------------------------------------------- 4. the round trip
def _weighted_kl(tr, t, cls, types):
    """the weighted KL of the batch under the student as it stands: the training forward and a loss-only launch, nothing updated"""
    eng = tr.engine
    both, B, mf = tr._check_tokens(t.ids_img, t.ids_ctrl, cls, types, t.mask_first)
    x, _ = tr._inputs_of(both, B, mf)
    eng.forward_train(cls, x, types, None, mf)
    lt = torch.empty(eng.M, device=x.device)
    ops.kd_fwd_bwd(eng.logits, t.logits, eng.V, None, 1.0, lt, None, eng.M, eng.V)
    w = t.sampled.float().view(-1)
    return float((lt.double() * w).sum() / w.sum())


@pytest.mark.parametrize('call,kind', [('joint', 'lora'), ('conditional', 'joint')])
def test_round_trip_from_a_guided_teacher(gpu_device, call, kind):
    B, dtype = 2, BF16
    cls, types = _labels(B)
    vae, teacher = _models('joint', dtype, gpu_device, deterministic_plan=True)
    ctrl, _ = _ids(vae, gpu_device, dtype, B)
    pns, L, V = teacher.cfg.pyramid.patch_nums, teacher.cfg.pyramid.L, teacher.cfg.vocab
    n = sum(pn * pn for pn in pns)
    if call == 'joint':
        gen = lambda **kw: teacher.autoregressive_infer_cfg(B, cls, g_seed=5, cfg=4.0, top_k=900, top_p=0.95, cond_type=types, **kw)
    else:
        # one seed per row: the per-request path (the joint case above takes the scalar one)
        gen = lambda **kw: teacher.conditional_infer_cfg(B, cls, g_seed=[5, 6], cfg=(4.0, 4.0, 4.0), top_k=900, top_p=0.95, cond_type=types, c_mask=ctrl, **kw)
    images, t = gen(distill_targets=True)
    # the same call traced, without the targets: same images, and the trace is what the targets hold
    images2 = gen(_trace=True)
    tr_ = teacher.last_trace
    assert torch.equal(images, images2)
    assert t.logits.shape == (B, L, V) and t.logits.dtype == F32 and torch.equal(t.logits, torch.cat(tr_['logits'], dim=1))
    drawn = [i[:B] for i in tr_['idx']]                                     # the first branch's draw of every scale, before the overwrites
    first = torch.cat([i[:, :pn * pn] for i, pn in zip(drawn, pns)], dim=1)
    second = torch.cat([i[:, pn * pn:] for i, pn in zip(drawn, pns)], dim=1)
    assert t.mask_first is True and t.ids_img.shape == t.ids_ctrl.shape == (B, n)
    assert torch.equal(t.ids_img, second)
    col = torch.ones(L, dtype=torch.bool)
    if call == 'joint':
        assert torch.equal(t.ids_ctrl, first)
    else:
        given = torch.cat(ctrl, dim=1).to(torch.int32)
        assert torch.equal(t.ids_ctrl, given) and not torch.equal(first, given)        # the ids the branch CONTINUED with, not its draw
        b = 0
        for pn in pns:
            col[b:b + pn * pn] = False
            b += 2 * pn * pn
    assert t.sampled.dtype == torch.bool and torch.equal(t.sampled.cpu(), col[None].expand(B, L))
    # a student copy, four updates on the batch as it is
    vae_s, student = _models(kind, dtype, gpu_device)
    tr = T.Trainer(student, vae_s, peak_lr=1e-3, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=50, clip=2.0, drop_path=False)
    before = _weighted_kl(tr, t, cls, types)
    first_step = {}
    for s in range(4):
        o = tr.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=t.loss(), mask_first=t.mask_first)
        assert o['synced']
        if s == 0:
            first_step = dict(loss=o['loss'].clone(), grads=_clone(tr.engine.grads()))
    after = _weighted_kl(tr, t, cls, types)
    print(f'\n[distill_train] {call}: weighted KL of the batch {before:.5f} -> {after:.5f} after four updates')
    assert before > 0 and after < before
    # forced tokens contribute exactly zero: garbage in their teacher rows changes neither the loss nor any gradient
    vae_g, student_g = _models(kind, dtype, gpu_device)
    tr_g = T.Trainer(student_g, vae_g, peak_lr=1e-3, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=50, clip=2.0, drop_path=False)
    garbage = t.logits.clone()
    if call == 'conditional':
        noise = (torch.randn(B, L, V, generator=torch.Generator().manual_seed(2)) * 25).to(gpu_device)
        garbage = torch.where(t.sampled[..., None], garbage, noise)
        assert not torch.equal(garbage, t.logits)
    o = tr_g.step_tokens(t.ids_img, t.ids_ctrl, cls, types, distill=DistillLoss(garbage, weights=t.sampled), mask_first=True)
    assert torch.equal(o['loss'], first_step['loss'])
    _same(tr_g.engine.grads(), first_step['grads'], 'grads')
    if call == 'conditional':
        w = t.sampled.view(-1)
        assert not bool(tr_g.engine.dlogits[~w].any()) and bool(tr_g.engine.dlogits[w].any())


def test_plain_var_targets_train_a_plain_var(gpu_device):
    """the VAR form: one half, ids_ctrl None, and the targets feed step_tokens as they are; logprobs=True rides along"""
    from controlvar_amd import models
    B, dtype = 2, BF16
    cls, _ = _labels(B)
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(gpu_device)
    make = lambda: models.build_var(vae, depth=2, compute_dtype=dtype, cond_drop_rate=0.0, deterministic_plan=True).to(gpu_device).eval()
    teacher = make()
    L, V = teacher.cfg.pyramid.L, teacher.cfg.vocab
    images, scores, t = teacher.autoregressive_infer_cfg(B, cls, g_seed=[3, 4], cfg=4.0, top_k=900, top_p=0.95, logprobs=True, distill_targets=True)
    logits, ids = torch.cat(teacher.last_trace['logits'], dim=1), torch.cat(teacher.last_trace['idx'], dim=1)
    images2 = teacher.autoregressive_infer_cfg(B, cls, g_seed=[3, 4], cfg=4.0, top_k=900, top_p=0.95, _trace=True)
    assert torch.equal(images, images2) and torch.equal(t.logits, torch.cat(teacher.last_trace['logits'], dim=1)) and torch.equal(t.logits, logits)
    assert t.ids_ctrl is None and torch.equal(t.ids_img, ids) and tuple(t.logits.shape) == (B, L, V) and bool(t.sampled.all())
    assert torch.equal(scores.sampled, t.sampled)
    student = make()
    tr = T.Trainer(student, vae, peak_lr=1e-3, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=50, clip=2.0, drop_path=False)
    kls = [tr.step_tokens(t.ids_img, t.ids_ctrl, cls, None, distill=t.loss(), mask_first=t.mask_first)['loss'].item() for _ in range(4)]
    assert kls[0] > 0 and kls[-1] < kls[0], kls
