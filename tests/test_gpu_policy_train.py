"""Training on token ids and the policy-gradient step on MI355X: Trainer.step_tokens, Trainer.token_logprobs and
TrainEngine.forward_backward(policy=...) on the depth-2 models of test_gpu_grad_accum.py (tiny VQVAE, condition dropout off, B = 2 .. 4).

Almost every statement is bitwise, torch.equal with no tolerance: the token step IS the pixel step without its tokenizer, the policy step IS the
supervised step with another loss launch - everything behind dlogits is the same code on the same buffers - and the kernels are deterministic.  The two
statements that are not (the log-probability of a rewarded sequence rises, the KL estimate becomes positive) are inequalities with no bound to tune."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import ops, train as T  # noqa: E402
from controlvar_amd.train import PolicyLoss  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
KW = dict(peak_lr=2e-3, weight_decay=0.05, sche='lin0', warmup_it=2, max_it=50, clip=2.0, drop_path=False)      # test_gpu_grad_accum.KW
CLS = [17, 403, 5, 999]
TYPES = [2, 0, 1, 3]
_IDS = {}


def _models(kind, dtype, dev, lora_dropout=0.0):
    from controlvar_amd import lora, models
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    if kind == 'var':
        return vae, models.build_var(vae, depth=2, compute_dtype=dtype, cond_drop_rate=0.0).to(dev).eval()
    kw = dict(cos_attn=True) if kind == 'cos' else {}
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0, **kw).to(dev).eval()
    if kind == 'lora':
        lora.add_lora(m, r=16, dropout=lora_dropout, seed=1)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for _, (_, Bm) in lora.adapters(m).items():      # B = 0 would make every dA zero and hide half of the gradients
                Bm.copy_(torch.randn(Bm.shape, generator=g) * 0.05)
    return vae, m


def _batch(dev, B=4):
    from controlvar_amd.synth import synth_images
    return synth_images(4, 256, seed=6)[:B].to(dev), synth_images(4, 256, seed=7)[:B].to(dev), torch.tensor(CLS[:B]), torch.tensor(TYPES[:B])


def _ids(vae, dev, dtype, B):
    """(ids_ctrl, ids_img) of the batch as the one-pass tokenizer of Trainer.tokenize produces them: computed once per precision, shared, never changed"""
    key = (dtype, B)
    if key not in _IDS:
        images, masks, _, _ = _batch(dev, B)
        both = vae.img_to_idxBl(torch.cat((masks, images), dim=0))
        _IDS[key] = ([t[:B].clone() for t in both], [t[B:].clone() for t in both])
    return _IDS[key]


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def _same(a, b, what=''):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _adv(B, L, dev, seed=0):
    g = torch.Generator().manual_seed(40 + seed)
    a = torch.randn(B, L, generator=g)
    a[:, ::7] = 0.0
    return a.to(dev)


# ---------------------------------------------------------------------------------------------------------------- 1. tokens == pixels
@pytest.mark.parametrize('kind,dtype,accum', [('joint', BF16, 1), ('joint', F32, 1), ('cos', BF16, 1), ('lora', BF16, 1), ('joint', BF16, 2)])
def test_step_tokens_on_the_tokenizers_ids_is_step_bit_for_bit(gpu_device, kind, dtype, accum):
    B = 2
    images, masks, cls, types = _batch(gpu_device, B)
    runs = []
    for tokens in (False, True):
        vae, m = _models(kind, dtype, gpu_device)
        tr = T.Trainer(m, vae, grad_accum=accum, **KW)
        ctrl, img = _ids(vae, gpu_device, dtype, B)
        log = []
        for s in range(2 * accum):
            sl = slice(0, B) if accum == 1 else slice(s % 2, s % 2 + 1)         # a window of two micro-batches of one sample
            if tokens:
                form = (lambda t: torch.cat(t, 1).int()) if s else (lambda t: t)   # the list of img_to_idxBl, then one flat int32 tensor
                o = tr.step_tokens(form([t[sl] for t in img]), form([t[sl] for t in ctrl]), cls[sl], types[sl])
            else:
                o = tr.step(images[sl], masks[sl], cls[sl], types[sl])
            log.append((o['loss'].clone(), o['synced'], o['micro'], o['lr'], o['wd'], None if o['grad_norm'] is None else o['grad_norm'].clone(),
                        _clone(tr.engine.grads()), _clone(m.state_dict())))
        assert tr.it == 2
        runs.append(log)
    for a, b in zip(*runs):
        assert torch.equal(a[0], b[0]) and a[1:5] == b[1:5] and (a[5] is None) == (b[5] is None) and (a[5] is None or torch.equal(a[5], b[5]))
        _same(a[6], b[6], 'grads')
        _same(a[7], b[7], 'parameters')
    assert any(not torch.equal(runs[0][0][7][k], runs[0][-1][7][k]) for k in runs[0][0][7])              # the steps did move the parameters


def test_step_tokens_trains_a_plain_var(gpu_device):
    """step() has no pixel entrance for a plain VAR (its tokenizer pass stacks a control half): the token step is held to the engine and optimizer calls
    it is made of, on x = idxBl_to_h(ids)"""
    B = 2
    images, _, cls, _ = _batch(gpu_device, B)
    out = []
    for tokens in (False, True):
        vae, m = _models('var', BF16, gpu_device)
        tr = T.Trainer(m, vae, **KW)
        idx = vae.img_to_idxBl(images)
        for _ in range(2):
            if tokens:
                o = tr.step_tokens(idx, None, cls, None)
                loss = o['loss']
            else:
                s = tr.sched
                T.lr_wd_annealing(s['sche'], tr.opt, s['peak_lr'], s['wd'], s['wd_end'], tr.it, s['wp_it'], s['max_it'], wp0=s['wp0'], wpe=s['wpe'])
                loss, _ = tr.engine.forward_backward(cls, torch.cat(vae.idxBl_to_h(idx), 1), None, torch.cat(idx, 1))
                tr.opt.step(tr.engine.grads(), tr.clip, 1, 1)
                tr.engine._transposed_weights()
                tr.it += 1
        out.append((loss.clone(), _clone(tr.engine.grads()), _clone(m.state_dict())))
    assert torch.equal(out[0][0], out[1][0])
    _same(out[0][1], out[1][1], 'grads')
    _same(out[0][2], out[1][2], 'parameters')


# ---------------------------------------------------------------------------------------------------------------- 2. / 3. the policy step at ratio 1
@pytest.mark.parametrize('kind', ['joint', 'lora'])
def test_policy_step_with_unit_advantages_is_the_supervised_step(gpu_device, kind):
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    out = []
    for policy in (False, True):
        vae, m = _models(kind, BF16, gpu_device)
        tr = T.Trainer(m, vae, **KW)
        ctrl, img = _ids(vae, gpu_device, BF16, B)
        for _ in range(2):
            o = tr.step_tokens(img, ctrl, cls, types, policy=PolicyLoss(torch.ones(B)) if policy else None)
        out.append((o['loss'].clone(), _clone(tr.engine.grads()), _clone(m.state_dict()), o))
    assert torch.equal(out[0][0], out[1][0])
    _same(out[0][1], out[1][1], 'grads')
    _same(out[0][2], out[1][2], 'parameters')
    o = out[1][3]
    assert o['mean_ratio'].item() == 1.0 and o['clip_frac'].item() == 0.0 and o['mean_kl'].item() == 0.0 and o['token_logprob'].shape == (B, m.cfg.pyramid.L)
    assert 'mean_ratio' not in out[0][3]


def test_old_logprob_from_token_logprobs_gives_ratio_one(gpu_device):
    """train() mode, DropPath and adapter dropout on, one drop_seed: the scoring forward IS the training forward, so every ratio is exactly 1.0f and the
    step equals the one without old_logprob - gradients and parameters; the reported loss differs by design (min(s1, s2) = A against the surrogate A lp)"""
    B = 3
    _, _, cls, types = _batch(gpu_device, B)
    out = []
    for with_old in (False, True):
        vae, m = _models('lora', BF16, gpu_device, lora_dropout=0.1)
        m.cfg = dataclasses.replace(m.cfg, drop_path_rate=0.5)      # the factory's 0.1 * 2 / 24 would hardly ever drop a row: make DropPath bite
        tr = T.Trainer(m, vae, train_mode=True, **dict(KW, drop_path=True))
        ctrl, img = _ids(vae, gpu_device, BF16, B)
        adv = _adv(B, m.cfg.pyramid.L, gpu_device)
        old = tr.token_logprobs(img, ctrl, cls, types, drop_seed=11).clone() if with_old else None
        if with_old:
            assert not torch.equal(old, tr.token_logprobs(img, ctrl, cls, types, drop_seed=12))           # the seed does matter
        o = tr.step_tokens(img, ctrl, cls, types, policy=PolicyLoss(adv, old_logprob=old, clip=(0.0, 0.0)), drop_seed=11)
        po = tr.engine.policy_out
        assert bool((po['ratio'] == 1.0).all()) and not bool(po['clipped'].any())
        if with_old:
            assert torch.equal(o['token_logprob'], old)
        out.append((_clone(tr.engine.grads()), _clone(m.state_dict()), tr.engine.dlogits.clone()))
    assert torch.equal(out[0][2], out[1][2])
    _same(out[0][0], out[1][0], 'grads')
    _same(out[0][1], out[1][1], 'parameters')


# ---------------------------------------------------------------------------------------------------------------- 4. only the loss kernel changed
@pytest.mark.parametrize('kind,dtype', [('joint', BF16), ('joint', F32), ('lora', BF16)])
def test_general_policy_step_is_the_walk_with_another_loss_launch(gpu_device, kind, dtype):
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    vae, m = _models(kind, dtype, gpu_device)
    tr = T.Trainer(m, vae, **KW)
    eng = tr.engine
    ctrl, img = _ids(vae, gpu_device, dtype, B)
    L = m.cfg.pyramid.L
    lp = tr.token_logprobs(img, ctrl, cls, types).clone()
    g = torch.Generator().manual_seed(5)
    old = lp + 0.4 * torch.randn(B, L, generator=g).to(gpu_device)                    # ratios on both sides of the window [0.8, 1.3]
    ref = lp + 0.3 * torch.randn(B, L, generator=g).to(gpu_device)
    mask = (torch.rand(B, L, generator=g) < 0.8).float().to(gpu_device)
    pol = PolicyLoss(_adv(B, L, gpu_device), old_logprob=old, ref_logprob=ref, clip=(0.2, 0.3), kl_coef=0.05)
    x, labels = tr._inputs_of([torch.cat((c, i), 0) for c, i in zip(ctrl, img)], B, True)
    loss, loss_tok = eng.forward_backward(cls, x, types, labels, mask, policy=pol)
    po, grads, dlogits, loss_tok = _clone(eng.policy_out), _clone(eng.grads()), eng.dlogits.clone(), loss_tok.clone()
    assert 0 < int(po['clipped'].sum()) < B * L and torch.equal(po['logprob'].view(B, L), lp)
    # the kernel on the engine's logits, by hand
    M, V = eng.M, eng.V
    w = mask.view(-1)
    gscale = 1.0 / (M * (float(w.mean()) + 1e-6))
    adv, o_, r_ = pol.rows(B, L, gpu_device)
    lt, dl, coef = torch.empty(M, device=gpu_device), torch.empty_like(dlogits), torch.empty(M, device=gpu_device)
    tg = labels.to(torch.int32).contiguous().view(-1)
    ops.pg_fwd_bwd(eng.logits, tg, adv, w, o_, r_, 0.2, 0.3, 0.05, gscale, lt, M, V, dlogits=dl, coef=coef)
    assert torch.equal(dl, dlogits) and torch.equal(lt, loss_tok) and torch.equal(coef, po['coef'])
    assert torch.equal(loss, (loss_tok * w).mean() / (w.mean() + 1e-6))
    # the model-free statement: forward + cross-entropy weighted by the kernel's own c * w + backward give the same gradients
    eng.forward_train(cls, x, types, None, True)
    ops.ce_fwd_bwd(eng.logits, tg, po['coef'], gscale, eng.loss_tok, eng.dlogits, M, V)
    assert torch.equal(eng.dlogits, dlogits)
    eng.backward()
    _same(eng.grads(), grads, 'grads')


# ---------------------------------------------------------------------------------------------------------------- 5. / 6. the loop closes
def test_rewarded_sequence_rises_and_punished_one_falls(gpu_device):
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    vae, m = _models('lora', BF16, gpu_device)
    tr = T.Trainer(m, vae, peak_lr=2e-3, weight_decay=0.0, sche='lin0', warmup_it=0, max_it=50, clip=2.0, drop_path=False)
    ctrl, img = _ids(vae, gpu_device, BF16, B)
    before = tr.token_logprobs(img, ctrl, cls, types).sum(1)
    adv = torch.tensor([1.0, -1.0])
    for _ in range(6):
        old = tr.token_logprobs(img, ctrl, cls, types).clone()
        o = tr.step_tokens(img, ctrl, cls, types, policy=PolicyLoss(adv, old_logprob=old, kl_coef=0.0))
        assert o['mean_ratio'].item() == 1.0 and o['synced']
    after = tr.token_logprobs(img, ctrl, cls, types).sum(1)
    print(f'\n[policy_train] sum of token log-probabilities: +1 {before[0].item():.2f} -> {after[0].item():.2f}   -1 {before[1].item():.2f} -> {after[1].item():.2f}')
    assert after[0].item() > before[0].item() and after[1].item() < before[1].item()


def test_kl_is_zero_at_the_reference_and_positive_after(gpu_device):
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    vae, m = _models('lora', BF16, gpu_device)
    tr = T.Trainer(m, vae, **KW)
    ctrl, img = _ids(vae, gpu_device, BF16, B)
    ref = tr.token_logprobs(img, ctrl, cls, types).clone()
    kls = []
    for _ in range(3):
        o = tr.step_tokens(img, ctrl, cls, types, policy=PolicyLoss(torch.tensor([1.0, -0.5]), ref_logprob=ref, kl_coef=0.05))
        kls.append(o['mean_kl'].item())
    assert kls[0] == 0.0 and kls[1] > 0.0 and kls[2] > 0.0, kls


# ---------------------------------------------------------------------------------------------------------------- 7. / 8. state
def test_resume_in_the_middle_of_a_policy_run(gpu_device, tmp_path):
    from controlvar_amd import checkpoint as ckpt
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    vae, m = _models('joint', BF16, gpu_device)
    tr = T.Trainer(m, vae, **KW)
    ctrl, img = _ids(vae, gpu_device, BF16, B)
    L = m.cfg.pyramid.L
    ref = tr.token_logprobs(img, ctrl, cls, types).clone()

    def step(t, s):
        old = t.token_logprobs(img, ctrl, cls, types).clone()
        return t.step_tokens(img, ctrl, cls, types, policy=PolicyLoss(_adv(B, L, gpu_device, s), old_logprob=old, ref_logprob=ref, kl_coef=0.05))
    for s in range(2):
        step(tr, s)
    path = ckpt.save_checkpoint(m, tr.opt, epoch=0, step=tr.it, save_dir=str(tmp_path), latest=True)
    want = step(tr, 2)
    want_sd = _clone(m.state_dict())
    vae2, m2 = _models('joint', BF16, gpu_device)
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(0.01)                        # the resumed values come from the file
    tr2 = T.Trainer(m2, vae2, **KW)
    steps, _ = ckpt.resume(m2, tr2.opt, path)
    assert steps == 2
    tr2.it = steps
    got = step(tr2, 2)
    for k in ('loss', 'mean_ratio', 'clip_frac', 'mean_kl', 'token_logprob', 'grad_norm'):
        assert torch.equal(got[k], want[k]), k
    assert got['lr'] == want['lr'] and want['mean_kl'].item() > 0.0
    _same(_clone(m2.state_dict()), want_sd, 'parameters')


def test_token_logprobs_leaves_gradients_and_the_window_alone(gpu_device):
    B = 2
    _, _, cls, types = _batch(gpu_device, B)
    out = []
    for score in (False, True):
        vae, m = _models('joint', BF16, gpu_device)
        tr = T.Trainer(m, vae, grad_accum=2, **KW)
        ctrl, img = _ids(vae, gpu_device, BF16, B)
        o = tr.step_tokens(img, ctrl, cls, types)
        assert not o['synced'] and tr.window.micro == 1 and tr.it == 0
        grads, params = _clone(tr.engine.grads()), _clone(m.state_dict())
        if score:
            lp = tr.token_logprobs([t[:1] for t in img], [t[:1] for t in ctrl], cls[:1], types[:1])       # another batch size on the way
            assert lp.shape == (1, m.cfg.pyramid.L) and lp.dtype == F32 and bool(torch.isfinite(lp).all())
            assert tr.window.micro == 1 and tr.it == 0
            _same(tr.engine.grads(), grads, 'grads')
            _same(m.state_dict(), params, 'parameters')
        o = tr.step_tokens(img, ctrl, cls, types)
        assert o['synced'] and tr.it == 1
        out.append((_clone(tr.engine.grads()), _clone(m.state_dict())))
    _same(out[0][0], out[1][0], 'grads')
    _same(out[0][1], out[1][1], 'parameters')
