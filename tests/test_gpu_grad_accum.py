"""Gradient accumulation through the training step on MI355X: TrainEngine.forward_backward(accumulate=...) and
Trainer(grad_accum=N).

The models are those of test_gpu_dp_two_ranks.py (tiny VQVAE, depth-2 transformer, DropPath and condition dropout off, a batch of 4 synthetic
images).  Two kinds of statement:
* bitwise - a window holds exactly the sum, in micro-batch order, of what the plain calls produce for its micro-batches (the kernel contract
  fp32(old + plain) carried through every gradient of every model variant), so torch.equal with no tolerance;
* against the concatenated batch - two micro-batches of 2 are two ranks of 2 summed in another place, so the bounds are exactly those
  test_gpu_dp_two_ranks.py puts on the same arithmetic."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
KW = dict(peak_lr=2e-3, weight_decay=0.05, sche='lin0', warmup_it=2, max_it=50, clip=2.0, drop_path=False)      # test_gpu_dp_two_ranks.KW
CLS = [17, 403, 5, 999]
TYPES = [2, 0, 1, 3]
SIZES = [(0, 1), (1, 3), (3, 4)]        # micro-batches of 1, 2, 1: T = 1360 < 1536 tokens takes the one-slice weight-gradient GEMM, T = 2720 the token split

VARIANTS = {'joint': {}, 'cos': dict(cos_attn=True), 'shared_aln': dict(shared_aln=True), 'type_pos': dict(type_pos=True), 'separator': dict(separator=True)}


def _models(kind, dtype, dev):
    from controlvar_amd import lora, models
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    if kind == 'var':
        return vae, models.build_var(vae, depth=2, compute_dtype=dtype, cond_drop_rate=0.0).to(dev).eval()
    kw = VARIANTS['joint' if kind == 'lora' else kind]
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0, **kw).to(dev).eval()
    if kind == 'lora':
        lora.add_lora(m, r=16, dropout=0.0, seed=1)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for _, (_, B) in lora.adapters(m).items():      # B = 0 would make every dA zero and hide half of the gradients
                B.copy_(torch.randn(B.shape, generator=g) * 0.05)
    return vae, m


def _images(dev):
    from controlvar_amd.synth import synth_images
    return synth_images(4, 256, seed=6).to(dev), synth_images(4, 256, seed=7).to(dev), torch.tensor(CLS), torch.tensor(TYPES)


def _tokens(kind, vae, m, dev):
    """(engine, cls, x, types, labels) of the batch of 4"""
    from controlvar_amd import train as T
    images, masks, cls, types = _images(dev)
    if kind == 'var':
        idx = vae.img_to_idxBl(images)
        return T.TrainEngine(m, drop_path=False), cls, torch.cat(vae.idxBl_to_h(idx), 1), None, torch.cat(idx, 1)
    tr = T.Trainer(m, vae, **KW)
    x, labels = tr.tokenize(images, masks)
    return tr.engine, cls, x, types, labels


def _clone(grads):
    return {k: v.clone() for k, v in grads.items()}


def _sl(t, a, b):
    return None if t is None else t[a:b]


def _plain_sum(eng, cls, x, types, labels, masks=None):
    """the reference of the bitwise tests: the plain gradients of the three micro-batches, added by torch in micro-batch order"""
    plain, losses = [], []
    for a, b in SIZES:
        loss, _ = eng.forward_backward(cls[a:b], x[a:b], _sl(types, a, b), labels[a:b], _sl(masks, a, b))
        plain.append(_clone(eng.grads())); losses.append(loss.clone())
    return {k: (plain[0][k] + plain[1][k]) + plain[2][k] for k in plain[0]}, plain, losses


def _window(eng, cls, x, types, labels, masks=None):
    losses = []
    for k, (a, b) in enumerate(SIZES):
        loss, _ = eng.forward_backward(cls[a:b], x[a:b], _sl(types, a, b), labels[a:b], _sl(masks, a, b), accumulate=k > 0)
        losses.append(loss.clone())
    return losses


# ---------------------------------------------------------------------------------------------------------------- 1. bitwise against the plain path
@pytest.mark.parametrize('kind,dtype', [('joint', BF16), ('joint', F32), ('var', BF16), ('cos', BF16), ('shared_aln', BF16), ('shared_aln', F32),
                                        ('type_pos', F32), ('separator', BF16), ('lora', BF16)])
def test_window_is_the_sum_of_the_plain_gradients_bit_for_bit(gpu_device, kind, dtype):
    vae, m = _models(kind, dtype, gpu_device)
    eng, cls, x, types, labels = _tokens(kind, vae, m, gpu_device)
    expect, plain, plain_losses = _plain_sum(eng, cls, x, types, labels)
    assert all(torch.isfinite(v).all() for v in expect.values())
    assert sum(int((plain[0][k] != plain[1][k]).any()) for k in expect) > len(expect) // 2      # the micro-batches do differ
    buffers = [b.data_ptr() for b in eng.buckets]
    losses = _window(eng, cls, x, types, labels)
    assert [b.data_ptr() for b in eng.buckets] == buffers                  # the batch size changed twice: the gradient buffers stayed
    got = eng.grads()
    assert set(got) == set(expect)
    assert {n for n, p in m.named_parameters() if p.requires_grad} <= set(got)
    for k in expect:
        assert torch.equal(got[k], expect[k]), (kind, k, float((got[k] - expect[k]).abs().max()))
    for a, b in zip(losses, plain_losses):                                 # the loss of a micro-batch is its own
        assert torch.equal(a, b)
    # and the first micro-batch of the next window overwrites: no term of this one survives
    eng.forward_backward(cls[:1], x[:1], _sl(types, 0, 1), labels[:1])
    for k in expect:
        assert torch.equal(eng.grads()[k], plain[0][k]), k


def test_a_window_after_a_poisoned_one_is_clean(gpu_device):
    """NaN inputs poison a whole window; the next window starts from overwriting stores everywhere (the staging copies included)"""
    vae, m = _models('shared_aln', BF16, gpu_device)
    eng, cls, x, types, labels = _tokens('shared_aln', vae, m, gpu_device)
    expect, _, _ = _plain_sum(eng, cls, x, types, labels)
    _window(eng, cls, torch.full_like(x, float('nan')), types, labels)
    poisoned = eng.grads()
    assert sum(int(torch.isnan(v).any()) for v in poisoned.values()) > len(poisoned) // 2
    _window(eng, cls, x, types, labels)
    for k, v in eng.grads().items():
        assert torch.equal(v, expect[k]), k


# ---------------------------------------------------------------------------------------------------------------- 2. against the concatenated batch
@pytest.mark.parametrize('dtype', [F32, BF16])
def test_two_micro_batches_of_two_equal_one_step_on_the_batch_of_four(gpu_device, dtype):
    """every bound below is the one test_gpu_dp_two_ranks.py uses for two ranks of 2 against one process on 4"""
    from controlvar_amd import train as T
    STEPS = 2
    images, masks, cls, types = _images(gpu_device)
    vae, m = _models('joint', dtype, gpu_device)
    tr = T.Trainer(m, vae, grad_accum=2, **KW)
    acc, g_acc = [], None
    for step in range(STEPS):
        o0 = tr.step(images[:2], masks[:2], cls[:2], types[:2])
        assert o0['synced'] is False and o0['micro'] == 0 and o0['grad_norm'] is None and tr.it == step
        o1 = tr.step(images[2:], masks[2:], cls[2:], types[2:])
        assert o1['synced'] is True and o1['micro'] == 1 and tr.it == step + 1
        torch.cuda.synchronize()
        assert torch.equal(o1['window_loss'], (o0['loss'] + o1['loss']) / 2)                # the mean of the micro-batch losses
        acc.append((float(o1['window_loss']), float(o1['grad_norm'])))
        if step == 0:
            g_acc = {k: v.detach().float().cpu().clone() for k, v in tr.engine.grads().items()}          # the SUM over the window
    sd_acc = {k: v.detach().cpu() for k, v in m.state_dict().items()}

    vae1, m1 = _models('joint', dtype, gpu_device)
    tr1 = T.Trainer(m1, vae1, **KW)
    single, g1 = [], None
    for step in range(STEPS):
        out = tr1.step(images, masks, cls, types)
        torch.cuda.synchronize()
        assert out['synced'] is True and out['micro'] == 0
        single.append((float(out['loss']), float(out['grad_norm'])))
        if step == 0:
            g1 = {k: v.detach().float().cpu().clone() for k, v in tr1.engine.grads().items()}
    fp32 = dtype == F32
    for step in range(STEPS):
        tol = (2e-5 if fp32 else 5e-3) * (1 if step == 0 else 3)
        print(f'[accum] {dtype} step {step}: window loss {acc[step][0]:.6f} / {single[step][0]:.6f}, grad norm {acc[step][1]:.6f} / {single[step][1]:.6f}')
        assert abs(acc[step][0] - single[step][0]) < tol, (step, acc[step][0], single[step][0])
        assert abs(acc[step][1] - single[step][1]) < (1e-4 if fp32 else 2e-2) * max(1.0, single[step][1]) * (1 if step == 0 else 3)
    worst_g = 0.0
    for k_, g in g1.items():
        sc = max(float(g.abs().max()), 1e-6)
        err = float((g_acc[k_] / 2 - g).abs().max()) / sc
        worst_g = max(worst_g, err)
        assert err < (2e-4 if fp32 else 6e-2), (k_, err)
    lr_total = sum(KW['peak_lr'] for _ in range(STEPS))
    sd = {k: v.detach().cpu() for k, v in m1.state_dict().items()}
    names = dict(m1.named_parameters())
    tot, far, worst_p = 0, 0, 0.0
    for k_, v in sd.items():
        if not v.is_floating_point() or k_ not in names:
            assert torch.equal(v, sd_acc[k_]), k_
            continue
        d = (v.float() - sd_acc[k_].float()).abs()
        worst_p = max(worst_p, float(d.max()))
        assert float(d.max()) <= 2.001 * lr_total, (k_, float(d.max()))
        tot += d.numel()
        far += int((d > (1e-2 if fp32 else 0.25) * lr_total).sum())
    print(f'[accum] {dtype}: worst gradient distance {worst_g:.2e}, worst parameter distance {worst_p:.2e}, {far} of {tot} beyond the bulk bound')
    assert far <= (1e-3 if fp32 else 5e-2) * tot, (far, tot)


# ---------------------------------------------------------------------------------------------------------------- 3. bookkeeping
def test_trainer_window_bookkeeping(gpu_device):
    from controlvar_amd import train as T
    images, masks, cls, types = _images(gpu_device)
    vae, m = _models('joint', BF16, gpu_device)
    tr = T.Trainer(m, vae, grad_accum=3, **KW)
    probe = dict(m.named_parameters())['blocks.0.ffn.fc1.weight']
    s = tr.sched
    for call in range(6):
        before, it = probe.detach().clone(), tr.it
        a = 2 * (call % 2)
        out = tr.step(images[a:a + 2], masks[a:a + 2], cls[a:a + 2], types[a:a + 2])
        assert out['micro'] == call % 3 and out['synced'] is (call % 3 == 2)
        assert it == call // 3 and tr.it == (call + 1) // 3
        assert out['lr'] == T.lr_wd_factors(s['sche'], s['peak_lr'], s['wd'], s['wd_end'], it, s['wp_it'], s['max_it'], s['wp0'], s['wpe'])[0]
        assert torch.isfinite(out['loss'])
        if out['synced']:
            assert not torch.equal(probe.detach(), before) and torch.isfinite(out['grad_norm']) and torch.isfinite(out['window_loss'])
        else:
            assert torch.equal(probe.detach(), before) and out['grad_norm'] is None and out['clip_coef'] is None
    assert tr.opt.steps == 2


def test_grad_accum_one_is_the_default_trainer_bit_for_bit(gpu_device):
    from controlvar_amd import train as T
    images, masks, cls, types = _images(gpu_device)
    states = []
    for kw in ({}, dict(grad_accum=1)):
        vae, m = _models('joint', BF16, gpu_device)
        tr = T.Trainer(m, vae, **kw, **KW)
        outs = [tr.step(images, masks, cls, types) for _ in range(2)]
        assert all(o['synced'] and o['micro'] == 0 for o in outs) and tr.it == 2
        assert all(torch.equal(o['window_loss'], o['loss']) for o in outs)
        states.append(({k: v.clone() for k, v in m.state_dict().items()}, [float(o['loss']) for o in outs], [float(o['grad_norm']) for o in outs]))
    assert states[0][1:] == states[1][1:]
    for k in states[0][0]:
        assert torch.equal(states[0][0][k], states[1][0][k]), k


# ---------------------------------------------------------------------------------------------------------------- 4. reducer
def test_one_all_reduce_pass_per_window(gpu_device):
    """force_reducer=True in a one-rank RCCL group (as tests/test_dp_runtime.py runs the plain step): the slabs travel once per window, in the
    micro-batch that closes it, and - SUM over one rank being the identity - leave the model bit-identical to the un-reduced window's"""
    import torch.distributed as dist
    from controlvar_amd import train as T
    os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
    os.environ.setdefault('MASTER_PORT', str(29300 + os.getpid() % 90))
    created = False
    if not dist.is_initialized():
        dist.init_process_group('nccl', rank=0, world_size=1, device_id=gpu_device)
        created = True
    try:
        images, masks, cls, types = _images(gpu_device)
        states = []
        for force in (False, True):
            vae, m = _models('joint', BF16, gpu_device)
            tr = T.Trainer(m, vae, grad_accum=2, force_reducer=force, **KW)
            outs = []
            for call in range(4):
                a = 2 * (call % 2)
                outs.append(tr.step(images[a:a + 2], masks[a:a + 2], cls[a:a + 2], types[a:a + 2]))
                if force and call % 2 == 0:
                    assert tr.engine.reducer is None                       # nothing is exchanged inside a window
            torch.cuda.synchronize()
            states.append(({k: v.clone() for k, v in m.state_dict().items()}, [float(o['loss']) for o in outs]))
            if force:
                red = tr.engine.reducer
                assert red is not None and red.active and red.stream is not None
                assert red.bytes_sent == 2 * sum(b.numel() * 4 for b in tr.engine.buckets)       # two windows, one pass each - not four
        assert states[0][1] == states[1][1]
        for k in states[0][0]:
            assert torch.equal(states[0][0][k], states[1][0][k]), k
    finally:
        if created:
            dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- 5. ignore_mask
def test_ignore_mask_per_micro_batch(gpu_device):
    """each micro-batch normalises by ITS mask ((loss * w).mean() / (w.mean() + 1e-6) over that micro-batch alone): the window is the sum of the
    per-micro-batch plain gradients, and the reported window loss the mean of the micro-batch losses"""
    from controlvar_amd import train as T
    vae, m = _models('joint', F32, gpu_device)
    eng, cls, x, types, labels = _tokens('joint', vae, m, gpu_device)
    g = torch.Generator().manual_seed(11)
    keep = torch.tensor([0.3, 0.5, 0.7, 0.9]).view(4, 1)
    masks = (torch.rand(4, labels.shape[1], generator=g) < keep).float().to(gpu_device)        # a different mask (and density) per sample
    expect, _, plain_losses = _plain_sum(eng, cls, x, types, labels, masks)
    losses = _window(eng, cls, x, types, labels, masks)
    for k, v in eng.grads().items():
        assert torch.equal(v, expect[k]), k
    assert all(torch.equal(a, b) for a, b in zip(losses, plain_losses))
    assert len({float(v) for v in losses}) == 3
    images, imasks, _, _ = _images(gpu_device)
    tr = T.Trainer(m, vae, grad_accum=2, **KW)
    o0 = tr.step(images[:2], imasks[:2], cls[:2], types[:2], ignore_mask=masks[:2])
    o1 = tr.step(images[2:], imasks[2:], cls[2:], types[2:], ignore_mask=masks[2:])
    assert not o0['synced'] and o1['synced']
    assert torch.equal(o1['window_loss'], (o0['loss'] + o1['loss']) / 2)
