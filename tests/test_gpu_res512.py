"""512 x 512 images (32 x 32 latents, PATCH_NUMS_512) on the GPU: the S = 32 quantizer kernels of csrc/msq.hip against the reference's recording
(res512_*.npz, tests/golden/make_golden_512.py) and the CPU oracle, and every layer above them at the new size - public tokenizer API, the
wide decoder, generation, one training step.  The last test pins the untouched S = 16 kernels to a recording of the previous library."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import golden, ids_parity, maxabs_on  # noqa: E402
from controlvar_amd import models, ops  # noqa: E402
from controlvar_amd import train as T  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS, PATCH_NUMS_512 as PN, VaeConfig, VarConfig, phi_index_map  # noqa: E402
from controlvar_amd.synth import synth_images, synth_vae_state, synth_var_state  # noqa: E402
from oracle import train_ref, var_ref, vqvae_ref  # noqa: E402
from oracle.vqvae_ref import MSQuant, Prec  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
ALT = (1, 2, 5, 11, 23, 32)
CROP = (slice(None), slice(None), slice(200, 216), slice(120, 136))          # the crop make_golden_512.py records


def t(a):
    return torch.from_numpy(np.asarray(a))


def make_vae(ch, dtype, dev, pns=PN):
    return models.build_vae(ch=ch, compute_dtype=dtype, v_patch_nums=pns).to(dev)


def oracle_q(pns=PN):
    return MSQuant(synth_vae_state(VaeConfig(ch=32, patch_nums=pns)), pns, phi_index_map(len(pns)))


def split(ids, pns):
    return list(torch.split(t(ids).long(), [p * p for p in pns], dim=1))


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ------------------------------------------------------------------------------ 1. fixture replay
def test_ms_encode_on_reference_features_32(gpu_device):
    """the reference's f (1, 32, 32, 32) -> the reference's 2 240 ids (strict), its final f_hat (<= 1e-4) and the oracle's margins (<= 1e-3):
    the bounds of test_ms_encode_bit_exact_on_reference_features"""
    g = golden('res512_a')
    vae = make_vae(32, F32, gpu_device)
    idx, fh, mg = vae._ms_encode(t(g['f']).to(gpu_device), want_fhat=True, want_margin=True)
    _, margins = oracle_q().f_to_idx(t(g['f']), return_margins=True)
    margins = torch.cat(margins, 1)
    n, ok = ids_parity(idx.cpu(), g['ids'], margins.numpy(), 1e-4, 'ms_encode S=32 on the reference features', strict=True)
    assert maxabs_on(fh.cpu() - t(g['fhat_last']), ok) < 1e-4
    assert maxabs_on(mg.cpu() - margins, ok) < 1e-3
    idx2, fh2, _ = vae._ms_encode(t(g['f']).to(gpu_device), want_fhat=True)                     # the matrix-pipe search
    assert torch.equal(idx2, idx) and torch.equal(fh2, fh)
    assert torch.equal(vae._ms_encode(t(g['f']).to(gpu_device))[0], idx)                        # and without f_hat_out


# ------------------------------------------------------------------------------ 2. random features
@pytest.mark.parametrize('pns,B,amp,seed', [(PN, 1, 0.5, 1), (PN, 3, 1.0, 2), (ALT, 1, 0.5, 1)])
def test_ms_encode_random_features_against_oracle_32(gpu_device, pns, B, amp, seed):
    """both search paths on random 32 x 32 maps, strict.  The oracle's smallest top-1/top-2 margin in these cases is 3.7e-4, 4.4e-4 and 9.1e-4
    (computed on the CPU), at least 3x the 1e-4 max(1, amp^2) rounding threshold of the 16 x 16 test: no token is near a tie, a flip is a bug."""
    vae = make_vae(32, F32, gpu_device, pns)
    f = torch.randn(B, 32, 32, 32, generator=torch.Generator().manual_seed(seed)) * amp
    ids_ref, margins = oracle_q(pns).f_to_idx(f, return_margins=True)
    ref, mref = torch.cat(ids_ref, 1).numpy(), torch.cat(margins, 1).numpy()
    assert mref.min() > 3e-4 * max(1.0, amp * amp)
    fd = f.to(gpu_device)
    for want_margin in (False, True):
        idx, fh, mg = vae._ms_encode(fd, want_fhat=True, want_margin=want_margin)
        ids_parity(idx.cpu(), ref, mref, 1e-4 * max(1.0, amp * amp), f'ms_encode S=32 random features {pns[-2]} B={B} margins={want_margin}', strict=True)
        if want_margin:
            assert float((mg.cpu() - t(mref)).abs().max()) < 1e-3 * max(1.0, amp * amp)
    # a caller-chosen list through _scale_tables equals the list as the constructor's
    if pns == ALT:
        other = make_vae(32, F32, gpu_device)._ms_encode(fd, want_fhat=True, v_patch_nums=ALT)
        assert torch.equal(other[0], idx) and torch.equal(other[1], fh)


# ------------------------------------------------------------------------------ 3. fast search == sequential search
def test_ms_encode_fast_search_equals_sequential_search_incl_ties_32(gpu_device):
    """as test_ms_encode_fast_search_equals_sequential_search_incl_ties: the second half of the codebook repeats the first, every minimum has an exact
    tie 2048 entries later; the matrix-pipe search (however its work is split at a scale) and the sequential search pick the lower index"""
    vae = make_vae(32, BF16, gpu_device)
    sd = vae.state_dict()
    E = sd['quantize.embedding.weight'].clone()
    E[2048:] = E[:2048]
    sd['quantize.embedding.weight'] = E
    vae.load_state_dict(sd)
    vae._packed = None
    f = (torch.randn(3, 32, 32, 32, generator=torch.Generator().manual_seed(4)) * 0.6).to(gpu_device)
    slow = vae._ms_encode(f, want_fhat=True, want_margin=True)
    fast = vae._ms_encode(f, want_fhat=True, want_margin=False)
    assert torch.equal(slow[0], fast[0]) and torch.equal(slow[1], fast[1])
    assert int(fast[0].max()) < 2048
    assert float(slow[2].min()) == 0.0 and float(slow[2].max()) == 0.0


# ------------------------------------------------------------------------------ 4. next input
@pytest.mark.parametrize('pns', [PN, ALT])
def test_next_input_every_scale_32(gpu_device, pns):
    """get_next_autoregressive_input at every scale against the oracle (<= 2e-5) on arbitrary h (a one-off codebook, as the 16 x 16 test does);
    nb = 3, nmaps = 2 bit-identical to the single map; an explicit pn_next equal to the scale; NaN fences around f_hat and the tokens stay NaN"""
    dev = gpu_device
    vae = make_vae(32, F32, dev, pns)
    q = oracle_q(pns)
    P = vae._pack()
    gen = torch.Generator().manual_seed(5)
    MAP = 32 * 32 * 32
    for si, pn in enumerate(pns):
        last = si == len(pns) - 1
        f0 = torch.randn(1, 32, 32, 32, generator=gen)
        h = torch.randn(1, 32, pn, pn, generator=gen)
        soft = h.reshape(1, 32, pn * pn).transpose(1, 2).contiguous()                      # (1, pn*pn, 32)
        f_ref, nxt = q.next_input(si, f0, h)
        f_hat = f0.to(dev).view(1, 1, 32, 32, 32).clone()
        tok = vae._next_input(si, None, f_hat, 1, 1, True, soft=soft.to(dev))
        assert float((f_hat.cpu().view(1, 32, 32, 32) - f_ref).abs().max()) <= 2e-5, si
        if not last:
            assert float((tok.cpu() - nxt.reshape(1, 32, -1).transpose(1, 2)).abs().max()) <= 2e-5, si
        else:
            assert tok is None
        # explicit pn_next = this scale
        f_hat2 = f0.to(dev).view(1, 1, 32, 32, 32).clone()
        tok2 = vae._next_input(si, None, f_hat2, 1, 1, True, soft=soft.to(dev), pn_next=pn)
        assert torch.equal(f_hat2, f_hat)
        assert float((tok2.cpu() - q.area(f_ref, pn).reshape(1, 32, -1).transpose(1, 2)).abs().max()) <= 2e-5, si
        # six maps between NaN fences, straight through the C entry point
        nb, nmaps, pnn = 3, 2, (pns[si + 1] if not last else pn)
        fbuf = torch.full((nb * nmaps + 2, MAP), float('nan'), device=dev)
        fbuf[1:-1] = f0.to(dev).reshape(1, MAP)
        tbuf = torch.full((nb * nmaps + 2, pnn * pnn * 32), float('nan'), device=dev)
        codebook = soft[0].to(dev).contiguous()                                          # (pn*pn, 32)
        idx = torch.arange(pn * pn, dtype=torch.int32, device=dev).repeat(nb * nmaps).contiguous()
        ops.ms_next_input(idx, codebook, P['phi_w'], P['phi_b'], P['up'], P['down'], fbuf[1:-1], tbuf[1:-1], nb, nmaps, pn, pnn, 32, 32,
                          P['phi_map'][si], P['tab_off'][si], P['tab_off'][list(pns).index(pnn)])
        assert torch.isnan(fbuf[0]).all() and torch.isnan(fbuf[-1]).all() and torch.isnan(tbuf[0]).all() and torch.isnan(tbuf[-1]).all()
        want_tok = tok if not last else tok2
        for m in range(nb * nmaps):
            assert torch.equal(fbuf[1 + m], f_hat.reshape(MAP)), (si, m)
            assert torch.equal(tbuf[1 + m], want_tok.reshape(-1)), (si, m)


# ------------------------------------------------------------------------------ 5. public API
def test_public_tokenizer_api_fp32_512(gpu_device):
    """img_to_idxBl / idxBl_to_h / idxBl_to_img on (2, 3, 512, 512) in parity mode against the reference's recording for image 0, the caller-chosen list
    against its own recording, and a list that ends at 16 raises as upstream (quant.py:193)"""
    g, gb = golden('res512_a'), golden('res512_b')
    vae = make_vae(32, F32, gpu_device)
    img = torch.cat((synth_images(1, 512, seed=1), synth_images(1, 512, seed=2))).to(gpu_device)
    ids = vae.img_to_idxBl(img)
    assert [tuple(i.shape) for i in ids] == [(2, p * p) for p in PN]
    zero = np.zeros((1, 2240), np.float32)
    ids_parity(torch.cat(ids, 1)[:1].cpu(), g['ids'], zero, 0.0, 'img_to_idxBl 512 ch32', strict=True)
    gi = [x.to(gpu_device) for x in split(g['ids'].astype(np.int64), PN)]
    var_in = torch.cat(vae.idxBl_to_h(gi), dim=1)
    assert var_in.shape == (1, 2239, 32)
    assert float((var_in.cpu() - t(g['var_in'])).abs().max()) <= 2e-5
    rec = vae.idxBl_to_img(gi, same_shape=True, last_one=True).cpu()
    assert rec.shape == (1, 3, 512, 512)
    assert float((rec[CROP] - t(g['rec_crop'])).abs().max()) <= 2e-3
    assert float((rec.mean(dim=(2, 3)) - t(g['rec_mean'])).abs().max()) <= 3e-4
    rec2 = vae.img_to_recon(img, last_one=True)[:1].cpu()                  # the same decode WITHOUT the clamp (vqvae.py:80-86 against :93)
    assert float(rec2.abs().max()) > 1.0
    assert float((rec2.clamp(-1, 1)[CROP] - t(g['rec_crop'])).abs().max()) <= 2e-3
    assert float((rec2.clamp(-1, 1) - rec).abs().max()) <= 2e-3
    alt = vae.img_to_idxBl(img, v_patch_nums=ALT)
    assert [tuple(i.shape) for i in alt] == [(2, p * p) for p in ALT]
    ids_parity(torch.cat(alt, 1)[:1].cpu(), gb['ids'], np.zeros((1, 1704), np.float32), 0.0, f'img_to_idxBl 512 v_patch_nums={ALT}', strict=True)
    with pytest.raises(AssertionError):
        vae.img_to_idxBl(img, v_patch_nums=DEFAULT_PATCH_NUMS)


# ------------------------------------------------------------------------------ 6. the wide decoder
def test_decoder_ch160_bf16_512_against_emulated_oracle(gpu_device):
    """ch = 160 decoder on one 32 x 32 f_hat, bf16: the only test that runs the wide halo convs, the GroupNorm tile partials at 4x the tiles per image
    and the 1 024-column softmax.  Bounds of test_decoder_bf16_against_emulated_oracle (tests/test_gpu_parity.py): as accurate as the faithful bf16
    model of itself (mean |err| within 1.3x, both against fp32), mean < 2e-2 and p99 < 0.1 on [-1, 1] pixels.  The two CPU oracle passes
    (fp32 and bf16-emulated, ~1.6 TFLOP each) take about 10 s together."""
    g = golden('res512_a')
    vae = make_vae(160, BF16, gpu_device)
    sd = synth_vae_state(VaeConfig(ch=160, patch_nums=PN))
    f_hat = t(g['fhat_last'])
    with torch.no_grad():
        emul = vqvae_ref.fhat_to_img(sd, f_hat, Prec(True))
        ref32 = vqvae_ref.fhat_to_img(sd, f_hat)
    got = vae.fhat_to_img(f_hat.to(gpu_device)).cpu()
    assert got.shape == (1, 3, 512, 512)
    e_gpu = (got - ref32).abs().flatten()
    e_emu = (emul - ref32).abs().flatten()
    print(f'[res512] ch160 bf16 decode: mean err gpu {e_gpu.mean():.3e} emulated {e_emu.mean():.3e}')
    assert e_gpu.mean() < 2e-2 and e_gpu.quantile(0.99) < 0.1
    assert e_gpu.mean() < 1.3 * e_emu.mean() + 1e-4, (e_gpu.mean().item(), e_emu.mean().item())
    assert (got - emul).abs().mean() < 2e-2


# ------------------------------------------------------------------------------ 7. generation
GEN_CFG = VarConfig(depth=2, embed_dim=128, num_heads=2, patch_nums=PN)
GEN_SEED = 12              # weight seed with the widest smallest greedy margin among seeds 0..23 (see the greedy test)


def make_cvar(vae, dtype, dev, seed=GEN_SEED):
    m = models.ControlVAR(vae, depth=2, embed_dim=128, num_heads=2, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                          init_seed=seed, cond_drop_rate=0.0)
    return m.to(dev).eval()


def oracle_generation():
    trace = {}
    with torch.no_grad():
        f = var_ref.generate(synth_var_state(GEN_CFG, GEN_SEED), GEN_CFG, oracle_q(), 2, torch.tensor([3, 7]), 1.5, top_k=1, cond_type=torch.tensor([0, 1]),
                             trace=trace)
        img = var_ref.decode_fhat(synth_vae_state(VaeConfig(ch=32, patch_nums=PN)), f)
    lg = torch.cat(trace['logits'], dim=1)
    top2 = lg.topk(2, dim=-1).values
    return torch.cat(trace['idx'], dim=1), (top2[..., 0] - top2[..., 1]), img


def test_generation_fp32_greedy_512_against_oracle(gpu_device):
    """ControlVAR depth 2, width 128, B = 2, cfg 1.5, greedy, parity mode: the 2 x 4 480 ids of oracle.var_ref.generate (strict) and its
    (2, 3, 1024, 512) image (<= 2e-3).  Greedy margins, computed on the CPU beforehand: the 256 x 256 greedy test labels its flips with a 2e-3
    logit margin; with 8 960 argmaxes over 4 096 logits about ten tokens fall below 2e-3 for EVERY weight seed (seeds 0..23 scanned: 7 to 18 tokens,
    smallest margins 1e-5 .. 8.3e-4), so no seed clears that figure.  Seed 12 has the widest smallest margin, 8.28e-4 - some 80x the ~1e-5 fp32
    summation-order noise of these logits - and the comparison stays strict: any flip fails."""
    ids_ref, margin, img_ref = cached('gen', oracle_generation)
    assert float(margin.min()) > 8e-4, float(margin.min())
    vae = make_vae(32, F32, gpu_device)
    m = make_cvar(vae, F32, gpu_device)
    img = m.autoregressive_infer_cfg(2, torch.tensor([3, 7]), g_seed=0, cfg=1.5, top_k=1, top_p=0.0, cond_type=torch.tensor([0, 1]), _trace=True).cpu()
    assert img.shape == (2, 3, 1024, 512)
    ids = torch.cat(m.last_trace['idx'], dim=1).cpu()
    n, ok = ids_parity(ids, ids_ref.numpy(), margin.numpy(), 2e-3, 'generation 512 d2 greedy', strict=True)
    assert maxabs_on(img - img_ref, ok) <= 2e-3


def test_generation_bf16_and_plain_var_512(gpu_device):
    """the same model in bf16 (runs, (2, 3, 1024, 512), finite, in [0, 1]); a plain VAR with the same list, (2, 3, 512, 512); the captured graph of a
    512 generation replays to the eager result"""
    vae = make_vae(32, BF16, gpu_device)
    m = make_cvar(vae, BF16, gpu_device)
    kw = dict(cfg=1.5, top_k=900, top_p=0.96)
    labels, types = torch.tensor([3, 7]), torch.tensor([0, 1])
    img = m.autoregressive_infer_cfg(2, labels, g_seed=3, cond_type=types, **kw)
    assert img.shape == (2, 3, 1024, 512) and torch.isfinite(img).all() and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    run = m.graphed_generator(2, **kw)
    assert torch.equal(run(labels, types, g_seed=3), img)
    v = models.VAR(vae, depth=2, embed_dim=128, num_heads=2, patch_nums=PN, compute_dtype=BF16, cond_drop_rate=0.0).to(gpu_device).eval()
    out = v.autoregressive_infer_cfg(2, labels, g_seed=3, **kw)
    assert out.shape == (2, 3, 512, 512) and torch.isfinite(out).all()


# ------------------------------------------------------------------------------ 8. a training step
def test_trainer_step_bf16_512(gpu_device):
    """Trainer.step at 512 x 512 (B = 2, depth 2, bf16, the tokenizer inside): the loss is finite and equals the fp32 oracle's on the same tokens within
    2e-2, the bound of test_training_step_bf16_close_to_fp32_oracle"""
    vae = make_vae(32, BF16, gpu_device)
    m = make_cvar(vae, BF16, gpu_device)
    tr = T.Trainer(m, vae, peak_lr=2e-3, weight_decay=0.05, weight_decay_end=0.01, sche='lin0', warmup_it=20, max_it=1000, clip=2.0, wp0=0.005, wpe=0.01,
                   drop_path=False)
    images, masks = synth_images(2, 512, seed=6).to(gpu_device), synth_images(2, 512, seed=7).to(gpu_device)
    cls, types = torch.tensor([17, 403]), torch.tensor([2, 0])
    x, labels = tr.tokenize(images, masks, True)
    assert x.shape == (2, 4478, 32) and labels.shape == (2, 4480)
    loss_r, _, _ = train_ref.loss_and_grads(synth_var_state(GEN_CFG, GEN_SEED), GEN_CFG, cls, x.float().cpu(), types, labels.cpu())
    out = tr.step(images, masks, cls, types, mask_first=True)
    assert torch.isfinite(out['loss']).all() and torch.isfinite(out['grad_norm']).all()
    assert abs(out['loss'].item() - loss_r.item()) < 2e-2, (out['loss'].item(), loss_r.item())


# ------------------------------------------------------------------------------ 9. S = 16 untouched
def msq16_outputs(dev):
    """what tests/golden/msq16_regression.npz holds (tests/golden/make_msq16_regression.py ran this on the library of the commit before the S = 32
    kernels): the S = 16 quantizer on two seeded feature batches - ids and f_hat of both search paths' shared result, and the f_hat / tokens of the
    per-scale next-input kernel fed with those ids"""
    vae = models.build_vae(ch=32, compute_dtype=F32).to(dev)
    out = {}
    for k, (seed, amp) in enumerate(((11, 0.7), (12, 1.5))):
        f = (torch.randn(2, 32, 16, 16, generator=torch.Generator().manual_seed(seed)) * amp).to(dev)
        idx, fh, _ = vae._ms_encode(f, want_fhat=True)
        idx_m, fh_m, mg = vae._ms_encode(f, want_fhat=True, want_margin=True)
        assert torch.equal(idx, idx_m) and torch.equal(fh, fh_m)
        ms = [i.long() for i in vae._split(idx)]
        out[f'ids_{k}'] = idx.cpu().numpy().astype(np.int16)
        out[f'fhat_{k}'] = fh.cpu().numpy()
        out[f'margin_{k}'] = mg.cpu().numpy()
        out[f'ni_fhat_{k}'] = vae._idx_to_fhat(ms).cpu().numpy()
        out[f'ni_tok_{k}'] = torch.cat(vae.idxBl_to_h(ms), dim=1).cpu().numpy()
    return out


def test_s16_kernels_bit_identical_to_the_previous_library(gpu_device):
    import os
    from conftest import GOLDEN
    assert os.path.exists(os.path.join(GOLDEN, 'msq16_regression.npz')), 'record it with tests/golden/make_msq16_regression.py on the previous library'
    g = golden('msq16_regression')
    got = msq16_outputs(gpu_device)
    assert set(got) == set(g)
    for k, v in got.items():
        assert np.array_equal(v, g[k]), k
