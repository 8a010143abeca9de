"""ControlVAR.graphed_conditional_generator on the MI355X: the captured conditional generation (control in, image out; image in, control
out) against the eager path of the same library - `vae.img_to_idxBl` + `conditional_infer_cfg`, which the gen_*_cmask / gen_*_cimg
fixtures pin to the reference.  Every comparison is bit for bit: the graph replays the launches the eager call makes, on static buffers.
Smallest models at which the capture can go wrong (those of test_hip_graph_replay_equals_eager), B = 3."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import models  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VarConfig  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
B, H = 3, 256
LTOT = sum(p * p for p in PN)
SAMPLING = dict(cfg=(3.0, 2.0, 1.0), top_k=900, top_p=0.96)
# (labels, condition types, seed of the synthetic given half, sampling seed)
SETS = ((torch.tensor([1, 2, 3]), torch.tensor([0, 1, 2]), 31, 11), (torch.tensor([7, 500, 999]), torch.tensor([3, 3, 0]), 32, 12345))
TEACH = {'control': 'c_mask', 'image': 'c_img'}


def make(dtype, dev, **flags):
    cfg = VarConfig(depth=3, embed_dim=256, num_heads=4, **flags)
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    m = models.ControlVAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                          type_pos=cfg.type_pos, bidirectional=cfg.bidirectional, cond_drop_rate=0.0).to(dev).eval()
    return vae, m


@pytest.fixture(scope='module')
def bf16_models(gpu_device):
    return make(BF16, gpu_device)


def given_half(vae, seed, dev):
    """synthetic pixels of the given half and their (valid) ids, as a user of the eager path gets them"""
    pix = synth_images(B, H, seed=seed).to(dev)
    return pix, vae.img_to_idxBl(pix)


def eager(m, given, labels, types, ids, seed, **sampling):
    return m.conditional_infer_cfg(B, labels, g_seed=seed, cond_type=types, **(sampling or SAMPLING), **{TEACH[given]: ids})


def check_ids_source(vae, m, given, dev):
    run = m.graphed_conditional_generator(B, given=given, source='ids', **SAMPLING)
    for k, (labels, types, pseed, seed) in enumerate(SETS):
        _, ids = given_half(vae, pseed, dev)
        # the reference's form (list of int64 tensors, here on the CPU), then one int32 device tensor
        src = [i.cpu() for i in ids] if k == 0 else torch.cat(ids, dim=1).to(torch.int32)
        a = run(labels, types, src, g_seed=seed)
        assert a.shape == (B, 3, 2 * H, H)
        assert torch.equal(a, eager(m, given, labels, types, ids, seed)), (given, k)
        assert torch.equal(run.ids().cpu(), torch.cat(ids, dim=1).to(torch.int32).cpu())
    c = run(labels, types, src, g_seed=seed + 1)
    assert not torch.equal(a, c)
    # a wrong shape or an id outside the codebook is refused on the host, and the buffers of the graph are untouched by the refused call
    for bad in (dict(label_B=labels[:2]), dict(cond_type=torch.zeros(B + 1, dtype=torch.long)), dict(source=src[:, :-1]), dict(source=[i.cpu() for i in ids][:-1]),
                dict(source=src.float())):
        args = dict(label_B=labels, cond_type=types, source=src)
        args.update(bad)
        with pytest.raises(ValueError, match='expected'):
            run(args['label_B'], args['cond_type'], args['source'], g_seed=seed)
    over = src.clone()
    over[1, 5] = 4096
    with pytest.raises(IndexError, match='index out of range'):
        run(labels, types, over, g_seed=seed)
    assert torch.equal(run(labels, types, src, g_seed=seed), a)


@pytest.mark.parametrize('given', ['control', 'image'])
def test_ids_in_replay_equals_eager(gpu_device, bf16_models, given):
    """cases 1 and 2: two (labels, types, ids, seed) sets through one graph equal conditional_infer_cfg(c_mask= / c_img=); another seed differs"""
    check_ids_source(*bf16_models, given, gpu_device)


def test_ids_in_replay_equals_eager_fp32(gpu_device):
    """case 8: the fp32 parity mode (exact-f32 kernels, fp32 tokeniser)"""
    check_ids_source(*make(F32, gpu_device), 'control', gpu_device)


@pytest.mark.parametrize('given', ['control', 'image'])
def test_greedy_replay_equals_eager(gpu_device, bf16_models, given):
    vae, m = bf16_models
    run = m.graphed_conditional_generator(B, given=given, cfg=(3.0, 2.0, 1.0), top_k=1, source='ids')
    labels, types, pseed, seed = SETS[0]
    _, ids = given_half(vae, pseed, gpu_device)
    a = run(labels, types, ids, g_seed=seed)
    assert torch.equal(a, eager(m, given, labels, types, ids, seed, cfg=(3.0, 2.0, 1.0), top_k=1))
    assert torch.equal(a, run(labels, types, ids, g_seed=seed + 1))          # greedy: the seed does not matter


@pytest.mark.parametrize('given', ['control', 'image'])
def test_pixels_in_replay_equals_eager_tokeniser_and_generation(gpu_device, bf16_models, given):
    """case 4: the graph's own tokeniser + generation + decode against img_to_idxBl followed by conditional_infer_cfg; the ids it produced
    are readable after the replay; other pixels through the same graph follow the new pixels"""
    vae, m = bf16_models
    run = m.graphed_conditional_generator(B, given=given, source='pixels', **SAMPLING)
    outs = []
    for labels, types, pseed, seed in SETS:
        pix, ids = given_half(vae, pseed, gpu_device)
        a = run(labels, types, pix if pseed == 31 else pix.cpu(), g_seed=seed)
        got = run.ids()
        assert got.dtype == torch.int32 and got.shape == (B, LTOT)
        assert torch.equal(got.long(), torch.cat(ids, dim=1))
        assert torch.equal(a, eager(m, given, labels, types, ids, seed))
        outs.append((a, got))
    assert not torch.equal(outs[0][1], outs[1][1])
    # same labels / types / seed as the last replay, the first set's pixels: the given half of the output follows the pixels
    pix0, ids0 = given_half(vae, SETS[0][2], gpu_device)
    labels, types, _, seed = SETS[1]
    c = run(labels, types, pix0, g_seed=seed)
    assert torch.equal(run.ids(), outs[0][1]) and torch.equal(c, eager(m, given, labels, types, ids0, seed))
    rows = slice(0, H) if given == 'control' else slice(H, 2 * H)
    assert torch.equal(c[:, :, rows], outs[0][0][:, :, rows]) and not torch.equal(c[:, :, rows], outs[1][0][:, :, rows])
    with pytest.raises(ValueError, match='expected pixels of shape'):
        run(labels, types, pix0[:, :, :128], g_seed=seed)
    with pytest.raises(ValueError, match='expected pixels of shape'):
        run(labels, types, ids0, g_seed=seed)


@pytest.mark.parametrize('given', ['control', 'image'])
def test_decode_generated_is_the_generated_half_of_decode_both(gpu_device, bf16_models, given):
    """case 5: one decoder pass of B maps instead of 2 B; an image's decoded bits do not depend on the batch it rides in"""
    vae, m = bf16_models
    both = m.graphed_conditional_generator(B, given=given, source='ids', decode='both', **SAMPLING)
    gen = m.graphed_conditional_generator(B, given=given, source='ids', decode='generated', **SAMPLING)
    rows = slice(H, 2 * H) if given == 'control' else slice(0, H)            # control on top, RGB below
    for labels, types, pseed, seed in SETS:
        _, ids = given_half(vae, pseed, gpu_device)
        a, g = both(labels, types, ids, g_seed=seed), gen(labels, types, ids, g_seed=seed)
        assert g.shape == (B, 3, H, H)
        assert torch.equal(g, a[:, :, rows])


def test_joint_and_conditional_graphs_coexist(gpu_device, bf16_models):
    """case 6: a joint graphed_generator and a conditional graph of one model alive together, replayed alternately, with an eager
    conditional call in between: each owns its K/V arena and split-K workspace"""
    vae, m = bf16_models
    joint = m.graphed_generator(B, cfg=3.0, top_k=900, top_p=0.96)
    cond = m.graphed_conditional_generator(B, given='control', source='ids', **SAMPLING)
    _, ids = given_half(vae, 33, gpu_device)
    for k in range(2):
        labels, types, _, seed = SETS[k]
        want_joint = m.autoregressive_infer_cfg(B, labels, g_seed=seed, cfg=3.0, top_k=900, top_p=0.96, cond_type=types)
        want_cond = eager(m, 'control', labels, types, ids, seed)
        a = joint(labels, types, g_seed=seed)
        b = cond(labels, types, ids, g_seed=seed)
        between = eager(m, 'control', labels, types, ids, seed)
        a2 = joint(labels, types, g_seed=seed)
        assert torch.equal(a, want_joint) and torch.equal(a2, want_joint), k
        assert torch.equal(b, want_cond) and torch.equal(between, want_cond), k
    assert torch.equal(cond(labels, types, ids, g_seed=seed), want_cond)


def test_bidirectional_model_is_captured(gpu_device):
    """case 7: the four-branch path never draws the order, so a bidirectional model (which graphed_generator refuses) captures as it is"""
    vae, m = make(BF16, gpu_device, bidirectional=True, type_pos=True)
    assert m.bidirectional
    with pytest.raises(NotImplementedError):
        m.graphed_generator(B)
    labels, types, pseed, seed = SETS[1]
    _, ids = given_half(vae, pseed, gpu_device)
    for given in ('control', 'image'):
        run = m.graphed_conditional_generator(B, given=given, source='ids', **SAMPLING)
        assert torch.equal(run(labels, types, ids, g_seed=seed), eager(m, given, labels, types, ids, seed)), given
