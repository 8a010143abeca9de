"""Region-constrained generation on the MI355X: the forced-token table against a host restatement of the cell rule, the forcing sampler against
`ops.cfg_sample_rows` (pinned to the scalar kernel by tests/test_gpu_request_params.py), and edit_infer_cfg / graphed_edit_generator against the
per-request joint path, the sources and the CPU oracle.  Every comparison of ids, logits and images is bit for bit: there is no tolerance here."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ids_parity  # noqa: E402
from controlvar_amd import models, ops  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, PATCH_NUMS_512 as PN512, VaeConfig, VarConfig, phi_index_map  # noqa: E402
from controlvar_amd.synth import synth_images, synth_vae_state, synth_var_state  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
V = 4096


# ------------------------------------------------------------------------------------------------------------- the cell rule, restated
def keep_cells(keep, pn):
    """(B, S, S) bool -> (B, pn * pn) bool: cell (i, j) covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns,
    kept iff twice the kept latent cells of the bin exceed its size (python integers; tests/test_edit_host.py checks this against area pooling)"""
    B, S = keep.shape[0], keep.shape[-1]
    out = torch.zeros(B, pn * pn, dtype=torch.bool)
    for b in range(B):
        m = keep[b].tolist()
        for i in range(pn):
            r0, r1 = i * S // pn, -((-(i + 1) * S) // pn)
            for j in range(pn):
                c0, c1 = j * S // pn, -((-(j + 1) * S) // pn)
                n = sum(1 for r in range(r0, r1) for c in range(c0, c1) if m[r][c])
                out[b, i * pn + j] = 2 * n > (r1 - r0) * (c1 - c0)
    return out


def host_table(pns, B, keep_ctrl, keep_img, src_ctrl, src_img, mask_first, mf):
    """forced (B, L) int64: per scale the halves in mask_first order, the source id where kept, -1 where free; src_* are lists of (B, pn^2)"""
    cols = []
    for si, pn in enumerate(pns):
        halves = {}
        for name, keep, src in (('ctrl', keep_ctrl, src_ctrl), ('img', keep_img, src_img)):
            free = torch.full((B, pn * pn), -1, dtype=torch.int64)
            halves[name] = free if keep is None else torch.where(keep_cells(keep.cpu(), pn), src[si].cpu().long(), free)
        cols += [halves['img']] if mf == 1 else ([halves['ctrl'], halves['img']] if mask_first else [halves['img'], halves['ctrl']])
    return torch.cat(cols, dim=1)


def some_masks(S, seed):
    """three differing masks: random at density 0.5, a centred square, a 1-cell checkerboard with one row kept on top of it"""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.rand(S, S, generator=g) < 0.5
    square = torch.zeros(S, S, dtype=torch.bool); square[S // 4:S - S // 4, S // 4:S - S // 4] = True
    ii = torch.arange(S)
    checker = (ii[:, None] + ii[None, :]) % 2 == 0
    checker[3] = True
    return torch.stack([rnd, square, checker])


def random_sources(pns, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V, (B, pn * pn), generator=g) for pn in pns]


# ------------------------------------------------------------------------------------------------------------- 1. the force table
@pytest.mark.parametrize('mf', [1, 2])
@pytest.mark.parametrize('mask_first', [True, False])
@pytest.mark.parametrize('pns', [PN, PN512], ids=['S16', 'S32'])
def test_force_table_equals_the_host_rule_bit_for_bit(gpu_device, pns, mask_first, mf):
    dev, B, S = gpu_device, 3, pns[-1]
    Lsrc = sum(pn * pn for pn in pns)
    L = mf * Lsrc
    keep = {'ctrl': some_masks(S, 1), 'img': some_masks(S, 2).flip(0)}
    keep['img'][1] = True                                       # one request keeps its whole image, pn = 1 token included
    src = {'ctrl': random_sources(pns, B, 3), 'img': random_sources(pns, B, 4)}
    flat = {h: torch.cat(src[h], dim=1).to(device=dev, dtype=torch.int32).contiguous() for h in src}
    FENCE, SENT = 64, -7
    for null in ((), ('ctrl',), ('img',), ('ctrl', 'img')):
        if mf == 1 and 'ctrl' not in null:
            continue                                            # a plain model has no control half
        k = {h: None if h in null else keep[h] for h in keep}
        buf = torch.full((B * L + 2 * FENCE,), SENT, dtype=torch.int32, device=dev)
        forced = buf[FENCE:FENCE + B * L].view(B, L)
        ops.edit_force_table(None if k['ctrl'] is None else k['ctrl'].to(dev).to(torch.uint8), None if k['img'] is None else k['img'].to(dev).to(torch.uint8),
                             None if k['ctrl'] is None else flat['ctrl'], None if k['img'] is None else flat['img'], pns, B, mask_first, mf, forced)
        want = host_table(pns, B, k['ctrl'], k['img'], src['ctrl'], src['img'], mask_first, mf)
        assert torch.equal(forced.cpu().long(), want), (null, int((forced.cpu().long() != want).sum()))
        assert bool((buf[:FENCE] == SENT).all()) and bool((buf[FENCE + B * L:] == SENT).all())
        if null != ('ctrl', 'img'):
            assert int((want >= 0).sum()) > 0 and int((want < 0).sum()) > 0


# ------------------------------------------------------------------------------------------------------------- 2. / 3. the sampler
TOP_K, TOP_P, SEEDS = [1, 900, 0], [0.0, 0.96, 0.0], [11, 2 ** 63 - 3, 5]          # greedy, top-k 900 / top-p 0.96, unfiltered


def tables(B, stage, dev):
    ratio = stage / 9
    coef = np.zeros((B, 4), dtype=np.float32)
    for b, g in enumerate([1.5, 4.0, 3.0][:B]):
        coef[b, :2] = [1 + g * ratio, -g * ratio]
    return (torch.from_numpy(coef).to(dev), torch.tensor(TOP_K[:B], dtype=torch.int32, device=dev), torch.tensor(TOP_P[:B], device=dev),
            torch.tensor(SEEDS[:B], dtype=torch.int64, device=dev))


def make_logits(B, l, ldv, Vc, seed, dev):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(2 * B, l, ldv, generator=g) * 3.0
    if ldv > Vc:
        lg[:, :, Vc:] = 100.0                                   # columns behind the codes: larger than every logit, never read
    return lg.to(dev)


def outputs(B, l, Vc, n_draw, dev):
    return (torch.full((n_draw * B, l), -1, dtype=torch.int32, device=dev), torch.full((B, l, Vc), float('nan'), device=dev),
            torch.full((B, l), float('nan'), device=dev), torch.full((B, l), -1, dtype=torch.int32, device=dev))


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize('Vc,ldv', [(V, V), (1000, 1024)])
@pytest.mark.parametrize('l', [2, 8, 512])
def test_nothing_forced_is_the_per_request_kernel_bit_for_bit(gpu_device, l, Vc, ldv):
    dev, B, stage = gpu_device, 3, 6
    lg = make_logits(B, l, ldv, Vc, 10 * l + Vc, dev)
    coef, k, p, s = tables(B, stage, dev)
    ref = outputs(B, l, Vc, 1, dev)
    ops.cfg_sample_rows(lg, B, 2, l, Vc, coef, k, p, s, stage, 1, *ref, ldv=ldv)
    got = outputs(B, l, Vc, 1, dev)
    forced = torch.full((B, l), -1, dtype=torch.int32, device=dev)
    ops.cfg_sample_edit(lg, B, 2, l, Vc, coef, k, p, s, stage, 1, got[0], forced, *got[1:], ldv=ldv)
    assert int(got[0].min()) >= 0 and int(got[0].max()) < Vc
    for name, x, y in zip(('idx', 'combined', 'margin', 'kept'), got, ref):
        assert same_bits(x, y), name
    assert bool((got[3][0] == 1).all()) and 1 < int(got[3][1].max()) <= 900          # the greedy row, the top-k 900 row


@pytest.mark.parametrize('Vc,ldv', [(V, V), (1000, 1024)])
@pytest.mark.parametrize('l', [2, 8, 512])
def test_mixed_forcing_leaves_the_free_tokens_alone_and_reads_no_logit_of_a_forced_one(gpu_device, l, Vc, ldv):
    dev, B, stage, n_draw = gpu_device, 3, 4, 2
    lg = make_logits(B, l, ldv, Vc, 20 * l + Vc, dev)
    coef, k, p, s = tables(B, stage, dev)
    ref = outputs(B, l, Vc, n_draw, dev)
    ops.cfg_sample_rows(lg, B, 2, l, Vc, coef, k, p, s, stage, n_draw, *ref, ldv=ldv)
    g = torch.Generator().manual_seed(l)
    ids = torch.randint(0, Vc, (B, l), generator=g)
    hit = torch.rand(B, l, generator=g) < 0.5
    hit[:, 0], hit[:, -1] = torch.tensor([True, False, True]), torch.tensor([False, True, True])
    wide = torch.full((B, l + 5), 12345, dtype=torch.int32)                  # this stage's columns inside a wider table: ldf = l + 5
    wide[:, 3:3 + l] = torch.where(hit, ids, torch.full_like(ids, -1)).int()
    forced = wide.to(dev)[:, 3:3 + l]

    def run(logits):
        out = outputs(B, l, Vc, n_draw, dev)
        ops.cfg_sample_edit(logits, B, 2, l, Vc, coef, k, p, s, stage, n_draw, out[0], forced, *out[1:], ldv=ldv)
        return out
    got = run(lg)
    h = hit.to(dev)
    idx, comb, mg, kept = got
    for d in range(n_draw):
        assert torch.equal(idx.view(n_draw, B, l)[d][h], ids.to(dev).int()[h])                      # the forced id in every draw row
        assert torch.equal(idx.view(n_draw, B, l)[d][~h], ref[0].view(n_draw, B, l)[d][~h])         # free tokens: the per-request kernel's
    assert same_bits(comb[~h], ref[1][~h]) and same_bits(mg[~h], ref[2][~h]) and torch.equal(kept[~h], ref[3][~h])
    assert bool((kept[h] == 0).all()) and bool((mg[h] == float('inf')).all())
    assert bool(torch.isnan(comb[h]).all())                                                         # the prefill: no combined row is written
    poisoned = lg.clone()
    poisoned.view(2, B, l, ldv)[:, h] = float('nan')                                                # both branches of every forced token
    for name, x, y in zip(('idx', 'combined', 'margin', 'kept'), run(poisoned), got):
        assert same_bits(x, y), name


# ------------------------------------------------------------------------------------------------------------- 4. - 11. end to end
def make(dtype, dev, plain=False):
    """the depth-2 transformer and ch = 32 VQVAE of __graft_entry__.smoke (weights: synth_var_state / synth_vae_state, which the oracle reads)"""
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    if plain:
        return vae, models.build_var(vae, depth=2, compute_dtype=dtype).to(dev).eval()
    return vae, models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype).to(dev).eval()


@pytest.fixture(scope='module')
def f32_models(gpu_device):
    return make(F32, gpu_device)


@pytest.fixture(scope='module')
def bf16_models(gpu_device):
    return make(BF16, gpu_device)


@pytest.fixture(scope='module')
def plain_models(gpu_device):
    return make(F32, gpu_device, plain=True)


@pytest.fixture(scope='module')
def src(gpu_device, f32_models):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = f32_models[0]
    return (vae.img_to_idxBl(synth_images(3, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(3, 256, seed=42).to(gpu_device)))


def hole(B, S=16, lo=4, hi=12):
    """keep everything outside the centred 8 x 8 square"""
    keep = torch.ones(B, S, S, dtype=torch.bool)
    keep[:, lo:hi, lo:hi] = False
    return keep


LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])


def trace_ids(m):
    return [x.clone() for x in m.last_trace['idx']]


def check_partial(m, B, produced, forced, rerun, keep_by_half, src_by_half, mf):
    """kept cells carry the source ids by the host rule; every free token is what the sampler drew at that token when the produced ids are
    teacher-forced through the per-request path (whose trace holds the draw before forcing)"""
    want = host_table(PN, B, keep_by_half.get('ctrl'), keep_by_half['img'], src_by_half.get('ctrl'), src_by_half['img'], True, mf)
    assert torch.equal(forced.cpu().long(), want)
    got = torch.cat(produced, dim=1).cpu().long()
    kept = want >= 0
    assert torch.equal(got[kept], want[kept])
    assert int(kept.sum()) > 0 and int((~kept).sum()) > 0
    rerun(produced)
    drawn = torch.cat(trace_ids(m), dim=1).cpu().long()
    assert torch.equal(drawn[~kept], got[~kept]), int((drawn[~kept] != got[~kept]).sum())
    return kept


def test_nothing_kept_equals_the_per_request_joint_call(gpu_device, bf16_models, src):
    vae, m = bf16_models
    B = 3
    want = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    ref = trace_ids(m)
    nothing = torch.zeros(B, 16, 16, dtype=torch.bool)
    for kw in (dict(), dict(src_img=src[1], src_ctrl=src[0]), dict(src_img=src[1], keep_img=nothing, src_ctrl=src[0], keep_ctrl=nothing.to(gpu_device))):
        got = m.edit_infer_cfg(B, LABELS, TYPES, trace=True, **kw, **ROWS)
        for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
            assert torch.equal(x, y), si
        assert torch.equal(got, want)
        assert bool((m.last_trace['forced'] == -1).all())


def test_everything_kept_reproduces_the_sources(gpu_device, f32_models, src):
    vae, m = f32_models
    B = 3
    img = m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=True, src_ctrl=src[0], keep_ctrl=torch.ones(B, 16, 16, dtype=torch.bool), trace=True, **ROWS)
    for si, x in enumerate(trace_ids(m)):
        assert torch.equal(x.long(), torch.cat((src[0][si], src[1][si]), dim=1)), si
    H = img.shape[-1]
    for half, ids in enumerate(src):                            # control on top, RGB below
        want = vae.idxBl_to_img(ids, same_shape=True, last_one=True) * 0.5 + 0.5
        assert torch.equal(img[:, :, half * H:(half + 1) * H], want), half


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
def test_a_partial_edit_keeps_the_kept_cells_and_samples_the_free_ones(gpu_device, bf16_models, f32_models, src, dtype):
    vae, m = bf16_models if dtype == BF16 else f32_models
    B = 3
    keep = hole(B)
    m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=keep, src_ctrl=src[0], keep_ctrl=True, trace=True, **ROWS)
    produced, forced = trace_ids(m), m.last_trace['forced'].clone()

    def rerun(ids):
        m._generate_rows(B, LABELS, ROWS['g_seed'], ROWS['cfg'], ROWS['top_k'], ROWS['top_p'], False, TYPES, False, None, None, force_idx=ids, trace=True)
    kept = check_partial(m, B, produced, forced, rerun, dict(ctrl=torch.ones(B, 16, 16, dtype=torch.bool), img=keep), dict(ctrl=src[0], img=src[1]), 2)
    assert int((~kept).sum()) == B * sum(int((~keep_cells(keep[:1], pn)).sum()) for pn in PN)         # free: the image's hole only


def test_free_tokens_are_the_cpu_oracles_greedy_tokens(gpu_device, f32_models, src):
    from oracle import var_ref
    from oracle.vqvae_ref import MSQuant
    vae, m = f32_models
    B = 2
    labels, types = LABELS[:B], TYPES[:B]
    keep = hole(B)
    m.edit_infer_cfg(B, labels, types, src_img=[t[:B] for t in src[1]], keep_img=keep, src_ctrl=[t[:B] for t in src[0]], keep_ctrl=True, trace=True,
                     g_seed=0, cfg=4.0, top_k=1)
    produced = [x.cpu().long() for x in trace_ids(m)]
    free = (m.last_trace['forced'] < 0).cpu().numpy()
    cfg = VarConfig(depth=2)
    sdv, sd = synth_vae_state(VaeConfig(ch=32)), synth_var_state(cfg)
    trace = {}
    with torch.no_grad():
        var_ref.generate(sd, cfg, MSQuant(sdv, PN, phi_index_map(10)), B, labels, 4.0, top_k=1, cond_type=types, force_idx=produced, trace=trace)
    got, ref = torch.cat(produced, dim=1).numpy(), torch.cat(trace['idx'], dim=1).numpy()
    assert free.sum() == B * sum(int((~keep_cells(keep[:1], pn)).sum()) for pn in PN)
    ids_parity(got[free], ref[free], np.zeros(int(free.sum())), 0.0, 'edit: free tokens against the oracle (fp32, greedy)', strict=True)


def test_a_request_does_not_depend_on_its_batch(gpu_device, bf16_models, src):
    """under deterministic_plan=True row b of a batch of three equals the B = 1 call on that request: ids and images bit for bit.  The requests
    differ in masks, sources, labels, seeds and top_k; one is greedy, one keeps nothing"""
    vae, m = bf16_models
    B = 3
    keep_img = torch.stack([hole(1)[0], torch.zeros(16, 16, dtype=torch.bool), some_masks(16, 5)[0]])
    keep_ctrl = torch.stack([torch.ones(16, 16, dtype=torch.bool), torch.zeros(16, 16, dtype=torch.bool), some_masks(16, 6)[1]])
    m.deterministic_plan = True
    try:
        img = m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=keep_img, src_ctrl=src[0], keep_ctrl=keep_ctrl, trace=True, **ROWS)
        batch = trace_ids(m)
        assert bool((m.last_trace['forced'][1] == -1).all())
        for b in range(B):
            one = {k: v[b] for k, v in ROWS.items()}
            img1 = m.edit_infer_cfg(1, LABELS[b:b + 1], TYPES[b:b + 1], src_img=[t[b:b + 1] for t in src[1]], keep_img=keep_img[b:b + 1],
                                    src_ctrl=[t[b:b + 1] for t in src[0]], keep_ctrl=keep_ctrl[b:b + 1], trace=True, **one)
            for si, (x, y) in enumerate(zip(batch, trace_ids(m))):
                assert torch.equal(x[b:b + 1], y), (b, si)
            assert torch.equal(img[b:b + 1], img1), b
    finally:
        m.deterministic_plan = False


def check_edit_graph(m, graph, B, given, eager_sources, bad_source):
    """two successive runs with different masks each equal their eager call; a refused run leaves the graph as it was"""
    masks = (dict(keep_img=hole(B), keep_ctrl=True), dict(keep_img=some_masks(16, 7), keep_ctrl=some_masks(16, 8).flip(0)))
    outs = []
    for mk in masks:
        a = graph(LABELS, TYPES, **given, **mk, **ROWS)
        assert torch.equal(a, m.edit_infer_cfg(B, LABELS, TYPES, **eager_sources, **mk, **ROWS))
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    forced, ids = graph.forced(), graph.ids()
    with pytest.raises(ValueError, match='keep_img: True, None or a bool tensor'):
        graph(LABELS, TYPES, **given, keep_img=torch.ones(B, 16, 15, dtype=torch.bool), keep_ctrl=None, **ROWS)
    with pytest.raises((IndexError, ValueError), match='src_img'):
        graph(LABELS, TYPES, **dict(given, src_img=bad_source), **masks[0], **ROWS)
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        graph(LABELS, TYPES, **given, **masks[0], **dict(ROWS, top_k=[1, V + 1, 0]))
    assert all(torch.equal(a, b) for a, b in zip(graph.ids(), ids)) and torch.equal(graph.forced(), forced)
    assert torch.equal(graph(LABELS, TYPES, **given, **masks[1], **ROWS), outs[1])
    # nothing kept: the masks default to None, and the graph is the per-request joint call
    assert torch.equal(graph(LABELS, TYPES, **ROWS), m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, **ROWS))


def test_a_graph_over_flat_ids_equals_the_eager_call(gpu_device, bf16_models, src):
    vae, m = bf16_models
    B = 3
    graph = m.graphed_edit_generator(B, source='ids', cfg=2.5, top_k=600, top_p=0.8)
    given = dict(src_img=src[1], src_ctrl=torch.cat(src[0], dim=1))
    bad = [t.clone() for t in src[1]]
    bad[4][2, 3] = V
    check_edit_graph(m, graph, B, given, dict(src_img=src[1], src_ctrl=src[0]), bad)
    # what was given at capture are the defaults of run
    mk = dict(keep_img=hole(B), keep_ctrl=True)
    assert torch.equal(graph(LABELS, TYPES, **given, **mk, g_seed=[4, 5, 6]),
                       m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], src_ctrl=src[0], **mk, g_seed=[4, 5, 6], cfg=2.5, top_k=600, top_p=0.8))


def test_a_graph_over_pixels_equals_tokeniser_plus_eager_call(gpu_device, bf16_models):
    vae, m = bf16_models
    B = 3
    pix = (synth_images(B, 256, seed=43).to(gpu_device), synth_images(B, 256, seed=44).to(gpu_device))
    ids = (vae.img_to_idxBl(pix[0]), vae.img_to_idxBl(pix[1]))
    graph = m.graphed_edit_generator(B, source='pixels', decode='generated')
    mk = dict(keep_img=hole(B), keep_ctrl=True)
    a = graph(LABELS, TYPES, src_ctrl=pix[0], src_img=pix[1], **mk, **ROWS)
    want = m.edit_infer_cfg(B, LABELS, TYPES, src_ctrl=ids[0], src_img=ids[1], **mk, **ROWS)
    H = want.shape[-1]
    assert a.shape == (B, 3, H, H) and torch.equal(a, want[:, :, H:])                       # decode='generated': the image map only
    for got, ref in zip(graph.ids(), ids):
        assert torch.equal(got.long(), torch.cat(ref, dim=1))
    mk2 = dict(keep_img=some_masks(16, 9), keep_ctrl=some_masks(16, 10))
    b = graph(LABELS, TYPES, src_ctrl=pix[0], src_img=pix[1], **mk2, **ROWS)
    assert torch.equal(b, m.edit_infer_cfg(B, LABELS, TYPES, src_ctrl=ids[0], src_img=ids[1], **mk2, **ROWS)[:, :, H:]) and not torch.equal(a, b)
    with pytest.raises(ValueError, match='src_img: expected pixels'):
        graph(LABELS, TYPES, src_ctrl=pix[0], src_img=pix[1][:, :, :128], **mk, **ROWS)
    with pytest.raises(ValueError, match='keep_ctrl: True, None or a bool tensor'):
        graph(LABELS, TYPES, src_ctrl=pix[0], src_img=pix[1], keep_img=hole(B), keep_ctrl=torch.ones(B, 16, 16), **ROWS)
    assert torch.equal(graph(LABELS, TYPES, src_ctrl=pix[0], src_img=pix[1], **mk, **ROWS), a)


def test_plain_var_nothing_kept_and_partial(gpu_device, plain_models, src):
    vae, m = plain_models
    B = 3
    want = m.autoregressive_infer_cfg(B, LABELS, _trace=True, **ROWS)
    ref = trace_ids(m)
    got = m.edit_infer_cfg(B, LABELS, src_img=src[1], trace=True, **ROWS)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), si
    assert torch.equal(got, want) and got.shape == (B, 3, 256, 256)
    keep = hole(B)
    m.edit_infer_cfg(B, LABELS, src_img=src[1], keep_img=keep, trace=True, **ROWS)
    produced, forced = trace_ids(m), m.last_trace['forced'].clone()

    def rerun(ids):
        m._generate_rows(B, LABELS, ROWS['g_seed'], ROWS['cfg'], ROWS['top_k'], ROWS['top_p'], False, None, False, None, None, force_idx=ids, trace=True)
    check_partial(m, B, produced, forced, rerun, dict(img=keep), dict(img=src[1]), 1)
