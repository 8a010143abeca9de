"""Token log-probabilities end to end on the MI355X: logprobs=True of the generation calls and their graphs, and score_infer_cfg.
Ids, images and every comparison between two paths of this library are bit for bit; log-probability and entropy are held against a float64
reference on the traced combined logits of the path that takes no scores, inside the bounds of tests/score_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import lora, models  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VarConfig  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402
from score_ref import score_ref, within_bounds  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
V, B = 4096, 3
CFGS = {'control': VarConfig(depth=2), 'var': VarConfig(depth=2, mask_factor=1, control=False, multi_cond=False),
        'cos': VarConfig(depth=30, embed_dim=128, num_heads=2)}
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only
CFG3 = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (0.5, 4.0, 2.0)]
FIELDS = ('logprob', 'entropy', 'rank', 'argmax', 'sampled')
_MODELS = {}


def make(kind, dtype, dev):
    """the depth-2 control / plain models and the depth-30 cosine-attention model of the existing GPU tests, built once; 'bank': the control
    model with two adapters attached"""
    key = (kind, dtype)
    if key not in _MODELS:
        cfg = CFGS['control' if kind == 'bank' else kind]
        vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
        if cfg.control:
            m = models.ControlVAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                                  cond_drop_rate=0.0)
        else:
            m = models.VAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, patch_nums=PN, compute_dtype=dtype, cond_drop_rate=0.0)
        m = m.to(dev).eval()
        if kind == 'bank':
            mods, sds = dict(m.named_modules()), []
            for k, r in enumerate((16, 5)):
                g, sd = torch.Generator().manual_seed(40 + k), {}
                for t in lora.target_names(m):
                    out_f, in_f = mods[t]._parameters['weight'].shape
                    sd[f'{t}.lora_A.default.weight'] = (torch.rand(r, in_f, generator=g) * 2 - 1) / in_f ** 0.5
                    sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * 0.2
                sds.append(sd)
            lora.attach_adapters(m, sds)
        _MODELS[key] = (vae, m)
    return _MODELS[key]


@pytest.fixture(scope='module')
def src(gpu_device):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = make('control', F32, gpu_device)[0]
    return (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))


def hole(n, S=16, lo=4, hi=12):
    keep = torch.ones(n, S, S, dtype=torch.bool)
    keep[:, lo:hi, lo:hi] = False
    return keep


def trace_ids(m):
    return [x.clone() for x in m.last_trace['idx']]


def halves(ids, plain=False):
    """per-scale (B, l) ids of a trace (rows 0 .. B-1, control first) -> dict(ids_ctrl=, ids_img=) as score_infer_cfg takes them"""
    if plain:
        return dict(ids_img=[x[:B].long() for x in ids])
    return dict(ids_ctrl=[x[:B, :pn * pn].long() for x, pn in zip(ids, PN)], ids_img=[x[:B, pn * pn:].long() for x, pn in zip(ids, PN)])


def same(a, b, what, fields=FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, f)


def check_layout(sc, L):
    assert [tuple(getattr(sc, f).shape) for f in FIELDS] == [(B, L)] * 5
    assert [getattr(sc, f).dtype for f in FIELDS] == [torch.float32, torch.float32, torch.int32, torch.int32, torch.bool]
    assert bool(torch.isfinite(sc.logprob).all()) and bool(torch.isfinite(sc.entropy).all()) and bool((sc.logprob <= 0).all())
    assert bool((sc.rank >= 0).all()) and bool((sc.rank < V).all()) and bool((sc.argmax >= 0).all()) and bool((sc.argmax < V).all())


def against_trace(sc, logits, ids, what, cols=None):
    """the float64 reference on traced combined logits (per scale (B, l, V) fp32) and the ids (per scale (B, l)): bounds, rank and argmax exact"""
    x = np.concatenate([t[:B].cpu().numpy() for t in logits], axis=1)
    tgt = np.concatenate([t[:B].cpu().numpy() for t in ids], axis=1)
    ref_lp, ref_ent, ref_rank, ref_am = score_ref(x, tgt)
    c = slice(None) if cols is None else cols
    assert np.array_equal(sc.rank.cpu().numpy()[:, c], ref_rank[:, c]), what
    assert np.array_equal(sc.argmax.cpu().numpy()[:, c], ref_am[:, c]), what
    a, b = within_bounds(sc.logprob.cpu().numpy()[:, c], sc.entropy.cpu().numpy()[:, c], ref_lp[:, c], ref_ent[:, c])
    print(f'[score] {what}: worst logprob error {a:.3f} of its bound, worst entropy error {b:.3f} of its bound')
    assert a <= 1.0 and b <= 1.0, (what, a, b)


# ------------------------------------------------------------------------------------------------------------- (a) nothing else changes
@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('path', ['joint', 'conditional', 'edit'])
def test_ids_and_images_are_bit_equal_with_and_without_the_keyword(gpu_device, src, path, dtype):
    vae, m = make('control', dtype, gpu_device)
    if path == 'joint':
        def call(**kw):
            return m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS, **kw)
    elif path == 'conditional':
        def call(**kw):
            return m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, c_mask=src[0], _trace=True, **dict(ROWS, cfg=CFG3), **kw)
    else:
        def call(**kw):
            return m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=hole(B), src_ctrl=src[0], keep_ctrl=True, trace=True, **ROWS, **kw)
    want = call()
    ref = trace_ids(m)
    got, sc = call(logprobs=True)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), (path, si)
    assert torch.equal(got, want)
    check_layout(sc, m.cfg.pyramid.L)
    if path == 'joint':
        assert bool(sc.sampled.all())
    elif path == 'conditional':
        ctrl = sc.half_mask('control')
        assert sc.mask_first and not bool(sc.sampled[:, ctrl].any()) and bool(sc.sampled[:, ~ctrl].all())
        assert float(sc.total(half='image', sampled_only=True)[0]) == float(sc.total(half='image')[0]) and float(sc.total(half='control', sampled_only=True)[0]) == 0.0


# ------------------------------------------------------------------------------------------------------------- (b) (c) (h) joint generation
@pytest.mark.parametrize('kind,dtype', [('control', BF16), ('control', F32), ('var', BF16), ('cos', BF16), ('bank', BF16)])
def test_scores_of_a_generation_equal_score_infer_cfg_and_the_reference_on_the_traced_logits(gpu_device, kind, dtype):
    vae, m = make(kind, dtype, gpu_device)
    plain = kind == 'var'
    extra = dict(adapter=[0, -1, 1]) if kind == 'bank' else {}
    who = dict() if plain else dict(cond_type=TYPES)
    _, sc = m.autoregressive_infer_cfg(B, LABELS, _trace=True, logprobs=True, **who, **ROWS, **extra)
    ids = trace_ids(m)
    check_layout(sc, m.cfg.pyramid.L)
    # (b) the same tokens, scored without a sampling launch
    if plain:
        given = m.score_infer_cfg(B, LABELS, cfg=ROWS['cfg'], **halves(ids, True), **extra)
    else:
        given = m.score_infer_cfg(B, LABELS, TYPES, cfg=ROWS['cfg'], **halves(ids), **extra)
    same(sc, given, kind, FIELDS[:4])
    assert not bool(given.sampled.any()) and bool(sc.sampled.all())
    assert torch.equal(given.total(), sc.total()) and bool((given.total(sampled_only=True) == 0).all())
    # (c) the path this change does not touch: teacher-forced per-request generation with _trace, float64 on its combined logits
    m.autoregressive_infer_cfg(B, LABELS, _force_idx=ids, _trace=True, **who, **ROWS, **extra)
    against_trace(sc, m.last_trace['logits'], ids, f'{kind} generation')
    # (h) the greedy row: its id is the argmax, rank 0, everywhere
    flat = torch.cat(ids, dim=1)
    assert bool((sc.rank[1] == 0).all()) and torch.equal(sc.argmax[1], flat[1])
    assert bool((sc.rank[0] > 0).any())                             # ... and the sampled row is not greedy everywhere
    assert torch.equal(sc.rank == 0, sc.argmax == flat[:B])
    per = sc.per_scale()
    assert len(per) == len(PN) and [tuple(p.logprob.shape) for p in per] == [tuple(x[:B].shape) for x in ids]
    assert torch.equal(torch.cat([p.logprob for p in per], dim=1), sc.logprob)


def test_a_bidirectional_model_scores_both_half_orders(gpu_device):
    """the generation draws its (control, image) order from python's `random`; score_infer_cfg is told it, and the halves of total() follow it"""
    import random
    cfg = VarConfig(depth=2, bidirectional=True, type_pos=True)
    vae = models.build_vae(ch=32, compute_dtype=BF16).to(gpu_device)
    m = models.ControlVAR(vae, depth=2, embed_dim=cfg.C, num_heads=cfg.H, mask_factor=2, multi_cond=True, bidirectional=True, type_pos=True, patch_nums=PN,
                          compute_dtype=BF16, cond_drop_rate=0.0).to(gpu_device).eval()
    seen = {}
    for pyseed in range(8):
        random.seed(pyseed)
        _, sc = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, logprobs=True, **ROWS)
        if sc.mask_first in seen:
            continue
        ids = trace_ids(m)
        first, second = [x[:B, :pn * pn].long() for x, pn in zip(ids, PN)], [x[:B, pn * pn:].long() for x, pn in zip(ids, PN)]
        kw = dict(ids_ctrl=first, ids_img=second) if sc.mask_first else dict(ids_img=first, ids_ctrl=second)
        given = m.score_infer_cfg(B, LABELS, TYPES, cfg=ROWS['cfg'], mask_first=sc.mask_first, **kw)
        assert given.mask_first == sc.mask_first
        same(sc, given, f'mask_first={sc.mask_first}', FIELDS[:4])
        lead = torch.cat([torch.arange(2 * pn * pn) < pn * pn for pn in PN]).to(gpu_device)          # the half that comes first at every scale
        want = torch.where(lead[None], sc.logprob.double(), 0.0).sum(dim=1)
        assert torch.equal(sc.total(half='control' if sc.mask_first else 'image'), want)
        seen[sc.mask_first] = sc.total()
    assert set(seen) == {True, False}


# ------------------------------------------------------------------------------------------------------------- (d) a request does not depend on its batch
def test_row_b_of_a_mixed_permuted_batch_equals_the_b1_call(gpu_device):
    vae, m = make('bank', BF16, gpu_device)
    adapter = [0, -1, 1]
    m.deterministic_plan = True
    try:
        for perm in ([0, 1, 2], [2, 0, 1]):
            rows = {k: [v[b] for b in perm] for k, v in ROWS.items()}
            img, sc = m.autoregressive_infer_cfg(B, LABELS[perm], cond_type=TYPES[perm], logprobs=True, adapter=[adapter[b] for b in perm], **rows)
            for slot, b in enumerate(perm):
                img1, sc1 = m.autoregressive_infer_cfg(1, LABELS[b:b + 1], cond_type=TYPES[b:b + 1], logprobs=True, adapter=[adapter[b]],
                                                       **{k: v[b] for k, v in ROWS.items()})
                assert torch.equal(img[slot:slot + 1], img1), (perm, b)
                for f in FIELDS:
                    x, y = getattr(sc, f)[slot:slot + 1], getattr(sc1, f)
                    assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (perm, b, f)
    finally:
        m.deterministic_plan = False


# ------------------------------------------------------------------------------------------------------------- (e) an edit
def test_an_edit_marks_the_kept_tokens_and_scores_them_as_score_infer_cfg_does(gpu_device, src):
    vae, m = make('control', BF16, gpu_device)
    _, sc = m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=hole(B), src_ctrl=src[0], keep_ctrl=True, trace=True, logprobs=True, **ROWS)
    forced, ids = m.last_trace['forced'].clone(), trace_ids(m)
    assert torch.equal(sc.sampled, forced < 0)
    assert 0 < int(sc.sampled.sum()) < sc.sampled.numel()
    ctrl = sc.half_mask('control')
    assert not bool(sc.sampled[:, ctrl].any())                      # the control half is kept whole
    given = m.score_infer_cfg(B, LABELS, TYPES, cfg=ROWS['cfg'], **halves(ids))
    same(sc, given, 'edit', FIELDS[:4])                             # kept and free tokens alike: the head computes their logits anyway
    kept = ~sc.sampled
    assert torch.equal(sc.logprob[kept].view(torch.int32), given.logprob[kept].view(torch.int32))
    assert torch.equal(sc.total(sampled_only=True), torch.where(sc.sampled, sc.logprob.double(), 0.0).sum(dim=1))
    # plain VAR: the one half it has
    vae1, m1 = make('var', BF16, gpu_device)
    _, sc1 = m1.edit_infer_cfg(B, LABELS, src_img=src[1], keep_img=hole(B), trace=True, logprobs=True, **ROWS)
    assert torch.equal(sc1.sampled, m1.last_trace['forced'] < 0) and tuple(sc1.logprob.shape) == (B, m1.cfg.pyramid.L)
    same(sc1, m1.score_infer_cfg(B, LABELS, cfg=ROWS['cfg'], **halves(trace_ids(m1), True)), 'plain edit', FIELDS[:4])


# ------------------------------------------------------------------------------------------------------------- (f) one half given
@pytest.mark.parametrize('given', ['control', 'image'])
def test_given_one_half_scores_the_other_as_the_four_branch_trace_does(gpu_device, src, given):
    vae, m = make('control', BF16, gpu_device)
    sc = m.score_infer_cfg(B, LABELS, TYPES, ids_ctrl=src[0], ids_img=src[1], given=given, cfg=CFG3)
    check_layout(sc, m.cfg.pyramid.L)
    assert not bool(sc.sampled.any()) and sc.mask_first
    # conditional_infer_cfg on the same tokens in all four branches: the given half through c_mask / c_img, the other through _force_idx
    both = [torch.cat((c, i), dim=1).repeat(4, 1) for c, i in zip(*src)]
    teach = dict(c_mask=src[0]) if given == 'control' else dict(c_img=src[1])
    m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, _force_idx=both, _trace=True, **dict(ROWS, cfg=CFG3), **teach)
    other = sc.half_mask('image' if given == 'control' else 'control').numpy()
    against_trace(sc, m.last_trace['logits'], both, f"given='{given}'", cols=other)
    against_trace(sc, m.last_trace['logits'], both, f"given='{given}', both halves")
    want = torch.where(torch.from_numpy(other)[None].to(gpu_device), sc.logprob.double(), 0.0).sum(dim=1)
    assert torch.equal(sc.total(half='image' if given == 'control' else 'control'), want)
    # one triple is broadcast; another guidance gives other scores
    one = m.score_infer_cfg(B, LABELS, TYPES, ids_ctrl=src[0], ids_img=src[1], given=given, cfg=CFG3[0])
    assert torch.equal(one.logprob[0].view(torch.int32), sc.logprob[0].view(torch.int32)) and not torch.equal(one.logprob[2], sc.logprob[2])


# ------------------------------------------------------------------------------------------------------------- (g) graphs
def test_graph_replays_equal_the_eager_calls_with_a_refused_run_in_between(gpu_device, src):
    vae, m = make('control', BF16, gpu_device)
    rows2 = dict(g_seed=[4, 5, 6], cfg=[0.5, 2.0, 4.0], top_k=[1, 50, 900], top_p=[0.0, 1.0, 0.9])
    labels2, types2 = torch.tensor([7, 3, 250]), torch.tensor([2, 1, 0])
    src2 = ([t.flip(0) for t in src[0]], [t.flip(0) for t in src[1]])

    def check(graph_call, eager_call, refused):
        for k, (lab, ty, rows, s) in enumerate(((LABELS, TYPES, ROWS, src), (labels2, types2, rows2, src2), (LABELS, TYPES, ROWS, src))):
            img, sc = graph_call(lab, ty, rows, s)
            img_e, sc_e = eager_call(lab, ty, rows, s)
            assert torch.equal(img, img_e), k
            same(sc, sc_e, k)
            if k == 0:
                first = (img, sc)
                with pytest.raises(RuntimeError, match='selected index k out of range'):
                    refused()
            if k == 1:
                assert not torch.equal(sc.logprob, first[1].logprob)
            if k == 2:                                              # the results are copies: a later replay did not change the first one's
                assert torch.equal(img, first[0])
                same(sc, first[1], 'replayed')

    g = m.graphed_generator(B, per_request=True, logprobs=True)
    check(lambda lab, ty, rows, s: g(lab, ty, **rows),
          lambda lab, ty, rows, s: m.autoregressive_infer_cfg(B, lab, cond_type=ty, logprobs=True, **rows),
          lambda: g(LABELS, TYPES, **dict(ROWS, top_k=[1, V + 1, 0])))
    del g
    g = m.graphed_conditional_generator(B, given='control', per_request=True, logprobs=True)
    check(lambda lab, ty, rows, s: g(lab, ty, s[0], **dict(rows, cfg=CFG3)),
          lambda lab, ty, rows, s: m.conditional_infer_cfg(B, lab, cond_type=ty, c_mask=s[0], logprobs=True, **dict(rows, cfg=CFG3)),
          lambda: g(LABELS, TYPES, src[0], **dict(ROWS, cfg=CFG3, top_k=[1, V + 1, 0])))
    del g
    g = m.graphed_edit_generator(B, logprobs=True)
    mk = dict(keep_img=hole(B), keep_ctrl=True)
    check(lambda lab, ty, rows, s: g(lab, ty, src_img=s[1], src_ctrl=s[0], **mk, **rows),
          lambda lab, ty, rows, s: m.edit_infer_cfg(B, lab, ty, src_img=s[1], src_ctrl=s[0], logprobs=True, **mk, **rows),
          lambda: g(LABELS, TYPES, src_img=src[1], src_ctrl=src[0], **mk, **dict(ROWS, top_k=[1, V + 1, 0])))
    # a graph captured without the keyword returns images only, as before
    g = m.graphed_generator(B, per_request=True)
    assert torch.is_tensor(g(LABELS, TYPES, **ROWS))
