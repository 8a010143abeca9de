"""kv_precision='fp8' end to end on MI355X: generation over an e4m3 K/V arena with one power-of-two scale per (token, head).

Logit distance.  On the depth-2 fixtures of the strict fp32 generation tests (tests/test_gpu_parity.py: GEN_CASES) the model runs in the fp32 mode, in the
bf16 mode, in the bf16 mode with the e4m3 cache, and under gemm_precision='fp8' without and with it, teacher-forced along the fixture's ids; the per-scale CFG
logits of the four reduced-precision modes are held against the FP32 MODE's logits on the same ids, relative to max|logit| of the scale, and reported side by
side.  KV8_REL_MEASURED / KV8_FP8_REL_MEASURED are the worst values of the two cache modes measured on MI355X over those fixtures, the asserted bounds twice
that - the margin X3_REL_BOUND and FP8_REL_BOUND take over their own measurements; it covers box-to-box fp32 ordering effects.  A regression fence, not a
quality claim.

Greedy ids.  How many of the ids each mode picks along that trace differ from the fixture's is printed and recorded; it is not asserted.

Inherited properties, once each at B = 3 on a depth-2 bf16 model with the e4m3 cache: a request does not depend on its batch (the scales are per token and
head: exact under deterministic_plan), one replay of each graphed generator equals the eager call, logprobs=True equals score_infer_cfg, a cos-attention
(d30-style) model runs and its row does not depend on the batch, forward() is a plain bf16 model's, a kv_precision=None model's bits are the same before and
after a model of this mode ran in the process, and the arena is uint8 at 17/32 of the bf16 arena's bytes."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import golden, record  # noqa: E402
from controlvar_amd import models  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402
from test_gpu_parity import GEN_CASES, make_vae, make_var  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
# measured on MI355X: worst per-scale max|logit - logit_fp32| / max|logit_fp32| over the fixtures below, teacher-forced along the fixture's ids
# bf16 + e4m3 cache: gen_var_d2_b2 1.438e-2; the other six fixtures 8.8e-3 ... 1.30e-2 (the bf16 mode on the same runs: 5.9e-3 ... 6.5e-3, gen_d2sa_b2 1.30e-2)
# gemm_precision='fp8' + e4m3 cache: gen_var_d2s_b2 6.250e-2; the other six 4.76e-2 ... 5.82e-2 (gemm_precision='fp8' alone: 4.98e-2 ... 6.74e-2 - the cache does
# not add to the distance of that mode, it moves it by a few percent either way)
KV8_REL_MEASURED = 1.44e-2                # compute_dtype=bfloat16, kv_precision='fp8'
KV8_FP8_REL_MEASURED = 6.3e-2             # ... with gemm_precision='fp8' as well
KV8_REL_BOUND = 2 * KV8_REL_MEASURED
KV8_FP8_REL_BOUND = 2 * KV8_FP8_REL_MEASURED

FIXTURES = {k: v for k, v in GEN_CASES.items() if v['cfg'].depth == 2}


def t(a):
    return torch.from_numpy(np.asarray(a))


def forced_run(m, case, forced):
    labels = torch.tensor(case['labels'])
    kw = dict(g_seed=0, cfg=case['scale'], top_k=1, top_p=0.0, _trace=True, _force_idx=forced)
    if case['cfg'].control and case['types'] is not None:
        kw['cond_type'] = torch.tensor(case['types'])
    if 'pyseed' in case:
        random.seed(case['pyseed'])
    img = m.autoregressive_infer_cfg(case['B'], labels, **kw)
    tr = m.last_trace
    return img.cpu(), [x.float().cpu().clone() for x in tr['logits']], [x.cpu().long().clone() for x in tr['idx']]


def arenas(m):
    return [ent[1] for ent in (m._arena or {}).values()]


def test_the_fixtures_are_the_depth_2_ones():
    assert len(FIXTURES) == 7 and KV8_REL_BOUND == 2 * KV8_REL_MEASURED and KV8_FP8_REL_BOUND == 2 * KV8_FP8_REL_MEASURED


@pytest.mark.parametrize('name', list(FIXTURES))
def test_logit_distance_to_the_fp32_mode_with_and_without_the_e4m3_cache(gpu_device, name):
    case = FIXTURES[name]
    g = golden(name)
    mf = case['cfg'].mask_factor
    ref_ids = t(g['ids'].astype(np.int64))
    forced, o = [], 0
    for p in PN:
        forced.append(ref_ids[:, o:o + mf * p * p].contiguous())
        o += mf * p * p
    m32 = make_var(make_vae(32, F32, gpu_device), case['cfg'], F32, gpu_device, seed=case.get('seed', 0))
    _, lg32, _ = forced_run(m32, case, forced)
    del m32
    m = make_var(make_vae(32, BF16, gpu_device), case['cfg'], BF16, gpu_device, seed=case.get('seed', 0))
    runs = {}
    for mode, (gp, kv) in {'bf16': (None, None), 'bf16+kv8': (None, 'fp8'), 'fp8': ('fp8', None), 'fp8+kv8': ('fp8', 'fp8')}.items():
        m.gemm_precision, m.kv_precision = gp, kv               # the switches on a built model
        img, lg, idx = forced_run(m, case, forced)
        assert torch.isfinite(img).all(), mode
        (a,) = arenas(m)
        assert isinstance(a, models.KV8Arena) == (kv == 'fp8') and (a.q.dtype == torch.uint8 if kv else a.dtype == BF16), mode
        worst = max(float((lg[si] - lg32[si]).abs().max()) / float(lg32[si].abs().max()) for si in range(len(PN)))
        runs[mode] = (worst, sum(int((a_ != b_).sum()) for a_, b_ in zip(idx, forced)))
    print(f'[kv8] {name}: worst per-scale logit distance to the fp32 mode, of max|logit|: ' + ', '.join(f'{k} {v[0]:.3e}' for k, v in runs.items())
          + f' (bounds: bf16+kv8 {KV8_REL_BOUND:.1e}, fp8+kv8 {KV8_FP8_REL_BOUND:.1e}); greedy ids moved against the reference: '
          + ', '.join(f'{k} {v[1]}' for k, v in runs.items()) + f' of {ref_ids.numel()}')
    record(f'kv8 {name}', kind='kv8_logits', bound=KV8_REL_BOUND, bound_fp8=KV8_FP8_REL_BOUND, total=int(ref_ids.numel()),
           **{'rel_' + k.replace('+', '_'): v[0] for k, v in runs.items()}, **{'flips_' + k.replace('+', '_'): v[1] for k, v in runs.items()})
    assert runs['bf16+kv8'][0] <= KV8_REL_BOUND
    assert runs['fp8+kv8'][0] <= KV8_FP8_REL_BOUND


# ================================================================================================ inherited properties
B = 3
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only
CFG3 = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (0.5, 4.0, 2.0)]
FIELDS = ('logprob', 'entropy', 'rank', 'argmax', 'sampled')


def build(dev, kv='fp8', **kw):
    vae = models.build_vae(ch=32, compute_dtype=BF16).to(dev)
    return vae, models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=BF16, cond_drop_rate=0.0,
                                         kv_precision=kv, **kw).to(dev).eval()


@pytest.fixture(scope='module')
def kv8_models(gpu_device):
    return build(gpu_device)


@pytest.fixture(scope='module')
def src(gpu_device, kv8_models):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = kv8_models[0]
    return (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))


def hole(n, S=16, lo=4, hi=12):
    keep = torch.ones(n, S, S, dtype=torch.bool)
    keep[:, lo:hi, lo:hi] = False
    return keep


def trace_ids(m):
    return [x.clone() for x in m.last_trace['idx']]


def same(a, b, what, fields=FIELDS):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape, (what, f)
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (what, f)


def permuted_batch_equals_b1(m, control=True):
    m.deterministic_plan = True
    try:
        perm = [2, 0, 1]
        rows = {k: [v[b] for b in perm] for k, v in ROWS.items()}
        types = (lambda sl: dict(cond_type=TYPES[sl])) if control else (lambda sl: {})
        img, sc = m.autoregressive_infer_cfg(B, LABELS[perm], logprobs=True, **types(perm), **rows)
        for slot, b in enumerate(perm):
            img1, sc1 = m.autoregressive_infer_cfg(1, LABELS[b:b + 1], logprobs=True, **types(slice(b, b + 1)), **{k: v[b] for k, v in ROWS.items()})
            assert torch.equal(img[slot:slot + 1], img1), b
            for f in FIELDS:
                x, y = getattr(sc, f)[slot:slot + 1], getattr(sc1, f)
                assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (b, f)
    finally:
        m.deterministic_plan = False


def test_row_b_of_a_permuted_batch_equals_the_b1_call(gpu_device, kv8_models):
    permuted_batch_equals_b1(kv8_models[1])


def test_a_cos_attention_model_runs_and_its_row_does_not_depend_on_the_batch(gpu_device):
    """the d30 configuration's path on a depth-2 plain VAR (a joint model takes it at depth 30 only): cos_qk_norm runs on the pass's scratch (Lmax = l,
    q_off = 0) in front of the append"""
    vae = models.build_vae(ch=32, compute_dtype=BF16).to(gpu_device)
    m = models.build_var(vae, depth=2, cos_attn=True, compute_dtype=BF16, cond_drop_rate=0.0, kv_precision='fp8').to(gpu_device).eval()
    assert m.cfg.uses_cos_attn
    permuted_batch_equals_b1(m, control=False)
    (a,) = arenas(m)
    assert isinstance(a, models.KV8Arena)


def test_scores_of_a_generation_equal_score_infer_cfg(gpu_device, kv8_models):
    vae, m = kv8_models
    _, sc = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, logprobs=True, **ROWS)
    ids = trace_ids(m)
    given = m.score_infer_cfg(B, LABELS, TYPES, cfg=ROWS['cfg'], ids_ctrl=[x[:B, :pn * pn].long() for x, pn in zip(ids, PN)],
                              ids_img=[x[:B, pn * pn:].long() for x, pn in zip(ids, PN)])
    same(sc, given, 'kv8 generation', FIELDS[:4])
    assert not bool(given.sampled.any()) and bool(sc.sampled.all())


def test_one_replay_of_each_graphed_generator_equals_the_eager_call(gpu_device, kv8_models, src):
    vae, m = kv8_models
    g = m.graphed_generator(B, per_request=True, logprobs=True)
    img, sc = g(LABELS, TYPES, **ROWS)
    img_e, sc_e = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, logprobs=True, **ROWS)
    assert torch.equal(img, img_e)
    same(sc, sc_e, 'joint')
    assert any(isinstance(x, tuple) and isinstance(x[1], models.KV8Arena) for x in g.owned)          # the captured arena is the e4m3 one
    del g
    g = m.graphed_conditional_generator(B, given='control', per_request=True, logprobs=True)
    img, sc = g(LABELS, TYPES, src[0], **dict(ROWS, cfg=CFG3))
    img_e, sc_e = m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, c_mask=src[0], logprobs=True, **dict(ROWS, cfg=CFG3))
    assert torch.equal(img, img_e)
    same(sc, sc_e, 'conditional')
    del g
    g = m.graphed_edit_generator(B, logprobs=True)
    mk = dict(keep_img=hole(B), keep_ctrl=True)
    img, sc = g(LABELS, TYPES, src_img=src[1], src_ctrl=src[0], **mk, **ROWS)
    img_e, sc_e = m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], src_ctrl=src[0], logprobs=True, **mk, **ROWS)
    assert torch.equal(img, img_e)
    same(sc, sc_e, 'edit')


def test_forward_on_a_model_of_this_mode_is_the_bf16_path(gpu_device, kv8_models):
    """forward() keeps the bf16 arena and the bf16 launches: the same bits as a plain bf16 model's"""
    vae, m = kv8_models
    _, m16 = build(gpu_device, kv=None)
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, m.cfg.pyramid.L - m.cfg.pyramid.first_l, 32, generator=gen).to(gpu_device)
    labels, types = torch.tensor([3, 7]), torch.tensor([0, 1])
    with torch.no_grad():
        a, b = m(labels, x, types, True), m16(labels, x, types, True)
    assert torch.equal(a, b)
    assert all(not isinstance(x, models.KV8Arena) and x.dtype == BF16 for x in arenas(m))


def test_a_plain_model_gives_the_same_bits_after_a_model_of_this_mode_ran_and_the_arena_is_17_32(gpu_device):
    vae, m = build(gpu_device, kv=None)

    def run():
        img = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
        return img, torch.cat(m.last_trace['idx'], dim=1), [x.clone() for x in m.last_trace['logits']]
    before = run()
    (a16,) = arenas(m)
    assert a16.dtype == BF16
    _, mx = build(gpu_device)
    mx.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, **ROWS)
    (a8,) = arenas(mx)
    assert a8.q.dtype == torch.uint8 and a8.scale.dtype == F32
    assert 32 * (a8.q.numel() * a8.q.element_size() + a8.scale.numel() * a8.scale.element_size()) == 17 * a16.numel() * a16.element_size()
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    for x, y in zip(before[2], after[2]):
        assert torch.equal(x, y)
    # and the two modes differ: the e4m3-cache model is not silently the bf16 one
    mx.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    assert not all(torch.equal(x, y) for x, y in zip(mx.last_trace['logits'], after[2]))
