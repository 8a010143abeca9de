"""gemm_precision='bf16x3' end to end on MI355X: the fp32 model with split-bf16 linear layers.

Logit distance.  On the fixtures of the strict fp32 generation tests (tests/test_gpu_parity.py: GEN_CASES and gen_d12_b2) the model runs in this mode, teacher-forced
along the fixture's ids, and its per-scale CFG logits are held against the FP32 MODE's logits on the same ids, relative to max|logit| of the scale.
X3_REL_MEASURED is the worst value measured on MI355X over those fixtures, X3_REL_BOUND twice that - the rule BF16_REL_BOUND was set by.  One condition is
derived, not measured: the operand error is 2^-17 against bf16's 2^-9, a factor 256, of which a factor 8 is left to the different summation plan - so
X3_REL_BOUND <= BF16_REL_BOUND / 32, asserted below.

Greedy ids.  The ids the mode picks along that trace against the fixture's ids and recorded margins: a flip is allowed only where the reference's own top-1 /
top-2 margin is below X3_REL_BOUND * max|logit| of the scale (conftest.ids_parity, strict=False), on all nine fixtures.  Measured on MI355X: 1 flip over the
nine fixtures' 24 480 ids - gen_d2sa_b2, scale 8, at a reference margin of 1.5e-5 (the bf16 mode moves 35-38 of 2 720, the fp32 mode 0).
The float / image checks run on the flip-free rows (maxabs_on, min_rows=1) of the fixtures whose recorded margins GUARANTEE such a row: computed on the host
from the fixtures' margins and the per-scale max|logit| of the fp32 mode, at the tolerance 6.2e-5 * max|logit| (1e-3 ... 5e-3) gen_d2_b2, gen_d30n_b2,
gen_d2b_b2, gen_var_d2s_b2 and gen_d12_b2 each keep one row whose every margin is above it (1 to 2 ids per fixture lie below); gen_d2_b4none (5 ids below,
spread over all four rows), gen_var_d2_b2 (2), gen_d2v_b2 (4) and gen_d2sa_b2 (8) do not and are dropped from the image checks (IMAGE_DROPPED) - their
logit distance and their ids are still checked.

Inherited properties, once each in this mode at B <= 4: a request does not depend on its batch (deterministic_plan), graph replays of the three generators
equal the eager calls, logprobs=True equals score_infer_cfg, an edit that keeps nothing is the joint call, a merged LoRA model equals the pre-merged one; the
cosine-attention, shared_aln and plain VAR models are among the fixtures.  And the two existing modes give the same bits before and after a model of this mode
was built and run in the process."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import golden, ids_parity, maxabs_on, record  # noqa: E402
from controlvar_amd import lora, models  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VarConfig  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402
from test_gpu_configs import BF16_REL_BOUND  # noqa: E402
from test_gpu_parity import GEN_CASES, make_vae, make_var  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
# measured on MI355X: worst per-scale max|logit_x3 - logit_fp32| / max|logit_fp32| over the fixtures below, teacher-forced along the fixture's ids
# gen_d2sa_b2 3.07e-5 (its max|logit| is 15-22 where the others reach 55-86); the other eight fixtures 1.29e-5 ... 1.75e-5
X3_REL_MEASURED = 3.1e-5
X3_REL_BOUND = 2 * X3_REL_MEASURED
V = 4096

IMAGE_DROPPED = ('gen_d2_b4none', 'gen_var_d2_b2', 'gen_d2v_b2', 'gen_d2sa_b2')       # no row guaranteed flip-free by the recorded margins: see above
FIXTURES = dict(GEN_CASES, gen_d12_b2=dict(cfg=VarConfig(depth=12), B=2, labels=[3, 7], scale=4.0, types=[0, 1], ch=160, img_tol=(3e-3, 3e-4)))


def t(a):
    return torch.from_numpy(np.asarray(a))


def test_the_bound_leaves_the_factor_the_operand_error_promises():
    assert X3_REL_BOUND == 2 * X3_REL_MEASURED and X3_REL_BOUND <= BF16_REL_BOUND / 32


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


@pytest.mark.parametrize('name', list(FIXTURES))
def test_logits_and_greedy_ids_along_the_references_trace(gpu_device, name):
    case = FIXTURES[name]
    g = golden(name)
    mf = case['cfg'].mask_factor
    vae = make_vae(case.get('ch', 32), F32, gpu_device)
    m = make_var(vae, case['cfg'], F32, gpu_device, seed=case.get('seed', 0))
    ref_ids = t(g['ids'].astype(np.int64))
    forced, o = [], 0
    for p in PN:
        forced.append(ref_ids[:, o:o + mf * p * p].contiguous())
        o += mf * p * p
    img32, lg32, _ = forced_run(m, case, forced)
    m.gemm_precision = 'bf16x3'                          # the switch on a built model: pack and arena are rebuilt
    img, lg, idx = forced_run(m, case, forced)
    assert m._pack().get('w_qkv_x3') is not None and 'w_qkv' not in m._pack()
    assert torch.isfinite(img).all()
    worst, o, flips, amaxes = 0.0, 0, 0, []
    rows_ok = np.ones(ref_ids.shape[0], dtype=bool)
    for si, p in enumerate(PN):
        l = mf * p * p
        amax = float(lg32[si].abs().max())
        rel = float((lg[si] - lg32[si]).abs().max()) / amax
        worst = max(worst, rel)
        amaxes.append(amax)
        n, ok = ids_parity(idx[si], forced[si], g['margin'][:, o:o + l], X3_REL_BOUND * amax, f'x3 {name} scale {si}', strict=False)
        flips += n
        rows_ok &= ok
        o += l
    print(f'[x3] {name}: worst per-scale logit distance to the fp32 mode {worst:.3e} of max|logit| (measured {X3_REL_MEASURED:.1e}, bound {X3_REL_BOUND:.1e}); '
          f'{flips} of {ref_ids.numel()} greedy ids flipped')
    record(f'x3 {name}', kind='x3_logits', worst_rel=worst, bound=X3_REL_BOUND, flips=flips, total=int(ref_ids.numel()), amax_per_scale=amaxes)
    assert worst <= X3_REL_BOUND
    assert torch.equal(img, img32)                       # the same ids through the same fp32 VQVAE
    if name in IMAGE_DROPPED:
        return
    tol_img, tol_mean = case.get('img_tol', (2e-3, 2e-4))
    assert maxabs_on(img[:, :, 100:116, 60:76] - t(g['img_crop']), rows_ok, min_rows=1) < tol_img
    assert maxabs_on(img[:, :, -20:-4, 200:216] - t(g['img_crop2']), rows_ok, min_rows=1) < tol_img
    assert maxabs_on(img.mean(dim=(2, 3)) - t(g['img_mean']), rows_ok, min_rows=1) < tol_mean


# ================================================================================================ inherited properties
B = 3
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only
CFG3 = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (0.5, 4.0, 2.0)]
FIELDS = ('logprob', 'entropy', 'rank', 'argmax', 'sampled')


def build(dev, gp='bf16x3', dtype=F32):
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    return vae, models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0,
                                         gemm_precision=gp).to(dev).eval()


@pytest.fixture(scope='module')
def x3_models(gpu_device):
    return build(gpu_device)


@pytest.fixture(scope='module')
def src(gpu_device, x3_models):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = x3_models[0]
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


def test_row_b_of_a_batch_equals_the_b1_call(gpu_device, x3_models):
    vae, m = x3_models
    m.deterministic_plan = True
    try:
        perm = [2, 0, 1]
        rows = {k: [v[b] for b in perm] for k, v in ROWS.items()}
        img, sc = m.autoregressive_infer_cfg(B, LABELS[perm], cond_type=TYPES[perm], logprobs=True, **rows)
        for slot, b in enumerate(perm):
            img1, sc1 = m.autoregressive_infer_cfg(1, LABELS[b:b + 1], cond_type=TYPES[b:b + 1], logprobs=True, **{k: v[b] for k, v in ROWS.items()})
            assert torch.equal(img[slot:slot + 1], img1), b
            for f in FIELDS:
                x, y = getattr(sc, f)[slot:slot + 1], getattr(sc1, f)
                assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y), (b, f)
    finally:
        m.deterministic_plan = False


def test_scores_of_a_generation_equal_score_infer_cfg(gpu_device, x3_models):
    vae, m = x3_models
    _, sc = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, logprobs=True, **ROWS)
    ids = trace_ids(m)
    given = m.score_infer_cfg(B, LABELS, TYPES, cfg=ROWS['cfg'], ids_ctrl=[x[:B, :pn * pn].long() for x, pn in zip(ids, PN)],
                              ids_img=[x[:B, pn * pn:].long() for x, pn in zip(ids, PN)])
    same(sc, given, 'x3 generation', FIELDS[:4])
    assert not bool(given.sampled.any()) and bool(sc.sampled.all())
    flat = torch.cat(ids, dim=1)
    assert bool((sc.rank[1] == 0).all()) and torch.equal(sc.argmax[1], flat[1])          # the greedy row


def test_an_edit_that_keeps_nothing_is_the_per_request_joint_call(gpu_device, x3_models, src):
    vae, m = x3_models
    want = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    ref = trace_ids(m)
    nothing = torch.zeros(B, 16, 16, dtype=torch.bool)
    for kw in (dict(), dict(src_img=src[1], keep_img=nothing, src_ctrl=src[0], keep_ctrl=nothing.to(gpu_device))):
        got = m.edit_infer_cfg(B, LABELS, TYPES, trace=True, **kw, **ROWS)
        for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
            assert torch.equal(x, y), si
        assert torch.equal(got, want)
        assert bool((m.last_trace['forced'] == -1).all())


def test_graph_replays_equal_the_eager_calls_with_a_refused_run_in_between(gpu_device, x3_models, src):
    vae, m = x3_models
    rows2 = dict(g_seed=[4, 5, 6], cfg=[0.5, 2.0, 4.0], top_k=[1, 50, 900], top_p=[0.0, 1.0, 0.9])
    labels2, types2 = torch.tensor([7, 3, 250]), torch.tensor([2, 1, 0])
    src2 = ([x.flip(0) for x in src[0]], [x.flip(0) for x in src[1]])

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


def test_a_merged_lora_model_equals_the_model_built_from_the_merged_weights(gpu_device):
    """W + s B A is folded in fp32 BEFORE the split, so the adapter costs nothing and changes nothing in this mode"""
    vae, m = build(gpu_device)
    lora.add_lora(m, r=16, dropout=0.0, seed=1)
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for _, (_, Bm) in lora.adapters(m).items():
            Bm.copy_(torch.randn(Bm.shape, generator=gen) * 0.2)
    m.eval()
    _, m2 = build(gpu_device)
    lora.add_lora(m2, dropout=0.0)
    lora.load_lora(m2, lora.lora_state_dict(m, 'peft'))
    lora.merge_lora(m2)
    m2.eval()
    assert m2.gemm_precision == 'bf16x3' and not lora.has_lora(m2)
    labels, types = torch.tensor([3, 7]), torch.tensor([0, 1])
    out = []
    for mm in (m, m2):
        img = mm.autoregressive_infer_cfg(2, labels, g_seed=0, cfg=4.0, top_k=1, cond_type=types, _trace=True)
        out.append((img, torch.cat(mm.last_trace['idx'], dim=1), [x.clone() for x in mm.last_trace['logits']]))
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][0], out[1][0])
    for a, b in zip(out[0][2], out[1][2]):
        assert torch.equal(a, b)
    # ... and the adapters did something: the base model picks other tokens
    _, m0 = build(gpu_device)
    m0.autoregressive_infer_cfg(2, labels, g_seed=0, cfg=4.0, top_k=1, cond_type=types, _trace=True)
    assert not torch.equal(torch.cat(m0.last_trace['idx'], dim=1), out[0][1])


def test_forward_on_a_model_of_this_mode_is_the_fp32_path(gpu_device, x3_models):
    """forward() runs the fp32 matrices (built on first use) in every gemm_precision: the same bits as an fp32 model's"""
    vae, m = x3_models
    _, m32 = build(gpu_device, gp=None)
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, m.cfg.pyramid.L - m.cfg.pyramid.first_l, 32, generator=gen).to(gpu_device)
    labels, types = torch.tensor([3, 7]), torch.tensor([0, 1])
    with torch.no_grad():
        a, b = m(labels, x, types, True), m32(labels, x, types, True)
    assert torch.equal(a, b)
    assert 'w_qkv' in m._pack() and 'w_qkv_x3' in m._pack()


@pytest.mark.parametrize('dtype', [BF16, F32], ids=['bf16', 'fp32'])
def test_the_existing_modes_give_the_same_bits_after_a_model_of_this_mode_ran(gpu_device, dtype):
    vae, m = build(gpu_device, gp=None, dtype=dtype)

    def run():
        img = m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
        return img, torch.cat(m.last_trace['idx'], dim=1), [x.clone() for x in m.last_trace['logits']]
    before = run()
    _, mx = build(gpu_device)
    mx.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, **ROWS)
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    for a, b in zip(before[2], after[2]):
        assert torch.equal(a, b)
    assert not any(k.endswith('_x3') for k in m._pack())
