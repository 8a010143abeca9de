"""Regional guidance on the MI355X (include/cvar_region.h): the weight table against the float64 restatement of tests/region_ref.py, the
per-token sampler and score launches against the per-request ones token by token, and region_infer_cfg / graphed_region_generator against the
per-request joint path, the edit path and each other.  Ids, logits, weights of pure bins and images are compared bit for bit; the table's other
entries within 1 fp32 ulp of the float64 value (half an ulp is the final rounding, the float64 sums of at most 1024 terms add about 1e-13 relative);
log-probabilities inside the bounds of tests/score_ref.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import region_ref as R  # noqa: E402
from controlvar_amd import lora, models, ops  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, PATCH_NUMS_512 as PN512  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402
from score_ref import combine_f32, score_ref, within_bounds  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
V = 4096
NAN = float('nan')


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def fenced(t, dev, fence=64):
    """t on the device between two NaN pads -> (the whole buffer, the view that holds t)"""
    buf = torch.full((t.numel() + 2 * fence,), NAN, dtype=t.dtype, device=dev)
    view = buf[fence:fence + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def pads_are_nan(buf, n, fence=64):
    return bool(torch.isnan(buf[:fence]).all()) and bool(torch.isnan(buf[fence + n:]).all())


# ------------------------------------------------------------------------------------------------------------- 3. the table
_REF = {}


def table_case(K, pns, mf, with_strength):
    """the inputs and the float64 reference of one case, computed once"""
    key = (K, pns[-1], mf, with_strength)
    if key not in _REF:
        B, S = 3, pns[-1]
        w = R.region_maps(B, K, S, 10 * K + S)
        st = None
        if with_strength:                                          # multiples of 1/4 in [0, 2]: their float64 sums are exact in any order, so pure bins
            st = (np.random.default_rng(S + K).integers(0, 9, (B, S, S)) / 4).astype(np.float32)          # stay exact under a strength map;
            st[2] = np.random.default_rng(5).random((S, S), dtype=np.float32) * 3                         # row 2: arbitrary factors
        cf = np.array([[1.5, 4.0, 0.25], [3.0, 0.0, 7.5], [0.7, 2.2, 1.1]])[:, :K]
        _REF[key] = (w, st, cf) + R.coef_ref(w, st, cf, pns, mf)
    return _REF[key]


@pytest.mark.parametrize('with_strength', [False, True], ids=['plain', 'strength'])
@pytest.mark.parametrize('mf', [1, 2])
@pytest.mark.parametrize('pns', [PN, PN512], ids=['S16', 'S32'])
@pytest.mark.parametrize('K', [1, 2, 3])
def test_table_against_the_float64_restatement(gpu_device, K, pns, mf, with_strength):
    dev, B, S = gpu_device, 3, pns[-1]
    w, st, cf, ref, pure = table_case(K, pns, mf, with_strength)
    L = ref.shape[1]
    wb, wd = fenced(torch.from_numpy(w), dev)
    sb, sd = fenced(torch.from_numpy(st), dev) if st is not None else (None, None)
    cb, cd = fenced(torch.from_numpy(cf.copy()), dev)
    runs = []
    for mask_first in (True, False, True):
        ob, out = fenced(torch.full((B, L, 4), NAN), dev)
        ops.region_coef_table(wd, sd, cd, pns, B, K, mask_first, mf, out)
        torch.cuda.synchronize()
        assert pads_are_nan(ob, out.numel()) and pads_are_nan(wb, wd.numel()) and pads_are_nan(cb, cd.numel())
        assert sb is None or pads_are_nan(sb, sd.numel())
        runs.append(out.clone())
    # the same inputs give the same bits; both halves read the same maps, so the order of the halves changes no value
    assert same_bits(runs[0], runs[2]) and same_bits(runs[0], runs[1])
    got = runs[0].cpu().numpy()
    assert np.isfinite(got).all()
    worst = float(R.ulps(got, ref).max())
    print(f'[region table] K={K} S={S} mf={mf} strength={with_strength}: worst entry {worst:.3f} fp32 ulp from the float64 value; '
          f'{int(pure.sum())} of {pure.size} tokens in pure bins')
    assert worst <= 1.0
    exact = pure.copy()
    if with_strength:
        exact[2] = False                                           # arbitrary factors: the mean of the strength is a rounded sum there
    assert exact[1].any() and (K == 1 or not pure[0].all())
    assert np.array_equal(got[exact].view(np.int32), ref[exact].astype(np.float32).view(np.int32))
    assert np.array_equal(got[:, :, K + 1:], np.zeros_like(got[:, :, K + 1:]))          # unused slots


def test_table_at_one_label_uniform_is_the_per_request_table(gpu_device):
    dev, B = gpu_device, 3
    cfgs = [1.5, 4.0, 0.3]
    for pns, mf in ((PN, 2), (PN512, 1)):
        S = pns[-1]
        want = models._request_table(B, cfgs, 0, 0.0, 0, False, V, len(pns)).coef
        out = torch.full((B, mf * sum(p * p for p in pns), 4), NAN, device=dev)
        ops.region_coef_table(torch.ones(B, 1, S, S, device=dev), None, torch.tensor(cfgs, dtype=torch.float64, device=dev)[:, None].contiguous(), pns, B, 1,
                              True, mf, out)
        o = 0
        for si, pn in enumerate(pns):
            n = mf * pn * pn
            assert same_bits(out[:, o:o + n].cpu(), want[si][:, None].expand(B, n, 4).contiguous()), si
            o += n


# ------------------------------------------------------------------------------------------------------------- 4. the sampler and the score launch
SETTINGS = {'greedy': ([1, 1], [0.0, 0.0]), 'top-k': ([900, 50], [0.0, 0.0]), 'top-p': ([0, 0], [0.96, 0.5]), 'mixed': ([1, 700], [0.0, 0.9])}


def map_inputs(nrep, dev, B=2, l=8):
    g = torch.Generator().manual_seed(100 + nrep)
    lg = (torch.randn(nrep * B, l, V, generator=g) * 3.0).to(dev)
    wide = torch.full((B, l + 5, 4), NAN)                          # this stage's columns inside a wider table: ldc = l + 5
    wide[:, 3:3 + l] = torch.randn(B, l, 4, generator=g) * 1.5
    wide[:, 3:3 + l, nrep:] = 0.0
    return lg, wide.to(dev)[:, 3:3 + l]


def outputs(B, l, dev):
    return (torch.full((B, l), -1, dtype=torch.int32, device=dev), torch.full((B, l, V), NAN, device=dev), torch.full((B, l), NAN, device=dev),
            torch.full((B, l), -1, dtype=torch.int32, device=dev))


@pytest.mark.parametrize('setting', list(SETTINGS))
@pytest.mark.parametrize('nrep', [2, 3, 4])
def test_map_sampler_token_by_token(gpu_device, nrep, setting):
    """token (b, t) equals cfg_sample_rows with that token's four weights as the row's.  The draw key holds t, so the per-request launch runs on the
    same logits (the same l, stage and seeds) once per t with the weights of column t, and column t of its outputs is compared"""
    dev, B, l, stage = gpu_device, 2, 8, 5
    lg, coef = map_inputs(nrep, dev)
    k = torch.tensor(SETTINGS[setting][0], dtype=torch.int32, device=dev)
    p = torch.tensor(SETTINGS[setting][1], device=dev)
    s = torch.tensor([11, 2 ** 63 - 3], dtype=torch.int64, device=dev)
    got = outputs(B, l, dev)
    ops.cfg_sample_map(lg, B, nrep, l, V, coef, k, p, s, stage, 1, got[0], None, *got[1:])
    assert int(got[0].min()) >= 0 and int(got[0].max()) < V
    for t in range(l):
        ref = outputs(B, l, dev)
        ops.cfg_sample_rows(lg, B, nrep, l, V, coef[:, t].contiguous(), k, p, s, stage, 1, *ref)
        for name, x, y in zip(('idx', 'combined', 'margin', 'kept'), got, ref):
            assert same_bits(x[:, t].contiguous(), y[:, t].contiguous()), (name, t)
    if setting == 'top-k':
        assert 1 < int(got[3][0].max()) <= 900 and 1 < int(got[3][1].max()) <= 50
    # forced tokens follow cvar_cfg_sample_edit's contract; NaN logits at those tokens change nothing
    g = torch.Generator().manual_seed(nrep)
    ids = torch.randint(0, V, (B, l), generator=g)
    hit = torch.rand(B, l, generator=g) < 0.5
    hit[:, 0], hit[:, -1] = torch.tensor([True, False]), torch.tensor([False, True])
    wide = torch.full((B, l + 3), 12345, dtype=torch.int32)
    wide[:, 2:2 + l] = torch.where(hit, ids, torch.full_like(ids, -1)).int()
    forced, h = wide.to(dev)[:, 2:2 + l], hit.to(dev)

    def run(logits):
        out = outputs(B, l, dev)
        ops.cfg_sample_map(logits, B, nrep, l, V, coef, k, p, s, stage, 1, out[0], forced, *out[1:])
        return out
    f = run(lg)
    assert torch.equal(f[0][h], ids.to(dev).int()[h]) and torch.equal(f[0][~h], got[0][~h])
    assert same_bits(f[1][~h], got[1][~h]) and same_bits(f[2][~h], got[2][~h]) and torch.equal(f[3][~h], got[3][~h])
    assert bool((f[3][h] == 0).all()) and bool((f[2][h] == float('inf')).all()) and bool(torch.isnan(f[1][h]).all())
    poisoned = lg.clone()
    poisoned.view(nrep, B, l, V)[:, h] = NAN
    for name, x, y in zip(('idx', 'combined', 'margin', 'kept'), run(poisoned), f):
        assert same_bits(x, y), name


@pytest.mark.parametrize('nrep', [2, 3, 4])
def test_score_map_token_by_token(gpu_device, nrep):
    dev, B, l = gpu_device, 2, 8
    lg, coef = map_inputs(nrep, dev)
    tgt = torch.randint(0, V, (B, l), generator=torch.Generator().manual_seed(nrep)).int()
    tgt[1, 2] = -1                                                  # a token without a target
    tgt = tgt.to(dev)

    def outs():
        return (torch.full((B, l, V), NAN, device=dev), torch.full((B, l), NAN, device=dev), torch.full((B, l), NAN, device=dev),
                torch.full((B, l), -7, dtype=torch.int32, device=dev), torch.full((B, l), -7, dtype=torch.int32, device=dev))
    got = outs()
    ops.score_map(lg, B, nrep, l, V, coef, tgt, *got)
    for t in range(l):
        ref = outs()
        ops.score_rows(lg, B, nrep, l, V, coef[:, t].contiguous(), tgt, *ref)
        for name, x, y in zip(('combined', 'logprob', 'entropy', 'rank', 'argmax'), got, ref):
            assert same_bits(x[:, t].contiguous(), y[:, t].contiguous()), (name, t)
    assert int(got[3][1, 2]) == -1 and float(got[1][1, 2]) == 0.0 and bool((got[1] <= 0).all())


# ------------------------------------------------------------------------------------------------------------- 5. - 11. end to end
MODES = {'bf16': (BF16, None, None), 'fp32': (F32, None, None), 'kv8': (BF16, None, 'fp8'), 'fp8': (BF16, 'fp8', None)}
_MODELS = {}


def model(kind, mode, dev, pns=PN):
    """built once per (kind, mode, scale list): depth 2, width 128, the tiny VQVAE, deterministic_plan=True (bits are compared across row counts)"""
    key = (kind, mode, pns[-1])
    if key not in _MODELS:
        dtype, gp, kvp = MODES[mode]
        vae = models.build_vae(ch=32, compute_dtype=dtype, v_patch_nums=pns).to(dev)
        kw = dict(depth=2, embed_dim=128, num_heads=2, patch_nums=pns, compute_dtype=dtype, cond_drop_rate=0.0, deterministic_plan=True, gemm_precision=gp,
                  kv_precision=kvp)
        m = models.VAR(vae, **kw) if kind == 'var' else models.ControlVAR(vae, mask_factor=2, multi_cond=True, **kw)
        _MODELS[key] = (vae, m.to(dev).eval())
    return _MODELS[key]


B = 3
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
OTHER = torch.tensor([7, 8, 9])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only


def trace_ids(m):
    return [x.clone() for x in m.last_trace['idx']]


def split_maps(K=2, S=16, n=B):
    """K vertical bands, one label each"""
    band = torch.clamp(torch.arange(S) * K // S, max=K - 1)
    return (band[None, None, None, :] == torch.arange(K)[None, :, None, None]).float().expand(n, K, S, S).contiguous()


def call(m, kind, labels, **kw):
    return m.region_infer_cfg(B, labels, **kw) if kind == 'var' else m.region_infer_cfg(B, labels, TYPES, **kw)


@pytest.mark.parametrize('kind', ['control', 'var'])
def test_one_label_uniform_is_the_per_request_joint_call(gpu_device, kind):
    vae, m = model(kind, 'bf16', gpu_device)
    want = m.autoregressive_infer_cfg(B, LABELS, _trace=True, **ROWS) if kind == 'var' else m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    ref = trace_ids(m)
    got = call(m, kind, LABELS[:, None], regions=torch.ones(B, 1, 16, 16), trace=True, **ROWS)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), si
    assert torch.equal(got, want)
    assert got.shape == ((B, 3, 256, 256) if kind == 'var' else (B, 3, 512, 256))


def test_zero_weight_is_absence(gpu_device):
    """label 0 owns every cell, label 1 weighs 0 everywhere: the middle term is 0 * l1, and the run is the K = 1 run with label 0 - whatever label 1 is"""
    vae, m = model('control', 'fp32', gpu_device)
    want = call(m, 'control', LABELS[:, None], regions=torch.ones(B, 1, 16, 16), trace=True, **ROWS)
    ref = trace_ids(m)
    maps = torch.cat([torch.full((B, 1, 16, 16), 2.5), torch.zeros(B, 1, 16, 16)], dim=1)
    for second in (OTHER, LABELS.flip(0)):
        got = call(m, 'control', torch.stack([LABELS, second], dim=1), regions=maps, trace=True, **ROWS)
        for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
            assert torch.equal(x, y), si
        assert torch.equal(got, want)
        assert bool((m.last_trace['coef'][:, :, 1] == 0).all())
    # ... and at K = 3 (nrep = 4 rows fed one drawn id row): labels 1 and 2 weigh 0
    maps3 = torch.cat([maps, torch.zeros(B, 1, 16, 16)], dim=1)
    got = call(m, 'control', torch.stack([LABELS, OTHER, LABELS.flip(0)], dim=1), regions=maps3, trace=True, **ROWS)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), si
    assert torch.equal(got, want)
    assert bool((m.last_trace['coef'][:, :, 1:3] == 0).all())


def test_locality_of_a_left_right_split(gpu_device):
    """at the last scale every bin is one latent cell, hence pure: a token on label k's side is combined from label k's row and the unconditional
    row with the K = 1 weights of the last stage, [1 + t, -t]"""
    vae, m = model('control', 'fp32', gpu_device)
    call(m, 'control', torch.stack([LABELS, OTHER], dim=1), regions=split_maps(), trace=True, **ROWS)
    tr = m.last_trace
    rows = tr['rows'][-1].cpu().numpy().reshape(3, B, -1, V)         # [label 0 ; label 1 ; unconditional]
    comb = tr['logits'][-1].cpu().numpy()
    one = models._request_table(B, ROWS['cfg'], 0, 0.0, 0, False, V, len(PN)).coef[-1].numpy()
    left = (torch.arange(16) < 8)[None, :].expand(16, 16).reshape(-1)
    side = torch.cat([left, left]).numpy()                             # both halves read the same maps
    for k, cols in ((0, side), (1, ~side)):
        want = combine_f32(rows[[k, 2]], one, V)
        assert np.array_equal(comb[:, cols], want[:, cols]), k
    assert not np.array_equal(comb[:, side], combine_f32(rows[[1, 2]], one, V)[:, side])
    # and at the first scale the one bin is half and half: both labels weigh in
    assert bool((tr['coef'][:, 0, :2] == 0.5).all())


@pytest.fixture(scope='module')
def src(gpu_device):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = model('control', 'fp32', gpu_device)[0]
    return (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))


def border(n=B, S=16, w=3):
    keep = torch.ones(n, S, S, dtype=torch.bool)
    keep[:, w:S - w, w:S - w] = False
    return keep


def test_kept_tokens_carry_the_source_ids_at_every_scale(gpu_device, src):
    vae, m = model('control', 'bf16', gpu_device)
    keep = border()
    call(m, 'control', torch.stack([LABELS, OTHER], dim=1), regions=split_maps(), src_img=src[1], keep_img=keep, src_ctrl=src[0], keep_ctrl=True, trace=True,
         **ROWS)
    produced, forced = trace_ids(m), m.last_trace['forced'].cpu().long()
    o = 0
    for si, pn in enumerate(PN):
        n = pn * pn
        kept = models.edit_keep_cells(keep, pn)
        assert torch.equal(produced[si][:, :n].cpu().long(), src[0][si].cpu().long())                      # the control half is kept whole
        got, want = produced[si][:, n:].cpu().long(), src[1][si].cpu().long()
        assert torch.equal(got[kept], want[kept]), si
        assert torch.equal(forced[:, o + n:o + 2 * n], torch.where(kept, want, torch.full_like(want, -1))), si
        o += 2 * n
    free = forced < 0
    assert int(free.sum()) > 0 and int((~free).sum()) > 0


def test_a_graph_replay_equals_the_eager_call_and_takes_new_maps_without_recapture(gpu_device, src):
    vae, m = model('control', 'bf16', gpu_device)
    graph = m.graphed_region_generator(B, 2, top_k=600, top_p=0.8)
    g = torch.Generator().manual_seed(3)
    reqs = [dict(labels=torch.stack([LABELS, OTHER], dim=1), regions=split_maps(), cfg=[1.5, 4.0, 3.0], g_seed=[11, 12, 2 ** 64 - 5]),
            dict(labels=torch.stack([OTHER, LABELS.flip(0)], dim=1), regions=torch.rand(B, 2, 16, 16, generator=g) + 0.01, cfg=[[2.0, 0.5], [1.0, 1.0], [0.0, 6.0]],
                 strength=torch.rand(B, 16, 16, generator=g) * 2, g_seed=[5, 6, 7], top_k=[1, 0, 300], top_p=[0.0, 0.7, 0.0],
                 src_img=src[1], keep_img=border(), src_ctrl=src[0], keep_ctrl=None)]
    outs = []
    for r in reqs:
        r = dict(r)
        labels = r.pop('labels')
        a = graph(labels, TYPES, **r)
        eager = m.region_infer_cfg(B, labels, TYPES, trace=True, **{'top_k': 600, 'top_p': 0.8, **r})
        assert torch.equal(a, eager)
        assert same_bits(graph.coef(), m.last_trace['coef'])
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    coef = graph.coef()
    bad = split_maps(); bad[1, :, 4, 4] = 0.0
    with pytest.raises(ValueError, match='a latent cell whose weights sum to 0'):
        graph(reqs[0]['labels'], TYPES, regions=bad)
    with pytest.raises(ValueError, match=r'label_B: expected shape \(3, 2\)'):
        graph(LABELS[:, None], TYPES, regions=torch.ones(B, 1, 16, 16))
    assert same_bits(graph.coef(), coef)                              # a refused run leaves the graph as it was
    r = dict(reqs[0]); labels = r.pop('labels')
    assert torch.equal(graph(labels, TYPES, **r), outs[0])


def test_logprobs_are_those_of_the_traced_combined_logits(gpu_device):
    vae, m = model('control', 'fp32', gpu_device)
    kw = dict(regions=split_maps(3), cfg=[[1.5, 2.0, 0.5], [4.0, 4.0, 4.0], [0.0, 3.0, 1.0]], strength=torch.rand(B, 16, 16, generator=torch.Generator().manual_seed(1)),
              g_seed=ROWS['g_seed'], top_k=ROWS['top_k'], top_p=ROWS['top_p'], trace=True)
    labels = torch.stack([LABELS, OTHER, LABELS.flip(0)], dim=1)
    want = call(m, 'control', labels, **kw)
    ref = trace_ids(m)
    got, sc = call(m, 'control', labels, logprobs=True, **kw)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), si
    assert torch.equal(got, want)
    x = np.concatenate([t.cpu().numpy() for t in m.last_trace['logits']], axis=1)
    tgt = np.concatenate([t[:B].cpu().numpy() for t in m.last_trace['idx']], axis=1)
    ref_lp, ref_ent, ref_rank, ref_am = score_ref(x, tgt)
    assert np.array_equal(sc.rank.cpu().numpy(), ref_rank) and np.array_equal(sc.argmax.cpu().numpy(), ref_am)
    a, b = within_bounds(sc.logprob.cpu().numpy(), sc.entropy.cpu().numpy(), ref_lp, ref_ent)
    print(f'[region logprobs] worst logprob error {a:.3f} of its bound, worst entropy error {b:.3f} of its bound')
    assert a <= 1.0 and b <= 1.0
    assert bool(sc.sampled.all()) and tuple(sc.logprob.shape) == (B, m.cfg.pyramid.L)


def check_smoke(m, img, shape, L):
    assert tuple(img.shape) == shape and bool(torch.isfinite(img).all()) and float(img.min()) >= 0.0 and float(img.max()) <= 1.0
    ids = torch.cat(trace_ids(m), dim=1)
    assert tuple(ids.shape) == (B, L) and int(ids.min()) >= 0 and int(ids.max()) < V


@pytest.mark.parametrize('mode', ['bf16', 'kv8', 'fp8'])
def test_smoke_per_precision(gpu_device, mode):
    vae, m = model('control', mode, gpu_device)
    img = call(m, 'control', torch.stack([LABELS, OTHER], dim=1), regions=split_maps(), trace=True, **ROWS)
    check_smoke(m, img, (B, 3, 512, 256), m.cfg.pyramid.L)


def test_smoke_with_a_per_request_adapter(gpu_device):
    dev = gpu_device
    vae = models.build_vae(ch=32, compute_dtype=BF16).to(dev)
    m = models.ControlVAR(vae, depth=2, embed_dim=128, num_heads=2, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=BF16, cond_drop_rate=0.0,
                          deterministic_plan=True).to(dev).eval()
    mods, sds = dict(m.named_modules()), []
    for k, r in enumerate((16, 5)):
        g, sd = torch.Generator().manual_seed(40 + k), {}
        for t in lora.target_names(m):
            out_f, in_f = mods[t]._parameters['weight'].shape
            sd[f'{t}.lora_A.default.weight'] = (torch.rand(r, in_f, generator=g) * 2 - 1) / in_f ** 0.5
            sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * 0.2
        sds.append(sd)
    lora.attach_adapters(m, sds)
    labels = torch.stack([LABELS, OTHER, LABELS.flip(0)], dim=1)
    base = call(m, 'control', labels, regions=split_maps(3), adapter=-1, trace=True, **ROWS)
    check_smoke(m, base, (B, 3, 512, 256), m.cfg.pyramid.L)
    img = call(m, 'control', labels, regions=split_maps(3), adapter=[0, -1, 1], trace=True, **ROWS)
    check_smoke(m, img, (B, 3, 512, 256), m.cfg.pyramid.L)
    assert torch.equal(img[1], base[1]) and not torch.equal(img[0], base[0])          # row 1 rides on the base model


def test_smoke_at_512(gpu_device):
    vae, m = model('var', 'bf16', gpu_device, PN512)
    img = call(m, 'var', torch.stack([LABELS, OTHER], dim=1), regions=split_maps(2, 32), strength=torch.full((B, 32, 32), 1.5), trace=True, **ROWS)
    check_smoke(m, img, (B, 3, 512, 512), m.cfg.pyramid.L)
