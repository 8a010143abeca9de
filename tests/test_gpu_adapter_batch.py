"""Per-request LoRA adapters end to end on the MI355X (lora.attach_adapters, ``adapter=`` of the generation calls).

Models: tests/test_gpu_lora.py's CFGS (control, var, cos, wide), three adapters of ranks 16 / 5 / 16 with random non-zero B (std 0.2).
One invariant carries most of the file: under deterministic_plan=True, row b of a batch is the B = 1 call with that row's own adapter and
sampling parameters, bit for bit, whatever slot it rides in; a row on adapter -1 is the model without a bank.  The values themselves are
pinned by the CPU oracle on merged weights (W + s B A per adapter), teacher-forced along the oracle's own ids."""
import pytest
import torch

from controlvar_amd import lora, models
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, VaeConfig, VarConfig, phi_index_map
from controlvar_amd.synth import synth_images, synth_vae_state
from oracle import var_ref
from oracle.vqvae_ref import MSQuant

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
CFGS = {'control': VarConfig(depth=2), 'var': VarConfig(depth=2, mask_factor=1, control=False, multi_cond=False),
        'cos': VarConfig(depth=30, embed_dim=128, num_heads=2),
        'wide': VarConfig(depth=2, embed_dim=320, num_heads=5)}      # C, 4C and 6C all end in a partial 512-column slab
RANKS = (16, 5, 16)
BF16_REL_BOUND = 2 * 4.1e-3          # tests/test_gpu_configs.py: twice the measured bf16 distance between GEMM plans, relative to max|logit| of the scale

# six requests: adapters mixed with the base model, sampled beside greedy
ADAPTER = [0, -1, 2, 1, 0, 2]
LABELS, TYPES = torch.tensor([1, 500, 999, 7, 3, 250]), torch.tensor([0, 3, 1, 2, 1, 0])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5, 14, 15, 16], cfg=[1.5, 4.0, 3.0, 0.5, 2.0, 4.0], top_k=[900, 1, 0, 50, 1, 900], top_p=[0.96, 0.0, 0.5, 1.0, 0.0, 0.9])

# Oracle test: the largest distance (absolute, over all scales and rows) of the merged-weights generation of the code before this change
# (tests/test_gpu_lora.py::_merged_copy: add_lora + load_lora + merge_lora, fp32 mode, default plan) to the CPU oracle's combined logits on
# the inputs of test_bank_rows_match_the_cpu_oracle_on_merged_weights, teacher-forced along the oracle's ids.  Measured on one MI355X with
# merged_distance() below; the bank path never enters the figure.
# Per request: adapter 0 1.106e-04, adapter 1 1.221e-04, adapter 2 9.537e-05, base model 5.722e-05.
# For comparison the bank path shows 1.431e-04 on the same batch, and none of
# the oracle's 5440 top-1 margins lies below the bound (1 below twice the bound).
MERGED_DISTANCE = 1.2207e-04
ORACLE_BOUND = 2 * MERGED_DISTANCE

_MODELS = {}


def make(cfg, dtype, dev, seed=0):
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    if cfg.control:
        m = models.ControlVAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, mask_factor=2, multi_cond=True, patch_nums=PN,
                              compute_dtype=dtype, cond_drop_rate=0.0, init_seed=seed)
    else:
        m = models.VAR(vae, depth=cfg.depth, embed_dim=cfg.C, num_heads=cfg.H, patch_nums=PN, compute_dtype=dtype, cond_drop_rate=0.0, init_seed=seed)
    return vae, m.to(dev).eval()


def adapter_state(m, r, seed, b_std=0.2):
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    sd = {}
    for t in lora.target_names(m):
        out_f, in_f = mods[t]._parameters['weight'].shape
        sd[f'{t}.lora_A.default.weight'] = (torch.rand(r, in_f, generator=g) * 2 - 1) / in_f ** 0.5
        sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * b_std
    return sd


def banked(kind, dtype, dev):
    """(vae, model with the three-adapter bank, the same model's weights without a bank), built once per (kind, dtype)"""
    key = (kind, dtype)
    if key not in _MODELS:
        vae, m = make(CFGS[kind], dtype, dev)
        _, base = make(CFGS[kind], dtype, dev)
        lora.attach_adapters(m, [adapter_state(m, r, 40 + k) for k, r in enumerate(RANKS)])
        _MODELS[key] = (vae, m, base)
    return _MODELS[key]


def gen(m, B, labels, types, **kw):
    if isinstance(m, models.VAR):
        return m.autoregressive_infer_cfg(B, labels, _trace=True, **kw)
    return m.autoregressive_infer_cfg(B, labels, cond_type=types, _trace=True, **kw)


def traced(m):
    tr = m.last_trace
    return ([x.clone() for x in tr['idx']], [x.clone() for x in tr['logits']], [x.clone() for x in tr['margin']])


def row_params(b):
    return {k: v[b] for k, v in ROWS.items()}


def assert_row_equals_single(batch, b, single, img, img1, what):
    for si, (x, y) in enumerate(zip(batch[1], single[1])):
        assert torch.equal(x[b], y[0]), (what, 'combined logits', b, si, float((x[b] - y[0]).abs().max()))
    for si, (x, y) in enumerate(zip(batch[0], single[0])):
        assert torch.equal(x[b], y[0]), (what, 'ids', b, si)
    assert torch.equal(img[b], img1[0]), (what, 'image', b)


class deterministic:
    def __init__(self, *ms):
        self.ms = ms

    def __enter__(self):
        for m in self.ms:
            m.deterministic_plan = True

    def __exit__(self, *a):
        for m in self.ms:
            m.deterministic_plan = False


# ------------------------------------------------------------------------------------------------------------- 1. adapters change the output
@pytest.mark.parametrize('kind', ['control', 'var', 'cos', 'wide'])
def test_adapters_change_the_output_and_minus_one_is_the_base_model(gpu_device, kind):
    vae, m, base = banked(kind, BF16, gpu_device)
    B = len(ADAPTER)
    with deterministic(m, base):
        gen(base, B, LABELS, TYPES, **ROWS)
        want = torch.cat(traced(base)[0], dim=1)
        img = gen(m, B, LABELS, TYPES, adapter=ADAPTER, **ROWS)
        got = torch.cat(traced(m)[0], dim=1)
    assert torch.isfinite(img).all()
    for b, a in enumerate(ADAPTER):
        if a < 0:
            assert torch.equal(got[b], want[b]), b
        else:
            assert not torch.equal(got[b], want[b]), b
    # two requests that differ in nothing but the adapter differ in their ids
    with deterministic(m):
        gen(m, 2, LABELS[:1].repeat(2), TYPES[:1].repeat(2), g_seed=5, cfg=3.0, top_k=1, adapter=[0, 2])
    ids = torch.cat(traced(m)[0], dim=1)
    assert not torch.equal(ids[0], ids[1])


# ------------------------------------------------------------------------------------------------------------- 2. row independence
@pytest.mark.parametrize('kind,dtype', [('control', BF16), ('var', BF16), ('cos', BF16), ('wide', BF16), ('control', F32), ('wide', F32)],
                         ids=lambda v: v if isinstance(v, str) else str(v)[6:])
def test_a_row_equals_its_batch_one_call_whatever_slot_it_rides_in(gpu_device, kind, dtype):
    vae, m, _ = banked(kind, dtype, gpu_device)
    B = len(ADAPTER)
    with deterministic(m):
        singles = []
        for b in range(B):
            img1 = gen(m, 1, LABELS[b:b + 1], TYPES[b:b + 1], adapter=[ADAPTER[b]], **row_params(b))
            singles.append((traced(m), img1))
        for perm in (list(range(B)), [4, 2, 0, 5, 1, 3]):
            p = torch.tensor(perm)
            img = gen(m, B, LABELS[p], TYPES[p], adapter=[ADAPTER[i] for i in perm], **{k: [v[i] for i in perm] for k, v in ROWS.items()})
            batch = traced(m)
            for slot, b in enumerate(perm):
                assert_row_equals_single(batch, slot, singles[b][0], img, singles[b][1], (kind, perm))
        # one int is broadcast
        img = gen(m, 2, LABELS[:2], TYPES[:2], adapter=1, g_seed=[14, 14], cfg=[0.5, 0.5], top_k=[50, 50], top_p=[1.0, 1.0])
        batch = traced(m)
        img1 = gen(m, 1, LABELS[1:2], TYPES[1:2], adapter=[1], g_seed=14, cfg=0.5, top_k=50, top_p=1.0)
        assert_row_equals_single(batch, 1, traced(m), img, img1, 'broadcast')


# ------------------------------------------------------------------------------------------------------------- 3. base rows
@pytest.mark.parametrize('kind,dtype', [('control', BF16), ('wide', BF16), ('var', F32)], ids=lambda v: v if isinstance(v, str) else str(v)[6:])
def test_all_minus_one_equals_the_call_without_adapter(gpu_device, kind, dtype):
    """deterministic plan: the extra K columns are exact zeros added to an unsliced, fixed-order sum - torch.equal.  Default plan: the K
    slicing of the wider call may differ, so the logits (teacher-forced along the plain call's ids) stay within BF16_REL_BOUND of max|logit|
    of the scale, and greedy ids agree wherever the plain call's top-1 margin exceeds that bound"""
    vae, m, _ = banked(kind, dtype, gpu_device)
    B = len(ADAPTER)
    with deterministic(m):
        want = gen(m, B, LABELS, TYPES, **ROWS)
        ref = traced(m)
        got = gen(m, B, LABELS, TYPES, adapter=-1, **ROWS)
        new = traced(m)
    for part in range(3):
        for si, (x, y) in enumerate(zip(new[part], ref[part])):
            assert torch.equal(x, y), (part, si)
    assert torch.equal(got, want)
    if dtype != BF16:
        return
    greedy = dict(g_seed=list(range(B)), cfg=[4.0] * B, top_k=[1] * B, top_p=[0.0] * B)
    gen(m, B, LABELS, TYPES, **greedy)
    ref = traced(m)
    gen(m, B, LABELS, TYPES, adapter=-1, _force_idx=[i.clone() for i in ref[0]], **greedy)
    new = traced(m)
    worst = 0.0
    for si in range(len(PN)):
        amax = float(ref[1][si].abs().max())
        d = float((new[1][si] - ref[1][si]).abs().max())
        worst = max(worst, d / amax)
        assert d <= BF16_REL_BOUND * amax, (si, d, amax)
        flip = new[0][si] != ref[0][si]
        assert not bool((flip & (ref[2][si] > BF16_REL_BOUND * amax)).any()), si
    print(f'[{kind}] adapter=-1 against no adapter under the default plan: largest logit distance {worst:.2e} of max|logit|')


# ------------------------------------------------------------------------------------------------------------- 4. the CPU oracle on merged weights
ORACLE_LABELS, ORACLE_TYPES, ORACLE_ADAPTER = torch.tensor([3, 7, 980, 421]), torch.tensor([0, 1, 3, 2]), [0, 1, 2, -1]


def cpu_state(m):
    return {k: v.detach().cpu() for k, v in m.state_dict().items()}


def oracle_traces(m):
    """per request of the oracle batch: the CPU oracle's trace of a B = 1 greedy cfg-4 generation on the base weights merged with the
    request's adapter (the base weights for -1)"""
    cfg = CFGS['control']
    msq = MSQuant(synth_vae_state(VaeConfig(ch=32)), PN, phi_index_map(10))
    sd = cpu_state(m)
    out = []
    for b, a in enumerate(ORACLE_ADAPTER):
        sd_eff = sd if a < 0 else lora.merged_adapter_state(sd, m._adapter_bank, a)
        trace = {}
        with torch.no_grad():
            var_ref.generate(sd_eff, cfg, msq, 1, ORACLE_LABELS[b:b + 1], 4.0, top_k=1, cond_type=ORACLE_TYPES[b:b + 1], trace=trace)
        out.append(trace)
    return out


def distance_to_oracle(tr, traces, rows):
    """(largest |combined logits - oracle|, tokens compared, tokens whose id differs though the oracle's margin exceeds `bound`) per bound fn"""
    worst, per_scale = 0.0, []
    for si in range(len(PN)):
        want = torch.cat([traces[b]['logits'][si] for b in rows])
        d = (tr[1][si].cpu() - want).abs().amax(dim=-1)
        worst = max(worst, float(d.max()))
        per_scale.append((want, d))
    return worst, per_scale


def merged_distance(dev):
    """the figure behind ORACLE_BOUND: the merged-weights generation (add_lora + load_lora + merge_lora: no line of the bank path) against
    the same oracle traces, request by request"""
    vae, m, _ = banked('control', F32, dev)
    traces = oracle_traces(m)
    worst = 0.0
    for b, a in enumerate(ORACLE_ADAPTER):
        _, m2 = make(CFGS['control'], F32, dev)
        if a >= 0:
            lora.add_lora(m2, r=RANKS[a], alpha=32, dropout=0.0)
            lora.load_lora(m2, adapter_state(m, RANKS[a], 40 + a))
            lora.merge_lora(m2)
        m2.eval()
        m2.autoregressive_infer_cfg(1, ORACLE_LABELS[b:b + 1], g_seed=0, cfg=4.0, top_k=1, cond_type=ORACLE_TYPES[b:b + 1], _trace=True,
                                    _force_idx=[t.clone() for t in traces[b]['idx']])
        d, _ = distance_to_oracle(traced(m2), traces, [b])
        print(f'merged weights, request {b} (adapter {a}): largest distance to the oracle {d:.3e}')
        worst = max(worst, d)
    return worst, traces


def test_bank_rows_match_the_cpu_oracle_on_merged_weights(gpu_device):
    """fp32 mode, greedy, cfg 4, one batch of four requests on adapters 0 / 1 / 2 / -1, teacher-forced along the oracle's ids (so that one flip
    cannot cascade).  The combined logits of every scale lie within ORACLE_BOUND of the oracle's on W + s B A of the row's adapter, and the
    ids equal the oracle's wherever the oracle's top-1 margin exceeds that bound; at most 1 % of the tokens fall under the exclusion.
    ORACLE_BOUND = 2 x MERGED_DISTANCE, the distance of the merged-weights path to the same traces (see MERGED_DISTANCE above)."""
    vae, m, _ = banked('control', F32, gpu_device)
    traces = oracle_traces(m)
    B = len(ORACLE_ADAPTER)
    force = [torch.cat([traces[b]['idx'][si] for b in range(B)]) for si in range(len(PN))]
    m.autoregressive_infer_cfg(B, ORACLE_LABELS, g_seed=0, cfg=4.0, top_k=[1] * B, cond_type=ORACLE_TYPES, _trace=True, _force_idx=force, adapter=ORACLE_ADAPTER)
    tr = traced(m)
    worst, per_scale = distance_to_oracle(tr, traces, range(B))
    excluded = total = 0
    for si, (want, d) in enumerate(per_scale):
        top2 = want.topk(2, dim=-1).values
        margin = top2[..., 0] - top2[..., 1]
        sure = margin > ORACLE_BOUND
        excluded += int((~sure).sum())
        total += sure.numel()
        flip = tr[0][si].cpu().long() != force[si].long()
        print(f'scale {si}: largest distance {float(d.max()):.3e}, {int(flip.sum())} ids differ, {int((~sure).sum())} of {sure.numel()} tokens under the margin')
        assert float(d.max()) <= ORACLE_BOUND, (si, float(d.max()))
        assert not bool((flip & sure).any()), si
    print(f'bank against the oracle: largest distance {worst:.3e} (bound {ORACLE_BOUND:.3e}), {excluded} of {total} tokens excluded')
    assert excluded <= 0.01 * total, (excluded, total)


# ------------------------------------------------------------------------------------------------------------- 5. graphs
def three(perm):
    p = torch.tensor(perm)
    return LABELS[p], TYPES[p], {k: [v[i] for i in perm] for k, v in ROWS.items()}


def test_one_graph_serves_every_mix_of_adapters(gpu_device):
    vae, m, _ = banked('control', BF16, gpu_device)
    B = 3
    labels, types, rows = three([0, 1, 2])
    graph = m.graphed_generator(B, cfg=2.5, top_k=600, top_p=0.8, per_request=True, adapters=True)
    outs = []
    for ad in ([0, -1, 2], [1, 1, 0], 2, None, [-1, -1, -1]):
        kw = {} if ad is None else dict(adapter=ad)
        a = graph(labels, types, **rows, **kw)
        assert torch.equal(a, m.autoregressive_infer_cfg(B, labels, cond_type=types, **rows, **kw)), ad
        outs.append(a)
    assert not torch.equal(outs[0], outs[1]) and torch.equal(outs[3], outs[4])
    # a refused run leaves every static buffer as it was
    with pytest.raises(ValueError, match='id out of range'):
        graph(LABELS[3:6], TYPES[3:6], **three([3, 4, 5])[2], adapter=[0, 3, 1])
    with pytest.raises(ValueError, match='one per batch row'):
        graph(LABELS[3:6], TYPES[3:6], **rows, adapter=[0, 1])
    a = graph(labels, types, **rows, adapter=[2, 0, 1])
    assert torch.equal(a, m.autoregressive_infer_cfg(B, labels, cond_type=types, **rows, adapter=[2, 0, 1]))
    plain = m.graphed_generator(B, cfg=2.5, top_k=600, top_p=0.8, per_request=True)
    with pytest.raises(TypeError, match='adapters=True'):
        plain(labels, types, **rows, adapter=[0, 0, 0])
    assert torch.equal(plain(labels, types, **rows), outs[3])


def test_the_edit_graph_takes_adapters(gpu_device):
    vae, m, _ = banked('control', BF16, gpu_device)
    B = 3
    labels, types, rows = three([0, 1, 2])
    src = (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))
    keep = torch.ones(B, 16, 16, dtype=torch.bool)
    keep[:, 4:12, 4:12] = False
    graph = m.graphed_edit_generator(B, source='ids', adapters=True)
    outs = []
    for ad in ([0, -1, 2], [1, 2, 2]):
        mk = dict(src_img=src[1], keep_img=keep, src_ctrl=src[0], keep_ctrl=True)
        a = graph(labels, types, **mk, **rows, adapter=ad)
        assert torch.equal(a, m.edit_infer_cfg(B, labels, types, **mk, **rows, adapter=ad)), ad
        outs.append(a)
    assert not torch.equal(outs[0], outs[1])
    with pytest.raises(ValueError, match='id out of range'):
        graph(labels, types, **mk, **rows, adapter=[0, 0, 5])
    a = graph(labels, types, **mk, **rows, adapter=[0, -1, 2])
    assert torch.equal(a, outs[0])
    plain = m.graphed_edit_generator(B, source='ids')
    with pytest.raises(TypeError, match='adapters=True'):
        plain(labels, types, **mk, **rows, adapter=0)


# ------------------------------------------------------------------------------------------------------------- 6. composition
def test_everything_kept_reproduces_the_sources_under_any_adapter(gpu_device):
    vae, m, _ = banked('control', F32, gpu_device)
    B = 3
    labels, types, rows = three([0, 1, 2])
    src = (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))
    img = m.edit_infer_cfg(B, labels, types, src_img=src[1], keep_img=True, src_ctrl=src[0], keep_ctrl=True, adapter=[0, -1, 2], **rows)
    H = img.shape[-1]
    for half, ids in enumerate(src):                            # control on top, RGB below
        want = vae.idxBl_to_img(ids, same_shape=True, last_one=True) * 0.5 + 0.5
        assert torch.equal(img[:, :, half * H:(half + 1) * H], want), half


def test_conditional_generation_rows_equal_their_batch_one_calls(gpu_device):
    vae, m, _ = banked('control', BF16, gpu_device)
    B = 3
    labels, types = LABELS[:B], TYPES[:B]
    ids = vae.img_to_idxBl(synth_images(B, 256, seed=31).to(gpu_device))
    triples = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (4.0, 0.5, 2.5)]
    ks, ps, seeds, ad = [1, 900, 0], [0.0, 0.96, 0.9], [21, 22, 23], [2, -1, 1]
    with deterministic(m):
        img = m.conditional_infer_cfg(B, labels, g_seed=seeds, cfg=triples, top_k=ks, top_p=ps, cond_type=types, c_mask=ids, _trace=True, adapter=ad)
        tr = m.last_trace
        batch = ([x.view(4, B, -1)[0].clone() for x in tr['idx']], [x.clone() for x in tr['logits']], None)
        for b in range(B):
            img1 = m.conditional_infer_cfg(1, labels[b:b + 1], g_seed=seeds[b], cfg=triples[b], top_k=ks[b], top_p=ps[b], cond_type=types[b:b + 1],
                                           c_mask=[i[b:b + 1] for i in ids], _trace=True, adapter=[ad[b]])
            tr = m.last_trace
            single = ([x.view(4, 1, -1)[0].clone() for x in tr['idx']], [x.clone() for x in tr['logits']], None)
            assert_row_equals_single(batch, b, single, img, img1, 'conditional')
        plain = m.conditional_infer_cfg(1, labels[:1], g_seed=seeds[0], cfg=triples[0], top_k=ks[0], top_p=ps[0], cond_type=types[:1], c_mask=[i[:1] for i in ids])
        assert not torch.equal(plain, img[:1])                 # row 0 rides on adapter 2
