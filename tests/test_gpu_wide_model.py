"""Models wider than 2048 channels on MI355X: depth 2, embed_dim 2304, 36 heads - the width of d36 - in every mode the library offers.

Two models on the ch32 VQVAE the other model tests use: a joint ControlVAR on DEFAULT_PATCH_NUMS (weight seed WSEED) and a VAR(shared_aln=True) on
PATCH_NUMS_512, the d36 configuration at depth 2.  No published d36 weights are loaded anywhere: every weight is synthetic (controlvar_amd.synth).

fp32 mode: greedy ids of autoregressive_infer_cfg and conditional_infer_cfg(c_mask=...) against the CPU oracle (oracle/var_ref.py) under the margin rule of
tests/test_gpu_parity.py - a flip is tolerated only where the oracle's own top-1 / top-2 margin is below 2e-3 (conftest.ids_parity, strict=False) - with a cap
that keeps the rule from hiding a failure: the oracle alone leaves at most 1 % of the ids below that margin.  WSEED = 6 was chosen on the CPU among the seeds
0 .. 7 (smallest margin of the two-way run 2.1e-4 ... 2.2e-3, at most 5 of 2 720 ids below 2e-3; seed 6 is the widest, 2.19e-3: none lies below 2e-3) and the cap is asserted
here on the oracle's margins.  forward() logits against var_ref.forward_logits at that file's 2e-3.

Every other mode makes the assertion its own test file makes at its own width: teacher-forced along the oracle's ids, per-scale CFG logits against the FP32
MODE's on the same ids relative to max|logit| of the scale, at the constants of those files (restated below with their citations); the properties - a request
does not depend on its batch, a graph replay equals the eager call, adapters mixed in a batch, an edit that keeps nothing, logprobs=True - bit for bit.
One Trainer.step in fp32 and bf16 against oracle/train_ref.loss_and_grads at the bounds of tests/test_gpu_train.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import ids_parity, record  # noqa: E402
from controlvar_amd import lora, models  # noqa: E402
from controlvar_amd import train as T  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, PATCH_NUMS_512 as PN512, VaeConfig, VarConfig, phi_index_map  # noqa: E402
from controlvar_amd.synth import synth_images, synth_vae_state, synth_var_state  # noqa: E402
from oracle import train_ref, var_ref  # noqa: E402
from oracle.vqvae_ref import MSQuant  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
C, H, DEPTH = 2304, 36, 2
WSEED = 6
CFG = VarConfig(depth=DEPTH, embed_dim=C, num_heads=H)                                                      # the joint ControlVAR
CFG512 = VarConfig(depth=DEPTH, embed_dim=C, num_heads=H, mask_factor=1, control=False, multi_cond=False, shared_aln=True, patch_nums=PN512)
MARGIN_TOL = 2e-3                    # tests/test_gpu_parity.py: the margin every fp32 generation test there labels its flips with
MARGIN_CAP = 0.01                    # at most this share of the oracle's ids may lie below MARGIN_TOL
FP32_LOGIT_BOUND = 2e-3              # tests/test_gpu_parity.py::test_forward_logits_fp32
BF16_REL_BOUND = 2 * 4.1e-3          # tests/test_gpu_configs.py:30: twice the measured bf16 distance, relative to max|logit| of the scale
X3_REL_BOUND = 2 * 3.1e-5            # tests/test_gpu_x3_generation.py:41
FP8_REL_BOUND = 2 * 6.8e-2           # tests/test_gpu_fp8_generation.py:35
KV8_REL_BOUND = 2 * 1.44e-2          # tests/test_gpu_kv8_generation.py:37
KV8_FP8_REL_BOUND = 2 * 6.3e-2       # tests/test_gpu_kv8_generation.py:38
LABELS2, TYPES2 = torch.tensor([3, 7]), torch.tensor([0, 1])
B3 = 3
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only

_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def make_joint(dtype, dev, vae_dtype=None, **kw):
    vae = models.build_vae(ch=32, compute_dtype=vae_dtype or dtype).to(dev)
    m = models.ControlVAR(vae, depth=DEPTH, embed_dim=C, num_heads=H, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                          init_seed=WSEED, cond_drop_rate=0.0, **kw)
    return vae, m.to(dev).eval()


def make_var512(dtype, dev):
    vae = models.build_vae(ch=32, compute_dtype=dtype, v_patch_nums=PN512).to(dev)
    m = models.VAR(vae, depth=DEPTH, embed_dim=C, num_heads=H, patch_nums=PN512, shared_aln=True, compute_dtype=dtype, init_seed=WSEED, cond_drop_rate=0.0)
    return vae, m.to(dev).eval()


@pytest.fixture(scope='module')
def joint32(gpu_device):
    return make_joint(F32, gpu_device)


@pytest.fixture(scope='module')
def joint16(gpu_device):
    return make_joint(BF16, gpu_device)


def msq():
    return MSQuant(synth_vae_state(VaeConfig(ch=32)), PN, phi_index_map(len(PN)))


def margins_of(logits):
    t2 = torch.cat(logits, dim=1).topk(2, dim=-1).values
    return (t2[..., 0] - t2[..., 1]).numpy()


def oracle_two_way():
    """-> ids (2, 1360), margins (2, 1360) of the oracle's greedy two-way generation; computed once"""
    def run():
        tr = {}
        with torch.no_grad():
            var_ref.generate(synth_var_state(CFG, WSEED), CFG, msq(), 2, LABELS2, 4.0, top_k=1, cond_type=TYPES2, trace=tr)
        return torch.cat(tr['idx'], dim=1), margins_of(tr['logits'])
    return cached('two_way', run)


def c_mask_ids():
    g = torch.Generator().manual_seed(77)
    return [torch.randint(0, 4096, (2, p * p), generator=g) for p in PN]


def oracle_four_way():
    def run():
        tr = {}
        with torch.no_grad():
            var_ref.generate(synth_var_state(CFG, WSEED), CFG, msq(), 2, torch.tensor([5, 6]), (4.0, 3.0, 2.0), top_k=1, cond_type=torch.tensor([2, 3]),
                             c_mask=c_mask_ids(), four_way=True, trace=tr)
        return torch.cat(tr['idx'], dim=1), margins_of(tr['logits'])
    return cached('four_way', run)


def forced_ids():
    ids, _ = oracle_two_way()
    out, o = [], 0
    for p in PN:
        out.append(ids[:, o:o + 2 * p * p].contiguous())
        o += 2 * p * p
    return out


def forced_run(m):
    img = m.autoregressive_infer_cfg(2, LABELS2, g_seed=0, cfg=4.0, top_k=1, top_p=0.0, cond_type=TYPES2, _trace=True, _force_idx=forced_ids())
    tr = m.last_trace
    return img.cpu(), [x.float().cpu().clone() for x in tr['logits']], [x.cpu().long().clone() for x in tr['idx']]


def rel_distance(lg, lg32):
    return max(float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(lg, lg32))


def cap_holds(margin, what):
    share = float((margin < MARGIN_TOL).mean())
    print(f'[wide] {what}: {int((margin < MARGIN_TOL).sum())} of {margin.size} oracle margins below {MARGIN_TOL:.0e} (smallest {float(margin.min()):.3e})')
    assert share <= MARGIN_CAP, (what, share)


# ================================================================================================ fp32 mode against the CPU oracle
def test_fp32_greedy_generation_against_the_oracle(gpu_device, joint32):
    ids_ref, margin = oracle_two_way()
    cap_holds(margin, f'two-way generation, weight seed {WSEED}')
    vae, m = joint32
    img = m.autoregressive_infer_cfg(2, LABELS2, g_seed=0, cfg=4.0, top_k=1, top_p=0.0, cond_type=TYPES2, _trace=True)
    assert img.shape == (2, 3, 512, 256) and torch.isfinite(img).all()
    ids = torch.cat(m.last_trace['idx'], dim=1).cpu()
    ids_parity(ids, ids_ref.numpy(), margin, MARGIN_TOL, 'wide d2 C2304 greedy generation', strict=False)


def test_fp32_conditional_generation_against_the_oracle(gpu_device, joint32):
    ids_ref, margin = oracle_four_way()
    cap_holds(margin, f'four-way generation, weight seed {WSEED}')
    vae, m = joint32
    img = m.conditional_infer_cfg(2, torch.tensor([5, 6]), g_seed=0, cfg=(4.0, 3.0, 2.0), top_k=1, cond_type=torch.tensor([2, 3]), _trace=True,
                                  c_mask=c_mask_ids())
    assert torch.isfinite(img).all()
    ids = torch.cat(m.last_trace['idx'], dim=1).cpu()
    assert ids.shape == ids_ref.shape == (8, 1360)                  # rows [branch][sample]: the combined logits of sample b serve rows b, 2 + b, 4 + b, 6 + b
    ids_parity(ids, ids_ref.numpy(), np.tile(margin, (4, 1)), MARGIN_TOL, 'wide d2 C2304 conditional generation (c_mask)', strict=False)


@pytest.mark.parametrize('which', ['joint', 'var512'])
def test_fp32_forward_logits_against_the_oracle(gpu_device, joint32, which):
    if which == 'joint':
        cfg, (vae, m), types = CFG, joint32, TYPES2
    else:
        cfg, (vae, m), types = CFG512, cached('var512_f32', lambda: make_var512(F32, gpu_device)), None
    py = cfg.pyramid
    x = torch.randn(2, py.L - py.first_l, 32, generator=torch.Generator().manual_seed(21))
    with torch.no_grad():
        ref = var_ref.forward_logits(synth_var_state(cfg, WSEED), cfg, LABELS2, x, types)
        got = m(LABELS2, x.to(gpu_device), types, True).cpu()               # what the oracle gets: no condition types for the plain VAR
    assert got.shape == ref.shape == (2, py.L, 4096)
    err = float((got - ref).abs().max())
    print(f'[wide] forward {which}: max |logit - oracle| {err:.3e} (max |logit| {float(ref.abs().max()):.1f})')
    assert err < FP32_LOGIT_BOUND


# ================================================================================================ the reduced-precision modes along the oracle's trace
@pytest.fixture(scope='module')
def traces(gpu_device, joint32, joint16):
    """per mode (logits per scale, ids per scale) of the teacher-forced run along the oracle's ids; every run made once"""
    out = {'fp32': forced_run(joint32[1])}
    m32 = joint32[1]
    m32.gemm_precision = 'bf16x3'
    try:
        out['bf16x3'] = forced_run(m32)
        assert m32._pack().get('w_qkv_x3') is not None
    finally:
        m32.gemm_precision = None
    m = joint16[1]
    try:
        for mode, (gp, kv) in {'bf16': (None, None), 'bf16+kv8': (None, 'fp8'), 'fp8': ('fp8', None), 'fp8+kv8': ('fp8', 'fp8')}.items():
            m.gemm_precision, m.kv_precision = gp, kv
            out[mode] = forced_run(m)
            assert torch.isfinite(out[mode][0]).all(), mode
    finally:
        m.gemm_precision, m.kv_precision = None, None
    return out


@pytest.mark.parametrize('mode,bound', [('bf16', BF16_REL_BOUND), ('bf16x3', X3_REL_BOUND), ('fp8', FP8_REL_BOUND), ('bf16+kv8', KV8_REL_BOUND),
                                        ('fp8+kv8', KV8_FP8_REL_BOUND)])
def test_logit_distance_to_the_fp32_mode(traces, mode, bound):
    lg32 = traces['fp32'][1]
    rel = rel_distance(traces[mode][1], lg32)
    flips = sum(int((a != b).sum()) for a, b in zip(traces[mode][2], forced_ids()))
    print(f'[wide] {mode}: worst per-scale logit distance to the fp32 mode {rel:.3e} of max|logit| (bound {bound:.1e}); {flips} of 2720 greedy ids moved')
    record(f'wide C2304 {mode}', kind='wide_logits', worst_rel=rel, bound=bound, flips=flips, total=2720)
    assert rel <= bound
    if mode == 'bf16x3':
        # tests/test_gpu_x3_generation.py: a flip only where the reference's own margin is below X3_REL_BOUND * max|logit| of the scale; the same image bits
        _, margin = oracle_two_way()
        o = 0
        for si, p in enumerate(PN):
            l = 2 * p * p
            ids_parity(traces[mode][2][si], forced_ids()[si], margin[:, o:o + l], X3_REL_BOUND * float(lg32[si].abs().max()), f'wide x3 scale {si}', strict=False)
            o += l
        assert torch.equal(traces[mode][0], traces['fp32'][0])


# ================================================================================================ inherited properties at width 2304
def trace_ids(m):
    return [x.clone() for x in m.last_trace['idx']]


def test_row_b_of_a_per_request_batch_equals_the_b1_call(gpu_device, joint16):
    vae, m = joint16
    m.deterministic_plan = True
    try:
        perm = [2, 0, 1]
        rows = {k: [v[b] for b in perm] for k, v in ROWS.items()}
        img = m.autoregressive_infer_cfg(B3, LABELS[perm], cond_type=TYPES[perm], _trace=True, **rows)
        ids = torch.cat(trace_ids(m), dim=1)
        for slot, b in enumerate(perm):
            img1 = m.autoregressive_infer_cfg(1, LABELS[b:b + 1], cond_type=TYPES[b:b + 1], _trace=True, **{k: v[b] for k, v in ROWS.items()})
            assert torch.equal(torch.cat(trace_ids(m), dim=1)[0], ids[slot]), b
            assert torch.equal(img[slot:slot + 1], img1), b
    finally:
        m.deterministic_plan = False


def test_one_graph_replay_equals_the_eager_call(gpu_device, joint16):
    vae, m = joint16
    g = m.graphed_generator(B3, per_request=True)
    img = g(LABELS, TYPES, **ROWS)
    assert torch.equal(img, m.autoregressive_infer_cfg(B3, LABELS, cond_type=TYPES, **ROWS))
    del g
    v = cached('var512_bf16', lambda: make_var512(BF16, gpu_device))[1]
    kw = dict(cfg=4.0, top_k=900, top_p=0.96)
    run = v.graphed_generator(2, **kw)
    out = run(LABELS2, g_seed=3)
    assert out.shape == (2, 3, 512, 512) and torch.isfinite(out).all()
    assert torch.equal(out, v.autoregressive_infer_cfg(2, LABELS2, g_seed=3, **kw))


def adapter_state(m, r, seed, b_std=0.2):
    """tests/test_gpu_adapter_batch.py::adapter_state"""
    g = torch.Generator().manual_seed(seed)
    mods = dict(m.named_modules())
    sd = {}
    for t in lora.target_names(m):
        out_f, in_f = mods[t]._parameters['weight'].shape
        sd[f'{t}.lora_A.default.weight'] = (torch.rand(r, in_f, generator=g) * 2 - 1) / in_f ** 0.5
        sd[f'{t}.lora_B.default.weight'] = torch.randn(out_f, r, generator=g) * b_std
    return sd


def test_two_adapters_mixed_in_one_batch(gpu_device):
    """row b of the batch is the B = 1 call with that row's own adapter, bit for bit; a row on adapter -1 is the model without a bank"""
    vae, m = make_joint(BF16, gpu_device)
    vae0, base = make_joint(BF16, gpu_device)
    lora.attach_adapters(m, [adapter_state(m, r, 40 + k) for k, r in enumerate((16, 5))])
    adapter = [0, -1, 1]
    m.deterministic_plan = base.deterministic_plan = True
    img = m.autoregressive_infer_cfg(B3, LABELS, cond_type=TYPES, _trace=True, adapter=adapter, **ROWS)
    ids, logits = torch.cat(trace_ids(m), dim=1), [x.clone() for x in m.last_trace['logits']]
    assert torch.isfinite(img).all()
    for b, a in enumerate(adapter):
        one = {k: v[b] for k, v in ROWS.items()}
        img1 = m.autoregressive_infer_cfg(1, LABELS[b:b + 1], cond_type=TYPES[b:b + 1], _trace=True, adapter=[a], **one)
        assert torch.equal(torch.cat(trace_ids(m), dim=1)[0], ids[b]) and torch.equal(img[b:b + 1], img1), b
        for si, (x, y) in enumerate(zip(logits, m.last_trace['logits'])):
            assert torch.equal(x[b], y[0]), (b, si)
        img0 = base.autoregressive_infer_cfg(1, LABELS[b:b + 1], cond_type=TYPES[b:b + 1], _trace=True, **one)
        same_as_base = torch.equal(torch.cat(trace_ids(base), dim=1)[0], ids[b])
        assert same_as_base == (a < 0), (b, a)
        if a < 0:
            assert torch.equal(img[b:b + 1], img0)


def test_an_edit_that_keeps_nothing_is_the_per_request_joint_call(gpu_device, joint16):
    vae, m = joint16
    want = m.autoregressive_infer_cfg(B3, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    ref = trace_ids(m)
    src = (vae.img_to_idxBl(synth_images(B3, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B3, 256, seed=42).to(gpu_device)))
    nothing = torch.zeros(B3, 16, 16, dtype=torch.bool)
    for kw in (dict(), dict(src_img=src[1], keep_img=nothing, src_ctrl=src[0], keep_ctrl=nothing.to(gpu_device))):
        got = m.edit_infer_cfg(B3, LABELS, TYPES, trace=True, **kw, **ROWS)
        for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
            assert torch.equal(x, y), si
        assert torch.equal(got, want)
        assert bool((m.last_trace['forced'] == -1).all())


def test_logprobs_leave_ids_and_images_unchanged(gpu_device, joint16):
    vae, m = joint16
    want = m.autoregressive_infer_cfg(B3, LABELS, cond_type=TYPES, _trace=True, **ROWS)
    ref = trace_ids(m)
    img, sc = m.autoregressive_infer_cfg(B3, LABELS, cond_type=TYPES, _trace=True, logprobs=True, **ROWS)
    for si, (x, y) in enumerate(zip(trace_ids(m), ref)):
        assert torch.equal(x, y), si
    assert torch.equal(img, want)
    flat = torch.cat(ref, dim=1)
    assert torch.isfinite(sc.logprob).all() and bool((sc.rank[1] == 0).all()) and torch.equal(sc.argmax[1], flat[1])          # row 1 is the greedy row


# ================================================================================================ one Trainer.step
def train_inputs(dev):
    return synth_images(2, 256, seed=6).to(dev), synth_images(2, 256, seed=7).to(dev), torch.tensor([17, 403]), torch.tensor([2, 0])


def trainer(m, vae):
    return T.Trainer(m, vae, peak_lr=2e-3, weight_decay=0.05, weight_decay_end=0.01, sche='lin0', warmup_it=20, max_it=1000, clip=1e9, wp0=0.005, wpe=0.01,
                     drop_path=False)


def oracle_step(x, labels, cls, types):
    """loss and gradients of the fp32 oracle on the tokens of the fp32 tokenizer (both trainers below tokenize with the fp32 VQVAE); computed once"""
    return cached('train', lambda: train_ref.loss_and_grads(synth_var_state(CFG, WSEED), CFG, cls, x.float().cpu(), types, labels.cpu()))


@pytest.mark.parametrize('dtype', [F32, BF16], ids=['fp32', 'bf16'])
def test_one_trainer_step_against_the_oracle(gpu_device, dtype):
    """B = 2, DropPath off, clipping out of reach.  fp32: every tensor's gradient norm of the step's backward pass within 1e-3 max(1, norm) of the oracle's,
    then the step's loss within 2e-5 and its total gradient norm within 1e-3 (tests/test_gpu_train.py:60, :69, :142); bf16: the loss within 2e-2 of the
    oracle's on the same tokens (tests/test_gpu_res512.py:260-262).  The wide forward kernels serve forward_train; the backward is cvar_ln_modulate_bwd's
    scalar row path."""
    vae, m = make_joint(dtype, gpu_device, vae_dtype=F32)
    m.train()
    tr = trainer(m, vae)
    images, masks, cls, types = train_inputs(gpu_device)
    x, labels = tr.tokenize(images, masks, True)
    loss_r, _, grads_r = oracle_step(x, labels, cls, types)
    if dtype == F32:
        # the backward pass the step runs, tensor by tensor.  The norms are taken on the host, as tests/test_gpu_train.py takes them: torch's device norm
        # of an fp32 tensor of >= 2^24 elements (fc1, fc2, ada_lin at this width) was measured 2e-3 off the host's on the same values
        tr.engine.forward_backward(cls, x, types, labels, mask_first=True)
        grads = tr.engine.grads()
        assert set(grads_r) <= set(grads)
        for n, gr in grads_r.items():
            got, ref = grads[n].cpu().norm().item(), gr.norm().item()
            assert abs(got - ref) < 1e-3 * max(1.0, ref), (n, got, ref)
    out = tr.step(images, masks, cls, types, mask_first=True)
    assert torch.isfinite(out['loss']).all() and torch.isfinite(out['grad_norm']).all()
    print(f'[wide] Trainer.step {dtype}: loss {out["loss"].item():.6f} oracle {loss_r.item():.6f}')
    if dtype == BF16:
        assert abs(out['loss'].item() - loss_r.item()) < 2e-2, (out['loss'].item(), loss_r.item())
        return
    assert abs(out['loss'].item() - loss_r.item()) < 2e-5, (out['loss'].item(), loss_r.item())
    total = float(torch.sqrt(sum(gr.double().pow(2).sum() for gr in grads_r.values())))
    assert abs(out['grad_norm'].item() - total) < 1e-3 * total, (out['grad_norm'].item(), total)            # tests/test_gpu_train.py:142
