"""The launch record of the training engine (controlvar_amd/train.py, TrainEngine.forward_backward) in full and LoRA mode against the recording in
tests/golden/train_launches.json, written by tests/golden/make_train_launches.py on the GPU at commit 216107e ("Support widths above 2048"): the
commit BEFORE the two buffer plans, the two forward block bodies and the two backward walks of the engine were folded into one each.

Recorder and run_length come from tests/test_gpu_generation_launches.py (no case produces token ids), bytes_digest from tests/test_gpu_block_pass_launches.py; what
those modules say about the text of a record holds here.  A stub reducer sits on the engine: its ready(idx) appends a ``ready(idx)`` line to the same
record, which pins the points at which the backward releases a gradient bucket.

Per case the fixture holds the number of launches (the ready lines included), the run-length-encoded op names, the sha256 of the full text, the
sha256 of the produced bytes and peak_bytes.  The produced bytes are, after every step of the case: the loss, loss_tok, logits, every grads() tensor
in sorted key order, then each bucket's raw contents (the buckets cover elements that no key views: the k-bias third of b_qkv, padding).  The first
four must be equal.  peak_bytes is an upper bound, asserted in a child process that runs the recording script, for the reason the block-pass module's
docstring gives; the per-case tests print theirs.  `paths` names the branch the weight gradients and the word-embedding gradient took (read off the op
names); the recording script asserts it against what the case's shapes and dtype say.

Every model is built, packed and given its Trainer (for Trainer.tokenize) before anything is recorded; a case tokenises in its setup, outside the
record, and runs on a fresh TrainEngine, so that it allocates the same whether it runs alone or behind the others.  The transition case changes its
model (add_lora, merge_lora) and therefore builds its own.

A case is one plain forward_backward at B = 1 and then one with accumulate=True at B = 2, in one record: M = 1360 tokens take the one-slice
weight-gradient GEMM, M = 2720 the token split, and the gradient buffers must survive the change of batch size.  The transition case is three plain
steps at B = 1 on one engine: full model, the same model after add_lora, and after merge_lora - the mode switch of TrainEngine._setup both ways.

When a later change alters launches ON PURPOSE, regenerate the fixture on the GPU with that change applied,

    python tests/golden/make_train_launches.py [--dump DIR]

and review the difference between the two commits' dumps.

Models: depth 2, 128 channels (hid = 512), 2 heads, ch=32 VQVAE, synthetic weights, fixed seeds, cond_drop_rate=0."""
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest
import torch

from conftest import GOLDEN
from controlvar_amd import lora, models
from controlvar_amd import train as T
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN
from controlvar_amd.synth import synth_images
from test_gpu_block_pass_launches import bytes_digest
from test_gpu_generation_launches import Recorder, run_length

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'train_launches.json')
F32, BF16 = torch.float32, torch.bfloat16
KW = dict(peak_lr=2e-3, weight_decay=0.05, sche='lin0', warmup_it=2, max_it=50, clip=2.0, drop_path=False)      # test_gpu_grad_accum.KW
CLS, TYPES = torch.tensor([17, 403, 5]), torch.tensor([2, 0, 1])
STEPS = ((0, 1, False), (1, 3, True))       # (first sample, end, accumulate): B = 1 plain, then B = 2 added to it
DROP_SEED = 77


# ------------------------------------------------------------------------------------------------------------- the models
# kind -> (compute dtype, builder keywords, LoRA (r, dropout) or None); 'var*' / 'cos*' = build_var, 'sa' = ControlVAR(aln=-1) as tests/test_gpu_train.py builds it
KINDS = {'joint_f32': (F32, {}, None), 'joint_bf16': (BF16, {}, None), 'var_bf16': (BF16, {}, None), 'cos_bf16': (BF16, dict(cos_attn=True), None),
         'shared_aln_f32': (F32, dict(shared_aln=True), None), 'shared_aln_bf16': (BF16, dict(shared_aln=True), None),
         'type_pos_f32': (F32, dict(type_pos=True), None), 'separator_bf16': (BF16, dict(separator=True), None), 'sa_f32': (F32, {}, None),
         'lora_joint_bf16': (BF16, {}, (16, 0.0)), 'lora_joint_f32': (F32, {}, (5, 0.3)), 'lora_var_bf16': (BF16, {}, (16, 0.0)),
         'lora_cos_bf16': (BF16, dict(cos_attn=True), (16, 0.0))}
_MODELS = {}


def _vae(dtype, dev):
    if dtype not in _MODELS:
        v = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
        v._pack(check=True)
        _MODELS[dtype] = v
    return _MODELS[dtype]


def _add_lora(m, r, p):
    """add_lora with the B matrices randomised as test_gpu_grad_accum._models does (B = 0 would make every dA zero)"""
    lora.add_lora(m, r=r, dropout=p, seed=1)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for _, (_, Bm) in lora.adapters(m).items():
            Bm.copy_(torch.randn(Bm.shape, generator=g) * 0.05)


def _build(kind, dev):
    dtype, kw, lo = KINDS[kind]
    vae = _vae(dtype, dev)
    if 'var' in kind or 'cos' in kind:         # cos-attention is a plain VAR's option: a ControlVAR has it at depth 30 only (spec.VarConfig.uses_cos_attn)
        m = models.build_var(vae, depth=2, compute_dtype=dtype, cond_drop_rate=0.0, **kw)
    elif kind == 'sa_f32':
        m = models.ControlVAR(vae, depth=2, embed_dim=128, num_heads=2, mask_factor=2, multi_cond=True, patch_nums=PN, compute_dtype=dtype,
                              cond_drop_rate=0.0, aln=-1, layer_scale=0.1)
        assert m.cfg.sa_block
    else:
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0, **kw)
    m = m.to(dev).eval()
    assert (m.cfg.C, m.cfg.depth, round(m.cfg.C * m.cfg.mlp_ratio)) == (128, 2, 512) and m.cfg.uses_cos_attn == ('cos' in kind)
    if lo is not None:
        _add_lora(m, *lo)
    m._pack(check=True)
    m._pack(check=True, base=True)
    return vae, m, None if isinstance(m, models.VAR) else T.Trainer(m, vae, **KW)


def model(kind, dev):
    """(vae, model, its Trainer - None for a plain VAR), built once per kind, weights packed (so that no case's record depends on which case came first)"""
    if kind not in _MODELS:
        _MODELS[kind] = _build(kind, dev)
    return _MODELS[kind]


def _tokens(vae, m, tr, dev, mask_first=True):
    """(cls, x, types, labels) of three samples: Trainer.tokenize on synthetic images; a plain VAR has no control half"""
    images, masks = synth_images(3, 256, seed=6).to(dev), synth_images(3, 256, seed=7).to(dev)
    if isinstance(m, models.VAR):
        idx = vae.img_to_idxBl(images)
        return CLS, torch.cat(vae.idxBl_to_h(idx), 1), None, torch.cat(idx, 1)
    x, labels = tr.tokenize(images, masks, mask_first)
    return CLS, x, TYPES, labels


class _Ready:
    """the stub reducer: the release points of the gradient buckets become lines of the record"""

    def __init__(self):
        self.rec = None

    def ready(self, idx):
        self.rec.names.append('ready')
        self.rec.lines.append(f'ready({idx})')


def _sl(t, a, b):
    return None if t is None else t[a:b]


def _produced(eng, loss):
    g = eng.grads()
    return [t.detach().float().cpu() for t in (loss, eng.loss_tok, eng.logits, *(g[k] for k in sorted(g)), *eng.buckets)]


# ------------------------------------------------------------------------------------------------------------- the cases: (setup(dev) -> state, run(state, rec) -> floats)
def _steps(kind, train=False, drop_path=False, mask_first=True, ignore=False):
    def setup(dev):
        vae, m, tr = model(kind, dev)
        masks = None
        batch = _tokens(vae, m, tr, dev, mask_first)
        if ignore:          # a different mask (and density) per sample, as test_gpu_grad_accum.test_ignore_mask_per_micro_batch draws it
            g = torch.Generator().manual_seed(11)
            masks = (torch.rand(3, batch[3].shape[1], generator=g) < torch.tensor([0.3, 0.5, 0.9]).view(3, 1)).float().to(dev)
        eng = T.TrainEngine(m, drop_path=drop_path, reducer=_Ready())
        return m, eng, batch, masks

    def run(st, rec):
        m, eng, (cls, x, types, labels), masks = st
        eng.reducer.rec = rec
        m.train(train)
        out = []
        try:
            for a, b, acc in STEPS:
                loss, _ = eng.forward_backward(cls[a:b], x[a:b], _sl(types, a, b), labels[a:b], _sl(masks, a, b), drop_seed=DROP_SEED,
                                               mask_first=mask_first, accumulate=acc)
                out += _produced(eng, loss)
        finally:
            m.eval()
        return out
    return setup, run


def _transition():
    def setup(dev):
        vae, m, tr = _build('joint_bf16', dev)           # its own model: the case changes it
        return m, T.TrainEngine(m, drop_path=False, reducer=_Ready()), _tokens(vae, m, tr, dev)

    def run(st, rec):
        m, eng, (cls, x, types, labels) = st
        eng.reducer.rec = rec
        out = []
        for change in (None, lambda: _add_lora(m, 16, 0.0), lambda: lora.merge_lora(m)):
            if change is not None:
                change()
            loss, _ = eng.forward_backward(cls[:1], x[:1], types[:1], labels[:1], drop_seed=DROP_SEED)
            out += _produced(eng, loss)
        return out
    return setup, run


CASES = {'full_' + k: _steps(k) for k in KINDS if not k.startswith('lora_')}
CASES.update({
    'full_joint_bf16_drop_path': _steps('joint_bf16', train=True, drop_path=True),           # gate_scale is set
    'full_joint_bf16_image_first': _steps('joint_bf16', mask_first=False),
    'full_joint_f32_ignore_mask': _steps('joint_f32', ignore=True),
    'lora_joint_bf16': _steps('lora_joint_bf16'),
    'lora_joint_f32_r5_dropout': _steps('lora_joint_f32', train=True, drop_path=True),      # adapter dropout 0.3 and DropPath, both seeded by drop_seed
    'lora_var_bf16': _steps('lora_var_bf16'),
    'lora_cos_bf16': _steps('lora_cos_bf16'),
    'transition_bf16_full_lora_merged': _transition(),
})


def paths_of(names):
    """which branch the weight gradients (TrainEngine._wgrad) and the word-embedding gradient took, from the op names of a record"""
    full = 'scatter_add_rows' in names                 # the embedding tail runs in the full model only
    return dict(wgrad=None if not full else 'gemm_tn' if 'gemm_tn' in names else 'transposes',
                word_embed=None if not full else 'one_pass' if 'wordembed_grad' in names else 'per_sample')


def record_case(name, dev):
    """-> (fixture entry, full text)"""
    for kind in KINDS:          # every model exists before anything is recorded
        model(kind, dev)
    random.seed(1234)
    torch.manual_seed(1234)
    setup, run = CASES[name]
    state = setup(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    with Recorder() as rec:
        floats = run(state, rec)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    text = '\n'.join(rec.lines) + '\n'
    return dict(launches=len(rec.lines), ops=run_length(rec.names), text_sha256=hashlib.sha256(text.encode()).hexdigest(), bytes_sha256=bytes_digest(floats),
                paths=paths_of(rec.names), peak_bytes=peak), text


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_training_step_issues_the_recorded_launches_on_the_recorded_bytes(gpu_device, name):
    assert os.path.exists(FIXTURE), 'record it with tests/golden/make_train_launches.py'
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got, _ = record_case(name, gpu_device)
    flat = lambda rle: [n for n, c in rle for _ in range(c)]
    a, b = flat(got['ops']), flat(want['ops'])
    if a != b:
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f'[launches] {name}: op names first differ at position {at}: issued {a[at:at + 3]}, recorded {b[at:at + 3]} ({len(a)} against {len(b)} launches)')
    print(f'[launches] {name}: {got["launches"]} launches, peak in this process {got["peak_bytes"]} bytes (recorded in a fresh one: {want["peak_bytes"]})')
    assert got['launches'] == want['launches'], (name, got['launches'], want['launches'])
    assert got['ops'] == want['ops'], name
    assert got['text_sha256'] == want['text_sha256'], (name, 'same op names, different arguments: diff the --dump texts')
    assert got['bytes_sha256'] == want['bytes_sha256'], (name, 'produced values')
    assert got['paths'] == want['paths'], name


def test_peak_memory_of_every_case_in_a_fresh_process_is_not_above_the_recorded_one(gpu_device, tmp_path):
    """the recording script itself, in a child process: every case's peak of max_memory_allocated() as the fixture's was taken - a fresh allocator, the
    cases in the script's order.  A buffer plan that allocates the full model's set for a LoRA engine shows here first."""
    out = tmp_path / 'train_launches.json'
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_train_launches.py'), '--out', str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(FIXTURE) as f:
        want = json.load(f)
    with open(out) as f:
        got = json.load(f)
    assert sorted(got) == sorted(want) == sorted(CASES)
    above = {}
    for name in sorted(want):
        print(f'[launches] {name}: peak {got[name]["peak_bytes"]} bytes, recorded {want[name]["peak_bytes"]}')
        assert {k: v for k, v in got[name].items() if k != 'peak_bytes'} == {k: v for k, v in want[name].items() if k != 'peak_bytes'}, name
        if got[name]['peak_bytes'] > want[name]['peak_bytes']:
            above[name] = (got[name]['peak_bytes'], want[name]['peak_bytes'])
    assert not above, above
