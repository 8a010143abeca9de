"""The launch record of the two layer walks of controlvar_amd/models.py - the transformer pass (ControlVAR._ada + _blocks_and_head) in every
gemm_precision / kv_precision / adapter-bank mode, and the VQVAE encoder / decoder walk in every encoder_precision - against the recording in
tests/golden/block_pass_launches.json, written by tests/golden/make_block_pass_launches.py on the GPU at commit 5aaa918 ("Add kv_precision='fp8'"):
the commit BEFORE the three per-mode copies of the pass and the _hp_* copy of the encoder were folded into one walk each.

tests/test_gpu_generation_launches.py (whose Recorder, run_length and ids_digest are used here) runs fp32 models only, so it never enters the
bf16x3, fp8, kv8, bf16, unfused-adaLN or high-precision-encoder branches; this module does.  Per case the fixture holds the number of launches, the
run-length-encoded op names, the sha256 of the full text, the sha256 of the produced bytes (int32 token ids under ids_sha256; fp32 logits / ada rows /
residual streams / f / images under bytes_sha256) and peak_bytes, the peak of torch.cuda.max_memory_allocated() over the case above what was allocated
when it began (after reset_peak_memory_stats()).  The first four must be equal - same launches and same bytes on the same hardware and compiler is an
equality, not a tolerance - and the peak must not lie above the recorded one.  max_memory_allocated() counts the cached blocks the allocator hands
out, an unsplit remainder included, so the same code reads differently depending on what the process ran before (the decoder case behind the whole
suite: 65 521 664 against 65 441 280 in a fresh process; two fresh processes at the recording's commit agreed on all 51 figures).  The peak is
therefore asserted where it is reproducible: the last test runs the recording script in a child process, as the fixture was made, and compares every
case's peak there; the per-case tests in this process check the four equalities and print their peak.

Every model is built and packed before anything is recorded.  What a case would otherwise find cached from an earlier one (the K/V arena of the stream,
the lazily built compute-dtype matrices of an x3 / fp8 model) is dropped in its setup, outside the record, so that a case allocates the same whether it
runs alone or behind the others.

Transformer pass cases call _ada and then _blocks_and_head twice into one arena of Lmax = 8 + l: l = 8 at q_off = 0, then l at q_off = 8, so that no
pass reads cache rows that were never written.  The shapes are R = 4, l = 16 (a small fused pass), and the two sides of models.FUSE_LN_BELOW:
M = FUSE_LN_BELOW - 1 rows, the last pass whose proj / fc2 also write the next adaLN rows, and M = FUSE_LN_BELOW, the first at which adaLN is its own
launch (4096 = 16 x 256 and 4097 = 17 x 241 with the value at the recording; no kernel refused either shape).

When a later change alters launches ON PURPOSE, regenerate the fixture on the GPU with that change applied,

    python tests/golden/make_block_pass_launches.py [--dump DIR]

and review the difference between the two commits' dumps.

Models: depth 2, 128 channels, 2 heads, ch=32 VQVAE, synthetic weights, fixed seeds."""
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
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN
from controlvar_amd.synth import synth_images
from test_gpu_generation_launches import Recorder, ids_digest, run_length

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'block_pass_launches.json')
B, V, C = 2, 4096, 128
F32, BF16 = torch.float32, torch.bfloat16
LAB, TY = torch.tensor([3, 977]), torch.tensor([1, 2])
LAB2, TY2 = torch.tensor([500, 0]), torch.tensor([3, 0])
L0 = 8                                       # rows per sequence of the first pass of a case


def _rows_by_len(M, least):
    """M = R * l with the smallest R >= least"""
    R = next(r for r in range(least, M + 1) if M % r == 0)
    return R, M // R


SHAPES = {'small': (4, 16), 'fused': _rows_by_len(models.FUSE_LN_BELOW - 1, 16), 'unfused': _rows_by_len(models.FUSE_LN_BELOW, 16)}


def bytes_digest(tensors):
    if not tensors:
        return None
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to(F32).cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------- the models
# kind -> (compute dtype, gemm_precision, kv_precision); 'bank' = bf16 with a two-adapter bank; 'cos_*' = build_var(..., cos_attn=True), a plain VAR
MODES = {'f32': (F32, None, None), 'bf16': (BF16, None, None), 'bank': (BF16, None, None), 'x3': (F32, 'bf16x3', None), 'fp8': (BF16, 'fp8', None),
         'kv8': (BF16, None, 'fp8'), 'fp8kv8': (BF16, 'fp8', 'fp8')}
COS = {'cos_bf16': MODES['bf16'], 'cos_kv8': MODES['kv8'], 'cos_fp8': MODES['fp8'], 'cos_fp8kv8': MODES['fp8kv8'], 'cos_x3': MODES['x3']}
VAES = {'vae_bf16': (BF16, None), 'vae_bf16_x3': (BF16, 'bf16x3'), 'vae_bf16_fp32': (BF16, 'fp32'), 'vae_f32': (F32, None)}
_MODELS = {}


def _vae(kind, dev):
    if kind not in _MODELS:
        T, ep = VAES[kind]
        v = models.build_vae(ch=32, compute_dtype=T, encoder_precision=ep).to(dev)
        v._pack(check=True)
        _MODELS[kind] = v
    return _MODELS[kind]


def model(kind, dev):
    """built once per kind, weights packed (so that no case's record depends on which case came first)"""
    if kind in VAES:
        return _vae(kind, dev)
    if kind not in _MODELS:
        T, gp, kv = (MODES if kind in MODES else COS)[kind]
        vae = _vae('vae_bf16' if T == BF16 else 'vae_f32', dev)
        if kind in COS:
            m = models.build_var(vae, depth=2, cos_attn=True, compute_dtype=T, cond_drop_rate=0.0, gemm_precision=gp, kv_precision=kv)
            assert m.cfg.uses_cos_attn
        else:
            m = models.ControlVAR(vae, depth=2, embed_dim=C, num_heads=2, patch_nums=PN, mask_factor=2, multi_cond=True, compute_dtype=T,
                                  cond_drop_rate=0.0, gemm_precision=gp, kv_precision=kv)
        m = m.to(dev).eval()
        if kind == 'bank':
            from test_gpu_adapter_batch import adapter_state
            lora.attach_adapters(m, [adapter_state(m, 16, 40 + k) for k in range(2)])
        m._pack(check=True)
        if kind == 'bank':
            lora.bank_pack(m)
        _MODELS[kind] = m
    return _MODELS[kind]


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _cold(m, repack=False):
    """outside the record: drop what an earlier case may have left cached on the model"""
    m._arena = None
    if repack:
        m._packed = None
        m._pack(check=True)
    return m


# ------------------------------------------------------------------------------------------------------------- the cases: (setup(dev) -> state, run(state) -> (ids, floats))
def _pass(kind, shape, det=False):
    R, l = SHAPES[shape]

    def setup(dev):
        m = _cold(model(kind, dev))
        ad = None
        if kind == 'bank':
            ad = (lora.bank_pack(m), torch.tensor([(0, -1, 1)[r % 3] for r in range(R)], dtype=torch.int32, device=dev))
        return m, ad, _randn(1, R * L0, C).to(dev), _randn(2, R * l, C).to(dev), _randn(3, R, C).to(dev)

    def run(st):
        m, ad, x0, x1, cond = st
        m.deterministic_plan = det
        try:
            arena = m._get_arena(R, L0 + l, m.kv_precision)
            ada = m._ada(cond, R, ad=ad)
            a = m._blocks_and_head(x0, ada, R, L0, 0, L0 + l, arena, ad=ad)
            b = m._blocks_and_head(x1, ada, R, l, L0, L0 + l, arena, ad=ad)
        finally:
            m.deterministic_plan = False
        return [], [ada, a, x0, b, x1]
    return setup, run


def _forward(kind, mask_first=True):
    def setup(dev):
        m = _cold(model(kind, dev), repack=True)            # the lazy compute-dtype matrices are built inside the case, every time
        py = m.cfg.pyramid
        return m, _randn(4, B, len(py.code_positions()) - py.first_l, m.cfg.cvae).to(dev)

    def run(st):
        m, tok = st
        with torch.no_grad():
            return [], [m(LAB, tok, cond_type=TY, mask_first=mask_first)]
    return setup, run


def _greedy(kind):
    def setup(dev):
        return _cold(model(kind, dev))

    def run(m):
        kw = {} if isinstance(m, models.VAR) else dict(cond_type=TY)
        if kind == 'bank':
            kw['adapter'] = [0, 1]
        m.autoregressive_infer_cfg(B, LAB, g_seed=5, cfg=2.0, top_k=1, _trace=True, **kw)
        return list(m.last_trace['idx']), []
    return setup, run


def _graph(kind):
    def setup(dev):
        return _cold(model(kind, dev))

    def run(m):
        g = m.graphed_generator(B, cfg=2.0, top_k=600, top_p=0.9)
        a = g(LAB, TY, g_seed=3).clone()
        b = g(LAB2, TY2, g_seed=4).clone()
        return [], [a, b]
    return setup, run


def _encode(kind):
    def setup(dev):
        return model(kind, dev), synth_images(B, 16 * PN[-1], seed=43).to(dev)

    def run(st):
        vae, img = st
        with torch.no_grad():
            vae._pack(check=True)
            f = vae._encode_f(img)
            return vae.img_to_idxBl(img), [f]
    return setup, run


def _decode(kind, same_shape):
    def setup(dev):
        g = torch.Generator().manual_seed(27)
        return model(kind, dev), [torch.randint(0, V, (B, pn * pn), generator=g).to(dev) for pn in PN]

    def run(st):
        vae, ids = st
        return [], list(vae.idxBl_to_img(ids, same_shape=same_shape))
    return setup, run


CASES = {}
for _k in MODES:
    for _s in SHAPES:
        CASES[f'pass_{_k}_{_s}'] = _pass(_k, _s)
    CASES[f'generate_{_k}'] = _greedy(_k)
for _k in ('bf16', 'x3', 'fp8'):
    CASES[f'pass_{_k}_small_deterministic_plan'] = _pass(_k, 'small', det=True)
for _k in COS:
    CASES[f'pass_{_k}_small'] = _pass(_k, 'small')
for _k in ('x3', 'fp8', 'kv8'):
    CASES[f'forward_{_k}'] = _forward(_k)
    CASES[f'forward_{_k}_image_first'] = _forward(_k, mask_first=False)
CASES['graph_fp8kv8'] = _graph('fp8kv8')
for _k in VAES:
    CASES[f'encode_{_k}'] = _encode(_k)
for _k in ('vae_bf16', 'vae_f32'):
    CASES[f'decode_{_k}_same_shape'] = _decode(_k, True)
    CASES[f'decode_{_k}_own_shapes'] = _decode(_k, False)          # HW = pn * pn: the padded-key branch of _attnblock where that is no multiple of the 16-byte chunk


def record_case(name, dev):
    """-> (fixture entry, full text)"""
    for kind in (*MODES, *COS, *VAES):          # every model exists before anything is recorded
        model(kind, dev)
    random.seed(1234)
    torch.manual_seed(1234)
    setup, run = CASES[name]
    state = setup(dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    with Recorder() as rec:
        ids, floats = run(state)
        torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    text = '\n'.join(rec.lines) + '\n'
    return dict(launches=len(rec.lines), ops=run_length(rec.names), text_sha256=hashlib.sha256(text.encode()).hexdigest(), ids_sha256=ids_digest(ids),
                bytes_sha256=bytes_digest(floats), peak_bytes=peak), text


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_walk_issues_the_recorded_launches_on_the_recorded_bytes(gpu_device, name):
    assert os.path.exists(FIXTURE), 'record it with tests/golden/make_block_pass_launches.py'
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
    assert got['ids_sha256'] == want['ids_sha256'], (name, 'token ids')
    assert got['bytes_sha256'] == want['bytes_sha256'], (name, 'produced values')


def test_peak_memory_of_every_case_in_a_fresh_process_is_not_above_the_recorded_one(gpu_device, tmp_path):
    """the recording script itself, in a child process: every case's peak of max_memory_allocated() as the fixture's was taken - a fresh allocator, the
    cases in the script's order.  (One child for all cases: a few seconds of start-up, then what the cases above take.)"""
    out = tmp_path / 'block_pass_launches.json'
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, 'make_block_pass_launches.py'), '--out', str(out)], capture_output=True, text=True, timeout=600)
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
