"""The launch record of the generation host path (controlvar_amd/models.py between the public API and _blocks_and_head): every entry point
must issue the same launches with the same arguments in the same order, on the same token ids, as the recording in
tests/golden/generation_launches.json - written by tests/golden/make_generation_launches.py on the GPU at the commit BEFORE the host path was
untangled into one sampling step, one per-request runner and one graph runner.

The recorder wraps every function defined in controlvar_amd.ops for the duration of a case and passes the call through.  Only calls made from
outside ops are logged (a depth counter), each as one canonical text line: the op name, then every argument bound to its parameter name -
numbers by repr, sequences element by element, None, and for a tensor its shape, strides, dtype, storage offset, device type and the index
of the first earlier tensor argument of the same call that shares its storage (``residual=x`` beside ``out=x``).  Addresses are not recorded;
the split-K workspace bookkeeping of ops, whose arguments are stream handles, is logged by name only.

Per case the fixture holds the number of launches, the run-length-encoded op names, the sha256 of the full text and the sha256 of the int32
token ids the case produced (last_trace['idx'], run.ids() / run.forced(), TokenScores.rank / .argmax), where it produces any.

When a later change alters launches ON PURPOSE, regenerate the fixture on the GPU with that change applied,

    python tests/golden/make_generation_launches.py [--dump DIR]

and review the difference: ``--dump DIR`` writes the full text of every case, so that the dumps of the two commits can be diffed.

Models: depth 2, 128 channels, ch=32 VQVAE, fp32, synthetic weights, B = 2, python's `random` seeded per case."""
import functools
import hashlib
import inspect
import json
import os
import random

import pytest
import torch

from conftest import GOLDEN
from controlvar_amd import lora, models, ops
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN
from controlvar_amd.synth import synth_images

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, 'generation_launches.json')
B, V = 2, 4096
LAB, TY = torch.tensor([3, 977]), torch.tensor([1, 2])
LAB2, TY2 = torch.tensor([500, 0]), torch.tensor([3, 0])
ROWS = dict(g_seed=[11, 2 ** 64 - 5], cfg=[1.5, 4.0], top_k=[900, 1], top_p=[0.96, 0.0])
ROWS2 = dict(g_seed=[7, 8], cfg=[3.0, 0.5], top_k=[0, 50], top_p=[0.5, 1.0])
ROWS4 = dict(ROWS, cfg=[[1.5, 2.0, 1.0], [3.0, 0.5, 2.0]])
ROWS4B = dict(ROWS2, cfg=[[0.5, 1.0, 4.0], [2.0, 2.0, 2.0]])


# ------------------------------------------------------------------------------------------------------------- the recorder
def _canon(v, seen):
    if torch.is_tensor(v):
        ptr = v.untyped_storage().data_ptr()
        alias = next((i for i, p in enumerate(seen) if p == ptr), None)
        seen.append(ptr)
        return (f'T(shape={tuple(v.shape)},stride={tuple(v.stride())},dtype={v.dtype},off={v.storage_offset()},dev={v.device.type},'
                f'alias={alias})')
    if v is None or isinstance(v, (bool, int, float, str, torch.dtype, torch.device)):
        return repr(v)
    if isinstance(v, (list, tuple)):
        return '[' + ','.join(_canon(x, seen) for x in v) + ']'
    if isinstance(v, dict):
        return '{' + ','.join(f'{k!r}:{_canon(v[k], seen)}' for k in sorted(v)) + '}'
    return f'<{type(v).__name__}>'


class Recorder:
    """with Recorder() as rec: ...  -> rec.lines, one per call into controlvar_amd.ops from outside it"""

    def __enter__(self):
        self.lines, self.names, self._depth, self._saved = [], [], 0, {}
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__:
                self._saved[name] = fn
                setattr(ops, name, self._wrap(name, fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(ops, name, fn)

    def _wrap(self, name, fn):
        sig = inspect.signature(fn)

        @functools.wraps(fn)
        def call(*a, **k):
            if self._depth == 0:
                self.names.append(name)
                if 'splitk_workspace' in name:              # arguments: stream handles
                    self.lines.append(name)
                else:
                    bound = sig.bind(*a, **k)
                    bound.apply_defaults()
                    seen = []
                    self.lines.append(name + '(' + ', '.join(f'{p}={_canon(v, seen)}' for p, v in bound.arguments.items()) + ')')
            self._depth += 1
            try:
                return fn(*a, **k)
            finally:
                self._depth -= 1
        return call


def run_length(names):
    out = []
    for n in names:
        if out and out[-1][0] == n:
            out[-1][1] += 1
        else:
            out.append([n, 1])
    return out


def ids_digest(tensors):
    if not tensors:
        return None
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to(torch.int32).cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------------------- the models
_MODELS = {}


def model(kind, dev):
    """built once per kind, weights packed (so that no case's record depends on which case came first)"""
    if kind not in _MODELS:
        vae = models.build_vae(ch=32, compute_dtype=torch.float32).to(dev)
        kw = dict(depth=2, embed_dim=128, num_heads=2, patch_nums=PN, compute_dtype=torch.float32, cond_drop_rate=0.0)
        if kind == 'var':
            m = models.VAR(vae, **kw)
        else:
            extra = {'two_pass': dict(separate_decoding=True, indep=False), 'separator': dict(separator=True)}.get(kind, {})
            m = models.ControlVAR(vae, mask_factor=2, multi_cond=True, **extra, **kw)
        m = m.to(dev).eval()
        if kind == 'banked':
            from test_gpu_adapter_batch import adapter_state
            lora.attach_adapters(m, [adapter_state(m, 16, 40 + k) for k in range(2)])
        m._pack(check=True); vae._pack(check=True)
        if kind == 'banked':
            lora.bank_pack(m)
        _MODELS[kind] = m
    return _MODELS[kind]


def rand_ids(seed, halves=1, rows=B):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, V, (rows, halves * pn * pn), generator=g) for pn in PN]


def keep_mask():
    S = PN[-1]
    k = torch.zeros(B, S, S, dtype=torch.bool)
    k[0, S // 4:S - S // 4, S // 4:S - S // 4] = True
    k[1, :, :S // 2] = True
    k[1, 3, :] = True
    return k


def trace_ids(m):
    return list(m.last_trace['idx'])


def score_ids(sc):
    return [sc.rank, sc.argmax]


# ------------------------------------------------------------------------------------------------------------- the cases
def _variant(kind, **kw):
    def case(dev):
        m = model(kind, dev)
        m.autoregressive_infer_cfg(B, LAB, g_seed=5, cfg=2.0, top_k=600, top_p=0.9, cond_type=TY, _trace=True, **kw)
        return trace_ids(m)
    return case


def _scalar(**kw):
    return _variant('control', **kw)


def _greedy(dev):
    m = model('control', dev)
    m.autoregressive_infer_cfg(B, LAB, g_seed=5, cfg=2.0, top_k=1, cond_type=TY, _trace=True)
    return trace_ids(m)


def _scalar_torch(dev):
    m = model('control', dev)
    m.sampler = 'torch'
    try:
        m.autoregressive_infer_cfg(B, LAB, g_seed=5, cfg=2.0, top_k=600, top_p=0.9, cond_type=TY, _trace=True)
    finally:
        m.sampler = 'counter'
    return trace_ids(m)


def _conditional(which):
    def case(dev):
        m = model('control', dev)
        m.conditional_infer_cfg(B, LAB, g_seed=5, cfg=(1.5, 2.0, 1.0), top_k=600, top_p=0.9, cond_type=TY, _trace=True, **{which: rand_ids(21)})
        return trace_ids(m)
    return case


def _rows(kind='control', logprobs=False, **kw):
    def case(dev):
        m = model(kind, dev)
        out = m.autoregressive_infer_cfg(B, LAB, cond_type=TY, _trace=True, logprobs=logprobs, **ROWS, **kw)
        return trace_ids(m) + (score_ids(out[1]) if logprobs else [])
    return case


def _rows_four(dev):
    m = model('control', dev)
    out = m.conditional_infer_cfg(B, LAB, cond_type=TY, c_mask=rand_ids(21), _trace=True, logprobs=True, **ROWS4)
    return trace_ids(m) + score_ids(out[1])


def _edit(kind='control', **kw):
    def case(dev):
        m = model(kind, dev)
        out = m.edit_infer_cfg(B, LAB, TY, src_img=rand_ids(22), keep_img=keep_mask(), trace=True, **ROWS, **kw)
        return trace_ids(m) + [m.last_trace['forced']] + (score_ids(out[1]) if kw.get('logprobs') else [])
    return case


def _score(given):
    def case(dev):
        m = model('control', dev)
        return score_ids(m.score_infer_cfg(B, LAB, TY, ids_img=rand_ids(22), ids_ctrl=rand_ids(23), given=given, cfg=[1.5, 4.0] if given is None else ROWS4['cfg']))
    return case


def _var_generate(dev):
    m = model('var', dev)
    m.autoregressive_infer_cfg(B, LAB, g_seed=5, cfg=2.0, top_k=600, top_p=0.9, _trace=True)
    return trace_ids(m)


def _var_edit(dev):
    m = model('var', dev)
    m.edit_infer_cfg(B, LAB, src_img=rand_ids(22), keep_img=keep_mask(), trace=True, **ROWS)
    return trace_ids(m) + [m.last_trace['forced']]


def _var_score(dev):
    return score_ids(model('var', dev).score_infer_cfg(B, LAB, ids_img=rand_ids(22), cfg=[1.5, 4.0]))


def _graph_scalar(dev):
    run = model('control', dev).graphed_generator(B, cfg=2.0, top_k=600, top_p=0.9)
    run(LAB, TY, g_seed=3)
    run(LAB2, TY2, g_seed=4)
    return []


def _graph_rows(dev):
    run = model('banked', dev).graphed_generator(B, per_request=True, adapters=True, logprobs=True)
    a = run(LAB, TY, adapter=[0, 1], **ROWS)[1]
    b = run(LAB2, TY2, adapter=[-1, 0], **ROWS2)[1]
    return score_ids(a) + score_ids(b)


def _graph_cond_scalar(dev):
    run = model('control', dev).graphed_conditional_generator(B, given='control', cfg=(1.5, 2.0, 1.0), top_k=600, top_p=0.9)
    out = []
    for lab, ty, ids, seed in ((LAB, TY, rand_ids(21), 3), (LAB2, TY2, torch.cat(rand_ids(24), dim=1), 4)):
        run(lab, ty, ids, g_seed=seed)
        out.append(run.ids())
    return out


def _graph_cond_rows(dev):
    run = model('control', dev).graphed_conditional_generator(B, given='image', source='pixels', decode='generated', per_request=True)
    out = []
    for lab, ty, seed, rows in ((LAB, TY, 43, ROWS4), (LAB2, TY2, 44, ROWS4B)):
        run(lab, ty, synth_images(B, 16 * PN[-1], seed=seed).to(dev), **rows)
        out.append(run.ids())
    return out


def _graph_edit(dev):
    run = model('control', dev).graphed_edit_generator(B, source='ids', logprobs=True)
    out = []
    for lab, ty, kw, rows in ((LAB, TY, dict(src_img=rand_ids(22), keep_img=keep_mask()), ROWS),
                              (LAB2, TY2, dict(src_img=rand_ids(25), keep_img=keep_mask().flip(0), src_ctrl=rand_ids(26), keep_ctrl=True), ROWS2)):
        sc = run(lab, ty, **kw, **rows)[1]
        out += list(run.ids()) + [run.forced()] + score_ids(sc)
    return out


CASES = {
    'scalar_plain': _scalar(),
    'scalar_more_smooth': _scalar(more_smooth=True),
    'scalar_greedy': _greedy,
    'scalar_force_idx': _scalar(_force_idx=rand_ids(20, halves=2)),
    'scalar_torch_sampler': _scalar_torch,
    'conditional_c_mask': _conditional('c_mask'),
    'conditional_c_img': _conditional('c_img'),
    'two_pass_plain': _variant('two_pass'),
    'two_pass_more_smooth': _variant('two_pass', more_smooth=True),
    'separator_joint': _variant('separator'),
    'rows_joint': _rows(),
    'rows_joint_logprobs': _rows(logprobs=True),
    'rows_joint_adapter': _rows('banked', logprobs=True, adapter=[0, 1]),
    'rows_four_branch_c_mask_logprobs': _rows_four,
    'edit_keep_img': _edit(),
    'edit_keep_ctrl_logprobs_adapter': _edit('banked', src_ctrl=rand_ids(23), keep_ctrl=True, logprobs=True, adapter=[1, -1]),
    'score_joint': _score(None),
    'score_given_control': _score('control'),
    'var_generate': _var_generate,
    'var_edit': _var_edit,
    'var_score': _var_score,
    'graph_scalar': _graph_scalar,
    'graph_rows_adapters_logprobs': _graph_rows,
    'graph_conditional_scalar_ids': _graph_cond_scalar,
    'graph_conditional_rows_pixels_generated': _graph_cond_rows,
    'graph_edit_ids_logprobs': _graph_edit,
}


def record_case(name, dev):
    """-> (fixture entry, full text)"""
    for kind in ('control', 'two_pass', 'separator', 'var', 'banked'):          # every model exists before anything is recorded
        model(kind, dev)
    random.seed(1234)
    torch.manual_seed(1234)
    with Recorder() as rec:
        ids = CASES[name](dev)
        torch.cuda.synchronize()
    text = '\n'.join(rec.lines) + '\n'
    return dict(launches=len(rec.lines), ops=run_length(rec.names), text_sha256=hashlib.sha256(text.encode()).hexdigest(), ids_sha256=ids_digest(ids)), text


@pytest.mark.parametrize('name', sorted(CASES))
def test_generation_issues_the_recorded_launches_on_the_recorded_ids(gpu_device, name):
    assert os.path.exists(FIXTURE), 'record it with tests/golden/make_generation_launches.py'
    with open(FIXTURE) as f:
        want = json.load(f)[name]
    got, _ = record_case(name, gpu_device)
    flat = lambda rle: [n for n, c in rle for _ in range(c)]
    a, b = flat(got['ops']), flat(want['ops'])
    if a != b:
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print(f'[launches] {name}: op names first differ at position {at}: issued {a[at:at + 3]}, recorded {b[at:at + 3]} ({len(a)} against {len(b)} launches)')
    assert got['launches'] == want['launches'], (name, got['launches'], want['launches'])
    assert got['ops'] == want['ops'], name
    assert got['text_sha256'] == want['text_sha256'], (name, 'same op names, different arguments: diff the --dump texts')
    assert got['ids_sha256'] == want['ids_sha256'], (name, 'token ids')
