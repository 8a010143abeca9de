"""Generation without guidance rows on MI355X (cfg=None), all under deterministic_plan=True and the counter sampler.

One invariant, torch.equal with no tolerance: cfg=None runs R = B transformer rows and returns the bits of cfg=0.0 - or cfg=(0, 0, 0) on the conditional
call - which runs 2 B (4 B) rows and weighs the guidance rows by zero: 1 * l0 + (-0) * l1 is l0, the plan makes a row's logits independent of the rows beside
it, and the draw key of branch 0 does not depend on the number of branches.  Held on the traced ids, the combined logits, f_hat and the images, for the joint
ControlVAR call, a plain VAR and the conditional call with either half given; greedy and top-k / top-p with a seed; bf16, fp32, kv_precision='fp8',
gemm_precision='bf16x3' and 'fp8'; scalar and per-request parameters; logprobs=True; and the two graphed generators against their eager calls.  The K/V
arena of an unguided call has B rows (its allocated shape is asserted, not a timing), and every refusal raises in words before anything is launched."""
import inspect

import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import models, ops  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
B = 3
LAB, TY = torch.tensor([3, 977, 500]), torch.tensor([1, 2, 0])
LAB2, TY2 = torch.tensor([500, 0, 41]), torch.tensor([3, 0, 2])
# (compute dtype, gemm_precision, kv_precision)
MODES = {'bf16': (BF16, None, None), 'fp32': (F32, None, None), 'kv8': (BF16, None, 'fp8'), 'bf16x3': (F32, 'bf16x3', None), 'fp8': (BF16, 'fp8', None)}
SCALAR = [dict(g_seed=5, top_k=1, top_p=0.0), dict(g_seed=2 ** 64 - 7, top_k=900, top_p=0.95)]                     # greedy; top-k / top-p with a seed
ROWS = [dict(g_seed=[11, 2 ** 64 - 5, 3], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])]                             # mixed per row, the greedy row between
_MODELS, _GIVEN = {}, {}


def model(kind, mode, dev):
    """built once per (kind, mode): depth 2, width 128, the tiny VQVAE"""
    key = (kind, mode)
    if key not in _MODELS:
        dtype, gp, kvp = MODES[mode]
        vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
        kw = dict(depth=2, embed_dim=128, num_heads=2, patch_nums=PN, compute_dtype=dtype, cond_drop_rate=0.0, deterministic_plan=True, gemm_precision=gp,
                  kv_precision=kvp)
        m = models.VAR(vae, **kw) if kind == 'var' else models.ControlVAR(vae, mask_factor=2, multi_cond=True, **kw)
        _MODELS[key] = (vae, m.to(dev).eval())
    return _MODELS[key]


def given_ids(vae, mode, dev):
    if mode not in _GIVEN:
        _GIVEN[mode] = [t.clone() for t in vae.img_to_idxBl(synth_images(B, 256, seed=32).to(dev))]
    return _GIVEN[mode]


def caller(call, vae, m, mode, dev, labels=LAB, types=TY):
    """-> gen(cfg_is_none, **params): the public call of `call` with cfg=None or its zero guidance"""
    if call == 'var':
        return lambda none, **p: m.autoregressive_infer_cfg(B, labels, cfg=None if none else 0.0, **p)
    if call == 'joint':
        return lambda none, **p: m.autoregressive_infer_cfg(B, labels, cond_type=types, cfg=None if none else 0.0, **p)
    arg = 'c_mask' if call == 'given_control' else 'c_img'
    ids = given_ids(vae, mode, dev)
    return lambda none, **p: m.conditional_infer_cfg(B, labels, cond_type=types, cfg=None if none else (0.0, 0.0, 0.0), **{arg: ids}, **p)


def traced(m, gen, none, **p):
    out = gen(none, _trace=True, **p)
    t = m.last_trace
    return out, [i[:B].clone() for i in t['idx']], [x.clone() for x in t['logits']], t['f_hat'].clone()


def arena_rows(m):
    """the row count of every K/V arena the model holds"""
    out = set()
    for _, buf in (m._arena or {}).values():
        out.add((buf.q if isinstance(buf, models.KV8Arena) else buf).shape[1])
    return out


class Launches:
    """with Launches() as n: ...  -> n.count, the calls into controlvar_amd.ops"""

    def __enter__(self):
        self.count, self._saved = 0, {}
        for name, fn in list(vars(ops).items()):
            if inspect.isfunction(fn) and fn.__module__ == ops.__name__:
                self._saved[name] = fn
                setattr(ops, name, self._wrap(fn))
        return self

    def __exit__(self, *exc):
        for name, fn in self._saved.items():
            setattr(ops, name, fn)

    def _wrap(self, fn):
        def call(*a, **k):
            self.count += 1
            return fn(*a, **k)
        return call


# ---------------------------------------------------------------------------------------------------------------- 1. cfg=None == cfg=0, bit for bit
@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('call', ['joint', 'var', 'given_control', 'given_image'])
def test_unguided_is_zero_guidance_bit_for_bit(gpu_device, call, mode):
    vae, m = model('var' if call == 'var' else 'cvar', mode, gpu_device)
    gen = caller(call, vae, m, mode, gpu_device)
    nrep = 4 if call.startswith('given') else 2
    seen = []
    for p in SCALAR + ROWS:
        m._arena = None
        img0, ids0, lg0, fh0 = traced(m, gen, False, **p)
        assert arena_rows(m) == {nrep * B}
        m._arena = None
        img1, ids1, lg1, fh1 = traced(m, gen, True, **p)
        assert arena_rows(m) == {B}                                            # the unguided call's K/V arena has B rows
        assert all(torch.equal(a, b) for a, b in zip(ids0, ids1)) and len(ids0) == len(ids1) == len(PN)
        assert all(torch.equal(a, b) for a, b in zip(lg0, lg1))
        assert torch.equal(fh0, fh1) and torch.equal(img0, img1)
        seen.append(torch.cat(ids1, dim=1))
    assert not torch.equal(seen[0], seen[1])                                   # the sampled call is not the greedy one


# ---------------------------------------------------------------------------------------------------------------- 2. logprobs=True
@pytest.mark.parametrize('call,mode', [('joint', 'bf16'), ('var', 'fp32'), ('given_control', 'bf16'), ('given_image', 'kv8')])
def test_token_scores_equal_the_zero_guidance_call(gpu_device, call, mode):
    vae, m = model('var' if call == 'var' else 'cvar', mode, gpu_device)
    gen = caller(call, vae, m, mode, gpu_device)
    for p in (SCALAR[1], ROWS[0]):
        img0, sc0 = gen(False, logprobs=True, **p)
        img1, sc1 = gen(True, logprobs=True, **p)
        assert torch.equal(img0, img1)
        for f in ('logprob', 'entropy', 'rank', 'argmax', 'sampled'):
            assert torch.equal(getattr(sc0, f), getattr(sc1, f)), f
        assert sc1.mask_first == sc0.mask_first and tuple(sc1.logprob.shape) == (B, m.cfg.pyramid.L)
        assert bool(sc1.sampled.all()) == (not call.startswith('given'))


# ---------------------------------------------------------------------------------------------------------------- 3. the graphed generators
@pytest.mark.parametrize('per_request', [False, True], ids=['scalar', 'rows'])
def test_graphed_generator_replays_to_the_eager_call(gpu_device, per_request):
    vae, m = model('cvar', 'bf16', gpu_device)
    run = m.graphed_generator(B, cfg=None, top_k=900, top_p=0.95, per_request=per_request)
    for labels, types, seed in ((LAB, TY, [5, 6, 7] if per_request else 5), (LAB2, TY2, [7, 8, 2 ** 64 - 9] if per_request else 77)):    # per row: the eager call's per-request path
        got = run(labels, types, g_seed=seed)
        want = m.autoregressive_infer_cfg(B, labels, cond_type=types, g_seed=seed, cfg=None, top_k=900, top_p=0.95)
        assert torch.equal(got, want)
    if per_request:
        got = run(LAB, TY, g_seed=[1, 2, 3], top_k=[1, 50, 0], top_p=[0.0, 0.5, 1.0])
        assert torch.equal(got, m.autoregressive_infer_cfg(B, LAB, cond_type=TY, g_seed=[1, 2, 3], cfg=None, top_k=[1, 50, 0], top_p=[0.0, 0.5, 1.0]))
        with pytest.raises(ValueError, match='captured with cfg=None'):
            run(LAB, TY, g_seed=1, cfg=1.5)
        guided = m.graphed_generator(B, cfg=1.5, per_request=True)
        with pytest.raises(ValueError, match='captured with guidance rows'):
            guided(LAB, TY, g_seed=1, cfg=None)


@pytest.mark.parametrize('per_request', [False, True], ids=['scalar', 'rows'])
def test_graphed_conditional_generator_replays_to_the_eager_call(gpu_device, per_request):
    vae, m = model('cvar', 'bf16', gpu_device)
    ids = given_ids(vae, 'bf16', gpu_device)
    ids2 = [t.flip(0).contiguous() for t in ids]
    run = m.graphed_conditional_generator(B, given='control', cfg=None, top_k=900, top_p=0.95, per_request=per_request)
    for labels, types, half, seed in ((LAB, TY, ids, [5, 6, 7] if per_request else 5), (LAB2, TY2, ids2, [7, 8, 2 ** 64 - 9] if per_request else 77)):
        got = run(labels, types, half, g_seed=seed)
        want = m.conditional_infer_cfg(B, labels, cond_type=types, g_seed=seed, cfg=None, top_k=900, top_p=0.95, c_mask=half)
        assert torch.equal(got, want)
    assert torch.equal(run.ids().long(), torch.cat(ids2, dim=1))


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_launch_nothing(gpu_device):
    vae, m = model('cvar', 'bf16', gpu_device)
    ids = given_ids(vae, 'bf16', gpu_device)
    flat = torch.cat(ids, dim=1)
    vae2 = models.build_vae(ch=32, compute_dtype=BF16).to(gpu_device)
    kw = dict(depth=2, embed_dim=128, num_heads=2, patch_nums=PN, compute_dtype=BF16, cond_drop_rate=0.0, mask_factor=2, multi_cond=True)
    sep = models.ControlVAR(vae2, separator=True, **kw).to(gpu_device).eval()
    two = models.ControlVAR(vae2, separate_decoding=True, indep=False, **kw).to(gpu_device).eval()
    with Launches() as n:
        with pytest.raises(NotImplementedError, match='adapter'):
            m.autoregressive_infer_cfg(B, LAB, cond_type=TY, cfg=None, adapter=0)
        m._adapter_bank = dict(n=1)
        try:
            with pytest.raises(NotImplementedError, match='adapter bank'):
                m.conditional_infer_cfg(B, LAB, cond_type=TY, cfg=None, c_mask=ids)
        finally:
            m._adapter_bank = None
        m.sampler = 'torch'
        try:
            for call in (lambda: m.autoregressive_infer_cfg(B, LAB, cond_type=TY, cfg=None), lambda: m.conditional_infer_cfg(B, LAB, cond_type=TY, cfg=None, c_mask=ids),
                         lambda: m.graphed_generator(B, cfg=None), lambda: m.graphed_conditional_generator(B, cfg=None)):
                with pytest.raises(NotImplementedError, match="sampler='torch'"):
                    call()
        finally:
            m.sampler = 'counter'
        with pytest.raises(NotImplementedError, match='two-pass'):
            two.autoregressive_infer_cfg(B, LAB, cond_type=TY, cfg=None)
        for call in (lambda: sep.autoregressive_infer_cfg(B, LAB, cond_type=TY, cfg=None), lambda: sep.graphed_generator(B, cfg=None)):
            with pytest.raises(NotImplementedError, match='separator'):
                call()
        with pytest.raises(NotImplementedError, match='edit_infer_cfg'):
            m.edit_infer_cfg(B, LAB, TY, src_img=flat, keep_img=True, cfg=None)
        with pytest.raises(NotImplementedError, match='graphed_edit_generator'):
            m.graphed_edit_generator(B, cfg=None)
        with pytest.raises(NotImplementedError, match='score_infer_cfg'):
            m.score_infer_cfg(B, LAB, TY, ids_img=flat, ids_ctrl=flat, cfg=None)
        assert n.count == 0
    # and the model still generates
    assert torch.equal(m.autoregressive_infer_cfg(B, LAB, cond_type=TY, g_seed=5, cfg=None, top_k=1),
                       m.autoregressive_infer_cfg(B, LAB, cond_type=TY, g_seed=5, cfg=0.0, top_k=1))
