"""Top-N alternatives and sparse distillation targets end to end on the MI355X, depth-2 models under deterministic_plan=True.
top_logprobs=N changes nothing else (ids, images and the old TokenScores fields bit for bit); the alternatives agree with the scores beside them
(top_ids[..., 0] == argmax, top_ids[..., rank] is the scored id with logprob's bits where rank < N); joint, conditional, edit and score_infer_cfg calls; graph
replays equal the eager calls; distill_topn returns the ids DistillTargets returns and the alternatives logprobs returns; step_tokens(distill=sparse) is
forward_train + ops.kd_topn_fwd_bwd + backward(); a one-hot sparse step is the supervised step (full and LoRA); a grad_accum window holds the sum."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import lora, models, ops, train as T  # noqa: E402
from controlvar_amd.models import SparseDistillTargets  # noqa: E402
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN  # noqa: E402
from controlvar_amd.synth import synth_images  # noqa: E402
from controlvar_amd.train import SparseDistillLoss  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
V, B, N = 4096, 3, 8
LABELS, TYPES = torch.tensor([1, 500, 999]), torch.tensor([0, 3, 1])
ROWS = dict(g_seed=[11, 12, 2 ** 64 - 5], cfg=[1.5, 4.0, 3.0], top_k=[900, 1, 0], top_p=[0.96, 0.0, 0.5])          # sampled, greedy, nucleus only
CFG3 = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (0.5, 4.0, 2.0)]
OLD = ('logprob', 'entropy', 'rank', 'argmax', 'sampled')
TOP = ('top_ids', 'top_logprobs', 'tail_logprob')
KW = dict(peak_lr=2e-3, weight_decay=0.05, sche='lin0', warmup_it=2, max_it=50, clip=2.0, drop_path=False)
_MODELS = {}


def make(kind, dtype, dev):
    """'control' / 'var': the depth-2 models, built once; 'lora' / 'joint': a fresh trainable control model (LoRA adapters with B != 0)"""
    if kind in ('control', 'var') and (kind, dtype) in _MODELS:
        return _MODELS[(kind, dtype)]
    vae = models.build_vae(ch=32, compute_dtype=dtype).to(dev)
    if kind == 'var':
        m = models.build_var(vae, depth=2, compute_dtype=dtype, cond_drop_rate=0.0, deterministic_plan=True).to(dev).eval()
    else:
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, cond_drop_rate=0.0,
                                     deterministic_plan=True).to(dev).eval()
    if kind == 'lora':
        lora.add_lora(m, r=16, dropout=0.0, seed=1)
        g = torch.Generator().manual_seed(3)
        with torch.no_grad():
            for _, (_, Bm) in lora.adapters(m).items():
                Bm.copy_(torch.randn(Bm.shape, generator=g) * 0.05)
    if kind in ('control', 'var'):
        _MODELS[(kind, dtype)] = (vae, m)
    return vae, m


@pytest.fixture(scope='module')
def src(gpu_device):
    """(control ids, image ids) of three synthetic pictures, computed once and left unchanged"""
    vae = make('control', BF16, gpu_device)[0]
    return (vae.img_to_idxBl(synth_images(B, 256, seed=41).to(gpu_device)), vae.img_to_idxBl(synth_images(B, 256, seed=42).to(gpu_device)))


def hole(n, S=16, lo=4, hi=12):
    keep = torch.ones(n, S, S, dtype=torch.bool)
    keep[:, lo:hi, lo:hi] = False
    return keep


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b, what, fields):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(bits(x), bits(y)), (what, f)


def check_alternatives(sc, ids, what, n=N):
    """the alternatives against the scores beside them; ids: the scored ids (B, L)"""
    L = sc.logprob.shape[1]
    assert [tuple(getattr(sc, f).shape) for f in TOP] == [(B, L, n), (B, L, n), (B, L)], what
    assert [getattr(sc, f).dtype for f in TOP] == [torch.int32, torch.float32, torch.float32], what
    assert torch.equal(sc.top_ids[..., 0], sc.argmax), what
    assert bool((sc.top_ids >= 0).all()) and bool((sc.top_ids < V).all()), what
    lp = sc.top_logprobs
    assert bool((lp[..., :-1] >= lp[..., 1:]).all()) and bool((lp <= 0).all()), what          # rank order: never increasing
    inside = sc.rank < n
    assert bool(inside.any()), what                                                            # (a peaked model may leave no token outside a large N)
    at = sc.rank.clamp(max=n - 1).long()[..., None]
    assert torch.equal(sc.top_ids.gather(2, at)[..., 0][inside], ids[inside]), what
    assert torch.equal(bits(sc.top_logprobs.gather(2, at)[..., 0][inside]), bits(sc.logprob[inside])), what
    assert not bool((sc.top_ids == ids[..., None])[~inside].any()), what                      # rank >= N: the id is not among the alternatives
    mass = sc.top_logprobs.double().exp().sum(-1) + sc.tail_logprob.double().exp()
    assert float((mass - 1).abs().max()) < 1e-4, what                                          # the N cells and the tail partition the distribution


def trace_ids(m):
    return torch.cat([x[:B] for x in m.last_trace['idx']], dim=1)


# ------------------------------------------------------------------------------------------------------------- nothing else changes
@pytest.mark.parametrize('path', ['joint', 'conditional', 'edit'])
def test_the_keyword_changes_nothing_else_and_the_alternatives_agree_with_the_scores(gpu_device, src, path):
    vae, m = make('control', BF16, gpu_device)
    if path == 'joint':
        call = lambda **kw: m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, _trace=True, **ROWS, **kw)
    elif path == 'conditional':
        call = lambda **kw: m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, c_mask=src[0], _trace=True, **dict(ROWS, cfg=CFG3), **kw)
    else:
        call = lambda **kw: m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], keep_img=hole(B), src_ctrl=src[0], keep_ctrl=True, trace=True, **ROWS, **kw)
    want, old = call(logprobs=True)
    ref = trace_ids(m)
    assert all(getattr(old, f) is None for f in TOP)
    got, sc = call(logprobs=True, top_logprobs=N)
    assert torch.equal(trace_ids(m), ref) and torch.equal(got, want)
    same(sc, old, path, OLD)
    # the ids the scores were taken of: the drawn ones, overwritten where a half was forced / kept
    ids = ref.clone()
    if path == 'conditional':
        b = 0
        for pn, given in zip(PN, src[0]):
            ids[:, b:b + pn * pn] = given.to(torch.int32)
            b += 2 * pn * pn
    check_alternatives(sc, ids, path)
    for one, whole in zip(sc.per_scale(), [(b, e) for b, e in sc._bounds()]):
        assert torch.equal(one.top_ids, sc.top_ids[:, whole[0]:whole[1]]) and torch.equal(one.tail_logprob, sc.tail_logprob[:, whole[0]:whole[1]])


def test_plain_var_and_another_n(gpu_device):
    vae, m = make('var', BF16, gpu_device)
    rows = dict(ROWS)
    want, old = m.autoregressive_infer_cfg(B, LABELS, logprobs=True, _trace=True, **rows)
    ids = trace_ids(m)
    for n in (1, 64):
        got, sc = m.autoregressive_infer_cfg(B, LABELS, logprobs=True, top_logprobs=n, **rows)
        assert torch.equal(got, want)
        same(sc, old, f'var N={n}', OLD)
        check_alternatives(sc, ids, f'var N={n}', n)


# ------------------------------------------------------------------------------------------------------------- given tokens
@pytest.mark.parametrize('given', [None, 'control'])
def test_score_infer_cfg_reports_the_alternatives_of_given_tokens(gpu_device, src, given):
    vae, m = make('control', BF16, gpu_device)
    kw = dict(ids_ctrl=src[0], ids_img=src[1], given=given, cfg=CFG3 if given else [1.5, 4.0, 0.0])
    old = m.score_infer_cfg(B, LABELS, TYPES, **kw)
    sc = m.score_infer_cfg(B, LABELS, TYPES, top_logprobs=N, **kw)
    same(sc, old, f'given={given}', OLD)
    ids = torch.cat([torch.cat((c, i), dim=1) for c, i in zip(*src)], dim=1).to(torch.int32)
    check_alternatives(sc, ids, f'given={given}')
    loss = sc.sparse_loss()
    assert isinstance(loss, SparseDistillLoss) and loss.top_ids is sc.top_ids and loss.tail_logprob is sc.tail_logprob and loss.weights is None
    with pytest.raises(ValueError, match='top_logprobs=N'):
        old.sparse_loss()


# ------------------------------------------------------------------------------------------------------------- graphs
def test_graph_replays_equal_the_eager_calls(gpu_device, src):
    vae, m = make('control', BF16, gpu_device)
    rows2 = dict(g_seed=[5, 6, 7], cfg=[0.0, 2.5, 4.0], top_k=[0, 50, 1], top_p=[0.0, 0.9, 0.0])
    mk = dict(keep_img=hole(B), keep_ctrl=True)
    cases = [
        (lambda: m.graphed_generator(B, per_request=True, logprobs=True, top_logprobs=N),
         lambda g, r: g(LABELS, TYPES, **r),
         lambda r: m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, logprobs=True, top_logprobs=N, **r)),
        (lambda: m.graphed_conditional_generator(B, given='control', per_request=True, logprobs=True, top_logprobs=N),
         lambda g, r: g(LABELS, TYPES, src[0], **dict(r, cfg=CFG3)),
         lambda r: m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, c_mask=src[0], logprobs=True, top_logprobs=N, **dict(r, cfg=CFG3))),
        (lambda: m.graphed_edit_generator(B, logprobs=True, top_logprobs=N),
         lambda g, r: g(LABELS, TYPES, src_img=src[1], src_ctrl=src[0], **mk, **r),
         lambda r: m.edit_infer_cfg(B, LABELS, TYPES, src_img=src[1], src_ctrl=src[0], logprobs=True, top_logprobs=N, **mk, **r)),
    ]
    for k, (capture, replay, eager) in enumerate(cases):
        g = capture()
        first = None
        for rows in (ROWS, rows2):
            img, sc = replay(g, rows)
            want, ref = eager(rows)
            assert torch.equal(img, want), k
            same(sc, ref, f'graph {k}', OLD + TOP)
            if first is None:
                first = (img, sc, {f: getattr(sc, f).clone() for f in TOP})
        for f in TOP:                                               # the results are copies: a later replay did not change the first one's
            assert torch.equal(bits(getattr(first[1], f)), bits(first[2][f])), (k, f)
        del g
    g = m.graphed_generator(B, per_request=True, logprobs=True)     # captured without the keyword: the scores hold no alternatives
    assert all(getattr(g(LABELS, TYPES, **ROWS)[1], f) is None for f in TOP)


# ------------------------------------------------------------------------------------------------------------- sparse targets of a generation
@pytest.mark.parametrize('call', ['joint', 'conditional'])
def test_distill_topn_returns_the_ids_of_distill_targets_and_the_alternatives_of_logprobs(gpu_device, src, call):
    vae, m = make('control', BF16, gpu_device)
    if call == 'joint':
        gen = lambda **kw: m.autoregressive_infer_cfg(B, LABELS, cond_type=TYPES, **ROWS, **kw)
    else:
        gen = lambda **kw: m.conditional_infer_cfg(B, LABELS, cond_type=TYPES, c_mask=src[0], **dict(ROWS, cfg=CFG3), **kw)
    images, dense = gen(distill_targets=True)
    images1, sc = gen(logprobs=True, top_logprobs=32)
    m.last_trace = None
    images2, t = gen(distill_topn=32)
    assert m.last_trace is None                                     # nothing traced: no (B, L, V) tensor was kept
    assert isinstance(t, SparseDistillTargets) and torch.equal(images2, images) and torch.equal(images1, images)
    assert torch.equal(t.ids_img, dense.ids_img) and torch.equal(t.ids_ctrl, dense.ids_ctrl) and torch.equal(t.sampled, dense.sampled) and t.mask_first is True
    for f in TOP:
        assert torch.equal(bits(getattr(t, f)), bits(getattr(sc, f))), f
    # the alternatives are the top of the dense guided logits, and the bytes are 63 times fewer
    top = dense.logits.log_softmax(-1).topk(32, dim=-1)
    assert float((top.values - t.top_logprobs).abs().max()) < 1e-4
    stored = sum(getattr(t, f).numel() * 4 for f in TOP)
    assert stored == B * m.cfg.pyramid.L * (32 * 8 + 4) and dense.logits.numel() * 4 / stored > 60
    # with logprobs=True the scores ride along, without the alternatives unless asked for
    _, sc2, t2 = gen(logprobs=True, distill_topn=32)
    same(sc2, sc, 'scores', OLD)
    assert sc2.top_ids is None and torch.equal(t2.top_ids, t.top_ids)
    _, sc3, t3 = gen(logprobs=True, top_logprobs=32, distill_topn=32)
    assert torch.equal(sc3.top_ids, t3.top_ids)
    loss = t.loss()
    assert isinstance(loss, SparseDistillLoss) and loss.weights is t.sampled and loss.N == 32


def test_distill_topn_with_scalar_arguments_takes_the_per_request_path(gpu_device):
    """the one difference to distill_targets=True: distill_topn always runs the per-request path, which broadcasts a scalar g_seed under the key the
    scalar call builds at B = 1.  At B = 1 the two calls draw the same sample; from B = 2 on distill_topn's ids are those of distill_targets=True with
    g_seed=[s] * B - row 0 is also the scalar-seed call's, the later rows are not"""
    vae, m = make('control', BF16, gpu_device)
    kw = dict(cfg=4.0, top_k=900, top_p=0.95)
    img_d, d = m.autoregressive_infer_cfg(1, LABELS[:1], g_seed=5, cond_type=TYPES[:1], distill_targets=True, **kw)
    img_t, t = m.autoregressive_infer_cfg(1, LABELS[:1], g_seed=5, cond_type=TYPES[:1], distill_topn=N, **kw)
    assert torch.equal(img_t, img_d) and torch.equal(t.ids_img, d.ids_img) and torch.equal(t.ids_ctrl, d.ids_ctrl)
    img_s, scalar = m.autoregressive_infer_cfg(2, LABELS[:2], g_seed=5, cond_type=TYPES[:2], distill_targets=True, **kw)
    img_r, rows = m.autoregressive_infer_cfg(2, LABELS[:2], g_seed=[5, 5], cond_type=TYPES[:2], distill_targets=True, **kw)
    img_t, t = m.autoregressive_infer_cfg(2, LABELS[:2], g_seed=5, cond_type=TYPES[:2], distill_topn=N, **kw)
    assert torch.equal(img_t, img_r) and torch.equal(t.ids_img, rows.ids_img) and torch.equal(t.ids_ctrl, rows.ids_ctrl)
    assert torch.equal(t.ids_img[0], scalar.ids_img[0]) and not torch.equal(t.ids_img[1], scalar.ids_img[1])
    top = rows.logits.log_softmax(-1).topk(N, dim=-1)
    assert float((top.values - t.top_logprobs).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------- the training step
def _ids(vae, dev, n):
    images, masks = synth_images(4, 256, seed=6)[:n].to(dev), synth_images(4, 256, seed=7)[:n].to(dev)
    both = vae.img_to_idxBl(torch.cat((masks, images), dim=0))
    return [t[:n].clone() for t in both], [t[n:].clone() for t in both]


def _clone(d):
    return {k: v.clone() for k, v in d.items()}


def _same(a, b, what=''):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _sparse_teacher(n, L, dev, seed=0, topn=32):
    """a sparse teacher from random dense logits through the kernel under test's sibling: ops.score_topn on (n, L, V) rows"""
    g = torch.Generator().manual_seed(70 + seed)
    std = torch.logspace(-1.5, 0.9, n * L).view(n, L, 1)
    z = (torch.randn(n, L, V, generator=g) * std).clamp(-30, 30).to(dev)
    ids = torch.empty(n, L, topn, dtype=torch.int32, device=dev)
    lp, tail = torch.empty(n, L, topn, device=dev), torch.empty(n, L, device=dev)
    ops.score_topn(z, n, 1, L, V, torch.tensor([[1.0, 0, 0, 0]], device=dev).repeat(n, 1), topn, ids, lp, tail)
    return ids, lp, tail


@pytest.mark.parametrize('kind,dtype', [('joint', BF16), ('joint', F32), ('lora', BF16)])
def test_sparse_distill_step_is_the_walk_with_another_loss_launch(gpu_device, kind, dtype):
    n = 2
    cls, types = LABELS[:n], TYPES[:n]
    vae, m = make(kind, dtype, gpu_device)
    tr = T.Trainer(m, vae, **KW)
    eng = tr.engine
    ctrl, img = _ids(vae, gpu_device, n)
    L = m.cfg.pyramid.L
    ids, lp, tail = _sparse_teacher(n, L, gpu_device)
    mask = (torch.rand(n, L, generator=torch.Generator().manual_seed(5)) < 0.8).float().to(gpu_device)
    o = tr.step_tokens(img, ctrl, cls, types, distill=SparseDistillLoss(ids, lp, tail, weights=mask))
    grads, dlogits, loss_tok, loss = _clone(eng.grads()), eng.dlogits.clone(), eng.loss_tok.clone(), o['loss'].clone()
    assert bool((loss_tok > 0).all()) and bool(dlogits.any())
    # the same parameters again (a fresh model: the step above updated this one): forward_train + the kernel by hand + backward()
    vae2, m2 = make(kind, dtype, gpu_device)
    tr2 = T.Trainer(m2, vae2, **KW)
    eng2 = tr2.engine
    x, _ = tr2._inputs_of([torch.cat((c, i), 0) for c, i in zip(ctrl, img)], n, True)
    eng2.forward_train(cls, x, types, None, True)
    M = eng2.M
    w = mask.view(-1)
    gscale = 1.0 / (M * (float(w.mean()) + 1e-6))
    lt, dl = torch.empty(M, device=gpu_device), torch.empty_like(dlogits)
    ops.kd_topn_fwd_bwd(eng2.logits, ids, lp, tail, 32, w, gscale, lt, dl, M, V)
    assert torch.equal(dl, dlogits) and torch.equal(lt, loss_tok)
    assert torch.equal(loss, (lt * w).mean() / (w.mean() + 1e-6))
    eng2.dlogits.copy_(dl)
    eng2.backward()
    _same(eng2.grads(), grads, 'grads')


@pytest.mark.parametrize('kind,dtype', [('joint', BF16), ('lora', BF16), ('joint', F32), ('lora', F32)])
def test_one_hot_sparse_step_is_the_supervised_step(gpu_device, kind, dtype):
    n = 2
    cls, types = LABELS[:n], TYPES[:n]
    out = []
    for sparse in (False, True):
        vae, m = make(kind, dtype, gpu_device)
        tr = T.Trainer(m, vae, **KW)
        ctrl, img = _ids(vae, gpu_device, n)
        L = m.cfg.pyramid.L
        labels = tr._inputs_of([torch.cat((c, i), 0) for c, i in zip(ctrl, img)], n, True)[1].to(gpu_device)
        hot = SparseDistillLoss(labels.view(n, L, 1).to(torch.int32).contiguous(), torch.zeros(n, L, 1, device=gpu_device))
        log = []
        for _ in range(2):
            o = tr.step_tokens(img, ctrl, cls, types, distill=hot if sparse else None)
            log.append((o['loss'].clone(), o['grad_norm'].clone(), _clone(tr.engine.grads()), _clone(m.state_dict())))
        out.append(log)
    for a, b in zip(*out):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        _same(a[2], b[2], 'grads')
        _same(a[3], b[3], 'parameters')
    assert any(not torch.equal(out[0][0][3][k], out[0][1][3][k]) for k in out[0][0][3])                  # the steps did move the parameters


@pytest.mark.parametrize('kind', ['joint', 'lora'])
def test_window_of_sparse_micro_batches_holds_the_sum(gpu_device, kind):
    n, dtype = 2, BF16
    cls, types = LABELS[:n], TYPES[:n]
    vae, m = make(kind, dtype, gpu_device)
    ctrl, img = _ids(vae, gpu_device, n)
    L = m.cfg.pyramid.L
    ids, lp, tail = _sparse_teacher(n, L, gpu_device, seed=1)
    w = (torch.rand(n, L, generator=torch.Generator().manual_seed(8)) < 0.7).float().to(gpu_device)
    one = lambda t, b: [s[b:b + 1] for s in t]
    part = lambda b: SparseDistillLoss(ids[b:b + 1], lp[b:b + 1], tail[b:b + 1], weights=w[b:b + 1])
    tr0 = T.Trainer(m, vae, **KW)
    plain = []
    for b in range(n):
        x, labels = tr0._inputs_of([torch.cat((c, i), 0) for c, i in zip(one(ctrl, b), one(img, b))], 1, True)
        tr0.engine.forward_backward(cls[b:b + 1], x, types[b:b + 1], labels, distill=part(b))
        plain.append(_clone(tr0.engine.grads()))
    assert any(bool((plain[0][k] != plain[1][k]).any()) for k in plain[0])
    vae2, m2 = make(kind, dtype, gpu_device)
    tr = T.Trainer(m2, vae2, grad_accum=2, **KW)
    for b in range(n):
        o = tr.step_tokens(one(img, b), one(ctrl, b), cls[b:b + 1], types[b:b + 1], distill=part(b))
        assert o['micro'] == b and o['synced'] == (b == 1)
    _same(tr.engine.grads(), {k: plain[0][k] + plain[1][k] for k in plain[0]}, 'window')
