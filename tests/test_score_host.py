"""Token log-probabilities, host side (no GPU): the float64 reference (tests/score_ref.py) against torch, a numpy emulation of the kernel's
order of evaluation against the bounds derived from that order, TokenScores' layout helpers, every refusal of logprobs=True and score_infer_cfg in
words, and cvar_score_rows in the ctypes table of include/cvar_serve.h."""
import os
import re

import numpy as np
import pytest
import torch

from controlvar_amd import _lib, models
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, PATCH_NUMS_512 as PN512
from score_ref import combine_f32, score_ref, within_bounds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# --------------------------------------------------------------------------------------------------------------- the entry point
def header_args(name):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'cvar_serve.h')).read(), flags=re.S)
    m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', src)
    assert m, f'{name} is not declared in include/cvar_serve.h'
    return [a.strip() for a in m.group(1).split(',')]


def test_score_rows_is_in_the_serve_table_with_the_headers_argument_count():
    args = header_args('cvar_score_rows')
    assert 'cvar_score_rows' in _lib.SERVE_SIGNATURES and 'cvar_score_rows' not in _lib.SIGNATURES
    res, argtypes = _lib.SERVE_SIGNATURES['cvar_score_rows']
    assert res is _lib.c_i and len(argtypes) == len(args) == 16
    for a, t in zip(args, argtypes):                              # pointers are c_void_p, everything else of this entry point an int
        assert t is (_lib.c_p if '*' in a else _lib.c_i), a
    assert _lib.SERVE_VERSION == 1                                # an added entry point changes no signature
    from controlvar_amd import ops
    assert callable(ops.score_rows)


def test_score_rows_refuses_its_arguments_with_a_status_and_without_a_launch():
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    lib = _lib.load()
    one = 8                                                       # any non-null address: nothing is launched on these paths
    args = dict(logits=one, B=2, nrep=2, l=3, V=4096, coef=one, target=one, ldt=3, comb=None, lp=one, en=None, rk=None, am=None, ldo=0, ldv=0, stream=None)

    def call(**kw):
        return lib.cvar_score_rows(*{**args, **kw}.values())
    for bad in (dict(logits=None), dict(coef=None), dict(target=None), dict(ldt=2), dict(lp=None), dict(B=0), dict(l=0), dict(V=0), dict(ldv=4095),
                dict(ldo=2)):
        assert call(**bad) == -1, bad                             # CVAR_EINVAL
    for bad in (dict(nrep=0), dict(nrep=5), dict(V=4097)):
        assert call(**bad) == -2, bad                             # CVAR_EUNSUPPORTED


def test_score_rows_torch_op_schema_and_fake_kernel():
    import controlvar_amd
    ns = controlvar_amd.register_torch_ops()
    from controlvar_amd import torch_ops
    assert 'score_rows' in torch_ops.OPS
    assert str(ns.score_rows.default._schema) == 'cvar::score_rows(Tensor logits, int B, int nrep, Tensor coef, Tensor target) -> (Tensor, Tensor, Tensor, Tensor)'
    with pytest.raises(RuntimeError, match='no CPU'):
        ns.score_rows(torch.zeros(4, 3, 16), 2, 2, torch.zeros(2, 4), torch.zeros(2, 3, dtype=torch.int32))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        out = ns.score_rows(torch.empty(4, 3, 16, device='cuda'), 2, 2, torch.empty(2, 4, device='cuda'), torch.empty(2, 3, dtype=torch.int32, device='cuda'))
        assert [tuple(t.shape) for t in out] == [(2, 3)] * 4 and [t.dtype for t in out] == [torch.float32, torch.float32, torch.int32, torch.int32]


# --------------------------------------------------------------------------------------------------------------- the reference
def random_rows(rng, n, V, std, nrep=2):
    lg = (rng.standard_normal((nrep, n, 1, V)) * std).astype(f32)
    coef = np.zeros((n, 4), dtype=f32)
    g = rng.uniform(0.0, 4.0, size=n)
    coef[:, 0], coef[:, 1] = 1 + g, -g                            # cfg weights up to 5 / -4
    if nrep == 4:
        coef[:, 2], coef[:, 3] = rng.uniform(-2, 2, size=n), rng.uniform(-2, 2, size=n)
    return lg, coef


def test_reference_equals_torch_log_softmax_in_float64():
    rng = np.random.default_rng(0)
    lg, coef = random_rows(rng, 40, 1000, 6.0, nrep=4)
    x = combine_f32(lg, coef, 1000)[:, 0]
    tgt = rng.integers(0, 1000, size=40)
    tgt[::7] = -1
    lp, ent, rank, am = score_ref(x, tgt)
    ls = torch.log_softmax(torch.from_numpy(x).double(), dim=-1)
    want = ls.gather(1, torch.from_numpy(np.maximum(tgt, 0))[:, None])[:, 0].numpy()
    assert np.abs(lp - np.where(tgt >= 0, want, 0.0)).max() < 1e-12
    assert np.abs(ent - (-(ls.exp() * ls).sum(dim=1)).numpy()).max() < 1e-12
    order = np.argsort(-x, axis=1, kind='stable')                  # descending, lowest index first among equals
    pos = np.array([int(np.where(order[i] == max(tgt[i], 0))[0][0]) for i in range(40)])
    assert np.array_equal(rank, np.where(tgt >= 0, pos, -1)) and np.array_equal(am, order[:, 0])
    # the combine: fp32 products rounded one by one, added in order
    b = 3
    want = f32(f32(f32(coef[b, 0] * lg[0, b, 0]) + f32(coef[b, 1] * lg[1, b, 0])) + f32(coef[b, 2] * lg[2, b, 0])) + f32(coef[b, 3] * lg[3, b, 0])
    assert x[b].tobytes() == want.astype(f32).tobytes()


def test_rank_counts_exact_ties_at_the_target_by_index_and_minus_inf_carries_no_mass():
    x = np.array([[2, 5, 5, 1, 5, 2, -np.inf, 2]], dtype=f32)
    for t, want in ((1, 0), (2, 1), (4, 2), (0, 3), (5, 4), (7, 5), (3, 6), (6, 7)):
        lp, ent, rank, am = score_ref(x, np.array([t]))
        assert rank[0] == want and am[0] == 1, t
        assert np.isfinite(ent[0]) and (np.isneginf(lp[0]) if t == 6 else np.isfinite(lp[0]))
    lp, ent, rank, am = score_ref(x, np.array([-1]))
    assert lp[0] == 0.0 and rank[0] == -1 and am[0] == 1


# --------------------------------------------------------------------------------------------------------------- the kernel's order, emulated
def emulate(x, tgt):
    """cvar_score_rows' order of evaluation in numpy float32 on combined rows x (n, V): thread tid owns elements tid + 256 j and adds them in
    increasing j, a 64-lane xor-shuffle tree, the four wave partials in order 0..3 -> (logprob, entropy) float32"""
    n, V = x.shape
    pad = np.full((n, 4096), -np.inf, dtype=f32)
    pad[:, :V] = x
    m = pad.max(axis=1)
    with np.errstate(invalid='ignore'):
        d = (pad - m[:, None]).astype(f32).reshape(n, 16, 256)    # [j][tid]
        ex = np.exp(d).astype(f32)
        term = np.where(ex != 0, (ex * d).astype(f32), f32(0))
    s, u = np.zeros((n, 256), dtype=f32), np.zeros((n, 256), dtype=f32)
    for j in range(16):
        s, u = (s + ex[:, j]).astype(f32), (u + term[:, j]).astype(f32)
    lane = np.arange(64)
    s, u = s.reshape(n, 4, 64), u.reshape(n, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        s, u = (s + s[:, :, lane ^ o]).astype(f32), (u + u[:, :, lane ^ o]).astype(f32)
    S = (((s[:, 0, 0] + s[:, 1, 0]).astype(f32) + s[:, 2, 0]).astype(f32) + s[:, 3, 0]).astype(f32)
    U = (((u[:, 0, 0] + u[:, 1, 0]).astype(f32) + u[:, 2, 0]).astype(f32) + u[:, 3, 0]).astype(f32)
    logS = np.log(S).astype(f32)
    xt = x[np.arange(n), tgt]
    return ((xt - m).astype(f32) - logS).astype(f32), (logS - (U / S).astype(f32)).astype(f32)


def test_an_emulation_of_the_kernels_order_stays_inside_the_bounds():
    """3000 rows: V in {4096, 1000, 257, 255, 1}, standard deviations 0.5 to 20, cfg weights up to 5 / -4, targets random and at the row minimum"""
    rng = np.random.default_rng(1)
    worst = [0.0, 0.0]
    for V in (4096, 1000, 257, 255, 1):
        for std in (0.5, 2.0, 6.0, 20.0):
            n = 150
            lg, coef = random_rows(rng, n, V, std)
            x = combine_f32(lg, coef, V)[:, 0]
            for tgt in (rng.integers(0, V, size=n), x.argmin(axis=1)):
                lp, ent = emulate(x, tgt)
                ref_lp, ref_ent, _, _ = score_ref(x, tgt)
                a, b = within_bounds(lp, ent, ref_lp, ref_ent)
                worst = [max(worst[0], a), max(worst[1], b)]
    print(f'[score] emulation: worst logprob error {worst[0]:.3f} of its bound, worst entropy error {worst[1]:.3f} of its bound')
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst


# --------------------------------------------------------------------------------------------------------------- TokenScores
@pytest.mark.parametrize('pns', [PN, PN512], ids=['S16', 'S32'])
@pytest.mark.parametrize('mask_first', [True, False])
def test_per_scale_and_total_against_hand_sums(pns, mask_first):
    B, mf = 2, 2
    L = mf * sum(pn * pn for pn in pns)
    g = torch.Generator().manual_seed(3)
    lp = -torch.rand(B, L, generator=g)
    sampled = torch.rand(B, L, generator=g) < 0.5
    ts = models.TokenScores(lp, lp * 2, torch.arange(B * L, dtype=torch.int32).view(B, L), torch.zeros(B, L, dtype=torch.int32), pns, mf, mask_first,
                            sampled=sampled)
    want = {k: np.zeros(B) for k in ('all', 'control', 'image', 'control_sampled')}
    o, scales = 0, ts.per_scale()
    assert len(scales) == len(pns)
    for pn, sc in zip(pns, scales):
        n = pn * pn
        assert tuple(sc.logprob.shape) == (B, 2 * n) and torch.equal(sc.logprob, lp[:, o:o + 2 * n]) and torch.equal(sc.rank, ts.rank[:, o:o + 2 * n])
        assert torch.equal(sc.sampled, sampled[:, o:o + 2 * n]) and torch.equal(sc.entropy, ts.entropy[:, o:o + 2 * n])
        first, second = ('control', 'image') if mask_first else ('image', 'control')
        for b in range(B):
            for t in range(2 * n):
                half = first if t < n else second
                v = float(lp[b, o + t])
                want['all'][b] += v
                want[half][b] += v
                if half == 'control' and bool(sampled[b, o + t]):
                    want['control_sampled'][b] += v
        o += 2 * n
    assert o == L
    tot = ts.total()
    assert tot.dtype == torch.float64 and tuple(tot.shape) == (B,)
    for got, key in ((tot, 'all'), (ts.total(half='control'), 'control'), (ts.total(half='image'), 'image'),
                     (ts.total(half='control', sampled_only=True), 'control_sampled')):
        assert np.allclose(got.numpy(), want[key], rtol=0, atol=1e-9), key
    assert np.allclose((ts.total(half='control') + ts.total(half='image')).numpy(), tot.numpy(), atol=1e-9)
    with pytest.raises(ValueError, match="half="):
        ts.total(half='both')
    # a token nobody asks for may hold -inf without poisoning a sum it is not part of
    lp2 = lp.clone()
    lp2[0, 0] = float('-inf')
    ts2 = models.TokenScores(lp2, lp, ts.rank, ts.argmax, pns, mf, mask_first)
    assert bool(torch.isfinite(ts2.total(half='image' if mask_first else 'control')).all()) and bool(ts2.sampled.all())


def test_a_plain_model_has_the_image_half_only():
    L = sum(pn * pn for pn in PN)
    lp = -torch.ones(1, L)
    ts = models.TokenScores(lp, lp, lp.int(), lp.int(), PN, 1, True, sampled=torch.zeros(L, dtype=torch.bool))
    assert float(ts.total()) == float(ts.total(half='image')) == -L and float(ts.total(sampled_only=True)) == 0.0
    assert tuple(ts.sampled.shape) == (1, L) and not bool(ts.sampled.any())
    with pytest.raises(ValueError, match='image half only'):
        ts.total(half='control')


# --------------------------------------------------------------------------------------------------------------- refusals, in words
@pytest.fixture(scope='module')
def model():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    return models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True)


LABELS, TYPES = torch.tensor([1, 2]), torch.tensor([0, 1])


def some_ids(B=2, pns=PN):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 4096, (B, pn * pn), generator=g) for pn in pns]


def test_logprobs_applies_the_refusals_of_per_request_mode(model):
    with pytest.raises(NotImplementedError, match='more_smooth is not offered'):
        model.autoregressive_infer_cfg(2, LABELS, cond_type=TYPES, more_smooth=True, logprobs=True)
    with pytest.raises(NotImplementedError, match='more_smooth is not offered'):
        model.edit_infer_cfg(2, LABELS, TYPES, more_smooth=True, logprobs=True)
    model.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
            model.autoregressive_infer_cfg(2, LABELS, cond_type=TYPES, logprobs=True)
        with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
            model.score_infer_cfg(2, LABELS, TYPES, ids_img=some_ids(), ids_ctrl=some_ids())
        with pytest.raises(NotImplementedError, match="sampler='torch'"):
            model.graphed_generator(2, per_request=True, logprobs=True)
    finally:
        model.sampler = 'counter'
    for kw in (dict(label_B=None, cond_type=TYPES), dict(label_B=LABELS, cond_type=None)):
        with pytest.raises(ValueError, match='must be given per row'):
            model.autoregressive_infer_cfg(2, kw['label_B'], cond_type=kw['cond_type'], logprobs=True)
        with pytest.raises(ValueError, match='must be given per row'):
            model.conditional_infer_cfg(2, kw['label_B'], cond_type=kw['cond_type'], logprobs=True)
        with pytest.raises(ValueError, match='must be given per row'):
            model.score_infer_cfg(2, kw['label_B'], kw['cond_type'], ids_img=some_ids(), ids_ctrl=some_ids())


def test_graphs_refuse_logprobs_without_per_request_before_anything_is_captured(model):
    with pytest.raises(ValueError, match='logprobs=True needs per_request=True'):
        model.graphed_generator(2, logprobs=True)
    with pytest.raises(ValueError, match='logprobs=True needs per_request=True'):
        model.graphed_conditional_generator(2, logprobs=True)


def test_separator_and_two_pass_models_are_refused():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    sep = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, separator=True)
    with pytest.raises(NotImplementedError, match='token log-probabilities: separator models are not offered'):
        sep.autoregressive_infer_cfg(2, LABELS, cond_type=TYPES, logprobs=True)
    with pytest.raises(NotImplementedError, match='token log-probabilities: separator models are not offered'):
        sep.score_infer_cfg(2, LABELS, TYPES, ids_img=some_ids(), ids_ctrl=some_ids())
    with pytest.raises(NotImplementedError, match='token log-probabilities: separator models are not offered'):
        sep.graphed_generator(2, per_request=True, logprobs=True)
    with pytest.raises(NotImplementedError, match='separator'):
        sep.graphed_conditional_generator(2, per_request=True, logprobs=True)
    with pytest.raises(NotImplementedError, match='separator models are not offered'):
        sep.edit_infer_cfg(2, LABELS, TYPES, logprobs=True)
    two = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, separate_decoding=True)
    with pytest.raises(NotImplementedError, match='two-pass separate_decoding branch'):
        two.autoregressive_infer_cfg(2, LABELS, cond_type=TYPES, logprobs=True)
    with pytest.raises(NotImplementedError, match='two-pass separate_decoding branch'):
        two.score_infer_cfg(2, LABELS, TYPES, ids_img=some_ids(), ids_ctrl=some_ids())
    with pytest.raises(NotImplementedError, match='two-pass separate_decoding branch'):
        two.graphed_generator(2, per_request=True, logprobs=True)


def test_score_infer_cfg_checks_ids_shapes_and_keywords_on_the_host(model):
    ids = some_ids()
    with pytest.raises(ValueError, match="given='both'"):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=ids, given='both')
    with pytest.raises(ValueError, match='ids_ctrl: the control half is scored too'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids)
    with pytest.raises(ValueError, match='ids_img: expected 10 id tensors'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids[:-1], ids_ctrl=ids)
    with pytest.raises(ValueError, match='ids_ctrl: expected integer ids of shape'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=torch.cat(ids, dim=1).float())
    bad = [t.clone() for t in ids]
    bad[3][1, 2] = 4096
    with pytest.raises(IndexError, match='ids_img: index out of range'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=bad, ids_ctrl=ids)
    with pytest.raises(ValueError, match='mask_first=False: only a bidirectional model'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=ids, mask_first=False)
    with pytest.raises(ValueError, match='triple'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=ids, given='control', cfg=[1.0, 2.0])
    with pytest.raises(ValueError, match='one per batch row'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=ids, cfg=[1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match='no bank attached'):
        model.score_infer_cfg(2, LABELS, TYPES, ids_img=ids, ids_ctrl=ids, adapter=0)


def test_plain_var_scores_the_image_half_only():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_var(vae, depth=2)
    with pytest.raises(ValueError, match='label_B must be given per row'):
        m.score_infer_cfg(2, None, ids_img=some_ids())
    with pytest.raises(ValueError, match='ids_img: expected 10 id tensors'):
        m.score_infer_cfg(2, LABELS, ids_img=some_ids()[1:])
