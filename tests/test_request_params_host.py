"""Per-request sampling parameters, host side (no GPU): the second header include/cvar_serve.h and its ctypes table, the host-built
request table (models._request_table), the refusals of per-request mode in words, and the cvar::cfg_sample_rows op's schema and fake kernel."""
import os
import re

import numpy as np
import pytest
import torch

from controlvar_amd import _lib, models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, NSTAGE = 4096, 10


def serve_symbols():
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'cvar_serve.h')).read(), flags=re.S)
    return sorted(set(re.findall(r'\b(cvar_[a-z0-9_]+)\s*\(', src)))


def test_every_serve_header_symbol_is_exported_and_bound_in_its_own_table():
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    lib = _lib.load()
    syms = serve_symbols()
    assert 'cvar_cfg_sample_rows' in syms and 'cvar_serve_version' in syms
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cvar_serve.h but not exported'
    assert set(_lib.SERVE_SIGNATURES) == set(syms)
    assert not set(_lib.SERVE_SIGNATURES) & set(_lib.SIGNATURES)
    assert lib.cvar_serve_version() == 1 == _lib.SERVE_VERSION
    assert lib.cvar_cfg_sample_rows.argtypes == _lib.SERVE_SIGNATURES['cvar_cfg_sample_rows'][1]        # load() bound the second table
    text = open(os.path.join(ROOT, 'include', 'cvar_serve.h')).read()
    assert 'entry points with no counterpart in the reference' in text


def test_null_tables_and_unsupported_arguments_return_a_status_without_a_launch():
    lib = _lib.load()
    one = 8                                                       # any non-null address: nothing is launched on these paths
    args = dict(logits=one, B=2, nrep=2, l=3, V=V, coef=one, top_k=one, top_p=one, seed=one, stage=0, n_draw=1, idx=one, comb=None, mg=None, kept=None,
                ldv=0, expo=None, soft=None, stream=None)

    def call(**kw):
        return lib.cvar_cfg_sample_rows(*{**args, **kw}.values())
    for table in ('logits', 'coef', 'top_k', 'top_p', 'seed', 'idx'):
        assert call(**{table: None}) == -1, table                 # CVAR_EINVAL
    assert call(B=0) == -1 and call(l=0) == -1 and call(V=1) == -1 and call(ldv=V - 1) == -1
    for bad in (dict(nrep=0), dict(nrep=5), dict(n_draw=0), dict(n_draw=5), dict(V=V + 1), dict(expo=one), dict(soft=one)):
        assert call(**bad) == -2, bad                             # CVAR_EUNSUPPORTED


# --------------------------------------------------------------------------------------------------------------- the request table
def table(B, cfg=1.5, top_k=0, top_p=0.0, g_seed=0, four_way=False):
    return models._request_table(B, cfg, top_k, top_p, g_seed, four_way, V, NSTAGE)


def test_scalars_broadcast_and_sequences_arrays_tensors_are_taken_per_row():
    t = table(3, cfg=2.0, top_k=900, top_p=0.96, g_seed=7)
    assert t.seed.tolist() == [7, 7, 7] and t.top_k.tolist() == [900] * 3
    assert t.top_p.dtype == torch.float32 and torch.equal(t.top_p, torch.full((3,), 0.96, dtype=torch.float32))
    assert t.coef.shape == (NSTAGE, 3, 4)
    t = table(3, cfg=[1.0, 2.5, 4.0], top_k=np.array([1, 0, 50]), top_p=torch.tensor([0.0, 0.5, 1.0]), g_seed=(5, 2 ** 64 + 6, -1))
    assert t.top_k.tolist() == [1, 0, 50] and t.top_k.dtype == torch.int32
    assert t.top_p.tolist() == [0.0, 0.5, 1.0]
    assert t.seed.dtype == torch.int64 and t.seed.tolist() == [5, 6, -1]          # modulo 2^64, stored as the int64 bit pattern
    assert float(t.coef[9, 1, 0]) == 3.5 and float(t.coef[9, 2, 1]) == -4.0
    assert table(2, top_k=-5).top_k.tolist() == [-1, -1]
    assert table(2, top_k=V).top_k.tolist() == [V, V]


def test_no_seed_draws_one_host_seed_per_row():
    torch.manual_seed(0)
    a = table(4, g_seed=None).seed
    torch.manual_seed(0)
    b = table(4, g_seed=None).seed
    assert torch.equal(a, b) and len(set(a.tolist())) == 4


@pytest.mark.parametrize('four_way', [False, True])
def test_coefficients_are_the_fp32_roundings_of_the_eager_expressions(four_way):
    B = 3
    cfgs = [(3.0, 2.0, 1.0), (1.5, 1.5, 1.5), (0.1, 7.3, 2.9)] if four_way else [1.5, 0.1, 7.3]
    t = table(B, cfg=cfgs, four_way=four_way)
    for si in range(NSTAGE):
        ratio = si / (NSTAGE - 1)                                 # _generate_core's expressions, in python doubles
        for b in range(B):
            if four_way:
                t1, t2, t3 = [c * ratio for c in cfgs[b]]
                coef = [1 + t1, t2 - t1, t3 - t2, -t3]
            else:
                s = cfgs[b] * ratio
                coef = [1 + s, -s, 0.0, 0.0]
            want = np.array(coef, dtype=np.float64).astype(np.float32)
            assert t.coef[si, b].numpy().tobytes() == want.tobytes(), (si, b)
    # one triple is the scalar form of the four-branch guidance
    if four_way:
        one = table(B, cfg=(3.0, 2.0, 1.0), four_way=True)
        assert torch.equal(one.coef[:, 1], t.coef[:, 0]) and torch.equal(one.coef[:, 2], t.coef[:, 0])
        as_array = table(B, cfg=torch.tensor(cfgs, dtype=torch.float64), four_way=True)
        assert torch.equal(as_array.host, t.host)


def test_the_table_is_one_contiguous_buffer():
    B = 5
    t = table(B, cfg=[1.0, 2.0, 3.0, 4.0, 5.0], top_k=[1, 2, 3, 4, 5], top_p=0.5, g_seed=[9, 8, 7, 6, 5])
    assert t.host.dtype == torch.uint8 and t.host.is_contiguous() and t.host.numel() == 8 * B + 4 * B + 4 * B + 16 * NSTAGE * B
    base = t.host.data_ptr()
    assert [v.data_ptr() - base for v in (t.seed, t.top_k, t.top_p, t.coef)] == [0, 8 * B, 12 * B, 16 * B]
    assert all(v.is_contiguous() for v in (t.seed, t.top_k, t.top_p, t.coef, t.coef[3]))
    copy = t.host.clone()                                         # what one host-to-device copy moves: views of the copy read the same values
    seed, top_k, top_p, coef = t.views(copy)
    assert seed.tolist() == [9, 8, 7, 6, 5] and top_k.tolist() == [1, 2, 3, 4, 5] and torch.equal(coef, t.coef) and torch.equal(top_p, t.top_p)


def test_wrong_lengths_and_shapes_raise_value_error_and_large_top_k_runtime_error():
    for bad in (dict(cfg=[1.0, 2.0]), dict(top_k=[1, 2, 3, 4]), dict(top_p=np.zeros((3, 1))), dict(g_seed=[1, 2]), dict(cfg=np.ones((3, 3))),
                dict(top_k=[1.5, 2, 3]), dict(g_seed=[1.0, 2.0, 3.0]), dict(cfg=['a', 'b', 'c'])):
        with pytest.raises(ValueError):
            table(3, **bad)
    for bad in (dict(cfg=1.5), dict(cfg=[1.0, 2.0, 3.0, 4.0]), dict(cfg=np.ones((2, 3))), dict(cfg=np.ones((3, 2)))):
        with pytest.raises(ValueError, match='triple'):
            table(3, four_way=True, **bad)
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        table(3, top_k=[1, V + 1, 0])
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        table(3, top_k=V + 1)


def test_per_request_mode_is_entered_by_any_non_scalar_parameter():
    pr = models._per_request
    assert not pr(1.5, 0, 0.0, None, False) and not pr(np.float32(1.5), torch.tensor(5), 0.5, 3, False)
    assert not pr((1.5, 1.5, 1.5), 900, 0.96, 0, True) and not pr(torch.tensor([3.0, 2.0, 1.0]), 0, 0.0, None, True)
    assert pr([1.5, 2.0], 0, 0.0, None, False) and pr(1.5, [1, 2], 0.0, None, False) and pr(1.5, 0, torch.zeros(2), None, False)
    assert pr(1.5, 0, 0.0, [1, 2], False) and pr(np.ones((2, 3)), 0, 0.0, None, True) and pr((1.5, 1.5, 1.5), 0, 0.0, [1, 2], True)


# --------------------------------------------------------------------------------------------------------------- refusals, in words
@pytest.fixture(scope='module')
def model():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    return models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True)


ROWS = dict(cfg=[1.5, 2.0], top_k=[1, 900], top_p=[0.0, 0.96], g_seed=[1, 2])


def test_more_smooth_torch_sampler_and_missing_labels_are_refused_with_their_reason(model):
    labels, types = torch.tensor([1, 2]), torch.tensor([0, 1])
    with pytest.raises(NotImplementedError, match='more_smooth is not offered'):
        model.autoregressive_infer_cfg(2, labels, cond_type=types, more_smooth=True, **ROWS)
    model.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
            model.autoregressive_infer_cfg(2, labels, cond_type=types, **ROWS)
    finally:
        model.sampler = 'counter'
    for kw in (dict(label_B=None, cond_type=types), dict(label_B=labels, cond_type=None)):
        with pytest.raises(ValueError, match='must be given per row.*one batch seed'):
            model.autoregressive_infer_cfg(2, kw['label_B'], cond_type=kw['cond_type'], g_seed=[1, 2])
        with pytest.raises(ValueError, match='must be given per row.*one batch seed'):
            model.conditional_infer_cfg(2, kw['label_B'], cond_type=kw['cond_type'], cfg=[(3.0, 2.0, 1.0), (1.0, 1.0, 1.0)])
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        model.autoregressive_infer_cfg(2, labels, cond_type=types, top_k=[1, V + 1])
    with pytest.raises(ValueError, match='one per batch row'):
        model.autoregressive_infer_cfg(2, labels, cond_type=types, top_k=[1, 2, 3])


def test_the_two_pass_branch_is_refused():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, separate_decoding=True)
    with pytest.raises(NotImplementedError, match='two-pass separate_decoding branch'):
        m.autoregressive_infer_cfg(2, torch.tensor([1, 2]), cond_type=torch.tensor([0, 1]), g_seed=[1, 2])


def test_plain_var_names_only_the_labels():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_var(vae, depth=2)
    with pytest.raises(ValueError, match='label_B must be given per row'):
        m.autoregressive_infer_cfg(2, None, top_k=[1, 2])


def test_a_graph_captured_without_per_request_refuses_the_keywords():
    """what run() of a per_request=False graph calls first (the capture itself needs the device)"""
    models._refuse_request_keywords(None, {})
    models._refuse_request_keywords(5, {})
    with pytest.raises(TypeError, match='cfg, top_k.*per_request=False'):
        models._refuse_request_keywords(None, dict(top_k=[1, 2], cfg=2.0))
    with pytest.raises(ValueError, match='per_request=False'):
        models._refuse_request_keywords([1, 2], {})


# --------------------------------------------------------------------------------------------------------------- the torch op
def test_cfg_sample_rows_schema_and_fake_kernel():
    import controlvar_amd
    ns = controlvar_amd.register_torch_ops()
    from controlvar_amd import torch_ops
    assert 'cfg_sample_rows' in torch_ops.OPS
    assert str(ns.cfg_sample_rows.default._schema) == ('cvar::cfg_sample_rows(Tensor logits, int B, int nrep, Tensor coef, Tensor top_k, Tensor top_p, Tensor seed, '
                                                       'int stage, int n_draw=1) -> Tensor')
    B, l = 3, 7
    with pytest.raises(RuntimeError, match='no CPU'):
        ns.cfg_sample_rows(torch.zeros(2 * B, l, V), B, 2, torch.zeros(B, 4), torch.zeros(B, dtype=torch.int32), torch.zeros(B), torch.zeros(B, dtype=torch.int64), 0)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        lg = torch.empty(4 * B, l, V, device='cuda')
        coef, k = torch.empty(B, 4, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')
        p, s = torch.empty(B, device='cuda'), torch.empty(B, dtype=torch.int64, device='cuda')
        out = ns.cfg_sample_rows(lg, B, 4, coef, k, p, s, 2, 4)
        assert out.shape == (4 * B, l) and out.dtype == torch.int32
        assert ns.cfg_sample_rows(lg[:2 * B], B, 2, coef, k, p, s, 0).shape == (B, l)
