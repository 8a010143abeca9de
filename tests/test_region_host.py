"""Regional guidance, host side (no GPU; DESIGN.md 4l, include/cvar_region.h): the eighth header against its ctypes table and the library's exports,
the statuses its entry points return without a launch, every refusal of region_infer_cfg / graphed_region_generator in words, the K-label row
layout, and the weight rule - tests/region_ref.py's float64 restatement against _request_table (bit for bit at K = 1, uniform) and against the
library's own host statement of the rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import region_ref as R
from controlvar_amd import _lib, models
from controlvar_amd.spec import DEFAULT_PATCH_NUMS as PN, PATCH_NUMS_512 as PN512

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4096
NAMES = ['cvar_region_coef_table', 'cvar_cfg_sample_map', 'cvar_score_map']


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.load()


def _declarations(header):
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    return {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'\b(cvar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src)}


# ------------------------------------------------------------------------------------------------ the ABI
def test_entry_points_are_declared_exported_and_bound(lib):
    from controlvar_amd import build, ops
    decl = _declarations('cvar_region.h')
    assert list(decl) == NAMES == list(_lib.REGION_SIGNATURES)
    for table in (_lib.SIGNATURES, _lib.SERVE_SIGNATURES, _lib.ACCUM_SIGNATURES, _lib.KVCACHE_SIGNATURES, _lib.WIDE_SIGNATURES, _lib.POLICY_SIGNATURES,
                  _lib.DISTILL_SIGNATURES):
        assert not set(NAMES) & set(table)

    def ctype(d):
        if d.startswith('const int*'):
            return C.POINTER(_lib.c_i)                           # the host array of scale sizes
        return _lib.c_p if '*' in d else {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[re.sub(r'\s+', ' ', d).rsplit(' ', 1)[0]]
    for name in NAMES:
        res, argtypes = _lib.REGION_SIGNATURES[name]
        assert res is _lib.c_i and argtypes == [ctype(d) for d in decl[name]], name
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
    assert _lib.ABI_VERSION == lib.cvar_abi_version() and _lib.SERVE_VERSION == 1 == lib.cvar_serve_version()
    assert set(_declarations('cvar.h')) == set(_lib.SIGNATURES) and set(_declarations('cvar_serve.h')) == set(_lib.SERVE_SIGNATURES)
    assert 'region.hip' in build.SOURCES and all(callable(getattr(ops, n)) for n in ('region_coef_table', 'cfg_sample_map', 'score_map'))


def test_the_library_refuses_without_a_launch(lib):
    """64 is a non-NULL, 16-byte aligned address that is never dereferenced: every call returns on the host"""
    one = 64
    pns = (C.c_int * 10)(*PN)
    targs = dict(regions=one, strength=one, cfg=one, pns=pns, nstage=10, B=2, K=2, S=16, mask_first=1, mf=2, coef=one, stream=None)

    def table(**kw):
        return lib.cvar_region_coef_table(*{**targs, **kw}.values())
    for bad in (dict(K=0), dict(K=4), dict(K=-1), dict(regions=None), dict(coef=None), dict(cfg=None), dict(pns=None), dict(B=0), dict(B=-3), dict(S=0),
                dict(nstage=17), dict(nstage=1), dict(nstage=0), dict(S=15), dict(S=32), dict(pns=(C.c_int * 10)(*([0] + list(PN[1:]))))):
        assert table(**bad) == -1, bad                            # CVAR_EINVAL
    for bad in (dict(mf=0), dict(mf=3), dict(coef=68), dict(B=1 << 22)):
        assert table(**bad) == -2, bad                            # CVAR_EUNSUPPORTED

    sargs = dict(logits=one, B=2, nrep=3, l=3, V=V, coef=one, ldc=3, top_k=one, top_p=one, seed=one, stage=0, n_draw=1, idx=one, comb=None, mg=None,
                 kept=None, ldv=0, expo=None, soft=None, forced=None, ldf=0, stream=None)

    def sample(**kw):
        return lib.cvar_cfg_sample_map(*{**sargs, **kw}.values())
    for name in ('logits', 'coef', 'top_k', 'top_p', 'seed', 'idx'):
        assert sample(**{name: None}) == -1, name
    assert sample(B=0) == -1 and sample(l=0) == -1 and sample(V=1) == -1 and sample(ldv=V - 1) == -1 and sample(ldc=2) == -1
    assert sample(forced=one, ldf=2) == -1
    for bad in (dict(nrep=0), dict(nrep=5), dict(n_draw=0), dict(n_draw=5), dict(V=V + 1), dict(expo=one), dict(soft=one)):
        assert sample(**bad) == -2, bad

    cargs = dict(logits=one, B=2, nrep=3, l=3, V=V, coef=one, ldc=3, target=one, ldt=3, comb=None, lp=one, ent=None, rank=None, am=None, ldo=0, ldv=0,
                 stream=None)

    def score(**kw):
        return lib.cvar_score_map(*{**cargs, **kw}.values())
    for bad in (dict(logits=None), dict(coef=None), dict(target=None), dict(lp=None), dict(B=0), dict(l=0), dict(V=0), dict(ldt=2), dict(ldc=2),
                dict(ldo=2), dict(ldv=V - 1)):
        assert score(**bad) == -1, bad
    for bad in (dict(nrep=0), dict(nrep=5), dict(V=V + 1)):
        assert score(**bad) == -2, bad


# ------------------------------------------------------------------------------------------------ the weight rule
@pytest.mark.parametrize('pns', [PN, PN512], ids=['S16', 'S32'])
@pytest.mark.parametrize('mf', [1, 2])
def test_one_label_uniform_maps_are_the_per_request_table_bit_for_bit(pns, mf):
    """K = 1, regions all ones, no strength: every token of stage si holds _request_table's [1 + t, -t, 0, 0] of that stage - for the restatement
    and for the library's host function"""
    B, S, cfgs = 3, pns[-1], [1.5, 4.0, 0.3]
    want = models._request_table(B, cfgs, 0, 0.0, 0, False, V, len(pns)).coef.numpy()               # (nstage, B, 4) fp32
    ones = np.ones((B, 1, S, S), dtype=np.float32)
    cf = np.array(cfgs, dtype=np.float64)[:, None]
    ref, pure = R.coef_ref(ones, None, cf, pns, mf)
    host = models.region_coef_reference(ones, None, cf, pns, mf)
    assert pure.all() and host.dtype == np.float32 and host.shape == ref.shape
    o = 0
    for si, pn in enumerate(pns):
        n = mf * pn * pn
        for name, got in (('restatement', ref[:, o:o + n].astype(np.float32)), ('host function', host[:, o:o + n])):
            assert np.array_equal(got.view(np.int32), np.broadcast_to(want[si][:, None], (B, n, 4)).view(np.int32)), (name, si)
        o += n
    assert o == ref.shape[1]


@pytest.mark.parametrize('K', [1, 2, 3])
def test_the_host_function_follows_the_restatement(K):
    """general maps with a strength map: the library's host statement of the rule (plain float64 sums) within 1 fp32 ulp of the fsum restatement,
    pure bins exact; the weights of a token sum to 1 where they are exact enough to say so"""
    B, S = 2, 16
    w = R.region_maps(B, K, S, 7 + K)
    st = np.random.default_rng(3).random((B, S, S), dtype=np.float32) * 2
    cf = np.array([[1.5, 3.0, 0.0], [4.0, 0.5, 2.0]])[:, :K]
    ref, pure = R.coef_ref(w, st, cf, PN, 2)
    got = models.region_coef_reference(w, st, cf, PN, 2)
    assert float(R.ulps(got, ref).max()) <= 1.0
    assert pure[1].all() if K == 1 else (pure[1].any() and not pure[1].all())
    assert np.abs(ref.sum(axis=2) - 1.0).max() < 1e-12           # sum_k wbar_k (1 + t_k) - sum_k wbar_k t_k = sum_k wbar_k = 1


# ------------------------------------------------------------------------------------------------ refusals, in words
@pytest.fixture(scope='module')
def model():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    return models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True)


LAB, TY = torch.tensor([[1, 2], [3, 4]]), torch.tensor([0, 1])


def maps(B=2, K=2, S=16):
    return torch.ones(B, K, S, S)


def test_wrong_shapes_are_refused(model):
    for bad in (torch.tensor([1, 2]), torch.tensor([[1, 2]]), torch.tensor([[1.0, 2.0], [3.0, 4.0]]), torch.zeros(2, 2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match='labels: integer class labels of shape'):
            model.region_infer_cfg(2, bad, TY, regions=maps())
    with pytest.raises(ValueError, match='labels: K = 4 labels per sample'):
        model.region_infer_cfg(2, torch.zeros(2, 4, dtype=torch.int64), TY, regions=maps(K=4))
    with pytest.raises((IndexError, ValueError, RuntimeError), match='labels'):
        model.region_infer_cfg(2, torch.tensor([[1, 2], [3, 5000]]), TY, regions=maps())
    for bad in (maps(K=1), maps(K=3), maps(B=3), maps(S=32), torch.ones(2, 2, 16, 15), torch.ones(2, 16, 16), maps().long(), 'maps', None):
        with pytest.raises(ValueError, match=r'regions: a floating-point tensor of shape \(2, 2, 16, 16\)'):
            model.region_infer_cfg(2, LAB, TY, regions=bad)
    for bad in (torch.ones(2, 16, 15), torch.ones(2, 2, 16, 16), torch.ones(16, 16), torch.ones(2, 16, 16, dtype=torch.int32), 1.0):
        with pytest.raises(ValueError, match=r'strength: None or a floating-point tensor of shape \(2, 16, 16\)'):
            model.region_infer_cfg(2, LAB, TY, regions=maps(), strength=bad)
    for bad in ([1.0, 2.0, 3.0], np.ones((2, 3)), np.ones((3, 2)), np.ones((2, 2, 1))):
        with pytest.raises(ValueError, match=r'cfg: a scalar, shape \(2,\)'):
            model.region_infer_cfg(2, LAB, TY, regions=maps(), cfg=bad)
    with pytest.raises(ValueError, match='cfg: numbers expected'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), cfg=['a', 'b'])


def test_bad_values_are_refused(model):
    for v in (-1.0, float('nan'), float('inf')):
        bad = maps(); bad[1, 0, 3, 4] = v
        with pytest.raises(ValueError, match='regions: finite, non-negative weights'):
            model.region_infer_cfg(2, LAB, TY, regions=bad)
        bad = torch.ones(2, 16, 16); bad[0, 5, 5] = v
        with pytest.raises(ValueError, match='strength: finite, non-negative factors'):
            model.region_infer_cfg(2, LAB, TY, regions=maps(), strength=bad)
    empty = maps(); empty[0, :, 7, 9] = 0.0
    with pytest.raises(ValueError, match='a latent cell whose weights sum to 0'):
        model.region_infer_cfg(2, LAB, TY, regions=empty)
    for bad in (float('nan'), float('inf'), [1.5, float('nan')], [[1.0, 2.0], [float('-inf'), 0.0]]):
        with pytest.raises(ValueError, match='cfg: finite guidance scales'):
            model.region_infer_cfg(2, LAB, TY, regions=maps(), cfg=bad)


def test_modes_that_are_not_offered_are_refused_in_words(model):
    with pytest.raises(NotImplementedError, match='regional guidance: more_smooth is not offered'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), more_smooth=True)
    with pytest.raises(NotImplementedError, match=r'region_infer_cfg: cfg=None .* is not offered here'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), cfg=None)
    with pytest.raises(NotImplementedError, match='regional guidance: the four-branch conditional call'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), given='control')
    model.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
            model.region_infer_cfg(2, LAB, TY, regions=maps())
        with pytest.raises(NotImplementedError, match='graphed_region_generator captures the counter sampler only'):
            model.graphed_region_generator(2, 2)
    finally:
        model.sampler = 'counter'
    with pytest.raises(ValueError, match='must be given per row'):
        model.region_infer_cfg(2, LAB, None, regions=maps())
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    for kw, words in ((dict(separate_decoding=True), 'regional guidance: separate_decoding models are not offered'),
                      (dict(separator=True), 'regional guidance: separator models are not offered')):
        m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, **kw)
        with pytest.raises(NotImplementedError, match=words):
            m.region_infer_cfg(2, LAB, TY, regions=maps())
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, bidirectional=True)
    with pytest.raises(NotImplementedError, match='the captured generator fixes the .* order'):
        m.graphed_region_generator(2, 2)
    for K in (0, 4, 1.5):
        with pytest.raises(ValueError, match='labels per sample'):
            model.graphed_region_generator(2, K)


def test_the_request_table_and_the_edit_halves_refuse_as_they_do_elsewhere(model):
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), top_k=[1, V + 1])
    with pytest.raises(ValueError, match='one per batch row'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), g_seed=[1, 2, 3])
    with pytest.raises(ValueError, match='keep_img is given without src_img'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), keep_img=torch.zeros(2, 16, 16, dtype=torch.bool))
    with pytest.raises(ValueError, match=r'keep_ctrl: True, None or a bool tensor of shape \(2, 16, 16\)'):
        model.region_infer_cfg(2, LAB, TY, regions=maps(), src_ctrl=[torch.zeros(2, pn * pn, dtype=torch.int64) for pn in PN], keep_ctrl=torch.ones(2, 16, 16))


def test_plain_var_has_the_image_half_only():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_var(vae, depth=2)
    with pytest.raises(TypeError):
        m.region_infer_cfg(2, LAB, regions=maps(), src_ctrl=[], keep_ctrl=True)
    with pytest.raises(ValueError, match='a latent cell whose weights sum to 0'):
        m.region_infer_cfg(2, LAB, regions=torch.zeros(2, 2, 16, 16))


def test_the_rows_of_a_sample_are_its_labels_then_the_unconditional_row(model):
    """[label_0 rows ; ... ; label_{K-1} rows ; unconditional rows], each block B rows; the sample's condition type on the conditional blocks, 4 below"""
    lab = torch.tensor([[1, 2, 3], [4, 5, 6]])
    la, ta = model._prepare_rows(2, lab, TY, False, 0, None, K=3)
    assert la.tolist() == [1, 4, 2, 5, 3, 6, model.num_classes, model.num_classes] and ta.tolist() == [0, 1, 0, 1, 0, 1, 4, 4]
    la, ta = model._prepare_rows(2, lab[:, :1], TY, False, 0, 2, K=1)
    la2, ta2 = model._prepare_rows(2, lab[:, 0], TY, False, 0, 2)
    assert torch.equal(la, la2) and torch.equal(ta, ta2)          # K = 1 is the joint call's [cond ; uncond]
