"""Region-constrained generation, host side (no GPU): the two entry points in include/cvar_serve.h and their ctypes table, the statuses they
return without a launch, every refusal of edit_infer_cfg in words, and the cell rule - which latent-resolution keep mask keeps which token of
which scale - restated here in python integers and checked against adaptive average pooling."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from controlvar_amd import _lib, models
from controlvar_amd.spec import DEFAULT_PATCH_NUMS, PATCH_NUMS_512

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 4096


# --------------------------------------------------------------------------------------------------------------- the ABI
def test_the_edit_entry_points_are_declared_exported_and_bound_and_the_version_stays_1():
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    lib = _lib.load()
    text = open(os.path.join(ROOT, 'include', 'cvar_serve.h')).read()
    syms = set(re.findall(r'\b(cvar_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', text, flags=re.S)))
    for s in ('cvar_edit_force_table', 'cvar_cfg_sample_edit'):
        assert s in syms, f'{s} is not declared in include/cvar_serve.h'
        assert hasattr(lib, s), f'{s} is not exported'
        assert s in _lib.SERVE_SIGNATURES and s not in _lib.SIGNATURES
        assert getattr(lib, s).argtypes == _lib.SERVE_SIGNATURES[s][1]
    # an added entry point changes no signature: the header's bump rule leaves the version alone, and the header says so
    assert lib.cvar_serve_version() == 1 == _lib.SERVE_VERSION
    assert 'joined at version 1' in text
    from controlvar_amd import ops
    assert callable(ops.edit_force_table) and callable(ops.cfg_sample_edit)


def test_null_and_unsupported_arguments_return_a_status_without_a_launch():
    import ctypes as C
    lib = _lib.load()
    one = 8                                                       # any non-null address: nothing is launched on these paths
    args = dict(logits=one, B=2, nrep=2, l=3, V=V, coef=one, top_k=one, top_p=one, seed=one, stage=0, n_draw=1, idx=one, comb=None, mg=None, kept=None,
                ldv=0, expo=None, soft=None, forced=one, ldf=3, stream=None)

    def sample(**kw):
        return lib.cvar_cfg_sample_edit(*{**args, **kw}.values())
    for table in ('logits', 'coef', 'top_k', 'top_p', 'seed', 'idx', 'forced'):
        assert sample(**{table: None}) == -1, table               # CVAR_EINVAL
    assert sample(B=0) == -1 and sample(l=0) == -1 and sample(V=1) == -1 and sample(ldv=V - 1) == -1 and sample(ldf=2) == -1
    for bad in (dict(nrep=0), dict(nrep=5), dict(n_draw=0), dict(n_draw=5), dict(V=V + 1), dict(expo=one), dict(soft=one)):
        assert sample(**bad) == -2, bad                           # CVAR_EUNSUPPORTED

    pns = (C.c_int * 10)(*DEFAULT_PATCH_NUMS)
    targs = dict(keep_ctrl=one, keep_img=one, src_ctrl=one, src_img=one, pns=pns, nstage=10, B=2, S=16, mask_first=1, mf=2, forced=one, stream=None)

    def table(**kw):
        return lib.cvar_edit_force_table(*{**targs, **kw}.values())
    for bad in (dict(forced=None), dict(pns=None), dict(B=0), dict(S=0), dict(nstage=0), dict(src_ctrl=None), dict(src_img=None), dict(S=15),
                dict(S=32), dict(mf=1), dict(pns=(C.c_int * 10)(*([0] + list(DEFAULT_PATCH_NUMS[1:]))))):
        assert table(**bad) == -1, bad                            # a mask without its source, a scale list that does not end at S, ...
    for bad in (dict(mf=0), dict(mf=3), dict(nstage=17)):
        assert table(**bad) == -2, bad


# --------------------------------------------------------------------------------------------------------------- the cell rule
def keep_cells(keep: torch.Tensor, pn: int) -> torch.Tensor:
    """(B, S, S) bool -> (B, pn * pn) bool: cell (i, j) covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns, and
    is kept iff twice the number of kept latent cells in that bin exceeds the bin's size (python integers throughout)"""
    B, S = keep.shape[0], keep.shape[-1]
    out = torch.zeros(B, pn * pn, dtype=torch.bool)
    for b in range(B):
        m = keep[b].tolist()
        for i in range(pn):
            r0, r1 = i * S // pn, -((-(i + 1) * S) // pn)
            for j in range(pn):
                c0, c1 = j * S // pn, -((-(j + 1) * S) // pn)
                n = sum(1 for r in range(r0, r1) for c in range(c0, c1) if m[r][c])
                out[b, i * pn + j] = 2 * n > (r1 - r0) * (c1 - c0)
    return out


def rule_masks(S: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(S)
    ms = [torch.rand(S, S, generator=g) < d for d in (0.1, 0.5, 0.9)]
    ms += [torch.ones(S, S, dtype=torch.bool), torch.zeros(S, S, dtype=torch.bool)]
    one_cell = torch.zeros(S, S, dtype=torch.bool); one_cell[S // 3, S - 2] = True
    one_row = torch.zeros(S, S, dtype=torch.bool); one_row[5] = True
    ii = torch.arange(S)
    checker = (ii[:, None] + ii[None, :]) % 2 == 0
    square = torch.zeros(S, S, dtype=torch.bool); square[S // 4:S - S // 4, S // 4:S - S // 4] = True
    return torch.stack(ms + [one_cell, one_row, checker, square])


@pytest.mark.parametrize('pns', [DEFAULT_PATCH_NUMS, PATCH_NUMS_512], ids=['S16', 'S32'])
def test_the_cell_rule_is_area_pooling_compared_with_one_half_exactly(pns):
    """the pooled means are multiples of 1 / (bin size) <= 1 / 1024, exact in float64, so `> 0.5` there is the integer majority"""
    S = pns[-1]
    keep = rule_masks(S)
    for pn in pns:
        want = (F.adaptive_avg_pool2d(keep.double()[:, None], pn)[:, 0] > 0.5).reshape(keep.shape[0], -1)
        got = keep_cells(keep, pn)
        assert torch.equal(got, want), pn
        if pn == S:
            assert torch.equal(got, keep.reshape(keep.shape[0], -1))          # the last scale is the mask itself
    checker = keep[7:8]
    for pn in pns:
        if S % pn == 0 and (S // pn) % 2 == 0:
            assert not keep_cells(checker, pn).any(), pn                       # exact halves stay free
    # the library's own host statement of the rule (what its documentation and its graphed generator's checks rest on) says the same
    for pn in pns:
        assert torch.equal(models.edit_keep_cells(keep, pn), keep_cells(keep, pn)), pn


# --------------------------------------------------------------------------------------------------------------- refusals, in words
@pytest.fixture(scope='module')
def model():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    return models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True)


def sources(B=2, pns=DEFAULT_PATCH_NUMS, fill=3):
    return [torch.full((B, pn * pn), fill, dtype=torch.int64) for pn in pns]


LAB, TY = torch.tensor([1, 2]), torch.tensor([0, 1])
KEEP = torch.zeros(2, 16, 16, dtype=torch.bool)


def test_more_smooth_torch_sampler_and_missing_labels_are_refused(model):
    with pytest.raises(NotImplementedError, match='more_smooth is not offered'):
        model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP, more_smooth=True)
    model.sampler = 'torch'
    try:
        with pytest.raises(NotImplementedError, match="sampler='torch' is not offered"):
            model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP)
    finally:
        model.sampler = 'counter'
    for lab, ty in ((None, TY), (LAB, None)):
        with pytest.raises(ValueError, match='must be given per row'):
            model.edit_infer_cfg(2, lab, ty, src_img=sources(), keep_img=KEEP)


def test_masks_of_the_wrong_shape_or_dtype_are_refused(model):
    for bad in (torch.zeros(2, 16, 15, dtype=torch.bool), torch.zeros(2, 32, 32, dtype=torch.bool), torch.zeros(3, 16, 16, dtype=torch.bool),
                torch.zeros(16, 16, dtype=torch.bool), torch.zeros(2, 16, 16), torch.zeros(2, 16, 16, dtype=torch.uint8), False, 'all', [[True]]):
        with pytest.raises(ValueError, match=r'keep_img: True, None or a bool tensor of shape \(2, 16, 16\)'):
            model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=bad)
        with pytest.raises(ValueError, match=r'keep_ctrl: True, None or a bool tensor of shape \(2, 16, 16\)'):
            model.edit_infer_cfg(2, LAB, TY, src_ctrl=sources(), keep_ctrl=bad)


def test_a_mask_without_its_source_is_refused(model):
    with pytest.raises(ValueError, match='keep_img is given without src_img'):
        model.edit_infer_cfg(2, LAB, TY, keep_img=KEEP)
    with pytest.raises(ValueError, match='keep_ctrl is given without src_ctrl'):
        model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP, keep_ctrl=True)


def test_sources_of_the_wrong_form_or_out_of_range_are_refused(model):
    short = sources()[:-1]
    wrong = sources(); wrong[3] = wrong[3][:, :-1]
    for bad in (short, wrong, sources(B=3), [t.float() for t in sources()], torch.zeros(2, 679, dtype=torch.int64), 'ids'):
        with pytest.raises(ValueError, match='src_img: expected'):
            model.edit_infer_cfg(2, LAB, TY, src_img=bad, keep_img=KEEP)
    for fill in (V, -1):
        with pytest.raises((IndexError, ValueError, RuntimeError), match='src_ctrl'):
            model.edit_infer_cfg(2, LAB, TY, src_ctrl=sources(fill=fill), keep_ctrl=True)
    big = sources(); big[9][1, 200] = V
    with pytest.raises((IndexError, ValueError, RuntimeError), match='src_img'):
        model.edit_infer_cfg(2, LAB, TY, src_img=big, keep_img=KEEP)


def test_per_request_tables_refuse_as_they_do_elsewhere(model):
    with pytest.raises(RuntimeError, match='selected index k out of range'):
        model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP, top_k=[1, V + 1])
    with pytest.raises(ValueError, match='one per batch row'):
        model.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP, g_seed=[1, 2, 3])


def test_the_two_pass_branch_and_separator_models_are_refused():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, separate_decoding=True)
    with pytest.raises(NotImplementedError, match='two-pass separate_decoding branch'):
        m.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP)
    m = models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, separator=True)
    with pytest.raises(NotImplementedError, match='separator models are not offered'):
        m.edit_infer_cfg(2, LAB, TY, src_img=sources(), keep_img=KEEP)


def test_plain_var_has_the_image_half_only():
    vae = models.build_vae(ch=32, compute_dtype=torch.float32)
    m = models.build_var(vae, depth=2)
    with pytest.raises(TypeError):
        m.edit_infer_cfg(2, LAB, src_ctrl=sources(), keep_ctrl=True)
    with pytest.raises(ValueError, match='label_B must be given per row'):
        m.edit_infer_cfg(2, None, src_img=sources(), keep_img=KEEP)
    with pytest.raises(ValueError, match='keep_img is given without src_img'):
        m.edit_infer_cfg(2, LAB, keep_img=True)


def test_generate_core_refuses_a_table_without_rows_or_with_four_branches(model):
    forced = torch.full((2, model.cfg.pyramid.L), -1, dtype=torch.int32)
    with pytest.raises(ValueError, match='forced: the per-request joint path only'):
        model._generate_core(2, None, None, False, models._RowDraw(None, forced=forced))
    with pytest.raises(ValueError, match='forced: the per-request joint path only'):
        model._generate_core(2, None, None, True, models._RowDraw((None, None, None, None), forced=forced))


# --------------------------------------------------------------------------------------------------------------- the torch ops
def test_the_two_ops_are_registered_with_schemas_and_fake_kernels():
    import controlvar_amd
    ns = controlvar_amd.register_torch_ops()
    from controlvar_amd import torch_ops
    assert 'edit_force_table' in torch_ops.OPS and 'cfg_sample_edit' in torch_ops.OPS
    assert str(ns.cfg_sample_edit.default._schema) == ('cvar::cfg_sample_edit(Tensor logits, int B, int nrep, Tensor coef, Tensor top_k, Tensor top_p, Tensor seed, '
                                                       'int stage, Tensor forced, int n_draw=1) -> Tensor')
    B, l = 3, 7
    with pytest.raises(RuntimeError, match='no CPU'):
        ns.edit_force_table(torch.zeros(B, 680, dtype=torch.int32), None, None, None, list(DEFAULT_PATCH_NUMS))
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        lg = torch.empty(2 * B, l, V, device='cuda')
        coef, k = torch.empty(B, 4, device='cuda'), torch.empty(B, dtype=torch.int32, device='cuda')
        p, s = torch.empty(B, device='cuda'), torch.empty(B, dtype=torch.int64, device='cuda')
        out = ns.cfg_sample_edit(lg, B, 2, coef, k, p, s, 2, torch.empty(B, l, dtype=torch.int32, device='cuda'))
        assert out.shape == (B, l) and out.dtype == torch.int32
        src = torch.empty(B, 680, dtype=torch.int32, device='cuda')
        keep = torch.empty(B, 16, 16, dtype=torch.uint8, device='cuda')
        assert ns.edit_force_table(src, keep, src, None, list(DEFAULT_PATCH_NUMS)).shape == (B, 1360)
        assert ns.edit_force_table(src, keep, None, None, list(DEFAULT_PATCH_NUMS), True, 1).shape == (B, 680)
