"""Widths above 2048, host side (no GPU; DESIGN.md 4k, include/cvar_wide.h): the fifth header against its ctypes table and the library's exports, the
refusals of the three entry points (returned before any launch, so dummy pointers do), the constructor's new limit, and what
tests/test_gpu_wide_kernels.py rests on: a numpy model of the wide kernels' lane order sits inside oracle/norm_ref.py's bound on every case, and the five
planted faults of norm_ref.LN_FWD_FAULTS, restated for the wide layout (tests/wide_ref.py), do not."""
import os
import re

import numpy as np
import pytest
import torch

import wide_ref as W
from oracle import norm_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['cvar_ln_modulate_wide', 'cvar_ln_modulate_split3_wide', 'cvar_ln_modulate_fp8_wide']
NARROW = {'cvar_ln_modulate_wide': ('cvar.h', 'SIGNATURES', 'cvar_ln_modulate'),
          'cvar_ln_modulate_split3_wide': ('cvar_serve.h', 'SERVE_SIGNATURES', 'cvar_ln_modulate_split3'),
          'cvar_ln_modulate_fp8_wide': ('cvar_serve.h', 'SERVE_SIGNATURES', 'cvar_ln_modulate_fp8')}


@pytest.fixture(scope='module')
def lib():
    from controlvar_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.load()


def _source(header):
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)


def _declarations(header):
    """name -> list of parameter declarations, comments stripped"""
    out = {}
    for m in re.finditer(r'\b(cvar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', _source(header)):
        args = m.group(2).strip()
        out[m.group(1)] = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
    return out


def _ctype_of(decl):
    from controlvar_amd import _lib
    d = re.sub(r'\s+', ' ', decl)
    if '*' in d:
        return _lib.c_p
    return {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[d.rsplit(' ', 1)[0]]


# ------------------------------------------------------------------------------------------------ the ABI
def test_wide_entry_points_are_declared_exported_and_bound(lib):
    from controlvar_amd import _lib
    decl = _declarations('cvar_wide.h')
    assert sorted(decl) == sorted(NAMES) == sorted(_lib.WIDE_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.SERVE_SIGNATURES) | set(_lib.ACCUM_SIGNATURES) | set(_lib.KVCACHE_SIGNATURES)
    assert not set(_lib.WIDE_SIGNATURES) & others
    norm = lambda d: re.sub(r'\s+', ' ', d)
    for name in NAMES:
        res, argtypes = _lib.WIDE_SIGNATURES[name]
        assert hasattr(lib, name), f'{name} declared in include/cvar_wide.h but not exported'
        assert res is _lib.c_i and argtypes == [_ctype_of(d) for d in decl[name]], (name, decl[name])
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res        # load() bound the fifth table
        # each takes its namesake's arguments: the same declarations in the header, the same ctypes row
        header, table, narrow = NARROW[name]
        assert [norm(d) for d in decl[name]] == [norm(d) for d in _declarations(header)[narrow]], name
        assert argtypes == getattr(_lib, table)[narrow][1], name


def test_the_older_headers_did_not_move(lib):
    from controlvar_amd import _lib, build
    assert _lib.ABI_VERSION == 22 and lib.cvar_abi_version() == 22
    assert _lib.SERVE_VERSION == 1 and lib.cvar_serve_version() == 1
    tables = {'cvar.h': _lib.SIGNATURES, 'cvar_serve.h': _lib.SERVE_SIGNATURES, 'cvar_accum.h': _lib.ACCUM_SIGNATURES, 'cvar_kvcache.h': _lib.KVCACHE_SIGNATURES}
    for h, table in tables.items():
        d = _declarations(h)
        assert not set(NAMES) & set(d), h
        assert set(d) == set(table), h                            # every header still is its table: the fifth one took nothing from them
    assert 'ops.hip' in build.SOURCES


def test_cmax_is_one_constant_and_covers_d40():
    from controlvar_amd import _lib
    m = re.search(r'#define\s+CVAR_WIDE_CMAX\s+(\d+)', _source('cvar_wide.h'))
    assert m, 'CVAR_WIDE_CMAX is not defined in include/cvar_wide.h'
    cmax = int(m.group(1))
    assert cmax == _lib.WIDE_CMAX == W.CMAX and cmax >= 2560 and cmax % 256 == 0


def test_the_library_refuses_without_a_launch(lib):
    """CVAR_EINVAL (-1): a NULL pointer, M <= 0, rows_per <= 0.  CVAR_EUNSUPPORTED (-2): C > CMAX, C % 4, ld_ada % 4, a misaligned pointer of the split3 /
    fp8 forms, a bad ldq.  `one` is a non-NULL, aligned address that is never dereferenced: every call below returns on the host."""
    one, C, cmax = 64, 2304, W.CMAX
    ln, s3, f8 = lib.cvar_ln_modulate_wide, lib.cvar_ln_modulate_split3_wide, lib.cvar_ln_modulate_fp8_wide
    for k in range(3):
        p = [one, one, one]
        p[k] = None
        assert ln(*p, C, 1, one, 0, 1, C, 1e-6, None) == -1 and s3(*p, C, 1, one, 1, C, 1e-6, None) == -1
        assert f8(*p, C, 1, one, C, one, 1, C, 1e-6, None) == -1
    assert ln(one, one, one, C, 1, None, 0, 1, C, 1e-6, None) == -1 and s3(one, one, one, C, 1, None, 1, C, 1e-6, None) == -1
    assert f8(one, one, one, C, 1, None, C, one, 1, C, 1e-6, None) == -1 and f8(one, one, one, C, 1, one, C, None, 1, C, 1e-6, None) == -1
    for M, rp in ((0, 1), (-3, 1), (1, 0), (1, -1)):
        assert ln(one, one, one, C, rp, one, 0, M, C, 1e-6, None) == -1 and s3(one, one, one, C, rp, one, M, C, 1e-6, None) == -1
        assert f8(one, one, one, C, rp, one, C, one, M, C, 1e-6, None) == -1
    for Cb, ld in ((cmax + 4, cmax + 4), (cmax + 256, cmax + 256), (2306, 2308), (2304, 2306)):          # C > CMAX (twice), C % 4, ld_ada % 4
        ldq = (Cb + 127) // 128 * 128
        assert ln(one, one, one, ld, 1, one, 0, 1, Cb, 1e-6, None) == -2 and ln(one, one, one, ld, 1, one, 1, 1, Cb, 1e-6, None) == -2
        assert s3(one, one, one, ld, 1, one, 1, Cb, 1e-6, None) == -2 and f8(one, one, one, ld, 1, one, ldq, one, 1, Cb, 1e-6, None) == -2
    assert ln(one, one, one, C, 1, one, 7, 1, C, 1e-6, None) == -2                                        # an unknown out_dtype
    for k in range(3):                                                                                      # x, scale, shift 16-byte aligned
        p = [one, one, one]
        p[k] = one + 4
        assert s3(*p, C, 1, one, 1, C, 1e-6, None) == -2 and f8(*p, C, 1, one, C, one, 1, C, 1e-6, None) == -2
    assert s3(one, one, one, C, 1, one + 4, 1, C, 1e-6, None) == -2                                       # out 8-byte aligned
    assert f8(one, one, one, C, 1, one + 8, C, one, 1, C, 1e-6, None) == -2                               # q 16-byte aligned
    assert f8(one, one, one, C, 1, one, C + 64, one, 1, C, 1e-6, None) == -2                              # ldq % 128
    assert f8(one, one, one, C, 1, one, C - 128, one, 1, C, 1e-6, None) == -2                             # ldq < C
    # the narrow entry points keep their limit
    assert lib.cvar_ln_modulate(one, one, one, 4104, 1, one, 0, 1, 2052, 1e-6, None) == -2


# ------------------------------------------------------------------------------------------------ the constructor
def test_d36_constructs_and_the_limit_names_cmax(monkeypatch):
    """the factories at depth 36 (C = 2304, 36 heads) go through the whole constructor.  Only the VALUES of the 2.3 G synthetic weights are left out: the
    constructor takes tensors of the shapes of spec.var_state_shapes whose matrices are left uninitialised (untouched pages cost neither time nor memory);
    it never reads them."""
    from controlvar_amd import models
    from controlvar_amd.spec import PATCH_NUMS_512, var_state_shapes

    def zeros(cfg, seed=0):
        big = lambda shape: int(np.prod(shape)) > 1 << 20           # the matrices: uninitialised, so that no page of them is ever touched
        return {k: torch.empty(shape) if big(shape) else torch.zeros(shape, dtype=torch.int64 if k in ('lvl_1L', 'type_1L', 'type_1L_') else torch.float32)
                for k, (shape, kind) in var_state_shapes(cfg).items()}
    vae = models.build_vae(ch=32, v_patch_nums=PATCH_NUMS_512)
    vae16 = models.build_vae(ch=32)
    with monkeypatch.context() as mp:
        mp.setattr(models, 'synth_var_state', zeros)
        v = models.build_var(vae, depth=36, shared_aln=True, patch_nums=PATCH_NUMS_512)
        c = models.build_control_var(vae16, depth=36, mask_type='interleave_append', multi_cond=True)
    assert (v.C, v.num_heads, v.depth) == (2304, 36, 36) and v.cfg.shared_aln and v.L == 2240
    assert (c.C, c.num_heads, c.depth) == (2304, 36, 36) and c.L == 1360
    assert sum(p.numel() for p in v.parameters()) > 2.2e9
    del v, c
    wide = W.CMAX + 64
    with pytest.raises(ValueError, match=rf'CVAR_WIDE_CMAX = {W.CMAX}'):
        models.VAR(vae, depth=1, embed_dim=wide, num_heads=wide // 64, patch_nums=PATCH_NUMS_512)
    models.VAR(vae, depth=1, embed_dim=W.CMAX, num_heads=W.CMAX // 64, patch_nums=PATCH_NUMS_512)           # the bound itself is served


# ------------------------------------------------------------------------------------------------ the model of the wide layout and its bound
def evaluate(n, fault=None):
    """-> {'f32' | 'bf16': model error / bound}"""
    C, M, rp, fam = W.CASES[n]
    x, s, b, ex, y32 = W.refs(n)
    m = W.forward_model(x.numpy(), s.numpy(), b.numpy(), rp, fault=fault)
    out = {}
    for dt in ('f32', 'bf16'):
        y = torch.from_numpy(m.y).to(torch.bfloat16).double().numpy() if dt == 'bf16' else m.y.astype(np.float64)
        out[dt] = N.ratio_of(y - ex.y, N.ln_fwd_bound(ex, y32, x, s, rp, dt == 'bf16').bound * np.ones_like(ex.y))
    return out


def test_the_cases_cover_the_shapes_of_the_issue():
    cs = set((C, M, rp) for C, M, rp, fam in W.CASES.values() if fam == 'unit')
    assert {(C, M, rp) for C in (2052, 2304, 2500, 2560, W.CMAX) for M, rp in ((9, 3), (5, 1), (1, 1))} <= cs
    assert {(c + 255) // 256 for c, *_ in W.CASES.values()} == {9, 10, 11, 12}


def test_the_wide_model_is_norm_refs_model_at_its_own_layout():
    """the wide kernels are ln_modulate_kernel's text at NV = 9 .. 12: the restated model and norm_ref.ln_forward_model agree bit for bit"""
    for n in (1, 7, 10, 13):
        C, M, rp, fam = W.CASES[n]
        x, s, b = W.inputs(n)
        a, r = W.forward_model(x.numpy(), s.numpy(), b.numpy(), rp), N.ln_forward_model(x.numpy(), s, b, rp)
        assert np.array_equal(a.y, r.y) and np.array_equal(a.rstd, r.rstd), W.name(n)


def test_wide_models_inside_the_bound():
    """fp32 at <= 0.5 of the bound, the bf16-rounded model at <= 1 (the 2^-8 |y64| term IS the worst case of that rounding): the rule of
    tests/test_norm_oracle_host.py"""
    print('\n[wide_host] ln_modulate_wide model / bound               f32    bf16')
    for n in W.CASES:
        r = evaluate(n)
        print(f'[wide_host] {W.name(n):46s} {r["f32"]:6.3f} {r["bf16"]:6.3f}')
        assert r['f32'] <= 0.5 and r['bf16'] <= 1.0, W.name(n)


# fault -> the case on which it must overshoot (ids of wide_ref.CASES): tails at C = 2500 (196 live elements in the tenth vector) and at C = 2052 (one live
# lane in the ninth), NV 256 = 2560 against C = 2500, eps on the small-variance rows, the group rule on M = 9 rows of three
FAULT_CASES = {'tail_out_of_mean': (7, 1), 'tail_out_of_var': (7, 1), 'div_nv256': (7,), 'no_eps': (20,), 'group_off_by_one': (7, 4)}


def test_planted_faults_land_outside_the_bound():
    assert set(FAULT_CASES) == set(N.LN_FWD_FAULTS) and W.CASES[7][0] == 2500 and W.CASES[1][0] == 2052 and W.CASES[20][3] == 'small_var'
    print('\n[wide_host] planted fault         case                                           error / bound  f32    bf16')
    for fault, cases in FAULT_CASES.items():
        for n in cases:
            r = evaluate(n, fault)
            print(f'[wide_host] {fault:20s} {W.name(n):46s} {r["f32"]:10.1f} {r["bf16"]:10.1f}')
            assert r['f32'] >= 10 and r['bf16'] >= 10, (fault, W.name(n), r)              # the house margin of tests/test_norm_oracle_host.py
