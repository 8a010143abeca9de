"""kv_precision='fp8', host side (no GPU; DESIGN.md 4j, include/cvar_kvcache.h): the per-head quantisation rule restated with tests/fp8_ref.py and
held against torch.float8_e4m3fn, the exactness the GPU identity test rests on (an e4m3 value times a power of two IS a bf16 value), the keyword and
its setter on the models, the arena's shapes and size, and the fourth ctypes table against its header."""
import os
import re

import numpy as np
import pytest
import torch

import fp8_ref as R8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['cvar_kv_append_fp8', 'cvar_attention_kv8']
F32, BF16 = torch.float32, torch.bfloat16


# ---------------------------------------------------------------------------------------------------------------- the rule
def quant_heads(x):
    """x [.., 64] fp32 values -> (bytes uint8 [.., 64], scale fp32 [..]): fp8_ref's row rule with K = 64, one row per head vector"""
    x = np.asarray(x, dtype=np.float32)
    flat = x.reshape(-1, 64)
    bad = ~np.isfinite(flat).all(axis=1)
    amax = np.where(bad, np.float32(0), np.abs(np.where(np.isfinite(flat), flat, 0)).max(axis=1)).astype(np.float32)
    k = R8.row_exponent(amax)
    inv = np.exp2(-k.astype(np.float64)).astype(np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        scaled = (flat * inv[:, None]).astype(np.float32)
    q = R8.encode_rne(np.where(bad[:, None], np.float32(np.nan), scaled))
    scale = np.where(bad, 1.0, np.exp2(k.astype(np.float64))).astype(np.float32)
    return q.reshape(x.shape), scale.reshape(x.shape[:-1])


def test_the_per_head_rule_against_torch_float8_e4m3fn():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((3, 7, 6, 64)) * np.exp2(rng.integers(-20, 21, size=(3, 7, 6, 1)))).astype(np.float32)
    x = R8.bf16_round(x)                                        # the kernel takes bf16 rows
    x[0, 0, 0] = 0.0
    x[0, 0, 1, 5] = np.nan
    x[0, 0, 2, 63] = np.inf
    x[0, 1, 0] = 0.0; x[0, 1, 0, 3] = 448.0 * 2.0 ** 5          # amax exactly at 448 * 2^k
    q, scale = quant_heads(x)
    assert q.shape == x.shape and scale.shape == x.shape[:-1]
    # the rule: k is the smallest integer with amax <= 448 * 2^k
    fin = np.isfinite(x).all(axis=-1)
    amax = np.abs(np.where(np.isfinite(x), x, 0)).max(axis=-1).astype(np.float64)
    nz = fin & (amax > 0)
    assert (amax[nz] <= 448.0 * scale[nz]).all() and (amax[nz] > 448.0 * scale[nz] / 2).all()
    assert scale[0, 0, 0] == np.float32(2.0 ** -60) and not q[0, 0, 0].any()
    assert scale[0, 0, 1] == 1.0 and (q[0, 0, 1] == 0x7F).all() and scale[0, 0, 2] == 1.0 and (q[0, 0, 2] == 0x7F).all()
    assert scale[0, 1, 0] == np.float32(2.0 ** 5) and q[0, 1, 0, 3] == 0x7E
    # the bytes: torch's own e4m3fn rounding of x / scale (exact division: a power of two)
    want = (torch.from_numpy(x[fin]) / torch.from_numpy(scale[fin])[:, None]).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(q[fin], want)
    # and torch decodes every byte as fp8_ref does
    allb = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(allb), np.isnan(R8.DECODE)) and np.array_equal(allb[~np.isnan(allb)], R8.DECODE[~np.isnan(R8.DECODE)])


def test_decoded_byte_times_scale_is_exactly_a_bf16_value():
    """for every code and every k in [-60, 100]: what the attention kernel's staging computes (fp32 product, upper 16 bits) is the exact value"""
    codes = np.arange(256, dtype=np.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    val = R8.decode(codes)                                                      # float64, exact
    for k in range(-60, 101):
        exact = val * 2.0 ** k                                                  # exact in float64
        f32 = (val.astype(np.float32) * np.float32(2.0 ** k)).astype(np.float32)
        assert np.array_equal(f32.astype(np.float64), exact), k                # the fp32 product does not round
        bits = f32.view(np.uint32)
        assert not (bits & 0xFFFF).any(), k                                     # ... and its lower 16 bits are empty: truncation to bf16 is exact
        assert np.array_equal(R8.bf16_round(f32), f32), k
        back = torch.from_numpy(f32).to(BF16).to(torch.float64).numpy()
        assert np.array_equal(back, exact), k


# ---------------------------------------------------------------------------------------------------------------- keyword and setter
def build(dtype, **kw):
    from controlvar_amd import models
    vae = models.build_vae(ch=32, compute_dtype=dtype)
    return models.build_control_var(vae, depth=2, mask_type='interleave_append', multi_cond=True, compute_dtype=dtype, **kw)


def test_keyword_accepted_combinations():
    from controlvar_amd import models
    assert models.KV_PRECISIONS == (None, 'fp8')
    assert build(BF16).kv_precision is None
    assert build(BF16, kv_precision='fp8').kv_precision == 'fp8'
    m = build(BF16, kv_precision='fp8', gemm_precision='fp8')
    assert (m.kv_precision, m.gemm_precision) == ('fp8', 'fp8')
    vae = models.build_vae(ch=32, compute_dtype=BF16)
    assert models.build_var(vae, depth=2, compute_dtype=BF16, kv_precision='fp8').kv_precision == 'fp8'
    m = build(BF16)
    m.kv_precision = 'fp8'; m.gemm_precision = 'fp8'; m.kv_precision = None; m.gemm_precision = None
    assert m.kv_precision is None
    with pytest.raises(ValueError, match='kv_precision must be one of'):
        build(BF16, kv_precision='int8')


def test_the_two_refusals_and_their_wording():
    with pytest.raises(ValueError, match=r"kv_precision='fp8' needs a compute_dtype=torch.bfloat16 model.*exists for exactness"):
        build(F32, kv_precision='fp8')
    m = build(F32)
    with pytest.raises(ValueError, match='needs a compute_dtype=torch.bfloat16 model'):
        m.kv_precision = 'fp8'
    assert m.kv_precision is None
    with pytest.raises(ValueError, match=r"not offered under gemm_precision='bf16x3'.*exists for exactness"):
        build(F32, gemm_precision='bf16x3', kv_precision='fp8')
    m = build(F32, gemm_precision='bf16x3')
    with pytest.raises(ValueError):
        m.kv_precision = 'fp8'
    assert m.kv_precision is None and m.gemm_precision == 'bf16x3'


def test_setting_it_drops_the_arena_and_keeps_the_pack():
    m = build(BF16)
    pack, arena = object(), {0: ('key', 'buffer')}
    m._packed, m._arena = pack, arena
    m.kv_precision = None                                  # no change: nothing dropped
    assert m._packed is pack and m._arena is arena
    m.kv_precision = 'fp8'
    assert m._packed is pack and m._arena is None
    m._arena = arena
    m.kv_precision = None
    assert m._packed is pack and m._arena is None


def test_arena_shapes_and_byte_count():
    from controlvar_amd import models
    depth, Rr, L, H = 24, 1024, 1360, 24
    sq, ss = models.kv8_arena_shapes(depth, Rr, L, H)
    assert sq == (depth, Rr, L, 2 * H * 64) and ss == (depth, Rr, L, 2 * H)
    n8 = int(np.prod(sq)) + 4 * int(np.prod(ss))
    n16 = depth * Rr * L * 2 * H * 64 * 2
    assert 32 * n8 == 17 * n16
    assert round(n16 / 1e9) == 205 and round(n8 / 1e9) == 109          # the headline shape
    a = models.KV8Arena(torch.empty(models.kv8_arena_shapes(2, 3, 5, 2)[0], dtype=torch.uint8), torch.empty(models.kv8_arena_shapes(2, 3, 5, 2)[1]))
    assert a.q.dtype == torch.uint8 and a.scale.dtype == F32 and a.nbytes * 32 == 17 * (2 * 3 * 5 * 2 * 2 * 64 * 2)
    assert int(np.prod(models.kv8_arena_shapes(1, 1032, 1360, 24)[0])) > 2 ** 32          # one layer of the large-offset test


# ---------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope='module')
def lib():
    from controlvar_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from controlvar_amd.build import build_lib
        build_lib(verbose=False)
    return _lib.load()


def _declarations(header):
    """name -> list of parameter declarations, comments stripped"""
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    out = {}
    for m in re.finditer(r'\b(cvar_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', src):
        args = m.group(2).strip()
        out[m.group(1)] = [] if args in ('', 'void') else [a.strip() for a in args.split(',')]
    return out


def _ctype_of(decl):
    from controlvar_amd import _lib
    import ctypes as C
    d = re.sub(r'\s+', ' ', decl)
    if re.match(r'const int\* ', d):
        return C.POINTER(_lib.c_i)
    if '*' in d:
        return _lib.c_p
    return {'int': _lib.c_i, 'int64_t': _lib.c_l, 'float': _lib.c_f}[d.rsplit(' ', 1)[0]]


def test_kvcache_entry_points_are_declared_exported_and_bound(lib):
    from controlvar_amd import _lib
    decl = _declarations('cvar_kvcache.h')
    assert sorted(decl) == sorted(NAMES) == sorted(_lib.KVCACHE_SIGNATURES)
    assert not set(_lib.KVCACHE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.SERVE_SIGNATURES) | set(_lib.ACCUM_SIGNATURES))
    for name in NAMES:
        res, argtypes = _lib.KVCACHE_SIGNATURES[name]
        assert hasattr(lib, name), f'{name} declared in include/cvar_kvcache.h but not exported'
        assert res is _lib.c_i and argtypes == [_ctype_of(d) for d in decl[name]], (name, decl[name])
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res        # load() bound the fourth table
    # cvar_attention_kv8 = cvar_attention_prescaled with (kv8, kv_scale) for (kv) and without the dtype
    pre = _declarations('cvar.h')['cvar_attention_prescaled']
    norm = lambda d: re.sub(r'\s+', ' ', d)
    assert [norm(x) for x in decl['cvar_attention_kv8'][2:]] == [norm(x) for x in pre[1:2] + pre[3:]]


def test_the_older_headers_did_not_move(lib):
    from controlvar_amd import _lib
    assert _lib.ABI_VERSION == 22 and lib.cvar_abi_version() == 22
    assert _lib.SERVE_VERSION == 1 and lib.cvar_serve_version() == 1
    for h in ('cvar.h', 'cvar_serve.h', 'cvar_accum.h'):
        assert not set(NAMES) & set(_declarations(h)), h
    from controlvar_amd import build
    assert 'kvcache.hip' in build.SOURCES


def test_host_calls_refuse_bad_arguments_without_a_gpu(lib):
    """argument checks come before any launch: CVAR_EINVAL (-1) for NULL pointers, empty sizes, rows outside the arena, misaligned pointers;
    CVAR_EUNSUPPORTED (-2) for a level whose hole hides keys [0, 64)"""
    import ctypes as C
    assert lib.cvar_kv_append_fp8(None, None, None, 1, 1, 8, 0, 1, None) == -1
    assert lib.cvar_kv_append_fp8(64, 128, 256, 1, 1, 8, 0, 0, None) == -1
    assert lib.cvar_kv_append_fp8(64, 128, 256, 1, 1, 8, 5, 4, None) == -1          # q_off + l > Lmax
    assert lib.cvar_kv_append_fp8(72, 128, 256, 1, 1, 8, 0, 1, None) == -1          # kv not 16-byte aligned
    assert lib.cvar_attention_kv8(None, None, None, 1, 1, 8, 0, 1, None, 0, None, None, None, None) == -1
    assert lib.cvar_attention_kv8(64, 256, 512, 1, 1, 8, 5, 4, None, 0, None, 1024, None, None) == -1
    lvl, holes = (C.c_int * 2)(100, 200), (C.c_int * 4)(0, 0, 0, 64)
    assert lib.cvar_attention_kv8(64, 256, 512, 1, 1, 256, 0, 200, lvl, 2, holes, 1024, None, None) == -2
