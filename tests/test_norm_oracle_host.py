"""What tests/test_gpu_norm_oracle.py rests on, established on the CPU (oracle/norm_ref.py):
  - the float64 oracles agree with torch.nn.functional / autograd in float64 to 1e-12 (they are not restatements of the kernels);
  - numpy models of the kernels' fp32 arithmetic stay at <= 0.5 of every bound on every case - a correct kernel can pass.  For a bf16 output the
    2^-8 |y64| term of the bound IS the worst case of the final rounding (half an ulp just above a power of two), so there the model before that
    rounding is held to 0.5 of the bound without the term, and the rounded model to the whole bound (|rn(y) - y64| <= 2^-8 |y| + |y - y64|);
  - planted faults in those models overshoot the bound by >= 10 x on a named case - a wrong kernel cannot;
  - outside the ill-conditioned families the bounds are tight against the reference's size (no vacuous case).
The tables are printed (pytest -s)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import norm_ref as N

F64 = torch.float64
_CACHE = {}


def once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ oracle sanity
def test_ln_oracles_against_torch_float64():
    for n in (8, 21, 25, 33):
        C, M, rp, fam, ld0 = N.LN_FWD_CASES[n]
        x, s, b = N.ln_fwd_inputs(n)
        ex = N.ln_forward(x, s, b, rp)
        g = torch.zeros(M, dtype=torch.long) if ld0 else torch.arange(M) // rp
        ref = F.layer_norm(x.double(), (C,), eps=N.EPS) * (1 + s.double()[g]) + b.double()[g]
        assert rel(ex.y, ref.numpy()) <= 1e-12, N.ln_fwd_name(n)
    for n in (8, 22, 40, 45):
        C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
        x, dy, s, dx_in = N.ln_bwd_inputs(n)
        ex = N.ln_backward(x, dy, s, dx_in, R, l)
        xt, st, sh = x.double().requires_grad_(True), s.double().requires_grad_(True), torch.zeros(R, C, dtype=F64, requires_grad=True)
        y = F.layer_norm(xt, (C,), eps=N.EPS) * (1 + st.repeat_interleave(l, 0)) + sh.repeat_interleave(l, 0)
        y.backward(dy.double())
        assert rel(ex.dx, (dx_in.double() + xt.grad).numpy()) <= 1e-12 and rel(ex.dx0, xt.grad.numpy()) <= 1e-12, N.ln_bwd_name(n)
        assert rel(ex.dscale, st.grad.numpy()) <= 1e-12 and rel(ex.dshift, sh.grad.numpy()) <= 1e-12, N.ln_bwd_name(n)


def test_gated_grad_oracle_against_autograd_float64():
    for n in (6, 7, 18):
        C, R, l, dt, form = N.GG_CASES[n]
        dx, f, gate, rs = N.gg_inputs(n)
        ex = N.gated_grad(dx, f, gate, rs, R, l)
        ft, gt = f.double().requires_grad_(True), gate.double().requires_grad_(True)
        r = torch.ones(R, dtype=F64) if rs is None else rs.double()
        (ft * (gt * r[:, None]).repeat_interleave(l, 0)).backward(dx.double())
        assert rel(ex.df, ft.grad.numpy()) <= 1e-12 and rel(ex.dgate, gt.grad.numpy()) <= 1e-12, N.gg_name(n)


def test_groupnorm_oracle_against_torch_float64():
    for n, silu in ((3, True), (7, False), (9, True), (25, False), (28, True)):
        C, G, HW, fam = N.GN_CASES[n]
        for dtype in N.gn_dtypes(n):
            x, w, b = N.gn_inputs(n, dtype)
            ex = N.groupnorm(x, w, b, G, silu=silu)
            ref = F.group_norm(x.double().permute(0, 2, 1), G, w.double(), b.double(), N.EPS).permute(0, 2, 1)
            ref = F.silu(ref) if silu else ref
            assert rel(ex.y, ref.numpy()) <= 1e-12, N.gn_name(n)
            xg = x.double().view(N.GN_B, HW, G, C // G)
            assert rel(ex.mean, xg.mean((1, 3)).numpy()) <= 1e-12
            assert rel(ex.rstd, (xg.var((1, 3), unbiased=False) + N.EPS).rsqrt().numpy()) <= 1e-12
            assert rel((as64(x) - ex.mean.repeat(C // G, 1)[:, None]) * ex.rstd.repeat(C // G, 1)[:, None] * as64(w) + as64(b), ex.lin) <= 1e-12


def as64(t):
    return N.as_np(t)


# ------------------------------------------------------------------------------------------------ per-case evaluation, shared by the tests below
def ln_fwd_eval(n, fault=None):
    """-> {'f32' | 'bf16': (ratio of model error to bound, share of elements with bound < 1e-4 max |ref|)}"""
    C, M, rp, fam, ld0 = N.LN_FWD_CASES[n]
    x, s, b = N.ln_fwd_inputs(n)
    ex, y32 = once(('lnf', n), lambda: (N.ln_forward(x, s, b, rp), N.ln_forward(x, s, b, rp, dtype=np.float32).y))
    m = N.ln_forward_model(x.numpy(), s, b, rp, fault=fault)
    out = {}
    for dt in ('f32', 'bf16'):
        y = torch.from_numpy(m.y).to(torch.bfloat16).double().numpy() if dt == 'bf16' else m.y.astype(np.float64)
        bd = N.ln_fwd_bound(ex, y32, x, s, rp, dt == 'bf16').bound * np.ones_like(ex.y)
        out[dt] = (N.ratio_of(y - ex.y, bd), float((bd < 1e-4 * np.abs(ex.y).max()).mean()))
    return out


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, np.float32)).to(torch.bfloat16).double().numpy()


def ln_bwd_eval(n, fault=None):
    """-> {'dx', 'dscale', 'dshift': ratio}, share of tight elements of dx"""
    C, R, l, dt, path, fam = N.LN_BWD_CASES[n]
    x, dy, s, dx_in = N.ln_bwd_inputs(n)
    ex, y32 = once(('lnb', n), lambda: (N.ln_backward(x, dy, s, dx_in, R, l), N.ln_backward(x, dy, s, dx_in, R, l, dtype=np.float32)))
    m = N.ln_backward_model(x.numpy(), dy, s, dx_in, R, l, nseg=N.ln_bwd_segments(n), waves=4 if path == 'fused' else 1, fault=fault)
    dyn = as64(dy)
    bx = N.ln_bwd_dx_bound(ex, y32.dx, x, dx_in).bound
    bs = N.colsum_bound(ex.dscale, y32.dscale, np.abs(dyn * ex.xhat), R, l, N.dscale_factor(ex, x, R, l)).bound
    bh = N.colsum_bound(ex.dshift, y32.dshift, np.abs(dyn), R, l).bound
    tight = float((bx < 1e-4 * np.abs(ex.dx).max()).mean())
    return dict(dx=N.ratio_of(m.dx - ex.dx, bx), dscale=N.ratio_of(m.dscale - ex.dscale, bs), dshift=N.ratio_of(m.dshift - ex.dshift, bh)), tight


def gg_eval(n):
    C, R, l, dt, form = N.GG_CASES[n]
    dx, f, gate, rs = N.gg_inputs(n)
    ex, y32 = N.gated_grad(dx, f, gate, rs, R, l), N.gated_grad(dx, f, gate, rs, R, l, dtype=np.float32)
    m = N.gated_grad_model(dx, f, gate, rs, R, l, nseg=N.gg_segments(n))
    r = np.ones(R) if rs is None else as64(rs)
    bg = N.colsum_bound(ex.dgate, y32.dgate, np.abs(as64(dx) * as64(f)) * np.repeat(r, l)[:, None], R, l).bound
    out = dict(df=N.ratio_of(m.df - ex.df, N.df_bound(ex.df, False)), dgate=N.ratio_of(m.dgate - ex.dgate, bg))
    if dt == 'bf16':
        out['df_rounded'] = N.ratio_of(bf16_round(m.df) - ex.df, N.df_bound(ex.df, True))          # held to the whole bound
    return out


def gn_eval(n, dtype, silu, fault=None):
    """-> ratio, largest K_g, share of tight elements"""
    C, G, HW, fam = N.GN_CASES[n]
    x, w, b = N.gn_inputs(n, dtype)
    ex = N.groupnorm(x, w, b, G, silu=silu)
    K = N.gn_conditioning(x, ex, G, as64(x)[:, 0])
    bd = N.gn_bound(x, ex, b, G, K, silu, dtype)
    m = N.groupnorm_model(x, w, b, G, silu=silu, vec=8 if dtype == 'bf16' else 4, fault=fault)
    r = N.ratio_of(m.y - ex.y, N.gn_bound(x, ex, b, G, K, silu, dtype, rounding=False))
    whole = N.ratio_of(bf16_round(m.y) - ex.y, bd) if dtype == 'bf16' else r
    return r, float(K.max()), float((bd < 1e-4 * np.abs(ex.y).max()).mean()), whole


def gn_tile_eval(n, silu, fault=None):
    C, G, t, p, fam, poor = N.GN_TILE_CASES[n]
    x, w, b, part = N.gn_tile_inputs(n)
    ex = N.groupnorm(x, w, b, G, silu=silu)
    K = N.gn_conditioning(x, ex, G, part[..., 2].astype(np.float64))
    m = N.groupnorm_tiles_model(x, part, w, b, G, silu=silu, fault=fault)
    return (N.ratio_of(m.y - ex.y, N.gn_bound(x, ex, b, G, K, silu, 'bf16', rounding=False)), float(K.max()),
            N.ratio_of(bf16_round(m.y) - ex.y, N.gn_bound(x, ex, b, G, K, silu, 'bf16')))


# ------------------------------------------------------------------------------------------------ the case tables cover what they claim
def test_case_tables_name_every_instantiation_and_edge():
    assert {N.ln_instance(C) for C, *_ in N.LN_FWD_CASES.values()} == set(N.LN_INSTANCES)
    fused = [c for c in N.LN_BWD_CASES.values() if c[4] == 'fused']
    assert {N.ln_instance(c[0]) for c in fused if (c[1], c[2]) == (2, 6)} == set(N.LN_INSTANCES)
    assert {(c[1], c[2]) for c in fused if c[0] in (260, 1536)} >= set(N.LN_BWD_SEGS)
    seg = lambda R, l: N.red_segments(R, l, N.RED_TARGET)
    assert seg(1, 1) == 1 and seg(2, 680) == 64 and -(-680 // 64) == 11 and 62 * 11 >= 680 and seg(300, 8) == 2 and seg(2, 30) == N.RED_S
    assert {c[3] for c in N.LN_FWD_CASES.values() if c[0] in (1000, 1536)} == set(N.LN_FAMILIES)
    assert any(c[4] for c in N.LN_FWD_CASES.values())
    assert {c[2] for c in N.GN_CASES.values() if c[0] == 32} == set(N.GN_HW)
    for C, G in N.GN_SHAPES:
        assert {c[2] for c in N.GN_CASES.values() if (c[0], c[1]) == (C, G)} >= {96, 1030}
    assert {c[3] for c in N.GN_CASES.values()} == set(N.GN_FAMILIES)
    assert N.ln_stats_floats(1) == 4 and N.ln_stats_floats(15) == 32 and N.ln_stats_floats(74) == 148


# ------------------------------------------------------------------------------------------------ bounds are feasible and not vacuous
def test_ln_forward_models_inside_half_the_bound_and_bounds_tight():
    print('\n[norm_host] ln_modulate model / bound           f32    bf16   tight share')
    for n in N.LN_FWD_CASES:
        r = ln_fwd_eval(n)
        print(f'[norm_host] {N.ln_fwd_name(n):42s} {r["f32"][0]:6.3f} {r["bf16"][0]:6.3f}   {r["f32"][1]:.3f}')
        assert r['f32'][0] <= 0.5 and r['bf16'][0] <= 1.0, N.ln_fwd_name(n)
        assert r['f32'][1] >= 0.95 or N.LN_FWD_CASES[n][3] in N.LN_FWD_ILL, N.ln_fwd_name(n)


def test_ln_backward_models_inside_half_the_bound_and_bounds_tight():
    print('\n[norm_host] ln_modulate_bwd model / bound                       dx  dscale  dshift   tight share')
    for n in N.LN_BWD_CASES:
        r, tight = ln_bwd_eval(n)
        print(f'[norm_host] {N.ln_bwd_name(n):52s} {r["dx"]:6.3f} {r["dscale"]:6.3f} {r["dshift"]:6.3f}   {tight:.3f}')
        assert max(r.values()) <= 0.5, (N.ln_bwd_name(n), r)
        assert tight >= 0.95 or N.LN_BWD_CASES[n][5] in N.LN_BWD_ILL, N.ln_bwd_name(n)


def test_gated_grad_models_inside_half_the_bound():
    print('\n[norm_host] gated_grad model / bound                df   dgate   df as bf16 (of the whole bound)')
    for n in N.GG_CASES:
        r = gg_eval(n)
        print(f'[norm_host] {N.gg_name(n):36s} {r["df"]:6.3f} {r["dgate"]:6.3f}   {r.get("df_rounded", 0):6.3f}')
        assert max(r['df'], r['dgate']) <= 0.5 and r.get('df_rounded', 0) <= 1.0, (N.gg_name(n), r)


def test_groupnorm_models_inside_half_the_bound_and_bounds_tight():
    print('\n[norm_host] groupnorm model / bound                     dtype  silu   ratio     K_g   tight share   rounded / whole bound')
    over = []
    for n in N.GN_CASES:
        for dtype in N.gn_dtypes(n):
            for silu in (False, True):
                r, K, tight, whole = gn_eval(n, dtype, silu)
                print(f'[norm_host] {N.gn_name(n):40s} {dtype:5s} {int(silu)}    {r:6.3f} {K:8.1f}   {tight:.3f}   {whole:6.3f}')
                if not (r <= 0.5 and whole <= 1.0):
                    over.append((N.gn_name(n), dtype, silu, r, whole))
                assert dtype == 'bf16' or tight >= 0.95 or N.GN_CASES[n][3] in N.GN_ILL or N.GN_CASES[n][2] == 1, (N.gn_name(n), tight)    # HW = 1: rstd = 1000
    for n in N.GN_TILE_CASES:
        for silu in (False, True):
            r, K, whole = gn_tile_eval(n, silu)
            print(f'[norm_host] tiles {N.gn_tile_name(n):34s} bf16  {int(silu)}    {r:6.3f} {K:8.1f}           {whole:6.3f}')
            if not (r <= 0.5 and whole <= 1.0):
                over.append(('tiles ' + N.gn_tile_name(n), 'bf16', silu, r, whole))
    assert not over, over


# ------------------------------------------------------------------------------------------------ bounds discriminate
# fault -> the case on which it must overshoot its bound by >= 10 x (ids of the case tables)
LN_FWD_FAULT_CASE = {'tail_out_of_mean': 4, 'tail_out_of_var': 4, 'div_nv256': 8, 'no_eps': 24, 'group_off_by_one': 23}
LN_BWD_FAULT_CASE = {'drop_mgx': 28, 'drop_segment': 28, 'last_row_twice': 28}
GN_FAULT_CASE = {'raw_sums': (29, 'f32'), 'drop_last_chunk': (6, 'f32'), 'skip_second_trip': (10, 'f32')}
GN_TILE_FAULT_CASE = {'ignore_tile_pivots': 3}


def test_planted_faults_overshoot_the_bounds():
    print('\n[norm_host] planted fault                case                                                 error / bound')
    rows = []
    for fault, n in LN_FWD_FAULT_CASE.items():
        rows.append((fault, N.ln_fwd_name(n), ln_fwd_eval(n, fault)['f32'][0]))
    for fault, n in LN_BWD_FAULT_CASE.items():
        rows.append((fault, N.ln_bwd_name(n), max(ln_bwd_eval(n, fault)[0].values())))
    for fault, (n, dtype) in GN_FAULT_CASE.items():
        rows.append((fault, N.gn_name(n), gn_eval(n, dtype, False, fault)[0]))
    for fault, n in GN_TILE_FAULT_CASE.items():
        rows.append((fault, 'tiles ' + N.gn_tile_name(n), gn_tile_eval(n, False, fault)[0]))
    for fault, name, r in rows:
        print(f'[norm_host] {fault:28s} {name:52s} {r:10.1f}')
    assert {r[0] for r in rows} == set(N.LN_FWD_FAULTS + N.LN_BWD_FAULTS + N.GN_FAULTS)
    assert all(r >= 10 for _, _, r in rows), [x for x in rows if x[2] < 10]
    # the same faults on the bf16 outputs (the bf16 rounding term widens the bound)
    for fault, n in LN_FWD_FAULT_CASE.items():
        assert ln_fwd_eval(n, fault)['bf16'][0] >= 10, fault
