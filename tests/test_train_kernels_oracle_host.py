"""What tests/test_gpu_train_kernels_oracle.py rests on, established on the CPU (oracle/train_kernels_ref.py):
  - the float64 oracles agree with torch (optim.AdamW, F.cross_entropy + autograd, F.gelu / F.silu + autograd, index_add_, clip_grad_norm_, sums)
    in float64 to 1e-12 - they are not restatements of the kernels;
  - numpy models of the kernels' arithmetic stay at <= 0.5 of every bound on every case of the tables - a correct kernel can pass (a bf16 output's
    2^-8 |ref| term IS its rounding's worst case: the model before that rounding is held to 0.5 of the bound without the term);
  - planted arithmetic faults in those models land outside the bounds - a wrong kernel cannot pass.  Factors (error / bound) as printed by
    test_planted_faults_land_outside_the_bounds (pytest -s):
        AdamW   eps inside the bias correction 1.7e5 (step 1000)      bc2 for sqrt(bc2) 2.1e5 (step 1000)      decay after the update 158
                moment from the unscaled gradient 5.6e6 (m)    group 0's wd for every tensor 53
                float32 powf corrections at betas (0.9, 0.999): 3.7 at step 2, 1.4 at step 7 (30 u and 11 u of the sum the bound is stated in;
                at betas (0.9, 0.95) they stay inside half the bound)
        CE      1 / se before the last wave partial 4.8e4      one-hot left unweighted 4e37 (a zero-weight row must stay exactly 0)
        clip    1e-6 dropped 3.1 (1.6e-7 of a norm of 6.3 against one float32 rounding)       pre_scale inside the square root 3.1e7
        sums    a colsum segment without its last row 246      wordembed rows without `skip` after a sample boundary 381
        act     gelu' cubic coefficient 0.044715 1.8e4      silu' without its 1 + 1.1e6
The tables are printed (pytest -s)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import train_kernels_ref as T

F64 = torch.float64
_CACHE = {}


def once(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max()))


# ------------------------------------------------------------------------------------------------ oracles against torch in float64
def test_adamw_oracle_against_torch_optim_float64_over_steps_and_groups():
    """two parameter groups, the steps 1 .. 8 in sequence from zero moments; the oracle is fed torch's own state before each step"""
    g_ = torch.Generator().manual_seed(1)
    lrs, wds = (3e-3, 1e-3), (0.05, 0.0)
    b1, b2, eps = T.f32(0.9), T.f32(0.999), T.f32(1e-8)
    ps = [torch.randn(301, generator=g_, dtype=F64).requires_grad_(True), torch.randn(77, generator=g_, dtype=F64).requires_grad_(True)]
    opt = torch.optim.AdamW([dict(params=[ps[0]], lr=T.f32(lrs[0]), weight_decay=T.f32(wds[0])), dict(params=[ps[1]], lr=T.f32(lrs[1]), weight_decay=T.f32(wds[1]))],
                            betas=(b1, b2), eps=eps)
    m = [np.zeros(301), np.zeros(77)]
    v = [np.zeros(301), np.zeros(77)]
    for step in range(1, 9):
        before = [p.detach().numpy().copy() for p in ps]
        grads = [torch.randn(p.shape, generator=g_, dtype=F64) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        for k in range(2):
            ex = T.adamw(before[k], grads[k].numpy(), m[k], v[k], step, lrs[k], 0.9, 0.999, 1e-8, wds[k])
            assert rel(ex.p, ps[k].detach().numpy()) <= 1e-12 and rel(ex.m, opt.state[ps[k]]['exp_avg'].numpy()) <= 1e-12
            assert rel(ex.v, opt.state[ps[k]]['exp_avg_sq'].numpy()) <= 1e-12, (step, k)
            m[k], v[k] = ex.m, ex.v
    # a late step: torch's state set by hand
    for step in (1000, 100000):
        p = torch.randn(50, generator=g_, dtype=F64).requires_grad_(True)
        opt = torch.optim.AdamW([p], lr=T.f32(3e-3), betas=(b1, T.f32(0.95)), eps=eps, weight_decay=T.f32(0.05))
        m0, v0, g = torch.randn(50, generator=g_, dtype=F64) * 0.1, torch.rand(50, generator=g_, dtype=F64) * 0.01, torch.randn(50, generator=g_, dtype=F64)
        opt.state[p] = dict(step=torch.tensor(float(step - 1)), exp_avg=m0.clone(), exp_avg_sq=v0.clone())
        before = p.detach().numpy().copy()
        p.grad = g
        opt.step()
        ex = T.adamw(before, g.numpy(), m0.numpy(), v0.numpy(), step, 3e-3, 0.9, 0.95, 1e-8, 0.05)
        assert rel(ex.p, p.detach().numpy()) <= 1e-12, step
    # gscale and the device scale multiply the gradient
    a = T.adamw(before, g.numpy() * T.f32(0.25) * T.f32(0.3), m0.numpy(), v0.numpy(), 7, 3e-3, 0.9, 0.95, 1e-8, 0.05)
    b = T.adamw(before, g.numpy(), m0.numpy(), v0.numpy(), 7, 3e-3, 0.9, 0.95, 1e-8, 0.05, gscale=0.25, gdev=0.3)
    assert rel(a.p, b.p) <= 1e-15


def test_ce_oracle_against_torch_float64():
    for n in (1, 7, 13, 25, 31, 38):           # finite families at several V
        V, fam, wk, gs = T.CE_CASES[n]
        if fam == 'neginf8':
            continue
        lg, tgt, w, gs = T.ce_inputs(n)
        ex = T.ce(lg, tgt, w, gs)
        x = lg.double().requires_grad_(True)
        lt = F.cross_entropy(x, tgt.long(), reduction='none')
        ww = torch.ones(T.CE_M, dtype=F64) if w is None else w.double()
        (lt * ww).sum().mul(T.f32(gs)).backward()
        assert rel(ex.loss, lt.detach().numpy()) <= 1e-12 and rel(ex.dlogits, x.grad.numpy()) <= 1e-12, T.ce_name(n)
    # -inf logits: torch's log_softmax is the reference of the loss on the finite targets
    n = [k for k, c in T.CE_CASES.items() if c[1] == 'neginf8' and c[0] == 257][0]
    lg, tgt, w, gs = T.ce_inputs(n)
    ex = T.ce(lg, tgt, w, gs)
    ref = -torch.log_softmax(lg.double(), 1)[torch.arange(T.CE_M), tgt.long()].numpy()
    fin = np.isfinite(ref)
    assert fin.any() and rel(ex.loss[fin], ref[fin]) <= 1e-12 and np.array_equal(np.isinf(ex.loss), ~fin)
    # a -inf logit has probability 0: its gradient is 0, or -w gscale where it is the target
    wg = (np.ones(T.CE_M) if w is None else T.as_np(w)) * T.f32(gs)
    hot = np.arange(257)[None] == T.as_np(tgt)[:, None]
    dead = np.isinf(T.as_np(lg))
    assert np.isfinite(ex.dlogits).all() and np.array_equal(ex.dlogits[dead], (-wg[:, None] * hot)[dead])


def test_activation_oracles_against_torch_float64():
    a, dh = T.act_inputs(257, 'f32')
    a = a[(a.abs() < 50)]           # torch's tanh form and the sigmoid form agree to 1e-12 where neither saturates; beyond, both are t or 0
    dh = dh[:a.numel()]
    ex = T.gelu(a, dh)
    x = a.double().requires_grad_(True)
    y = F.gelu(x, approximate='tanh')
    y.backward(dh.double())
    assert rel(ex.y, y.detach().numpy()) <= 1e-12 and rel(ex.dy, x.grad.numpy()) <= 1e-12
    assert abs(T.GELU_C3 - 3 * T.GELU_C) < 1e-12
    x = a.double().requires_grad_(True)
    F.silu(x).backward(dh.double())
    assert rel(T.silu_bwd(a, dh).dx, x.grad.numpy()) <= 1e-12
    # the derivatives cross zero where the case tables say
    assert abs(T.gelu(np.array([-0.7524614])).grad[0]) < 1e-6 and abs(T.silu_bwd(np.array([-1.2784645]), np.ones(1)).grad[0]) < 1e-6


def test_reduction_oracles_against_torch_float64():
    A, o = T.colsum_inputs(5)
    assert rel(T.colsum(A, o), (o.double() + A.double().sum(0)).numpy()) <= 1e-12
    A, o = T.rowsum_inputs(9)
    assert rel(T.rowsum(A, o), (o.double() + A.double().sum(1)).numpy()) <= 1e-12
    src, dst = T.scatter_inputs(255)
    ref = dst.double().index_add_(0, torch.tensor(T.SCATTER_IDX), src.double())
    assert rel(T.scatter_add(src, dst), ref.numpy()) <= 1e-12
    n = 1
    B, npr, skip, C = T.WE_CASES[n]
    rows, _ = T.we_layout(n)
    dx, tok = T.we_inputs(n)
    used = dx.view(B, rows, C)[:, skip:skip + npr].reshape(B * npr, C).double()
    ex = T.wordembed(dx, tok, B, npr, rows, skip)
    assert rel(ex.dW, (used.t() @ tok.double()).numpy()) <= 1e-12 and rel(ex.db, used.sum(0).numpy()) <= 1e-12
    n = 6
    x, f, gate, rs = T.gr_inputs(n)
    dt, _, gr, C, M = T.GR_CASES[n]
    g = (gate.double() * rs.double()[:, None]).repeat_interleave(gr, 0)[:M]
    assert rel(T.gate_residual(x, f, gate, rs, gr).y, (x.double() + g * f.double()).numpy()) <= 1e-12


def test_sumsq_and_clip_oracles_against_clip_grad_norm_float64():
    xs = [T.sumsq_inputs(n) for n in (2, 4, 6)]
    parts = np.concatenate([T.sumsq(x).partial for x in xs])
    ps = [torch.zeros(x.numel(), dtype=F64).requires_grad_(True) for x in xs]
    for p, x in zip(ps, xs):
        p.grad = x.double().clone()
    total = torch.nn.utils.clip_grad_norm_(ps, 2.0).item()
    ex = T.clip_coef(parts, parts.size, 1.0, 2.0)
    assert abs(ex.norm - total) <= 1e-12 * total and abs(ex.coef - min(1.0, 2.0 / (total + 1e-6))) <= 1e-12
    assert rel(ps[0].grad.numpy(), (xs[0].double() * ex.coef).numpy()) <= 1e-12
    for x in xs:
        assert abs(T.sumsq(x).partial.sum() - float((x.double() ** 2).sum())) <= 1e-12 * float((x.double() ** 2).sum())
    assert T.clip_coef(parts, parts.size, 0.5, 0.0).coef == 1.0 and T.clip_coef(parts, parts.size, 0.5, -1.0).coef == 1.0
    assert abs(T.clip_coef(parts, parts.size, 0.5, 2.0).norm - 0.5 * total) <= 1e-12 * total


# ------------------------------------------------------------------------------------------------ per-case evaluation
def adam_eval(n, fault=None):
    """-> {'p', 'm', 'v': model error / bound}, the largest p error in units of u (|p'| + |p| + A)"""
    p, g, m, v, blk = T.adam_inputs(n)
    kw = T.adam_args(n)
    ex = once(('adam', n), lambda: T.adamw(p, g, m, v, **kw))
    md = T.adamw_model(p, g, m, v, fault=fault, **kw)
    r = dict(p=T.ratio_of(md.p - ex.p, ex.p_bound), m=T.ratio_of(md.m - ex.m, ex.m_bound), v=T.ratio_of(md.v - ex.v, ex.v_bound))
    return r, r['p'] * T.ADAM_K_P


def adam_multi_eval(name, fault=None):
    sizes, groups, lrs, wds, w16 = T.ADAM_MULTI[name]
    worst = {}
    for i, (p, g, m, v) in enumerate(T.adam_multi_inputs(name)):
        kw = dict(T.ADAM_MULTI_ARGS, lr=lrs[groups[i]], wd=wds[groups[i]])
        ex = T.adamw(p, g, m, v, **kw)
        md = T.adamw_model(p, g, m, v, **dict(kw, wd=wds[0] if fault == 'group0_wd' else kw['wd']))
        worst[i] = max(T.ratio_of(md.p - ex.p, ex.p_bound), T.ratio_of(md.m - ex.m, ex.m_bound), T.ratio_of(md.v - ex.v, ex.v_bound))
    return worst


def ce_eval(n, fault=None):
    lg, tgt, w, gs = T.ce_inputs(n)
    ex = once(('ce', n), lambda: T.ce(lg, tgt, w, gs))
    md = T.ce_model(lg, tgt, w, gs, fault=fault)
    return dict(loss=T.ratio_of(T.abs_err(md.loss, ex.loss), ex.loss_bound), dl=T.ratio_of(T.abs_err(md.dlogits, ex.dlogits), ex.dl_bound),
                dl_bf16=T.ratio_of(T.abs_err(T.bf16_round(md.dlogits), ex.dlogits), ex.dl_bound + T.BF16_HALF_ULP * np.abs(ex.dlogits)))


def colsum_eval(n, fault=None):
    A, o = T.colsum_inputs(n)
    o = o if T.colsum_layout(n)[3] else None
    ref, yard = T.colsum(A, o), T.colsum(A, o, dtype=np.float32)
    return T.ratio_of(T.colsum_model(A, o, fault=fault) - ref, T.colsum_bound(A, o, ref, yard).bound)


def we_eval(n, fault=None):
    B, npr, skip, C = T.WE_CASES[n]
    rows, _ = T.we_layout(n)
    dx, tok = T.we_inputs(n)
    ex, y32 = once(('we', n), lambda: (T.wordembed(dx, tok, B, npr, rows, skip), T.wordembed(dx, tok, B, npr, rows, skip, dtype=np.float32)))
    md = T.wordembed_model(dx, tok, B, npr, rows, skip, fault=fault)
    bw, bb = T.we_bounds(n, ex, y32)
    return T.ratio_of(md.dW - ex.dW, bw.bound), T.ratio_of(md.db - ex.db, bb.bound)


def act_eval(n, dt, fault=None):
    a, dh = T.act_inputs(n, dt)
    ex, md = T.gelu(a, dh), T.gelu_model(a, dh, fault=fault)
    sx, sm = T.silu_bwd(a.float(), dh.float()), T.silu_bwd_model(a.float(), dh.float(), fault=fault)
    return dict(gelu=T.ratio_of(T.abs_err(md.y, ex.y), ex.y_bound), gelu_bwd=T.ratio_of(T.abs_err(md.dy, ex.dy), ex.dy_bound),
                silu_bwd=T.ratio_of(T.abs_err(sm.dx, sx.dx), sx.bound),
                gelu_rounded=T.ratio_of(T.abs_err(T.bf16_round(md.y), ex.y), ex.y_bound + T.BF16_HALF_ULP * np.abs(ex.y)),
                gelu_bwd_rounded=T.ratio_of(T.abs_err(T.bf16_round(md.dy), ex.dy), ex.dy_bound + T.BF16_HALF_ULP * np.abs(ex.dy)))


# ------------------------------------------------------------------------------------------------ the tables cover what they claim
def test_case_tables_name_every_size_step_and_edge():
    c = T.ADAM_CASES.values()
    assert {x[0] for x in c} == set(T.ADAM_N) and {(x[1], x[2]) for x in c if x[0] == 10007} >= {(s, b) for s in T.ADAM_STEPS for b in T.ADAM_BETAS}
    assert {x[3] for x in c} == {0.0, 0.05} and any(x[4] == 0 for x in c) and {x[5] is None for x in c} == {True, False}
    assert {(x[0], x[1]) for x in T.CE_CASES.values()} == {(V, f) for V in T.CE_V for f in T.CE_FAMILIES} and {x[2] for x in T.CE_CASES.values()} == set(T.CE_WEIGHTS)
    assert {x[1] for x in T.COLSUM_CASES.values()} == set(T.COLSUM_M) and {x[2] for x in T.COLSUM_CASES.values()} >= {1, 8, 200, 264, 520}
    assert [T.colsum_segments(M) for M in (63, 64, 127, 128, 4095, 4097)] == [(1, 63), (1, 64), (1, 127), (2, 64), (63, 65), (64, 65)]
    assert {x[2] for x in T.ROWSUM_CASES.values()} == set(T.ROWSUM_NCOLS) and {x[1] for x in T.ROWSUM_CASES.values()} == {1, 3, 4, 5}
    assert [T.wordembed_slices(B * n)[0] for B, n, s, C in T.WE_CASES.values()] == [1, 4, 4, 16, 16, 32]
    assert [B * n for B, n, s, C in T.WE_CASES.values()] == [255, 256, 4095, 4096, 32767, 32768]
    for B, n, s, C in T.WE_CASES.values():      # a slice holds a sample boundary
        assert B == 1 or T.wordembed_slices(B * n)[1] != n
    assert {x[0] for x in T.CLIP_CASES.values()} == set(T.CLIP_COUNTS) and {x[3] for x in T.CLIP_CASES.values()} == {'mid', 'below', 'huge', 'zero'}
    dt, rs, gr, C, M = T.GR_CASES[max(T.GR_CASES)]
    assert M * (C // 4) > 8192 * 256


# ------------------------------------------------------------------------------------------------ bounds are feasible
def test_adamw_models_inside_half_the_bound():
    print('\n[train_host] adamw model / bound                                        p      m      v    p in u (|p\'| + |p| + A)')
    for n in T.ADAM_CASES:
        r, pu = adam_eval(n)
        print(f'[train_host] {T.adam_name(n):58s} {r["p"]:6.3f} {r["m"]:6.3f} {r["v"]:6.3f}   {pu:5.2f}')
        assert max(r.values()) <= 0.5, (T.adam_name(n), r)
    for name in T.ADAM_MULTI:
        w = adam_multi_eval(name)
        print(f'[train_host] adamw_multi {name}: worst model / bound per tensor', {k: round(v, 3) for k, v in w.items()})
        assert max(w.values()) <= 0.5, (name, w)


def test_adamw_exact_cases():
    """lr = 0 leaves p's bits alone; the all-zero block gives exactly 0 without NaN"""
    n = [k for k, c in T.ADAM_CASES.items() if c[4] == 0.0][0]
    p, g, m, v, blk = T.adam_inputs(n)
    md = T.adamw_model(p, g, m, v, **T.adam_args(n))
    assert np.array_equal(md.p.view(np.int32), p.numpy().view(np.int32)) and not np.array_equal(md.m, m.numpy())
    for n in (3, 9):
        p, g, m, v, blk = T.adam_inputs(n)
        md, ex = T.adamw_model(p, g, m, v, **T.adam_args(n)), T.adamw(p, g, m, v, **T.adam_args(n))
        z = blk == 3
        assert z.any() and all((t[z] == 0).all() for t in (md.p, md.m, md.v, ex.p, ex.m, ex.v))


def test_ce_models_inside_half_the_bound():
    print('\n[train_host] ce model / bound                                  loss      dl   dl as bf16 (of the whole bound)')
    for n in T.CE_CASES:
        r = ce_eval(n)
        print(f'[train_host] {T.ce_name(n):48s} {r["loss"]:6.3f} {r["dl"]:6.3f}   {r["dl_bf16"]:6.3f}')
        assert r['loss'] <= 0.5 and r['dl'] <= 0.5 and r['dl_bf16'] <= 1.0, (T.ce_name(n), r)


def test_reduction_models_inside_half_the_bound():
    print('\n[train_host] reductions: model / bound')
    for n in T.COLSUM_CASES:
        r = colsum_eval(n)
        print(f'[train_host] colsum {T.colsum_name(n):40s} {r:6.3f}')
        assert r <= 0.5, T.colsum_name(n)
    for n, (dt, R, nc) in T.ROWSUM_CASES.items():
        A, o = T.rowsum_inputs(n)
        o = o if n % 2 == 0 else None
        vec = 4 if dt == 'f32' else 8
        ref, yard = T.rowsum(A, o), T.rowsum(A, o, dtype=np.float32)
        r = T.ratio_of(T.rowsum_model(A, vec, o) - ref, T.rowsum_bound(A, vec, o, ref, yard).bound)
        print(f'[train_host] rowsum {n}-{dt}-{R}x{nc}: {r:6.3f}')
        assert r <= 0.5, n
    for n in T.WE_CASES:
        rw, rb = we_eval(n)
        print(f'[train_host] wordembed {T.we_name(n):40s} dW {rw:6.3f}  db {rb:6.3f}')
        assert max(rw, rb) <= 0.5, T.we_name(n)
    for C in T.SCATTER_C:
        src, dst = T.scatter_inputs(C)
        ref, yard = T.scatter_add(src, dst), T.scatter_add(src, dst, dtype=np.float32)
        r = T.ratio_of(yard - ref, T.scatter_bound(src, dst, ref, ref).bound)          # the float32 oracle is the kernel's order: held to the floor alone
        print(f'[train_host] scatter_add_rows C{C}: {r:6.3f}')
        assert r <= 0.5, C


def test_sumsq_and_clip_models_inside_half_the_bound():
    for n in T.SUMSQ_CASES:
        x = T.sumsq_inputs(n)
        ex = T.sumsq(x)
        r = T.ratio_of(T.sumsq_model(x) - ex.partial, ex.bound)
        print(f'[train_host] sumsq {n}-{T.SUMSQ_CASES[n]}: {r:6.3f}  (partials {ex.partial.min():.3e} .. {ex.partial.max():.3e})')
        assert r <= 0.5 and np.isfinite(ex.partial).all(), n
    worst = 0.0
    for n, (c, ps, mn, kind) in T.CLIP_CASES.items():
        part = T.clip_inputs(n)
        ex, md = T.clip_coef(part, c, ps, mn), T.clip_coef_model(part, c, ps, mn)
        # the outputs' float32 rounding is the bound's u term: before it the model is held to 0.5 of the rest, after it to the whole bound
        dbl = 1 - T.U / T._clip_bound_rel(c)
        r = max(T.ratio_of(md.norm64 - ex.norm, dbl * ex.norm_bound), T.ratio_of(md.coef64 - ex.coef, dbl * ex.coef_bound))
        whole = max(T.ratio_of(md.norm - ex.norm, ex.norm_bound), T.ratio_of(md.coef - ex.coef, ex.coef_bound))
        worst = max(worst, r)
        assert r <= 0.5 and whole <= 1.0, (n, T.CLIP_CASES[n], r, whole)
        if kind in ('below', 'zero') or mn <= 0:
            assert md.coef == 1.0 and ex.coef_bound == 0.0
        if kind == 'zero':
            assert md.norm == 0.0
    print(f'[train_host] clip_coef: worst model / bound {worst:.3f} (before the float32 rounding of the outputs)')


def test_activation_and_gate_models_inside_half_the_bound():
    print('\n[train_host] activations: model / bound       gelu  gelu_bwd  silu_bwd   gelu, gelu_bwd as bf16 (whole bound)')
    for n in T.ACT_N + (4099,):
        for dt in ('f32', 'bf16'):
            r = act_eval(n, dt)
            print(f'[train_host] n{n}-{dt:5s}                          {r["gelu"]:6.3f}   {r["gelu_bwd"]:6.3f}   {r["silu_bwd"]:6.3f}   {r["gelu_rounded"]:6.3f} {r["gelu_bwd_rounded"]:6.3f}')
            assert max(r['gelu'], r['gelu_bwd'], r['silu_bwd']) <= 0.5 and max(r['gelu_rounded'], r['gelu_bwd_rounded']) <= 1.0, (n, dt, r)
    a, dh = T.act_inputs(257, 'f32')
    md = T.gelu_model(a, dh)
    assert np.isfinite(md.y).all() and np.isfinite(md.dy).all() and np.isfinite(T.silu_bwd_model(a, dh).dx).all()
    for n in list(T.GR_CASES)[:-1]:
        x, f, gate, rs = T.gr_inputs(n)
        ex, y32 = T.gate_residual(x, f, gate, rs, T.GR_CASES[n][2]), T.gate_residual(x, f, gate, rs, T.GR_CASES[n][2], dtype=np.float32)
        r = T.ratio_of(y32.y - ex.y, ex.bound)           # elementwise: the float32 yardstick is the kernel's own arithmetic
        assert r <= 0.5, T.gr_name(n)


# ------------------------------------------------------------------------------------------------ bounds discriminate
def test_planted_faults_land_outside_the_bounds():
    rows = []
    late = [k for k, c in T.ADAM_CASES.items() if c[:3] == (10007, 1000, (0.9, 0.999))][0]
    s7 = [k for k, c in T.ADAM_CASES.items() if c[:3] == (10007, 7, (0.9, 0.999)) and c[4] > 0][0]
    gs7 = [k for k, c in T.ADAM_CASES.items() if c[1] == 7 and c[5] is not None and c[0] >= 255][0]
    s2 = [k for k, c in T.ADAM_CASES.items() if c[:3] == (10007, 2, (0.9, 0.999))][0]
    wd7 = [k for k, c in T.ADAM_CASES.items() if c[:2] == (10007, 7) and c[3] > 0 and c[4] > 0][0]
    rows.append(('adamw eps_inside', T.adam_name(late), adam_eval(late, 'eps_inside')[0]['p']))
    rows.append(('adamw bc2_for_sqrt', T.adam_name(late), adam_eval(late, 'bc2_for_sqrt')[0]['p']))
    rows.append(('adamw decay_after', T.adam_name(wd7), adam_eval(wd7, 'decay_after')[0]['p']))
    rows.append(('adamw unscaled_moment', T.adam_name(gs7), adam_eval(gs7, 'unscaled_moment')[0]['m']))
    rows.append(('adamw_multi group0_wd', 'six', max(adam_multi_eval('six', 'group0_wd').values())))
    rows.append(('adamw powf step 2', T.adam_name(s2), adam_eval(s2, 'powf')[0]['p']))
    rows.append(('adamw powf step 7', T.adam_name(s7), adam_eval(s7, 'powf')[0]['p']))
    cen = [k for k, c in T.CE_CASES.items() if c[:3] == (4096, 'normal', 'none') or (c[0] == 4096 and c[1] == 'normal')][0]
    cew = [k for k, c in T.CE_CASES.items() if c[2] == 'mixed' and c[1] == 'normal' and c[3] != 1.0][0]
    rows.append(('ce inv_before_last_partial', T.ce_name(cen), ce_eval(cen, 'inv_before_last_partial')['dl']))
    rows.append(('ce onehot_unweighted', T.ce_name(cew), ce_eval(cew, 'onehot_unweighted')['dl']))
    n = [k for k, c in T.CLIP_CASES.items() if c[3] == 'mid' and c[2] == 2.0][0]
    c, ps, mn, kind = T.CLIP_CASES[n]
    ex = T.clip_coef(T.clip_inputs(n), c, ps, mn)
    for fault in T.CLIP_FAULTS:
        if fault == 'pre_scale_inside':
            n2 = [k for k, cc in T.CLIP_CASES.items() if cc[3] == 'mid' and cc[2] == 2.0 and cc[1] != 1.0][0]
            c2, ps2, mn2, _ = T.CLIP_CASES[n2]
            e2, md = T.clip_coef(T.clip_inputs(n2), c2, ps2, mn2), T.clip_coef_model(T.clip_inputs(n2), c2, ps2, mn2, fault)
            rows.append((f'clip {fault}', str(T.CLIP_CASES[n2]), abs(md.norm - e2.norm) / e2.norm_bound))
        else:
            md = T.clip_coef_model(T.clip_inputs(n), c, ps, mn, fault)
            rows.append((f'clip {fault}', str(T.CLIP_CASES[n]), abs(md.coef - ex.coef) / ex.coef_bound))
    cs = [k for k, c in T.COLSUM_CASES.items() if c[1] == 4097 and c[3] == 'unit'][0]
    rows.append(('colsum drop_last_row', T.colsum_name(cs), colsum_eval(cs, 'drop_last_row')))
    rows.append(('wordembed no_skip_after_first_sample', T.we_name(3), max(we_eval(3, 'no_skip_after_first_sample'))))
    rows.append(('gelu_bwd gelu_c3', 'n257 f32', act_eval(257, 'f32', 'gelu_c3')['gelu_bwd']))
    rows.append(('silu_bwd silu_no_one', 'n257 f32', act_eval(257, 'f32', 'silu_no_one')['silu_bwd']))
    print('\n[train_host] planted fault                           case                                                        error / bound')
    for fault, name, r in rows:
        print(f'[train_host] {fault:40s} {name:58s} {r:12.3g}')
    # the float32 powf corrections (11 u against 8 u at step 7) and the dropped 1e-6 (1.6e-7 of a norm of 6.3) are the smallest faults of the list
    assert all(r > 1.0 for _, _, r in rows), [x for x in rows if not x[2] > 1.0]
    assert all(r >= 3 for f, _, r in rows if 'step 7' not in f), [x for x in rows if x[2] < 3]
    # and the default betas do not care which way the corrections are formed (the fix moves nothing there)
    d7 = [k for k, c in T.ADAM_CASES.items() if c[:3] == (10007, 7, (0.9, 0.95))][0]
    assert adam_eval(d7, 'powf')[0]['p'] <= 0.5
