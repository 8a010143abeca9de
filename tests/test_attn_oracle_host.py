"""CPU checks of oracle/attn_ref.py, the judge of tests/test_gpu_attn_train_oracle.py: the float64 oracle against a second
formula, the visibility contract against the reference's mask, the rounding yardstick on every case of the shared table, and the
size of the two structural errors the GPU bound has to stay below."""
import pytest
import torch

from oracle import attn_ref as A

torch.set_num_threads(8)

TENSORS = ('dQ', 'dK', 'dV')
RAGGED, HOLES = 6, 9                       # case numbers of the ragged and the hole structure


@pytest.fixture(scope='module')
def solved():
    """case number -> (qkv, dout, vis, float64 oracle), computed once"""
    res = {}
    for n, (R, H, l, Lmax, ends, holes) in A.CASES.items():
        qkv, dout = A.case_inputs(n)
        vis = A.visibility(l, ends, holes)
        res[n] = (qkv, dout, vis, A.attention_fwd_bwd_f64(qkv, dout, A.SCALE, vis))
    return res


def test_case_table_is_what_the_kernels_accept():
    """strictly increasing ends that finish at l, at most 32 levels, every hole in front of its own level"""
    assert sorted(A.CASES) == list(range(1, 12))
    for n, (R, H, l, Lmax, ends, holes) in A.CASES.items():
        assert 1 <= l <= Lmax
        if ends:
            assert len(ends) <= 32 and ends[-1] == l and all(a < b for a, b in zip([0] + ends, ends))
        if holes:
            assert len(holes) == len(ends)
            for (lo, hi), begin in zip(holes, [0] + ends[:-1]):
                assert hi <= lo or (0 <= lo and hi <= begin)
    assert len(A.CASES[7][4]) == 32 and A.CASES[3][3] > A.CASES[3][2]
    assert A.CASES[9][5] == [(0, 0), (0, 7), (0, 0), (14, 45), (0, 0), (76, 140), (0, 0), (204, 333)]


@pytest.mark.parametrize('n', [RAGGED, HOLES])
def test_autograd_oracle_equals_the_written_out_backward(solved, n):
    """dV = P^T dO, dS = P o (dP - D), dQ = dS K scale, dK = dS^T Q scale in float64, no autograd: <= 1e-12 relative"""
    qkv, dout, vis, ex = solved[n]
    f = A.attention_bwd_formula(qkv, dout, ex.out, ex.lse, A.SCALE, vis)
    for name in TENSORS:
        a, b = A.thirds(f)[name], A.thirds(ex.dqkv)[name]
        assert float((a - b).abs().max() / b.abs().max()) <= 1e-12, name
    # and the forward: rows of softmax sum to one over the visible keys only
    q, k, v = A.split_heads(qkv)
    p = torch.exp(q @ k.transpose(-1, -2) * A.SCALE - ex.lse[..., None])
    assert float((p * vis).sum(-1).sub(1).abs().max()) <= 1e-12
    assert float((A.heads_to_rows((p * vis) @ v) - ex.out).abs().max()) <= 1e-12


@pytest.mark.parametrize('kw', [dict(), dict(separate_decoding=True, indep=True)], ids=['default', 'sepdec_indep'])
def test_visibility_equals_the_reference_mask(kw):
    """(lvl_end, holes) of the model configuration -> visibility == the attention bias the functional oracle (oracle.var_ref) masks with"""
    from controlvar_amd.spec import VarConfig, attention_levels
    from controlvar_amd.synth import synth_var_state
    from oracle import var_ref  # noqa: F401  (the consumer of sd['attn_bias_for_masking'])
    cfg = VarConfig(depth=2, **kw)
    ends, holes = attention_levels(cfg)
    bias = synth_var_state(cfg, 3)['attn_bias_for_masking'][0, 0]
    assert (holes is not None) == bool(kw)
    assert torch.equal(A.visibility(cfg.pyramid.L, ends, holes), bias == 0)


def test_visibility_edges():
    assert A.visibility(5).all()
    v = A.visibility(6, [2, 6], [(0, 0), (0, 1)])
    assert v.tolist() == [[1, 1, 0, 0, 0, 0]] * 2 + [[0, 1, 1, 1, 1, 1]] * 4


def test_emulation_stays_inside_the_yardstick_condition(solved):
    """a condition on the INPUTS of the GPU test (amp 1.0, scale 0.125, seed = case number): the bf16 emulation's row error against
    the float64 oracle is <= 2e-2 for dQ, dK, dV and out on every case, so that the GPU bound 3 x emulation stays below 6e-2 - a
    factor of four under the smallest structural signature (test_structural_errors_are_far_above_the_bound)."""
    for n, (qkv, dout, vis, ex) in solved.items():
        em = A.attention_bwd_emulated(qkv, dout, ex.out, ex.lse, A.SCALE, vis)
        out, lse_a, lse_b = A.attention_fwd_emulated(qkv, A.SCALE, vis)
        errs = {name: A.row_error(A.thirds(em)[name], A.thirds(ex.dqkv)[name], dout) for name in TENSORS}
        errs['out'] = A.row_error(out, ex.out, dout)
        print(f'[attn yardstick] case {n}: ' + ' '.join(f'{k} {v:.2e}' for k, v in errs.items())
              + f' lse {float((lse_a - ex.lse).abs().max()):.1e} / {float((lse_b - ex.lse).abs().max()):.1e}')
        for name, e in errs.items():
            assert e <= 2e-2, (n, name, e)
        if n == 1:        # one key: P = 1, dQ = dK = 0, dV = dO, out = v - nothing to round
            assert max(errs.values()) == 0.0


def _off_by_one(ends, which, delta):
    e = list(ends)
    e[which] += delta
    return e


@pytest.mark.parametrize('n', [RAGGED, HOLES])
def test_structural_errors_are_far_above_the_bound(solved, n):
    """the two injected errors, applied to the float64 backward's masking only (exact O and lse): the last key of the sequence
    ignored; one level end off by one.  Each moves some token row of dQ, dK or dV by >= 0.2 of its norm - the GPU bound is < 6e-2."""
    R, H, l, Lmax, ends, holes = A.CASES[n]
    qkv, dout, vis, ex = solved[n]
    wrong = {'last key dropped': A.attention_bwd_formula(qkv, dout, ex.out, ex.lse, A.SCALE, vis, drop_last_key=True)}
    for which in (3, len(ends) // 2):
        for delta in (-1, 1):
            vis_w = A.visibility(l, _off_by_one(ends, which, delta), holes)
            wrong[f'end {which} {delta:+d}'] = A.attention_bwd_formula(qkv, dout, ex.out, ex.lse, A.SCALE, vis_w)
    for what, w in wrong.items():
        errs = {name: A.row_error(A.thirds(w)[name], A.thirds(ex.dqkv)[name], dout) for name in TENSORS}
        print(f'[attn sensitivity] case {n}, {what}: ' + ' '.join(f'{k} {v:.2f}' for k, v in errs.items()))
        assert max(errs.values()) >= 0.2, (n, what, errs)


def test_cos_norm_oracle_against_the_closed_form():
    """autograd through normalize * exp(clamp_max) against dx = (g' - x_t (x_t . g')) / |x|, dsm = (g . x_t) sm written out; the
    clamp passes the gradient at equality (torch's clamp_max) and blocks it above"""
    g = torch.Generator().manual_seed(1)
    N, H = 6, 4
    q, k, gq, gk = (torch.randn(N, H, 64, generator=g, dtype=torch.float64) for _ in range(4))
    s = torch.tensor([0.2, 1.4, A.LN100, 5.0], dtype=torch.float32)
    r = A.cos_qk_norm_fwd_bwd_f64(q, k, s, gq, gk)
    sm = s.double().clamp_max(float(torch.tensor(A.LN100, dtype=torch.float32))).exp().view(1, H, 1)
    xt = q / q.norm(dim=-1, keepdim=True)
    dq = (gq * sm - xt * (xt * gq * sm).sum(-1, keepdim=True)) / q.norm(dim=-1, keepdim=True)
    kt = k / k.norm(dim=-1, keepdim=True)
    dk = (gk - kt * (kt * gk).sum(-1, keepdim=True)) / k.norm(dim=-1, keepdim=True)
    dsm = (gq * xt).sum(-1) * sm[..., 0]
    assert float((r.dq - dq).abs().max()) <= 1e-12 * float(dq.abs().max())
    assert float((r.dk - dk).abs().max()) <= 1e-12 * float(dk.abs().max())
    assert float((r.dsm_tok[:, :3] - dsm[:, :3]).abs().max()) <= 1e-12 * float(dsm.abs().max())
    assert float(r.dsm_tok[:, 2].abs().min()) > 0 and float(r.dsm_tok[:, 3].abs().max()) == 0.0
    assert torch.equal(r.norms[..., 0], q.norm(dim=-1)) and abs(float(sm[0, 2, 0]) - 100.0) < 1e-4
    # the bf16 view of the same function stays within bf16 rounding of it, including the head at the clamp
    qb, kb, gqb, gkb = (A.bf16(t) for t in (q, k, gq, gk))
    rb = A.cos_qk_norm_fwd_bwd_f64(qb, kb, s, gqb, gkb)
    edq, edk, edsm = A.cos_qk_norm_bwd_emulated(qb, kb, s, gqb, gkb)
    assert A.row_error(edq, rb.dq, gqb) <= 2e-2 and A.row_error(edk, rb.dk, gkb) <= 2e-2
    assert A.temperature_error(edsm, rb.dsm_tok, gqb, s) <= 1e-2
    assert float(edsm[:, 2].abs().min()) > 0 and float(edsm[:, 3].abs().max()) == 0.0
