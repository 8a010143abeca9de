"""CPU checks of the cached (inference) forward in oracle/attn_ref.py, the judge of tests/test_gpu_attn_fwd_oracle.py: the case
table against what the entry points accept, the visibility contract against the training one and the reference's mask, the float64
oracle against the training oracle, and the two conditions on the INPUTS the GPU bound rests on - the bf16 emulation stays within
5e-3 of float64 in the per-row metric (so the bound 3 x emulation is < 1.5e-2), and a forward that is wrong at the end of the key
range or in its level table is several bounds away."""
import pytest
import torch

from oracle import attn_ref as A

torch.set_num_threads(8)

LEVELS, HOLES = 9, 10                      # case numbers of the teacher-forced and the indep / separate_decoding structure
Q64, PLAIN_MAP, XCD_MAP = 12, 4, 7


def cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope='module')
def solved():
    """(case, scale) -> dict of operands, mask and per query form ('pre': q' with ln 2, 'raw': q with scale) the float64 out / lse
    and the emulation's row error against it, computed once"""
    res = {}
    for n, scale in A.FWD_RUNS:
        R, H, Lmax, q_off, l, ends, holes = A.FWD_CASES[n]
        kv, q, qp = A.fwd_case_inputs(n, scale)
        vis = A.visibility_cached(q_off, l, ends, holes)
        d = dict(kv=kv, vis=vis, R=R)
        for form, (qq, s_mul) in dict(pre=(qp, A.LN2), raw=(q, scale)).items():
            out, lse = A.attention_cached_f64(qq, kv, s_mul, vis)
            out_e, lse_a, lse_b = A.attention_cached_emulated(qq, kv, s_mul, vis)
            d[form] = dict(q=qq, s_mul=s_mul, out=out, lse=lse, yard=A.row_error_fwd(out_e, out, R),
                           lse_yard=(float((lse_a - lse).abs().max()), float((lse_b - lse).abs().max())))
        res[n, scale] = d
    return res


def test_case_table_is_what_the_kernels_accept():
    """q_off + l <= Lmax; strictly increasing ends that finish at q_off + l, at most 32 levels, every hole in front of its own level
    and none over all of [0, 64) (the prescaled entry point refuses that); case 12 meets the 64-query rule of cvar_attention_impl
    and its first two samples alone do not; cases 4 and 7 take the plain and the XCD-grouped block-id mapping."""
    assert sorted(A.FWD_CASES) == list(range(1, 14))
    for n, (R, H, Lmax, q_off, l, ends, holes) in A.FWD_CASES.items():
        assert R >= 1 and H >= 1 and l >= 1 and q_off >= 0 and q_off + l <= Lmax, n
        assert R >= 4 or n == 11
        if ends:
            assert len(ends) <= 32 and ends[-1] == q_off + l and all(a < b for a, b in zip([0] + ends, ends)), n
        if holes:
            assert len(holes) == len(ends)
            for (lo, hi), begin in zip(holes, [0] + ends[:-1]):
                assert hi <= lo or (0 <= lo and hi <= begin), n
                assert not (hi > lo and lo <= 0 and hi >= 64), n
    rule = lambda R, H, l: l >= 192 and cdiv(l, 256) * 256 - l < 64 and cdiv(l, 256) * H * R >= 512
    R, H, _, _, l, _, _ = A.FWD_CASES[Q64]
    assert rule(R, H, l) and not rule(2, H, l)
    assert [n for n, (R, H, _, _, l, _, _) in A.FWD_CASES.items() if rule(R, H, l)] == [Q64]
    assert (A.FWD_CASES[PLAIN_MAP][0] * A.FWD_CASES[PLAIN_MAP][1]) % 8 != 0
    assert (A.FWD_CASES[XCD_MAP][0] * A.FWD_CASES[XCD_MAP][1]) % 8 == 0
    assert A.FWD_CASES[4][2] > A.FWD_CASES[4][3] + A.FWD_CASES[4][4]            # arena rows behind q_off + l
    assert (A.FWD_CASES[5][3] + A.FWD_CASES[5][4]) % 64 == 0                    # key count on a tile edge
    assert A.FWD_CASES[A.COS_CASE][:5] == A.FWD_CASES[XCD_MAP][:5]
    assert sorted(A.FWD_RUNS) == sorted(set(A.FWD_RUNS)) and len(A.FWD_RUNS) == 18


def test_case_inputs_are_bf16_values_in_their_regimes():
    """operands are bf16 values; q' is one rounding of bf16(q) * scale * log2 e; the spike, the near-uniform and the all-negative
    sample are where the docstring puts them; case 13 has unit-norm keys and queries of norm 100, 30, 5, 100"""
    R, H, Lmax, q_off, l, _, _ = A.FWD_CASES[3]
    kv, q, qp = A.fwd_case_inputs(3, 0.125)
    for t in (kv, q, qp):
        assert t.dtype == torch.float32 and torch.equal(t, t.to(torch.bfloat16).float())
    assert torch.equal(qp, (q.double() * (0.125 * A.LOG2E)).float().to(torch.bfloat16).float())
    kn = kv[..., :H * 64].norm(dim=-1)
    assert int(kn[1].argmax()) == (q_off + l - 1) // 2 and float(kn[1].max()) > 8 * float(kn[0].max())
    assert float(q[2].abs().max()) < 0.1 * float(q[0].abs().max())
    assert float(q[3].min()) >= 0 and float(kv[3, :, :H * 64].max()) <= 0
    assert torch.equal(A.fwd_case_inputs(3, 1.0)[0], kv) and torch.equal(A.fwd_case_inputs(3, 1.0)[1], q)
    R, H, Lmax, q_off, l, _, _ = A.FWD_CASES[A.COS_CASE]
    kv, q, _ = A.fwd_case_inputs(A.COS_CASE, 1.0)
    assert float((kv[..., :H * 64].view(R, Lmax, H, 64).norm(dim=-1) - 1).abs().max()) < 2.0 ** -7
    qn = q.view(R, l, H, 64).norm(dim=-1)
    for r, want in enumerate(A.COS_Q_NORMS):
        assert float((qn[r] / want - 1).abs().max()) < 2.0 ** -7


def test_visibility_cached_is_the_rows_of_the_training_visibility():
    for n, (R, H, Lmax, q_off, l, ends, holes) in A.FWD_CASES.items():
        v = A.visibility_cached(q_off, l, ends, holes)
        assert v.shape == (l, q_off + l) and v.dtype == torch.bool
        assert torch.equal(v, A.visibility(q_off + l, ends, holes)[q_off:])
        assert bool(v.any(1).all()) and (ends is not None or bool(v.all()))
    # level ends are absolute positions: the same call cut out of the whole sequence's mask
    ends, holes = A.FWD_CASES[HOLES][5:]
    whole = A.visibility(120, ends, holes)
    assert torch.equal(A.visibility_cached(40, 80, ends, holes), whole[40:120, :120])
    assert torch.equal(A.visibility_cached(0, 40, ends[:2], holes[:2]), whole[:40, :40])


def test_visibility_cached_equals_the_reference_mask_scale_by_scale():
    """indep + separate_decoding: one cached call per scale with the level table cut at the scale's end sees what the attention bias
    of the functional oracle (oracle.var_ref) lets rows [begin, end) see; the level ends of case 10 are two scales of this structure"""
    from controlvar_amd.spec import VarConfig, attention_levels
    from controlvar_amd.synth import synth_var_state
    from oracle import var_ref  # noqa: F401  (the consumer of sd['attn_bias_for_masking'])
    cfg = VarConfig(depth=2, separate_decoding=True, indep=True)
    ends, holes = attention_levels(cfg)
    bias = synth_var_state(cfg, 3)['attn_bias_for_masking'][0, 0]
    assert holes is not None
    for i, (b, e) in enumerate(zip(cfg.pyramid.begin, cfg.pyramid.end)):
        n_lvl = 2 * (i + 1)
        assert ends[n_lvl - 1] == e
        assert torch.equal(A.visibility_cached(b, e - b, ends[:n_lvl], holes[:n_lvl]), (bias == 0)[b:e, :e]), i
    _, _, _, q_off, l, ends10, holes10 = A.FWD_CASES[HOLES]
    halves = lambda bounds: [x for b, e in bounds for x in (b + (e - b) // 2, e)]
    assert ends10 == halves([(0, q_off), (q_off, q_off + l)])
    assert holes10[3] == (q_off, q_off + l // 2)            # the image half of the call's scale does not see its control half


def test_cached_oracle_equals_the_training_oracle_at_q_off_0():
    """attention_cached_f64 on (q third, k | v thirds) of the training cases: out and lse of attention_fwd_bwd_f64 to 1e-12; and the
    emulation wrapper is the generalised emulation on the same split"""
    for n, (R, H, l, Lmax, ends, holes) in A.CASES.items():
        qkv, dout = A.case_inputs(n)
        C = H * 64
        vis = A.visibility(l, ends, holes)
        assert torch.equal(vis, A.visibility_cached(0, l, ends, holes))
        ex = A.attention_fwd_bwd_f64(qkv, dout, A.SCALE, vis)
        out, lse = A.attention_cached_f64(qkv[..., :C], qkv[..., C:], A.SCALE, vis)
        assert float((out - ex.out).abs().max()) <= 1e-12 and float((lse - ex.lse).abs().max()) <= 1e-12, n
        a, b = A.attention_fwd_emulated(qkv, A.SCALE, vis), A.attention_cached_emulated(qkv[..., :C], qkv[..., C:], A.SCALE, vis)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_cached_oracle_reads_only_the_visible_arena_rows_and_both_query_forms_agree():
    """rows [q_off + l, Lmax) of the arena do not enter; q' with ln 2 is q with scale up to the one rounding of q'"""
    R, H, Lmax, q_off, l, _, _ = A.FWD_CASES[4]
    kv, q, qp = A.fwd_case_inputs(4, 0.125)
    vis = A.visibility_cached(q_off, l)
    out, lse = A.attention_cached_f64(q, kv, 0.125, vis)
    kv2 = kv.clone()
    kv2[:, q_off + l:] = float('nan')
    out2, lse2 = A.attention_cached_f64(q, kv2, 0.125, vis)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    out_x, _ = A.attention_cached_f64(q.double() * (0.125 * A.LOG2E), kv, A.LN2, vis)
    assert float((out_x - out).abs().max()) <= 1e-12
    out_p, _ = A.attention_cached_f64(qp, kv, A.LN2, vis)
    assert 0 < A.row_error_fwd(out_p, out, R)[0] < 5e-2


def test_row_error_fwd_takes_its_floor_per_sample():
    ref = torch.ones(2 * 3, 128, dtype=torch.float64)
    ref[3:] *= 1e-3                                                      # sample 1 is a thousand times smaller
    got = ref.clone()
    got[4, 64:] *= 1.1
    worst, per = A.row_error_fwd(got, ref, 2)
    assert per[0] == 0.0 and abs(per[1] - 0.1 / 1.05) < 1e-12 and worst == per[1]
    got[0, 0] = float('nan')
    assert A.row_error_fwd(got, ref, 2)[0] == float('inf')


def test_emulation_stays_inside_the_yardstick_condition(solved):
    """a condition on the INPUTS of the GPU test (seed = case number), not a measurement of any kernel: the bf16 emulation's
    row_error_fwd against float64 is <= 5e-3 for every case, every sample, both scales and both query forms, so the GPU bound
    3 x max(emulation, 1e-3) is < 1.5e-2 everywhere."""
    for (n, scale), d in solved.items():
        for form in ('pre', 'raw'):
            worst, per = d[form]['yard']
            print(f'[attn fwd yardstick] case {n} scale {scale} {form}: ' + ' '.join(f'{v:.2e}' for v in per)
                  + '  lse %.1e / %.1e' % d[form]['lse_yard'])
            assert all(v <= 5e-3 for v in per), (n, scale, form, per)
            assert worst > 0 and 3 * max(worst, 1e-3) < 1.5e-2


def test_a_forward_wrong_at_the_end_of_the_key_range_is_far_above_the_bound(solved):
    """a condition on the inputs at scale 0.125, cases 2 - 12: the float64 forward that ignores every query's last visible key moves
    EVERY sample's row_error_fwd by at least twice the case's bf16 bound 3 x max(emulation, 1e-3) - in both query forms.  Scale 1.0
    and case 13 carry no such condition: a one-hot row does not depend on its last key; those runs are there for the shift
    arithmetic (first-tile shift below -128, scores of +-90 in the log2 domain)."""
    for n in range(2, 13):
        d = solved[n, A.FWD_SCALE]
        wrong_vis = A.drop_last_visible_key(d['vis'])
        for form in ('pre', 'raw'):
            f = d[form]
            limit = 3 * max(f['yard'][0], 1e-3)
            _, per = A.row_error_fwd(A.attention_cached_f64(f['q'], d['kv'], f['s_mul'], wrong_vis)[0], f['out'], d['R'])
            print(f'[attn fwd sensitivity] case {n} {form}, last visible key ignored: ' + ' '.join(f'{v:.3f}' for v in per) + f'  bound {limit:.2e}')
            assert all(v >= 2 * limit for v in per), (n, form, per, limit)


def test_the_whole_tensor_metric_lets_the_same_wrong_forward_through(solved):
    """what the per-row metric is for: on case 8 the forward without each query's last visible key stays below the 1.2e-2 that
    test_attention_prescaled_equals_the_reference_softmax asserts on max|got - ref| / max|ref|"""
    d = solved[8, A.FWD_SCALE]
    f = d['pre']
    wrong = A.attention_cached_f64(f['q'], d['kv'], f['s_mul'], A.drop_last_visible_key(d['vis']))[0]
    whole = float((wrong - f['out']).abs().max() / f['out'].abs().max())
    print(f'[attn fwd sensitivity] case 8, whole-tensor metric of the forward without the last visible key: {whole:.2e}')
    assert whole < 1.2e-2 < A.row_error_fwd(wrong, f['out'], d['R'])[0]


@pytest.mark.parametrize('n', [LEVELS, HOLES])
def test_a_wrong_level_table_is_far_above_the_bound(solved, n):
    """cases 9 and 10 at scale 0.125: every inner level end one too large, and (case 10) the holes ignored, move every sample by >= 0.2"""
    R, H, Lmax, q_off, l, ends, holes = A.FWD_CASES[n]
    d = solved[n, A.FWD_SCALE]
    wrong = {'inner ends + 1': A.visibility_cached(q_off, l, [e + 1 for e in ends[:-1]] + ends[-1:], holes)}
    if holes:
        wrong['holes ignored'] = A.visibility_cached(q_off, l, ends, None)
    for what, vis_w in wrong.items():
        for form in ('pre', 'raw'):
            f = d[form]
            _, per = A.row_error_fwd(A.attention_cached_f64(f['q'], d['kv'], f['s_mul'], vis_w)[0], f['out'], R)
            print(f'[attn fwd sensitivity] case {n} {form}, {what}: ' + ' '.join(f'{v:.2f}' for v in per))
            assert all(v >= 0.2 for v in per), (n, what, form, per)
