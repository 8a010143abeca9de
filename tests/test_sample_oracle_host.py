"""The sampler oracle (oracle/sample_ref.py) checked on the CPU, before tests/test_gpu_sample_oracle.py trusts it: its kept sets against the
reference filter and a brute-force restatement, its hash against hand-computed values, the share of draws and rows it leaves ambiguous on
the GPU test's own inputs (the caps), and the power of the distribution statistic."""
import numpy as np
import pytest
import torch

import sample_cases as C
from oracle import sample_ref as S
from oracle.var_ref import topk_topp_mask_


# ------------------------------------------------------------------------------------------------------------------ kept sets
def brute_kept(x, k, p):
    """the contract, one row at a time, by sorting: Python floats and loops, nothing shared with kept_sets but the rules"""
    x = [float(v) for v in x]
    V = len(x)
    kth = sorted(x, reverse=True)[k - 1] if 0 < k < V else -np.inf
    top = max(x)
    w = [np.exp(v - top) if v >= kth and v > -np.inf else 0.0 for v in x]
    w = [v if v >= S.FLOOR else 0.0 for v in w]
    Z = sum(w)
    tau = -np.inf
    if p > 0:
        keep_from = min(max(1.0 - float(np.float32(p)), 0.0), 1.0)
        tau = top
        for val in sorted(set(x)):
            if sum(wi for wi, xi in zip(w, x) if xi <= val) > keep_from * Z:
                tau = val
                break
    return np.array([xi >= kth and xi >= tau and wi > 0 for xi, wi in zip(x, w)])


@pytest.mark.parametrize('k,p', [(0, 0.0), (40, 0.0), (0, 0.5), (40, 0.9), (0, 0.96), (299, 0.0), (300, 1.0), (150, 0.999)])
def test_kept_mask_equals_the_reference_filter_without_ties(k, p):
    g = np.random.default_rng(5)
    x = (g.standard_normal((64, 300)) * 2.0).astype(np.float32)
    ma, mb, delta, amb = S.kept_sets(x, k, p)
    assert (delta > 0).all() and (delta < 1e-4).all()
    ref = torch.isfinite(topk_topp_mask_(torch.from_numpy(x).double(), k, float(np.float32(p)))).numpy()
    clear = ~amb
    assert clear.sum() >= 60                                    # away from the threshold: nearly every row
    assert np.array_equal(ma[clear], ref[clear]) and np.array_equal(mb[clear], ref[clear])
    for r in np.nonzero(amb)[0]:                                # at the threshold: the reference is one of the two candidates
        assert np.array_equal(ma[r], ref[r]) or np.array_equal(mb[r], ref[r])


@pytest.mark.parametrize('k,p', [(0, 0.0), (20, 0.0), (0, 0.5), (20, 0.9), (0, 0.96), (119, 0.0), (120, 1.0), (60, 0.999), (0, 1e-9), (0, 1.5)])
def test_kept_mask_equals_the_brute_force_restatement_on_ties(k, p):
    g = np.random.default_rng(6)
    x = (np.round(g.standard_normal((24, 120)) * 2.5 * 4) / 4).astype(np.float32)          # the 0.25 grid: ties at both cuts
    x[3, :10] = -np.inf
    x[4, 5:100] = -np.inf                                       # -inf inside the top-k count
    x[5] = np.where(x[5] == 0, -0.0, x[5])
    x[6, 7] -= 40.0                                             # a zero-mass token
    ma, mb, _, amb = S.kept_sets(x, k, p)
    n_tied_cut = 0
    for r in range(x.shape[0]):
        ref = brute_kept(x[r], k, p)
        assert np.array_equal(ma[r], ref) or np.array_equal(mb[r], ref), (r, k, p)
        if not amb[r]:
            assert np.array_equal(ma[r], ref)
        kept_vals = x[r][ref]
        n_tied_cut += int((kept_vals == kept_vals.min()).sum() > 1)
    if 0 < k < 119 or 0 < p < 1:
        assert n_tied_cut > 0                                   # the grid does put ties on the cut


def test_signed_zero_and_zero_mass_rules():
    x = np.full((1, 16), -0.0, dtype=np.float32)
    x[0, :3] = (2.0, 1.0, 0.0)                                  # +0.0 at the third place
    x[0, 12:] = -3.0
    ma, _, _, _ = S.kept_sets(x, 3, 0.0)
    assert ma[0, :12].all() and not ma[0, 12:].any()            # -0.0 == +0.0: the tie with the k-th value is kept
    y = np.zeros((1, 8), dtype=np.float32)
    y[0, 4:] = -28.0                                            # exp(-28) < 2^-40
    ma, mb, _, amb = S.kept_sets(y, 0, 0.0)
    assert not amb[0] and ma[0].tolist() == [True] * 4 + [False] * 4
    assert S.floor_band(np.array([[0.0, -40 * np.log(2.0)]]))[0].tolist() == [False, True]


# ------------------------------------------------------------------------------------------------------------------ the hash
def test_counter_u_pinned_values():
    # splitmix64 against the published test vector (state 0 -> first output of the reference generator)
    assert S.splitmix64(0) == 0xE220A8397B1DCDAF
    # 53-bit numerators (h >> 11), computed by hand with 64-bit wrap-around integer arithmetic, outside this module
    for (seed, stage, key_row, t), top53 in (((0, 0, 0, 0), 0x1B9A7A5C4682A8), ((0, 19, 5, 63), 0x964F60CF2746D),
                                             ((2 ** 64 - 1, 0, 0, 0), 0x562BB73BC7FE2), ((2 ** 63 + 5, 19, 15, 63), 0xEAC5481EED842),
                                             ((1234, 3, 7, 7), 0xB961E2E3D3D98)):
        assert S.counter_u(seed, stage, key_row, t) == top53 / 2.0 ** 53, (seed, stage, key_row, t)
    assert S.counter_u(0, 0, 0, 0) == 0.862607174134685
    h0 = S.splitmix64(0xC0FFEE1234)                             # seed 0
    assert S.counter_u(0, 0, 0, 0) == (S.splitmix64(h0) >> 11) / 2.0 ** 53
    # each field lands where the contract puts it: stage << 48, key_row << 16, t
    assert S.counter_u(0, 19, 5, 63) == (S.splitmix64(h0 ^ (19 << 48) ^ (5 << 16) ^ 63) >> 11) / 2.0 ** 53
    assert S.counter_u(2 ** 64 - 1, 0, 0, 0) == (S.splitmix64(S.splitmix64((2 ** 64 - 1) ^ 0xC0FFEE1234)) >> 11) / 2.0 ** 53
    assert S.counter_u(2 ** 64 + 7, 1, 2, 3) == S.counter_u(7, 1, 2, 3)                       # the seed is taken mod 2^64
    for u in (S.counter_u(0, 0, 0, 0), S.counter_u(2 ** 63 + 5, 19, 15, 63)):
        assert 0.0 <= u < 1.0 and u * 2.0 ** 53 == int(u * 2.0 ** 53)
    g = S.counter_u_grid(11, 3, [0, 1, 2], range(5))
    assert g.shape == (3, 5) and g[2, 4] == S.counter_u(11, 3, 2, 4)


@pytest.mark.parametrize('B', [1, 4])
def test_counter_u_changes_with_every_key_field(B):
    base = dict(seed=1234, stage=3, d=1, b=B - 1, t=7)

    def u(seed, stage, d, b, t):
        return S.counter_u(seed, stage, d * B + b, t)
    seen = {u(**base)}
    for field, other in (('seed', 1235), ('stage', 4), ('d', 2), ('t', 8)) + ((('b', 0),) if B > 1 else ()):
        v = u(**{**base, field: other})
        assert v not in seen, field
        seen.add(v)
    # all (d, b, t) of a launch at this B draw distinct numbers
    us = {u(1234, 3, d, b, t) for d in range(4) for b in range(B) for t in range(64)}
    assert len(us) == 4 * B * 64


# ------------------------------------------------------------------------------------------------------------------ the caps
def ambiguity(x, k, p, u, srt=None):
    """-> (draws with more than one candidate, draws, rows with two kept sets, rows, rows with more than two)"""
    ma, mb, _, amb = S.kept_sets(x, k, p, srt)
    cand = S.candidates(x, ma, u)
    n = cand.sum(axis=2)
    assert (n >= 1).all()
    return int((n > 1).sum()), n.size, int(amb.sum()), amb.size, int((S.count_classes_between(x[amb], ma[amb], mb[amb]) > 1).sum()) if amb.any() else 0


@pytest.mark.slow
def test_caps_on_the_gpu_tests_inputs():
    """computed from the oracle alone: at most 5 % of a case's draws and 2 % of all draws may have more than one right answer, at most 2 % of
    the rows two right kept sets.  A family that breaks a cap is changed, not the cap."""
    tot_d = tot_n = tot_a = tot_r = 0
    worst = (0.0, None)
    for V, nrep, sigma in C.FAMILIES:
        prm = C.family_params(V, nrep, sigma)
        _, x = C.build(V, nrep, sigma, prm['ldv'])
        u = C.draw_us(prm['seed'], prm['seed_dev'], prm['stage'], prm['n_draw'], 'scalar')
        srt = S.presort(x)
        for k, p in C.filters(V):
            d, n, a, r, many = ambiguity(x, k, p, u, srt)
            assert many == 0, (V, nrep, sigma, k, p)
            assert d <= 0.05 * n, (V, nrep, sigma, k, p, d / n)
            worst = max(worst, (d / n, (V, nrep, sigma, k, p)))
            tot_d, tot_n, tot_a, tot_r = tot_d + d, tot_n + n, tot_a + a, tot_r + r
        # the per-request form of the family
        coef, ks, ps, seeds = C.rows_tables(V, nrep, sigma)
        _, xr = C.build(V, nrep, sigma, prm['ldv'], coef=np.repeat(coef[:, :nrep], C.L, axis=0), tag=1)
        ur = C.draw_us(0, 0, prm['stage'], prm['n_draw'], 'rows', seeds)
        d, n, a, r, many = ambiguity(xr, np.repeat(ks, C.L), np.repeat(ps, C.L), ur)
        assert many == 0 and d <= 0.05 * n, (V, nrep, sigma, 'rows', d / n)
        tot_d, tot_n, tot_a, tot_r = tot_d + d, tot_n + n, tot_a + a, tot_r + r
    print(f'[caps] draws with two candidates: {tot_d} of {tot_n} ({100 * tot_d / tot_n:.3f} %), worst case {100 * worst[0]:.2f} % at {worst[1]}; '
          f'rows with two kept sets: {tot_a} of {tot_r} ({100 * tot_a / tot_r:.3f} %)')
    assert tot_d <= 0.02 * tot_n
    assert tot_a <= 0.02 * tot_r


# ------------------------------------------------------------------------------------------------------------------ power
N_DRAWS = 32768


def test_chi2_limit_closed_form():
    # Wilson-Hilferty at tail 1e-9 against the exact chi-square quantiles (83.479 at 20 dof, 180.480 at 80, 414.545 at 255): within 2.5 %
    for dof, exact in ((20, 83.479), (80, 180.480), (255, 414.545)):
        assert abs(S.chi2_limit(dof) / exact - 1) < 0.025, (dof, S.chi2_limit(dof))
    assert S.chi2_limit(100) < S.chi2_limit(101)


def test_distribution_statistic_passes_right_draws_and_fails_wrong_ones():
    x = S.distribution_row().astype(np.float64)[None]
    mask = np.ones_like(x, dtype=bool)
    probs = S.masses(x)[0] / S.masses(x)[0].sum()
    u = np.random.default_rng(99).random((1, N_DRAWS))
    good = S.draw(x, mask, u)[0]
    stat, dof = S.pearson(good, probs)
    lim = S.chi2_limit(dof)
    lo, hi = S.pair_share_bounds(probs, 1, N_DRAWS)
    share = float((good[1:] == good[:-1]).mean())
    print(f'[power] right draws: chi2 {stat:.1f} <= {lim:.1f} at {dof} dof; equal adjacent pairs {share:.5f} in [{lo:.5f}, {hi:.5f}]')
    assert dof >= 200                                           # the light tokens keep bins of their own
    assert stat <= lim and lo <= share <= hi
    # the same uniform numbers through the CDF of 1.03 x
    tilted = S.draw(1.03 * x, mask, u)[0]
    stat_t, _ = S.pearson(tilted, probs)
    # ... and through a CDF that lost one boundary: a light-group token of about 1 % of the mass never comes out, its neighbour in the walk gets its share
    order, _ = S.cdf(x, mask)
    y = x.copy()
    j = 100
    y[0, order[j]] = np.log(0.01 / (1 - 0.01) * (np.exp(x[0]).sum() - np.exp(x[0, order[j]])))
    py = S.masses(y)[0] / S.masses(y)[0].sum()
    assert abs(py[order[j]] - 0.01) < 1e-9
    uy = np.random.default_rng(98).random((1, N_DRAWS))
    right_y = S.draw(y, mask, uy)[0]
    stat_y, dof_y = S.pearson(right_y, py)
    broken = np.where(right_y == order[j], order[j + 1], right_y)
    stat_b, _ = S.pearson(broken, py)
    print(f'[power] tilted by 1.03: chi2 {stat_t:.1f} > {lim:.1f}; boundary removed: {stat_b:.1f} > {S.chi2_limit(dof_y):.1f} (intact: {stat_y:.1f})')
    assert stat_t > lim
    assert stat_y <= S.chi2_limit(dof_y) and stat_b > S.chi2_limit(dof_y)
