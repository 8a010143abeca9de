"""The default ("counter") sampler - sample_token<*, false> of csrc/sample.hip through ops.cfg_sample and ops.cfg_sample_rows - against the
float64 / exact-integer oracle of oracle/sample_ref.py, draw by draw.  The oracle restates the sampler's contract: value
thresholds with ties kept, the zero-mass rule, the splitmix64 key, the inverse-CDF walk in ascending (e mod 256, e div 256).  A draw is
right iff it lies in the oracle's candidate set for its u (one token, or the neighbours of a CDF boundary within the derived delta of u);
`kept` is right iff it is the size of one of the oracle's kept sets.  No draw and no row is skipped.  tests/test_sample_oracle_host.py shows
on the CPU that the candidate sets are single tokens for more than 98 % of these very draws.

The distribution tests at the end do not use the oracle's hash: they would notice a weakness of the generator that the restated hash shares."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import sample_cases as C  # noqa: E402
from controlvar_amd import ops  # noqa: E402
from oracle import sample_ref as S  # noqa: E402

I64 = 2 ** 63


def as_i64(seed):
    seed &= S.M64
    return seed - 2 ** 64 if seed >= I64 else seed


def launch(dev, lg, Bn, l, V, nrep, n_draw, stage, ldv=0, *, coef=None, top_k=None, top_p=None, seed=0, seed_dev=0, tables=None):
    """one launch of either form -> (idx (Bn * l, n_draw), kept (Bn * l,), combined (Bn * l, V)) as numpy, rows in (b, t) order"""
    idx = torch.full((n_draw * Bn, l), -1, dtype=torch.int32, device=dev)
    comb = torch.full((Bn, l, V), float('nan'), device=dev)
    kept = torch.full((Bn, l), -1, dtype=torch.int32, device=dev)
    if tables is None:
        sd = torch.tensor([as_i64(seed_dev)], dtype=torch.int64, device=dev) if seed_dev else None
        ops.cfg_sample(lg, Bn, nrep, l, V, list(coef), int(top_k), float(top_p), seed, stage, n_draw, idx, comb, None, kept, seed_dev=sd, ldv=ldv)
    else:
        cf, ks, ps, seeds = tables
        ops.cfg_sample_rows(lg, Bn, nrep, l, V, torch.from_numpy(cf).to(dev), torch.from_numpy(ks).to(dev), torch.from_numpy(ps).to(dev),
                            torch.tensor([as_i64(s) for s in seeds], dtype=torch.int64, device=dev), stage, n_draw, idx, comb, None, kept, ldv=ldv)
    torch.cuda.synchronize()
    return (idx.cpu().numpy().reshape(n_draw, Bn * l).T.astype(np.int64), kept.cpu().numpy().reshape(-1).astype(np.int64),
            comb.cpu().numpy().reshape(Bn * l, V))


def check(x, top_k, top_p, u, kept, idx, what, srt=None):
    """kept is one of the oracle's candidate counts; every draw lies in the candidates computed against that kept set"""
    ma, mb, _, amb = S.kept_sets(x, top_k, top_p, srt)
    na, nb = ma.sum(axis=1), mb.sum(axis=1)
    bad = np.nonzero((kept != na) & (kept != nb))[0]
    assert bad.size == 0, f'{what}: kept differs from the oracle in {bad.size} rows, first row {bad[0]}: {kept[bad[0]]} against {na[bad[0]]} / {nb[bad[0]]}'
    mask = np.where((kept == na)[:, None], ma, mb)
    assert ((idx >= 0) & (idx < x.shape[1])).all(), f'{what}: an id outside [0, V)'
    cand = S.candidates(x, mask, u)
    ok = np.take_along_axis(cand, idx[:, :, None], axis=2)[:, :, 0]
    r, d = np.nonzero(~ok)
    assert r.size == 0, (f'{what}: {r.size} of {ok.size} draws outside the oracle\'s candidates; first at row {r[0]}, draw {d[0]}: '
                         f'got {idx[r[0], d[0]]}, candidates {np.nonzero(cand[r[0], d[0]])[0].tolist()}, u = {u[r[0], d[0]]!r}')
    return int((cand.sum(axis=2) > 1).sum()), int(amb.sum())


# ------------------------------------------------------------------------------------------------------------------ (a) scalar form
@pytest.mark.parametrize('V,nrep,sigma', C.FAMILIES)
def test_every_draw_of_the_scalar_form(gpu_device, V, nrep, sigma):
    prm = C.family_params(V, nrep, sigma)
    lg, x_host = C.build(V, nrep, sigma, prm['ldv'])
    dlg = torch.from_numpy(lg.reshape(nrep * C.B, C.L, -1)).to(gpu_device)
    u = C.draw_us(prm['seed'], prm['seed_dev'], prm['stage'], prm['n_draw'], 'scalar')
    srt, n_two, n_amb = None, 0, 0
    for k, p in C.filters(V):
        idx, kept, x = launch(gpu_device, dlg, C.B, C.L, V, nrep, prm['n_draw'], prm['stage'], prm['ldv'], coef=C.COEF[nrep], top_k=k, top_p=p,
                              seed=prm['seed'], seed_dev=prm['seed_dev'])
        assert np.array_equal(x, x_host), 'combined logits differ from the float32 restatement (the inputs were cleared of the floor band on it)'
        srt = srt or S.presort(x)
        a, b = check(x, k, p, u, kept, idx, f'V={V} nrep={nrep} sigma={sigma} top_k={k} top_p={p} {prm}', srt)
        n_two, n_amb = n_two + a, n_amb + b
    print(f'[sample oracle] V={V} nrep={nrep} sigma={sigma}: {7 * u.size} draws checked, {n_two} with two candidates; {7 * C.B * C.L} rows, {n_amb} with two kept sets')


# ------------------------------------------------------------------------------------------------------------------ (b) per-request form
@pytest.mark.parametrize('V,nrep,sigma', C.FAMILIES)
def test_every_draw_of_the_per_request_form(gpu_device, V, nrep, sigma):
    prm = C.family_params(V, nrep, sigma)
    tables = C.rows_tables(V, nrep, sigma)
    coef, ks, ps, seeds = tables
    lg, x_host = C.build(V, nrep, sigma, prm['ldv'], coef=np.repeat(coef[:, :nrep], C.L, axis=0), tag=1)
    dlg = torch.from_numpy(lg.reshape(nrep * C.B, C.L, -1)).to(gpu_device)
    idx, kept, x = launch(gpu_device, dlg, C.B, C.L, V, nrep, prm['n_draw'], prm['stage'], prm['ldv'], tables=tables)
    assert np.array_equal(x, x_host)
    u = C.draw_us(0, 0, prm['stage'], prm['n_draw'], 'rows', seeds)                          # keyed by d alone, seed[b]
    check(x, np.repeat(ks, C.L), np.repeat(ps, C.L), u, kept, idx, f'rows V={V} nrep={nrep} sigma={sigma} k={ks.tolist()} p={ps.tolist()}')


# ------------------------------------------------------------------------------------------------------------------ (c) hand-built rows
def hand_rows():
    """name -> (x (V,) float32, top_k, top_p, expected kept or None)"""
    g = np.random.default_rng(77)
    rows = {}
    for V in (300, 1000, 4096):
        rows[f'equal_V{V}'] = (np.full(V, 1.25, dtype=np.float32), 0, 0.0, V)
    rows['equal_topk'] = (np.full(1000, -3.0, dtype=np.float32), 50, 0.9, 1000)              # everything ties with both cuts
    one = np.full(1000, -100.0, dtype=np.float32)
    one[999] = 2.0                                                                           # the last, partly empty element slot
    rows['one_token'] = (one, 0, 0.0, 1)
    rows['one_token_p1'] = (one, 0, 1.0, 1)
    inf = (g.standard_normal(300) * 1.5).astype(np.float32)
    inf[g.permutation(300)[:250]] = -np.inf
    rows['inf_unfiltered'] = (inf, 0, 0.0, 50)
    rows['inf_in_topk'] = (inf, 100, 0.0, 50)                                               # the 100th largest value is -inf: every finite token stays
    rows['inf_nucleus'] = (inf, 0, 0.9, None)
    for i, (V, k, p) in enumerate(((300, 20, 0.0), (1000, 0, 0.9), (4096, 50, 0.96), (4096, 900, 0.0))):
        rows[f'grid{i}'] = ((np.round(g.standard_normal(V) * 2.5 * 4) / 4).astype(np.float32), k, p, None)
    z = np.full(300, -0.0, dtype=np.float32)
    z[[5, 100, 299]] = (3.0, 1.0, 0.5)
    z[7] = 0.0                                                                               # +0.0 is the 4th largest value, -0.0 everywhere else ...
    z[200:260] = -2.0                                                                        # ... but here
    rows['signed_zero'] = (z, 4, 0.0, 240)
    zr = -z
    zr[zr == 2.0] = -2.0
    zr[[5, 100, 299]] = (3.0, 1.0, 0.5)
    rows['signed_zero_rev'] = (zr.astype(np.float32), 4, 0.0, 240)                          # -0.0 at the 4th place, +0.0 elsewhere
    tail = (g.standard_normal(1000) * 1.0).astype(np.float32)
    tail[500:] -= np.float32(36.0)                                                           # more than 28 nats below the maximum: zero mass
    rows['tail'] = (tail, 0, 0.0, 500)
    rows['tail_p1'] = (tail, 1000, 1.0, 500)
    rows['tail_topk'] = (tail, 999, 0.0, 500)
    rows['tail_nucleus'] = (tail, 0, 0.999, None)
    return rows


HAND = hand_rows()
HAND_L, HAND_DRAWS = 16, 4


def exact_equal_row_tokens(V, seed, stage, key_rows, l):
    """all V masses equal: the masses are exact, and the draw is order[floor(u V)] - the documented element order and nothing else"""
    order = S.draw_order(V)
    out = np.empty((l, len(key_rows)), dtype=np.int64)
    for t in range(l):
        for i, r in enumerate(key_rows):
            m = int(S.counter_u(seed, stage, r, t) * 2 ** 53)
            out[t, i] = order[(m * V) >> 53]
    return out


@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_built_rows_scalar_form(gpu_device, name):
    x0, k, p, n_kept = HAND[name]
    V = x0.size
    assert not S.floor_band(x0).any()
    seed, stage = 2 ** 63 + 5, 19
    dlg = torch.from_numpy(np.tile(x0, (HAND_L, 1))[None]).to(gpu_device)                    # B = 1, the row at every t
    idx, kept, x = launch(gpu_device, dlg, 1, HAND_L, V, 1, HAND_DRAWS, stage, coef=[1.0], top_k=k, top_p=p, seed=seed)
    assert np.array_equal(x.view(np.uint32), np.tile(x0, (HAND_L, 1)).view(np.uint32))       # bits: the signed zeros arrive as built
    u = np.array([[S.counter_u(seed, stage, d, t) for d in range(HAND_DRAWS)] for t in range(HAND_L)])
    check(x, k, p, u, kept, idx, name)
    if n_kept is not None:
        assert (kept == n_kept).all(), (name, kept.tolist(), n_kept)
    if name.startswith('equal'):
        assert np.array_equal(idx, exact_equal_row_tokens(V, seed, stage, range(HAND_DRAWS), HAND_L)), name
    if name.startswith('one_token'):
        assert (idx == 999).all()


@pytest.mark.parametrize('V', [300, 1000, 4096])
def test_hand_built_rows_per_request_form(gpu_device, V):
    names = [n for n in sorted(HAND) if HAND[n][0].size == V]
    Bn = len(names)
    x0 = np.stack([HAND[n][0] for n in names])
    ks = np.array([HAND[n][1] for n in names], dtype=np.int32)
    ps = np.array([HAND[n][2] for n in names], dtype=np.float32)
    seeds = [(0x9E3779B97F4A7C15 * (i + 1)) & S.M64 for i in range(Bn)]
    coef = np.zeros((Bn, 4), dtype=np.float32)
    coef[:, 0] = 1.0
    stage = 0
    dlg = torch.from_numpy(np.repeat(x0[:, None, :], HAND_L, axis=1).copy()).to(gpu_device)
    idx, kept, x = launch(gpu_device, dlg, Bn, HAND_L, V, 1, HAND_DRAWS, stage, tables=(coef, ks, ps, seeds))
    u = np.array([[S.counter_u(seeds[b], stage, d, t) for d in range(HAND_DRAWS)] for b in range(Bn) for t in range(HAND_L)])
    check(x, np.repeat(ks, HAND_L), np.repeat(ps, HAND_L), u, kept, idx, f'hand-built rows, V={V}: {names}')
    for b, n in enumerate(names):
        rows = slice(b * HAND_L, (b + 1) * HAND_L)
        if HAND[n][3] is not None:
            assert (kept[rows] == HAND[n][3]).all(), (n, kept[rows].tolist())
        if n.startswith('equal'):
            assert np.array_equal(idx[rows], exact_equal_row_tokens(V, seeds[b], stage, range(HAND_DRAWS), HAND_L)), n


def test_a_draw_that_lands_on_a_boundary_of_unit_masses(gpu_device):
    """The strictness of "exceeds".  One heavy token, last in the walk, behind 4095 tokens 27.5 nats below it: exp(-27.5) 2^40 = 1.2534, so
    each light token holds exactly ONE unit of 2^-40 (0.25 away from either neighbouring integer: out of any rounding's reach) and
    Z_kept = 2^40 + 4095 units exactly.  For u < 2^-28 the target floor(u Z) is a small integer n, the cumulative masses are 1, 2, 3, ... and
    the first that EXCEEDS n belongs to the token at place n of the walk; a walk that stops at >= returns place n - 1.  The draws below
    have such u (found with sample_cases.find_small_u; their u is re-derived here with the oracle's hash)."""
    V = 4096
    order = S.draw_order(V)
    x0 = np.full(V, -27.5, dtype=np.float32)
    x0[order[-1]] = 0.0
    assert int(np.exp(-27.5) * 2 ** 40) == 1 and abs(np.exp(-27.5) * 2 ** 40 - 1.25) < 0.01
    Zk = 2 ** 40 + (V - 1)
    for seed, stage, d, t in C.SMALL_U:
        u = S.counter_u(seed, stage, d, t)
        n = int(u * 2 ** 53) * Zk >> 53                                                      # floor(u Z) in integers
        assert 1 <= n < V - 1, (seed, stage, d, t, u)
        l = t + 1
        dlg = torch.from_numpy(np.tile(x0, (l, 1))[None]).to(gpu_device)
        idx, kept, _ = launch(gpu_device, dlg, 1, l, V, 1, d + 1, stage, coef=[1.0], top_k=0, top_p=0.0, seed=seed)
        assert (kept == V).all()
        assert idx[t, d] == order[n], (seed, stage, d, t, int(idx[t, d]), int(order[n]), int(order[n - 1]))


# ------------------------------------------------------------------------------------------------------------------ (d) distribution
N_DRAWS = 32768


def dist_launch(dev, x0, Bn, l, n_draw, seed, stage):
    dlg = torch.from_numpy(np.tile(x0, (Bn, l, 1))).to(dev)
    idx = torch.full((n_draw * Bn, l), -1, dtype=torch.int32, device=dev)
    ops.cfg_sample(dlg, Bn, 1, l, x0.size, [1.0], 0, 0.0, seed, stage, n_draw, idx)
    torch.cuda.synchronize()
    return idx.cpu().numpy().astype(np.int64)                                                # (n_draw * Bn, l): chains along t


def dist_probs(x0):
    w = S.masses(x0.astype(np.float64))[0]
    return w / w.sum()


def assert_distribution(tokens, chains, probs, what):
    """tokens: every draw; chains: (n_chains, len) arrays whose neighbours along axis 1 must be independent"""
    assert tokens.size == N_DRAWS
    stat, dof = S.pearson(tokens, probs)
    lim = S.chi2_limit(dof)
    lo, hi = S.pair_share_bounds(probs, chains.shape[0], chains.shape[1])
    share = float((chains[:, 1:] == chains[:, :-1]).mean())
    print(f'[sample distribution] {what}: chi2 {stat:.1f} (limit {lim:.1f}, {dof} dof); equal neighbours {share:.5f} in [{lo:.5f}, {hi:.5f}]')
    assert stat <= lim, (what, stat, lim, dof)
    assert lo <= share <= hi, (what, share, lo, hi)


def test_distribution_of_one_launch(gpu_device):
    x0 = S.distribution_row()
    idx = dist_launch(gpu_device, x0, 8, 1024, 4, 20240607, 3)
    assert_distribution(idx, idx, dist_probs(x0), 'one launch, B = 8, l = 1024, n_draw = 4: neighbours along t')


def test_distribution_over_seeds(gpu_device):
    x0 = S.distribution_row()
    idx = np.stack([dist_launch(gpu_device, x0, 8, 16, 4, 1000 + s, 5) for s in range(64)])   # (64 seeds, 32, 16)
    probs = dist_probs(x0)
    assert_distribution(idx, idx.reshape(64, -1).T, probs, '64 consecutive seeds: neighbours along the seed')
    assert_distribution(idx, idx.reshape(-1, 16), probs, '64 consecutive seeds: neighbours along t')


def test_distribution_over_stages(gpu_device):
    x0 = S.distribution_row()
    idx = np.stack([dist_launch(gpu_device, x0, 8, 64, 4, 77, st) for st in range(16)])       # (16 stages, 32, 64)
    probs = dist_probs(x0)
    assert_distribution(idx, idx.reshape(16, -1).T, probs, 'stages 0..15: neighbours along the stage')
    assert_distribution(idx, np.moveaxis(idx.reshape(16, 4, 8, 64), 1, -1).reshape(-1, 4), probs, 'stages 0..15: neighbours along the draw row d')
