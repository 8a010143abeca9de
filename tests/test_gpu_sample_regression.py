"""The sampler kernels of csrc/sample.hip against a recording of the library BEFORE the scalar and the per-request kernels were given one
shared body (tests/golden/sample_regression.npz, written by tests/golden/make_sample_regression.py on that library).  The merge may not
reorder one floating-point operation, so every output - ids, kept-set sizes, margins, combined logits, soft embeddings - is compared bit
for bit: no tolerance anywhere.

Every launch is B = 3 rows of l tokens (at most 15 workgroups).  Two logits sets per shape: seeded randn * 2.5, and one quantised to multiples
of 0.25 under dyadic weights, whose combined logits are multiples of 1/8 (two branches) or 1/32 (four) - exact ties at the top-k value and at the nucleus cut - with each
row's maximum copied to two more columns (an exact tie at the maximum)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from controlvar_amd import ops  # noqa: E402

B, CV, STAGE = 3, 32, 3
# (l, V, ldv, nrep, n_draw): V = 1000 is no multiple of the 256 threads (the e < V guards) in rows of ldv = 1024 floats (a head wider than the codebook)
# l = 5 goes with V = 1000: there the token stride of the logits (ldv), that of the combined logits (V) and the tile all differ, which l = 5 at
# V = ldv = 4096 would not add to, and its 61 440 combined logits per weight set would not fit the fixture
SHAPES = ((1, 4096, 0, 2, 1), (1, 4096, 0, 4, 4), (5, 1000, 1024, 2, 1), (5, 1000, 1024, 4, 4))
# combine weights: fp32-inexact ones for the randn set, dyadic ones for the quantised set (sums of products stay exact: ties survive the combine)
COEF = {'randn': {2: [1.3, -0.3], 4: [1.3, -0.15, -0.075, -0.075]}, 'ties': {2: [1.5, -0.5], 4: [1.5, -0.25, -0.125, -0.125]}}
TOP_P_EXTREMES = (1e-9, 1.5)                                    # below 2^-24 (1 - top_p rounds to 1 in float) and above 1: both ends of the clamp of lim
NOISE_CASES = ((0, 0.0), (50, 0.5), (900, 0.96))                # the race and more_smooth: unfiltered, both filters narrow, both filters wide
SEEDS = (11, 2 ** 64 - 3, 123456789012345)                      # per-request rows: one seed has its top bit set
ROW_SCALE = (1.0, 0.5, 2.0)                                     # per-request rows: row b combines with the scalar weights times ROW_SCALE[b]


def counter_cases(V):
    return [(k, p) for k in (0, 1, 50, 900, V) for p in (0.0, 0.5, 0.96)] + [(0, p) for p in TOP_P_EXTREMES] + [(50, p) for p in TOP_P_EXTREMES]


def make_logits(kind, l, V, ldv, nrep, gen):
    ld = ldv or V
    lg = torch.randn(nrep * B, l, ld, generator=gen) * 2.5
    if kind == 'ties':
        lg = (lg * 4).round() / 4
        comb = sum(c * lg.view(nrep, B, l, ld)[r] for r, c in enumerate(COEF[kind][nrep]))[..., :V]      # exact: dyadic weights
        top = comb.argmax(-1)
        for b in range(B):
            for t in range(l):
                e = int(top[b, t])
                for off in (7, 501):
                    lg.view(nrep, B, l, ld)[:, b, t, (e + off) % V] = lg.view(nrep, B, l, ld)[:, b, t, e]
    if ld > V:
        lg[:, :, V:] = 100.0                                    # behind the codes: larger than every logit, must never be read
    return lg


def row_coefs(kind, nrep):
    """one weight set per row: the scalar set times a power of two, so that row b's combined logits are EXACTLY the scalar launch's times
    ROW_SCALE[b] (scaling by a power of two commutes with every rounding) and need no copy of their own in the fixture"""
    c = torch.zeros(B, 4)
    for b, s in enumerate(ROW_SCALE):
        c[b, :nrep] = torch.tensor(COEF[kind][nrep]) * s
    return c


def sample_outputs(dev):
    out = {}
    gen = torch.Generator().manual_seed(20)
    for l, V, ldv, nrep, n_draw in SHAPES:
        for kind in ('randn', 'ties'):
            tag = f'{kind}_l{l}_V{V}_r{nrep}_d{n_draw}'
            host = make_logits(kind, l, V, ldv, nrep, gen)
            out[f'{tag}.logits64'] = host.reshape(-1)[:64].numpy().copy()
            lg = host.to(dev)
            coef = COEF[kind][nrep]
            E = torch.randn(V, CV, generator=gen).to(dev)
            expo = torch.empty(n_draw * B, l, V).exponential_(generator=gen)
            expo[0, 0, 3] = 0.0                                 # q = 0: inf where column 3 is kept, 0 / 0 = NaN where it is masked - it wins both ways
            expo = expo.to(dev)
            gumbel = (-torch.empty(n_draw * B, l, V).exponential_(generator=gen).log()).to(dev)
            seed_dev = torch.tensor([2 ** 40 + 17], dtype=torch.int64, device=dev)
            first = {}
            rec = {'cases': [], 'ids': [], 'kept': [], 'margin': [], 'soft_cases': [], 'soft_out': []}       # one stacked array each: launches in order

            def launch(name, top_k, top_p, soft=False, **kw):
                idx = torch.full((n_draw * B, l), -1, dtype=torch.int32, device=dev)
                comb = torch.full((B, l, V), float('nan'), device=dev)
                mg = torch.full((B, l), float('nan'), device=dev)
                kept = torch.full((B, l), -1, dtype=torch.int32, device=dev)
                if soft:
                    kw.update(codebook=E, smooth_mul=0.7, smooth_tau=0.27, soft_out=torch.full((n_draw * B, l, CV), float('nan'), device=dev))
                ops.cfg_sample(lg, B, nrep, l, V, coef, top_k, top_p, 1234, STAGE, n_draw, idx, comb, mg, kept, ldv=ldv, **kw)
                if 'combined' not in first:                     # stored once per (logits, weights): every later launch must reproduce it
                    first['combined'] = comb
                    out[f'{tag}.combined'] = comb.cpu().numpy()
                assert torch.equal(comb, first['combined']), (tag, name)
                record(f'{name}_k{top_k}_p{top_p}', idx, kept, mg, kw.get('soft_out'))

            def record(case, idx, kept, mg, soft_out=None):
                rec['cases'].append(case)
                rec['ids'].append(idx.cpu().numpy()), rec['kept'].append(kept.cpu().numpy()), rec['margin'].append(mg.cpu().numpy())
                if soft_out is not None:
                    rec['soft_cases'].append(case), rec['soft_out'].append(soft_out.cpu().numpy())

            for k, p in counter_cases(V):                       # cfg_greedy_kernel (top_k == 1) and cfg_sample_kernel<false, false>
                launch('counter', k, p)
            launch('seed_dev', 50, 0.5, seed_dev=seed_dev)
            launch('seed_dev', 1, 0.0, seed_dev=seed_dev)
            for k, p in NOISE_CASES + ((1, 0.0),):              # <false, true>; the race at top_k == 1 draws among the tied maxima
                launch('race', k, p, expo=expo)
            for k, p in NOISE_CASES:
                launch('soft_gumbel', k, p, soft=True, gumbel=gumbel)                      # <true, false>, injected Gumbel noise
            launch('soft_counter', 900, 0.96, soft=True, seed_dev=seed_dev)                # <true, false>, the counter generator's own noise
            launch('soft_race_gumbel', 50, 0.5, soft=True, gumbel=gumbel, expo=expo)       # <true, true>
            launch('soft_race_counter', 900, 0.96, soft=True, expo=expo)

            # cfg_sample_rows_kernel on mixed tables: a greedy, a filtered and an unfiltered row, each with its own seed and weights
            rc = row_coefs(kind, nrep).to(dev)
            seeds = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in SEEDS], dtype=torch.int64, device=dev)
            for ti, (ks, ps) in enumerate((((1, 50, 0), (0.96, 0.5, 0.0)), ((900, V, 1), (0.96, 1e-9, 1.5)))):
                idx = torch.full((n_draw * B, l), -1, dtype=torch.int32, device=dev)
                comb = torch.full((B, l, V), float('nan'), device=dev)
                mg = torch.full((B, l), float('nan'), device=dev)
                kept = torch.full((B, l), -1, dtype=torch.int32, device=dev)
                ops.cfg_sample_rows(lg, B, nrep, l, V, rc, torch.tensor(ks, dtype=torch.int32, device=dev), torch.tensor(ps, device=dev), seeds, STAGE,
                                    n_draw, idx, comb, mg, kept, ldv=ldv)
                assert torch.equal(comb, first['combined'] * torch.tensor(ROW_SCALE, device=dev).view(B, 1, 1)), (tag, 'rows', ti)
                record(f'rows{ti}', idx, kept, mg)
            for name, arrays in rec.items():
                out[f'{tag}.{name}'] = np.stack(arrays)
    return out


def first_difference(k, a, b, g):
    """the launch at which stacked array k differs, by its recorded name"""
    tag, name = k.rsplit('.', 1)
    if a.shape != b.shape or name not in ('ids', 'kept', 'margin', 'soft_out'):
        return k
    cases = g[tag + ('.soft_cases' if name == 'soft_out' else '.cases')]
    return k, [str(c) for c, x, y in zip(cases, a, b) if not np.array_equal(x, y)][:4]


def test_sampler_kernels_bit_identical_to_the_previous_library(gpu_device):
    path = os.path.join(GOLDEN, 'sample_regression.npz')
    assert os.path.exists(path), 'record it with tests/golden/make_sample_regression.py on the previous library'
    g = dict(np.load(path))
    got = sample_outputs(gpu_device)
    assert set(got) == set(g)
    for k in sorted(got):                                       # the inputs first: a drifting generator reports itself, not a sampler bug
        if k.endswith('.logits64'):
            assert np.array_equal(got[k], g[k]), f'{k}: the seeded inputs differ from the recorded ones'
    for k in sorted(got):
        assert got[k].dtype == g[k].dtype and np.array_equal(got[k], g[k]), first_difference(k, got[k], g[k], g)
    # the quantised set does hold the ties it is there for: more than top_k survivors, and a zero margin at every maximum
    for l, V, _, nrep, n_draw in SHAPES:
        tag = f'ties_l{l}_V{V}_r{nrep}_d{n_draw}'
        cases = list(g[f'{tag}.cases'])
        assert (g[f'{tag}.kept'][cases.index('counter_k900_p0.0')] > 900).any() and not g[f'{tag}.margin'][cases.index('counter_k1_p0.0')].any(), tag
