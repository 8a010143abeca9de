"""cvar_score_rows on the MI355X against the float64 reference of tests/score_ref.py: log-probability and entropy inside the bounds derived from
the kernel's order of evaluation, `combined` / argmax against the sampler's (bit for bit), rank exact; ties, -inf, negative targets, views, row
independence, every output pointer alone, fences, refused arguments, and the headline shape (2^31 logits)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from controlvar_amd import _lib, ops  # noqa: E402
from score_ref import combine_f32, score_ref, within_bounds  # noqa: E402

FENCE = 64
NAMES = ('combined', 'logprob', 'entropy', 'rank', 'argmax')


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_coef(B, nrep, seed, dev=None):
    rng = np.random.default_rng(seed)
    coef = np.zeros((B, 4), dtype=np.float32)
    g = rng.uniform(0.0, 4.0, size=B)
    coef[:, 0] = 1 + g
    if nrep > 1:
        coef[:, 1] = -g
    for r in range(2, nrep):
        coef[:, r] = rng.uniform(-2, 2, size=B)
    coef[:, nrep:] = np.nan                                        # entries >= nrep are not used
    return coef


def make_logits(B, nrep, l, V, ldv, seed, std=4.0):
    g = torch.Generator().manual_seed(seed)
    lg = torch.randn(nrep * B, l, ldv, generator=g) * std
    if ldv > V:
        lg[:, :, V:] = 1000.0                                      # columns behind the codes: larger than every logit, never read
    return lg


class Out:
    """the five outputs, NaN / sentinel-prefilled between fences"""

    def __init__(self, B, l, V, dev, want=NAMES):
        self.bufs, self.views = {}, {}
        for name in NAMES:
            n = B * l * (V if name == 'combined' else 1)
            if name in ('rank', 'argmax'):
                buf = torch.full((n + 2 * FENCE,), -77, dtype=torch.int32, device=dev)
            else:
                buf = torch.full((n + 2 * FENCE,), float('nan'), dtype=torch.float32, device=dev)
            self.bufs[name] = buf
            self.views[name] = buf[FENCE:FENCE + n].view((B, l, V) if name == 'combined' else (B, l)) if name in want else None
        self.n = {name: B * l * (V if name == 'combined' else 1) for name in NAMES}

    def args(self):
        return [self.views[n] for n in NAMES]

    def untouched(self, name):
        b = self.bufs[name]
        return bool(torch.isnan(b).all()) if b.dtype == torch.float32 else bool((b == -77).all())

    def fences_ok(self):
        for name, b in self.bufs.items():
            for part in (b[:FENCE], b[FENCE + self.n[name]:]):
                if not (bool(torch.isnan(part).all()) if b.dtype == torch.float32 else bool((part == -77).all())):
                    return False
        return True


def run(lg, B, nrep, l, V, ldv, coef, target, dev, want=NAMES):
    out = Out(B, l, V, dev, want)
    ops.score_rows(lg, B, nrep, l, V, coef, target, *out.args(), ldv=ldv)
    torch.cuda.synchronize()
    return out


def check_against_reference(out, lg, coef, target, B, nrep, l, V, ldv, what):
    """bounds for logprob / entropy, everything else exact; returns the reference rank"""
    x = combine_f32(lg.cpu().numpy().reshape(nrep, B, l, ldv), coef, V)
    ref_lp, ref_ent, ref_rank, ref_am = score_ref(x, target.cpu().numpy())
    v = out.views
    assert v['combined'].cpu().numpy().tobytes() == x.tobytes(), what
    assert np.array_equal(v['rank'].cpu().numpy(), ref_rank), what
    assert np.array_equal(v['argmax'].cpu().numpy(), ref_am), what
    a, b = within_bounds(v['logprob'].cpu().numpy(), v['entropy'].cpu().numpy(), ref_lp, ref_ent)
    print(f'[score] {what}: worst logprob error {a:.3f} of its bound, worst entropy error {b:.3f} of its bound')
    assert a <= 1.0 and b <= 1.0, (what, a, b)
    assert out.fences_ok(), what
    return ref_rank


# ------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize('V,ldv', [(4096, 4096), (1000, 1024), (257, 320), (1, 8)])
@pytest.mark.parametrize('nrep', [1, 2, 4])
def test_sweep_against_the_reference_and_the_sampler(gpu_device, nrep, V, ldv):
    dev = gpu_device
    for B in (1, 3):
        for l in (1, 2, 37):
            seed = 1000 * B + 10 * l + nrep
            lg = make_logits(B, nrep, l, V, ldv, seed).to(dev)
            coef_h = make_coef(B, nrep, seed)
            coef = torch.from_numpy(coef_h).to(dev)
            g = torch.Generator().manual_seed(seed + 1)
            target = torch.randint(0, V, (B, l), generator=g, dtype=torch.int32)
            target[0, 0] = V - 1
            out = run(lg, B, nrep, l, V, ldv, coef, target.to(dev), dev)
            what = f'B={B} nrep={nrep} l={l} V={V} ldv={ldv}'
            # half of the targets become the greedy id, so that rank == 0 is met on purpose and not by luck
            am = out.views['argmax'].cpu()
            target = torch.where(torch.rand(B, l, generator=g) < 0.5, am, target)
            out = run(lg, B, nrep, l, V, ldv, coef, target.to(dev), dev)
            rank = check_against_reference(out, lg, coef_h, target, B, nrep, l, V, ldv, what)
            assert np.array_equal(rank == 0, (target == am).numpy()), what
            if V > 1:                                               # the sampler takes V >= 2; at V = 1 the reference above pins combined and argmax
                idx = torch.full((B, l), -1, dtype=torch.int32, device=dev)
                comb = torch.full((B, l, V), float('nan'), device=dev)
                ops.cfg_sample_rows(lg, B, nrep, l, V, torch.nan_to_num(coef), torch.ones(B, dtype=torch.int32, device=dev), torch.zeros(B, device=dev),
                                    torch.zeros(B, dtype=torch.int64, device=dev), 0, 1, idx, comb, ldv=ldv)
                assert same_bits(out.views['combined'], comb), what
                assert torch.equal(out.views['argmax'], idx), what
                assert torch.equal(out.views['rank'] == 0, target.to(dev) == idx), what
            else:
                assert bool((out.views['argmax'] == 0).all()) and bool((out.views['rank'] == 0).all())
                assert bool((out.views['logprob'] == 0).all()) and bool((out.views['entropy'] == 0).all())


# ------------------------------------------------------------------------------------------------------------- ties and special values
def test_exact_ties_at_the_maximum_and_at_the_target(gpu_device):
    """integer-valued logits and weights: the combine is exact and ties are certain"""
    dev, B, nrep, l, V = gpu_device, 2, 2, 5, 1000
    g = torch.Generator().manual_seed(7)
    lg = torch.randint(-6, 7, (nrep * B, 1, V), generator=g).float().repeat(1, l, 1)          # the l tokens of a row share their logits: one row, five targets
    lg[:B, :, [17, 600]], lg[B:, :, [17, 600]] = 6.0, -6.0         # two columns at the largest possible value: a tie at the maximum in every row
    coef_h = np.array([[2, -1, 0, 0], [3, -2, 0, 0]], dtype=np.float32)
    x = combine_f32(lg.numpy().reshape(nrep, B, l, V), coef_h, V)
    target = torch.zeros(B, l, dtype=torch.int32)
    for b in range(B):
        for t in range(l):
            row = x[b, t]
            tied_max = np.flatnonzero(row == row.max())
            assert tied_max.size >= 2 and 17 in tied_max and 600 in tied_max
            vals, counts = np.unique(row, return_counts=True)
            mid = np.flatnonzero(row == vals[np.argmax(counts)])
            target[b, t] = int((tied_max[-1], tied_max[0], mid[0], mid[-1], mid[len(mid) // 2])[t])
    out = run(lg.to(dev), B, nrep, l, V, V, torch.from_numpy(coef_h).to(dev), target.to(dev), dev)
    rank = check_against_reference(out, lg, coef_h, target, B, nrep, l, V, V, 'ties')
    assert (rank[:, 1] == 0).all() and (rank[:, 0] > 0).all()      # the first of the tied maxima is the greedy id, the last one is not
    assert (rank[:, 3] > rank[:, 4]).all() and (rank[:, 4] > rank[:, 2]).all()


def test_minus_inf_entries_and_negative_targets(gpu_device):
    dev, B, nrep, l, V, ldv = gpu_device, 3, 2, 4, 257, 320
    lg = make_logits(B, nrep, l, V, ldv, 11)
    lg[:B, :, 5] = float('-inf')                                    # weight > 0 on branch 0: the combined logit is -inf
    lg[:B, 1, 100:200] = float('-inf')
    coef_h = make_coef(B, nrep, 11)
    coef_h[:, 1] = -np.abs(coef_h[:, 1])
    lg[B:, :, 5] = 1.0                                              # keep (-inf) + finite, never (-inf) - (-inf)
    lg[B:, 1, 100:200] = 1.0
    target = torch.tensor([[5, 150, 7, -1], [-1, 5, 256, 0], [3, -5, 5, 5]], dtype=torch.int32)
    out = run(lg.to(dev), B, nrep, l, V, ldv, torch.from_numpy(coef_h).to(dev), target.to(dev), dev)
    check_against_reference(out, lg, coef_h, target, B, nrep, l, V, ldv, '-inf and negative targets')
    lp, rk = out.views['logprob'].cpu(), out.views['rank'].cpu()
    neg = target < 0
    assert bool((lp[neg] == 0).all()) and bool((rk[neg] == -1).all())
    at_inf = (target == 5) | ((target == 150) & (torch.arange(l)[None] == 1))
    assert bool(torch.isneginf(lp[at_inf]).all()) and int(at_inf.sum()) == 5
    assert bool(torch.isfinite(out.views['entropy']).all())
    assert bool(torch.isfinite(lp[~at_inf]).all())


# ------------------------------------------------------------------------------------------------------------- views and independence
def test_target_and_outputs_may_be_column_slices_of_wider_tables(gpu_device):
    dev, B, nrep, l, V, L = gpu_device, 3, 2, 37, 1000, 101
    lg = make_logits(B, nrep, l, V, 1024, 21).to(dev)
    coef = torch.from_numpy(make_coef(B, nrep, 21)).to(dev)
    g = torch.Generator().manual_seed(22)
    table = torch.randint(0, V, (B, L), generator=g, dtype=torch.int32).to(dev)
    target = table[:, 40:40 + l]
    assert target.stride(0) == L and not target.is_contiguous()
    ref = run(lg, B, nrep, l, V, 1024, coef, target.contiguous(), dev)
    wide = {n: torch.full((B, L), -77 if n in ('rank', 'argmax') else float('nan'), dtype=torch.int32 if n in ('rank', 'argmax') else torch.float32, device=dev)
            for n in NAMES[1:]}
    ops.score_rows(lg, B, nrep, l, V, coef, target, None, *[wide[n][:, 40:40 + l] for n in NAMES[1:]], ldv=1024)
    for n in NAMES[1:]:
        assert same_bits(wide[n][:, 40:40 + l], ref.views[n]), n
        rest = torch.cat((wide[n][:, :40], wide[n][:, 40 + l:]), dim=1)
        assert bool((rest == -77).all()) if n in ('rank', 'argmax') else bool(torch.isnan(rest).all()), n
    with pytest.raises(ValueError, match='share one row stride'):
        ops.score_rows(lg, B, nrep, l, V, coef, target, None, wide['logprob'][:, 40:40 + l], ref.views['entropy'], ldv=1024)
    with pytest.raises(ValueError, match='target must be an int32'):
        ops.score_rows(lg, B, nrep, l, V, coef, table.long()[:, :l], None, ref.views['logprob'], ldv=1024)


@pytest.mark.parametrize('nrep', [2, 4])
def test_row_b_of_a_batch_equals_the_b1_call_in_every_slot(gpu_device, nrep):
    dev, B, l, V, ldv = gpu_device, 3, 37, 1000, 1024
    lg = make_logits(B, nrep, l, V, ldv, 31).to(dev)
    coef = torch.from_numpy(make_coef(B, nrep, 31)).to(dev)
    g = torch.Generator().manual_seed(32)
    target = torch.randint(-1, V, (B, l), generator=g, dtype=torch.int32).to(dev)
    for perm in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        p = torch.tensor(perm, device=dev)
        lg_p = lg.view(nrep, B, l, ldv)[:, p].reshape(nrep * B, l, ldv).contiguous()
        batch = run(lg_p, B, nrep, l, V, ldv, coef[p].contiguous(), target[p].contiguous(), dev)
        for slot, b in enumerate(perm):
            lg_1 = lg.view(nrep, B, l, ldv)[:, b].contiguous()
            one = run(lg_1, 1, nrep, l, V, ldv, coef[b:b + 1].contiguous(), target[b:b + 1].contiguous(), dev)
            for n in NAMES:
                assert same_bits(batch.views[n][slot:slot + 1], one.views[n]), (perm, b, n)


# ------------------------------------------------------------------------------------------------------------- pointers, fences, refusals
def test_each_output_pointer_alone_and_all_together(gpu_device):
    dev, B, nrep, l, V, ldv = gpu_device, 3, 2, 5, 257, 320
    lg = make_logits(B, nrep, l, V, ldv, 41).to(dev)
    coef = torch.from_numpy(make_coef(B, nrep, 41)).to(dev)
    target = torch.randint(0, V, (B, l), generator=torch.Generator().manual_seed(42), dtype=torch.int32).to(dev)
    full = run(lg, B, nrep, l, V, ldv, coef, target, dev)
    assert full.fences_ok() and not any(full.untouched(n) for n in NAMES)
    for name in NAMES:
        alone = run(lg, B, nrep, l, V, ldv, coef, target, dev, want=(name,))
        assert same_bits(alone.views[name], full.views[name]), name
        assert alone.fences_ok() and all(alone.untouched(n) for n in NAMES if n != name), name
    with pytest.raises(_lib.CvarError, match='cvar_score_rows'):
        run(lg, B, nrep, l, V, ldv, coef, target, dev, want=())


def test_refused_arguments_return_their_status(gpu_device):
    dev, B, nrep, l, V = gpu_device, 2, 2, 3, 64
    lib = _lib.load()
    lg = make_logits(B, nrep, l, V, V, 51).to(dev)
    coef = torch.from_numpy(np.nan_to_num(make_coef(B, nrep, 51))).to(dev)
    target = torch.zeros(B, l, dtype=torch.int32, device=dev)
    lp = torch.full((B, l), float('nan'), device=dev)
    args = dict(logits=lg.data_ptr(), B=B, nrep=nrep, l=l, V=V, coef=coef.data_ptr(), target=target.data_ptr(), ldt=l, comb=None, lp=lp.data_ptr(), en=None,
                rk=None, am=None, ldo=0, ldv=0, stream=None)

    def call(**kw):
        return lib.cvar_score_rows(*{**args, **kw}.values())
    for bad in (dict(logits=None), dict(coef=None), dict(target=None), dict(ldt=l - 1), dict(lp=None), dict(B=0), dict(l=0), dict(V=0), dict(ldv=V - 1),
                dict(ldo=l - 1)):
        assert call(**bad) == -1, bad                             # CVAR_EINVAL
    for bad in (dict(nrep=0), dict(nrep=5), dict(V=4097)):
        assert call(**bad) == -2, bad                             # CVAR_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool(torch.isnan(lp).all())                             # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(lp).all())


# ------------------------------------------------------------------------------------------------------------- the headline shape
def test_headline_shape_rows_equal_the_same_op_in_eight_batch_chunks(gpu_device):
    """B = 512, nrep = 2, l = 512, V = 4096: 2^31 logits (8.6 GB), the second branch's offsets reach past 2^31 elements.  Device-generated,
    non-periodic data; every row of all five outputs against the op on 8 chunks of 64 rows."""
    dev, B, nrep, l, V = gpu_device, 512, 2, 512, 4096
    g = torch.Generator(device=dev).manual_seed(61)
    lg = torch.empty(nrep * B, l, V, device=dev)
    assert lg.numel() == 2 ** 31
    lg.normal_(0.0, 4.0, generator=g)
    coef = torch.from_numpy(make_coef(B, nrep, 61)).to(dev)
    target = torch.randint(-1, V, (B, l), generator=g, device=dev, dtype=torch.int32)
    full = {n: torch.full((B, l, V) if n == 'combined' else (B, l), -77 if n in ('rank', 'argmax') else float('nan'),
                          dtype=torch.int32 if n in ('rank', 'argmax') else torch.float32, device=dev) for n in NAMES}
    ops.score_rows(lg, B, nrep, l, V, coef, target, *[full[n] for n in NAMES])
    Bc = B // 8
    for c in range(8):
        rows = slice(c * Bc, (c + 1) * Bc)
        lg_c = torch.cat([lg[r * B + c * Bc:r * B + (c + 1) * Bc] for r in range(nrep)]).contiguous()
        part = {n: torch.empty_like(full[n][rows]) for n in NAMES}
        ops.score_rows(lg_c, Bc, nrep, l, V, coef[rows].contiguous(), target[rows].contiguous(), *[part[n] for n in NAMES])
        for n in NAMES:
            assert same_bits(full[n][rows], part[n]), (c, n)
    assert bool(torch.isfinite(full['entropy']).all()) and bool((full['rank'][target < 0] == -1).all())
    assert bool((full['rank'][target >= 0] >= 0).all()) and bool((full['logprob'][target >= 0] <= 0).all())
