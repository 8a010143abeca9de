"""cvar_score_topn on the MI355X (include/cvar_topn.h) against the kernel that exists and against tests/topn_ref.py.  For every (b, t, i),
cvar_score_rows on target = top_id[b, t, i] must return rank i and the bits of top_logprob[b, t, i]; the ids equal the float64-free restatement of the rank
order (value descending, id ascending); tail_logprob lies inside the bound derived in topn_ref.py (nothing is measured on the kernel).  Sweep: V 4096 / 1000 /
300 / 37 / 2 x nrep 1 / 2 / 4 x N 1 / 5 / 32 / 64 (N > V included) x (B, l) = (1, 1) / (3, 5); the logits' padding columns (ldv > V) and the unused weights
hold NaN, the outputs are column slices of wider (B, L, N) / (B, L) tables between fences.  Hand-built rows: all equal, ties on a 0.25 grid, -inf entries,
signed zeros.  Row b of a batch equals its B = 1 call; every refusal leaves the outputs untouched."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import topn_ref as R  # noqa: E402
from conftest import record  # noqa: E402
from controlvar_amd import _lib, ops  # noqa: E402
from oracle import train_kernels_ref as T  # noqa: E402

FENCE = 64
NAN = float('nan')


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make_coef(B, nrep, seed):
    rng = np.random.default_rng(seed)
    coef = np.full((B, 4), np.nan, dtype=np.float32)               # entries >= nrep are not used
    g = rng.uniform(0.0, 4.0, size=B)
    coef[:, 0] = 1 + g
    if nrep > 1:
        coef[:, 1] = -g
    for r in range(2, nrep):
        coef[:, r] = rng.uniform(-2, 2, size=B)
    return coef


def make_logits(B, nrep, l, V, ldv, seed, std=4.0):
    lg = torch.randn(nrep * B, l, ldv, generator=torch.Generator().manual_seed(seed)) * std
    lg[:, :, V:] = NAN                                             # columns behind the codes: a read poisons the row
    return lg


class Out:
    """top_id / top_logprob / tail_logprob as the columns [off, off + l) of (B, L, N) / (B, L) tables, sentinel-filled, between fences"""

    def __init__(self, B, l, N, dev, L=None, off=0, want=('id', 'lp', 'tail')):
        L = L or l
        self.spec = {'id': ((B, L, N), torch.int32, -77), 'lp': ((B, L, N), torch.float32, NAN), 'tail': ((B, L), torch.float32, NAN)}
        self.bufs, self.tables, self.views = {}, {}, {}
        for name, (shape, dtype, fill) in self.spec.items():
            n = int(np.prod(shape))
            self.bufs[name] = torch.full((n + 2 * FENCE,), fill, dtype=dtype, device=dev)
            self.tables[name] = self.bufs[name][FENCE:FENCE + n].view(shape)
            self.views[name] = self.tables[name][:, off:off + l] if name in want else None
        self.cols = (off, off + l)

    @staticmethod
    def _is_fill(t):
        return bool(torch.isnan(t).all()) if t.dtype == torch.float32 else bool((t == -77).all())

    def untouched(self, name):
        return self._is_fill(self.bufs[name])

    def only_the_views_written(self):
        for name, tab in self.tables.items():
            b, n = self.bufs[name], tab.numel()
            if not (self._is_fill(b[:FENCE]) and self._is_fill(b[FENCE + n:]) and self._is_fill(tab[:, :self.cols[0]]) and self._is_fill(tab[:, self.cols[1]:])):
                return False
        return True


def run(dev, lg, coef, B, nrep, l, V, ldv, N, **kw):
    out = Out(B, l, N, dev, **kw)
    ops.score_topn(lg, B, nrep, l, V, coef, N, out.views['id'], out.views['lp'], out.views['tail'], ldv=ldv)
    torch.cuda.synchronize()
    return out


def check_against_score_rows(dev, lg, coef, ids, lps, B, nrep, l, V, ldv, N, what):
    """one cvar_score_rows launch over the N-fold repeated tokens: target = top_id[b, t, i] -> rank i and top_logprob's bits"""
    lgN = lg.repeat_interleave(N, dim=1).contiguous()
    target = ids.reshape(B, l * N).contiguous()
    lp = torch.full((B, l * N), NAN, device=dev)
    rk = torch.full((B, l * N), -77, dtype=torch.int32, device=dev)
    ops.score_rows(lgN, B, nrep, l * N, V, coef, target, None, lp, None, rk, None, ldv=ldv)
    torch.cuda.synchronize()
    want_rank = torch.arange(N, dtype=torch.int32, device=dev).repeat(B, l)
    real = target >= 0
    assert torch.equal(real, want_rank < V), what                   # exactly min(N, V) real entries per token, in front
    assert torch.equal(rk[real], want_rank[real]), what
    got = lps.reshape(B, l * N)
    assert same_bits(got[real], lp[real]), what
    assert bool(torch.isneginf(got[~real]).all()) and bool((target[~real] == -1).all()), what


def check_against_reference(out, lg, coef_h, B, nrep, l, V, N, what):
    """ids exact, tail inside its bound -> tail error / bound"""
    ref = R.score_reference(R.combine32(lg[:, :, :V].cpu(), np.nan_to_num(coef_h), B, nrep), N)
    assert np.array_equal(out.views['id'].cpu().numpy(), ref.ids), what
    tail = out.views['tail'].cpu().double().numpy()
    empty = ref.S_tail == 0
    assert bool(np.isneginf(tail[empty]).all()), what
    gone = np.isneginf(tail) & ~empty                               # a tail whose whole mass lies under fp32's smallest normal may vanish
    assert bool(ref.tail_may_vanish[gone].all()), what
    live = ~empty & ~gone
    return T.ratio_of(T.abs_err(tail[live], ref.tail[live]), ref.tail_bound[live]) if live.any() else 0.0


# ------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize('V,ldv', [(4096, 4104), (1000, 1024), (300, 320), (37, 40), (2, 8)])
@pytest.mark.parametrize('nrep', [1, 2, 4])
def test_sweep_against_score_rows_and_the_reference(gpu_device, nrep, V, ldv):
    dev, worst = gpu_device, 0.0
    for N in (1, 5, 32, 64):
        for B, l, L, off in ((1, 1, None, 0), (3, 5, 11, 4)):
            seed = 1000 * B + 10 * N + nrep
            lg = make_logits(B, nrep, l, V, ldv, seed).to(dev)
            coef_h = make_coef(B, nrep, seed)
            coef = torch.from_numpy(coef_h).to(dev)
            what = f'B={B} nrep={nrep} l={l} V={V} ldv={ldv} N={N}'
            out = run(dev, lg, coef, B, nrep, l, V, ldv, N, L=L, off=off)
            assert out.only_the_views_written(), what
            worst = max(worst, check_against_reference(out, lg, coef_h, B, nrep, l, V, N, what))
            check_against_score_rows(dev, lg, coef, out.views['id'], out.views['lp'], B, nrep, l, V, ldv, N, what)
    print(f'\n[score_topn] V={V} nrep={nrep}: worst tail_logprob error {worst:.3f} of its bound')
    record('score_topn', V=V, nrep=nrep, tail=worst)
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------------------- hand-built rows
def hand_rows(V):
    """(5, V) fp32 rows: all equal; ties on a 0.25 grid; -inf entries (more of them than anything else); signed zeros above -1; a 0.25 grid with -inf"""
    g = torch.Generator().manual_seed(V)
    rows = torch.zeros(5, V)
    rows[0] = 1.75
    rows[1] = torch.randint(-8, 9, (V,), generator=g).float() / 4
    rows[2] = float('-inf')
    keep = torch.randperm(V, generator=g)[:max(1, V // 6)]
    rows[2, keep] = torch.randn(keep.numel(), generator=g)
    rows[3] = -1.0
    zeros = torch.randperm(V, generator=g)[:max(2, V // 3)]
    rows[3, zeros] = torch.where(torch.rand(zeros.numel(), generator=g) < 0.5, 0.0, -0.0)
    rows[4] = torch.randint(-3, 4, (V,), generator=g).float() / 4
    rows[4, torch.randperm(V, generator=g)[:V // 2]] = float('-inf')
    return rows


@pytest.mark.parametrize('V', [300, 37])
def test_hand_built_rows_ties_minus_inf_and_signed_zeros(gpu_device, V):
    dev, B, nrep = gpu_device, 1, 1
    rows = hand_rows(V)
    assert bool((rows[3] == 0).sum() >= 2) and bool(torch.signbit(rows[3][rows[3] == 0]).any()) and not bool(torch.signbit(rows[3][rows[3] == 0]).all())
    l = rows.shape[0]
    lg = torch.full((B, l, V + 3), NAN)
    lg[0, :, :V] = rows
    coef_h = np.array([[1, np.nan, np.nan, np.nan]], dtype=np.float32)
    coef = torch.from_numpy(coef_h).to(dev)
    for N in (1, 5, 32, 64):
        what = f'hand rows V={V} N={N}'
        out = run(dev, lg.to(dev), coef, B, nrep, l, V, V + 3, N)
        frac = check_against_reference(out, lg, coef_h, B, nrep, l, V, N, what)
        assert frac <= 1.0, (what, frac)
        check_against_score_rows(dev, lg.to(dev), coef, out.views['id'], out.views['lp'], B, nrep, l, V, V + 3, N, what)
        ids, lp, tail = out.views['id'].cpu(), out.views['lp'].cpu(), out.views['tail'].cpu()
        n = min(N, V)
        assert torch.equal(ids[0, 0, :n], torch.arange(n, dtype=torch.int32)), what          # all equal: ids 0 .. N-1
        assert same_bits(lp[0, 0, :n], lp[0, 0, :1].expand(n)), what
        finite2 = int(torch.isfinite(rows[2]).sum())                                         # the -inf row: finite codes first, then -inf ones by id
        assert bool(torch.isfinite(lp[0, 2, :min(n, finite2)]).all()) and bool(torch.isneginf(lp[0, 2, finite2:]).all()), what
        if n > finite2:
            minus = torch.nonzero(torch.isneginf(rows[2])).flatten()[:n - finite2].int()
            assert torch.equal(ids[0, 2, finite2:n], minus) and bool(torch.isneginf(tail[0, 2])), what
        nz = int((rows[3] == 0).sum())                                                       # signed zeros tie: ascending ids whatever the sign
        assert torch.equal(ids[0, 3, :min(n, nz)], torch.nonzero(rows[3] == 0).flatten()[:min(n, nz)].int()), what


# ------------------------------------------------------------------------------------------------------------- independence, pointers, refusals
@pytest.mark.parametrize('nrep', [2, 4])
def test_row_b_of_a_batch_equals_the_b1_call_in_every_slot(gpu_device, nrep):
    dev, B, l, V, ldv, N = gpu_device, 3, 5, 1000, 1024, 32
    lg = make_logits(B, nrep, l, V, ldv, 31).to(dev)
    coef = torch.from_numpy(make_coef(B, nrep, 31)).to(dev)
    for perm in ([0, 1, 2], [2, 0, 1]):
        p = torch.tensor(perm, device=dev)
        lg_p = lg.view(nrep, B, l, ldv)[:, p].reshape(nrep * B, l, ldv).contiguous()
        batch = run(dev, lg_p, coef[p].contiguous(), B, nrep, l, V, ldv, N, L=9, off=2)
        for slot, b in enumerate(perm):
            one = run(dev, lg.view(nrep, B, l, ldv)[:, b].contiguous(), coef[b:b + 1].contiguous(), 1, nrep, l, V, ldv, N)
            for n in ('id', 'lp', 'tail'):
                assert same_bits(batch.views[n][slot:slot + 1], one.views[n]), (perm, b, n)


def test_each_output_pointer_alone(gpu_device):
    dev, B, nrep, l, V, ldv, N = gpu_device, 3, 2, 5, 300, 320, 8
    lg = make_logits(B, nrep, l, V, ldv, 41).to(dev)
    coef = torch.from_numpy(make_coef(B, nrep, 41)).to(dev)
    full = run(dev, lg, coef, B, nrep, l, V, ldv, N)
    for want in (('id',), ('lp',), ('id', 'tail'), ('lp', 'tail')):
        part = run(dev, lg, coef, B, nrep, l, V, ldv, N, want=want)
        for n in ('id', 'lp', 'tail'):
            if n in want:
                assert same_bits(part.views[n], full.views[n]), (want, n)
            else:
                assert part.untouched(n), (want, n)
    with pytest.raises(_lib.CvarError, match='cvar_score_topn'):
        run(dev, lg, coef, B, nrep, l, V, ldv, N, want=('tail',))
    with pytest.raises(ValueError, match='N must be an integer in 1..64'):
        ops.score_topn(lg, B, nrep, l, V, coef, 65, full.views['id'], full.views['lp'], ldv=ldv)
    with pytest.raises(ValueError, match='top_id must be a int32'):
        ops.score_topn(lg, B, nrep, l, V, coef, N, full.views['id'].long(), full.views['lp'], ldv=ldv)
    with pytest.raises(ValueError, match='share one row stride'):
        wide = torch.zeros(B, 9, N, device=dev)
        ops.score_topn(lg, B, nrep, l, V, coef, N, full.views['id'], wide[:, 2:2 + l], ldv=ldv)


def test_refused_arguments_return_their_status_before_any_write(gpu_device):
    dev, B, nrep, l, V, N = gpu_device, 2, 2, 3, 64, 8
    lib = _lib.load()
    lg = make_logits(B, nrep, l, V, V, 51).to(dev)
    coef = torch.from_numpy(np.nan_to_num(make_coef(B, nrep, 51))).to(dev)
    out = Out(B, l, N, dev)
    args = dict(logits=lg.data_ptr(), B=B, nrep=nrep, l=l, V=V, coef=coef.data_ptr(), N=N, ids=out.views['id'].data_ptr(), lp=out.views['lp'].data_ptr(),
                tail=out.views['tail'].data_ptr(), ldo=0, ldv=0, stream=None)

    def call(**kw):
        return lib.cvar_score_topn(*{**args, **kw}.values())
    for bad in (dict(logits=None), dict(coef=None), dict(ids=None, lp=None), dict(B=0), dict(l=0), dict(V=0), dict(ldv=V - 1), dict(ldo=l - 1)):
        assert call(**bad) == -1, bad                             # CVAR_EINVAL
    for bad in (dict(nrep=0), dict(nrep=5), dict(V=4097), dict(N=0), dict(N=65), dict(N=-1)):
        assert call(**bad) == -2, bad                             # CVAR_EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(out.untouched(n) for n in ('id', 'lp', 'tail'))     # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert out.only_the_views_written() and bool((out.views['id'] >= 0).all()) and bool(torch.isfinite(out.views['tail']).all())
