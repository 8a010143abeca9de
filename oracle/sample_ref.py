"""Float64 / exact-integer oracle of the default ("counter") sampler of csrc/sample.hip: sample_token<*, false>.

Written from the sampler's CONTRACT (DESIGN.md "The counter sampler's contract"), not from the kernel's arithmetic: numpy float64 for the
masses, Python integers for the hash, a sort where the kernel runs a radix select.  The product never imports this file.

The oracle takes the combined logits as its input (their bits are tested elsewhere) and answers three questions per row:

  kept_sets   which tokens survive top-k and the nucleus cut (value thresholds, ties kept, the maximum always kept),
  counter_u   which uniform number u in [0, 1) the generator hands to draw (seed, stage, key_row, t),
  candidates  which tokens a correct kernel may return for that u.

What the kernel may differ by, and no more.  The kernel forms its masses in fp32 and quantises them to multiples of 2^-40 of the maximum's
mass; the oracle forms them in float64.  A CDF boundary of the kernel therefore lies within `delta` of the oracle's, and a draw whose u is
closer than that to a boundary has two right answers.  delta is derived below from the documented precision of the instructions, never from
what the kernel returns:

  element e with d = max - x_e carries a relative mass error  eps_e <= (2 d + 4) 2^-24 :
      d 2^-24   the fp32 subtraction x_e - max (half an ulp of a number of size d, moved into the exponent),
      d 2^-24   the fp32 product (x_e - max) * log2(e) inside __expf,
      4 2^-24   the hardware exp2 (V_EXP_F32: 1 ulp in the CDNA ISA guide = 2^-23 relative) and the conversion to an integer mass
                (the fp32 product by 2^40 is exact; one more 2^-23 is allowed for it),
  and an absolute error of one unit of 2^-40 from the floor of that conversion.  A boundary F_j = (partial sum) / Z of the kept set then moves
  by at most
      2 * sum_e(w_e eps_e) / Z_kept  +  (V + 1) 2^-40 / Z_kept          (masses relative to the maximum's: w_max = 1)
  - once for the partial sum and once for Z, the + 1 for the floor of u * Z.  `delta` is FOUR times this value.  The factor covers the
  per-instruction figures, which are documentation and not measurements (and the rounding of the fp32 constant log2(e), 0.22 d 2^-24, which the
  sum above leaves out).  For the masses of a typical row this is a few 1e-6.

The nucleus cut compares an ascending partial sum with (1 - top_p) Z.  Its error is bounded the same way, but per boundary: only the elements
below the boundary and the share (1 - top_p) of Z's error enter (`_cut_delta`), again times four.  The row's delta would be a valid bound there
too, but a needlessly wide one: deep in the tail the cumulative masses of neighbouring tokens lie closer together than it.  A row whose cut lies
within its bound of a cumulative mass has two right kept sets; both are returned.  For top_p >= 1 the cut is "exceeds 0", which the zero-mass
rule below decides exactly.

Zero-mass tokens.  A mass below 2^-40 of the maximum's quantises to zero.  Such a token is in the value-rule set but is never drawn, adds
nothing to any sum and is not counted in `kept`; the oracle models exactly that (FLOOR).  Whether a mass within a relative 1e-4 of the floor
(far more than eps_e) becomes zero depends on the kernel's rounding: `floor_band` finds such elements, and test inputs are built without them.
"""
from __future__ import annotations

import math
from statistics import NormalDist

import numpy as np

M64 = (1 << 64) - 1
FLOOR = 2.0 ** -40                       # smallest mass (relative to the maximum's) that the sampler keeps
FLOOR_BAND = 1e-4                        # relative half-width of the band around FLOOR inside which either outcome is right
SAFETY = 4.0                             # delta = SAFETY * the derived bound (see the module text)
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------ the generator
def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def counter_u(seed: int, stage: int, key_row: int, t: int) -> float:
    """u of draw (seed, stage, key_row, t): exact (53 bits times 2^-53 is a float64).  key_row = d * B + b in the scalar form (seed = the
    call's seed plus the device-resident one, mod 2^64), key_row = d with seed = seed[b] in the per-request form."""
    h0 = splitmix64((int(seed) & M64) ^ 0xC0FFEE1234)
    h = splitmix64(h0 ^ ((int(stage) << 48) & M64) ^ ((int(key_row) << 16) & M64) ^ int(t))
    return (h >> 11) * 2.0 ** -53


def counter_u_grid(seed: int, stage: int, key_rows, ts) -> np.ndarray:
    """counter_u over the grid key_rows x ts -> float64 (len(key_rows), len(ts))"""
    return np.array([[counter_u(seed, stage, r, t) for t in ts] for r in key_rows], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------ masses and delta
def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    return x[None] if x.ndim == 1 else x


def masses(x, mask=None):
    """w_e = exp(x_e - max) in float64 over `mask` (default: everything), zero below FLOOR.  The maximum is taken over the whole row: it is
    always kept."""
    x = _rows(x)
    with np.errstate(invalid='ignore'):
        w = np.exp(x - x.max(axis=1, keepdims=True))
    w = np.where(np.isnan(w), 0.0, w)
    if mask is not None:
        w = np.where(mask, w, 0.0)
    return np.where(w < FLOOR, 0.0, w)


def floor_band(x):
    """True where a mass lies so close to FLOOR that the kernel's rounding decides whether it survives (test inputs must have none)"""
    x = _rows(x)
    with np.errstate(invalid='ignore'):
        w = np.exp(x - x.max(axis=1, keepdims=True))
    return np.abs(w / FLOOR - 1.0) <= FLOOR_BAND


def _eps(x):
    """relative mass error bound per element, (2 d + 4) 2^-24 (0 where the mass is 0 anyway)"""
    x = _rows(x)
    d = x.max(axis=1, keepdims=True) - x
    return np.where(np.isfinite(d), (2.0 * d + 4.0) * U24, 0.0)


def delta_of(x, mask):
    """the row's delta for the CDF over `mask`: SAFETY * (2 sum(w eps) / Z + (V + 1) 2^-40 / Z), w relative to the maximum"""
    x = _rows(x)
    w = masses(x, mask)
    Z = w.sum(axis=1)
    return SAFETY * (2.0 * (w * _eps(x)).sum(axis=1) + (x.shape[1] + 1) * FLOOR) / Z


# ------------------------------------------------------------------------------------------------------------------ kept sets
def presort(x):
    """-> (order, xs): the ascending stable sort of every row, to share among calls of kept_sets on the same rows"""
    x = _rows(x)
    order = np.argsort(x, axis=1, kind='stable')
    return order, np.take_along_axis(x, order, axis=1)


def topk_mask(x, top_k, sorted_rows=None):
    """x_e >= the k-th largest value for 0 < k < V (ties kept; -0.0 == +0.0 as floats compare), everything otherwise"""
    x = _rows(x)
    R, V = x.shape
    k = np.broadcast_to(np.asarray(top_k, dtype=np.int64), (R,))
    _, xs = sorted_rows or presort(x)
    kth = xs[np.arange(R), V - np.clip(k, 1, V)]
    kth = np.where((k > 0) & (k < V), kth, -np.inf)
    return x >= kth[:, None]


def kept_sets(x, top_k, top_p, sorted_rows=None):
    """-> (mask_a, mask_b, delta, ambiguous).  mask_a is the kept set with every doubtful comparison of the nucleus cut decided towards
    keeping, mask_b towards cutting; they are equal (ambiguous False) unless a cumulative mass lies within the cut's error bound of
    (1 - top_p).  Both exclude zero-mass tokens.  delta is the row's delta over the top-k set.
    top_k, top_p: scalars or one per row; top_p is taken as the float32 the kernel receives."""
    x = _rows(x)
    R, V = x.shape
    sorted_rows = sorted_rows or presort(x)
    mk = topk_mask(x, top_k, sorted_rows)
    w = masses(x, mk)
    Z = w.sum(axis=1)
    delta = delta_of(x, mk)
    p = np.broadcast_to(np.asarray(top_p, dtype=np.float32), (R,)).astype(np.float64)
    keep_from = np.clip(1.0 - p, 0.0, 1.0)
    order, xs = sorted_rows
    ws = np.take_along_axis(w, order, axis=1)
    es = np.take_along_axis(w * _eps(x), order, axis=1)
    nz = np.cumsum(ws > 0, axis=1)
    last = np.ones((R, V), dtype=bool)
    last[:, :-1] = xs[:, :-1] != xs[:, 1:]                       # last element of its value class

    def class_end(c):                                            # value of c at the end of each element's class
        c = np.where(last, c, np.inf)
        return np.minimum.accumulate(c[:, ::-1], axis=1)[:, ::-1]
    cum = class_end(np.cumsum(ws, axis=1)) / Z[:, None]
    cut_delta = _cut_delta(class_end(np.cumsum(es, axis=1)), class_end(nz.astype(np.float64)), es.sum(axis=1), keep_from, V, Z)
    exact = (keep_from == 0.0)[:, None]                          # top_p >= 1: "exceeds 0" is decided by the zero-mass rule alone
    qa = np.where(exact, cum > 0.0, cum > keep_from[:, None] - cut_delta)
    qb = np.where(exact, cum > 0.0, cum > keep_from[:, None] + cut_delta)
    qa[:, -1] = qb[:, -1] = True                                 # the maximum is always kept
    tau_a = xs[np.arange(R), qa.argmax(axis=1)]
    tau_b = xs[np.arange(R), qb.argmax(axis=1)]
    off = (p <= 0.0)[:, None]                                    # top_p <= 0: no nucleus cut
    ma = mk & (w > 0) & (off | (x >= tau_a[:, None]))
    mb = mk & (w > 0) & (off | (x >= tau_b[:, None]))
    return ma, mb, delta, (ma != mb).any(axis=1)


def _cut_delta(err_below, n_below, err_all, keep_from, V, Z):
    """error bound of (ascending partial sum) / Z against keep_from, per boundary: the partial sum is off by at most the errors of the
    elements below the boundary, keep_from * Z by that share of Z's error, and each by one unit of 2^-40 per element (plus one for the
    floor of keep_from * Z).  Its relative-error part never exceeds delta_of's: err_below <= err_all and keep_from <= 1."""
    kf = keep_from[:, None]
    return SAFETY * (err_below + kf * err_all[:, None] + (n_below + kf * V + 1.0) * FLOOR) / Z[:, None]


def count_classes_between(x, ma, mb):
    """number of distinct values kept by mask_a and not by mask_b, per row (0: unambiguous; 1: two candidate sets; more: several)"""
    x = _rows(x)
    return np.array([len(np.unique(r[a & ~b])) for r, a, b in zip(x, ma, mb)])


# ------------------------------------------------------------------------------------------------------------------ the draw
def draw_order(V: int) -> np.ndarray:
    """the documented element order of the inverse-CDF walk: ascending (e mod 256, e div 256)"""
    e = np.arange(V)
    return e[np.lexsort((e // 256, e % 256))]


def cdf(x, mask):
    """-> (order, F): F[r, j] = cumulative kept mass up to and including element order[j], over Z_kept (float64)"""
    x = _rows(x)
    order = draw_order(x.shape[1])
    w = masses(x, mask)[:, order]
    F = np.cumsum(w, axis=1)
    return order, F / F[:, -1:]


def candidates(x, mask, u, delta=None):
    """-> bool (R, n_u, V): the tokens whose float64 CDF interval [F_{j-1}, F_j) meets [u - delta, u + delta].  u: (R, n_u).  A kernel draw
    is right iff it is one of them; every draw has at least one.  Zero-mass tokens (empty intervals) are never candidates."""
    x = _rows(x)
    R, V = x.shape
    u = np.asarray(u, dtype=np.float64).reshape(R, -1)
    if delta is None:
        delta = delta_of(x, mask)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), (R,))
    order, F = cdf(x, mask)
    out = np.zeros((R, u.shape[1], V), dtype=bool)
    for r in range(R):
        f = F[r]
        nonempty = np.diff(f, prepend=0.0) > 0
        first = np.searchsorted(f, u[r] - delta[r], side='right')        # first j with F_j > u - delta
        last = np.searchsorted(f, u[r] + delta[r], side='right')         # last j with F_{j-1} <= u + delta (F_{-1} = 0)
        for i, (a, b) in enumerate(zip(first, np.minimum(last, V - 1))):
            out[r, i, order[a:b + 1]] = nonempty[a:b + 1]
    return out


def draw(x, mask, u):
    """the oracle's own token for u (delta = 0): first kept element in the documented order whose cumulative mass exceeds u * Z_kept"""
    x = _rows(x)
    u = np.asarray(u, dtype=np.float64).reshape(x.shape[0], -1)
    order, F = cdf(x, mask)
    j = np.array([np.searchsorted(f, v, side='right') for f, v in zip(F, u)])
    return order[np.minimum(j, x.shape[1] - 1)]


# ------------------------------------------------------------------------------------------------------------------ statistics
TAIL = 1e-9


def chi2_limit(dof: int, tail: float = TAIL) -> float:
    """upper `tail` quantile of chi-square(dof) by Wilson-Hilferty: dof (1 - 2/(9 dof) + z sqrt(2/(9 dof)))^3, z the normal quantile"""
    z = NormalDist().inv_cdf(1.0 - tail)
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + z * math.sqrt(a)) ** 3


def merge_small_bins(expected, minimum=10.0):
    """-> bin id per token: tokens in ascending expectation are pooled until a pool reaches `minimum`; a last pool that stays short joins
    the one before it.  Tokens with expectation >= minimum keep a bin of their own."""
    expected = np.asarray(expected, dtype=np.float64)
    order = np.argsort(expected, kind='stable')
    ids = np.empty(expected.size, dtype=np.int64)
    cur, acc = 0, 0.0
    for e in order:
        ids[e] = cur
        acc += expected[e]
        if acc >= minimum:
            cur, acc = cur + 1, 0.0
    if acc > 0.0 and cur > 0:                                    # a short last pool (the largest tokens never end up here)
        ids[ids == cur] = cur - 1
    return ids


def pearson(tokens, probs, minimum=10.0):
    """-> (statistic, dof) of the draws `tokens` against the float64 probabilities `probs`, bins with expectation < minimum merged"""
    tokens = np.asarray(tokens).reshape(-1)
    probs = np.asarray(probs, dtype=np.float64)
    n = tokens.size
    ids = merge_small_bins(probs * n, minimum)
    nb = int(ids.max()) + 1
    E = np.bincount(ids, weights=probs * n, minlength=nb)
    O = np.bincount(ids[tokens], minlength=nb).astype(np.float64)
    keep = E > 0
    stat = float((((O - E) ** 2)[keep] / E[keep]).sum())
    if O[~keep].sum() > 0:                                       # a draw of a token with probability zero
        stat = math.inf
    return stat, int(keep.sum()) - 1


def pair_share_bounds(probs, n_chains, chain_len, sigmas=6.0):
    """-> (lo, hi) for the share of equal adjacent pairs in n_chains independent chains of chain_len independent draws from `probs`.
    Mean q = sum p^2.  Neighbouring pairs share a draw: cov = sum p^3 - q^2, so the count over one chain of m = chain_len - 1 pairs has
    variance m q (1 - q) + 2 (m - 1) cov."""
    p = np.asarray(probs, dtype=np.float64)
    q = float((p ** 2).sum())
    cov = float((p ** 3).sum()) - q * q
    m = chain_len - 1
    var = n_chains * (m * q * (1 - q) + 2 * (m - 1) * cov)
    s = sigmas * math.sqrt(var) / (n_chains * m)
    return q - s, q + s


def distribution_row(V: int = 256) -> np.ndarray:
    """the row of the distribution tests (float32): one heavy token, the others near 6.2 nats below it with a +-0.3 spread, so that the
    light tokens hold about a third of the mass in equal-sized shares (expectation ~40 each in 32 768 draws: no bin is merged away) and sit
    on every thread and element slot.  A tilt of the logits moves mass between the two groups, which the Pearson statistic sees in a single
    well-filled bin; a positional bias shows among the light tokens."""
    g = np.random.default_rng(256)
    x = (-6.2 + g.uniform(-0.3, 0.3, size=V)).astype(np.float32)
    x[37] = 0.0
    return x
