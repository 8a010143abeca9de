"""Input families shared by tests/test_sample_oracle_host.py (the caps, computed on the CPU from the oracle alone) and
tests/test_gpu_sample_oracle.py (the same inputs through the kernels).  numpy only: the host file runs without torch on the device.

One family = (V, nrep, sigma): l = 64 tokens x B = 4 rows, one logits row per (b, t), drawn as sigma * randn before the combine.  The combine
is restated in float32 with separately rounded products and sums, so that the combined logits are known on the CPU bit for bit; elements
whose mass would lie in the oracle's undecidable band around the 2^-40 floor are moved out of it before anything runs (`build`)."""
import zlib

import numpy as np

from oracle import sample_ref as S

L, B = 64, 4
VS = (4096, 1000, 300)
NREPS = (1, 2, 4)
SIGMAS = (0.3, 1.0, 2.5)
COEF = {1: [1.0], 2: [1.5, -0.5], 4: [1.3, -0.15, -0.075, -0.075]}
SEEDS = (0, 2 ** 63 + 5, 2 ** 64 - 1)
STAGES = (0, 19)
FAMILIES = [(V, nrep, sigma) for V in VS for nrep in NREPS for sigma in SIGMAS]
# (seed, stage, d, t) of B = 1 scalar launches whose u is below 2^-28: the first hits of find_small_u() below
SMALL_U = ((1647351, 19, 0, 55), (1923148, 19, 0, 19))


def filters(V):
    return [(0, 0.0), (900, 0.96), (0, 0.5), (50, 0.0), (600, 0.999), (V, 1.0), (V - 1, 0.0)]


def family_index(V, nrep, sigma):
    return FAMILIES.index((V, nrep, sigma))


def family_params(V, nrep, sigma):
    """what rides along with a family, cycled so that every value meets every V: seed, seed_dev, stage, n_draw, ldv"""
    i = family_index(V, nrep, sigma)
    seed = SEEDS[(i + i // 3) % 3]
    return dict(seed=seed, seed_dev=(2 ** 40 + 17) if i % 5 == 2 else 0, stage=STAGES[(i + i // 9) % 2], n_draw=(1, 4)[(i // 3 + i) % 2],
                ldv=V + 64 if (V, nrep, sigma) in ((1000, 2, 1.0), (300, 4, 2.5)) else 0)


def build(V, nrep, sigma, ldv=0, coef=None, rows=B * L, tag=0):
    """-> (logits (nrep, rows, ld) float32, combined (rows, V) float32) with no mass in the floor band.  coef: (rows, nrep) or (nrep,)"""
    ld = ldv or V
    g = np.random.default_rng(zlib.crc32(repr((V, nrep, sigma, tag)).encode()))
    lg = (g.standard_normal((nrep, rows, ld)) * sigma).astype(np.float32)
    if ld > V:
        lg[:, :, V:] = 100.0                                     # behind the codes: larger than every logit, must never be read
    coef = np.asarray(COEF[nrep] if coef is None else coef, dtype=np.float32)
    cf = coef.T[:, :, None] if coef.ndim == 2 else coef[:, None, None]

    def comb():
        v = cf[0] * lg[0, :, :V]
        for r in range(1, nrep):
            v = v + cf[r] * lg[r, :, :V]
        return v
    for _ in range(8):
        x = comb()
        band = S.floor_band(x)
        if not band.any():
            return lg, x
        lg[0, :, :V][band] += np.float32(1.0)                    # lift the element clear of the floor
    raise AssertionError('could not clear the floor band')


def draw_us(seed, seed_dev, stage, n_draw, form, seeds_rows=None):
    """-> u (B * L rows in (b, t) order, n_draw).  form 'scalar': key_row = d B + b, seed + seed_dev; 'rows': key_row = d, seed[b]"""
    u = np.empty((B, L, n_draw))
    for b in range(B):
        for d in range(n_draw):
            for t in range(L):
                if form == 'scalar':
                    u[b, t, d] = S.counter_u((seed + seed_dev) & S.M64, stage, d * B + b, t)
                else:
                    u[b, t, d] = S.counter_u(seeds_rows[b], stage, d, t)
    return u.reshape(B * L, n_draw)


def rows_tables(V, nrep, sigma):
    """per-request tables of a family: row b gets its own weights (the family's times a factor that is no power of two), filter and seed"""
    fl = filters(V)
    i = family_index(V, nrep, sigma)
    pick = [fl[(i + 2 * b) % len(fl)] for b in range(B)]
    coef = np.zeros((B, 4), dtype=np.float32)
    for b, s in enumerate((1.0, 0.7, 1.15, 0.9)):
        coef[b, :nrep] = np.asarray(COEF[nrep], dtype=np.float32) * np.float32(s)
    seeds = [SEEDS[(i + b) % 3] if b < 3 else 123456789012345 + i for b in range(B)]
    return coef, np.array([k for k, _ in pick], dtype=np.int32), np.array([p for _, p in pick], dtype=np.float32), seeds


def find_small_u(limit=2.0 ** -28, seeds=range(0, 1 << 22), chunk=1 << 15, n_t=64, n_d=4, stages=STAGES, want=2):
    """search (seed, stage, d, t) of a B = 1 scalar launch whose u is below `limit` (a few minutes of numpy; not run by any test: the
    hits the tests pin were found with it, and the tests re-derive their u with the oracle's exact hash)"""
    def mix(x):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))
    grid = np.array([(s << 48) ^ (d << 16) ^ t for s in stages for d in range(n_d) for t in range(n_t)], dtype=np.uint64)
    keys = [(s, d, t) for s in stages for d in range(n_d) for t in range(n_t)]
    top = np.uint64(int(limit * 2.0 ** 64))
    hits = []
    with np.errstate(over='ignore'):
        for s0 in range(seeds.start, seeds.stop, chunk):
            sd = np.arange(s0, min(s0 + chunk, seeds.stop), dtype=np.uint64)
            h = mix(mix(sd ^ np.uint64(0xC0FFEE1234))[:, None] ^ grid[None, :])
            for i, j in zip(*np.nonzero(h < top)):
                hits.append((int(sd[i]),) + keys[j])
            if len(hits) >= want:
                break
    return hits
