"""float64 reference of cvar_score_rows (include/cvar_serve.h), shared by tests/test_score_host.py, test_gpu_score_rows.py and test_gpu_logprobs.py.

The combine is formed as the kernel forms it - fp32 products, rounded separately, added in fp32 in the order ((c0 l0 + c1 l1) + c2 l2) + c3 l3; numpy's
float32 arithmetic rounds every operation, so this is exact, and the kernel's `combined` is compared with it (and with the sampler's) bit for bit.  The
scores are then float64 functions of those fp32 values: rank and argmax are defined on them (ties are ties of fp32 values), and the bounds below cover
what the fp32 reduction adds, which is what their derivation counts."""
import numpy as np

# |logprob - ref| <= LP_ABS + LP_REL |ref|, |entropy - ref| <= ENT_ABS: from the kernel's order of evaluation (one rounding per expf term plus at most
# 24 additions on the exponent sum, about 1.6e-6 relative; logf of a value <= 4096, about 1e-6; two subtractions at 2^-24 of their results; doubled;
# the entropy bound is the same sum scaled by log V = 8.3) - not measured on the code under test
LP_ABS, LP_REL, ENT_ABS = 5e-6, 2.4e-7, 2e-5


def combine_f32(logits, coef, V):
    """logits (nrep, B, l, ldv) fp32, coef (B, 4) fp32 -> (B, l, V) fp32"""
    lg, cf = np.asarray(logits, dtype=np.float32)[..., :V], np.asarray(coef, dtype=np.float32)
    x = cf[:, 0, None, None] * lg[0]
    for r in range(1, lg.shape[0]):
        x = x + cf[:, r, None, None] * lg[r]
    return x


def score_ref(x, target):
    """x (..., V) fp32 combined logits, target (...) int -> logprob, entropy (float64), rank, argmax (int64); target < 0: logprob 0, rank -1"""
    x, target = np.asarray(x), np.asarray(target).astype(np.int64)
    x64 = x.astype(np.float64)
    d = x64 - x64.max(axis=-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        ex = np.exp(d)
        S = ex.sum(axis=-1)
        ent = np.log(S) - np.where(ex > 0, ex * d, 0.0).sum(axis=-1) / S
        t = np.maximum(target, 0)
        dt = np.take_along_axis(d, t[..., None], axis=-1)[..., 0]
        logprob = np.where(target >= 0, dt - np.log(S), 0.0)
    xt = np.take_along_axis(x, t[..., None], axis=-1)
    ahead = (x > xt) | ((x == xt) & (np.arange(x.shape[-1]) < t[..., None]))
    rank = np.where(target >= 0, ahead.sum(axis=-1), -1)
    return logprob, ent, rank, x.argmax(axis=-1)


def within_bounds(logprob, entropy, ref_logprob, ref_entropy):
    """(worst logprob error / its bound, worst entropy error / its bound); a -inf reference must be met exactly"""
    logprob, entropy = np.asarray(logprob, dtype=np.float64), np.asarray(entropy, dtype=np.float64)
    inf = np.isinf(ref_logprob)
    assert np.array_equal(logprob[inf], ref_logprob[inf])
    assert np.isfinite(entropy).all() and np.isfinite(logprob[~inf]).all()
    lp = np.abs(logprob[~inf] - ref_logprob[~inf]) / (LP_ABS + LP_REL * np.abs(ref_logprob[~inf]))
    en = np.abs(entropy - ref_entropy) / ENT_ABS
    return (float(lp.max()) if lp.size else 0.0), float(en.max())
