// CFG combine + greedy / top-k / top-p sampling over the 4096-way codebook (one workgroup per token).
//   combine: ((c0*l0 + c1*l1) + c2*l2) + c3*l3 with separately rounded products - the evaluation order of
//            control_var.py:295-298 / 501-502, so the combined logits are bit-identical to the reference's.
//   greedy : argmax, lowest index on ties, plus the top1-top2 margin (used for margin-aware parity checks).
//   sample : radix-select thresholds for top-k (ties kept, helpers.py:9-10) and the nucleus cut on the ascending
//            cumulative mass (helpers.py:12-15), inverse-CDF draw from a counter-based generator (no sort); or, with caller-drawn
//            Exp(1) noise q, torch.multinomial's draw for one sample per row: argmax(p / q) over the softmax p of the masked logits.
//   One text serves the scalar launch (cvar_cfg_sample: parameters in the kernel arguments) and the per-request launch (cvar_cfg_sample_rows: one
//   parameter set per batch row in device tables): greedy_token and sample_token are templates on the parameter struct and reach whatever differs
//   per row through the accessors below, nothing else.  A third form (cvar_cfg_sample_map, include/cvar_region.h) reads the combine weights per TOKEN.
#include "cvar_common.h"
#include "../../include/cvar_serve.h"
#include "../../include/cvar_region.h"
#include "../../include/cvar_topn.h"

struct SampleParams {
    const float* logits;
    int B, nrep, l, V;
    float coef[4];
    int top_k;
    float top_p;
    unsigned long long seed;
    const unsigned long long* seed_dev;     // optional device-resident seed added to `seed` (lets a captured hipGraph draw fresh samples)
    int stage, n_draw;
    int* idx_out;
    float* combined;
    float* margin;
    int* kept;
    int ldv;                                // row stride of `logits` in floats (>= V: a wider head whose first V columns are the codes)
    // more_smooth (control_var.py:511-515; helpers.py:22-36): soft code embedding of the top-k / top-p MASKED logits
    //   soft_out[(d*B + b)][t][:] = softmax_v( (lg_v * smooth_mul + g_v) / smooth_tau ) . codebook[v][:]      over the kept v
    const float* codebook;                  // [V][Cvae] fp32; NULL: no soft output
    int Cvae;
    float smooth_mul, smooth_tau;
    const float* gumbel;                    // optional injected Gumbel noise [n_draw*B][l][V] (tests); NULL: drawn from the counter generator
    float* soft_out;
    // ABI 22: caller-drawn Exp(1) noise [n_draw*B][l][V] (row stride V).  Non-NULL: the draw is torch.multinomial's one-sample path,
    // argmax_v(softmax(masked)_v / expo_v) (the race), instead of the counter generator's inverse-CDF lookup
    const float* expo;
};

// Per-request form (include/cvar_serve.h): one batch row = one request.  Combine weights, top_k, top_p and seed are read per row b from device
// tables (block-uniform loads: one workgroup per token).  No expo / soft_out: cvar_cfg_sample_rows refuses both.
struct RowSampleParams {
    const float* logits;
    int B, nrep, l, V, ldv;
    const float* coef;                      // [B][4] fp32, this stage's weights (host-rounded: never recomputed from cfg_b here)
    const int* top_k;                       // [B]   <= 0 or >= V: no top-k filter; 1: greedy
    const float* top_p;                     // [B]
    const unsigned long long* seed;         // [B]
    int stage, n_draw;
    int* idx_out;
    float* combined;
    float* margin;
    int* kept;
};

// Per-token form (include/cvar_region.h, regional guidance): the per-request form with the combine weights read per token (b, t) from this stage's
// slice of a [B][L][4] table, row stride ldc tokens.  Still a block-uniform load: one workgroup per token.  Everything else is the base's.
struct MapSampleParams : RowSampleParams {
    long ldc;
};

// ---- what differs between the forms: where a row's parameters come from, and which row keys the generator --------------------------------
// The per-request draw is keyed by (seed_b, stage, d, t) - the key the scalar form builds at B = 1, where d * 1 + 0 = d.  With everything else in
// one text, row b of a per-request launch is bit for bit the scalar launch at B = 1 on that row's logits, whatever rides beside it.
// seed_of is evaluated where a draw uses it, never handed down as a value: a by-value seed costs the SOFT instances 28 VGPRs and a wave per SIMD.
__device__ __forceinline__ const float* coef_of(const SampleParams& p, long, long) { return p.coef; }
__device__ __forceinline__ const float* coef_of(const RowSampleParams& p, long b, long) { return p.coef + b * 4; }
__device__ __forceinline__ const float* coef_of(const MapSampleParams& p, long b, long t) { return p.coef + (b * p.ldc + t) * 4; }
__device__ __forceinline__ int top_k_of(const SampleParams& p, long) { return p.top_k; }
__device__ __forceinline__ int top_k_of(const RowSampleParams& p, long b) { return p.top_k[b]; }
__device__ __forceinline__ float top_p_of(const SampleParams& p, long) { return p.top_p; }
__device__ __forceinline__ float top_p_of(const RowSampleParams& p, long b) { return p.top_p[b]; }
__device__ __forceinline__ unsigned long long seed_of(const SampleParams& p, long) { return p.seed + (p.seed_dev ? p.seed_dev[0] : 0ull); }
__device__ __forceinline__ unsigned long long seed_of(const RowSampleParams& p, long b) { return p.seed[b]; }
__device__ __forceinline__ long key_row(const SampleParams& p, int d, long b) { return (long)d * p.B + b; }
__device__ __forceinline__ long key_row(const RowSampleParams&, int d, long) { return d; }

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

template <class P>
__device__ __forceinline__ float combine_logits(const P& p, long b, long t, int e) {
    const long rowstride = (long)p.l * p.ldv;
    const float* base = p.logits + (b * p.l + t) * p.ldv + e;
    const float* cf = coef_of(p, b, t);
    float v = __fmul_rn(cf[0], base[0]);
    for (int r = 1; r < p.nrep; ++r) v = __fadd_rn(v, __fmul_rn(cf[r], base[(long)r * p.B * rowstride]));
    return v;
}

// the rank order of the greedy id and of cvar_score_rows - value descending (floats compared as floats), id ascending - for the top-N rounds.  It restates
// merge_top2's predicate on purpose: merge_top2 written through this helper compiled cfg_greedy_kernel to 13 VGPRs instead of 11 and the two score kernels to
// 50 instead of 48, and the resource lines of the existing kernels are kept as they are
__device__ __forceinline__ bool rank_before(float a, int ia, float b, int ib) { return (a > b) || (a == b && ia < ib); }

struct Top2 { float b1; int i1; float b2; };
__device__ __forceinline__ Top2 merge_top2(Top2 a, Top2 b) {
    Top2 o;
    const bool a_first = (a.b1 > b.b1) || (a.b1 == b.b1 && a.i1 < b.i1);
    if (a_first) { o.b1 = a.b1; o.i1 = a.i1; o.b2 = fmaxf(a.b2, b.b1); }
    else { o.b1 = b.b1; o.i1 = b.i1; o.b2 = fmaxf(b.b2, a.b1); }
    return o;
}

// argmax with the lowest index among tied maxima, the id in all n_draw rows, kept = 1
template <class P>
__device__ __forceinline__ void greedy_token(const P& p) {
    __shared__ float sb1[4], sb2[4];
    __shared__ int si1[4];
    const int tid = threadIdx.x;
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    Top2 best = {-INFINITY, 0x7fffffff, -INFINITY};
    for (int e = tid; e < p.V; e += 256) {
        const float v = combine_logits(p, b, t, e);
        if (p.combined) p.combined[bt * p.V + e] = v;
        Top2 cur = {v, e, -INFINITY};
        best = merge_top2(best, cur);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 other;
        other.b1 = __shfl_xor(best.b1, o, 64); other.i1 = __shfl_xor(best.i1, o, 64); other.b2 = __shfl_xor(best.b2, o, 64);
        best = merge_top2(best, other);
    }
    if ((tid & 63) == 0) { sb1[tid >> 6] = best.b1; si1[tid >> 6] = best.i1; sb2[tid >> 6] = best.b2; }
    __syncthreads();
    if (tid == 0) {
        Top2 r = {sb1[0], si1[0], sb2[0]};
        for (int w = 1; w < 4; ++w) { Top2 o = {sb1[w], si1[w], sb2[w]}; r = merge_top2(r, o); }
        for (int d = 0; d < p.n_draw; ++d) p.idx_out[((long)d * p.B + b) * p.l + t] = r.i1;
        if (p.margin) p.margin[bt] = r.b1 - r.b2;
        if (p.kept) p.kept[bt] = 1;
    }
}

__global__ __launch_bounds__(256) void cfg_greedy_kernel(const SampleParams p) { greedy_token(p); }

// ---- top-k / top-p sampling without a sort ---------------------------------------------------------------------
// Both filters of helpers.py:8-15 are VALUE thresholds: top-k keeps v >= (k-th largest value) (ties kept), the nucleus
// cut keeps the elements whose ascending cumulative probability exceeds 1-p, i.e. v >= tau_p.  Each threshold is found
// by a 4-pass byte-wise radix select over order-preserving integer keys (count histogram for top-k, probability-mass
// histogram for top-p).  Masses are quantised to 2^-40 and accumulated as 64-bit integers: exact, order independent,
// bit-reproducible.  The draw is an inverse-CDF lookup over the kept elements in a fixed (thread-major) order: ascending (e mod 256, e div 256).
// A mass below 2^-40 of the maximum's quantises to zero: such a token is never drawn and is not counted in `kept` (the sampler's contract).
__device__ __forceinline__ unsigned f2key(float f) {           // monotone: a < b  <=>  key(a) < key(b), and a == b  <=>  key(a) == key(b):
    unsigned u = __float_as_uint(f);                           // -0.0 takes the key of +0.0 (they compare equal: a tie with the cut is kept)
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <typename TV>
__device__ __forceinline__ TV wave_incl_scan(TV v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const TV n = __shfl_up(v, o, 64); if (lane >= o) v += n; }
    return v;
}
// exclusive prefix of one value per thread over the 256-thread block (+ block total through `total`)
template <typename TV>
__device__ __forceinline__ TV block_excl_scan(TV v, TV* wsum /*[4]*/, TV& total) {
    const TV inc = wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) wsum[w] = inc;
    __syncthreads();
    TV base = 0;
    for (int i = 0; i < w; ++i) base += wsum[i];
    total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    return base + inc - v;
}

// argmax order of torch (first index on ties; a NaN beats every number, the first NaN wins): does (a, ia) come before (b, ib)?
__device__ __forceinline__ bool race_before(float a, int ia, float b, int ib) {
    const bool na = a != a, nb = b != b;
    if (na || nb) return na && (!nb || ia < ib);
    return a > b || (a == b && ia < ib);
}

// SOFT = false (every launch without more_smooth): the soft-embedding block and its registers compile away (146 -> ~90 VGPRs: the kernel is
// bound by memory and LDS latency, and went 44 % slower when the block cost it two of its five waves per SIMD).
// RACE = true (expo != NULL): the draw is torch.multinomial's one-sample path on the caller's noise; RACE = false compiles the counter draw only.
template <bool SOFT, bool RACE, class P>
__device__ __forceinline__ void sample_token(const P& p) {
    constexpr int EPT = 16;
    typedef unsigned long long u64;
    __shared__ int hist_cnt[256];
    __shared__ u64 hist_mass[256];
    __shared__ u64 wsum64[4];
    __shared__ int wsum32[4];
    __shared__ float wmaxs[4], wmax2[4];
    __shared__ unsigned sel_digit;
    __shared__ u64 sel_below;
    __shared__ int sel_k;
    const int tid = threadIdx.x;
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    float v[EPT];
    unsigned key[EPT];
    float best = -INFINITY, second = -INFINITY;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const int e = i * 256 + tid;                   // thread-strided ownership: coalesced loads
        float x = -INFINITY;
        if (e < p.V) {
            x = combine_logits(p, b, t, e);
            if (p.combined) p.combined[bt * p.V + e] = x;
        }
        v[i] = x; key[i] = f2key(x);
        if (x > best) { second = best; best = x; } else if (x > second) second = x;
    }
    // block max (+ second max for the margin output)
    {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, 64), os = __shfl_xor(second, o, 64);
            second = fmaxf(fminf(best, ob), fmaxf(second, os));
            best = fmaxf(best, ob);
        }
        if ((tid & 63) == 0) { wmaxs[tid >> 6] = best; wmax2[tid >> 6] = second; }
        __syncthreads();
        best = wmaxs[0]; second = wmax2[0];
        for (int w = 1; w < 4; ++w) { second = fmaxf(fminf(best, wmaxs[w]), fmaxf(second, wmax2[w])); best = fmaxf(best, wmaxs[w]); }
        if (p.margin && tid == 0) p.margin[bt] = best - second;
    }
    const float vmax = best;

    // ---- top-k threshold key
    unsigned tk = 0;
    const int top_k = top_k_of(p, b);
    if (top_k > 0 && top_k < p.V) {
        unsigned prefix = 0;
        int kk = top_k;
        for (int ps = 3; ps >= 0; --ps) {
            hist_cnt[tid] = 0;
            if (tid == 0) { sel_digit = 0u; sel_k = kk; }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EPT; ++i) {
                const bool match = (ps == 3) || ((key[i] >> (8 * (ps + 1))) == prefix);
                if (match && i * 256 + tid < p.V) atomicAdd(&hist_cnt[(key[i] >> (8 * ps)) & 255], 1);
            }
            __syncthreads();
            const int dd = 255 - tid;                              // thread t owns digit 255-t: suffix counts become a prefix scan
            const int c = hist_cnt[dd];
            int tot;
            const int above = block_excl_scan<int>(c, wsum32, tot);   // elements with a larger digit
            if (above < kk && above + c >= kk) { sel_digit = (unsigned)dd; sel_k = kk - above; }
            __syncthreads();
            prefix = (prefix << 8) | sel_digit;
            kk = sel_k;
            __syncthreads();
        }
        tk = prefix;
    }
    // ---- quantised masses of the top-k set
    u64 wq[EPT];
    u64 local = 0;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        const bool in = (i * 256 + tid < p.V) && key[i] >= tk;
        wq[i] = in ? (u64)(__expf(v[i] - vmax) * 1099511627776.0f) : 0ull;      // 2^40
        local += wq[i];
    }
    u64 Z;
    (void)block_excl_scan<u64>(local, wsum64, Z);
    // ---- nucleus threshold key: smallest key whose ascending cumulative mass exceeds (1 - top_p) * Z
    unsigned tp = 0;
    const float top_p = top_p_of(p, b);
    if (top_p > 0.f) {
        // (1 - top_p) in double and clamped: top_p < 2^-24 would round 1 - top_p to 1 in float (lim == Z: no bucket qualifies), and
        // top_p > 1 would cast a negative double to u64.  lim <= Z - 1 guarantees that exactly one bucket per pass satisfies the
        // selection below; Z > 0 always (the maximum carries mass 2^40).  The last (largest) element is therefore always kept, as
        // helpers.py:14 does.  Elements TIED with the cut value are all kept here (value threshold), where the reference cuts
        // inside the tie by sort order - a difference only for exactly equal logits.
        const double keep_from = fmin(fmax(1.0 - (double)top_p, 0.0), 1.0);
        u64 lim = (u64)(keep_from * (double)Z);
        if (lim >= Z) lim = Z - 1;
        unsigned prefix = 0;
        u64 below = 0;
        for (int ps = 3; ps >= 0; --ps) {
            hist_mass[tid] = 0ull;
            if (tid == 0) { sel_digit = 255u; sel_below = below; }      // defined even if no bucket were selected
            __syncthreads();
#pragma unroll
            for (int i = 0; i < EPT; ++i) {
                const bool match = (ps == 3) || ((key[i] >> (8 * (ps + 1))) == prefix);
                if (match && wq[i]) atomicAdd(&hist_mass[(key[i] >> (8 * ps)) & 255], wq[i]);
            }
            __syncthreads();
            const u64 c = hist_mass[tid];
            u64 tot;
            const u64 before = below + block_excl_scan<u64>(c, wsum64, tot);   // mass of smaller digits (ascending)
            if (before <= lim && before + c > lim) { sel_digit = (unsigned)tid; sel_below = before; }
            __syncthreads();
            prefix = (prefix << 8) | sel_digit;
            below = sel_below;
            __syncthreads();
        }
        tp = prefix;
    }
    const unsigned thr = tk > tp ? tk : tp;
    u64 keepsum = 0;
    int nkeep = 0;
#pragma unroll
    for (int i = 0; i < EPT; ++i) {
        if (!(key[i] >= thr && wq[i])) wq[i] = 0ull;
        keepsum += wq[i];
        nkeep += wq[i] ? 1 : 0;
    }
    u64 Zk;
    const u64 excl = block_excl_scan<u64>(keepsum, wsum64, Zk);
    if (p.kept) {
        int tot;
        (void)block_excl_scan<int>(nkeep, wsum32, tot);
        if (tid == 0) p.kept[bt] = tot;
    }
    if constexpr (RACE) {
        // torch.multinomial(softmax(masked), 1, generator) = argmax_v(p_v / q_v) with q = empty_like(p).exponential_(generator) (ATen's
        // one-sample path): the same IEEE fp32 steps as softmax then div - p_v = expf(x_v - m) / S over the kept v, 0 elsewhere (the -inf
        // of the masked logits), then p_v / q_v over ALL V columns, so that 0 / 0 (a masked v meeting q_v = 0) is a NaN and wins as in torch.
        // m = vmax (the maximum is always kept).  The kept set is the value threshold above: top-k ties kept, top_k == 1 keeps every maximum.
        __shared__ float red_s[4], rmax[4];
        __shared__ int ridx[4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < EPT; ++i)
            if (i * 256 + tid < p.V && key[i] >= thr) s = __fadd_rn(s, expf(__fsub_rn(v[i], vmax)));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
        if ((tid & 63) == 0) red_s[tid >> 6] = s;
        __syncthreads();
        const float S = __fadd_rn(__fadd_rn(red_s[0], red_s[1]), __fadd_rn(red_s[2], red_s[3]));
        for (int d = 0; d < p.n_draw; ++d) {
            const long row = (long)d * p.B + b;
            const float* q = p.expo + (row * p.l + t) * (long)p.V;
            float best_r = -INFINITY;
            int best_i = 0x7fffffff;
#pragma unroll
            for (int i = 0; i < EPT; ++i) {
                const int e = i * 256 + tid;
                if (e < p.V) {
                    const float pv = key[i] >= thr ? __fdiv_rn(expf(__fsub_rn(v[i], vmax)), S) : 0.f;
                    const float r = __fdiv_rn(pv, q[e]);
                    if (race_before(r, e, best_r, best_i)) { best_r = r; best_i = e; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float orr = __shfl_xor(best_r, o, 64);
                const int oi = __shfl_xor(best_i, o, 64);
                if (race_before(orr, oi, best_r, best_i)) { best_r = orr; best_i = oi; }
            }
            __syncthreads();                               // rmax / ridx of the previous draw are read
            if ((tid & 63) == 0) { rmax[tid >> 6] = best_r; ridx[tid >> 6] = best_i; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < 4; ++w)
                    if (race_before(rmax[w], ridx[w], best_r, best_i)) { best_r = rmax[w]; best_i = ridx[w]; }
                p.idx_out[row * p.l + t] = best_i;
            }
        }
    } else {
        for (int d = 0; d < p.n_draw; ++d) {
            unsigned long long h = splitmix64(seed_of(p, b) ^ 0xC0FFEE1234ull);
            h = splitmix64(h ^ ((unsigned long long)p.stage << 48) ^ ((unsigned long long)key_row(p, d, b) << 16) ^ (unsigned long long)t);
            const double u = (double)(h >> 11) * (1.0 / 9007199254740992.0);       // 53 bits -> [0,1)
            u64 target = (u64)(u * (double)Zk);
            if (target >= Zk) target = Zk > 0 ? Zk - 1 : 0;
            if (excl <= target && target < excl + keepsum) {                        // exactly one thread
                u64 run = excl;
                int pick = tid;
#pragma unroll
                for (int i = 0; i < EPT; ++i) {
                    run += wq[i];
                    if (run > target) { pick = i * 256 + tid; break; }
                }
                p.idx_out[((long)d * p.B + b) * p.l + t] = pick;
            }
        }
    }
    if constexpr (SOFT) {
    if (p.soft_out) {
        // Gumbel-softmax over the KEPT logits (the reference masks `logits` in place before it calls gumbel_softmax_with_rng), then the
        // expectation of the code vectors under it.  One pass per draw row: the reference draws fresh noise for every replicated row.
        __shared__ float red[4];
        __shared__ float accs[4][32];
        for (int d = 0; d < p.n_draw; ++d) {
            const long row = (long)d * p.B + b;
            float z[EPT];
            float zmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < EPT; ++i) {
                const int e = i * 256 + tid;
                z[i] = -INFINITY;
                if (e < p.V && key[i] >= thr) {
                    float g;
                    if (p.gumbel) g = p.gumbel[(row * p.l + t) * (long)p.V + e];
                    else {
                        unsigned long long h = splitmix64(seed_of(p, b) ^ 0x5EEDF00D77ull);
                        h = splitmix64(h ^ ((unsigned long long)p.stage << 52) ^ ((unsigned long long)key_row(p, d, b) << 28) ^ ((unsigned long long)t << 12) ^ (unsigned long long)e);
                        const float u = ((float)(h >> 40) + 0.5f) * (1.0f / 16777216.0f);          // (0, 1)
                        g = -__logf(-__logf(u));                                                 // -log(Exp(1) sample)
                    }
                    z[i] = (v[i] * p.smooth_mul + g) / p.smooth_tau;
                    zmax = fmaxf(zmax, z[i]);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) zmax = fmaxf(zmax, __shfl_xor(zmax, o, 64));
            __syncthreads();
            if ((tid & 63) == 0) red[tid >> 6] = zmax;
            __syncthreads();
            zmax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
            float acc[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = 0.f;
            float wsum = 0.f;
#pragma unroll
            for (int i = 0; i < EPT; ++i) {
                const float w = z[i] > -INFINITY ? __expf(z[i] - zmax) : 0.f;
                if (w > 0.f) {
                    wsum += w;
                    const float* er = p.codebook + (long)(i * 256 + tid) * p.Cvae;
                    for (int c = 0; c < p.Cvae; ++c) acc[c] = fmaf(w, er[c], acc[c]);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                wsum += __shfl_xor(wsum, o, 64);
#pragma unroll
                for (int c = 0; c < 32; ++c) acc[c] += __shfl_xor(acc[c], o, 64);
            }
            __syncthreads();
            if ((tid & 63) == 0) {
                red[tid >> 6] = wsum;
                for (int c = 0; c < p.Cvae; ++c) accs[tid >> 6][c] = acc[c];
            }
            __syncthreads();
            if (tid < p.Cvae) {
                const float tot = (red[0] + red[1]) + (red[2] + red[3]);
                const float a = (accs[0][tid] + accs[1][tid]) + (accs[2][tid] + accs[3][tid]);
                p.soft_out[(row * p.l + t) * (long)p.Cvae + tid] = a / tot;
            }
        }
    }
    }
}

template <bool SOFT, bool RACE>
__global__ __launch_bounds__(256) void cfg_sample_kernel(const SampleParams p) { sample_token<SOFT, RACE>(p); }

// A row with top_k_b == 1 leaves through greedy_token (lowest index among tied maxima, kept = 1), never through a draw among the ties.  The branch
// is block-uniform and sits ahead of the sampler's sixteen loads per thread: a greedy reduction over those loaded values cost 121 VGPRs and a wave.
__global__ __launch_bounds__(256) void cfg_sample_rows_kernel(const RowSampleParams p) {
    if (p.top_k[blockIdx.x / p.l] == 1) { greedy_token(p); return; }
    sample_token<false, false>(p);
}

// Region-constrained generation (include/cvar_serve.h): token (b, t) is forced to forced[b * ldf + t] when that is >= 0.  The load is block-uniform
// and sits ahead of everything else: a forced token leaves before it reads a logit.  forced / ldf ride beside RowSampleParams, not inside it, so
// that cfg_sample_rows_kernel keeps its argument block and its instruction stream.
__global__ __launch_bounds__(256) void cfg_sample_edit_kernel(const RowSampleParams p, const int* __restrict__ forced, const int ldf) {
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    const int id = forced[b * ldf + t];
    if (id >= 0) {
        if (threadIdx.x == 0) {
            for (int d = 0; d < p.n_draw; ++d) p.idx_out[((long)d * p.B + b) * p.l + t] = id;
            if (p.margin) p.margin[bt] = INFINITY;
            if (p.kept) p.kept[bt] = 0;
        }
        return;
    }
    if (p.top_k[b] == 1) { greedy_token(p); return; }
    sample_token<false, false>(p);
}

// Regional guidance (include/cvar_region.h): the per-token form, with cfg_sample_edit_kernel's forcing when a table is given (forced == NULL: nothing
// is forced).  A kernel of its own, so that the two above keep their argument blocks and instruction streams.
__global__ __launch_bounds__(256) void cfg_sample_map_kernel(const MapSampleParams p, const int* __restrict__ forced, const int ldf) {
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    const int id = forced ? forced[b * ldf + t] : -1;
    if (id >= 0) {
        if (threadIdx.x == 0) {
            for (int d = 0; d < p.n_draw; ++d) p.idx_out[((long)d * p.B + b) * p.l + t] = id;
            if (p.margin) p.margin[bt] = INFINITY;
            if (p.kept) p.kept[bt] = 0;
        }
        return;
    }
    if (p.top_k[b] == 1) { greedy_token(p); return; }
    sample_token<false, false>(p);
}

// ---- token log-probabilities (cvar_score_rows, include/cvar_serve.h) ------------------------------------------------------------------------
// Scores a GIVEN id per token under the unfiltered CFG-combined distribution: log-probability, entropy, rank and the greedy id.  The combine is
// combine_logits above (the sampler's text: `combined` and the argmax are the sampler's bits), the parameters of a row come from the same coef
// table through coef_of.  The order of evaluation depends on nothing but (V, tid): thread tid owns elements tid + 256 j and adds them in
// increasing j, a 64-lane xor-shuffle tree follows, the four wave partials are added in order 0..3.  No atomics; accurate expf / logf.
struct ScoreParams {
    const float* logits;
    int B, nrep, l, V, ldv;
    const float* coef;                      // [B][4] fp32, this stage's weights: the sampler's table
    const int* target;                      // [B][ldt] int32; < 0: the token has no target
    int ldt, ldo;                           // row strides of target and of the four per-token outputs (>= l)
    float* combined;
    float* logprob;
    float* entropy;
    int* rank;
    int* argmax;
};
struct MapScoreParams : ScoreParams {       // cvar_score_map (include/cvar_region.h): the weights per token, as MapSampleParams reads them
    long ldc;
};
__device__ __forceinline__ const float* coef_of(const ScoreParams& p, long b, long) { return p.coef + b * 4; }
__device__ __forceinline__ const float* coef_of(const MapScoreParams& p, long b, long t) { return p.coef + (b * p.ldc + t) * 4; }

// The fixed order of S, shared by score_token and the top-N kernel so that their bits cannot drift apart: a term is expf(x - m) with the difference
// rounded first; a wave adds its lanes' partials over the xor tree; the four wave partials are added in order 0..3; logprob = (x - m) - logf(S).
__device__ __forceinline__ float score_wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = __fadd_rn(s, __shfl_xor(s, o, 64));
    return s;
}
__device__ __forceinline__ float score_waves_0123(const float* w) { return __fadd_rn(__fadd_rn(__fadd_rn(w[0], w[1]), w[2]), w[3]); }
__device__ __forceinline__ float score_logprob(float x, float m, float logS) { return __fsub_rn(__fsub_rn(x, m), logS); }

template <class P>
__device__ __forceinline__ void score_token(const P& p) {
    constexpr int EPT = 16;
    __shared__ float sb1[4], ssum[4], sent[4];           // the second maximum feeds nothing here: it is not kept
    __shared__ int si1[4], scnt[4];
    const int tid = threadIdx.x;
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    int tgt = p.target[b * p.ldt + t];                             // block-uniform
    if (tgt >= p.V) tgt = -1;                                      // out of contract (the host checks ids): nothing outside the row is read
    float v[EPT];
    Top2 best = {-INFINITY, 0x7fffffff, -INFINITY};
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = j * 256 + tid;                               // thread-strided ownership: the row is read once, coalesced
        float x = -INFINITY;
        if (e < p.V) {
            x = combine_logits(p, b, t, e);
            if (p.combined) p.combined[bt * p.V + e] = x;
            Top2 cur = {x, e, -INFINITY};
            best = merge_top2(best, cur);                          // greedy_token's loop order: increasing e per thread
        }
        v[j] = x;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Top2 other;
        other.b1 = __shfl_xor(best.b1, o, 64); other.i1 = __shfl_xor(best.i1, o, 64); other.b2 = __shfl_xor(best.b2, o, 64);
        best = merge_top2(best, other);
    }
    if ((tid & 63) == 0) { sb1[tid >> 6] = best.b1; si1[tid >> 6] = best.i1; }
    __syncthreads();
    Top2 r = {sb1[0], si1[0], -INFINITY};
    for (int w = 1; w < 4; ++w) { Top2 o = {sb1[w], si1[w], -INFINITY}; r = merge_top2(r, o); }
    const float m = r.b1;
    // the target's value: every thread evaluates the combine at the target column (a block-uniform load) - the owning lane's bits
    const float xt = tgt >= 0 ? combine_logits(p, b, t, tgt) : 0.f;
    float s = 0.f, u = 0.f;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = j * 256 + tid;
        if (e < p.V) {
            const float d = __fsub_rn(v[j], m);
            const float ex = expf(d);
            s = __fadd_rn(s, ex);
            if (ex != 0.f) u = __fadd_rn(u, __fmul_rn(ex, d));     // a -inf logit carries no mass: 0 * -inf never forms
            cnt += (v[j] > xt || (v[j] == xt && e < tgt)) ? 1 : 0;
        }
    }
    s = score_wave_sum(s);
    u = score_wave_sum(u);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) { ssum[tid >> 6] = s; sent[tid >> 6] = u; scnt[tid >> 6] = cnt; }
    __syncthreads();
    if (tid == 0) {
        const float S = score_waves_0123(ssum);
        const float U = score_waves_0123(sent);
        const float logS = logf(S);
        const long o = b * p.ldo + t;
        if (p.logprob) p.logprob[o] = tgt >= 0 ? score_logprob(xt, m, logS) : 0.f;
        if (p.entropy) p.entropy[o] = __fsub_rn(logS, __fdiv_rn(U, S));
        if (p.rank) p.rank[o] = tgt >= 0 ? (scnt[0] + scnt[1]) + (scnt[2] + scnt[3]) : -1;
        if (p.argmax) p.argmax[o] = r.i1;
    }
}

__global__ __launch_bounds__(256) void cfg_score_rows_kernel(const ScoreParams p) { score_token(p); }
__global__ __launch_bounds__(256) void cfg_score_map_kernel(const MapScoreParams p) { score_token(p); }

// ---- the N most likely codes (cvar_score_topn, include/cvar_topn.h) --------------------------------------------------------------------------
// score_token's row in score_token's registers (combine_logits, thread-strided ownership), then N rounds of a block arg-max in score_token's
// rank order - value descending, id ascending, floats compared as floats - over the elements no earlier round took.  A thread keeps the best of
// its own sixteen and rescans them only after it owned a winner, so a round is one 64-lane tree, one barrier (the wave slots are double-buffered
// on the round's parity) and a four-way merge.  The order is rank_before, merge_top2's predicate restated (see there), so round 0's winner is score_token's maximum, bits
// included; S goes through score_token's own helpers (score_wave_sum, score_waves_0123, score_logprob), and the tail sum runs in the same order over
// the elements left.
struct TopnParams {
    const float* logits;
    int B, nrep, l, V, ldv;
    const float* coef;                      // [B][4] fp32: the table cvar_score_rows reads
    int N, ldo;
    int* top_id;
    float* top_logprob;
    float* tail_logprob;
};
__device__ __forceinline__ const float* coef_of(const TopnParams& p, long b, long) { return p.coef + b * 4; }

__global__ __launch_bounds__(256) void cfg_score_topn_kernel(const TopnParams p) {
    constexpr int EPT = 16;
    constexpr int NONE = 0x7fffffff;                               // loses every tie: a real -inf element ranks ahead of "nothing left"
    __shared__ float swv[2][4], sel_v[64], ssum[4], stail[4];
    __shared__ int swi[2][4], sel_i[64];
    const int tid = threadIdx.x;
    const long bt = blockIdx.x;
    const long b = bt / p.l, t = bt % p.l;
    float v[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = j * 256 + tid;
        v[j] = e < p.V ? combine_logits(p, b, t, e) : -INFINITY;
    }
    unsigned taken = 0u;
    float lv = -INFINITY;
    int li = NONE;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = j * 256 + tid;
        if (e < p.V && rank_before(v[j], e, lv, li)) { lv = v[j]; li = e; }
    }
    for (int r = 0; r < p.N; ++r) {
        float wv = lv;
        int wi = li;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(wv, o, 64);
            const int oi = __shfl_xor(wi, o, 64);
            if (rank_before(ov, oi, wv, wi)) { wv = ov; wi = oi; }
        }
        if ((tid & 63) == 0) { swv[r & 1][tid >> 6] = wv; swi[r & 1][tid >> 6] = wi; }
        __syncthreads();
        wv = swv[r & 1][0]; wi = swi[r & 1][0];
        for (int w = 1; w < 4; ++w)
            if (rank_before(swv[r & 1][w], swi[r & 1][w], wv, wi)) { wv = swv[r & 1][w]; wi = swi[r & 1][w]; }
        if (tid == 0) { sel_v[r] = wv; sel_i[r] = wi; }
        if (wi < p.V && (wi & 255) == tid) {                       // the owner strikes it and rescans its sixteen
            taken |= 1u << (wi >> 8);
            lv = -INFINITY; li = NONE;
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const int e = j * 256 + tid;
                if (e < p.V && !((taken >> j) & 1u) && rank_before(v[j], e, lv, li)) { lv = v[j]; li = e; }
            }
        }
    }
    __syncthreads();
    const float m = sel_v[0];
    float s = 0.f, st = 0.f;
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = j * 256 + tid;
        if (e < p.V) {
            const float d = __fsub_rn(v[j], m);
            const float ex = expf(d);
            s = __fadd_rn(s, ex);
            if (!((taken >> j) & 1u)) st = __fadd_rn(st, ex);
        }
    }
    s = score_wave_sum(s);
    st = score_wave_sum(st);
    if ((tid & 63) == 0) { ssum[tid >> 6] = s; stail[tid >> 6] = st; }
    __syncthreads();
    const float S = score_waves_0123(ssum);
    const float logS = logf(S);
    const long o = b * p.ldo + t;
    if (tid < p.N) {
        const int id = sel_i[tid];
        const bool real = id < p.V;
        if (p.top_id) p.top_id[o * p.N + tid] = real ? id : -1;
        if (p.top_logprob) p.top_logprob[o * p.N + tid] = real ? score_logprob(sel_v[tid], m, logS) : -INFINITY;
    }
    if (p.tail_logprob && tid == 0) {
        const float St = score_waves_0123(stail);
        p.tail_logprob[o] = St > 0.f ? __fsub_rn(logf(St), logS) : -INFINITY;
    }
}

extern "C" int cvar_cfg_sample(const float* logits, int B, int nrep, int l, int V, const float* coef_host,
                               int top_k, float top_p, uint64_t seed, const uint64_t* seed_dev, int stage, int n_draw,
                               int32_t* idx_out, float* combined, float* margin, int32_t* kept, int ldv,
                               const float* codebook, int Cvae, float smooth_mul, float smooth_tau, const float* gumbel, float* soft_out,
                               const float* expo, void* stream) {
    if (!logits || !coef_host || !idx_out || B <= 0 || l <= 0 || V <= 1) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || n_draw < 1 || n_draw > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    if (soft_out && (!codebook || Cvae < 1 || Cvae > 32 || !(smooth_tau > 0.f))) return CVAR_EINVAL;
    if (soft_out && top_k == 1) return CVAR_EUNSUPPORTED;          // greedy: the masked softmax is one-hot, the soft embedding IS codebook[idx]
    SampleParams p;
    p.expo = expo;
    p.ldv = ldv ? ldv : V;
    p.codebook = codebook; p.Cvae = Cvae; p.smooth_mul = smooth_mul; p.smooth_tau = smooth_tau; p.gumbel = gumbel; p.soft_out = soft_out;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V;
    for (int i = 0; i < 4; ++i) p.coef[i] = i < nrep ? coef_host[i] : 0.f;
    p.top_k = top_k; p.top_p = top_p; p.seed = seed; p.seed_dev = (const unsigned long long*)seed_dev; p.stage = stage; p.n_draw = n_draw;
    p.idx_out = idx_out; p.combined = combined; p.margin = margin; p.kept = kept;
    dim3 grid((unsigned)((long)B * l)), block(256);
    if (expo) {                                                    // the race, top_k == 1 included: every tied maximum is kept and drawn among
        if (soft_out) hipLaunchKernelGGL((cfg_sample_kernel<true, true>), grid, block, 0, as_stream(stream), p);
        else hipLaunchKernelGGL((cfg_sample_kernel<false, true>), grid, block, 0, as_stream(stream), p);
    } else if (top_k == 1) hipLaunchKernelGGL(cfg_greedy_kernel, grid, block, 0, as_stream(stream), p);
    else if (soft_out) hipLaunchKernelGGL((cfg_sample_kernel<true, false>), grid, block, 0, as_stream(stream), p);
    else hipLaunchKernelGGL((cfg_sample_kernel<false, false>), grid, block, 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_serve_version(void) { return 1; }

extern "C" int cvar_cfg_sample_rows(const float* logits, int B, int nrep, int l, int V, const float* coef, const int32_t* top_k,
                                    const float* top_p, const int64_t* seed, int stage, int n_draw, int32_t* idx_out, float* combined,
                                    float* margin, int32_t* kept, int ldv, const float* expo, float* soft_out, void* stream) {
    if (!logits || !coef || !top_k || !top_p || !seed || !idx_out || B <= 0 || l <= 0 || V <= 1) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || n_draw < 1 || n_draw > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    if (expo || soft_out) return CVAR_EUNSUPPORTED;                // caller-drawn noise and more_smooth have no per-row form
    RowSampleParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.top_k = (const int*)top_k; p.top_p = top_p; p.seed = (const unsigned long long*)seed;
    p.stage = stage; p.n_draw = n_draw;
    p.idx_out = idx_out; p.combined = combined; p.margin = margin; p.kept = kept;
    hipLaunchKernelGGL(cfg_sample_rows_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_score_rows(const float* logits, int B, int nrep, int l, int V, const float* coef, const int32_t* target, int ldt,
                               float* combined, float* logprob, float* entropy, int32_t* rank, int32_t* argmax, int ldo, int ldv, void* stream) {
    if (!logits || !coef || !target || B <= 0 || l <= 0 || V < 1 || ldt < l || (ldo != 0 && ldo < l)) return CVAR_EINVAL;
    if (!combined && !logprob && !entropy && !rank && !argmax) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    ScoreParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.target = (const int*)target; p.ldt = ldt; p.ldo = ldo ? ldo : l;
    p.combined = combined; p.logprob = logprob; p.entropy = entropy; p.rank = (int*)rank; p.argmax = (int*)argmax;
    hipLaunchKernelGGL(cfg_score_rows_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_cfg_sample_edit(const float* logits, int B, int nrep, int l, int V, const float* coef, const int32_t* top_k,
                                    const float* top_p, const int64_t* seed, int stage, int n_draw, int32_t* idx_out, float* combined,
                                    float* margin, int32_t* kept, int ldv, const float* expo, float* soft_out, const int32_t* forced, int ldf,
                                    void* stream) {
    if (!logits || !coef || !top_k || !top_p || !seed || !idx_out || B <= 0 || l <= 0 || V <= 1) return CVAR_EINVAL;
    if (!forced || ldf < l) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || n_draw < 1 || n_draw > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    if (expo || soft_out) return CVAR_EUNSUPPORTED;
    RowSampleParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.top_k = (const int*)top_k; p.top_p = top_p; p.seed = (const unsigned long long*)seed;
    p.stage = stage; p.n_draw = n_draw;
    p.idx_out = idx_out; p.combined = combined; p.margin = margin; p.kept = kept;
    hipLaunchKernelGGL(cfg_sample_edit_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p, (const int*)forced, ldf);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

// ---- regional guidance (include/cvar_region.h): the sampler and the score launch with per-token combine weights ---------------------------------
extern "C" int cvar_cfg_sample_map(const float* logits, int B, int nrep, int l, int V, const float* coef, int ldc, const int32_t* top_k,
                                   const float* top_p, const int64_t* seed, int stage, int n_draw, int32_t* idx_out, float* combined,
                                   float* margin, int32_t* kept, int ldv, const float* expo, float* soft_out, const int32_t* forced, int ldf,
                                   void* stream) {
    if (!logits || !coef || !top_k || !top_p || !seed || !idx_out || B <= 0 || l <= 0 || V <= 1) return CVAR_EINVAL;
    if (ldc < l || (forced && ldf < l)) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || n_draw < 1 || n_draw > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    if (expo || soft_out) return CVAR_EUNSUPPORTED;                // as the per-row form: no caller-drawn noise, no more_smooth
    MapSampleParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.top_k = (const int*)top_k; p.top_p = top_p; p.seed = (const unsigned long long*)seed;
    p.stage = stage; p.n_draw = n_draw;
    p.idx_out = idx_out; p.combined = combined; p.margin = margin; p.kept = kept;
    p.ldc = ldc;
    hipLaunchKernelGGL(cfg_sample_map_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p, (const int*)forced, ldf);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_score_map(const float* logits, int B, int nrep, int l, int V, const float* coef, int ldc, const int32_t* target, int ldt,
                              float* combined, float* logprob, float* entropy, int32_t* rank, int32_t* argmax, int ldo, int ldv, void* stream) {
    if (!logits || !coef || !target || B <= 0 || l <= 0 || V < 1 || ldt < l || ldc < l || (ldo != 0 && ldo < l)) return CVAR_EINVAL;
    if (!combined && !logprob && !entropy && !rank && !argmax) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || V > 4096) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    MapScoreParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.target = (const int*)target; p.ldt = ldt; p.ldo = ldo ? ldo : l;
    p.combined = combined; p.logprob = logprob; p.entropy = entropy; p.rank = (int*)rank; p.argmax = (int*)argmax;
    p.ldc = ldc;
    hipLaunchKernelGGL(cfg_score_map_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

// ---- the N most likely codes (include/cvar_topn.h): cvar_score_rows' launch shape and refusals ---------------------------------------------------
extern "C" int cvar_score_topn(const float* logits, int B, int nrep, int l, int V, const float* coef, int N, int32_t* top_id, float* top_logprob,
                               float* tail_logprob, int ldo, int ldv, void* stream) {
    if (!logits || !coef || B <= 0 || l <= 0 || V < 1 || (ldo != 0 && ldo < l)) return CVAR_EINVAL;
    if (!top_id && !top_logprob) return CVAR_EINVAL;
    if (nrep < 1 || nrep > 4 || V > 4096 || N < 1 || N > 64) return CVAR_EUNSUPPORTED;
    if (ldv != 0 && ldv < V) return CVAR_EINVAL;
    TopnParams p;
    p.logits = logits; p.B = B; p.nrep = nrep; p.l = l; p.V = V; p.ldv = ldv ? ldv : V;
    p.coef = coef; p.N = N; p.ldo = ldo ? ldo : l;
    p.top_id = (int*)top_id; p.top_logprob = top_logprob; p.tail_logprob = tail_logprob;
    hipLaunchKernelGGL(cfg_score_topn_kernel, dim3((unsigned)((long)B * l)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}
