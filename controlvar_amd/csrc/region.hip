// Regional guidance: the per-token combine weights of every scale from latent-resolution region maps (include/cvar_region.h).
//   One wave per token of the generation order, in the shape of edit_force_table_kernel.  Cell (i, j) of scale pn covers the latent rows
//   floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the same columns.  The lanes walk the bin 64 cells at a time (the pn = 1 token of a 32 x 32 latent
//   reads 1024 cells: 16 steps); each lane adds its cells' normalised weights and strength in float64 in increasing cell order, a 64-lane xor-shuffle
//   tree follows, and lane 0 forms the four weights and stores them as one 16-byte vector.  The order of evaluation depends on nothing but the bin:
//   the same inputs give the same bits.  No atomics, no LDS, one vector store per token, 64-bit indexing.
#include "cvar_common.h"
#include "../../include/cvar_region.h"

struct RegionTableParams {
    const float* regions;                   // [B][K][S][S], >= 0, every latent cell with a positive sum over k
    const float* strength;                  // [B][S][S], >= 0; NULL = 1
    const double* cfg;                      // [B][K]
    int pn[16];
    int nstage, B, K, S, mf;
    int L;                                  // sum mf * pn^2
    float* coef;                            // [B][L][4]
};

__global__ __launch_bounds__(256) void region_coef_table_kernel(const RegionTableParams p) {
    const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;          // wave-uniform: the token of this wave
    const int lane = threadIdx.x & 63;
    if (g >= (long)p.B * p.L) return;
    const long b = g / p.L;
    int off = (int)(g % p.L), pn = p.pn[0], si = 0;
    for (; si < p.nstage; ++si) {                                        // the token's scale
        pn = p.pn[si];
        const int n = p.mf * pn * pn;
        if (off < n) break;
        off -= n;
    }
    const int cell = off % (pn * pn);                                    // both halves read the same maps: the order of the halves changes no value
    const int i = cell / pn, j = cell % pn;
    const int r0 = i * p.S / pn, r1 = ((i + 1) * p.S + pn - 1) / pn;
    const int c0 = j * p.S / pn, c1 = ((j + 1) * p.S + pn - 1) / pn;
    const int bw = c1 - c0, n = (r1 - r0) * bw;
    const long SS = (long)p.S * p.S;
    const float* w = p.regions + b * p.K * SS;
    const float* st = p.strength ? p.strength + b * SS : nullptr;
    double acc[3] = {0.0, 0.0, 0.0}, accg = 0.0;
    for (int q = lane; q < n; q += 64) {
        const long c = (long)(r0 + q / bw) * p.S + c0 + q % bw;
        double wk[3], s = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            wk[k] = k < p.K ? (double)w[k * SS + c] : 0.0;
            if (k < p.K) s += wk[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < p.K) acc[k] += wk[k] / s;
        if (st) accg += (double)st[c];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += __shfl_xor(acc[k], o, 64);
        accg += __shfl_xor(accg, o, 64);
    }
    if (lane != 0) return;
    const double gbar = st ? accg / (double)n : 1.0;
    const double ratio = (double)si / (double)(p.nstage - 1);
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    double neg = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (k < p.K) {
            const double wbar = acc[k] / (double)n;
            const double t = (p.cfg[b * p.K + k] * gbar) * ratio;
            out[k] = (float)(wbar * (1.0 + t));
            neg += wbar * t;
            if (k == p.K - 1) out[k + 1] = (float)(-neg);
        }
    }
    *reinterpret_cast<float4*>(p.coef + g * 4) = make_float4(out[0], out[1], out[2], out[3]);
}

extern "C" int cvar_region_coef_table(const float* regions, const float* strength, const double* cfg, const int* patch_nums, int nstage, int B, int K,
                                      int S, int mask_first, int mask_factor, float* coef, void* stream) {
    (void)mask_first;
    if (!regions || !cfg || !coef || !patch_nums || B <= 0 || S <= 0 || K < 1 || K > 3 || nstage < 2 || nstage > 16) return CVAR_EINVAL;
    if (mask_factor != 1 && mask_factor != 2) return CVAR_EUNSUPPORTED;
    if (S > 1024) return CVAR_EUNSUPPORTED;
    if (((uintptr_t)coef & 15) != 0) return CVAR_EUNSUPPORTED;           // one 16-byte store per token
    RegionTableParams p;
    long L = 0;
    for (int i = 0; i < 16; ++i) p.pn[i] = 1;
    for (int i = 0; i < nstage; ++i) {
        if (patch_nums[i] < 1 || patch_nums[i] > S) return CVAR_EINVAL;
        p.pn[i] = patch_nums[i];
        L += (long)mask_factor * patch_nums[i] * patch_nums[i];
    }
    if (patch_nums[nstage - 1] != S) return CVAR_EINVAL;
    if ((long)B * L >= (1l << 31) / 64) return CVAR_EUNSUPPORTED;        // 64 threads per token in a 32-bit grid
    p.regions = regions; p.strength = strength; p.cfg = cfg;
    p.nstage = nstage; p.B = B; p.K = K; p.S = S; p.mf = mask_factor; p.L = (int)L;
    p.coef = coef;
    hipLaunchKernelGGL(region_coef_table_kernel, dim3((unsigned)(((long)B * L + 3) / 4)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}
