// Region-constrained generation: the forced-token table of every scale from latent-resolution keep masks (include/cvar_serve.h).
//   One wave per token of the generation order.  Cell (i, j) of scale pn covers the latent rows floor(i S / pn) .. ceil((i + 1) S / pn) - 1 and the
//   same columns - the bins of F.interpolate(mode='area'), with which the quantizer forms that token (quant.py:199,238).  The lanes walk the bin
//   64 cells at a time, a ballot + popcount counts the kept ones (the pn = 1 token of a 32 x 32 latent reads 1024 cells: 16 steps), and lane 0
//   stores the source id when 2 * kept > bin size (a strict majority in integers: an exact half stays free), -1 otherwise.
//   No atomics, no LDS, one vector store per token.
#include "cvar_common.h"
#include "../../include/cvar_serve.h"

struct ForceTableParams {
    const unsigned char* keep[2];           // [0] control, [1] image: [B][S][S], NULL = nothing kept
    const int* src[2];                      // [B][Lsrc] ids of the half, scale after scale
    int pn[16];
    int nstage, B, S, mask_first, mf;
    int L, Lsrc;                            // sum mf * pn^2, sum pn^2
    int* forced;                            // [B][L]
};

__global__ __launch_bounds__(256) void edit_force_table_kernel(const ForceTableParams p) {
    const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;          // wave-uniform: the token of this wave
    const int lane = threadIdx.x & 63;
    if (g >= (long)p.B * p.L) return;
    const long b = g / p.L;
    int off = (int)(g % p.L), soff = 0, pn = p.pn[0];
    for (int si = 0; si < p.nstage; ++si) {                              // the token's scale: offsets into forced (off) and into src (soff)
        pn = p.pn[si];
        const int n = p.mf * pn * pn;
        if (off < n) break;
        off -= n; soff += pn * pn;
    }
    const int first = off < pn * pn;
    const int cell = first ? off : off - pn * pn;
    const int half = p.mf == 1 ? 1 : (first == (p.mask_first != 0) ? 0 : 1);      // 0 control, 1 image
    const unsigned char* keep = p.keep[half];
    int id = -1;
    if (keep) {                                                          // wave-uniform
        const int i = cell / pn, j = cell % pn;
        const int r0 = i * p.S / pn, r1 = ((i + 1) * p.S + pn - 1) / pn;
        const int c0 = j * p.S / pn, c1 = ((j + 1) * p.S + pn - 1) / pn;
        const int w = c1 - c0, n = (r1 - r0) * w;
        const unsigned char* m = keep + b * p.S * p.S;
        int cnt = 0;
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            const bool on = k < n && m[(r0 + k / w) * p.S + c0 + k % w] != 0;
            cnt += __popcll(__ballot(on));
        }
        if (2 * cnt > n) id = p.src[half][b * p.Lsrc + soff + cell];
    }
    if (lane == 0) p.forced[g] = id;
}

extern "C" int cvar_edit_force_table(const uint8_t* keep_ctrl, const uint8_t* keep_img, const int32_t* src_ctrl, const int32_t* src_img,
                                     const int* patch_nums, int nstage, int B, int S, int mask_first, int mask_factor, int32_t* forced,
                                     void* stream) {
    if (!forced || !patch_nums || B <= 0 || S <= 0 || nstage < 1) return CVAR_EINVAL;
    if ((keep_ctrl && !src_ctrl) || (keep_img && !src_img)) return CVAR_EINVAL;
    if (mask_factor != 1 && mask_factor != 2) return CVAR_EUNSUPPORTED;
    if (nstage > 16 || S > 1024) return CVAR_EUNSUPPORTED;
    if (mask_factor == 1 && keep_ctrl) return CVAR_EINVAL;               // a plain model has no control half
    ForceTableParams p;
    long L = 0, Lsrc = 0;
    for (int i = 0; i < 16; ++i) p.pn[i] = 1;
    for (int i = 0; i < nstage; ++i) {
        if (patch_nums[i] < 1 || patch_nums[i] > S) return CVAR_EINVAL;
        p.pn[i] = patch_nums[i];
        Lsrc += (long)patch_nums[i] * patch_nums[i];
    }
    if (patch_nums[nstage - 1] != S) return CVAR_EINVAL;
    L = mask_factor * Lsrc;
    if ((long)B * L >= (1l << 31) / 64) return CVAR_EUNSUPPORTED;        // 64 threads per token in a 32-bit grid
    p.keep[0] = keep_ctrl; p.keep[1] = keep_img; p.src[0] = (const int*)src_ctrl; p.src[1] = (const int*)src_img;
    p.nstage = nstage; p.B = B; p.S = S; p.mask_first = mask_first; p.mf = mask_factor; p.L = (int)L; p.Lsrc = (int)Lsrc;
    p.forced = (int*)forced;
    hipLaunchKernelGGL(edit_force_table_kernel, dim3((unsigned)(((long)B * L + 3) / 4)), dim3(256), 0, as_stream(stream), p);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}
