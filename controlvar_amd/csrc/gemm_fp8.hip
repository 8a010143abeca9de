// gemm_precision='fp8' (include/cvar_serve.h): the row quantiser and the e4m3 GEMM for gfx950 (MI355X).
//
//   C[row(m), n] = epilogue( (sum_k qA[m,k] qW[n,k] * a_scale[m]) * w_scale[n] )
//
// The GEMM keeps the shape of the bf16 tiles of gemm.hip: a K tile is 128 bytes per row, moved global -> LDS by 16-byte DMA chunks
// (global_load_lds_dwordx4), two LDS stages, one barrier per K tile, the chunk index XOR-swizzled with (row >> 1) & 7 on the source
// side.  128 bytes of e4m3 are ONE k-step of v_mfma_scale_f32_16x16x128_f8f6f4: a lane's fragment is 32 bytes (two adjacent chunks),
// and a wave issues one MFMA per 16x16 block per K tile.  The hardware block scales are the constant 1.0 (e8m0 0x7F).
// Operand lane map: the A and the B operand of the instruction use one map (row / column = lane & 15, the 32 bytes of lane group
// lane >> 4 are the same k positions on both sides), so a sum over k only needs both fragments read from the same chunks.
// The W fragment goes first (as in the bf16 tiles): lane & 15 is then the output row and the four registers of a lane are four
// consecutive output columns 4 (lane >> 4) + r - the quads the shared epilogue takes.
// K ascends in blocks of 128 with no K slices, and every 16x16 block is its own accumulator chain: the bits of an output element do
// not depend on M, the tile or the batch.
#include "cvar_common.h"
#include "gemm_params.h"
#include "fp8_quant.h"
#include "../../include/cvar_serve.h"

static __device__ __attribute__((aligned(16))) unsigned int cvar_fp8_zero_chunk[4] = {0u, 0u, 0u, 0u};

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef int v8i_t __attribute__((ext_vector_type(8)));
typedef int v4i_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------
// Row pass: one wave per row, as split3_kernel.  TX = float or bf16_t.
// ------------------------------------------------------------------------------------------------
template <typename TX>
__global__ __launch_bounds__(256) void quant_rows_fp8_kernel(const TX* __restrict__ x, long ldx, long M, int K, unsigned char* __restrict__ q, long ldq,
                                                             float* __restrict__ scale) {
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const TX* xr = x + m * ldx;
    unsigned ab = 0u;
    for (int c = lane; c < K; c += 64) ab = max(ab, fp8_abs_bits(Elem<TX>::ld(xr + c)));
    ab = wave_max_u32(ab);
    const bool bad = ab >= 0x7f800000u;
    const int k = fp8_row_exp(ab);
    const float inv = fp8_pow2(-k);
    unsigned char* qr = q + m * ldq;
    // four bytes per lane and store; columns >= K (K % 4 != 0 and the pad up to ldq) are zero bytes
    for (long c = (long)lane * 4; c < ldq; c += 256) {
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = c + e < K ? Elem<TX>::ld(xr + c + e) * inv : 0.f;
        unsigned w = bad ? 0x7f7f7f7fu : fp8_pack4(v[0], v[1], v[2], v[3]);
        if (c + 4 > K) w &= c >= K ? 0u : (0xffffffffu >> (8 * (int)(c + 4 - K)));
        *(unsigned*)(qr + c) = w;
    }
    if (lane == 0) scale[m] = bad ? 1.0f : fp8_pow2(k);
}

extern "C" int cvar_quant_rows_fp8(const void* x, int x_dtype, int64_t ldx, int64_t M, int K, void* q, int64_t ldq, float* scale, void* stream) {
    if (!x || !q || !scale || M <= 0 || K <= 0) return CVAR_EINVAL;
    if (x_dtype != CVAR_F32 && x_dtype != CVAR_BF16) return CVAR_EUNSUPPORTED;
    if (ldq % 128 || ldq < K || ldx < K || ((uintptr_t)q & 3)) return CVAR_EUNSUPPORTED;
    const long blocks = (M + 3) / 4;
    if (blocks > 0x7fffffffL) return CVAR_EUNSUPPORTED;
    if (x_dtype == CVAR_F32)
        hipLaunchKernelGGL(quant_rows_fp8_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const float*)x, (long)ldx, (long)M, K,
                           (unsigned char*)q, (long)ldq, scale);
    else
        hipLaunchKernelGGL(quant_rows_fp8_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const bf16_t*)x, (long)ldx, (long)M, K,
                           (unsigned char*)q, (long)ldq, scale);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

// ------------------------------------------------------------------------------------------------
// The epilogue of one output quad (row m, columns n .. n + 3, those < N) on the scaled sums v: gemm_epilogue_quad's arithmetic in its order
// (gemm_params.h; the fields cvar_gemm_fp8 refuses - pre_act, aux, gate_scale - are not here).  ONE text for both access forms: vec = the
// 16-byte loads and stores of the fast path (the caller checked the alignments and N % 4 == 0), otherwise element accesses with the
// column bound, so that any N and any alignment is served with the same bits.  b4: the bias of the four columns (zeros without one).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fp8_epilogue_quad(const GemmParams& p, int m, int n, f32x4_t v, f32x4_t b4, bool vec) {
    const int nc = vec ? 4 : min(4, p.N - n);
    long orow = m;
    if (p.remap_l > 0) {
        const int sq = fast_div(m, p.remap_magic, p.remap_shift);
        orow = (long)sq * p.remap_L + p.remap_off + (m - sq * p.remap_l);
    }
    f32x4_t g4 = {1.f, 1.f, 1.f, 1.f}, r4 = {0.f, 0.f, 0.f, 0.f};
    if (p.gate) {
        const float* grow = p.gate + (long)fast_div(m, p.gate_magic, p.gate_shift) * p.ldg + n;
        if (vec) g4 = *(const f32x4_t*)grow;
        else {
            if (nc > 0) g4[0] = grow[0];
            if (nc > 1) g4[1] = grow[1];
            if (nc > 2) g4[2] = grow[2];
            if (nc > 3) g4[3] = grow[3];
        }
    }
    if (p.residual) {
        const long ro = (long)m * p.ldr + n;
        if (vec && p.res_dtype == CVAR_BF16) {
            const bf16x4_t q = *(const bf16x4_t*)((const bf16_t*)p.residual + ro);
#pragma unroll
            for (int e = 0; e < 4; ++e) r4[e] = bf16_to_f32((bf16_t)q[e]);
        } else if (vec) r4 = *(const f32x4_t*)((const float*)p.residual + ro);
        else {
            if (nc > 0) r4[0] = ld_any(p.residual, p.res_dtype, ro);
            if (nc > 1) r4[1] = ld_any(p.residual, p.res_dtype, ro + 1);
            if (nc > 2) r4[2] = ld_any(p.residual, p.res_dtype, ro + 2);
            if (nc > 3) r4[3] = ld_any(p.residual, p.res_dtype, ro + 3);
        }
    }
    float x[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        x[e] = v[e] * p.alpha;
        if (p.bias) x[e] += b4[e];
        if (p.act == CVAR_ACT_GELU_TANH) x[e] = gelu_tanh_f(x[e]);
        if (p.gate) x[e] *= g4[e];
        if (p.residual) x[e] += r4[e];
        if (p.split_n > 0 && n + e < p.split_n) x[e] *= p.split_alpha;
    }
    if (vec) {                                             // split_n % 4 == 0: a quad lies on one side of the column split
        void* dst = p.C;
        long off = orow * p.ldc + n;
        if (p.split_n > 0) {
            if (n < p.split_n) { dst = p.Cs; off = (long)m * p.ld_split + n; }
            else off = orow * p.ldc + (n - p.split_n);
        }
        if (p.out_dtype == CVAR_BF16) *(bf16x4_t*)((bf16_t*)dst + off) = pack_bf16x4(x);
        else *(f32x4_t*)((float*)dst + off) = f32x4_t{x[0], x[1], x[2], x[3]};
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (e >= nc) continue;
        if (p.split_n > 0 && n + e < p.split_n) st_any(p.Cs, p.out_dtype, (long)m * p.ld_split + n + e, x[e]);
        else st_any(p.C, p.out_dtype, orow * p.ldc + (n + e - max(p.split_n, 0)), x[e]);
    }
}

// ------------------------------------------------------------------------------------------------
// BM x BN tile on WM x WN waves; each wave owns (BM / WM) x (BN / WN) as 16x16 blocks.
// ------------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void cvar_gemm_fp8_kernel(const GemmParams p, const float* __restrict__ a_scale, const float* __restrict__ w_scale) {
    constexpr int NW = WM * WN;
    constexpr int A_INSTR = BM / 8, B_INSTR = BN / 8;          // 1 KiB DMA pieces (8 rows x 128 B) per K tile
    static_assert(A_INSTR % NW == 0 && B_INSTR % NW == 0, "tile / wave mismatch");
    constexpr int A_PER_W = A_INSTR / NW, B_PER_W = B_INSTR / NW;
    constexpr int STAGE = (BM + BN) * 128;
    constexpr int SUB_M = BM / WM, SUB_N = BN / WN;
    constexpr int MI = SUB_M / 16, NJ = SUB_N / 16;
    static_assert(SUB_M % 16 == 0 && SUB_N % 16 == 0, "sub-tile must be 16x16 blocks");
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    int m0, n0;
    gemm_tile_origin(p, (int)blockIdx.x, BM, BN, m0, n0);

    // per-lane DMA sources: row (piece * 8 + lane >> 3), LDS slot lane & 7 <- global chunk slot ^ ((row >> 1) & 7); rows past M / N read zeros
    const char* const zero = (const char*)cvar_fp8_zero_chunk;
    const int lr = lane >> 3, slot = lane & 7;
    const char* a_ptr[A_PER_W];
    const char* w_ptr[B_PER_W];
#pragma unroll
    for (int jj = 0; jj < A_PER_W; ++jj) {
        const int row = (wave + jj * NW) * 8 + lr;
        const int m = m0 + row;
        a_ptr[jj] = m < p.M ? p.A + (long)m * p.lda + (slot ^ ((row >> 1) & 7)) * 16 : nullptr;
    }
#pragma unroll
    for (int jj = 0; jj < B_PER_W; ++jj) {
        const int row = (wave + jj * NW) * 8 + lr;
        const int n = n0 + row;
        w_ptr[jj] = n < p.N ? p.W + (long)n * p.ldw + (slot ^ ((row >> 1) & 7)) * 16 : nullptr;
    }
    auto issue_tile = [&](int kt, int stage) {
        char* sbase = smem + stage * STAGE;
#pragma unroll
        for (int jj = 0; jj < A_PER_W; ++jj) {
            const char* src = a_ptr[jj] ? a_ptr[jj] + (long)kt * 128 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + (wave + jj * NW) * 1024), 16, 0, 0);
        }
#pragma unroll
        for (int jj = 0; jj < B_PER_W; ++jj) {
            const char* src = w_ptr[jj] ? w_ptr[jj] + (long)kt * 128 : zero;
            __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(sbase + BM * 128 + (wave + jj * NW) * 1024), 16, 0, 0);
        }
    };

    f32x4_t acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K >> 7;
    const int l15 = lane & 15, kq = lane >> 4, sw = (l15 >> 1) & 7;
    const int c0 = ((2 * kq) ^ sw) * 16, c1 = ((2 * kq + 1) ^ sw) * 16;      // the two chunks of this lane group's 32 k bytes
    auto frag = [&](const char* rowp) {
        const v4i_t lo = *(const v4i_t*)(rowp + c0), hi = *(const v4i_t*)(rowp + c1);
        return v8i_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };

    issue_tile(0, 0);
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        // this wave's pieces of tile kt have landed; behind the barrier everybody's have, and nobody reads tile kt - 1's stage any more
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if (kt + 1 < nk) issue_tile(kt + 1, cur ^ 1);
        const char* As = smem + cur * STAGE + (wm * SUB_M + l15) * 128;
        const char* Bs = smem + cur * STAGE + BM * 128 + (wn * SUB_N + l15) * 128;
        v8i_t bw[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) bw[j] = frag(Bs + j * 16 * 128);
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const v8i_t af = frag(As + i * 16 * 128);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(bw[j], af, acc[i][j], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
        }
        cur ^= 1;
    }

    // ---- epilogue (fp8_epilogue_quad): accumulators -> LDS (a 16-row staging region per wave, in the released pipeline stages) -> row-major quads, so that the bias / gate /
    // residual loads and the C stores are 16-byte accesses of whole row segments (SUB_N columns = SUB_N / 4 lanes per row).
    // C/D layout with the W fragment first: lane & 15 = output row inside the block, the four registers = columns 4 (lane >> 4) + r.
    __syncthreads();                                       // every wave has read its last fragments: the stages are free
    constexpr int EROW = SUB_N + 4;                        // fp32 row stride of the staging region (16-byte aligned, rows on distinct banks)
    constexpr int LPR = SUB_N / 4;                         // lanes per output row
    constexpr int RPP = 64 / LPR;                          // rows per pass
    static_assert(64 % LPR == 0 && 16 % RPP == 0 && NW * 16 * EROW * 4 <= 2 * STAGE, "epilogue staging must fit the pipeline LDS");
    float* stg = (float*)smem + wave * (16 * EROW);
    const int erow = lane / LPR, ecol = (lane % LPR) * 4;
    const int n = n0 + wn * SUB_N + ecol;
    const int out4 = p.out_dtype == CVAR_BF16 ? 7 : 15;
    const bool vec_ok = ((p.N & 3) == 0) && ((p.ldc & 3) == 0) && (((uintptr_t)p.C & out4) == 0) && (((uintptr_t)w_scale & 15) == 0) &&
                        (!p.residual || (((p.ldr & 3) == 0) && (((uintptr_t)p.residual & (p.res_dtype == CVAR_BF16 ? 7 : 15)) == 0))) &&
                        (!p.gate || (((p.ldg & 3) == 0) && (((uintptr_t)p.gate & 15) == 0))) && (!p.bias || (((uintptr_t)p.bias & 15) == 0)) &&
                        (p.split_n <= 0 || (((p.split_n & 3) == 0) && ((p.ld_split & 3) == 0) && (((uintptr_t)p.Cs & out4) == 0)));
    // per-lane constants of the row-major phase: the column quad never changes
    f32x4_t ws4 = {0.f, 0.f, 0.f, 0.f}, b4 = {0.f, 0.f, 0.f, 0.f};
    if (n < p.N) {
        if (vec_ok) {
            ws4 = *(const f32x4_t*)(w_scale + n);
            if (p.bias) b4 = *(const f32x4_t*)(p.bias + n);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ws4[e] = n + e < p.N ? w_scale[n + e] : 0.f;
                if (p.bias && n + e < p.N) b4[e] = p.bias[n + e];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) *(f32x4_t*)(stg + l15 * EROW + j * 16 + 4 * kq) = acc[i][j];
        __builtin_amdgcn_wave_barrier();                   // (the LDS serves one wave's accesses in order: the rows below see the stores above)
#pragma unroll
        for (int ps = 0; ps < 16 / RPP; ++ps) {
            const int r = ps * RPP + erow;
            const int m = m0 + wm * SUB_M + i * 16 + r;
            f32x4_t v = *(const f32x4_t*)(stg + r * EROW + ecol);
            if (m >= p.M || n >= p.N) continue;
            const float sa = a_scale[m];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (v[e] * sa) * ws4[e];
            fp8_epilogue_quad(p, m, n, v, b4, vec_ok);
        }
        __builtin_amdgcn_wave_barrier();                   // the next block row overwrites the staging rows
    }
}

template <int BM, int BN, int WM, int WN>
static int launch_fp8(const GemmParams& gp, const float* a_scale, const float* w_scale, hipStream_t st) {
    GemmParams p = gp;
    p.tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    p.group_m = p.K >= 4096 ? 4 : 8;
    const size_t lds = 2 * (BM + BN) * 128;
    auto kfn = cvar_gemm_fp8_kernel<BM, BN, WM, WN>;
    static unsigned char lds_set[64] = {0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !lds_set[dev]) {
        (void)hipFuncSetAttribute((const void*)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (dev >= 0 && dev < 64) lds_set[dev] = 1;
    }
    hipLaunchKernelGGL(kfn, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(WM * WN * 64), lds, st, p, a_scale, w_scale);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_gemm_fp8(const cvar_gemm_desc* d, const float* a_scale, const float* w_scale, void* stream) {
    if (!d || !d->A || !d->W || !d->C || !a_scale || !w_scale) return CVAR_EINVAL;
    if (d->M <= 0 || d->N <= 0 || d->K <= 0) return CVAR_EINVAL;
    if (d->conv || d->batch > 1 || d->ws || d->ln_out || d->gn_part || d->pre_act || d->aux || d->gate_scale || d->act == CVAR_ACT_GELU_GRAD) return CVAR_EUNSUPPORTED;
    if (d->act != CVAR_ACT_NONE && d->act != CVAR_ACT_GELU_TANH) return CVAR_EUNSUPPORTED;
    if (d->K % 128 || d->lda % 16 || d->ldw % 16 || d->lda < d->K || d->ldw < d->K) return CVAR_EUNSUPPORTED;
    if (((uintptr_t)d->A & 15) || ((uintptr_t)d->W & 15)) return CVAR_EINVAL;
    if (d->out_dtype != CVAR_BF16 && d->out_dtype != CVAR_F32) return CVAR_EUNSUPPORTED;
    if (d->residual && d->res_dtype != CVAR_BF16 && d->res_dtype != CVAR_F32) return CVAR_EUNSUPPORTED;
    if (d->gate && d->gate_rows <= 0) return CVAR_EINVAL;
    if (d->split_n < 0 || d->split_n >= d->N) return CVAR_EINVAL;
    if (d->split_n > 0) {
        if (!d->C_split || d->ld_split < d->split_n) return CVAR_EINVAL;
        if (d->remap_l <= 0 || d->residual || d->gate || d->act != CVAR_ACT_NONE) return CVAR_EUNSUPPORTED;
        if ((d->split_n & 7) || (d->N & 7) || (d->ld_split & 7) || (d->ldc & 7) || ((uintptr_t)d->C_split & 15) || ((uintptr_t)d->C & 15)) return CVAR_EUNSUPPORTED;
    }
    GemmParams p;
    p.M = d->M; p.N = d->N; p.K = d->K;
    p.A = (const char*)d->A; p.lda = d->lda; p.W = (const char*)d->W; p.ldw = d->ldw;
    p.strideA = p.strideW = p.strideC = p.strideR = 0;
    p.conv = 0; p.Hin = p.Win = p.Cin = p.Hout = p.Wout = p.stride = p.up = 0;
    p.alpha = d->alpha; p.bias = d->bias; p.act = d->act;
    p.gate = d->gate; p.ldg = d->ldg; p.gate_rows = d->gate_rows;
    p.residual = d->residual; p.res_dtype = d->res_dtype; p.ldr = d->ldr;
    p.C = d->C; p.out_dtype = d->out_dtype; p.ldc = d->ldc;
    p.C2 = nullptr; p.aux = nullptr; p.gate_scale = nullptr; p.in_dtype = CVAR_BF16;
    p.remap_l = d->remap_l; p.remap_L = d->remap_L; p.remap_off = d->remap_off;
    p.Cs = d->C_split; p.split_n = d->split_n; p.ld_split = d->ld_split; p.split_alpha = d->split_alpha == 0.0f ? 1.0f : d->split_alpha;
    p.tiles_m = p.tiles_n = 0;
    p.cv_adv = p.cv_rem = 0; p.conv_bytes = 0;
    make_fast_div(p.remap_l, &p.remap_magic, &p.remap_shift);
    make_fast_div(p.gate ? p.gate_rows : 1, &p.gate_magic, &p.gate_shift);
    p.split_tiles = 0; p.split_stride = 0;
    p.tile_cfg = 0; p.stagger = 0; p.group_m = 0; p.nt = 0;
    hipStream_t st = as_stream(stream);
    // the 256x256 tile where it fills the chip at all; the 128x128 tile for small M and narrow N (same bits: one accumulator chain per 16x16 block)
    if (d->M >= 1024 && d->N >= 256) return launch_fp8<256, 256, 2, 4>(p, a_scale, w_scale, st);
    return launch_fp8<128, 128, 2, 2>(p, a_scale, w_scale, st);
}
