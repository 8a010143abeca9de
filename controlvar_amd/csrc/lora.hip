// lora.hip - the rank-r adapter branch of LoRA fine-tuning (controlvar_amd/lora.py, DESIGN.md "LoRA").
//
// A target layer computes y = x W^T + b + s * (drop(x) A^T) B^T (peft's LoRA Linear, r <= 16).  The base GEMM and its fused
// epilogue stay in cvar_gemm: the rank-r term enters it through K-augmentation ([x | u] against [W | B]), so these kernels
// only produce and consume the skinny M x r tensors:
//   cvar_lora_down   u = s * drop(x) A^T           (forward; also du = dY B with p = 0, s = 1 in the backward)
//   cvar_lora_dx     dx = (dx + s * drop'(du A)) * gelu'(aux)      (in place after the base data-gradient GEMM)
//   cvar_lora_wgrad  G[n, j] = s * sum_m drop(Y)[m, n] Z[m, j]    (dB = dY^T u, dA = s du^T drop(x)), split-M fp32 partials +
//                    a fixed-order finish: no float atomics, bit-identical on every run
//   cvar_lora_down_rows  the per-row form of cvar_lora_down for inference (include/cvar_serve.h): every sequence of a batch picks its own
//                    adapter of a bank, no dropout; the other slots' columns of the K-augmented operand are written as zeros
// The dropout keep mask of (seed, tag, row, column) is a counter-based hash: forward and backward regenerate it, nothing is stored.
#include "cvar_common.h"
#include "../../include/cvar_accum.h"
#include "../../include/cvar_serve.h"

#define LORA_R 16           // rank held in registers; r < 16 leaves the upper accumulators unused

__host__ __device__ __forceinline__ uint32_t lora_mix(uint32_t h) {
    h ^= h >> 16; h *= 0x7feb352du;
    h ^= h >> 15; h *= 0x846ca68bu;
    h ^= h >> 16;
    return h;
}

static uint32_t lora_key(uint64_t seed, uint32_t tag) {
    uint32_t h = lora_mix((uint32_t)seed ^ 0x9e3779b9u);
    h = lora_mix(h ^ (uint32_t)(seed >> 32));
    return lora_mix(h ^ (tag * 0x85ebca6bu + 0x632be5abu));
}

__device__ __forceinline__ uint32_t lora_row_key(uint32_t key, uint32_t row) { return lora_mix(key ^ (row * 0xc2b2ae35u)); }
__device__ __forceinline__ bool lora_keep(uint32_t row_key, uint32_t col, uint32_t thresh) {
    return lora_mix(row_key + col * 0x9e3779b9u) >= thresh;
}

struct LoraMask {
    uint32_t key, thresh;
    float inv_keep;
    int on;
};

static LoraMask lora_mask(float p, uint64_t seed, uint32_t tag) {
    LoraMask mk;
    mk.key = lora_key(seed, tag);
    const double t = (double)p * 4294967296.0;
    mk.thresh = t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
    mk.inv_keep = p > 0.f ? 1.0f / (1.0f - p) : 1.0f;
    mk.on = p > 0.f;
    return mk;
}

// 8 consecutive elements <-> floats (16-byte aligned; the host checks pointers and leading dimensions)
__device__ __forceinline__ void ld8(const bf16_t* p, float* v) {
    const uint4 q = *(const uint4*)p;
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
__device__ __forceinline__ void ld8(const float* p, float* v) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void st8(bf16_t* p, const float* v) {
    const uint4 q = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
    *(uint4*)p = q;
}
__device__ __forceinline__ void st8(float* p, const float* v) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void copy8(const bf16_t* s, bf16_t* d) { *(uint4*)d = *(const uint4*)s; }
__device__ __forceinline__ void copy8(const float* s, float* d) { *(float4*)d = *(const float4*)s; *(float4*)(d + 4) = *(const float4*)(s + 4); }

template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> {
    uint4 q;
    __device__ __forceinline__ void load(const bf16_t* p) { q = *(const uint4*)p; }
    __device__ __forceinline__ void store(bf16_t* p) const { *(uint4*)p = q; }
    __device__ __forceinline__ void to(float* v) const {
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
};
template <> struct Raw8<float> {
    float4 a, b;
    __device__ __forceinline__ void load(const float* p) { a = *(const float4*)p; b = *(const float4*)(p + 4); }
    __device__ __forceinline__ void store(float* p) const { *(float4*)p = a; *(float4*)(p + 4) = b; }
    __device__ __forceinline__ void to(float* v) const { v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w; }
};

// ---- down projection ------------------------------------------------------------------------------------------------
// block = 4 waves x ROWS rows; per 512-column slab the block stages A[0:r][slab] in LDS once (instead of every wave reading it from
// L2 per row group), lane owns 8 columns of the slab and accumulates ROWS x 16 partial dot products, which one transposing butterfly
// (63 shuffles for 64 values) reduces so that lane l ends with (row l / 16, rank column l % 16)
// The body is shared by lora_down_kernel and lora_down_rows_kernel (one text, so a row of either is the same sum): the wave's rows are
// m0 .. m0 + ROWS - 1, those at or past m_end are skipped; returns the lane's reduced value, unscaled
template <typename T, int ROWS>
__device__ __forceinline__ float lora_down_body(const T* __restrict__ x, long ldx, const T* __restrict__ A, long lda, T* __restrict__ xc, long ldxc,
                                                T (*As)[512], const long m0, const long M, int K, int r, const LoraMask& mk) {
    static_assert(ROWS * LORA_R == 64, "one reduced value per lane");
    const int lane = threadIdx.x & 63;
    float acc[ROWS * LORA_R];
#pragma unroll
    for (int i = 0; i < ROWS * LORA_R; ++i) acc[i] = 0.f;
    uint32_t rk[ROWS];
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr) rk[rr] = lora_row_key(mk.key, (uint32_t)(m0 + rr));
    Raw8<T> nx[ROWS];                                   // the next slab's rows, loaded while the current one is computed
#pragma unroll
    for (int rr = 0; rr < ROWS; ++rr)
        if (m0 + rr < M && lane * 8 < K) nx[rr].load(x + (m0 + rr) * ldx + lane * 8);
    for (int kb = 0; kb < K; kb += 512) {
        Raw8<T> cur[ROWS];
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) cur[rr] = nx[rr];
        __syncthreads();
        for (int c = threadIdx.x; c < LORA_R * 64; c += 256) {
            const int j = c >> 6, kk = (c & 63) * 8;
            if (j < r && kb + kk < K) copy8(A + (long)j * lda + kb + kk, &As[j][kk]);
        }
        const int k0 = kb + lane * 8;
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr)
            if (m0 + rr < M && k0 + 512 < K) nx[rr].load(x + (m0 + rr) * ldx + k0 + 512);
        __syncthreads();
        if (k0 >= K) continue;
        float xv[ROWS][8];
#pragma unroll
        for (int rr = 0; rr < ROWS; ++rr) {
            const long m = m0 + rr;
            if (m < M) {
                cur[rr].to(xv[rr]);
                if (xc) cur[rr].store(xc + m * ldxc + k0);
                if (mk.on) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) xv[rr][e] *= lora_keep(rk[rr], (uint32_t)(k0 + e), mk.thresh) ? mk.inv_keep : 0.f;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) xv[rr][e] = 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < LORA_R; ++j) {
            if (j < r) {
                float a[8];
                ld8(&As[j][lane * 8], a);
#pragma unroll
                for (int rr = 0; rr < ROWS; ++rr)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[rr * LORA_R + j] = fmaf(xv[rr][e], a[e], acc[rr * LORA_R + j]);
            }
        }
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const bool hi = (lane & w) != 0;
#pragma unroll
        for (int i = 0; i < w; ++i) {
            const float send = hi ? acc[i] : acc[i + w];
            const float keep = hi ? acc[i + w] : acc[i];
            acc[i] = keep + __shfl_xor(send, w, 64);
        }
    }
    return acc[0];
}

template <typename T, int ROWS>
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ A, long lda, T* __restrict__ u,
                                                        long ldu, T* __restrict__ xc, long ldxc, int M, int K, int r, float scale, LoraMask mk) {
    __shared__ __attribute__((aligned(16))) T As[LORA_R][512];
    const int lane = threadIdx.x & 63;
    const long m0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;        // no early exit: every wave joins the slab barriers
    const float v = lora_down_body<T, ROWS>(x, ldx, A, lda, xc, ldxc, As, m0, (long)M, K, r, mk);
    const long m = m0 + lane / LORA_R;
    const int j = lane % LORA_R;
    if (m < M && j < r) Elem<T>::st(u + m * ldu + j, scale * v);
}

// ---- per-row adapters (inference; include/cvar_serve.h) -------------------------------------------------------------------
// block = (sequence, 16-row chunk of its l rows): the slot is block-uniform and read once, ahead of everything else, so a block never
// stages an A slab for rows of another adapter.  The reduction is lora_down_body with r = 16 and no dropout; the wave then writes its
// rows' kpad columns behind K: the slot's 16 values, zeros in every other 8-column group.  A slot < 0 block copies and zero-fills
// without touching the bank.
template <typename T>
__global__ __launch_bounds__(256) void lora_down_rows_kernel(const T* __restrict__ x, long ldx, const T* __restrict__ bank, long lda,
                                                             const float* __restrict__ scale, const int* __restrict__ slot, int l, int chunks,
                                                             T* __restrict__ xa, long ldxa, int kpad, T* __restrict__ xc, long ldxc, int K) {
    __shared__ __attribute__((aligned(16))) T As[LORA_R][512];
    const int seq = blockIdx.x / chunks;
    const int s = slot[seq];
    const int lane = threadIdx.x & 63;
    const long m_end = ((long)seq + 1) * l;
    const long m0 = (long)seq * l + ((long)(blockIdx.x % chunks) * 4 + (threadIdx.x >> 6)) * 4;
    if (s >= 0) {
        LoraMask mk;
        mk.key = 0; mk.thresh = 0; mk.inv_keep = 1.f; mk.on = 0;
        const float v = lora_down_body<T, 4>(x, ldx, bank + (long)s * LORA_R * lda, lda, xc, ldxc, As, m0, m_end, K, LORA_R, mk);
        const long m = m0 + lane / LORA_R;
        if (m < m_end) Elem<T>::st(xa + m * ldxa + K + s * LORA_R + lane % LORA_R, scale[s] * v);
    } else if (xc) {
        for (int rr = 0; rr < 4; ++rr)
            if (m0 + rr < m_end)
                for (int k0 = lane * 8; k0 < K; k0 += 512) copy8(x + (m0 + rr) * ldx + k0, xc + (m0 + rr) * ldxc + k0);
    }
    const int g8 = kpad >> 3;                               // 8-column groups per row; groups 2 s and 2 s + 1 hold the slot's values
    float z[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0.f;
    for (int c = lane; c < 4 * g8; c += 64) {
        const int rr = c / g8, g = c % g8;
        if (m0 + rr < m_end && (s < 0 || (g >> 1) != s)) st8(xa + (m0 + rr) * ldxa + K + g * 8, z);
    }
}

// ---- data gradient of the adapter branch (in place) ----------------------------------------------------------------------
// thread = 8 columns x DX_ROWS rows; A's 16 x 8 slice stays in registers across the rows, the next row's operands are loaded
// before the current one is finished (one row in flight per thread)
#define DX_ROWS 16
template <typename T, typename TD>
struct DxRow {
    float v[8], g[8], d[LORA_R];
    __device__ __forceinline__ void load(const TD* dx, long lddx, const T* du, long lddu, const T* aux, long ldaux, int m, int k0, int r) {
        ld8(dx + (long)m * lddx + k0, v);
        if (aux) ld8(aux + (long)m * ldaux + k0, g);
        ld8(du + (long)m * lddu, d);                        // du rows: 16 elements, 16-byte aligned (host-checked)
        ld8(du + (long)m * lddu + 8, d + 8);
#pragma unroll
        for (int j = 0; j < LORA_R; ++j) d[j] = j < r ? d[j] : 0.f;           // columns >= r are not written by anyone
    }
};

template <typename T, typename TD>
__global__ __launch_bounds__(256) void lora_dx_kernel(TD* __restrict__ dx, long lddx, const T* __restrict__ du, long lddu, const T* __restrict__ A,
                                                      long lda, const T* __restrict__ aux, long ldaux, int M, int K, int r, float scale, LoraMask mk) {
    const int k0 = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (k0 >= K) return;
    float a[LORA_R][8];
#pragma unroll
    for (int j = 0; j < LORA_R; ++j) {
        if (j < r) ld8(A + (long)j * lda + k0, a[j]);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) a[j][e] = 0.f;
        }
    }
    const int mb = blockIdx.y * DX_ROWS, me = min(M, mb + DX_ROWS);
    DxRow<T, TD> cur, nxt;
    cur.load(dx, lddx, du, lddu, aux, ldaux, mb, k0, r);
    for (int m = mb; m < me; ++m) {
        if (m + 1 < me) nxt.load(dx, lddx, du, lddu, aux, ldaux, m + 1, k0, r);
        float s8[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) s8[e] = 0.f;
#pragma unroll
        for (int j = 0; j < LORA_R; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) s8[e] = fmaf(cur.d[j], a[j][e], s8[e]);
        const uint32_t rk = lora_row_key(mk.key, (uint32_t)m);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float keep = mk.on ? (lora_keep(rk, (uint32_t)(k0 + e), mk.thresh) ? mk.inv_keep : 0.f) : 1.f;
            o[e] = cur.v[e] + scale * keep * s8[e];
            if (aux) o[e] *= gelu_tanh_grad(cur.g[e]);
        }
        st8(dx + (long)m * lddx + k0, o);
        cur = nxt;
    }
}

// ---- skinny weight gradients -----------------------------------------------------------------------------------------------
// block = 512 columns of Y (2 per thread, one 4- / 8-byte load per row) x one M slice; Z rows of the slice are staged in LDS 64 at a
// time and read as broadcasts
#define WG_MCHUNK 64
#define WG_COLS 2
#define WG_UNROLL 4
__device__ __forceinline__ void ld2(const bf16_t* p, float* v) {
    const unsigned q = *(const unsigned*)p;
    v[0] = __uint_as_float(q << 16); v[1] = __uint_as_float(q & 0xffff0000u);
}
__device__ __forceinline__ void ld2(const float* p, float* v) {
    const float2 a = *(const float2*)p;
    v[0] = a.x; v[1] = a.y;
}

template <typename T>
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const T* __restrict__ Y, long ldy, const T* __restrict__ Z, long ldz, int M, int N, int r,
                                                         int rows_per_split, LoraMask mk, float* __restrict__ ws) {
    __shared__ float zs[WG_MCHUNK][LORA_R];
    const int n0 = (blockIdx.x * 256 + threadIdx.x) * WG_COLS;
    const int s = blockIdx.y;
    const int mb = s * rows_per_split, me = min(M, mb + rows_per_split);
    float acc[WG_COLS][LORA_R];
#pragma unroll
    for (int c = 0; c < WG_COLS; ++c)
#pragma unroll
        for (int j = 0; j < LORA_R; ++j) acc[c][j] = 0.f;
    for (int mc = mb; mc < me; mc += WG_MCHUNK) {
        __syncthreads();
        for (int i = threadIdx.x; i < WG_MCHUNK * LORA_R; i += 256) {
            const int mm = i / LORA_R, j = i % LORA_R;
            const int m = mc + mm;
            zs[mm][j] = (m < me && j < r) ? Elem<T>::ld(Z + (long)m * ldz + j) : 0.f;
        }
        __syncthreads();
        if (n0 < N) {
            const int cnt = min(WG_MCHUNK, me - mc);
            for (int mm = 0; mm < cnt; mm += WG_UNROLL) {         // WG_UNROLL independent row loads in flight; Z rows past the slice are zero
                float y[WG_UNROLL][WG_COLS];
#pragma unroll
                for (int u = 0; u < WG_UNROLL; ++u) {
                    if (mm + u < cnt) ld2(Y + (long)(mc + mm + u) * ldy + n0, y[u]);
                    else y[u][0] = y[u][1] = 0.f;
                }
#pragma unroll
                for (int u = 0; u < WG_UNROLL; ++u) {
                    if (mk.on) {
                        const uint32_t rk = lora_row_key(mk.key, (uint32_t)(mc + mm + u));
#pragma unroll
                        for (int c = 0; c < WG_COLS; ++c) y[u][c] *= lora_keep(rk, (uint32_t)(n0 + c), mk.thresh) ? mk.inv_keep : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < LORA_R; ++j) {
                        const float z = zs[mm + u][j];
#pragma unroll
                        for (int c = 0; c < WG_COLS; ++c) acc[c][j] = fmaf(y[u][c], z, acc[c][j]);
                    }
                }
            }
        }
    }
    if (n0 < N) {
#pragma unroll
        for (int c = 0; c < WG_COLS; ++c)
#pragma unroll
            for (int j = 0; j < LORA_R; ++j) ws[((long)s * N + n0 + c) * LORA_R + j] = acc[c][j];
    }
}

// block = 64 outputs x 4 split groups: group g sums the splits g, g + 4, ... in order, the four group sums are added in a fixed order
// ACC (cvar_lora_wgrad_acc, gradient accumulation): the old output is added last - fp32(old + plain)
template <bool ACC>
__global__ __launch_bounds__(256) void lora_wgrad_finish_kernel(const float* __restrict__ ws, int nsplit, int N, int r, float scale, float* __restrict__ out,
                                                                long os_n, long os_j) {
    __shared__ float part[4][64];
    const int g = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * 64 + (threadIdx.x & 63);
    const bool live = i < (long)N * LORA_R;
    float acc = 0.f;
    if (live)
        for (int s = g; s < nsplit; s += 4) acc += ws[(long)s * N * LORA_R + i];
    part[g][threadIdx.x & 63] = acc;
    __syncthreads();
    if (g != 0 || !live) return;
    const int n = (int)(i / LORA_R), j = (int)(i % LORA_R);
    if (j >= r) return;
    const int t = threadIdx.x;
    const float v = scale * (((part[0][t] + part[1][t]) + part[2][t]) + part[3][t]);
    out[n * os_n + j * os_j] = ACC ? out[n * os_n + j * os_j] + v : v;
}

__global__ __launch_bounds__(256) void lora_mask_kernel(float* __restrict__ out, int M, int K, LoraMask mk) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)M * K) return;
    const int m = (int)(i / K), k = (int)(i % K);
    out[i] = (!mk.on || lora_keep(lora_row_key(mk.key, (uint32_t)m), (uint32_t)k, mk.thresh)) ? 1.f : 0.f;
}

// ---- C ABI -----------------------------------------------------------------------------------------------------------------
static bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static void wgrad_plan(int M, int N, int* nsplit, int* rows_per_split) {
    const int nbn = cdiv(N, 256 * WG_COLS);
    int ns = max(1, min(cdiv(1024, nbn), cdiv(M, WG_MCHUNK)));
    const int rps = cdiv(cdiv(M, ns), WG_MCHUNK) * WG_MCHUNK;
    *rows_per_split = rps;
    *nsplit = cdiv(M, rps);
}

extern "C" int64_t cvar_lora_wgrad_ws_floats(int M, int N) {
    if (M <= 0 || N <= 0) return 0;
    int ns, rps;
    wgrad_plan(M, N, &ns, &rps);
    return (int64_t)ns * N * LORA_R;
}

extern "C" int cvar_lora_down(const void* x, int64_t ldx, const void* A, int64_t lda, void* u, int64_t ldu, void* x_copy, int64_t ld_copy, int M, int K,
                              int r, int dtype, float scale, float p, uint64_t seed, uint32_t tag, void* stream) {
    if (!x || !A || !u || M <= 0 || K <= 0 || r <= 0) return CVAR_EINVAL;
    if (r > LORA_R || K % 8 || ldx % 8 || lda % 8 || ldx < K || lda < K || ldu < r || !al16(x) || !al16(A)) return CVAR_EUNSUPPORTED;
    if (x_copy && (ld_copy % 8 || ld_copy < K || !al16(x_copy))) return CVAR_EUNSUPPORTED;
    if (p < 0.f || p >= 1.f) return CVAR_EINVAL;
    const LoraMask mk = lora_mask(p, seed, tag);
    const dim3 grid(cdiv(M, 16)), block(256);
    if (dtype == CVAR_BF16)
        hipLaunchKernelGGL((lora_down_kernel<bf16_t, 4>), grid, block, 0, as_stream(stream), (const bf16_t*)x, (long)ldx, (const bf16_t*)A, (long)lda,
                           (bf16_t*)u, (long)ldu, (bf16_t*)x_copy, (long)ld_copy, M, K, r, scale, mk);
    else if (dtype == CVAR_F32)
        hipLaunchKernelGGL((lora_down_kernel<float, 4>), grid, block, 0, as_stream(stream), (const float*)x, (long)ldx, (const float*)A, (long)lda,
                           (float*)u, (long)ldu, (float*)x_copy, (long)ld_copy, M, K, r, scale, mk);
    else return CVAR_EUNSUPPORTED;
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_lora_down_rows(const void* x, int64_t ldx, const void* A_bank, int64_t lda, const float* scale, const int32_t* slot, int n_slots,
                                   int R, int l, void* xa, int64_t ldxa, int kpad, void* x_copy, int64_t ld_copy, int K, int dtype, void* stream) {
    if (!x || !A_bank || !scale || !slot || !xa || R <= 0 || l < 1 || K <= 0 || n_slots < 1 || n_slots > 8) return CVAR_EINVAL;
    if (kpad % 16 || kpad < 16 * n_slots) return CVAR_EINVAL;
    if (K % 8 || ldx % 8 || lda % 8 || ldxa % 8 || ldx < K || lda < K || ldxa < (int64_t)K + kpad || !al16(x) || !al16(A_bank) || !al16(xa))
        return CVAR_EUNSUPPORTED;
    if (x_copy && (ld_copy % 8 || ld_copy < K || !al16(x_copy))) return CVAR_EUNSUPPORTED;
    const int chunks = cdiv(l, 16);
    if ((int64_t)R * l > 0x7fffffff || (int64_t)R * chunks > 0x7fffffff) return CVAR_EUNSUPPORTED;
    const dim3 grid(R * chunks), block(256);
    if (dtype == CVAR_BF16)
        hipLaunchKernelGGL((lora_down_rows_kernel<bf16_t>), grid, block, 0, as_stream(stream), (const bf16_t*)x, (long)ldx, (const bf16_t*)A_bank, (long)lda,
                           scale, (const int*)slot, l, chunks, (bf16_t*)xa, (long)ldxa, kpad, (bf16_t*)x_copy, (long)ld_copy, K);
    else if (dtype == CVAR_F32)
        hipLaunchKernelGGL((lora_down_rows_kernel<float>), grid, block, 0, as_stream(stream), (const float*)x, (long)ldx, (const float*)A_bank, (long)lda,
                           scale, (const int*)slot, l, chunks, (float*)xa, (long)ldxa, kpad, (float*)x_copy, (long)ld_copy, K);
    else return CVAR_EUNSUPPORTED;
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_lora_dx(void* dx, int64_t lddx, int dx_dtype, const void* du, int64_t lddu, const void* A, int64_t lda, const void* aux, int64_t ldaux,
                            int M, int K, int r, int dtype, float scale, float p, uint64_t seed, uint32_t tag, void* stream) {
    if (!dx || !du || !A || M <= 0 || K <= 0 || r <= 0) return CVAR_EINVAL;
    if (r > LORA_R || K % 8 || lddx % 8 || lda % 8 || lddx < K || lda < K || lddu < LORA_R || lddu % 8 || !al16(dx) || !al16(A) || !al16(du))
        return CVAR_EUNSUPPORTED;
    if (aux && (ldaux % 8 || ldaux < K || !al16(aux))) return CVAR_EUNSUPPORTED;
    if (p < 0.f || p >= 1.f) return CVAR_EINVAL;
    const LoraMask mk = lora_mask(p, seed, tag);
    const dim3 grid(cdiv(K, 2048), cdiv(M, DX_ROWS)), block(256);
    hipStream_t st = as_stream(stream);
    if (dtype == CVAR_BF16 && dx_dtype == CVAR_BF16)
        hipLaunchKernelGGL((lora_dx_kernel<bf16_t, bf16_t>), grid, block, 0, st, (bf16_t*)dx, (long)lddx, (const bf16_t*)du, (long)lddu, (const bf16_t*)A,
                           (long)lda, (const bf16_t*)aux, (long)ldaux, M, K, r, scale, mk);
    else if (dtype == CVAR_BF16 && dx_dtype == CVAR_F32)
        hipLaunchKernelGGL((lora_dx_kernel<bf16_t, float>), grid, block, 0, st, (float*)dx, (long)lddx, (const bf16_t*)du, (long)lddu, (const bf16_t*)A,
                           (long)lda, (const bf16_t*)aux, (long)ldaux, M, K, r, scale, mk);
    else if (dtype == CVAR_F32 && dx_dtype == CVAR_F32)
        hipLaunchKernelGGL((lora_dx_kernel<float, float>), grid, block, 0, st, (float*)dx, (long)lddx, (const float*)du, (long)lddu, (const float*)A,
                           (long)lda, (const float*)aux, (long)ldaux, M, K, r, scale, mk);
    else return CVAR_EUNSUPPORTED;
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

static int lora_wgrad_run(const void* Y, int64_t ldy, const void* Z, int64_t ldz, int M, int N, int r, int dtype, float scale, float p, uint64_t seed,
                          uint32_t tag, float* ws, int64_t ws_floats, float* out, int64_t os_n, int64_t os_j, bool accumulate, void* stream) {
    if (!Y || !Z || !ws || !out || M <= 0 || N <= 0 || r <= 0) return CVAR_EINVAL;
    if (r > LORA_R || ldy < N || ldz < r || N % WG_COLS || ldy % WG_COLS || ((uintptr_t)Y & (WG_COLS * (dtype == CVAR_BF16 ? 2 : 4) - 1)))
        return CVAR_EUNSUPPORTED;
    if (p < 0.f || p >= 1.f) return CVAR_EINVAL;
    if (ws_floats < cvar_lora_wgrad_ws_floats(M, N)) return CVAR_EINVAL;
    int ns, rps;
    wgrad_plan(M, N, &ns, &rps);
    const LoraMask mk = lora_mask(p, seed, tag);
    hipStream_t st = as_stream(stream);
    const dim3 grid(cdiv(N, 256 * WG_COLS), ns), block(256);
    if (dtype == CVAR_BF16)
        hipLaunchKernelGGL((lora_wgrad_kernel<bf16_t>), grid, block, 0, st, (const bf16_t*)Y, (long)ldy, (const bf16_t*)Z, (long)ldz, M, N, r, rps, mk, ws);
    else if (dtype == CVAR_F32)
        hipLaunchKernelGGL((lora_wgrad_kernel<float>), grid, block, 0, st, (const float*)Y, (long)ldy, (const float*)Z, (long)ldz, M, N, r, rps, mk, ws);
    else return CVAR_EUNSUPPORTED;
    CVAR_CHECK_LAUNCH();
    const dim3 fgrid(cdiv((int64_t)N * LORA_R, 64));
    if (accumulate) hipLaunchKernelGGL(lora_wgrad_finish_kernel<true>, fgrid, block, 0, st, ws, ns, N, r, scale, out, (long)os_n, (long)os_j);
    else hipLaunchKernelGGL(lora_wgrad_finish_kernel<false>, fgrid, block, 0, st, ws, ns, N, r, scale, out, (long)os_n, (long)os_j);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}

extern "C" int cvar_lora_wgrad(const void* Y, int64_t ldy, const void* Z, int64_t ldz, int M, int N, int r, int dtype, float scale, float p, uint64_t seed,
                               uint32_t tag, float* ws, int64_t ws_floats, float* out, int64_t os_n, int64_t os_j, void* stream) {
    return lora_wgrad_run(Y, ldy, Z, ldz, M, N, r, dtype, scale, p, seed, tag, ws, ws_floats, out, os_n, os_j, false, stream);
}

extern "C" int cvar_lora_wgrad_acc(const void* Y, int64_t ldy, const void* Z, int64_t ldz, int M, int N, int r, int dtype, float scale, float p, uint64_t seed,
                                   uint32_t tag, float* ws, int64_t ws_floats, float* out, int64_t os_n, int64_t os_j, int accumulate, void* stream) {
    return lora_wgrad_run(Y, ldy, Z, ldz, M, N, r, dtype, scale, p, seed, tag, ws, ws_floats, out, os_n, os_j, accumulate != 0, stream);
}

extern "C" int cvar_lora_dropout_mask(float* out, int M, int K, float p, uint64_t seed, uint32_t tag, void* stream) {
    if (!out || M <= 0 || K <= 0) return CVAR_EINVAL;
    if (p < 0.f || p >= 1.f) return CVAR_EINVAL;
    const LoraMask mk = lora_mask(p, seed, tag);
    hipLaunchKernelGGL(lora_mask_kernel, dim3(cdiv((int64_t)M * K, 256)), dim3(256), 0, as_stream(stream), out, M, K, mk);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}
