// kv_precision='fp8' (include/cvar_kvcache.h): the append pass of the e4m3 K/V arena for gfx950 (MI355X).  The attention kernel that reads the
// arena is the KV8 instantiation of attn_mfma_bf16_kernel (attn.hip).
#include "cvar_common.h"
#include "fp8_quant.h"
#include "../../include/cvar_kvcache.h"

// One head vector (64 bf16 = 128 bytes) per 8 lanes: one 16-byte load per lane, the amax over the 8 lanes by three shuffles, one 8-byte store per
// lane and one scale per vector.  Vector v of the pass is columns [64 j, 64 j + 64) of scratch row v / 2H (j = v % 2H: the k heads, then the v heads),
// so the scratch is read front to back; its arena row is (r, q_off + t).  A bandwidth-trivial pass: 128 bytes in, 68 out per vector.
__global__ __launch_bounds__(256) void kv_append_fp8_kernel(const bf16_t* __restrict__ kv, unsigned char* __restrict__ kv8, float* __restrict__ kv_scale,
                                                            long nvec, int H2, int Lmax, int q_off, int l) {
    const long v = (long)blockIdx.x * 32 + (threadIdx.x >> 3);
    if (v >= nvec) return;                              // whole 8-lane groups leave together
    const int sub = threadIdx.x & 7;
    const bf16x8_t in = *(const bf16x8_t*)(kv + v * 64 + sub * 8);
    float x[8];
    unsigned ab = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) { x[e] = bf16_to_f32((bf16_t)in[e]); ab = max(ab, fp8_abs_bits(x[e])); }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) ab = max(ab, (unsigned)__shfl_xor((int)ab, o, 64));
    const bool bad = ab >= 0x7f800000u;
    const int k = fp8_row_exp(ab);
    const float inv = fp8_pow2(-k);
    const long row = v / H2;                            // r * l + t
    const int j = (int)(v - row * H2);
    const long arow = (row / l) * Lmax + q_off + row % l;
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
    u32x2_t w;
    w[0] = bad ? 0x7f7f7f7fu : fp8_pack4(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
    w[1] = bad ? 0x7f7f7f7fu : fp8_pack4(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv);
    *(u32x2_t*)(kv8 + (arow * H2 + j) * 64 + sub * 8) = w;
    if (sub == 0) kv_scale[arow * H2 + j] = bad ? 1.0f : fp8_pow2(k);
}

extern "C" int cvar_kv_append_fp8(const void* kv, void* kv8, float* kv_scale, int R, int H, int Lmax, int q_off, int l, void* stream) {
    if (!kv || !kv8 || !kv_scale || R <= 0 || H <= 0 || l <= 0 || q_off < 0 || q_off + l > Lmax) return CVAR_EINVAL;
    if (((uintptr_t)kv & 15) || ((uintptr_t)kv8 & 7) || ((uintptr_t)kv_scale & 3)) return CVAR_EINVAL;
    const long nvec = (long)R * l * 2 * H;
    const long blocks = (nvec + 31) / 32;
    if (blocks > 0x7fffffffL) return CVAR_EUNSUPPORTED;
    hipLaunchKernelGGL(kv_append_fp8_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), (const bf16_t*)kv, (unsigned char*)kv8, kv_scale,
                       nvec, 2 * H, Lmax, q_off, l);
    CVAR_CHECK_LAUNCH();
    return CVAR_OK;
}
