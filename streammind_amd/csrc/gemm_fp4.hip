// MXFP4 (OCP MX v1.0: e2m1 elements, one e8m0 scale per 32 consecutive k of an output row) LLM weights: quantiser / packer,
// unpacker, the bf16 expansion for calls with more than 16 rows, the <= 16-row weight-streaming kernel on the CDNA4
// block-scaled matrix instruction (v_mfma_scale_f32_16x16x128_f8f6f4, A = e2m1 via cbsz 4, B = e4m3), -- SM_W_FP4_MFMA -- the
// 17..128-row weight stream on the same instruction with the activations requantised once per call, and -- SM_W_FP4_GEMM -- the
// tiled GEMM for more than 128 rows on the same prepass (both at the end of the file).
//
// Image (common.h, "MXFP4 packed layout"): per 16-row group one contiguous stream of KS = ceil(K / 128) code chunks of 1 KiB
// -- lane (g, i) of chunk ks holds the 32 codes of W[rg*16 + i][ks*128 + g*32 .. +31], i.e. ONE MX block, 16 bytes, which is
// exactly that lane's A operand of one MFMA -- followed by ceil(KS / 4) scale chunks of 256 B: lane (g, i)'s dword of scale
// chunk q holds the e8m0 bytes of ITS blocks of code chunks 4q .. 4q+3 (byte h = chunk 4q + h), so the lane that feeds
// scale_a receives the byte with one 4-byte load per four 16-byte loads.  4.25 bits per weight.
// The instruction's operand map, measured with one-hot operands: an e2m1 operand (four registers) holds k = 32g .. 32g+31 of its
// row in lane (g, i), in order; an e4m3 operand (eight registers) holds k = 16g .. 16g+15 in its first sixteen bytes and
// k = 64 + 16g .. 64 + 16g+15 in the other sixteen; either way the scale operand of lane (G, i) applies to k = 32G .. 32G+31.
// The weight image follows the first map, the requantised activations in LDS the second.
//
// The <= 16-row kernel.  Grid (row groups, K slices); a block owns one 16-row group and `qps` quads (a quad = four k-steps of
// 128 = one scale dword) of K; its waves take the quads round robin and keep a register ring of D = 2 quads (8.25 KiB per wave
// and matrix) in flight: all loads of a quad are issued before any is consumed, a consumed slot is refilled at once.  The
// codes go from HBM into the matrix pipe as they are -- no conversion instruction on the hot path.
//   The activations are the B operand.  Before the weight stream is consumed the block requantises its x rows (fp32 or
// 16-bit, optionally RMS-normalised: norm_gamma) ONCE into LDS: every 32-block of a row becomes an e4m3 "hi" term with its own
// e8m0 scale (block maximum scaled into [128, 256): no saturation) plus an e4m3 "lo" term, the RNE-rounded residual x - hi
// with a scale of its own.  hi is round-to-nearest, so |x - hi| <= 2^-4 of x's binade and the signed residual carries four
// more bits below that: |x - hi - lo| <= 2^-9 of the binade -- bf16's own rounding bound is 2^-8.  The mode is weight-only
// in effect (unlike SM_W_FP8_MFMA, which rounds activations to e4m3).  Two MFMAs per weight fragment (hi, lo; four with the
// SwiGLU dual image); matrix time stays far below the fragment's HBM time at these row counts.  The first x block of every
// thread is fetched BEFORE the first weight loads (vmcnt retires in order), quantised while they fly; the barriers are raw
// s_barriers (__syncthreads would drain the weight loads).
//   LDS: 264 B per (k-step, row) of x (128 hi + 128 lo + 4 x 2 scale bytes), 44 KiB at most.  One row of K = 14336 needs
// 29 KiB; where M x K does not fit (>= 6 rows at K = 4096) K is cut over blockIdx.y, the slices leave raw fp32 partial sums
// in the split-K slabs and the shared slab-sum pass applies the epilogue (fixed slab order: deterministic).  The partial sums
// of the waves of a block meet in LDS in wave order.
//   Epilogue: store4 of linear_common.h (bias, act, fp32 residual, fp32 and / or 16-bit output, SwiGLU of the dual image).
//   Measured (tools/decode_bench.py --fp4, Mistral-7B shapes, batch 1, one run on one box): 539.6 tokens/s against 523.4 on fp8 and 348.0
// on bf16 weights -- 3 % faster than fp8, not the factor the bytes suggest.  The time is inside this kernel (1.81 of 1.85 ms per token in
// the weight-streaming launches), which streams at 1.1 TB/s (q|k|v, o) to 2.8 TB/s (down) on its own bytes: it is the bound, not HBM.
// Suspected, not yet traced: the x requantisation every block does before its first MFMA, the norm statistics' round trip, one block
// per CU at N = 4096.  More than a few rows are not tuned -- a 16-stream batched decode step takes 5.7 ms against 3.0 ms on fp8 (one-wave
// blocks, every block requantising all rows): DESIGN.md, "MXFP4 weights".  The memory saving -- 3.8 GB instead of 14.2 GB of LLM
// linears -- stands either way.
#include <algorithm>
#include <map>
#include <mutex>
#include <type_traits>

#include "linear_common.h"

typedef __attribute__((ext_vector_type(8))) int i32x8;

// ------------------------------------------------------------------------------------------------ quantiser / packer
// one thread = one lane slot of one code chunk = one MX block of 32 (zeros beyond N / K)
__global__ void quant_pack_fp4_kernel(const bf16_t* __restrict__ w, int N, int K, int ldw, char* __restrict__ out, int KS, size_t total) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= total) return;
    const int lane = (int)(c & 63);
    const size_t rest = c >> 6;
    const int ks = (int)(rest % KS), rg = (int)(rest / KS);
    const int n = rg * 16 + (lane & 15), k0 = ks * 128 + (lane >> 4) * 32;
    float v[32];
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        v[j] = (n < N && k0 + j < K) ? bf2f(w[(size_t)n * ldw + k0 + j]) : 0.f;
        am = fmaxf(am, fabsf(v[j]));
    }
    // X = 2^(floor(log2 max|w|) - 2), as the e8m0 byte; all-zero block: 127
    int e = am > 0.f ? ilogbf(am) - 2 + 127 : 127;
    e = e < 0 ? 0 : (e > 254 ? 254 : e);
    uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 32; ++j) {
        const float s = ldexpf(v[j], 127 - e);                        // w / X, exact
        const float t = fabsf(s);
        // RNE onto {0, 0.5, 1, 1.5, 2, 3, 4, 6}: the grid's step is 0.5 below 2, 1 below 4, 2 above; ties go to the even code
        float q = t < 2.f ? rintf(t * 2.f) * 0.5f : t < 4.f ? rintf(t) : rintf(t * 0.5f) * 2.f;
        q = fminf(q, 6.f);                                            // saturate
        uint32_t code = q < 2.f ? (uint32_t)(q * 2.f) : q < 4.f ? (uint32_t)q + 2u : (uint32_t)(q * 0.5f) + 4u;
        if (s < 0.f && code) code |= 8u;
        o[j >> 3] |= code << ((j & 7) * 4);                           // element 2b in the low nibble of byte b
    }
    char* rgp = out + (size_t)rg * fp4_rg_bytes(KS);
    *(u32x4*)(rgp + (size_t)ks * 1024 + lane * 16) = u32x4{o[0], o[1], o[2], o[3]};
    uint8_t* sp = (uint8_t*)(rgp + (size_t)KS * 1024 + (size_t)(ks >> 2) * 256 + lane * 4);
    sp[ks & 3] = (uint8_t)e;
    if (ks == KS - 1)
        for (int h = (ks & 3) + 1; h < 4; ++h) sp[h] = 127;           // the padding of the last scale dword
}

extern "C" size_t sm_packed_fp4_bytes(int N, int K) {
    return (size_t)((N + 15) / 16) * fp4_rg_bytes((K + 127) / 128);
}

extern "C" int sm_quant_pack_weight_fp4(const void* w, int N, int K, int ldw, void* out, void* stream) {
    SM_REQUIRE(w && out && N > 0 && K > 0 && ldw >= K, "sm_quant_pack_weight_fp4: bad args N=%d K=%d ldw=%d", N, K, ldw);
    const int KS = (K + 127) / 128;
    const size_t total = (size_t)((N + 15) / 16) * KS * 64;
    quant_pack_fp4_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)w, N, K, ldw, (char*)out, KS, total);
    SM_LAUNCH_CHECK();
    return SM_OK;
}

// code (4 bits) x 2^(e - 127) as fp32: exact, and exact in bf16 too (two significant bits)
__device__ __forceinline__ float fp4_value(uint32_t code, float scale) {
    const uint32_t m = code & 1u, ex = (code >> 1) & 3u;
    const float a = ex ? __uint_as_float(((126u + ex) << 23) | (m << 22)) : 0.5f * (float)m;
    return (code & 8u) ? -a * scale : a * scale;
}
__device__ __forceinline__ float e8m0_value(uint32_t e) { return __uint_as_float(e ? e << 23 : 0x00400000u); }

// PACKED = false: row-major bf16 [N][ldo]; PACKED = true: the packed bf16 image of common.h with KS32 = ceil(K / 32) k-steps
// (what calls with more than 16 rows multiply with).  One thread = one MX block.
template <bool PACKED>
__global__ void unpack_fp4_kernel(const char* __restrict__ in, int N, int K, int KS, bf16_t* __restrict__ out, int ldo, size_t total) {
    const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= total) return;
    const int lane = (int)(c & 63);
    const size_t rest = c >> 6;
    const int ks = (int)(rest % KS), rg = (int)(rest / KS);
    const int i = lane & 15, g = lane >> 4;
    const char* rgp = in + (size_t)rg * fp4_rg_bytes(KS);
    const u32x4 q = *(const u32x4*)(rgp + (size_t)ks * 1024 + lane * 16);
    const uint32_t sd = *(const uint32_t*)(rgp + (size_t)KS * 1024 + (size_t)(ks >> 2) * 256 + lane * 4);
    const float sc = e8m0_value((sd >> ((ks & 3) * 8)) & 0xffu);
    if constexpr (PACKED) {
        const int KS32 = (K + 31) >> 5, ks32 = ks * 4 + g;
        if (ks32 >= KS32) return;
        u32x4* dst = (u32x4*)out + ((size_t)rg * KS32 + ks32) * 64 + i;
#pragma unroll
        for (int gg = 0; gg < 4; ++gg) {              // 8 elements = one dword of codes = one lane slot (gg, i) of the bf16 chunk
            const uint32_t d = q[gg];
            uint32_t o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = pack2bf(fp4_value((d >> (8 * j)) & 15u, sc), fp4_value((d >> (8 * j + 4)) & 15u, sc));
            dst[gg * 16] = u32x4{o[0], o[1], o[2], o[3]};
        }
    } else {
        const int n = rg * 16 + i, k0 = ks * 128 + g * 32;
        if (n >= N) return;
#pragma unroll
        for (int j = 0; j < 32; ++j)
            if (k0 + j < K) out[(size_t)n * ldo + k0 + j] = (bf16_t)f2bf(fp4_value((q[j >> 3] >> ((j & 7) * 4)) & 15u, sc));
    }
}

extern "C" int sm_unpack_weight_fp4(const void* packed, int N, int K, void* out_bf16, int ldo, void* stream) {
    SM_REQUIRE(packed && out_bf16 && N > 0 && K > 0 && ldo >= K, "sm_unpack_weight_fp4: bad args N=%d K=%d ldo=%d", N, K, ldo);
    const int KS = (K + 127) / 128;
    const size_t total = (size_t)((N + 15) / 16) * KS * 64;
    unpack_fp4_kernel<false><<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const char*)packed, N, K, KS, (bf16_t*)out_bf16, ldo, total);
    SM_LAUNCH_CHECK();
    return SM_OK;
}

// fp4 image -> packed bf16 image of sm_packed_elems(N, K) elements (every slot written: padding rows / columns decode to zero)
int launch_dequant_fp4(const void* w4, int N, int K, void* dst, hipStream_t st) {
    const int KS = (K + 127) / 128;
    const size_t total = (size_t)((N + 15) / 16) * KS * 64;
    unpack_fp4_kernel<true><<<(unsigned)((total + 255) / 256), 256, 0, st>>>((const char*)w4, N, K, KS, (bf16_t*)dst, 0, total);
    SM_LAUNCH_CHECK();
    return SM_OK;
}

// ------------------------------------------------------------------------------------------------ activation requantiser
__device__ __forceinline__ uint32_t pk4_fp8(float a, float b, float c, float d) {
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
    return (uint32_t)r;
}
// 32 consecutive k of one row -> e4m3 hi + e4m3 lo (the residual of hi), each with an e8m0 scale byte (sc16 = hi | lo << 8)
__device__ __forceinline__ void quant32_hi_lo(float (&v)[32], uint32_t (&hi)[8], uint32_t (&lo)[8], uint32_t& sc16) {
    float am = 0.f;
#pragma unroll
    for (int j = 0; j < 32; ++j) am = fmaxf(am, fabsf(v[j]));
    // hi scale 2^(floor(log2 max) - 7): the block maximum lands in [128, 256), below e4m3's 448
    int eh = (int)(__float_as_uint(am) >> 23) - 7;
    eh = am > 0.f ? (eh < 1 ? 1 : eh) : 127;
    const float inv = __uint_as_float((uint32_t)(254 - eh) << 23);
    float am2 = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        float s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = v[4 * d + j] * inv;
        hi[d] = pk4_fp8(s[0], s[1], s[2], s[3]);
        const f32x2 b0 = __builtin_amdgcn_cvt_pk_f32_fp8(hi[d], false), b1 = __builtin_amdgcn_cvt_pk_f32_fp8(hi[d], true);
        v[4 * d] = s[0] - b0[0]; v[4 * d + 1] = s[1] - b0[1]; v[4 * d + 2] = s[2] - b1[0]; v[4 * d + 3] = s[3] - b1[1];      // exact
#pragma unroll
        for (int j = 0; j < 4; ++j) am2 = fmaxf(am2, fabsf(v[4 * d + j]));
    }
    // lo scale relative to hi's: 2^tl with the residual maximum in [128, 256) (it is at most 8: tl <= -4)
    int tl = (int)(__float_as_uint(am2) >> 23) - 134;
    const int tmin = eh < 100 ? -eh : -100;
    tl = am2 > 0.f ? (tl < tmin ? tmin : tl) : 0;
    const float inv2 = __uint_as_float((uint32_t)(127 - tl) << 23);
#pragma unroll
    for (int d = 0; d < 8; ++d) lo[d] = pk4_fp8(v[4 * d] * inv2, v[4 * d + 1] * inv2, v[4 * d + 2] * inv2, v[4 * d + 3] * inv2);
    sc16 = (uint32_t)eh | ((uint32_t)(eh + tl) << 8);
}

// ------------------------------------------------------------------------------------------------ the <= 16-row kernel
#define FP4_X_BYTES 264            // LDS bytes per (k-step, row): 128 hi + 128 lo + 4 x (hi, lo) scale bytes
template <int WAVES, bool XF32, bool DUAL, bool NORM>
__global__ __launch_bounds__(WAVES * 64) void skinny_fp4_kernel(LinArgs a, int qps, float* __restrict__ ws, float* __restrict__ ws2) {
    static_assert(!NORM || XF32, "fused RMSNorm: fp32 activations");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int D = 2, PER = DUAL ? 8 : 4, NT = WAVES * 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rg = blockIdx.x, i = lane & 15, g = lane >> 4;
    const int M = a.M, KS = (a.K + 127) >> 7, KQ = (KS + 3) >> 2;
    const int q0 = blockIdx.y * qps, q1 = min(KQ, q0 + qps);
    const int ks0 = q0 * 4, ksn = min(KS, q1 * 4) - ks0;              // k-steps of this block's K slice
    float* const red = (float*)smem;                                    // [WAVES][PER][64] partial sums
    float* const nsum = red + WAVES * PER * 64;                         // NORM: [16][WAVES] sums of squares
    char* const xq = (char*)(nsum + (NORM ? 16 * WAVES : 0));           // [ksn][M][hi 128 | lo 128]
    uint16_t* const xsc = (uint16_t*)(xq + (size_t)ksn * M * 256);      // [ksn][M][4]
    const size_t rgb = fp4_rg_bytes(KS);
    const char* const wrg = (const char*)a.w + (size_t)rg * rgb;
    const char* const wrg2 = DUAL ? (const char*)a.w2 + (size_t)rg * rgb : nullptr;

    // ---- x: one thread per 32-block b = (ksl * M + m) * 4 + gg of the slice
    const int nblk = ksn * M * 4;
    struct XRaw { std::conditional_t<XF32, f32x4, u32x4> v[XF32 ? 8 : 4]; };
    auto x_load = [&](int b, XRaw& r) {
        const int gg = b & 3, t = b >> 2, m = t % M, k = (ks0 + t / M) * 128 + gg * 32;
        const bool on = k < a.K;                                         // K % 32 == 0: whole blocks (the padding of the last k-step is zero)
        const char* p = (const char*)a.x + ((size_t)m * a.ldx + (on ? k : 0)) * (XF32 ? 4 : 2);
#pragma unroll
        for (int j = 0; j < (XF32 ? 8 : 4); ++j) {
            r.v[j] = *(const std::conditional_t<XF32, f32x4, u32x4>*)(p + j * 16);
            if (!on) r.v[j] = std::conditional_t<XF32, f32x4, u32x4>{0, 0, 0, 0};
        }
    };
    auto x_quant_store = [&](int b, const XRaw& r) {
        float v[32];
        if constexpr (XF32) {
#pragma unroll
            for (int j = 0; j < 32; ++j) v[j] = r.v[j >> 2][j & 3];
        } else {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t d = r.v[j >> 2][j & 3];
                v[2 * j] = bf2f(d & 0xffff);
                v[2 * j + 1] = bf2f(d >> 16);
            }
        }
        if constexpr (NORM) {                                            // sm_norm's formula, kept in fp32: gamma * (x * rstd)
            const int gg = b & 3, t = b >> 2, m = t % M, k = (ks0 + t / M) * 128 + gg * 32;
            float tot = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) tot += nsum[m * WAVES + w];
            const float rs = rsqrtf(tot / (float)a.K + a.neps);
            if (k < a.K) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const f32x4 gm = *(const f32x4*)(a.ngamma + k + 4 * j);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[4 * j + e] = gm[e] * (v[4 * j + e] * rs);
                }
            }
        }
        uint32_t hi[8], lo[8], sc;
        quant32_hi_lo(v, hi, lo, sc);
        // e4m3 operand map: block G = b & 3 -- its first 16 k are half G >> 1 of lane group 2 (G & 1), the next 16 the same half of the group after it
        char* dst = xq + (size_t)(b >> 2) * 256 + (b & 1) * 64 + ((b >> 1) & 1) * 16;
        *(u32x4*)dst = u32x4{hi[0], hi[1], hi[2], hi[3]};
        *(u32x4*)(dst + 32) = u32x4{hi[4], hi[5], hi[6], hi[7]};
        *(u32x4*)(dst + 128) = u32x4{lo[0], lo[1], lo[2], lo[3]};
        *(u32x4*)(dst + 160) = u32x4{lo[4], lo[5], lo[6], lo[7]};
        xsc[b] = (uint16_t)sc;
    };
    if constexpr (NORM) {                                                // row sums of squares first (the launcher keeps K whole: one slice)
        for (int m = 0; m < M; ++m) {
            const float* xm = (const float*)a.x + (size_t)m * a.ldx;
            float sq = 0.f;
            for (int c = tid; c < (a.K >> 2); c += NT) {
                const f32x4 q = *(const f32x4*)(xm + (size_t)c * 4);
                sq += q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
            }
            sq = wave_sum(sq);
            if (lane == 0) nsum[m * WAVES + wave] = sq;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }
    XRaw xr0;
    if (tid < nblk) x_load(tid, xr0);                                   // ahead of the weights in the vector-memory queue
    auto x_phase = [&]() {
        if (tid < nblk) x_quant_store(tid, xr0);
        for (int b = tid + NT; b < nblk; b += NT) {
            XRaw r;
            x_load(b, r);
            x_quant_store(b, r);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    };

    // ---- weights: a ring of D quads per wave and matrix
    struct Quad { u32x4 c[4]; uint32_t s; };
    const int nq = q1 - q0, nw = wave < nq ? (nq - wave + WAVES - 1) / WAVES : 0;
    auto issue = [&](int c, Quad& w, Quad& w2) {
        const int q = q0 + wave + c * WAVES;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int ks = min(4 * q + h, KS - 1);                       // the last quad may be short: re-read, skipped below
            w.c[h] = __builtin_nontemporal_load((const u32x4*)(wrg + (size_t)ks * 1024) + lane);
            if (DUAL) w2.c[h] = __builtin_nontemporal_load((const u32x4*)(wrg2 + (size_t)ks * 1024) + lane);
        }
        w.s = __builtin_nontemporal_load((const uint32_t*)(wrg + (size_t)KS * 1024 + (size_t)q * 256) + lane);
        if (DUAL) w2.s = __builtin_nontemporal_load((const uint32_t*)(wrg2 + (size_t)KS * 1024 + (size_t)q * 256) + lane);
    };
    f32x4 acc = {0, 0, 0, 0}, acc2 = {0, 0, 0, 0};
    const int mrow = i < M ? i : 0;                // B columns >= M: any finite-or-not data, their D columns are never stored
    auto consume = [&](const Quad& w, const Quad& w2, int c) {
        const int q = q0 + wave + c * WAVES;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int ks = 4 * q + h;
            if (ks < KS) {                                               // wave-uniform
                const int t = (ks - ks0) * M + mrow;
                const char* xb = xq + (size_t)t * 256 + g * 32;           // this lane's 16 + 16 k of the row (e4m3 operand map)
                const u32x4 h0 = *(const u32x4*)xb, h1 = *(const u32x4*)(xb + 16), l0 = *(const u32x4*)(xb + 128), l1 = *(const u32x4*)(xb + 144);
                const uint32_t sx = xsc[t * 4 + g];
                const i32x8 bh = {(int)h0[0], (int)h0[1], (int)h0[2], (int)h0[3], (int)h1[0], (int)h1[1], (int)h1[2], (int)h1[3]};
                const i32x8 bl = {(int)l0[0], (int)l0[1], (int)l0[2], (int)l0[3], (int)l1[0], (int)l1[1], (int)l1[2], (int)l1[3]};
                const int sxh = (int)(sx & 0xffu), sxl = (int)(sx >> 8);
                // cbsz 4: A is e2m1 (its first four registers), blgp 0: B is e4m3; scale bytes in byte 0 of the scale operands
                const i32x8 af = {(int)w.c[h][0], (int)w.c[h][1], (int)w.c[h][2], (int)w.c[h][3], 0, 0, 0, 0};
                const int sa = (int)((w.s >> (8 * h)) & 0xffu);
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bh, acc, 4, 0, 0, sa, 0, sxh);
                acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bl, acc, 4, 0, 0, sa, 0, sxl);
                if (DUAL) {
                    const i32x8 af2 = {(int)w2.c[h][0], (int)w2.c[h][1], (int)w2.c[h][2], (int)w2.c[h][3], 0, 0, 0, 0};
                    const int sa2 = (int)((w2.s >> (8 * h)) & 0xffu);
                    acc2 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af2, bh, acc2, 4, 0, 0, sa2, 0, sxh);
                    acc2 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af2, bl, acc2, 4, 0, 0, sa2, 0, sxl);
                }
            }
        }
    };
    Quad wq[D], wq2[D];
    int done = 0, issued, live;
    if (nw >= 2 * D) {
        // the ring proper, with a straight-line entry of its own (as skinny_fp8_kernel: predicated issues in front of the loop make
        // the compiler's wait-count analysis drain the queue at the top of every round)
#pragma unroll
        for (int u = 0; u < D; ++u) issue(u, wq[u], wq2[u]);
        x_phase();
        issued = live = D;
        for (; issued + D <= nw; issued += D, done += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                consume(wq[u], wq2[u], done + u);
                issue(issued + u, wq[u], wq2[u]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        issued = live = min(nw, D);
#pragma unroll
        for (int u = 0; u < D; ++u)
            if (u < live) issue(u, wq[u], wq2[u]);
        x_phase();
    }
    const int rem = nw - issued;                    // < D quads left: each takes the registers of the quad just consumed
#pragma unroll
    for (int u = 0; u < D; ++u)
        if (u < live) {
            consume(wq[u], wq2[u], done + u);
            if (u < rem) issue(issued + u, wq[u], wq2[u]);
        }
#pragma unroll
    for (int u = 0; u < D - 1; ++u)
        if (u < rem) consume(wq[u], wq2[u], issued + u);

    if (WAVES > 1) {                                // K cut over the waves: partial sums meet in LDS, summed in wave order
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            red[(wave * PER + r) * 64 + lane] = acc[r];
            if (DUAL) red[(wave * PER + 4 + r) * 64 + lane] = acc2[r];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = 0.f, s2 = 0.f;
            for (int w = 0; w < WAVES; ++w) {
                s += red[(w * PER + r) * 64 + lane];
                if (DUAL) s2 += red[(w * PER + 4 + r) * 64 + lane];
            }
            acc[r] = s;
            if (DUAL) acc2[r] = s2;
        }
    }
    // D[n = 4g + r][m = i] (the C / D map of every 16 x 16 MFMA): lane (g, i) owns outputs n0 .. n0 + 3 of row i
    const int n0 = rg * 16 + g * 4;
    if (ws) {                                       // K slices: raw partial sums into slab blockIdx.y, [m][N padded to 4]
        if (i >= M || n0 >= a.N) return;
        const int ldw = (a.N + 3) & ~3;
        const size_t o = ((size_t)blockIdx.y * M + i) * ldw + n0;
        for (int r = 0; r < 4; ++r)
            if (n0 + r < a.N) { ws[o + r] = acc[r]; if (DUAL) ws2[o + r] = acc2[r]; }
        return;
    }
    store4(a, i, n0, acc, DUAL ? &acc2 : nullptr);
}

template <int WAVES>
static int launch_fp4_waves(const LinArgs& a, bool xf32, bool dual, int qps, int S, float* ws, float* ws2, hipStream_t st) {
    const bool norm = a.ngamma != nullptr;
    const dim3 grid(a.NRG, S), block(WAVES * 64);
    const size_t sh = ((size_t)WAVES * (dual ? 8 : 4) * 64 + (norm ? 16 * WAVES : 0)) * sizeof(float) + (size_t)qps * 4 * a.M * FP4_X_BYTES;
#define F4(XF, DU, NO) skinny_fp4_kernel<WAVES, XF, DU, NO><<<grid, block, sh, st>>>(a, qps, ws, ws2)
    if (norm) { if (dual) F4(true, true, true); else F4(true, false, true); }
    else if (xf32) { if (dual) F4(true, true, false); else F4(true, false, false); }
    else { if (dual) F4(false, true, false); else F4(false, false, false); }
#undef F4
    SM_LAUNCH_CHECK();
    return SM_OK;
}

// sm_linear with SM_W_FP4 and M <= 16 (linear.hip validated the call)
int launch_skinny_fp4(const LinArgs& a, bool xf32, hipStream_t st) {
    const bool dual = a.w2 != nullptr;
    const int KS = (a.K + 127) / 128, KQ = (KS + 3) / 4;
    int qps = (44 * 1024) / (FP4_X_BYTES * 4 * a.M);                    // quads of x per block that fit the LDS budget (>= 2 at 16 rows; + 16.5 KiB of sums < 64 KiB)
    if (qps > KQ) qps = KQ;
    const int S = (KQ + qps - 1) / qps;
    qps = (KQ + S - 1) / S;                                             // even slices
    SM_REQUIRE(!a.ngamma || S == 1, "sm_linear: fp4 weights with fused RMSNorm need the normalised rows in one K slice (M=%d K=%d)", a.M, a.K);
    float *ws = nullptr, *ws2 = nullptr;
    if (S > 1) {
        const size_t slab = (size_t)S * a.M * ((a.N + 3) & ~3);
        int rc = splitk_workspace(st, slab * sizeof(float) * (dual ? 2 : 1), &ws);
        if (rc) return rc;
        if (dual) ws2 = ws + slab;
    }
    // waves per block: at least two quads per wave where K allows (a ring needs something to ring)
    int rc;
    if (qps >= 16) rc = launch_fp4_waves<8>(a, xf32, dual, qps, S, ws, ws2, st);
    else if (qps >= 4) rc = launch_fp4_waves<4>(a, xf32, dual, qps, S, ws, ws2, st);
    else rc = launch_fp4_waves<1>(a, xf32, dual, qps, S, ws, ws2, st);
    if (rc || S == 1) return rc;
    return launch_splitk_reduce(a, ws, S, (a.N + 3) & ~3, st, ws2);
}

// ------------------------------------------------------------------------------------------------ 17..128 rows (SM_W_FP4_MFMA)
// One pass over the 4-bit codes per call, the activations requantised ONCE per call and shared by every block (the <= 16-row kernel
// requantises all rows in every block: 16 streams cost 5.7 ms per step there).
//   Prepass (quant_rows_fp4x_kernel, grid (16-row fragments, K slices of four k-steps)): one thread per 32-block, quant32_hi_lo, written
// fragment-major into a per-HIP-stream workspace [k-step][fragment][F4W_TILE]: a tile is 1 KiB of first halves of the e4m3 "hi" operand
// (lane (g, i): row i, k = 16g .. 16g+15), 1 KiB of second halves (k = 64 + 16g ..), the same 2 KiB for "lo", then lane (G, i)'s two scale
// bytes -- a B fragment is two 16-byte reads per lane and half, each 1 KiB contiguous per wave (no bank conflict, no shuffling).  The
// fragment count is the main kernel's template value (2, 4, 8): rows >= M and k >= K are zero blocks with scale 127.
//   Main kernel (wstream_fp4_kernel<MF, DUAL>, 384 threads, grid (column blocks, K slabs)) on the lines of wstream.hip:
//   * W never touches LDS.  Each of the four consumer waves owns TWO 16-row weight groups (DUAL: the gate and the up group of the same 16
//     columns, w and w2; else neighbours: a column block is 128 weight rows) and keeps a register ring of D = 2 quads per group in flight
//     (17 KiB per wave, 68 KiB per block), non-temporal loads from HBM, the Quad of the <= 16-row kernel; the codes are the A operand as they are.
//   * X goes through a two-stage LDS ring of k-steps (MF x 4224 B per stage: 33 KiB at 128 rows) filled by TWO loader waves from the
//     workspace (L2 hits; a register ring of F4W_PF k-steps in flight), so the consumers' vmcnt queues hold HBM loads only.  One raw
//     s_barrier per k-step hands stage t + 1 over and frees stage t - 1 (the loader writes exactly one k-step ahead: two stages suffice).
//   * Each B fragment pair (hi, lo) read from LDS feeds four MFMAs (two weight groups x hi / lo): 64 B of ds_read per lane per four MFMAs.
//     Accumulators: MF fragments x 4 floats per group; MF is a template value so 17..32 rows pay for two fragments, not eight.
//   Arithmetic: at 128 rows a wave issues 32 block-scaled MFMAs per k-step against 2 KiB of codes (8 at 32 rows), which would bound the kernel
// near 2.4 TB/s on the 4-bit bytes if a 16x16x128 e4m3 step took 64 clk.  Measured (tools/decode_bench.py --fp4-groups, one run on one box,
// Mistral-7B shapes): gate | up streams at 2.2 / 1.4 / 0.85 TB/s at 32 / 64 / 128 rows, a batched decode step takes 3.78 / 5.27 / 8.44 ms against
// 4.31 / 4.71 / 6.14 on bf16 -- ahead at 32 streams only.  Not the matrix pipe and not the x loads: without MFMAs, without MFMAs and B-fragment reads, and
// without x loads (tools/experiments/wstream_fp4_probe.hip) gate | up at 128 rows goes 61.8 -> 56.2 / 46.3 / 56.7 us, without all three 33.9 -- the costs
// add, i.e. the k-step is a serial chain between its two barriers with one consumer wave per SIMD ("MXFP4 weights").
//   Grid: N = 4096 gives 32 column blocks, so the K quads are cut into up to 8 slabs (4 above 64 rows: a slab is M x N fp32 written and
// read again) of at least two quads; slabs leave raw partial sums in the split-K workspace and launch_splitk_reduce applies the epilogue in
// slab order (deterministic).  One slab: store4 in the kernel.  Ragged shapes follow the <= 16-row kernel: a short last quad re-reads the
// last chunk and skips its MFMAs (every wave still meets the barrier), rows >= M / columns >= N are never stored.
#define F4W_TILE 4224              // bytes per (k-step, 16-row fragment) of requantised x: 2 KiB hi + 2 KiB lo + 64 x (hi, lo) scale bytes
#define F4W_PF 2                   // k-steps of x in flight per loader wave (registers)
// experiment switches of tools/experiments/wstream_fp4_probe.hip (all 0 in the product): F4W_X_NOMFMA: no MFMAs (the operands are still consumed),
// F4W_X_NOXREAD: no B-fragment reads from LDS, F4W_X_NOXLOAD: the loaders fetch nothing from the workspace (barriers and LDS writes stay)
#ifndef F4W_X_NOMFMA
#define F4W_X_NOMFMA 0
#endif
#ifndef F4W_X_NOXREAD
#define F4W_X_NOXREAD 0
#endif
#ifndef F4W_X_NOXLOAD
#define F4W_X_NOXLOAD 0
#endif
#define F4W_PREPASS_TAG (1LL << 62)  // sm_prof_read_tag key of the prepass launches: this | K

template <bool XF32>
__global__ __launch_bounds__(256) void quant_rows_fp4x_kernel(const void* __restrict__ x, int M, int K, int ldx, int MF, int KS, char* __restrict__ xq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mg = blockIdx.x, ks = blockIdx.y * 4 + wave;
    if (ks >= KS) return;
    const int i = lane >> 2, G = lane & 3, m = mg * 16 + i, k = ks * 128 + G * 32;     // a row's four blocks sit in neighbouring lanes: 256 / 512 B contiguous
    float v[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) v[j] = 0.f;
    if (m < M && k < K) {                                                // K % 32 == 0: whole blocks
        const char* p = (const char*)x + ((size_t)m * ldx + k) * (XF32 ? 4 : 2);
        if constexpr (XF32) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const f32x4 q = *(const f32x4*)(p + j * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[4 * j + e] = q[e];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const u32x4 q = *(const u32x4*)(p + j * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[8 * j + 2 * e] = bf2f(q[e] & 0xffff); v[8 * j + 2 * e + 1] = bf2f(q[e] >> 16); }
            }
        }
    }
    uint32_t hi[8], lo[8], sc;
    quant32_hi_lo(v, hi, lo, sc);
    // e4m3 operand map: block G's first 16 k are half G >> 1 of lane group 2 (G & 1), the next 16 the same half of the group after it
    char* const tile = xq + ((size_t)ks * MF + mg) * F4W_TILE;
    char* const d = tile + (G >> 1) * 1024 + ((G & 1) * 32 + i) * 16;
    *(u32x4*)d = u32x4{hi[0], hi[1], hi[2], hi[3]};
    *(u32x4*)(d + 256) = u32x4{hi[4], hi[5], hi[6], hi[7]};
    *(u32x4*)(d + 2048) = u32x4{lo[0], lo[1], lo[2], lo[3]};
    *(u32x4*)(d + 2048 + 256) = u32x4{lo[4], lo[5], lo[6], lo[7]};
    *(uint16_t*)(tile + 4096 + (G * 16 + i) * 2) = (uint16_t)sc;
}

template <int MF, bool DUAL>
__global__ __launch_bounds__(384) void wstream_fp4_kernel(LinArgs a, const char* __restrict__ xq, int qps, float* __restrict__ ws, float* __restrict__ ws2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];         // [2][MF][F4W_TILE]
    constexpr int STG = MF * F4W_TILE, U = STG / 16, NL = (U + 127) / 128, D = 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KS = (a.K + 127) >> 7, KQ = (KS + 3) >> 2;
    const int q0 = blockIdx.y * qps, nq = min(KQ, q0 + qps) - q0;
    const int ks0 = q0 * 4, nks = min(KS, ks0 + nq * 4) - ks0;         // k-steps that exist; every wave meets 1 + 4 nq barriers (whole quads)

    if (wave >= 4) {
        // ---- two loader waves: k-step t of the workspace (U 16-byte units, contiguous) into stage t & 1, unit l + 128 j per lane
        const int l = (wave - 4) * 64 + lane;
        const u32x4* const src = (const u32x4*)(xq + (size_t)ks0 * STG) + l;
        u32x4 xr[F4W_PF][NL];
        auto fetch = [&](int t, u32x4 (&r)[NL]) {
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if ((j + 1) * 128 <= U || l + j * 128 < U) r[j] = F4W_X_NOXLOAD ? u32x4{0, 0, 0, 0} : src[(size_t)t * U + j * 128];
        };
        auto put = [&](int t, const u32x4 (&r)[NL]) {
            u32x4* const dst = (u32x4*)(smem + (t & 1) * STG) + l;
#pragma unroll
            for (int j = 0; j < NL; ++j)
                if ((j + 1) * 128 <= U || l + j * 128 < U) dst[j * 128] = r[j];
        };
        fetch(0, xr[0]);
        if (1 < nks) fetch(1, xr[1]);
        put(0, xr[0]);
        if (2 < nks) fetch(2, xr[0]);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                                   // stage 0 is in LDS
        // iteration t (behind the barrier that published stage t): k-step t + 1 (ring slot (t + 1) % PF) into stage (t + 1) & 1 -- last read during
        // k-step t - 1, closed by that barrier --, refill the slot with k-step t + 1 + PF, barrier (it publishes stage t + 1)
        auto ltrip = [&](int t0, auto steady) {
            constexpr bool STEADY = decltype(steady)::value;
#pragma unroll
            for (int d = 0; d < F4W_PF; ++d) {
                const int t = t0 + d;
                if (STEADY || t + 1 < nks) put(t + 1, xr[(d + 1) % F4W_PF]);
                if (STEADY || t + 1 + F4W_PF < nks) fetch(t + 1 + F4W_PF, xr[(d + 1) % F4W_PF]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        int t0 = 0;
        for (; t0 + 2 * F4W_PF < nks; t0 += F4W_PF) ltrip(t0, std::true_type{});
        for (; t0 < nq * 4; t0 += F4W_PF) ltrip(t0, std::false_type{});
        return;
    }

    // ---- four consumer waves
    const int i = lane & 15, g = lane >> 4;
    const int rgA = DUAL ? blockIdx.x * 4 + wave : blockIdx.x * 8 + wave * 2, rgB = DUAL ? rgA : rgA + 1;
    const size_t rgb = fp4_rg_bytes(KS);
    const char* const wA = (const char*)a.w + (size_t)(rgA < a.NRG ? rgA : 0) * rgb;
    const char* const wB = (const char*)(DUAL ? a.w2 : a.w) + (size_t)(rgB < a.NRG ? rgB : 0) * rgb;
    struct Quad { u32x4 c[4]; uint32_t s; };
    auto issue = [&](int c, Quad& qa, Quad& qb) {
        const int q = q0 + c;
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int ks = min(4 * q + h, KS - 1);                       // the last quad may be short: re-read, skipped below
            qa.c[h] = __builtin_nontemporal_load((const u32x4*)(wA + (size_t)ks * 1024) + lane);
            qb.c[h] = __builtin_nontemporal_load((const u32x4*)(wB + (size_t)ks * 1024) + lane);
        }
        qa.s = __builtin_nontemporal_load((const uint32_t*)(wA + (size_t)KS * 1024 + (size_t)q * 256) + lane);
        qb.s = __builtin_nontemporal_load((const uint32_t*)(wB + (size_t)KS * 1024 + (size_t)q * 256) + lane);
    };
    f32x4 accA[MF], accB[MF];
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) accA[mf] = accB[mf] = f32x4{0, 0, 0, 0};
    auto consume = [&](const Quad& qa, const Quad& qb, int c) {
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int t = 4 * c + h;
            if (t < nks) {                                               // block-uniform
                const char* const st = smem + (t & 1) * STG;
                const i32x8 afA = {(int)qa.c[h][0], (int)qa.c[h][1], (int)qa.c[h][2], (int)qa.c[h][3], 0, 0, 0, 0};
                const i32x8 afB = {(int)qb.c[h][0], (int)qb.c[h][1], (int)qb.c[h][2], (int)qb.c[h][3], 0, 0, 0, 0};
                const int saA = (int)((qa.s >> (8 * h)) & 0xffu), saB = (int)((qb.s >> (8 * h)) & 0xffu);
#pragma unroll
                for (int mf = 0; mf < MF; ++mf) {
                    const char* const xb = st + mf * F4W_TILE + lane * 16;
                    u32x4 h0 = {0, 0, 0, 0}, h1 = h0, l0 = h0, l1 = h0;
                    uint32_t sx = 0x7f7fu;
                    if (!F4W_X_NOXREAD) {
                        h0 = *(const u32x4*)xb; h1 = *(const u32x4*)(xb + 1024); l0 = *(const u32x4*)(xb + 2048); l1 = *(const u32x4*)(xb + 3072);
                        sx = *(const uint16_t*)(st + mf * F4W_TILE + 4096 + lane * 2);
                    }
                    if (F4W_X_NOMFMA) {
                        accA[mf] += __builtin_bit_cast(f32x4, (h0 ^ h1) + sx);
                        accB[mf] += __builtin_bit_cast(f32x4, l0 ^ l1);
                        if (mf == 0) { accA[0] += __builtin_bit_cast(f32x4, qa.c[h] + (uint32_t)saA); accB[0] += __builtin_bit_cast(f32x4, qb.c[h] + (uint32_t)saB); }
                        continue;
                    }
                    const i32x8 bh = {(int)h0[0], (int)h0[1], (int)h0[2], (int)h0[3], (int)h1[0], (int)h1[1], (int)h1[2], (int)h1[3]};
                    const i32x8 bl = {(int)l0[0], (int)l0[1], (int)l0[2], (int)l0[3], (int)l1[0], (int)l1[1], (int)l1[2], (int)l1[3]};
                    const int sxh = (int)(sx & 0xffu), sxl = (int)(sx >> 8);
                    // cbsz 4: A is e2m1 (its first four registers), blgp 0: B is e4m3; scale bytes in byte 0 of the scale operands
                    accA[mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afA, bh, accA[mf], 4, 0, 0, saA, 0, sxh);
                    accB[mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afB, bh, accB[mf], 4, 0, 0, saB, 0, sxh);
                    accA[mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afA, bl, accA[mf], 4, 0, 0, saA, 0, sxl);
                    accB[mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afB, bl, accB[mf], 4, 0, 0, saB, 0, sxl);
                }
            }
            // this wave's reads of stage t have returned: the loaders may overwrite it behind the NEXT barrier; this one publishes stage t + 1
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
    };
    Quad wq[D], wq2[D];
    int done = 0, issued, live;
    if (nq >= 2 * D) {                              // the ring proper, with a straight-line entry of its own (as skinny_fp4_kernel)
#pragma unroll
        for (int u = 0; u < D; ++u) issue(u, wq[u], wq2[u]);
        __builtin_amdgcn_s_barrier();               // stage 0 is in LDS
        asm volatile("" ::: "memory");
        issued = live = D;
        for (; issued + D <= nq; issued += D, done += D) {
#pragma unroll
            for (int u = 0; u < D; ++u) {
                consume(wq[u], wq2[u], done + u);
                issue(issued + u, wq[u], wq2[u]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else {
        issued = live = min(nq, D);
#pragma unroll
        for (int u = 0; u < D; ++u)
            if (u < live) issue(u, wq[u], wq2[u]);
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }
    const int rem = nq - issued;                    // < D quads left: each takes the registers of the quad just consumed
#pragma unroll
    for (int u = 0; u < D; ++u)
        if (u < live) {
            consume(wq[u], wq2[u], done + u);
            if (u < rem) issue(issued + u, wq[u], wq2[u]);
        }
#pragma unroll
    for (int u = 0; u < D - 1; ++u)
        if (u < rem) consume(wq[u], wq2[u], issued + u);

    // ---- epilogue.  acc[mf]: lane (g, i) holds n = rg * 16 + 4g + 0..3 of row m = mf * 16 + i; rows >= M / columns >= N are not stored
    const int nA = rgA * 16 + g * 4, nB = rgB * 16 + g * 4, ldw = (a.N + 3) & ~3;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = mf * 16 + i;
        if (m >= a.M) continue;
        if (ws) {                                   // K slabs: raw partial sums into slab blockIdx.y, [m][N padded to 4]
            const size_t o = ((size_t)blockIdx.y * a.M + m) * ldw;
            for (int r = 0; r < 4; ++r) {
                if (nA + r < a.N) ws[o + nA + r] = accA[mf][r];
                if (nB + r < a.N) (DUAL ? ws2 : ws)[o + nB + r] = accB[mf][r];
            }
        } else if (DUAL) {
            const f32x4 up = accB[mf];              // (a copy: &accB[mf] made the whole array address-taken and put it into scratch, MFMA loop included)
            store4(a, m, nA, accA[mf], &up);
        } else {
            store4(a, m, nA, accA[mf], nullptr);
            store4(a, m, nB, accB[mf], nullptr);
        }
    }
}

// per-HIP-stream workspace of the requantised activations (grown on demand; steady state allocates nothing)
static std::mutex g_x4_mu;
static std::map<hipStream_t, std::pair<void*, size_t>> g_x4;
void release_fp4_workspace(hipStream_t st) {
    std::lock_guard<std::mutex> lk(g_x4_mu);
    auto e = g_x4.find(st);
    if (e != g_x4.end()) { if (e->second.first) (void)hipFree(e->second.first); g_x4.erase(e); }
}

// the prepass: the rows of a call requantised into the stream's workspace as MF fragments per k-step (rows >= M: zero blocks)
static int requant_rows_fp4(const LinArgs& a, bool xf32, int MF, int prof_cls, hipStream_t st, char** out) {
    const int KS = (a.K + 127) / 128;
    const size_t need = (size_t)KS * MF * F4W_TILE;
    char* xq;
    {
        std::lock_guard<std::mutex> lk(g_x4_mu);
        auto& e = g_x4[st];
        if (e.second < need) {
            if (e.first) { SM_HIP(hipStreamSynchronize(st)); (void)hipFree(e.first); e.first = nullptr; e.second = 0; }
            SM_HIP(hipMalloc(&e.first, need));
            e.second = need;
        }
        xq = (char*)e.first;
    }
    {   // (profiling tags: the prepass under F4W_PREPASS_TAG | K, the product with its slab sum under the shape tag of the other weight streams)
        SmProfScope prof(prof_cls, st, F4W_PREPASS_TAG | (unsigned)a.K);
        const dim3 qgrid(MF, (KS + 3) / 4);
        if (xf32) quant_rows_fp4x_kernel<true><<<qgrid, 256, 0, st>>>(a.x, a.M, a.K, a.ldx, MF, KS, xq);
        else quant_rows_fp4x_kernel<false><<<qgrid, 256, 0, st>>>(a.x, a.M, a.K, a.ldx, MF, KS, xq);
        SM_LAUNCH_CHECK();
    }
    *out = xq;
    return SM_OK;
}

template <int MF>
static int launch_wstream_fp4_mf(const LinArgs& a, bool xf32, hipStream_t st) {
    const bool dual = a.w2 != nullptr;
    const int KS = (a.K + 127) / 128, KQ = (KS + 3) / 4;
    char* xq;
    if (int rc = requant_rows_fp4(a, xf32, MF, SM_PROF_SKINNY, st, &xq)) return rc;
    SmProfScope prof(SM_PROF_SKINNY, st, ((long long)a.N << 32) | (unsigned)a.K);
    // K slabs: fill 256 CUs, at least two quads per slab, at most 8 slabs (4 above 64 rows: every slab is M x N fp32 written and read again)
    const int CB = dual ? cdiv(a.NRG, 4) : cdiv(a.NRG, 8);
    int S = std::min(std::min(MF > 4 ? 4 : 8, cdiv(256, CB)), std::max(1, KQ / 2));
    const int qps = cdiv(KQ, S);
    S = cdiv(KQ, qps);
    float *ws = nullptr, *ws2 = nullptr;
    if (S > 1) {
        const size_t slab = (size_t)S * a.M * ((a.N + 3) & ~3);
        int rc = splitk_workspace(st, slab * sizeof(float) * (dual ? 2 : 1), &ws);
        if (rc) return rc;
        if (dual) ws2 = ws + slab;
    }
    constexpr size_t sh = 2 * (size_t)MF * F4W_TILE;
    if (sh > 64 * 1024) {                           // (MF = 8: 66 KiB, above the default limit; a function attribute is per device: set once on each)
        static std::mutex mu;
        static bool attr_set[64] = {};
        int dev = 0;
        SM_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= 64 || !attr_set[dev]) {
            SM_HIP(hipFuncSetAttribute((const void*)wstream_fp4_kernel<MF, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            SM_HIP(hipFuncSetAttribute((const void*)wstream_fp4_kernel<MF, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            if (dev >= 0 && dev < 64) attr_set[dev] = true;
        }
    }
    const dim3 grid(CB, S);
    if (dual) wstream_fp4_kernel<MF, true><<<grid, 384, sh, st>>>(a, xq, qps, ws, ws2);
    else wstream_fp4_kernel<MF, false><<<grid, 384, sh, st>>>(a, xq, qps, ws, ws2);
    SM_LAUNCH_CHECK();
    if (S == 1) return SM_OK;
    return launch_splitk_reduce(a, ws, S, (a.N + 3) & ~3, st, ws2);
}

// sm_linear with SM_W_FP4_MFMA and 17..128 rows (linear.hip validated the call)
int launch_wstream_fp4(const LinArgs& a, bool xf32, hipStream_t st) {
    if (a.M <= 32) return launch_wstream_fp4_mf<2>(a, xf32, st);
    if (a.M <= 64) return launch_wstream_fp4_mf<4>(a, xf32, st);
    return launch_wstream_fp4_mf<8>(a, xf32, st);
}

// ------------------------------------------------------------------------------------------------ above 128 rows (SM_W_FP4_GEMM)
// A tiled GEMM on the lines of gemm_fp8_kernel: above 128 rows both operands are re-used across tiles, so both go through LDS.  The semantics are
// those of the 17..128-row path -- the prepass above requantises the rows once per call (e4m3 hi + lo per 32-block), fragment count padded to whole
// m tiles so that a tile load never leaves the workspace -- and so is the error class: a prefill chunk that crosses 128 rows does not move the logits.
//   Block: four waves, tile 128 weight rows (n) x BM activation rows (m) x one k-step of 128; a wave owns 64 n x BM / 2 m, four A fragments against
// BM / 32 B fragment pairs (hi, lo): an A fragment read from LDS feeds 2 x BM / 32 MFMAs.  BM = 128 above 256 rows, 64 up to there (a third m tile
// of 128 would be mostly padding); K slabs fill the chip where the tiles alone do not.
//   Stage (one k-step): 8 x 1 KiB of codes, the image's chunks as they are (a lane's 16 bytes are its A operand); 8 x 256 B of scale dwords -- the
// scale chunk of the k-step's quad, fetched with every k-step of the quad: three of four are L2 hits, and every stage is the same list of loads, so the
// counted waits are constants; the lane picks byte ks & 3 --; BM / 16 workspace tiles of F4W_TILE bytes, contiguous, copied as they are in 1-KiB
// wave-instructions (the ragged last one at BM = 64 re-reads the last 16 bytes into padding of the stage).  43 KiB at BM = 128, 27 KiB at BM = 64.
//   Ring: three stages filled TWO k-steps ahead by LDS-DMA (129 / 81 KiB of the CU's 160: one block per CU -- a k-step is 16-32 MFMAs per wave, the
// matrix pipe is the bound by an order of magnitude over the 43 KiB of DMA, and a deeper ring covers an L2 round trip where a second block would
// only halve the ring), counted vmcnt waits, one raw s_barrier per k-step (gemm_fp8_kernel has the reasons).
//   SwiGLU dual (w / w2): a block's 128 weight rows are 64 gate rows and the 64 up rows of the same columns; a wave holds both for its 32 columns and
// store4 (or the slab sum) applies SiLU(gate) * up.  Ragged shapes: row groups >= NRG re-read the last group and rows >= N / >= M are never stored;
// a last k-step beyond K is zero blocks on the x side and zero codes on the w side; the scale chunk of a short last quad is whole in the image.
//   Tile order: XCD-banded as gemm_fp8_kernel; m fastest (the blocks of a column tile share its codes in one L2) unless the requantised rows are the
// heavier operand (2.06 x M bytes per k against 0.53 x N), then n fastest.
#define FP4_GEMM_VMWAIT(n) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(n) : "memory")

template <int BM, bool DUAL>
__global__ __launch_bounds__(256) void gemm_fp4_kernel(LinArgs a, const char* __restrict__ xq, int tiles_m, int tiles_n, int qps, int n_fast,
                                                       float* __restrict__ ws, float* __restrict__ ws2) {
    constexpr int MF = BM / 32;                       // B fragment pairs per wave
    constexpr int XB = (BM / 16) * F4W_TILE;          // bytes of x per stage
    constexpr int NI = (XB + 1023) / 1024;            // ... in wave-instructions of 1 KiB
    constexpr int STAGE = 8192 + 2048 + NI * 1024;
    constexpr int NXF = NI / 4, EXTRA = NI % 4;       // x instructions per wave: NXF, one more for waves < EXTRA
    constexpr int LW = 4 + NXF;                       // loads per wave and stage (2 code pieces, 2 scale pieces, x)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int wn = wave >> 1, wm = wave & 1;
    int bid = blockIdx.x;
    {   // XCD-banded tile order (block b runs on XCD b % 8): an XCD works on neighbouring tiles and shares their operands in its L2
        const int nblk = tiles_m * tiles_n, q = nblk >> 3, r = nblk & 7;
        const int xcd = bid & 7, idx = bid >> 3;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    const int tile_n = n_fast ? bid % tiles_n : bid / tiles_m, tile_m = n_fast ? bid / tiles_n : bid % tiles_m;
    const int KS = (a.K + 127) >> 7;
    const int ks0 = blockIdx.y * qps * 4, nks = min(KS, ks0 + qps * 4) - ks0;         // this slab's k-steps (whole quads but the last)
    const size_t rgb = fp4_rg_bytes(KS);

    // staging sources: wave w brings weight pieces 2w, 2w + 1 (codes and scale dwords) and x instructions w, w + 4, ...
    const char* wsrc[2];
    const char* ssrc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = wave * 2 + u;                   // piece p: row group tile_n * 8 + p; DUAL: gate group tile_n * 4 + p, pieces 4..7 the up groups
        const char* img = (const char*)((DUAL && p >= 4) ? a.w2 : a.w);
        int rg = DUAL ? tile_n * 4 + (p & 3) : tile_n * 8 + p;
        if (rg >= a.NRG) rg = a.NRG - 1;
        wsrc[u] = img + (size_t)rg * rgb + (size_t)ks0 * 1024 + lane * 16;
        ssrc[u] = img + (size_t)rg * rgb + (size_t)KS * 1024 + lane * 4;
    }
    const size_t xstep = (size_t)tiles_m * (BM / 16) * F4W_TILE;                      // the workspace's bytes per k-step
    const char* const xsrc = xq + (size_t)ks0 * xstep + (size_t)tile_m * XB;
    int xoff[NXF + 1];
#pragma unroll
    for (int p = 0; p <= NXF; ++p) xoff[p] = min(((p * 4 + wave) * 64 + lane) * 16, XB - 16);
    auto stage = [&](int t, int slot) {
        char* const sb = smem + slot * STAGE;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            glds16(wsrc[u] + (size_t)t * 1024, sb + (wave * 2 + u) * 1024);
            __builtin_amdgcn_global_load_lds((gbl_ptr_t)(ssrc[u] + (size_t)((ks0 + t) >> 2) * 256), (lds_ptr_t)(sb + 8192 + (wave * 2 + u) * 256), 4, 0, 0);
        }
        const char* const xs = xsrc + (size_t)t * xstep;
#pragma unroll
        for (int p = 0; p < NXF; ++p) glds16(xs + xoff[p], sb + 10240 + (p * 4 + wave) * 1024);
        if (wave < EXTRA) glds16(xs + xoff[NXF], sb + 10240 + (NXF * 4 + wave) * 1024);
    };
    f32x4 acc[4][MF];
#pragma unroll
    for (int nf = 0; nf < 4; ++nf)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[nf][mf] = f32x4{0, 0, 0, 0};

    stage(0, 0);
    if (nks > 1) stage(1, 1);
    int slot = 0;
    for (int t = 0; t < nks; ++t) {
        // this wave's loads of k-step t have landed (those of t + 1 may stay in flight: vmcnt retires in order) ...
        if (t + 1 < nks) {
            if (wave < EXTRA) FP4_GEMM_VMWAIT(LW + 1);
            else FP4_GEMM_VMWAIT(LW);
        } else {
            FP4_GEMM_VMWAIT(0);
        }
        __builtin_amdgcn_s_barrier();                 // ... everyone's; and every wave is done reading the slot of k-step t - 1
        asm volatile("" ::: "memory");
        if (t + 2 < nks) stage(t + 2, slot == 0 ? 2 : slot - 1);
        const char* const sb = smem + slot * STAGE;
        const int hb = ((ks0 + t) & 3) * 8;
        i32x8 bh[MF], bl[MF];
        int sxh[MF], sxl[MF];
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            const char* const xb = sb + 10240 + (wm * MF + mf) * F4W_TILE;
            const u32x4 h0 = *(const u32x4*)(xb + lane * 16), h1 = *(const u32x4*)(xb + 1024 + lane * 16);
            const u32x4 l0 = *(const u32x4*)(xb + 2048 + lane * 16), l1 = *(const u32x4*)(xb + 3072 + lane * 16);
            const uint32_t sx = *(const uint16_t*)(xb + 4096 + lane * 2);
            bh[mf] = i32x8{(int)h0[0], (int)h0[1], (int)h0[2], (int)h0[3], (int)h1[0], (int)h1[1], (int)h1[2], (int)h1[3]};
            bl[mf] = i32x8{(int)l0[0], (int)l0[1], (int)l0[2], (int)l0[3], (int)l1[0], (int)l1[1], (int)l1[2], (int)l1[3]};
            sxh[mf] = (int)(sx & 0xffu); sxl[mf] = (int)(sx >> 8);
        }
#pragma unroll
        for (int nf = 0; nf < 4; ++nf) {
            const int piece = DUAL ? (nf >> 1) * 4 + wn * 2 + (nf & 1) : wn * 4 + nf;
            const u32x4 c = *(const u32x4*)(sb + piece * 1024 + lane * 16);
            const uint32_t sd = *(const uint32_t*)(sb + 8192 + piece * 256 + lane * 4);
            // cbsz 4: A is e2m1 (its first four registers), blgp 0: B is e4m3; scale bytes in byte 0 of the scale operands
            const i32x8 af = {(int)c[0], (int)c[1], (int)c[2], (int)c[3], 0, 0, 0, 0};
            const int sa = (int)((sd >> hb) & 0xffu);
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                acc[nf][mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bh[mf], acc[nf][mf], 4, 0, 0, sa, 0, sxh[mf]);
                acc[nf][mf] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(af, bl[mf], acc[nf][mf], 4, 0, 0, sa, 0, sxl[mf]);
            }
        }
        slot = slot == 2 ? 0 : slot + 1;
    }

    // ---- epilogue.  acc[nf][mf]: lane (g, i) holds n = n0 .. n0 + 3 of row m; rows >= M / columns >= N are not stored
    const int ldw = (a.N + 3) & ~3;
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) {
        const int m = tile_m * BM + wm * (BM / 2) + mf * 16 + i;
        if (m >= a.M) continue;
#pragma unroll
        for (int nf = 0; nf < (DUAL ? 2 : 4); ++nf) {
            const int n0 = (DUAL ? tile_n * 4 + wn * 2 + nf : tile_n * 8 + wn * 4 + nf) * 16 + g * 4;
            if (n0 >= a.N) continue;
            const f32x4 v = acc[nf][mf], up = acc[DUAL ? nf + 2 : nf][mf];           // (copies: no address of the accumulator array is taken)
            if (ws) {                                 // K slabs: raw partial sums into slab blockIdx.y, [m][N padded to 4]
                const size_t o = ((size_t)blockIdx.y * a.M + m) * ldw + n0;
                *(f32x4*)(ws + o) = v;
                if (DUAL) *(f32x4*)(ws2 + o) = up;
            } else {
                store4(a, m, n0, v, DUAL ? &up : nullptr);
            }
        }
    }
}

template <int BM>
static int launch_gemm_fp4_bm(const LinArgs& a, bool xf32, hipStream_t st) {
    const bool dual = a.w2 != nullptr;
    const int KS = (a.K + 127) / 128, KQ = (KS + 3) / 4;
    const int tiles_m = cdiv(a.M, BM), tiles_n = dual ? cdiv(a.NRG, 4) : cdiv(a.NRG, 8);
    char* xq;
    if (int rc = requant_rows_fp4(a, xf32, tiles_m * (BM / 16), SM_PROF_GEMM, st, &xq)) return rc;
    SmProfScope prof(SM_PROF_GEMM, st, ((long long)a.N << 32) | (unsigned)a.K);
    // K slabs where the tiles do not fill 256 CUs (o and down at a few hundred rows): whole quads, at least two per slab, at most 8 slabs
    const int blocks = tiles_m * tiles_n;
    int S = std::max(1, std::min(std::min(8, 256 / blocks), KQ / 2));
    const int qps = cdiv(KQ, S);
    S = cdiv(KQ, qps);
    float *ws = nullptr, *ws2 = nullptr;
    if (S > 1) {
        const size_t slab = (size_t)S * a.M * ((a.N + 3) & ~3);
        int rc = splitk_workspace(st, slab * sizeof(float) * (dual ? 2 : 1), &ws);
        if (rc) return rc;
        if (dual) ws2 = ws + slab;
    }
    constexpr int sh = 3 * (8192 + 2048 + (((BM / 16) * F4W_TILE + 1023) / 1024) * 1024);
    {   // (above the default limit of 64 KiB; a function attribute is per device: set once on each)
        static std::mutex mu;
        static bool attr_set[64] = {};
        int dev = 0;
        SM_HIP(hipGetDevice(&dev));
        std::lock_guard<std::mutex> lk(mu);
        if (dev < 0 || dev >= 64 || !attr_set[dev]) {
            SM_HIP(hipFuncSetAttribute((const void*)gemm_fp4_kernel<BM, false>, hipFuncAttributeMaxDynamicSharedMemorySize, sh));
            SM_HIP(hipFuncSetAttribute((const void*)gemm_fp4_kernel<BM, true>, hipFuncAttributeMaxDynamicSharedMemorySize, sh));
            if (dev >= 0 && dev < 64) attr_set[dev] = true;
        }
    }
    const int n_fast = (long)tiles_m * BM * 4 > (long)a.N * (dual ? 2 : 1);          // 2.06 x M against 0.53 x N bytes per k
    const dim3 grid(blocks, S);
    if (dual) gemm_fp4_kernel<BM, true><<<grid, 256, sh, st>>>(a, xq, tiles_m, tiles_n, qps, n_fast, ws, ws2);
    else gemm_fp4_kernel<BM, false><<<grid, 256, sh, st>>>(a, xq, tiles_m, tiles_n, qps, n_fast, ws, ws2);
    SM_LAUNCH_CHECK();
    if (S == 1) return SM_OK;
    return launch_splitk_reduce(a, ws, S, (a.N + 3) & ~3, st, ws2);
}

// sm_linear with SM_W_FP4_GEMM above 128 rows (linear.hip validated the call)
int launch_gemm_fp4(const LinArgs& a, bool xf32, hipStream_t st) {
    if (a.M > 256) return launch_gemm_fp4_bm<128>(a, xf32, st);
    return launch_gemm_fp4_bm<64>(a, xf32, st);
}
