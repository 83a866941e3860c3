// FP8 (OCP e4m3) K / V cache: the producers (RoPE + quantise + append) and the expansion back to bf16 for chunk attention.  The format stands in
// common.h (next to the MXFP4 block); the consumer of single-token steps is decode_attn_fp8_kernel (attention.hip).
//
// One (token, KV head) row of 128 values shares one fp32 scale = amax / 448 (1.0 for an all-zero row); codes are RNE(x / scale) saturated at +-448, so a
// kernel never emits the NaN codes 0x7F / 0xFF.  K is quantised AFTER RoPE, from the fp32 rotation (no bf16 rounding in between); V from the fp32 product.
// head_dim 128 only.  q leaves as bf16 with the arithmetic of rope_kv_kernel (vecops.hip), bit for bit.
#include "common.h"
#include "host.h"

// 4 floats -> 4 e4m3 codes in one dword (element 0 in the low byte).  The clamp makes the saturation explicit and turns a NaN input into -448 (v_max / v_min
// return the non-NaN operand): no NaN code is ever stored.
__device__ __forceinline__ uint32_t kv8_pk4(float a, float b, float c, float d) {
    const float lo = -448.f, hi = 448.f;
    int r = 0;
    r = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(a, lo), hi), fminf(fmaxf(b, lo), hi), r, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(fminf(fmaxf(c, lo), hi), fminf(fmaxf(d, lo), hi), r, true);
    return (uint32_t)r;
}
// the rotation of a K head: every product and the sum rounded to fp32 on its own (no contraction), so that the quantised values -- and with them amax and the
// scale -- are those of the plain fp32 RoPE whatever the compiler would fuse.  q keeps the expression of rope_kv_kernel as it compiles there (bit-identical q).
__device__ __forceinline__ void kv8_rope_pair(float a, float b, float c, float s, float& o0, float& o1) {
#pragma clang fp contract(off)
    const float ac = a * c, bs = b * s, bc = b * c, as = a * s;
    o0 = ac - bs;
    o1 = bc + as;
}
__device__ __forceinline__ float kv8_scale(float amax) { return amax > 0.f ? amax / 448.0f : 1.0f; }

// where the scales start inside the two buffers of a layer (bytes): behind the codes
__host__ __device__ __forceinline__ size_t kv8_scale_off(int S_max, int KV) { return (size_t)S_max * KV * 128; }

// ---- one row.  Lane L of the 64-lane block owns the rotation pairs (d, d + 64), d = 2 (L & 31) + {0, 1}: the lower half-wave produces the two outputs at d, the
// upper half-wave those at d + 64 -- every lane ends with two ADJACENT outputs, so a K head's codes are gathered 8 lanes -> 16 bytes with four shuffles
// and leave as eight 16-byte stores; q leaves as one dword per lane.  A V head: lane L owns dims 2 L, 2 L + 1 (V^T of a single row is a strided byte per dim).
// X: the row's source, indexable (plain fp32 row, or the unsummed split-K slabs of the q|k|v product summed on load).
template <class X>
__device__ __forceinline__ void rope_kv_fp8_row(const X& x, int pos, int hd, int H, int KV, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                bf16_t* __restrict__ qdst, uint8_t* __restrict__ kc, uint8_t* __restrict__ vtc, int S_max) {
    const int lane = threadIdx.x;
    if (hd < H + KV) {
        const int j = (lane & 31) * 2, up = lane >> 5;
        float o[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const float c = cos_tab[(size_t)pos * 64 + j + e], s = sin_tab[(size_t)pos * 64 + j + e];
            const float a = x[j + e], b = x[j + e + 64];
            float o0 = a * c - b * s, o1 = b * c + a * s;
            if (hd >= H) kv8_rope_pair(a, b, c, s, o0, o1);
            o[e] = up ? o1 : o0;
        }
        if (hd < H) {
            *(uint32_t*)(qdst + j + up * 64) = pack2bf(o[0], o[1]);
            return;
        }
        const float sc = kv8_scale(wave_max(fmaxf(fabsf(o[0]), fabsf(o[1]))));
        const uint32_t h = kv8_pk4(o[0] / sc, o[1] / sc, 0.f, 0.f) & 0xffffu;
        const uint32_t w0 = h | ((uint32_t)__shfl_down((int)h, 1, 64) << 16);             // valid in even lanes: 4 codes
        const uint32_t w1 = (uint32_t)__shfl_down((int)w0, 2, 64), w2 = (uint32_t)__shfl_down((int)w0, 4, 64), w3 = (uint32_t)__shfl_down((int)w0, 6, 64);
        const int kh = hd - H;
        uint8_t* row = kc + ((size_t)pos * KV + kh) * 128;
        if ((lane & 7) == 0) *(u32x4*)(row + lane * 2) = u32x4{w0, w1, w2, w3};          // lane 8 t: codes 16 t .. 16 t + 15 (lanes >= 32: dims 64 ..)
        if (lane == 0) ((float*)(kc + kv8_scale_off(S_max, KV)))[(size_t)pos * KV + kh] = sc;
    } else {
        const int kh = hd - H - KV;
        const float a = x[2 * lane], b = x[2 * lane + 1];
        const float sc = kv8_scale(wave_max(fmaxf(fabsf(a), fabsf(b))));
        const uint32_t h = kv8_pk4(a / sc, b / sc, 0.f, 0.f);
        uint8_t* col = vtc + ((size_t)kh * 128 + 2 * lane) * S_max + pos;
        col[0] = (uint8_t)(h & 0xff);
        col[S_max] = (uint8_t)((h >> 8) & 0xff);
        if (lane == 0) ((float*)(vtc + kv8_scale_off(S_max, KV)))[(size_t)kh * S_max + pos] = sc;
    }
}
struct Kv8PlainRow { const float* p; __device__ float operator[](int i) const { return p[i]; } };
// the q|k|v product's UNSUMMED split-K slabs ([n][rows][(H + 2 KV) dh], sm_linear_leave_slabs), summed in slab order: the arithmetic of the reduce launch this replaces
struct Kv8SlabRow { const float* p; int n; size_t st;
                    __device__ float operator[](int i) const { if (n <= 0) return p[i]; float v = 0.f; for (int s_ = 0; s_ < n; ++s_) v += p[(size_t)s_ * st + i]; return v; } };

// grid (token, head slot): slots as in rope_kv_kernel (q heads, k heads, v heads)
__global__ __launch_bounds__(64) void rope_kv_fp8_kernel(const float* __restrict__ qkv, int pos0, int H, int KV, const float* __restrict__ cos_tab,
                                                         const float* __restrict__ sin_tab, bf16_t* __restrict__ q, uint8_t* __restrict__ kc,
                                                         uint8_t* __restrict__ vtc, int S_max) {
    const int t = blockIdx.x, hd = blockIdx.y;
    const Kv8PlainRow x = {qkv + ((size_t)t * (H + 2 * KV) + hd) * 128};
    rope_kv_fp8_row(x, pos0 + t, hd, H, KV, cos_tab, sin_tab, q + ((size_t)t * H + (hd < H ? hd : 0)) * 128, kc, vtc, S_max);
}
// S streams x one token each (the batched decode step): row t = stream t at ITS position, appended to ITS caches (device-side pointer table)
__global__ __launch_bounds__(64) void rope_kv_fp8_seg_kernel(const float* __restrict__ qkv, int H, int KV, const float* __restrict__ cos_tab,
                                                             const float* __restrict__ sin_tab, bf16_t* __restrict__ q, SmDecodeSegTab tab, int S_max,
                                                             int nslab, size_t sstride) {
    const int t = blockIdx.x, hd = blockIdx.y;
    const Kv8SlabRow x = {qkv + ((size_t)t * (H + 2 * KV) + hd) * 128, nslab, sstride};
    rope_kv_fp8_row(x, tab.pos0[t] + tab.step, hd, H, KV, cos_tab, sin_tab, q + ((size_t)t * H + (hd < H ? hd : 0)) * 128, (uint8_t*)tab.kc[t], (uint8_t*)tab.vtc[t], S_max);
}

// ---- a chunk of rows (prefill, n >= 32): one 256-thread block per (64 tokens, head slot), four lanes per token as in rope_kv_tile_kernel.  q / k heads: a lane
// rotates 16 (d, d + 64) pairs with 16-byte loads; a K head's amax meets over the token's four lanes (two xor-shuffles) and each lane stores its 2 x 16 codes as
// two 16-byte stores.  v heads: a lane holds 32 dims of its token, the amax is taken over the four lanes BEFORE the transpose, the codes cross a [128][64] byte
// tile in LDS and leave as 64 consecutive positions of one dim per wave-store.  Same arithmetic as the row form above: identical bytes.
// (the body, shared with the ragged form below: rows t0 .. t0 + 63 of a run of n rows that starts at qkv / q and sits at positions pos0 ..)
__device__ __forceinline__ void rope_kv_fp8_tile(const float* __restrict__ qkv, int n, int pos0, int t0, int hd, int H, int KV, const float* __restrict__ cos_tab,
                                                 const float* __restrict__ sin_tab, bf16_t* __restrict__ q, uint8_t* __restrict__ kc, uint8_t* __restrict__ vtc,
                                                 int S_max, uint8_t (&tile)[128][64 + 4]) {
    constexpr int DH = 128, HALF = 64;
    const int tid = threadIdx.x;
    const int tl = tid >> 2, part = tid & 3;
    const bool live = t0 + tl < n;
    const int t = live ? t0 + tl : n - 1;              // a dead lane redoes the last row (the shuffles below need all four lanes of a token) and stores nothing
    const int pos = pos0 + t;
    const int ld = (H + 2 * KV) * DH;
    if (hd < H + KV) {
        const float* x = qkv + (size_t)t * ld + (size_t)hd * DH + part * 16;
        const float* cp = cos_tab + (size_t)pos * HALF + part * 16;
        const float* sp = sin_tab + (size_t)pos * HALF + part * 16;
        float r0[16], r1[16];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const f32x4 a = *(const f32x4*)(x + v * 4), b = *(const f32x4*)(x + HALF + v * 4);
            const f32x4 c = *(const f32x4*)(cp + v * 4), s_ = *(const f32x4*)(sp + v * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                r0[v * 4 + e] = a[e] * c[e] - b[e] * s_[e]; r1[v * 4 + e] = b[e] * c[e] + a[e] * s_[e];
                if (hd >= H) kv8_rope_pair(a[e], b[e], c[e], s_[e], r0[v * 4 + e], r1[v * 4 + e]);
            }
        }
        if (hd < H) {
            if (!live) return;
            bf16_t* dst = q + ((size_t)t * H + hd) * DH + part * 16;
            uint32_t o0[8], o1[8];
#pragma unroll
            for (int v = 0; v < 8; ++v) { o0[v] = pack2bf(r0[2 * v], r0[2 * v + 1]); o1[v] = pack2bf(r1[2 * v], r1[2 * v + 1]); }
            *(u32x4*)(dst) = u32x4{o0[0], o0[1], o0[2], o0[3]};
            *(u32x4*)(dst + 8) = u32x4{o0[4], o0[5], o0[6], o0[7]};
            *(u32x4*)(dst + HALF) = u32x4{o1[0], o1[1], o1[2], o1[3]};
            *(u32x4*)(dst + HALF + 8) = u32x4{o1[4], o1[5], o1[6], o1[7]};
            return;
        }
        float am = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) am = fmaxf(am, fmaxf(fabsf(r0[e]), fabsf(r1[e])));
        am = fmaxf(am, __shfl_xor(am, 1, 64));
        am = fmaxf(am, __shfl_xor(am, 2, 64));
        const float sc = kv8_scale(am);
        if (!live) return;
        uint32_t c0[4], c1[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            c0[v] = kv8_pk4(r0[4 * v] / sc, r0[4 * v + 1] / sc, r0[4 * v + 2] / sc, r0[4 * v + 3] / sc);
            c1[v] = kv8_pk4(r1[4 * v] / sc, r1[4 * v + 1] / sc, r1[4 * v + 2] / sc, r1[4 * v + 3] / sc);
        }
        const int kh = hd - H;
        uint8_t* row = kc + ((size_t)pos * KV + kh) * DH + part * 16;
        *(u32x4*)row = u32x4{c0[0], c0[1], c0[2], c0[3]};
        *(u32x4*)(row + HALF) = u32x4{c1[0], c1[1], c1[2], c1[3]};
        if (part == 0) ((float*)(kc + kv8_scale_off(S_max, KV)))[(size_t)pos * KV + kh] = sc;
        return;
    }
    const int kh = hd - H - KV;
    {
        const float* x = qkv + (size_t)t * ld + (size_t)hd * DH + part * 32;
        f32x4 a[8];
        float am = 0.f;
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            a[v] = *(const f32x4*)(x + v * 4);
            am = fmaxf(am, fmaxf(fmaxf(fabsf(a[v][0]), fabsf(a[v][1])), fmaxf(fabsf(a[v][2]), fabsf(a[v][3]))));
        }
        am = fmaxf(am, __shfl_xor(am, 1, 64));
        am = fmaxf(am, __shfl_xor(am, 2, 64));
        const float sc = kv8_scale(am);
        if (live) {
#pragma unroll
            for (int v = 0; v < 8; ++v) {
                const uint32_t w = kv8_pk4(a[v][0] / sc, a[v][1] / sc, a[v][2] / sc, a[v][3] / sc);
#pragma unroll
                for (int e = 0; e < 4; ++e) tile[part * 32 + v * 4 + e][tl] = (uint8_t)((w >> (8 * e)) & 0xff);
            }
            if (part == 0) ((float*)(vtc + kv8_scale_off(S_max, KV)))[(size_t)kh * S_max + pos] = sc;
        }
    }
    __syncthreads();
    const int lane = tid & 63, w = tid >> 6;
    if (t0 + lane < n) {
        uint8_t* dstv = vtc + ((size_t)kh * DH + w * 32) * S_max + pos0 + t0 + lane;
#pragma unroll 8
        for (int e = 0; e < 32; ++e) dstv[(size_t)e * S_max] = tile[w * 32 + e][lane];
    }
}
__global__ __launch_bounds__(256) void rope_kv_fp8_tile_kernel(const float* __restrict__ qkv, int n, int pos0, int H, int KV, const float* __restrict__ cos_tab,
                                                               const float* __restrict__ sin_tab, bf16_t* __restrict__ q, uint8_t* __restrict__ kc,
                                                               uint8_t* __restrict__ vtc, int S_max) {
    __shared__ uint8_t tile[128][64 + 4];
    rope_kv_fp8_tile(qkv, n, pos0, blockIdx.x * 64, blockIdx.y, H, KV, cos_tab, sin_tab, q, kc, vtc, S_max, tile);
}
// ---- the rows of S streams in one matrix (sm_group_llm_prefill): seg [S][4] = (row0, n, pos0, cap) per stream, tiles [n_tiles][2] = (stream, first row of a
// 64-row tile of that stream's rows) -- the tables of sm_rope_kv_append_ragged.  One block per (tile, head slot) runs the tile body above on its stream's run of
// rows, at the stream's positions, into the stream's buffers with the stream's cap (V^T pitch, start of the scales): the bytes of sm_rope_kv_append_fp8 per
// stream, also for streams of fewer than 32 rows (where that call takes the row kernel: identical bytes).  Nothing outside [pos0, pos0 + n) is written.
__global__ __launch_bounds__(256) void rope_kv_fp8_ragged_kernel(const float* __restrict__ qkv, const int32_t* __restrict__ seg, const int32_t* __restrict__ tiles,
                                                                 int H, int KV, const float* __restrict__ cos_tab, const float* __restrict__ sin_tab,
                                                                 bf16_t* __restrict__ q, void* const* __restrict__ kc_tab, void* const* __restrict__ vtc_tab) {
    __shared__ uint8_t tile[128][64 + 4];
    const int sidx = tiles[2 * blockIdx.x], t0 = tiles[2 * blockIdx.x + 1];
    const int row0 = seg[4 * sidx], n = seg[4 * sidx + 1], pos0 = seg[4 * sidx + 2], cap = seg[4 * sidx + 3];
    rope_kv_fp8_tile(qkv + (size_t)row0 * (H + 2 * KV) * 128, n, pos0, t0, blockIdx.y, H, KV, cos_tab, sin_tab, q + (size_t)row0 * H * 128, (uint8_t*)kc_tab[sidx],
                     (uint8_t*)vtc_tab[sidx], cap, tile);
}

static int kv8_check(const char* who, int dh, int KV, int H, int S_max) {
    SM_REQUIRE(dh == 128, "%s: the fp8 K / V cache takes head_dim 128 only (got %d)", who, dh);
    SM_REQUIRE(KV > 0 && H > 0 && H % KV == 0 && S_max > 0 && S_max % 64 == 0, "%s: H %% KV, S_max %% 64", who);
    return SM_OK;
}
extern "C" int sm_rope_kv_append_fp8(const float* qkv, int n, int pos0, int H, int KV, int dh, const float* cos_tab, const float* sin_tab, void* q,
                                     void* kcache, void* vtcache, int S_max, void* stream) {
    SM_REQUIRE(qkv && q && cos_tab && sin_tab && kcache && vtcache && n > 0 && pos0 >= 0 && pos0 + n <= S_max, "sm_rope_kv_append_fp8: bad args (pos0=%d n=%d S_max=%d)", pos0, n, S_max);
    int rc = kv8_check("sm_rope_kv_append_fp8", dh, KV, H, S_max);
    if (rc) return rc;
    SM_REQUIRE(((uintptr_t)kcache & 15) == 0 && ((uintptr_t)vtcache & 15) == 0 && ((uintptr_t)q & 15) == 0, "sm_rope_kv_append_fp8: q and the caches must be 16-byte aligned");
    if (n >= 32 && ((uintptr_t)qkv & 15) == 0 && ((uintptr_t)cos_tab & 15) == 0 && ((uintptr_t)sin_tab & 15) == 0)
        rope_kv_fp8_tile_kernel<<<dim3((n + 63) / 64, H + 2 * KV), 256, 0, (hipStream_t)stream>>>(qkv, n, pos0, H, KV, cos_tab, sin_tab, (bf16_t*)q, (uint8_t*)kcache,
                                                                                                (uint8_t*)vtcache, S_max);
    else
        rope_kv_fp8_kernel<<<dim3(n, H + 2 * KV), 64, 0, (hipStream_t)stream>>>(qkv, pos0, H, KV, cos_tab, sin_tab, (bf16_t*)q, (uint8_t*)kcache, (uint8_t*)vtcache, S_max);
    SM_LAUNCH_CHECK();
    return SM_OK;
}
extern "C" int sm_rope_kv_append_fp8_ragged(const float* qkv, const int32_t* seg_dev, const int32_t* tiles_dev, int n_tiles, int H, int KV, const float* cos_tab,
                                            const float* sin_tab, void* q, void* const* kc_tab_dev, void* const* vtc_tab_dev, void* stream) {
    SM_REQUIRE(qkv && seg_dev && tiles_dev && cos_tab && sin_tab && q && kc_tab_dev && vtc_tab_dev && n_tiles > 0 && H > 0 && KV > 0 && H % KV == 0, "sm_rope_kv_append_fp8_ragged: bad args");
    SM_REQUIRE((((uintptr_t)qkv | (uintptr_t)q | (uintptr_t)cos_tab | (uintptr_t)sin_tab) & 15) == 0, "sm_rope_kv_append_fp8_ragged: qkv, q and the RoPE tables must be 16-byte aligned");
    rope_kv_fp8_ragged_kernel<<<dim3(n_tiles, H + 2 * KV), 256, 0, (hipStream_t)stream>>>(qkv, seg_dev, tiles_dev, H, KV, cos_tab, sin_tab, (bf16_t*)q, kc_tab_dev, vtc_tab_dev);
    SM_LAUNCH_CHECK();
    return SM_OK;
}
int sm_rope_kv_append_fp8_seg_tab(const float* qkv, int S, int H, int KV, int dh, const float* cos_tab, const float* sin_tab, void* q, const SmDecodeSegTab& tab,
                                  int S_max, void* stream, int nslab, size_t slab_stride) {
    SM_REQUIRE(qkv && q && cos_tab && sin_tab && S > 0 && tab.kc && tab.vtc && tab.pos0 && nslab >= 0 && nslab <= 64, "sm_rope_kv_append_fp8_seg_tab: bad args");
    int rc = kv8_check("sm_rope_kv_append_fp8_seg_tab", dh, KV, H, S_max);
    if (rc) return rc;
    rope_kv_fp8_seg_kernel<<<dim3(S, H + 2 * KV), 64, 0, (hipStream_t)stream>>>(qkv, H, KV, cos_tab, sin_tab, (bf16_t*)q, tab, S_max, nslab, slab_stride);
    SM_LAUNCH_CHECK();
    return SM_OK;
}

// ---- expansion for chunk attention: codes * scale -> bf16, keys [k_lo, k_hi), into scratch buffers of the bf16 cache's layout (K [S_max][KV * 128],
// V^T [KV * 128][S_max]).  One lane = 16 codes: a 16-byte load, two 16-byte stores.  blockIdx.y = 0: K (a lane's 16 codes are 16 dims of one key: one scale);
// 1: V^T (16 consecutive positions of one dim: four 16-byte scale loads; the chunks at the range's ends store their in-range elements one by one, so nothing
// outside [k_lo, k_hi) is written).
__device__ __forceinline__ void kv8_unpack16(u32x4 c, float (&f)[16]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(c[w], false), b = __builtin_amdgcn_cvt_pk_f32_fp8(c[w], true);
        f[4 * w] = a[0]; f[4 * w + 1] = a[1]; f[4 * w + 2] = b[0]; f[4 * w + 3] = b[1];
    }
}
__global__ __launch_bounds__(256) void kv_fp8_expand_kernel(const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vtc, int k_lo, int k_hi, int KV, int S_max,
                                                            bf16_t* __restrict__ k_out, bf16_t* __restrict__ vt_out) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    float f[16];
    if (blockIdx.y == 0) {
        const int cpr = KV * 8;                                   // 16-code chunks per key row
        if (idx >= (long)(k_hi - k_lo) * cpr) return;
        const int key = k_lo + (int)(idx / cpr), ch = (int)(idx % cpr);
        const float sc = ((const float*)(kc + kv8_scale_off(S_max, KV)))[(size_t)key * KV + (ch >> 3)];
        kv8_unpack16(*(const u32x4*)(kc + (size_t)key * KV * 128 + ch * 16), f);
        bf16_t* dst = k_out + (size_t)key * KV * 128 + ch * 16;
        *(u32x4*)dst = u32x4{pack2bf(f[0] * sc, f[1] * sc), pack2bf(f[2] * sc, f[3] * sc), pack2bf(f[4] * sc, f[5] * sc), pack2bf(f[6] * sc, f[7] * sc)};
        *(u32x4*)(dst + 8) = u32x4{pack2bf(f[8] * sc, f[9] * sc), pack2bf(f[10] * sc, f[11] * sc), pack2bf(f[12] * sc, f[13] * sc), pack2bf(f[14] * sc, f[15] * sc)};
        return;
    }
    const int c_lo = k_lo >> 4, ncol = ((k_hi + 15) >> 4) - c_lo;  // 16-position chunks that touch the range
    if (idx >= (long)KV * 128 * ncol) return;
    const int row = (int)(idx / ncol), p0 = (c_lo + (int)(idx % ncol)) * 16;
    const float* sp = (const float*)(vtc + kv8_scale_off(S_max, KV)) + (size_t)(row >> 7) * S_max + p0;
    float s[16];
#pragma unroll
    for (int w = 0; w < 4; ++w) { const f32x4 v = *(const f32x4*)(sp + 4 * w); s[4 * w] = v[0]; s[4 * w + 1] = v[1]; s[4 * w + 2] = v[2]; s[4 * w + 3] = v[3]; }
    kv8_unpack16(*(const u32x4*)(vtc + (size_t)row * S_max + p0), f);
    bf16_t* dst = vt_out + (size_t)row * S_max + p0;
    if (p0 >= k_lo && p0 + 16 <= k_hi) {
        *(u32x4*)dst = u32x4{pack2bf(f[0] * s[0], f[1] * s[1]), pack2bf(f[2] * s[2], f[3] * s[3]), pack2bf(f[4] * s[4], f[5] * s[5]), pack2bf(f[6] * s[6], f[7] * s[7])};
        *(u32x4*)(dst + 8) = u32x4{pack2bf(f[8] * s[8], f[9] * s[9]), pack2bf(f[10] * s[10], f[11] * s[11]), pack2bf(f[12] * s[12], f[13] * s[13]), pack2bf(f[14] * s[14], f[15] * s[15])};
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (p0 + e >= k_lo && p0 + e < k_hi) dst[e] = (bf16_t)f2bf(f[e] * s[e]);
    }
}
extern "C" int sm_kv_fp8_expand(const void* kcache, const void* vtcache, int k_lo, int k_hi, int KV, int dh, int S_max, void* k_out, void* vt_out, void* stream) {
    SM_REQUIRE(kcache && vtcache && k_out && vt_out && k_lo >= 0 && k_lo < k_hi && k_hi <= S_max, "sm_kv_fp8_expand: bad args (k_lo=%d k_hi=%d S_max=%d)", k_lo, k_hi, S_max);
    int rc = kv8_check("sm_kv_fp8_expand", dh, KV, KV, S_max);
    if (rc) return rc;
    SM_REQUIRE((((uintptr_t)kcache | (uintptr_t)vtcache | (uintptr_t)k_out | (uintptr_t)vt_out) & 15) == 0, "sm_kv_fp8_expand: buffers must be 16-byte aligned");
    const long nk_items = (long)(k_hi - k_lo) * KV * 8, nv_items = (long)KV * 128 * (((k_hi + 15) >> 4) - (k_lo >> 4));
    const long items = nk_items > nv_items ? nk_items : nv_items;
    kv_fp8_expand_kernel<<<dim3((unsigned)((items + 255) / 256), 2), 256, 0, (hipStream_t)stream>>>((const uint8_t*)kcache, (const uint8_t*)vtcache, k_lo, k_hi, KV, S_max,
                                                                                                  (bf16_t*)k_out, (bf16_t*)vt_out);
    SM_LAUNCH_CHECK();
    return SM_OK;
}
