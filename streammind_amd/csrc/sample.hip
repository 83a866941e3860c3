// Device-side temperature / top-k / top-p sampling of one row of fp32 logits (sm_sample_rows, the sampled decode tail of sm_llm_decode and the
// sampled stage of sm_group_llm_decode).  Replaces the host-side torch.sort + softmax + cumsum + multinomial of HF generate(do_sample=True)
// (serve/model_worker.py passes temperature / top_p), which cost a device-to-host sync and a handful of launches per token.
//
// THE RULE.  Row l[0..V), parameters (temperature T > 0, top_k >= 0, 0 < top_p <= 1), HF's warper order (temperature, top-k, top-p):
//   x_v = (l_v - max l) / T,  e_v = exp(x_v),  p_v = e_v / sum e;   above(v) = sum of p_w over l_w > l_v (strictly);  rank(v) = #{w : l_w > l_v}
//   v is KEPT iff (top_k == 0 or rank(v) < top_k) and (top_p >= 1 or above(v) < top_p)
// = TopPLogitsWarper with min_tokens_to_keep = 1 made independent of the sort order: tokens with EQUAL logits are kept or dropped together (the only
// difference from HF, and only at an exact tie on the boundary; -0.0 and +0.0 are equal).  Top-p uses the softmax over the FULL row, as the host sampler
// (StreamMindModel._sample) does; with top_k > 0 HF renormalises over the top-k survivors first -- this rule does not.  The top token is always kept.
// With a uniform u in [0, 1) and Z = sum of e_v over the kept tokens, the chosen token is the first v IN TOKEN-ID ORDER whose inclusive kept-CDF exceeds
// u * Z (if rounding runs off the end: the last kept token with mass).  -inf logits have mass 0 and are never chosen; rows with NaN or +inf are unsupported.
// u comes from the caller or from Philox4x32-10 (the published round function, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85):
// key = (seed low word, seed high word), counter = (pos low, pos high, 0, 0), u = (out[0] >> 8) * 2^-24, pos = the absolute context index the chosen token
// will occupy -- so a stream's ids do not depend on how a reply is cut into n_steps calls, on single versus batched decode, or on KV prefix reuse.
//
// THE KERNEL.  One 1024-thread block per row.
//  * Row resident in LDS: the row is read from HBM / L2 once into dynamic LDS (V * 4 bytes: 125 KB for Mistral's 32 000, beside 24.4 KB of histograms,
//    inside gfx950's 160 KB per block; the opt-in limit is set with hipFuncSetAttribute against what the device reports).  Rows that do not fit take the
//    same code with the row pointer left in global memory (the L2-resident row is re-read per pass); the choice is by size only.
//  * Mass is FIXED POINT: q_v = floor(e_v * 2^40) in 64-bit integers (e_v <= 1, so a row of 2^17 tokens sums below 2^57; a term's quantisation is 2^-40 of
//    the top token's mass, 3e-8 of the row at most over 32 000 tokens, and tokens below e^-27.7 carry no mass).  Every sum below -- histogram bins, their
//    scan, the CDF -- is an INTEGER sum, so the boundary, Z and the token are bit-reproducible whatever order the LDS atomics land in, and identical
//    between the three entry shapes.  e_v = v_exp_f32((l_v - max) * (1 / T) * log2 e): 1 ulp, ~|x| 2^-24 relative from the argument's rounding.
//  * Selection without a sort: l_v -> monotone 32-bit key; the boundary key B = the smallest key k with #{key > k} < top_k and mass{key > k} < top_p * total
//    is found by a radix select in three passes (11 / 11 / 10 bits).  A pass histograms mass (ds_add_u64) and count (ds_add_u32) of the keys that match the
//    digits decided so far, a block-wide suffix scan over the 2048 bins (two bins per thread, wave scan by __shfl_down, one LDS exchange across the 16 waves)
//    gives what lies above every bin, and the one thread whose bin is the lowest that still satisfies both conditions publishes the digit.  The first pass
//    also yields the row total.  kept = {key >= B}; Z and the kept count fall out of the last pass.
//  * Draw: thread t owns the contiguous ids [t * per, (t + 1) * per) with per ODD (a power-of-two stride would put all 64 lanes on one LDS bank); thread-local
//    kept mass, wave inclusive scan by __shfl_up, one LDS exchange, and the owning thread walks its run to the first id whose CDF exceeds floor(u * Z).
//  * A row whose rule is greedy takes the arg-max branch of the same launch (first maximum wins, as torch.argmax and the arg-max kernels).
// Three entry shapes over the one device function: rows of a dense matrix (rules by value, 32 rows per launch), the fused decode tail (choose + write the
// pending token + emit the id + gather the embedding row: the sampled twin of argmax_emit_embed_kernel) and the segmented form of the batched decode
// (per-stream token words and rules by value up to 32 streams, a device-side table beyond).
#include "common.h"
#include "host.h"

#define SMP_THREADS 1024
#define SMP_WAVES (SMP_THREADS / 64)
#define SMP_BINS 2048

struct SmpShared {
    unsigned long long hm[SMP_BINS];     // mass per bin (fixed point)
    uint32_t hc[SMP_BINS];               // keys per bin
    unsigned long long wm[SMP_WAVES];
    uint32_t wc[SMP_WAVES];
    float wf[SMP_WAVES];
    int wi[SMP_WAVES];
    unsigned long long total, sel_m, bin_m;
    uint32_t sel_c, bin_c, sel_d;
    int winner;
    float mx;
};

__device__ __forceinline__ uint32_t smp_key(float l) {
    l += 0.0f;                                         // -0.0 -> +0.0: equal logits share a key
    const uint32_t u = __float_as_uint(l);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long smp_mass(float l, float mx, float inv_t) {
#pragma clang fp contract(off)
    const float e = __builtin_amdgcn_exp2f((l - mx) * inv_t * 1.44269504088896341f);
    return (unsigned long long)(e * 1099511627776.0f);         // * 2^40, exact; e <= 1
}
__device__ __forceinline__ unsigned long long shfl_down64(unsigned long long x, int o) {
    return ((unsigned long long)(uint32_t)__shfl_down((int)(x >> 32), o, 64) << 32) | (uint32_t)__shfl_down((int)(uint32_t)x, o, 64);
}
__device__ __forceinline__ unsigned long long shfl_up64(unsigned long long x, int o) {
    return ((unsigned long long)(uint32_t)__shfl_up((int)(x >> 32), o, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)x, o, 64);
}
// Philox4x32-10, first output word
__device__ __forceinline__ uint32_t smp_philox(uint64_t seed, uint64_t pos) {
    uint32_t c0 = (uint32_t)pos, c1 = (uint32_t)(pos >> 32), c2 = 0, c3 = 0, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0, hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}

// first maximum of the row (lowest index wins ties), known to every thread on return
__device__ __forceinline__ int smp_argmax(const float* __restrict__ g, int V, SmpShared& sh) {
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int v = threadIdx.x; v < V; v += SMP_THREADS) {
        const float t = g[v];
        if (t > best) { best = t; idx = v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(idx, o, 64);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sh.wf[w] = best; sh.wi[w] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < SMP_WAVES; ++k)
            if (sh.wf[k] > best || (sh.wf[k] == best && sh.wi[k] < idx)) { best = sh.wf[k]; idx = sh.wi[k]; }
        sh.winner = idx;
    }
    __syncthreads();
    return sh.winner;
}

// the rule above on one row; RES: the row is copied to `lds_row` first and every pass reads it there.  Returns the token in every thread.
template <bool RES>
__device__ __forceinline__ int smp_sample(const float* __restrict__ g, int V, const SmSampleRule& r, bool have_u, float u, float* lds_row, SmpShared& sh,
                                          uint32_t* kept_n, float* kept_mass) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const float* row = RES ? lds_row : g;
    // ---- the row's maximum (and its copy into LDS)
    float mx = -INFINITY;
    for (int v = tid; v < V; v += SMP_THREADS) {
        const float l = g[v];
        if (RES) lds_row[v] = l;
        mx = fmaxf(mx, l);
    }
    mx = wave_max(mx);
    if (lane == 0) sh.wf[w] = mx;
    if (tid == 0) { sh.sel_d = 0; sh.winner = 0; }           // a row outside the contract (NaN) must still leave an id inside [0, V)
    __syncthreads();
    mx = sh.wf[0];
#pragma unroll
    for (int k = 1; k < SMP_WAVES; ++k) mx = fmaxf(mx, sh.wf[k]);
    const float inv_t = r.inv_t;
    // ---- radix select of the boundary key
    const uint32_t K = r.top_k > 0 ? (uint32_t)r.top_k : 0xffffffffu;
    unsigned long long P = ~0ull, total = 0, acc_m = 0;
    uint32_t acc_c = 0, prefix = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; ++pass) {
        sh.hm[2 * tid] = 0; sh.hm[2 * tid + 1] = 0; sh.hc[2 * tid] = 0; sh.hc[2 * tid + 1] = 0;
        __syncthreads();
        const int dshift = pass == 0 ? 21 : pass == 1 ? 10 : 0, pshift = pass == 1 ? 21 : 10;
        const uint32_t dmask = pass == 2 ? 1023u : 2047u;
        for (int v = tid; v < V; v += SMP_THREADS) {
            const float l = row[v];
            const uint32_t key = smp_key(l);
            if (pass > 0 && (key >> pshift) != prefix) continue;
            const uint32_t b = (key >> dshift) & dmask;
            atomicAdd(&sh.hm[b], smp_mass(l, mx, inv_t));
            atomicAdd(&sh.hc[b], 1u);
        }
        __syncthreads();
        // suffix scan over the bins: sm / sc = mass / count of the bins >= 2 * tid
        const unsigned long long m0 = sh.hm[2 * tid], m1 = sh.hm[2 * tid + 1];
        const uint32_t c0 = sh.hc[2 * tid], c1 = sh.hc[2 * tid + 1];
        unsigned long long sm = m0 + m1;
        uint32_t sc = c0 + c1;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned long long ym = shfl_down64(sm, o);
            const uint32_t yc = (uint32_t)__shfl_down((int)sc, o, 64);
            if (lane + o < 64) { sm += ym; sc += yc; }
        }
        if (lane == 0) { sh.wm[w] = sm; sh.wc[w] = sc; }
        __syncthreads();
        for (int k = w + 1; k < SMP_WAVES; ++k) { sm += sh.wm[k]; sc += sh.wc[k]; }
        if (pass == 0) {
            if (tid == 0) sh.total = sm;
            __syncthreads();
            total = sh.total;
            if (r.top_p < 1.0f) P = (unsigned long long)ceil((double)r.top_p * (double)total);       // integer a: a < top_p * total <=> a < ceil(top_p * total)
        }
        // cond(d): what lies above bin d (plus what the decided digits left above) satisfies both bounds; true at the top, monotone; the digit is the lowest d it holds for
        const unsigned long long a1m = acc_m + (sm - m0 - m1), a0m = a1m + m1, am = a0m + m0;
        const uint32_t a1c = acc_c + (sc - c0 - c1), a0c = a1c + c1, ac = a0c + c0;
        const bool ok1 = a1c < K && a1m < P, ok0 = a0c < K && a0m < P, okm = ac < K && am < P;
        if (ok1 && !ok0) { sh.sel_d = 2 * tid + 1; sh.sel_m = a1m; sh.sel_c = a1c; sh.bin_m = m1; sh.bin_c = c1; }
        else if (ok0 && (tid == 0 || !okm)) { sh.sel_d = 2 * tid; sh.sel_m = a0m; sh.sel_c = a0c; sh.bin_m = m0; sh.bin_c = c0; }
        __syncthreads();
        prefix = (prefix << (pass == 2 ? 10 : 11)) | sh.sel_d;
        acc_m = sh.sel_m; acc_c = sh.sel_c;
    }
    const uint32_t B = prefix;
    const unsigned long long Z = acc_m + sh.bin_m;           // mass / number of the keys >= B
    *kept_n = acc_c + sh.bin_c;
    *kept_mass = (float)((double)Z / (double)total);
    // ---- draw
    if (!have_u) u = (float)(smp_philox(r.seed, (uint64_t)r.pos) >> 8) * (1.0f / 16777216.0f);
    unsigned long long target = (unsigned long long)((double)u * (double)Z);
    if (target >= Z) target = Z - 1;
    const int per = ((V + SMP_THREADS - 1) / SMP_THREADS) | 1;
    const long long s0 = (long long)tid * per;
    const int v0 = s0 < V ? (int)s0 : V, v1 = s0 + per < V ? (int)(s0 + per) : V;
    unsigned long long loc = 0;
    for (int v = v0; v < v1; ++v) {
        const float l = row[v];
        if (smp_key(l) >= B) loc += smp_mass(l, mx, inv_t);
    }
    unsigned long long inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = shfl_up64(inc, o);
        if (lane >= o) inc += y;
    }
    __syncthreads();                                         // sh.wm / sh.bin_* of the last pass have been read by everyone
    if (lane == 63) sh.wm[w] = inc;
    __syncthreads();
    for (int k = 0; k < w; ++k) inc += sh.wm[k];
    unsigned long long c = inc - loc;
    if (c <= target && target < inc) {                       // exactly one thread: the scan's total is Z
        int tok = v0;
        for (int v = v0; v < v1; ++v) {
            const float l = row[v];
            if (smp_key(l) >= B) { c += smp_mass(l, mx, inv_t); if (c > target) { tok = v; break; } }
        }
        sh.winner = tok;
    }
    __syncthreads();
    return sh.winner;
}

template <class PACK> __device__ __forceinline__ SmSampleRule smp_rule(const PACK& pk, int m) { return pk.r[m]; }
template <> __device__ __forceinline__ SmSampleRule smp_rule<SmSampleTab>(const SmSampleTab& pk, int m) { SmSampleRule r = pk.r[m]; r.pos += pk.step; return r; }

// tail: the decode step's extras (all optional) -- the id also goes to *emit, and its embedding row to emb[0..D)
struct SmSampleTail { int32_t* emit; const bf16_t* table; int D; float* emb; int f16; };

template <class PACK, bool RES>
__global__ __launch_bounds__(SMP_THREADS) void sample_kernel(const float* __restrict__ lg, int V, int ld, PACK pk, const float* __restrict__ u_opt,
                                                             int32_t* __restrict__ kept_out, float* __restrict__ mass_out, SmSampleTail tail) {
    extern __shared__ float smp_row[];
    __shared__ SmpShared sh;
    const int m = blockIdx.x;
    const SmSampleRule r = smp_rule(pk, m);
    const float* g = lg + (size_t)m * ld;
    uint32_t kept_n = 1;
    float kept_mass = 0.f;
    int tok;
    if (r.greedy) tok = smp_argmax(g, V, sh);
    else tok = smp_sample<RES>(g, V, r, u_opt != nullptr, u_opt ? u_opt[m] : 0.f, smp_row, sh, &kept_n, &kept_mass);
    if ((unsigned)tok >= (unsigned)V) tok = 0;               // (an all -inf / NaN row: unsupported, but never an index outside the embedding table)
    if (threadIdx.x == 0) {
        *pk.tok[m] = tok;
        if (tail.emit) *tail.emit = tok;
        if (kept_out) kept_out[m] = (int32_t)kept_n;
        if (mass_out) mass_out[m] = kept_mass;
    }
    if (tail.emb)
        for (int c = threadIdx.x; c < tail.D; c += SMP_THREADS)
            tail.emb[c] = tail.f16 ? h2f(tail.table[(size_t)tok * tail.D + c]) : bf2f(tail.table[(size_t)tok * tail.D + c]);
}

// ------------------------------------------------------------------------------------------------ host
// rows of at most this many columns stay in LDS: the per-block maximum the device reports less the kernel's static LDS; 0 on error
static int smp_resident_max(size_t* dyn_limit) {
    static int vmax = -1;
    static size_t limit = 0;
    if (vmax < 0) {
        int dev = 0, lds = 0;
        hipFuncAttributes fa;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess ||
            hipFuncGetAttributes(&fa, (const void*)sample_kernel<SmSamplePack, true>) != hipSuccess) { (void)hipGetLastError(); return 0; }
        const long room = (long)lds - (long)fa.sharedSizeBytes - 256;
        limit = room > 0 ? (size_t)room : 0;
        if (limit > 65536) {
            if (hipFuncSetAttribute((const void*)sample_kernel<SmSamplePack, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) != hipSuccess ||
                hipFuncSetAttribute((const void*)sample_kernel<SmSampleTab, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)limit) != hipSuccess) {
                (void)hipGetLastError();
                limit = 65536 - fa.sharedSizeBytes - 256;
            }
        }
        vmax = (int)(limit / 4);
    }
    if (dyn_limit) *dyn_limit = limit;
    return vmax;
}

template <class PACK>
static int smp_launch(const float* logits, int M, int V, int ld, const PACK& pk, const float* u, int32_t* kept, float* mass, const SmSampleTail& tail, void* stream) {
    const bool res = V <= smp_resident_max(nullptr);
    if (res) sample_kernel<PACK, true><<<M, SMP_THREADS, (size_t)V * 4, (hipStream_t)stream>>>(logits, V, ld, pk, u, kept, mass, tail);
    else sample_kernel<PACK, false><<<M, SMP_THREADS, 0, (hipStream_t)stream>>>(logits, V, ld, pk, u, kept, mass, tail);
    SM_LAUNCH_CHECK();
    return SM_OK;
}

int sm_sampling_check(const sm_sampling_t* p, const char* who) {
    SM_REQUIRE(p->temperature > 0.f && p->top_p > 0.f && p->top_k >= 0, "%s: temperature %g must be > 0, top_p %g > 0, top_k %d >= 0", who, (double)p->temperature,
               (double)p->top_p, p->top_k);
    return SM_OK;
}
SmSampleRule sm_sample_rule(const sm_sampling_t* p, int64_t pos) {
    SmSampleRule r;
    r.greedy = !p || !(p->temperature > 0.f);
    r.inv_t = r.greedy ? 1.f : 1.0f / p->temperature;
    r.top_p = r.greedy ? 1.f : p->top_p;
    r.top_k = r.greedy ? 0 : p->top_k;
    r.seed = r.greedy ? 0 : p->seed;
    r.pos = pos;
    return r;
}

extern "C" int sm_sample_rows(const float* logits, int M, int V, int ld, const sm_sampling_t* params_host, int n_params, const int64_t* pos_host,
                              const float* u_dev_opt, int32_t* tok_out, int32_t* kept_out_opt, float* kept_mass_out_opt, void* stream) {
    SM_REQUIRE(logits && params_host && tok_out && M > 0 && V >= 1 && ld >= V && (n_params == 1 || n_params == M), "sm_sample_rows: bad args (M=%d V=%d ld=%d n_params=%d)", M, V, ld, n_params);
    SM_REQUIRE(u_dev_opt || pos_host, "sm_sample_rows: neither uniforms nor positions for the device generator");
    for (int i = 0; i < n_params; ++i) { int rc = sm_sampling_check(&params_host[i], "sm_sample_rows"); if (rc) return rc; }
    const SmSampleTail none = {nullptr, nullptr, 0, nullptr, 0};
    for (int m0 = 0; m0 < M; m0 += SM_MAX_SEG) {
        const int n = M - m0 < SM_MAX_SEG ? M - m0 : SM_MAX_SEG;
        SmSamplePack pk;
        for (int t = 0; t < n; ++t) {
            pk.r[t] = sm_sample_rule(&params_host[n_params == 1 ? 0 : m0 + t], pos_host ? pos_host[m0 + t] : 0);
            pk.tok[t] = tok_out + m0 + t;
        }
        int rc = smp_launch(logits + (size_t)m0 * ld, n, V, ld, pk, u_dev_opt ? u_dev_opt + m0 : nullptr, kept_out_opt ? kept_out_opt + m0 : nullptr,
                            kept_mass_out_opt ? kept_mass_out_opt + m0 : nullptr, none, stream);
        if (rc) return rc;
    }
    return SM_OK;
}

// the sampled decode tail: one row, the pending-token word, optionally the emitted id and the embedding row of the next step
int sm_sample_tail(const float* logits, int V, const SmSampleRule& rule, int32_t* next_tok, int32_t* emit, const void* table, int D, float* emb, int f16, void* stream) {
    SmSamplePack pk;
    pk.r[0] = rule; pk.tok[0] = next_tok;
    const SmSampleTail tail = {emit, (const bf16_t*)table, D, emb, f16};
    return smp_launch(logits, 1, V, V, pk, nullptr, nullptr, nullptr, tail, stream);
}
int sm_sample_rows_seg(const float* logits, int S, int V, int ld, const SmSamplePack& pk, void* stream) {
    SM_REQUIRE(logits && S > 0 && S <= SM_MAX_SEG && V > 0, "sm_sample_rows_seg: bad args");
    return smp_launch(logits, S, V, ld, pk, nullptr, nullptr, nullptr, SmSampleTail{nullptr, nullptr, 0, nullptr, 0}, stream);
}
int sm_sample_rows_tab(const float* logits, int S, int V, int ld, const SmSampleTab& tab, void* stream) {
    SM_REQUIRE(logits && S > 0 && V > 0 && tab.r && tab.tok, "sm_sample_rows_tab: bad args");
    return smp_launch(logits, S, V, ld, tab, nullptr, nullptr, nullptr, SmSampleTail{nullptr, nullptr, 0, nullptr, 0}, stream);
}
