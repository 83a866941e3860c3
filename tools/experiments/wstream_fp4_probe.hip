// What paces wstream_fp4_kernel (csrc/gemm_fp4.hip, SM_W_FP4_MFMA at 17..128 rows) on the products of a batched decode step?  The same kernel with pieces
// removed: -DF4W_X_NOMFMA=1 (operands consumed, no matrix instruction), -DF4W_X_NOXREAD=1 (no B-fragment reads from LDS), -DF4W_X_NOXLOAD=1 (the loader waves
// fetch nothing from the x workspace; barriers and LDS writes stay).  Times are the prepass + main kernel per call (the slab sum is stubbed out).
//   for F in "" -DF4W_X_NOXLOAD=1 -DF4W_X_NOMFMA=1 "-DF4W_X_NOMFMA=1 -DF4W_X_NOXREAD=1" "-DF4W_X_NOMFMA=1 -DF4W_X_NOXREAD=1 -DF4W_X_NOXLOAD=1"; do
//     hipcc --offload-arch=gfx950 -O3 -std=c++17 $F tools/experiments/wstream_fp4_probe.hip -o /tmp/f4p && /tmp/f4p; done
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../streammind_amd/csrc/gemm_fp4.hip"
thread_local char g_sm_err[512];
int g_sm_prof_mask = 0;
void sm_prof_begin_(int, hipStream_t, long long) {}
void sm_prof_end_(int, hipStream_t) {}
static float* g_slab = nullptr;
int splitk_workspace(hipStream_t, size_t bytes, float** out) { if (!g_slab) hipMalloc((void**)&g_slab, (size_t)2 * 8 * 128 * 14336 * 4); *out = g_slab; return bytes <= (size_t)2 * 8 * 128 * 14336 * 4 ? 0 : -1; }
int launch_splitk_reduce(const LinArgs&, const float*, int, int, hipStream_t, const float*) { return 0; }
int main() {
    struct { const char* name; int N, K, dual; } shapes[] = {{"gate|up dual", 14336, 4096, 1}, {"down", 4096, 14336, 0}, {"qkv", 6144, 4096, 0}, {"o", 4096, 4096, 0}};
    for (int M : {32, 64, 128})
        for (auto& sh : shapes) {
            const size_t wb = sm_packed_fp4_bytes(sh.N, sh.K);
            void *w, *w2, *x, *ob;
            hipMalloc(&w, wb); hipMalloc(&w2, wb); hipMalloc(&x, (size_t)M * sh.K * 2); hipMalloc(&ob, (size_t)M * sh.N * 4);
            hipMemset(w, 0x11, wb); hipMemset(w2, 0x11, wb); hipMemset(x, 0x11, (size_t)M * sh.K * 2);
            LinArgs a; memset(&a, 0, sizeof(a));
            a.w = (const bf16x8*)w; a.w2 = sh.dual ? (const bf16x8*)w2 : nullptr; a.N = sh.N; a.K = sh.K; a.KS = sh.K / 32; a.NRG = sh.N / 16; a.x = x; a.M = M; a.ldx = sh.K;
            a.out_bf16 = sh.dual ? (bf16_t*)ob : nullptr; a.ldo_bf16 = sh.N; a.out_f32 = sh.dual ? nullptr : (float*)ob; a.ldo = sh.N;
            hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
            for (int it = 0; it < 3; ++it) if (launch_wstream_fp4(a, false, 0)) { printf("launch failed: %s\n", g_sm_err); return 1; }
            hipEventRecord(e0);
            for (int it = 0; it < 20; ++it) launch_wstream_fp4(a, false, 0);
            hipEventRecord(e1); hipEventSynchronize(e1);
            float ms; hipEventElapsedTime(&ms, e0, e1);
            printf("M=%3d %-13s N=%5d K=%5d: %6.1f us  %.2f TB/s of codes   [NOMFMA=%d NOXREAD=%d NOXLOAD=%d]\n", M, sh.name, sh.N, sh.K, ms * 50, (double)wb * (sh.dual ? 2 : 1) / (ms * 50e-6) / 1e12,
                   F4W_X_NOMFMA, F4W_X_NOXREAD, F4W_X_NOXLOAD);
            hipFree(w); hipFree(w2); hipFree(x); hipFree(ob);
        }
    return hipDeviceSynchronize() == hipSuccess ? 0 : 1;
}
