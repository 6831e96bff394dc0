// Micro-benchmark of the SCAN main-loop STRUCTURE (one 256-thread workgroup per CU):
// per "half chunk": 36 fp32 MFMAs consuming fragments read from LDS one half earlier, 10 ds_read_b128 for the
// next half; every other half: 7 ds_write_b128 + 7 global loads (prefetch distance 2 chunks) + a barrier.
//
// Second part (`ksched`): the GENERATED main-loop statement itself, instruction for instruction, one kernel per schedule of
// tools/gen_scan_mainloop.py (SCHEDULES), with the operands set up as csrc/scan_mainloop.inc does.  Cycles per chunk are the
// s_memtime difference of two chunk counts (prologue, tail and park cancel), median over workgroups, with one workgroup per
// CU ("lone") and with two that start together ("pair": both multiply all the time).
//   python tools/gen_scan_mainloop.py --ubench tools/ubench/mfma_pipe_gen
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench/mfma_pipe.hip -o tools/ubench/mfma_pipe
//   tools/ubench/mfma_pipe [sched]          # "sched": only the second part
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int VARIANT>
__global__ __launch_bounds__(256, 1) void k(int iters, const char *__restrict__ gsrc, float *out) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    f32x4 acc[9];
    for (int m = 0; m < 9; ++m) acc[m] = f32x4{0, 0, 0, 0};
    const int tid = threadIdx.x;
    f32x4 fa[9], fb, ga[9], gb;  // two fragment sets
    f32x4 s0[7], s1[7];
    for (int i = 0; i < 7; ++i) { s0[i] = f32x4{1, 1, 1, 1}; s1[i] = f32x4{2, 2, 2, 2}; }
    for (int i = tid; i < 2 * 28672 / 16; i += 256) reinterpret_cast<f32x4 *>(lds)[i] = f32x4{1e-3f, 2e-3f, 3e-3f, 4e-3f};
    __syncthreads();
    const unsigned ra = (tid & 63) * 16, wa = tid * 16;
    const unsigned vo = tid * 16;
#define FREAD(A, B, OFF) { B = *reinterpret_cast<const f32x4 *>(lds + ra + (OFF) + 2304); \
    _Pragma("unroll") for (int m = 0; m < 9; ++m) A[m] = *reinterpret_cast<const f32x4 *>(lds + ra + (OFF) + m * 256); }
#define FMFMA(A, B) { _Pragma("unroll") for (int c = 0; c < 4; ++c) _Pragma("unroll") for (int m = 0; m < 9; ++m) \
    acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(A[m][c], B[c], acc[m], 0, 0, 0); }
#define LSTORE(S, OFF) { _Pragma("unroll") for (int i = 0; i < 7; ++i) *reinterpret_cast<f32x4 *>(lds + wa + (OFF) + i * 4096) = S[i]; }
#define GLOAD(S, KC) { const char *b_ = gsrc + (size_t)((KC) & 31) * 28672; \
    _Pragma("unroll") for (int i = 0; i < 7; ++i) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(S[i]) : "v"(vo + i * 4096), "s"(b_) : "memory"); }
#define VMWAIT(S) asm volatile("s_waitcnt vmcnt(7)" : "+v"(S[0]), "+v"(S[1]), "+v"(S[2]), "+v"(S[3]), "+v"(S[4]), "+v"(S[5]), "+v"(S[6])::"memory");
#define PIN __builtin_amdgcn_sched_barrier(0);
#define SGB(m, n) __builtin_amdgcn_sched_group_barrier(m, n, 0);
#define ILV_A { _Pragma("unroll") for (int i_ = 0; i_ < 7; ++i_) { SGB(0x008, 1) SGB(0x200, 1) } \
    _Pragma("unroll") for (int i_ = 0; i_ < 7; ++i_) { SGB(0x008, 1) SGB(0x020, 1) } \
    _Pragma("unroll") for (int i_ = 0; i_ < 10; ++i_) { SGB(0x008, 1) SGB(0x100, 1) } SGB(0x008, 12) }
#define ILV_B { _Pragma("unroll") for (int i_ = 0; i_ < 10; ++i_) { SGB(0x008, 1) SGB(0x100, 1) } SGB(0x008, 26) }
#define BARRIER { if (VARIANT == 3 || VARIANT == 4 || VARIANT == 10) __syncthreads(); \
    if (VARIANT == 5) { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); } \
    if (VARIANT == 6) { asm volatile("s_barrier" ::: "memory"); } \
    if (VARIANT == 7) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); } \
    if (VARIANT == 8) { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); } }
    GLOAD(s0, 0) GLOAD(s1, 1)
    FREAD(fa, fb, 0)
    for (int it = 0; it < iters; it += 2) {
        // chunk A (buffer 0 -> park into buffer 1)
        if (VARIANT >= 2) { VMWAIT(s1) LSTORE(s1, 28672) GLOAD(s1, it + 3) }
        if (VARIANT >= 1) FREAD(ga, gb, 1024)
        if (VARIANT == 4) PIN
        FMFMA(fa, fb)
        if (VARIANT >= 9) { ILV_A }
        if (VARIANT >= 4) PIN
        BARRIER
        if (VARIANT >= 1) FREAD(fa, fb, 28672)
        if (VARIANT == 4) PIN
        FMFMA(ga, gb)
        if (VARIANT >= 9) { ILV_B }
        if (VARIANT == 4) PIN
        // chunk B (buffer 1 -> park into buffer 0)
        if (VARIANT >= 2) { VMWAIT(s0) LSTORE(s0, 0) GLOAD(s0, it + 4) }
        if (VARIANT >= 1) FREAD(ga, gb, 28672 + 1024)
        if (VARIANT == 4) PIN
        FMFMA(fa, fb)
        if (VARIANT >= 9) { ILV_A }
        if (VARIANT == 4) PIN
        BARRIER
        if (VARIANT >= 1) FREAD(fa, fb, 0)
        if (VARIANT == 4) PIN
        FMFMA(ga, gb)
        if (VARIANT >= 9) { ILV_B }
        if (VARIANT == 4) PIN
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    float s = 0;
    for (int m = 0; m < 9; ++m) s += acc[m][0] + acc[m][1] + acc[m][2] + acc[m][3];
    for (int i = 0; i < 7; ++i) s += s0[i][0] + s1[i][0];
    out[blockIdx.x * 256 + tid] = s;
}

template <int V>
void run(const char *name, int iters, const char *g, float *out) {
    hipFuncSetAttribute(reinterpret_cast<const void *>(k<V>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    for (int rep = 0; rep < 2; ++rep) {
        hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
        hipEventRecord(e0);
        hipLaunchKernelGGL(k<V>, dim3(256), dim3(256), 100 * 1024, 0, iters, g, out);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float t; hipEventElapsedTime(&t, e0, e1);
        if (rep) printf("%-44s %8.3f ms -> %7.1f cycles per chunk of 72 MFMAs @2.35GHz (ideal 2304)\n", name, t, t * 1e-3 * 2.35e9 / iters);
    }
}
#if __has_include("mfma_pipe_gen/schedules.h")
#define HAVE_SCHED 1
constexpr int SC_MT = 144, SC_NT = 64, SC_ROWS = SC_MT + SC_NT + 16, SC_LDT = SC_MT + 4;
constexpr int NK_LO = 35, NK_HI = 291;               // chunks per launch; row pitch = NK_HI * 128 bytes for both
constexpr int A_TILES = 8, B_TILES = 16;

template <int V>
__global__ __launch_bounds__(256, 2) void ksched(const char *__restrict__ img, const char *__restrict__ wt, int nk, unsigned rowbytes,
                                                 unsigned long long *__restrict__ cyc) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, fg = lane >> 4;
    const char *abase = img + (size_t)(blockIdx.x % A_TILES) * SC_MT * rowbytes;
    const char *bbase = wt + (size_t)(blockIdx.x % B_TILES) * SC_NT * rowbytes;
    const char *bbase2 = bbase + 32 * (size_t)rowbytes;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) char *)smem_raw;
    const int p = tid & 7, r8 = tid >> 3, r4 = (tid & 127) >> 3;
    auto a_off = [&](int row) -> unsigned { return (unsigned)row * rowbytes + p * 16u; };
    auto l_off = [&](int row) -> unsigned { return lds0 + (unsigned)(p * SC_ROWS + (row ^ p)) * 16u; };
    const unsigned va0 = a_off(r8), va1 = a_off(r8 + 32), va2 = a_off(r8 + 64), va3 = a_off(r8 + 96);
    const unsigned va4 = wave < 2 ? a_off(128 + r4) : p * 16u;
    const unsigned la0 = l_off(r8), la4 = wave < 2 ? l_off(128 + r4) : l_off(SC_MT + SC_NT + r4);
    const unsigned vb0 = (unsigned)r8 * rowbytes + p * 16u;
    const unsigned ra0 = lds0 + (unsigned)((fg) * SC_ROWS + (fi ^ fg)) * 16u;
    const unsigned ra1 = lds0 + (unsigned)((4 + fg) * SC_ROWS + (fi ^ (4 + fg))) * 16u;
    const unsigned rb0 = ra0 + (unsigned)(SC_MT + wave * 16) * 16u, rb1 = ra1 + (unsigned)(SC_MT + wave * 16) * 16u;
    const unsigned park_addr = lds0 + (unsigned)(((wave * 16 + fi) * SC_LDT + fg * 4) * 4);
    const int nmain = nk - 3;
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#define SCHED_BODY
#include "mfma_pipe_gen/schedules.h"
#undef SCHED_BODY
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) cyc[blockIdx.x * 4 + wave] = t1 - t0;
}

static double median(std::vector<unsigned long long> v) { std::sort(v.begin(), v.end()); return (double)v[v.size() / 2]; }

template <int V>
void run_sched(const char *name, const char *img, const char *wt, unsigned long long *cyc) {
    hipFuncSetAttribute(reinterpret_cast<const void *>(ksched<V>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const unsigned rowbytes = NK_HI * 128;
    double res[2], mhz[2];
    for (int pair = 0; pair < 2; ++pair) {                    // lone: 100 KiB of LDS keeps a second workgroup off the CU
        const int blocks = pair ? 512 : 256, lds = pair ? 64 * 1024 : 100 * 1024;
        double c[2], ms[2];
        for (int w = 0; w < 2; ++w) {
            const int nk = w ? NK_HI : NK_LO;
            std::vector<unsigned long long> h(blocks * 4);
            for (int rep = 0; rep < 3; ++rep) {
                hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
                hipEventRecord(e0);
                hipLaunchKernelGGL(ksched<V>, dim3(blocks), dim3(256), lds, 0, img, wt, nk, rowbytes, cyc);
                hipEventRecord(e1);
                if (hipEventSynchronize(e1) != hipSuccess) { printf("%s: launch failed\n", name); exit(1); }
                float t; hipEventElapsedTime(&t, e0, e1); ms[w] = t;
                hipEventDestroy(e0); hipEventDestroy(e1);
            }
            hipMemcpy(h.data(), cyc, h.size() * 8, hipMemcpyDeviceToHost);
            c[w] = median(h);
        }
        res[pair] = (c[1] - c[0]) / (NK_HI - NK_LO) / (pair ? 2 : 1);
        mhz[pair] = (c[1] - c[0]) / ((ms[1] - ms[0]) * 1e3);
    }
    printf("%-32s lone %7.1f cycles per chunk (%5.1f %% of 2304)   pair %7.1f per chunk and workgroup (%5.1f %%)   clock %4.0f / %4.0f MHz\n", name,
           res[0], 230400.0 / res[0], res[1], 230400.0 / res[1], mhz[0], mhz[1]);
    fflush(stdout);
}

void run_all_sched() {
    const size_t abytes = (size_t)A_TILES * SC_MT * NK_HI * 128, bbytes = (size_t)B_TILES * SC_NT * NK_HI * 128;
    char *img, *wt; unsigned long long *cyc;
    hipMalloc(&img, abytes); hipMalloc(&wt, bbytes); hipMalloc(&cyc, 512 * 4 * 8);
    std::vector<float> h(std::max(abytes, bbytes) / 4);
    unsigned x = 12345u;
    for (auto &v : h) { x = x * 1664525u + 1013904223u; v = ((int)(x >> 8) % 2001 - 1000) * 1e-3f; }
    hipMemcpy(img, h.data(), abytes, hipMemcpyHostToDevice); hipMemcpy(wt, h.data(), bbytes, hipMemcpyHostToDevice);
#define SCHED(i, name) run_sched<i>(name, img, wt, cyc);
#define SCHED_LIST
#include "mfma_pipe_gen/schedules.h"
#undef SCHED_LIST
}
#endif

int main(int argc, char **argv) {
#ifdef HAVE_SCHED
    if (argc > 1 && !strcmp(argv[1], "sched")) { run_all_sched(); return 0; }
#endif
    char *g; float *out;
    hipMalloc(&g, 64 * 28672 + 65536); hipMemset(g, 0, 64 * 28672 + 65536); hipMalloc(&out, 256 * 256 * 4);
    const int it = 20000;
    run<0>("mfma only", it, g, out);
    run<1>("+ pipelined fragment reads", it, g, out);
    run<2>("+ park (7 ds_write) + 7 gloads per chunk", it, g, out);
    run<3>("+ barrier per chunk", it, g, out);
    run<4>("+ sched_barrier pins", it, g, out);
    run<5>("asm lgkmcnt(0)+s_barrier", it, g, out);
    run<6>("asm s_barrier only (racy)", it, g, out);
    run<7>("asm lgkmcnt(0) only (no barrier)", it, g, out);
    run<8>("fence+s_barrier builtin", it, g, out);
    run<9>("interleaved 1 mem op per MFMA, no barrier", it, g, out);
    run<10>("interleaved + __syncthreads", it, g, out);
#ifdef HAVE_SCHED
    run_all_sched();
#endif
    return 0;
}
