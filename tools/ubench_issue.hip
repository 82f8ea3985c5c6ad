// Issue-cost micro-benchmark on gfx950: what one more instruction per step costs a wave that runs the E-step's
// dependent forward chain (the step of tools/ubench_chain.hip, variant 1: fma(e1, dpp_shr(x), e0 * x)).
// One workgroup; 64 * W threads -> W waves (W = 4: one per SIMD, a lone wave; W = 8: two per SIMD).
// Every variant adds, per step, instructions that nothing depends on and that never stall; the difference to the
// bare chain is their issue cost.  The extras are inline assembly, so the compiler neither merges nor drops them.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench_issue.hip -o tools/ubench_issue && tools/ubench_issue
#include <hip/hip_runtime.h>
#include <cstdio>

template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    long long x = __builtin_bit_cast(long long, v);
    x = __builtin_amdgcn_update_dpp(0ll, x, CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, x);
}

constexpr int kSteps = 4096;

enum Extra { kNone, kWait, kNop, kSalu, kValu };

template <Extra X, int CNT>
__global__ void k_issue(const double *in, double *out, long long *cyc) {
    double x = in[threadIdx.x], e0 = in[threadIdx.x + 2], e1 = in[threadIdx.x + 3];
    unsigned v[6] = {threadIdx.x, threadIdx.x + 1, threadIdx.x + 2, threadIdx.x + 3, threadIdx.x + 4, threadIdx.x + 5};
    unsigned s = blockDim.x;
    __syncthreads();
    const long long t0 = clock64();
#pragma unroll 16
    for (int i = 0; i < kSteps; ++i) {
        x = fma(e1, dpp<0x111>(x), e0 * x);
        if constexpr (X == kWait) asm volatile("s_waitcnt lgkmcnt(15)");  // never stalls: nothing is outstanding
        if constexpr (X == kNop) asm volatile("s_nop 0");
        if constexpr (X == kSalu) asm volatile("s_add_u32 %0, %0, 1" : "+s"(s) : : "scc");
        if constexpr (X == kValu) {
#pragma unroll
            for (int q = 0; q < CNT; ++q) asm volatile("v_add_u32 %0, %0, %0" : "+v"(v[q]));
        }
    }
    const long long t1 = clock64();
    out[threadIdx.x] = x + (double)(v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + s);
    if ((threadIdx.x & 63) == 0) cyc[threadIdx.x / 64] = t1 - t0;
}

template <Extra X, int CNT>
double run(const char *name, double *din, double *dout, long long *dcyc, int waves, double base) {
    hipLaunchKernelGGL((k_issue<X, CNT>), dim3(1), dim3(64 * waves), 0, 0, din, dout, dcyc);
    hipLaunchKernelGGL((k_issue<X, CNT>), dim3(1), dim3(64 * waves), 0, 0, din, dout, dcyc);
    long long h[16];
    if (hipMemcpy(h, dcyc, sizeof(long long) * waves, hipMemcpyDeviceToHost) != hipSuccess) {
        printf("%-34s waves %2d  failed\n", name, waves);
        return 0.0;
    }
    double mx = 0;
    for (int w = 0; w < waves; ++w) mx = h[w] > mx ? h[w] : mx;
    const double c = mx / kSteps;
    printf("%-34s waves %2d  %7.2f cycles/step (s_memtime)  %+6.2f over the bare chain\n", name, waves, c, base > 0 ? c - base : 0.0);
    return c;
}

int main() {
    double *din, *dout;
    long long *dcyc;
    if (hipMalloc(&din, 2048 * sizeof(double)) != hipSuccess || hipMalloc(&dout, 2048 * sizeof(double)) != hipSuccess ||
        hipMalloc(&dcyc, 16 * sizeof(long long)) != hipSuccess) {
        printf("no device memory\n");
        return 1;
    }
    double h[2048];
    for (int i = 0; i < 2048; ++i) h[i] = 1.0 + 1e-9 * i;
    (void)hipMemcpy(din, h, sizeof(h), hipMemcpyHostToDevice);
    for (int w : {4, 8}) {
        const double a = run<kNone, 0>("(a) forward step chain", din, dout, dcyc, w, 0.0);
        run<kWait, 0>("(b) + s_waitcnt lgkmcnt(15)", din, dout, dcyc, w, a);
        run<kNop, 0>("(c) + s_nop 0", din, dout, dcyc, w, a);
        run<kSalu, 0>("(d) + s_add_u32", din, dout, dcyc, w, a);
        const double e1 = run<kValu, 1>("(e) + 1 v_add_u32", din, dout, dcyc, w, a);
        run<kValu, 2>("(f) + 2 v_add_u32", din, dout, dcyc, w, a);
        run<kValu, 4>("(f) + 4 v_add_u32", din, dout, dcyc, w, a);
        const double e6 = run<kValu, 6>("(f) + 6 v_add_u32", din, dout, dcyc, w, a);
        printf("slope, waves %2d: %.2f cycles per extra v_add_u32 (from 1 to 6 per step)\n", w, (e6 - e1) / 5.0);
    }
    return 0;
}
