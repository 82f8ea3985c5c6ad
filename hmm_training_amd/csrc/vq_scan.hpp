// vq_scan.hpp — the nearest-centroid scan shared by the VQ encoder (vq.hip) and the LBG assign kernel (lbg.hip): the
// one copy of the arithmetic that tests/test_gpu_vq.py pins to np.linalg.norm bit for bit.  Each distance is
//     d = fma(x_{D-1}, x_{D-1}, ... fma(x_1, x_1, x_0 * x_0)),  x_i = f_i - c_i,   s = sqrt(d)
// with the correctly rounded fp64 sqrt; the comparison is a strict '<' on s and the first minimum wins.  sqrt is
// monotone, so s < s_best needs d < d_best: the sqrt is only evaluated for those candidates.  A NaN distance never
// wins (NaN < x is false), as in the reference: a frame with none keeps index 0 and distance +inf.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hmmbw {

// FPL frames per lane against K centroid rows read with wave-uniform SCALAR loads (c: row 0 at its first scanned
// column, rows `stride` doubles apart; K must be wave-uniform).  x[q][d] = frame q's scanned columns.
template <int D, int FPL>
__device__ __forceinline__ void vq_scan_scalar(const double (&x)[FPL][D], const double *__restrict__ c, int stride, int K,
                                               double (&best_s)[FPL], int (&arg)[FPL]) {
    double best_d[FPL];
#pragma unroll
    for (int q = 0; q < FPL; ++q) {
        best_s[q] = INFINITY;
        best_d[q] = INFINITY;
        arg[q] = 0;
    }
    // centroid k + 1's row is loaded (into SGPRs) while centroid k is scanned
    double cn[D];
#pragma unroll
    for (int d = 0; d < D; ++d) cn[d] = c[d];
    for (int k = 0; k < K; ++k) {
        double cc[D];
#pragma unroll
        for (int d = 0; d < D; ++d) cc[d] = cn[d];
        c += stride;
        if (k + 1 < K) {
#pragma unroll
            for (int d = 0; d < D; ++d) cn[d] = c[d];
        }
        double acc[FPL];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int q = 0; q < FPL; ++q) {
                const double e = x[q][d] - cc[d];
                acc[q] = (d == 0) ? e * e : __builtin_fma(e, e, acc[q]);
            }
        // only candidates with acc < best_d can have sqrt(acc) < best_s (sqrt is monotone); after the
        // first few centroids that is rare, so the sqrt sits behind a real branch
        bool any = false;
#pragma unroll
        for (int q = 0; q < FPL; ++q) any = any || (acc[q] < best_d[q]);
        if (__builtin_expect(__any(any), 0)) {
#pragma unroll
            for (int q = 0; q < FPL; ++q) {
                if (acc[q] < best_d[q]) {
                    const double sq = __builtin_sqrt(acc[q]);
                    if (sq < best_s[q]) {
                        best_s[q] = sq;
                        best_d[q] = acc[q];
                        arg[q] = k;
                    }
                }
            }
        }
    }
}

// One frame per lane (x[d], d < D <= DMAX) against a codebook staged in LDS as [K][D].
template <int DMAX>
__device__ __forceinline__ void vq_scan_lds(const double (&x)[DMAX], int D, const double *sC, int K, double &best_s,
                                            int &arg) {
    double best_d = INFINITY;
    best_s = INFINITY;
    arg = 0;
    for (int k = 0; k < K; ++k) {
        const double *c = sC + k * D;
        double acc = 0.0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            if (d >= D) break;
            const double e = x[d] - c[d];
            acc = (d == 0) ? e * e : __builtin_fma(e, e, acc);
        }
        if (acc < best_d) {
            const double s = __builtin_sqrt(acc);
            if (s < best_s) {
                best_s = s;
                best_d = acc;
                arg = k;
            }
        }
    }
}

// the staging loop of vq_scan_lds's codebook: columns [col0, col0 + D) of K rows
__device__ __forceinline__ void vq_stage_codebook(double *sC, const double *__restrict__ cents, int stride, int col0, int D,
                                                  int K) {
    for (int i = threadIdx.x; i < K * D; i += blockDim.x) {
        const int k = i / D, d = i - k * D;
        sC[i] = cents[(long long)k * stride + col0 + d];
    }
}

}  // namespace hmmbw
