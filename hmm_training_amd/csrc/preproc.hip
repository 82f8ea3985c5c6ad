// preproc.hip — signal conditioning (hmmbw_preprocess, hmmbw_window_overlap; include/hmmbw.h) for gfx950: what the
// reference does on the host before anything else, sample by sample in Python: the pre-emphasis filter 1 - 0.95 z^-1
// (preemphasis.py:174-183), the power / zero-crossing trim of a recording to where speech is (slice_signal,
// preemphasis.py:222-294 and HMM/live_testing.py:48-120) and the live recogniser's in-place overlapping Hamming window
// (preemphasis.py:189-212).
//
// k_preprocess: one workgroup per recording, so that the recording's maxima and its first / last kept frame never
// leave the workgroup and nothing waits on the host or on another workgroup.
//   filter       y[i] = x[i] - fl(c x[i-1]), y[0] = 0: four samples per lane (one 8-byte load of int16 samples, two
//                16-byte loads of doubles, the predecessor from the cache; two 16-byte stores) between the recording's
//                first and last multiple of four, single samples at its ragged ends.  The product is __dmul_rn: rounded
//                on its own, never contracted into the subtraction (the unit is also built with -ffp-contract=off).
//   statistics   a wave per frame over the y just written (the recording's own lines, still in the cache): sum of
//                squares / length and half the sum of |sign - sign|, one wave reduction each.  The last frame's odd
//                length is pre_frame_len (preproc_plan.hpp).  A recording of at most kPreLdsFrames frames keeps the
//                pairs in the LDS; a longer one computes them a second time in the search (same lanes, same order:
//                the same bits).
//   bounds       the maxima over the workgroup, then first kept frame (thresholds zf, pf) and last kept frame (zl, pl),
//                or (0, nf) when no frame passes the first pair; bounds_out gets (first hop, last hop).
// k_window_overlap: every sample of [start, finish) is multiplied by the table entry of each window frame that covers
// it, in ascending frame order (the order of the reference's in-place loop, hence its bits); the partial last frame
// spares the last sample.  A recording is spread over gridDim.y workgroups.
#include "host.hpp"
#include "lane_ops.hpp"
#include "preproc_plan.hpp"

namespace hmmbw {

struct PreArgs {
    const void *x;          // int16 or double [n_samples]
    const long long *off;   // [n_rec + 1]
    double *y;              // [n_samples]
    long long *bounds;      // [n_rec][2]
    double *stats;          // [sum nf][2] or nullptr
    double coeff, zf, pf, zl, pl;
    int win, hop;
};

__device__ __forceinline__ double pre_sign(double v) { return (double)((v > 0.0) - (v < 0.0)); }

template <class S>
__device__ __forceinline__ double pre_filter1(const S *x, long long i, long long lo, double c) {
    return i == lo ? 0.0 : (double)x[i] - __dmul_rn(c, (double)x[i - 1]);
}

// four samples from p (a multiple of 4 with lo <= p, p + 4 <= hi) as doubles
__device__ __forceinline__ void pre_load4(const double *x, long long p, double (&v)[4]) {
    const double2 a = *reinterpret_cast<const double2 *>(x + p), b = *reinterpret_cast<const double2 *>(x + p + 2);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
}
__device__ __forceinline__ void pre_load4(const short *x, long long p, double (&v)[4]) {
    const short4 a = *reinterpret_cast<const short4 *>(x + p);
    v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
}

template <class S>
__device__ void pre_filter(const S *__restrict__ x, double *__restrict__ y, long long lo, long long hi, double c,
                           int tid, int nt) {
    // [a, b): the whole groups of four at multiples of four; without the alignment every sample goes alone
    const size_t load_bytes = sizeof(S) == 2 ? 8 : 16;
    const bool aligned = ((size_t)x & (load_bytes - 1)) == 0 && ((size_t)y & 15) == 0;
    long long a = lo, b = lo;
    if (aligned) {
        a = (lo + 3) & ~3LL;
        if (a > hi) a = hi;
        b = a + ((hi - a) & ~3LL);
    }
    for (long long i = lo + tid; i < a; i += nt) y[i] = pre_filter1(x, i, lo, c);
    for (long long i = b + tid; i < hi; i += nt) y[i] = pre_filter1(x, i, lo, c);
#pragma unroll 4  // x and y do not overlap: the loads of four steps go out before the first store
    for (long long p = a + 4LL * tid; p < b; p += 4LL * nt) {
        double v[4];
        pre_load4(x, p, v);
        const double y0 = p == lo ? 0.0 : v[0] - __dmul_rn(c, (double)x[p - 1]);
        const double y1 = v[1] - __dmul_rn(c, v[0]), y2 = v[2] - __dmul_rn(c, v[1]), y3 = v[3] - __dmul_rn(c, v[2]);
        *reinterpret_cast<double2 *>(y + p) = double2{y0, y1};
        *reinterpret_cast<double2 *>(y + p + 2) = double2{y2, y3};
    }
}

// (zcr, power) of the frame y[s, s + len) of a recording, complete in every lane of the wave
__device__ __forceinline__ void pre_frame_stats(const double *y, long long s, int len, int lane, double &zcr, double &power) {
    // kPreUnroll x 64 samples per step, all loads of a step issued before the first use: the phase waits on the
    // cache's latency, not on arithmetic (a frame of 320 is one step).  A sample past the frame is read as 0 and
    // adds +0 to the squares; each lane sums in ascending j whatever the unroll.
    constexpr int kPreUnroll = 8;
    double sq = 0.0, cr = 0.0;
    for (int j0 = lane; j0 < len; j0 += 64 * kPreUnroll) {
        double v[kPreUnroll], nx[kPreUnroll];
#pragma unroll
        for (int k = 0; k < kPreUnroll; ++k) {
            const int j = j0 + 64 * k;
            v[k] = j < len ? y[s + j] : 0.0;
            nx[k] = j + 1 < len ? y[s + j + 1] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < kPreUnroll; ++k) {
            sq += v[k] * v[k];
            if (j0 + 64 * k + 1 < len) cr += fabs(pre_sign(nx[k]) - pre_sign(v[k]));
        }
    }
    sq = gsum<64>(sq);
    cr = gsum<64>(cr);  // small integers: exact
    power = sq / (double)len;
    zcr = 0.5 * cr;
}

template <class S>
__global__ void __launch_bounds__(1024) k_preprocess(PreArgs a) {
    __shared__ double sZ[kPreLdsFrames], sP[kPreLdsFrames], sRed[16];
    __shared__ unsigned long long sFirst, sBase;
    __shared__ long long sLast;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const long long r = blockIdx.x;
    const long long lo = a.off[r], hi = a.off[r + 1], n = hi - lo;
    const int win = a.win, hop = a.hop;
    if (tid == 0) {
        sFirst = ~0ULL;
        sBase = 0ULL;
        sLast = -1;
    }
    if (n > 0) pre_filter(static_cast<const S *>(a.x), a.y, lo, hi, a.coeff, tid, nt);
    if (n < 0 || !pre_rec_ok(n, win, hop)) {  // the host refuses these where it knows the lengths: no frame, no bounds
        if (tid == 0) a.bounds[2 * r] = a.bounds[2 * r + 1] = 0;
        return;
    }
    __syncthreads();  // y is written (and the workgroup's stores are visible to its waves)
    if (a.stats) {    // the row of this recording's first frame: the frames of the recordings before it
        unsigned long long before = 0;
        for (long long q = tid; q < r; q += nt) {
            const long long nq = a.off[q + 1] - a.off[q];
            if (nq >= 0 && pre_rec_ok(nq, win, hop)) before += (unsigned long long)pre_frame_count(nq, win, hop);
        }
        if (before) atomicAdd(&sBase, before);
        __syncthreads();
    }
    const long long nf = pre_frame_count(n, win, hop);
    const bool cached = nf <= kPreLdsFrames;
    const double *y = a.y + lo;
    double mz = 0.0, mp = 0.0;  // zcr and power are never negative
    for (long long f = wave; f < nf; f += nw) {
        double z, p;
        pre_frame_stats(y, f * hop, (int)pre_frame_len(n, win, hop, f), lane, z, p);
        mz = fmax(mz, z);
        mp = fmax(mp, p);
        if (lane == 0) {
            if (cached) sZ[f] = z, sP[f] = p;
            if (a.stats) {
                double *row = a.stats + 2 * ((long long)sBase + f);
                row[0] = z;
                row[1] = p;
            }
        }
    }
    mz = block_reduce(mz, sRed, true);
    mp = block_reduce(mp, sRed, true);
    const double tzf = a.zf * mz, tpf = a.pf * mp, tzl = a.zl * mz, tpl = a.pl * mp;
    long long first = LLONG_MAX, last = -1;
    for (long long f = wave; f < nf; f += nw) {
        double z, p;
        if (cached) {
            z = sZ[f], p = sP[f];
        } else {
            pre_frame_stats(y, f * hop, (int)pre_frame_len(n, win, hop, f), lane, z, p);
        }
        if ((a.zf < 0.0 || z > tzf) && p > tpf && f < first) first = f;
        if ((a.zl < 0.0 || z > tzl) && p > tpl) last = f;
    }
    if (lane == 0) {
        if (first != LLONG_MAX) atomicMin(&sFirst, (unsigned long long)first);
        if (last >= 0) atomicMax(&sLast, last);
    }
    __syncthreads();
    if (tid == 0) {
        long long f0 = 0, f1 = nf;
        if (sFirst != ~0ULL) {
            f0 = (long long)sFirst;
            f1 = sLast >= 0 ? sLast : f0;  // (the reference raises where the second pair keeps nothing)
        }
        const long long start = f0 * hop, finish = f1 * hop;
        a.bounds[2 * r] = start < n ? start : n;  // never past the recording, as a slice would clip them
        a.bounds[2 * r + 1] = finish < n ? finish : n;
    }
}

__global__ void __launch_bounds__(256) k_window_overlap(double *__restrict__ t, const long long *__restrict__ off,
                                                        const long long *__restrict__ bounds,
                                                        const double *__restrict__ w, int wlen, int whop) {
    const long long r = blockIdx.x;
    const long long lo = off[r], n = off[r + 1] - lo, st = bounds[2 * r], fi = bounds[2 * r + 1];
    if (n <= 0 || st < 0 || fi > n || st > fi) return;  // bounds outside the recording: nothing is touched
    const long long m = fi - st, q = pre_window_frames(m, wlen, whop);
    if (q < 0) return;
    double *base = t + lo + st;
    const long long step = (long long)gridDim.y * blockDim.x;
    for (long long j = (long long)blockIdx.y * blockDim.x + threadIdx.x; j < m; j += step) {
        const long long i0 = j >= wlen ? (j - wlen) / whop + 1 : 0;  // the first frame that reaches j
        const long long i1 = j / whop < q ? j / whop : q;            // the last one that starts at or before j
        if (i0 > i1) continue;
        double v = base[j];
        for (long long i = i0; i <= i1; ++i) {
            const long long k = j - i * whop;
            if (k < wlen && (i < q || j < m - 1)) v = v * w[k];  // frame q is the partial one: it spares sample m - 1
        }
        base[j] = v;
    }
}

}  // namespace hmmbw

using namespace hmmbw;

extern "C" int hmmbw_preprocess(void *stream, const void *samples, int sample_kind, const int64_t *rec_offsets,
                                const int64_t *rec_offsets_host, int64_t n_rec, double coeff, int win, int hop,
                                const double *factors, double *filtered_out, int64_t *bounds_out, double *stats_out) {
    const int v = pre_validate(n_rec, sample_kind, coeff, win, hop, factors,
                               samples && rec_offsets && filtered_out && bounds_out);
    if (v == kPreInvalid)
        return fail(HMMBW_E_INVALID, "hmmbw_preprocess: need n_rec >= 0, a known sample_kind, win >= 2, 1 <= hop <= win, "
                                     "four factors and a coefficient that are numbers, and every pointer but stats_out "
                                     "and rec_offsets_host");
    if (v != kPreOk) return fail(HMMBW_E_UNSUPPORTED, "hmmbw_preprocess: win > 65536 or n_rec >= 2^31");
    if (rec_offsets_host) {
        const int vo = pre_validate_offsets(reinterpret_cast<const long long *>(rec_offsets_host), n_rec, win, hop);
        if (vo == kPreInvalid)
            return fail(HMMBW_E_INVALID, "hmmbw_preprocess: rec_offsets must ascend from 0 and every recording needs "
                                         "more than win - hop samples (and at least 2): it has no frame otherwise");
        if (vo != kPreOk) return fail(HMMBW_E_UNSUPPORTED, "hmmbw_preprocess: more than 2^46 samples");
    }
    if (n_rec == 0) return HMMBW_OK;
    PreArgs a{};
    a.x = samples;
    a.off = reinterpret_cast<const long long *>(rec_offsets);
    a.y = filtered_out;
    a.bounds = reinterpret_cast<long long *>(bounds_out);
    a.stats = stats_out;
    a.coeff = coeff;
    a.zf = factors[0], a.pf = factors[1], a.zl = factors[2], a.pl = factors[3];
    a.win = win;
    a.hop = hop;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)n_rec), block((unsigned)pre_block(n_rec));
    if (sample_kind == HMMBW_SAMPLES_I16)
        hipLaunchKernelGGL(k_preprocess<short>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_preprocess<double>, grid, block, 0, st, a);
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}

extern "C" int hmmbw_window_overlap(void *stream, double *samples, const int64_t *rec_offsets, const int64_t *bounds,
                                    int64_t n_rec, const double *window, int wlen, int whop) {
    const int v = pre_window_validate(n_rec, wlen, whop, samples && rec_offsets && bounds && window);
    if (v == kPreInvalid)
        return fail(HMMBW_E_INVALID, "hmmbw_window_overlap: need n_rec >= 0, wlen >= 1, whop >= 1 and every pointer");
    if (v != kPreOk)
        return fail(HMMBW_E_UNSUPPORTED, "hmmbw_window_overlap: more than 8 window frames cover a sample "
                                         "(ceil(wlen / whop) > 8), wlen > 65536 or n_rec >= 2^31");
    if (n_rec == 0) return HMMBW_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(k_window_overlap, dim3((unsigned)n_rec, (unsigned)pre_window_chunks(n_rec)), dim3(256), 0, st,
                       samples, reinterpret_cast<const long long *>(rec_offsets),
                       reinterpret_cast<const long long *>(bounds), window, wlen, whop);
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}
