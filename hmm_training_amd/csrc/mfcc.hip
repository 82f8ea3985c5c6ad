// mfcc.hip — the MFCC front end (hmmbw_mfcc, hmmbw_mfcc_tables; include/hmmbw.h) for gfx950: what the reference
// computes with one librosa.feature.mfcc call per 20 ms frame (RawDataMFCC.calculate_mfcc, CodeVector/
// codevector_classes.py:226-250; once more on every load of a frame file, :217-224).
//
// One frame of L samples is one STFT column with n_fft = L: window, |DFT|^2 over L/2 + 1 bins, mel bands, decibels
// with the top_db floor, DCT-II.  k_mfcc does all of it for a tile of 16 frames per workgroup (4 waves):
//   load and fold   the frames are views into the sample buffer (frame_starts); each is windowed and folded once,
//                   e[n] = y[n] + y[L-n], o[n] = y[n] - y[L-n] (e[0] = y[0], e[L/2] = y[L/2], o = 0 there), into two
//                   LDS images [16][Hs].  Re X_k = sum_{n<H} e[n] cos(2 pi k n / L), Im X_k = -sum o[n] sin(...):
//                   half the products of the plain DFT.  A non-finite sample is read as 0 and flags its frame.
//   DFT             the two sums are GEMMs on the fp64 matrix cores, v_mfma_f64_16x16x4_f64 with the 16 frames as
//                   rows (A[frame = lane & 15][n = 4 ks + (lane >> 4)]) and 16 bins as columns (B[n][bin = lane & 15]).
//                   B is the [L][2] twiddle table in LDS at (bin * n) mod L, advanced by (4 bin) mod L per step with
//                   an add and a conditional subtract; one 16-byte read feeds the cos and the sin product.  Wave w
//                   owns the bin blocks w, w + 4, ...: the A operands are read once per step for all of them.  A
//                   direct DFT on purpose: L = 320 = 2^6 5 and the remainder lengths are no powers of two.  H is
//                   padded to a multiple of 4 with zero samples; the bins are padded to a multiple of 16, and the
//                   padding bins (above Nyquist: valid table indices, real spectrum values) are never read again.
//   tail            |X|^2 -> LDS [16][Ps], over the folded images once every wave is through with them; lane (frame, filter) sums its filter's band [first, last] (found once per
//                   workgroup from the dense filter bank), 10 log10(max(amin, .)); lane (frame, coefficient) takes
//                   the frame's maximum, applies the top_db floor and the DCT row, and stores n_mfcc doubles.
// Every frame length 2 .. 512 takes this one path (a length of 13 runs a single bin block on one wave; the other
// waves' blocks are padding whose results are dropped).  All tables are arguments.
#include "host.hpp"
#include "mfcc_plan.hpp"

namespace hmmbw {

typedef double f64x4 __attribute__((ext_vector_type(4)));
// v_mfma_f64_16x16x4_f64: C/D col = lane & 15, row = (lane >> 4) + 4 reg; A[lane & 15][lane >> 4], B[lane >> 4][lane & 15]
// (the layout estep_mfma.hpp states and its tests pin)
__device__ __forceinline__ f64x4 mfma_f64(double a, double b, f64x4 c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

constexpr int kMfccWaves = 4;
constexpr unsigned kMfccMaxGrid = 1024;  // workgroups loop over tiles: the twiddles and bands are staged once each

struct MfccArgs {
    const double *x;         // [n_samples]
    const long long *starts; // [F]
    const double *window, *twiddle, *mel, *dct;
    double *out;
    long long n_samples, F, ntiles, out_stride;
    int L, n_mels, n_mfcc;
    double amin, top_db;
};

__global__ void __launch_bounds__(256) k_mfcc_check(const long long *__restrict__ starts, long long F, int L,
                                                    long long n_samples, int *__restrict__ bad) {
    for (long long f = (long long)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (long long)gridDim.x * blockDim.x)
        if (!mfcc_frame_in_range(starts[f], L, n_samples)) atomicOr(bad, 1);
}

// NBW: bin blocks per wave (ceil(blocks / 4)).  Two workgroups per CU at the least (<= 256 registers per lane): with
// that bound the compiler keeps the MFMA accumulators in VGPRs; without it it chose the AGPR form and copied all 8 NBW
// accumulator registers to VGPRs and back in every step of the DFT loop, each copy waiting for its MFMA to retire.
template <int NBW>
__global__ void __launch_bounds__(64 * kMfccWaves, 2) k_mfcc(MfccArgs a) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const int L = a.L, H = mfcc_half(L), Hp = mfcc_half_padded(L), Hs = mfcc_fold_stride(L), Ps = mfcc_power_stride(L);
    const int n_mels = a.n_mels, Ds = mfcc_db_stride(n_mels), nblk = mfcc_bin_blocks(L);
    const MfccLds lay = mfcc_lds(L, n_mels);
    double *sTw = smem + lay.twiddle, *sE = smem + lay.even, *sO = smem + lay.odd, *sP = smem + lay.power;
    double *sDb = smem + lay.db;
    int *sBand = reinterpret_cast<int *>(smem + lay.band);  // [n_mels][2]: first, last
    int *sFlag = reinterpret_cast<int *>(smem + lay.flag);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = lane & 15, g = lane >> 4;

    for (int i = tid; i < 2 * L; i += blockDim.x) sTw[i] = a.twiddle[i];
    for (int m = tid; m < n_mels; m += blockDim.x) {
        sBand[2 * m] = H;
        sBand[2 * m + 1] = -1;
    }
    __syncthreads();
    for (int i = tid; i < n_mels * H; i += blockDim.x)
        if (a.mel[i] != 0.0) {
            const int m = i / H, k = i - m * H;
            atomicMin(&sBand[2 * m], k);
            atomicMax(&sBand[2 * m + 1], k);
        }

    for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        __syncthreads();  // the tile before is through with the images (and the bands are complete)
        if (tid < kMfccTile) sFlag[tid] = 0;
        __syncthreads();
        // ---- load, window, fold ----
        // a wave owns the frames w, w + 4, w + 8, w + 12 and loads one column of all four at a time: 8 sample loads in
        // flight per lane instead of 2 (the phase waits on memory, not on arithmetic)
        {
            constexpr int Q = kMfccTile / kMfccWaves;
            long long st4[Q];
            bool ok4[Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int f = w + kMfccWaves * q;
                const long long gf = tile * kMfccTile + f;
                ok4[q] = gf < a.F;
                st4[q] = ok4[q] ? a.starts[gf] : 0;
                if (ok4[q] && !mfcc_frame_in_range(st4[q], L, a.n_samples)) {  // the host checked: never read out of bounds
                    ok4[q] = false;
                    sFlag[f] = 1;
                }
            }
            for (int n = lane; n < Hp; n += 64) {
                const bool in = n < H, pair = in && n > 0 && 2 * n < L;
                const double w0 = in ? a.window[n] : 0.0, w1 = pair ? a.window[L - n] : 0.0;
                double x0[Q], x1[Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    x0[q] = ok4[q] && in ? a.x[st4[q] + n] : 0.0;
                    x1[q] = ok4[q] && pair ? a.x[st4[q] + L - n] : 0.0;
                }
#pragma unroll
                for (int q = 0; q < Q; ++q) {
                    const int f = w + kMfccWaves * q;
                    if (!isfinite(x0[q]) || !isfinite(x1[q])) {
                        sFlag[f] = 1;
                        if (!isfinite(x0[q])) x0[q] = 0.0;
                        if (!isfinite(x1[q])) x1[q] = 0.0;
                    }
                    const double y0 = x0[q] * w0, y1 = x1[q] * w1;  // y1 = 0 where n has no partner
                    sE[f * Hs + n] = y0 + y1;
                    sO[f * Hs + n] = pair ? y0 - y1 : 0.0;
                }
            }
        }
        __syncthreads();
        // ---- DFT: P[frame][bin] = Re^2 + Im^2 ----
        {
            f64x4 re[NBW], im[NBW];
            int idx[NBW], step[NBW];
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                re[j] = f64x4{0.0, 0.0, 0.0, 0.0};
                im[j] = f64x4{0.0, 0.0, 0.0, 0.0};
                const int bin = 16 * (w + kMfccWaves * j) + col;  // < 16 (4 NBW) <= 320: the products below fit int
                idx[j] = (bin * g) % L;
                step[j] = (4 * bin) % L;
            }
            const double *pe = sE + col * Hs + g, *po = sO + col * Hs + g;
            for (int ks = 0; ks < Hp; ks += 4) {
                const double ae = pe[ks], ao = po[ks];
#pragma unroll
                for (int j = 0; j < NBW; ++j) {
                    const double2 t = *reinterpret_cast<const double2 *>(sTw + 2 * idx[j]);
                    re[j] = mfma_f64(ae, t.x, re[j]);
                    im[j] = mfma_f64(ao, t.y, im[j]);
                    idx[j] += step[j];
                    if (idx[j] >= L) idx[j] -= L;
                }
            }
            __syncthreads();  // P takes the place of the folded images: every wave has read its A operands
#pragma unroll
            for (int j = 0; j < NBW; ++j) {
                const int blk = w + kMfccWaves * j;
                if (blk < nblk) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        sP[(g + 4 * r) * Ps + 16 * blk + col] = re[j][r] * re[j][r] + im[j][r] * im[j][r];
                }
            }
        }
        __syncthreads();
        // ---- mel bands, decibels ----
        for (int item = tid; item < kMfccTile * n_mels; item += blockDim.x) {
            const int f = item & 15, m = item >> 4;
            const int first = sBand[2 * m], last = sBand[2 * m + 1];
            const double *wrow = a.mel + (long long)m * H, *p = sP + f * Ps;
            double s = 0.0;
            for (int k = first; k <= last; ++k) s += wrow[k] * p[k];
            sDb[f * Ds + m] = 10.0 * log10(fmax(a.amin, s));
        }
        __syncthreads();
        // ---- top_db floor, DCT ----
        for (int item = tid; item < kMfccTile * a.n_mfcc; item += blockDim.x) {
            const int f = item & 15, i = item >> 4;
            const long long gf = tile * kMfccTile + f;
            if (gf >= a.F) continue;  // the ragged last tile's rows are not stored
            const double *db = sDb + f * Ds, *drow = a.dct + i * n_mels;
            double floor_db = -INFINITY;
            if (a.top_db >= 0.0) {
                double mx = db[0];
                for (int m = 1; m < n_mels; ++m) mx = fmax(mx, db[m]);
                floor_db = mx - a.top_db;
            }
            double c = 0.0;
            for (int m = 0; m < n_mels; ++m) c += drow[m] * fmax(db[m], floor_db);
            a.out[gf * a.out_stride + i] = sFlag[f] ? 0.0 : c;
        }
    }
}

struct MfccFlag {
    int *dev = nullptr, *host = nullptr;
    ~MfccFlag() {
        dfree(dev);
        cached_free(host, kPinnedBlock);
    }
};

}  // namespace hmmbw

using namespace hmmbw;

extern "C" int hmmbw_mfcc_tables(int frame_len, double sample_rate, int n_mels, int n_mfcc, double *window,
                                 double *twiddle, double *mel, double *dct) {
    const int v = mfcc_tables_validate(frame_len, sample_rate, n_mels, n_mfcc, window && twiddle && mel && dct);
    if (v == kMfccInvalid)
        return fail(HMMBW_E_INVALID, "hmmbw_mfcc_tables: need frame_len >= 2, sample_rate > 0, n_mels >= 1, "
                                     "1 <= n_mfcc <= n_mels and the four arrays");
    if (v != kMfccOk) return fail(HMMBW_E_UNSUPPORTED, "hmmbw_mfcc_tables: frame_len > 512 or n_mels > 64");
    mfcc_tables(frame_len, sample_rate, n_mels, n_mfcc, window, twiddle, mel, dct);
    return HMMBW_OK;
}

extern "C" int hmmbw_mfcc(void *stream, const double *samples, int64_t n_samples, const int64_t *frame_starts,
                          int64_t n_frames, int frame_len, const double *window, const double *twiddle,
                          const double *mel, int n_mels, const double *dct, int n_mfcc, double amin, double top_db,
                          double *out, int64_t out_stride) {
    const int v = mfcc_validate(n_samples, n_frames, frame_len, n_mels, n_mfcc, amin, out_stride,
                                samples && frame_starts && window && twiddle && mel && dct && out);
    if (v == kMfccInvalid)
        return fail(HMMBW_E_INVALID, "hmmbw_mfcc: need n_frames >= 0, frame_len >= 2, frames within n_samples, "
                                     "n_mels >= 1, 1 <= n_mfcc <= n_mels, out_stride >= n_mfcc, amin > 0 and every "
                                     "pointer");
    if (v != kMfccOk) return fail(HMMBW_E_UNSUPPORTED, "hmmbw_mfcc: frame_len > 512 or n_mels > 64");
    if (n_frames == 0) return HMMBW_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    {  // the frame table lives on the device: one pass over it and 4 bytes back before anything reads through it
        MfccFlag fl;
        if (int rc = dalloc(&fl.dev, 1)) return rc;
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&fl.host), sizeof(int), kPinnedBlock));
        HIP_TRY(hipMemsetAsync(fl.dev, 0, sizeof(int), st));
        const unsigned cg = (unsigned)std::min<long long>((n_frames + 255) / 256, 1024);
        hipLaunchKernelGGL(k_mfcc_check, dim3(cg), dim3(256), 0, st, (const long long *)frame_starts,
                           (long long)n_frames, frame_len, (long long)n_samples, fl.dev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(fl.host, fl.dev, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (*fl.host) return fail(HMMBW_E_INVALID, "hmmbw_mfcc: a frame starts before 0 or runs past n_samples");
    }
    MfccArgs a{};
    a.x = samples;
    a.starts = reinterpret_cast<const long long *>(frame_starts);
    a.window = window;
    a.twiddle = twiddle;
    a.mel = mel;
    a.dct = dct;
    a.out = out;
    a.n_samples = n_samples;
    a.F = n_frames;
    a.ntiles = (n_frames + kMfccTile - 1) / kMfccTile;
    a.out_stride = out_stride;
    a.L = frame_len;
    a.n_mels = n_mels;
    a.n_mfcc = n_mfcc;
    a.amin = amin;
    a.top_db = top_db;
    const size_t lds = mfcc_lds_bytes(frame_len, n_mels);
    if (lds > kMfccLdsBudget) return fail(HMMBW_E_UNSUPPORTED, "hmmbw_mfcc: the tile does not fit the LDS");
    const int nbw = (mfcc_bin_blocks(frame_len) + kMfccWaves - 1) / kMfccWaves;
    void (*kern)(MfccArgs) = nullptr;
    switch (nbw) {
        case 1: kern = k_mfcc<1>; break;
        case 2: kern = k_mfcc<2>; break;
        case 3: kern = k_mfcc<3>; break;
        case 4: kern = k_mfcc<4>; break;
        case 5: kern = k_mfcc<5>; break;
        default: return fail(HMMBW_E_UNSUPPORTED, "hmmbw_mfcc: frame_len > 512");
    }
    if (lds > 64 * 1024)
        if (int rc = allow_lds(reinterpret_cast<const void *>(kern), lds)) return rc;
    const unsigned grid = (unsigned)std::min<long long>(a.ntiles, kMfccMaxGrid);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * kMfccWaves), lds, st, a);
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}
