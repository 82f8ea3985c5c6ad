// lbg.hip — LBG codebook training (hmmbw_lbg_train, include/hmmbw.h) for gfx950: the reference's createCodeVector,
// CodeVector/codevector_functions.py:442-531 (MFCC variant), three nested Python loops there.
//
// One pass = two launches.
//   k_lbg_assign_*: lanes own frames as in the encoder and run the encoder's scan (vq_scan.hpp: the one copy of the
//     bit-exact arithmetic); each lane then adds its frame's whole row and a count into per-workgroup LDS accumulators
//     [K][stride + 1] (ds_add_f64), its winning distance into a distortion slot, and the workgroup flushes the lot to
//     one of kLbgCopies global accumulator copies with fp64 atomics.  Workgroups loop over frame tiles, so a launch
//     flushes at most kLbgMaxGrid times however many frames there are.  With K = 2..8 every lane of a ds_add_f64
//     hits the same few addresses; reducing the rows per cluster across the wave first (lane_ops.hpp's gsum) was
//     measured against that at K = 2, 8 and 64 and lost at all three (0.38 / 0.39 / 1.39 ms per pass of 2M frames
//     against 0.15 / 0.14 / 0.23 ms, profiles/lbg/bench_lbg.json), so per-lane LDS atomics serve every K; the
//     reduced form stays behind HMMBW_LBG_WAVE_K for that A/B (tools/lbg_bench.py) and its test.
//   k_lbg_update (one workgroup): folds the copies in a fixed order, writes the means (zeros for an empty cluster),
//     clears the accumulators, and advances the device-side state (lbg_plan.hpp: stop rule, record, split), so that
//     the host never decides anything per pass.  The assign kernel reads the number of centroids in use from that
//     state and both kernels are no-ops once it says done.
// c0 is the same accumulate path with every frame in row 0 and no scan (state.generation == 0).
// The host enqueues kLbgChunk passes, reads the state and the chunk's records back, and goes on until done.
#include "host.hpp"
#include "lane_ops.hpp"
#include "lbg_plan.hpp"
#include "vq_scan.hpp"

namespace hmmbw {

constexpr unsigned kLbgMaxGrid = 1024;  // 4 workgroups per CU
constexpr int kLbgFpl = 2;              // frames per lane of the scalar-load scan, as the encoder's

struct LbgDev {
    LbgState st;
    hmmbw_lbg_record ring[kLbgChunk];  // record r of the call sits in slot r % kLbgChunk
};

struct LbgArgs {
    long long F, ntiles, accL;  // accL: doubles of one global accumulator copy = lbg_acc_doubles(Kmax, stride)
    int stride, col0, dims, Kmax, wave_k, G;
    double *acc;     // [kLbgCopies][accL]: [0] distortion, then K rows of (stride sums, count)
    double *means;   // the caller's centroids buffer: the means of the last update
    double *gens;    // or nullptr
    int *assign;     // or nullptr
    LbgDev *dev;
    double eps, up, down;
    long long max_it;
};

// Add the rows of this lane's FPL frames (first frame f0; arg / dist from the scan) into the workgroup's accumulators.
template <int FPL>
__device__ __forceinline__ void lbg_accumulate(const LbgArgs &a, const double *__restrict__ frames, double *sAcc, int K,
                                               bool with_dist, long long f0, const int (&arg)[FPL],
                                               const double (&dist)[FPL]) {
    const int W = a.stride + 1;
    bool valid[FPL];
#pragma unroll
    for (int q = 0; q < FPL; ++q) valid[q] = f0 + q < a.F;
    if (K <= a.wave_k) {
        // the A/B form: per cluster across the wave first (every lane takes part: the loops are wave-uniform)
        const bool lead = (threadIdx.x & 63) == 0;
        for (int c = 0; c < W; ++c) {
            double v[FPL];
#pragma unroll
            for (int q = 0; q < FPL; ++q) v[q] = !valid[q] ? 0.0 : (c < a.stride ? frames[(f0 + q) * a.stride + c] : 1.0);
            for (int k = 0; k < K; ++k) {
                double s = 0.0;
#pragma unroll
                for (int q = 0; q < FPL; ++q) s += (valid[q] && arg[q] == k) ? v[q] : 0.0;
                s = gsum<64>(s);
                if (lead && s != 0.0) atomicAdd(&sAcc[1 + k * W + c], s);
            }
        }
    } else {
#pragma unroll
        for (int q = 0; q < FPL; ++q) {
            if (!valid[q]) continue;
            double *row = sAcc + 1 + arg[q] * W;
            const double *fr = frames + (f0 + q) * a.stride;
            for (int c = 0; c < a.stride; ++c) atomicAdd(&row[c], fr[c]);
            atomicAdd(&row[a.stride], 1.0);
        }
    }
    if (with_dist) {
        double d = 0.0;
#pragma unroll
        for (int q = 0; q < FPL; ++q) d += valid[q] ? dist[q] : 0.0;
        d = gsum<64>(d);
        if ((threadIdx.x & 63) == 0 && d != 0.0) atomicAdd(&sAcc[0], d);
    }
    if (a.assign) {
#pragma unroll
        for (int q = 0; q < FPL; ++q)
            if (valid[q]) a.assign[f0 + q] = arg[q];
    }
}

__device__ __forceinline__ void lbg_flush(const LbgArgs &a, const double *sAcc, int n) {
    double *g = a.acc + (long long)(blockIdx.x % kLbgCopies) * a.accL;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = sAcc[i];
        if (v != 0.0) unsafeAtomicAdd(&g[i], v);
    }
}

// STAGED = false: D = 12 scanned columns, centroid rows by scalar loads, kLbgFpl frames per lane.
// STAGED = true: any dims <= 64, the codebook's scanned columns staged in LDS behind the accumulators.
template <bool STAGED>
__global__ void __launch_bounds__(256) k_lbg_assign(const double *__restrict__ frames, const double *__restrict__ cents,
                                                    LbgArgs a) {
    extern __shared__ double sAcc[];
    constexpr int FPL = STAGED ? 1 : kLbgFpl;
    if (a.dev->st.done) return;
    const int gen = __builtin_amdgcn_readfirstlane(a.dev->st.generation);
    const int K = __builtin_amdgcn_readfirstlane(a.dev->st.K_now);  // <= Kmax: lbg_advance doubles it only below G
    const int n = (int)lbg_acc_doubles(K, a.stride);
    for (int i = threadIdx.x; i < n; i += blockDim.x) sAcc[i] = 0.0;
    double *sC = sAcc + lbg_acc_doubles(a.Kmax, a.stride);
    if (STAGED && gen > 0) vq_stage_codebook(sC, cents, a.stride, a.col0, a.dims, K);
    __syncthreads();
    for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const long long f0 = (tile * 256 + threadIdx.x) * FPL;
        int arg[FPL];
        double dist[FPL];
#pragma unroll
        for (int q = 0; q < FPL; ++q) {
            arg[q] = 0;
            dist[q] = 0.0;
        }
        if (gen > 0) {
            if constexpr (STAGED) {
                double x[kLbgMaxStagedDims];
                const long long f = f0 < a.F ? f0 : a.F - 1;
#pragma unroll
                for (int d = 0; d < kLbgMaxStagedDims; ++d) x[d] = (d < a.dims) ? frames[f * a.stride + a.col0 + d] : 0.0;
                vq_scan_lds<kLbgMaxStagedDims>(x, a.dims, sC, K, dist[0], arg[0]);
            } else {
                double x[FPL][kLbgScalarDims];
#pragma unroll
                for (int q = 0; q < FPL; ++q) {
                    const long long f = f0 + q < a.F ? f0 + q : a.F - 1;
#pragma unroll
                    for (int d = 0; d < kLbgScalarDims; ++d) x[q][d] = frames[f * a.stride + a.col0 + d];
                }
                vq_scan_scalar<kLbgScalarDims, FPL>(x, cents + a.col0, a.stride, K, dist, arg);
            }
        }
        lbg_accumulate<FPL>(a, frames, sAcc, K, gen > 0, f0, arg, dist);
    }
    __syncthreads();
    lbg_flush(a, sAcc, n);
}

__global__ void __launch_bounds__(256) k_lbg_update(double *__restrict__ cents, LbgArgs a) {
    __shared__ LbgStep s_step;
    LbgState *st = &a.dev->st;
    if (st->done) return;
    const int K = st->K_now;
    const int W = a.stride + 1, tid = threadIdx.x;
    __syncthreads();  // every thread has read the state that thread 0 advances below
    for (int i = tid; i < K * a.stride; i += blockDim.x) {
        const int k = i / a.stride, c = i - k * a.stride;
        double sum = 0.0, cnt = 0.0;
        for (int cp = 0; cp < kLbgCopies; ++cp) {  // fixed order
            const double *g = a.acc + cp * a.accL + 1 + (long long)k * W;
            sum += g[c];
            cnt += g[a.stride];
        }
        a.means[i] = cnt > 0.0 ? sum / cnt : 0.0;  // np.mean: the sum divided by the count; np.zeros when empty
    }
    double dist = 0.0;
    if (tid == 0)
        for (int cp = 0; cp < kLbgCopies; ++cp) dist += a.acc[cp * a.accL];
    __syncthreads();
    const int n = (int)lbg_acc_doubles(K, a.stride);
    for (int cp = 0; cp < kLbgCopies; ++cp)
        for (int i = tid; i < n; i += blockDim.x) a.acc[cp * a.accL + i] = 0.0;
    if (tid == 0) {
        LbgState s = *st;
        const LbgStep r = lbg_advance(s, dist, a.eps, a.max_it, a.G);
        if (r.record) {
            hmmbw_lbg_record &rec = a.dev->ring[(s.n_records - 1) % kLbgChunk];
            rec.generation = r.generation;
            rec.iteration = (int32_t)r.iteration;
            rec.distortion = dist;
            rec.diff = r.diff;
        }
        *st = s;
        s_step = r;
    }
    __syncthreads();
    const LbgStep r = s_step;
    for (int i = tid; i < K * a.stride; i += blockDim.x) {
        const double m = a.means[i];
        if (r.stop && a.gens) a.gens[lbg_gen_offset(r.generation) * a.stride + i] = m;
        if (r.split) {  // row k -> rows 2k and 2k + 1 of the next generation (:394-409)
            const int k = i / a.stride, c = i - k * a.stride;
            cents[(2 * k) * a.stride + c] = m * a.up;
            cents[(2 * k + 1) * a.stride + c] = m * a.down;
        } else if (!r.stop) {
            cents[i] = m;
        }
    }
}

// HMMBW_LBG_WAVE_K (diagnostics, tools/lbg_bench.py's A/B): the largest K whose rows are reduced across the wave
// before the LDS atomics.  Default 0 = never: the measurement is in DESIGN §6 "LBG codebook training".
constexpr int kLbgWaveK = 0;
static int lbg_wave_k() {
    const char *e = std::getenv("HMMBW_LBG_WAVE_K");
    return e && *e ? std::atoi(e) : kLbgWaveK;
}

struct LbgWork {
    double *cents = nullptr, *acc = nullptr;
    LbgDev *dev = nullptr, *host = nullptr;
    ~LbgWork() {
        dfree(cents);
        dfree(acc);
        dfree(dev);
        cached_free(host, kPinnedBlock);
    }
};

}  // namespace hmmbw

extern "C" int hmmbw_lbg_train(void *stream, const double *frames, int64_t n_frames, int frame_stride, int first_dim,
                               int dims, int n_centroids, double epsilon, int64_t max_iterations, double split_up,
                               double split_down, double *centroids, double *generations, int32_t *assignments,
                               hmmbw_lbg_record *records, int64_t records_cap, int64_t *n_records) {
    const int v = lbg_validate(n_frames, frame_stride, first_dim, dims, n_centroids, epsilon, max_iterations,
                               frames != nullptr, centroids != nullptr);
    if (v == kLbgInvalid)
        return fail(HMMBW_E_INVALID,
                    "hmmbw_lbg_train: need n_frames >= 1 (No raw data provided), n_centroids a power of two >= 2, "
                    "dims >= 1, 0 <= first_dim, first_dim + dims <= frame_stride, max_iterations >= 1, epsilon >= 0, "
                    "frames and centroids");
    if (v != kLbgOk)
        return fail(HMMBW_E_UNSUPPORTED, "hmmbw_lbg_train: accumulators (and staged codebook) beyond 160 KiB of LDS, "
                                         "or dims > 64 other than 12");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int K = n_centroids, G = lbg_generations(K);
    const bool staged = lbg_scan_staged(dims);
    LbgWork w;
    LbgArgs a{};
    a.F = n_frames;
    a.ntiles = (n_frames + 256 * (staged ? 1 : kLbgFpl) - 1) / (256 * (staged ? 1 : kLbgFpl));
    a.accL = lbg_acc_doubles(K, frame_stride);
    a.stride = frame_stride;
    a.col0 = first_dim;
    a.dims = dims;
    a.Kmax = K;
    a.wave_k = lbg_wave_k();
    a.G = G;
    a.eps = epsilon;
    a.up = split_up;
    a.down = split_down;
    a.max_it = max_iterations;
    if (int rc = dalloc(&w.cents, (size_t)K * frame_stride)) return rc;
    if (int rc = dalloc(&w.acc, (size_t)kLbgCopies * a.accL)) return rc;
    if (int rc = dalloc(&w.dev, 1)) return rc;
    HIP_TRY(cached_alloc(reinterpret_cast<void **>(&w.host), sizeof(LbgDev), kPinnedBlock));
    a.acc = w.acc;
    a.means = centroids;
    a.gens = generations;
    a.assign = assignments;
    a.dev = w.dev;
    const size_t lds = lbg_lds_bytes(K, frame_stride, dims);
    auto assign = staged ? k_lbg_assign<true> : k_lbg_assign<false>;
    if (lds > 64 * 1024)
        if (int rc = allow_lds(reinterpret_cast<const void *>(assign), lds)) return rc;
    const unsigned grid = (unsigned)std::min<long long>(a.ntiles, kLbgMaxGrid);

    *w.host = LbgDev{};
    w.host->st = lbg_initial_state();
    HIP_TRY(hipMemcpyAsync(w.dev, w.host, sizeof(LbgDev), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(w.acc, 0, sizeof(double) * kLbgCopies * a.accL, st));
    HIP_TRY(hipStreamSynchronize(st));  // the pinned block is read back into below
    const long long bound = 1 + lbg_max_passes(G, max_iterations);  // c0's pass and every generation to its cap
    long long enq = 0, seen = 0;
    bool done = false;
    while (!done && enq < bound) {
        const long long nq = std::min<long long>(kLbgChunk, bound - enq);
        for (long long i = 0; i < nq; ++i) {
            hipLaunchKernelGGL(assign, dim3(grid), dim3(256), lds, st, frames, (const double *)w.cents, a);
            hipLaunchKernelGGL(k_lbg_update, dim3(1), dim3(256), 0, st, w.cents, a);
        }
        HIP_TRY(hipGetLastError());
        enq += nq;
        HIP_TRY(hipMemcpyAsync(w.host, w.dev, sizeof(LbgDev), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const LbgState &s = w.host->st;
        for (; seen < s.n_records; ++seen)
            if (records && seen < records_cap) records[seen] = w.host->ring[seen % kLbgChunk];
        done = s.done != 0;
    }
    if (!done) return fail(HMMBW_E_STATE, "hmmbw_lbg_train: the device state did not reach done within its bound");
    if (n_records) *n_records = seen;
    return HMMBW_OK;
}
