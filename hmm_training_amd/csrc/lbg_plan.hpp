// lbg_plan.hpp — the pure part of hmmbw_lbg_train (lbg.hip): argument validation, the LDS bound, the offsets of the
// generations in the [2K - 1]-row output, and the state machine that the update kernel advances once per pass (the
// reference's stop rule, its split indexing and the record count; createCodeVector,
// CodeVector/codevector_functions.py:442-531).  Plain C++17 with no HIP dependency, so that a host compiler can build
// a probe of it (tests/native/lbg_plan_probe.cpp); the kernel and the host code of lbg.hip both call it.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HMMBW_HD __host__ __device__
#else
#define HMMBW_HD
#endif

namespace hmmbw {

constexpr int kLbgOk = 0, kLbgInvalid = -1, kLbgUnsupported = -3;  // HMMBW_OK / _E_INVALID / _E_UNSUPPORTED

// LDS of one assign-and-accumulate workgroup: K rows of (stride sums + 1 count), the distortion slot, and, when the
// scan is not the scalar-load form of the reference's 12 dims, the staged codebook [K][dims].  The bound is the
// CU's whole 160 KiB (one workgroup per CU then): K = 1024 at stride 13 needs 112 KiB + 8 B with scalar loads.
constexpr size_t kLbgLdsBudget = size_t(160) << 10;
constexpr int kLbgScalarDims = 12;   // the scan that reads centroid rows with scalar loads (vq_scan.hpp)
constexpr int kLbgMaxStagedDims = 64;  // registers of the LDS-staged scan
constexpr int kLbgCopies = 4;        // global accumulator copies the workgroups' flushes are spread over
constexpr int kLbgChunk = 16;        // passes enqueued between two reads of the device state (and the record ring)

HMMBW_HD constexpr long long lbg_acc_doubles(int K, int stride) { return 1 + (long long)K * (stride + 1); }
HMMBW_HD constexpr bool lbg_scan_staged(int dims) { return dims != kLbgScalarDims; }
HMMBW_HD constexpr long long lbg_lds_doubles(int K, int stride, int dims) {
    return lbg_acc_doubles(K, stride) + (lbg_scan_staged(dims) ? (long long)K * dims : 0);
}
HMMBW_HD constexpr size_t lbg_lds_bytes(int K, int stride, int dims) {
    return (size_t)lbg_lds_doubles(K, stride, dims) * sizeof(double);
}

HMMBW_HD constexpr bool lbg_pow2(long long k) { return k >= 2 && (k & (k - 1)) == 0; }
// G = int(log2(K)) generations after c0
HMMBW_HD constexpr int lbg_generations(long long K) {
    int g = 0;
    while (K > 1) {
        K >>= 1;
        ++g;
    }
    return g;
}
// first row of generation g (g = 0 is c0, one row; generation g has 2^g rows) in the generations output
HMMBW_HD constexpr long long lbg_gen_offset(int g) { return (1LL << g) - 1; }
HMMBW_HD constexpr long long lbg_gen_rows(int g) { return 1LL << g; }
HMMBW_HD constexpr long long lbg_total_rows(int K) { return 2LL * K - 1; }
// passes (c0's accumulate pass not counted) a call can make at the most; saturates
HMMBW_HD constexpr long long lbg_max_passes(int G, long long max_iterations) {
    return max_iterations > (INT64_MAX - 1) / (G > 0 ? G : 1) ? INT64_MAX - 1 : (long long)G * max_iterations;
}

// the arguments of hmmbw_lbg_train that do not need the device (pointers as "is it there")
HMMBW_HD inline int lbg_validate(long long n_frames, int stride, int first_dim, int dims, int K, double epsilon,
                                 long long max_iterations, bool have_frames, bool have_centroids) {
    if (n_frames < 1 || !lbg_pow2(K) || dims < 1 || first_dim < 0 || stride < 1) return kLbgInvalid;
    if ((long long)first_dim + dims > stride) return kLbgInvalid;
    if (max_iterations < 1 || !(epsilon >= 0.0)) return kLbgInvalid;  // !(>=): negative or NaN
    if (!have_frames || !have_centroids) return kLbgInvalid;
    if (lbg_scan_staged(dims) && dims > kLbgMaxStagedDims) return kLbgUnsupported;
    if (K > (1 << 20) || stride > (1 << 16)) return kLbgUnsupported;  // keeps the sizes below in range
    if (lbg_lds_bytes(K, stride, dims) > kLbgLdsBudget) return kLbgUnsupported;
    if (n_frames > (1LL << 40)) return kLbgUnsupported;
    return kLbgOk;
}

// The device-side state.  generation 0 is the c0 pass: every frame goes to row 0 without a scan.
struct LbgState {
    int32_t generation;
    int32_t K_now;
    int32_t done;
    int32_t pad;
    long long iteration;  // passes made in this generation
    long long n_records;  // passes made in all generations
    double prev;          // the previous pass's distortion (0 at the start of a generation)
};
HMMBW_HD inline LbgState lbg_initial_state() { return LbgState{0, 1, 0, 0, 0, 0, 0.0}; }

struct LbgStep {
    bool record;  // the pass counts (not c0): append (generation, iteration, distortion, diff)
    bool stop;    // the generation ends with this pass: copy it to the generations output
    bool split;   // ... and the next generation starts from its split
    int generation;  // the generation this pass belonged to
    long long iteration;
    double diff;
};

// the reference's loop condition (:485), negated: a NaN diff stops (NaN > eps is false)
HMMBW_HD inline bool lbg_stop(double diff, double epsilon, long long iteration, long long max_iterations) {
    return !(diff > epsilon && iteration < max_iterations);
}

// One pass has been accumulated with distortion `dist`: advance the state (:509-521).
HMMBW_HD inline LbgStep lbg_advance(LbgState &s, double dist, double epsilon, long long max_iterations, int G) {
    LbgStep r{};
    r.generation = s.generation;
    if (s.generation == 0) {
        r.stop = true;
    } else {
        s.iteration += 1;
        s.n_records += 1;
        r.diff = __builtin_fabs(s.prev - dist);  // NaN stays NaN
        s.prev = dist;
        r.record = true;
        r.iteration = s.iteration;
        r.stop = lbg_stop(r.diff, epsilon, s.iteration, max_iterations);
    }
    if (r.stop) {
        if (s.generation < G) {
            r.split = true;
            s.generation += 1;
            s.K_now *= 2;
            s.iteration = 0;
            s.prev = 0.0;
        } else {
            s.done = 1;
        }
    }
    return r;
}

}  // namespace hmmbw
