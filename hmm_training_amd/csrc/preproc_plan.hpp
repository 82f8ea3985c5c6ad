// preproc_plan.hpp — the pure part of hmmbw_preprocess and hmmbw_window_overlap (preproc.hip): the frame count of a
// recording and the odd length of its last frame, the frame count and the partial frame of the overlapping window,
// argument validation and launch shapes.  The arithmetic restated is the reference's filter_signal / slice_signal
// (preemphasis.py:174-294; HMM/live_testing.py:48-120 is slice_signal with two pairs of thresholds) and
// hamming_window (preemphasis.py:189-212).  Plain C++17 with no HIP dependency, so that a host compiler can build a
// probe of it (tests/native/preproc_plan_probe.cpp); the kernels and the host code of preproc.hip both call it.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HMMBW_HD __host__ __device__
#else
#define HMMBW_HD
#endif

namespace hmmbw {

constexpr int kPreOk = 0, kPreInvalid = -1, kPreUnsupported = -3;  // HMMBW_OK / _E_INVALID / _E_UNSUPPORTED

constexpr int kPreMaxWin = 1 << 16;      // frame sums index a frame with an int and count crossings in a double
constexpr int kPreMaxCover = 8;          // frames of the overlapping window that cover one sample: ceil(wlen / whop)
constexpr int kPreMaxWlen = 1 << 16;
constexpr int kPreLdsFrames = 1024;      // a recording of at most this many frames keeps its statistics in the LDS
constexpr long long kPreMaxRec = (1LL << 31) - 1;  // recordings per call (one workgroup each: the grid's x)
constexpr long long kPreMaxSamples = 1LL << 46;

// ---- frames of the statistics (slice_signal) ----
// int((n - win) / hop) + 1 with Python's int(): truncation toward zero, which C++'s division is as well.  A recording
// shorter than win still has one frame while n > win - hop.
HMMBW_HD constexpr long long pre_frame_count(long long n, int win, int hop) { return (n - win) / hop + 1; }
// a recording the reference can process: at least one frame, and that frame not empty (it spares the last sample)
HMMBW_HD constexpr bool pre_rec_ok(long long n, int win, int hop) { return n >= 2 && pre_frame_count(n, win, hop) >= 1; }
// frame i < nf - 1 has win samples from i hop; the last one runs from (nf - 1) hop to n - 1 (exclusive)
HMMBW_HD constexpr long long pre_frame_len(long long n, int win, int hop, long long i) {
    return i < pre_frame_count(n, win, hop) - 1 ? win : n - 1 - i * hop;
}
HMMBW_HD constexpr long long pre_last_frame_len(long long n, int win, int hop) {
    return pre_frame_len(n, win, hop, pre_frame_count(n, win, hop) - 1);
}

// ---- the overlapping window (hamming_window) over a trimmed signal of m samples ----
// q full frames; q < 0: nothing happens at all
HMMBW_HD constexpr long long pre_window_frames(long long m, int wlen, int whop) { return (m - wlen) / whop + 1; }
// the partial frame q covers [q whop, m - 1) with the table's first entries (0 where q < 0 or nothing is left)
HMMBW_HD constexpr long long pre_window_partial(long long m, int wlen, int whop) {
    const long long q = pre_window_frames(m, wlen, whop);
    if (q < 0) return 0;
    const long long left = m - 1 - q * whop;
    return left < 0 ? 0 : (left < wlen ? left : wlen);
}
HMMBW_HD constexpr int pre_window_cover(int wlen, int whop) { return (wlen + whop - 1) / whop; }

// ---- validation: what the host can see (rec_offsets_host may be absent: the lengths are then the device's matter) ----
HMMBW_HD inline int pre_validate(long long n_rec, int sample_kind, double coeff, int win, int hop, const double *factors,
                                 bool have_pointers) {
    if (n_rec < 0 || (sample_kind != 0 && sample_kind != 1) || !have_pointers || !factors) return kPreInvalid;
    if (win < 2 || hop < 1 || hop > win || !(coeff == coeff)) return kPreInvalid;
    for (int i = 0; i < 4; ++i)
        if (!(factors[i] == factors[i])) return kPreInvalid;  // NaN
    if (win > kPreMaxWin || n_rec > kPreMaxRec) return kPreUnsupported;
    return kPreOk;
}
// the offsets as the host knows them: ascending from 0, every recording one the reference can process
inline int pre_validate_offsets(const long long *off, long long n_rec, int win, int hop) {
    if (n_rec > 0 && off[0] != 0) return kPreInvalid;
    for (long long r = 0; r < n_rec; ++r) {
        if (off[r + 1] < off[r]) return kPreInvalid;
        if (!pre_rec_ok(off[r + 1] - off[r], win, hop)) return kPreInvalid;
    }
    if (n_rec > 0 && off[n_rec] > kPreMaxSamples) return kPreUnsupported;
    return kPreOk;
}
HMMBW_HD inline int pre_window_validate(long long n_rec, int wlen, int whop, bool have_pointers) {
    if (n_rec < 0 || wlen < 1 || whop < 1 || !have_pointers) return kPreInvalid;
    if (wlen > kPreMaxWlen || pre_window_cover(wlen, whop) > kPreMaxCover || n_rec > kPreMaxRec) return kPreUnsupported;
    return kPreOk;
}

// ---- launch shapes ----
// hmmbw_preprocess: one workgroup per recording (the maxima and the first / last search stay inside it); few
// recordings get 16 waves each (the live case: one recording, latency), many get 4 (more workgroups per CU)
HMMBW_HD constexpr int pre_block(long long n_rec) { return n_rec < 512 ? 1024 : 256; }
// hmmbw_window_overlap: every sample on its own, so a recording is spread over `y` workgroups of 256 lanes
HMMBW_HD constexpr int pre_window_chunks(long long n_rec) {
    return n_rec >= 1024 ? 1 : (n_rec <= 16 ? 64 : (int)(1024 / n_rec));
}

}  // namespace hmmbw
