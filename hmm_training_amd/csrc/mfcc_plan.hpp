// mfcc_plan.hpp — the pure part of hmmbw_mfcc (mfcc.hip): argument validation, the frame table of a signal, the padded
// sizes and the LDS layout of one 16-frame tile, and the builder of the tables the kernel reads (window, twiddles, mel
// filter bank, DCT).  The arithmetic restated is librosa.feature.mfcc(y=frame, sr, n_mfcc, n_fft=len(frame),
// hop_length=None, center=False, n_mels) as RawDataMFCC.calculate_mfcc calls it (CodeVector/codevector_classes.py:
// 226-250); the framing is AudioProcessor._split_into_frames_with_overlap (:413-431).  Plain C++17 with no HIP
// dependency, so that a host compiler can build a probe of it (tests/native/mfcc_plan_probe.cpp); the kernel and the
// host code of mfcc.hip both call it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define HMMBW_HD __host__ __device__
#else
#define HMMBW_HD
#endif

namespace hmmbw {

constexpr int kMfccOk = 0, kMfccInvalid = -1, kMfccUnsupported = -3;  // HMMBW_OK / _E_INVALID / _E_UNSUPPORTED

constexpr int kMfccTile = 16;          // frames per workgroup tile = MFMA rows
constexpr int kMfccMaxFrameLen = 512;  // the tile's folded frames, twiddles and spectrum stay within the CU's LDS
constexpr int kMfccMaxMels = 64;
constexpr int kMfccMinTail = 12;       // a remainder frame needs MORE samples than this (:428)
constexpr size_t kMfccLdsBudget = size_t(160) << 10;

// ---- sizes ----
HMMBW_HD constexpr int mfcc_half(int L) { return L / 2 + 1; }                      // H: samples after the fold = bins
HMMBW_HD constexpr int mfcc_half_padded(int L) { return (mfcc_half(L) + 3) & ~3; }  // the MFMA's k = 4
HMMBW_HD constexpr int mfcc_bins_padded(int L) { return (mfcc_half(L) + 15) & ~15; }  // the MFMA's 16 columns
// row strides (doubles) of the LDS images: folded samples [16][Hs], Hs = 2 mod 4, so that the A-operand read (16
// rows x 2 consecutive columns per half-wave) touches 32 different 8-byte banks; power spectrum [16][Ps], Ps odd, so
// that the 16 frames of one bin sit in different banks for the mel sums
HMMBW_HD constexpr int mfcc_fold_stride(int L) { return mfcc_half_padded(L) + 2; }
HMMBW_HD constexpr int mfcc_power_stride(int L) { return mfcc_bins_padded(L) + 1; }
HMMBW_HD constexpr int mfcc_db_stride(int n_mels) { return n_mels | 1; }

// the LDS of one workgroup, in doubles, in this order
struct MfccLds {
    int twiddle, even, odd, power, db, band, flag, total;
};
HMMBW_HD constexpr MfccLds mfcc_lds(int L, int n_mels) {
    MfccLds l{};
    l.twiddle = 0;                                       // [L][2]
    l.even = l.twiddle + 2 * L;                          // [16][Hs]
    l.odd = l.even + kMfccTile * mfcc_fold_stride(L);    // [16][Hs]
    l.power = l.even;                                    // [16][Ps]: written when the folded images are spent
    const int fold = 2 * kMfccTile * mfcc_fold_stride(L), power = kMfccTile * mfcc_power_stride(L);
    l.db = l.even + (fold > power ? fold : power);       // [16][Ds]
    l.band = l.db + kMfccTile * mfcc_db_stride(n_mels);  // int [n_mels][2]: first, last
    l.flag = l.band + n_mels;                            // int [16]
    l.total = l.flag + kMfccTile / 2;
    return l;
}
HMMBW_HD constexpr size_t mfcc_lds_bytes(int L, int n_mels) { return (size_t)mfcc_lds(L, n_mels).total * sizeof(double); }
// 16 x 16 output blocks of one tile, and the matrix instructions of one tile (real and imaginary sums)
HMMBW_HD constexpr int mfcc_bin_blocks(int L) { return mfcc_bins_padded(L) / 16; }
HMMBW_HD constexpr long long mfcc_tile_mfmas(int L, int waves) {
    const int per_wave = (mfcc_bin_blocks(L) + waves - 1) / waves;  // every wave runs the same count
    return 2LL * waves * per_wave * (mfcc_half_padded(L) / 4);
}

// ---- validation: the arguments of hmmbw_mfcc that do not need the device (pointers as "are they all there") ----
HMMBW_HD inline int mfcc_validate(long long n_samples, long long n_frames, int frame_len, int n_mels, int n_mfcc,
                                  double amin, long long out_stride, bool have_pointers) {
    if (n_frames < 0 || n_samples < 0 || frame_len < 2 || n_mels < 1 || n_mfcc < 1 || n_mfcc > n_mels)
        return kMfccInvalid;
    if (out_stride < n_mfcc || !(amin > 0.0) || !have_pointers) return kMfccInvalid;  // !(>): zero, negative or NaN
    if (frame_len > kMfccMaxFrameLen || n_mels > kMfccMaxMels) return kMfccUnsupported;
    if (n_frames > (1LL << 40) || n_samples > (1LL << 46)) return kMfccUnsupported;
    if (n_frames > 0 && frame_len > n_samples) return kMfccInvalid;  // no frame fits
    return kMfccOk;
}
HMMBW_HD constexpr bool mfcc_frame_in_range(long long start, int frame_len, long long n_samples) {
    return start >= 0 && start <= n_samples - frame_len;
}
// the arguments of hmmbw_mfcc_tables
HMMBW_HD inline int mfcc_tables_validate(int frame_len, double sample_rate, int n_mels, int n_mfcc, bool have_pointers) {
    if (frame_len < 2 || n_mels < 1 || n_mfcc < 1 || n_mfcc > n_mels || !(sample_rate > 0.0) || !have_pointers)
        return kMfccInvalid;
    if (frame_len > kMfccMaxFrameLen || n_mels > kMfccMaxMels) return kMfccUnsupported;
    return kMfccOk;
}

// ---- the frame table (:413-431): full frames every hop samples, then one remainder frame of its own length ----
HMMBW_HD constexpr long long mfcc_full_frames(long long n_samples, int frame_size, int hop_size) {
    return n_samples >= frame_size ? (n_samples - frame_size) / hop_size + 1 : 0;
}
HMMBW_HD constexpr long long mfcc_tail_len(long long n_samples, int frame_size, int hop_size) {
    const long long last = mfcc_full_frames(n_samples, frame_size, hop_size) * hop_size;
    return last < n_samples && n_samples - last > kMfccMinTail ? n_samples - last : 0;
}
HMMBW_HD constexpr long long mfcc_frame_count(long long n_samples, int frame_size, int hop_size) {
    return mfcc_full_frames(n_samples, frame_size, hop_size) + (mfcc_tail_len(n_samples, frame_size, hop_size) > 0);
}
// starts / lengths have room for mfcc_frame_count entries; returns the count (-1: frame_size or hop_size < 1)
inline long long mfcc_frame_table(long long n_samples, int frame_size, int hop_size, long long *starts,
                                  long long *lengths) {
    if (frame_size < 1 || hop_size < 1 || n_samples < 0) return -1;
    const long long full = mfcc_full_frames(n_samples, frame_size, hop_size);
    for (long long i = 0; i < full; ++i) {
        starts[i] = i * hop_size;
        lengths[i] = frame_size;
    }
    const long long tail = mfcc_tail_len(n_samples, frame_size, hop_size);
    if (tail > 0) {
        starts[full] = full * hop_size;
        lengths[full] = tail;
    }
    return full + (tail > 0);
}

// ---- tables ----
// Slaney's mel scale (librosa.hz_to_mel / mel_to_hz, htk=False): linear below 1 kHz, logarithmic above
inline double mfcc_hz_to_mel(double f) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
inline double mfcc_mel_to_hz(double m) {
    const double f_sp = 200.0 / 3, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return m >= min_log_mel ? min_log_hz * std::exp(logstep * (m - min_log_mel)) : f_sp * m;
}
// mel_frequencies(n, 0, fmax): np.linspace over the mel axis (arange * step + start, the last point set to stop)
inline double mfcc_mel_point(int i, int n, double fmax) {
    const double lo = mfcc_hz_to_mel(0.0), hi = mfcc_hz_to_mel(fmax);
    if (n == 1) return mfcc_mel_to_hz(lo);
    const double step = (hi - lo) / (n - 1);
    return mfcc_mel_to_hz(i == n - 1 ? hi : i * step + lo);
}

// One row of librosa.filters.mel(sr, n_fft = L, n_mels, fmin = 0, fmax = sr / 2, norm = 'slaney'): the triangle is
// computed in fp64 and stored into a float32 array, which is then scaled in place by the fp64 Slaney factor (the
// product in fp64, rounded to float32 again).  The row is returned as fp64 values that are exactly those float32s.
inline void mfcc_mel_row(int m, int L, double sample_rate, int n_mels, double *row) {
    const int H = mfcc_half(L);
    const double fmax = sample_rate / 2;
    const double f0 = mfcc_mel_point(m, n_mels + 2, fmax), f1 = mfcc_mel_point(m + 1, n_mels + 2, fmax),
                 f2 = mfcc_mel_point(m + 2, n_mels + 2, fmax);
    const double d0 = f1 - f0, d1 = f2 - f1, enorm = 2.0 / (f2 - f0);
    const double val = 1.0 / (L * (1.0 / sample_rate));  // np.fft.rfftfreq(n = L, d = 1 / sr)
    for (int k = 0; k < H; ++k) {
        const double fk = k * val;
        const double lower = -(f0 - fk) / d0, upper = (f2 - fk) / d1;
        const double low = lower < upper ? lower : upper;
        const double tri = low > 0.0 ? low : 0.0;  // +0 outside the triangle, whatever the sign of a zero ramp
        const float stored = (float)tri;
        row[k] = (double)(float)((double)stored * enorm);
    }
}
// [first, count] of a filter row: every non-zero lies in [first, first + count); count 0 for an all-zero row
inline void mfcc_band(const double *row, int H, int *first, int *count) {
    int lo = H, hi = -1;
    for (int k = 0; k < H; ++k)
        if (row[k] != 0.0) {
            if (k < lo) lo = k;
            hi = k;
        }
    *first = hi < 0 ? 0 : lo;
    *count = hi < 0 ? 0 : hi - lo + 1;
}

// window [L]: periodic Hann; twiddle [L][2]: cos and sin of 2 pi m / L (long double, rounded once);
// mel [n_mels][L / 2 + 1]; dct [n_mfcc][n_mels]: the first rows of the orthonormal DCT-II
inline void mfcc_tables(int L, double sample_rate, int n_mels, int n_mfcc, double *window, double *twiddle, double *mel,
                        double *dct) {
    const long double two_pi = 2.0L * 3.14159265358979323846264338327950288L;
    for (int n = 0; n < L; ++n) {
        const long double a = two_pi * n / L;
        window[n] = (double)(0.5L - 0.5L * cosl(a));
        twiddle[2 * n] = (double)cosl(a);
        twiddle[2 * n + 1] = (double)sinl(a);
    }
    const int H = mfcc_half(L);
    for (int m = 0; m < n_mels; ++m) mfcc_mel_row(m, L, sample_rate, n_mels, mel + (size_t)m * H);
    for (int i = 0; i < n_mfcc; ++i)
        for (int m = 0; m < n_mels; ++m) {
            const long double scale = i == 0 ? sqrtl(1.0L / n_mels) : sqrtl(2.0L / n_mels);
            dct[i * n_mels + m] = (double)(scale * cosl(two_pi / 2 * i * (2 * m + 1) / (2.0L * n_mels)));
        }
}

}  // namespace hmmbw
