// phase_stamps.hpp — diagnostics builds only: per-wave time stamps inside the E-step kernels.  In the release
// build every macro here is empty.
//   -DHMMBW_PHASE_TIMES (tools/phase_times.py): wall-clock stamps of the small E-step's phases, read back with
//       hmmbw_debug_phase_times.
//   -DHMMBW_CHUNK_TIMES on top of it (tools/phase_times.py --chunks, tools/wide_chunk_times.py): shader-clock
//       stamps per chunk of the sweeps, read back with hmmbw_debug_chunk_times / hmmbw_debug_wide_chunk_times.
#pragma once
#include <hip/hip_runtime.h>

namespace hmmbw {

#ifdef HMMBW_PHASE_TIMES
constexpr int kPhaseWaves = 1 << 16;
constexpr int kPhaseSlots = 16;
static __device__ unsigned long long g_phase[kPhaseWaves][kPhaseSlots];
#define PHASE(k)                                                                               \
    do {                                                                                       \
        const long long w_ = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   \
        if ((threadIdx.x & 63) == 0 && w_ < kPhaseWaves) g_phase[w_][k] = wall_clock64();      \
    } while (0)
// where the wave runs: HW_ID (wave, SIMD, CU, shader array, engine fields) in slot 15, XCC_ID in slot 14
#define PHASE_HWID()                                                                                    \
    do {                                                                                                \
        const long long w_ = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);            \
        if ((threadIdx.x & 63) == 0 && w_ < kPhaseWaves) {                                              \
            g_phase[w_][15] = (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);                      \
            g_phase[w_][14] = (unsigned)__builtin_amdgcn_s_getreg((15 << 11) | 20);                     \
        }                                                                                               \
    } while (0)
// wait for every outstanding memory operation of the wave, then stamp
#define PHASE_DRAIN(k)                   \
    do {                                 \
        __builtin_amdgcn_s_waitcnt(0);   \
        PHASE(k);                        \
    } while (0)
static __device__ unsigned long long g_chunk[4096][2][64];
#else
#define PHASE(k) \
    do {         \
    } while (0)
#define PHASE_HWID() \
    do {             \
    } while (0)
#define PHASE_DRAIN(k) \
    do {               \
    } while (0)
#endif

// shader-clock stamp at the start of forward (d = 0) / backward (d = 1) chunk c (c < 64); only with
// -DHMMBW_CHUNK_TIMES too: its conditional stores inside the sweeps change their s_waitcnt placement
#if defined(HMMBW_PHASE_TIMES) && defined(HMMBW_CHUNK_TIMES)
#define CHUNKSTAMP(d, c)                                                                       \
    do {                                                                                       \
        const long long w_ = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);   \
        if ((threadIdx.x & 63) == 0 && w_ < 4096 && (c) < 64) g_chunk[w_][d][c] = clock64();   \
    } while (0)
#else
#define CHUNKSTAMP(d, c) \
    do {                 \
    } while (0)
#endif

}  // namespace hmmbw
