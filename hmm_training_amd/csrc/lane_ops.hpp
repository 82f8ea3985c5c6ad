// lane_ops.hpp — cross-lane and small per-lane helpers of the kernels: DPP / permlane moves and the group and
// wave reductions built on them, the fused broadcast products of the dense recursions, the symbol / exponent
// pack accessors, LDS byte addresses, and the workgroup reduction.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

namespace hmmbw {

// ---------------------------------------------------------------------------------------------
// Cross-lane helpers (DPP on gfx950; 64-bit operands are split or use v_mov_b64_dpp)
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
    long long x = __builtin_bit_cast(long long, v);
    x = __builtin_amdgcn_update_dpp(0ll, x, CTRL, 0xF, 0xF, true);
    return __builtin_bit_cast(double, x);
}

template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) {
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true);
}

// lane ^ 16 / lane ^ 32 partners of a double without LDS: v_permlane16_swap / v_permlane32_swap (VALU) on
// both halves.  Each returns (own, partner) in an order that depends on the row, so combine the pair with a
// commutative operation only (every lane of the pair then gets the bitwise-identical result).
template <bool P32>
__device__ __forceinline__ void swap_pair(double v, double &a, double &b) {
    const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
    const auto l = P32 ? __builtin_amdgcn_permlane32_swap(lo, lo, false, false)
                       : __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto h = P32 ? __builtin_amdgcn_permlane32_swap(hi, hi, false, false)
                       : __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    a = __hiloint2double((int)h[0], (int)l[0]);
    b = __hiloint2double((int)h[1], (int)l[1]);
}
template <bool P32>
__device__ __forceinline__ double add_swap(double v) {
    double a, b;
    swap_pair<P32>(v, a, b);
    return a + b;
}
template <bool P32>
__device__ __forceinline__ double max_swap(double v) {
    double a, b;
    swap_pair<P32>(v, a, b);
    return fmax(a, b);
}

// Sum over a group of G lanes (butterfly; every lane gets the bitwise-identical result because
// each level adds the same two partial sums, only commuted).  No LDS round trip: DPP within a row,
// permlane swaps across rows (round 6: the ds_bpermute of __shfl_xor cost ~120 cycles per level).
template <int G>
__device__ __forceinline__ double gsum(double x) {
    if constexpr (G >= 2) x += dpp<0xB1>(x);   // quad_perm [1,0,3,2]
    if constexpr (G >= 4) x += dpp<0x4E>(x);   // quad_perm [2,3,0,1]
    if constexpr (G >= 8) x += dpp<0x141>(x);  // row_half_mirror
    if constexpr (G >= 16) x += dpp<0x140>(x); // row_mirror
    if constexpr (G >= 32) x = add_swap<false>(x);
    if constexpr (G >= 64) x = add_swap<true>(x);
    return x;
}

// max over the wave, complete in every lane
__device__ __forceinline__ double wave_max(double x) {
    x = fmax(x, dpp<0xB1>(x));
    x = fmax(x, dpp<0x4E>(x));
    x = fmax(x, dpp<0x141>(x));
    x = fmax(x, dpp<0x140>(x));
    x = max_swap<false>(x);
    return max_swap<true>(x);
}

// Sum over the lanes of a wave that share (lane mod G), e.g. the U sequences of a G-lane-group layout: the
// result is complete in every lane (the order of the additions may differ between lanes).
template <int G>
__device__ __forceinline__ double usum(double x) {
    if constexpr (G <= 2) x += __shfl_xor(x, 2);
    if constexpr (G <= 4) x += dpp<0x124>(x);   // row_ror:4
    if constexpr (G <= 8) x += dpp<0x128>(x);   // row_ror:8
    if constexpr (G <= 16) x = add_swap<false>(x);
    return add_swap<true>(x);
}

// min over the lanes of a wave that share (lane mod G), ints (DPP in the row, permlane swaps across rows)
template <int G>
__device__ __forceinline__ int umin_i32(int x) {
    if constexpr (G <= 2) x = min(x, __shfl_xor(x, 2));
    if constexpr (G <= 4) x = min(x, dpp_i32<0x124>(x));  // row_ror:4
    if constexpr (G <= 8) x = min(x, dpp_i32<0x128>(x));  // row_ror:8
    if constexpr (G <= 16) {
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        x = min((int)r[0], (int)r[1]);
    }
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
    return min((int)r[0], (int)r[1]);
}

template <int G>
__device__ __forceinline__ int gmax_i32(int e) {
    if constexpr (G >= 2) e = max(e, dpp_i32<0xB1>(e));
    if constexpr (G >= 4) e = max(e, dpp_i32<0x4E>(e));
    if constexpr (G >= 8) e = max(e, dpp_i32<0x141>(e));
    if constexpr (G >= 16) e = max(e, dpp_i32<0x140>(e));
    if constexpr (G >= 32) {  // across rows: lane ^ 16, then lane ^ 32 (the posterior kernels' 32- and 64-lane groups)
        const auto r = __builtin_amdgcn_permlane16_swap((unsigned)e, (unsigned)e, false, false);
        e = max((int)r[0], (int)r[1]);
    }
    if constexpr (G >= 64) {
        const auto r = __builtin_amdgcn_permlane32_swap((unsigned)e, (unsigned)e, false, false);
        e = max((int)r[0], (int)r[1]);
    }
    return e;
}

// Exponent that steers the power-of-two scaling: frexp exponent of the group's largest entry
// (entries are >= 0), kZeroExp when the whole group is zero.
constexpr int kZeroExp = -8192;
template <int G>
__device__ __forceinline__ int group_exp(double z) {
    return gmax_i32<G>(z > 0.0 ? __builtin_amdgcn_frexp_exp(z) : kZeroExp);
}

// Value of lane I of this lane's G-group.
template <int G, int I>
__device__ __forceinline__ double gbcast(double v, int lane) {
    if constexpr (G == 2) {
        return dpp<(I) | ((I) << 2) | ((2 + I) << 4) | ((2 + I) << 6)>(v);
    } else if constexpr (G == 4) {
        return dpp<(I) * 0x55>(v);
    } else if constexpr (G == 8) {
        const double lo = dpp<0x150 + I>(v);
        const double hi = dpp<0x150 + 8 + I>(v);
        return (lane & 8) ? hi : lo;
    } else {
        static_assert(G == 16, "group size");
        return dpp<0x150 + I>(v);  // row_newbcast:I
    }
}

__device__ __forceinline__ double readlane_f64(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

// Value of lane I of this lane's GV-group for the groups of the decoder and the posterior kernels
// (viterbi_plan.hpp: 8, 16, 32 or 64 lanes): DPP up to 16 lanes, v_readlane for 32 and 64.
template <int GV, int I>
__device__ __forceinline__ double gbcast_wide(double v, int lane) {
    if constexpr (GV <= 16) {
        return gbcast<GV, I>(v, lane);
    } else if constexpr (GV == 32) {
        const double lo = readlane_f64(v, I), hi = readlane_f64(v, 32 + I);
        return (lane & 32) ? hi : lo;
    } else {
        return readlane_f64(v, I);
    }
}

template <int B, int E, class F>
__device__ __forceinline__ void sfor(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        sfor<B + 1, E>(f);
    }
}

// Dense-A cross-lane products with the broadcast fused into the multiply-add: gfx950's 64-bit DPP
// ("DP ALU DPP") has only row_newbcast, which broadcasts lane L of every 16-lane row, so for G-lane
// groups (G = 4, 8, 16) one v_fmac_f64_dpp per group position Q, with bank_mask restricting the write
// to that group's lanes, gives  acc += z(lane I of this lane's group) * a  in 16 / G instructions, in
// place of a broadcast, a select and an fma per group (the compiler does not fuse 64-bit DPP moves).
template <int G, int I, int Q>
__device__ __forceinline__ void fmac_bcast1(double &acc, double z, double a) {
    constexpr int lane = Q * G + I;
    constexpr int bm = ((1 << (G / 4)) - 1) << (Q * G / 4);
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:%4"
                 : "+v"(acc) : "v"(z), "v"(a), "i"(lane), "i"(bm));
}
// VALU write -> DPP read of that VGPR needs 2 wait states; the compiler does not see the DPP read
// inside the asm, so the first fused product after z is written goes behind this.
__device__ __forceinline__ void dpp_guard(double z) { asm volatile("s_nop 1" ::"v"(z)); }

// acc0 += sum over even i of a[i] z(lane i), acc1 the odd i (two chains), per G-lane group.  (Four
// chains, i mod 4, measured slower at dense cfg3: 76-77 against 71-73 us, profiles/r5/ab_dense_dot4.txt.)
template <int G, int N>
__device__ __forceinline__ void bcast_dot(double &acc0, double &acc1, double z, const double (&a)[N]) {
    dpp_guard(z);
    sfor<0, (N + 1) / 2>([&](auto P) {
        constexpr int i0 = 2 * decltype(P)::value, i1 = i0 + 1;
        sfor<0, 16 / G>([&](auto Q) {
            fmac_bcast1<G, i0, decltype(Q)::value>(acc0, z, a[i0]);
            if constexpr (i1 < N) fmac_bcast1<G, i1, decltype(Q)::value>(acc1, z, a[i1]);
        });
    });
}

// Dense xi partial sums of a G = 8 wave (lane = 8 u + j) on the 4x4x4 f64 MFMA: its block is lane
// bits 2-3, A lane 16k + 4blk + m holds A[m][k], B lane 16k + 4blk + n holds B[k][n], D lane
// 16m + 4blk + n holds D[m][n] (tools/ubench_mfma4.hip, profiles/r3/ubench_mfma4x4x4.txt).  With
// z as A and v as B, block (j >> 2, u & 1) sums over the seqs u >> 1:
//   X[0] lane 16m + 4jh + 8u0 + n:  sum z_t(4jh + m) v_{t+1}(4jh + n)            (diagonal 4x4 blocks)
//   X[1] with v row_half_mirrored (state j -> 7 - j):  ... v_{t+1}(4(1 - jh) + 3 - n)  (off-diagonal)
// The accumulation is off the forward/backward chains, so the MFMA's ~44-cycle SrcC latency is
// hidden; it replaces 16 v_fmac_f64_dpp per step (bcast_acc).
__device__ __forceinline__ void xi_mfma8(double (&X)[2], double zs, double vd) {
    X[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(zs, vd, X[0], 0, 0, 0);
    X[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(zs, dpp<0x141>(vd), X[1], 0, 0, 0);  // row_half_mirror
}

// S[i] += z(lane i) * w for every state i of the group
template <int G, int N, int NS>
__device__ __forceinline__ void bcast_acc(double (&S)[NS], double z, double w) {
    dpp_guard(z);
    sfor<0, 16 / G>([&](auto Q) {
        sfor<0, N>([&](auto I) { fmac_bcast1<G, decltype(I)::value, decltype(Q)::value>(S[decltype(I)::value], z, w); });
    });
}

// ---------------------------------------------------------------------------------------------
// Symbol / exponent packs (8 x 16 bits in a uint4), power-of-two scaling, LDS byte addresses
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int sym_of(const uint4 &p, int s) {
    const unsigned w = s < 2 ? p.x : (s < 4 ? p.y : (s < 6 ? p.z : p.w));
    return (s & 1) ? int(w >> 16) : int(w & 0xFFFFu);
}

__device__ __forceinline__ int exp_of(const uint4 &p, int s) {  // signed int16 lanes of a pack
    const unsigned w = s < 2 ? p.x : (s < 4 ? p.y : (s < 6 ? p.z : p.w));
    return (s & 1) ? int((int)w >> 16) : int((int)(w << 16) >> 16);
}

__device__ __forceinline__ uint4 pack_exps(const int *e) {
    uint4 p;
    p.x = (unsigned)(e[0] & 0xFFFF) | ((unsigned)e[1] << 16);
    p.y = (unsigned)(e[2] & 0xFFFF) | ((unsigned)e[3] << 16);
    p.z = (unsigned)(e[4] & 0xFFFF) | ((unsigned)e[5] << 16);
    p.w = (unsigned)(e[6] & 0xFFFF) | ((unsigned)e[7] << 16);
    return p;
}

__device__ __forceinline__ double pow2_scale(double x, int e) { return __builtin_amdgcn_ldexp(x, -e); }

// 32-bit LDS byte address of a pointer into shared memory, and back (kept in one VGPR instead of
// being re-derived from its parts)
typedef __attribute__((address_space(3))) char lds_char;
__device__ __forceinline__ unsigned lds_addr(const char *p) {
    return (unsigned)(size_t)(const lds_char *)p;
}
__device__ __forceinline__ char *lds_ptr(unsigned a) {
    return (char *)(lds_char *)(size_t)a;
}

// A pointer whose value is the same in every lane of the wave, said so to the compiler: it then lives in an
// SGPR pair, and base + (32-bit per-lane byte offset) becomes the saddr form of global_load / global_store
// (one VGPR of address, no 64-bit add).
template <class T>
__device__ __forceinline__ T *wave_uniform_ptr(T *p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    // (rebuilt as a pointer into global memory: from a bare integer the accesses would become flat ones)
    typedef __attribute__((address_space(1))) T global_T;
    return (T *)(global_T *)(((unsigned long long)hi << 32) | lo);
}
// The object of type T at base + off bytes (off unsigned, 32 or 64 bits wide: zero-extended, see wave_uniform_ptr)
template <class T, class O>
__device__ __forceinline__ T &at_byte(T *base, O off) {
    static_assert(std::is_unsigned<O>::value, "byte offsets are unsigned");
    using C = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return *reinterpret_cast<T *>(reinterpret_cast<C *>(base) + (size_t)off);
}

// s_waitcnt immediate (gfx9 encoding) that waits until at most n LDS / scalar-memory operations are outstanding
// and leaves vmcnt and expcnt alone
constexpr int lgkmcnt_imm(int n) { return 0xC07F | (n << 8); }

// ---------------------------------------------------------------------------------------------
// Block reductions
// ---------------------------------------------------------------------------------------------
__device__ double block_reduce(double x, double *sh, bool is_max) {
    const int tid = threadIdx.x;
    x = is_max ? wave_max(x) : gsum<64>(x);
    __syncthreads();
    if ((tid & 63) == 0) sh[tid >> 6] = x;
    __syncthreads();
    if (tid < 64) {
        const int nw = blockDim.x >> 6;
        double y = tid < nw ? sh[tid] : (is_max ? -INFINITY : 0.0);
        y = is_max ? wave_max(y) : gsum<64>(y);
        if (tid == 0) sh[0] = y;
    }
    __syncthreads();
    const double r = sh[0];
    __syncthreads();
    return r;
}

}  // namespace hmmbw
