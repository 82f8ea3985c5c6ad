// word_units.hpp — what the word-lane units share (internal): wordnet.hip, embedded.hip and align.hip give every
// sequence a group of lanes, one lane per word or transcript position, over a bank of word models; this is the
// plumbing around that.  Device side: the row load, the one-lane neighbour shifts and the EmbedTab fill, nothing
// else (the kernel bodies stay written out: DESIGN section 6, "What the word-lane units share", has the
// instruction counts of the attempts to share more).  Host side: the kernel picker over (group width, N), the slot
// arguments all five slot kernels name alike (viterbi.hip and posterior.hip use that helper too), the checks of the
// bank and of the transcripts with their messages, the staging of both, and the buffers wordnet.hip and align.hip
// keep in the context.  Header only: it adds no translation unit.
#pragma once

#include "host.hpp"
#include "embed_plan.hpp"
#include "lane_ops.hpp"

namespace hmmbw {

// ---------------------------------------------------------------------------------------------
// Device side
// ---------------------------------------------------------------------------------------------

// a lane's N values of one table row (NP doubles, 16-B aligned when NP >= 2)
template <int N>
__device__ __forceinline__ void load_row(const double *p, double (&r)[N]) {
    if constexpr (N == 1) {
        r[0] = p[0];
    } else {
        const double2 *p2 = reinterpret_cast<const double2 *>(p);
#pragma unroll
        for (int h = 0; h < (N + 1) / 2; ++h) {
            const double2 x = p2[h];
            r[2 * h] = x.x;
            if (2 * h + 1 < N) r[2 * h + 1] = x.y;
        }
    }
}

// the value of lane l - 1 / l + 1 of the group, edge at the group's edge (0 in the linear domain, -inf in the log one)
template <int GW>
__device__ __forceinline__ double from_left(double x, int l, double edge) {
    double nb;
    if constexpr (GW <= 16) nb = dpp<0x111>(x);  // row_shr:1
    else nb = __shfl_up(x, 1, GW);
    return l > 0 ? nb : edge;
}
template <int GW>
__device__ __forceinline__ double from_right(double x, int l, double edge) {
    double nb;
    if constexpr (GW <= 16) nb = dpp<0x101>(x);  // row_shl:1
    else nb = __shfl_down(x, 1, GW);
    return l < GW - 1 ? nb : edge;
}
// the value of lane l - 2 / l + 2 of the group (the source past an optional transcript position).  A 16-lane DPP
// row holds two groups of 8: the two lanes at the group's edge take the edge value, never the other group's.
// from_left2 takes the lane's own condition in place of l (take implies l >= 2: position l - 1 is optional), so that
// the edge and the flag cost one select.
template <int GW>
__device__ __forceinline__ double from_left2(double x, bool take, double edge) {
    double nb;
    if constexpr (GW <= 16) nb = dpp<0x112>(x);  // row_shr:2
    else nb = __shfl_up(x, 2, GW);
    return take ? nb : edge;
}
template <int GW>
__device__ __forceinline__ double from_right2(double x, int l, double edge) {
    double nb;
    if constexpr (GW <= 16) nb = dpp<0x102>(x);  // row_shl:2
    else nb = __shfl_down(x, 2, GW);
    return l < GW - 2 ? nb : edge;
}

// element e of the EmbedTab tables (embed_plan.hpp, NP = embed_np(N)) from the staged linear bank pi [W][N] |
// A [W][N][N] | B [W][N][K]; 0 in the padding.  The callers form the three pointers and NP before their loops: taking
// the block's start and forming them here costs each of the two kernels a scalar register (profiles/word_units).
__device__ __forceinline__ double embed_bank_value(const double *pi, const double *A, const double *B, int W, int N,
                                                   int NP, int K, const EmbedTab &o, long long e) {
    double v = 0.0;
    if (e < o.A) {
        const int w = (int)(e / NP), j = (int)(e % NP);
        if (j < N) v = pi[w * N + j];
    } else if (e < o.B) {
        if (e - o.A < (long long)W * N * N) v = A[e - o.A];
    } else {
        const long long x = e - o.B;
        const long long k = x / ((long long)W * NP);
        const int w = (int)(x / NP % W), j = (int)(x % NP);
        if (j < N) v = B[((long long)w * N + j) * K + k];
    }
    return v;
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------

// f(integral_constant GW, integral_constant N) for the group width (8, 16, 32, else 64) and the states (1 .. 7,
// else 8) of a launch: a unit's f returns its kernel of that shape for the flags it captured
template <class F>
auto pick_gw_n(int GW, int N, F f) {
    auto states = [&](auto gw) {
        switch (N) {
            case 1: return f(gw, std::integral_constant<int, 1>{});
            case 2: return f(gw, std::integral_constant<int, 2>{});
            case 3: return f(gw, std::integral_constant<int, 3>{});
            case 4: return f(gw, std::integral_constant<int, 4>{});
            case 5: return f(gw, std::integral_constant<int, 5>{});
            case 6: return f(gw, std::integral_constant<int, 6>{});
            case 7: return f(gw, std::integral_constant<int, 7>{});
            default: return f(gw, std::integral_constant<int, 8>{});
        }
    };
    switch (GW) {
        case 8: return states(std::integral_constant<int, 8>{});
        case 16: return states(std::integral_constant<int, 16>{});
        case 32: return states(std::integral_constant<int, 32>{});
        default: return states(std::integral_constant<int, 64>{});
    }
}

// the fields the slot kernels' argument structs (VArgs, PArgs, WArgs, EmArgs, AlArgs) name alike
template <class Args>
void fill_slot_args(const hmmbw_ctx *c, Args &a) {
    a.sym = c->d_sym;  // never d_sym2: the row tables' packs (or symbol ids)
    a.wave_symoff = c->d_wsym;
    a.slot_len = c->d_slen;
    a.slot_seq = c->d_sseq;
    a.nslots = (long long)c->h_slen.size();  // layout slots, padding included (ViterbiPlan::nslots)
    a.U = c->U;
    a.K = c->K;
    const long long div = viterbi_pack_div(c->lds_tables(), c->G, 0);  // rows of G entries, no pad column
    a.div = (int)div;
    a.shift = viterbi_pack_shift(div);
}

inline long long loaded_symbols(const hmmbw_ctx *c) {
    long long total = 0;
    for (int T : c->h_slen) total += T;
    return total;
}

// *total gets the number of loaded symbols, which a path's length has to be
inline int check_path_len(const hmmbw_ctx *c, long long path_len, long long *total) {
    *total = loaded_symbols(c);
    if (path_len != *total)
        return fail(HMMBW_E_INVALID, "path_len " + std::to_string(path_len) + " is not the number of loaded symbols (" +
                                         std::to_string(*total) + ")");
    return HMMBW_OK;
}

// a bank of n_words models of the context's shape within a unit's limits, its parameters finite and non-negative;
// bad_value: the unit's message for one that is not
inline int check_word_bank(const hmmbw_ctx *c, int n_words, const double *pi, const double *A, const double *B,
                           int max_words, int max_states, const char *bad_value) {
    if (n_words < 1) return fail(HMMBW_E_INVALID, "n_words " + std::to_string(n_words) + " < 1");
    if (n_words > max_words)
        return fail(HMMBW_E_UNSUPPORTED, "n_words " + std::to_string(n_words) + " > " + std::to_string(max_words));
    if (c->N > max_states)
        return fail(HMMBW_E_UNSUPPORTED, "word models of N " + std::to_string(c->N) + " > " + std::to_string(max_states) + " states");
    const long long W = n_words, N = c->N, K = c->K;
    if (!wordnet_weights_ok(pi, W * N) || !wordnet_weights_ok(A, W * N * N) || !wordnet_weights_ok(B, W * N * K))
        return fail(HMMBW_E_INVALID, bad_value);
    return HMMBW_OK;
}

// one transcript per loaded sequence
inline int check_n_seq(const hmmbw_ctx *c, int64_t n_seq) {
    if (n_seq != c->R)
        return fail(HMMBW_E_INVALID, "n_seq " + std::to_string(n_seq) + " is not the number of loaded sequences (" +
                                         std::to_string(c->R) + ")");
    return HMMBW_OK;
}

// embed_transcripts_check's verdict as its message, and the longest transcript within max_words (*longest; count
// as embed_transcripts_check takes it)
inline int check_transcripts(const int64_t *off, const int32_t *ids, int64_t n_seq, int W, int max_words,
                             long long *longest, long long *count) {
    switch (embed_transcripts_check(off, ids, n_seq, W, longest, count)) {
        case 0: break;
        case 1: return fail(HMMBW_E_INVALID, "an empty transcript");
        case 2: return fail(HMMBW_E_INVALID, "a word id outside [0, " + std::to_string(W) + ")");
        default: return fail(HMMBW_E_INVALID, "word_offsets do not start at 0 or decrease");
    }
    if (*longest > max_words)
        return fail(HMMBW_E_UNSUPPORTED, "a transcript of " + std::to_string(*longest) + " words > " + std::to_string(max_words));
    return HMMBW_OK;
}

// embed_optional_check's verdict as its message (opt may be nullptr: nothing to check but the count)
inline int check_optional(const int64_t *off, const int32_t *ids, const uint8_t *opt, int64_t n_seq, int W,
                          long long *mand) {
    switch (embed_optional_check(off, ids, opt, n_seq, W, mand)) {
        case 0: return HMMBW_OK;
        case 1: return fail(HMMBW_E_INVALID, "an optional flag other than 0 or 1");
        case 2: return fail(HMMBW_E_INVALID, "two adjacent optional transcript positions");
        default: return fail(HMMBW_E_INVALID, "a transcript without a mandatory position");
    }
}

template <class T>
int upload(T *d, const std::vector<T> &h) {
    if (!h.empty()) HIP_TRY(hipMemcpy(d, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return HMMBW_OK;
}

// the bank, staged in h as one block of n_in doubles and copied up: pi | A | B, and where n_in has room for them
// (wordnet_in_len) the word loop's init | G, ones where the caller gave none
inline int stage_bank(double *dst, std::vector<double> &h, long long n_in, const double *pi, const double *A,
                      const double *B, long long W, long long N, long long K, const double *init = nullptr,
                      const double *G = nullptr) {
    h.assign((size_t)n_in, 1.0);
    double *hp = std::copy(pi, pi + W * N, h.data());
    hp = std::copy(A, A + W * N * N, hp);
    hp = std::copy(B, B + W * N * K, hp);
    if (init) std::copy(init, init + W, hp);
    if (G) std::copy(G, G + W * W, hp + W);
    return upload(dst, h);
}

// the transcripts (CSR, n_pos positions) as the kernels' types
inline int upload_transcripts(long long *d_off, int *d_ids, const int64_t *off, const int32_t *ids, int64_t n_seq,
                              long long n_pos) {
    if (int rc = upload(d_off, std::vector<long long>(off, off + n_seq + 1))) return rc;
    return upload(d_ids, std::vector<int>(ids, ids + n_pos));
}

// a buffer of at least n elements: kept while it is large enough
template <class T>
int grow(hmmbw_ctx *c, T *&p, size_t &have, size_t n) {
    if (p && have >= n) return HMMBW_OK;
    sync_ctx(c);
    dfree(p);
    have = 0;
    if (int rc = dalloc(&p, n)) return rc;
    have = n;
    return HMMBW_OK;
}

// what wordnet.hip and align.hip keep alike (n: hmmbw_ctx::Wordnet or ::Align) for the loaded observations and this
// bank shape: slot_out and the device logp of the decoder's plan, the back-pointer row offsets of the group width
// (a new width drops the unit's back-pointers, which the caller allocates with its other path buffers), and the
// staging and table buffers
template <class Unit>
int word_decode_buffers(hmmbw_ctx *c, Unit &n, int GW, size_t n_in, size_t n_tab) {
    if (int rc = viterbi_plan_ready(c)) return rc;
    if (n.GW != GW) {
        sync_ctx(c);
        dfree(n.d_psi_off);
        dfree(n.d_bp);
        n.GW = 0;
        const ViterbiPlan P = plan_viterbi_group(c->h_slen, c->h_sseq, c->R, GW);
        if (int rc = dalloc(&n.d_psi_off, P.psi_off.size())) return rc;
        if (int rc = upload(n.d_psi_off, P.psi_off)) return rc;
        n.rows = P.psi_rows;
        n.nvw = P.nvw;
        n.GW = GW;
    }
    if (int rc = grow(c, n.d_in, n.n_in, n_in)) return rc;
    return grow(c, n.d_tab, n.n_tab, n_tab);
}

}  // namespace hmmbw
