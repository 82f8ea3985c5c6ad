// peer.hip — the peer all-reduce: its kernels, the receive regions (pool, validation, in-process links),
// the three exchange calls and the hmmbw_peer_* ABI.  The only unit that names hmmbw_ctx::peer's fields.
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "host.hpp"

namespace hmmbw {

// ---------------------------------------------------------------------------------------------
// Peer all-reduce (HMMBW_OPT_ALLREDUCE = 1; include/hmmbw.h).  The reference's sums over all recordings
// (hmm_training.py:415-424 pi over the global R, :429-500 A and B, :503 L) become ONE elementwise sum of
// the ranks' statistics buffers per EM iteration.  Every rank owns a receive region in its HBM:
//   [2 iteration parities][world slots][slot doubles], then flags [world][chunks] (uint64 sequence numbers)
// The buffer is cut into chunks of kPeerThreads x dpt doubles (dpt chosen so a payload has <= 32 chunks).
//   push   workgroup (chunk c, peer p) writes chunk c of this rank's buffer into slot `rank` of p's region
//          with system-scope write-through stores, waits for them (vmcnt(0) in every wave, then the
//          barrier) and release-stores the iteration's sequence number into p's flag (rank, c);
//   reduce workgroup c's first wave polls its region's W flags of chunk c (system-scope loads + s_sleep,
//          bounded by wall-clock ticks: on expiry the iteration state records HMMBW_E_TIMEOUT and stops
//          EM), then the workgroup sums the W slots in rank order into the buffer, so every rank holds
//          bitwise-identical sums.
// k_peer_allreduce does both in ONE launch (hmmbw_iterate's loop: one kernel boundary, as RCCL's);
// the split ABI runs them as k_peer_push (in _begin) and k_peer_reduce (in _end), so several ranks that
// share one stream (the in-process tests) never wait on a push queued behind them.
// Parity double-buffering is enough: a rank can push iteration e + 2 into p's slot only after its own
// reduce of e + 1, which needs p's push of e + 1, which p enqueues after its reduce of e.
// ---------------------------------------------------------------------------------------------
constexpr int kMaxPeers = 16;
constexpr int kPeerThreads = 256;
constexpr int kPeerMaxChunks = 32;

struct PeerArgs {
    double *region[kMaxPeers];  // every rank's receive region, as addressable from this device
    long long n;                // payload doubles
    long long slot;             // slot stride (n rounded up to 256 B)
    long long nch;              // chunks
    int dpt;                    // doubles per thread per chunk (chunk = kPeerThreads x dpt)
    int world, rank;
    double perturb;             // diagnostics (HMMBW_DIAG_PEER_PERTURB): element 0 of this rank's push x (1 + perturb)
};

__device__ __forceinline__ unsigned long long *peer_flags(double *region, const PeerArgs &P) {
    return reinterpret_cast<unsigned long long *>(region + 2LL * P.world * P.slot);
}

__device__ __forceinline__ void peer_push_chunk(const double *src, const PeerArgs &P, unsigned long long seq,
                                                long long c, int p) {
    const long long base = c * kPeerThreads * P.dpt + threadIdx.x;
    double *dst = P.region[p] + ((long long)(seq & 1) * P.world + P.rank) * P.slot;
    for (int k = 0; k < P.dpt; ++k) {
        const long long i = base + (long long)k * kPeerThreads;
        if (i < P.n) __hip_atomic_store(dst + i, i == 0 ? src[i] * (1.0 + P.perturb) : src[i], __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_SYSTEM);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's write-through stores are acknowledged
    __syncthreads();
    // The flag is a write-through store too, issued after every payload store of the workgroup was
    // acknowledged: that orders it after them.  A release would add an L2 write-back at system scope
    // (every dirty line of this XCD, e.g. the E-step's checkpoints), which the payload does not need.
    if (threadIdx.x == 0)
        __hip_atomic_store(peer_flags(P.region[p], P) + (long long)P.rank * P.nch + c, seq, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// returns false (and stops EM with HMMBW_E_TIMEOUT) when a flag did not arrive in time
__device__ __forceinline__ bool peer_reduce_chunk(double *dst, const PeerArgs &P, unsigned long long seq,
                                                  IterState *state, long long timeout_ticks, long long c) {
    __shared__ int ok;
    const int tid = threadIdx.x;
    double *reg = P.region[P.rank];
    if (tid < 64) {  // one wave polls: lane q watches rank q's flag of this chunk
        const unsigned long long *fl = peer_flags(reg, P) + c;
        bool got = tid >= P.world;
        const unsigned long long t0 = wall_clock64();
        while (true) {
            if (!got) got = __hip_atomic_load(fl + (long long)tid * P.nch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) >= seq;
            if (__all(got)) break;
            if ((long long)(wall_clock64() - t0) > timeout_ticks) break;
            __builtin_amdgcn_s_sleep(2);
        }
        const int all = __all(got);
        if (tid == 0) ok = all;
    }
    __syncthreads();
    if (!ok) {
        if (tid == 0) {
            state->error = HMMBW_E_TIMEOUT;
            state->error_src = kErrPeer;
            state->done = 1;
        }
        return false;
    }
    // no acquire fence (it would invalidate this XCD's L2): the slot loads below are system-scope loads,
    // which bypass the caches and are issued after the flags were seen
    const double *slots = reg + (long long)(seq & 1) * P.world * P.slot;
    const long long base = c * kPeerThreads * P.dpt + tid;
    for (int k = 0; k < P.dpt; ++k) {
        const long long i = base + (long long)k * kPeerThreads;
        if (i < P.n) {
            double v = 0.0;
            for (int q = 0; q < P.world; ++q)
                v += __hip_atomic_load(slots + q * P.slot + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            dst[i] = v;
        }
    }
    return true;
}

__global__ void __launch_bounds__(kPeerThreads) k_peer_push(const double *src, PeerArgs P, unsigned long long seq,
                                                            const IterState *state) {
    if (state->done) return;  // identical on every rank: no rank pushes, none waits
    peer_push_chunk(src, P, seq, blockIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(kPeerThreads) k_peer_reduce(double *dst, PeerArgs P, unsigned long long seq,
                                                              IterState *state, long long timeout_ticks) {
    if (state->done) return;
    (void)peer_reduce_chunk(dst, P, seq, state, timeout_ticks, blockIdx.x);
}

// push + wait + sum in one launch: workgroup (c, p) pushes chunk c to rank p; the one whose p is this
// rank (its own slot, the nearest memory) then waits for chunk c's W flags and sums them into `sum` (not
// into buf, which the other workgroups of this launch may still be pushing).  At most 32 x 16 workgroups
// of 256 threads, all resident at once, so a waiting workgroup never holds a slot a pushing one needs
// (and every wait is bounded anyway).
__global__ void __launch_bounds__(kPeerThreads) k_peer_allreduce(const double *buf, double *sum, PeerArgs P,
                                                                 unsigned long long seq, IterState *state,
                                                                 long long timeout_ticks) {
    if (state->done) return;
    peer_push_chunk(buf, P, seq, blockIdx.x, blockIdx.y);
    if ((int)blockIdx.y != P.rank) return;
    (void)peer_reduce_chunk(sum, P, seq, state, timeout_ticks, blockIdx.x);
}

// Validation of a new uncached / fine-grained peer region (peer_region_alloc): the pattern is written with the
// push's system-scope stores, then read back with the reduce's system-scope loads and with ordinary loads;
// every mismatch is counted.  Recycled pages can return stale data to kernel loads after a change of memory
// type (see peer_region_alloc), which this catches before the region carries any statistics.
__device__ __forceinline__ double region_pattern(long long i, unsigned seed) {
    return (double)(((unsigned long long)i * 2654435761ull + seed) & 0xFFFFFFull) + 0.5;
}
__global__ void k_region_fill(double *r, long long n, unsigned seed) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        __hip_atomic_store(r + i, region_pattern(i, seed), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__global__ void k_region_check(const double *r, long long n, unsigned seed, unsigned *bad) {
    unsigned nb = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double want = region_pattern(i, seed);
        nb += __hip_atomic_load(r + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != want;
        nb += r[i] != want;
    }
    if (nb) atomicAdd(bad, nb);
}

// ---------------------------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------------------------

// In-process attachments (hmmbw_peer_attach): region -> the contexts whose peer.regions hold it.  A context
// that frees its region detaches every context still attached to it, so a later push of theirs fails with
// HMMBW_E_STATE instead of writing into memory the allocator may already have handed to another buffer.
struct PeerLinks {
    std::mutex mu;
    std::map<const void *, std::vector<hmmbw_ctx *>> users;
};
static PeerLinks &peer_links() {
    static PeerLinks *p = new PeerLinks;  // never destroyed
    return *p;
}

// drop the attached peer regions (closing the IPC mappings of other ranks' regions)
void peer_detach(hmmbw_ctx *c) {
    for (void *p : c->peer.mapped) (void)hipIpcCloseMemHandle(p);
    c->peer.mapped.clear();
    {
        PeerLinks &pl = peer_links();
        std::lock_guard<std::mutex> lk(pl.mu);
        for (double *r : c->peer.regions) {
            auto it = pl.users.find(r);
            if (it == pl.users.end()) continue;
            auto &v = it->second;
            v.erase(std::remove(v.begin(), v.end(), c), v.end());
            if (v.empty()) pl.users.erase(it);
        }
    }
    c->peer.regions.clear();
    c->peer.on = false;
}

std::string peer_off_msg(const hmmbw_ctx *c) {
    return c->peer.revoked ? "peer all-reduce: a rank's region this context was attached to has been freed "
                             "(its context was destroyed or re-sized its region); attach again"
                           : "peer all-reduce selected but no regions attached (hmmbw_peer_open / _attach)";
}

// this context's region is about to be freed: detach every other context attached to it (in-process)
static void peer_revoke(hmmbw_ctx *c) {
    if (!c->peer.region) return;
    PeerLinks &pl = peer_links();
    std::lock_guard<std::mutex> lk(pl.mu);
    auto it = pl.users.find(c->peer.region);
    if (it == pl.users.end()) return;
    for (hmmbw_ctx *u : it->second) {
        if (u == c) continue;
        for (double *r : u->peer.regions) {  // u's other links go too: its exchange is broken as a whole
            if (r == c->peer.region) continue;
            auto jt = pl.users.find(r);
            if (jt == pl.users.end()) continue;
            auto &w = jt->second;
            w.erase(std::remove(w.begin(), w.end(), u), w.end());
            if (w.empty()) pl.users.erase(jt);
        }
        u->peer.regions.clear();
        u->peer.on = false;
        u->peer.revoked = true;
    }
    pl.users.erase(it);
}

// Memory of the peer receive regions (HMMBW_PEER_MEM).  Other GPUs write payload and flags into a region
// over xGMI while this GPU's reduce kernel polls it.  coarse (default): hipMalloc, allocated and freed with
// its context; the writers' stores are system-scope write-through and the reader's loads system-scope.
// uncached / finegrained: the hipExtMallocWithFlags kinds RCCL keeps its flags in.
// The cause of round 5's failures (wrong statistics in later contexts of one process, once a
// MEMORY_APERTURE_VIOLATION), measured in round 6 (tools/uc_stale.py, profiles/r6/uc_stale.txt, tools/peer_diag.py,
// profiles/r6/peer_diag.txt): the driver hands a freed ordinary block's addresses to the next uncached /
// fine-grained allocation, and kernel loads from such a region (system-scope and ordinary alike) can then
// return stale or foreign data while hipMemcpy reads what was written; an L2 write-back + invalidate between
// the two lives does not clear it.  In the suite, the wide path's 2.2 MB region of rank 0 landed on the
// addresses of the previous test's freed coarse region: every push landed (checked by hipMemcpy), but the
// reduce kernel read zeros and 1e-20 (another context's B floor) for some entries, so the M-step's A and B
// were wrong; the reverse transition (a freed special region's pages back as an ordinary buffer that kernels
// read) fits the aperture violation, an address formed from offsets that came back as foreign data.
// Fp64 atomics themselves sum exactly on every kind (tools/uc_probe.py).  Hence: special regions come from a
// per-process pool and never go back to the driver (no special -> ordinary transition), and a new one is
// validated with the push's stores and the reduce's loads before use (catches the ordinary -> special one;
// a region that fails is quarantined, kept allocated and unused).  Separately, in-process attachments
// (hmmbw_peer_attach) are revoked when their region is freed (peer_revoke), so no context can push through a
// pointer to a freed region.  Cross-GPU coherence of either kind over xGMI is unmeasured here.
struct PeerPool {
    std::mutex mu;
    std::vector<std::tuple<int, unsigned, size_t, void *>> free;  // (device, flags, bytes, region)
    std::map<void *, std::tuple<int, unsigned, size_t>> owned;
    std::vector<void *> quarantined;
    long long validated = 0, rejected = 0;
};
static PeerPool &peer_pool() {
    static PeerPool *p = new PeerPool;  // never destroyed (its regions live for the process)
    return *p;
}

// 0: the region reads back what was written; > 0: mismatching reads; < 0: HIP error
static long long validate_region(void *p, size_t bytes) {
    const long long n = (long long)(bytes / sizeof(double));
    unsigned *d_bad = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&d_bad), sizeof(unsigned)) != hipSuccess) return -1;
    unsigned bad = 0;
    long long rc = 0;
    for (unsigned seed = 1; seed <= 2 && rc == 0; ++seed) {
        if (hipMemset(d_bad, 0, sizeof(unsigned)) != hipSuccess) { rc = -1; break; }
        hipLaunchKernelGGL(k_region_fill, dim3(256), dim3(256), 0, nullptr, static_cast<double *>(p), n, seed);
        if (hipDeviceSynchronize() != hipSuccess) { rc = -1; break; }
        hipLaunchKernelGGL(k_region_check, dim3(256), dim3(256), 0, nullptr, static_cast<const double *>(p), n, seed, d_bad);
        if (hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) { rc = -1; break; }
        rc = bad;
    }
    (void)hipFree(d_bad);
    return rc;
}

static int peer_region_alloc(hmmbw_ctx *c, size_t b) {
    c->peer.special = false;
    const char *pm = std::getenv("HMMBW_PEER_MEM");
    const std::string kind = pm ? pm : "coarse";
    if (kind == "coarse") {
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&c->peer.region), b));
        ledger_add(c->peer.region, b, "peer region (coarse)");
        return HMMBW_OK;
    }
    if (kind != "uncached" && kind != "finegrained")
        return fail(HMMBW_E_INVALID, "HMMBW_PEER_MEM must be coarse, uncached or finegrained");
    const unsigned fl = kind == "finegrained" ? hipDeviceMallocFinegrained : hipDeviceMallocUncached;
    c->peer.special = true;
    PeerPool &pp = peer_pool();
    std::lock_guard<std::mutex> lk(pp.mu);
    size_t best = SIZE_MAX;
    long long bi = -1;
    for (size_t i = 0; i < pp.free.size(); ++i) {  // smallest free region of this device and kind that fits
        const auto &f = pp.free[i];
        if (std::get<0>(f) == c->device && std::get<1>(f) == fl && std::get<2>(f) >= b && std::get<2>(f) < best) {
            best = std::get<2>(f);
            bi = (long long)i;
        }
    }
    if (bi >= 0) {
        c->peer.region = static_cast<double *>(std::get<3>(pp.free[(size_t)bi]));
        pp.free.erase(pp.free.begin() + bi);
        return HMMBW_OK;
    }
    // whole 2 MB units: in the probe only allocations past 2 MB that were not a multiple of it (2.25 MB, the
    // wide path's region at world 2) read back wrong after an ordinary -> special reuse (uc_stale.txt)
    const size_t nb = (b + (size_t(2) << 20) - 1) / (size_t(2) << 20) * (size_t(2) << 20);
    for (int attempt = 0; attempt < 8; ++attempt) {
        void *p = nullptr;
        HIP_TRY(hipExtMallocWithFlags(&p, nb, fl));
        ledger_add(p, nb, kind == "finegrained" ? "peer region (fine-grained)" : "peer region (uncached)");
        const long long bad = validate_region(p, nb);
        if (bad < 0) return fail(HMMBW_E_HIP, "validating a new peer region failed");
        if (bad == 0) {
            pp.validated += 1;
            pp.owned[p] = std::make_tuple(c->device, fl, nb);
            c->peer.region = static_cast<double *>(p);
            return HMMBW_OK;
        }
        pp.rejected += 1;
        pp.quarantined.push_back(p);  // stale pages: never used, never freed
    }
    return fail(HMMBW_E_HIP, "no " + kind + " peer region read back what was written (8 attempts quarantined): use "
                "HMMBW_PEER_MEM=coarse");
}

// callers synchronise the device first (no launch of this context still writes the region)
static void peer_region_free(hmmbw_ctx *c) {
    if (!c->peer.region) return;
    peer_revoke(c);
    if (c->peer.special) {  // back to the pool, never to the driver
        PeerPool &pp = peer_pool();
        std::lock_guard<std::mutex> lk(pp.mu);
        auto it = pp.owned.find(c->peer.region);
        if (it != pp.owned.end())
            pp.free.emplace_back(std::get<0>(it->second), std::get<1>(it->second), std::get<2>(it->second), c->peer.region);
        c->peer.region = nullptr;
        return;
    }
    ledger_remove(c->peer.region, "hipFree (peer region)");
    (void)hipFree(c->peer.region);
    c->peer.region = nullptr;
}

void peer_destroy(hmmbw_ctx *c) {
    peer_detach(c);
    peer_region_free(c);
    dfree(c->peer.d_xsum);
}

int peer_info(const hmmbw_ctx *c, int key, int64_t *value) {
    switch (key) {
        case HMMBW_INFO_PEER_CHUNKS: *value = c->peer.region ? c->peer.nch : 0; return HMMBW_OK;
        case HMMBW_INFO_PEER_SUM_PTR: *value = (int64_t)(intptr_t)c->peer.d_xsum; return HMMBW_OK;
        case HMMBW_INFO_PEER_REGIONS_VALIDATED:
        case HMMBW_INFO_PEER_REGIONS_REJECTED: {
            PeerPool &pp = peer_pool();
            std::lock_guard<std::mutex> lk(pp.mu);
            *value = key == HMMBW_INFO_PEER_REGIONS_VALIDATED ? pp.validated : pp.rejected;
            return HMMBW_OK;
        }
        default: return fail(HMMBW_E_INVALID, "unknown option " + std::to_string(key));
    }
}

// Peer all-reduce halves (kernels above): push this rank's buffer to every rank's slot `rank` after the
// E-step, and wait for / sum every rank's slot before the M-step.
static PeerArgs peer_args(const hmmbw_ctx *c) {
    PeerArgs P{};
    for (int r = 0; r < c->peer.world; ++r) P.region[r] = c->peer.regions[(size_t)r];
    P.n = c->peer.n;
    P.slot = c->peer.slot;
    P.nch = c->peer.nch;
    P.dpt = c->peer.dpt;
    P.world = c->peer.world;
    P.rank = c->rank;
    P.perturb = c->peer.perturb;
    return P;
}

// the regions were sized for this payload and world
static int check_payload(const hmmbw_ctx *c, long long len) {
    if (len != c->peer.n || c->peer.world != c->world)
        return fail(HMMBW_E_STATE, "the all-reduce payload changed after hmmbw_peer_region (rank, world or options "
                                   "set after it): set up the peer regions again");
    return HMMBW_OK;
}

int peer_push(hmmbw_ctx *c, const double *buf, long long len) {
    if (int rc = check_payload(c, len)) return rc;
    c->peer.seq += 1;
    hipLaunchKernelGGL(k_peer_push, dim3((unsigned)c->peer.nch, (unsigned)c->peer.world), dim3(kPeerThreads), 0,
                       c->stream, buf, peer_args(c), c->peer.seq, c->state());
    HIP_TRY(hipGetLastError());
    return HMMBW_OK;
}

// hmmbw_iterate's loop: push, wait and sum in one launch (k_peer_allreduce)
int peer_allreduce(hmmbw_ctx *c, double *buf, long long len) {
    if (int rc = check_payload(c, len)) return rc;
    c->peer.seq += 1;
    const long long ticks = ms_to_ticks(c, std::max(1LL, c->peer_timeout_ms));
    hipLaunchKernelGGL(k_peer_allreduce, dim3((unsigned)c->peer.nch, (unsigned)c->peer.world), dim3(kPeerThreads), 0,
                       c->stream, buf, c->peer.d_xsum, peer_args(c), c->peer.seq, c->state(), ticks);
    HIP_TRY(hipGetLastError());
    c->ar_cur = c->peer.d_xsum;  // the pending M-step reads the sums
    return HMMBW_OK;
}

// the sums go to d_xsum, which becomes the pending M-step's source (mr_end)
int peer_reduce(hmmbw_ctx *c) {
    const long long ticks = ms_to_ticks(c, std::max(1LL, c->peer_timeout_ms));
    hipLaunchKernelGGL(k_peer_reduce, dim3((unsigned)c->peer.nch), dim3(kPeerThreads), 0, c->stream, c->peer.d_xsum,
                       peer_args(c), c->peer.seq, c->state(), ticks);
    HIP_TRY(hipGetLastError());
    c->ar_cur = c->peer.d_xsum;
    return HMMBW_OK;
}

// what hmmbw_peer_attach and hmmbw_peer_open both ask for (src: the regions or the handles)
static int check_attach(const hmmbw_ctx *c, const void *src, int64_t n_seq_global) {
    if (!c || !src) return fail(HMMBW_E_INVALID, "null argument");
    if (n_seq_global < 0) return fail(HMMBW_E_INVALID, "negative sequence count");
    if (int rc = check_closed(c)) return rc;
    if (!c->peer.region || c->peer.world != c->world || c->peer.n != c->ar_payload())
        return fail(HMMBW_E_STATE, "no current peer region (hmmbw_peer_region first, after set_rank and options)");
    return HMMBW_OK;
}

}  // namespace hmmbw

extern "C" {

int hmmbw_peer_region(hmmbw_ctx *c, void **region, int64_t *bytes) {
    if (!c || !region || !bytes) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = check_closed(c)) return rc;
    if (c->world > kMaxPeers) return fail(HMMBW_E_UNSUPPORTED, "peer all-reduce: at most 16 ranks");
    if (int rc = set_device(c)) return rc;
    const long long n = c->ar_payload();
    const long long dpt = std::min(64LL, std::max(1LL, (n + (long long)kPeerThreads * kPeerMaxChunks - 1) /
                                                       ((long long)kPeerThreads * kPeerMaxChunks)));
    const long long slot = (n + 31) / 32 * 32, nch = (n + kPeerThreads * dpt - 1) / (kPeerThreads * dpt);
    const size_t b = sizeof(double) * 2 * (size_t)c->world * (size_t)slot +
                     sizeof(unsigned long long) * (size_t)c->world * (size_t)nch;
    if (!c->peer.region || c->peer.n != n || c->peer.world != c->world) {
        peer_detach(c);
        HIP_TRY(hipDeviceSynchronize());
        peer_region_free(c);
        // its own allocation (exported with hipIpcGetMemHandle), never a block of the cache
        if (int rc = peer_region_alloc(c, b)) return rc;
        HIP_TRY(hipMemset(c->peer.region, 0, b));
        dfree(c->peer.d_xsum);
        if (int rc = dalloc(&c->peer.d_xsum, (size_t)slot)) return rc;
        HIP_TRY(hipMemset(c->peer.d_xsum, 0, sizeof(double) * (size_t)slot));
        c->peer.bytes = b;
        c->peer.n = n;
        c->peer.slot = slot;
        c->peer.nch = nch;
        c->peer.dpt = (int)dpt;
        c->peer.world = c->world;
    }
    *region = c->peer.region;
    *bytes = (int64_t)c->peer.bytes;
    return HMMBW_OK;
}

int hmmbw_peer_ipc_handle(hmmbw_ctx *c, void *handle_out) {
    if (!c || !handle_out) return fail(HMMBW_E_INVALID, "null argument");
    if (!c->peer.region) return fail(HMMBW_E_STATE, "no peer region (hmmbw_peer_region first)");
    if (int rc = set_device(c)) return rc;
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, c->peer.region));
    static_assert(sizeof(h) == 64, "HIP IPC handles are 64 bytes");
    std::memcpy(handle_out, &h, sizeof(h));
    return HMMBW_OK;
}

static int peer_attach_impl(hmmbw_ctx *c, const std::vector<double *> &regions, int64_t n_seq_global) {
    HIP_TRY(hipDeviceSynchronize());
    // a fresh exchange: clear this rank's slots and flags (every rank attaches before any iterates)
    HIP_TRY(hipMemset(c->peer.region, 0, c->peer.bytes));
    c->peer.regions = regions;
    {
        PeerLinks &pl = peer_links();
        std::lock_guard<std::mutex> lk(pl.mu);
        for (double *r : regions) pl.users[r].push_back(c);
    }
    c->peer.seq = 0;
    c->peer.on = true;
    c->peer.revoked = false;
    // diagnostics: one rank pushes a wrong payload, so the exchange disagrees with any other all-reduce
    // (tests/test_bench.py drives bench.py's leg check with it)
    c->peer.perturb = 0.0;
    if (const char *pe = std::getenv("HMMBW_DIAG_PEER_PERTURB")) {
        const char *colon = std::strchr(pe, ':');
        if (colon && std::atoi(pe) == c->rank) c->peer.perturb = std::atof(colon + 1);
    }
    c->R_global = n_seq_global;  // the R of hmm_training.py:424 for hmmbw_iterate's loop
    return HMMBW_OK;
}

int hmmbw_peer_attach(hmmbw_ctx *c, void *const *regions, int64_t n_seq_global) {
    if (int rc = check_attach(c, regions, n_seq_global)) return rc;
    if (regions[c->rank] != c->peer.region) return fail(HMMBW_E_INVALID, "regions[rank] must be this context's own region");
    std::vector<double *> reg((size_t)c->world);
    for (int r = 0; r < c->world; ++r) {
        if (!regions[r]) return fail(HMMBW_E_INVALID, "null peer region");
        reg[(size_t)r] = static_cast<double *>(regions[r]);
    }
    if (int rc = set_device(c)) return rc;
    peer_detach(c);
    return peer_attach_impl(c, reg, n_seq_global);
}

int hmmbw_peer_open(hmmbw_ctx *c, const void *handles, int64_t n_seq_global) {
    if (int rc = check_attach(c, handles, n_seq_global)) return rc;
    if (int rc = set_device(c)) return rc;
    peer_detach(c);
    std::vector<double *> reg((size_t)c->world, nullptr);
    const char *hb = static_cast<const char *>(handles);
    for (int r = 0; r < c->world; ++r) {
        if (r == c->rank) {
            reg[(size_t)r] = c->peer.region;
            continue;
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, hb + 64 * (size_t)r, sizeof(h));
        void *p = nullptr;
        const hipError_t e = hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            peer_detach(c);
            return fail(HMMBW_E_HIP, "hipIpcOpenMemHandle (rank " + std::to_string(r) + "): " + hipGetErrorString(e));
        }
        c->peer.mapped.push_back(p);
        reg[(size_t)r] = static_cast<double *>(p);
    }
    return peer_attach_impl(c, reg, n_seq_global);
}

}  // extern "C"
