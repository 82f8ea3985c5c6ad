// alloc.hip — the block cache of small device buffers and pinned blocks, and the allocation ledger
// (interface in host.hpp).
#include <map>
#include <mutex>
#include <tuple>

#include "host.hpp"

namespace hmmbw {

// Block cache of the small device buffers and the pinned snapshot blocks.  The drop-in API builds and
// destroys one context per hmm_training call (HMM/hmm_training.py:265-267), and hipFree /
// hipHostFree synchronise the device and return memory to the driver: a word-sized context (20
// utterances) spent about 1 ms in hmmbw_ctx_destroy, as long as its 30 EM iterations.  Blocks up to
// kCacheMaxBlock bytes are rounded up to a power of two and kept per (device, kind, size) for the next
// context, up to kCacheMaxBytes per kind and device (a word-sized context holds well under 1 MB);
// larger buffers go straight to the driver.  hmmbw_cache_trim returns every cached block.
// Reused blocks are not cleared: every buffer is initialised by its owner, as after hipMalloc.
constexpr size_t kCacheMaxBlock = size_t(4) << 20;
constexpr size_t kCacheMaxBytes = size_t(32) << 20;
struct BlockCache {
    std::mutex mu;
    std::map<std::tuple<int, int, size_t>, std::vector<void *>> free;  // (device, kind, bytes) -> blocks
    std::map<void *, std::pair<int, size_t>> size_of;                   // cached-class block -> (kind, bytes)
    std::map<std::pair<int, int>, size_t> held;                          // (device, kind) -> bytes cached
};
BlockCache &block_cache() {
    static BlockCache *bc = new BlockCache;  // never destroyed: blocks may be released at process exit
    return *bc;
}
size_t cache_class(size_t bytes) {
    size_t c = 256;
    while (c < bytes) c <<= 1;
    return c;
}

// Allocation ledger (HMMBW_DEBUG_ALLOC=1, diagnostics): every driver allocation the library holds, with the
// blocks the cache has handed out; a new allocation that overlaps a held one, a block handed out twice and a
// free of an unknown block are reported on stderr.
struct Ledger {
    std::mutex mu;
    std::map<uintptr_t, std::pair<size_t, std::string>> held;  // start -> (bytes, what)
    std::map<uintptr_t, int> out;                              // cached blocks handed out
};
bool ledger_on() {
    static const bool on = std::getenv("HMMBW_DEBUG_ALLOC") && std::atoi(std::getenv("HMMBW_DEBUG_ALLOC")) != 0;
    return on;
}
Ledger &ledger() {
    static Ledger *l = new Ledger;
    return *l;
}
void ledger_add(const void *p, size_t bytes, const char *what) {
    if (!ledger_on() || !p) return;
    Ledger &L = ledger();
    std::lock_guard<std::mutex> lk(L.mu);
    const uintptr_t a = (uintptr_t)p;
    auto it = L.held.upper_bound(a);
    if (it != L.held.end() && it->first < a + bytes)
        fprintf(stderr, "HMMBW_DEBUG_ALLOC: %s [%#lx, +%zu) overlaps held %s [%#lx, +%zu)\n", what, (unsigned long)a, bytes,
                it->second.second.c_str(), (unsigned long)it->first, it->second.first);
    if (it != L.held.begin()) {
        auto jt = std::prev(it);
        if (jt->first + jt->second.first > a)
            fprintf(stderr, "HMMBW_DEBUG_ALLOC: %s [%#lx, +%zu) overlaps held %s [%#lx, +%zu)\n", what, (unsigned long)a,
                    bytes, jt->second.second.c_str(), (unsigned long)jt->first, jt->second.first);
    }
    L.held[a] = std::make_pair(bytes, std::string(what));
}
void ledger_remove(const void *p, const char *what) {
    if (!ledger_on() || !p) return;
    Ledger &L = ledger();
    std::lock_guard<std::mutex> lk(L.mu);
    if (!L.held.erase((uintptr_t)p)) fprintf(stderr, "HMMBW_DEBUG_ALLOC: %s of unknown %p\n", what, p);
}
void ledger_out(const void *p, bool take) {
    if (!ledger_on() || !p) return;
    Ledger &L = ledger();
    std::lock_guard<std::mutex> lk(L.mu);
    int &n = L.out[(uintptr_t)p];
    n += take ? 1 : -1;
    if (n > 1) fprintf(stderr, "HMMBW_DEBUG_ALLOC: cached block %p handed out twice\n", p);
    if (n < 0) fprintf(stderr, "HMMBW_DEBUG_ALLOC: cached block %p freed twice\n", p);
}

hipError_t cached_alloc(void **p, size_t bytes, int kind) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (bytes > kCacheMaxBlock) {
        const hipError_t e = kind == kDevBlock ? hipMalloc(p, bytes)
                                               : hipHostMalloc(p, bytes, hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess && kind == kDevBlock) ledger_add(*p, bytes, "hipMalloc (large)");
        return e;
    }
    const size_t cls = cache_class(bytes);
    BlockCache &bc = block_cache();
    {
        std::lock_guard<std::mutex> lk(bc.mu);
        auto it = bc.free.find(std::make_tuple(dev, kind, cls));
        if (it != bc.free.end() && !it->second.empty()) {
            *p = it->second.back();
            it->second.pop_back();
            bc.held[std::make_pair(dev, kind)] -= cls;
            if (kind == kDevBlock) ledger_out(*p, true);
            return hipSuccess;
        }
    }
    const hipError_t e = kind == kDevBlock ? hipMalloc(p, cls)
                                           : hipHostMalloc(p, cls, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lk(bc.mu);
        bc.size_of[*p] = std::make_pair(kind, cls);
    }
    if (e == hipSuccess && kind == kDevBlock) {
        ledger_add(*p, cls, "hipMalloc (cached class)");
        ledger_out(*p, true);
    }
    return e;
}
void cached_free(void *p, int kind) {
    if (!p) return;
    int dev = 0;
    (void)hipGetDevice(&dev);
    BlockCache &bc = block_cache();
    if (kind == kDevBlock && bc.size_of.count(p)) ledger_out(p, false);
    {
        std::lock_guard<std::mutex> lk(bc.mu);
        auto it = bc.size_of.find(p);
        if (it != bc.size_of.end()) {
            const size_t cls = it->second.second;
            size_t &held = bc.held[std::make_pair(dev, kind)];
            if (held + cls <= kCacheMaxBytes) {
                bc.free[std::make_tuple(dev, kind, cls)].push_back(p);
                held += cls;
                return;
            }
            bc.size_of.erase(it);
        }
    }
    if (kind == kDevBlock) {
        ledger_remove(p, "hipFree");
        (void)hipFree(p);
    } else {
        (void)hipHostFree(p);
    }
}
// Release every cached block (all devices); returns the bytes given back to the driver.
size_t cache_trim() {
    BlockCache &bc = block_cache();
    std::vector<std::tuple<int, int, void *>> out;
    size_t bytes = 0;
    {
        std::lock_guard<std::mutex> lk(bc.mu);
        for (auto &kv : bc.free) {
            for (void *p : kv.second) {
                out.emplace_back(std::get<0>(kv.first), std::get<1>(kv.first), p);
                bytes += std::get<2>(kv.first);
                bc.size_of.erase(p);
            }
        }
        bc.free.clear();
        bc.held.clear();
    }
    int dev0 = 0;
    (void)hipGetDevice(&dev0);
    for (auto &t : out) {
        (void)hipSetDevice(std::get<0>(t));
        if (std::get<1>(t) == kDevBlock) {
            ledger_remove(std::get<2>(t), "hipFree (trim)");
            (void)hipFree(std::get<2>(t));
        } else {
            (void)hipHostFree(std::get<2>(t));
        }
    }
    (void)hipSetDevice(dev0);
    return bytes;
}

}  // namespace hmmbw

extern "C" int hmmbw_cache_trim(int64_t *bytes_released) {
    const size_t b = cache_trim();
    if (bytes_released) *bytes_released = (int64_t)b;
    return HMMBW_OK;
}
