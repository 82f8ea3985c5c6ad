// group.hip — grouped launches and the hmmbw_group_* ABI.
#include "host.hpp"

// ---------------------------------------------------------------------------------------------
// Groups: several single-rank contexts of one shape advanced by ONE grouped launch per EM iteration
// (k_estep_small_group).  The reference trains its word models one after another (HMM/main.py:147-152
// -> training_with_save, hmm_training.py:215-247) and scores every (recording, model) pair with its
// own forward pass (hmm_testing.py:139-161); a group does each in one launch.
// ---------------------------------------------------------------------------------------------

struct hmmbw_group {
    std::vector<hmmbw_ctx *> m;
    // argument slabs ([n_launch][n] EArgs + [n_launch][n + 1] first-workgroup tables): pinned staging,
    // device copy, and the event after the last launch that reads it; reused round-robin
    struct Slab {
        char *host = nullptr, *dev = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
    };
    std::vector<Slab> slabs;
    size_t next = 0;
    EventPairs timed;  // timing pairs (start, stop)
    int timing = 0;
    long long timing_seq = 0;
};

namespace {

int group_check(hmmbw_group *g, bool need_armed) {
    if (!g || g->m.empty()) return fail(HMMBW_E_INVALID, "null or empty group");
    hmmbw_ctx *c0 = g->m[0];
    for (hmmbw_ctx *c : g->m) {
        if (int rc = check_ready(c, need_armed)) return rc;
        if (c->world != 1) return fail(HMMBW_E_STATE, "group members are single-rank contexts");
        if (c->ar_open) return fail(HMMBW_E_STATE, "a group member has an open iteration (hmmbw_iterate_end first)");
        if (c->device != c0->device || c->stream != c0->stream)
            return fail(HMMBW_E_INVALID, "group members must share the device and the stream");
        if (c->N != c0->N || c->K != c0->K || c->topo != c0->topo || c->wide || !c->lds_tables())
            return fail(HMMBW_E_UNSUPPORTED, "group members must share N, M and topology (small-N path with LDS tables)");
    }
    return HMMBW_OK;
}

// Enqueue n_launch grouped launches; plans[l * n + i] is member i's plan for launch l.
int group_launch(hmmbw_group *g, const std::vector<Plan> &plans, int n_launch, bool timed) {
    const int n = (int)g->m.size();
    hipStream_t st = g->m[0]->stream;
    const size_t args_b = sizeof(EArgs) * (size_t)n, start_b = sizeof(long long) * (size_t)(n + 1);
    const size_t per = (args_b + start_b + 255) & ~(size_t)255;
    const size_t need = per * (size_t)n_launch;
    if (g->slabs.size() < 4) g->slabs.resize(4);
    hmmbw_group::Slab &sl = g->slabs[g->next];
    g->next = (g->next + 1) % g->slabs.size();
    if (sl.ev) HIP_TRY(hipEventSynchronize(sl.ev));  // its previous launches have read it
    else HIP_TRY(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (sl.cap < need) {
        if (sl.host) HIP_TRY(hipHostFree(sl.host));
        if (sl.dev) {
            ledger_remove(sl.dev, "hipFree (group args)");
            HIP_TRY(hipFree(sl.dev));
        }
        sl.host = sl.dev = nullptr;
        sl.cap = 0;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sl.host), need));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sl.dev), need));
        ledger_add(sl.dev, need, "hipMalloc (group args)");
        sl.cap = need;
    }
    std::vector<unsigned> grid((size_t)n_launch, 0);
    size_t lds = 0;
    for (int l = 0; l < n_launch; ++l) {
        EArgs *A = reinterpret_cast<EArgs *>(sl.host + per * l);
        long long *S = reinterpret_cast<long long *>(sl.host + per * l + args_b);
        long long b = 0;
        for (int i = 0; i < n; ++i) {
            const Plan &p = plans[(size_t)l * n + i];
            A[i] = p.a;
            S[i] = b;
            b += p.grid;
            lds = std::max(lds, p.lds);
        }
        S[n] = b;
        grid[(size_t)l] = (unsigned)b;
    }
    HIP_TRY(hipMemcpyAsync(sl.dev, sl.host, need, hipMemcpyHostToDevice, st));
    const GroupFn f = plans[0].gfn;
    if (lds > 64 * 1024)
        if (int rc = allow_lds(reinterpret_cast<const void *>(f), lds)) return rc;
    for (int l = 0; l < n_launch; ++l) {
        if (grid[(size_t)l] == 0) continue;
        GroupArgs ga{reinterpret_cast<const EArgs *>(sl.dev + per * l),
                     reinterpret_cast<const long long *>(sl.dev + per * l + args_b), n};
        const bool t = timed && g->timing && (g->timing_seq++ % g->timing) == 0;
        if (t)
            if (int rc = g->timed.take(st)) return rc;
        hipLaunchKernelGGL(f, dim3(grid[(size_t)l]), dim3(kBlock), lds, st, ga);
        HIP_TRY(hipGetLastError());
        if (t)
            if (int rc = g->timed.done(st)) return rc;
    }
    HIP_TRY(hipEventRecord(sl.ev, st));
    return HMMBW_OK;
}

}  // namespace

extern "C" {

int hmmbw_group_create(hmmbw_ctx *const *ctxs, int n, hmmbw_group **out) {
    if (!out || (!ctxs && n > 0)) return fail(HMMBW_E_INVALID, "null argument");
    if (n <= 0) return fail(HMMBW_E_INVALID, "a group needs at least one context");
    *out = nullptr;
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]) return fail(HMMBW_E_INVALID, "null context in group");
        for (int k = 0; k < i; ++k)
            if (ctxs[k] == ctxs[i]) return fail(HMMBW_E_INVALID, "a context appears twice in the group");
    }
    hmmbw_group *g = new hmmbw_group();
    g->m.assign(ctxs, ctxs + n);
    if (int rc = group_check(g, false)) {  // members must be set up and of one groupable shape
        delete g;
        return rc;
    }
    *out = g;
    return HMMBW_OK;
}

int hmmbw_group_destroy(hmmbw_group *g) {
    if (!g) return HMMBW_OK;
    if (!g->m.empty()) (void)hipSetDevice(g->m[0]->device);
    for (auto &sl : g->slabs) {
        if (sl.ev) {
            (void)hipEventSynchronize(sl.ev);
            (void)hipEventDestroy(sl.ev);
        }
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.dev) {
            ledger_remove(sl.dev, "hipFree (group args)");
            (void)hipFree(sl.dev);
        }
    }
    g->timed.destroy();
    delete g;
    return HMMBW_OK;
}

int hmmbw_group_iterate(hmmbw_group *g, int64_t n_iter) {
    if (int rc = group_check(g, true)) return rc;
    if (n_iter <= 0) return HMMBW_OK;
    const int n = (int)g->m.size();
    constexpr int64_t kBatch = 64;  // launches per argument slab
    std::vector<Plan> plans;
    for (int64_t i0 = 0; i0 < n_iter; i0 += kBatch) {
        const int nl = (int)std::min<int64_t>(kBatch, n_iter - i0);
        plans.assign((size_t)nl * n, Plan{});
        // Members whose M-step cannot run in the E-step prologue need their own M-step kernel
        // between two grouped launches; then the batch is one launch at a time.
        bool all_merge = true;
        for (hmmbw_ctx *c : g->m) all_merge = all_merge && c->can_merge();
        const int step = all_merge ? nl : 1;
        for (int l0 = 0; l0 < nl; l0 += step) {
            for (int l = l0; l < l0 + step; ++l)
                for (int i = 0; i < n; ++i) {
                    hmmbw_ctx *c = g->m[(size_t)i];
                    long long e = 0;
                    if (int rc = next_estep(c, &e)) return rc;
                    Plan &p = plans[(size_t)l * n + i];
                    // allow_join = false: a grouped kernel never runs the joined map
                    if (int rc = plan_estep(c, c->io_local(e), false, &p)) return rc;
                    if (!p.gfn || p.gfn != plans[0].gfn || p.block != kBlock)
                        return fail(HMMBW_E_UNSUPPORTED, "group members need the same grouped kernel");
                    // planned here, enqueued later: the launch reads the slots through the plan's pointers, so
                    // the flip a context's own launch does when it is enqueued is this loop's
                    if (p.flip) c->scur ^= 1;
                    // map.nblocks, not last_nll (which only a context's own launch sets): without the joined map
                    // and outside the deterministic mode, ncopies sources and a pair per workgroup
                    pend_local(c, e, c->map.nblocks);
                }
            if (step == nl) {
                if (int rc = group_launch(g, plans, nl, true)) return rc;
            } else {
                std::vector<Plan> one(plans.begin() + (size_t)l0 * n, plans.begin() + (size_t)(l0 + 1) * n);
                if (int rc = group_launch(g, one, 1, true)) return rc;
                for (hmmbw_ctx *c : g->m)
                    if (!c->can_merge())
                        if (int rc = flush_mstep(c)) return rc;
            }
        }
    }
    return HMMBW_OK;
}

int hmmbw_group_score(hmmbw_group *g, double *out) {
    if (int rc = group_check(g, false)) return rc;
    if (!out) return fail(HMMBW_E_INVALID, "null argument");
    const int n = (int)g->m.size();
    std::vector<Plan> plans((size_t)n);
    for (int i = 0; i < n; ++i) {
        hmmbw_ctx *c = g->m[(size_t)i];
        if (int rc = flush_mstep(c)) return rc;
        if (int rc = plan_score(c, &plans[(size_t)i])) return rc;
        if (!plans[(size_t)i].gfn || plans[(size_t)i].gfn != plans[0].gfn)
            return fail(HMMBW_E_UNSUPPORTED, "group members need the same grouped kernel");
    }
    if (int rc = group_launch(g, plans, 1, false)) return rc;
    long long off = 0;
    for (hmmbw_ctx *c : g->m) {
        if (c->R > 0)
            HIP_TRY(hipMemcpyAsync(out + off, c->d_logp, sizeof(double) * c->R, hipMemcpyDeviceToHost, c->stream));
        off += c->R;
    }
    HIP_TRY(hipStreamSynchronize(g->m[0]->stream));
    return HMMBW_OK;
}

int hmmbw_group_timing(hmmbw_group *g, int enable, double *total_ms, int64_t *count) {
    if (!g || g->m.empty()) return fail(HMMBW_E_INVALID, "null or empty group");
    if (int rc = set_device(g->m[0])) return rc;
    if (int rc = g->timed.drain()) return rc;
    if (total_ms) *total_ms = g->timed.ms;
    if (count) *count = g->timed.n;
    if (enable >= 0) {
        g->timing = enable;
        g->timing_seq = 0;
        g->timed.ms = 0.0;
        g->timed.n = 0;
    }
    return HMMBW_OK;
}

}  // extern "C"
