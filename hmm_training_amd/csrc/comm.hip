// comm.hip — the native RCCL communicator: loader, the all-reduce of the multi-rank hmmbw_iterate, and
// the hmmbw_comm_* ABI.
#include <dlfcn.h>

#include <cstring>

#include "host.hpp"

namespace hmmbw {
namespace {

// RCCL entry points, resolved at run time from the RCCL library already in the process (the one
// torch loaded), so that one RCCL instance serves torch.distributed and the engine.
struct Rccl {
    bool ok = false;
    ncclResult_t (*get_unique_id)(ncclUniqueId *) = nullptr;
    ncclResult_t (*comm_init_rank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
    ncclResult_t (*all_reduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                               hipStream_t) = nullptr;
    const char *(*error_string)(ncclResult_t) = nullptr;
    ncclResult_t (*comm_count)(ncclComm_t, int *) = nullptr;  // optional (hmmbw_comm_info)
};

int rccl_load(const char *path, Rccl **out) {
    static Rccl r;
    static std::string err;
    if (!r.ok) {
        void *h = nullptr;
        if (path && *path) h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail(HMMBW_E_UNSUPPORTED, std::string("cannot load RCCL: ") + dlerror());
        r.get_unique_id = reinterpret_cast<decltype(r.get_unique_id)>(dlsym(h, "ncclGetUniqueId"));
        r.comm_init_rank = reinterpret_cast<decltype(r.comm_init_rank)>(dlsym(h, "ncclCommInitRank"));
        r.comm_destroy = reinterpret_cast<decltype(r.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
        r.all_reduce = reinterpret_cast<decltype(r.all_reduce)>(dlsym(h, "ncclAllReduce"));
        r.error_string = reinterpret_cast<decltype(r.error_string)>(dlsym(h, "ncclGetErrorString"));
        r.comm_count = reinterpret_cast<decltype(r.comm_count)>(dlsym(h, "ncclCommCount"));
        if (!r.get_unique_id || !r.comm_init_rank || !r.comm_destroy || !r.all_reduce || !r.error_string)
            return fail(HMMBW_E_UNSUPPORTED, "RCCL library lacks the ncclGetUniqueId / ncclCommInitRank / "
                                             "ncclCommDestroy / ncclAllReduce / ncclGetErrorString symbols");
        r.ok = true;
    }
    *out = &r;
    return HMMBW_OK;
}

int rccl_fail(const Rccl *r, ncclResult_t e, const char *what) {
    return fail(HMMBW_E_HIP, std::string(what) + ": " + (r && r->error_string ? r->error_string(e) : "RCCL error"));
}

}  // namespace

int comm_allreduce(hmmbw_ctx *c, double *buf, long long len) {
    Rccl *r = nullptr;
    if (int rc = rccl_load(nullptr, &r)) return rc;
    ncclResult_t e = r->all_reduce(buf, buf, (size_t)len, ncclFloat64, ncclSum, c->comm, c->stream);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclAllReduce");
    return HMMBW_OK;
}

void comm_destroy(hmmbw_ctx *c) {
    if (!c->comm) return;
    Rccl *r = nullptr;
    if (rccl_load(nullptr, &r) == HMMBW_OK) (void)r->comm_destroy(c->comm);
    c->comm = nullptr;
}

}  // namespace hmmbw

extern "C" {

int hmmbw_comm_probe(const char *rccl_path) {
    Rccl *r = nullptr;
    return rccl_load(rccl_path, &r);
}

int hmmbw_comm_unique_id(const char *rccl_path, void *id_out) {
    if (!id_out) return fail(HMMBW_E_INVALID, "null argument");
    Rccl *r = nullptr;
    if (int rc = rccl_load(rccl_path, &r)) return rc;
    ncclUniqueId id;
    ncclResult_t e = r->get_unique_id(&id);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclGetUniqueId");
    std::memcpy(id_out, &id, sizeof(id));
    return HMMBW_OK;
}

int hmmbw_comm_init(hmmbw_ctx *c, const char *rccl_path, const void *id, int rank, int world, int64_t n_seq_global) {
    if (!c || !id) return fail(HMMBW_E_INVALID, "null argument");
    if (world < 1 || rank < 0 || rank >= world) return fail(HMMBW_E_INVALID, "need 0 <= rank < world");
    if (c->world != world || c->rank != rank) return fail(HMMBW_E_STATE, "hmmbw_set_rank first, with the same rank/world");
    if (n_seq_global < 0) return fail(HMMBW_E_INVALID, "negative sequence count");
    Rccl *r = nullptr;
    if (int rc = rccl_load(rccl_path, &r)) return rc;
    if (int rc = set_device(c)) return rc;
    if (c->comm) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        (void)r->comm_destroy(c->comm);
        c->comm = nullptr;
    }
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    ncclResult_t e = r->comm_init_rank(&comm, world, uid, rank);
    if (e != ncclSuccess) return rccl_fail(r, e, "ncclCommInitRank");
    sync_ctx(c);
    dfree(c->d_ext);
    if (int rc = dalloc(&c->d_ext, (size_t)c->stats_len())) {
        (void)r->comm_destroy(comm);
        return rc;
    }
    HIP_TRY(hipMemset(c->d_ext, 0, sizeof(double) * (size_t)c->stats_len()));
    c->ext_len = c->stats_len();
    c->comm = comm;
    c->R_global = n_seq_global;
    return HMMBW_OK;
}

int hmmbw_comm_payload(const hmmbw_ctx *c, int64_t *n_doubles) {
    if (!c || !n_doubles) return fail(HMMBW_E_INVALID, "null argument");
    *n_doubles = c->ar_len_last;
    return HMMBW_OK;
}

int hmmbw_comm_info(hmmbw_ctx *c, int *n_ranks, double *total_ms, int64_t *count, int reset) {
    if (!c) return fail(HMMBW_E_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    int n = 0;
    if (c->comm) {
        Rccl *r = nullptr;
        if (int rc = rccl_load(nullptr, &r)) return rc;
        n = -1;  // communicator exists but this RCCL has no ncclCommCount
        if (r->comm_count) {
            ncclResult_t e = r->comm_count(c->comm, &n);
            if (e != ncclSuccess) return rccl_fail(r, e, "ncclCommCount");
        }
    }
    if (int rc = c->ar_timed.drain()) return rc;
    if (n_ranks) *n_ranks = n;
    if (total_ms) *total_ms = c->ar_timed.ms;
    if (count) *count = c->ar_timed.n;
    if (reset) {
        c->ar_timed.ms = 0.0;
        c->ar_timed.n = 0;
        c->ar_seq = 0;
    }
    return HMMBW_OK;
}

}  // extern "C"
