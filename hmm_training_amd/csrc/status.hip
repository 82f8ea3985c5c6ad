// status.hip — reading the training state: hmmbw_get_status, the stream snapshots hmmbw_status_post / _wait and
// the live host mirror (HMMBW_OPT_LIVE_STATUS, hmmbw_status_live_wait).
#include <atomic>

#include "host.hpp"

namespace hmmbw {

// Status snapshot for hmmbw_status_post: the state record and the iteration records [first, iteration)
// written straight into pinned host memory (one small launch on the stream instead of DMA copies).
__global__ void __launch_bounds__(256) k_snapshot(const IterState *st, const double *hist, long long first,
                                                   IterState *hst, double *hrec) {
    const IterState s = *st;
    const long long n = min(max(s.iteration - first, 0LL), (long long)kHist);
    for (long long i = threadIdx.x; i < n; i += blockDim.x) {
        const long long k = (first + i) % kHist;
        hrec[2 * i] = hist[2 * k];
        hrec[2 * i + 1] = hist[2 * k + 1];
    }
    if (threadIdx.x == 0) *hst = s;
}

// message of a device-side stop (IterState::error, set with done by a bounded wait that expired)
static std::string device_error(const IterState &h) {
    if (h.error_src == kErrWorkQueue)
        return "EM stopped on a device-side failure: a wide work-queue backward sweep did not see its tile's "
               "forward sweep finish within HMMBW_OPT_WQ_TIMEOUT_MS";
    return "EM stopped on a device-side failure: a rank did not deliver its statistics to the peer all-reduce "
           "within HMMBW_OPT_PEER_TIMEOUT_MS";
}

// every reader's answer: the status of h; a device-side stop is the call's error
static int fill_status(const IterState &h, hmmbw_status *st) {
    st->iterations = h.iteration;
    st->done = h.done;
    st->converged = h.converged;
    st->last_log_likelihood = h.last_L;
    st->last_diff = h.last_diff;
    if (h.error) return fail(h.error, device_error(h));
    return HMMBW_OK;
}

// Records [first, first + count) of a window the caller has validated.  hist is the device ring or its live mirror
// (origin < 0: iteration i lies at i % kHist) or a snapshot, linear from its first iteration `origin`.
static void copy_records(const volatile double *hist, int64_t origin, int64_t first, int64_t count,
                         hmmbw_iter_record *rec) {
    for (int64_t i = 0; i < count; ++i) {
        const int64_t k = origin < 0 ? (first + i) % kHist : first + i - origin;
        rec[i].log_likelihood = hist[2 * k];
        rec[i].diff = hist[2 * k + 1];
    }
}

// the ring's window check and copy (hmmbw_get_status, hmmbw_status_live_wait)
static int ring_records(const IterState &h, const volatile double *hist, int64_t first, int64_t count,
                        hmmbw_iter_record *rec) {
    if (!rec || count <= 0) return HMMBW_OK;
    if (first < 0 || first + count > h.iteration || first < h.iteration - kHist)
        return fail(HMMBW_E_INVALID, "requested iteration records are not available");
    copy_records(hist, -1, first, count, rec);
    return HMMBW_OK;
}

int live_status_set(hmmbw_ctx *c, bool on) {
    if (int rc = set_device(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));  // no launch of the old setting is still in flight
    if (!on) {
        cached_free(c->h_live, kPinnedBlock);
        c->h_live = nullptr;
        return HMMBW_OK;
    }
    if (c->h_live) return HMMBW_OK;
    HIP_TRY(cached_alloc(reinterpret_cast<void **>(&c->h_live), sizeof(LiveBlock), kPinnedBlock));
    // seed the mirror with the state as it stands (records of a pending M-step follow when it runs)
    IterState h{};
    HIP_TRY(hipMemcpy(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(c->h_live->hist, c->d_hist, sizeof(double) * 2 * (size_t)kHist, hipMemcpyDeviceToHost));
    c->h_live->slot[h.iteration & 1] = h;
    std::atomic_thread_fence(std::memory_order_release);
    reinterpret_cast<volatile unsigned long long &>(c->h_live->pub) =
        ((unsigned long long)c->live_epoch << 32) | (unsigned long long)(unsigned)h.iteration;
    return HMMBW_OK;
}

void status_free(hmmbw_ctx *c) {
    for (auto &sn : c->snaps) {
        if (sn.ev) (void)hipEventDestroy(sn.ev);
        cached_free(sn.st, kPinnedBlock);
        cached_free(sn.hist, kPinnedBlock);
    }
    cached_free(c->h_live, kPinnedBlock);
}

}  // namespace hmmbw

extern "C" {

int hmmbw_get_status(hmmbw_ctx *c, hmmbw_status *st, hmmbw_iter_record *rec, int64_t first, int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (int rc = set_device(c)) return rc;
    if (int rc = flush_mstep(c)) return rc;
    IterState h{};
    HIP_TRY(hipMemcpyAsync(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost, c->stream));
    std::vector<double> hist(2 * (size_t)kHist);
    if (rec && count > 0)
        HIP_TRY(hipMemcpyAsync(hist.data(), c->d_hist, sizeof(double) * hist.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = fill_status(h, st)) return rc;
    return ring_records(h, hist.data(), first, count, rec);
}

int hmmbw_status_post(hmmbw_ctx *c, int64_t first, int64_t *ticket) {
    if (!c || !ticket) return fail(HMMBW_E_INVALID, "null argument");
    if (first < 0) return fail(HMMBW_E_INVALID, "negative first iteration");
    if (int rc = set_device(c)) return rc;
    hmmbw_ctx::Snap &sn = c->snaps[c->snap_next % 2];
    if (!sn.ev) {
        HIP_TRY(hipEventCreateWithFlags(&sn.ev, hipEventDisableTiming));
        // fine-grained host memory the snapshot kernel writes (visible once its event has completed)
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&sn.st), sizeof(IterState), kPinnedBlock));
        HIP_TRY(cached_alloc(reinterpret_cast<void **>(&sn.hist), sizeof(double) * 2 * (size_t)kHist, kPinnedBlock));
    } else {
        HIP_TRY(hipEventSynchronize(sn.ev));  // the slot's previous snapshot has landed (two posts ago)
    }
    // no flush: a pending (merged) M-step stays pending, so the snapshot holds the records of every
    // iteration enqueued so far except the last one
    hipLaunchKernelGGL(k_snapshot, dim3(1), dim3(256), 0, c->stream, c->state(), c->d_hist, (long long)first, sn.st,
                       sn.hist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(sn.ev, c->stream));
    sn.first = first;
    sn.ticket = c->snap_next++;
    *ticket = sn.ticket;
    return HMMBW_OK;
}

int hmmbw_status_wait(hmmbw_ctx *c, int64_t ticket, hmmbw_status *st, hmmbw_iter_record *rec, int64_t first,
                      int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (ticket < 0 || ticket >= c->snap_next || ticket < c->snap_next - 2)
        return fail(HMMBW_E_INVALID, "status ticket is not one of the last two posted");
    if (int rc = set_device(c)) return rc;
    hmmbw_ctx::Snap &sn = c->snaps[ticket % 2];
    HIP_TRY(hipEventSynchronize(sn.ev));  // this snapshot only, not the work enqueued after it
    const IterState h = *sn.st;
    if (int rc = fill_status(h, st)) return rc;
    if (rec && count > 0) {
        if (first < sn.first || first + count > h.iteration || first + count > sn.first + kHist ||
            first < h.iteration - kHist)  // overwritten in the ring before the snapshot was taken
            return fail(HMMBW_E_INVALID, "requested iteration records are not in this snapshot");
        copy_records(sn.hist, sn.first, first, count, rec);
    }
    return HMMBW_OK;
}

int hmmbw_status_live_wait(hmmbw_ctx *c, int64_t iterations, hmmbw_status *st, hmmbw_iter_record *rec,
                           int64_t first, int64_t count) {
    if (!c || !st) return fail(HMMBW_E_INVALID, "null argument");
    if (!c->h_live) return fail(HMMBW_E_STATE, "HMMBW_OPT_LIVE_STATUS is off");
    if (int rc = set_device(c)) return rc;
    volatile LiveBlock *lv = c->h_live;
    IterState h{};
    bool have = false;
    for (long long spin = 0;; ++spin) {
        const unsigned long long p0 = lv->pub;
        std::atomic_thread_fence(std::memory_order_acquire);
        if ((unsigned)(p0 >> 32) == c->live_epoch) {
            const long long n = (long long)(unsigned)(p0 & 0xffffffffULL);
            const volatile IterState &sl = lv->slot[n & 1];
            h.prev_L = sl.prev_L;
            h.last_L = sl.last_L;
            h.last_diff = sl.last_diff;
            h.epsilon = sl.epsilon;
            h.iteration = sl.iteration;
            h.max_iterations = sl.max_iterations;
            h.done = sl.done;
            h.converged = sl.converged;
            h.error = sl.error;
            std::atomic_thread_fence(std::memory_order_acquire);
            const unsigned long long p1 = lv->pub;
            // the slot is rewritten only by the record after next: two publications apart
            const bool stable = (unsigned)(p1 >> 32) == c->live_epoch && (long long)(unsigned)(p1 & 0xffffffffULL) <= n + 1;
            if (stable && h.iteration == n && (n >= iterations || h.done)) {
                have = true;
                break;
            }
        }
        // the stream ran dry without the record (a pending M-step, a device-side stop the mirror does not
        // carry, or a reset): the device state is the answer
        if ((spin & 63) == 63 && hipStreamQuery(c->stream) == hipSuccess) {
            const unsigned long long p2 = lv->pub;
            if ((unsigned)(p2 >> 32) == c->live_epoch && (long long)(unsigned)(p2 & 0xffffffffULL) >= iterations) continue;
            break;
        }
    }
    std::vector<double> dh;
    if (!have) {
        HIP_TRY(hipMemcpy(&h, c->state(), sizeof(IterState), hipMemcpyDeviceToHost));
        if (rec && count > 0) {
            dh.resize(2 * (size_t)kHist);
            HIP_TRY(hipMemcpy(dh.data(), c->d_hist, sizeof(double) * dh.size(), hipMemcpyDeviceToHost));
        }
    }
    if (int rc = fill_status(h, st)) return rc;
    return ring_records(h, have ? lv->hist : dh.data(), first, count, rec);
}

}  // extern "C"
