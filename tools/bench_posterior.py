#!/usr/bin/env python3
"""State posteriors (hmmbw_posterior) beside the forward scorer (hmmbw_score) and one E-step iteration
(hmmbw_iterate) on the same context: time per call from HIP events on the engine's stream.

Shapes: cfg3 (10,000 x T=200, N=8, K=256) left-to-right and dense, and the cfg5 shard (6,250 x T=400, N=64,
K=1024).  Every call is timed on its own after a warm-up; the median and the 10th / 90th percentiles are reported,
so the spread stands beside the figure.  Three forms of the call: gamma into a device tensor (no copy to the host
but the log-likelihoods, 8 bytes per sequence), the path only (the library's scratch buffer; the copy of the path,
4 bytes per symbol, is included), and log P only (the forward alone).  The gamma form is also set against its
traffic floor: alpha_hat written, read back and gamma written, 3 x total x N x 8 bytes at 8 TB/s; the ratio is
reported, nothing is gated on it.

    python tools/bench_posterior.py [--reps 40] [--warmup 5] [--out profiles/posterior/bench_posterior.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("cfg3_lr", 10_000, 200, 8, 256, "left_to_right"), ("cfg3_dense", 10_000, 200, 8, 256, "dense"),
          ("cfg5_shard", 6_250, 400, 64, 1024, "dense")]
HBM_BYTES_PER_US = 8.0e6  # 8 TB/s, the datasheet rate


def spread(us):
    us = np.sort(np.asarray(us))
    return {"median_us": float(np.median(us)), "p10_us": float(np.percentile(us, 10)),
            "p90_us": float(np.percentile(us, 90)), "n": int(us.size)}


def timed(torch, stream, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    dev = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1) * 1e3)
    return spread(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_posterior: no HIP device")
    from hmm_training_amd._lib import check
    from hmm_training_amd.engine import BaumWelchEngine
    from hmm_training_amd.hmm_training import default_initial_params
    rows = []
    for name, R, T, N, K, topology in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        rng = np.random.default_rng(0)
        pi, A, _ = default_initial_params(N, K)
        if topology == "dense":
            A = 0.5 * A + 0.5 * rng.dirichlet(np.ones(N), size=N)
        B = rng.dirichlet(np.full(K, 2.0), size=N)
        offsets = np.arange(R + 1, dtype=np.int64) * T
        symbols = rng.integers(0, K, size=R * T).astype(np.int32)
        total = R * T
        with BaumWelchEngine(N, K, topology=topology) as e:
            e.set_observations(offsets=offsets, symbols=symbols)
            e.set_params(pi, A, B)
            st = torch.cuda.current_stream(e.device)
            # the C calls themselves, into buffers made once: no Python work between the events
            logp, path, ctx, L = np.zeros(R), np.zeros(total, dtype=np.int32), e._ctx, e._lib
            gam = torch.empty((total, N), dtype=torch.float64, device=f"cuda:{e.device}")
            g, lp, pa = ctypes.c_void_p(gam.data_ptr()), logp.ctypes.data, path.ctypes.data
            res = {"shape": name, "sequences": R, "T": T, "N": N, "K": K, "topology": e.topology,
                   "device": torch.cuda.get_device_name(e.device),
                   "posterior_gamma": timed(torch, st, lambda: check(L.hmmbw_posterior(ctx, g, total * N, None, total, lp)),
                                            a.warmup, a.reps),
                   "posterior_path_only": timed(torch, st, lambda: check(L.hmmbw_posterior(ctx, None, total * N, pa, total, None)),
                                                a.warmup, a.reps),
                   "posterior_logp_only": timed(torch, st, lambda: check(L.hmmbw_posterior(ctx, None, total * N, None, total, lp)),
                                                a.warmup, a.reps),
                   "score": timed(torch, st, lambda: check(L.hmmbw_score(ctx, lp)), a.warmup, a.reps)}
            # the timed calls compute what the tests check: rows that sum to 1, the scorer's log P
            g1, p1, l1 = e.posterior()
            res["max_row_sum_error"] = float((g1.sum(dim=1) - 1.0).abs().max().item())
            res["max_logp_rel_diff_to_score"] = float(np.max(np.abs(l1 - e.score()) / np.abs(l1)))
            del g1
            # one EM iteration (E-step; its M-step runs in the prologue of the next launch) on the same context,
            # with a stop rule that never fires; after the posterior timings, so those see the initial parameters
            e.reset(0.0, 10 ** 9)
            res["estep_iteration"] = timed(torch, st, lambda: check(L.hmmbw_iterate(ctx, 1)), a.warmup, a.reps)
        floor = 3.0 * total * N * 8 / HBM_BYTES_PER_US
        res["gamma_traffic_floor_us"] = floor
        res["ratio_gamma_over_floor"] = res["posterior_gamma"]["median_us"] / floor
        for k in ("score", "estep_iteration"):
            res[f"ratio_gamma_over_{k}"] = res["posterior_gamma"]["median_us"] / res[k]["median_us"]
        res["ratio_logp_only_over_score"] = res["posterior_logp_only"]["median_us"] / res["score"]["median_us"]
        rows.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_posterior.py", "reps": a.reps, "warmup": a.warmup, "results": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
