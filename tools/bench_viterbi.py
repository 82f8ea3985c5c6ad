#!/usr/bin/env python3
"""Viterbi decoding (hmmbw_viterbi) against the forward scorer (hmmbw_score) on the same context: time per
call from HIP events on the engine's stream, and the host's wall time of the same (synchronous) calls.

Shapes: cfg3 (10,000 x T=200, N=8, K=256) left-to-right and dense, and the cfg5 shard (6,250 x T=400, N=64,
K=1024).  Every call is timed on its own after a warm-up; the median, the minimum and the 10th / 90th
percentiles are reported, so the spread stands beside the figure.  A decode with paths includes the copy of
the path (4 bytes per symbol) to the host, a scores-only decode and the scorer copy 8 bytes per sequence.

    python tools/bench_viterbi.py [--reps 40] [--warmup 5] [--out profiles/viterbi/bench_viterbi.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("cfg3_lr", 10_000, 200, 8, 256, "left_to_right"), ("cfg3_dense", 10_000, 200, 8, 256, "dense"),
          ("cfg5_shard", 6_250, 400, 64, 1024, "dense")]


def spread(us):
    us = np.sort(np.asarray(us))
    return {"median_us": float(np.median(us)), "min_us": float(us[0]), "p10_us": float(np.percentile(us, 10)),
            "p90_us": float(np.percentile(us, 90)), "max_us": float(us[-1]), "n": int(us.size)}


def timed(torch, stream, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e6)
        dev.append(e0.elapsed_time(e1) * 1e3)
    return {"events": spread(dev), "wall": spread(wall)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_viterbi: no HIP device")
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
        with BaumWelchEngine(N, K, topology=topology) as e:
            e.set_observations(offsets=offsets, symbols=symbols)
            e.set_params(pi, A, B)
            st = torch.cuda.current_stream(e.device)
            # the C calls themselves, into buffers made once: no Python work between the events
            logp, path, ctx, L = np.zeros(R), np.zeros(R * T, dtype=np.int32), e._ctx, e._lib
            res = {"shape": name, "sequences": R, "T": T, "N": N, "K": K, "topology": e.topology,
                   "device": torch.cuda.get_device_name(e.device),
                   "viterbi_paths": timed(torch, st, lambda: check(L.hmmbw_viterbi(ctx, logp.ctypes.data, path.ctypes.data,
                                                                                  R * T)), a.warmup, a.reps),
                   "viterbi_scores_only": timed(torch, st, lambda: check(L.hmmbw_viterbi(ctx, logp.ctypes.data, None, R * T)),
                                                a.warmup, a.reps),
                   "score": timed(torch, st, lambda: check(L.hmmbw_score(ctx, logp.ctypes.data)), a.warmup, a.reps)}
            # the same decode twice: the timed code computes what the tests check
            p1, l1 = e.viterbi()
            _, l2 = e.viterbi(paths=False)
            res["finite_logp"] = int(np.isfinite(l1).sum())
            res["scores_only_bit_identical"] = bool(l1.tobytes() == l2.tobytes())
        sc = res["score"]["events"]["median_us"]
        res["ratio_paths_over_score"] = res["viterbi_paths"]["events"]["median_us"] / sc
        res["ratio_scores_only_over_score"] = res["viterbi_scores_only"]["events"]["median_us"] / sc
        rows.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_viterbi.py", "reps": a.reps, "warmup": a.warmup, "results": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
