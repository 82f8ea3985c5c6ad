#!/usr/bin/env python3
"""Connected-word decoding (hmmbw_wordnet_decode) against the only other way to do the job, hmmbw_viterbi on the
hand-built composite model of W N states, on the same observations: time per call from HIP events on the engine's
stream, and the host's wall time of the same (synchronous) calls.

Shapes: 10 words x 5 states, K = 256, 10,000 x T = 200, left-to-right (the composite has 50 states and runs), and
10 words x 8 states dense (80 states: the composite cannot run, the absolute time only).  Every call is timed on
its own after a warm-up; the median, the minimum and the 10th / 90th percentiles are reported.  A decode with paths
includes the staging of the bank, the log tables, and the copy of the path and the start flags (5 bytes per
symbol) to the host; the composite decode copies 4 bytes per symbol.

    python tools/bench_wordnet.py [--reps 40] [--warmup 5] [--only NAME] [--out profiles/wordnet/bench_wordnet.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_viterbi import timed  # noqa: E402  (the protocol: HIP events per call, warm-up, spread)

SHAPES = [("w10_n5_lr", 10, 5, 256, 10_000, 200, "left_to_right"), ("w10_n8_dense", 10, 8, 256, 10_000, 200, "dense")]


def make_bank(W, N, K, topology, rng):
    from hmm_training_amd.hmm_training import default_initial_params
    pi0, A0, _ = default_initial_params(N, K)
    pi = np.tile(pi0, (W, 1))
    A = np.tile(A0, (W, 1, 1))
    if topology == "dense":
        pi = rng.dirichlet(np.ones(N), size=W)
        A = 0.5 * A + 0.5 * rng.dirichlet(np.ones(N), size=(W, N))
    B = rng.dirichlet(np.full(K, 2.0), size=(W, N))
    return pi, A, B, rng.dirichlet(np.ones(W)), 0.3 * rng.dirichlet(np.ones(W), size=W)


def composite(pi, A, B, init, G):
    """The W N-state model whose ordinary Viterbi score is the word-loop score (connected-word decoding)."""
    W, N = pi.shape
    Ac = np.zeros((W * N, W * N))
    for w in range(W):
        Ac[w * N:(w + 1) * N, w * N:(w + 1) * N] = A[w]
    for v in range(W):
        Ac[v * N + N - 1] = np.maximum(Ac[v * N + N - 1], (G[v][:, None] * pi).reshape(-1))
    return (init[:, None] * pi).reshape(-1), Ac, B.reshape(W * N, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_wordnet: no HIP device")
    from hmm_training_amd._lib import check
    from hmm_training_amd.engine import BaumWelchEngine
    rows = []
    for name, W, N, K, R, T, topology in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        rng = np.random.default_rng(0)
        pi, A, B, init, G = make_bank(W, N, K, topology, rng)
        offsets = np.arange(R + 1, dtype=np.int64) * T
        symbols = rng.integers(0, K, size=R * T).astype(np.int32)
        res = {"shape": name, "words": W, "N": N, "K": K, "sequences": R, "T": T, "topology": topology}
        logp, path, start = np.zeros(R), np.zeros(R * T, dtype=np.int32), np.zeros(R * T, dtype=np.uint8)
        with BaumWelchEngine(N, K) as e:
            e.set_observations(offsets=offsets, symbols=symbols)
            st = torch.cuda.current_stream(e.device)
            res["device"] = torch.cuda.get_device_name(e.device)
            ctx, L = e._ctx, e._lib

            def call(g, with_paths):
                check(L.hmmbw_wordnet_decode(ctx, W, pi.ctypes.data, A.ctypes.data, B.ctypes.data, init.ctypes.data,
                                             g.ctypes.data if g is not None else None, 0, logp.ctypes.data,
                                             path.ctypes.data if with_paths else None,
                                             start.ctypes.data if with_paths else None, R * T))
            # the C calls themselves, into buffers made once: no Python work between the events
            res["wordnet_paths"] = timed(torch, st, lambda: call(G, True), a.warmup, a.reps)
            res["wordnet_scores_only"] = timed(torch, st, lambda: call(G, False), a.warmup, a.reps)
            res["wordnet_paths_no_word_trans"] = timed(torch, st, lambda: call(None, True), a.warmup, a.reps)
            # the same decode twice: the timed code computes what the tests check
            _, _, l1 = e.wordnet_decode(pi, A, B, init, G)
            _, _, l2 = e.wordnet_decode(pi, A, B, init, G, paths=False)
            res["finite_logp"] = int(np.isfinite(l1).sum())
            res["scores_only_bit_identical"] = bool(l1.tobytes() == l2.tobytes())
        if W * N <= 64:
            cpi, cA, cB = composite(pi, A, B, init, G)
            with BaumWelchEngine(W * N, K, topology="dense") as e:
                e.set_observations(offsets=offsets, symbols=symbols)
                e.set_params(cpi, cA, cB)
                st = torch.cuda.current_stream(e.device)
                ctx, L = e._ctx, e._lib
                res["composite_viterbi_paths"] = timed(
                    torch, st, lambda: check(L.hmmbw_viterbi(ctx, logp.ctypes.data, path.ctypes.data, R * T)), a.warmup, a.reps)
                res["composite_viterbi_scores_only"] = timed(
                    torch, st, lambda: check(L.hmmbw_viterbi(ctx, logp.ctypes.data, None, R * T)), a.warmup, a.reps)
                _, l3 = e.viterbi(paths=False)
            res["max_rel_logp_difference_to_composite"] = float(np.max(np.abs(l3 - l1) / np.abs(l3)))
            for k in ("paths", "scores_only"):
                res[f"ratio_composite_over_wordnet_{k}"] = (res[f"composite_viterbi_{k}"]["events"]["median_us"] /
                                                           res[f"wordnet_{k}"]["events"]["median_us"])
        rows.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_wordnet.py", "reps": a.reps, "warmup": a.warmup, "results": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
