#!/usr/bin/env python3
"""Embedded training (hmmbw_embedded_train): the time of one iteration (E-step, per-word M-step, convergence step)
from HIP events on the engine's stream, beside two references measured in the same run, neither of which is the
code under test:
  (a) the NumPy checker of the tests (tests/embedded_ref.py) doing the same iteration on the host (on the long
      shape on the first --checker-utts utterances, scaled to all of them: it says so);
  (b) hmmbw_posterior on the same loaded observations for a single dense model of min(64, L N) states, L the longest
      transcript: the existing kernel that does the nearest amount of work per frame (one lane per composite state
      instead of one lane per word instance).

Shapes: 10 words x N = 5 left-to-right, K = 256; 2,000 utterances of 3 to 5 words, and 200 utterances of 64 words,
about 20 frames per word.  A call is synchronous and stages the bank, allocates the workspace and reads the bank back,
so the iteration's time is the difference of a call of 1 + --iters iterations and a call of 1 iteration, divided by
--iters (all within one 16-iteration chunk: one read of the device state either way); the whole 1-iteration call is
reported beside it.  Every call is timed on its own after a warm-up; medians, minima and the 10th / 90th percentiles.

    python tools/bench_embedded.py [--reps 20] [--warmup 3] [--iters 8] [--only NAME] [--out profiles/embedded/bench_embedded.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_viterbi import timed  # noqa: E402  (the protocol: HIP events per call, warm-up, spread)

#          name          W   N  K    R     words    frames per word
SHAPES = [("short_3to5", 10, 5, 256, 2000, (3, 5), 20), ("long_64", 10, 5, 256, 200, (64, 64), 20)]


def make_case(W, N, K, R, words, per_word, rng):
    from hmm_training_amd.hmm_training import default_initial_params
    pi0, A0, _ = default_initial_params(N, K)
    bank = (np.tile(pi0, (W, 1)), np.tile(A0, (W, 1, 1)), rng.dirichlet(np.full(K, 2.0), size=(W, N)))
    lens = rng.integers(words[0], words[1] + 1, size=R)
    transcripts = [[int(x) for x in rng.integers(0, W, size=int(L))] for L in lens]
    T = [int(L) * per_word + int(rng.integers(-per_word // 4, per_word // 4 + 1)) for L in lens]
    return bank, transcripts, [rng.integers(0, K, size=t) for t in T]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--checker-utts", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    a = ap.parse_args()
    assert 1 <= a.iters <= 15
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_embedded: no HIP device")
    import embedded_ref as ER
    from hmm_training_amd._lib import check
    from hmm_training_amd.engine import BaumWelchEngine
    from hmm_training_amd.hmm_training import default_initial_params
    rows = []
    for name, W, N, K, R, words, per_word in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        rng = np.random.default_rng(0)
        (pi, A, B), transcripts, obs = make_case(W, N, K, R, words, per_word, rng)
        longest = max(len(t) for t in transcripts)
        res = {"shape": name, "words": W, "N": N, "K": K, "utterances": R, "longest_transcript": longest,
               "frames": int(sum(len(o) for o in obs)), "instances": int(sum(len(t) for t in transcripts))}
        off = np.zeros(R + 1, dtype=np.int64)
        np.cumsum([len(t) for t in transcripts], out=off[1:])
        ids = np.concatenate(transcripts).astype(np.int32)
        with BaumWelchEngine(N, K) as e:
            e.set_observations(obs)
            st = torch.cuda.current_stream(e.device)
            res["device"] = torch.cuda.get_device_name(e.device)
            ctx, L = e._ctx, e._lib
            p, q, b = pi.copy(), A.copy(), B.copy()

            def call(iters):
                p[:], q[:], b[:] = pi, A, B  # the start bank again: the call trains in place
                check(L.hmmbw_embedded_train(ctx, W, p.ctypes.data, q.ctypes.data, b.ctypes.data, off.ctypes.data,
                                             ids.ctypes.data, R, 0, 0.0, iters, 0, None, 0, None, None))
            one = timed(torch, st, lambda: call(1), a.warmup, a.reps)
            many = timed(torch, st, lambda: call(1 + a.iters), a.warmup, a.reps)
            res["call_1_iteration"], res[f"call_{1 + a.iters}_iterations"] = one, many
            res["iteration_us"] = (many["events"]["median_us"] - one["events"]["median_us"]) / a.iters
            # the timed code computes what the tests check
            got = e.embedded_train(pi, A, B, transcripts, epsilon=0.0, max_iterations=1, normalise=False)
        n_chk = R if R * longest <= 20000 else min(R, a.checker_utts)
        t0 = time.perf_counter()
        ref = ER.train(obs[:n_chk], transcripts[:n_chk], pi, A, B, 0.0, 1)
        res["checker_us"] = (time.perf_counter() - t0) * 1e6 * R / n_chk
        res["checker_utterances_timed"] = n_chk
        res["max_rel_logp_difference_to_checker"] = float(np.max(np.abs(got[4][:n_chk] - ref[4]) / np.abs(ref[4])))
        # (b) one dense model of min(64, L N) states on the same observations
        Np = min(64, longest * N)
        ppi, pA, _ = default_initial_params(Np, K)
        pA = 0.5 * pA + 0.5 * rng.dirichlet(np.ones(Np), size=Np)
        pB = rng.dirichlet(np.full(K, 2.0), size=Np)
        with BaumWelchEngine(Np, K, topology="dense") as e:
            e.set_observations(obs)
            e.set_params(ppi, pA, pB)
            st = torch.cuda.current_stream(e.device)
            total = res["frames"]
            g = torch.empty((total, Np), dtype=torch.float64, device=f"cuda:{e.device}")
            logp = np.zeros(R)
            ctx, L = e._ctx, e._lib
            res["posterior_states"] = Np
            res["posterior"] = timed(torch, st, lambda: check(L.hmmbw_posterior(
                ctx, ctypes_ptr(g), total * Np, None, total, logp.ctypes.data)), a.warmup, a.reps)
        res["ratio_iteration_over_posterior"] = res["iteration_us"] / res["posterior"]["events"]["median_us"]
        res["ratio_checker_over_iteration"] = res["checker_us"] / res["iteration_us"]
        rows.append(res)
        print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/bench_embedded.py", "reps": a.reps, "warmup": a.warmup, "iters": a.iters,
                       "results": rows}, fh, indent=1)
            fh.write("\n")


def ctypes_ptr(tensor):
    import ctypes
    return ctypes.c_void_p(tensor.data_ptr())


if __name__ == "__main__":
    main()
