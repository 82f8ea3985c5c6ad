#!/usr/bin/env python3
"""Forced alignment (hmmbw_align) beside its yardstick, the loop decoder (hmmbw_wordnet_decode).

    python tools/align_bench.py [--seqs 10000] [--steps 200] [--reps 9] [--out profiles/align/bench_align.json]
    python tools/align_bench.py --optional 9 [--out profiles/optional/bench_align_optional.json]

The GPU step is a fresh child process under its own `timeout`.  One context holds --seqs utterances of --steps
frames (uniform random symbols); the bank has 10 left-to-right word models of N = 5 states over K = 256 symbols
(tests/wordnet_ref.py, bank); every utterance has a transcript of 3 to 5 words.  On that context, from the same
process, the four calls are timed in turn:

* align, paths:   hmmbw_align with path_out and bounds_out,
* align, scores:  hmmbw_align with logp_out alone (no back-pointers are stored),
* loop, paths:    hmmbw_wordnet_decode with path_out and start_out, word_init = word_trans = NULL,
* loop, scores:   hmmbw_wordnet_decode with logp_out alone,

all with the END_FINAL rule.  Both entry points are synchronous, so a pair of HIP events recorded around a call
brackets the whole call: the staging of the bank (and of the transcripts), the table kernel, the decoding kernel and
the read-back of the results into pageable host memory.  After a warm-up of 3 calls each (buffers allocated, code
loaded), the median, minimum and maximum of --reps calls are reported, with the wall-clock time of the same calls.
The loop decoder does strictly more per step (a max over the words, 16-lane groups for 10 words where a transcript
of 5 words takes 8), and answers another question: the two are not interchangeable.

With --optional WORD (an index into the bank) the same utterances get transcripts of 3 to 5 of the other words with
WORD as an optional position before, between and after them (`sil? w sil? w sil?`, 7 to 11 positions), and two
calls are timed instead, each with and without paths: hmmbw_align_optional with the flags, and hmmbw_align on the
same transcripts with WORD written in as mandatory, which is the same chain length and group width.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, N, K = 10, 5, 256


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def step_run(a):
    import torch

    import wordnet_ref as WR
    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    rng = np.random.default_rng(7)
    pi, A, B, _, _ = WR.bank(W, N, K, "left_to_right", rng)
    R, T = a.seqs, a.steps
    obs = list(rng.integers(0, K, size=(R, T)))
    lens = rng.integers(3, 6, size=R)
    off = np.zeros(R + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = rng.integers(0, W, size=int(off[-1])).astype(np.int32)
    logp = np.zeros(R)
    path = np.zeros(R * T, dtype=np.int32)
    start = np.zeros(R * T, dtype=np.uint8)
    bounds = np.zeros(int(off[-1]), dtype=np.int32)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    if a.optional is not None:
        return step_optional(a, rng, pi, A, B, obs, lens)
    out = {"seqs": R, "steps": T, "words": W, "states": N, "symbols": K, "positions": int(off[-1])}
    with BaumWelchEngine(N, K) as e:
        e.set_observations(obs)
        lib, ctx = e._lib, e._ctx

        def align(paths):
            _lib.check(lib.hmmbw_align(ctx, W, p(pi), p(A), p(B), p(off), p(ids), R, _lib.ALIGN_END_FINAL, p(logp),
                                       p(path) if paths else None, R * T, p(bounds) if paths else None, len(bounds)))

        def loop(paths):
            _lib.check(lib.hmmbw_wordnet_decode(ctx, W, p(pi), p(A), p(B), None, None, _lib.WORDNET_END_FINAL, p(logp),
                                                p(path) if paths else None, p(start) if paths else None, R * T))

        for name, fn, paths in (("align_paths", align, True), ("align_scores", align, False),
                                ("loop_paths", loop, True), ("loop_scores", loop, False)):
            for _ in range(3):
                fn(paths)
            ev, wall = [], []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                fn(paths)
                e1.record()
                e1.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                ev.append(e0.elapsed_time(e1))
            out[name] = {"event_ms": spread(ev), "wall_ms": spread(wall), "logp_sum": float(logp[np.isfinite(logp)].sum()),
                         "finite": int(np.isfinite(logp).sum())}
    for kind in ("paths", "scores"):
        out[f"align_over_loop_{kind}"] = out[f"align_{kind}"]["event_ms"]["median"] / out[f"loop_{kind}"]["event_ms"]["median"]
    print(json.dumps(out))


def timed_calls(torch, fn, reps):
    for _ in range(3):
        fn()
    ev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(e0.elapsed_time(e1))
    return {"event_ms": spread(ev), "wall_ms": spread(wall)}


def step_optional(a, rng, pi, A, B, obs, lens):
    import torch

    from hmm_training_amd import _lib
    from hmm_training_amd.engine import BaumWelchEngine
    sil = a.optional
    if not 0 <= sil < W:
        raise SystemExit(f"--optional {sil} is no word of the bank (0 .. {W - 1})")
    R, T = a.seqs, a.steps
    others = np.array([w for w in range(W) if w != sil])
    ids, flags = [], []
    off = np.zeros(R + 1, dtype=np.int64)
    for r, n in enumerate(lens):
        ws = others[rng.integers(0, W - 1, size=int(n))]
        t = np.full(2 * int(n) + 1, sil, dtype=np.int32)
        t[1::2] = ws
        f = np.ones(2 * int(n) + 1, dtype=np.uint8)
        f[1::2] = 0
        ids.append(t)
        flags.append(f)
        off[r + 1] = off[r] + len(t)
    ids, flags = np.concatenate(ids), np.concatenate(flags)
    logp = np.zeros(R)
    path = np.zeros(R * T, dtype=np.int32)
    bounds = np.zeros(int(off[-1]), dtype=np.int32)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    out = {"seqs": R, "steps": T, "words": W, "states": N, "symbols": K, "positions": int(off[-1]),
           "optional_word": sil, "optional_positions": int(flags.sum())}
    with BaumWelchEngine(N, K) as e:
        e.set_observations(obs)
        lib, ctx = e._lib, e._ctx

        def call(optional, paths):
            head = (ctx, W, p(pi), p(A), p(B), p(off), p(ids))
            tail = (R, _lib.ALIGN_END_FINAL, p(logp), p(path) if paths else None, R * T, p(bounds) if paths else None,
                    len(bounds))
            if optional:
                _lib.check(lib.hmmbw_align_optional(*head, p(flags), *tail))
            else:
                _lib.check(lib.hmmbw_align(*head, *tail))

        for name, optional, paths in (("optional_paths", True, True), ("optional_scores", True, False),
                                      ("mandatory_paths", False, True), ("mandatory_scores", False, False)):
            out[name] = timed_calls(torch, lambda: call(optional, paths), a.reps)
            out[name].update(logp_sum=float(logp[np.isfinite(logp)].sum()), finite=int(np.isfinite(logp).sum()))
            if paths and optional:
                out["positions_passed_over"] = int((bounds < 0).sum()) if np.isfinite(logp).all() else None
    for kind in ("paths", "scores"):
        out[f"optional_over_mandatory_{kind}"] = (out[f"optional_{kind}"]["event_ms"]["median"] /
                                                  out[f"mandatory_{kind}"]["event_ms"]["median"])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", type=int, default=10000)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="profiles/align/bench_align.json, or with --optional "
                    "profiles/optional/bench_align_optional.json")
    ap.add_argument("--optional", type=int, default=None, metavar="WORD",
                    help="time hmmbw_align_optional with this word of the bank as an optional position at every gap")
    ap.add_argument("--step", choices=["run"], default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", *(("align", "bench_align.json") if a.optional is None
                                                 else ("optional", "bench_align_optional.json")))
    if a.step:
        return step_run(a)
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step", "run", "--seqs", str(a.seqs),
           "--steps", str(a.steps), "--reps", str(a.reps)]
    if a.optional is not None:
        cmd += ["--optional", str(a.optional)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"the GPU step failed ({r.returncode}): nothing more is run")
    out = json.loads(r.stdout.strip().splitlines()[-1])
    out["method"] = "see tools/align_bench.py"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
