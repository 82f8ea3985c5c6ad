#!/usr/bin/env python3
"""LBG codebook training (hmmbw_lbg_train) against its floor, the VQ encoder's scan.

    python tools/lbg_bench.py [--frames 2000000] [--parent-lib PATH/libhmmbw.so] [--out profiles/lbg/bench_lbg.json]

Every GPU step is a fresh child process under its own `timeout`; the first step that fails ends the run.  Steps:

* pass:     the time of ONE assign-and-accumulate + update pass at K centroids, stride 13, dims 12.  hmmbw_lbg_train
            has no per-pass clock and is synchronous, so the time comes from whole calls with epsilon = 0 (every
            generation runs to its cap): with T_K(m) the wall time of a call with n_centroids = K and max_iterations =
            m, T_K(m2) - T_K(m1) holds m2 - m1 extra passes of every generation 1..log2 K, and subtracting the same
            difference at K / 2 leaves the extra passes of the last generation alone.  Calls alternate and the median
            of --reps differences is reported with its spread.
* small-k:  the same at K = 2, 8, 64 with the rows reduced across the wave first (HMMBW_LBG_WAVE_K=1024) and with
            per-lane LDS atomics only (HMMBW_LBG_WAVE_K=0).
* encoder:  hmmbw_vq_encode alone (device events, 20 launches after 3) on the same frames and the trained centroids,
            with this tree's library and, given --parent-lib, with a library built from the parent commit.
* run:      one real training run (epsilon 1e-3, 100 passes at the most): passes per generation and wall time.

The frames are the encoder's full-size shape of tests/test_gpu_vq.py: 256 Gaussian clusters, 2,000,000 frames.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M1, M2 = 2, 18  # max_iterations of the two calls whose difference is timed


def make_frames(F, seed=7):
    rng = np.random.default_rng(seed)
    cents = rng.normal(size=(256, 13)) * 4.0
    return cents[rng.integers(0, 256, size=F)] + rng.normal(size=(F, 13))


class Trainer:
    """hmmbw_lbg_train on frames resident on the device; returns (seconds, passes per generation)."""

    def __init__(self, F):
        import torch

        from hmm_training_amd._lib import LbgRecord, check, lib
        self.torch, self.check, self.L, self.Rec = torch, check, lib(), LbgRecord
        self.F = F
        self.tf = torch.from_numpy(make_frames(F)).cuda()
        self.tc = torch.empty((1024, 13), dtype=torch.float64, device="cuda")
        self.st = torch.cuda.current_stream().cuda_stream

    def train(self, K, max_it, eps=0.0):
        cap = 16 * max_it
        rec = (self.Rec * cap)()
        n = ctypes.c_int64(0)
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.check(self.L.hmmbw_lbg_train(ctypes.c_void_p(self.st), ctypes.c_void_p(self.tf.data_ptr()), self.F, 13, 1, 12, K,
                                          eps, max_it, 1.001, 0.999, ctypes.c_void_p(self.tc.data_ptr()), None, None,
                                          ctypes.cast(rec, ctypes.c_void_p), cap, ctypes.byref(n)))
        dt = time.perf_counter() - t0
        gens = [r.generation for r in rec[:n.value]]
        return dt, [gens.count(g) for g in range(1, max(gens) + 1)]

    def pass_ms(self, K, reps):
        """ms of one pass of the last generation of a K-centroid run (see the module docstring)."""
        sizes = [K] if K == 2 else [K, K // 2]
        for k in sizes:  # warm every shape
            self.train(k, M1)
        diffs, notes = [], set()
        for _ in range(reps):
            t = {}
            for k in sizes:
                for m in (M1, M2):
                    t[k, m] = self.train(k, m)
            extra = t[K, M2][1][-1] - t[K, M1][1][-1]
            if extra != M2 - M1 or (K > 2 and t[K, M2][1][:-1] != t[K // 2, M2][1]):
                notes.add("a generation stopped before its cap (diff == 0): pass counts differ between the calls")
            d = t[K, M2][0] - t[K, M1][0] - (t[K // 2, M2][0] - t[K // 2, M1][0] if K > 2 else 0.0)
            diffs.append(1e3 * d / max(extra, 1))
        return {"K": K, "ms": statistics.median(diffs), "min_ms": min(diffs), "max_ms": max(diffs), "reps": reps,
                "notes": sorted(notes)}


def step_pass(a):
    tr = Trainer(a.frames)
    print(json.dumps({"pass": tr.pass_ms(a.K, a.reps), "wave_k": os.environ.get("HMMBW_LBG_WAVE_K", "default")}))


def step_small_k(a):
    tr = Trainer(a.frames)
    out = {}
    for K in (2, 8, 64):
        row = {}
        for name, env in (("wave_reduce", "1024"), ("lds_atomics", "0")):  # alternating forms per K
            os.environ["HMMBW_LBG_WAVE_K"] = env
            row[name] = tr.pass_ms(K, a.reps)
        out[str(K)] = row
    print(json.dumps({"small_k": out}))


def step_run(a):
    tr = Trainer(a.frames)
    tr.train(a.K, 2)
    dt, passes = tr.train(a.K, 100, 1e-3)
    print(json.dumps({"run": {"K": a.K, "epsilon": 1e-3, "max_iterations": 100, "passes_per_generation": passes,
                              "seconds": dt, "ms_per_pass_all_generations": 1e3 * dt / sum(passes)}}))


def step_encoder(a):
    import torch
    path = a.lib or os.path.join(ROOT, "hmm_training_amd", "libhmmbw.so")
    L = ctypes.CDLL(path)  # the parent's library lacks the new symbol: bind the encoder alone
    L.hmmbw_vq_encode.restype = ctypes.c_int
    L.hmmbw_vq_encode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    tf = torch.from_numpy(make_frames(a.frames)).cuda()
    tc = torch.from_numpy(np.load(a.centroids)).cuda()
    ts = torch.empty(a.frames, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()

    def go():
        rc = L.hmmbw_vq_encode(ctypes.c_void_p(st.cuda_stream), ctypes.c_void_p(tf.data_ptr()), a.frames, 13, 1, 12,
                               ctypes.c_void_p(tc.data_ptr()), tc.shape[0], ctypes.c_void_p(ts.data_ptr()), None)
        if rc != 0:
            raise RuntimeError(f"hmmbw_vq_encode: {rc}")
    for _ in range(3):
        go()
    times = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(20):
            go()
        e1.record(st)
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / 20)
    print(json.dumps({"encoder": {"lib": os.path.basename(path), "ms": statistics.median(times), "min_ms": min(times),
                                  "max_ms": max(times), "checksum": int(ts.to(torch.int64).sum().item())}}))


def step_centroids(a):
    """The trained K-centroid codebook of the frames, for the encoder steps."""
    from hmm_training_amd.codevector import lbg_train
    res = lbg_train(make_frames(a.frames), a.K, 10, 1e-3)
    np.save(a.centroids, res.centroids)
    print(json.dumps({"centroids": {"K": a.K, "passes": len(res.records)}}))


STEPS = {"pass": step_pass, "small-k": step_small_k, "run": step_run, "encoder": step_encoder, "centroids": step_centroids}


def child(step, a, limit, extra=(), env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--frames",
           str(a.frames), "--K", str(a.K), "--reps", str(a.reps), "--centroids", a.centroids, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step} failed ({r.returncode}): nothing more is run")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2_000_000)
    ap.add_argument("--K", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libhmmbw.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lbg", "bench_lbg.json"))
    ap.add_argument("--centroids", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    a.centroids = a.centroids or os.path.splitext(os.path.abspath(a.out))[0] + "_centroids.npy"
    env = {k: v for k, v in os.environ.items() if k != "HMMBW_LBG_WAVE_K"}
    os.environ.clear()
    os.environ.update(env)
    out = {"frames": a.frames, "stride": 13, "dims": 12, "method": "see tools/lbg_bench.py", "m1_m2": [M1, M2]}
    out.update(child("centroids", a, 300))
    out.update(child("pass", a, 300))
    enc = child("encoder", a, 300)["encoder"]
    out["encoder_this_tree"] = enc
    if a.parent_lib:
        par = child("encoder", a, 300, ["--lib", os.path.abspath(a.parent_lib)])["encoder"]
        again = child("encoder", a, 300)["encoder"]  # alternated: the spread of the same code
        out["encoder_parent_commit"] = par
        out["encoder_this_tree_again"] = again
        out["pass_over_parent_encoder"] = out["pass"]["ms"] / par["ms"]
        assert par["checksum"] == enc["checksum"], "the two encoders disagree"
    else:
        out["encoder_parent_commit"] = "not measured (no --parent-lib)"
        out["pass_over_encoder"] = out["pass"]["ms"] / enc["ms"]
    out.update(child("run", a, 300))
    out.update(child("small-k", a, 600))
    os.remove(a.centroids)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
