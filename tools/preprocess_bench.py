#!/usr/bin/env python3
"""Signal conditioning (hmmbw_preprocess, hmmbw_window_overlap) against its two yardsticks.

    python tools/preprocess_bench.py [--recordings 2000,1] [--reps 9] [--out profiles/preprocess/bench_preprocess.json]

Every GPU step is a fresh child process under its own `timeout`; the first step that fails ends the run.  Steps:

* gpu:   R recordings x 32,000 samples (R = 2,000 and R = 1, the live case), batch mode (one launch) and live mode (two
         launches back to back), samples resident as int16 and as float64.  `kernel_ms`: device events around K calls
         in a row on resident buffers, divided by K, after a warm-up; median, minimum and maximum of --reps windows.
         `end_to_end_ms`: a host clock around frontend.preprocess_recordings' device part (one upload of the samples
         and offsets from pageable host memory, the launches, a synchronise), without the read-back of the result.
         Beside them, in the same process and alternating with the kernel windows, `copy_ms`: a device-to-device copy
         that moves the bytes the algorithm has to move (samples in, 8 bytes per sample out, and in live mode the
         trimmed samples read and written once more), i.e. a copy of half that many bytes: the floor a streaming
         kernel can be held to.  `ratio_to_copy` is kernel over copy.
* cpu:   the vectorised NumPy restatement (tests/preprocess_ref.py) on one CPU thread, per recording of 32,000 samples.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N = 32000
DISTINCT = 40


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def recordings(R):
    import preprocess_ref as P
    base = [P.golden_input(N, ("middle", "start", "end")[i % 3], 500 + i)[:, 0] for i in range(min(R, DISTINCT))]
    return [base[i % len(base)] for i in range(R)]


def step_gpu(a):
    import torch

    import preprocess_ref as P
    from hmm_training_amd import frontend
    from hmm_training_amd._lib import SAMPLES_F64, SAMPLES_I16, check, lib
    R = a.recordings
    dev = torch.device("cuda", torch.cuda.current_device())
    sigs = recordings(R)
    offs = np.arange(R + 1, dtype=np.int64) * N
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    toff = torch.from_numpy(offs).to(dev)
    y = torch.empty(R * N, dtype=torch.float64, device=dev)
    bounds = torch.zeros((R, 2), dtype=torch.int64, device=dev)
    tw = torch.from_numpy(P.window_table()).to(dev)
    K = 5 if R >= 100 else 50
    out = []
    for kind in ("int16", "float64"):
        host = np.concatenate(sigs).astype(np.int16 if kind == "int16" else np.float64)
        tx = torch.from_numpy(host).to(dev)
        for mode in ("batch", "live"):
            fac = np.array(frontend.FACTORS[mode])

            def go():
                check(lib().hmmbw_preprocess(st, p(tx), SAMPLES_I16 if kind == "int16" else SAMPLES_F64, p(toff),
                                             ctypes.c_void_p(offs.ctypes.data), R, 0.95, 320, 160,
                                             ctypes.c_void_p(fac.ctypes.data), p(y), p(bounds), None))
                if mode == "live":
                    check(lib().hmmbw_window_overlap(st, p(y), p(toff), p(bounds), R, p(tw), 320, 128))
            go()
            torch.cuda.synchronize()
            trimmed = int((bounds[:, 1] - bounds[:, 0]).clamp(min=0).sum().item())
            moved = host.nbytes + 8 * R * N + (16 * trimmed if mode == "live" else 0)
            src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)

            def window(fn):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / K
            for _ in range(3):
                window(go)
                window(lambda: dst.copy_(src))
            kms, cms = [], []
            for _ in range(a.reps):  # alternating: both see the same neighbours on the machine
                kms.append(window(go))
                cms.append(window(lambda: dst.copy_(src)))
            sig_in = [s.astype(host.dtype) for s in sigs]
            frontend._conditioned_on_device(sig_in[:2], 16000, mode, None, None, dev)
            torch.cuda.synchronize()
            ems = []
            for _ in range(min(a.reps, 5)):
                t0 = time.perf_counter()
                frontend._conditioned_on_device(sig_in, 16000, mode, None, None, dev)
                torch.cuda.synchronize()
                ems.append(1e3 * (time.perf_counter() - t0))
            r = {"recordings": R, "samples": R * N, "upload": kind, "mode": mode, "calls_per_window": K,
                 "kernel_ms": spread(kms), "copy_ms": spread(cms), "bytes_moved": moved, "trimmed_samples": trimmed,
                 "ratio_to_copy": statistics.median(kms) / statistics.median(cms),
                 "kernel_gb_per_s": moved / statistics.median(kms) / 1e6, "end_to_end_ms": spread(ems),
                 "ns_per_sample": 1e6 * statistics.median(kms) / (R * N)}
            out.append(r)
            print(json.dumps(r), flush=True)
        del tx
    print(json.dumps({"gpu": out}))


def step_cpu(a):
    import preprocess_ref as P
    sigs = recordings(6)
    out = {}
    for mode, (fac, win) in (("batch", (P.BATCH, False)), ("live", (P.LIVE, True))):
        P.preprocess(sigs[0], fac, win)
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for s in sigs:
                P.preprocess(s, fac, win)
            ms.append(1e3 * (time.perf_counter() - t0) / len(sigs))
        out[mode] = spread(ms)
    print(json.dumps({"cpu_ms_per_recording": out}))


STEPS = {"gpu": step_gpu, "cpu": step_cpu}


def child(step, a, R, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
           "--recordings", str(R), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, OMP_NUM_THREADS="1") if step == "cpu" else None)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step} failed ({r.returncode}): nothing more is run")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recordings", default="2000,1")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess", "bench_preprocess.json"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    a = ap.parse_args()
    if a.step:
        a.recordings = int(a.recordings)
        return STEPS[a.step](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"samples_per_recording": N, "method": "see tools/preprocess_bench.py", "gpu": []}
    out.update(child("cpu", a, 0, 200))
    for R in (int(s) for s in a.recordings.split(",")):
        out["gpu"] += child("gpu", a, R, 400)["gpu"]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
