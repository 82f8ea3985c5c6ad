#!/usr/bin/env python3
"""The MFCC front end (hmmbw_mfcc, frontend.encode_recordings) against its two yardsticks.

    python tools/mfcc_bench.py [--sizes 4200,2000000] [--reps 7] [--out profiles/mfcc/bench_mfcc.json]

Every GPU step is a fresh child process under its own `timeout`; the first step that fails ends the run.  Steps:

* kernel:  hmmbw_mfcc at L = 320 on F overlapping frames (hop 160) of one resident signal, F = 4,200 (the reference's
           data set) and 2,000,000 (BASELINE cfg3: 10,000 utterances x 200 frames).  Wall time of the whole
           call to the end of its kernel (the call's own range check and 4-byte read-back included), after a warm-up
           of 3 calls; median, minimum and maximum of --reps calls.  Beside it the kernel's own floor: the matrix
           instructions one wave issues per tile (mfcc_plan.hpp: 2 x bin blocks per wave x (Hp / 4)) x 64 cycles at the
           2.4 GHz peak clock, times the tiles the busiest CU gets (a tile's 4 waves take the CU's 4 SIMDs).
* encode:  frontend.encode_recordings end to end (host framing, one upload, hmmbw_mfcc, hmmbw_vq_encode against 256
           centroids, symbols back) on F / 200 signals of 32,160 samples: 200 full frames and a remainder frame of 160 each,
           so every call runs two frame-length classes.
* cpu:     the NumPy / SciPy restatement (tests/mfcc_ref.py) per frame on one CPU thread, with its tables prebuilt
           and as the reference calls it (tables rebuilt per frame, as librosa's filter-bank cache miss would).
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

L, HOP, WAVES, CLOCK_GHZ, MFMA_CYCLES = 320, 160, 4, 2.4, 64


def make_signal(n, seed=5):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return 1e3 * (np.sin(2 * np.pi * 440.0 * t) + 0.5 * np.sin(2 * np.pi * 1900.0 * t) + 0.1 * rng.normal(size=n))


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def wave_mfmas(frame_len):
    H = frame_len // 2 + 1
    blocks = ((H + 15) // 16 + WAVES - 1) // WAVES
    return 2 * blocks * (((H + 3) // 4 * 4) // 4)


def step_kernel(a):
    import torch

    from hmm_training_amd._lib import check, lib
    from hmm_training_amd.frontend import _device_tables
    F = a.frames
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.from_numpy(make_signal((F - 1) * HOP + L)).to(dev)
    starts = torch.arange(F, dtype=torch.int64, device=dev) * HOP
    out = torch.empty((F, 13), dtype=torch.float64, device=dev)
    win, tw, mel, dct = _device_tables(L, 16000.0, 26, 13, dev)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def go():
        check(lib().hmmbw_mfcc(ctypes.c_void_p(st), p(x), x.numel(), p(starts), F, L, p(win), p(tw), p(mel), 26, p(dct), 13,
                               1e-10, 80.0, p(out), 13))
        torch.cuda.synchronize()
    for _ in range(3):
        go()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        go()
        ms.append(1e3 * (time.perf_counter() - t0))
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    tiles = (F + 15) // 16
    floor_ms = 1e3 * -(-tiles // cus) * wave_mfmas(L) * MFMA_CYCLES / (CLOCK_GHZ * 1e9)
    r = {"frames": F, "ms_per_call": spread(ms), "ns_per_frame": 1e6 * statistics.median(ms) / F, "cus": cus, "tiles": tiles,
         "mfma_per_wave_per_tile": wave_mfmas(L), "floor_ms": floor_ms, "ratio_to_floor": statistics.median(ms) / floor_ms,
         "checksum": float(out.sum().item())}
    print(json.dumps({"kernel": r}))


def step_encode(a):
    import torch

    from hmm_training_amd.frontend import encode_recordings
    n_sig = max(a.frames // 200, 1)
    per = 199 * HOP + L  # 32,160 samples: 200 full frames and, by the reference's rule, a remainder frame of 160
    base = make_signal(per * min(n_sig, 50)).reshape(-1, per)
    signals = [base[i % len(base)] for i in range(n_sig)]
    rng = np.random.default_rng(1)
    codebook = rng.normal(size=(256, 13)) * 20.0
    sym = encode_recordings(signals[:2], codebook)  # warm: library, tables, allocator
    assert len(sym[0]) == 201
    s = []
    for _ in range(a.reps if a.frames <= 100000 else min(a.reps, 3)):
        t0 = time.perf_counter()
        sym = encode_recordings(signals, codebook)
        torch.cuda.synchronize()
        s.append(time.perf_counter() - t0)
    F = sum(len(x) for x in sym)
    print(json.dumps({"encode": {"signals": n_sig, "frames": F, "seconds": spread(s),
                                 "us_per_frame": 1e6 * statistics.median(s) / F}}))


def step_cpu(a):
    import mfcc_ref as R
    frames = [make_signal(L, seed=i) for i in range(200)]
    win, mel, dct = R.window(L), R.mel_filters(L), R.dct_matrix(13, 26)
    out = {}
    for name, kw in (("tables_prebuilt", dict(win=win, mel=mel, dct=dct)), ("as_the_reference_calls_it", {})):
        R.mfcc_rows(frames[:10], **kw)
        us = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            R.mfcc_rows(frames, **kw)
            us.append(1e6 * (time.perf_counter() - t0) / len(frames))
        out[name] = spread(us)
    print(json.dumps({"cpu_us_per_frame": out}))


STEPS = {"kernel": step_kernel, "encode": step_encode, "cpu": step_cpu}


def child(step, a, frames, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--frames",
           str(frames), "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"step {step} failed ({r.returncode}): nothing more is run")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4200,2000000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mfcc", "bench_mfcc.json"))
    ap.add_argument("--step", choices=sorted(STEPS), default=None)
    ap.add_argument("--frames", type=int, default=4200)
    a = ap.parse_args()
    if a.step:
        return STEPS[a.step](a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out = {"frame_len": L, "hop": HOP, "method": "see tools/mfcc_bench.py", "clock_ghz": CLOCK_GHZ, "kernel": [], "encode": []}
    out.update(child("cpu", a, 0, 200))
    for F in (int(s) for s in a.sizes.split(",")):
        out["kernel"].append(child("kernel", a, F, 200)["kernel"])
        print(json.dumps(out["kernel"][-1]), flush=True)
        out["encode"].append(child("encode", a, F, 400)["encode"])
        print(json.dumps(out["encode"][-1]), flush=True)
    cpu = out["cpu_us_per_frame"]["tables_prebuilt"]["median"]
    for k in out["kernel"]:
        k["cpu_over_gpu_per_frame"] = cpu * 1e3 / k["ns_per_frame"]
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
