#!/usr/bin/env python3
"""Generate the LBG fixtures under tests/golden/ from the REFERENCE implementation.

Like make_golden.py this runs ONLY where the reference tree is mounted read-only at /root/reference.  It imports the
reference's own ``CodeVector/codevector_functions.py`` (with empty stand-ins for ``librosa`` and ``spectrum``, which
the LBG path never calls), builds ``RawDataMFCC(raw_samples=np.zeros(0), mfcc=row)`` frames and calls the MFCC
``createCodeVector`` (:442-531).  Recorded per case: the frames, K, epsilon, max_iterations, the returned centroids,
every generation, the passes each generation made (from its "Converged after" line), every frame's final
``parent_centroid_id``, the printed lines and the reference's wall time.

Seeds are searched so that the checker (tests/lbg_ref.py) finds every pass's assignment margin >= 1e-10 and stop
margin >= 1e-9 x distortion, and no printed ``%.6f`` figure within 1e-9 relative of a rounding boundary: the GPU
tests then compare against these files with a tolerance, and their stdout verbatim.

Only the resulting ``.npz`` data files travel.  Regenerate with:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_lbg.py
"""
from __future__ import annotations

import contextlib
import io
import os
import re
import sys
import time
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))  # tests/: the checker

import lbg_ref  # noqa: E402


def _import_reference():
    sys.dont_write_bytecode = True
    for name in ("librosa", "spectrum"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["spectrum"].poly2lsf = lambda *a, **k: None
    sys.modules["spectrum"].lsf2poly = lambda *a, **k: None
    sys.path.insert(0, os.path.join(REF, "CodeVector"))
    import codevector_classes  # noqa: E402
    import codevector_functions  # noqa: E402
    return codevector_functions, codevector_classes


CF, CC = _import_reference()


def run_reference(frames, K, epsilon, max_iterations):
    raw = [CC.RawDataMFCC(raw_samples=np.zeros(0), mfcc=row.copy()) for row in frames]
    buf = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(buf):
        cents, gens = CF.createCodeVector(raw, centroids_quantity=K, max_iterations=max_iterations, epsilon=epsilon,
                                          save_updates=False)
    seconds = time.perf_counter() - t0
    lines = buf.getvalue().splitlines()
    passes = [int(m.group(1)) for m in (re.match(r"  Converged after (\d+) iterations", l) for l in lines) if m]
    return dict(centroids=np.stack([c.mfcc for c in cents]), generations=[np.stack([c.mfcc for c in g]) for g in gens],
                passes=np.array(passes, np.int64), assignments=np.array([f.parent_centroid_id for f in raw], np.int64),
                generation=np.array([f.generation for f in raw], np.int64), stdout=lines, seconds=seconds)


def save(name, frames, K, epsilon, max_iterations, ref, note):
    gens = {f"gen_{g}": a for g, a in enumerate(ref["generations"])}
    np.savez_compressed(os.path.join(OUT, f"{name}.npz"), frames=frames, K=np.int64(K), epsilon=np.float64(epsilon),
                        max_iterations=np.int64(max_iterations), centroids=ref["centroids"], passes=ref["passes"],
                        assignments=ref["assignments"], frame_generation=ref["generation"],
                        stdout=np.array(ref["stdout"], dtype=str), reference_seconds=np.float64(ref["seconds"]),
                        note=np.array(note), **gens)
    print(f"[golden] {name}: F={len(frames)} K={K} passes={ref['passes'].tolist()} reference {ref['seconds']:.2f} s")


def clustered(rng, F, D=13, clusters=16, scale=0.01):
    # small coordinates keep the distortion near 20: 1e-9 of it is far below the 1e-6 the printed lines resolve
    centres = rng.normal(scale=6.0 * scale, size=(clusters, D))
    return centres[rng.integers(0, clusters, size=F)] + rng.normal(scale=scale, size=(F, D))


def dyadic(rng, F, D=13, points=5):
    pts = rng.integers(-399, 400, size=(points, D)) / 8.0  # multiples of 1/8 in (-50, 50)
    return pts[rng.integers(0, points, size=F)]


def main():
    # 1. clustered Gaussian frames, the reference's 12-dims shape; some generation runs to its 10th pass at least,
    #    so that an "Iteration 10:" line is printed.
    for seed in range(400, 480):
        frames = clustered(np.random.default_rng(seed), 600)
        chk = lbg_ref.lbg(frames, 16, 1e-5, 100)
        if lbg_ref.margins_ok(chk) and lbg_ref.prints_safely(chk) and max(chk.passes) >= 10:
            ref = run_reference(frames, 16, 1e-5, 100)
            assert ref["passes"].tolist() == chk.passes and np.array_equal(ref["assignments"], chk.assignments)
            save("lbg_k16", frames, 16, 1e-5, 100, ref, f"clustered Gaussian frames (seed {seed})")
            break
    else:
        raise RuntimeError("no seed for lbg_k16")

    # 2. dyadic frames: every centroid sum is exact in fp64 in any order, so the centroids are bit-identical whatever
    #    the summation order; 5 distinct points leave 11 of the 16 rows empty (zeros).
    for seed in range(500, 600):
        frames = dyadic(np.random.default_rng(seed), 96)
        ref = run_reference(frames, 16, 1e-3, 100)
        empty = int(np.sum(np.all(ref["centroids"] == 0.0, axis=1)))
        if empty == 11 and ref["passes"].tolist() == [3, 3, 3, 3]:
            chk = lbg_ref.lbg(frames, 16, 1e-3, 100)
            assert all(np.array_equal(a, b) for a, b in zip(chk.generations, ref["generations"])), "not bit-identical"
            save("lbg_dyadic_k16", frames, 16, 1e-3, 100, ref, f"dyadic frames from 5 points (seed {seed})")
            break
    else:
        raise RuntimeError("no seed for lbg_dyadic_k16")


if __name__ == "__main__":
    main()
