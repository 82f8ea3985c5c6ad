"""LBG codebook training on the MI355X: the step that produces ``codevector.json``.

Replaces the MFCC ``createCodeVector`` of the reference's CodeVector pipeline
(CodeVector/codevector_functions.py:442-531; three nested Python loops there) with ``hmmbw_lbg_train``
(include/hmmbw.h): every assignment pass, centroid update, stop decision and split runs on the device.

* ``lbg_train``: arrays in, arrays out;
* ``createCodeVector``: the drop-in, same signature, same printed lines, ``io.Centroid`` lists out.

Stated deviations of the drop-in:
* ``centroids_quantity < 2`` raises ValueError (the reference returns the two untrained split rows of c0);
* with ``save_updates`` and ``output_dir`` only ``training_summary.json`` is written: the updated-frames JSON and
  pickle dumps need the reference's raw-sample frame class.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .io import Centroid

RECORD_DTYPE = np.dtype([("generation", np.int32), ("iteration", np.int32), ("distortion", np.float64),
                         ("diff", np.float64)], align=True)


@dataclass
class LBGResult:
    centroids: np.ndarray          # [K, D]: the last generation
    generations: List[np.ndarray]  # [c0 (1 row), generation 1 (2 rows), ..., generation G (K rows)]
    records: np.ndarray            # RECORD_DTYPE, one per assignment pass
    assignments: np.ndarray        # [F] int64: the last pass's nearest centroid of every frame


def n_generations(centroids_quantity) -> int:
    """int(log2(q)), the reference's generation count (:465); ValueError below 2."""
    if not centroids_quantity >= 2:
        raise ValueError(f"centroids_quantity must be at least 2, got {centroids_quantity}")
    return int(np.log2(centroids_quantity))


def lbg_train(frames, n_centroids: int = 256, max_iterations: int = 100, epsilon: float = 1e-3, first_dim: int = 1,
              dims: Optional[int] = None, split: Tuple[float, float] = (1.001, 0.999),
              device: Optional[int] = None) -> LBGResult:
    """LBG over ``frames`` [F, D] (numpy array, or a torch.float64 tensor on the device): nearest centroid over the
    columns [first_dim, first_dim + dims) (dims None: to the last column), means over all D columns.
    ``n_centroids`` must be a power of two >= 2 (hmmbw_lbg_train)."""
    import torch

    from ._lib import LbgRecord, check, lib
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.float64 or frames.dim() != 2:
            raise ValueError("frames tensor must be [F, D] torch.float64")
        if not frames.is_cuda:
            frames = frames.numpy()
    if not isinstance(frames, torch.Tensor):
        frames = np.ascontiguousarray(frames, dtype=np.float64)
        if frames.ndim != 2:
            raise ValueError("frames must be [F, D]")
    F, D = int(frames.shape[0]), int(frames.shape[1])
    if F < 1:
        raise ValueError("No raw data provided")
    K = int(n_centroids)
    if dims is None:
        dims = D - first_dim
    if isinstance(frames, torch.Tensor):
        dev = frames.device
        tf = frames.contiguous()
    else:
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
        tf = None
    L = lib()
    with torch.cuda.device(dev):
        if tf is None:
            tf = torch.from_numpy(frames).to(dev)
        rows = max(K, 1)
        tc = torch.empty((rows, D), dtype=torch.float64, device=dev)
        tg = torch.empty((max(2 * rows - 1, 1), D), dtype=torch.float64, device=dev)
        ta = torch.empty(F, dtype=torch.int32, device=dev)
        G = int(math.log2(K)) if K >= 1 else 0
        cap = max(G * int(min(max(max_iterations, 0), 1 << 20)), 1)
        rec = (LbgRecord * cap)()
        n = ctypes.c_int64(0)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(L.hmmbw_lbg_train(ctypes.c_void_p(stream), ctypes.c_void_p(tf.data_ptr()), F, D, int(first_dim), int(dims),
                                K, float(epsilon), int(max_iterations), float(split[0]), float(split[1]),
                                ctypes.c_void_p(tc.data_ptr()), ctypes.c_void_p(tg.data_ptr()),
                                ctypes.c_void_p(ta.data_ptr()), ctypes.cast(rec, ctypes.c_void_p), cap, ctypes.byref(n)))
        cents = tc.cpu().numpy()
        gens = tg.cpu().numpy()
        assign = ta.cpu().numpy().astype(np.int64)
    records = np.frombuffer(rec, dtype=RECORD_DTYPE, count=min(n.value, cap)).copy()
    generations = [gens[(1 << g) - 1:(2 << g) - 1].copy() for g in range(G + 1)]
    return LBGResult(centroids=cents, generations=generations, records=records, assignments=assign)


def _print_passes(records: np.ndarray, G: int) -> None:
    """The reference's per-generation lines (:473, :512-516)."""
    for g in range(1, G + 1):
        print(f"\nGeneration {g}: Creating {2 ** g} centroids")
        rs = records[records["generation"] == g]
        for r in rs:
            if r["iteration"] % 10 == 0:
                print(f"  Iteration {r['iteration']}: dist={r['distortion']:.6f}, diff={r['diff']:.6f}")
        print(f"  Converged after {len(rs)} iterations (diff={rs[-1]['diff']:.6f})")


def _write_summary(frames: Sequence, output_dir: str) -> None:
    """training_summary.json of save_updated_training_frames (:342-380), with the lines it prints for it."""
    print(f"Saving updated training frames to {output_dir}...")
    os.makedirs(output_dir, exist_ok=True)
    summary = {"total_frames": len(frames), "max_generation": max(f.generation for f in frames),
               "centroid_assignments": {}}
    for f in frames:
        summary["centroid_assignments"][f.parent_centroid_id] = \
            summary["centroid_assignments"].get(f.parent_centroid_id, 0) + 1
    path = os.path.join(output_dir, "training_summary.json")
    with open(path, "w") as fh:
        json.dump(summary, fh, indent=2)
    print(f"  Saved training summary: {path}")
    print(f"  Total frames: {summary['total_frames']}")
    print(f"  Max generation: {summary['max_generation']}")
    print(f"  Centroids used: {len(summary['centroid_assignments'])}")


def createCodeVector(raw_data_vocabulary, centroids_quantity: int = 256, max_iterations=100, epsilon: float = 0.001,
                     save_updates: bool = True, output_dir: Optional[str] = None,
                     device: Optional[int] = None) -> Tuple[List[Centroid], List[List[Centroid]]]:
    """Drop-in for the reference's MFCC createCodeVector (:442-531): frames are objects with ``.mfcc``; returns
    (centroids, generations) as lists of io.Centroid and sets ``parent_centroid_id`` and ``generation`` on every
    frame.  A quantity that is not a power of two gives 2**int(log2(q)) centroids, as the reference does."""
    if not raw_data_vocabulary:
        raise ValueError("No raw data provided")
    G = n_generations(centroids_quantity)
    print(f"Creating codevector with {centroids_quantity} centroids...")
    print(f"Using {len(raw_data_vocabulary)} frames for training")
    print("\n" + "=" * 50)
    print("Verifying frame calculations...")  # verify_frame_calculations (:321-339) can find no issue (:330)
    print(f"  ✓ All {len(raw_data_vocabulary)} frames have proper calculations")
    print("=" * 50)
    Fm = np.stack([np.asarray(f.mfcc, dtype=np.float64).reshape(-1) for f in raw_data_vocabulary])
    res = lbg_train(Fm, n_centroids=2 ** G, max_iterations=max_iterations, epsilon=epsilon, device=device)
    _print_passes(res.records, G)
    for f, k in zip(raw_data_vocabulary, res.assignments):
        f.parent_centroid_id = int(k)
        f.generation = G
    print("\nCodevector creation complete!")
    if save_updates and output_dir:
        print("\n" + "=" * 50)
        _write_summary(raw_data_vocabulary, output_dir)
        print("=" * 50)
    generations = [[Centroid(mfcc=row.copy(), id=i) for i, row in enumerate(g)] for g in res.generations]
    return [Centroid(mfcc=row.copy(), id=i) for i, row in enumerate(res.centroids)], generations
