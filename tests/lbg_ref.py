"""NumPy checker of the LBG tests: the contract of hmmbw_lbg_train restated (createCodeVector,
CodeVector/codevector_functions.py:442-531, MFCC variant), with the two margins that say whether a tolerance
comparison against it is meaningful.

The centroid sums may be taken in any order (np.mean here).  The distances follow the encoder's definition
(hmm_training_amd/csrc/vq_scan.hpp): d = fma(x_n, x_n, ... fma(x_1, x_1, x_0 * x_0)), s = sqrt(d), strict '<' on s,
first minimum, a NaN never wins.  NumPy has no fused multiply-add, so `fma` below builds the correctly rounded one
from error-free transformations and one rounding to odd (Boldo and Melquiond, "Emulation of a FMA and correctly
rounded sums: proved algorithms using rounding to odd", IEEE TC 2008); tests/test_lbg.py checks the distances against
oracle.vq, which is pinned to np.linalg.norm bit for bit.

Every generation makes at least one pass, as hmmbw_lbg_train does.  The reference means the same ("diff = epsilon +
100  # Ensure at least one iteration", :476) but makes none when epsilon + 100 == epsilon in fp64 (epsilon >= 2^60 or
so): a stated deviation.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List

import numpy as np

_SPLIT = 134217729.0  # 2^27 + 1


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    p = a * b
    ca, cb = _SPLIT * a, _SPLIT * b
    ah = ca - (ca - a)
    bh = cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_odd_sum(a, b):
    """a + b rounded to odd: exact sums as they are, inexact ones to the neighbour with an odd last bit."""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma(a, b, c):
    """round(a * b + c) with one rounding, elementwise (finite operands well inside the exponent range)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        uh, ul = _two_prod(a, b)
        th, tl = _two_sum(c, uh)
        r = th + _round_odd_sum(tl, ul)
        plain = a * b + c  # NaN / inf operands: the transformations above do not apply
    return np.where(np.isfinite(r) & np.isfinite(uh), r, plain)


def distances(frames, centroids, first_dim=1, dims=None, block=2048):
    """[F][K] distances over the columns [first_dim, first_dim + dims), the encoder's arithmetic."""
    frames = np.asarray(frames, np.float64)
    centroids = np.asarray(centroids, np.float64)
    dims = frames.shape[1] - first_dim if dims is None else dims
    out = np.empty((len(frames), len(centroids)))
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(0, len(frames), block):
            fb = frames[b:b + block]
            acc = None
            for d in range(first_dim, first_dim + dims):
                e = fb[:, d:d + 1] - centroids[None, :, d]
                acc = e * e if acc is None else fma(e, e, acc)
            out[b:b + block] = np.sqrt(acc)
    return out


def nearest(s):
    """(index, winning distance) per row of the distance matrix: first minimum, a NaN never wins (+inf, index 0
    when nothing does)."""
    sc = np.where(np.isnan(s), np.inf, s)
    arg = np.argmin(sc, axis=1)
    return arg, sc[np.arange(len(sc)), arg]


def assignment_margin(s, arg, centroids, first_dim, dims):
    """min over frames of (second-best - best) / second-best, where the second best is taken over the centroids
    whose scanned columns are not bit-identical to the winner's; inf when no frame has such a rival."""
    cols = np.ascontiguousarray(centroids[:, first_dim:first_dim + dims])
    _, cls = np.unique(cols.view(np.int64), axis=0, return_inverse=True)  # bit patterns: -0.0 != 0.0, NaN == NaN
    cls = cls.reshape(-1)
    sc = np.where(np.isnan(s), np.inf, s)
    best = sc[np.arange(len(sc)), arg]
    rival = np.where(cls[None, :] == cls[arg][:, None], np.inf, sc)
    second = rival.min(axis=1) if rival.shape[1] else np.full(len(sc), np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(np.isfinite(second), (second - best) / second, np.inf)
    m = np.where(np.isnan(m), 0.0, m)  # 0 / 0: two different rows at distance 0
    return float(m.min()) if len(m) else float("inf")


def scan(frames, centroids, first_dim=1, dims=None, top=4):
    """(index, winning distance, assignment margin) of one pass, without the full exact distance matrix: the rows
    are reduced to one representative per bit pattern (its first occurrence), plain (unfused, a few ulp off)
    distances pick each frame's `top` closest representatives, and only those get the encoder's exact arithmetic.
    The true winner and runner-up are among them unless `top` different rows lie within a few 1e-15 relative of the
    winner, and then the margin reported is that small.  Equal to distances / nearest / assignment_margin otherwise
    (tests/test_lbg.py)."""
    frames = np.asarray(frames, np.float64)
    centroids = np.asarray(centroids, np.float64)
    dims = frames.shape[1] - first_dim if dims is None else dims
    cols = np.ascontiguousarray(centroids[:, first_dim:first_dim + dims])
    _, first = np.unique(cols.view(np.int64), axis=0, return_index=True)
    reps = np.sort(first)  # ascending: a tie between representatives goes to the lower index
    C = cols[reps]
    X = frames[:, first_dim:first_dim + dims]
    top = min(top, len(reps))
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros((len(X), len(C)))
        for d in range(dims):
            e = X[:, d:d + 1] - C[None, :, d]
            acc += e * e
        acc = np.where(np.isnan(acc), np.inf, acc)
        cand = np.sort(np.argpartition(acc, top - 1, axis=1)[:, :top], axis=1) if top < len(reps) else \
            np.broadcast_to(np.arange(len(reps)), (len(X), len(reps)))
        ex = None
        for d in range(dims):
            e = X[:, d:d + 1] - C[cand, d]
            ex = e * e if ex is None else fma(e, e, ex)
        s = np.sqrt(ex)
    pos, best = nearest(s)
    arg = np.where(np.isinf(best), 0, reps[cand[np.arange(len(X)), pos]])
    sc = np.where(np.isnan(s), np.inf, s)
    sc[np.arange(len(X)), pos] = np.inf
    second = sc.min(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(np.isfinite(second), (second - best) / second, np.inf)
    m = np.where(np.isnan(m), 0.0, m)
    return arg, best, float(m.min())


@dataclass
class LBGCheck:
    centroids: np.ndarray
    generations: List[np.ndarray]
    assignments: np.ndarray
    passes: List[int]                 # passes made per generation 1..G
    records: np.ndarray               # REC: one entry per pass


REC = np.dtype([("generation", np.int32), ("iteration", np.int32), ("distortion", np.float64), ("diff", np.float64),
                ("assign_margin", np.float64), ("stop_margin", np.float64)])


def lbg(frames, n_centroids, epsilon=1e-3, max_iterations=100, first_dim=1, dims=None, split=(1.001, 0.999)) -> LBGCheck:
    frames = np.asarray(frames, np.float64)
    F, D = frames.shape
    if F < 1:
        raise ValueError("No raw data provided")
    dims = D - first_dim if dims is None else dims
    G = int(np.log2(n_centroids))
    with np.errstate(invalid="ignore", over="ignore"):
        cents = frames.mean(axis=0, keepdims=True)
        generations = [cents.copy()]
        recs, passes = [], []
        arg = np.zeros(F, np.int64)
        for g in range(1, G + 1):
            new = np.empty((2 * len(cents), D))
            new[0::2] = cents * split[0]
            new[1::2] = cents * split[1]
            cents = new
            prev, it = 0.0, 0
            while True:  # at least one pass (see the module docstring), then the reference's condition (:485)
                it += 1
                arg, best, margin = scan(frames, cents, first_dim, dims)
                dist = float(np.sum(best))
                new = np.zeros_like(cents)
                for k in np.unique(arg):
                    new[k] = frames[arg == k].mean(axis=0)
                cents = new
                diff = abs(prev - dist)
                prev = dist
                recs.append((g, it, dist, diff, margin, abs(diff - epsilon)))
                if not (diff > epsilon and it < max_iterations):
                    break
            passes.append(it)
            generations.append(cents.copy())
    return LBGCheck(centroids=cents, generations=generations, assignments=arg, passes=passes,
                    records=np.array(recs, dtype=REC))


def margins_ok(chk: LBGCheck, assign_min=1e-10, stop_rel=1e-9) -> bool:
    """Every pass's assignment margin >= assign_min and stop margin >= stop_rel x distortion: rounding in the
    centroid sums cannot change a decision, so a tolerance comparison with this check is meaningful."""
    r = chk.records
    return bool(np.all(r["assign_margin"] >= assign_min) and np.all(r["stop_margin"] >= stop_rel * r["distortion"]))


def near_print_boundary(x, rel=1e-9, places=6, scale=None) -> bool:
    """x sits within rel x scale (scale: |x| unless given; for a diff, the distortions it is the difference of) of
    a value where its '%.6f' rendering changes."""
    if not np.isfinite(x):
        return False
    unit = 10.0 ** places
    scaled = abs(x) * unit
    frac = scaled - np.floor(scaled)
    return abs(frac - 0.5) <= rel * (abs(x) if scale is None else scale) * unit


def printed_figures(chk: LBGCheck):
    """(value, scale) of every dist= / diff= figure createCodeVector prints: every 10th pass's pair and each
    generation's last diff."""
    r = chk.records
    out = []
    for i in np.flatnonzero(r["iteration"] % 10 == 0):
        out += [(r["distortion"][i], None), (r["diff"][i], r["distortion"][i])]
    for i in np.cumsum(chk.passes) - 1:
        out.append((r["diff"][i], r["distortion"][i]))
    return out


def prints_safely(chk: LBGCheck) -> bool:
    return not any(near_print_boundary(x, scale=sc) for x, sc in printed_figures(chk))
