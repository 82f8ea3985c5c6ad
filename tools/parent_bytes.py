#!/usr/bin/env python3
"""Do two builds of the library train to the same bytes?

    python tools/parent_bytes.py PARENT.so NEW.so [--out FILE.json]

In deterministic mode (HMMBW_OPT_DETERMINISTIC: no floating-point atomics, runs are bitwise repeatable) three small
shapes (left-to-right N = 4, K = 16; dense N = 5, K = 32; wide N = 20, K = 24; 70 sequences of 1..40 symbols) are
trained for 5 iterations through hmmbw_iterate and through hmmbw_iterate_begin / _end (two in-process ranks, the
all-reduce summed here).  Each library runs in a fresh child process of its own (HMMBW_LIB) under its own time
limit; the second starts only if the first ended well.  Compared: the bytes of pi, A, B (not normalised) and of
every iteration record.  With identical kernels and an identical launch sequence they are equal; exit 1 if not.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"lr": (4, 16, "left_to_right"), "dense": (5, 32, "dense"), "wide": (20, 24, "dense")}
ITERS, R = 5, 70


def child(out):
    sys.path.insert(0, ROOT)
    import torch
    from hmm_training_amd.engine import BaumWelchEngine, shard_bounds
    from hmm_training_amd.hmm_training import default_initial_params
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.restype = ctypes.c_int
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]

    def allreduce(bufs):  # sum the ranks' device buffers in place, in rank order
        n = bufs[0][1]
        torch.cuda.synchronize()
        tot = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        tmp = torch.empty_like(tot)
        for ptr, _ in bufs:
            assert hip.hipMemcpy(ctypes.c_void_p(tmp.data_ptr()), ctypes.c_void_p(ptr), 8 * n, 3) == 0
            tot += tmp
        torch.cuda.synchronize()
        for ptr, _ in bufs:
            assert hip.hipMemcpy(ctypes.c_void_p(ptr), ctypes.c_void_p(tot.data_ptr()), 8 * n, 3) == 0
        torch.cuda.synchronize()

    def taken(e):
        _, recs = e.status(0, ITERS)
        return [np.array(recs)] + [np.asarray(x) for x in e.params(normalise=False)]

    res = {}
    for name, (N, K, topology) in SHAPES.items():
        rng = np.random.default_rng(100 + N)
        obs = [rng.integers(0, K, size=int(t)) for t in rng.integers(1, 41, size=R)]
        pi, A, B = default_initial_params(N, K)
        if topology == "dense":
            A = 0.5 * A + 0.5 * rng.dirichlet(np.ones(N), size=N)
        B = rng.dirichlet(np.full(K, 2.0), size=N)
        with BaumWelchEngine(N, K, topology=topology, deterministic=True) as e:
            e.set_observations(obs)
            e.set_params(pi, A, B)
            e.reset(0.0, ITERS)
            e.enqueue_iterations(ITERS)
            for what, x in zip(("records", "pi", "A", "B"), taken(e)):
                res[f"{name}/iterate/{what}"] = x
        engines = []
        try:
            for r, (lo, hi) in enumerate(shard_bounds([len(o) for o in obs], 2)):
                e = BaumWelchEngine(N, K, topology=topology, deterministic=True, rank=r, world_size=2)
                e.set_observations(obs[lo:hi], n_seq_global=R)
                e.set_params(pi, A, B)
                e.reset(0.0, ITERS)
                engines.append(e)
            for _ in range(ITERS):
                bufs = [e.iterate_begin() for e in engines]
                allreduce(bufs)
                for e in engines:
                    e.iterate_end()
            for r, e in enumerate(engines):
                for what, x in zip(("records", "pi", "A", "B"), taken(e)):
                    res[f"{name}/begin_end/rank{r}/{what}"] = x
        finally:
            for e in engines:
                e.close()
    np.savez(out, **res)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--out", default="parent_bytes.json")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    got = []
    for side, lib in (("parent", a.parent), ("new", a.new)):
        npz = f"{a.out}.{side}.npz"
        env = dict(os.environ, HMMBW_LIB=os.path.abspath(lib))
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), lib, lib,
                            "--child", npz], env=env)
        if r.returncode != 0:  # a fault, an abort or the time limit: nothing more is started
            sys.exit(f"{side} ({lib}): child ended with {r.returncode}")
        d = np.load(npz)
        got.append({k: d[k] for k in d.files})
        os.remove(npz)
    rows, same = [], set(got[0]) == set(got[1])
    for k in sorted(set(got[0]) & set(got[1])):
        x, y = got[0][k], got[1][k]
        eq = x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
        same = same and eq
        rows.append({"what": k, "bytes": x.nbytes, "sha256_parent": hashlib.sha256(x.tobytes()).hexdigest()[:16],
                     "sha256_new": hashlib.sha256(y.tobytes()).hexdigest()[:16], "equal": eq})
    with open(a.out, "w") as f:
        json.dump({"what": __doc__.split("\n\n")[2].replace("\n", " "), "iterations": ITERS, "all_equal": same,
                   "compared": rows}, f, indent=1)
    print(f"{len(rows)} arrays, " + ("all bytes equal" if same else "DIFFERENCES: "
                                     + ", ".join(r["what"] for r in rows if not r["equal"])))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
