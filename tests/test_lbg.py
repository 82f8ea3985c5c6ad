"""LBG codebook training without a GPU: the NumPy checker of the GPU tests (tests/lbg_ref.py) against the fixtures
recorded from the reference's createCodeVector and against the oracle's distances; the new entry point in the
header, the binding table and the built library; the pure plan of hmmbw_lbg_train
(hmm_training_amd/csrc/lbg_plan.hpp) through a stand-alone probe built with the address and undefined-behaviour
sanitizers; the codebook file round trip; and the drop-in's argument handling that needs no device."""
import math
import os
import re
import subprocess
import types

import numpy as np
import pytest

import lbg_ref as R
from conftest import GOLDEN, ROOT
from test_lds_layout import _host_compiler


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    G = int(math.log2(int(z["K"])))
    return z, [z[f"gen_{g}"] for g in range(G + 1)]


@pytest.fixture(scope="module")
def checked():
    out = {}
    for name in ("lbg_k16", "lbg_dyadic_k16"):
        z, gens = golden(name)
        out[name] = (z, gens, R.lbg(z["frames"], int(z["K"]), float(z["epsilon"]), int(z["max_iterations"])))
    return out


# --------------------------------------------------------------------------------------------------------------
# the checker
# --------------------------------------------------------------------------------------------------------------
def test_fma_is_one_rounding():
    # against exact rational arithmetic, on operands chosen to need the third rounding step
    from fractions import Fraction
    rng = np.random.default_rng(3)
    a = rng.normal(size=4000) * 2.0 ** rng.integers(-20, 20, size=4000)
    b = rng.normal(size=4000) * 2.0 ** rng.integers(-20, 20, size=4000)
    c = -a * b * (1 + rng.integers(-3, 4, size=4000) * 2.0 ** -52) + rng.normal(size=4000) * 2.0 ** -70
    got = R.fma(a, b, c)
    for x, y, z, g in zip(a[:600], b[:600], c[:600], got[:600]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        assert g == float(exact), (x, y, z)  # float(Fraction) rounds to nearest even
    assert R.fma(3.0, 3.0, 1.0) == 10.0 and np.isnan(R.fma(np.nan, 1.0, 1.0)) and R.fma(np.inf, 1.0, 1.0) == np.inf


def test_checker_distances_are_the_encoders(oracle):
    rng = np.random.default_rng(11)
    frames = rng.normal(size=(300, 13))
    cents = rng.normal(size=(40, 13))
    cents[7] = cents[3]
    frames[5] = cents[3]
    idx, dist = oracle.vq(frames, cents, return_dist=True)
    s = R.distances(frames, cents)
    arg, best = R.nearest(s)
    assert np.array_equal(arg, idx)
    assert np.array_equal(best, dist)  # bit for bit
    assert arg[5] == 3 and best[5] == 0.0
    # every entry, not only the winners, is np.linalg.norm's value
    for f, k in [(0, 0), (17, 39), (299, 7)]:
        assert s[f, k] == np.linalg.norm(frames[f, 1:] - cents[k, 1:])
    # other column ranges: the oracle scans [1, D), so give it the range behind a dummy column
    fr21, c21 = rng.normal(size=(50, 21)), rng.normal(size=(9, 21))
    idx, dist = oracle.vq(np.hstack([np.zeros((50, 1)), fr21]), np.hstack([np.ones((9, 1)), c21]), return_dist=True)
    arg, best = R.nearest(R.distances(fr21, c21, first_dim=0, dims=21))
    assert np.array_equal(arg, idx) and np.array_equal(best, dist)


def test_checker_fast_scan_equals_the_full_matrix():
    rng = np.random.default_rng(2)
    fr, ce = rng.normal(size=(400, 13)) * 3.0, rng.normal(size=(40, 13)) * 3.0
    ce[7] = ce[3]
    ce[20:30] = 0.0
    fr[5] = ce[3]
    fr[9] = np.nan
    fr[11] = 0.5 * (ce[1] + ce[2])
    s = R.distances(fr, ce)
    arg, best = R.nearest(s)
    arg2, best2, margin2 = R.scan(fr, ce)
    assert np.array_equal(arg, arg2) and np.array_equal(best, best2)
    assert margin2 == R.assignment_margin(s, arg, ce, 1, 12)
    assert arg[9] == 0 and best[9] == np.inf
    one = R.scan(fr, ce[:1])
    assert np.all(one[0] == 0) and one[2] == np.inf


def test_checker_matches_reference_goldens(checked):
    z, gens, chk = checked["lbg_k16"]
    assert chk.passes == z["passes"].tolist()
    assert np.array_equal(chk.assignments, z["assignments"])
    np.testing.assert_allclose(chk.centroids, z["centroids"], rtol=1e-9, atol=0)
    for a, b in zip(chk.generations, gens):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=0)
    assert R.margins_ok(chk) and R.prints_safely(chk)
    assert np.all(z["frame_generation"] == 4)

    z, gens, chk = checked["lbg_dyadic_k16"]
    assert chk.passes == z["passes"].tolist() == [3, 3, 3, 3]
    assert np.array_equal(chk.assignments, z["assignments"])
    assert np.array_equal(chk.centroids, z["centroids"])  # bit-equal: every sum is exact
    assert all(np.array_equal(a, b) for a, b in zip(chk.generations, gens))
    assert int(np.sum(np.all(z["centroids"] == 0.0, axis=1))) == 11


def test_checker_margins_and_nan():
    # two frames, two centroids: the margins are what hand arithmetic gives
    frames = np.array([[0.0, 0.0], [0.0, 4.0]])
    chk = R.lbg(frames, 2, epsilon=0.5, max_iterations=10)
    # c0 = (0, 2) -> rows (0, 2.002), (0, 1.998): pass 1 distances 2.002|1.998 and 1.998|2.002
    r = chk.records[0]
    np.testing.assert_allclose(r["distortion"], 2 * 1.998, rtol=1e-12)
    np.testing.assert_allclose(r["assign_margin"], (2.002 - 1.998) / 2.002, rtol=1e-9)
    np.testing.assert_allclose(r["stop_margin"], abs(2 * 1.998 - 0.5), rtol=1e-12)
    assert chk.passes == [3] and chk.assignments.tolist() == [1, 0]
    assert chk.records[2]["distortion"] == 0.0 and chk.records[2]["diff"] == 0.0
    # bit-identical rows are not rivals: the split of a zero row stays zero, the first wins, the margin is inf
    chk = R.lbg(np.zeros((3, 2)), 2, epsilon=0.5, max_iterations=4)
    assert chk.assignments.tolist() == [0, 0, 0] and chk.records[0]["assign_margin"] == np.inf
    assert np.all(chk.centroids == 0.0)
    # the reference's own termination on a NaN frame: distortion inf, then diff = |inf - inf| = NaN ends the loop
    fr = np.random.default_rng(1).normal(size=(40, 13))
    fr[7] = np.nan
    chk = R.lbg(fr, 4)
    assert chk.passes == [2, 2] and np.all(np.isinf(chk.records["distortion"]))
    assert np.isnan(chk.records["diff"][[1, 3]]).all()
    with pytest.raises(ValueError):
        R.lbg(np.zeros((0, 13)), 2)


# --------------------------------------------------------------------------------------------------------------
# header, binding table, library, package
# --------------------------------------------------------------------------------------------------------------
def test_entry_point_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    assert "hmmbw_lbg_train" in _lib.EXPORTED
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    m = re.search(r"^int hmmbw_lbg_train\(([^;]*)\);", header, flags=re.M)
    assert m, "hmmbw_lbg_train not declared"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 17 == len(_lib.lib().hmmbw_lbg_train.argtypes)
    assert params[0] == "void *stream" and params[-1] == "int64_t *n_records"
    assert re.search(r"typedef struct \{[^}]*int32_t generation;[^}]*int32_t iteration;[^}]*double distortion;[^}]*"
                     r"double diff;[^}]*\} hmmbw_lbg_record;", header)
    import ctypes
    assert ctypes.sizeof(_lib.LbgRecord) == 24
    assert hasattr(_lib.lib(), "hmmbw_lbg_train")
    assert "hmmbw_lbg_train is a new entry point of version 5" in re.sub(r"\s+", " ", header)
    assert any(os.path.basename(src) == "lbg.hip" for src, _, _ in build.units())
    # one copy of the scan: both units include it and neither restates the fma chain
    csrc = os.path.join(ROOT, "hmm_training_amd", "csrc")
    for unit in ("vq.hip", "lbg.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "vq_scan.hpp"' in text and "__builtin_fma" not in text and "__builtin_sqrt" not in text


def test_names_resolve():
    import hmm_training_amd
    from hmm_training_amd import codevector, io
    assert hmm_training_amd.lbg_train is codevector.lbg_train
    assert hmm_training_amd.createCodeVector is codevector.createCodeVector
    assert hmm_training_amd.save_centroids is io.save_centroids
    for name in ("lbg_train", "createCodeVector", "save_centroids"):
        assert name in hmm_training_amd.__all__


# --------------------------------------------------------------------------------------------------------------
# lbg_plan.hpp under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lbg_plan") / "lbg_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "lbg_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [l.split() for l in out.splitlines()]
    return run


@pytest.mark.parametrize("K", [2, 4, 16, 256, 1024])
def test_plan_generation_offsets(probe, K):
    rows = probe("offsets", K)
    G = int(math.log2(K))
    assert rows[0] == ["G", str(G)]
    pos = 0
    for g in range(G + 1):
        assert rows[1 + g] == ["gen", str(g), str(pos), str(2 ** g)]  # c0 first, generations back to back
        pos += 2 ** g
    assert rows[-1] == ["total", str(2 * K - 1)] and pos == 2 * K - 1


def test_plan_validation(probe):
    ok = dict(F=10, stride=13, first=1, dims=12, K=16, eps=1e-3, it=100, f=1, c=1)

    def code(**kw):
        a = dict(ok, **kw)
        return int(probe("validate", a["F"], a["stride"], a["first"], a["dims"], a["K"], a["eps"], a["it"], a["f"], a["c"])[0][0])
    assert code() == 0
    assert code(F=1) == 0 and code(K=2) == 0 and code(eps=0.0) == 0 and code(eps="inf") == 0 and code(it=1) == 0
    for bad in (dict(F=0), dict(F=-3), dict(K=0), dict(K=1), dict(K=3), dict(K=48), dict(K=-16), dict(dims=0), dict(dims=-1),
                dict(first=2), dict(first=-1, dims=3), dict(stride=12), dict(it=0), dict(it=-5), dict(eps=-1e-9),
                dict(eps="nan"), dict(f=0), dict(c=0)):
        assert code(**bad) == -1, bad
    # the LDS bound: accumulators 8 (1 + K (stride + 1)) bytes + staged codebook 8 K dims for dims != 12, <= 160 KiB
    assert code(K=1024) == 0                       # 112 KiB + 8: must be admitted
    assert code(K=2048) == -3                      # 224 KiB
    assert code(K=1024, stride=18, dims=12) == 0   # 8 (1 + 1024 19) = 155,656
    assert code(K=1024, stride=19, dims=12) == -3  # 8 (1 + 1024 20) = 163,848: 8 bytes over
    assert code(K=32, stride=21, first=0, dims=21) == 0
    assert code(K=1024, stride=13, first=0, dims=13) == -3  # + staged 104 KiB
    assert code(K=4, stride=80, first=0, dims=65) == -3     # staged scan holds 64 columns
    assert code(K=4, stride=80, first=0, dims=64) == 0


def test_plan_lds_bytes(probe):
    staged, acc, lds, budget = (int(x) for x in probe("lds", 256, 13, 12)[0])
    assert (staged, acc, lds, budget) == (0, 1 + 256 * 14, 8 * (1 + 256 * 14), 160 * 1024)  # the issue's 28 KB
    staged, acc, lds, _ = (int(x) for x in probe("lds", 8, 4, 4)[0])
    assert (staged, acc, lds) == (1, 1 + 8 * 5, 8 * (1 + 8 * 5 + 8 * 4))
    assert int(probe("lds", 1024, 13, 12)[0][2]) == 114696 <= budget


def test_plan_pass_bound(probe):
    assert int(probe("passes", 8, 100)[0][0]) == 800
    assert int(probe("passes", 1, 1)[0][0]) == 1
    assert int(probe("passes", 10, 2 ** 62)[0][0]) == 2 ** 63 - 2  # saturates


def parse_run(rows):
    out = []
    for r in rows:
        out.append(dict(record=int(r[0]), stop=int(r[1]), split=int(r[2]), gen=int(r[3]), it=int(r[4]), diff=float(r[5]),
                        s_gen=int(r[7]), K=int(r[8]), done=int(r[9]), s_it=int(r[10]), n=int(r[11]), prev=float(r[12])))
    return out


def test_plan_state_machine(probe):
    # c0's pass makes no record and always splits; generation 1 stops when diff <= eps; the last generation sets done
    p = parse_run(probe("run", 0.5, 100, 2, 123.0, 10.0, 9.0, 8.8, 7.0, 7.0, 99.0))
    assert [x["record"] for x in p] == [0, 1, 1, 1, 1, 1]
    assert (p[0]["stop"], p[0]["split"], p[0]["s_gen"], p[0]["K"], p[0]["n"], p[0]["prev"]) == (1, 1, 1, 2, 0, 0.0)
    assert [x["diff"] for x in p[1:4]] == [10.0, 1.0, pytest.approx(0.2)]  # prev starts at 0
    assert [x["it"] for x in p[1:4]] == [1, 2, 3] and [x["stop"] for x in p[1:4]] == [0, 0, 1]
    assert (p[3]["split"], p[3]["s_gen"], p[3]["K"], p[3]["s_it"], p[3]["prev"], p[3]["done"]) == (1, 2, 4, 0, 0.0, 0)
    assert (p[4]["gen"], p[4]["it"], p[4]["diff"], p[4]["stop"]) == (2, 1, 7.0, 0)   # prev was reset to 0
    assert (p[5]["diff"], p[5]["stop"], p[5]["split"], p[5]["done"], p[5]["n"]) == (0.0, 1, 0, 1, 5)
    assert len(p) == 6  # nothing advances once done
    # the cap: max_iterations = 2 ends every generation on its second pass whatever the diff
    p = parse_run(probe("run", 0.0, 2, 3, 0, 5, 4, 5, 4, 5, 4))
    assert [x["stop"] for x in p] == [1, 0, 1, 0, 1, 0, 1] and p[-1]["done"] == 1 and p[-1]["K"] == 8 and p[-1]["n"] == 6
    # diff == eps stops (the loop needs diff > eps)
    p = parse_run(probe("run", 1.0, 100, 1, 0, 3.0, 2.0))
    assert p[2]["diff"] == 1.0 and p[2]["stop"] == 1 and p[2]["done"] == 1
    # a NaN diff ends the generation: inf, then |inf - inf|
    p = parse_run(probe("run", 1e-3, 100, 2, 0, "inf", "inf", "inf", "inf"))
    assert [x["stop"] for x in p] == [1, 0, 1, 0, 1] and math.isnan(p[2]["diff"]) and math.isnan(p[4]["diff"])
    assert p[1]["diff"] == math.inf and p[4]["done"] == 1
    # ... and a NaN distortion on the first pass
    p = parse_run(probe("run", 1e-3, 100, 1, 0, "nan"))
    assert p[1]["stop"] == 1 and p[1]["done"] == 1 and p[1]["it"] == 1
    # epsilon = 1e30: one pass per generation, back to back
    p = parse_run(probe("run", 1e30, 100, 4, 0, 9, 8, 7, 6))
    assert [x["stop"] for x in p] == [1] * 5 and [x["K"] for x in p] == [2, 4, 8, 16, 16] and p[-1]["n"] == 4


# --------------------------------------------------------------------------------------------------------------
# the codebook file and the drop-in's host side
# --------------------------------------------------------------------------------------------------------------
def test_save_centroids_round_trip(tmp_path):
    import json

    from hmm_training_amd.io import Centroid, load_centroids, save_centroids
    rng = np.random.default_rng(5)
    cents = [Centroid(mfcc=rng.normal(size=13) * 10.0 ** rng.integers(-8, 8), id=i) for i in range(8)]
    cents[3].mfcc[:] = 0.0
    path = str(tmp_path / "codevector.json")
    save_centroids(path, cents)
    back = load_centroids(path)
    assert [c.id for c in back] == list(range(8))
    assert all(np.array_equal(a.mfcc, b.mfcc) for a, b in zip(cents, back))  # repr round trip: bit-equal
    # the reference's format (codevector_classes.py:321-326, 548-556): a list of {"mfcc": [...], "id": k}, indent 2
    text = open(path).read()
    data = json.loads(text)
    assert list(data[0].keys()) == ["mfcc", "id"] and len(data[0]["mfcc"]) == 13
    assert text.startswith('[\n  {\n    "mfcc": [\n      ')


def test_create_code_vector_argument_handling(capsys):
    from hmm_training_amd import codevector
    with pytest.raises(ValueError, match="No raw data provided"):
        codevector.createCodeVector([])
    frames = [types.SimpleNamespace(mfcc=np.zeros(13))]
    for q in (1, 0, -4):
        with pytest.raises(ValueError):
            codevector.createCodeVector(frames, centroids_quantity=q)
    assert capsys.readouterr().out == ""  # nothing is printed before the arguments are accepted
    assert codevector.n_generations(256) == 8 and codevector.n_generations(300) == 8 and codevector.n_generations(2) == 1
    assert codevector.n_generations(3) == 1 and codevector.n_generations(1023) == 9
    import inspect
    names = list(inspect.signature(codevector.createCodeVector).parameters)
    assert names[:6] == ["raw_data_vocabulary", "centroids_quantity", "max_iterations", "epsilon", "save_updates",
                         "output_dir"]
    d = inspect.signature(codevector.createCodeVector).parameters
    assert (d["centroids_quantity"].default, d["max_iterations"].default, d["epsilon"].default, d["save_updates"].default,
            d["output_dir"].default) == (256, 100, 0.001, True, None)
