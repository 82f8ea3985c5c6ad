"""LBG codebook training on the GPU (hmmbw_lbg_train, hmm_training_amd/codevector.py) against the fixtures recorded
from the reference's createCodeVector and against the NumPy checker (tests/lbg_ref.py).

The order in which the centroid sums and the distortion are added up is unspecified, so most cases compare within the
project's statistics tolerance, 1e-9 relative.  That is only meaningful where rounding cannot change a decision:
each such case first asserts FROM THE CHECKER that every pass's assignment margin is >= 1e-10 and every stop margin
>= 1e-9 x distortion (sums of <= 5,000 terms carry about 6e-13 relative error).  Measured with the checker for the
shapes and seeds below: assignment margins 9.0e-9 .. 6.7e-7, stop margins >= 3.9e-8 x distortion.

Three cases are compared bit for bit instead, because every centroid sum in them is exact in fp64 in any order: the
dyadic fixture, F = 1 and F = 5 with K = 8 (frames with coordinates that are multiples of 1/8).  The assignment
margin cannot be asserted there and need not be: a centroid that holds a single frame x splits into 1.001 x and
0.999 x, which x is equally near to within 1e-13 (measured 8.5e-14 .. 1.4e-13, whatever the seed), but with exact
sums the GPU's centroids ARE the checker's, so the same arithmetic decides.  Their distortions (a sum of square
roots) are still compared within 1e-9, with the stop margin asserted.

A frame row of NaN is the reference's own termination path: the distortion is +inf, the second pass's diff is
|inf - inf| = NaN and ends the generation (two passes per generation, as the reference itself runs it).
"""
import ctypes
import io
import json
import math
import os
from contextlib import redirect_stdout
from types import SimpleNamespace as NS

import numpy as np
import pytest

import lbg_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

RTOL = 1e-9  # the project's statistics tolerance


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    G = int(math.log2(int(z["K"])))
    return z, [z[f"gen_{g}"] for g in range(G + 1)]


def clustered(seed, F, D=13, clusters=16):
    rng = np.random.default_rng(seed)
    centres = rng.normal(scale=6.0, size=(clusters, D))
    return centres[rng.integers(0, clusters, size=F)] + rng.normal(scale=1.0, size=(F, D))


def dyadic_points(seed, F, D=13):
    return np.random.default_rng(seed).integers(-399, 400, size=(F, D)) / 8.0


def passes_of(records, G):
    return [int(np.sum(records["generation"] == g)) for g in range(1, G + 1)]


def compare(res, chk, frames, exact=False):
    """res (hmm_training_amd.codevector.LBGResult) against the checker's run."""
    G = len(chk.generations) - 1
    assert passes_of(res.records, G) == chk.passes
    assert np.array_equal(res.assignments, chk.assignments)
    assert len(res.generations) == G + 1
    atol = RTOL * float(np.max(np.abs(frames)))  # zero rows
    for a, b in zip(res.generations + [res.centroids], chk.generations + [chk.centroids]):
        assert a.shape == b.shape
        if exact:
            assert np.array_equal(a, b)
        else:
            np.testing.assert_allclose(a, b, rtol=RTOL, atol=atol)
            assert np.array_equal(np.all(a == 0.0, axis=1), np.all(b == 0.0, axis=1))  # empty rows are exactly 0.0
    assert np.array_equal(res.records["generation"], chk.records["generation"])
    assert np.array_equal(res.records["iteration"], chk.records["iteration"])
    np.testing.assert_allclose(res.records["distortion"], chk.records["distortion"], rtol=RTOL, atol=0)
    # diff is a difference of two distortions: within the tolerance of those
    assert np.all(np.abs(res.records["diff"] - chk.records["diff"]) <= 2 * RTOL * chk.records["distortion"])


def assert_margins(chk, assignment=True):
    r = chk.records
    print("assignment margin min", r["assign_margin"].min(), "stop margin / distortion min",
          np.min(r["stop_margin"] / np.maximum(r["distortion"], 1e-300)))
    if assignment:
        assert np.all(r["assign_margin"] >= 1e-10)
    assert np.all(r["stop_margin"] >= 1e-9 * r["distortion"])


# --------------------------------------------------------------------------------------------------------------
# the reference's fixtures
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def k16():
    z, gens = golden("lbg_k16")
    chk = R.lbg(z["frames"], 16, float(z["epsilon"]), int(z["max_iterations"]))
    return z, gens, chk


def test_golden_k16(k16):
    """The reference's own run, dims == 12: the scalar-load scan."""
    from hmm_training_amd.codevector import lbg_train
    z, gens, chk = k16
    assert_margins(chk)
    res = lbg_train(z["frames"], 16, int(z["max_iterations"]), float(z["epsilon"]))
    assert passes_of(res.records, 4) == z["passes"].tolist()
    assert np.array_equal(res.assignments, z["assignments"])
    np.testing.assert_allclose(res.centroids, z["centroids"], rtol=RTOL, atol=0)
    for a, b in zip(res.generations, gens):
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=0)
    compare(res, chk, z["frames"])


def test_golden_dyadic_bit_equal():
    from hmm_training_amd.codevector import lbg_train
    z, gens = golden("lbg_dyadic_k16")
    res = lbg_train(z["frames"], 16, int(z["max_iterations"]), float(z["epsilon"]))
    assert passes_of(res.records, 4) == z["passes"].tolist() == [3, 3, 3, 3]
    assert np.array_equal(res.centroids, z["centroids"])
    assert all(np.array_equal(a, b) for a, b in zip(res.generations, gens))
    assert np.array_equal(res.assignments, z["assignments"])  # the duplicates resolve to the first
    empty = np.all(z["centroids"] == 0.0, axis=1)
    assert empty.sum() == 11
    assert np.all(res.centroids[empty].view(np.int64) == 0)  # exactly +0.0
    # the split of a zero row stays zero: a row that is empty in generation g is two empty rows in g + 1
    for g in range(1, 4):
        for i in np.flatnonzero(np.all(res.generations[g] == 0.0, axis=1)):
            assert np.all(res.generations[g + 1][2 * i:2 * i + 2] == 0.0)
    assert set(res.assignments[np.isin(res.assignments, np.flatnonzero(empty))]) == set()


# --------------------------------------------------------------------------------------------------------------
# shapes
# --------------------------------------------------------------------------------------------------------------
TOLERANCE_CASES = {
    # name: (frames, K, epsilon, max_iterations, first_dim, dims)
    "F257_K2": (lambda: clustered(0, 257), 2, 1e-3, 100, 1, None),           # one generation, ragged last workgroup
    "F1000_K32_D21": (lambda: clustered(0, 1000, 21, 32), 32, 1e-3, 100, 0, 21),
    "F300_K8_D4": (lambda: clustered(0, 300, 4, 8), 8, 1e-3, 100, 0, 4),      # the LDS-staged scan
    "F3000_K256_cap8": (lambda: clustered(0, 3000, 13, 256), 256, 1e-3, 8, 1, None),  # every generation ends on the cap
    "eps_1e30": (lambda: clustered(0, 500), 16, 1e30, 100, 1, None),          # one pass per generation, back to back
}


@pytest.mark.parametrize("name", list(TOLERANCE_CASES))
def test_shapes_within_tolerance(name):
    from hmm_training_amd.codevector import lbg_train
    make, K, eps, max_it, first, dims = TOLERANCE_CASES[name]
    frames = make()
    chk = R.lbg(frames, K, eps, max_it, first, dims)
    assert_margins(chk)
    res = lbg_train(frames, K, max_it, eps, first_dim=first, dims=dims)
    compare(res, chk, frames)
    G = int(math.log2(K))
    if name == "F3000_K256_cap8":
        assert chk.passes == [8] * G
    if name == "eps_1e30":
        assert chk.passes == [1] * G and len(res.records) == G
    if name == "F257_K2":
        assert G == 1 and len(res.generations) == 2


@pytest.mark.parametrize("name", ["F257_K2", "F300_K8_D4"])
def test_small_k_wave_reduction_form(name, monkeypatch):
    """The measured alternative of the accumulate step (rows reduced per cluster across the wave before the LDS
    atomics, HMMBW_LBG_WAVE_K): the same results."""
    from hmm_training_amd.codevector import lbg_train
    monkeypatch.setenv("HMMBW_LBG_WAVE_K", "8")
    make, K, eps, max_it, first, dims = TOLERANCE_CASES[name]
    frames = make()
    chk = R.lbg(frames, K, eps, max_it, first, dims)
    assert_margins(chk)
    compare(lbg_train(frames, K, max_it, eps, first_dim=first, dims=dims), chk, frames)


@pytest.mark.parametrize("F,K", [(1, 2), (5, 8)])
def test_exact_sums_bit_equal(F, K):
    """Fewer frames than centroids: empty rows, singletons; dyadic coordinates make every sum exact."""
    from hmm_training_amd.codevector import lbg_train
    frames = dyadic_points(5, F)
    chk = R.lbg(frames, K)
    assert_margins(chk, assignment=False)
    res = lbg_train(frames, K)
    compare(res, chk, frames, exact=True)
    assert np.sum(np.all(res.centroids == 0.0, axis=1)) >= K - F


def test_device_tensor_input_and_split_factors():
    import torch

    from hmm_training_amd.codevector import lbg_train
    frames = clustered(0, 300, 4, 8)
    chk = R.lbg(frames, 4, 1e-3, 100, 0, 4, split=(1.01, 0.98))
    assert_margins(chk)
    res = lbg_train(torch.from_numpy(frames).cuda(), 4, first_dim=0, dims=4, split=(1.01, 0.98))
    compare(res, chk, frames)


# --------------------------------------------------------------------------------------------------------------
# the ABI: NaN, short record buffers, NULL outputs, status codes
# --------------------------------------------------------------------------------------------------------------
def abi_call(frames, K, eps=1e-3, max_it=100, first=1, dims=None, stride=None, want_gens=True, want_assign=True,
             records_cap=None, null_frames=False, null_centroids=False, n_frames=None):
    """hmmbw_lbg_train through ctypes; returns (status, centroids, generations, assignments, records, n_records)."""
    import torch

    from hmm_training_amd._lib import LbgRecord, lib
    F, D = frames.shape
    stride = D if stride is None else stride
    dims = D - first if dims is None else dims
    rows = max(K, 1)
    tf = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    tc = torch.full((rows, D), -7.0, dtype=torch.float64, device="cuda")
    tg = torch.full((2 * rows - 1, D), -7.0, dtype=torch.float64, device="cuda")
    ta = torch.full((max(F, 1),), -7, dtype=torch.int32, device="cuda")
    cap = 4096 if records_cap is None else records_cap
    rec = (LbgRecord * max(cap, 1))()
    n = ctypes.c_int64(-1)
    rc = lib().hmmbw_lbg_train(
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), None if null_frames else ctypes.c_void_p(tf.data_ptr()),
        F if n_frames is None else n_frames, stride, first, dims, K, eps, max_it, 1.001, 0.999,
        None if null_centroids else ctypes.c_void_p(tc.data_ptr()), ctypes.c_void_p(tg.data_ptr()) if want_gens else None,
        ctypes.c_void_p(ta.data_ptr()) if want_assign else None, ctypes.cast(rec, ctypes.c_void_p), cap, ctypes.byref(n))
    torch.cuda.synchronize()
    from hmm_training_amd.codevector import RECORD_DTYPE
    records = np.frombuffer(rec, dtype=RECORD_DTYPE, count=max(cap, 1)).copy()
    return rc, tc.cpu().numpy(), tg.cpu().numpy(), ta.cpu().numpy(), records, n.value


def test_nan_frame_row_terminates_like_the_reference():
    from hmm_training_amd.codevector import lbg_train
    from hmm_training_amd.hmm_training import vq_encode
    frames = np.random.default_rng(1).normal(size=(40, 13))
    frames[7] = np.nan
    chk = R.lbg(frames, 4)
    assert chk.passes == [2, 2]
    res = lbg_train(frames, 4)
    assert passes_of(res.records, 2) == [2, 2]
    assert np.all(np.isinf(res.records["distortion"])) and np.all(res.records["distortion"] > 0)
    assert np.isinf(res.records["diff"][0]) and np.isnan(res.records["diff"][1]) and np.isnan(res.records["diff"][3])
    assert np.array_equal(res.assignments, chk.assignments) and res.assignments[7] == 0  # a NaN distance never wins
    for a, b in zip(res.generations, chk.generations):
        assert np.array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(a, b, rtol=RTOL, atol=RTOL, equal_nan=True)
    # no later GPU call is affected
    clean = clustered(0, 257)
    compare(lbg_train(clean, 2), R.lbg(clean, 2), clean)
    cents = np.random.default_rng(2).normal(size=(8, 13))
    assert np.array_equal(vq_encode(clean, cents), R.nearest(R.distances(clean, cents))[0])


def test_short_record_buffer_and_null_outputs(k16):
    z, gens, chk = k16
    total = int(np.sum(z["passes"]))
    rc, cents, g, a, records, n = abi_call(z["frames"], 16, float(z["epsilon"]), records_cap=5, want_gens=False,
                                           want_assign=False)
    assert rc == 0 and n == total > 5  # the number made, not the number stored
    np.testing.assert_allclose(cents, z["centroids"], rtol=RTOL, atol=0)
    assert np.all(g == -7.0) and np.all(a == -7)  # NULL outputs: nothing written anywhere else
    assert np.array_equal(records["iteration"][:5], chk.records["iteration"][:5])
    np.testing.assert_allclose(records["distortion"][:5], chk.records["distortion"][:5], rtol=RTOL)
    rc, cents, g, a, records, n = abi_call(z["frames"], 16, float(z["epsilon"]), records_cap=0)
    assert rc == 0 and n == total and records["generation"][0] == 0
    np.testing.assert_allclose(g[15:], z["centroids"], rtol=RTOL, atol=0)
    assert np.array_equal(a, z["assignments"])


def test_status_codes():
    from hmm_training_amd import _lib
    fr = clustered(0, 64)
    ok = abi_call(fr, 4, max_it=2)
    assert ok[0] == 0 and ok[5] == 4
    INV, UNS = _lib.HMMBW_E_INVALID, _lib.HMMBW_E_UNSUPPORTED
    assert abi_call(fr, 4, n_frames=0)[0] == INV
    assert abi_call(fr, 4, n_frames=-1)[0] == INV
    for K in (0, 1, 3, 12, -4):
        assert abi_call(fr, K)[0] == INV, K
    assert abi_call(fr, 4, dims=0)[0] == INV
    assert abi_call(fr, 4, first=2, dims=12)[0] == INV   # first_dim + dims > frame_stride
    assert abi_call(fr, 4, first=-1, dims=12)[0] == INV
    assert abi_call(fr, 4, max_it=0)[0] == INV
    assert abi_call(fr, 4, eps=-1e-12)[0] == INV
    assert abi_call(fr, 4, eps=float("nan"))[0] == INV
    assert abi_call(fr, 4, null_frames=True)[0] == INV
    assert abi_call(fr, 4, null_centroids=True)[0] == INV
    assert abi_call(fr, 4, n_frames=0)[0] == INV and b"No raw data provided" in _lib.lib().hmmbw_last_error()
    with pytest.raises(ValueError):
        _lib.check(INV)
    # the LDS bound (lbg_plan.hpp): K = 1024 at stride 13 runs, K = 2048 does not fit, nor K = 1024 staged
    assert abi_call(fr, 2048)[0] == UNS
    assert abi_call(fr, 1024, first=0, dims=13)[0] == UNS
    wide = np.random.default_rng(0).normal(size=(8, 80))
    assert abi_call(wide, 2, first=0, dims=65)[0] == UNS
    fr = dyadic_points(7, 64)  # exact sums: bit for bit (see the module docstring)
    rc, cents, g, a, records, n = abi_call(fr, 1024, eps=1e30)
    assert rc == 0 and n == 10
    chk = R.lbg(fr, 1024, 1e30)
    assert np.array_equal(a, chk.assignments) and np.array_equal(cents, chk.centroids)
    assert np.array_equal(g[1023:], chk.centroids) and np.array_equal(g[:1], chk.generations[0])


# --------------------------------------------------------------------------------------------------------------
# the drop-in and the command line
# --------------------------------------------------------------------------------------------------------------
def test_create_code_vector_prints_the_references_lines(k16, tmp_path):
    from hmm_training_amd.codevector import createCodeVector
    from hmm_training_amd.hmm_training import get_observations
    from hmm_training_amd.io import Centroid
    z, gens, chk = k16
    assert_margins(chk)
    # no printed dist= / diff= figure sits within 1e-9 (of itself; of the distortions it is the difference of) of a
    # value where its %.6f rendering changes: the lines must then be the reference's character for character
    assert any(r["iteration"] % 10 == 0 for r in chk.records), "the fixture prints no 'Iteration 10:' line"
    assert R.prints_safely(chk)
    frames = [NS(mfcc=row.copy()) for row in z["frames"]]
    buf = io.StringIO()
    with redirect_stdout(buf):
        cents, generations = createCodeVector(frames, centroids_quantity=int(z["K"]), max_iterations=int(z["max_iterations"]),
                                              epsilon=float(z["epsilon"]))
    assert buf.getvalue().splitlines() == z["stdout"].tolist()
    assert all(isinstance(c, Centroid) for c in cents) and [c.id for c in cents] == list(range(16))
    np.testing.assert_allclose(np.stack([c.mfcc for c in cents]), z["centroids"], rtol=RTOL, atol=0)
    assert [len(g) for g in generations] == [1, 2, 4, 8, 16] and generations[3][5].id == 5
    assert [f.parent_centroid_id for f in frames] == z["assignments"].tolist()
    assert all(f.generation == 4 for f in frames)
    # the result feeds get_observations unchanged; parent_centroid_id was assigned against the centroids before the
    # last update, the encoder sees the updated ones: equal to the oracle-pinned arithmetic on those
    obs = get_observations([frames[:100], frames[100:]], cents)
    want = R.nearest(R.distances(z["frames"], np.stack([c.mfcc for c in cents])))[0]
    assert np.array_equal(np.concatenate(obs), want)

    # a quantity that is not a power of two: 2**int(log2(q)) centroids; the summary file with the reference's keys
    out = str(tmp_path / "cv")
    buf = io.StringIO()
    with redirect_stdout(buf):
        c12, g12 = createCodeVector(frames, centroids_quantity=12, max_iterations=3, epsilon=float(z["epsilon"]), output_dir=out)
    assert len(c12) == 8 and [len(g) for g in g12] == [1, 2, 4, 8]
    assert buf.getvalue().splitlines()[0] == "Creating codevector with 12 centroids..."
    summary = json.load(open(os.path.join(out, "training_summary.json")))
    assert list(summary) == ["total_frames", "max_generation", "centroid_assignments"]
    assert summary["total_frames"] == 600 and summary["max_generation"] == 3
    assert sum(summary["centroid_assignments"].values()) == 600
    assert os.listdir(out) == ["training_summary.json"]


def test_main_codebook_end_to_end(tmp_path, capsys):
    from hmm_training_amd.io import load_centroids
    from hmm_training_amd.main import _cli
    frames = clustered(3, 90, clusters=4)
    paths = []
    for i in range(2):
        p = str(tmp_path / f"rec{i}_frames.json")
        with open(p, "w") as fh:
            json.dump([{"mfcc_vector": f.tolist(), "frame_number": t} for t, f in enumerate(frames[45 * i:45 * i + 45])], fh)
        paths.append(p)
    out = str(tmp_path / "CodeVector" / "codevector.json")
    assert _cli(["codebook", "--frames", *paths, "--out", out, "--centroids", "4", "--epsilon", "0.001"]) == 0
    printed = capsys.readouterr().out
    assert "Creating codevector with 4 centroids..." in printed and "Using 90 frames for training" in printed
    assert f"Saved 4 centroids to {out}" in printed
    chk = R.lbg(frames, 4)
    assert_margins(chk)
    got = load_centroids(out)
    assert [c.id for c in got] == [0, 1, 2, 3]
    np.testing.assert_allclose(np.stack([c.mfcc for c in got]), chk.centroids, rtol=RTOL, atol=0)
