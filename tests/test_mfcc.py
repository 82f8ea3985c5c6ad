"""The MFCC front end without a GPU: the NumPy / SciPy restatement of the contract (tests/mfcc_ref.py) checked against
itself; the pure plan of hmmbw_mfcc (hmm_training_amd/csrc/mfcc_plan.hpp: frame table, validation, sizes, tables)
through a stand-alone probe built with the address and undefined-behaviour sanitizers; the new entry points in the
header, the binding table and the built library; and the package's names."""
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import mfcc_ref as R
from conftest import ROOT
from test_lds_layout import _host_compiler

TABLE_LENGTHS = [13, 14, 161, 200, 319, 320, 512]


# --------------------------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------------------------
def test_two_forms_agree_on_the_gpu_tests_inputs():
    # the figure the GPU tolerance is derived from (mfcc_ref.GPU_TOL = 100 x CPU_FORMS_DIFF); the 1000-frame case is
    # taken at its first 250 frames here to keep the long-double DFT short
    worst = 0.0
    for F, L in R.PARITY_CASES:
        frames = R.parity_inputs(F, L)[:250]
        worst = max(worst, float(np.abs(R.mfcc_rows(frames) - R.mfcc_rows(frames, form=R.mfcc_direct)).max()))
    print("largest difference between the two CPU forms:", worst)
    assert worst <= R.CPU_FORMS_DIFF
    assert R.GPU_TOL == 100 * R.CPU_FORMS_DIFF <= 1e-9


def test_silent_nan_and_scaling():
    for form in (R.mfcc, R.mfcc_direct):
        c = form(np.zeros(320))
        assert abs(c[0] + 100.0 * np.sqrt(26.0)) < 1e-12 and np.all(np.abs(c[1:]) < 1e-12)
        x = R.tone_frames(4, 320, 3)[2].copy()
        x[100] = np.nan
        assert np.array_equal(form(x), np.zeros(13))
        x[100] = -np.inf
        assert np.array_equal(form(x), np.zeros(13))
    # a loud frame times 10: every band moves by 20 dB, none sits on a floor, so only c[0] moves, by 20 sqrt(26)
    x = 100.0 * R.tone_frames(4, 320, 3)[2]
    d = R.mfcc(10.0 * x) - R.mfcc(x)
    assert abs(d[0] - 20.0 * np.sqrt(26.0)) < 1e-11 and np.all(np.abs(d[1:]) < 1e-11)
    # integer and column input are the reference's astype(float).flatten()
    xi = np.round(x).astype(np.int16)
    assert np.array_equal(R.mfcc(xi), R.mfcc(xi.astype(np.float64)))
    assert np.array_equal(R.mfcc(xi.reshape(-1, 1)), R.mfcc(xi))
    # top_db off, other settings
    assert R.mfcc(x, top_db=-1.0).shape == (13,) and R.mfcc(x, sr=8000, n_mfcc=20, n_mels=40).shape == (20,)


def test_filter_bank_shape_and_dct():
    W = R.mel_filters(320)
    assert W.dtype == np.float32 and W.shape == (26, 161) and np.all(W >= 0)
    assert np.all(W.max(axis=1) > 0)  # no empty filter at the reference's settings
    peaks = W.argmax(axis=1)
    assert np.all(np.diff(peaks) > 0)
    D = R.dct_matrix(13, 26)
    np.testing.assert_allclose(D @ D.T, np.eye(13), atol=1e-14)
    np.testing.assert_allclose(D[0], np.full(26, 1 / np.sqrt(26)), rtol=1e-15)
    x = np.random.default_rng(0).normal(size=26)
    import scipy.fft
    np.testing.assert_allclose(D @ x, scipy.fft.dct(x, type=2, norm="ortho")[:13], atol=1e-14)


def test_encode_case_margins():
    # the condition of the GPU end-to-end test: the reference's own margin exceeds 1e-6 on EVERY frame
    signals, rows, codebook = R.encode_case()
    assert [len(r) for r in rows] == [len(R.frame_table(len(s))[0]) for s in signals]
    allrows = np.concatenate(rows)
    assert len(allrows) == 54 and codebook.shape == (64, 13)
    m = R.vq_margins(allrows, codebook)
    print("smallest margin:", m.min())
    assert m.min() > 1e-6


# --------------------------------------------------------------------------------------------------------------
# mfcc_plan.hpp under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mfcc_plan") / "mfcc_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "mfcc_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [l.split() for l in out.splitlines()]
    return run


@pytest.mark.parametrize("n", [0, 12, 13, 319, 320, 332, 333, 480, 1000, 32000])
def test_plan_frame_table(probe, n):
    starts, lengths = R.frame_table(n)
    rows = probe("frames", n, 320, 160)
    assert rows[0] == [str(len(starts)), str(len(starts))]
    assert [(int(a), int(b)) for a, b in rows[1:]] == list(zip(starts, lengths))


def test_plan_frame_table_other_sizes(probe):
    for n, fs, hop in [(1000, 400, 100), (50, 25, 25), (64, 64, 7), (13, 320, 160), (400, 200, 300)]:
        starts, lengths = R.frame_table(n, fs, hop)
        rows = probe("frames", n, fs, hop)
        assert [(int(a), int(b)) for a, b in rows[1:]] == list(zip(starts, lengths)), (n, fs, hop)
    assert probe("frames", 100, 0, 160)[0] == ["0", "-1"] and probe("frames", 100, 320, 0)[0] == ["0", "-1"]


def test_plan_validation(probe):
    ok = dict(ns=1000, F=5, L=320, mels=26, mfcc=13, amin=1e-10, stride=13, p=1)

    def code(**kw):
        a = dict(ok, **kw)
        return int(probe("validate", a["ns"], a["F"], a["L"], a["mels"], a["mfcc"], a["amin"], a["stride"], a["p"])[0][0])
    assert code() == 0
    assert code(F=0) == 0 and code(F=0, ns=0) == 0 and code(L=2) == 0 and code(L=512, ns=512) == 0
    assert code(mels=64, mfcc=64, stride=64) == 0 and code(mfcc=1, mels=1) == 0 and code(stride=1000) == 0
    assert code(amin="inf") == 0
    for bad in (dict(p=0), dict(F=-1), dict(L=1), dict(L=0), dict(L=-320), dict(mels=0), dict(mfcc=0), dict(mfcc=27),
                dict(stride=12), dict(stride=0), dict(amin=0.0), dict(amin=-1e-10), dict(amin="nan"), dict(ns=-1),
                dict(ns=319), dict(ns=0)):  # the last two: no frame of 320 fits
        assert code(**bad) == -1, bad
    assert code(L=513) == -3 and code(L=513, ns=10) == -3 and code(mels=65) == -3 and code(L=100000) == -3
    assert code(L=1, mels=65) == -1  # invalid before unsupported
    # a frame that runs past the end
    inr = lambda s, L, n: int(probe("inrange", s, L, n)[0][0])  # noqa: E731
    assert inr(0, 320, 320) == 1 and inr(680, 320, 1000) == 1 and inr(681, 320, 1000) == 0
    assert inr(-1, 320, 1000) == 0 and inr(0, 320, 319) == 0 and inr(2 ** 62, 320, 1000) == 0
    # the table call
    tv = lambda *a: int(probe("tvalidate", *a)[0][0])  # noqa: E731
    assert tv(320, 16000, 26, 13, 1) == 0 and tv(2, 1, 1, 1, 1) == 0 and tv(512, 8000, 64, 64, 1) == 0
    for a in [(1, 16000, 26, 13, 1), (320, 0, 26, 13, 1), (320, "nan", 26, 13, 1), (320, -5, 26, 13, 1),
              (320, 16000, 0, 13, 1), (320, 16000, 26, 0, 1), (320, 16000, 26, 27, 1), (320, 16000, 26, 13, 0)]:
        assert tv(*a) == -1, a
    assert tv(513, 16000, 26, 13, 1) == -3 and tv(320, 16000, 65, 13, 1) == -3


@pytest.mark.parametrize("L", [2, 13, 14, 161, 200, 319, 320, 511, 512])
def test_plan_sizes(probe, L):
    rows = probe("sizes", L, 26)
    H, Hp, Kp, Hs, Ps, blocks = (int(x) for x in rows[0])
    assert H == L // 2 + 1
    assert Hp % 4 == 0 and H <= Hp < H + 4 and Kp % 16 == 0 and H <= Kp < H + 16 and blocks == Kp // 16
    assert Hs >= Hp and Hs % 4 == 2 and Ps >= Kp and Ps % 2 == 1  # the bank arguments of the header comment
    # the A-operand read of a half-wave: 16 rows x 2 consecutive columns in 32 different 8-byte banks
    assert len({(r * Hs + c) % 32 for r in range(16) for c in range(2)}) == 32
    tw, ev, od, pw, db, band, flag, total = (int(x) for x in rows[1])
    # the power spectrum takes the place of the two folded images (the longer of the two regions is reserved)
    assert tw == 0 and ev == 2 * L and od == ev + 16 * Hs and pw == ev and db == ev + max(32 * Hs, 16 * Ps)
    assert band == db + 16 * 27 and flag == band + 26 and total == flag + 8
    assert ev % 2 == 0  # the 16-byte twiddle reads start at an even double
    lds, budget = (int(x) for x in rows[2])
    assert lds == 8 * total <= budget == 160 * 1024


def test_plan_lds_budget_and_mfma_count(probe):
    assert int(probe("sizes", 512, 64)[2][0]) <= 160 * 1024  # the largest admitted shape fits
    assert int(probe("sizes", 320, 26)[2][0]) <= 160 * 1024 // 3  # three workgroups per CU at the reference's length
    # L = 320: H = 161 -> 164 = 41 steps of 4; 176 bins = 11 blocks, 3 per wave on 4 waves; real and imaginary
    assert int(probe("mfmas", 320, 4)[0][0]) == 2 * 4 * 3 * 41
    assert int(probe("mfmas", 13, 4)[0][0]) == 2 * 4 * 1 * 2
    assert int(probe("mfmas", 512, 4)[0][0]) == 2 * 4 * 5 * 65


def _tables(probe, L, sr=16000, n_mels=26, n_mfcc=13):
    out = {"mel": {}, "band": {}, "dct": {}}

    def vals(words):
        return np.array([struct.unpack("<d", bytes.fromhex(w)[::-1])[0] for w in words])
    for r in probe("tables", L, sr, n_mels, n_mfcc):
        if r[0] in ("window", "twiddle"):
            out[r[0]] = vals(r[1:])
        elif r[0] == "band":
            out["band"][int(r[1])] = (int(r[2]), int(r[3]))
        else:
            out[r[0]][int(r[1])] = vals(r[2:])
    out["mel"] = np.stack([out["mel"][m] for m in range(n_mels)])
    out["dct"] = np.stack([out["dct"][i] for i in range(n_mfcc)])
    return out


@pytest.mark.parametrize("L", TABLE_LENGTHS)
def test_plan_tables(probe, L):
    t = _tables(probe, L)
    # the filter bank: the restatement's float32 values, bit for bit
    W = R.mel_filters(L)
    assert t["mel"].shape == W.shape
    assert np.array_equal(t["mel"].astype(np.float32).view(np.uint32), W.view(np.uint32))
    assert np.array_equal(t["mel"], W.astype(np.float64))  # and held as exactly those values
    for m in range(26):
        first, count = t["band"][m]
        nz = np.flatnonzero(W[m])
        if len(nz) == 0:
            assert count == 0
        else:
            assert first == nz[0] and first + count == nz[-1] + 1
    # window, twiddles, DCT: within 2 units in the last place of the table's own scale (entries near a zero of the
    # cosine are compared absolutely: their error enters the sums at the scale of the other entries)
    ulp = 2.0 ** -52
    n = np.arange(L, dtype=np.longdouble)
    pi = np.arctan2(np.longdouble(0), np.longdouble(-1))
    assert np.abs(t["window"] - R.window(L)).max() <= 2 * ulp
    assert np.abs(t["window"] - (0.5 - 0.5 * np.cos(2 * pi * n / L)).astype(np.float64)).max() <= ulp
    tw = t["twiddle"].reshape(L, 2)
    assert np.abs(tw[:, 0] - np.cos(2 * pi * n / L).astype(np.float64)).max() <= 2 * ulp
    assert np.abs(tw[:, 1] - np.sin(2 * pi * n / L).astype(np.float64)).max() <= 2 * ulp
    assert tw[0, 0] == 1.0 and tw[0, 1] == 0.0
    D = R.dct_matrix(13, 26)
    assert np.abs(t["dct"] - D).max() <= 2 * ulp * np.abs(D).max()


def test_plan_tables_other_settings(probe):
    t = _tables(probe, 256, sr=8000, n_mels=40, n_mfcc=20)
    W = R.mel_filters(256, sr=8000, n_mels=40)
    assert np.array_equal(t["mel"].astype(np.float32).view(np.uint32), W.view(np.uint32))
    assert np.abs(t["dct"] - R.dct_matrix(20, 40)).max() <= 2 * 2.0 ** -52


def test_restatement_takes_the_library_tables(probe):
    # the optional tables of the restatement: handing it the plan's gives the same rows to rounding
    t = _tables(probe, 200)
    frames = R.tone_frames(8, 200, 5)
    a = R.mfcc_rows(frames)
    b = R.mfcc_rows(frames, win=t["window"], mel=t["mel"], dct=t["dct"])
    assert np.abs(a - b).max() <= R.GPU_TOL


# --------------------------------------------------------------------------------------------------------------
# header, binding table, library, package
# --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    for name, n_params, first, last in (("hmmbw_mfcc_tables", 8, "int frame_len", "double *dct"),
                                        ("hmmbw_mfcc", 16, "void *stream", "int64_t out_stride")):
        assert name in _lib.EXPORTED
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M)
        assert m, name + " not declared"
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert len(params) == n_params == len(getattr(_lib.lib(), name).argtypes)
        assert params[0] == first and params[-1] == last
    flat = re.sub(r"\s+", " ", header)
    assert "hmmbw_mfcc and hmmbw_mfcc_tables are new entry points of version 5" in flat
    assert _lib.lib().hmmbw_abi_version() == 5 == _lib.ABI_VERSION
    for word in ("HMMBW_E_INVALID: a null pointer, n_frames < 0, frame_len < 2", "HMMBW_E_UNSUPPORTED: frame_len > 512",
                 "n_frames == 0 returns HMMBW_OK"):
        assert word in flat
    assert any(os.path.basename(src) == "mfcc.hip" and stem == "mfcc" for src, _, stem in build.units())
    # the tables are arguments: the kernel unit computes no cosine, sine or mel point of its own
    text = open(os.path.join(ROOT, "hmm_training_amd", "csrc", "mfcc.hip")).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert '#include "mfcc_plan.hpp"' in text and not re.search(r"\b(cos|sin|sincos|cospi|sinpi|exp)\s*\(", code)


def test_tables_entry_point_on_the_host():
    # hmmbw_mfcc_tables fills HOST arrays: it runs without a device
    import ctypes

    from hmm_training_amd import _lib
    L, H = 320, 161
    w, tw, mel, dct = np.empty(L), np.empty((L, 2)), np.empty((26, H)), np.empty((13, 26))
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    assert _lib.lib().hmmbw_mfcc_tables(L, 16000.0, 26, 13, ptr(w), ptr(tw), ptr(mel), ptr(dct)) == 0
    assert np.array_equal(mel.astype(np.float32).view(np.uint32), R.mel_filters(L).view(np.uint32))
    assert np.abs(w - R.window(L)).max() <= 2 * 2.0 ** -52
    assert _lib.lib().hmmbw_mfcc_tables(1, 16000.0, 26, 13, ptr(w), ptr(tw), ptr(mel), ptr(dct)) == -1
    assert _lib.lib().hmmbw_mfcc_tables(513, 16000.0, 26, 13, ptr(w), ptr(tw), ptr(mel), ptr(dct)) == -3
    assert _lib.lib().hmmbw_mfcc_tables(L, 16000.0, 26, 13, None, ptr(tw), ptr(mel), ptr(dct)) == -1


def test_names_resolve():
    import hmm_training_amd
    from hmm_training_amd import frontend, io
    for name in ("frame_table", "mfcc_frames", "mfcc_recordings", "encode_recordings"):
        assert getattr(hmm_training_amd, name) is getattr(frontend, name)
        assert name in hmm_training_amd.__all__
    d = inspect.signature(frontend.frame_table).parameters
    assert list(d) == ["n_samples", "frame_size", "hop_size"] and (d["frame_size"].default, d["hop_size"].default) == (320, 160)
    d = inspect.signature(frontend.mfcc_frames).parameters
    assert (d["sample_rate"].default, d["n_mfcc"].default, d["n_mels"].default) == (16000, 13, 26)
    d = inspect.signature(io.load_frames).parameters
    assert d["recompute_mfcc"].default is False


@pytest.mark.parametrize("n", [0, 12, 13, 319, 320, 332, 333, 480, 1000, 32000])
def test_python_frame_table(n):
    from hmm_training_amd.frontend import frame_table
    starts, lengths = frame_table(n)
    ref = R.frame_table(n)
    assert starts.dtype == np.int64 and lengths.dtype == np.int64
    assert starts.tolist() == ref[0] and lengths.tolist() == ref[1]
    with pytest.raises(ValueError):
        frame_table(n, frame_size=0)
    with pytest.raises(ValueError):
        frame_table(n, hop_size=0)


def test_features_cli_arguments():
    from hmm_training_amd import main
    with pytest.raises(SystemExit):
        main._cli(["features"])  # needs --signals and --out-dir
