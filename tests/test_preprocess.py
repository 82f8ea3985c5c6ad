"""Signal conditioning without a GPU: the NumPy restatement of the contract (tests/preprocess_ref.py) against what the
reference's own loops gave (tests/golden/preprocess.npz); the margin condition the GPU tests rest on; the two else
branches; the pure plan of hmmbw_preprocess / hmmbw_window_overlap (hmm_training_amd/csrc/preproc_plan.hpp) through a
stand-alone probe built with the address and undefined-behaviour sanitizers; and the plumbing: header, binding table,
library, package names, command line, read_wav."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import preprocess_ref as R
from conftest import GOLDEN, ROOT
from test_lds_layout import _host_compiler


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "preprocess.npz"))


def test_golden_file_holds_the_generator_inputs(golden):
    cases = R.golden_inputs()
    assert [n for n, _ in cases] == list(golden["names"]) and len(cases) == 33
    for name, x in cases:
        assert x.dtype == np.int16 and x.shape == golden[f"{name}/input"].shape
        assert np.array_equal(x, golden[f"{name}/input"])
    assert os.path.getsize(os.path.join(GOLDEN, "preprocess.npz")) < 1 << 20
    # the shapes the cases are there for
    for name in golden["names"]:
        n = len(golden[f"{name}/input"])
        b = golden[f"{name}/batch_bounds"].tolist()
        if n < 480:
            assert len(golden[f"{name}/zcr"]) == 1 and b == [0, 0]
    assert golden["n480_middle/batch_bounds"].tolist() == [0, 160] == golden["n481_middle/batch_bounds"].tolist()
    for name in ("n1000_middle", "n4000_middle", "n4000_end"):
        b = golden[f"{name}/batch_bounds"]
        assert 0 < b[0] < b[1] < len(golden[f"{name}/input"]) - 160  # interior: not frame 0, not the last frame


# --------------------------------------------------------------------------------------------------------------
# 1. the restatement against the reference
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in R.golden_inputs()])
def test_restatement_against_golden(golden, name):
    x = golden[f"{name}/input"]
    for factors, window, bkey, okey in ((R.BATCH, False, "batch_bounds", "batch_trimmed"),
                                        (R.LIVE, True, "live_bounds", "live_windowed")):
        got = R.preprocess(x, factors, window)
        assert [got["start"], got["finish"]] == golden[f"{name}/{bkey}"].tolist()
        assert np.array_equal(got["zcr"], golden[f"{name}/zcr"])
        rel = np.abs(got["power"] - golden[f"{name}/power"]) / golden[f"{name}/power"]
        assert rel.max() <= R.POWER_RTOL
        want = golden[f"{name}/{okey}"]
        assert want.shape == (len(got["out"]), 1)
        assert np.array_equal(got["out"], want[:, 0])
    # float64 upload of the same samples is the same arithmetic
    assert np.array_equal(R.filter_signal(x.astype(np.float64)), R.filter_signal(x))


# --------------------------------------------------------------------------------------------------------------
# 2. margins: no frame's power sits on a threshold, so that a power good to 2e-13 decides as the reference decides
# --------------------------------------------------------------------------------------------------------------
def test_margin_condition(golden):
    worst = np.inf
    for name, x in R.golden_inputs() + R.special_inputs():
        _, power = R.frame_stats(R.filter_signal(x))
        for factors in (R.BATCH, R.LIVE):
            m = R.power_margin(power, factors)
            worst = min(worst, m)
            assert m > R.MARGIN, (name, factors, m)
    for name in golden["names"]:  # and on the reference's own figures
        for factors in (R.BATCH, R.LIVE):
            assert R.power_margin(golden[f"{name}/power"], factors) > R.MARGIN
    print("smallest relative distance of a power from a threshold:", worst)


# --------------------------------------------------------------------------------------------------------------
# 3. the else branches
# --------------------------------------------------------------------------------------------------------------
def test_else_branches():
    z = R.preprocess(R.zeros_input(1000), R.BATCH)
    assert z["else_branch"] and (z["start"], z["finish"]) == (0, 5 * 160) and np.all(z["power"] == 0.0)
    x = R.live_else_input()
    live = R.preprocess(x, R.LIVE, window=True)
    kf, _ = R.keep_masks(live["zcr"], live["power"], R.LIVE)
    assert live["else_branch"] and not kf.any()
    nf = R.frame_count(len(x))
    assert (live["start"], live["finish"]) == (0, nf * 160) and nf == 19
    # each test alone would keep frames: it is the conjunction that fails
    assert (live["zcr"] > 0.08 * live["zcr"].max()).any() and (live["power"] > 0.15 * live["power"].max()).any()
    assert not R.preprocess(x, R.BATCH)["else_branch"]
    # the square wave: a sign change at every step, and the half-integers of sign(0) = 0 at y[0]
    sq = R.preprocess(R.square_input(1000), R.LIVE)
    assert sq["zcr"][0] == 318.5 and sq["zcr"][1] == 319.0 and sq["zcr"].max() == sq["zcr"][-1] == 1000 - 1 - 640 - 1


def test_encode_case_margins():
    # the condition of the GPU raw -> symbols test, as tests/test_mfcc.py states it for encode_recordings: the
    # reference's own margin exceeds 1e-6 on EVERY frame
    import mfcc_ref as M
    signals, cond, rows, codebook = R.encode_case()
    assert [len(s) for s in signals] == [4000] * 3 and [len(c) for c in cond] == [800, 800, 640]
    assert [len(r) for r in rows] == [5, 5, 4] and codebook.shape == (64, 13)
    m = M.vq_margins(np.concatenate(rows), codebook)
    print("smallest margin:", m.min())
    assert m.min() > 1e-6


def test_window_restatement_shapes():
    w = R.window_table()
    assert w.shape == (320,) and abs(w[0] - 0.08) < 1e-15 and abs(w[-1] - 0.08) < 1e-15
    rng = np.random.default_rng(3)
    for m in (0, 1, 64, 65, 160, 319, 320, 321, 448, 960):
        t = rng.normal(size=m) * 1000
        out = R.window_overlap(t)
        q, part = R.window_frames(m)
        if q < 0:
            assert np.array_equal(out, t)
            continue
        if q == 0:  # the partial frame alone: it spares the last sample
            assert np.array_equal(out[:m - 1], t[:m - 1] * w[:m - 1]) and out[m - 1] == t[m - 1] and part == m - 1
    # three frames cover sample 300 of a 960-sample signal, in ascending order
    t = rng.normal(size=960)
    assert R.window_overlap(t)[300] == ((t[300] * w[300]) * w[172]) * w[44]


# --------------------------------------------------------------------------------------------------------------
# 3b. other geometries: the reference at 8, 22.05 and 44.1 kHz (tests/golden/preprocess_rates.npz), the margin
#     condition of every input the GPU shape tests use (tests/test_gpu_preprocess_shapes.py), other window tables
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_rates():
    return np.load(os.path.join(GOLDEN, "preprocess_rates.npz"))


def test_power_rtol():
    assert R.power_rtol(478) <= R.POWER_RTOL and R.power_rtol(1438) <= 3.2e-13 and R.power_rtol(1438) > 3.19e-13
    assert R.longest_frame(R.GOLDEN_LENGTHS) == 478 and R.longest_frame([1322], 882, 441) == 1321
    assert R.longest_frame([882 * 6 + 5], 882, 441) == 886 and R.longest_frame([883], 882, 441) == 882


def test_golden_rates_file_holds_the_generator_inputs(golden_rates):
    cases = R.rate_inputs()
    assert [n for n, _, _ in cases] == list(golden_rates["names"]) and len(cases) == 12
    assert [R.rate_geometry(sr) for sr in R.RATES] == [(160, 80), (441, 220), (882, 441)]
    for name, sr, x in cases:
        assert x.dtype == np.int16 and np.array_equal(x, golden_rates[f"{name}/input"])
        assert int(golden_rates[f"{name}/sample_rate"]) == sr
        win, hop = R.rate_geometry(sr)
        n, nf = len(x), len(golden_rates[f"{name}/zcr"])
        assert nf == R.frame_count(n, win, hop)
        if n < win + hop:  # one frame: bounds (0, 0)
            assert nf == 1 and golden_rates[f"{name}/batch_bounds"].tolist() == [0, 0]
            assert golden_rates[f"{name}/live_bounds"].tolist() == [0, 0]
        assert (f"{name}/live_windowed" in golden_rates) == (int(golden_rates[f"{name}/windowed_raised"]) == 0)
    assert os.path.getsize(os.path.join(GOLDEN, "preprocess_rates.npz")) < 200 << 10
    for sr in R.RATES:  # the longest possible last frame is there, and a trim that is interior
        win, hop = R.rate_geometry(sr)
        assert R.longest_frame([win + hop - 1], win, hop) == win + hop - 2
        b = golden_rates[f"sr{sr}_n{6 * win + 5}/batch_bounds"]
        assert 0 < b[0] < b[1] < 6 * win + 5 - hop


@pytest.mark.parametrize("name", [n for n, _, _ in R.rate_inputs()])
def test_restatement_against_golden_rates(golden_rates, name):
    g = lambda k: golden_rates[f"{name}/{k}"]  # noqa: E731
    x, sr = g("input"), int(g("sample_rate"))
    win, hop = R.rate_geometry(sr)
    rtol = R.power_rtol(R.longest_frame([len(x)], win, hop))
    for factors, window, bkey, okey in ((R.BATCH, False, "batch_bounds", "batch_trimmed"),
                                        (R.LIVE, True, "live_bounds", "live_windowed")):
        got = R.preprocess(x, factors, window, win=win, hop=hop)
        assert [got["start"], got["finish"]] == g(bkey).tolist()
        assert np.array_equal(got["zcr"], g("zcr"))
        rel = np.abs(got["power"] - g("power")) / g("power")
        assert rel.max() <= rtol
        if window and int(g("windowed_raised")):  # the reference has no output there; the restatement clips
            assert 192 < len(got["out"]) < 320
            continue
        want = g(okey)
        assert want.shape == (len(got["out"]), 1)
        assert np.array_equal(got["out"], want[:, 0])
    by_rate = R.preprocess(x, R.LIVE, True, sr=sr)  # the sample rate alone gives the same geometry
    assert (by_rate["start"], by_rate["finish"]) == (got["start"], got["finish"]) and np.array_equal(by_rate["power"], got["power"])


def test_margin_condition_other_geometries(golden_rates):
    """the condition of test_margin_condition for every input of tests/test_gpu_preprocess_shapes.py and of
    preprocess_rates.npz, each at its own geometry"""
    worst = {}

    def check(tag, x, win, hop):
        _, power = R.frame_stats(R.filter_signal(x), win, hop)
        for factors in (R.BATCH, R.LIVE):
            m = R.power_margin(power, factors)
            worst[tag] = min(worst.get(tag, np.inf), m)
            assert m > R.MARGIN, (tag, win, hop, factors, m)

    for name, sr, x in R.rate_inputs():
        check(f"rate {sr}", x, *R.rate_geometry(sr))
        for factors in (R.BATCH, R.LIVE):  # and on the reference's own figures
            assert R.power_margin(golden_rates[f"{name}/power"], factors) > R.MARGIN
    for win, hop in R.GEOMETRIES:
        for x in R.geometry_inputs(win, hop):
            check(f"geometry {win}/{hop}", x, win, hop)
    for n_rec in R.BATCH_SIZES:
        for x in R.batch_inputs(n_rec):
            check(f"batch of {n_rec}", x, R.WIN, R.HOP)
    for name, x in R.extreme_inputs():
        check(name, x, R.WIN, R.HOP)
    for x in R.nonfinite_batch()[::2]:  # the finite two
        check("neighbours of the non-finite recording", x, R.WIN, R.HOP)
    for tag, m in worst.items():
        print(f"smallest relative distance of a power from a threshold, {tag}: {m:.3g}")
    print("smallest of all:", min(worst.values()))


def test_tie_inputs_are_exact():
    """the exact-tie recordings do not need the margin: their powers are exact doubles in any summation order, and
    the ties are the deliberate ones; every other frame is farther than MARGIN from every threshold"""
    fr = R.tie_frames()
    assert all(f.dtype == np.int16 and len(f) == 64 and f[0] == 0 and f[-1] == 0 for f in fr.values())
    assert np.all(fr["loud"] % 2 == 0) and np.array_equal(fr["half"] * 2, fr["loud"])
    cases = R.tie_inputs()
    assert [c[0] for c in cases] == ["half_first", "half_last", "cross_first", "cross_last"]
    for name, x, at, loud in cases:
        y = R.filter_signal(x, R.TIE_COEFF)
        assert np.array_equal(y * 2, np.round(y * 2)) and (y * y).sum() * 4 < 2.0 ** 53
        zcr, power = R.frame_stats(y, R.TIE_WIN, R.TIE_WIN)
        nf = len(zcr)
        assert nf == len(x) // 64 and power[-1] == 0.0 and zcr[-1] == 0.0 and len(x) % 64 == 37
        assert power.max() == power[loud] and zcr.max() == zcr[loud] == 62.0
        # sums in another order: the same bits
        sl = R.frame_slices(len(y), R.TIE_WIN, R.TIE_WIN)
        assert all(float(np.sum((y[a:b] * y[a:b])[::-1])) / (b - a) == power[i] for i, (a, b) in enumerate(sl))
        if name.startswith("half"):
            assert power[at] == 0.25 * power[loud] and zcr[at] == zcr[loud]
        else:
            assert zcr[at] == 0.5 * zcr[loud] and 0.0 < power[at] < 1e-4 * power[loud]
        for factors in R.TIE_FACTORS:
            for pf in {factors[1], factors[3]}:
                d = np.abs(power - pf * power.max())
                on = np.flatnonzero(d == 0.0).tolist()
                if pf == 0.0:
                    assert on == [i for i in range(nf) if power[i] == 0.0] and len(on) >= 2  # the silent frames
                elif pf == 0.25:
                    assert on == ([at] if name.startswith("half") else [])
                else:
                    assert on == [loud]
                assert np.all(d[d > 0.0] > R.MARGIN * max(pf, 1e-3) * power.max())
    # what the strict comparisons decide
    want = {"half_first": [(128, 128), (0, 128), (0, 256), (0, 128)], "half_last": [(64, 64), (64, 192), (0, 320), (64, 192)],
            "cross_first": [(128, 128), (128, 128), (0, 256), (0, 128)],
            "cross_last": [(64, 64), (64, 64), (0, 320), (64, 192)]}
    for name, x, at, loud in cases:
        got = [R.preprocess(x, f, win=64, hop=64, coeff=0.5) for f in R.TIE_FACTORS]
        assert [(g["start"], g["finish"]) for g in got] == want[name]
        assert [g["else_branch"] for g in got] == [False, False, True, False]


def _window_loop(t, w, whop):
    """hamming_window's loop, element by element: q full frames in ascending order, each clipped to the signal, then
    the partial frame from q whop that spares the last sample"""
    t = [float(v) for v in t]
    m, wlen = len(t), len(w)
    q = int((m - wlen) / whop) + 1  # Python's int(): toward zero
    for i in range(q + 1):
        start = i * whop
        stop = m - 1 if i == q else min(start + wlen, m)
        for j in range(start, stop):
            t[j] = t[j] * float(w[j - start])
    return np.array(t, dtype=np.float64)


@pytest.mark.parametrize("wlen,whop", R.WINDOW_TABLES)
def test_window_restatement_other_tables(wlen, whop):
    w = R.random_table(wlen)
    rng = np.random.default_rng(5)
    lengths = R.window_lengths(wlen, whop)
    assert {0, 1, wlen, wlen + whop + 1, 3 * wlen + 1} <= set(lengths)
    if whop >= 2:  # a negative quotient that truncation and flooring round differently
        assert any(m < wlen and (m - wlen) % whop != 0 for m in lengths)
    for m in lengths:
        t = rng.normal(size=m) * 1000
        out = R.window_overlap(t, w, whop)
        assert np.array_equal(out, _window_loop(t, w, whop)), m
        q, part = R.window_frames(m, wlen, whop)
        assert q == int((m - wlen) / whop) + 1 and 0 <= part < max(wlen, 1)
        if q < 0:
            assert np.array_equal(out, t)
        elif m > 1 and not (q >= 1 and (q - 1) * whop + wlen >= m):
            assert out[m - 1] == t[m - 1]  # the last sample is spared unless a clipped full frame reaches it
    if whop > wlen:  # gaps between the frames stay as they are
        t = rng.normal(size=3 * whop + 2)
        out = R.window_overlap(t, w, whop)
        for i in range(3):
            assert np.array_equal(out[i * whop + wlen:(i + 1) * whop], t[i * whop + wlen:(i + 1) * whop])
            assert not np.array_equal(out[i * whop:i * whop + wlen], t[i * whop:i * whop + wlen])


# --------------------------------------------------------------------------------------------------------------
# 4. preproc_plan.hpp under the sanitizers (a stand-alone program: nothing is loaded into Python)
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("preproc_plan") / "preproc_plan_probe")
    src = os.path.join(ROOT, "tests", "native", "preproc_plan_probe.cpp")
    subprocess.run([_host_compiler(), "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", src, "-o", exe], check=True)

    def run(*args):
        out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout
        return [int(v) for v in out.split()]
    return run


@pytest.mark.parametrize("n", [160, 161, 319, 320, 321, 479, 480, 481, 32000])
def test_plan_frames(probe, n):
    nf, last, ok = probe("frames", n, 320, 160)
    assert nf == R.frame_count(n)
    if n == 160:
        assert (nf, ok) == (0, 0)
        return
    assert ok == 1 and nf >= 1
    a, b = R.frame_slices(n)[-1]
    assert last == b - a and last <= 320 + 160 - 2
    assert {161: (1, 160), 319: (1, 318), 320: (1, 319), 321: (1, 320), 479: (1, 478), 480: (2, 319), 481: (2, 320),
            32000: (199, 319)}[n] == (nf, last)


def test_plan_frames_other_sizes(probe):
    for n, win, hop in [(1000, 400, 100), (50, 25, 25), (64, 64, 7), (10, 4, 4), (2, 2, 1), (1, 2, 2), (100, 320, 300)]:
        nf, last, ok = probe("frames", n, win, hop)
        assert nf == R.frame_count(n, win, hop)
        assert ok == int(nf >= 1 and n >= 2)
        if ok:
            a, b = R.frame_slices(n, win, hop)[-1]
            assert last == b - a >= 1


@pytest.mark.parametrize("m", [0, 1, 64, 65, 160, 319, 320, 321, 448, 960])
def test_plan_window(probe, m):
    q, part, cover = probe("window", m, 320, 128)
    assert (q, part) == R.window_frames(m) and cover == 3
    assert {0: (-1, 0), 1: (-1, 0), 64: (-1, 0), 65: (0, 64), 160: (0, 159), 319: (1, 190), 320: (1, 191),
            321: (1, 192), 448: (2, 191), 960: (6, 191)}[m] == (q, part)


def test_plan_validation(probe):
    ok = dict(R=3, kind=1, c=0.95, win=320, hop=160, f=(-1, 0.015, -1, 0.015), p=1)

    def code(**kw):
        a = dict(ok, **kw)
        return probe("validate", a["R"], a["kind"], a["c"], a["win"], a["hop"], *a["f"], a["p"])[0]
    assert code() == 0 and code(kind=0) == 0 and code(R=0) == 0 and code(win=2, hop=1) == 0 and code(hop=320) == 0
    assert code(win=65536, hop=1) == 0
    for bad in (dict(R=-1), dict(kind=2), dict(kind=-1), dict(win=1, hop=1), dict(hop=0), dict(hop=321), dict(p=0),
                dict(c="nan"), dict(f=(0.08, "nan", 0.03, 0.1))):
        assert code(**bad) == -1, bad
    assert code(win=65537) == -3 and code(R=2 ** 31) == -3
    assert code(win=65537, hop=0) == -1  # invalid before unsupported
    off = lambda *o, win=320, hop=160: probe("offsets", win, hop, *o)[0]  # noqa: E731
    assert off(0, 161) == 0 and off(0, 161, 400, 32400) == 0
    assert off(0, 160) == -1            # no frame
    assert off(0, 500, 660) == -1       # the second recording has 160 samples
    assert off(5, 500) == -1 and off(0, 500, 400) == -1
    assert off(0, 1, win=2, hop=2) == -1 and off(0, 2, win=2, hop=2) == 0
    assert off(0, 2 ** 46 + 1) == -3
    wv = lambda *a: probe("wvalidate", *a)[0]  # noqa: E731
    assert wv(1, 320, 128, 1) == 0 and wv(0, 320, 128, 1) == 0 and wv(1, 320, 40, 1) == 0 and wv(1, 10, 100, 1) == 0
    assert wv(1, 320, 39, 1) == -3      # 9 frames cover a sample
    assert wv(1, 65537, 65537, 1) == -3
    for a in [(-1, 320, 128, 1), (1, 0, 128, 1), (1, 320, 0, 1), (1, 320, 128, 0)]:
        assert wv(*a) == -1, a


def test_plan_launch_shapes(probe):
    assert probe("shapes", 1) == [1024, 64] and probe("shapes", 33) == [1024, 31]
    assert probe("shapes", 511) == [1024, 2] and probe("shapes", 512) == [256, 2] and probe("shapes", 2000) == [256, 1]
    for r in (1, 16, 17, 100, 1023, 1024, 10 ** 6):
        block, chunks = probe("shapes", r)
        assert block in (256, 1024) and 1 <= chunks <= 64


# --------------------------------------------------------------------------------------------------------------
# 5. header, binding table, library, package, command line, files
# --------------------------------------------------------------------------------------------------------------
def test_entry_points_declared_bound_and_exported():
    from hmm_training_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "hmmbw.h")).read()
    for name, n_params, first, last in (("hmmbw_preprocess", 13, "void *stream", "double *stats_out"),
                                        ("hmmbw_window_overlap", 8, "void *stream", "int whop")):
        assert name in _lib.EXPORTED
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, flags=re.M)
        assert m, name + " not declared"
        params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        assert len(params) == n_params == len(getattr(_lib.lib(), name).argtypes)
        assert params[0] == first and params[-1] == last
    assert re.search(r"#define HMMBW_SAMPLES_F64 0\b", header) and re.search(r"#define HMMBW_SAMPLES_I16 1\b", header)
    assert (_lib.SAMPLES_F64, _lib.SAMPLES_I16) == (0, 1)
    flat = re.sub(r"\s+", " ", header)
    assert "hmmbw_preprocess and hmmbw_window_overlap are new entry points of version 5" in flat
    assert _lib.lib().hmmbw_abi_version() == 5 == _lib.ABI_VERSION
    unit = [(src, extra) for src, extra, stem in build.units() if stem == "preproc"]
    assert len(unit) == 1 and os.path.basename(unit[0][0]) == "preproc.hip" and "-ffp-contract=off" in unit[0][1]
    text = open(unit[0][0]).read()
    assert '#include "preproc_plan.hpp"' in text and "__dmul_rn" in text


def test_invalid_arguments_need_no_device():
    # validation comes before any HIP call: the codes without a GPU
    import ctypes

    from hmm_training_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64)
    p = ctypes.c_void_p(buf.ctypes.data)  # never dereferenced: every call below is refused first
    fac = np.array(R.BATCH)
    pf = ctypes.c_void_p(fac.ctypes.data)
    off160 = np.array([0, 160], dtype=np.int64)
    INV, UNS = _lib.HMMBW_E_INVALID, _lib.HMMBW_E_UNSUPPORTED
    assert L.hmmbw_preprocess(None, p, 1, p, ctypes.c_void_p(off160.ctypes.data), 1, 0.95, 320, 160, pf, p, p, None) == INV
    assert b"no frame" in L.hmmbw_last_error()
    assert L.hmmbw_preprocess(None, p, 1, p, None, 1, 0.95, 160, 320, pf, p, p, None) == INV  # hop > win
    assert L.hmmbw_preprocess(None, p, 2, p, None, 1, 0.95, 320, 160, pf, p, p, None) == INV
    assert L.hmmbw_preprocess(None, None, 1, p, None, 1, 0.95, 320, 160, pf, p, p, None) == INV
    assert L.hmmbw_preprocess(None, p, 1, p, None, 1, 0.95, 70000, 160, pf, p, p, None) == UNS
    assert L.hmmbw_preprocess(None, p, 1, p, None, 0, 0.95, 320, 160, pf, p, p, None) == 0   # nothing to do
    assert L.hmmbw_window_overlap(None, p, p, p, 1, p, 320, 39) == UNS
    assert b"ceil(wlen / whop) > 8" in L.hmmbw_last_error()
    assert L.hmmbw_window_overlap(None, p, p, p, 1, p, 0, 128) == INV
    assert L.hmmbw_window_overlap(None, p, p, None, 1, p, 320, 128) == INV
    assert L.hmmbw_window_overlap(None, p, p, p, 0, p, 320, 128) == 0


def test_names_resolve():
    import inspect

    import hmm_training_amd
    from hmm_training_amd import frontend, hmm_testing, io
    for name, home in (("preprocess_recordings", frontend), ("encode_raw_recordings", frontend),
                       ("recognise_recordings", hmm_testing), ("read_wav", io)):
        assert getattr(hmm_training_amd, name) is getattr(home, name)
        assert name in hmm_training_amd.__all__
    d = inspect.signature(frontend.preprocess_recordings).parameters
    assert list(d) == ["signals", "sample_rate", "mode", "factors", "window", "device", "return_stats"]
    assert (d["sample_rate"].default, d["mode"].default, d["window"].default, d["return_stats"].default) == \
        (16000, "batch", None, False)
    assert inspect.signature(frontend.encode_raw_recordings).parameters["mode"].default == "batch"
    assert inspect.signature(hmm_testing.recognise_recordings).parameters["mode"].default == "live"
    assert frontend.FACTORS == {"batch": R.BATCH, "live": R.LIVE} and frontend.PREEMPHASIS == R.COEFF
    assert np.array_equal(frontend.hamming_table(), R.window_table())
    assert "float32" in frontend.preprocess_recordings.__doc__  # the stated deviation
    # encode_recordings keeps its signature
    assert list(inspect.signature(frontend.encode_recordings).parameters) == \
        ["signals", "centroids", "sample_rate", "n_mels", "frame_size", "hop_size", "device"]


def test_cli_arguments():
    from hmm_training_amd import main
    for argv in (["preprocess"], ["preprocess", "--wav", "a.wav"], ["preprocess", "--out-dir", "x"], ["recognise"]):
        with pytest.raises(SystemExit):
            main._cli(argv)


def _write_wav(path, samples, rate):
    samples = np.asarray(samples, dtype="<i2")
    with wave.open(str(path), "wb") as w:
        w.setnchannels(samples.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(samples.tobytes())


def test_read_wav_round_trip(tmp_path, capsys):
    from hmm_training_amd import main
    from hmm_training_amd.io import read_wav
    rng = np.random.default_rng(0)
    mono = rng.integers(-32768, 32768, size=(1000, 1)).astype(np.int16)
    stereo = rng.integers(-32768, 32768, size=(777, 2)).astype(np.int16)
    _write_wav(tmp_path / "m.wav", mono, 16000)
    _write_wav(tmp_path / "s.wav", stereo, 44100)
    x, rate = read_wav(str(tmp_path / "m.wav"))
    assert rate == 16000 and x.dtype == np.int16 and np.array_equal(x, mono)
    x, rate = read_wav(tmp_path / "s.wav")
    assert rate == 44100 and x.shape == (777, 2) and np.array_equal(x, stereo)
    # a file that is not at 16 kHz is refused with a message, before anything touches the device
    assert main._cli(["preprocess", "--wav", str(tmp_path / "s.wav"), "--out-dir", str(tmp_path / "out")]) == 1
    assert "44100 Hz" in capsys.readouterr().out and not (tmp_path / "out").exists()
    with wave.open(str(tmp_path / "b.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(1)
        w.setframerate(16000)
        w.writeframes(bytes(100))
    with pytest.raises(ValueError):
        read_wav(str(tmp_path / "b.wav"))
