"""Signal conditioning on the GPU away from 16 kHz and small aligned batches: other frame geometries (a frame longer
than one 512-sample step of the frame sums, shorter than a wave, hop == win, win != 2 hop), 511 / 512 / 1100 recordings
(the 4-wave launch, the statistics base past one stride, one window chunk), base pointers off the allocator's
alignment (the sample-by-sample filter), other window tables (gaps, whop == wlen, wlen == 1), exact ties on all four
comparisons, full-scale and non-finite samples.

Everything is compared with the restatement (tests/preprocess_ref.py), which tests/test_preprocess.py holds against
the reference at 8, 16, 22.05 and 44.1 kHz: filtered signal, zcr, bounds, trimmed and windowed signals for equality,
power within preprocess_ref.power_rtol(longest frame) = 2 (L + 2) 2^-53.  Bounds can be compared for equality because
no frame's power lies within 1e-9 of a threshold (test_preprocess.test_margin_condition_other_geometries), except in
the tie test, whose powers are exact doubles in any summation order (test_preprocess.test_tie_inputs_are_exact).
"""
import functools
import os

import numpy as np
import pytest

import preprocess_ref as R
from conftest import GOLDEN
from preprocess_gpu import MODES, check_against, offsets_of, preprocess, window_overlap

pytestmark = pytest.mark.gpu

F64 = pytest.mark.parametrize("as_f64", [False, True], ids=["int16", "float64"])
BOTH_MODES = pytest.mark.parametrize("mode", ["batch", "live"])


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


@pytest.fixture(scope="module")
def golden_rates():
    return np.load(os.path.join(GOLDEN, "preprocess_rates.npz"))


# the restatement of every batch, computed once and never written to
@functools.lru_cache(maxsize=None)
def _geometry_case(win, hop):
    return R.geometry_inputs(win, hop)


@functools.lru_cache(maxsize=None)
def _geometry_wants(win, hop, mode):
    factors, window, _, _ = MODES[mode]
    return [R.preprocess(x, factors, window, win=win, hop=hop) for x in _geometry_case(win, hop)]


@functools.lru_cache(maxsize=None)
def _batch_case(n_rec):
    return R.batch_inputs(n_rec)


@functools.lru_cache(maxsize=None)
def _batch_wants(n_rec, mode):
    factors, window, _, _ = MODES[mode]
    return [R.preprocess(x, factors, window) for x in _batch_case(n_rec)]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------------
# a. frame geometries
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,hop", R.GEOMETRIES, ids=[f"{w}-{h}" for w, h in R.GEOMETRIES])
@BOTH_MODES
@F64
def test_frame_geometries(win, hop, mode, as_f64):
    signals, wants = _geometry_case(win, hop), _geometry_wants(win, hop, mode)
    lengths = [len(s) for s in signals]
    assert lengths == R.geometry_lengths(win, hop) and len(lengths) == 12
    assert {n % 4 for n in lengths} == {0, 1, 2, 3} and max(win - hop + 1, 2) in lengths and win + hop - 1 in lengths
    longest = R.longest_frame(lengths, win, hop)
    assert longest == (win + hop - 2 if hop > 1 else win)
    if win + hop - 2 > 512:
        assert longest > 512  # the frame sums take a second step of 512 samples
    if hop * 8 < win:
        assert max(len(w["zcr"]) for w in wants) > 1024  # and the search computes the statistics again
    rc, y, bounds, stats, offs = preprocess(signals, MODES[mode][0], as_f64, win=win, hop=hop)
    assert rc == 0
    rtol = R.power_rtol(longest)
    worst = check_against(wants, y, bounds, stats, offs, rtol=rtol, names=lengths)
    print(f"geometry ({win}, {hop}) {mode}: largest relative power difference {worst:.3g}, power_rtol {rtol:.3g}")


@pytest.mark.parametrize("sr", R.RATES)
@BOTH_MODES
@F64
def test_sample_rates_against_the_reference(golden_rates, sr, mode, as_f64):
    from hmm_training_amd.frontend import preprocess_recordings
    factors, window, bkey, okey = MODES[mode]
    win, hop = R.rate_geometry(sr)
    cases = [(name, x) for name, rate, x in R.rate_inputs() if rate == sr]
    assert [len(x) for _, x in cases] == list(R.rate_lengths(win, hop))
    signals = [x.astype(np.float64) if as_f64 else x for _, x in cases]
    wants = [R.preprocess(x, factors, window, sr=sr) for _, x in cases]
    trimmed, bounds, stats = preprocess_recordings(signals, sample_rate=sr, mode=mode, return_stats=True)
    rtol = R.power_rtol(win + hop - 2)
    worst = check_against(wants, None, bounds, np.concatenate(stats), offsets_of(signals), trimmed, rtol=rtol,
                          names=[n for n, _ in cases])
    print(f"{sr} Hz {mode}: largest relative power difference {worst:.3g}, power_rtol {rtol:.3g}")
    for r, (name, x) in enumerate(cases):  # and the reference's own output
        assert np.array_equal(golden_rates[f"{name}/input"], x)
        assert bounds[r].tolist() == golden_rates[f"{name}/{bkey}"].tolist(), name
        assert np.array_equal(stats[r][:, 0], golden_rates[f"{name}/zcr"]), name
        gp = golden_rates[f"{name}/power"]
        assert (np.abs(stats[r][:, 1] - gp) / gp).max() <= rtol, name
        if window and int(golden_rates[f"{name}/windowed_raised"]):
            continue  # the reference raised: the restatement above is the whole comparison
        assert np.array_equal(trimmed[r], golden_rates[f"{name}/{okey}"]), name


# --------------------------------------------------------------------------------------------------------------
# b. batch sizes: 511 (16 waves), 512 (4 waves, with a recording of more than 1024 frames), 1100
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rec", R.BATCH_SIZES)
def test_batch_sizes(n_rec):
    signals, wants = _batch_case(n_rec), _batch_wants(n_rec, "batch")
    assert len(signals) == n_rec and sum(len(s) for s in signals) < 2_000_000
    assert R.offset_length_residues(signals) == {(a, b) for a in range(4) for b in range(4)}
    lengths = [len(s) for i, s in enumerate(signals) if not (n_rec == 512 and i == 300)]
    assert min(lengths) >= 161 and max(lengths) <= 700
    if n_rec == 512:
        assert len(wants[300]["zcr"]) == 1061 > 1024 and not wants[300]["else_branch"]
    rc, y, bounds, stats, offs = preprocess(signals, R.BATCH, as_f64=False)
    assert rc == 0
    worst = check_against(wants, y, bounds, stats, offs)
    print(f"batch of {n_rec}: largest relative power difference {worst:.3g}, power_rtol {R.power_rtol(478):.3g}")
    # without the host's copy of the offsets, and as doubles: the same
    rc, y2, b2, st2, _ = preprocess(signals, R.BATCH, as_f64=True, host_offsets=False)
    assert rc == 0 and _same_bytes(y2, y) and _same_bytes(b2, bounds) and _same_bytes(st2, stats)


@pytest.mark.parametrize("n_rec", R.BATCH_SIZES)
def test_batch_sizes_live_with_window(n_rec):
    # hmmbw_preprocess and hmmbw_window_overlap back to back: the window over 2, 2 and 1 workgroups per recording
    from hmm_training_amd.frontend import preprocess_recordings
    signals, wants = _batch_case(n_rec), _batch_wants(n_rec, "live")
    trimmed, bounds, stats = preprocess_recordings(signals, mode="live", return_stats=True)
    assert bounds.shape == (n_rec, 2) and len(trimmed) == n_rec == len(stats)
    check_against(wants, None, bounds, np.concatenate(stats), offsets_of(signals), trimmed)
    # the inputs give the window both of its shapes often: full frames, and the partial frame alone
    assert sum(len(w["out"]) >= 320 for w in wants) > 32 and sum(0 < len(w["out"]) <= 192 for w in wants) > 32


@pytest.mark.parametrize("n_rec", [40, 1024])
def test_window_overlap_batches(n_rec):
    rng = np.random.default_rng(13 + n_rec)
    start, tail = 37, 21
    ms = rng.integers(0, 1200, size=n_rec)
    ms[:10] = (0, 1, 64, 65, 160, 319, 320, 321, 448, 960)
    recs = [rng.normal(size=int(m) + start + tail) * 1000.0 for m in ms]
    bounds = np.array([[start, start + int(m)] for m in ms], dtype=np.int64)
    offs = offsets_of(recs)
    w = R.window_table()
    rc, got = window_overlap(np.concatenate(recs), offs, bounds, w, R.WHOP)
    assert rc == 0
    for r, m in enumerate(ms):
        g, src = got[offs[r]:offs[r + 1]], recs[r]
        assert np.array_equal(g[:start], src[:start]) and np.array_equal(g[start + m:], src[start + m:]), (r, m)
        assert np.array_equal(g[start:start + m], R.window_overlap(src[start:start + m], w)), (r, m)


# --------------------------------------------------------------------------------------------------------------
# c. base pointers off the allocator's alignment: the filter goes sample by sample, and gives the same bytes
# --------------------------------------------------------------------------------------------------------------
@BOTH_MODES
@F64
def test_misaligned_base_pointers(mode, as_f64):
    signals = [x for _, x in R.golden_inputs()]
    assert len(signals) == 33
    factors, window, _, _ = MODES[mode]
    rc, y, bounds, stats, offs = preprocess(signals, factors, as_f64)
    assert rc == 0
    check_against([R.preprocess(x, factors, window) for x in signals], y, bounds, stats, offs)
    # samples + 1 is 2 bytes (int16) or 8 bytes (float64) past the alignment of the vector loads, filtered_out + 1
    # 8 bytes past that of the vector stores; preprocess() asserts that the spare elements around filtered_out keep
    # their fill
    for x_shift, y_shift in ((1, 0), (0, 1), (1, 1)):
        rc, y2, b2, st2, _ = preprocess(signals, factors, as_f64, x_shift=x_shift, y_shift=y_shift)
        assert rc == 0, (x_shift, y_shift)
        assert _same_bytes(y2, y) and _same_bytes(b2, bounds) and _same_bytes(st2, stats), (x_shift, y_shift)


# --------------------------------------------------------------------------------------------------------------
# d. window tables
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wlen,whop", R.WINDOW_TABLES, ids=[f"{a}-{b}" for a, b in R.WINDOW_TABLES])
def test_window_tables(wlen, whop):
    rng = np.random.default_rng(17)
    w = R.random_table(wlen)
    start, tail = 37, 21
    ms = R.window_lengths(wlen, whop)
    if whop > wlen:
        ms = ms + [3 * whop + 2]  # three gaps between frames
    recs = [rng.normal(size=m + start + tail) * 1000.0 for m in ms]
    bounds = [[start, start + m] for m in ms]
    offs = offsets_of(recs)
    rc, got = window_overlap(np.concatenate(recs), offs, bounds, w, whop)
    assert rc == 0
    for r, m in enumerate(ms):
        g, src = got[offs[r]:offs[r + 1]], recs[r]
        assert np.array_equal(g[:start], src[:start]) and np.array_equal(g[start + m:], src[start + m:]), m
        assert np.array_equal(g[start:start + m], R.window_overlap(src[start:start + m], w, whop)), m
        if m >= 2 and R.window_frames(m, wlen, whop)[0] >= 0:
            assert not np.array_equal(g[start:start + m], src[start:start + m]), m


# --------------------------------------------------------------------------------------------------------------
# e. exact ties: all four comparisons are strict
# --------------------------------------------------------------------------------------------------------------
@F64
def test_exact_ties(as_f64):
    cases = R.tie_inputs()
    signals = [x for _, x, _, _ in cases]
    for factors in R.TIE_FACTORS:
        wants = [R.preprocess(x, factors, win=R.TIE_WIN, hop=R.TIE_WIN, coeff=R.TIE_COEFF) for x in signals]
        rc, y, bounds, stats, offs = preprocess(signals, factors, as_f64, win=R.TIE_WIN, hop=R.TIE_WIN,
                                                coeff=R.TIE_COEFF)
        assert rc == 0
        # the power bit for bit: every sum is an exact double
        assert np.array_equal(stats[:, 1], np.concatenate([w["power"] for w in wants])), factors
        check_against(wants, y, bounds, stats, offs, rtol=0.0, names=[c[0] for c in cases])
    # what a tie decides (test_preprocess.test_tie_inputs_are_exact holds the restatement to these): with >= on the
    # first pair the tied frame 0 would be the start, with >= on the second the tied frame 3 the finish
    rc, _, bounds, _, _ = preprocess(signals, R.TIE_FACTORS[0], as_f64, win=64, hop=64, coeff=0.5)
    assert bounds.tolist() == [[128, 128], [64, 64], [128, 128], [64, 64]]
    rc, _, bounds, _, _ = preprocess(signals, R.TIE_FACTORS[1], as_f64, win=64, hop=64, coeff=0.5)
    assert bounds.tolist() == [[0, 128], [64, 192], [128, 128], [64, 64]]


# --------------------------------------------------------------------------------------------------------------
# f. full-scale and non-finite samples
# --------------------------------------------------------------------------------------------------------------
@BOTH_MODES
@F64
def test_full_scale_samples(mode, as_f64):
    factors, window, _, _ = MODES[mode]
    names, signals = zip(*R.extreme_inputs())
    assert signals[0].min() == -32768 and signals[0].max() == 32767 == signals[1].min()
    wants = [R.preprocess(x, factors, window) for x in signals]
    assert wants[0]["y"][1] == 32767 + 0.95 * 32768 and wants[0]["zcr"][1] == 319.0
    rc, y, bounds, stats, offs = preprocess(signals, factors, as_f64)
    assert rc == 0
    check_against(wants, y, bounds, stats, offs, names=names)


@BOTH_MODES
def test_non_finite_samples_stay_within_their_recording(mode):
    factors, window, _, _ = MODES[mode]
    signals = R.nonfinite_batch()
    bad = signals[1][:, 0]
    assert np.isnan(bad).any() and np.isposinf(bad).any() and np.isneginf(bad).any()
    assert not np.isfinite(bad[0]) and not np.isfinite(bad[-1])
    assert all(np.isfinite(s).all() for s in signals[::2])
    rc, y, bounds, stats, offs = preprocess(signals, factors, as_f64=True)
    assert rc == 0
    nf = [R.frame_count(len(s)) for s in signals]
    assert len(stats) == sum(nf)
    rows = np.concatenate([[0], np.cumsum(nf)])
    # the neighbours: the bytes they give when they are alone, at their own rows
    for r in (0, 2):
        rc, y1, b1, st1, _ = preprocess([signals[r]], factors, as_f64=True)
        assert rc == 0
        assert _same_bytes(y[offs[r]:offs[r + 1]], y1) and _same_bytes(bounds[r:r + 1], b1)
        assert _same_bytes(stats[rows[r]:rows[r + 1]], st1)
        want = R.preprocess(signals[r], factors, window)
        check_against([want], y1, b1, st1, np.array([0, len(y1)]))
    # the recording itself: the filter is the same arithmetic, the bounds lie within it
    with np.errstate(invalid="ignore"):
        want_y = R.filter_signal(signals[1])
    mid = y[offs[1]:offs[2]]
    assert np.isnan(want_y).any() and np.array_equal(mid, want_y, equal_nan=True)
    n = len(mid)
    start, finish = bounds[1].tolist()
    assert 0 <= start and finish <= n
    # the window on those bounds touches nothing outside [start, finish) (and nothing at all if start > finish)
    rc, got = window_overlap(y, offs, bounds, R.window_table(), R.WHOP)
    assert rc == 0
    lo, hi = offs[1] + start, offs[1] + max(finish, start)
    assert _same_bytes(got[offs[1]:lo], y[offs[1]:lo]) and _same_bytes(got[hi:offs[2]], y[hi:offs[2]])
    for r in (0, 2):
        w = R.preprocess(signals[r], factors, window=True)
        a = offs[r] + w["start"]
        assert np.array_equal(got[a:a + len(w["out"])], w["out"])
        assert _same_bytes(got[offs[r]:a], y[offs[r]:a])
        assert _same_bytes(got[a + len(w["out"]):offs[r + 1]], y[a + len(w["out"]):offs[r + 1]])
