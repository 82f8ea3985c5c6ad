"""Signal conditioning on the GPU (hmmbw_preprocess, hmmbw_window_overlap, hmm_training_amd.frontend) against the NumPy
restatement of the contract (tests/preprocess_ref.py), which tests/test_preprocess.py holds against the reference's own
output (tests/golden/preprocess.npz).

The filtered signal, zcr, bounds, trimmed and windowed signals are compared for equality; power within
preprocess_ref.POWER_RTOL = 2e-13 relative (two summation orders of at most 478 non-negative terms).  Bounds can be
compared for equality because no frame's power lies within 1e-9 of a threshold (test_preprocess.test_margin_condition).
"""
import ctypes
import os

import numpy as np
import pytest

import preprocess_ref as R
from conftest import GOLDEN
from preprocess_gpu import MODES, check_against, p as _p, preprocess as _preprocess

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


@pytest.fixture(scope="module")
def cases():
    """name -> (input, {mode: restatement}) for the golden and the special inputs, computed once"""
    out = {}
    for name, x in R.golden_inputs() + R.special_inputs():
        out[name] = (x, {m: R.preprocess(x, f, w) for m, (f, w, _, _) in MODES.items()})
    return out


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "preprocess.npz"))


def _check_against(names, cases, mode, y, bounds, stats, offs, trimmed=None):
    check_against([cases[n][1][mode] for n in names], y, bounds, stats, offs, trimmed, names=names)


# --------------------------------------------------------------------------------------------------------------
# 1. the golden inputs: one ragged batch of 33, and two of them alone
# --------------------------------------------------------------------------------------------------------------
GOLDEN_NAMES = [n for n, _ in R.golden_inputs()]


@pytest.mark.parametrize("which", ["all", "n161_middle", "n481_middle"])
@pytest.mark.parametrize("mode", ["batch", "live"])
@pytest.mark.parametrize("as_f64", [False, True], ids=["int16", "float64"])
def test_golden_inputs(cases, golden, which, mode, as_f64):
    from hmm_training_amd.frontend import preprocess_recordings
    names = GOLDEN_NAMES if which == "all" else [which]
    signals = [cases[n][0] for n in names]
    factors, window, bkey, okey = MODES[mode]
    # the C entry point: filtered_out over every whole recording, bounds, statistics
    rc, y, bounds, stats, offs = _preprocess(signals, factors, as_f64)
    assert rc == 0
    _check_against(names, cases, mode, y, bounds, stats, offs)
    # the Python entry point: trimmed (and windowed) signals, and the reference's own output
    sig = [s.astype(np.float64) for s in signals] if as_f64 else signals
    trimmed, b2, st2 = preprocess_recordings(sig, mode=mode, return_stats=True)
    assert b2.dtype == np.int64 and b2.shape == (len(names), 2) and np.array_equal(b2, bounds)
    _check_against(names, cases, mode, None, b2, np.concatenate(st2), offs, trimmed)
    assert np.array_equal(np.concatenate(st2), stats)
    for r, name in enumerate(names):
        assert b2[r].tolist() == golden[f"{name}/{bkey}"].tolist()
        assert np.array_equal(trimmed[r], golden[f"{name}/{okey}"]), name
    t3, b3 = preprocess_recordings(sig, mode=mode)  # without the statistics: the same
    assert np.array_equal(b3, b2) and all(np.array_equal(a, b) for a, b in zip(t3, trimmed))


# --------------------------------------------------------------------------------------------------------------
# 2. else branches, the square wave, a recording longer than the LDS holds statistics for
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["batch", "live"])
def test_else_branches_square_wave_and_long_recording(cases, mode):
    from hmm_training_amd.frontend import preprocess_recordings
    names = ["n1000_middle", "zeros", "live_else", "n4000_end", "square", "long", "n481_end"]
    assert cases["zeros"][1]["batch"]["else_branch"] and cases["zeros"][1]["live"]["else_branch"]
    assert cases["live_else"][1]["live"]["else_branch"] and not cases["live_else"][1]["batch"]["else_branch"]
    assert len(cases["long"][1]["live"]["zcr"]) == 1061 > 1024 and not cases["long"][1]["live"]["else_branch"]
    sq = cases["square"][1]["live"]["zcr"]
    assert sq[0] == 318.5 and sq.max() == 358.0
    signals = [cases[n][0] for n in names]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in signals])]).astype(np.int64)
    trimmed, bounds, stats = preprocess_recordings(signals, mode=mode, return_stats=True)
    _check_against(names, cases, mode, None, bounds, np.concatenate(stats), offs, trimmed)
    rc, y, b2, st2, _ = _preprocess(signals, MODES[mode][0], as_f64=False, host_offsets=False)  # lengths unchecked
    assert rc == 0
    _check_against(names, cases, mode, y, b2, st2, offs)
    rc, y3, b3, _, _ = _preprocess(signals, MODES[mode][0], as_f64=True, stats=False)  # stats_out = NULL
    assert rc == 0 and np.array_equal(b3, b2) and np.array_equal(y3, y)


# --------------------------------------------------------------------------------------------------------------
# 3. hmmbw_window_overlap alone
# --------------------------------------------------------------------------------------------------------------
WINDOW_M = (0, 1, 64, 65, 160, 319, 320, 321, 448, 960)


def test_window_overlap_alone():
    import torch

    from hmm_training_amd import _lib
    rng = np.random.default_rng(11)
    start, tail = 37, 21
    recs = [rng.normal(size=m + start + tail) * 1000.0 for m in WINDOW_M]
    bounds = [[start, start + m] for m in WINDOW_M]
    # three recordings whose bounds do not lie within them: untouched
    recs += [rng.normal(size=500) for _ in range(3)]
    bounds += [[-5, 300], [100, 501], [400, 100]]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    x = np.concatenate(recs)
    w = R.window_table()
    t, toff, tw = torch.from_numpy(x).cuda(), torch.from_numpy(offs).cuda(), torch.from_numpy(w).cuda()
    tb = torch.tensor(bounds, dtype=torch.int64, device="cuda")
    rc = _lib.lib().hmmbw_window_overlap(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), _p(t), _p(toff),
                                         _p(tb), len(recs), _p(tw), 320, 128)
    torch.cuda.synchronize()
    assert rc == 0
    got = t.cpu().numpy()
    for r, m in enumerate(WINDOW_M):
        g, src = got[offs[r]:offs[r + 1]], recs[r]
        assert np.array_equal(g[:start], src[:start]) and np.array_equal(g[start + m:], src[start + m:]), m
        assert np.array_equal(g[start:start + m], R.window_overlap(src[start:start + m], w)), m
        if m > 64:
            assert not np.array_equal(g[start:start + m], src[start:start + m])
    assert np.array_equal(got[offs[len(WINDOW_M)]:], x[offs[len(WINDOW_M)]:])
    # another table and hop: 8 frames cover a sample
    w2 = rng.uniform(0.5, 1.5, size=64)
    src = rng.normal(size=700)
    t, tw = torch.from_numpy(src).cuda(), torch.from_numpy(w2).cuda()
    toff = torch.tensor([0, 700], dtype=torch.int64, device="cuda")
    tb = torch.tensor([[0, 700]], dtype=torch.int64, device="cuda")
    rc = _lib.lib().hmmbw_window_overlap(None, _p(t), _p(toff), _p(tb), 1, _p(tw), 64, 8)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(t.cpu().numpy(), R.window_overlap(src, w2, 8))


# --------------------------------------------------------------------------------------------------------------
# 4. invalid arguments: the code, and nothing launched
# --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing():
    import torch

    from hmm_training_amd import _lib
    from hmm_training_amd.frontend import preprocess_recordings
    INV, UNS = _lib.HMMBW_E_INVALID, _lib.HMMBW_E_UNSUPPORTED
    x160 = [np.arange(160, dtype=np.int16)]
    rc, y, bounds, _, _ = _preprocess(x160, R.BATCH, as_f64=False)
    assert rc == INV and np.all(y == -7.0) and np.all(bounds == -7)
    rc, y, bounds, _, _ = _preprocess([np.arange(1000, dtype=np.int16), x160[0]], R.LIVE, as_f64=True)
    assert rc == INV and np.all(y == -7.0) and np.all(bounds == -7)
    rc, y, bounds, _, _ = _preprocess([np.arange(1000, dtype=np.int16)], R.BATCH, as_f64=False, win=160, hop=320)
    assert rc == INV and np.all(y == -7.0) and np.all(bounds == -7)
    t = torch.full((1000,), 3.0, dtype=torch.float64, device="cuda")
    off = torch.tensor([0, 1000], dtype=torch.int64, device="cuda")
    b = torch.tensor([[0, 1000]], dtype=torch.int64, device="cuda")
    w = torch.full((320,), 0.5, dtype=torch.float64, device="cuda")
    assert _lib.lib().hmmbw_window_overlap(None, _p(t), _p(off), _p(b), 1, _p(w), 320, 39) == UNS
    torch.cuda.synchronize()
    assert torch.all(t == 3.0).item()
    with pytest.raises(ValueError):
        preprocess_recordings(x160)
    with pytest.raises(ValueError):
        preprocess_recordings([np.zeros(1000)], mode="offline")
    assert preprocess_recordings([])[0] == []
    # without the host's copy of the offsets a recording that has no frame gets (0, 0) and no statistics; its
    # neighbours are what they are without it
    sig = [R.golden_input(1000, "middle", 1), x160[0].reshape(-1, 1), R.golden_input(640, "middle", 2)]
    rc, y, bounds, stats, offs = _preprocess(sig, R.BATCH, as_f64=False, host_offsets=False)
    assert rc == 0 and bounds[1].tolist() == [0, 0]
    ref = [R.preprocess(sig[0], R.BATCH), R.preprocess(sig[2], R.BATCH)]
    assert bounds[0].tolist() == [ref[0]["start"], ref[0]["finish"]] and bounds[2].tolist() == [ref[1]["start"], ref[1]["finish"]]
    assert np.array_equal(y[:1000], ref[0]["y"]) and np.array_equal(y[1160:], ref[1]["y"])
    assert np.array_equal(y[1000:1160], R.filter_signal(x160[0]))
    assert np.array_equal(stats[:8, 0], np.concatenate([ref[0]["zcr"], ref[1]["zcr"]]))


# --------------------------------------------------------------------------------------------------------------
# 5. raw recording -> symbols
# --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encode_case():
    import mfcc_ref as M
    signals, cond, rows, codebook = R.encode_case()
    assert M.vq_margins(np.concatenate(rows), codebook).min() > 1e-6  # the condition (tests/test_preprocess.py)
    return signals, [R.nearest(r, codebook) for r in rows], codebook


def test_encode_raw_recordings(encode_case):
    import torch

    from hmm_training_amd.frontend import encode_raw_recordings, encode_recordings, preprocess_recordings
    from hmm_training_amd.io import Centroid
    signals, want, codebook = encode_case
    got = encode_raw_recordings(signals, codebook, mode="live")
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    cents = [Centroid(mfcc=c, id=i) for i, c in enumerate(codebook)]
    with torch.cuda.stream(torch.cuda.Stream()):
        again = encode_raw_recordings(signals, cents, mode="live")
    assert all(np.array_equal(a, b) for a, b in zip(again, got))
    # the two stages apart give the same symbols
    trimmed, _ = preprocess_recordings(signals, mode="live")
    assert all(np.array_equal(a, b) for a, b in zip(encode_recordings(trimmed, codebook), got))
    # batch mode differs (no window, other thresholds), and a recording that trims to nothing has no symbols
    other = encode_raw_recordings(signals + [R.golden_input(200, "middle", 3)], codebook)
    assert [len(o) for o in other] == [7, 6, 6, 0]  # frame_table of 1120, 960, 960 and 0 trimmed samples
    assert encode_raw_recordings([], codebook) == []


# --------------------------------------------------------------------------------------------------------------
# 6. raw recording -> ranked words
# --------------------------------------------------------------------------------------------------------------
def test_recognise_recordings(encode_case):
    from hmm_training_amd import HMMTrained
    from hmm_training_amd.frontend import encode_raw_recordings
    from hmm_training_amd.hmm_testing import recognise_recordings, score_matrix
    signals, want, codebook = encode_case
    rng = np.random.default_rng(0)

    def model(word):
        A, B = rng.random((4, 4)) + 0.1, rng.random((4, 64)) + 0.1
        return HMMTrained(states=4, symbols=64, A=A / A.sum(1, keepdims=True), B=B / B.sum(1, keepdims=True),
                          Pi=np.full(4, 0.25), word=word)
    models = [model("uno"), model("dos"), model("tres")]
    twin = models[1]
    models.append(HMMTrained(states=4, symbols=64, A=twin.A.copy(), B=twin.B.copy(), Pi=twin.Pi.copy(), word="dos2"))
    sigs = signals[:2] + [R.golden_input(200, "middle", 3)] + signals[2:]
    scores, ranking = recognise_recordings(sigs, models, codebook)
    assert scores.shape == (4, 4) and len(ranking) == 4
    obs = encode_raw_recordings(sigs, codebook, mode="live")
    assert [len(o) for o in obs] == [5, 5, 0, 4]
    live = [0, 1, 3]
    assert np.array_equal(scores[live], score_matrix([obs[r] for r in live], models))
    assert np.all(np.isfinite(scores[live])) and np.all(scores[live] < 0)
    assert np.all(scores[2] == -np.inf) and ranking[2] == ["uno", "dos", "tres", "dos2"]
    words = [m.word for m in models]
    for r in live:
        assert np.array_equal(scores[r, 1], scores[r, 3])  # the twin ties
        order = sorted(range(4), key=lambda m: scores[r, m], reverse=True)
        assert ranking[r] == [words[m] for m in order]
        assert ranking[r].index("dos") + 1 == ranking[r].index("dos2")  # and the tie keeps the models' order
        assert list(scores[r, [words.index(w) for w in ranking[r]]]) == sorted(scores[r], reverse=True)
