"""The MFCC front end on the GPU (hmmbw_mfcc, hmm_training_amd.frontend) against the NumPy / SciPy restatement of the
contract (tests/mfcc_ref.py).

Tolerance: mfcc_ref.GPU_TOL = 100 x the largest difference between the restatement's two forms (FFT and long-double
direct DFT) over these very inputs, 1.137e-13 (tests/test_mfcc.py asserts that figure), i.e. 1.137e-11 absolute, below
the project's 1e-9.
"""
import ctypes
import json
import os

import numpy as np
import pytest

import lbg_ref
import mfcc_ref as R

pytestmark = pytest.mark.gpu

TOL = R.GPU_TOL


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")


def check_rows(got, want, what=""):
    assert got.shape == want.shape and got.dtype == np.float64
    assert np.all(np.isfinite(got))
    d = float(np.abs(got - want).max()) if got.size else 0.0
    print(f"{what} largest |gpu - ref| = {d:.3e} (tolerance {TOL:.3e})")
    assert d <= TOL


@pytest.fixture(scope="module")
def ref320():
    """The 1000-frame input at L = 320 and its reference rows, computed once."""
    frames = R.parity_inputs(1000, 320)
    return frames, R.mfcc_rows(frames)


# --------------------------------------------------------------------------------------------------------------
# parity
# --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,L", R.PARITY_CASES)
def test_parity(F, L, ref320):
    from hmm_training_amd.frontend import mfcc_frames
    if (F, L) == (1000, 320):
        frames, want = ref320
    else:
        frames = R.parity_inputs(F, L)
        want = R.mfcc_rows(frames)
    check_rows(mfcc_frames(frames), want, f"F={F} L={L}")


def test_silent_nan_inf_int16_and_columns(ref320):
    from hmm_training_amd.frontend import mfcc_frames
    frames = [f.copy() for f in ref320[0][:32]]
    want = ref320[1][:32].copy()
    frames[5] = np.zeros(320)
    frames[6][17] = np.nan       # in the first half of the fold
    frames[7][300] = -np.inf     # in the mirrored half
    frames[20][0] = np.inf
    frames[21][160] = np.nan     # the unpaired middle sample
    want[5] = R.mfcc(frames[5])
    for i in (6, 7, 20, 21):
        want[i] = 0.0
    got = mfcc_frames(frames)
    check_rows(got, want, "tile with silent / NaN / Inf frames")
    for i in (6, 7, 20, 21):
        assert np.array_equal(got[i], np.zeros(13))
    assert abs(got[5, 0] + 100.0 * np.sqrt(26.0)) <= TOL and np.all(np.abs(got[5, 1:]) <= TOL)
    # the neighbours of the flagged frames are what they are without them
    clean = mfcc_frames([f for f in ref320[0][:32]])
    keep = [i for i in range(32) if i not in (5, 6, 7, 20, 21)]
    assert np.array_equal(got[keep], clean[keep])
    # int16 samples and (L, 1) columns are the reference's astype(float).flatten()
    ints = [np.round(f * (1000.0 / max(np.abs(f).max(), 1e-300))).astype(np.int16) for f in ref320[0][:20]]
    want_i = R.mfcc_rows(ints)
    check_rows(mfcc_frames(ints), want_i, "int16")
    check_rows(mfcc_frames([x.reshape(-1, 1) for x in ints]), want_i, "(L, 1)")
    assert mfcc_frames([]).shape == (0, 13)


def test_mixed_lengths_in_one_call():
    from hmm_training_amd.frontend import mfcc_frames
    frames = []
    for i, L in enumerate([320, 13, 320, 200, 14, 320, 2, 511, 200, 320]):
        frames.append(R.tone_frames(1, L, 50 + i)[0] * 100.0)
    check_rows(mfcc_frames(frames), R.mfcc_rows(frames), "mixed lengths")


# --------------------------------------------------------------------------------------------------------------
# the C ABI: out_stride, settings, status codes
# --------------------------------------------------------------------------------------------------------------
def _call(samples, starts, L, out, out_stride, n_mels=26, n_mfcc=13, sr=16000.0, amin=1e-10, top_db=80.0, n_frames=None,
          n_samples=None, mel_scale=None):
    """hmmbw_mfcc on torch tensors; returns the status."""
    import torch

    from hmm_training_amd._lib import lib
    H = L // 2 + 1 if L >= 0 else 1
    host = [np.zeros(max(L, 1)), np.zeros((max(L, 1), 2)), np.zeros((max(n_mels, 1), H)),
            np.zeros((max(n_mfcc, 1), max(n_mels, 1)))]
    if 2 <= L <= 512 and 1 <= n_mfcc <= n_mels <= 64:
        assert lib().hmmbw_mfcc_tables(L, sr, n_mels, n_mfcc, *[ctypes.c_void_p(a.ctypes.data) for a in host]) == 0
    if mel_scale is not None:
        host[2] *= np.asarray(mel_scale)[:, None]
    dev = [torch.from_numpy(a).cuda() for a in host]
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib().hmmbw_mfcc(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(samples),
                          samples.numel() if n_samples is None else n_samples, p(starts),
                          starts.numel() if n_frames is None else n_frames, L, p(dev[0]), p(dev[1]), p(dev[2]), n_mels,
                          p(dev[3]), n_mfcc, amin, top_db, p(out), out_stride)
    torch.cuda.synchronize()
    return rc


def test_out_stride_leaves_the_other_columns():
    import torch
    frames = R.parity_inputs(17, 320)
    want = R.mfcc_rows(frames)
    x = torch.from_numpy(np.concatenate(frames)).cuda()
    starts = torch.arange(17, dtype=torch.int64, device="cuda") * 320
    # stride 13 into a larger buffer: rows 3 .. 19 of a [25, 13] frame buffer
    buf = torch.full((25, 13), -7.0, dtype=torch.float64, device="cuda")
    assert _call(x, starts, 320, buf[3:], 13) == 0
    got = buf.cpu().numpy()
    check_rows(got[3:20], want, "stride 13")
    assert np.all(got[:3] == -7.0) and np.all(got[20:] == -7.0)
    # stride 16 > n_mfcc: columns 13 .. 15 stay
    buf = torch.full((17, 16), -7.0, dtype=torch.float64, device="cuda")
    assert _call(x, starts, 320, buf, 16) == 0
    got = buf.cpu().numpy()
    check_rows(np.ascontiguousarray(got[:, :13]), want, "stride 16")
    assert np.all(got[:, 13:] == -7.0)


def test_settings():
    import torch

    from hmm_training_amd.frontend import mfcc_frames
    frames = R.parity_inputs(18, 200)
    check_rows(mfcc_frames(frames, sample_rate=8000, n_mfcc=20, n_mels=40),
               R.mfcc_rows(frames, sr=8000, n_mfcc=20, n_mels=40), "n_mels 40, n_mfcc 20, sr 8000")
    check_rows(mfcc_frames(frames, n_mels=64, n_mfcc=64), R.mfcc_rows(frames, n_mels=64, n_mfcc=64), "n_mels 64")
    # the floor at 20 dB bites on tone-plus-noise frames; top_db < 0 switches it off
    frames = R.parity_inputs(18, 320)
    floor20, without = R.mfcc_rows(frames, top_db=20.0), R.mfcc_rows(frames, top_db=-1.0)
    assert np.abs(floor20 - without).max() > 1.0
    check_rows(mfcc_frames(frames, top_db=20.0), floor20, "top_db 20")
    check_rows(mfcc_frames(frames, top_db=-1.0), without, "top_db off")
    check_rows(mfcc_frames(frames, top_db=0.0), R.mfcc_rows(frames, top_db=0.0), "top_db 0")
    check_rows(mfcc_frames(frames, amin=1e-3), R.mfcc_rows(frames, amin=1e-3), "amin 1e-3")
    # ... against the default 80 dB too.  A band 80 dB under the frame's peak carries the DFT's rounding error 1e4
    # times enlarged, whoever computes it, so the range is made with the tables instead: the upper six filters
    # scaled by 1e-10 (100 dB), which keeps every band as accurate as it was.
    scale = np.ones(26)
    scale[20:] = 1e-10
    loud = [f * (1.0 / R.AMPLITUDES[i % 4]) * 1e3 for i, f in enumerate(frames)]  # all at 1e3: nothing near amin
    mel = R.mel_filters(320).astype(np.float64) * scale[:, None]
    with80, off = R.mfcc_rows(loud, mel=mel), R.mfcc_rows(loud, mel=mel, top_db=-1.0)
    assert np.abs(with80 - off).max() > 1.0
    x = torch.from_numpy(np.concatenate(loud)).cuda()
    starts = torch.arange(18, dtype=torch.int64, device="cuda") * 320
    out = torch.zeros((18, 13), dtype=torch.float64, device="cuda")
    assert _call(x, starts, 320, out, 13, mel_scale=scale) == 0
    check_rows(out.cpu().numpy(), with80, "scaled filters, top_db 80")
    assert _call(x, starts, 320, out, 13, mel_scale=scale, top_db=-0.5) == 0
    check_rows(out.cpu().numpy(), off, "scaled filters, top_db off")


def test_status_codes():
    import torch

    from hmm_training_amd import _lib
    from hmm_training_amd.frontend import mfcc_frames
    x = torch.from_numpy(np.concatenate(R.parity_inputs(4, 320))).cuda()
    starts = torch.tensor([0, 320, 640, 960], dtype=torch.int64, device="cuda")
    out = torch.full((4, 13), -7.0, dtype=torch.float64, device="cuda")
    assert _call(x, starts, 320, out, 13) == 0
    INV, UNS = _lib.HMMBW_E_INVALID, _lib.HMMBW_E_UNSUPPORTED
    assert _call(x, starts, 1, out, 13) == INV
    assert _call(x, starts, 513, out, 13) == UNS
    assert _call(x, starts, 320, out, 13, n_mels=65) == UNS
    assert _call(x, starts, 320, out, 13, n_mels=12) == INV      # n_mfcc > n_mels
    assert _call(x, starts, 320, out, 13, n_mfcc=0) == INV
    assert _call(x, starts, 320, out, 12) == INV                 # out_stride < n_mfcc
    assert _call(x, starts, 320, out, 13, amin=0.0) == INV
    assert _call(x, starts, 320, out, 13, amin=float("nan")) == INV
    assert _call(x, starts, 320, out, 13, n_frames=-1) == INV
    out.fill_(-7.0)
    past = torch.tensor([0, 320, 640, 961], dtype=torch.int64, device="cuda")
    assert _call(x, past, 320, out, 13) == INV                   # a frame past the end: nothing is written
    assert _call(x, torch.tensor([0, -1], dtype=torch.int64, device="cuda"), 320, out, 13) == INV
    assert _call(x, starts, 320, out, 13, n_samples=1279) == INV
    assert b"past n_samples" in _lib.lib().hmmbw_last_error()
    assert _call(x, starts, 320, out, 13, n_frames=0) == 0       # OK, launches nothing
    assert np.all(out.cpu().numpy() == -7.0)
    # null pointers
    L = _lib.lib()
    p = ctypes.c_void_p(x.data_ptr())
    assert L.hmmbw_mfcc(None, None, 1280, p, 4, 320, p, p, p, 26, p, 13, 1e-10, 80.0, p, 13) == INV
    assert L.hmmbw_mfcc(None, p, 1280, p, 4, 320, p, p, p, 26, p, 13, 1e-10, 80.0, None, 13) == INV
    # the Python layer raises what the status maps to
    with pytest.raises(ValueError):
        mfcc_frames([np.zeros(1)])
    with pytest.raises(ValueError):
        mfcc_frames([np.zeros(320)], n_mfcc=27)
    with pytest.raises(_lib.HMMBWError):
        mfcc_frames([np.zeros(513)])


# --------------------------------------------------------------------------------------------------------------
# recordings: frames as views, signal -> symbols, signal -> codebook
# --------------------------------------------------------------------------------------------------------------
def test_recordings_are_views_of_the_signal():
    from hmm_training_amd.frontend import frame_table, mfcc_frames, mfcc_recordings
    signals = [R.signal(1000, 1), R.signal(320, 2), R.signal(333, 3)]
    rows = mfcc_recordings(signals)
    assert [len(r) for r in rows] == [6, 2, 2]  # 5 full + 200; 1 full + 160; 1 full + 173
    slices = []
    for s in signals:
        st, ln = frame_table(len(s))
        assert (st.tolist(), ln.tolist()) == R.frame_table(len(s))
        slices += [s[a:a + n] for a, n in zip(st, ln)]
    assert [len(x) for x in slices] == [320] * 5 + [200, 320, 160, 320, 173]
    # same kernel, same length class: bit for bit
    assert np.array_equal(np.concatenate(rows), mfcc_frames(slices))
    check_rows(np.concatenate(rows), R.mfcc_rows(slices), "recordings")
    assert [r.shape for r in mfcc_recordings([np.zeros(5), R.signal(400, 4)])] == [(0, 13), (2, 13)]
    assert mfcc_recordings([]) == []


def test_encode_recordings_end_to_end(oracle):
    from hmm_training_amd import HMMTrained, calculate_log_likelihood, get_observations
    from hmm_training_amd.frontend import encode_recordings
    from hmm_training_amd.io import Centroid, Frame
    signals, rows, codebook = R.encode_case()
    assert R.vq_margins(np.concatenate(rows), codebook).min() > 1e-6  # the condition (tests/test_mfcc.py)
    cents = [Centroid(mfcc=c, id=i) for i, c in enumerate(codebook)]
    got = encode_recordings(signals, cents)
    assert len(got) == len(signals)
    for g, r in zip(got, rows):
        assert len(g) == len(r)
        if len(r):
            assert g.dtype == np.int64
            assert np.array_equal(g, oracle.vq(r, codebook))  # every frame
    for g, g2 in zip(got, encode_recordings(signals, codebook)):  # the codebook as an array
        assert np.array_equal(g, g2)
    # the same types as get_observations on the reference's rows, the empty recording included
    want = get_observations([[Frame(mfcc=x) for x in r] for r in rows], cents)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    # ... and it feeds the scorer unchanged
    rng = np.random.default_rng(0)
    A = rng.random((4, 4)) + 0.1
    B = rng.random((4, 64)) + 0.1
    hmm = HMMTrained(states=4, symbols=64, A=A / A.sum(1, keepdims=True), B=B / B.sum(1, keepdims=True),
                     Pi=np.full(4, 0.25), word="w")
    ll = calculate_log_likelihood(got[4], hmm)
    assert np.isfinite(ll) and ll < 0.0
    assert ll == calculate_log_likelihood(want[4], hmm)


def test_lbg_train_on_device_made_rows():
    from hmm_training_amd import lbg_train
    from hmm_training_amd.frontend import mfcc_recordings
    signals = [R.signal(n, 20 + i) for i, n in enumerate((8000, 6400, 4013))]
    rows_t, counts = mfcc_recordings(signals, return_tensor=True)
    assert rows_t.is_cuda and counts == [50, 40, 25] and tuple(rows_t.shape) == (115, 13)
    rows = rows_t.cpu().numpy()
    res = lbg_train(rows_t, n_centroids=4)
    chk = lbg_ref.lbg(rows, 4)
    assert lbg_ref.margins_ok(chk)
    assert [int(np.sum(res.records["generation"] == g)) for g in (1, 2)] == chk.passes
    assert np.array_equal(res.assignments, chk.assignments)
    np.testing.assert_allclose(res.centroids, chk.centroids, rtol=1e-9, atol=0)


# --------------------------------------------------------------------------------------------------------------
# files
# --------------------------------------------------------------------------------------------------------------
def test_load_frames_recompute(tmp_path):
    from hmm_training_amd.io import load_frames
    sig = R.signal(1000, 9)
    st, ln = R.frame_table(len(sig))
    data = [{"raw_samples": sig[a:a + n].tolist(), "sample_rate": 16000, "n_channels": 1, "frame_duration_ms": 20.0,
             "mfcc_vector": [float(i)] * 13, "parent_centroid_id": 0, "generation": 0, "frame_number": i,
             "recording": "r"} for i, (a, n) in enumerate(zip(st, ln))]
    data.append(dict(data[0], raw_samples=[], mfcc_vector=[5.0] * 13, frame_number=len(st)))  # no samples: kept
    path = str(tmp_path / "r_frames.json")
    with open(path, "w") as fh:
        json.dump(data, fh)
    stored = load_frames(path)
    assert all(np.array_equal(f.mfcc, np.full(13, float(i))) for i, f in enumerate(stored[:-1]))  # the default stays
    fresh = load_frames(path, recompute_mfcc=True)
    assert [f.frame_number for f in fresh] == list(range(len(st) + 1)) and fresh[0].recording == "r"
    want = R.mfcc_rows([sig[a:a + n] for a, n in zip(st, ln)])
    check_rows(np.stack([f.mfcc for f in fresh[:-1]]), want, "recomputed")
    assert np.array_equal(fresh[-1].mfcc, np.full(13, 5.0))


def test_main_features_round_trip(tmp_path, capsys):
    from hmm_training_amd.io import load_centroids, load_frames
    from hmm_training_amd.main import _cli
    sigs = {"alpha": R.signal(3000, 31), "beta": R.signal(2333, 32).astype(np.float32).reshape(-1, 1)}
    paths = []
    for name, s in sigs.items():
        p = str(tmp_path / f"{name}.npy")
        np.save(p, s)
        paths.append(p)
    out_dir = str(tmp_path / "frames")
    assert _cli(["features", "--signals", *paths, "--out-dir", out_dir]) == 0
    printed = capsys.readouterr().out
    frame_files = [os.path.join(out_dir, f"{n}_frames.json") for n in sigs]
    for (name, s), path in zip(sigs.items(), frame_files):
        assert f"Saved {len(R.frame_table(len(s))[0])} frames to {path}" in printed
        data = json.load(open(path))
        # the fields of RawDataMFCC.to_dict, in its order
        assert list(data[0]) == ["raw_samples", "sample_rate", "n_channels", "frame_duration_ms", "mfcc_vector",
                                 "parent_centroid_id", "generation", "frame_number", "recording"]
        flat = np.asarray(s).astype(float).flatten()
        st, ln = R.frame_table(len(flat))
        assert [d["frame_number"] for d in data] == list(range(len(st))) and data[0]["recording"] == name
        assert [len(d["raw_samples"]) for d in data] == ln
        assert data[1]["raw_samples"] == flat[160:480].tolist()
        frames = load_frames(path)
        want = R.mfcc_rows([flat[a:a + n] for a, n in zip(st, ln)])
        check_rows(np.stack([f.mfcc for f in frames]), want, name)
        again = load_frames(path, recompute_mfcc=True)
        assert all(np.array_equal(a.mfcc, b.mfcc) for a, b in zip(frames, again))  # repr round trip, same kernel
    book = str(tmp_path / "codevector.json")
    assert _cli(["codebook", "--frames", *frame_files, "--out", book, "--centroids", "4"]) == 0
    assert len(load_centroids(book)) == 4
