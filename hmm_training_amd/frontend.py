"""The MFCC front end on the MI355X: processed signal -> frames -> MFCC rows -> observation symbols.

Replaces the per-frame ``librosa.feature.mfcc`` call of the reference's RawDataMFCC.calculate_mfcc
(CodeVector/codevector_classes.py:226-250) and the framing of AudioProcessor._split_into_frames_with_overlap
(:413-431; HMM/live_testing.py:207-225 is the same rule) with ``hmmbw_mfcc`` (include/hmmbw.h): every frame of a batch
of recordings in one launch per distinct frame length, the rows left on the device for ``hmmbw_vq_encode`` and
``hmmbw_lbg_train``.

* ``frame_table``: the (starts, lengths) of a signal's frames;
* ``mfcc_frames``: RawDataMFCC.calculate_mfcc for each frame of a list;
* ``mfcc_recordings``: signals in, one [T_r, n_mfcc] array per signal out;
* ``encode_recordings``: signals in, observation symbols out (process_recording + get_observations).

In front of it, signal conditioning (``hmmbw_preprocess``, ``hmmbw_window_overlap``): the reference's preemphasis.py
and the do_preemphasis of its live recogniser, raw recording -> processed signal:

* ``preprocess_recordings``: raw recordings in, trimmed (and windowed) signals and their bounds out;
* ``encode_raw_recordings``: raw recordings in, observation symbols out, nothing on the host in between.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

AMIN = 1e-10    # librosa.power_to_db's defaults, which librosa.feature.mfcc uses
TOP_DB = 80.0
MIN_TAIL = 12   # a remainder frame needs more samples than this (:428)
PREEMPHASIS = 0.95                      # filter_signal, preemphasis.py:179
FACTORS = {"batch": (-1.0, 0.015, -1.0, 0.015),   # (zf, pf, zl, pl): slice_signal of preemphasis.py:256 (no zcr test)
           "live": (0.08, 0.15, 0.03, 0.10)}      # ... and of HMM/live_testing.py:80-88
WINDOW_LEN, WINDOW_HOP = 320, 128       # hamming_window, preemphasis.py:190-191

_tables: Dict[tuple, tuple] = {}  # (L, sample_rate, n_mels, n_mfcc, device) -> (window, twiddle, mel, dct) on the device


def frame_table(n_samples: int, frame_size: int = 320, hop_size: int = 160) -> Tuple[np.ndarray, np.ndarray]:
    """(starts, lengths), int64, of the frames of a signal of ``n_samples`` samples: full frames every ``hop_size``
    samples, then one remainder frame from ``n_full * hop_size`` to the end if it has more than 12 samples."""
    n, fs, hop = int(n_samples), int(frame_size), int(hop_size)
    if fs < 1 or hop < 1:
        raise ValueError("frame_size and hop_size must be at least 1")
    full = (n - fs) // hop + 1 if n >= fs else 0
    starts = np.arange(full, dtype=np.int64) * hop
    lengths = np.full(full, fs, dtype=np.int64)
    last = full * hop
    if last < n and n - last > MIN_TAIL:
        starts = np.append(starts, np.int64(last))
        lengths = np.append(lengths, np.int64(n - last))
    return starts, lengths


def _device(device):
    import torch
    return torch.device("cuda", torch.cuda.current_device() if device is None else int(device))


def _device_tables(L: int, sample_rate: float, n_mels: int, n_mfcc: int, dev):
    """The four tables of one frame length on the device (hmmbw_mfcc_tables, cached)."""
    import torch

    from ._lib import check, lib
    key = (int(L), float(sample_rate), int(n_mels), int(n_mfcc), str(dev))
    t = _tables.get(key)
    if t is None:
        H = L // 2 + 1
        host = [np.empty(max(L, 1)), np.empty((max(L, 1), 2)), np.empty((max(n_mels, 1), H)),
                np.empty((max(n_mfcc, 1), max(n_mels, 1)))]
        check(lib().hmmbw_mfcc_tables(int(L), float(sample_rate), int(n_mels), int(n_mfcc),
                                      *[ctypes.c_void_p(a.ctypes.data) for a in host]))
        t = tuple(torch.from_numpy(a).to(dev) for a in host)
        _tables[key] = t
    return t


def _run(samples, starts: np.ndarray, lengths: np.ndarray, out, dev, sample_rate, n_mfcc, n_mels, amin, top_db) -> None:
    """Enqueue hmmbw_mfcc for every distinct frame length; rows land in ``out`` [F, stride] (device) in frame order."""
    import torch

    from ._lib import check, lib
    L_ = lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_samples = int(samples.numel())
    keep = []  # device buffers the enqueued kernels read
    for L in np.unique(lengths):
        sel = np.flatnonzero(lengths == L)
        if starts[sel].min() < 0 or starts[sel].max() + int(L) > n_samples:
            raise ValueError("a frame runs past the end of the samples")
        win, tw, mel, dct = _device_tables(int(L), sample_rate, n_mels, n_mfcc, dev)
        ts = torch.from_numpy(np.ascontiguousarray(starts[sel])).to(dev)
        keep.append(ts)
        if len(sel) == len(lengths):
            dst = out
        else:
            dst = torch.empty((len(sel), out.shape[1]), dtype=torch.float64, device=dev)
        check(L_.hmmbw_mfcc(ctypes.c_void_p(stream), ctypes.c_void_p(samples.data_ptr()), n_samples,
                            ctypes.c_void_p(ts.data_ptr()), len(sel), int(L), ctypes.c_void_p(win.data_ptr()),
                            ctypes.c_void_p(tw.data_ptr()), ctypes.c_void_p(mel.data_ptr()), int(n_mels),
                            ctypes.c_void_p(dct.data_ptr()), int(n_mfcc), float(amin), float(top_db),
                            ctypes.c_void_p(dst.data_ptr()), int(out.shape[1])))
        if dst is not out:
            out[torch.from_numpy(sel).to(dev), :n_mfcc] = dst[:, :n_mfcc]
    del keep  # torch's caching allocator keeps a freed block on its stream: the kernels above run first


def _as_signal(x) -> np.ndarray:
    return np.asarray(x).astype(float).flatten()  # the reference's conversion (:235)


def _check_settings(n_mfcc, n_mels):
    if int(n_mels) < 1 or int(n_mfcc) < 1 or int(n_mfcc) > int(n_mels):
        raise ValueError("need n_mels >= 1 and 1 <= n_mfcc <= n_mels")


def _rows_on_device(signals: Sequence, sample_rate, n_mfcc, n_mels, frame_size, hop_size, amin, top_db, dev):
    """(rows [F, n_mfcc] on the device or None when F == 0, frames per signal): one upload of the concatenated signals."""
    import torch
    sigs = [_as_signal(s) for s in signals]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    starts, lengths, counts = [], [], []
    for s, o in zip(sigs, offs[:-1]):
        st, ln = frame_table(len(s), frame_size, hop_size)
        starts.append(st + o)
        lengths.append(ln)
        counts.append(len(st))
    starts = np.concatenate(starts) if starts else np.zeros(0, np.int64)
    lengths = np.concatenate(lengths) if lengths else np.zeros(0, np.int64)
    if len(starts) == 0:
        return None, counts
    if lengths.min() < 2:
        raise ValueError("a frame needs at least 2 samples")
    tx = torch.from_numpy(np.concatenate(sigs)).to(dev)
    out = torch.empty((len(starts), int(n_mfcc)), dtype=torch.float64, device=dev)
    _run(tx, starts, lengths, out, dev, sample_rate, n_mfcc, n_mels, amin, top_db)
    return out, counts


def mfcc_frames(frames: Sequence, sample_rate: int = 16000, n_mfcc: int = 13, n_mels: int = 26, amin: float = AMIN,
                top_db: float = TOP_DB, device: Optional[int] = None) -> np.ndarray:
    """[F, n_mfcc]: RawDataMFCC.calculate_mfcc of every frame of ``frames`` (arrays of any lengths >= 2, also (L, 1)
    columns and integer dtypes).  A frame with a non-finite sample gives zeros, as the reference's except branch."""
    import torch
    _check_settings(n_mfcc, n_mels)
    fr = [_as_signal(f) for f in frames]
    if not fr:
        return np.zeros((0, int(n_mfcc)))
    lengths = np.array([len(f) for f in fr], dtype=np.int64)
    if lengths.min() < 2:
        raise ValueError("a frame needs at least 2 samples")
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)
    dev = _device(device)
    with torch.cuda.device(dev):
        tx = torch.from_numpy(np.concatenate(fr)).to(dev)
        out = torch.empty((len(fr), int(n_mfcc)), dtype=torch.float64, device=dev)
        _run(tx, starts, lengths, out, dev, sample_rate, n_mfcc, n_mels, amin, top_db)
        return out.cpu().numpy()


def mfcc_recordings(signals: Sequence, sample_rate: int = 16000, n_mfcc: int = 13, n_mels: int = 26,
                    frame_size: int = 320, hop_size: int = 160, amin: float = AMIN, top_db: float = TOP_DB,
                    device: Optional[int] = None, return_tensor: bool = False):
    """One [T_r, n_mfcc] array per signal, its frames by ``frame_table``.  With ``return_tensor`` the rows of all signals
    stay on the device: (tensor [sum T_r, n_mfcc], [T_r, ...]) — what ``lbg_train`` takes as it is."""
    import torch
    _check_settings(n_mfcc, n_mels)
    dev = _device(device)
    with torch.cuda.device(dev):
        out, counts = _rows_on_device(signals, sample_rate, n_mfcc, n_mels, frame_size, hop_size, amin, top_db, dev)
        if out is None:
            out = torch.zeros((0, int(n_mfcc)), dtype=torch.float64, device=dev)
        if return_tensor:
            return out, counts
        rows = out.cpu().numpy()
    pos = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [rows[pos[i]:pos[i + 1]].copy() for i in range(len(counts))]


def _raw_signal(x) -> np.ndarray:
    """Column 0 of a 2-D recording (the reference reads signal[i, 0]); int16 stays int16, the rest becomes float64."""
    a = np.asarray(x)
    if a.ndim == 2:
        a = a[:, 0]
    elif a.ndim != 1:
        raise ValueError("a recording is a 1-D array or an (n, channels) array")
    return np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float64))


def hamming_table(wlen: int = WINDOW_LEN) -> np.ndarray:
    """The reference's window table (preemphasis.py:194-195), built with NumPy as it builds it."""
    return 0.54 - 0.46 * np.cos((2 * np.pi * np.arange(wlen)) / (wlen - 1))


def _conditioned_on_device(signals: Sequence, sample_rate, mode, factors, window, dev, want_stats=False):
    """Enqueue hmmbw_preprocess (and hmmbw_window_overlap) on the current stream.  Returns (y [N] on the device,
    bounds [R, 2] on the device, offsets (host, int64 [R + 1]), stats [sum nf, 2] on the device or None)."""
    import torch

    from ._lib import SAMPLES_F64, SAMPLES_I16, check, lib
    if mode not in FACTORS:
        raise ValueError("mode is 'batch' or 'live'")
    fac = np.ascontiguousarray(FACTORS[mode] if factors is None else factors, dtype=np.float64)
    if fac.shape != (4,):
        raise ValueError("factors are (zf, pf, zl, pl)")
    if window is None:
        window = mode == "live"
    sigs = [_raw_signal(s) for s in signals]
    as_i16 = all(s.dtype == np.int16 for s in sigs)
    if not as_i16:
        sigs = [s.astype(np.float64) for s in sigs]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    win, hop = int(0.02 * sample_rate), int(0.01 * sample_rate)
    R = len(sigs)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    tx = torch.from_numpy(np.concatenate(sigs) if R else np.zeros(0)).to(dev)
    toff = torch.from_numpy(offs).to(dev)
    y = torch.empty(int(offs[-1]), dtype=torch.float64, device=dev)
    bounds = torch.zeros((R, 2), dtype=torch.int64, device=dev)
    stats = None
    if want_stats:
        nf = sum(max(int((len(s) - win) / hop) + 1, 0) for s in sigs) if hop > 0 else 0
        stats = torch.zeros((nf, 2), dtype=torch.float64, device=dev)
    L_ = lib()
    if R == 0:
        return y, bounds, offs, stats
    check(L_.hmmbw_preprocess(stream, p(tx), SAMPLES_I16 if as_i16 else SAMPLES_F64, p(toff),
                              ctypes.c_void_p(offs.ctypes.data), R, PREEMPHASIS, win, hop,
                              ctypes.c_void_p(fac.ctypes.data), p(y), p(bounds), p(stats) if want_stats else None))
    if window is not False and window is not None:
        table = hamming_table() if window is True else np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
        tw = torch.from_numpy(table).to(dev)
        check(L_.hmmbw_window_overlap(stream, p(y), p(toff), p(bounds), R, p(tw), len(table), WINDOW_HOP))
    return y, bounds, offs, stats


def preprocess_recordings(signals: Sequence, sample_rate: int = 16000, mode: str = "batch", factors=None, window=None,
                          device: Optional[int] = None, return_stats: bool = False):
    """(trimmed, bounds): the reference's signal conditioning of every raw recording, on the GPU (hmmbw_preprocess):
    the filter 1 - 0.95 z^-1, the power / zero-crossing trim, and in live mode the overlapping Hamming window.

    ``signals``: 1-D arrays or (n, channels) arrays (column 0 is taken, as the reference does); int16 recordings go
    up as int16.  ``mode``: "batch" is preemphasis.py (what it ``np.save``s under Data/Processed), "live" is
    HMM/live_testing.do_preemphasis; ``factors`` (zf, pf, zl, pl) overrides the mode's thresholds; ``window`` is
    False (off, batch default), True (the 320-sample Hamming table at hop 128, live default) or a table of its own.
    ``trimmed`` is a list of (m, 1) float64 arrays, ``bounds`` int64 [R, 2] (start, finish) within each recording.
    With ``return_stats`` a third value: one [nf, 2] array (zcr, power) per recording.
    A recording too short for one 20 ms frame raises ValueError, as the reference raises.  All arithmetic is fp64: for
    int16 and float64 recordings the result is the reference's bit for bit; the float32 arithmetic NumPy 2 gives the
    reference's filter for a float32 recording is not reproduced."""
    import torch
    dev = _device(device)
    with torch.cuda.device(dev):
        y, bounds, offs, stats = _conditioned_on_device(signals, sample_rate, mode, factors, window, dev, return_stats)
        yh, bh = y.cpu().numpy(), bounds.cpu().numpy()
        sh = stats.cpu().numpy() if return_stats else None
    trimmed = [yh[o + b[0]:o + b[1]].reshape(-1, 1).copy() for o, b in zip(offs[:-1], bh)]
    if not return_stats:
        return trimmed, bh
    win, hop = int(0.02 * sample_rate), int(0.01 * sample_rate)
    nf = [int((int(n) - win) / hop) + 1 for n in np.diff(offs)]
    pos = np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)
    return trimmed, bh, [sh[pos[i]:pos[i + 1]].copy() for i in range(len(nf))]


def _codebook_array(centroids) -> np.ndarray:
    if isinstance(centroids, np.ndarray):
        return np.ascontiguousarray(centroids, dtype=np.float64)
    if len(centroids) == 0:
        return np.zeros((0, 13))
    return np.stack([np.asarray(c.mfcc, dtype=np.float64).reshape(-1) for c in centroids])


def encode_raw_recordings(signals: Sequence, centroids, mode: str = "batch", sample_rate: int = 16000, factors=None,
                          window=None, n_mels: int = 26, frame_size: int = 320, hop_size: int = 160,
                          device: Optional[int] = None) -> List[np.ndarray]:
    """Observation symbols of every RAW recording: hmmbw_preprocess (and the window in live mode), hmmbw_mfcc and
    hmmbw_vq_encode on one stream; the conditioned signal and the MFCC rows never leave the device.  The frames of
    recording r are ``frame_table(m_r)`` from its trimmed start.  One small read-back (the bounds, [R, 2]) sits
    between the stages: the frame count is a host argument of hmmbw_mfcc.  Returns what ``encode_recordings`` returns
    for the conditioned signals: an int64 array per recording (an empty array where nothing is left)."""
    import torch

    from ._lib import check, lib
    C = _codebook_array(centroids)
    K, D = C.shape
    if K > 0:
        _check_settings(D, n_mels)
    dev = _device(device)
    with torch.cuda.device(dev):
        y, bounds, offs, _ = _conditioned_on_device(signals, sample_rate, mode, factors, window, dev)
        bh = bounds.cpu().numpy()  # the one read-back
        starts, lengths, counts = [], [], []
        for o, (b0, b1) in zip(offs[:-1], bh):
            st, ln = frame_table(max(int(b1 - b0), 0), frame_size, hop_size)
            starts.append(st + int(o) + int(b0))
            lengths.append(ln)
            counts.append(len(st))
        starts = np.concatenate(starts) if starts else np.zeros(0, np.int64)
        lengths = np.concatenate(lengths) if lengths else np.zeros(0, np.int64)
        if K == 0:  # get_observations with an empty codebook
            return [np.zeros(T, dtype=np.int64) for T in counts]
        F = len(starts)
        if F == 0:
            return [np.array([]) for _ in counts]
        if lengths.min() < 2:
            raise ValueError("a frame needs at least 2 samples")
        rows = torch.empty((F, D), dtype=torch.float64, device=dev)
        _run(y, starts, lengths, rows, dev, sample_rate, D, n_mels, AMIN, TOP_DB)
        if D < 2:
            sym = np.zeros(F, dtype=np.int64)
        else:
            tc = torch.from_numpy(C).to(dev)
            ts = torch.empty(F, dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(lib().hmmbw_vq_encode(ctypes.c_void_p(stream), ctypes.c_void_p(rows.data_ptr()), F, D, 1, D - 1,
                                        ctypes.c_void_p(tc.data_ptr()), K, ctypes.c_void_p(ts.data_ptr()), None))
            sym = ts.cpu().numpy().astype(np.int64)
    out, pos = [], 0
    for T in counts:
        out.append(sym[pos:pos + T] if T else np.array([]))
        pos += T
    return out


def encode_recordings(signals: Sequence, centroids, sample_rate: int = 16000, n_mels: int = 26, frame_size: int = 320,
                      hop_size: int = 160, device: Optional[int] = None) -> List[np.ndarray]:
    """Observation symbols of every signal: framing -> hmmbw_mfcc -> hmmbw_vq_encode on one stream, the MFCC rows never
    leaving the device.  ``centroids`` is a list of objects with ``.mfcc`` (io.Centroid) or an array [K, D]; the rows
    have D coefficients.  Returns what get_observations returns: an int64 array per recording."""
    import torch

    from ._lib import check, lib
    if isinstance(centroids, np.ndarray):
        C = np.ascontiguousarray(centroids, dtype=np.float64)
    elif len(centroids) == 0:
        C = np.zeros((0, 13))
    else:
        C = np.stack([np.asarray(c.mfcc, dtype=np.float64).reshape(-1) for c in centroids])
    K, D = C.shape
    if K == 0:  # get_observations with an empty codebook
        return [np.zeros(len(frame_table(len(_as_signal(s)), frame_size, hop_size)[0]), dtype=np.int64) for s in signals]
    _check_settings(D, n_mels)
    dev = _device(device)
    with torch.cuda.device(dev):
        rows, counts = _rows_on_device(signals, sample_rate, D, n_mels, frame_size, hop_size, AMIN, TOP_DB, dev)
        if rows is None:
            return [np.array([]) for _ in counts]
        F = int(rows.shape[0])
        if D < 2:  # every distance is norm([]) = 0: the first centroid wins
            sym = np.zeros(F, dtype=np.int64)
        else:
            tc = torch.from_numpy(C).to(dev)
            ts = torch.empty(F, dtype=torch.int32, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            check(lib().hmmbw_vq_encode(ctypes.c_void_p(stream), ctypes.c_void_p(rows.data_ptr()), F, D, 1, D - 1,
                                        ctypes.c_void_p(tc.data_ptr()), K, ctypes.c_void_p(ts.data_ptr()), None))
            sym = ts.cpu().numpy().astype(np.int64)
    out, pos = [], 0
    for T in counts:
        out.append(sym[pos:pos + T] if T else np.array([]))
        pos += T
    return out
