"""The MFCC contract in NumPy / SciPy: what hmmbw_mfcc must compute (include/hmmbw.h), restated from the defaults of
librosa 0.11.0's ``librosa.feature.mfcc(y=frame, sr=16000, n_mfcc=13, n_fft=len(frame), hop_length=None,
center=False, n_mels=26)``, the call of RawDataMFCC.calculate_mfcc (CodeVector/codevector_classes.py:226-250).
librosa itself is not available to the tests; DESIGN §6 "MFCC front end" says what that leaves unverified.

Two forms: ``mfcc`` takes the spectrum from np.fft.rfft, ``mfcc_direct`` from a direct DFT with long-double twiddles.
Both take optional tables (window, mel, dct), so that a test can hand them the library's.
"""
import numpy as np
import scipy.fft
import scipy.signal

AMIN = 1e-10
TOP_DB = 80.0


def frame_table(n_samples, frame_size=320, hop_size=160):
    """AudioProcessor._split_into_frames_with_overlap (:413-431), as (starts, lengths)."""
    starts, lengths = [], []
    for i in range(0, n_samples - frame_size + 1, hop_size):
        starts.append(i)
        lengths.append(frame_size)
    last_start = len(starts) * hop_size
    if last_start < n_samples:
        if n_samples - last_start > 12:
            starts.append(last_start)
            lengths.append(n_samples - last_start)
    return starts, lengths


def hz_to_mel(f):
    f = np.asanyarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    mels = f / f_sp
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    if f.ndim:
        t = f >= min_log_hz
        mels[t] = min_log_mel + np.log(f[t] / min_log_hz) / logstep
    elif f >= min_log_hz:
        mels = min_log_mel + np.log(f / min_log_hz) / logstep
    return mels


def mel_to_hz(mels):
    mels = np.asanyarray(mels, dtype=np.float64)
    f_sp = 200.0 / 3
    freqs = f_sp * mels
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    t = mels >= min_log_mel
    freqs[t] = min_log_hz * np.exp(logstep * (mels[t] - min_log_mel))
    return freqs


def mel_filters(L, sr=16000, n_mels=26):
    """librosa.filters.mel(sr=sr, n_fft=L, n_mels=n_mels) (fmin 0, fmax sr / 2, htk=False, norm='slaney'): float32."""
    weights = np.zeros((n_mels, 1 + L // 2), dtype=np.float32)
    fftfreqs = np.fft.rfftfreq(n=L, d=1.0 / sr)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(0.0), hz_to_mel(sr / 2), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, fftfreqs)
    for i in range(n_mels):
        lower = -ramps[i] / fdiff[i]
        upper = ramps[i + 2] / fdiff[i + 1]
        weights[i] = np.maximum(0, np.minimum(lower, upper))  # the float32 store
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    weights *= enorm[:, np.newaxis]  # fp64 product, stored as float32
    weights += 0.0  # the zero ramp at 0 Hz comes out as -0.0: a zero weight either way, kept as +0.0 here
    return weights


def window(L):
    return scipy.signal.get_window("hann", L, fftbins=True)


def dct_matrix(n_mfcc, n_mels):
    """Rows 0 .. n_mfcc - 1 of the orthonormal DCT-II, taken from scipy.fft.dct itself."""
    return scipy.fft.dct(np.eye(n_mels), type=2, norm="ortho", axis=0)[:n_mfcc]


def _tail(P, L, sr, n_mfcc, n_mels, mel, dct, amin, top_db):
    W = (mel_filters(L, sr, n_mels) if mel is None else np.asarray(mel)).astype(np.float64)
    M = W @ P
    dB = 10.0 * np.log10(np.maximum(amin, M))
    if top_db is not None and top_db >= 0:
        dB = np.maximum(dB, dB.max() - top_db)
    if dct is None:
        return scipy.fft.dct(dB, type=2, norm="ortho")[:n_mfcc]
    return np.asarray(dct, dtype=np.float64) @ dB


def _prepare(frame):
    return np.asarray(frame).astype(float).flatten()


def mfcc(frame, sr=16000, n_mfcc=13, n_mels=26, win=None, mel=None, dct=None, amin=AMIN, top_db=TOP_DB):
    """One frame's MFCC [n_mfcc]; a frame with a non-finite sample gives zeros (calculate_mfcc's except branch)."""
    x = _prepare(frame)
    if not np.all(np.isfinite(x)):
        return np.zeros(n_mfcc)
    L = len(x)
    y = x * (window(L) if win is None else np.asarray(win, dtype=np.float64))
    P = np.abs(np.fft.rfft(y, n=L)) ** 2
    return _tail(P, L, sr, n_mfcc, n_mels, mel, dct, amin, top_db)


def mfcc_direct(frame, sr=16000, n_mfcc=13, n_mels=26, win=None, mel=None, dct=None, amin=AMIN, top_db=TOP_DB):
    """The same with a direct DFT: twiddles in long double, products and sums in long double, rounded once."""
    x = _prepare(frame)
    if not np.all(np.isfinite(x)):
        return np.zeros(n_mfcc)
    L = len(x)
    y = (x * (window(L) if win is None else np.asarray(win, dtype=np.float64))).astype(np.longdouble)
    k = np.arange(L // 2 + 1)
    kn = np.outer(k, np.arange(L)) % L
    pi = np.arctan2(np.longdouble(0), np.longdouble(-1))  # np.pi is a double
    ang = 2 * pi * kn.astype(np.longdouble) / L
    re = np.cos(ang) @ y
    im = np.sin(ang) @ y
    P = (re * re + im * im).astype(np.float64)
    return _tail(P, L, sr, n_mfcc, n_mels, mel, dct, amin, top_db)


def mfcc_rows(frames, form=mfcc, **kw):
    n_mfcc = kw.get("n_mfcc", 13)
    return np.stack([form(f, **kw) for f in frames]) if len(frames) else np.zeros((0, n_mfcc))


# --- the inputs the CPU and the GPU tests share -----------------------------------------------------------------
AMPLITUDES = (1e-6, 1e-3, 1.0, 3e4)


def tone_frames(F, L, seed, sr=16000):
    """F frames of L samples: one or two tones plus white noise 20 dB below, amplitudes cycling over AMPLITUDES."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    out = []
    for f in range(F):
        a = AMPLITUDES[f % len(AMPLITUDES)]
        f1, f2 = rng.uniform(80.0, 0.45 * sr, size=2)
        x = np.sin(2 * np.pi * f1 * t + rng.uniform(0, 6.28)) + 0.5 * (f % 2) * np.sin(2 * np.pi * f2 * t)
        out.append(a * (x + 0.1 * rng.normal(size=L)))
    return out


PARITY_CASES = [(1, 320), (15, 320), (16, 320), (17, 320), (1000, 320), (18, 13), (18, 14), (18, 161), (18, 200),
                (18, 319), (18, 512)]


def parity_inputs(F, L):
    return tone_frames(F, L, seed=1000 * L + F)


def signal(n, seed, amp=1000.0, sr=16000):
    """A speech-like test signal: a few drifting tones under an envelope, plus noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = np.zeros(n)
    for _ in range(4):
        f0 = rng.uniform(100.0, 3500.0)
        x += rng.uniform(0.2, 1.0) * np.sin(2 * np.pi * (f0 + rng.uniform(-200, 200) * t) * t + rng.uniform(0, 6.28))
    env = 0.3 + np.abs(np.sin(2 * np.pi * rng.uniform(2.0, 9.0) * t + rng.uniform(0, 3.0)))
    return amp * (env * x + 0.05 * rng.normal(size=n))


# The largest absolute difference between the two forms above over every frame of PARITY_CASES (measured while the
# tests were written; tests/test_mfcc.py asserts it): one unit in the last place of c[0] = -509.9, the silent-level
# rows.  The GPU tolerance is 100 times that, and never above the project's 1e-9.
CPU_FORMS_DIFF = 2.0 ** -43  # 1.137e-13
GPU_TOL = min(100 * CPU_FORMS_DIFF, 1e-9)


# --- the end-to-end case: signals -> symbols against a 64-centroid codebook ------------------------------------------
ENCODE_LENGTHS = (1000, 320, 333, 2500, 4013, 12, 700)
ENCODE_SEED = 7


def encode_case():
    """(signals, reference rows per signal, codebook [64, 13]).  The codebook is drawn around the rows' own mean and
    spread, so every centroid is a plausible neighbour."""
    signals = [signal(n, ENCODE_SEED * 100 + i) for i, n in enumerate(ENCODE_LENGTHS)]
    rows = []
    for s in signals:
        starts, lengths = frame_table(len(s))
        rows.append(mfcc_rows([s[a:a + l] for a, l in zip(starts, lengths)]))
    allrows = np.concatenate(rows)
    rng = np.random.default_rng(ENCODE_SEED)
    pick = rng.integers(0, len(allrows), size=64)
    codebook = allrows[pick] + rng.normal(size=(64, 13)) * allrows.std(axis=0) * 0.5
    return signals, rows, codebook


def vq_margins(rows, codebook):
    """second-nearest minus nearest distance over the columns [1, 13) of every row"""
    d = np.sqrt(((rows[:, None, 1:] - codebook[None, :, 1:]) ** 2).sum(axis=2))
    d.sort(axis=1)
    return d[:, 1] - d[:, 0]
