"""A vectorised NumPy restatement of the signal-conditioning contract (include/hmmbw.h, hmmbw_preprocess and
hmmbw_window_overlap): the filter 1 - 0.95 z^-1, the frame statistics with the last frame's odd length, the two pairs
of thresholds and the in-place overlapping window, each as the contract words it and none of it read from the package.
tests/golden/preprocess.npz holds what the reference's own loops give for the inputs of ``golden_inputs``;
tests/test_preprocess.py compares the two, and the GPU tests compare the kernels with this file.
"""
import numpy as np

COEFF = 0.95
BATCH = (-1.0, 0.015, -1.0, 0.015)
LIVE = (0.08, 0.15, 0.03, 0.10)
WLEN, WHOP = 320, 128
SR, WIN, HOP = 16000, 320, 160

# power: a sum of at most 478 non-negative terms in any order carries at most about (L + 2) 2^-53 relative error; two
# orders (NumPy's pairwise sum, a wave reduction) differ by at most twice that, 1.07e-13
POWER_RTOL = 2e-13
MARGIN = 1e-9   # every frame's power is farther than this (relative) from every power threshold in use


def power_rtol(longest):
    """the bound above for a geometry whose longest frame has ``longest`` samples (win + hop - 2 at the most): L squares
    rounded once each, L - 1 additions and one division, in two orders; 1.07e-13 at 478, 3.2e-13 at 1438"""
    return 2.0 * (longest + 2) * 2.0 ** -53


def longest_frame(lengths, win=WIN, hop=HOP):
    """the longest frame of recordings of these lengths"""
    return max(b - a for n in lengths for a, b in frame_slices(n, win, hop)[-2:])


def rate_geometry(sr):
    """(win, hop) as the reference derives them from a sample rate"""
    return int(0.02 * sr), int(0.01 * sr)


GOLDEN_LENGTHS = (161, 200, 319, 320, 321, 479, 480, 481, 640, 1000, 4000)
PLACEMENTS = ("middle", "start", "end")


def trunc_div(a, b):
    """int(a / b) of Python for integers: toward zero"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def column(x):
    x = np.asarray(x)
    return x[:, 0] if x.ndim == 2 else x


def filter_signal(x, coeff=COEFF):
    x = column(x).astype(np.float64)
    y = np.zeros(len(x))
    y[1:] = x[1:] - coeff * x[:-1]   # NumPy rounds the product on its own
    return y


def frame_count(n, win=WIN, hop=HOP):
    return trunc_div(n - win, hop) + 1


def frame_slices(n, win=WIN, hop=HOP):
    nf = frame_count(n, win, hop)
    if nf < 1:
        raise ValueError("no frame")
    return [(i * hop, i * hop + win) for i in range(nf - 1)] + [((nf - 1) * hop, n - 1)]


def frame_stats(y, win=WIN, hop=HOP):
    """(zcr [nf], power [nf])"""
    sl = frame_slices(len(y), win, hop)
    zcr, power = np.zeros(len(sl)), np.zeros(len(sl))
    for i, (a, b) in enumerate(sl):
        f = y[a:b]
        s = np.sign(f)
        zcr[i] = 0.5 * np.abs(s[1:] - s[:-1]).sum()
        power[i] = (f * f).sum() / len(f)
    return zcr, power


def keep_masks(zcr, power, factors):
    zf, pf, zl, pl = factors
    mz, mp = zcr.max(), power.max()
    kf = (power > pf * mp) & ((zcr > zf * mz) if zf >= 0 else True)
    kl = (power > pl * mp) & ((zcr > zl * mz) if zl >= 0 else True)
    return kf, kl


def bounds_of(zcr, power, factors, hop=HOP):
    """(start, finish, took_else_branch)"""
    kf, kl = keep_masks(zcr, power, factors)
    if kf.any():
        return int(np.flatnonzero(kf)[0]) * hop, int(np.flatnonzero(kl)[-1]) * hop, False
    return 0, len(zcr) * hop, True


def window_table(wlen=WLEN):
    return 0.54 - 0.46 * np.cos((2 * np.pi * np.arange(wlen)) / (wlen - 1))


def window_frames(m, wlen=WLEN, whop=WHOP):
    """(q, length of the partial frame)"""
    q = trunc_div(m - wlen, whop) + 1
    return q, (0 if q < 0 else max(0, m - 1 - q * whop))


def window_overlap(t, w=None, whop=WHOP):
    """the in-place loop over frames, ascending (a full frame is clipped to the signal where the reference raises)"""
    w = window_table() if w is None else np.asarray(w, dtype=np.float64)
    t = np.array(t, dtype=np.float64).reshape(-1)
    m, wlen = len(t), len(w)
    q, part = window_frames(m, wlen, whop)
    for i in range(max(q, 0)):
        seg = t[i * whop:i * whop + wlen]
        seg *= w[:len(seg)]
    if q >= 0 and part > 0:
        t[q * whop:q * whop + part] *= w[:part]
    return t


def preprocess(x, factors, window=False, sr=SR, *, win=None, hop=None, coeff=COEFF, wlen=WLEN, whop=WHOP):
    """dict: y, zcr, power, start, finish, else_branch, out (the trimmed, optionally windowed signal).  ``win`` and
    ``hop`` default to the sample rate's 20 ms and 10 ms; the window is the Hamming table of ``wlen`` at hop ``whop``.
    The bounds are clipped to the recording, as a slice clips them."""
    rwin, rhop = rate_geometry(sr)
    win, hop = rwin if win is None else win, rhop if hop is None else hop
    y = filter_signal(x, coeff)
    zcr, power = frame_stats(y, win, hop)
    start, finish, other = bounds_of(zcr, power, factors, hop)
    start, finish = min(start, len(y)), min(finish, len(y))
    out = y[start:finish].copy()
    if window:
        out = window_overlap(out, window_table(wlen), whop)
    return dict(y=y, zcr=zcr, power=power, start=start, finish=finish, else_branch=other, out=out)


def power_margin(power, factors):
    """smallest relative distance of a frame's power from a power threshold in use"""
    mp = power.max()
    if mp == 0.0:
        return np.inf
    worst = np.inf
    for f in {factors[1], factors[3]}:
        worst = min(worst, float(np.abs(power - f * mp).min() / (f * mp)))
    return worst


# --- inputs ------------------------------------------------------------------------------------------------------------
def golden_input(n, placement, seed):
    """int16 (n, 1): Gaussian noise (sigma 20) plus a Hann-shaped burst of two tones (440 Hz, 2.3 kHz; amplitude 6000)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(scale=20.0, size=n)
    blen = max(n // 3, 40)
    a = {"middle": (n - blen) // 2, "start": 0, "end": n - blen}[placement]
    t = np.arange(blen) / SR
    burst = 6000.0 * np.hanning(blen) * 0.5 * (np.sin(2 * np.pi * 440.0 * t) + np.sin(2 * np.pi * 2300.0 * t))
    x[a:a + blen] += burst
    return np.clip(np.round(x), -32768, 32767).astype(np.int16).reshape(-1, 1)


def golden_inputs():
    """[(name, int16 column)]: 33 cases"""
    out = []
    for i, n in enumerate(GOLDEN_LENGTHS):
        for j, p in enumerate(PLACEMENTS):
            out.append((f"n{n}_{p}", golden_input(n, p, 1000 + 10 * i + j)))
    return out


def zeros_input(n=1000):
    return np.zeros((n, 1), dtype=np.int16)


def live_else_input(n=3200, seed=5):
    """quiet noise with many zero crossings, then a loud 50 Hz tone with few: no frame passes both live tests (a
    silent stretch longer than a frame lies between the two, so that no frame holds some of each)"""
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    a, b = n // 2 - 200, n // 2 + 200
    x[:a] = rng.choice([-3.0, 3.0], size=a)
    x[b:] = 20000.0 * np.sin(2 * np.pi * 50.0 * np.arange(n - b) / SR + 0.3)
    return np.round(x).astype(np.int16).reshape(-1, 1)


def square_input(n=1000, amp=1000):
    """period of 2 samples: sign changes at every step"""
    x = np.where(np.arange(n) % 2 == 0, amp, -amp)
    return x.astype(np.int16).reshape(-1, 1)


ENCODE_SEED = 7


def encode_case():
    """(signals, live-mode conditioned signals, MFCC rows per signal, codebook [64, 13]) of the raw -> symbols test:
    the three 4000-sample golden inputs, and a codebook drawn as mfcc_ref.encode_case draws its own"""
    import mfcc_ref as M
    signals = [x for name, x in golden_inputs() if name.startswith("n4000_")]
    cond = [preprocess(x, LIVE, window=True)["out"] for x in signals]
    rows = []
    for s in cond:
        starts, lengths = M.frame_table(len(s))
        rows.append(M.mfcc_rows([s[a:a + l] for a, l in zip(starts, lengths)]))
    allrows = np.concatenate(rows)
    rng = np.random.default_rng(ENCODE_SEED)
    pick = rng.integers(0, len(allrows), size=64)
    codebook = allrows[pick] + rng.normal(size=(64, 13)) * allrows.std(axis=0) * 0.5
    return signals, cond, rows, codebook


def nearest(rows, codebook):
    """the first nearest centroid over the columns [1, 13) of every row"""
    d = np.sqrt(((rows[:, None, 1:] - codebook[None, :, 1:]) ** 2).sum(axis=2))
    return d.argmin(axis=1).astype(np.int64)


def special_inputs():
    """[(name, int16 column)] of the GPU tests beyond the golden cases"""
    return [("zeros", zeros_input()), ("live_else", live_else_input()), ("square", square_input()),
            ("long", long_input())]


def long_input(n=170000, seed=9):
    """more frames than the kernel keeps in the LDS (1024): a burst in noise"""
    rng = np.random.default_rng(seed)
    x = rng.normal(scale=20.0, size=n)
    a, blen = n // 3, n // 4
    t = np.arange(blen) / SR
    x[a:a + blen] += 5000.0 * np.hanning(blen) * np.sin(2 * np.pi * 700.0 * t)
    return np.round(x).astype(np.int16).reshape(-1, 1)


# --- inputs at other geometries ------------------------------------------------------------------------------------------
RATES = (8000, 22050, 44100)   # (160, 80), (441, 220), (882, 441)


def rate_input(n, seed):
    """int16 (n, 1) for any n >= 2: Gaussian noise (sigma 20) plus a Hann-shaped burst of two tones (0.0275 and 0.14375
    cycles per sample: 440 Hz and 2.3 kHz at 16 kHz; amplitude 6000) over the middle third"""
    rng = np.random.default_rng(seed)
    x = rng.normal(scale=20.0, size=n)
    blen = n // 3
    a = (n - blen) // 2
    t = np.arange(blen)
    x[a:a + blen] += 6000.0 * np.hanning(blen) * 0.5 * (np.sin(2 * np.pi * 0.0275 * t) + np.sin(2 * np.pi * 0.14375 * t))
    return np.clip(np.round(x), -32768, 32767).astype(np.int16).reshape(-1, 1)


def rate_lengths(win, hop):
    """one frame at its shortest, one frame at its longest (win + hop - 2 samples), and two with several frames"""
    return (win - hop + 1, win + hop - 1, 3 * win + 7, 6 * win + 5)


def rate_inputs():
    """[(name, sample rate, int16 column)]: the 12 cases of tests/golden/preprocess_rates.npz"""
    out = []
    for i, sr in enumerate(RATES):
        for j, n in enumerate(rate_lengths(*rate_geometry(sr))):
            out.append((f"sr{sr}_n{n}", sr, rate_input(n, 2000 + 10 * i + j)))
    return out


GEOMETRIES = ((160, 80), (441, 220), (882, 441), (960, 480), (60, 30), (2, 1), (64, 64), (513, 1), (1024, 1024))


def geometry_lengths(win, hop):
    """the 12 lengths of one geometry's ragged batch: the shortest recording (2 samples where win - hop + 1 is less),
    win, win + hop - 1 (the longest last frame), 2 win, 3 win + 7, 12 win + 5 and six consecutive lengths (every
    length mod 4).  At hop < win / 8 shorter ones, so that the frames stay in the low thousands: win + 700 and
    3 win + 7, which then has more than the 1024 frames whose statistics the kernel keeps."""
    short = hop * 8 < win
    lengths = [max(win - hop + 1, 2), win, win + hop - 1, 2 * win]
    lengths += [win + 700, 3 * win + 7] if short else [3 * win + 7, 12 * win + 5]
    return lengths + [(win if short else 2 * win) + 1 + k for k in range(6)]


def geometry_inputs(win, hop):
    """[int16 column] of geometry_lengths"""
    return [rate_input(n, 3000 + 100 * GEOMETRIES.index((win, hop)) + k) for k, n in enumerate(geometry_lengths(win, hop))]


BATCH_SIZES = (511, 512, 1100)


def batch_inputs(n_rec):
    """[int16 column]: n_rec recordings of 161 to 700 samples at (320, 160); the batch of 512 holds long_input() in
    its middle (more than 1024 frames on the 4-wave launch)"""
    rng = np.random.default_rng(4000 + n_rec)
    lengths = rng.integers(161, 701, size=n_rec)
    out = [rate_input(int(n), 5000 + 2000 * BATCH_SIZES.index(n_rec) + k) for k, n in enumerate(lengths)]
    if n_rec == 512:
        out[300] = long_input()
    return out


def offset_length_residues(signals):
    """{(offset mod 4, length mod 4)} of a concatenated batch"""
    seen, off = set(), 0
    for s in signals:
        seen.add((off % 4, len(s) % 4))
        off += len(s)
    return seen


# --- exact ties ----------------------------------------------------------------------------------------------------------
TIE_COEFF, TIE_WIN = 0.5, 64
TIE_FACTORS = ((-1.0, 0.25, -1.0, 0.25), (0.5, 0.0, 0.5, 0.0), (-1.0, 1.0, -1.0, 1.0), (-1.0, 0.0, -1.0, 0.0))


def tie_frames():
    """dict of int16 frames of 64 samples that each begin and end with a zero, so that with hop == win the filtered
    frame is the same wherever it stands (y[0] = 0 as at a recording's start, and no frame sees its neighbour):
    ``loud`` (even values that alternate in sign over [1, 62): zcr 62 after the filter, counting the halves at the two
    zeros), ``half`` (loud / 2: exactly a quarter of its power, the same zcr), ``cross`` (quiet, alternating over
    [1, 31): zcr exactly 31) and ``silent``.  With coeff = 0.5 every filtered sample is a multiple of 0.5, every square
    one of 0.25 and every frame's sum an exact double in any order."""
    def alternating(k, amp):
        x = np.zeros(64, dtype=np.int64)
        j = np.arange(1, k)
        x[1:k] = np.where(j % 2 == 0, 1, -1) * amp(j)
        return x
    loud = alternating(62, lambda j: 2 * (1000 + 13 * j))
    cross = alternating(31, lambda j: 10 + j % 3)
    return dict(loud=loud.astype(np.int16), half=(loud // 2).astype(np.int16), cross=cross.astype(np.int16),
                silent=np.zeros(64, dtype=np.int16))


def tie_inputs():
    """[(name, int16 column, index of the tied frame, index of the loud frame)]: the tied frame before the loud one (it
    would move ``start``) and after it (it would move ``finish``); a silent frame and 37 silent samples at the end, so
    that the last frame (101 samples less the spared one) holds nothing"""
    fr = tie_frames()
    out = []
    for tied in ("half", "cross"):
        first = [fr[tied], fr["silent"], fr["loud"], fr["silent"]]
        last = [fr["silent"], fr["loud"], fr["silent"], fr[tied], fr["silent"]]
        for name, blocks, at, loud in ((f"{tied}_first", first, 0, 2), (f"{tied}_last", last, 3, 1)):
            x = np.concatenate(blocks + [np.zeros(37, dtype=np.int16)])
            out.append((name, x.reshape(-1, 1), at, loud))
    return out


# --- extremes ------------------------------------------------------------------------------------------------------------
def extreme_inputs(n=1001):
    """[(name, int16 column)]: full-scale alternation and a full-scale constant"""
    alt = np.where(np.arange(n) % 2 == 0, -32768, 32767).astype(np.int16)
    return [("alternating", alt.reshape(-1, 1)), ("constant", np.full((n, 1), 32767, dtype=np.int16))]


def nonfinite_batch():
    """three float64 recordings; the middle one holds NaN, +Inf and -Inf, some of them on its first and last samples"""
    a = rate_input(1003, 6001).astype(np.float64)
    c = rate_input(802, 6003).astype(np.float64)
    b = rate_input(1501, 6002).astype(np.float64)
    b[[0, 400, 401, 900], 0] = np.nan
    b[[5, 650], 0] = np.inf
    b[[6, 1200, 1500], 0] = -np.inf
    return [a, b, c]


# --- window tables -------------------------------------------------------------------------------------------------------
WINDOW_TABLES = ((1, 1), (5, 5), (4, 10), (320, 40), (882, 441), (4096, 512))


def window_lengths(wlen, whop):
    """trimmed lengths around every change of the frame count, and those where (m - wlen) / whop is negative and not
    whole: wlen - whop + 1 (truncation gives 0, flooring -1) and wlen - whop - 1 (-1 against -2: a partial frame or
    nothing at all)"""
    m = {0, 1, wlen - 1, wlen, wlen + 1, wlen + whop - 1, wlen + whop, wlen + whop + 1, 3 * wlen + 1}
    if whop >= 2:
        m |= {wlen - whop + 1, wlen - whop - 1}
    return sorted(v for v in m if v >= 0)


def random_table(wlen, seed=21):
    return np.random.default_rng(seed + wlen).uniform(0.5, 1.5, size=wlen)
