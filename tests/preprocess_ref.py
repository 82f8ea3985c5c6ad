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


def preprocess(x, factors, window=False, sr=SR):
    """dict: y, zcr, power, start, finish, else_branch, out (the trimmed, optionally windowed signal)"""
    win, hop = int(0.02 * sr), int(0.01 * sr)
    y = filter_signal(x)
    zcr, power = frame_stats(y, win, hop)
    start, finish, other = bounds_of(zcr, power, factors, hop)
    out = y[start:finish].copy()
    if window:
        out = window_overlap(out)
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
