#!/usr/bin/env python3
"""Generate tests/golden/preprocess.npz and tests/golden/preprocess_rates.npz from the REFERENCE implementation.

Like make_golden.py this runs ONLY where the reference tree is mounted read-only at /root/reference.  It imports the
reference's own ``preemphasis.py`` and ``HMM/live_testing.py`` with empty stand-ins for the modules they import and
never call on this path (``librosa``, ``soundfile``, ``spectrum``, ``seaborn``, ``sounddevice``, ``wavio``,
``sklearn.metrics``; matplotlib on the ``Agg`` backend) and runs, for every input of tests/preprocess_ref.golden_inputs:

* batch mode: ``preemphasis.filter_signal`` then ``preemphasis.slice_signal``;
* live mode: ``live_testing.do_preemphasis`` (its plot switched off), and ``live_testing.slice_signal`` once more for
  the bounds, which do_preemphasis does not return.

slice_signal keeps zcr and power to itself; they are recorded as the arguments of its own ``np.max`` calls, through a
stand-in for the module's ``np`` that passes everything else on to NumPy.

Recorded per case: the input, both modes' bounds, zcr, power, the batch-mode trimmed signal and the live-mode windowed
signal.  preprocess_rates.npz holds the same for tests/preprocess_ref.rate_inputs: recordings at 8000, 22050 and
44100 Hz, whose frames are (160, 80), (441, 220) and (882, 441) samples.  There the reference's ``hamming_window``
raises ValueError where the trimmed signal is shorter than its 320-sample table and yet has a full frame by its count
(192 < m < 320): such a case records ``windowed_raised = 1`` and no windowed signal.  Only the resulting ``.npz`` data
files travel.  Regenerate with:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_preprocess.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))  # tests/: the inputs

import preprocess_ref as R  # noqa: E402


def _import_reference():
    sys.dont_write_bytecode = True
    import matplotlib
    matplotlib.use("Agg")
    for name in ("librosa", "soundfile", "spectrum", "seaborn", "sounddevice", "wavio", "sklearn", "sklearn.metrics"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["spectrum"].poly2lsf = lambda *a, **k: None
    sys.modules["spectrum"].lsf2poly = lambda *a, **k: None
    for name in ("confusion_matrix", "classification_report", "accuracy_score"):
        setattr(sys.modules["sklearn.metrics"], name, lambda *a, **k: None)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "HMM"))
    import preemphasis  # noqa: E402
    import live_testing  # noqa: E402
    return preemphasis, live_testing


P, LT = _import_reference()


class _RecordingNumpy:
    """NumPy, but np.max remembers what it was given"""

    def __init__(self):
        self.seen = []

    def max(self, a, *args, **kw):
        self.seen.append(np.array(a, copy=True))
        return np.max(a, *args, **kw)

    def __getattr__(self, name):
        return getattr(np, name)


def run_reference(x, sr=R.SR):
    n = x.shape[0]
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        y = P.filter_signal(x, n)["filtered_signal"]
        b = P.slice_signal(y, sr, n)
        rec = _RecordingNumpy()
        LT.np = rec
        try:
            l = LT.slice_signal(y, sr, n)
        finally:
            LT.np = np
        LT.display_graphs = lambda *a, **k: None
        try:
            windowed = LT.do_preemphasis(x, sr)
        except ValueError:  # hamming_window: a full frame of 320 over a shorter trimmed signal
            windowed = None
    zcr, power = rec.seen[0], rec.seen[1]  # max_zcr = 0.08 * np.max(zcr); max_power = 0.15 * np.max(power)
    out = dict(zcr=zcr.reshape(-1), power=power.reshape(-1), batch_bounds=np.array([b["start_idx"], b["finish_idx"]], np.int64),
               live_bounds=np.array([l["start_idx"], l["finish_idx"]], np.int64),
               batch_trimmed=np.asarray(b["trimmed_signal"], dtype=np.float64))
    if windowed is not None:
        out["live_windowed"] = np.asarray(windowed, dtype=np.float64)
    return out


def main():
    arrays, names = {}, []
    for name, x in R.golden_inputs():
        ref = run_reference(x)
        names.append(name)
        arrays[f"{name}/input"] = x
        for k, v in ref.items():
            arrays[f"{name}/{k}"] = v
        print(f"[golden] {name}: batch {ref['batch_bounds'].tolist()} live {ref['live_bounds'].tolist()} "
              f"frames {len(ref['zcr'])}")
    path = os.path.join(OUT, "preprocess.npz")
    np.savez_compressed(path, names=np.array(names, dtype=str), **arrays)
    print(f"[golden] wrote {path}: {os.path.getsize(path)} bytes")
    arrays, names = {}, []
    for name, sr, x in R.rate_inputs():
        ref = run_reference(x, sr)
        names.append(name)
        arrays[f"{name}/input"] = x
        arrays[f"{name}/sample_rate"] = np.int64(sr)
        arrays[f"{name}/windowed_raised"] = np.int64("live_windowed" not in ref)
        for k, v in ref.items():
            arrays[f"{name}/{k}"] = v
        print(f"[golden] {name}: batch {ref['batch_bounds'].tolist()} live {ref['live_bounds'].tolist()} "
              f"frames {len(ref['zcr'])} windowed {'raised' if 'live_windowed' not in ref else 'ok'}")
    path = os.path.join(OUT, "preprocess_rates.npz")
    np.savez_compressed(path, names=np.array(names, dtype=str), **arrays)
    print(f"[golden] wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
