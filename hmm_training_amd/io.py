"""On-disk formats either side of the path: the codebook and per-recording
frame JSON written by the reference's CodeVector pipeline.

* codevector.json: ``[{"mfcc": [...13], "id": k}, ...]`` (codevector_classes.py:321-342, 548-556)
* ``*_frames.json``: ``[{"raw_samples": [...], "mfcc_vector": [...13], ...}, ...]``
  (codevector_classes.py:251-279, 477-495).

The reference's RawDataMFCC.__post_init__ recomputes every frame's MFCC with librosa each time a frame file is
loaded (codevector_classes.py:217-224) and so ignores the stored ``mfcc_vector``.  ``load_frames`` uses the stored
vector by default (stated deviation: no work, and files without raw samples load); ``recompute_mfcc=True`` does what
the reference does, on the GPU (frontend.mfcc_frames).
"""
from __future__ import annotations

import json
from dataclasses import dataclass, field
from typing import List

import numpy as np


@dataclass
class Centroid:
    mfcc: np.ndarray = field(default_factory=lambda: np.zeros(13))
    id: int = 0


@dataclass
class Frame:
    mfcc: np.ndarray
    frame_number: int = 0
    recording: str = ""


def load_centroids(path: str) -> List[Centroid]:
    with open(path) as fh:
        data = json.load(fh)
    return [Centroid(mfcc=np.asarray(d["mfcc"], dtype=np.float64).reshape(-1), id=d.get("id", i))
            for i, d in enumerate(data)]


def save_centroids(path: str, centroids) -> None:
    """Write the codebook as DataStorage.save_centroids does (codevector_classes.py:548-556): a JSON list of
    CentroidDataMFCC.to_dict() = ``{"mfcc": [...], "id": k}`` (:321-326) with indent 2, which load_centroids reads."""
    data = [{"mfcc": np.asarray(c.mfcc, dtype=np.float64).reshape(-1).tolist(), "id": int(c.id)} for c in centroids]
    with open(path, "w") as fh:
        json.dump(data, fh, indent=2)


def read_wav(path: str):
    """(samples int16 [n, channels], framerate) of a 16-bit PCM .wav file, with the standard library's ``wave`` as
    the reference's open_file / assing_step_time read it (preemphasis.py:127-170)."""
    import wave
    with wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2:
            raise ValueError(f"{path}: {8 * w.getsampwidth()}-bit samples; 16-bit PCM is what the reference reads")
        channels, rate = w.getnchannels(), w.getframerate()
        raw = w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype="<i2").astype(np.int16).reshape(-1, channels), rate


def load_frames(path: str, recompute_mfcc: bool = False) -> List[Frame]:
    """The frames of a ``*_frames.json``.  ``recompute_mfcc``: every frame's MFCC is computed from its ``raw_samples``
    at its ``sample_rate`` (RawDataMFCC.__post_init__, :217-224; a frame without samples keeps its stored vector)."""
    with open(path) as fh:
        data = json.load(fh)
    frames = [Frame(mfcc=np.asarray(d["mfcc_vector"], dtype=np.float64).reshape(-1),
                    frame_number=d.get("frame_number", 0), recording=d.get("recording", "")) for d in data]
    if recompute_mfcc:
        from .frontend import mfcc_frames
        by_rate = {}
        for i, d in enumerate(data):
            if len(d.get("raw_samples", ())) > 0:
                by_rate.setdefault(d.get("sample_rate", 16000), []).append(i)
        for rate, idx in by_rate.items():
            rows = mfcc_frames([np.asarray(data[i]["raw_samples"]) for i in idx], sample_rate=rate)
            for i, row in zip(idx, rows):
                frames[i].mfcc = row.copy()
    return frames
