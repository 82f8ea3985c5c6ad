"""``train`` / ``test`` entry points of the reference's HMM/main.py (:46-197) on the MI355X engine,
``codebook``, the LBG training of the codebook they read, and ``features``, the frame files both read (the
reference's CodeVector pipeline).

    python -m hmm_training_amd.main train [--max-iterations 2] [--data ../Data]
    python -m hmm_training_amd.main test  [--data ../Data]
    python -m hmm_training_amd.main codebook --frames PATH [PATH ...] --out codevector.json
                                             [--centroids 256 --max-iterations 100 --epsilon 0.001]
    python -m hmm_training_amd.main features --signals PATH.npy [PATH.npy ...] --out-dir DIR
    python -m hmm_training_amd.main preprocess --wav PATH.wav [PATH.wav ...] --out-dir DIR
    python -m hmm_training_amd.main recognise --wav PATH.wav [PATH.wav ...] [--models DIR] [--data ../Data]

Same on-disk layout as the reference:
* ``<data>/CodeVector/codevector.json`` — the codebook;
* ``<data>/<TrainHMM|Test>/<word>/<recording>/*_frames.json`` — the recordings;
* ``<data>/ResultsHMM/<word>.json`` — the trained models (DataStorageHMM's default directory).

The same messages are printed, in the same order. Two things differ:
* training runs every word model together, one grouped E-step launch per EM iteration
  (``hmm_training_group``; each model still stops on its own rule, so the saved models equal the
  reference's word-by-word training); ``grouped=False`` trains word by word through the drop-in
  ``training_with_save``;
* testing goes through ``test_hmm`` (one scoring launch for all (recording, model) pairs).
The confusion-matrix plot (``create_confusion_matrix``, matplotlib) is out of scope; ``test``
returns the labels instead.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import logging
import sys
import os
import random
from collections import defaultdict
from pathlib import Path
from typing import Dict, List, Optional

from .hmm_classes import DataStorageHMM, HMMTrained
from .hmm_testing import test_hmm
from .hmm_training import get_observations, hmm_training_group, training_with_save
from .io import Centroid, Frame, load_centroids, load_frames, save_centroids

logger = logging.getLogger(__name__)


def load_all_recordings_by_word(base_dir="../Data", purpose="TrainHMM", print_messages=True,
                                print_summary=True) -> Dict[str, List[List[Frame]]]:
    """{word: [recording frames, ...]} from ``<base_dir>/<purpose>/<word>/<rec>/*_frames.json``
    (main.py:46-102; the first frame file of each recording directory, directory order)."""
    all_words: Dict[str, List[List[Frame]]] = defaultdict(list)
    purpose_path = Path(base_dir) / purpose
    if not purpose_path.exists():
        print(f"Warning: Directory {purpose_path} does not exist")
        return dict(all_words)
    if print_messages:
        print(f"Loading recordings from {purpose_path}")
    for word_dir in purpose_path.iterdir():
        if not word_dir.is_dir():
            continue
        if print_messages:
            print(f"  Processing word: {word_dir.name}")
        for recording_dir in word_dir.iterdir():
            if not recording_dir.is_dir():
                continue
            frame_files = list(recording_dir.glob("*_frames.json"))
            if frame_files:
                frames = load_frames(str(frame_files[0]))
                if print_messages:
                    print(f"  Loaded {len(frames)} frames from {frame_files[0]}")
                if frames:
                    all_words[word_dir.name].append(frames)
                    if print_messages:
                        print(f"    Added recording with {len(frames)} frames from {recording_dir.name}")
    result = dict(all_words)
    if print_summary:
        print("\nSummary:")
        print(f"  Total words: {len(result)}")
        for word, recordings in result.items():
            print(f"    {word}: {len(recordings)} recordings with {sum(len(r) for r in recordings)} total frames")
    return result


def load_mfcc_centroids(base_dir="../Data", print_messages=True) -> List[Centroid]:
    """The codebook ``<base_dir>/CodeVector/codevector.json`` (main.py:105-130), [] if absent."""
    path = os.path.join(base_dir, "CodeVector", "codevector.json")
    if not os.path.exists(path):
        return []
    centroids = load_centroids(path)
    if print_messages:
        print("\nLoading codevector:")
        print(f"  Loaded codevector with {len(centroids)} centroids")
        c = random.choice(centroids)
        print("  Example random centroid:")
        print(f"   id: {c.id}")
        print(f"   Power: {c.mfcc[0]:.3f}")
        print(" ".join(f"   {x:.3f}" for x in c.mfcc[1:]))
        print("\n")
    return centroids


def _train_grouped(recordings_by_word, centroids, show_progress, max_iterations, load_initial_params,
                   model_dir, n_states=4) -> Optional[List[HMMTrained]]:
    """All words in one group (hmm_training_group), printing each word's lines in word order exactly
    as the word-by-word loop does.  None when the grouped run cannot start (the caller then runs the
    word-by-word loop, which reproduces the reference's partial output and error for bad input)."""
    heads, obs_sets, words = [], [], []
    try:
        for word_name, word_recordings in recordings_by_word.items():
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                print(f"\nTraining HMM for word: '{word_name}' with {len(word_recordings)} recordings")
                print("Converting recordings to observations...")  # training_with_save, hmm_training.py:215-247
                observations = get_observations(word_recordings, centroids)
                print(f"Generated {len(observations)} observation sequences")
                print(f"Sequence lengths: {[len(obs) for obs in observations]}")
                print("Starting Baum-Welch training...")
            heads.append(buf.getvalue())
            obs_sets.append(observations)
            words.append(word_name)
        parts: List[str] = []
        results = hmm_training_group(obs_sets, N=n_states, M=len(centroids), max_iterations=max_iterations,
                                     show_progress=show_progress, word_names=words,
                                     load_initial_params=load_initial_params, stdout_parts=parts)
    except Exception:
        return None
    trained = []
    for i, word_name in enumerate(words):
        sys.stdout.write(heads[i] + parts[i])
        A, B, pi = results[i]
        model = HMMTrained(states=n_states, symbols=len(centroids), A=A, B=B, Pi=pi, word=word_name)
        if model_dir is None:
            DataStorageHMM.save_hmm(model, print_messages=False)
        else:
            DataStorageHMM.save_hmm(model, base_dir=model_dir, print_messages=False)
        trained.append(model)
        print(f"Model saved for word: '{model.word}'")
    return trained


def train_hmm(show_progress=True, max_iterations=100, load_initial_params=False, base_dir="../Data",
              model_dir: Optional[str] = None, grouped: bool = True) -> Optional[List[HMMTrained]]:
    """Train one HMM per word (main.py:133-164); None on any error, as the reference."""
    print("Starting HMM training for all words...")
    try:
        centroids = load_mfcc_centroids(base_dir, print_messages=False)
        print(f"Loaded {len(centroids)} centroids")
        recordings_by_word = load_all_recordings_by_word(base_dir, purpose="TrainHMM", print_messages=False)
        print(f"Loaded recordings for {len(recordings_by_word)} words")
        trained = None
        if grouped:
            trained = _train_grouped(recordings_by_word, centroids, show_progress, max_iterations,
                                     load_initial_params, model_dir)
        if trained is None:  # word by word (the reference's loop, main.py:147-152)
            trained = []
            words = recordings_by_word.items()
        else:
            words = ()
        for word_name, word_recordings in words:
            print(f"\nTraining HMM for word: '{word_name}' with {len(word_recordings)} recordings")
            model = training_with_save(word_recordings, centroids, word_name, max_iterations=max_iterations,
                                       show_progress=show_progress, load_initial_params=load_initial_params,
                                       base_dir=model_dir)
            trained.append(model)
            print(f"Model saved for word: '{model.word}'")
        print("\nHMM training completed successfully!")
        print(f"Total models trained: {len(trained)}")
        print(f"Words trained: {[h.word for h in trained]}")
        return trained
    except Exception as e:  # the reference logs and returns None (main.py:162-164)
        logger.error(f"Error during HMM training: {e}")
        return None


def test(show_progress=False, base_dir="../Data", model_dir: Optional[str] = None):
    """Classify the Test recordings with the saved models (main.py:167-197); returns
    (true_labels, predicted_labels), or None when there is nothing to test."""
    print("Loading trained HMM models...")
    all_hmm = DataStorageHMM.load_all_hmms(base_dir=model_dir) if model_dir else DataStorageHMM.load_all_hmms()
    if not all_hmm:
        print("No trained HMM models found. Please train models first.")
        return None
    print(f"Loaded {len(all_hmm)} HMM models for words: {[h.word for h in all_hmm]}")
    test_recordings = load_all_recordings_by_word(base_dir, purpose="Test", print_messages=False)
    print(f"Loaded test recordings for {len(test_recordings)} words")
    trained_words = {h.word for h in all_hmm}
    filtered = {w: r for w, r in test_recordings.items() if w in trained_words}
    if not filtered:
        print("No test recordings found for trained words.")
        return None
    print(f"Testing on {len(filtered)} words: {list(filtered.keys())}")
    true_labels, predicted = test_hmm(all_hmm, filtered, base_dir=base_dir, show_progress=show_progress)
    return true_labels, predicted


def codebook(frame_paths: List[str], out: str, centroids_quantity: int = 256, max_iterations: int = 100,
             epsilon: float = 0.001) -> List[Centroid]:
    """Train the codebook on the frames of every ``*_frames.json`` in ``frame_paths`` (createCodeVector on the
    GPU) and write it to ``out`` in the codevector.json format."""
    from .codevector import createCodeVector
    frames: List[Frame] = []
    for path in frame_paths:
        loaded = load_frames(path)
        print(f"Loaded {len(loaded)} frames from {path}")
        frames.extend(loaded)
    centroids, _ = createCodeVector(frames, centroids_quantity=centroids_quantity, max_iterations=max_iterations,
                                    epsilon=epsilon, save_updates=False)
    out_dir = os.path.dirname(os.path.abspath(out))
    os.makedirs(out_dir, exist_ok=True)
    save_centroids(out, centroids)
    print(f"Saved {len(centroids)} centroids to {out}")
    return centroids


def features(signal_paths: List[str], out_dir: str, sample_rate: int = 16000) -> List[str]:
    """Frame every processed signal (``Data/Processed/<word>/*.npy``) and compute its frames' MFCC on the GPU; write
    ``<out_dir>/<stem>_frames.json`` with the fields of RawDataMFCC.to_dict (codevector_classes.py:252-264), which
    ``codebook`` and ``load_all_recordings_by_word`` read.  Returns the paths written."""
    import json

    import numpy as np

    from .frontend import frame_table, mfcc_recordings
    signals = [np.asarray(np.load(p)).astype(float).flatten() for p in signal_paths]
    rows = mfcc_recordings(signals, sample_rate=sample_rate)
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for path, sig, mf in zip(signal_paths, signals, rows):
        stem = Path(path).stem
        starts, lengths = frame_table(len(sig))
        data = [{"raw_samples": sig[a:a + n].tolist(), "sample_rate": sample_rate, "n_channels": 1,
                 "frame_duration_ms": 20.0, "mfcc_vector": mf[i].tolist(), "parent_centroid_id": 0, "generation": 0,
                 "frame_number": i, "recording": stem} for i, (a, n) in enumerate(zip(starts, lengths))]
        out = os.path.join(out_dir, f"{stem}_frames.json")
        with open(out, "w") as fh:
            json.dump(data, fh, indent=2)
        print(f"    Saved {len(data)} frames to {out}")
        written.append(out)
    return written


def _read_16k(wav_paths: List[str], sample_rate: int = 16000):
    """The int16 samples of every file, or None (with a message) when one is not at ``sample_rate``: the reference
    resamples such a file in place (check_metadata), which is out of scope here."""
    from .io import read_wav
    signals = []
    for path in wav_paths:
        samples, rate = read_wav(path)
        if rate != sample_rate:
            print(f"{path}: sample rate {rate} Hz, not {sample_rate} Hz; resample it first (not done here)")
            return None
        signals.append(samples)
    return signals


def preprocess(wav_paths: List[str], out_dir: str, sample_rate: int = 16000) -> Optional[List[str]]:
    """The reference's preemphasis.py on the GPU: filter and trim every ``.wav`` recording and write
    ``<out_dir>/<stem>.npy``, the (m, 1) float64 array the reference saves under Data/Processed, which ``features``
    reads.  None when a file is refused."""
    import numpy as np

    from .frontend import preprocess_recordings
    signals = _read_16k(wav_paths, sample_rate)
    if signals is None:
        return None
    trimmed, bounds = preprocess_recordings(signals, sample_rate=sample_rate, mode="batch")
    os.makedirs(out_dir, exist_ok=True)
    written = []
    for path, t, b in zip(wav_paths, trimmed, bounds):
        out = os.path.join(out_dir, f"{Path(path).stem}.npy")
        np.save(out, t)
        print(f"    Saved samples [{int(b[0])}, {int(b[1])}) of {path} to {out}")
        written.append(out)
    return written


def recognise(wav_paths: List[str], base_dir="../Data", model_dir: Optional[str] = None, sample_rate: int = 16000):
    """HMM/live_testing.main for recordings on disk: live-mode conditioning, symbols, every model's log-likelihood, and
    its two printed lines per recording.  Returns (scores, ranking) or None."""
    from .hmm_testing import recognise_recordings
    all_hmm = DataStorageHMM.load_all_hmms(base_dir=model_dir) if model_dir else DataStorageHMM.load_all_hmms()
    if not all_hmm:
        print("No trained HMM models found. Please train models first.")
        return None
    centroids = load_mfcc_centroids(base_dir, print_messages=False)
    signals = _read_16k(wav_paths, sample_rate)
    if signals is None:
        return None
    scores, ranking = recognise_recordings(signals, all_hmm, centroids, mode="live", sample_rate=sample_rate)
    words = [h.word for h in all_hmm]
    for path, row, order in zip(wav_paths, scores, ranking):
        if len(wav_paths) > 1:
            print(path)
        by_word = dict(zip(words, row))
        print("Likelihoods ")
        print(" ".join(f"{w}: {float(by_word[w]):.3f}" for w in words), end=" ")
        print("\n")
        print("Sorted: ")
        print(" ".join(f"{w}: {float(by_word[w]):.3f}" for w in order), end=" ")
        print("\n")
    return scores, ranking


def _cli(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("command", choices=["train", "test", "codebook", "features", "preprocess", "recognise"])
    ap.add_argument("--wav", nargs="+", default=None, help="preprocess, recognise: raw 16 kHz recordings (.wav)")
    ap.add_argument("--data", default="../Data")
    ap.add_argument("--models", default=None, help="model directory (default: DataStorageHMM's)")
    # `python main.py train` runs train_hmm(show_progress=True, max_iterations=2) (HMM/main.py:268);
    # codebook: createCodeVector's default of 100
    ap.add_argument("--max-iterations", type=int, default=None)
    ap.add_argument("--load-initial-params", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--frames", nargs="+", default=None, help="codebook: *_frames.json files to train on")
    ap.add_argument("--out", default=None, help="codebook: the codevector.json to write")
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--epsilon", type=float, default=0.001)
    ap.add_argument("--signals", nargs="+", default=None, help="features: processed signals (.npy)")
    ap.add_argument("--out-dir", default=None, help="features: where the <stem>_frames.json files go")
    ap.add_argument("--sample-rate", type=int, default=16000)
    a = ap.parse_args(argv)
    if a.command == "features":
        if not a.signals or not a.out_dir:
            ap.error("features needs --signals and --out-dir")
        features(a.signals, a.out_dir, sample_rate=a.sample_rate)
        return 0
    if a.command == "preprocess":
        if not a.wav or not a.out_dir:
            ap.error("preprocess needs --wav and --out-dir")
        return 0 if preprocess(a.wav, a.out_dir, sample_rate=a.sample_rate) is not None else 1
    if a.command == "recognise":
        if not a.wav:
            ap.error("recognise needs --wav")
        return 0 if recognise(a.wav, base_dir=a.data, model_dir=a.models, sample_rate=a.sample_rate) is not None else 1
    if a.command == "codebook":
        if not a.frames or not a.out:
            ap.error("codebook needs --frames and --out")
        codebook(a.frames, a.out, centroids_quantity=a.centroids,
                 max_iterations=100 if a.max_iterations is None else a.max_iterations, epsilon=a.epsilon)
        return 0
    if a.max_iterations is None:
        a.max_iterations = 2
    if a.command == "train":
        ok = train_hmm(show_progress=not a.quiet, max_iterations=a.max_iterations,
                       load_initial_params=a.load_initial_params, base_dir=a.data, model_dir=a.models)
        return 0 if ok is not None else 1
    res = test(base_dir=a.data, model_dir=a.models)
    if res is None:
        return 1
    t, p = res
    acc = sum(x == y for x, y in zip(t, p)) / max(len(t), 1)
    print(f"Accuracy: {100.0 * acc:.2f}% ({len(t)} recordings)")
    return 0


if __name__ == "__main__":
    raise SystemExit(_cli())
