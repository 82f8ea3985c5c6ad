"""Forward-only scoring, the drop-in for HMM/hmm_testing.py (calculate_log_likelihood :49-104,
test_hmm :107-163), on the MI355X engine.

``score_matrix`` is the batched form: every (sequence, model) log-likelihood in one grouped HIP launch,
instead of the reference's per-pair Python forward pass.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from .engine import BaumWelchEngine, EngineGroup
from .hmm_classes import HMMTrained
from .hmm_training import _check_optional, get_observations, transcript_ids


def score_matrix(observations: Sequence[np.ndarray], models: Sequence[HMMTrained], device=None) -> np.ndarray:
    """[len(observations), len(models)] log P(O_r | model_m) (hmm_testing.py:49-104 per entry).

    Models of one shape (N, M, resolved topology) are scored together by ONE grouped launch over all
    (sequence, model) pairs (hmmbw_group_score); a model the grouped kernel does not take (N > 16,
    tables too large for LDS) gets its own launch."""
    out = np.full((len(observations), len(models)), -np.inf)
    if len(observations) == 0 or len(models) == 0:
        return out
    engines = []
    try:
        for hmm in models:
            N, M = int(hmm.states), int(np.asarray(hmm.B).shape[1])
            eng = BaumWelchEngine(N, M, device=device)
            engines.append(eng)
            eng.set_observations(observations)
            eng.set_params(np.asarray(hmm.Pi), np.asarray(hmm.A), np.asarray(hmm.B))
        buckets = {}
        for m, eng in enumerate(engines):
            key = (eng.N, eng.M, eng.topology) if eng.N <= 16 else ("single", m)
            buckets.setdefault(key, []).append(m)
        for members in buckets.values():
            try:
                grp = EngineGroup([engines[m] for m in members])
            except Exception:
                grp = None
            if grp is None:
                for m in members:
                    out[:, m] = engines[m].score()
                continue
            with grp:
                for m, col in zip(members, grp.score()):
                    out[:, m] = col
    finally:
        for eng in engines:
            eng.close()
    return out


def viterbi_decode(observations: Sequence[np.ndarray], hmm: HMMTrained, device=None) -> Tuple[List[np.ndarray], np.ndarray]:
    """(paths, logp): the most likely state sequence of every recording under one model and its
    log-probability, all sequences in one launch (BaumWelchEngine.viterbi).  A sequence no path explains has
    logp -inf and a path of -1."""
    if len(observations) == 0:
        return [], np.zeros(0)
    N, M = int(hmm.states), int(np.asarray(hmm.B).shape[1])
    with BaumWelchEngine(N, M, device=device) as eng:
        eng.set_observations(observations)
        eng.set_params(np.asarray(hmm.Pi), np.asarray(hmm.A), np.asarray(hmm.B))
        return eng.viterbi()


def posterior_decode(observations: Sequence[np.ndarray], hmm: HMMTrained,
                     device=None) -> Tuple[List[np.ndarray], List[np.ndarray], np.ndarray]:
    """(gammas, paths, logp): the smoothed state posteriors gamma_t(i) = P(q_t = i | O, lambda) of every recording
    under one model as host [T_r, N] arrays, the state with the largest gamma at every step, and log P(O | lambda),
    all sequences in one launch (BaumWelchEngine.posterior).  A sequence with P(O) = 0 has logp -inf, zero rows
    and a path of -1."""
    if len(observations) == 0:
        return [], [], np.zeros(0)
    N, M = int(hmm.states), int(np.asarray(hmm.B).shape[1])
    with BaumWelchEngine(N, M, device=device) as eng:
        eng.set_observations(observations)
        eng.set_params(np.asarray(hmm.Pi), np.asarray(hmm.A), np.asarray(hmm.B))
        gamma, paths, logp = eng.posterior()
        return np.split(gamma.cpu().numpy(), eng._offsets[1:-1]), paths, logp


def segments_from_path(path: np.ndarray, starts: np.ndarray, N: int, words: Sequence) -> List[Tuple[object, int, int]]:
    """[(word, start_frame, end_frame_exclusive), ...] of one decoded sequence: a segment opens at every frame whose
    start flag is set and carries the word of its composite state (path[t] // N).  A repeated word gives two
    segments, a held word one.  A sequence without a path (all -1) has no segments."""
    path, starts = np.asarray(path), np.asarray(starts)
    if path.size == 0 or path[0] < 0:
        return []
    first = np.flatnonzero(starts)
    ends = np.append(first[1:], path.size)
    return [(words[int(path[s]) // N], int(s), int(e)) for s, e in zip(first, ends)]


def decode_words(observations: Sequence[np.ndarray], models: Sequence[HMMTrained], word_init=None, word_trans=None,
                 end_final: bool = True, device=None) -> Tuple[List[List[Tuple[object, int, int]]], np.ndarray]:
    """(segments, logp): which words were spoken, and where, in every recording: the best path through a loop of the
    word models, all sequences in one launch (BaumWelchEngine.wordnet_decode).  segments[r] lists (word,
    start_frame, end_frame_exclusive) with the models' .word names.  word_init [W] and word_trans [W, W] are
    non-negative weights (a grammar and a word-insertion penalty; None: all ones).  The models must share one shape."""
    if len(observations) == 0:
        return [], np.zeros(0)
    if len(models) == 0:
        raise ValueError("no word models")
    N, M = int(models[0].states), int(np.asarray(models[0].B).shape[1])
    for hmm in models:
        if int(hmm.states) != N or np.asarray(hmm.B).shape != (N, M) or np.asarray(hmm.A).shape != (N, N):
            raise ValueError("connected-word decoding needs word models of one shape (N states, M symbols)")
    pi = np.stack([np.asarray(h.Pi, dtype=np.float64).reshape(N) for h in models])
    A = np.stack([np.asarray(h.A, dtype=np.float64) for h in models])
    B = np.stack([np.asarray(h.B, dtype=np.float64) for h in models])
    words = [h.word for h in models]
    with BaumWelchEngine(N, M, device=device) as eng:
        eng.set_observations(observations)
        paths, starts, logp = eng.wordnet_decode(pi, A, B, word_init, word_trans, end_final=end_final)
    return [segments_from_path(p, s, N, words) for p, s in zip(paths, starts)], logp


def align_words(observations: Sequence[np.ndarray], transcripts: Sequence[Sequence], models: Sequence[HMMTrained],
                end_final: bool = True, device=None, optional=None) -> Tuple[List[List[Tuple[object, int, int]]], np.ndarray]:
    """(segments, logp): where each word of a known utterance lies: the best path of every recording through the
    chain of the word models its transcript names, all sequences in one launch (BaumWelchEngine.align).
    transcripts[r] lists the models' .word names spoken in recording r, as train_connected takes them.  segments[r]
    lists (word, start_frame, end_frame_exclusive), one per transcript position, in order; it is [] where no path
    explains the recording (logp -inf; a recording shorter than its transcript is one).  end_final: every
    recording ends in the last state of its last word, as train_connected and decode_words assume by default.
    optional: one boolean sequence per transcript, True where the position may be passed over (with_optional builds
    the usual `sil? one sil? two sil?`); a position the path passes over gives no segment, and a segment ends where
    the next visited position starts.  The models must share one shape."""
    if len(models) == 0:
        raise ValueError("no word models")
    N, M = int(models[0].states), int(np.asarray(models[0].B).shape[1])
    for hmm in models:
        if int(hmm.states) != N or np.asarray(hmm.B).shape != (N, M) or np.asarray(hmm.A).shape != (N, N):
            raise ValueError("forced alignment needs word models of one shape (N states, M symbols)")
    if len(transcripts) != len(observations):
        raise ValueError(f"{len(transcripts)} transcripts for {len(observations)} recordings")
    ids = transcript_ids(transcripts, models)
    _check_optional(optional, transcripts)
    if len(observations) == 0:
        return [], np.zeros(0)
    pi = np.stack([np.asarray(h.Pi, dtype=np.float64).reshape(N) for h in models])
    A = np.stack([np.asarray(h.A, dtype=np.float64) for h in models])
    B = np.stack([np.asarray(h.B, dtype=np.float64) for h in models])
    with BaumWelchEngine(N, M, device=device) as eng:
        eng.set_observations(list(observations))
        _, bounds, logp = eng.align(pi, A, B, ids, end_final=end_final, optional=optional)
    segments = []
    for r, (b, words) in enumerate(zip(bounds, ids)):
        if logp[r] == -np.inf:
            segments.append([])
            continue
        seen = np.flatnonzero(b >= 0)          # the visited positions
        ends = np.append(b[seen][1:], len(observations[r]))
        segments.append([(models[words[l]].word, int(b[l]), int(e)) for l, e in zip(seen, ends)])
    return segments, logp


def recognise_recordings(signals: Sequence, models: Sequence[HMMTrained], centroids, mode: str = "live",
                         sample_rate: int = 16000, device=None) -> Tuple[np.ndarray, List[list]]:
    """(scores [R, W], ranking): HMM/live_testing.main from do_preemphasis to the sorted dictionary, without the
    microphone and for any number of recordings: raw recording -> conditioning -> frames -> MFCC -> symbols
    (frontend.encode_raw_recordings) -> log P(O | model) of every model (score_matrix, one launch).  ranking[r] lists
    the models' .word names by descending score; ties keep the models' order, as Python's stable sort keeps the
    dictionary's.  A recording that trims to no frame has no observation: its row is -inf throughout and it takes no
    part in the scoring launch."""
    from .frontend import encode_raw_recordings
    obs = encode_raw_recordings(signals, centroids, mode=mode, sample_rate=sample_rate, device=device)
    scores = np.full((len(obs), len(models)), -np.inf)
    live = [r for r, o in enumerate(obs) if len(o) > 0]
    if live and len(models):
        scores[live] = score_matrix([obs[r] for r in live], models, device=device)
    words = [h.word for h in models]
    ranking = [[words[m] for m in sorted(range(len(words)), key=lambda m: row[m], reverse=True)] for row in scores]
    return scores, ranking


def calculate_log_likelihood(recording_observations: np.ndarray, hmm: HMMTrained) -> float:
    """log P(O | lambda) of one sequence under one linear-domain model (hmm_testing.py:49-104)."""
    return float(score_matrix([np.asarray(recording_observations)], [hmm])[0, 0])


def test_hmm(all_hmm: List[HMMTrained], test_recordings_dict: Dict[str, list], base_dir="../Data",
             show_progress=False, centroids=None) -> Tuple[List[str], List[str]]:
    """Classify every test recording by the max forward log-likelihood (hmm_testing.py:107-163)."""
    print("Starting HMM testing...")
    if centroids is None:
        from .io import load_centroids
        centroids = load_centroids(os.path.join(base_dir, "CodeVector", "codevector.json"))
    print("Phase 1: Converting recordings to observations...")
    observations: Dict[str, List[np.ndarray]] = {}
    for word, recordings in test_recordings_dict.items():
        print(f"  Converting {len(recordings)} recordings for word: '{word}'")
        observations[word] = get_observations(recordings, centroids)
    print("Phase 2: Testing all recording-HMM combinations...")
    true_labels, predicted = [], []
    for true_word, obs_list in observations.items():
        print(f"Testing {len(obs_list)} recordings for word: '{true_word}'")
        scores = score_matrix(obs_list, all_hmm) if obs_list else np.zeros((0, len(all_hmm)))
        for r in range(len(obs_list)):
            best, pred = -float("inf"), None
            for m, hmm in enumerate(all_hmm):
                if scores[r, m] > best:  # strict '>' keeps the first best model (:151)
                    best, pred = scores[r, m], hmm.word
            if show_progress:
                print(f"  Recording {r + 1} likelihoods: {dict(zip([h.word for h in all_hmm], scores[r]))}")
                print(f"  True: '{true_word}' -> Predicted: '{pred}'")
            true_labels.append(true_word)
            predicted.append(pred if pred else "unknown")
    return true_labels, predicted
