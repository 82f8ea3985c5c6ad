"""hmm_training_amd — MI355X-native Baum-Welch trainer for discrete HMMs.

Drop-in for DemianMArin/HMM_Training's HMM/hmm_training.py, hmm_classes.py and hmm_testing.py;
the EM hot path runs in hand-written gfx950 HIP kernels behind the C ABI of include/hmmbw.h.
"""
from .hmm_classes import DataStorageHMM, HMMTrained  # noqa: F401

__all__ = ["HMMTrained", "DataStorageHMM", "hmm_training", "training_with_save", "get_observations",
           "calculate_log_likelihood", "viterbi_decode", "posterior_decode", "decode_words", "align_words",
           "BaumWelchEngine",
           "lbg_train",
           "createCodeVector", "save_centroids", "train_connected", "frame_table", "mfcc_frames", "mfcc_recordings",
           "encode_recordings", "with_optional", "read_wav", "preprocess_recordings", "encode_raw_recordings",
           "recognise_recordings"]


def __getattr__(name):
    # the engine-backed entry points load libhmmbw.so (and torch) lazily
    if name in ("hmm_training", "training_with_save", "get_observations", "safe_log", "safe_exp", "log_sum_exp",
                "train_connected", "with_optional"):
        from . import hmm_training as _ht
        return getattr(_ht, name)
    if name in ("calculate_log_likelihood", "score_matrix", "test_hmm", "viterbi_decode", "posterior_decode",
                "decode_words", "align_words", "segments_from_path"):
        from . import hmm_testing as _te
        return getattr(_te, name)
    if name in ("lbg_train", "createCodeVector", "LBGResult"):
        from . import codevector as _cv
        return getattr(_cv, name)
    if name in ("frame_table", "mfcc_frames", "mfcc_recordings", "encode_recordings", "preprocess_recordings",
                "encode_raw_recordings"):
        from . import frontend as _fe
        return getattr(_fe, name)
    if name == "recognise_recordings":
        from .hmm_testing import recognise_recordings
        return recognise_recordings
    if name == "read_wav":
        from .io import read_wav
        return read_wav
    if name == "save_centroids":
        from .io import save_centroids
        return save_centroids
    if name == "BaumWelchEngine":
        from .engine import BaumWelchEngine
        return BaumWelchEngine
    raise AttributeError(name)
