"""CTC beam-search decoding with an n-gram language model: host mirror of the reference's `kenlm_directory` branch
(speechless/net.py:171-177, 444-451) over libspeechless_host.so (csrc_host/beam_search.cpp).

A KenLM directory of the reference holds a `vocabulary` file -- one line with the allowed characters, compared (lower-
cased) against the net's alphabet at construction (net.py:171-177) -- and the language model for the patched
TensorFlow.  KenLM's binary format cannot be read without KenLM, so this implementation takes the model as an ARPA
file in the same directory (`lm.arpa`, or the only `*.arpa` there).
"""
import ctypes
from pathlib import Path

import numpy as np

from ._host_lib import host_lib

# net.py:447-450
KENLM_WEIGHT = .8
WORD_COUNT_WEIGHT = 0.
VALID_WORD_COUNT_WEIGHT = 2.3
DEFAULT_BEAM_WIDTH = 100  # tf.nn.ctc_beam_search_decoder's default


def _lib():
    return host_lib()


class NGramLanguageModel:
    """ARPA n-gram model with back-off (what KenLM's FullScore().prob returns, log10)."""

    def __init__(self, arpa_path):
        err = ctypes.create_string_buffer(512)
        self._lib = _lib()
        self._handle = self._lib.sl_host_lm_load_arpa(str(arpa_path).encode("utf8"), err, len(err))
        if not self._handle:
            raise ValueError("cannot load language model: {}".format(err.value.decode("utf8", "replace")))
        self.order = self._lib.sl_host_lm_order(self._handle)

    def score(self, sentence):
        """log10 P(<s> sentence </s>), like kenlm.Model.score."""
        return float(self._lib.sl_host_lm_score_sentence(self._handle, sentence.encode("utf8")))

    def __del__(self):
        if getattr(self, "_handle", None):
            self._lib.sl_host_lm_free(self._handle)
            self._handle = None


def expected_characters(kenlm_directory):
    """net.py:171-174: the single line of <kenlm_directory>/vocabulary, lower-cased, as a character list."""
    lines = (Path(kenlm_directory) / "vocabulary").read_text(encoding="utf8").splitlines()
    if len(lines) != 1:
        raise AssertionError("Expected exactly one line in {}".format(Path(kenlm_directory) / "vocabulary"))
    return list(lines[0].lower())


def find_arpa(kenlm_directory):
    directory = Path(kenlm_directory)
    if (directory / "lm.arpa").exists():
        return directory / "lm.arpa"
    candidates = sorted(directory.glob("*.arpa"))
    if len(candidates) != 1:
        raise ValueError("{} must hold the language model as lm.arpa (or exactly one *.arpa file); KenLM binary models "
                         "cannot be read without KenLM".format(directory))
    return candidates[0]


class CtcBeamSearchDecoder:
    """tf.nn.ctc_beam_search_decoder over the net's probabilities, optionally scored by a language model."""

    def __init__(self, allowed_characters, language_model=None, beam_width=DEFAULT_BEAM_WIDTH, merge_repeated=False,
                 kenlm_weight=KENLM_WEIGHT, word_count_weight=WORD_COUNT_WEIGHT,
                 valid_word_count_weight=VALID_WORD_COUNT_WEIGHT, epsilon=1e-8, threads=8):
        self._lib = _lib()
        self.allowed_characters = list(allowed_characters)
        self.beam_width = beam_width
        self.merge_repeated = merge_repeated
        self.epsilon = epsilon
        self.threads = threads
        self.language_model = language_model
        self._scorer = None
        if language_model is not None:
            alphabet = np.array([ord(c) for c in self.allowed_characters], dtype=np.uint32)
            self._scorer = self._lib.sl_host_scorer_create(language_model._handle, alphabet.ctypes.data, len(alphabet),
                                                           kenlm_weight, word_count_weight, valid_word_count_weight)

    @classmethod
    def from_kenlm_directory(cls, kenlm_directory, allowed_characters, **kw):
        return cls(allowed_characters, NGramLanguageModel(find_arpa(kenlm_directory)), **kw)

    def decode(self, probabilities, prediction_lengths):
        """probabilities: (B, T', K) float array; returns (list of index lists, log-probabilities (B,))."""
        probs = np.ascontiguousarray(probabilities, dtype=np.float32)
        b, t, k = probs.shape
        if k != len(self.allowed_characters) + 1:
            raise ValueError("{} classes for an alphabet of {} characters + blank".format(k, len(self.allowed_characters)))
        lengths = np.ascontiguousarray(np.asarray(prediction_lengths).reshape(-1), dtype=np.int32)
        out = np.empty((b, t), dtype=np.int32)
        out_len = np.empty((b,), dtype=np.int32)
        log_prob = np.empty((b,), dtype=np.float32)
        rc = self._lib.sl_host_ctc_beam_search(probs.ctypes.data, lengths.ctypes.data, b, t, k, k - 1, self.beam_width,
                                               1 if self.merge_repeated else 0, self.epsilon, self._scorer,
                                               out.ctypes.data, out_len.ctypes.data, log_prob.ctypes.data, self.threads)
        if rc != 0:
            raise ValueError("sl_host_ctc_beam_search rejected its arguments")
        return [list(map(int, out[i, :out_len[i]])) for i in range(b)], log_prob

    def __del__(self):
        if getattr(self, "_scorer", None):
            self._lib.sl_host_scorer_free(self._scorer)
            self._scorer = None


# limits of the device decoder (sl_ctc_beam_search, include/speechless_hip.h)
GPU_MAX_CLASSES = 64
GPU_MAX_BEAM_WIDTH = 128
GPU_MAX_LM_ORDER = 6


class BeamSearchLimitError(ValueError):
    """A shape or model outside what the GPU beam-search kernel supports."""


def export_scorer_tables(scorer_handle):
    """The host scorer flattened into numpy arrays (sl_host_scorer_export, include/speechless_host.h)."""
    lib = _lib()
    nodes, slots = ctypes.c_int64(), ctypes.c_int64()
    order, n_labels = ctypes.c_int(), ctypes.c_int()
    rc = lib.sl_host_scorer_export_sizes(scorer_handle, ctypes.byref(nodes), ctypes.byref(slots), ctypes.byref(order),
                                         ctypes.byref(n_labels))
    if rc != 0:
        raise ValueError("sl_host_scorer_export_sizes failed with status {} (-2: two characters of the alphabet are the "
                         "same code point)".format(rc))
    t = dict(trie_child=np.empty((nodes.value, n_labels.value), np.int32),
             trie_min=np.empty((nodes.value, n_labels.value), np.float32),
             trie_word=np.empty((nodes.value,), np.int32),
             ngrams=np.empty((slots.value, 8), np.uint32),
             params=np.empty((4,), np.float32), ids=np.empty((3,), np.int32))
    rc = lib.sl_host_scorer_export(scorer_handle, t["trie_child"].ctypes.data, t["trie_min"].ctypes.data,
                                   t["trie_word"].ctypes.data, t["ngrams"].ctypes.data, t["params"].ctypes.data,
                                   t["ids"].ctypes.data)
    if rc != 0:
        raise ValueError("sl_host_scorer_export failed with status {}".format(rc))
    t["order"] = order.value
    return t


def _upload_scorer(hip, characters, language_model, kenlm_weight, word_count_weight, valid_word_count_weight, device):
    """The host scorer over `characters`, flattened and uploaded: (dict of device tensors that keeps the memory alive,
    the BeamLm structure of their pointers and scalars)."""
    import torch
    host = CtcBeamSearchDecoder(characters, language_model, beam_width=1, kenlm_weight=kenlm_weight,
                                word_count_weight=word_count_weight, valid_word_count_weight=valid_word_count_weight)
    t = export_scorer_tables(host._scorer)
    dev = {name: torch.from_numpy(t[name].view(np.int32) if name == "ngrams" else t[name]).to(device)
           for name in ("trie_child", "trie_min", "trie_word", "ngrams")}
    p, ids = t["params"], t["ids"]
    lm = hip.BeamLm(dev["trie_child"].data_ptr(), dev["trie_min"].data_ptr(), dev["trie_word"].data_ptr(),
                    dev["ngrams"].data_ptr(), t["trie_word"].shape[0], t["ngrams"].shape[0], t["order"],
                    int(ids[0]), int(ids[1]), int(ids[2]), float(p[0]), float(p[1]), float(p[2]), float(p[3]))
    return dev, lm


def _check_gpu_limits(k, beam_width, language_model):
    if not 2 <= k <= GPU_MAX_CLASSES:
        raise BeamSearchLimitError("the GPU beam search takes 2..{} classes (one lane each), not {}".format(
            GPU_MAX_CLASSES, k))
    if not 1 <= beam_width <= GPU_MAX_BEAM_WIDTH:
        raise BeamSearchLimitError("the GPU beam search takes a beam width of 1..{}, not {}".format(
            GPU_MAX_BEAM_WIDTH, beam_width))
    if language_model is not None and not 1 <= language_model.order <= GPU_MAX_LM_ORDER:
        raise BeamSearchLimitError("the GPU beam search takes a language model of order 1..{}, not {}".format(
            GPU_MAX_LM_ORDER, language_model.order))


def _to_device(array, dtype, device):
    import torch
    if isinstance(array, torch.Tensor):
        if array.device.type != "cuda":
            array = array.to(device)
        return array.to(dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(array), dtype={torch.float32: np.float32,
                                                                            torch.int32: np.int32}[dtype])).to(device)


class _GpuBeamSearchDecoder:
    """What the two GPU decoders share: the limits, the uploaded scorer tables, the workspace, and the call itself."""

    def __init__(self, allowed_characters, n_classes, language_model, beam_width, kenlm_weight, word_count_weight,
                 valid_word_count_weight, device):
        import torch
        from . import _lib as hip
        self.allowed_characters = list(allowed_characters)
        _check_gpu_limits(n_classes, beam_width, language_model)
        self.beam_width = beam_width
        self.language_model = language_model
        self.device = torch.device(device)
        self._hip = hip
        self._tables = None
        self._lm = None
        self._workspace = None
        if language_model is not None:
            self._tables, self._lm = _upload_scorer(hip, self.allowed_characters, language_model, kenlm_weight,
                                                    word_count_weight, valid_word_count_weight, self.device)

    @classmethod
    def from_kenlm_directory(cls, kenlm_directory, allowed_characters, **kw):
        return cls(allowed_characters, NGramLanguageModel(find_arpa(kenlm_directory)), **kw)

    def _lengths(self, prediction_lengths, b, device):
        import torch
        lengths = _to_device(prediction_lengths, torch.int32, device).reshape(-1)
        if lengths.numel() != b:
            raise ValueError("{} lengths for a batch of {}".format(lengths.numel(), b))
        return lengths

    def _run(self, entry, scores, b, t, k, *args_before_lm):
        """entry(*args_before_lm, lm, out, out_len, score, workspace, workspace bytes, stream) on the device of `scores`, the
        (B, T', K) tensor; returns (list of index lists, scores (B,) numpy)."""
        import torch
        lib = self._hip.lib()
        need = lib.raw(entry + "_workspace_bytes")(b, t, k, self.beam_width)
        if need == 0:
            raise BeamSearchLimitError("the GPU beam search cannot take a ({}, {}, {}) batch at beam width {}".format(
                b, t, k, self.beam_width))
        device = scores.device
        if self._workspace is None or self._workspace.numel() < need or self._workspace.device != device:
            self._workspace = torch.empty((need,), dtype=torch.uint8, device=device)
        out = torch.empty((b, t), dtype=torch.int32, device=device)
        out_len = torch.empty((b,), dtype=torch.int32, device=device)
        score = torch.empty((b,), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            stream = torch.cuda.current_stream().cuda_stream
            lib.call(entry, *args_before_lm, ctypes.byref(self._lm) if self._lm is not None else None, out.data_ptr(),
                     out_len.data_ptr(), score.data_ptr(), self._workspace.data_ptr(), self._workspace.numel(), stream)
        out, out_len, score = out.cpu().numpy(), out_len.cpu().numpy(), score.cpu().numpy()
        if (out_len < 0).any():
            raise RuntimeError(entry + ": node arena overflow")
        return [list(map(int, out[i, :out_len[i]])) for i in range(b)], score


class GpuCtcBeamSearchDecoder(_GpuBeamSearchDecoder):
    """CtcBeamSearchDecoder on the GPU (ctc_beam.hip): the same search and the same results, one wave per utterance.
    The language model's tables are exported from the host scorer and uploaded once.  Limits: at most 64 classes,
    beam width 1..128, language-model order <= 6 (BeamSearchLimitError, a ValueError, otherwise)."""

    def __init__(self, allowed_characters, language_model=None, beam_width=DEFAULT_BEAM_WIDTH, merge_repeated=False,
                 kenlm_weight=KENLM_WEIGHT, word_count_weight=WORD_COUNT_WEIGHT,
                 valid_word_count_weight=VALID_WORD_COUNT_WEIGHT, epsilon=1e-8, threads=8, device="cuda:0"):
        characters = list(allowed_characters)
        super().__init__(characters, len(characters) + 1, language_model, beam_width, kenlm_weight, word_count_weight,
                         valid_word_count_weight, device)
        self.merge_repeated = merge_repeated
        self.epsilon = epsilon
        self.threads = threads  # unused: kept so that the constructor matches CtcBeamSearchDecoder's

    def decode(self, probabilities, prediction_lengths):
        """probabilities: (B, T', K) numpy array or float32 tensor on the GPU (used in place); prediction_lengths: (B,)
        numbers, numpy or tensor.  Returns (list of index lists, log-probabilities (B,) numpy), as CtcBeamSearchDecoder."""
        import torch
        probs = _to_device(probabilities, torch.float32, self.device)
        if probs.dim() != 3:
            raise ValueError("probabilities must be (B, T', K)")
        b, t, k = probs.shape
        if k != len(self.allowed_characters) + 1:
            raise ValueError("{} classes for an alphabet of {} characters + blank".format(k, len(self.allowed_characters)))
        lengths = self._lengths(prediction_lengths, b, probs.device)
        return self._run("sl_ctc_beam_search", probs, b, t, k, probs.data_ptr(), lengths.data_ptr(), b, t, k, k - 1,
                         self.beam_width, 1 if self.merge_repeated else 0, self.epsilon)


class GpuAsgBeamSearchDecoder(_GpuBeamSearchDecoder):
    """The ASG beam search on the GPU (asg_beam.hip; definition: include/speechless_hip.h, sl_asg_beam_search): a max search
    over grapheme prefixes under emissions + transition scores, scored by the n-gram model when there is one.  The graphemes
    are the allowed characters and the two repeat marks (AsgGraphemeEncoding); the scorer is built over the characters, and
    a repeat mark feeds it the characters it stands for.  Limits: at most 64 graphemes, beam width 1..128, language-model
    order <= 6 (BeamSearchLimitError, a ValueError, otherwise)."""

    def __init__(self, allowed_characters, language_model=None, beam_width=DEFAULT_BEAM_WIDTH, kenlm_weight=KENLM_WEIGHT,
                 word_count_weight=WORD_COUNT_WEIGHT, valid_word_count_weight=VALID_WORD_COUNT_WEIGHT, device="cuda:0"):
        characters = list(allowed_characters)
        self.grapheme_set_size = len(characters) + 2
        _check_gpu_limits(self.grapheme_set_size, beam_width, language_model)  # (first, as ever: the base's comes too late)
        if language_model is not None and not characters:
            raise BeamSearchLimitError("a language model needs at least one character beside the two repeat marks")
        super().__init__(characters, self.grapheme_set_size, language_model, beam_width, kenlm_weight, word_count_weight,
                         valid_word_count_weight, device)

    def decode(self, logq, trans, init, prediction_lengths):
        """logq: (B, T', K) emissions, trans: (K, K) [from][to], init: (K,) -- numpy arrays or float32 tensors on the GPU
        (used in place); prediction_lengths: (B,) numbers, numpy or tensor.  Returns (list of grapheme index lists, scores
        (B,) numpy)."""
        import torch
        logq = _to_device(logq, torch.float32, self.device)
        if logq.dim() != 3:
            raise ValueError("logq must be (B, T', K)")
        b, t, k = logq.shape
        if k != self.grapheme_set_size:
            raise ValueError("{} classes for {} characters + 2 repeat marks".format(k, len(self.allowed_characters)))
        trans = _to_device(trans, torch.float32, logq.device)
        init = _to_device(init, torch.float32, logq.device)
        if tuple(trans.shape) != (k, k) or tuple(init.shape) != (k,):
            raise ValueError("ASG scores must have shapes ({0}, {0}) and ({0},), not {1} and {2}".format(
                k, tuple(trans.shape), tuple(init.shape)))
        lengths = self._lengths(prediction_lengths, b, logq.device)
        return self._run("sl_asg_beam_search", logq, b, t, k, logq.data_ptr(), trans.data_ptr(), init.data_ptr(),
                         lengths.data_ptr(), b, t, k, self.beam_width)
