"""speechless_amd -- MI355X-native implementation of the speechless Wav2Letter hot path (conv stack fwd/bwd + CTC).

Importing the package never touches the GPU; `Wav2Letter` / `Engine` need libspeechless_hip.so (see build.py) and a
ROCm device, and raise instead of falling back to the CPU.
"""
from .grapheme_encoding import CtcGraphemeEncoding, english_frequent_characters, german_frequent_characters  # noqa: F401


def __getattr__(name):
    if name in ("Wav2Letter", "Adam", "SGD", "RMSprop", "Adagrad", "Adadelta", "Adamax", "LabeledSpectrogram", "ExpectationVsPrediction", "ExpectationsVsPredictions",
                "ExpectationsVsPredictionsInBatches", "ExpectationsVsPredictionsInGroupedBatches"):
        from . import net
        return getattr(net, name)
    if name in ("PositionalLabel", "CtcAlignment", "AsgAlignment", "cut_sections", "cut_section_spans", "word_spans",
                "WordConfidence", "ScoredAlignment", "grapheme_spans", "cut_section_grapheme_spans", "PhraseHit"):
        from . import alignment
        return getattr(alignment, name)
    if name == "window_plan":
        from .longform import window_plan
        return window_plan
    if name == "Engine":
        from .engine import Engine
        return Engine
    raise AttributeError(name)
