"""Result types of CTC forced alignment (Wav2Letter.alignment_batch / positional_label_batch).

`PositionalLabel` is the reference's word-timing label (speechless/labeled_example.py:32-60): `(word, (start, end))`
sections, which LabeledExampleFromFile.sections() (:219-234) uses to cut long recordings.  `CtcAlignment` is one
utterance's Viterbi alignment (include/speechless_hip.h, sl_ctc_align) turned into character and word frame ranges."""
from typing import Callable, List, Optional, Tuple

import numpy as np


class PositionalLabel:
    """Words with (start, end) positions -- samples, seconds or frames, whatever the producer used."""

    def __init__(self, labeled_sections: List[Tuple[str, Tuple[float, float]]]):
        if not labeled_sections:
            raise ValueError("Sections must be specified.")
        if any(section_range is None for _, section_range in labeled_sections):
            raise ValueError("Range must be specified.")
        self.labeled_sections = labeled_sections
        self.labels = [word for word, _ in labeled_sections]
        self.label = " ".join(self.labels)

    def convert_range_to_seconds(self, original_sample_rate: int) -> "PositionalLabel":
        """Sections positioned in samples of `original_sample_rate` -> the same sections in seconds."""
        return PositionalLabel([(word, (start / original_sample_rate, end / original_sample_rate))
                                for word, (start, end) in self.labeled_sections])

    def with_corrected_labels(self, correction: Callable[[str], str]) -> "PositionalLabel":
        return PositionalLabel([(correction(word), section_range) for word, section_range in self.labeled_sections])

    def serialize(self) -> str:
        """One `word|start|end` line per section."""
        return "\n".join("{}|{}|{}".format(word, start, end) for word, (start, end) in self.labeled_sections)

    @staticmethod
    def deserialize(serialized: str) -> "PositionalLabel":
        sections = []
        for line in serialized.splitlines():
            word, start, end = line.split("|")
            sections.append((word, (float(start), float(end))))
        return PositionalLabel(sections)


class CtcAlignment:
    """The best CTC path of one utterance through its label.

    frame_label_positions: int32 (T',), -1 where the path is on a blank (and past the utterance's frames), otherwise the
    index into `label` of the character the frame is aligned to.  log_probability: the path's log-probability, -inf when
    the frames cannot hold the label (then every position is -1 and there are no character or word ranges)."""

    def __init__(self, label: str, log_probability: float, frame_label_positions):
        self.label = label
        self.log_probability = float(log_probability)
        self.frame_label_positions = np.asarray(frame_label_positions, dtype=np.int32)
        self.feasible = self.log_probability != -np.inf
        # (first, end) half-open output-frame range per character of the label: a feasible CTC path visits every label
        # position in one contiguous run of at least one frame
        self.character_frames = []  # type: List[Tuple[int, int]]
        if self.feasible:
            positions = self.frame_label_positions
            for i in range(len(label)):
                frames = np.flatnonzero(positions == i)
                if frames.size == 0:
                    raise ValueError("alignment path skips character {} of {!r}".format(i, label))
                self.character_frames.append((int(frames[0]), int(frames[-1]) + 1))
        # (word, (first, end)) per space-separated word: from its first character's first frame to its last one's end
        self.word_frames = []  # type: List[Tuple[str, Tuple[int, int]]]
        if self.feasible:
            i = 0
            while i < len(label):
                if label[i] == " ":
                    i += 1
                    continue
                j = i
                while j < len(label) and label[j] != " ":
                    j += 1
                self.word_frames.append((label[i:j], (self.character_frames[i][0], self.character_frames[j - 1][1])))
                i = j

    def positional_label(self, seconds_per_frame: float) -> Optional[PositionalLabel]:
        """The word ranges in seconds (output frame t covers [t, t + 1) * seconds_per_frame), or None when the
        utterance is infeasible or has no words."""
        if not self.word_frames:
            return None
        return PositionalLabel([(word, (first * seconds_per_frame, end * seconds_per_frame))
                                for word, (first, end) in self.word_frames])

    @staticmethod
    def from_path(label: str, log_probability: float, path) -> "CtcAlignment":
        """From sl_ctc_align's output row: lattice states (odd s = label position (s - 1) / 2, even = blank, -1 = none)."""
        path = np.asarray(path, dtype=np.int32)
        positions = np.where((path >= 0) & (path % 2 == 1), (path - 1) // 2, -1)
        return CtcAlignment(label, log_probability, positions.astype(np.int32))

    def __repr__(self):
        return "CtcAlignment({!r}, log_probability={}, words={})".format(self.label, self.log_probability, self.word_frames)
