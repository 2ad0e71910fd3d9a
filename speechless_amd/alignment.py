"""Result types of forced alignment (Wav2Letter.alignment_batch / positional_label_batch / align_recording under CTC,
asg_alignment_batch / asg_positional_label_batch / asg_align_recording under ASG).

`PositionalLabel` is the reference's word-timing label (speechless/labeled_example.py:32-60): `(word, (start, end))`
sections, which LabeledExampleFromFile.sections() (:219-234) uses to cut long recordings.  `CtcAlignment` is one
utterance's Viterbi alignment (include/speechless_hip.h, sl_ctc_align) turned into character and word frame ranges;
`AsgAlignment` is the same for the ASG criterion (sl_asg_align / sl_asg_align_long), whose path runs over the run-length-encoded label.
`ScoredAlignment` adds the confidences of sl_ctc_segment_scores to a `CtcAlignment` (Wav2Letter.word_confidence_batch /
predict_with_confidence_batch / confidence_of_recording), or those of sl_asg_segment_scores to an `AsgAlignment` (the asg_ methods
of the same names): a `WordConfidence` per word and the posterior of the whole label.
`PhraseHit` is one occurrence of a phrase that the phrase search found (sl_ctc_spot; Wav2Letter.find_phrases_batch /
find_phrases_in_recording)."""
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


def word_spans(label: str) -> List[Tuple[int, int]]:
    """(char_begin, char_end), half-open, of each space-separated word of `label` (any run of spaces separates)"""
    spans = []
    i = 0
    while i < len(label):
        if label[i] == " ":
            i += 1
            continue
        j = i
        while j < len(label) and label[j] != " ":
            j += 1
        spans.append((i, j))
        i = j
    return spans


def _word_frames(label: str, character_frames) -> List[Tuple[str, Tuple[int, int]]]:
    """(word, (first, end)) per space-separated word of `label`: from its first character's first frame to its last one's end"""
    return [(label[i:j], (character_frames[i][0], character_frames[j - 1][1])) for i, j in word_spans(label)]


class _WordTimings:
    """what an alignment with `word_frames` offers on top of them"""
    word_frames = []  # type: List[Tuple[str, Tuple[int, int]]]

    def positional_label(self, seconds_per_frame: float) -> Optional[PositionalLabel]:
        """The word ranges in seconds (output frame t covers [t, t + 1) * seconds_per_frame), or None when the
        utterance is infeasible or has no words."""
        if not self.word_frames:
            return None
        return PositionalLabel([(word, (first * seconds_per_frame, end * seconds_per_frame))
                                for word, (first, end) in self.word_frames])


class CtcAlignment(_WordTimings):
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
        self.word_frames = _word_frames(label, self.character_frames) if self.feasible else []

    @staticmethod
    def from_path(label: str, log_probability: float, path) -> "CtcAlignment":
        """From sl_ctc_align's output row: lattice states (odd s = label position (s - 1) / 2, even = blank, -1 = none)."""
        path = np.asarray(path, dtype=np.int32)
        positions = np.where((path >= 0) & (path % 2 == 1), (path - 1) // 2, -1)
        return CtcAlignment(label, log_probability, positions.astype(np.int32))

    def __repr__(self):
        return "CtcAlignment({!r}, log_probability={}, words={})".format(self.label, self.log_probability, self.word_frames)


def _section_groups(words, max_frames: int) -> List[Tuple[List[int], Tuple[int, int]]]:
    """the grouping and the cut rule of cut_sections / cut_section_spans: (indices of the section's words, (first, end))"""
    groups = []  # type: List[List[int]]
    for i, (_, (first, end)) in enumerate(words):
        if groups and end - words[groups[-1][0]][1][0] <= max_frames:
            groups[-1].append(i)
        else:
            groups.append([i])
    sections = []
    for n, group in enumerate(groups):
        start = words[group[0]][1][0]
        end = words[group[-1]][1][1]
        if n > 0:
            start = (words[group[0] - 1][1][1] + start) // 2
        if n + 1 < len(groups):
            end = (end + words[group[-1] + 1][1][0]) // 2
        sections.append((group, (start, end)))
    return sections


def cut_sections(alignment, max_frames: int) -> List[Tuple[str, Tuple[int, int]]]:
    """Cuts an aligned recording (Wav2Letter.align_recording, or asg_align_recording) into sections of whole words, (text, (first, end)) in output
    frames: what LabeledExampleFromFile.sections() (labeled_example.py:219-234) needs to turn a long recording into utterances.
    Greedy: a section takes words while its last word's end - its first word's first <= max_frames; a single word longer
    than that is a section by itself.  The cut between two sections lies at the midpoint (integer floor) of the gap between
    the neighbouring words; the first section starts at its first word's first frame, the last ends at its last word's end.
    Empty for an infeasible alignment (or one without words)."""
    words = alignment.word_frames
    return [(" ".join(words[i][0] for i in group), frames) for group, frames in _section_groups(words, max_frames)]


def cut_section_spans(alignment, max_frames: int) -> List[Tuple[str, Tuple[int, int], Tuple[int, int]]]:
    """cut_sections with each section's character span in alignment.label: (text, (first, end), (char_begin, char_end)), from
    its first word's first character to its last word's last (so label[char_begin:char_end] keeps the label's own spacing,
    where the text joins the words with single spaces).  What Wav2Letter.confidence_of_recording scores."""
    words = alignment.word_frames
    spans = word_spans(alignment.label)
    return [(" ".join(words[i][0] for i in group), frames, (spans[group[0]][0], spans[group[-1]][1]))
            for group, frames in _section_groups(words, max_frames)]


class WordConfidence:
    """One word of a scored alignment: its output frames [first, end) and the log of its segment posterior -- the
    probability that those frames, read on their own, say exactly the word (sl_ctc_segment_scores; under ASG
    sl_asg_segment_scores, where a word in mid-utterance is read given the grapheme the label puts before it)."""

    def __init__(self, word: str, first: int, end: int, log_posterior: float):
        self.word = word
        self.first = int(first)
        self.end = int(end)
        self.log_posterior = float(log_posterior)

    @property
    def confidence(self) -> float:
        return float(np.exp(self.log_posterior))

    def __repr__(self):
        return "WordConfidence({!r}, ({}, {}), confidence={:.4f})".format(self.word, self.first, self.end, self.confidence)


class ScoredAlignment:
    """A CtcAlignment or an AsgAlignment (anything with `label` and `word_frames`) with confidences.  words: a WordConfidence
    per word of alignment.word_frames, in order (empty when the alignment is infeasible or has no words).  log_posterior: the
    whole label over all of the utterance's frames, log p(label | audio) = minus the CTC loss, or minus the ASG loss (-inf when
    infeasible)."""

    def __init__(self, alignment, word_log_posteriors, log_posterior: float):
        word_log_posteriors = [float(x) for x in word_log_posteriors]
        if len(word_log_posteriors) != len(alignment.word_frames):
            raise ValueError("{} word scores for the {} words of {!r}".format(len(word_log_posteriors), len(alignment.word_frames),
                                                                            alignment.label))
        self.alignment = alignment
        self.words = [WordConfidence(word, first, end, score)
                      for (word, (first, end)), score in zip(alignment.word_frames, word_log_posteriors)]
        self.log_posterior = float(log_posterior)

    @property
    def label(self) -> str:
        return self.alignment.label

    def __repr__(self):
        return "ScoredAlignment({!r}, log_posterior={}, words={})".format(self.label, self.log_posterior, self.words)


class PhraseHit:
    """One occurrence of a phrase found by the phrase search (sl_ctc_spot; Wav2Letter.find_phrases_batch /
    find_phrases_in_recording): its output frames [first, end) -- the first and the last of them frames of a letter --, the
    log-probability of its best path over those frames, and the log of its segment posterior: the probability that those frames,
    read on their own, say exactly the phrase (sl_ctc_segment_scores; nan where it was not asked for)."""

    def __init__(self, phrase: str, first: int, end: int, log_probability: float, log_posterior: float = float("nan")):
        self.phrase = phrase
        self.first = int(first)
        self.end = int(end)
        self.log_probability = float(log_probability)
        self.log_posterior = float(log_posterior)

    def confidence(self) -> float:
        """the segment posterior as a probability; nan without one"""
        return float(np.exp(self.log_posterior))

    def seconds(self, seconds_per_frame: float) -> Tuple[float, float]:
        """(start, end) in seconds, where one OUTPUT frame lasts seconds_per_frame"""
        return self.first * float(seconds_per_frame), self.end * float(seconds_per_frame)

    def __eq__(self, other):
        return isinstance(other, PhraseHit) and (self.phrase, self.first, self.end, self.log_probability) == \
            (other.phrase, other.first, other.end, other.log_probability) and \
            (self.log_posterior == other.log_posterior or (np.isnan(self.log_posterior) and np.isnan(other.log_posterior)))

    def __repr__(self):
        return "PhraseHit({!r}, ({}, {}), log_probability={:.4f}, confidence={:.4f})".format(
            self.phrase, self.first, self.end, self.log_probability, self.confidence())


def _characters_per_grapheme(label: str) -> List[Tuple[int, bool]]:
    """(characters, is a repeat mark) per grapheme of the ASG encoding of `label`: a letter stands for 1 character; a run of
    two / three equal letters is written as the letter and a repeat mark that stands for 1 / 2 characters.
    (AsgGraphemeEncoding.encode refuses longer runs.)"""
    counts = []
    i = 0
    while i < len(label):
        j = i
        while j < len(label) and label[j] == label[i]:
            j += 1
        if j - i > 3:
            raise ValueError("{}-fold repetition found, ASG only supports up to 3-fold.".format(j - i))
        counts.extend([[(1, False)], [(1, False), (1, True)], [(1, False), (2, True)]][j - i - 1])
        i = j
    return counts


def grapheme_spans(label: str, char_spans) -> List[Tuple[int, int]]:
    """(begin, end), half-open, in the ASG encoding of `label` of each (char_begin, char_end) span of `label` (word_spans',
    or a section's of cut_section_spans): what sl_asg_segment_scores takes as a label range.  A letter and its repeat mark
    belong wholly to the span that holds the run; a span that begins or ends inside a run of equal characters would split
    such a pair -- between words only a run of spaces can be split -- and raises ValueError."""
    first = {0: 0}  # character offset at which a run begins (or the label ends) -> graphemes before it
    chars = graphemes = 0
    for count, is_mark in _characters_per_grapheme(label):
        if not is_mark:
            first[chars] = graphemes
        chars += count
        graphemes += 1
    first[chars] = graphemes
    spans = []
    for begin, end in char_spans:
        if not 0 <= begin <= end <= len(label):
            raise ValueError("span ({}, {}) outside the {} characters of {!r}".format(begin, end, len(label), label))
        for p in (begin, end):
            if 0 < p < len(label) and label[p - 1] == label[p]:
                raise ValueError("span ({}, {}) splits the run of {!r} at character {} of {!r}: a letter and its repeat mark "
                                 "are scored together".format(begin, end, label[p], p, label))
        spans.append((first[begin], first[end]))
    return spans


def cut_section_grapheme_spans(alignment, max_frames: int) -> List[Tuple[str, Tuple[int, int], Tuple[int, int]]]:
    """cut_section_spans for an AsgAlignment, with each section's span in the ENCODED label: (text, (first, end),
    (grapheme_begin, grapheme_end)).  What Wav2Letter.asg_confidence_of_recording scores."""
    sections = cut_section_spans(alignment, max_frames)
    spans = grapheme_spans(alignment.label, [chars for _, _, chars in sections])
    return [(text, frames, span) for (text, frames, _), span in zip(sections, spans)]


def encode_transcripts(encoding, transcripts) -> list:
    """the ASG-encoded label (a list of grapheme indices) of every transcript of a decode under `encoding` (an
    AsgGraphemeEncoding), or None in place of one the encoding refuses: a decoded grapheme sequence may stack repeat marks
    (letter, thrice, letter ...) into a run of more than three equal letters, which encode() cannot write.  What
    Wav2Letter.asg_predict_with_confidence_batch aligns and scores."""
    rows = []
    for transcript in transcripts:
        try:
            rows.append([int(g) for g in encoding.encode(transcript)])
        except ValueError:
            rows.append(None)
    return rows


class AsgAlignment(_WordTimings):
    """The best ASG path of one utterance through its encoded label (no blank: every frame lies on a grapheme).

    encoded_label: the label as AsgGraphemeEncoding.encode writes it (a run of two / three equal letters is the letter and
    a repeat mark).  frame_grapheme_positions: int32 (T',), the index into `encoded_label` of the grapheme the frame is
    aligned to, -1 past the utterance's frames.  log_probability: the path's score, -inf when the frames cannot hold the
    label or -inf scores close every path (then every position is -1 and there are no ranges)."""

    def __init__(self, label: str, encoded_label, log_probability: float, frame_grapheme_positions):
        self.label = label
        self.encoded_label = [int(g) for g in encoded_label]
        self.log_probability = float(log_probability)
        self.frame_grapheme_positions = np.asarray(frame_grapheme_positions, dtype=np.int32)
        self.feasible = self.log_probability != -np.inf
        counts = _characters_per_grapheme(label)
        if len(counts) != len(self.encoded_label):
            raise ValueError("{!r} is written with {} graphemes, not {}".format(label, len(counts), len(self.encoded_label)))
        # (first, end) half-open output-frame range per encoded grapheme: contiguous, non-empty, covering [0, T_b)
        self.grapheme_frames = []  # type: List[Tuple[int, int]]
        # the same per character of `label`: a letter takes its grapheme's range; of a run written as letter + mark the
        # first character takes the letter's range and the one or two others take the mark's
        self.character_frames = []  # type: List[Tuple[int, int]]
        if self.feasible:
            # one linear pass: the path's runs of equal positions, then per grapheme the number of its runs and where its
            # only one lies (a long recording has thousands of graphemes over tens of thousands of frames)
            positions = self.frame_grapheme_positions.reshape(-1)
            n = len(counts)
            starts = np.concatenate([[0], np.flatnonzero(positions[1:] != positions[:-1]) + 1]) if positions.size else \
                np.zeros(0, dtype=np.int64)
            ends = np.concatenate([starts[1:], [positions.size]])
            values = positions[starts]
            mine = (values >= 0) & (values < n)
            runs = np.bincount(values[mine], minlength=n)
            first = np.full(n, -1, dtype=np.int64)
            last = np.full(n, -1, dtype=np.int64)
            first[values[mine][::-1]] = starts[mine][::-1]  # (reversed: the earliest run of a grapheme is written last)
            last[values[mine][::-1]] = ends[mine][::-1]
            end = 0
            for i, (count, _) in enumerate(counts):
                if runs[i] != 1 or first[i] != end:
                    raise ValueError("alignment path does not pass grapheme {} of {!r} in one run behind grapheme {}".format(
                        i, label, i - 1))
                end = int(last[i])
                self.grapheme_frames.append((int(first[i]), end))
                self.character_frames.extend([self.grapheme_frames[-1]] * count)
        self.word_frames = _word_frames(label, self.character_frames) if self.feasible else []

    @staticmethod
    def from_path(label: str, encoded_label, twice_index: int, thrice_index: int, score: float, path) -> "AsgAlignment":
        """From sl_asg_align's output row: the state = position in the encoded label per frame, -1 = none.  twice_index /
        thrice_index: the encoding's repeat marks, checked against where the label's runs put them."""
        if any(is_mark and int(g) != (twice_index if count == 1 else thrice_index)
               for g, (count, is_mark) in zip(encoded_label, _characters_per_grapheme(label))):
            raise ValueError("encoded label of {!r} does not hold its repeat marks ({}, {}) where its runs are".format(
                label, twice_index, thrice_index))
        return AsgAlignment(label, encoded_label, score, np.asarray(path, dtype=np.int32))

    def __repr__(self):
        return "AsgAlignment({!r}, log_probability={}, words={})".format(self.label, self.log_probability, self.word_frames)
