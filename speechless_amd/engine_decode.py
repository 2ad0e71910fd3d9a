"""What runs on the probabilities behind forward() outside the training step: greedy / Viterbi / beam decoding, the four forced
aligners, the CTC and ASG segment posteriors, the CTC phrase search, long recordings (longform.py) and the error counts.  One host
path each: the aligners differ by a row of _ALIGNERS, their label batches pass check_label_batch, their tensors live in
buffers._AlignBuffers (the segment posteriors differ by a row of _SEGMENTERS, theirs live in _SegmentBuffers; the phrase search's
queries pass check_queries, its tensors live in _SpotBuffers).  Methods of Engine."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import longform
from .buffers import _AlignBuffers, _SegmentBuffers, _SpotBuffers
from .error_counts import host_counts, pack_rows


class _Aligner(NamedTuple):
    """one forced aligner: its entry point (Engine's method has the same name without the sl_ prefix; the workspace query is
    <entry>_workspace_bytes), its launch tag, and for a _long aligner the most letters a label may have with the refusal's text
    (which goes on to name the entry point)"""
    entry: str
    tag: str
    max_label: Optional[int] = None
    too_long: Optional[str] = None


_ALIGNERS = {  # (kind, long)
    ("ctc", False): _Aligner("sl_ctc_align", "align"),
    ("asg", False): _Aligner("sl_asg_align", "asg_align"),
    ("ctc", True): _Aligner("sl_ctc_align_long", "align_long", longform.ALIGN_MAX_LABEL,
                            "labels of {} letters: forced alignment takes at most {}"),
    ("asg", True): _Aligner("sl_asg_align_long", "asg_align_long", longform.ASG_ALIGN_MAX_LABEL,
                            "labels of {} graphemes: ASG forced alignment takes at most {}"),
}


class _Segmenter(NamedTuple):
    """one segment-posterior kernel: its entry point (the workspace query is <entry>_workspace_bytes; under ASG it also takes
    the class count), its launch tag (the _long method's: tag + "_long"), whether it runs under the ASG criterion (labels in
    [0, K), no blank, the engine's score tables) or over the CTC lattice (labels in [0, K - 1), blank = K - 1), and the most
    label positions a segment may span with the word the refusal uses for them"""
    entry: str
    tag: str
    asg: bool
    max_label: int
    unit: str


_SEGMENTERS = {
    "ctc": _Segmenter("sl_ctc_segment_scores", "segment_scores", False, longform.SEGMENT_MAX_LABEL, "letters"),
    "asg": _Segmenter("sl_asg_segment_scores", "asg_segment_scores", True, longform.ASG_SEGMENT_MAX_LABEL, "graphemes"),
}
_SPOT = "sl_ctc_spot"
_VITERBI = "sl_asg_viterbi"
_GREEDY = "sl_greedy_decode"


def check_label_batch(labels, lengths, batch, n_labels, *, blank=None, in_len=None, max_letters=None, too_long_text=None,
                      check_lengths=True):
    """What the engine asks of a label batch, on the host: (B, Lmax) with B lengths -- (B,) or (B, 1) -- and every index of row
    b below lengths[b] in [0, n_labels).  blank: the CTC blank's index (n_labels = K - 1), named in the refusal; None under
    ASG, where every one of the K classes is a label.  The _long aligners also pass their B prediction lengths in_len (numpy)
    and the most letters a label may have, max_letters, with the refusal's text too_long_text.  check_lengths=False is
    Engine.set_labels: it has never asked for B lengths, each within its row -- a length beyond the row takes the whole row.
    Returns (labels, lengths), int32 numpy."""
    labels = np.asarray(labels, dtype=np.int32)
    lab_len = np.asarray(lengths, dtype=np.int32).reshape(-1)
    if labels.ndim != 2 or labels.shape[0] != batch or (check_lengths and lab_len.shape[0] != batch) or \
            (in_len is not None and in_len.shape[0] != batch):
        raise ValueError("label batch must be (B, Lmax) with B lengths" if in_len is None else
                         "label batch must be (B, Lmax) with B label lengths and B prediction lengths")
    if max_letters is not None and labels.shape[1] > max_letters:
        raise ValueError(too_long_text.format(labels.shape[1], max_letters))
    for i in range(batch):
        if check_lengths and not 0 <= lab_len[i] <= labels.shape[1]:
            raise ValueError("label length {} of utterance {} outside [0, {}]".format(lab_len[i], i, labels.shape[1]))
        row = labels[i, :lab_len[i]]
        if row.size and (row.min() < 0 or row.max() >= n_labels):
            raise ValueError("label {} holds an index outside [0, {})".format(i, n_labels) +
                             ("" if blank is None else " (blank is {})".format(blank)))
    return labels, lab_len


def check_segments(segments, batch, kind="ctc"):
    """What the engine asks of the segments of ctc_segment_scores / asg_segment_scores (row _SEGMENTERS[kind]), on the host:
    (N, 5) integers {b, frame_begin, frame_end, label_begin, label_end} with N >= 1, b in [0, batch), 0 <= begin <= end for both
    ranges and a label span of at most longform.SEGMENT_MAX_LABEL letters (ASG_SEGMENT_MAX_LABEL encoded graphemes); the first
    row that breaks a rule is named.  Returns them as contiguous int32 numpy."""
    row = _SEGMENTERS[kind]
    seg = np.asarray(segments)
    if seg.ndim != 2 or seg.shape[1] != 5 or seg.shape[0] < 1 or not np.issubdtype(seg.dtype, np.integer):
        raise ValueError("segments must be an (N, 5) integer array of (b, frame_begin, frame_end, label_begin, label_end), N >= 1")
    seg = seg.astype(np.int64)
    bad = (seg[:, 0] < 0) | (seg[:, 0] >= batch) | (seg[:, 1] < 0) | (seg[:, 2] < seg[:, 1]) | (seg[:, 3] < 0) | \
        (seg[:, 4] < seg[:, 3]) | (seg[:, 4] - seg[:, 3] > row.max_label) | (seg[:, 1:].max(axis=1) >= 2 ** 31)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("segment {0} = {1}: need b in [0, {2}), 0 <= begin <= end for frames and {4}, and at most {3} {4} "
                         "({5})".format(i, seg[i].tolist(), batch, row.max_label, row.unit, row.entry))
    return np.ascontiguousarray(seg, dtype=np.int32)


def check_queries(queries, lengths, utterances, min_scores, max_hits, batch, n_labels):
    """What the engine asks of the queries of ctc_spot, on the host: (N, Qmax) integers with N >= 1 and 1 <= Qmax <=
    longform.SPOT_MAX_PHRASE, N lengths in [1, Qmax], N utterances in [0, batch), N thresholds that are no NaN, every index of row
    i below lengths[i] in [0, n_labels), and 1 <= max_hits <= longform.SPOT_MAX_HITS; the first query that breaks a rule is
    named.  Returns (queries, lengths, utterances int32, thresholds float32, max_hits int), contiguous numpy."""
    q = np.asarray(queries)
    if q.ndim != 2 or q.shape[0] < 1 or q.shape[1] < 1 or not np.issubdtype(q.dtype, np.integer):
        raise ValueError("queries must be an (N, Qmax) integer array, N >= 1 and Qmax >= 1")
    if q.shape[1] > longform.SPOT_MAX_PHRASE:
        raise ValueError("queries of {} letters: the phrase search takes at most {} ({})".format(
            q.shape[1], longform.SPOT_MAX_PHRASE, _SPOT))
    n = q.shape[0]
    length = np.asarray(lengths, dtype=np.int64).reshape(-1)
    utt = np.asarray(utterances, dtype=np.int64).reshape(-1)
    thresholds = np.asarray(min_scores, dtype=np.float32).reshape(-1)
    if length.shape[0] != n or utt.shape[0] != n or thresholds.shape[0] != n:
        raise ValueError("queries must come with N lengths, N utterances and N thresholds")
    if not 1 <= int(max_hits) <= longform.SPOT_MAX_HITS:
        raise ValueError("max_hits = {} outside [1, {}] ({})".format(max_hits, longform.SPOT_MAX_HITS, _SPOT))
    bad = (length < 1) | (length > q.shape[1]) | (utt < 0) | (utt >= batch) | np.isnan(thresholds)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("query {}: length {}, utterance {}, threshold {}: need a length in [1, {}], an utterance in [0, {}) and a "
                         "threshold that is a number".format(i, length[i], utt[i], thresholds[i], q.shape[1], batch))
    for i in range(n):
        row = q[i, :length[i]]
        if row.min() < 0 or row.max() >= n_labels:
            raise ValueError("query {} holds an index outside [0, {}) (blank is {})".format(i, n_labels, n_labels))
    return (np.ascontiguousarray(q, dtype=np.int32), length.astype(np.int32), utt.astype(np.int32),
            np.ascontiguousarray(thresholds), int(max_hits))


def _merge_repeats(paths):
    """per-frame ASG paths (rows of grapheme indices, -1 past the utterance) -> index lists with repeats merged"""
    decoded = []
    for row in paths:
        row = row[row >= 0]
        decoded.append([int(g) for g in row[np.concatenate([[True], row[1:] != row[:-1]])]] if row.size else [])
    return decoded


class DecodeAlignMixin:
    # ------------------------------------------------------------------ decoding

    def _launch_greedy(self, tag, probs, lens, out, out_len, frame_argmax, b, t):
        """one greedy CTC decode of (b, t, K) probabilities (frame_argmax: None where nobody asks for it) -> index lists"""
        k = self.grapheme_set_size
        self._launch(tag, _GREEDY, probs.data_ptr(), lens.data_ptr(), out.data_ptr(), out_len.data_ptr(),
                     None if frame_argmax is None else frame_argmax.data_ptr(), b, t, k, k - 1, self._stream())
        dec, n = out.cpu().numpy(), out_len.cpu().numpy()
        return [list(map(int, dec[i, :n[i]])) for i in range(b)]

    def greedy_decode(self, prediction_lengths=None):
        """Greedy CTC decode of the current probabilities.  Returns (list of index lists, frame argmax (B,T') numpy)."""
        buf = self.cur
        if prediction_lengths is not None:
            self.set_input_lengths(prediction_lengths)
        decoded = self._launch_greedy("decode", buf.probs, buf.input_len, buf.decoded, buf.decoded_len, buf.frame_argmax,
                                      buf.batch, buf.t_out)
        return decoded, buf.frame_argmax.cpu().numpy()

    def beam_search(self, decoder, prediction_lengths=None):
        """CTC beam search (decoder: decoder.GpuCtcBeamSearchDecoder) over the current probabilities, in place on the
        device: no host copy of the probabilities, no gradient buffers.  Returns (list of index lists, log-probabilities
        (B,) numpy), as the decoder's decode()."""
        buf = self.cur
        if prediction_lengths is not None:
            self.set_input_lengths(prediction_lengths)
        return decoder.decode(buf.probs, buf.input_len)  # launched on the current stream, behind forward()

    def _launch_asg_viterbi(self, tag, logq, lens, path, score, ws, b, t):
        """one ASG Viterbi decode of (b, t, K) emissions under the engine's scores into path (b * t int32) and score ->
        (index lists with repeats merged, per-frame paths (b, t) numpy with -1 past the utterance)"""
        trans, init = self._asg_views(self.asg_params)
        self._launch(tag, _VITERBI, logq.data_ptr(), trans.data_ptr(), init.data_ptr(), lens.data_ptr(), path.data_ptr(),
                     score.data_ptr(), b, t, self.grapheme_set_size, ws.data_ptr(), ws.numel(), self._stream())
        paths = path.view(b, t).cpu().numpy()
        return _merge_repeats(paths), paths

    def asg_viterbi(self, prediction_lengths=None):
        """greedy_decode() for the ASG criterion: the best letter sequence under emissions + scores (the ASG Viterbi kernel on
        the current logq), repeats merged.  Returns (list of index lists, per-frame path (B, T') numpy with -1 past T_b)."""
        self._require_asg("asg_viterbi()")
        buf = self.cur
        if prediction_lengths is not None:
            self.set_input_lengths(prediction_lengths)
        buf.grow("asg_vit_ws", self.lib.raw(_VITERBI + "_workspace_bytes")(buf.batch, buf.tt_pad, self.grapheme_set_size), 16)
        if buf.asg_score is None:
            buf.asg_score = torch.zeros((buf.batch,), dtype=torch.float32, device=self.device)
        # (the path goes where greedy_decode keeps its per-frame result: int32 (B, T'))
        return self._launch_asg_viterbi("asg_viterbi", buf.logq, buf.input_len, buf.frame_argmax, buf.asg_score, buf.asg_vit_ws,
                                        buf.batch, buf.t_out)

    def asg_beam_search(self, decoder, prediction_lengths=None):
        """asg_viterbi() with a beam and, if the decoder has one, the n-gram language model (decoder:
        decoder.GpuAsgBeamSearchDecoder): sl_asg_beam_search over the current logq and the engine's asg_trans / asg_init, in
        place on the device and on the current stream.  Returns (list of grapheme index lists, scores (B,) numpy)."""
        self._require_asg("asg_beam_search()")
        buf = self.cur
        if prediction_lengths is not None:
            self.set_input_lengths(prediction_lengths)
        trans, init = self._asg_views(self.asg_params)
        return decoder.decode(buf.logq, trans, init, buf.input_len)

    # ------------------------------------------------------------------ forced alignment

    def _long_logq(self, logq):
        """the logq argument of the _long methods, checked -> (contiguous logq, B, T')"""
        k = self.grapheme_set_size
        if logq.dim() != 3 or logq.shape[2] != k or logq.dtype != torch.float32 or not logq.is_cuda:
            raise ValueError("logq must be a float32 (B, T', {}) tensor on the device".format(k))
        return logq.contiguous(), int(logq.shape[0]), int(logq.shape[1])

    def _align(self, kind, long, logq, label_batch, label_lengths, prediction_lengths):
        """The four forced aligners (row _ALIGNERS[kind, long]): over the current buffer set's logq with its input lengths and
        tensors of that set (buf.align: frames = tt_pad), or -- long -- over a given logq with tensors of the engine's
        (_long_align).  Checks in this order: the criterion, logq (long), the labels.  Returns (paths int32 (B, T') numpy,
        scores float32 (B,) numpy)."""
        row = _ALIGNERS[kind, long]
        asg = kind == "asg"
        if asg:
            self._require_asg(row.entry[len("sl_"):] + "()")
        elif self.criterion == "asg":
            raise ValueError("criterion='asg': forced alignment runs over the CTC lattice (blank = K - 1); not supported")
        k = self.grapheme_set_size
        if long:
            buf, in_len = None, np.asarray(prediction_lengths, dtype=np.int32).reshape(-1)
            logq, batch, t_out = self._long_logq(logq)
            frames = t_out
        else:
            buf, in_len = self.cur, None
            logq, batch, t_out, frames = buf.logq, buf.batch, buf.t_out, buf.tt_pad
        labels, lab_len = check_label_batch(
            label_batch, label_lengths, batch, k if asg else k - 1, blank=None if asg else k - 1, in_len=in_len,
            max_letters=row.max_label, too_long_text=row.too_long and "{} ({})".format(row.too_long, row.entry))
        query = row.entry + "_workspace_bytes"
        if long:
            ab = self._long_align = self._long_align or _AlignBuffers(self.device, query)
        else:
            ab = buf.align = buf.align or _AlignBuffers(self.device, query)
        ab.ensure(batch, frames, max(int(labels.shape[1]), 1))
        ab.labels.zero_()  # (at least as wide as the labels)
        ab.labels[:, :labels.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(labels)))
        ab.label_len.copy_(torch.from_numpy(lab_len))
        if long:
            lens = ab.input_len
            lens.copy_(torch.from_numpy(in_len))
        else:
            self.set_input_lengths(prediction_lengths)
            lens = buf.input_len
        path = ab.path[:batch * t_out]
        scores = [t.data_ptr() for t in self._asg_views(self.asg_params)] if asg else []  # trans, init
        try:
            self._launch(row.tag, row.entry, logq.data_ptr(), *scores, ab.labels.data_ptr(), ab.label_len.data_ptr(),
                         lens.data_ptr(), path.data_ptr(), ab.score.data_ptr(), batch, t_out, k, ab.labels.shape[1],
                         ab.ws.data_ptr(), ab.ws.numel(), self._stream())
        except Exception:
            # a refused launch (labels wider than the entry point takes) must not leave its tensors behind: they are grown
            # only, and their width is the l_max of every later call on this buffer set
            if long:
                self._long_align = None
            else:
                buf.align = None
            raise
        return path.view(batch, t_out).cpu().numpy(), ab.score.cpu().numpy()

    def ctc_align(self, label_batch, label_lengths, prediction_lengths):
        """CTC forced alignment (Viterbi) of the labels on the current buffer set's logq -- the distribution ctc() sees --
        after forward().  label_batch: int (B, Lmax) padded with anything; lengths: (B,) or (B, 1).  Returns (paths int32
        (B, T') numpy: the lattice state of the best path per frame, -1 past the utterance's length or for every frame of
        an infeasible one; scores float32 (B,) numpy: its log-probability, -inf when infeasible).  Semantics: the entry point
        of the same name in include/speechless_hip.h.  Uses tensors of its own: no gradient buffers, labels of ctc()
        untouched."""
        return self._align("ctc", False, None, label_batch, label_lengths, prediction_lengths)

    def asg_align(self, label_batch, label_lengths, prediction_lengths):
        """ctc_align() for the ASG criterion: the best segmentation of the (run-length-encoded) labels over the frames under
        the current buffer set's logq -- the emissions asg_viterbi() sees -- and the engine's asg_trans / asg_init, after
        forward().  label_batch: int (B, Lmax) padded with anything; lengths: (B,) or (B, 1).  Returns (paths int32 (B, T')
        numpy: the label position of the best path per frame, -1 past the utterance's length or for every frame of an
        infeasible one; scores float32 (B,) numpy: the path's score, -inf when infeasible).  Semantics: the entry point of
        the same name in include/speechless_hip.h.  Uses tensors of its own: no gradient buffers, labels of asg() untouched."""
        return self._align("asg", False, None, label_batch, label_lengths, prediction_lengths)

    def ctc_align_long(self, logq, label_batch, label_lengths, prediction_lengths):
        """ctc_align() beyond 511 letters, on a given (B, T', K) fp32 logq tensor in HBM (forward_long's): one launch of the
        entry point of the same name (include/speechless_hip.h; labels of up to longform.ALIGN_MAX_LABEL letters).  Does not
        touch the current buffer set.  label_batch: int (B, Lmax) padded with anything; lengths: (B,) or (B, 1).  Returns
        (paths int32 (B, T') numpy, scores float32 (B,) numpy) as ctc_align does."""
        return self._align("ctc", True, logq, label_batch, label_lengths, prediction_lengths)

    def asg_align_long(self, logq, label_batch, label_lengths, prediction_lengths):
        """asg_align() beyond 511 graphemes, on a given (B, T', K) fp32 logq tensor in HBM (forward_long's) and the engine's
        asg_trans / asg_init: one launch of the entry point of the same name (include/speechless_hip.h; encoded labels of up
        to longform.ASG_ALIGN_MAX_LABEL graphemes).  Does not touch the current buffer set.  label_batch: int (B, Lmax) padded
        with anything; lengths: (B,) or (B, 1).  Returns (paths int32 (B, T') numpy, scores float32 (B,) numpy) as asg_align
        does."""
        return self._align("asg", True, logq, label_batch, label_lengths, prediction_lengths)

    # ------------------------------------------------------------------ segment posteriors

    def _segment_scores(self, kind, long, logq, label_batch, prediction_lengths, segments):
        """The two segment-posterior kernels (row _SEGMENTERS[kind]) over the current buffer set's logq with its input lengths
        (tensors: buf.segment), or -- long -- over a given logq with its prediction lengths (tensors: _long_segment).  Checks in
        _align's order: the criterion, logq (long), the segments, the labels -- of each row the positions that some segment
        covers.  Returns float32 (N,) numpy."""
        row = _SEGMENTERS[kind]
        tag = row.tag + ("_long" if long else "")
        if row.asg:
            self._require_asg(tag + "()")
        elif self.criterion == "asg":
            raise ValueError("criterion='asg': segment posteriors run over the CTC lattice (blank = K - 1); not supported")
        k = self.grapheme_set_size
        if long:
            buf, in_len = None, np.asarray(prediction_lengths, dtype=np.int32).reshape(-1)
            logq, batch, t_out = self._long_logq(logq)
        else:
            buf, in_len = self.cur, None
            logq, batch, t_out = buf.logq, buf.batch, buf.t_out
        seg = check_segments(segments, batch, kind)
        labels = np.asarray(label_batch, dtype=np.int32)
        covered = np.zeros((batch,), dtype=np.int32)
        np.maximum.at(covered, seg[:, 0], seg[:, 4])
        labels, _ = check_label_batch(labels, np.minimum(covered, labels.shape[1] if labels.ndim == 2 else 0), batch,
                                      k if row.asg else k - 1, blank=None if row.asg else k - 1, in_len=in_len)
        n, seg_l_max = int(seg.shape[0]), int((seg[:, 4] - seg[:, 3]).max())
        query = (row.entry + "_workspace_bytes", (k,) if row.asg else ())
        if long:
            sb = self._long_segment = self._long_segment or _SegmentBuffers(self.device, *query)
        else:
            sb = buf.segment = buf.segment or _SegmentBuffers(self.device, *query)
        sb.ensure(batch, max(int(labels.shape[1]), 1), n, seg_l_max)
        sb.labels.zero_()  # (at least as wide as the labels)
        sb.labels[:, :labels.shape[1]].copy_(torch.from_numpy(np.ascontiguousarray(labels)))
        sb.segments[:n].copy_(torch.from_numpy(seg))
        if long:
            lens = sb.input_len
            lens.copy_(torch.from_numpy(in_len))
        else:
            lens = buf.input_len
        scores = [t.data_ptr() for t in self._asg_views(self.asg_params)] if row.asg else []  # trans, init
        self._launch(tag, row.entry, logq.data_ptr(), *scores, sb.labels.data_ptr(), lens.data_ptr(), sb.segments.data_ptr(),
                     sb.out.data_ptr(), batch, t_out, k, sb.labels.shape[1], n, seg_l_max, sb.ws.data_ptr(), sb.ws.numel(),
                     self._stream())
        return sb.out[:n].cpu().numpy()

    def ctc_segment_scores(self, label_batch, segments):
        """CTC segment posteriors on the current buffer set's logq after forward(), under the input lengths of the last
        set_input_lengths (ctc_align sets them): per row {b, frame_begin, frame_end, label_begin, label_end} of segments -- an
        (N, 5) integer array, half-open ranges -- the log of the probability that those frames of utterance b, read on their
        own, say exactly those letters of row b of label_batch (int (B, Lmax); at most longform.SEGMENT_MAX_LABEL letters per
        segment).  With a word's range of a forced alignment: the word's confidence; over all frames and the whole label: minus
        the CTC loss.  Returns float32 (N,) numpy, -inf where the frames cannot hold the letters.  Semantics: the entry point
        sl_ctc_segment_scores of include/speechless_hip.h.  Uses tensors of its own, reused across calls."""
        return self._segment_scores("ctc", False, None, label_batch, None, segments)

    def ctc_segment_scores_long(self, logq, label_batch, prediction_lengths, segments):
        """ctc_segment_scores() on a given (B, T', K) fp32 logq tensor in HBM (forward_long's) with its B prediction lengths:
        one launch whatever the number of segments.  Does not touch the current buffer set."""
        return self._segment_scores("ctc", True, logq, label_batch, prediction_lengths, segments)

    def asg_segment_scores(self, label_batch, segments):
        """ctc_segment_scores() for the ASG criterion, on the current buffer set's logq -- the emissions asg_viterbi() and
        asg_align() see -- and the engine's asg_trans / asg_init, under the input lengths of the last set_input_lengths
        (asg_align sets them): per segment row the constrained forward score of those ENCODED graphemes of row b of label_batch
        (indices in [0, K), no blank; at most longform.ASG_SEGMENT_MAX_LABEL per segment) over those frames minus the forward
        score of the full graph over the same frames, both started from g0 where the segment begins the label and else from the
        scores out of the grapheme before it: the log of a proper probability.  Over all frames and the whole label: minus the
        ASG loss.  Returns float32 (N,) numpy, -inf where the frames cannot hold the graphemes or -inf scores close every path.
        Semantics: the entry point sl_asg_segment_scores of include/speechless_hip.h.  Uses tensors of its own."""
        return self._segment_scores("asg", False, None, label_batch, None, segments)

    def asg_segment_scores_long(self, logq, label_batch, prediction_lengths, segments):
        """asg_segment_scores() on a given (B, T', K) fp32 logq tensor in HBM (forward_long's) with its B prediction lengths:
        one launch whatever the number of segments.  Does not touch the current buffer set."""
        return self._segment_scores("asg", True, logq, label_batch, prediction_lengths, segments)

    # ------------------------------------------------------------------ phrase search

    def _spot(self, long, logq, queries, query_lengths, query_utterances, min_scores, max_hits, prediction_lengths):
        """sl_ctc_spot over the current buffer set's logq with its input lengths (tensors: buf.spot), or -- long -- over a given
        logq with its prediction lengths (tensors: _long_spot).  Checks in _segment_scores' order: the criterion, logq (long),
        the queries.  Returns (hits int32 (N, max_hits, 2), scores float32 (N, max_hits), counts int32 (N,)) numpy."""
        tag = "spot_long" if long else "spot"
        if self.criterion == "asg":
            raise ValueError("criterion='asg': the phrase search runs over the CTC lattice (blank = K - 1); not supported")
        k = self.grapheme_set_size
        if long:
            buf, in_len = None, np.asarray(prediction_lengths, dtype=np.int32).reshape(-1)
            logq, batch, t_out = self._long_logq(logq)
            if in_len.shape[0] != batch:
                raise ValueError("ctc_spot_long needs B prediction lengths")
        else:
            buf = self.cur
            logq, batch, t_out = buf.logq, buf.batch, buf.t_out
        queries, lengths, utterances, thresholds, max_hits = check_queries(queries, query_lengths, query_utterances, min_scores,
                                                                           max_hits, batch, k - 1)
        n, q_max = queries.shape
        if long:
            sp = self._long_spot = self._long_spot or _SpotBuffers(self.device)
        else:
            sp = buf.spot = buf.spot or _SpotBuffers(self.device)
        sp.ensure(batch, t_out, n, q_max, max_hits)
        sp.queries.zero_()  # (at least as wide as the queries)
        sp.queries[:n, :q_max].copy_(torch.from_numpy(queries))
        sp.query_len[:n].copy_(torch.from_numpy(lengths))
        sp.query_utt[:n].copy_(torch.from_numpy(utterances))
        sp.min_score[:n].copy_(torch.from_numpy(thresholds))
        if long:
            lens = sp.input_len
            lens.copy_(torch.from_numpy(in_len))
        else:
            if prediction_lengths is not None:
                self.set_input_lengths(prediction_lengths)
            lens = buf.input_len
        self._launch(tag, _SPOT, logq.data_ptr(), lens.data_ptr(), sp.queries.data_ptr(), sp.query_len.data_ptr(),
                     sp.query_utt.data_ptr(), sp.min_score.data_ptr(), sp.hits.data_ptr(), sp.hit_score.data_ptr(),
                     sp.n_hits.data_ptr(), None, None, batch, t_out, k, n, sp.queries.shape[1], max_hits, sp.ws.data_ptr(),
                     sp.ws.numel(), self._stream())
        return (sp.hits[:n * max_hits * 2].view(n, max_hits, 2).cpu().numpy(), sp.hit_score[:n * max_hits].view(n, max_hits).cpu().numpy(),
                sp.n_hits[:n].cpu().numpy())

    def ctc_spot(self, queries, query_lengths, query_utterances, min_scores, max_hits, prediction_lengths=None):
        """CTC phrase search on the current buffer set's logq after forward(): where each query -- row i of queries (int (N,
        Qmax), padded with anything), its first query_lengths[i] letters -- is said in utterance query_utterances[i], under the
        input lengths of the last set_input_lengths (or prediction_lengths, which sets them).  Up to max_hits (1 .. 64)
        occurrences per query that do not overlap, best first, each with the log-probability of its best path of at least
        min_scores[i] (-inf: any finite score).  Returns (hits int32 (N, max_hits, 2) numpy: output frames [first, end), -1 in
        unused slots; scores float32 (N, max_hits) numpy, -inf there; counts int32 (N,) numpy).  Semantics: the entry point
        sl_ctc_spot of include/speechless_hip.h.  Uses tensors of its own, reused across calls; one launch whatever the number of
        queries, outside every recorded launch list."""
        return self._spot(False, None, queries, query_lengths, query_utterances, min_scores, max_hits, prediction_lengths)

    def ctc_spot_long(self, logq, queries, query_lengths, query_utterances, min_scores, max_hits, prediction_lengths):
        """ctc_spot() on a given (B, T', K) fp32 logq tensor in HBM (forward_long's) with its B prediction lengths: one launch
        whatever the number of queries and frames (the workspace takes 8 bytes per query and frame).  Does not touch the current
        buffer set."""
        return self._spot(True, logq, queries, query_lengths, query_utterances, min_scores, max_hits, prediction_lengths)

    # ------------------------------------------------------------------ long recordings (longform.py)

    def forward_long(self, input_2d, window_input_frames=None, batch_windows=8):
        """forward() over a recording of any length: the windows of longform.window_plan run through forward() in batches of
        up to batch_windows, and the output frames of each that equal a single pass over the whole recording are copied on
        the device into tensors of this call's own.  input_2d: (T, F) numpy or float32 tensor.  Returns (probs, logq), fp32
        (1, ceil(T / ratio), K) in HBM; nothing but the input crosses PCIe.  window_input_frames: None = DEFAULT_WINDOW."""
        if self.front_plan is not None:
            raise ValueError("forward_long: raw-wave input is not supported (the window geometry of the sample-rate front "
                             "layer is out of scope)")
        if isinstance(input_2d, np.ndarray):
            src = torch.from_numpy(np.ascontiguousarray(input_2d, dtype=np.float32)).to(self.device, non_blocking=True)
        else:
            src = input_2d.to(device=self.device, dtype=torch.float32).contiguous()
        if src.dim() != 2 or src.shape[0] < 1:
            raise ValueError("forward_long takes one recording: (frames, bins) with at least one frame")
        window = longform.DEFAULT_WINDOW if window_input_frames is None else int(window_input_frames)
        plan = longform.window_plan(int(src.shape[0]), self.plans, window)
        k = self.grapheme_set_size
        frames_out = plan[-1].out_end
        probs = torch.empty((1, frames_out, k), dtype=torch.float32, device=self.device)
        logq = torch.empty((1, frames_out, k), dtype=torch.float32, device=self.device)
        step = max(int(batch_windows), 1)
        for i in range(0, len(plan), step):
            part = plan[i:i + step]
            batch = torch.stack([src[w.input_start:w.input_start + w.input_length] for w in part])
            self.forward(batch)
            buf = self.cur
            for row, w in enumerate(part):
                probs[0, w.out_start:w.out_end].copy_(buf.probs[row, w.keep_start:w.keep_end])
                logq[0, w.out_start:w.out_end].copy_(buf.logq[row, w.keep_start:w.keep_end])
        return probs, logq

    def greedy_decode_long(self, probs):
        """Greedy CTC decode (greedy_decode's kernel) of a (B, T', K) fp32 probability tensor in HBM, e.g. forward_long's, over
        all of its frames.  Returns a list of index lists.  The kernel keeps a recording's frame argmax in LDS: beyond
        longform.GREEDY_DECODE_MAX_FRAMES output frames it raises longform.RecordingTooLongError."""
        b, t_out, _ = probs.shape
        if t_out > longform.GREEDY_DECODE_MAX_FRAMES:
            raise longform.RecordingTooLongError(
                "greedy decoding takes at most {} output frames per recording ({} keeps them in LDS), not {}".format(
                    longform.GREEDY_DECODE_MAX_FRAMES, _GREEDY, t_out))
        if t_out == 0:
            return [[] for _ in range(b)]
        dev = self.device
        lens = torch.full((b,), t_out, dtype=torch.int32, device=dev)
        out = torch.zeros((b, t_out), dtype=torch.int32, device=dev)
        out_len = torch.zeros((b,), dtype=torch.int32, device=dev)
        return self._launch_greedy("decode_long", probs.contiguous(), lens, out, out_len, None, b, t_out)

    def asg_viterbi_long(self, logq):
        """asg_viterbi() on a given (B, T', K) fp32 logq tensor in HBM (forward_long's), over all of its frames: one launch
        of asg_viterbi's kernel whose workspace is sized for that T' (its backpointers spill there, so T' has no limit but
        memory).  Does not touch the current buffer set.  Returns (list of index lists with repeats merged as asg_viterbi
        merges them, per-frame paths (B, T') numpy)."""
        self._require_asg("asg_viterbi_long()")
        logq, batch, t_out = self._long_logq(logq)
        if t_out == 0:
            return [[] for _ in range(batch)], np.zeros((batch, 0), dtype=np.int32)
        if self._long_viterbi is None:
            self._long_viterbi = _AlignBuffers(self.device, _VITERBI + "_workspace_bytes")
        lv = self._long_viterbi
        lv.ensure(batch, t_out, self.grapheme_set_size)  # (its workspace query takes the class count; the labels go unused)
        lv.input_len.fill_(t_out)
        return self._launch_asg_viterbi("asg_viterbi_long", logq, lv.input_len, lv.path[:batch * t_out], lv.score, lv.ws,
                                        batch, t_out)

    # ------------------------------------------------------------------ error counts

    def error_counts(self, space_index):
        """Letter and word error counts of the greedy transcriptions against the labels, after forward() + set_labels() +
        greedy_decode(): one sl_edit_distance launch on buf.labels / label_len and buf.decoded / decoded_len where they lie.
        space_index: the word separator's index, < 0 for an alphabet without one.  Returns (letter_errors, word_errors),
        int32 (B,) numpy -- net.edit_distance of the decoded strings and of their .split()."""
        buf = self.cur
        return self._edit_distance(buf, buf.labels, buf.label_len, buf.decoded, buf.decoded_len, space_index)

    def edit_distance_batch(self, expected_rows, predicted_rows, space_index):
        """error_counts for index lists that live on the host, as the beam decoders return them: pads both sides, uploads
        them in one copy and makes the same launch.  Returns the same tuple.  Any number of rows; the staging and result
        tensors belong to the current buffer set, so a forward pass (or load_input) comes first."""
        if len(expected_rows) != len(predicted_rows) or len(expected_rows) == 0:
            raise ValueError("need as many expected as predicted rows, and at least one")
        buf = self.cur
        a, a_len = pack_rows(expected_rows)
        b, b_len = pack_rows(predicted_rows)
        n = len(a_len)
        staged = buf.ensure_edit_rows(self, a.size + b.size + 2 * n)
        staged.copy_(torch.from_numpy(np.concatenate([a.ravel(), b.ravel(), a_len, b_len])))
        a_dev, b_dev, a_len_dev, b_len_dev = staged.split([a.size, b.size, n, n])
        return self._edit_distance(buf, a_dev.view(a.shape), a_len_dev, b_dev.view(b.shape), b_len_dev, space_index)

    def _edit_distance(self, buf, a, a_len, b, b_len, space_index):
        n, a_max, b_max = int(a.shape[0]), int(a.shape[1]), int(b.shape[1])
        if not self.lib.raw("sl_edit_distance_supported")(a_max, b_max):
            # rows beyond what the kernel keeps in LDS (include/speechless_hip.h): the host function counts this batch
            a, a_len, b, b_len = (t.cpu().numpy() for t in (a, a_len, b, b_len))
            return host_counts([a[i, :a_len[i]].tolist() for i in range(n)], [b[i, :b_len[i]].tolist() for i in range(n)],
                               space_index)
        out = buf.ensure_error_counts(self, n)
        self._launch("edit_distance", "sl_edit_distance", a.data_ptr(), a_len.data_ptr(), a.stride(0), b.data_ptr(),
                     b_len.data_ptr(), b.stride(0), n, a_max, b_max, int(space_index), out[0].data_ptr(), out[1].data_ptr(),
                     out[2].data_ptr(), self._stream())
        counts = out.cpu().numpy()
        if (counts[:2] < 0).any():
            raise ValueError("utterance {}: a length outside its row (expected rows hold {}, predicted rows {})".format(
                int(np.argmax((counts[:2] < 0).any(axis=0))), a_max, b_max))
        return counts[0].copy(), counts[1].copy()
