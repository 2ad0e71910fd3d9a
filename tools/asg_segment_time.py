#!/usr/bin/env python
"""sl_asg_segment_scores (csrc/asg_segment.hip) alone: microseconds per call, HIP events around each of --iters calls after
--warmup, on the learnt-alignment regime of tests/asg_cases.py, beside sl_ctc_segment_scores on the same frames, labels and
segments (which reads the last class, the thrice mark that these labels never hold, as its blank) and beside the ASG forced
aligner that produced the word ranges, all taking turns call by call in the same run:
  32 x 500 frames, about 20 words per utterance: every word over its aligned frames and every whole utterance, one launch,
  beside sl_asg_align;
  one recording of 30 000 frames and 8000 encoded graphemes: every word, and every section of
  alignment.cut_section_grapheme_spans at 1000 frames, one launch each, beside sl_asg_align_long.
One JSON line per measurement; --out writes them as a list (profiles/asg_segment_time.json).

    python tools/asg_segment_time.py --out profiles/asg_segment_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))

LETTERS = "abcdefghijklmnopqrstuvwxyz"


def random_label(rng, enc, graphemes):
    """words of 1 .. 8 letters (about 4.5 and a space) with runs of two here and there and none of three, whose ENCODING has
    exactly `graphemes` graphemes"""
    text = ""
    while len(enc.encode(text)) < graphemes:
        word = ""
        for c in rng.randint(0, 26, size=rng.randint(1, 9)):
            if len(word) >= 2 and word[-1] == word[-2] == LETTERS[c]:
                c = (c + 1) % 26
            word += LETTERS[c]
        text += word + " "
    while len(enc.encode(text)) > graphemes or text.endswith(" "):
        text = text[:-1]
    while len(enc.encode(text)) < graphemes:  # (a letter that differs from the one before adds exactly one grapheme)
        text += "b" if text.endswith("a") else "a"
    return text


class Case:
    """logq, tables, encoded labels and the aligner's call on them; the aligner runs once here, for the word ranges"""

    def __init__(self, lib, batch, frames, graphemes, long, seed):
        import torch
        from asg_cases import asg_regime_logits
        from speechless_amd import english_frequent_characters
        from speechless_amd.alignment import AsgAlignment
        from speechless_amd.grapheme_encoding import AsgGraphemeEncoding
        enc = AsgGraphemeEncoding(english_frequent_characters)
        k = self.k = enc.grapheme_set_size
        rng = np.random.RandomState(seed)
        dev = "cuda:0"
        self.lib, self.batch, self.frames = lib, batch, frames
        self.texts = [random_label(rng, enc, int(n)) for n in graphemes]
        encoded = [enc.encode(t) for t in self.texts]
        assert all(enc.asg_thrice not in e for e in encoded)
        width = max(len(e) for e in encoded)
        labels = np.zeros((batch, width), dtype=np.int32)
        logits = np.zeros((batch, frames, k), dtype=np.float32)
        for i, e in enumerate(encoded):
            labels[i, :len(e)] = e
            logits[i] = asg_regime_logits(rng, e, frames, k, "learnt")
        lg = torch.tensor(logits, device=dev)
        probs, self.logq = torch.zeros_like(lg), torch.zeros_like(lg)
        self.trans = torch.tensor(rng.uniform(-1, 1, size=(k, k)).astype(np.float32), device=dev)
        self.init = torch.tensor(rng.uniform(-1, 1, size=k).astype(np.float32), device=dev)
        self.lab = torch.tensor(labels, device=dev)
        self.ll = torch.tensor([len(e) for e in encoded], dtype=torch.int32, device=dev)
        self.il = torch.full((batch,), frames, dtype=torch.int32, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream
        lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), self.logq.data_ptr(), batch, frames, k, k, frames * k, 1e-8,
                 self.st)
        name = "sl_asg_align_long" if long else "sl_asg_align"
        self.path = torch.zeros((batch, frames), dtype=torch.int32, device=dev)
        self.score = torch.zeros((batch,), dtype=torch.float32, device=dev)
        need = lib.raw(name + "_workspace_bytes")(batch, frames, width)
        self.ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.align = dict(name=name, what="aligner", args=(
            self.logq.data_ptr(), self.trans.data_ptr(), self.init.data_ptr(), self.lab.data_ptr(), self.ll.data_ptr(),
            self.il.data_ptr(), self.path.data_ptr(), self.score.data_ptr(), batch, frames, k, width, self.ws.data_ptr(), need,
            self.st))
        lib.call(name, *self.align["args"])
        paths, scores = self.path.cpu().numpy(), self.score.cpu().numpy()
        self.alignments = [AsgAlignment.from_path(t, e, enc.asg_twice, enc.asg_thrice, s, p)
                           for t, e, s, p in zip(self.texts, encoded, scores, paths)]
        self.keep = []

    def segment_calls(self, segments, what):
        """the ASG call and the CTC call on the same segments"""
        import torch
        seg = np.ascontiguousarray(segments, dtype=np.int32)
        n, seg_l_max = seg.shape[0], int((seg[:, 4] - seg[:, 3]).max())
        sg = torch.tensor(seg, device="cuda:0")
        calls = []
        for name in ("sl_asg_segment_scores", "sl_ctc_segment_scores"):
            out = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
            self.keep += [sg, out]
            tables = (self.trans.data_ptr(), self.init.data_ptr()) if "asg" in name else ()
            calls.append(dict(name=name, what=what, segments=n, seg_l_max=seg_l_max, out=out, args=(
                self.logq.data_ptr(), *tables, self.lab.data_ptr(), self.il.data_ptr(), sg.data_ptr(), out.data_ptr(), self.batch,
                self.frames, self.k, self.lab.shape[1], n, seg_l_max, None, 0, self.st)))
        return calls

    def word_segments(self, whole):
        from speechless_amd.alignment import grapheme_spans, word_spans
        segments = []
        for b, a in enumerate(self.alignments):
            spans = grapheme_spans(a.label, word_spans(a.label))
            segments += [(b, first, end, g0, g1) for (_, (first, end)), (g0, g1) in zip(a.word_frames, spans)]
            if whole:
                segments.append((b, 0, self.frames, 0, len(a.encoded_label)))
        return segments


def take_turns(lib, calls, warmup, iters):
    """every call once per round, so that all see the same clocks and the same state of the caches; microseconds per call"""
    import torch
    times = [[] for _ in calls]
    for i in range(warmup + iters):
        for j, c in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lib.call(c["name"], *c["args"])
            b.record()
            b.synchronize()
            if i >= warmup:
                times[j].append(1e3 * a.elapsed_time(b))
    rows = []
    for c, ts in zip(calls, times):
        r = {"call": c["name"], "what": c["what"], "iters": iters, "us_median": float(np.median(ts)), "us_min": float(np.min(ts)),
             "us_max": float(np.max(ts))}
        if "out" in c:
            out = c["out"].cpu().numpy()
            r.update(segments=c["segments"], seg_l_max=c["seg_l_max"], finite=int(np.isfinite(out).sum()),
                     mean_log_posterior=float(out[np.isfinite(out)].mean()) if np.isfinite(out).any() else None)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    args = ap.parse_args()
    from speechless_amd._lib import lib as load
    from speechless_amd.alignment import cut_section_grapheme_spans
    lib = load()
    results = []

    def report(rows, **extra):
        for r in rows:
            r.update(extra)
            results.append(r)
            print(json.dumps(r), flush=True)

    rng = np.random.RandomState(args.seed)
    case = Case(lib, 32, 500, rng.randint(100, 121, size=32), False, args.seed + 1)
    words = sum(len(a.word_frames) for a in case.alignments)
    report(take_turns(lib, case.segment_calls(case.word_segments(True), "every word and every whole utterance") + [case.align],
                      args.warmup, args.iters), shape="32 x 500 frames", words=words)
    del case
    case = Case(lib, 1, 30000, [8000], True, args.seed + 2)
    sections = [(0, first, end, g0, g1) for _, (first, end), (g0, g1) in cut_section_grapheme_spans(case.alignments[0], 1000)]
    report(take_turns(lib, case.segment_calls(case.word_segments(False), "every word") +
                      case.segment_calls(sections, "every section of 1000 frames") + [case.align], args.warmup, args.iters),
           shape="one recording: 30000 frames, 8000 encoded graphemes", words=len(case.alignments[0].word_frames),
           sections=len(sections))
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
