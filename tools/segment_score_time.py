#!/usr/bin/env python
"""sl_ctc_segment_scores (csrc/ctc_segment.hip) alone: microseconds per call, HIP events around each of --iters calls after
--warmup, on the learnt-alignment regime of tools/fuzz_ctc.py, each beside the forced aligner that produced its word ranges, the
two taking turns call by call in the same run:
  config 3's shape -- 32 x 500 frames, about 20 words per utterance: every word over its aligned frames and every whole
  utterance, one launch, beside sl_ctc_align;
  one recording of 30 000 frames and 8000 letters: every word, and every section of alignment.cut_section_spans at 1000 frames,
  one launch each, beside sl_ctc_align_long.
One JSON line per measurement; --out writes them as a list (profiles/segment_score_time.json).

    python tools/segment_score_time.py --out profiles/segment_score_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

K = 29  # a .. z, the space, one more, the blank
SPACE = 26
ALPHABET = "abcdefghijklmnopqrstuvwxyz "


def random_label(rng, letters):
    """words of 1 .. 8 letters (about 4.5 and a space: 20 words in 110 letters), exactly `letters` characters"""
    text = ""
    while len(text) < letters:
        text += "".join(ALPHABET[c] for c in rng.randint(0, 26, size=rng.randint(1, 9))) + " "
    return text[:letters].rstrip(" ").ljust(letters, "a")


class Case:
    """logq, labels and the aligner's call on them; the aligner runs once here, for the word ranges"""

    def __init__(self, lib, batch, frames, letters, long, seed):
        import torch
        from fuzz_ctc import regime_logits
        from speechless_amd.alignment import CtcAlignment
        rng = np.random.RandomState(seed)
        dev = "cuda:0"
        self.lib, self.batch, self.frames = lib, batch, frames
        self.texts = [random_label(rng, int(n)) for n in letters]
        width = max(len(t) for t in self.texts)
        labels = np.zeros((batch, width), dtype=np.int32)
        logits = np.zeros((batch, frames, K), dtype=np.float32)
        for i, text in enumerate(self.texts):
            labels[i, :len(text)] = [ALPHABET.index(c) for c in text]
            logits[i] = regime_logits(rng, list(labels[i, :len(text)]), frames, K, "learnt")
        lg = torch.tensor(logits, device=dev)
        probs, self.logq = torch.zeros_like(lg), torch.zeros_like(lg)
        self.lab = torch.tensor(labels, device=dev)
        self.ll = torch.tensor([len(t) for t in self.texts], dtype=torch.int32, device=dev)
        self.il = torch.full((batch,), frames, dtype=torch.int32, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream
        lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), self.logq.data_ptr(), batch, frames, K, K, frames * K, 1e-8,
                 self.st)
        name = "sl_ctc_align_long" if long else "sl_ctc_align"
        self.path = torch.zeros((batch, frames), dtype=torch.int32, device=dev)
        self.score = torch.zeros((batch,), dtype=torch.float32, device=dev)
        need = lib.raw(name + "_workspace_bytes")(batch, frames, width)
        self.ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.align = dict(name=name, what="aligner", args=(
            self.logq.data_ptr(), self.lab.data_ptr(), self.ll.data_ptr(), self.il.data_ptr(), self.path.data_ptr(),
            self.score.data_ptr(), batch, frames, K, width, self.ws.data_ptr(), need, self.st))
        lib.call(name, *self.align["args"])
        paths, scores = self.path.cpu().numpy(), self.score.cpu().numpy()
        self.alignments = [CtcAlignment.from_path(t, s, p) for t, s, p in zip(self.texts, scores, paths)]
        self.keep = []

    def segment_call(self, segments, what):
        import torch
        seg = np.ascontiguousarray(segments, dtype=np.int32)
        n, seg_l_max = seg.shape[0], int((seg[:, 4] - seg[:, 3]).max())
        sg = torch.tensor(seg, device="cuda:0")
        out = torch.zeros((n,), dtype=torch.float32, device="cuda:0")
        self.keep += [sg, out]
        return dict(name="sl_ctc_segment_scores", what=what, segments=n, seg_l_max=seg_l_max, out=out, args=(
            self.logq.data_ptr(), self.lab.data_ptr(), self.il.data_ptr(), sg.data_ptr(), out.data_ptr(), self.batch, self.frames, K,
            self.lab.shape[1], n, seg_l_max, None, 0, self.st))

    def word_segments(self, whole):
        from speechless_amd.alignment import word_spans
        segments = []
        for b, a in enumerate(self.alignments):
            segments += [(b, first, end, c0, c1) for (_, (first, end)), (c0, c1) in zip(a.word_frames, word_spans(a.label))]
            if whole:
                segments.append((b, 0, self.frames, 0, len(a.label)))
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
                     mean_log_posterior=float(out[np.isfinite(out)].mean()))
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
    from speechless_amd.alignment import cut_section_spans
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
    report(take_turns(lib, [case.segment_call(case.word_segments(True), "every word and every whole utterance"), case.align],
                      args.warmup, args.iters), shape="config 3: 32 x 500 frames", words=words)
    del case
    case = Case(lib, 1, 30000, [8000], True, args.seed + 2)
    sections = [(0, first, end, c0, c1) for _, (first, end), (c0, c1) in cut_section_spans(case.alignments[0], 1000)]
    report(take_turns(lib, [case.segment_call(case.word_segments(False), "every word"),
                            case.segment_call(sections, "every section of 1000 frames"), case.align], args.warmup, args.iters),
           shape="one recording: 30000 frames, 8000 letters", words=len(case.alignments[0].word_frames), sections=len(sections))
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
