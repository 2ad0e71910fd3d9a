#!/usr/bin/env python
"""sl_ctc_spot (csrc/ctc_spot.hip) alone: microseconds per call, HIP events around each of --iters calls after --warmup, on the
batches of tools/segment_score_time.py (the learnt-alignment regime of tools/fuzz_ctc.py), the calls of a group taking turns call
by call in the same run:
  config 3's shape -- 32 x 500 frames: every word of the batch (660 at the default seed) as a query in its own utterance, one
  launch; the 32 whole labels (100 .. 120 letters) as one query per utterance, one launch -- the same letters, frames and waves
  as sl_ctc_align, whose per-frame time it is held against; beside sl_ctc_align and sl_ctc_segment_scores over every word;
  one recording of 30 000 frames: 1, 64 and 1024 of its words as queries, one launch each, 8 hits per query.
One JSON line per measurement; --out writes them as a list (profiles/ctc_spot_time.json).

    python tools/ctc_spot_time.py --out profiles/ctc_spot_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from segment_score_time import ALPHABET, K, Case, take_turns  # noqa: E402

MAX_HITS = 8


def spot_call(case, phrases, utterances, what):
    """one sl_ctc_spot call over the case's logq: phrases (strings) searched in the utterances of the same index"""
    import torch
    dev = "cuda:0"
    n, q_max = len(phrases), max(len(p) for p in phrases)
    queries = np.zeros((n, q_max), dtype=np.int32)
    for row, p in zip(queries, phrases):
        row[:len(p)] = [ALPHABET.index(c) for c in p]
    qs = torch.tensor(queries, device=dev)
    ql = torch.tensor([len(p) for p in phrases], dtype=torch.int32, device=dev)
    qu = torch.tensor(list(utterances), dtype=torch.int32, device=dev)
    ms = torch.full((n,), float("-inf"), dtype=torch.float32, device=dev)
    hits = torch.zeros((n, MAX_HITS, 2), dtype=torch.int32, device=dev)
    hit_score = torch.zeros((n, MAX_HITS), dtype=torch.float32, device=dev)
    n_hits = torch.zeros((n,), dtype=torch.int32, device=dev)
    need = case.lib.raw("sl_ctc_spot_workspace_bytes")(n, case.frames, q_max)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    case.keep += [qs, ql, qu, ms, hits, hit_score, n_hits, ws]
    return dict(name="sl_ctc_spot", what=what, queries=n, q_max=q_max, workspace_bytes=int(need), n_hits=n_hits, best=hit_score,
                args=(case.logq.data_ptr(), case.il.data_ptr(), qs.data_ptr(), ql.data_ptr(), qu.data_ptr(), ms.data_ptr(),
                      hits.data_ptr(), hit_score.data_ptr(), n_hits.data_ptr(), None, None, case.batch, case.frames, K, n, q_max,
                      MAX_HITS, ws.data_ptr(), need, case.st))


def timed(lib, calls, warmup, iters, frames):
    rows = take_turns(lib, calls, warmup, iters)
    for r, c in zip(rows, calls):
        r["ns_per_frame"] = 1e3 * r["us_median"] / frames
        if c["name"] == "sl_ctc_spot":
            best = c["best"].cpu().numpy()[:, 0]
            r.update(queries=c["queries"], q_max=c["q_max"], workspace_bytes=c["workspace_bytes"], max_hits=MAX_HITS,
                     hits=int(c["n_hits"].cpu().numpy().sum()), mean_best_log_probability=float(best[np.isfinite(best)].mean()))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    args = ap.parse_args()
    from speechless_amd._lib import lib as load
    lib = load()
    results = []

    def report(rows, **extra):
        for r in rows:
            r.update(extra)
            results.append(r)
            print(json.dumps(r), flush=True)

    rng = np.random.RandomState(args.seed)
    case = Case(lib, 32, 500, rng.randint(100, 121, size=32), False, args.seed + 1)
    words = [(b, w) for b, a in enumerate(case.alignments) for w, _ in a.word_frames]
    report(timed(lib, [spot_call(case, [w for _, w in words], [b for b, _ in words], "every word in its utterance"),
                       spot_call(case, case.texts, range(32), "every whole label in its utterance"),
                       case.segment_call(case.word_segments(False), "every word"), case.align], args.warmup, args.iters, 500),
           shape="config 3: 32 x 500 frames", words=len(words))
    del case
    case = Case(lib, 1, 30000, [8000], True, args.seed + 2)
    words = [w for w, _ in case.alignments[0].word_frames]
    calls = [spot_call(case, [words[(7 * i) % len(words)] for i in range(n)], [0] * n, "{} of its words".format(n))
             for n in (1, 64, 1024)]
    report(timed(lib, calls, args.warmup, args.iters, 30000), shape="one recording: 30000 frames", words=len(words))
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
