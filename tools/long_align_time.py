#!/usr/bin/env python
"""sl_ctc_align_long alone: ms per call, HIP events around each of --iters calls after --warmup, on logq of a learnt-alignment
regime (tools/fuzz_ctc.py), at two shapes:
  1 x 30 000 frames with an 8000-letter label (a ten-minute recording's lattice, 16 waves), and
  8 x 4000 frames with labels of 300 .. 511 letters (the config-5 shard of tools/align_time.py, 1 wave), where sl_ctc_align --
  the default for such labels -- takes turns with it, call by call, in the same run.
One JSON line per shape; --out writes them as a list (profiles/long_align_time.json).

    python tools/long_align_time.py --out profiles/long_align_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

# batch, frames, shortest label, longest label, also time sl_ctc_align
SHAPES = [(1, 30000, 8000, 8000, False), (8, 4000, 300, 511, True)]


def time_shape(lib, batch, frames, l_lo, l_hi, both, k, warmup, iters, seed):
    import torch
    from fuzz_ctc import regime_logits
    rng = np.random.RandomState(seed)
    dev = "cuda:0"
    lens = [int(rng.randint(l_lo, l_hi + 1)) for _ in range(batch)]
    lens[0] = l_hi  # the launch's l_max (waves per recording) is that of the longest label
    labels = np.zeros((batch, l_hi), dtype=np.int32)
    logits = np.zeros((batch, frames, k), dtype=np.float32)
    for i, n in enumerate(lens):
        labels[i, :n] = rng.randint(0, k - 1, size=n)
        logits[i] = regime_logits(rng, list(labels[i, :n]), frames, k, "learnt")
    lg = torch.tensor(logits, device=dev)
    probs, logq = torch.zeros_like(lg), torch.zeros_like(lg)
    lab = torch.tensor(labels, device=dev)
    ll = torch.tensor(lens, dtype=torch.int32, device=dev)
    il = torch.full((batch,), frames, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), batch, frames, k, k, frames * k, 1e-8, st)
    names = ["sl_ctc_align_long"] + (["sl_ctc_align"] if both else [])
    calls = {}
    for name in names:
        path = torch.zeros((batch, frames), dtype=torch.int32, device=dev)
        score = torch.zeros((batch,), dtype=torch.float32, device=dev)
        need = lib.raw(name + "_workspace_bytes")(batch, frames, l_hi)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        calls[name] = ((logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(), batch,
                        frames, k, l_hi, ws.data_ptr(), need, st), path, score, ws, need)
    times = {name: [] for name in names}
    for i in range(warmup + iters):
        for name in names:  # taking turns: both see the same clocks and the same state of the caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            lib.call(name, *calls[name][0])
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    out = {"batch": batch, "frames": frames, "labels": [l_lo, l_hi], "k": k, "iters": iters}
    for name in names:
        _, path, score, _, need = calls[name]
        out[name] = {"ms_median": float(np.median(times[name])), "ms_min": float(np.min(times[name])),
                     "workspace_bytes": int(need), "feasible": int(np.isfinite(score.cpu().numpy()).sum())}
    out["us_per_frame"] = 1e3 * out["sl_ctc_align_long"]["ms_median"] / frames
    if both:
        same = torch.equal(calls[names[0]][1], calls[names[1]][1]) and torch.equal(calls[names[0]][2], calls[names[1]][2])
        out["same_bytes"] = bool(same)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    args = ap.parse_args()
    from speechless_amd._lib import lib
    results = []
    for shape in SHAPES:
        results.append(time_shape(lib(), *shape, args.k, args.warmup, args.iters, args.seed))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
