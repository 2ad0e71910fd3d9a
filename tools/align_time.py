#!/usr/bin/env python
"""sl_ctc_align alone: ms per call at a batch / frame count / label-length range, HIP events around each of --iters calls
after --warmup, on logq of a learnt-alignment regime (tools/fuzz_ctc.py).  One JSON line per shape.

    python tools/align_time.py                       # config 3's shape (32 x 500, labels 100..200) and the config-5 shard
    python tools/align_time.py --shape 8,4000,300,511 --k 29"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

SHAPES = [(32, 500, 100, 200), (8, 4000, 300, 511)]  # batch, frames, shortest label, longest label


def time_shape(lib, batch, frames, l_lo, l_hi, k, warmup, iters, seed):
    import torch
    from fuzz_ctc import regime_logits
    rng = np.random.RandomState(seed)
    dev = "cuda:0"
    lens = [int(rng.randint(l_lo, l_hi + 1)) for _ in range(batch)]
    lens[0] = l_hi  # the launch's l_max (states per lane) is that of the longest label
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
    path = torch.zeros((batch, frames), dtype=torch.int32, device=dev)
    score = torch.zeros((batch,), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), batch, frames, k, k, frames * k, 1e-8, st)
    need = lib.raw("sl_ctc_align_workspace_bytes")(batch, frames, l_hi)
    ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    args = (logq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(), batch, frames,
            k, l_hi, ws.data_ptr(), need, st)
    for _ in range(warmup):
        lib.call("sl_ctc_align", *args)
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        lib.call("sl_ctc_align", *args)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    feasible = int(np.isfinite(score.cpu().numpy()).sum())
    return {"batch": batch, "frames": frames, "labels": [l_lo, l_hi], "k": k, "workspace_bytes": int(need),
            "backpointers": "LDS" if need == 0 else "HBM", "ms_median": float(np.median(times)),
            "ms_min": float(np.min(times)), "iters": iters, "feasible": feasible}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="batch,frames,shortest label,longest label (repeatable)")
    ap.add_argument("--k", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    from speechless_amd._lib import lib
    shapes = [tuple(int(v) for v in s.split(",")) for s in args.shape] if args.shape else SHAPES
    for shape in shapes:
        print(json.dumps(time_shape(lib(), *shape, args.k, args.warmup, args.iters, args.seed)), flush=True)


if __name__ == "__main__":
    main()
