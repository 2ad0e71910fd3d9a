#!/usr/bin/env python
"""sl_asg_align_long alone: ms per call, HIP events around each of --iters calls after --warmup, with sl_ctc_align_long taking
turns with it, call by call, on the same frames in the same run.  ONE recording at two sizes:
  1 x 30 000 frames with a label of 8000 graphemes (a ten-minute recording: 16 waves in both kernels), and
  1 x 6000 frames with a label of 1500 graphemes (two minutes: 4 waves in both kernels).
logq: 30 classes of a learnt-alignment regime (tools/fuzz_ctc.py), the label's values in [0, 29) so that it is a label of both
criteria (for CTC class 29 is the blank); the ASG scores are U(-1, 1).  One JSON line per size; --out writes them as a list
(profiles/asg_long_align_time.json).

    python tools/asg_long_align_time.py --out profiles/asg_long_align_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

SIZES = [(30000, 8000), (6000, 1500)]  # frames, graphemes of the one recording
K = 30


def time_size(lib, frames, graphemes, warmup, iters, seed):
    import torch
    from fuzz_ctc import regime_logits
    rng = np.random.RandomState(seed)
    dev = "cuda:0"
    labels = rng.randint(0, K - 1, size=(1, graphemes)).astype(np.int32)
    logits = regime_logits(rng, list(labels[0]), frames, K, "learnt")[None].astype(np.float32)
    lg = torch.tensor(logits, device=dev)
    probs, logq = torch.zeros_like(lg), torch.zeros_like(lg)
    lab = torch.tensor(labels, device=dev)
    ll = torch.tensor([graphemes], dtype=torch.int32, device=dev)
    il = torch.tensor([frames], dtype=torch.int32, device=dev)
    trans = torch.tensor(rng.uniform(-1, 1, size=(K, K)).astype(np.float32), device=dev)
    init = torch.tensor(rng.uniform(-1, 1, size=K).astype(np.float32), device=dev)
    st = torch.cuda.current_stream().cuda_stream
    lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), 1, frames, K, K, frames * K, 1e-8, st)
    names = ["sl_asg_align_long", "sl_ctc_align_long"]
    calls = {}
    for name in names:
        path = torch.zeros((1, frames), dtype=torch.int32, device=dev)
        score = torch.zeros((1,), dtype=torch.float32, device=dev)
        need = lib.raw(name + "_workspace_bytes")(1, frames, graphemes)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        scores = (trans.data_ptr(), init.data_ptr()) if name == "sl_asg_align_long" else ()
        calls[name] = ((logq.data_ptr(),) + scores + (lab.data_ptr(), ll.data_ptr(), il.data_ptr(), path.data_ptr(),
                                                      score.data_ptr(), 1, frames, K, graphemes, ws.data_ptr(), need, st),
                       path, score, ws, need)
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
    out = {"batch": 1, "frames": frames, "graphemes": graphemes, "k": K, "iters": iters}
    for name in names:
        _, path, score, _, need = calls[name]
        out[name] = {"ms_median": float(np.median(times[name])), "ms_min": float(np.min(times[name])),
                     "ms_max": float(np.max(times[name])), "us_per_frame": 1e3 * float(np.median(times[name])) / frames,
                     "workspace_bytes": int(need), "feasible": int(np.isfinite(score.cpu().numpy()).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    args = ap.parse_args()
    from speechless_amd._lib import lib
    results = []
    for frames, graphemes in SIZES:
        results.append(time_size(lib(), frames, graphemes, args.warmup, args.iters, args.seed))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
