#!/usr/bin/env python
"""Times sl_asg_align alone at configuration 3's shape (B = 32, T' = 500 output frames, the English alphabet: K = 30 under ASG,
random labels of about 80 graphemes), with sl_ctc_align (K = 29, the same labels, lengths and logits) and sl_asg_viterbi (the
full-graph decode over the same emissions and scores) beside it in the same run, and writes profiles/asg_align_time.json.

Every kernel is warmed up, then timed --reps times with HIP events around --calls back-to-back launches, the three kernels
taking turns inside a repetition; the file holds the median per call and the spread (min, 10th / 90th percentile).
    python tools/asg_align_time.py [--batch 32] [--frames 500] [--label 80] [--reps 200] [--calls 20] [--out FILE]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--label", type=int, default=80, help="mean label length; lengths are drawn from U{label - 20 .. label + 20}")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=20, help="launches inside one timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "asg_align_time.json"))
    args = ap.parse_args()
    import torch
    from speechless_amd import _lib
    lib = _lib.lib()
    b, t, k = args.batch, args.frames, 30
    rng = np.random.RandomState(0)
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    lg = rng.randn(b, t, k).astype(np.float32)
    lo, hi = max(1, args.label - 20), args.label + 20
    lab_len = rng.randint(lo, hi + 1, size=b).astype(np.int32)
    lab_len[0] = hi  # the launch's l_max (states per lane) is that of the longest label
    labels = np.zeros((b, hi), dtype=np.int32)
    for i, n in enumerate(lab_len):
        labels[i, :n] = rng.randint(0, k - 2, size=n)  # (below 28: valid CTC labels of the 29-class comparison too)
    lab, ll = torch.tensor(labels, device=dev), torch.tensor(lab_len, device=dev)
    il = torch.full((b,), t, dtype=torch.int32, device=dev)
    path = torch.zeros((b, t), dtype=torch.int32, device=dev)
    score = torch.zeros((b,), dtype=torch.float32, device=dev)

    def softmax(kk):
        logits = torch.tensor(np.ascontiguousarray(lg[:, :, :kk]), device=dev)
        probs = torch.zeros((b, t, kk), dtype=torch.float32, device=dev)
        logq = torch.zeros_like(probs)
        lib.call("sl_softmax_logq", logits.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, kk, kk, t * kk, 1e-8, st)
        return logq

    def workspace(name, *shape):
        need = lib.raw(name)(*shape)
        return torch.empty((max(need, 16),), dtype=torch.uint8, device=dev), need

    logq, clogq = softmax(k), softmax(k - 1)
    trans = torch.tensor(rng.uniform(-2, 2, size=(k, k)).astype(np.float32), device=dev)
    init = torch.tensor(rng.uniform(-2, 2, size=k).astype(np.float32), device=dev)
    aws, aneed = workspace("sl_asg_align_workspace_bytes", b, t, hi)
    cws, cneed = workspace("sl_ctc_align_workspace_bytes", b, t, hi)
    vws, vneed = workspace("sl_asg_viterbi_workspace_bytes", b, t, k)
    runs = {
        "sl_asg_align": lambda: lib.call("sl_asg_align", logq.data_ptr(), trans.data_ptr(), init.data_ptr(), lab.data_ptr(),
                                         ll.data_ptr(), il.data_ptr(), path.data_ptr(), score.data_ptr(), b, t, k, hi,
                                         aws.data_ptr(), aneed, st),
        "sl_ctc_align": lambda: lib.call("sl_ctc_align", clogq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(),
                                         path.data_ptr(), score.data_ptr(), b, t, k - 1, hi, cws.data_ptr(), cneed, st),
        "sl_asg_viterbi": lambda: lib.call("sl_asg_viterbi", logq.data_ptr(), trans.data_ptr(), init.data_ptr(), il.data_ptr(),
                                           path.data_ptr(), score.data_ptr(), b, t, k, vws.data_ptr(), vneed, st),
    }
    feasible = {}
    for name, run in runs.items():
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        feasible[name] = int(np.isfinite(score.cpu().numpy()).sum())
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # the kernels take turns: whatever else the machine does meets all three alike
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                run()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.calls * 1e3)
    result = {
        "shape": {"batch": b, "frames": t, "k_asg": k, "k_ctc": k - 1, "l_max": int(hi), "label_lengths": "U{%d..%d}" % (lo, hi),
                  "logits": "N(0, 1)", "scores": "U(-2, 2)"},
        "warmup": args.warmup, "reps": args.reps, "calls_per_window": args.calls,
        "what": "microseconds per call: HIP events around `calls_per_window` back-to-back launches on one stream",
        "workspace_bytes": {"sl_asg_align": int(aneed), "sl_ctc_align": int(cneed), "sl_asg_viterbi": int(vneed)},
        "feasible_rows": feasible,
        "device": torch.cuda.get_device_name(0),
    }
    for name, us in times.items():
        result[name + "_us"] = {"median": round(float(np.median(us)), 1), "min": round(float(np.min(us)), 1),
                                "p10": round(float(np.percentile(us, 10)), 1), "p90": round(float(np.percentile(us, 90)), 1)}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
