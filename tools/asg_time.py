#!/usr/bin/env python
"""Times sl_asg_loss_grad and sl_asg_viterbi alone at configuration 3's shape (B = 32, T' = 500, K = 30, label lengths from
U{20..200}), with sl_ctc_loss_grad (K = 29, the same labels, lengths and logits) beside them in the same run, and writes
profiles/asg_time.json.
    python tools/asg_time.py [--batch 32] [--frames 500] [--lmax 200] [--reps 50] [--out profiles/asg_time.json]"""
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
    ap.add_argument("--lmax", type=int, default=200)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "asg_time.json"))
    args = ap.parse_args()
    import torch
    from speechless_amd import _lib
    lib = _lib.lib()
    b, t, k = args.batch, args.frames, 30
    rng = np.random.RandomState(0)
    dev = "cuda:0"
    st = torch.cuda.current_stream().cuda_stream
    lg = rng.randn(b, t, k).astype(np.float32)
    lab_len = rng.randint(20, args.lmax + 1, size=b).astype(np.int32)
    labels = np.zeros((b, args.lmax), dtype=np.int32)
    for i, n in enumerate(lab_len):
        labels[i, :n] = rng.randint(0, k - 2, size=n)  # (below 28: valid CTC labels of the 29-class comparison too)
    lab, ll = torch.tensor(labels, device=dev), torch.tensor(lab_len, device=dev)
    il = torch.full((b,), t, dtype=torch.int32, device=dev)
    loss = torch.zeros((b,), dtype=torch.float32, device=dev)
    dl = torch.zeros((b, t, 128), dtype=torch.bfloat16, device=dev)

    def softmax(kk):
        logits = torch.tensor(np.ascontiguousarray(lg[:, :, :kk]), device=dev)
        probs = torch.zeros((b, t, kk), dtype=torch.float32, device=dev)
        logq = torch.zeros_like(probs)
        lib.call("sl_softmax_logq", logits.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, kk, kk, t * kk, 1e-8, st)
        return probs, logq

    def timed(run):
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.reps):
            run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps * 1e3

    probs, logq = softmax(k)
    trans = torch.tensor(rng.uniform(-2, 2, size=(k, k)).astype(np.float32), device=dev)
    init = torch.tensor(rng.uniform(-2, 2, size=k).astype(np.float32), device=dev)
    dtrans, dinit = torch.zeros_like(trans), torch.zeros_like(init)
    need = lib.raw("sl_asg_workspace_bytes")(b, t, k, args.lmax)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    asg_us = timed(lambda: lib.call(
        "sl_asg_loss_grad", probs.data_ptr(), logq.data_ptr(), trans.data_ptr(), init.data_ptr(), lab.data_ptr(), ll.data_ptr(),
        il.data_ptr(), loss.data_ptr(), dl.data_ptr(), dtrans.data_ptr(), dinit.data_ptr(), b, t, k, args.lmax, 0, 128, t * 128,
        _lib.SL_BF16, 1e-8, 1.0 / b, ws.data_ptr(), need, st))
    asg_loss = float(loss.mean())
    path = torch.zeros((b, t), dtype=torch.int32, device=dev)
    score = torch.zeros((b,), dtype=torch.float32, device=dev)
    vneed = lib.raw("sl_asg_viterbi_workspace_bytes")(b, t, k)
    vws = torch.empty((max(vneed, 16),), dtype=torch.uint8, device=dev)
    vit_us = timed(lambda: lib.call("sl_asg_viterbi", logq.data_ptr(), trans.data_ptr(), init.data_ptr(), il.data_ptr(),
                                    path.data_ptr(), score.data_ptr(), b, t, k, vws.data_ptr(), vneed, st))
    cprobs, clogq = softmax(k - 1)
    cneed = lib.raw("sl_ctc_workspace_bytes")(b, t, args.lmax)
    cws = torch.empty((cneed,), dtype=torch.uint8, device=dev)
    ctc_us = timed(lambda: lib.call(
        "sl_ctc_loss_grad", cprobs.data_ptr(), clogq.data_ptr(), lab.data_ptr(), ll.data_ptr(), il.data_ptr(), loss.data_ptr(),
        dl.data_ptr(), b, t, k - 1, args.lmax, 0, 128, t * 128, _lib.SL_BF16, 1e-8, 1.0 / b, cws.data_ptr(), cneed, st))
    result = {
        "shape": {"batch": b, "frames": t, "k_asg": k, "k_ctc": k - 1, "l_max": args.lmax, "label_lengths": "U{20..%d}" % args.lmax,
                  "logits": "N(0, 1)", "gradient_dtype": "bf16"},
        "reps": args.reps,
        "sl_asg_loss_grad_us_per_call": round(asg_us, 1),
        "sl_asg_viterbi_us_per_call": round(vit_us, 1),
        "sl_ctc_loss_grad_us_per_call": round(ctc_us, 1),
        "asg_workspace_bytes": int(need),
        "ctc_workspace_bytes": int(cneed),
        "asg_mean_loss": asg_loss,
        "ctc_mean_loss": float(loss.mean()),
        "device": torch.cuda.get_device_name(0),
    }
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
    print(json.dumps(result, sort_keys=True))


if __name__ == "__main__":
    main()
