#!/usr/bin/env python
"""Where test_and_predict_batch spends its time with the error counts on the host and on the GPU
(Wav2Letter(error_count_device=...), csrc/edit_distance.hip).  Batch: BASELINE config 2 -- 32 utterances x 1000 frames x
128 mel bins (bench.py's input, seed 1000), labels of U{20..200} indices in 0..27 (bench.py's label seed, 2000).  Two
regimes: `random_init` -- the net's own greedy predictions, long and noisy -- and `equal` -- the probabilities overwritten
after the forward pass so that the greedy decode returns exactly the labels (the short, cheap end; the loss of that regime
is meaningless).  Per regime: wall time of test_and_predict_batch for "host" and "gpu" (median, min, max of --iters calls
after --warmup), the kernel's own duration from its dispatch timestamps (sl_profile_next_kernel), the forward pass of the
same batch (HIP events around the launches, input resident) and the kernel as a fraction of it.  One JSON line per regime.

    python tools/eval_time.py [--out profiles/eval_time.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, FRAMES, MEL = 32, 1000, 128


def make_batch(characters):
    from speechless_amd.net import LabeledSpectrogram
    x = np.random.RandomState(1000).randn(BATCH, FRAMES, MEL).astype(np.float32)
    rng = np.random.RandomState(2000)
    lengths = rng.randint(20, 201, size=BATCH)
    labels = ["".join(characters[i] for i in rng.randint(0, 28, size=n)) for n in lengths]
    return [LabeledSpectrogram("u{}".format(i), label, x[i]) for i, label in enumerate(labels)]


def forced_probabilities(net, batch, t_out):
    """(B, T', K) one-hot rows whose greedy decode is the label: label i on frame 2 i + 1, blank everywhere else"""
    k = net.grapheme_encoding.grapheme_set_size
    probs = np.zeros((len(batch), t_out, k), dtype=np.float32)
    probs[:, :, k - 1] = 1.0
    for row, example in zip(probs, batch):
        for i, index in enumerate(net.grapheme_encoding.encode_label_batch([example.label])[0]):
            row[2 * i + 1, k - 1], row[2 * i + 1, index] = 0.0, 1.0
    return probs


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min": round(float(np.min(values)), 4),
            "max": round(float(np.max(values)), 4), "n": len(values)}


def measure(regime, args):
    import torch
    from speechless_amd import Wav2Letter, english_frequent_characters
    batch = make_batch(english_frequent_characters)
    row = {"regime": regime, "batch": BATCH, "frames": FRAMES, "label_lengths": [min(len(x.label) for x in batch),
                                                                                   max(len(x.label) for x in batch)]}
    results = {}
    for device in ("host", "gpu"):
        net = Wav2Letter(MEL, english_frequent_characters, seed=2, error_count_device=device)
        engine = net.eval_engine
        if regime == "equal":
            plain_forward = engine.forward
            forced = torch.from_numpy(forced_probabilities(net, batch, FRAMES // 2)).to(engine.device)

            def forward(x, plain_forward=plain_forward, engine=engine, forced=forced):
                plain_forward(x)
                engine.cur.probs.copy_(forced)
                return engine.cur.probs
            engine.forward = forward
        for _ in range(args.warmup):
            results[device] = net.test_and_predict_batch(batch)
        times = []
        for _ in range(args.iters if device == "gpu" else args.host_iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[device] = net.test_and_predict_batch(batch)
            times.append((time.perf_counter() - t0) * 1e3)
        row["test_and_predict_batch_ms_" + device] = spread(times)
        if device == "host":
            from speechless_amd.net import ExpectationVsPrediction
            counting = []
            for _ in range(args.host_iters):  # the part "gpu" replaces, alone: the result objects built again
                t0 = time.perf_counter()
                for r in results[device].results:
                    ExpectationVsPrediction(r.expected, r.predicted, r.loss)
                counting.append((time.perf_counter() - t0) * 1e3)
            row["host_error_counting_ms"] = spread(counting)
            continue
        engine.kernel_timeline = ({"edit_distance"}, [])
        for _ in range(args.iters):
            net.test_and_predict_batch(batch)
        torch.cuda.synchronize()
        row["edit_distance_kernel_ms"] = spread([a.elapsed_time(b) for _, a, b in engine.kernel_timeline[1]])
        engine.kernel_timeline = None
        forward_ms = []
        if regime == "equal":
            engine.forward = plain_forward
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            engine.forward()  # the batch is resident: launches only
            b.record()
            b.synchronize()
            forward_ms.append(a.elapsed_time(b))
        row["forward_ms"] = spread(forward_ms)
        row["kernel_fraction_of_forward"] = round(row["edit_distance_kernel_ms"]["median"] / row["forward_ms"]["median"], 4)
    host, gpu = results["host"].results, results["gpu"].results
    row["counts_equal"] = [(r.letter_error_count, r.word_error_count) for r in host] == \
        [(r.letter_error_count, r.word_error_count) for r in gpu]
    row["mean_predicted_length"] = float(np.mean([len(r.predicted) for r in gpu]))
    row["speedup"] = round(row["test_and_predict_batch_ms_host"]["median"] / row["test_and_predict_batch_ms_gpu"]["median"], 2)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5, help="timed calls with the counts on the host (about 1 s each)")
    ap.add_argument("--out", help="also write the rows to this JSON file")
    args = ap.parse_args()
    rows = []
    for regime in ("random_init", "equal"):
        rows.append(measure(regime, args))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
