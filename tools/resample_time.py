#!/usr/bin/env python
"""sl_resample_polyphase alone: ms per launch for 32 utterances of 10 s, HIP events around each of --iters launches after
--warmup, for 44.1 -> 16, 48 -> 16 and 8 -> 16 kHz.  Taking turns with it, launch by launch in the same run: the rest of the front
end on the converted batch (sl_stft_power_db + mel projection + z-normalisation: SpectrogramExtractor.batch_device) and the H2D
copy of the same source-rate samples out of pageable memory (what the staged pipeline does).  One JSON line per rate pair;
--out writes them as a list (profiles/resample_time.json).

    python tools/resample_time.py --out profiles/resample_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000)]


def time_pair(sr_orig, sr_new, batch, seconds, warmup, iters, seed):
    import torch
    from speechless_amd.resample import Resampler
    from speechless_amd.spectrogram import SpectrogramExtractor
    dev = "cuda:0"
    rng = np.random.RandomState(seed)
    n_in = int(seconds * sr_orig)
    host = torch.from_numpy(rng.uniform(-0.5, 0.5, size=batch * n_in).astype(np.float32))
    lengths = np.full(batch, n_in, dtype=np.int32)
    offsets = np.arange(batch, dtype=np.int64) * n_in
    flat = torch.empty_like(host, device=dev)
    off_dev, len_dev = torch.from_numpy(offsets).to(dev), torch.from_numpy(lengths).to(dev)
    rs = Resampler(sr_orig, sr_new, dev)
    extractor = SpectrogramExtractor(sample_rate=sr_new, device=dev)
    fe_bufs = {}

    def copy():
        flat.copy_(host, non_blocking=True)

    copy()
    out_flat, out_off, out_len, out_lengths = rs.batch_device(flat, off_dev, len_dev, lengths)

    def convert():  # the launch alone (batch_device also copies the output offsets and lengths to the device)
        rs.launch(flat, off_dev, len_dev, out_flat, out_off, batch)

    frames_dev = torch.tensor([extractor.frame_count(int(n)) for n in out_lengths], dtype=torch.int32, device=dev)

    def front_end():
        extractor.batch_device(out_flat, out_off, out_len, out_lengths, frames_dev, bufs=fe_bufs)

    steps = {"h2d_copy": copy, "resample": convert, "front_end_rest": front_end}
    times = {name: [] for name in steps}
    for i in range(warmup + iters):
        for name, fn in steps.items():  # taking turns: all three see the same clocks and the same state of the caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    n_out = int(out_lengths[0])
    macs = batch * n_out * rs.width
    result = {"sr_orig": sr_orig, "sr_new": sr_new, "batch": batch, "seconds": seconds, "bank": [rs.q, rs.width], "iters": iters,
              "samples_in": batch * n_in, "samples_out": batch * n_out, "multiply_adds": macs}
    for name in steps:
        result[name] = {"ms_median": float(np.median(times[name])), "ms_min": float(np.min(times[name])),
                        "ms_max": float(np.max(times[name]))}
    result["resample"]["gmac_per_s"] = macs / (result["resample"]["ms_median"] * 1e-3) / 1e9
    result["resample_over_front_end_rest"] = result["resample"]["ms_median"] / result["front_end_rest"]["ms_median"]
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    args = ap.parse_args()
    results = []
    for sr_orig, sr_new in PAIRS:
        results.append(time_pair(sr_orig, sr_new, args.batch, args.seconds, args.warmup, args.iters, args.seed))
        print(json.dumps(results[-1]), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
