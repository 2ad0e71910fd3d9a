#!/usr/bin/env python
"""sl_stft in each mode and sl_istft alone: ms per launch for 32 utterances of 10 s at 16 kHz (n_fft 512, hop 128), HIP events
around each of --iters launches after --warmup, taking turns launch by launch with sl_stft_power_db in the same run (the
comparison for the forward modes).  Beside each time: the bytes the launch must move (samples in and rows out, or the other
way round; each counted once, padding columns included where the launch writes them) and the GB/s that makes.  One JSON
line; --out also writes it to a file (profiles/istft_time.json).

    python tools/istft_time.py --out profiles/istft_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def measure(batch, seconds, n_fft, hop, warmup, iters, seed):
    import torch
    from speechless_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(seed)
    n = int(seconds * 16000)
    bins = n_fft // 2 + 1
    frames = 1 + n // hop
    stride = (bins + 63) // 64 * 64  # the padded rows SpectrogramExtractor hands the mel projection
    audio = torch.from_numpy(rng.uniform(-0.5, 0.5, size=batch * n).astype(np.float32)).to(dev)
    offsets = torch.arange(batch, dtype=torch.int64, device=dev) * n
    lengths = torch.full((batch,), n, dtype=torch.int32, device=dev)
    frames_dev = torch.full((batch,), frames, dtype=torch.int32, device=dev)
    real = torch.empty((batch, frames, stride), dtype=torch.float32, device=dev)
    spec = torch.empty((batch, frames, 2 * bins), dtype=torch.float32, device=dev)
    n_out = hop * (frames - 1)
    back = torch.empty((batch * n_out,), dtype=torch.float32, device=dev)
    back_off = torch.arange(batch, dtype=torch.int64, device=dev) * n_out
    st = torch.cuda.current_stream(dev).cuda_stream
    head = (audio.data_ptr(), offsets.data_ptr(), lengths.data_ptr())

    def forward(mode):
        out, row = (spec, 2 * bins) if mode == _lib.STFT_COMPLEX else (real, stride)
        return lambda: lib.call("sl_stft", *head, out.data_ptr(), batch, frames, n_fft, hop, row, frames * row, mode, -150.0, st)

    steps = {
        "sl_stft_power_db": lambda: lib.call("sl_stft_power_db", *head, real.data_ptr(), batch, frames, n_fft, hop, stride,
                                             frames * stride, -150.0, st),
        "sl_stft_power": forward(_lib.STFT_POWER),
        "sl_stft_amplitude": forward(_lib.STFT_AMPLITUDE),
        "sl_stft_power_level": forward(_lib.STFT_POWER_LEVEL),
        "sl_stft_complex": forward(_lib.STFT_COMPLEX),
        # (runs behind sl_stft_complex: the spectrum it inverts is the one that launch has just written)
        "sl_istft": lambda: lib.call("sl_istft", spec.data_ptr(), frames_dev.data_ptr(), back.data_ptr(), back_off.data_ptr(),
                                     batch, frames, n_fft, hop, 2 * bins, frames * 2 * bins, st),
    }
    real_bytes = 4 * batch * (n + frames * stride)
    complex_bytes = 4 * batch * (n + frames * 2 * bins)
    moved = {name: real_bytes for name in steps}
    moved["sl_stft_complex"] = complex_bytes
    moved["sl_istft"] = 4 * batch * (frames * 2 * bins + n_out)
    times = {name: [] for name in steps}
    for i in range(warmup + iters):
        for name, fn in steps.items():  # taking turns: every launch sees the same clocks and the same state of the caches
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                times[name].append(a.elapsed_time(b))
    err = float((back.view(batch, n_out) - audio.view(batch, n)[:, :n_out]).abs().max())
    result = {"batch": batch, "seconds": seconds, "n_fft": n_fft, "hop": hop, "frames": frames, "row_stride": stride, "iters": iters,
              "istft_tile_frames": lib.raw("sl_istft_tile_frames")(n_fft, hop), "round_trip_max_abs_error": err}
    for name in steps:
        ms = float(np.median(times[name]))
        result[name] = {"ms_median": ms, "ms_min": float(np.min(times[name])), "ms_max": float(np.max(times[name])),
                        "bytes": moved[name], "gb_per_s": moved[name] / (ms * 1e-3) / 1e9}
    base = result["sl_stft_power_db"]["ms_median"]
    for name in steps:
        result[name]["over_sl_stft_power_db"] = result[name]["ms_median"] / base
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--n-fft", type=int, default=512)
    ap.add_argument("--hop", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the result to this file")
    args = ap.parse_args()
    result = measure(args.batch, args.seconds, args.n_fft, args.hop, args.warmup, args.iters, args.seed)
    print(json.dumps(result), flush=True)
    if args.out:
        Path(args.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
