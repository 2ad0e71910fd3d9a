#!/usr/bin/env python
"""Raw-wave input on the plane paths: what the fused window gather (sl_wave_frames_planes) costs beside the two launches it
replaces (sl_wave_frames into fp32 windows + sl_splitf16 / sl_split3), and what the 12-layer raw-wave net costs on f16x3 beside
bf16x3 -- forward pass and whole training step, input and labels resident.  Batch: 32 utterances x 128 000 samples (8 s at
16 kHz), one sample channel; labels of U{20..100} indices.  HIP events around the launches, the two sides of a comparison
alternating call by call; medians and [min, max] over --iters calls after --warmup, as tools/eval_time.py reports them.
One JSON line per measurement.

    python tools/wave_planes_time.py [--out profiles/wave_f16x3_time.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BATCH, SAMPLES, CIN, K, STRIDE, CHANNELS = 32, 128000, 1, 250, 160, 256


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min": round(float(np.min(values)), 4),
            "max": round(float(np.max(values)), 4), "n": len(values)}


def timed(fns, args):
    """HIP events around each call of every function of `fns` ({name: function}), the functions ALTERNATING call by call (what
    shares the box moves both alike): {name: spread of --iters calls after --warmup}"""
    import torch
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(args.iters):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return {name: spread(values) for name, values in out.items()}


def gather_rows(args):
    import torch
    from speechless_amd import _lib
    from speechless_amd.plan import same_padding
    lib = _lib.lib()
    t_out, pad_l, _ = same_padding(SAMPLES, K, STRIDE)
    audio = torch.from_numpy((0.1 * np.random.RandomState(1).randn(BATCH, SAMPLES, CIN)).astype(np.float32)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for fmt, code, split, scale in (("f16", _lib.SL_F16, "sl_splitf16", 1024.0), ("bf16", _lib.SL_BF16, "sl_split3", 1.0)):
        fused = torch.zeros((BATCH, t_out, 3 * CHANNELS), dtype=torch.int16, device="cuda")
        two = torch.zeros_like(fused)
        frames32 = torch.zeros((BATCH, t_out, CHANNELS), dtype=torch.float32, device="cuda")
        scaled = audio * scale  # (the two-launch path has no scale argument: the samples are scaled beforehand, not timed)

        def one():
            lib.call("sl_wave_frames_planes", audio.data_ptr(), fused.data_ptr(), BATCH, SAMPLES, CIN, K, STRIDE, pad_l, t_out,
                     CHANNELS, fused.stride(0), scale, code, st)

        def both():
            lib.call("sl_wave_frames", scaled.data_ptr(), frames32.data_ptr(), BATCH, SAMPLES, CIN, K, STRIDE, pad_l, t_out,
                     CHANNELS, frames32.stride(0), _lib.SL_F32, st)
            lib.call(split, frames32.data_ptr(), two.data_ptr(), None, BATCH, t_out, CHANNELS, frames32.stride(0), 0,
                     two.stride(0), 0, st)
        row = {"measurement": "gather", "planes": fmt, "batch": BATCH, "samples": SAMPLES, "frames": t_out}
        row.update(timed({"fused_ms": one, "two_launches_ms": both}, args))
        torch.cuda.synchronize()
        row["planes_equal"] = bool(torch.equal(fused, two))
        row["plane_bytes"] = fused.numel() * 2
        row["fused_over_two_launches"] = round(row["fused_ms"]["median"] / row["two_launches_ms"]["median"], 3)
        rows.append(row)
    return rows


def net_rows(args):
    import torch
    from speechless_amd.engine import Engine, wav2letter_layer_specs
    from speechless_amd.net import Wav2Letter
    specs = wav2letter_layer_specs(CIN, 29, use_raw_wave_input=True)
    weights = Wav2Letter._glorot_uniform(specs, 2)
    x = (0.1 * np.random.RandomState(1000).randn(BATCH, SAMPLES, CIN)).astype(np.float32)
    rng = np.random.RandomState(2000)
    lab_len = rng.randint(20, 101, size=BATCH).astype(np.int32)
    labels = -np.ones((BATCH, int(lab_len.max())), dtype=np.int32)
    for i, n in enumerate(lab_len):
        labels[i, :n] = rng.randint(0, 28, size=n)
    pred_len = np.full((BATCH,), SAMPLES // 320, dtype=np.int32)
    engines = {}
    for dtype in ("f16x3", "bf16x3"):
        eng = engines[dtype] = Engine(specs, 29, dtype=dtype)
        eng.set_weights(weights)
        eng.load_input(x)
        eng.set_labels(labels, lab_len, pred_len)
    rows = {dtype: {"measurement": "net", "dtype": dtype, "batch": BATCH, "samples": SAMPLES, "layers": len(eng.all_specs)}
            for dtype, eng in engines.items()}
    for key, call in (("gather_ms", lambda eng: eng._front_gather(eng.cur, eng.cur.front_src)),
                      ("forward_ms", lambda eng: eng.forward()),
                      ("train_step_ms", lambda eng: eng.train_step_resident())):
        if key == "train_step_ms":
            for dtype, eng in engines.items():
                rows[dtype]["loss_before"] = round(float(eng.ctc().mean().item()), 4)
        got = timed({dtype: (lambda eng=eng: call(eng)) for dtype, eng in engines.items()}, args)
        for dtype in engines:
            rows[dtype][key] = got[dtype]
    torch.cuda.synchronize()
    for dtype, eng in engines.items():
        rows[dtype]["loss_after"] = round(float(eng.cur.loss.mean().item()), 4)
    return list(rows.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", help="also write the rows to this JSON file")
    args = ap.parse_args()
    rows = []
    for row in gather_rows(args) + net_rows(args):
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
