#!/usr/bin/env python
"""One batch through the GPU beam search (GpuCtcBeamSearchDecoder, ctc_beam.hip) and through the host decoder
(CtcBeamSearchDecoder, 16 threads): wall time per batch of each, and whether their transcripts agree.  Beam 100, k = 29,
no language model and a synthetic 3-gram model of 20 000 words (speechless_amd/synthetic_lm.py).  Acoustics: a random
character path with blanks, the path's class 5 above unit-normal logits (peaky, as a trained net's output).

    python tools/beam_time.py                 # 32 x 500 and 8 x 4000 frames
    python tools/beam_time.py --host-only     # the host decoder alone (no GPU needed)"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ALPHABET = list("abcdefghijklmnopqrstuvwxyz' ")
SHAPES = [(32, 500), (8, 4000)]


def acoustics(rng, batch, frames, k, sharpness=5.0):
    logits = rng.randn(batch, frames, k).astype(np.float32)
    for b in range(batch):
        t = 0
        while t < frames:
            c = rng.randint(k - 1)
            for _ in range(rng.randint(1, 4)):
                if t < frames:
                    logits[b, t, c] += sharpness
                    t += 1
            for _ in range(rng.randint(0, 3)):
                if t < frames:
                    logits[b, t, k - 1] += sharpness
                    t += 1
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--words", type=int, default=20000)
    args = ap.parse_args()
    from speechless_amd.decoder import CtcBeamSearchDecoder, GpuCtcBeamSearchDecoder, NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    tmp = Path(tempfile.mkdtemp())
    write_synthetic_arpa(tmp / "lm.arpa", ALPHABET, args.words, order=3, seed=1)
    lm = NGramLanguageModel(tmp / "lm.arpa")
    rng = np.random.RandomState(0)
    for batch, frames in SHAPES:
        probs = acoustics(rng, batch, frames, len(ALPHABET) + 1)
        lengths = [frames] * batch
        for name, model in (("none", None), ("3-gram {} words".format(args.words), lm)):
            row = {"batch": batch, "frames": frames, "k": len(ALPHABET) + 1, "beam": 100, "lm": name}
            host = CtcBeamSearchDecoder(ALPHABET, model, beam_width=100, threads=16)
            t0 = time.perf_counter()
            want, want_lp = host.decode(probs, lengths)
            row["host_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            if not args.host_only:
                import torch
                gpu = GpuCtcBeamSearchDecoder(ALPHABET, model, beam_width=100)
                dprobs = torch.from_numpy(probs).cuda()
                dlen = torch.tensor(lengths, dtype=torch.int32).cuda()
                got, got_lp = gpu.decode(dprobs, dlen)  # warm-up (and the workspace)
                times = []
                for _ in range(args.iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    got, got_lp = gpu.decode(dprobs, dlen)  # includes the copy of the results to the host
                    times.append((time.perf_counter() - t0) * 1e3)
                row["gpu_ms_median"] = round(float(np.median(times)), 3)
                row["gpu_ms_min"] = round(float(np.min(times)), 3)
                row["speedup"] = round(row["host_ms"] / row["gpu_ms_median"], 1)
                row["transcripts_equal"] = got == want
                row["max_rel_dlogp"] = float(np.max(np.abs(got_lp - want_lp) / np.maximum(1.0, np.abs(want_lp))))
            row["mean_len"] = float(np.mean([len(w) for w in want]))
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
