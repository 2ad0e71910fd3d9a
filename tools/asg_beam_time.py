#!/usr/bin/env python
"""One batch through the ASG beam search on the GPU (GpuAsgBeamSearchDecoder, asg_beam.hip) and, in the same run and on the
same shape, through the CTC beam search (GpuCtcBeamSearchDecoder, ctc_beam.hip, 29 classes) and the ASG Viterbi decode
(sl_asg_viterbi): wall time per batch of each, the copy of the results to the host included.  Beam 100, k = 30 (28
characters + the two repeat marks), no language model and a synthetic 3-gram model of 20 000 words
(speechless_amd/synthetic_lm.py).  Acoustics: a random grapheme path, the path's class 5 above unit-normal logits
(peaky, as a trained net's output); the CTC batch is tools/beam_time.py's.  Transition scores U(-1, 1), start scores 0.

    python tools/asg_beam_time.py             # 32 x 500 and 8 x 4000 frames -> profiles/asg_beam_time.json"""
import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

ALPHABET = list("abcdefghijklmnopqrstuvwxyz' ")
SHAPES = [(32, 500), (8, 4000)]
BEAM = 100


def asg_emissions(rng, batch, frames, k, sharpness=5.0):
    """log-softmax of peaky logits: runs of one to three frames per grapheme, no two adjacent runs of the same grapheme"""
    logits = rng.randn(batch, frames, k).astype(np.float32)
    for b in range(batch):
        t, last = 0, -1
        while t < frames:
            c = rng.randint(k)
            if c == last:
                continue
            last = c
            for _ in range(rng.randint(1, 4)):
                if t < frames:
                    logits[b, t, c] += sharpness
                    t += 1
    z = logits - logits.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


def median_ms(call, iters):
    import torch
    call()  # warm-up (and the workspace)
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()  # includes the copy of the results to the host
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times)), 3), round(float(np.min(times)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--words", type=int, default=20000)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "asg_beam_time.json"))
    args = ap.parse_args()
    import torch
    from beam_time import acoustics
    from speechless_amd import _lib
    from speechless_amd.decoder import GpuAsgBeamSearchDecoder, GpuCtcBeamSearchDecoder, NGramLanguageModel
    from speechless_amd.synthetic_lm import write_synthetic_arpa
    tmp = Path(tempfile.mkdtemp())
    write_synthetic_arpa(tmp / "lm.arpa", ALPHABET, args.words, order=3, seed=1)
    lm = NGramLanguageModel(tmp / "lm.arpa")
    lib = _lib.lib()
    rng = np.random.RandomState(0)
    k = len(ALPHABET) + 2
    rows = []
    for batch, frames in SHAPES:
        logq = torch.from_numpy(asg_emissions(rng, batch, frames, k)).cuda()
        trans = torch.from_numpy(rng.uniform(-1, 1, size=(k, k)).astype(np.float32)).cuda()
        init = torch.zeros((k,), dtype=torch.float32).cuda()
        probs = torch.from_numpy(acoustics(rng, batch, frames, k - 1)).cuda()
        dlen = torch.tensor([frames] * batch, dtype=torch.int32).cuda()

        path = torch.empty((batch, frames), dtype=torch.int32).cuda()
        score = torch.empty((batch,), dtype=torch.float32).cuda()
        need = lib.raw("sl_asg_viterbi_workspace_bytes")(batch, frames, k)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8).cuda()

        def viterbi():
            lib.call("sl_asg_viterbi", logq.data_ptr(), trans.data_ptr(), init.data_ptr(), dlen.data_ptr(), path.data_ptr(),
                     score.data_ptr(), batch, frames, k, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
            return path.cpu().numpy(), score.cpu().numpy()

        viterbi_ms = median_ms(viterbi, args.iters)
        for name, model in (("none", None), ("3-gram {} words".format(args.words), lm)):
            row = {"batch": batch, "frames": frames, "k": k, "beam": BEAM, "lm": name}
            asg = GpuAsgBeamSearchDecoder(ALPHABET, model, beam_width=BEAM)
            ctc = GpuCtcBeamSearchDecoder(ALPHABET, model, beam_width=BEAM)
            row["asg_beam_ms_median"], row["asg_beam_ms_min"] = median_ms(lambda: asg.decode(logq, trans, init, dlen), args.iters)
            row["ctc_beam_ms_median"], row["ctc_beam_ms_min"] = median_ms(lambda: ctc.decode(probs, dlen), args.iters)
            row["asg_viterbi_ms_median"], row["asg_viterbi_ms_min"] = viterbi_ms
            row["ctc_over_asg"] = round(row["ctc_beam_ms_median"] / row["asg_beam_ms_median"], 2)
            row["mean_len"] = float(np.mean([len(w) for w in asg.decode(logq, trans, init, dlen)[0]]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps({"device": torch.cuda.get_device_name(0), "iters": args.iters, "rows": rows},
                                         indent=1) + "\n")


if __name__ == "__main__":
    main()
