"""Times the fused update + operand repack launch of every optimizer rule (and of Adam) over configuration 3's trainable layer
set -- all eleven layers at the real widths, bf16 operands -- and writes profiles/optimizer_time.json.

One engine per rule, gradients filled with random numbers (the kernels are HBM-bound: the values do not matter); per rule
WARMUP launches, then REPS launches each between two timing events (speechless_amd._hipevents: timestamps only, no
system-scope release); the rules are measured in interleaved rounds so that clock drift hits all of them alike.  Reported per
rule: median, 10th and 90th percentile in microseconds, and the fp32 bytes the rule moves per parameter.

    python tools/optimizer_time.py [--reps 200] [--warmup 20] [--out profiles/optimizer_time.json]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RULES = ["adam", "sgd", "rmsprop", "adagrad", "adadelta", "adamax"]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=200)
    parser.add_argument("--warmup", type=int, default=20)
    parser.add_argument("--rounds", type=int, default=4)
    parser.add_argument("--out", default=str(ROOT / "profiles" / "optimizer_time.json"))
    args = parser.parse_args()
    import torch
    from speechless_amd._hipevents import TimingEvent
    from speechless_amd.engine import Engine, wav2letter_layer_specs
    specs = wav2letter_layer_specs(128, 29)
    engines = {}
    for rule in RULES:
        eng = Engine(specs, 29, dtype="bf16", optimizer=rule, momentum=0.9, lr=1e-6)
        eng.params.normal_(0.0, 0.02)
        eng.grads.normal_(0.0, 1e-3)
        eng.repack_weights()
        eng._packed_dirty = False
        engines[rule] = eng
    times = {rule: [] for rule in RULES}
    stream = torch.cuda.current_stream()
    for rnd in range(args.rounds):
        for rule in RULES:
            eng = engines[rule]
            for _ in range(args.warmup):
                eng.adam_step()
            torch.cuda.synchronize()
            for _ in range(args.reps // args.rounds):
                start, stop = TimingEvent(), TimingEvent()
                start.record(stream)
                eng.adam_step()
                stop.record(stream)
                times[rule].append(1e3 * start.elapsed_time(stop))
    numel = engines["adam"].param_numel
    result = {"device": torch.cuda.get_device_name(0), "parameters": int(numel), "dtype": "bf16", "reps": args.reps,
              "warmup_per_round": args.warmup, "rounds": args.rounds, "rules": {}}
    for rule in RULES:
        t = np.array(times[rule])
        slots = engines[rule].opt_slots
        fp32_bytes = 4 * ((2 + slots) + (1 + slots))  # reads p, g, slots; writes p, slots (+ 2 x 2 bytes of bf16 operands)
        result["rules"][rule] = {"median_us": float(np.median(t)), "p10_us": float(np.percentile(t, 10)),
                                 "p90_us": float(np.percentile(t, 90)), "launches": int(t.size), "state_slots": slots,
                                 "bytes_per_parameter": fp32_bytes + 4,
                                 "GB_per_s_at_median": float((fp32_bytes + 4) * numel / np.median(t) / 1e3)}
        print(rule, result["rules"][rule])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
