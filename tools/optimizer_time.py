"""Times the fused update + operand repack launch of every optimizer rule (and of Adam) over configuration 3's trainable layer
set -- all eleven layers at the real widths, bf16 operands (--dtype: another operand format) -- and writes
profiles/optimizer_time.json.

One engine per rule, gradients filled with random numbers (the kernels are HBM-bound: the values do not matter); per rule
WARMUP launches, then REPS launches each between two timing events (speechless_amd._hipevents: timestamps only, no
system-scope release); the rules are measured in interleaved rounds so that clock drift hits all of them alike.  Reported per
rule: median, 10th and 90th percentile in microseconds, and the fp32 bytes the rule moves per parameter.

    python tools/optimizer_time.py [--reps 200] [--warmup 20] [--dtype bf16] [--rules adam,sgd] [--out profiles/optimizer_time.json]

SL_LIB_PATH selects a probe build: for A/B turns of two builds of the library, one process per turn."""
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
    parser.add_argument("--dtype", default="bf16", help="bf16, bf16x3, f16x3 or f32")
    parser.add_argument("--rules", default=",".join(RULES), help="comma-separated subset of " + ",".join(RULES))
    parser.add_argument("--out", default=str(ROOT / "profiles" / "optimizer_time.json"))
    args = parser.parse_args()
    rules = args.rules.split(",")
    import torch
    from speechless_amd._hipevents import TimingEvent
    from speechless_amd.engine import Engine, wav2letter_layer_specs
    specs = wav2letter_layer_specs(128, 29)
    engines = {}
    for rule in rules:
        eng = Engine(specs, 29, dtype=args.dtype, optimizer=rule, momentum=0.9, lr=1e-6)
        eng.params.normal_(0.0, 0.02)
        eng.grads.normal_(0.0, 1e-3)
        eng.repack_weights()
        eng._packed_dirty = False
        engines[rule] = eng
    times = {rule: [] for rule in rules}
    stream = torch.cuda.current_stream()
    for rnd in range(args.rounds):
        for rule in rules:
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
    numel = engines[rules[0]].param_numel
    result = {"device": torch.cuda.get_device_name(0), "parameters": int(numel), "dtype": args.dtype, "reps": args.reps,
              "warmup_per_round": args.warmup, "rounds": args.rounds, "rules": {}}
    for rule in rules:
        t = np.array(times[rule])
        slots = engines[rule].opt_slots
        fp32_bytes = 4 * ((2 + slots) + (1 + slots))  # reads p, g, slots; writes p, slots (+ the two operand copies)
        operand_bytes = 2 * {"bf16": 2, "f32": 4}.get(args.dtype, 6)
        result["rules"][rule] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max()),
                                 "p10_us": float(np.percentile(t, 10)),
                                 "p90_us": float(np.percentile(t, 90)), "launches": int(t.size), "state_slots": slots,
                                 "bytes_per_parameter": fp32_bytes + operand_bytes,
                                 "GB_per_s_at_median": float((fp32_bytes + operand_bytes) * numel / np.median(t) / 1e3)}
        print(rule, result["rules"][rule])
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps({"written": args.out}))


if __name__ == "__main__":
    main()
