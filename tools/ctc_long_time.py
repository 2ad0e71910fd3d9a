#!/usr/bin/env python
"""sl_ctc_loss_grad alone on labels beyond 511 letters (csrc/ctc_long.hip): ms per call, HIP events around each of --iters calls
after --warmup, on the learnt-alignment regime of tools/fuzz_ctc.py, 8 x 4000 frames, bf16 gradient rows 128 wide:
  l_max 1000 and l_max 2047 (labels of l_max / 2 .. l_max letters, the first one l_max), each with sl_ctc_align_long on the same
  logq and labels taking turns with it, call by call;
  l_max 511 on the kernels of ctc.hip and l_max 512 -- the SAME labels padded by one column -- on those of ctc_long.hip, taking
  turns: the step a user pays at the boundary.
--mid: what the wave lattice does not take below 512 letters -- l_max 256, 384 and 511 at K = 29, and 100 letters at K = 64 -- on
  the double log-domain lattice that runs by default and on the fp32 one (sl_ctc_select(1): what ran there before), taking turns
  in one process; --parent-lib adds a third column, the same call into another build of the library (the commit before).
One JSON line per measurement; --out writes them as a list (profiles/ctc_long_time.json, profiles/ctc_mid_time.json).

    python tools/ctc_long_time.py --out profiles/ctc_long_time.json
    python tools/ctc_long_time.py --mid [--parent-lib PATH] --out profiles/ctc_mid_time.json"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

BATCH, FRAMES = 8, 4000


def lattice_states(l_max):
    return 2 * l_max + 1


class Case:
    """logq, probs and labels of one shape in HBM, and the argument lists of the calls on them"""

    def __init__(self, lib, l_max, k, seed, lens=None):
        import torch
        from fuzz_ctc import regime_logits
        rng = np.random.RandomState(seed)
        dev = "cuda:0"
        self.lib, self.l_max, self.k = lib, l_max, k
        if lens is None:
            lens = [int(rng.randint(l_max // 2, l_max + 1)) for _ in range(BATCH)]
            lens[0] = l_max
        self.lens = lens
        width = max(max(lens), 1)
        labels = np.zeros((BATCH, width), dtype=np.int32)
        logits = np.zeros((BATCH, FRAMES, k), dtype=np.float32)
        for i, n in enumerate(lens):
            labels[i, :n] = rng.randint(0, k - 1, size=n)
            logits[i] = regime_logits(rng, list(labels[i, :n]), FRAMES, k, "learnt")
        self.labels = labels
        lg = torch.tensor(logits, device=dev)
        self.probs, self.logq = torch.zeros_like(lg), torch.zeros_like(lg)
        self.ll = torch.tensor(lens, dtype=torch.int32, device=dev)
        self.il = torch.full((BATCH,), FRAMES, dtype=torch.int32, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream
        lib.call("sl_softmax_logq", lg.data_ptr(), self.probs.data_ptr(), self.logq.data_ptr(), BATCH, FRAMES, k, k, FRAMES * k,
                 1e-8, self.st)
        self.keep = []

    def loss_call(self, l_max, select=None, lib=None, column=None):
        """sl_ctc_loss_grad at label-batch width l_max (>= the labels' own width: padded columns); select: sl_ctc_select(that)
        before every call; lib: the build of the library to call instead of the case's own"""
        import torch
        from speechless_amd import _lib
        dev = "cuda:0"
        labels = np.zeros((BATCH, l_max), dtype=np.int32)
        labels[:, :self.labels.shape[1]] = self.labels
        lab = torch.tensor(labels, device=dev)
        loss = torch.zeros((BATCH,), dtype=torch.float32, device=dev)
        dl = torch.zeros((BATCH, FRAMES, 128), dtype=torch.bfloat16, device=dev)
        need = (lib or self.lib).raw("sl_ctc_workspace_bytes")(BATCH, FRAMES, l_max)
        ws = torch.empty((need,), dtype=torch.uint8, device=dev)
        self.keep += [lab, ws]
        args = (self.probs.data_ptr(), self.logq.data_ptr(), lab.data_ptr(), self.ll.data_ptr(), self.il.data_ptr(),
                loss.data_ptr(), dl.data_ptr(), BATCH, FRAMES, self.k, l_max, 0, 128, FRAMES * 128, _lib.SL_BF16, 1e-8,
                1.0 / BATCH, ws.data_ptr(), need, self.st)
        call = dict(name="sl_ctc_loss_grad", args=args, l_max=l_max, workspace_bytes=int(need), loss=loss, grad=dl)
        if select is not None:
            call["select"] = select
        if lib is not None:
            call["lib"] = lib
        if column is not None:
            call["column"] = column
        return call

    def align_call(self):
        import torch
        dev = "cuda:0"
        l_max = self.labels.shape[1]
        lab = torch.tensor(self.labels, device=dev)
        path = torch.zeros((BATCH, FRAMES), dtype=torch.int32, device=dev)
        score = torch.zeros((BATCH,), dtype=torch.float32, device=dev)
        need = self.lib.raw("sl_ctc_align_long_workspace_bytes")(BATCH, FRAMES, l_max)
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
        self.keep += [lab, ws, path]
        args = (self.logq.data_ptr(), lab.data_ptr(), self.ll.data_ptr(), self.il.data_ptr(), path.data_ptr(), score.data_ptr(),
                BATCH, FRAMES, self.k, l_max, ws.data_ptr(), need, self.st)
        return dict(name="sl_ctc_align_long", args=args, l_max=l_max, workspace_bytes=int(need), score=score)


def take_turns(lib, calls, warmup, iters):
    """every call once per round, so that all see the same clocks and the same state of the caches; ms per call"""
    import torch
    times = [[] for _ in calls]
    for i in range(warmup + iters):
        for j, c in enumerate(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if "select" in c:  # (host state of the library, outside the timed interval)
                c.get("lib", lib).call("sl_ctc_select", c["select"])
            a.record()
            c.get("lib", lib).call(c["name"], *c["args"])
            b.record()
            b.synchronize()
            if i >= warmup:
                times[j].append(a.elapsed_time(b))
    out = []
    for c, ts in zip(calls, times):
        r = {"call": c["name"], "batch": BATCH, "frames": FRAMES, "l_max": c["l_max"], "lattice_states": lattice_states(c["l_max"]),
             "iters": iters, "ms_median": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)),
             "us_per_frame": 1e3 * float(np.median(ts)) / FRAMES, "workspace_bytes": c["workspace_bytes"]}
        if "column" in c:
            r["column"] = c["column"]
        if "select" in c:
            c.get("lib", lib).call("sl_ctc_select", 0)
        if "loss" in c:
            loss = c["loss"].cpu().numpy()
            r["feasible"] = int(np.isfinite(loss).sum())
            r["mean_loss"] = float(loss.mean())
        else:
            r["feasible"] = int(np.isfinite(c["score"].cpu().numpy()).sum())
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=29)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", help="also write the results, as a JSON list, to this file")
    ap.add_argument("--mid", action="store_true", help="256 .. 511 letters and K = 64 instead: double against fp32 log-domain lattice")
    ap.add_argument("--parent-lib", help="--mid: another build of libspeechless_hip.so to take turns with this one")
    args = ap.parse_args()
    import torch
    from speechless_amd._lib import HipLibrary, lib as load
    lib = load()
    results = []

    def report(rows, **extra):
        for r in rows:
            r.update(extra)
            results.append(r)
            print(json.dumps(r), flush=True)

    if args.mid:
        parent = HipLibrary(args.parent_lib) if args.parent_lib else None
        for k, l_max in ((29, 256), (29, 384), (29, 511), (64, 100)):
            case = Case(lib, l_max, k, args.seed + l_max)
            calls = [case.loss_call(l_max, select=0, column="double log-domain lattice (default)"),
                     case.loss_call(l_max, select=1, column="fp32 log-domain lattice (sl_ctc_select 1)")]
            if parent is not None:
                calls.append(case.loss_call(l_max, select=0, lib=parent, column="parent build (default)"))
            rows = take_turns(lib, calls, args.warmup, args.iters)
            grads = [c["grad"].float().cpu().numpy() for c in calls]
            report(rows, k=k, labels=[l_max // 2, l_max], ratio_to_fp32=rows[0]["ms_median"] / rows[1]["ms_median"],
                   grad_max_abs_diff_to_default=[float(np.abs(g - grads[0]).max()) for g in grads])
            del case, calls
            torch.cuda.empty_cache()
        if args.out:
            Path(args.out).write_text(json.dumps(results, indent=1) + "\n")
        return
    for l_max in (1000, 2047):
        case = Case(lib, l_max, args.k, args.seed + l_max)
        report(take_turns(lib, [case.loss_call(l_max), case.align_call()], args.warmup, args.iters), labels=[l_max // 2, l_max])
        del case
        torch.cuda.empty_cache()
    # the boundary: labels of 256 .. 511 letters, at l_max 511 and padded by one column to 512 (both ctc_long.hip since 256 ..
    # 511 letters run there: the step between 576- and 640-thread work-groups; --mid has the fp32 lattice beside it)
    case = Case(lib, 511, args.k, args.seed + 511)
    short, padded = case.loss_call(511), case.loss_call(512)
    rows = take_turns(lib, [short, padded], args.warmup, args.iters)
    ls, lp = short["loss"].cpu().numpy(), padded["loss"].cpu().numpy()
    gs, gp = short["grad"].float().cpu().numpy(), padded["grad"].float().cpu().numpy()
    report(rows, labels=[255, 511], boundary_step=rows[1]["ms_median"] / rows[0]["ms_median"],
           lattice_state_ratio=lattice_states(512) / lattice_states(511),
           loss_rel_diff=float(np.abs(ls - lp).max() / np.abs(ls).max()), grad_max_abs_diff=float(np.abs(gs - gp).max()))
    if args.out:
        Path(args.out).write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
