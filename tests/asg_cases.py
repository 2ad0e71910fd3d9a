"""Shared helpers of tests/test_asg_cases.py (CPU) and tests/test_gpu_asg_mid.py (GPU): emission regimes and score tables of
the size a trained ASG net has, the batches both modules use, sl_asg_loss_grad with every output optional, and the bounds.

Emission regimes (asg_regime_logits).  "uniform", "sharp" and "collapse" are tools/fuzz_ctc.regime_logits, unchanged.  "learnt"
and "wrong" are ASG-shaped -- there is no blank: the T frames are cut into len(label) non-empty runs, and `strength` (drawn from
uniform(6, 40) as in fuzz_ctc, or given) is added to letter l_s on every frame of run s; "wrong" lays the runs out for a copy of
the label in which 40 % of the letters are replaced by another letter.

Score tables (asg_scores).  "random": uniform(-2, 2), what tests/test_gpu_asg.py draws.  "bigram": trans[i, j] = +s for every
pair adjacent in some label of the batch, trans[i, i] = +s / 2, -s everywhere else; init = +s on the letters that start a label,
-s elsewhere.  "hostile": the bigram tables negated -- the label's own path is the one the tables punish.  s is 12 or 30: with
eps = 1e-8 one frame changes a value of the probability-domain denominator lattices by a factor between 1e-21 and 1e13.

Bounds (check_tight).  sl_asg_loss_grad rounds to fp32 exactly once per output -- dz = (float)(grad_scale * (x - p * inner)),
loss = (float)(logz - N), (float)(grad_scale * sum) in the reduce -- and everything before is double arithmetic on the fp32
probabilities the float64 restatement (tests/test_asg.py, asg_reference_batch) is given too.  So:
  dlogits       : every entry within 1e-6 * grad_scale (entries are at most 2 in magnitude: half an fp32 ulp is 1.2e-7)
  loss          : |got - ref| <= 1e-6 |ref| + 1e-6
  dtrans, dinit : |got - ref| <= 1e-6 |ref| + 1e-6 * grad_scale
  rows at and past T_b exactly zero; an infeasible utterance (L = 0, T_b = 0, L > T_b) +inf from kernel and restatement, all its
  dlogits rows zero, nothing added to the table gradients.
The floor of double arithmetic under these bounds -- asg_reference against float64 autograd at 511 letters, 900 frames and
s = 30 -- is below 1e-7 (tests/test_asg_cases.py asserts that; 9.4e-10 on dtrans is the largest distance its cases give).  eps and
grad_scale reach the kernel as floats, so the restatement is given float(np.float32(eps)) and float(np.float32(grad_scale)).
"""
import sys
from pathlib import Path

import numpy as np

from test_asg import EPS, asg_reference_batch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT / "tools") not in sys.path:
    sys.path.insert(0, str(ROOT / "tools"))
from fuzz_ctc import regime_logits as fuzz_regime_logits  # noqa: E402

REGIMES = ("uniform", "sharp", "collapse", "learnt", "wrong")
SCORE_KINDS = ("random", "bigram", "hostile")
FILL = 7.5        # what every output holds before a call: an entry the kernel does not write shows
MAX_FRAMES = 900  # no case of the GPU module has more frames
TIGHT = 1e-6


# ------------------------------------------------------------------------------------------------------------ generators
def asg_regime_logits(rng, label, t, k, kind, strength=None):
    """(t, k) float32 logits of one utterance in regime `kind` (module docstring).  A label that is empty or longer than t gets
    no runs (plain noise)."""
    if kind in ("uniform", "sharp", "collapse"):
        return fuzz_regime_logits(rng, label, t, k, kind)
    if kind not in ("learnt", "wrong"):
        raise ValueError("unknown regime {!r}".format(kind))
    lg = rng.randn(t, k).astype(np.float32)
    lab = [int(c) for c in label]
    if kind == "wrong":  # c + 1 .. c + k - 1 (mod k): always another letter, at k = 2 the other one
        lab = [int((c + 1 + rng.randint(0, k - 1)) % k) if rng.rand() < 0.4 else c for c in lab]
    if strength is None:
        strength = rng.uniform(6, 40)
    n = len(lab)
    if 0 < n <= t:
        cuts = np.sort(rng.choice(np.arange(1, t), size=n - 1, replace=False)) if n > 1 else np.array([], dtype=int)
        bounds = np.concatenate([[0], cuts, [t]]).astype(int)
        for s, c in enumerate(lab):
            lg[bounds[s]:bounds[s + 1], c] += np.float32(strength)
    return lg


def asg_scores(rng, labels_list, k, kind, s=None):
    """(trans (k, k) [from][to], init (k,)) float32 of kind "random", "bigram" or "hostile" (module docstring)"""
    if kind == "random":
        return rng.uniform(-2, 2, size=(k, k)).astype(np.float32), rng.uniform(-2, 2, size=k).astype(np.float32)
    if kind not in ("bigram", "hostile"):
        raise ValueError("unknown score kind {!r}".format(kind))
    if s not in (12, 30):
        raise ValueError("bigram / hostile scores take s = 12 or 30")
    trans = np.full((k, k), -float(s), dtype=np.float32)
    init = np.full(k, -float(s), dtype=np.float32)
    for label in labels_list:
        for a, c in zip(label, label[1:]):
            trans[a, c] = s
        if len(label):
            init[label[0]] = s
    trans[np.arange(k), np.arange(k)] = s / 2.0
    if kind == "hostile":
        trans, init = -trans, -init
    return trans, init


def frames_of(specs):
    """T_b per utterance of specs = [(L, slack, regime)]: L + slack (a negative slack makes an utterance infeasible, never
    below zero frames)"""
    return [max(int(n) + int(slack), 0) for n, slack, _ in specs]


def t_out_of(specs):
    """the frames of the batch: the largest T_b -- plus one when that sum is a multiple of 4, so that asg_grad_kernel's last
    work-group (4 frames) is full in some batches and partial in the others, and no utterance reaches t_out in the former"""
    t_max = max(frames_of(specs) + [1])
    return t_max + 1 if (t_max + 1) % 4 == 0 else t_max


def build_asg_batch(rng, k, specs, t_out=None, strength=None):
    """specs: [(L, slack, regime)] -> (logits (B, t_out, k) with zero rows past T_b, labels_list, input_len).  Letters are drawn
    from all k (no blank), adjacent equal letters included."""
    labels_list = [[int(c) for c in rng.randint(0, k, size=n)] for n, _, _ in specs]
    input_len = frames_of(specs)
    t_out = t_out_of(specs) if t_out is None else t_out
    assert max(input_len) <= t_out <= MAX_FRAMES
    logits = np.zeros((len(specs), t_out, k), dtype=np.float32)
    for i, (label, t_b, (_, _, regime)) in enumerate(zip(labels_list, input_len, specs)):
        if t_b > 0:
            logits[i, :t_b] = asg_regime_logits(rng, label, t_b, k, regime, strength=strength)
    return logits, labels_list, input_len


# -------------------------------------------------------------------------------------- the cases of tests/test_gpu_asg_mid.py
# both sides of every asg_lattice_kernel<NS> instantiation (lm <= 64 / 128 / 256 / 512), the middle of the widest, and 511: the
# last state of lane 63 at eight states per lane
BOUNDARY_LENGTHS = (63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 511)
TABLE_SHAPES = ((29, 511), (64, 511), (64, 255), (63, 300), (34, 129), (3, 300), (2, 300))  # (k, L)
TABLE_SCORES = (("bigram", 12), ("bigram", 30), ("hostile", 30))
FUZZ_CALLS = ((2, "hostile", 30), (29, "random", None), (64, "bigram", 30), (29, "bigram", 12))  # (k, score kind, s) per call of 8


def boundary_specs(index):
    n = BOUNDARY_LENGTHS[index]
    return [(n, slack, REGIMES[(3 * index + j) % 5]) for j, slack in enumerate((0, 1, n // 4))]


def table_specs(n):
    return [(n, 0, "learnt"), (n, 9, "wrong"), (n // 2, 40, "sharp"), (n // 3, 200, "collapse")]


def chunk_batches():
    """[(specs, t_out)]: for L = 5 and L = 300, T_b = L .. L + 17 spread over three batches of six with a common t_out, the
    t_out of the six batches covering every residue mod 4; then L = 1 with T_b = 7, 8, 9"""
    out = []
    for n in (5, 300):
        for j in range(3):
            slacks = [j + 3 * i for i in range(6)]
            t_max = n + slacks[-1]
            want = (len(out) + 1) % 4
            t_out = t_max + 1 + (want - (t_max + 1)) % 4  # the first count above t_max with that residue
            out.append(([(n, slack, REGIMES[(i + j) % 5]) for i, slack in enumerate(slacks)], t_out))
    out.append(([(1, 6, "learnt"), (1, 7, "sharp"), (1, 8, "wrong")], 10))
    return out


# a tight 511-letter label, L = 0, L = 1, 300 letters with input_len below t_out, 400 letters in 380 frames, T_b = 0
MIXED_511_SPECS = [(511, 0, "learnt"), (0, 500, "collapse"), (1, 332, "wrong"), (300, 111, "sharp"), (400, -20, "uniform"),
                   (3, -3, "learnt")]
MIXED_511_FEASIBLE = (0, 2, 3)


def fuzz_stream():
    """four calls of eight utterances: [(k, score kind, s, specs)]; L from 1 to 511, slack from 0 to 300 (at most 900 frames),
    the regimes in turn"""
    rng = np.random.RandomState(511)
    calls = []
    for c, (k, kind, s) in enumerate(FUZZ_CALLS):
        specs = []
        for i in range(8):
            n = (511, 1)[c] if (i == 3 and c < 2) else int(rng.randint(1, 512))
            slack = min(int(rng.randint(0, 301)), MAX_FRAMES - n)
            specs.append((n, slack, REGIMES[(8 * c + i) % 5]))
        calls.append((k, kind, s, specs))
    return calls


MODE_CASES = {  # name -> (k, destination row stride, specs)
    "300_letters": (29, 40, [(300, 0, "wrong"), (280, 30, "uniform"), (5, 100, "learnt")]),
    "60_letters_64_classes": (64, 72, [(60, 0, "sharp"), (50, 10, "learnt"), (0, 30, "collapse")]),
}
WORKSPACE_LENGTHS = (300, 60, 511)


def workspace_specs(n):
    return [(n, 0, "sharp"), (n // 2, 25, "learnt"), (n // 3 + 5, -5, "wrong")]  # the last one infeasible: it writes no lattice


def all_gpu_specs():
    """every (specs, t_out) the GPU module runs -- for the frame limit"""
    out = [(boundary_specs(i), None) for i in range(len(BOUNDARY_LENGTHS))]
    out += [(table_specs(n), None) for _, n in TABLE_SHAPES]
    out += chunk_batches()
    out += [(MIXED_511_SPECS, None)]
    out += [(specs, None) for _, _, _, specs in fuzz_stream()]
    out += [(specs, None) for _, _, specs in MODE_CASES.values()]
    out += [(workspace_specs(n), None) for n in WORKSPACE_LENGTHS]
    return [(specs, t_out_of(specs) if t_out is None else t_out) for specs, t_out in out]


# ------------------------------------------------------------------------------------------------------------ the kernel
class AsgRun:
    """what run_asg returns, everything as numpy.  dl is the (B, T', K) window of the destination (None for a bf16 one),
    dest the whole destination (uint16 bit patterns for bf16) -- all of it, whether or not a pointer was passed."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def outputs(self):
        return self.loss, self.dest, self.dg, self.dg0


def run_asg(hip_lib, logits, g, g0, labels_list, input_len, eps=EPS, grad_scale=1.0, l_max=None, ws=None, dlogits=True,
            tables=True, dest="f32", halo=0, rs=None, pad=0, k=None):
    """sl_softmax_logq, then sl_asg_loss_grad.  Every output starts from FILL.  ws: a uint8 tensor used as the workspace with
    whatever it holds (default: a fresh one of exactly sl_asg_workspace_bytes).  dlogits=False / tables=False: NULL in place of
    dlogits / of dtrans AND dinit (the buffers exist all the same and are returned: they must still hold FILL).  dest: "f32" or
    "bf16", with g_row0 = halo, row stride rs (default k) and batch stride (T' + 2 halo) rs + pad."""
    import torch
    from speechless_amd import _lib
    b, t, kk = logits.shape
    k = kk if k is None else k
    assert t <= MAX_FRAMES
    dev = "cuda:0"
    l_max = max([len(lab) for lab in labels_list] + [1]) if l_max is None else l_max
    labels = np.zeros((b, max(l_max, 1)), dtype=np.int32)
    for i, lab in enumerate(labels_list):
        labels[i, :len(lab)] = lab
    st = torch.cuda.current_stream().cuda_stream
    lg = torch.tensor(logits, dtype=torch.float32, device=dev)
    probs = torch.zeros((b, t, kk), dtype=torch.float32, device=dev)
    logq = torch.zeros_like(probs)
    hip_lib.call("sl_softmax_logq", lg.data_ptr(), probs.data_ptr(), logq.data_ptr(), b, t, kk, kk, t * kk, eps, st)
    tg = torch.tensor(np.asarray(g), dtype=torch.float32, device=dev)
    tg0 = torch.tensor(np.asarray(g0), dtype=torch.float32, device=dev)
    lab_t = torch.tensor(labels, dtype=torch.int32, device=dev)
    ll = torch.tensor([len(lab) for lab in labels_list], dtype=torch.int32, device=dev)
    il = torch.tensor(list(input_len), dtype=torch.int32, device=dev)
    loss = torch.full((b,), FILL, dtype=torch.float32, device=dev)
    rs = k if rs is None else rs
    bs = (t + 2 * halo) * rs + pad
    dst = torch.full((b * bs,), FILL, dtype=torch.bfloat16 if dest == "bf16" else torch.float32, device=dev)
    dg = torch.full((k, k), FILL, dtype=torch.float32, device=dev)
    dg0 = torch.full((k,), FILL, dtype=torch.float32, device=dev)
    need = hip_lib.raw("sl_asg_workspace_bytes")(b, t, k, l_max)
    if ws is None:
        ws = torch.empty((max(need, 16),), dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    rc = hip_lib.raw("sl_asg_loss_grad")(probs.data_ptr(), logq.data_ptr(), tg.data_ptr(), tg0.data_ptr(), lab_t.data_ptr(),
                                         ll.data_ptr(), il.data_ptr(), loss.data_ptr(), dst.data_ptr() if dlogits else None,
                                         dg.data_ptr() if tables else None, dg0.data_ptr() if tables else None, b, t, k, l_max,
                                         halo, rs, bs, _lib.SL_BF16 if dest == "bf16" else _lib.SL_F32, eps, grad_scale,
                                         ws.data_ptr(), need, st)
    torch.cuda.synchronize()
    whole = dst.view(torch.int16).cpu().numpy().view(np.uint16) if dest == "bf16" else dst.cpu().numpy()
    dl = None
    if dest == "f32" and k == kk:
        rows = whole.reshape(b, bs)[:, :(t + 2 * halo) * rs].reshape(b, t + 2 * halo, rs)
        dl = np.ascontiguousarray(rows[:, halo:halo + t, :k])
    return AsgRun(rc=rc, probs=probs.cpu().numpy(), loss=loss.cpu().numpy(), dl=dl, dest=whole, dg=dg.cpu().numpy(),
                  dg0=dg0.cpu().numpy(), geometry=(b, t, k, halo, rs, bs))


def expected_destination(dl, geometry, bf16):
    """the whole destination after a call that wrote the fp32 result `dl`: FILL everywhere but [halo, halo + T') x [0, K) of
    every utterance, there dl (bf16: rounded to nearest even, as bit patterns)"""
    import torch
    b, t, k, halo, rs, bs = geometry
    want = torch.full((b * bs,), FILL, dtype=torch.bfloat16 if bf16 else torch.float32)
    src = torch.from_numpy(np.ascontiguousarray(dl))
    for i in range(b):
        rows = want[i * bs:i * bs + (t + 2 * halo) * rs].view(t + 2 * halo, rs)
        rows[halo:halo + t, :k] = src[i].to(want.dtype)
    return want.view(torch.int16).numpy().view(np.uint16) if bf16 else want.numpy()


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ the bounds
def tight_errors(probs, loss, dl, dg, dg0, g, g0, labels_list, input_len, eps=EPS, grad_scale=1.0):
    """distances from the float64 restatement on the same fp32 probabilities, each in units of its bound's scale (at most
    TIGHT = 1e-6 to pass): {"loss": |d| / (|ref| + 1), "dlogits": |d| / grad_scale, "dtrans" / "dinit": |d| / (|ref| +
    grad_scale)} per utterance (loss, dlogits) or over the batch; plus the restatement itself"""
    eps, grad_scale = float(np.float32(eps)), float(np.float32(grad_scale))
    ref = asg_reference_batch(probs.astype(np.float64), np.asarray(g, dtype=np.float64), np.asarray(g0, dtype=np.float64),
                              labels_list, input_len, eps=eps, grad_scale=grad_scale)
    ref_loss, ref_dl, ref_dg, ref_dg0 = ref
    fin = np.isfinite(ref_loss)
    with np.errstate(invalid="ignore"):
        e_loss = np.where(fin, np.abs(loss - ref_loss) / (np.abs(ref_loss) + 1.0), 0.0)
    err = {"loss": e_loss}
    if dl is not None:
        err["dlogits"] = np.abs(dl - ref_dl).reshape(len(labels_list), -1).max(1) / grad_scale
    if dg is not None:
        err["dtrans"] = float((np.abs(dg - ref_dg) / (np.abs(ref_dg) + grad_scale)).max())
        err["dinit"] = float((np.abs(dg0 - ref_dg0) / (np.abs(ref_dg0) + grad_scale)).max())
    return err, ref


def check_tight(run, g, g0, labels_list, input_len, eps=EPS, grad_scale=1.0, regimes=None, tables=True):
    """The bounds of the module docstring on an AsgRun (run.dl None: a call without dlogits; tables=False: one without dtrans /
    dinit).  Prints every figure before it asserts; returns the worst error per output, in units of its bound's scale."""
    assert run.rc == 0
    t_out = run.probs.shape[1]
    dg, dg0 = (run.dg, run.dg0) if tables else (None, None)
    err, (ref_loss, ref_dl, ref_dg, ref_dg0) = tight_errors(run.probs, run.loss, run.dl, dg, dg0, g, g0, labels_list, input_len,
                                                            eps, grad_scale)
    for i, label in enumerate(labels_list):
        t_b = min(max(int(input_len[i]), 0), t_out)
        print("utterance %d: %3d letters, %3d of %3d frames, %-8s loss %.9g (float64 %.9g, error %.2e)%s" % (
            i, len(label), t_b, t_out, regimes[i] if regimes else "", run.loss[i], ref_loss[i], err["loss"][i],
            "" if run.dl is None else ", dlogits error %.2e of grad_scale" % err["dlogits"][i]))
    if tables:
        print("dtrans error %.2e (largest entry %.4g), dinit error %.2e" % (err["dtrans"], np.abs(ref_dg).max(), err["dinit"]))
    for i, label in enumerate(labels_list):
        t_b = min(max(int(input_len[i]), 0), t_out)
        if 0 < len(label) <= t_b:
            assert np.isfinite(ref_loss[i]), (i, ref_loss[i], "the case is meant to be feasible")
            assert abs(run.loss[i] - ref_loss[i]) <= TIGHT * abs(ref_loss[i]) + TIGHT, (i, run.loss[i], ref_loss[i])
        else:
            assert np.isposinf(ref_loss[i]) and np.isposinf(run.loss[i]), (i, run.loss[i], ref_loss[i])
            assert run.dl is None or not run.dl[i].any(), (i, "an infeasible utterance has no gradient")
        if run.dl is not None:
            assert err["dlogits"][i] <= TIGHT, (i, err["dlogits"][i])
            assert not run.dl[i, t_b:].any(), (i, "rows at and past T_b must be exactly zero")
    if tables:
        assert np.isfinite(run.dg).all() and np.isfinite(run.dg0).all()
        assert err["dtrans"] <= TIGHT and err["dinit"] <= TIGHT, (err["dtrans"], err["dinit"])
    worst = {"loss": float(err["loss"].max())}
    if run.dl is not None:
        worst["dlogits"] = float(err["dlogits"].max())
    if tables:
        worst["dtrans"], worst["dinit"] = err["dtrans"], err["dinit"]
    return worst
