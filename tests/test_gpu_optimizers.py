"""GPU tests of the Keras 2.0.x optimizers beside Adam (SGD, RMSprop, Adagrad, Adadelta, Adamax): the flat kernel against the
float64 restatement of test_optimizers.py, the fused update + repack launch against the flat one bit for bit on all four
operand formats, the engine's training step, the missing second state buffer of the one-slot rules, two data-parallel ranks
with the sharded optimizer, Wav2Letter with each optimizer class through a saved optimizer state, and Adam unchanged.

Shapes: test_gpu_parity.make_case on the REAL layer widths (250 -> 256 and 2000 -> 2048 channel padding, the ones channel),
b = 2, t = 64 and b = 3, t = 77.

THE BOUNDS (u = 2^-24, half an ulp of fp32 relative to the value):
  state slots   |s_gpu - s_ref| <= 2e-5 |s_ref| + E_s           (2e-5: what Adam's v is held to, a handful of fp32 roundings
                                                                 and the fp32 value of 1 - rho / 1 - beta)
  parameters    |p_gpu - p_ref| <= N u |p_ref| + 2e-5 sum_k |step_k| + E_p,   N = max(2, number of updates compared over)
                for the two updates of the kernel tests this is the 1.2e-7 |p'| + 2e-5 |p' - p| of a stored value rounded
                twice; every further update rounds the stored master once more, whatever the rule.
E_s, E_p are zero for the rules whose slots are sums of non-negative terms (RMSprop, Adagrad, Adadelta).  The slot m of SGD
(momentum m - lr g) and of Adamax (b1 m + (1 - b1) g) is a sum of terms of either sign: when they cancel, the rounding of the
TERMS (u each for the product, the inherited m, the fp32 coefficient; one more for the sum: 4 u) is not small against the
result, and no arithmetic in fp32 can make it so.  The running bound of that error is carried along with the restatement:
  E_m' = c E_m + 4 u (c |m| + w |g|)        (c, w) = (momentum, lr) for SGD, (b1, 1 - b1) for Adamax
  E_p  = E_m' (SGD), (1 + momentum) E_m' (nesterov), lr_t E_m' / (u' + eps) (Adamax)
Without cancellation c |m| + w |g| = |m'| and 4 u = 2.4e-7 disappears in the 2e-5.
Adadelta needs no wider constant: its step g sqrt(d + eps) / sqrt(a' + eps) is two roots, a product and a quotient over
operands that carry <= 5e-7 (a': three roundings and the fp32 value of 1 - rho, halved by the root; d likewise) -- about
1e-6 relative, a twentieth of 2e-5; d' = rho d + (1 - rho) u^2 doubles that and stays inside 2e-5 too."""
import os

import numpy as np
import pytest

from test_gpu_optimizer_clip import case_with_norm, train
from test_gpu_parity import make_case, make_engine, run_loss_and_grads
from test_optimizers import KERAS_DEFAULTS, SLOTS, keras_optimizer_step
from test_optimizer_clip import keras_clipped_gradients, keras_decayed_lr
from test_parallel import _engine_case, _free_port

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CASES = {  # name -> (rule, Keras hyper-parameters): the defaults, momentum for SGD
    "sgd": ("sgd", dict(lr=0.01, momentum=0.9)),
    "nesterov": ("sgd", dict(lr=0.01, momentum=0.9, nesterov=True)),
    "rmsprop": ("rmsprop", {}),
    "adagrad": ("adagrad", {}),
    "adadelta": ("adadelta", {}),
    "adamax": ("adamax", {}),
}
ENGINE_NAMES = {"epsilon": "adam_epsilon"}


def engine_kwargs(rule, hyper):
    return dict(optimizer=rule, **{ENGINE_NAMES.get(k, k): v for k, v in hyper.items()})


class Restated:
    """the float64 restatement of consecutive updates of a list of tensors, with the running bounds of the module docstring"""

    def __init__(self, rule, params, hyper, decay=0.0, clipnorm=0.0, clipvalue=0.0):
        self.rule, self.h = rule, dict(KERAS_DEFAULTS[rule], **hyper)
        self.settings = dict(decay=decay, clipnorm=clipnorm, clipvalue=clipvalue)
        self.params = [np.asarray(p, dtype=np.float64) for p in params]
        self.slots = [[np.zeros_like(p) for p in self.params] for _ in range(SLOTS[rule])]
        self.e_m = [np.zeros_like(p) for p in self.params]
        self.e_p = [np.zeros_like(p) for p in self.params]
        self.moved = [np.zeros_like(p) for p in self.params]
        self.it = 0

    def step(self, grads):
        h, rule = self.h, self.rule
        clipped, n = keras_clipped_gradients(grads, self.settings["clipnorm"], self.settings["clipvalue"])
        lr = keras_decayed_lr(h["lr"], self.settings["decay"], self.it)
        before, m_before = self.params, self.slots[0]
        self.params, self.slots, _ = keras_optimizer_step(rule, self.params, grads, self.slots, self.it, **self.settings, **h)
        for i, g in enumerate(clipped):
            if rule == "sgd":
                c, w = h["momentum"], lr
            elif rule == "adamax":
                c, w = h["beta_1"], 1.0 - h["beta_1"]
            else:
                continue
            self.e_m[i] = c * self.e_m[i] + 4 * U * (c * np.abs(m_before[i]) + w * np.abs(g))
            if rule == "sgd":
                self.e_p[i] = self.e_p[i] + (1.0 + h["momentum"] if h["nesterov"] else 1.0) * self.e_m[i]
            else:
                lr_t = lr / (1.0 - h["beta_1"] ** (self.it + 1))
                self.e_p[i] = self.e_p[i] + lr_t * self.e_m[i] / (self.slots[1][i] + h["epsilon"])
        for i in range(len(self.params)):
            self.moved[i] = self.moved[i] + np.abs(self.params[i] - before[i])
        self.it += 1
        return n

    def worst_ratios(self, got_params, got_slots):
        """largest |difference| / bound over all tensors, for the parameters and for each slot"""
        n_roundings = max(2, self.it)
        worst = [0.0] * (1 + len(self.slots))
        for i, ref in enumerate(self.params):
            bound = n_roundings * U * np.abs(ref) + 2e-5 * self.moved[i] + self.e_p[i] + 1e-30
            worst[0] = max(worst[0], float(np.max(np.abs(got_params[i].astype(np.float64) - ref) / bound)))
            for k, slot in enumerate(self.slots):
                bound = 2e-5 * np.abs(slot[i]) + (self.e_m[i] if k == 0 else 0.0) + 1e-30
                worst[1 + k] = max(worst[1 + k], float(np.max(np.abs(got_slots[k][i].astype(np.float64) - slot[i]) / bound)))
        return worst


def opt_rule(rule, h, lr, t):
    from speechless_amd import _lib
    r = _lib.OptRule()
    r.rule = _lib.OPT_RULES[rule]
    r.lr = lr / (1.0 - h["beta_1"] ** t) if rule == "adamax" else lr
    r.momentum, r.nesterov, r.rho = h.get("momentum", 0.0), int(h.get("nesterov", False)), h.get("rho", 0.0)
    r.beta1, r.beta2, r.eps = h.get("beta_1", 0.0), h.get("beta_2", 0.0), h.get("epsilon", 0.0)
    return r


# ------------------------------------------------------------------------------------------ 1. the flat kernel alone
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_flat_kernel_two_steps_against_the_restatement(hip_lib, name, clip):
    """n = 4, 1028 (one block and one vector) and 4100; p ~ +-1, |g| from 1e-6 to 10 with exact zeros; two updates from zero
    state; with clip: *grad_scale = 0.5 and clipvalue 0.25 (the restatement gets the factor as a pre-scaled gradient: 0.5 g is
    exact).  Bounds: the module docstring."""
    import torch
    rule, hyper = CASES[name]
    st = torch.cuda.current_stream().cuda_stream
    for n in (4, 1028, 4100):
        rng = np.random.RandomState(n)
        p0 = rng.randn(n).astype(np.float32)
        grads = []
        for _ in range(2):
            g = (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-6, 1, size=n)).astype(np.float32)
            g[rng.rand(n) < 0.05] = 0.0
            g[1] = 0.0
            grads.append(g)
        ref = Restated(rule, [p0], hyper, clipvalue=0.25 if clip else 0.0)
        tp = torch.tensor(p0, device="cuda:0")
        slots = [torch.zeros_like(tp) for _ in range(SLOTS[rule])]
        scale = torch.tensor([0.5], dtype=torch.float32, device="cuda:0")
        for t, g in enumerate(grads, start=1):
            tg = torch.tensor(g, device="cuda:0")
            hip_lib.call("sl_optimizer_step", tp.data_ptr(), tg.data_ptr(), slots[0].data_ptr(),
                         slots[1].data_ptr() if len(slots) == 2 else None, n, opt_rule(rule, ref.h, ref.h["lr"], t),
                         scale.data_ptr() if clip else None, 0.25 if clip else 0.0, st)
            torch.cuda.synchronize()
            assert np.array_equal(tg.cpu().numpy(), g)  # the gradient itself is not rewritten
            ref.step([g.astype(np.float64) * (0.5 if clip else 1.0)])
        worst = ref.worst_ratios([tp.cpu().numpy()], [[s.cpu().numpy()] for s in slots])
        print("flat", name, "clip" if clip else "plain", "n", n, "worst ratio to the bound: p, slots", worst)
        assert max(worst) <= 1.0, (name, n, worst)
        assert np.abs(tp.cpu().numpy() - p0).max() > 0


# ------------------------------------------------------------------------------------------ 2. fused against flat
def engine_state(eng):
    return [eng.params, eng.adam_m] + ([eng.adam_v] if eng.adam_v is not None else []) + \
        [w for w in eng.w_fwd + eng.w_dgrad if w is not None]


@pytest.mark.parametrize("frozen,clip", [pytest.param(0, False, id="0"), pytest.param(3, False, id="3"),
                                         pytest.param(0, True, id="0-clip")])
@pytest.mark.parametrize("dtype", ["bf16", "f32", "bf16x3", "f16x3"])
@pytest.mark.parametrize("name", ["adam", "nesterov", "rmsprop", "adagrad", "adadelta", "adamax"])
def test_fused_launch_equals_flat_launch_and_repack_bit_for_bit(name, dtype, frozen, clip):
    """two updates (the second from non-zero state): adam_step(fused=True) against adam_step(fused=False) + repack_weights();
    masters, slots and both operand copies of every layer byte-identical.  Six rules x four operand formats x (plain, clipped):
    every instantiation of the fused kernel against the flat kernel's.

    clip: both engines get clipnorm = half the norm n0 of the first backward (as ENGINE_CASES) and clipvalue = half the median
    |g| of that backward.  The first update therefore runs with the factor clipnorm / n0 = 0.5 on the device, and of the scaled
    elements 0.5 |g| those above the median exceed clipvalue = 0.5 median and are clamped, those below pass (the median counts
    the exact zeros of dead channels, so more than half of the non-zero elements clamp: the counts are printed).  Asserted on
    the first update; the second update's norm is whatever the first one left, and it is clipped with the same settings."""
    import torch
    rule, hyper = dict(CASES, adam=("adam", {}))[name]
    case = make_case(b=2, t=64, seed=3)
    extra = {}
    if clip:
        _, n0, median = case_with_norm(2, 64, dtype)  # (the same case: make_case(b=2, t=64, seed=3))
        extra = dict(clipnorm=0.5 * n0, clipvalue=0.5 * median)
    engines = [make_engine(case, dtype, frozen_layer_count=frozen, **engine_kwargs(rule, hyper), **extra) for _ in range(2)]
    start = engines[0].params.clone()
    for it in range(2):
        for eng, fused in zip(engines, (True, False)):
            run_loss_and_grads(eng, case)
            if clip and it == 0:
                factor = float(eng._norm_out[1].item())
                scaled = eng.grads.abs() * factor
                print("fused" if fused else "flat", name, dtype, "clip factor", factor, "clipvalue", extra["clipvalue"],
                      "clamped", int((scaled > extra["clipvalue"]).sum()), "of", int((scaled > 0).sum()), "non-zero")
                assert factor < 1.0
                assert bool((scaled > extra["clipvalue"]).any())
                assert bool(((scaled > 0) & (scaled < extra["clipvalue"])).any())
            eng.adam_step(fused=fused)
            if not fused:
                eng.repack_weights()
        torch.cuda.synchronize()
        for a, b in zip(engine_state(engines[0]), engine_state(engines[1])):
            assert torch.equal(a, b)
    assert not torch.equal(engines[0].params, start) and engines[0].adam_iterations == 2
    assert (engines[0].adam_v is None) == (dict(SLOTS, adam=2)[rule] == 1)


# ------------------------------------------------------------------------------------------ 3. the engine's step
# Learning rates: as test_gpu_optimizer_clip chooses them -- at random init three updates of 1e-4 per element (Adam) raise the
# gradient norm fivefold, so every rule gets a rate that moves an element by about 1e-4 or less per update: SGD 1e-5 (steps
# lr * g with |g| up to ~1), RMSprop / Adamax 1e-4 (steps ~ lr), Adagrad 1e-4, Adadelta lr = 0.1 (steps ~ lr * sqrt(eps) = 1e-5).
ENGINE_CASES = {
    "sgd": ("sgd", dict(lr=1e-5, momentum=0.9), {}),
    "rmsprop": ("rmsprop", dict(lr=1e-4), {}),
    "adagrad": ("adagrad", dict(lr=1e-4), {}),
    "adadelta": ("adadelta", dict(lr=0.1), {}),
    "adamax": ("adamax", dict(lr=1e-4), {}),
    "nesterov_clipnorm_decay": ("sgd", dict(lr=1e-5, momentum=0.9, nesterov=True), dict(decay=0.5, clipnorm=0.5)),
    "adadelta_clipnorm_decay": ("adadelta", dict(lr=0.1), dict(decay=0.5, clipnorm=0.5)),
}


@pytest.mark.parametrize("name", list(ENGINE_CASES))
def test_three_engine_steps_match_the_restatement(name):
    """bf16, b = 3, t = 77; the restatement is fed the engine's own (unclipped) gradients of each step; clipnorm = 0.5 n0.
    Masters and slots after every step against the bounds of the module docstring (N = 2 for the first two steps, 3 for
    the third: the stored master has been rounded three times by then)."""
    import torch
    rule, hyper, extra = ENGINE_CASES[name]
    case, n0, _ = case_with_norm(3, 77, "bf16")
    extra = dict(extra)
    if "clipnorm" in extra:
        extra["clipnorm"] *= n0
    eng = make_engine(case, "bf16", **engine_kwargs(rule, hyper), **extra)
    ref = Restated(rule, [a for pair in case["weights"] for a in pair], hyper, **extra)
    for it in range(3):
        train(eng, case)
        torch.cuda.synchronize()
        n = ref.step([a.astype(np.float64) for pair in eng.get_gradients() for a in pair])
        if "clipnorm" in extra:
            assert abs(float(eng.grad_norm.item()) - n) <= 1e-6 * n and (it > 0 or n >= extra["clipnorm"])
        state = eng.get_optimizer_state()
        assert state["optimizer"] == rule and state["iterations"] == it + 1 and ("v" in state) == (SLOTS[rule] == 2)
        got_slots = [[a for pair in state[key] for a in pair] for key in ("m", "v")[:SLOTS[rule]]]
        worst = ref.worst_ratios([a for pair in eng.get_weights() for a in pair], got_slots)
        print("engine", name, "step", it + 1, "norm", n, "worst ratio to the bound: p, slots", worst)
        assert max(worst) <= 1.0, (name, it, worst)
    moved = max(float(m.max()) for m in ref.moved)
    assert 1e-7 < moved < 1e-2, moved


# ------------------------------------------------------------------------------------------ 4. one slot, one launch
def test_a_one_slot_rule_allocates_no_second_buffer_and_launches_one_update():
    import torch
    case = make_case(b=2, t=64, seed=3)
    for rule in ("sgd", "rmsprop", "adagrad"):
        eng = make_engine(case, "bf16", optimizer=rule)
        assert eng.adam_v is None and eng.adam_m is not None and eng.opt_slots == 1
    eng = make_engine(case, "bf16", optimizer="sgd", momentum=0.9)
    seen = []
    launch = eng._launch
    eng._launch = lambda tag, name, *args: (seen.append((name, tag, args)), launch(tag, name, *args))
    train(eng, case)
    train(eng, case)
    torch.cuda.synchronize()
    updates = [(name, tag, args) for name, tag, args in seen if tag.startswith("opt")]
    layers = len(eng._trainable_layers())
    assert layers <= 16 and len(updates) == 2 * -(-layers // 16)
    for name, tag, args in updates:
        assert name == "sl_optimizer_pack_layers" and tag == "opt:sgd:{}..{}".format(eng.all_plans[0].spec.name,
                                                                                      eng.all_plans[layers - 1].spec.name)
        assert args[3] is None  # no pointer to a second state buffer
    assert not any("adam" in tag or "adam" in name for name, tag, _ in seen)
    for ops in eng.cur.launch_lists.values():
        assert not any("adam" in (getattr(op, "tag", "") or "") for op in ops)
    assert make_engine(case, "bf16", optimizer="adadelta").adam_v is not None
    with pytest.raises(ValueError, match="optimizer"):
        make_engine(case, "bf16", optimizer="nadam")


# ------------------------------------------------------------------------------------------ 5. sharded optimizer, two ranks
def _shard_worker(rank, world, port, out_dir, shard, rule, hyper):
    import torch
    import torch.distributed as dist
    from speechless_amd.engine import Engine
    from speechless_amd.parallel import GradBucketReducer, shard_range
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)  # both ranks share cuda:0: gloo moves the bytes
    specs, weights, x, labels, lab_len, pred_len = _engine_case()
    eng = Engine(specs, 29, dtype="f32", device="cuda:0", **engine_kwargs(rule, hyper))
    eng.set_weights(weights)
    reducer = GradBucketReducer(eng.grads, eng.bucket_ranges(), shard_optimizer=shard)
    lo, hi = shard_range(x.shape[0], rank, world)
    seen = []
    launch = eng._launch
    eng._launch = lambda tag, name, *args: (seen.append(tag), launch(tag, name, *args))
    for _ in range(2):
        eng.train_step(x[lo:hi], labels[lo:hi], lab_len[lo:hi], pred_len[lo:hi], reducer)
    torch.cuda.synchronize()
    assert any(tag.startswith("opt_shard:{}:".format(rule)) for tag in seen) == shard
    state = eng.get_optimizer_state()  # (sharded: a collective that gathers exactly the slots that exist)
    assert ("v" in state) == (SLOTS[rule] == 2) and state["optimizer"] == rule
    arrays = [a for pair in eng.get_weights() for a in pair]
    for key in ("m", "v")[:SLOTS[rule]]:
        arrays += [a for pair in state[key] for a in pair]
    np.savez(os.path.join(out_dir, "rank{}_{}.npz".format(rank, int(shard))), *arrays)
    dist.destroy_process_group()


@pytest.mark.parametrize("name", ["sgd", "adadelta"])
def test_two_ranks_with_and_without_the_sharded_optimizer_agree_bit_for_bit(tmp_path, name):
    """SGD with momentum (one slot) and Adadelta (two): weights and gathered optimizer state after two steps byte-identical
    with and without shard_optimizer=True, and equal on both ranks"""
    import torch.multiprocessing as mp
    rule, hyper = CASES[name]
    hyper = dict(hyper, lr=1e-3 if rule == "sgd" else 1.0)
    for shard in (False, True):
        mp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path), shard, rule, hyper), nprocs=2, join=True)
    files = {(rank, shard): np.load(str(tmp_path / "rank{}_{}.npz".format(rank, shard))) for rank in (0, 1) for shard in (0, 1)}
    base = files[(0, 0)]
    specs, weights = _engine_case()[:2]
    assert len(base.files) == 2 * len(specs) * (1 + SLOTS[rule])
    for key, other in files.items():
        for arr in base.files:
            assert base[arr].tobytes() == other[arr].tobytes(), (key, arr)
    assert not np.array_equal(base["arr_0"], weights[0][0]) and base["arr_{}".format(2 * len(specs))].any()


# ------------------------------------------------------------------------------------------ 6. Wav2Letter
def _batch():
    from speechless_amd.net import LabeledSpectrogram
    rng = np.random.RandomState(3)
    words = ["she", "was", "abc", "a", "zoo"]
    return [LabeledSpectrogram(id="u{}".format(i), label=" ".join(rng.choice(words, size=rng.randint(1, 3))),
                               spectrogram=rng.randn(int(rng.randint(60, 78)), 128)) for i in range(3)]


SMALL = dict(main_filter_count=20, out_filter_count=40, inner_count=1)  # the toy stack of the other GPU tests


@pytest.mark.parametrize("cls,kw", [("SGD", dict(lr=1e-3, momentum=0.9, nesterov=True)), ("RMSprop", dict(lr=1e-4)),
                                    ("Adagrad", dict(lr=1e-3, decay=0.5)), ("Adadelta", {}), ("Adamax", dict(clipvalue=1e-3))])
def test_wav2letter_resumes_from_a_saved_optimizer_state_bit_for_bit(tmp_path, cls, kw):
    import torch
    from speechless_amd import Wav2Letter, english_frequent_characters, net as net_module

    def new(**more):
        return Wav2Letter(128, english_frequent_characters, optimizer=getattr(net_module, cls)(**kw), compute_dtype="bf16",
                          layer_sizes=SMALL, seed=5, **more)

    batch = _batch()
    straight = new()
    assert straight.engine.optimizer == cls.lower()
    for _ in range(2):
        straight.train_on_batch(batch)
    straight.predictive_net.save_weights(tmp_path / straight.model_file_name(2))
    straight.save_optimizer_state(tmp_path, 2)
    straight.train_on_batch(batch)
    resumed = new(load_model_from_directory=tmp_path, load_epoch=2, load_optimizer_state=True)
    assert resumed.engine.adam_iterations == 2
    resumed.train_on_batch(batch)
    torch.cuda.synchronize()
    for a, b in zip(engine_state(straight.engine), engine_state(resumed.engine)):
        assert torch.equal(a, b)
    cold = new(load_model_from_directory=tmp_path, load_epoch=2)  # without the state the third step is another one
    cold.train_on_batch(batch)
    assert not torch.equal(cold.engine.params, straight.engine.params)
    data = np.load(str(tmp_path / straight.optimizer_state_file_name(2)))
    assert str(data["optimizer"]) == cls.lower() and ("striding_conv/kernel/v" in data.files) == (cls in ("Adadelta", "Adamax"))


def test_wav2letter_asg_with_sgd_moves_the_tables_as_the_restatement_does():
    import torch
    from speechless_amd import SGD, Wav2Letter, english_frequent_characters
    net = Wav2Letter(128, english_frequent_characters, optimizer=SGD(0.01, momentum=0.9), criterion="asg", layer_sizes=SMALL,
                     seed=4, compute_dtype="bf16")
    eng = net.engine
    assert eng.asg_adam_v is None and sorted(eng.get_asg_state()) == ["init", "init_m", "trans", "trans_m"]
    batch = _batch()
    ref = Restated("sgd", [eng.asg_params.cpu().numpy()], dict(lr=0.01, momentum=0.9))
    for _ in range(2):
        net.train_on_batch(batch)
        torch.cuda.synchronize()
        ref.step([eng.asg_grads.cpu().numpy().astype(np.float64)])
    worst = ref.worst_ratios([eng.asg_params.cpu().numpy()], [[eng.asg_adam_m.cpu().numpy()]])
    print("asg tables under SGD: worst ratio to the bound: p, m", worst)
    assert max(worst) <= 1.0
    assert np.abs(eng.asg_trans.cpu().numpy()).max() > 1e-5 and np.abs(eng.asg_init.cpu().numpy()).max() > 1e-5


# ------------------------------------------------------------------------------------------ 7. Adam unchanged
def test_an_explicit_adam_engine_is_the_default_engine():
    import torch
    case = make_case(b=2, t=64, seed=3)
    runs = []
    for kw in ({}, dict(optimizer="adam")):
        eng = make_engine(case, "bf16", **kw)
        seen = []
        launch = eng._launch
        eng._launch = lambda tag, name, *args, seen=seen, launch=launch: (seen.append((name, tag)), launch(tag, name, *args))
        train(eng, case)
        train(eng, case)
        torch.cuda.synchronize()
        runs.append((eng, seen))
    (a, tags_a), (b, tags_b) = runs
    assert tags_a == tags_b and tags_a[-1][0] == "sl_adam_pack_layers" and tags_a[-1][1].startswith("adam:")
    for x, y in zip(engine_state(a), engine_state(b)):
        assert torch.equal(x, y)
    assert a.adam_v is not None and "optimizer" not in a.get_optimizer_state()
