"""The fused update + operand repack launch (sl_*_pack_layers) at the shapes where its tiling can go wrong: cut tiles in both
directions, tables whose tiles cross layer boundaries, SL_ADAM_MAX_LAYERS layers, a layer without w_dgrad, offsets that are
multiples of 4 and not of 64.  The reference of p and the state slots is the flat launch (sl_adam_step / sl_optimizer_step,
clipped or not) on the same values, bit for bit; the reference of w_fwd and w_dgrad is a host repack of the resulting p
(transpose, tap flip, torch round-to-nearest-even narrow types, [hi | hi | lo] planes); every buffer sits in a sentinel pattern
that must come back unchanged outside the layers' blocks."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEAD, GAP = 20, 12  # floats in front of the first layer block / between two blocks: offsets % 4 == 0, never % 64 == 0
OPERAND_GAP = 24    # elements between two layers' operand copies (16-byte aligned for every element size)
ADAM_HOW = (3, 1e-3, 0.9, 0.999, 1e-8)  # step, lr, beta1, beta2, eps
W_SCALE = 64.0
FORMATS = {"bf16": (1, "bfloat16"), "f32": (1, "float32"), "bf16x3": (3, "bfloat16"), "f16x3": (3, "float16")}


def block_numel(k, cin, cout):
    return k * cin * cout + cout


def layout(shapes):
    """offsets of the layer blocks in the flat fp32 buffers, and the buffers' length"""
    offsets, at = [], LEAD
    for shape in shapes:
        offsets.append(at)
        at += block_numel(*shape) + GAP
        at += 4 if at % 64 == 0 else 0
    assert all(o % 4 == 0 and o % 64 != 0 for o in offsets)
    return offsets, at + (-at) % 4


def narrow_bits(x, fmt):
    """x (fp32 numpy) in the operand format, as the integers of its bits; planes: (hi, lo)"""
    import torch
    planes, name = FORMATS[fmt]
    x = x.reshape(-1).copy().reshape(x.shape)  # (a flipped axis of length 1 keeps its negative stride through ascontiguousarray)
    t = torch.from_numpy(x)
    if name == "float32":
        return (x.view(np.int32),)
    dt = getattr(torch, name)
    if fmt == "f16x3":
        t = t * W_SCALE  # (a power of two: exact)
    hi = t.to(dt)
    if planes == 1:
        return (hi.view(torch.int16).numpy(),)
    lo = (t - hi.float()).to(dt)
    return hi.view(torch.int16).numpy(), lo.view(torch.int16).numpy()


def host_repack(w, fmt):
    """w [k][cin][cout] (fp32) -> the bits of w_fwd [cout][k][planes * cin] and w_dgrad [cin][k - 1 - tap][planes * cout]"""
    out = []
    for view in (w.transpose(2, 0, 1), w[::-1].transpose(1, 0, 2)):
        bits = narrow_bits(np.ascontiguousarray(view), fmt)
        out.append(bits[0] if len(bits) == 1 else np.concatenate([bits[0], bits[0], bits[1]], axis=-1))
    return out


class Case:
    """random p, g and state in flat buffers, and the operand buffers, both with sentinels around the layers' blocks"""

    def __init__(self, shapes, fmt, seed, null_dgrad=()):
        import torch
        from speechless_amd import _lib
        self.shapes, self.fmt = shapes, fmt
        self.planes, name = FORMATS[fmt]
        self.offsets, self.n = layout(shapes)
        rng = np.random.RandomState(seed)
        self.host = {"p": (rng.randn(self.n) * 0.05).astype(np.float32), "g": (rng.randn(self.n) * 0.5).astype(np.float32),
                     "s0": rng.randn(self.n).astype(np.float32), "s1": np.abs(rng.randn(self.n)).astype(np.float32)}
        self.int_type = np.int32 if name == "float32" else np.int16
        self.sentinel = 0x5A5A5A5A if name == "float32" else 0x5A5A
        self.torch_int = torch.int32 if name == "float32" else torch.int16
        self.fwd_at, self.dgrad_at, at_f, at_d = [], [], OPERAND_GAP, OPERAND_GAP
        for i, (k, cin, cout) in enumerate(shapes):
            self.fwd_at.append(at_f)
            at_f += self.planes * k * cin * cout + OPERAND_GAP
            self.dgrad_at.append(None if i in null_dgrad else at_d)
            if i not in null_dgrad:
                at_d += self.planes * k * cin * cout + OPERAND_GAP
        self.fwd_len, self.dgrad_len = at_f, at_d
        self.lib_module = _lib

    def device_state(self, nonnegative_s0):
        import torch
        host = dict(self.host)
        if nonnegative_s0:
            host["s0"] = np.abs(host["s0"])
        return {name: torch.tensor(a, device="cuda:0") for name, a in host.items()}

    def operand_buffers(self):
        import torch
        return [torch.full((n,), self.sentinel, dtype=self.torch_int, device="cuda:0") for n in (self.fwd_len, self.dgrad_len)]

    def table(self, wf, wd):
        size = wf.element_size()
        table = (self.lib_module.AdamLayer * len(self.shapes))()
        for entry, shape, off, fa, da in zip(table, self.shapes, self.offsets, self.fwd_at, self.dgrad_at):
            entry.offset, entry.w_fwd = off, wf.data_ptr() + fa * size
            entry.w_dgrad = None if da is None else wd.data_ptr() + da * size
            entry.k, entry.cin_pad, entry.cout_pad = shape
        return table

    def expected_operands(self, p):
        """both operand buffers as the host repack of p (numpy, the whole flat buffer) leaves them"""
        fwd = np.full(self.fwd_len, self.sentinel, dtype=self.int_type)
        dgrad = np.full(self.dgrad_len, self.sentinel, dtype=self.int_type)
        for (k, cin, cout), off, fa, da in zip(self.shapes, self.offsets, self.fwd_at, self.dgrad_at):
            f, d = host_repack(p[off:off + k * cin * cout].reshape(k, cin, cout), self.fmt)
            fwd[fa:fa + f.size] = f.reshape(-1)
            if da is not None:
                dgrad[da:da + d.size] = d.reshape(-1)
        return fwd, dgrad


def make_rule(_lib, rule):
    return _lib.OptRule(rule=_lib.OPT_RULES[rule], lr=1e-3, momentum=0.9, nesterov=1, rho=0.95, beta1=0.9, beta2=0.999, eps=1e-7)


def run_fused_and_flat(hip_lib, case, rule="adam", clip=False):
    """the fused launch over the whole table and the flat launch over every layer block, on equal values"""
    import torch
    _lib = case.lib_module
    st = torch.cuda.current_stream().cuda_stream
    two = _lib.OPT_SLOTS[rule] == 2
    nonneg = rule in ("rmsprop", "adagrad", "adadelta")
    scale = torch.tensor([0.5], dtype=torch.float32, device="cuda:0")
    how_clip = (scale.data_ptr(), 0.25) if clip else (None, 0.0)
    opt_rule = make_rule(_lib, rule)

    def ptrs(t, shift=0):
        return tuple(t[name].data_ptr() + 4 * shift if (name != "s1" or two) else None for name in ("p", "g", "s0", "s1"))

    fused = case.device_state(nonneg)
    wf, wd = case.operand_buffers()
    table, n_layers = case.table(wf, wd), len(case.shapes)
    if rule == "adam":
        tail = how_clip if clip else ()
        suffix = "_clipped" if clip else ""
        if case.fmt in ("bf16", "f32"):
            dtype = _lib.SL_BF16 if case.fmt == "bf16" else _lib.SL_F32
            hip_lib.call("sl_adam_pack_layers" + suffix, *ptrs(fused), table, n_layers, dtype, *ADAM_HOW, *tail, st)
        elif case.fmt == "bf16x3":
            hip_lib.call("sl_split3_adam_pack_layers" + suffix, *ptrs(fused), table, n_layers, *ADAM_HOW, *tail, st)
        else:
            hip_lib.call("sl_splitf16_adam_pack_layers" + suffix, *ptrs(fused), table, n_layers, *ADAM_HOW, W_SCALE, *tail, st)
    elif case.fmt in ("bf16", "f32"):
        dtype = _lib.SL_BF16 if case.fmt == "bf16" else _lib.SL_F32
        hip_lib.call("sl_optimizer_pack_layers", *ptrs(fused), table, n_layers, dtype, ctypes.byref(opt_rule), *how_clip, st)
    elif case.fmt == "bf16x3":
        hip_lib.call("sl_split3_optimizer_pack_layers", *ptrs(fused), table, n_layers, ctypes.byref(opt_rule), *how_clip, st)
    else:
        hip_lib.call("sl_splitf16_optimizer_pack_layers", *ptrs(fused), table, n_layers, ctypes.byref(opt_rule), W_SCALE,
                     *how_clip, st)
    flat = case.device_state(nonneg)
    for shape, off in zip(case.shapes, case.offsets):
        n = block_numel(*shape)
        if rule == "adam" and clip:
            hip_lib.call("sl_adam_step_clipped", *ptrs(flat, off), n, *ADAM_HOW, *how_clip, st)
        elif rule == "adam":
            hip_lib.call("sl_adam_step", *ptrs(flat, off), n, *ADAM_HOW, st)
        else:
            hip_lib.call("sl_optimizer_step", *ptrs(flat, off), n, ctypes.byref(opt_rule), *how_clip, st)
    torch.cuda.synchronize()
    return fused, flat, wf, wd


def check(hip_lib, case, rule="adam", clip=False):
    import torch
    fused, flat, wf, wd = run_fused_and_flat(hip_lib, case, rule, clip)
    where = (case.shapes, case.fmt, rule, clip)
    for name in ("p", "s0", "s1", "g"):
        # (the flat launch touches the layers' blocks only: equality of the whole buffers is also the sentinel check)
        assert torch.equal(fused[name].view(torch.int32), flat[name].view(torch.int32)), (name,) + where
    assert np.array_equal(fused["g"].cpu().numpy().view(np.int32), case.host["g"].view(np.int32)), where
    p = fused["p"].cpu().numpy()
    assert not np.array_equal(p, case.host["p"]), where  # (the update did run)
    lo, hi = case.offsets[0], case.offsets[-1] + block_numel(*case.shapes[-1])
    outside = np.ones(case.n, dtype=bool)
    for shape, off in zip(case.shapes, case.offsets):
        outside[off:off + block_numel(*shape)] = False
    assert lo == LEAD and hi <= case.n and np.array_equal(p[outside].view(np.int32), case.host["p"][outside].view(np.int32))
    want_fwd, want_dgrad = case.expected_operands(p)
    assert np.array_equal(wf.cpu().numpy(), want_fwd), ("w_fwd",) + where
    assert np.array_equal(wd.cpu().numpy(), want_dgrad), ("w_dgrad",) + where


@pytest.mark.parametrize("cout", [64, 128, 192, 320])
@pytest.mark.parametrize("cin", [32, 64, 96])
def test_every_cut_of_the_tile_at_one_two_and_seven_taps(hip_lib, cin, cout):
    """cin_pad in {32, 64, 96} x cout_pad in {64, 128, 192, 320}, k in {1, 2, 7} as the three layers of one table"""
    check(hip_lib, Case([(1, cin, cout), (2, cin, cout), (7, cin, cout)], "bf16", seed=cin + cout))


def test_a_table_of_three_different_layers_one_of_them_without_w_dgrad(hip_lib):
    check(hip_lib, Case([(7, 96, 320), (1, 32, 64), (2, 64, 192)], "bf16", seed=5, null_dgrad=(1,)))
    check(hip_lib, Case([(2, 64, 128), (7, 32, 192), (1, 96, 64)], "bf16x3", seed=6, null_dgrad=(0,)))


def test_the_longest_table_of_the_smallest_layers(hip_lib):
    """SL_ADAM_MAX_LAYERS (16) layers of 1 x 32 x 64: every tile is cut and every second tile is a bias tile"""
    check(hip_lib, Case([(1, 32, 64)] * 16, "bf16", seed=7))
    from speechless_amd import _lib
    case = Case([(1, 32, 64)] * 17, "bf16", seed=7)
    wf, wd = case.operand_buffers()
    t = case.device_state(False)
    args = [t[name].data_ptr() for name in ("p", "g", "s0", "s1")]
    assert hip_lib.raw("sl_adam_pack_layers")(*args, case.table(wf, wd), 17, _lib.SL_BF16, *ADAM_HOW, None) != 0


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("rule", ["adam", "sgd", "rmsprop", "adagrad", "adadelta", "adamax"])
def test_every_rule_clipped_and_not(hip_lib, rule, clip):
    check(hip_lib, Case([(2, 96, 192)], "bf16", seed=11), rule, clip)


@pytest.mark.parametrize("shapes", [[(2, 96, 192)], [(7, 64, 320), (1, 32, 128)]])
@pytest.mark.parametrize("fmt", ["bf16", "f32", "bf16x3", "f16x3"])
def test_every_operand_format(hip_lib, fmt, shapes):
    check(hip_lib, Case(shapes, fmt, seed=13))
    if fmt in ("bf16x3", "f16x3"):  # another rule and clipping through the plane formats' own entry points
        check(hip_lib, Case(shapes, fmt, seed=14), "rmsprop", True)


@pytest.mark.parametrize("fmt", ["bf16", "f32"])
def test_pack_only_rewrites_the_operands_and_nothing_else(hip_lib, fmt):
    import torch
    from speechless_amd import _lib
    case = Case([(7, 96, 320), (1, 32, 64), (2, 64, 192)], fmt, seed=17, null_dgrad=(2,))
    p = torch.tensor(case.host["p"], device="cuda:0")
    wf, wd = case.operand_buffers()
    hip_lib.call("sl_pack_layers", p.data_ptr(), case.table(wf, wd), 3, _lib.SL_BF16 if fmt == "bf16" else _lib.SL_F32,
                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy().view(np.int32), case.host["p"].view(np.int32))
    want_fwd, want_dgrad = case.expected_operands(case.host["p"])
    assert np.array_equal(wf.cpu().numpy(), want_fwd) and np.array_equal(wd.cpu().numpy(), want_dgrad)
