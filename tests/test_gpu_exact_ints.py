"""The bf16-storing launches held to ZERO tolerance: operands from tests/exact_ints.py make every partial sum an integer below
2^24 and every stored value an integer of at most 8 significant bits, so accumulation order, split-K, tile shape and the output
rounding cannot matter and every element must equal the int64 reference (assert_exact).  Every test also checks the layout:
halo rows and rows beyond t_out untouched / zero, padded channels zero, the ones channel 1 on valid frames."""
import ctypes
import functools

import numpy as np
import pytest

import exact_ints as xi
from test_gpu_parity import NT_CONFIGS, _nt_cfg, make_case, make_engine

pytestmark = pytest.mark.gpu

REAL, PADDED, ONES = xi.NT_REAL, xi.NT_PADDED, xi.NT_PADDED - 1


def _np(t):
    return t.float().cpu().numpy()


# ------------------------------------------------------------------------------------------ a. sl_conv1d_nt, bf16 out
def _nt_tile_rows():
    """row-tile heights of NT_CONFIGS: wm waves of 16 * it rows (it = 5: the it = 4 tile; 32x32 MFMA: 64 rows per wave)"""
    return sorted({wm * (64 if m32 else 16 * (4 if it in (0, 5) else it)) for (wm, _, _, _, it, m32, _, _) in NT_CONFIGS})


@functools.lru_cache(maxsize=None)
def _nt_reference(family, taps, t_out, batch):
    # impulses on both sides of every multiple of 16 rows: that is every edge of every tile height of the table
    assert all(h % 16 == 0 for h in _nt_tile_rows())
    case = xi.nt_case(family, taps, t_out, batch, seed=taps, tiles=(16,))
    want = xi.nt_expected(case)
    for y in want.values():
        assert np.abs(y).max() <= xi.BF16_MAX_EXACT
    return case, want


class _NtLaunch:
    """one sl_conv1d_nt geometry as test_every_nt_tile_configuration_against_float64 lays it out, with bf16 outputs"""
    HALO = 48

    def __init__(self, hip_lib, case):
        import torch
        from speechless_amd import _lib
        self.lib, self._lib, self.torch = hip_lib, _lib, torch
        batch, t_out, cin = case["x"].shape
        taps, _, cout = case["w"].shape
        self.batch, self.t_out, self.cout = batch, t_out, cout
        halo = self.HALO
        self.rows = rows = halo + ((t_out + 255) // 256) * 256 + halo
        self.dev = dev = torch.device("cuda:0")
        self.st = torch.cuda.current_stream().cuda_stream
        pad_l = (taps - 1) // 2
        x = np.zeros((batch, rows, cin), dtype=np.float32)
        x[:, halo:halo + t_out] = case["x"]
        mask = np.zeros((batch, rows, cout), dtype=np.float32)
        mask[:, halo:halo + t_out] = case["mask"]
        self.x = torch.tensor(x).to(torch.bfloat16).to(dev)
        self.mask = torch.tensor(mask).to(torch.bfloat16).to(dev)
        self.bias = torch.tensor(case["bias"].astype(np.float32)).to(dev)
        self.w = self.pack(case["w"])
        g = self.geom = _lib.ConvGeom()
        g.batch, g.t_out, g.taps, g.cin, g.cout = batch, t_out, taps, cin, cout
        g.x_row0, g.x_row_stride, g.x_batch_stride = halo - pad_l, cin, rows * cin
        g.y_row0, g.y_row_stride, g.y_batch_stride = halo, cout, rows * cout

    def pack(self, w):
        torch, _lib = self.torch, self._lib
        taps, cin, cout = w.shape
        master = torch.tensor(w.astype(np.float32)).to(self.dev)
        packed = torch.zeros((cout, taps, cin), dtype=torch.bfloat16, device=self.dev)
        self.lib.call("sl_pack_weights", master.data_ptr(), packed.data_ptr(), None, taps, cin, cout, _lib.SL_BF16, self.st)
        return packed

    def run(self, epilogue, cfg, w=None):
        """(rc, whole output tensor as float numpy, rows outside [0, t_out) pre-filled with 7)"""
        torch, _lib = self.torch, self._lib
        epi = {"none": _lib.EPI_NONE, "bias_relu": _lib.EPI_BIAS_RELU, "relu_mask": _lib.EPI_RELU_MASK}[epilogue]
        need = self.lib.raw("sl_conv1d_nt_workspace_bytes")(ctypes.byref(self.geom), _lib.SL_BF16, cfg)
        ws = torch.empty((max(int(need), 16),), dtype=torch.uint8, device=self.dev)
        y = torch.full((self.batch, self.rows, self.cout), 7.0, dtype=torch.bfloat16, device=self.dev)
        rc = self.lib.raw("sl_conv1d_nt")(self.x.data_ptr(), (self.w if w is None else w).data_ptr(),
                                          self.bias.data_ptr() if epilogue == "bias_relu" else None,
                                          self.mask.data_ptr() if epilogue == "relu_mask" else None, y.data_ptr(),
                                          ctypes.byref(self.geom), epi, _lib.SL_BF16, 0, cfg, ws.data_ptr(), ws.numel(), self.st)
        if rc != 0:
            return rc, None
        torch.cuda.synchronize()
        return 0, _np(y)

    def check_layout(self, got, epilogue, where):
        halo, t_out = self.HALO, self.t_out
        assert (got[:, :halo] == 7.0).all() and (got[:, halo + t_out:] == 7.0).all(), (where, "rows outside [0, t_out) written")
        valid = got[:, halo:halo + t_out]
        assert not valid[:, :, REAL:ONES].any(), (where, "padded channels")
        assert (valid[:, :, ONES] == (1 if epilogue == "bias_relu" else 0)).all(), (where, "ones channel")


@pytest.mark.parametrize("family", ["A", "B"])
@pytest.mark.parametrize("epilogue", ["bias_relu", "relu_mask", "none"])
@pytest.mark.parametrize("taps,t_out,batch", [(7, 300, 3), (32, 140, 2), (5, 129, 5)])
def test_every_nt_tile_configuration_with_bf16_output_is_exact(hip_lib, taps, t_out, batch, epilogue, family):
    """sl_conv1d_nt storing bf16 with EVERY configuration of NT_CONFIGS, the three epilogues the engine launches, 256 channels
    in the engine's layout (250 real, ones channel last), dense {0, 1} input with sparse weights (A) and impulses on both
    sides of every tile edge with dense weights (B): equal to the int64 reference in every element"""
    case, want = _nt_reference(family, taps, t_out, batch)
    nt = _NtLaunch(hip_lib, case)
    halo = nt.HALO
    ran = 0
    for (wm, wn, stg, ks, it, m32, gml, slab) in NT_CONFIGS:
        where = "nt {} {} cfg {}".format(family, epilogue, (wm, wn, stg, ks, it, m32, gml, slab))
        rc, got = nt.run(epilogue, _nt_cfg(wm, wn, stg, ks, it, m32, gml, slab))
        if rc != 0:  # a configuration the geometry rules out: must say so cleanly
            assert rc == -1 and "invalid tile configuration" in hip_lib.last_error(), (where, rc, hip_lib.last_error())
            continue
        xi.assert_exact(got[:, halo:halo + t_out], want[epilogue], where)
        nt.check_layout(got, epilogue, where)
        ran += 1
    assert ran >= len(NT_CONFIGS) - 8
    print("sl_conv1d_nt bf16-out {} {} taps {} t_out {} batch {}: {} of {} configurations ran".format(
        family, epilogue, taps, t_out, batch, ran, len(NT_CONFIGS)))


# ------------------------------------------------------------------------------------------ f. a planted difference
def test_a_one_tap_weight_difference_is_localised(hip_lib):
    """one NT forward whose weights differ from the reference's by 1 in ONE (tap, cin, cout) entry: the mismatches are exactly
    column cout on exactly the frames whose tap-shifted input at cin is non-zero -- the harness localises a one-tap error"""
    taps, t_out, batch = 7, 300, 3
    case, want = _nt_reference("A", taps, t_out, batch)
    nt = _NtLaunch(hip_lib, case)
    tap, cin, cout = 5, 123, 77
    w = case["w"].copy()
    w[tap, cin, cout] += 1
    rc, got = nt.run("none", 0, nt.pack(w))
    assert rc == 0, hip_lib.last_error()
    got = got[:, nt.HALO:nt.HALO + t_out]
    pad_l = (taps - 1) // 2
    shifted = np.zeros((batch, t_out), dtype=np.int64)  # x[b, t + tap - pad_l, cin]
    lo, hi = max(0, pad_l - tap), min(t_out, t_out + pad_l - tap)
    shifted[:, lo:hi] = case["x"][:, lo + tap - pad_l: hi + tap - pad_l, cin]
    expect = np.zeros(got.shape, dtype=bool)
    expect[:, :, cout] = shifted != 0
    assert expect.sum() > 100
    assert np.array_equal(got != want["none"], expect)
    with pytest.raises(xi.NotExact) as err:
        xi.assert_exact(got, want["none"], "planted")
    assert "{} of".format(int(expect.sum())) in str(err.value) and "by c // 64: {}: {}".format(cout // 64, int(expect.sum())) in str(err.value)
    xi.assert_exact(got - expect * shifted[:, :, None], want["none"], "planted difference removed")


# ------------------------------------------------------------------------------------------ engine-level helpers
@pytest.fixture(scope="module")
def bf16_engine():
    case = make_case(b=3, t=150, seed=30)
    return make_engine(case, "bf16")


def _set_layer(eng, i, w, b=None):
    """integer weights (and real-channel biases) of layer i into the fp32 masters; the ones channel's bias stays 1"""
    import torch
    p = eng.plans[i]
    wv, bv = eng.layer_param_views(eng.params, p)
    wv.zero_()
    wv[:, :w.shape[1], :w.shape[2]] = torch.tensor(w.astype(np.float32)).to(eng.device)
    bv[:p.spec.cout] = 0 if b is None else torch.tensor(b.astype(np.float32)).to(eng.device)
    eng._packed_dirty = True


def _store(eng, tensor, t_out, values, ones):
    """values (B, t_out, C) into the halo'd layout of an activation / gradient buffer, everything else zero"""
    import torch
    from speechless_amd.engine import HALO
    full = torch.zeros_like(tensor)
    full[:, HALO:HALO + t_out, :values.shape[2]] = torch.tensor(values.astype(np.float32)).to(eng.torch_dtype)
    if ones:
        full[:, HALO:HALO + t_out, -1] = 1  # the ones channel a forward pass would have put there
    tensor.copy_(full)


def _check_stored(tensor, t_out, want, ones, where):
    """a stored activation / gradient: the real channels equal `want` in every element, halo rows and rows beyond t_out are
    zero, padded channels are zero, the ones channel (activations) is 1 on valid frames"""
    from speechless_amd.engine import HALO
    raw = _np(tensor)
    c = want.shape[2]
    xi.assert_exact(raw[:, HALO:HALO + t_out, :c], want, where)
    assert not raw[:, :HALO].any() and not raw[:, HALO + t_out:].any(), (where, "halo rows / rows beyond t_out")
    last = raw.shape[2] - 1 if ones else raw.shape[2]
    assert not raw[:, HALO:HALO + t_out, c:last].any(), (where, "padded channels")
    if ones:
        assert (raw[:, HALO:HALO + t_out, -1] == 1).all(), (where, "ones channel")


# ------------------------------------------------------------------------------------------ b. sl_conv1d_chain
CHAIN_LENGTHS = [47, 48, 49, 63, 64, 65, 77, 95, 96, 97, 128, 129, 300]
CHAIN_LAYERS = list(range(1, 8))
CHAIN_SKIPPED = set()
CHAIN_DENSE_AT = 3  # family B: three shifting layers in front of the dense one and three behind it


@functools.lru_cache(maxsize=None)
def _chain_reference(t_out):
    out = {}
    x, weights = xi.family_a_stack(seed=t_out, batch=3, t=t_out)
    layers = xi.run_stack(x, weights)
    out["A fwd"] = (x, weights, [y for _, y in layers])
    g_top, wts, masks = xi.family_a_backward_run(t_out, x, layers)
    out["A bwd"] = (g_top, wts, masks, xi.run_stack_backward(g_top, wts, masks))
    x, weights = xi.family_b_stack(seed=t_out, batch=3, t_out=t_out, dense_at=CHAIN_DENSE_AT)
    out["B fwd"] = (x, weights, [y for _, y in xi.run_stack(x, weights)])
    g_top, wts, masks = xi.family_b_backward_run(t_out, 3, t_out, CHAIN_DENSE_AT)
    out["B bwd"] = (g_top, wts, masks, xi.run_stack_backward(g_top, wts, masks))
    for key, case in out.items():
        assert max(int(np.abs(v).max()) for v in case[-1]) <= xi.BF16_MAX_EXACT, key
    return out


@pytest.mark.parametrize("rows", [48, 64])
@pytest.mark.parametrize("t_out", CHAIN_LENGTHS)
def test_fused_inner_layers_are_exact_at_every_layer(hip_lib, bf16_engine, t_out, rows):
    """sl_conv1d_chain over the seven inner layers (250 -> 250, 7 taps, batch 3) with 48- and 64-frame tiles forced, forward
    (BIAS_RELU) and input gradient (RELU_MASK), lengths on both sides of every tile edge: EVERY layer's stored activation /
    gradient equals the int64 reference.  Family A is the whole dense stack; family B has impulses on both sides of every 48-
    and 64-row tile edge and at both utterance ends, shifted through the recomputed halo rows of three layers on either side
    of one dense layer, so a wrong halo row changes an output."""
    import torch
    from speechless_amd import _lib
    eng = bf16_engine
    buf = eng.load_input(np.zeros((3, 2 * t_out, eng.specs[0].cin), dtype=np.float32))
    buf.ensure_backward(eng)
    assert buf.t_out == t_out
    st = torch.cuda.current_stream().cuda_stream
    n = len(CHAIN_LAYERS)
    top = CHAIN_LAYERS[-1]
    fwd_geom, dgrad_geom = buf.fwd_geom[CHAIN_LAYERS[0]], buf.dgrad_geom[top]
    supported = all(hip_lib.raw("sl_conv1d_chain_supported")(ctypes.byref(g), n, _lib.SL_BF16) for g in (fwd_geom, dgrad_geom))
    if not supported:
        CHAIN_SKIPPED.add(t_out)
        assert t_out not in (77, 300) and len(CHAIN_SKIPPED) <= 3, sorted(CHAIN_SKIPPED)
        pytest.skip("sl_conv1d_chain_supported returns 0 for t_out = {}".format(t_out))
    ref = _chain_reference(t_out)
    try:
        hip_lib.call("sl_conv1d_chain_select", rows)
        assert hip_lib.raw("sl_conv1d_chain_plan")(ctypes.byref(fwd_geom), n, _lib.SL_BF16) == rows
        for family in ("A", "B"):
            # ---- forward: x into the activation in front of the run
            x, weights, ys_ref = ref[family + " fwd"]
            for i, (w, b) in zip(CHAIN_LAYERS, weights):
                _set_layer(eng, i, w, b)
            eng.repack_weights()
            _store(eng, buf.y[0], t_out, x, ones=True)
            for i in CHAIN_LAYERS:
                buf.y[i].fill_(3)  # whatever the launch must write is wrong until it does; the rest is cleared below
                buf.y[i][:, :_halo()].zero_()
                buf.y[i][:, _halo() + t_out:].zero_()
            ys, ws, biases = eng._chain_table("fwd", CHAIN_LAYERS, buf)
            hip_lib.call("sl_conv1d_chain", buf.y[0].data_ptr(), ys, ws, biases, None, ctypes.byref(fwd_geom), n,
                         _lib.EPI_BIAS_RELU, _lib.SL_BF16, st)
            torch.cuda.synchronize()
            for i, want in zip(CHAIN_LAYERS, ys_ref):
                _check_stored(buf.y[i], t_out, want, True, "chain {} fwd rows {} t_out {} layer {}".format(family, rows, t_out, i))
            # ---- input gradients from the top of the run: masks into the activations, the gradient into g[top]
            g_top, wts, masks, gs_ref = ref[family + " bwd"]
            for i, (w, _) in zip(CHAIN_LAYERS, wts):
                _set_layer(eng, i, w)
            eng.repack_weights()
            dlayers = CHAIN_LAYERS[::-1]
            for i, m in zip(CHAIN_LAYERS, masks):
                _store(eng, buf.y[i - 1], t_out, m, ones=True)
            _store(eng, buf.g[top], t_out, g_top, ones=False)
            for i in dlayers:
                buf.g[i - 1].fill_(3)
                buf.g[i - 1][:, :_halo()].zero_()
                buf.g[i - 1][:, _halo() + t_out:].zero_()
            gs, wd, mk = eng._chain_table("dgrad", dlayers, buf)
            hip_lib.call("sl_conv1d_chain", buf.g[top].data_ptr(), gs, wd, None, mk, ctypes.byref(dgrad_geom), n,
                         _lib.EPI_RELU_MASK, _lib.SL_BF16, st)
            torch.cuda.synchronize()
            for i, want in zip(dlayers, gs_ref):
                _check_stored(buf.g[i - 1], t_out, want, False,
                              "chain {} bwd rows {} t_out {} gradient in front of layer {}".format(family, rows, t_out, i))
    finally:
        hip_lib.call("sl_conv1d_chain_select", 0)


def _halo():
    from speechless_amd.engine import HALO
    return HALO


# ------------------------------------------------------------------------------------------ c. engine level
def test_engine_forward_is_exact_through_the_depth_with_and_without_the_fused_run_and_replayed():
    """Engine(dtype='bf16').forward on the whole-stack family-A case (stride-2 first layer with 48 taps in its pair view, the
    seven inner layers, the 2000-channel layers; P = N = 2 keeps every stored activation at most 255) with the launch choosers'
    own picks: every stored activation of layers 0-9 equals the int64 reference with use_chain on, replayed from the recorded
    launch list, and with use_chain off -- and the three runs are bit-identical.  (The softmax behind layer 10 is not exact.)"""
    import torch
    from speechless_amd.engine import Engine, wav2letter_layer_specs
    x, weights, strides = xi.engine_case()
    layers = xi.run_stack(x, weights, strides)
    t_out = layers[0][1].shape[1]
    eng = Engine(wav2letter_layer_specs(x.shape[2], weights[-1][1].shape[0]), weights[-1][1].shape[0], dtype="bf16")
    assert [(s.name, s.kernel_size, s.stride) for s in eng.specs] == [(n, k, s) for n, k, s, _, _ in xi.ENGINE_LAYERS]
    eng.set_weights([(w.astype(np.float32), b.astype(np.float32)) for w, b in weights])
    runs = {}
    for name, chain in (("chain", True), ("chain replayed", True), ("single launches", False)):
        eng.use_chain = chain
        if eng.cur is not None:
            for y in eng.cur.y:
                y.zero_()
        recorded = eng.cur is not None and len(eng.cur.launch_lists)
        eng.forward(x.astype(np.float32))
        torch.cuda.synchronize()
        buf = eng.cur
        assert buf.t_out == t_out
        if name == "chain replayed":
            assert recorded == 1 and len(buf.launch_lists) == 1  # this run replayed the list the first one recorded
        for i in range(10):
            _check_stored(buf.y[i], t_out, layers[i][1], eng._has_ones_output(eng.plans[i]), "engine forward ({}) layer {}".format(name, i))
        runs[name] = [y.clone() for y in buf.y]
    for name in ("chain replayed", "single launches"):
        for i, (a, b) in enumerate(zip(runs["chain"], runs[name])):
            assert torch.equal(a, b), (name, i)


# ------------------------------------------------------------------------------------------ d. backward pieces
@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("layer", [0, 1, 8, 9, 10])
def test_backward_kernels_of_one_layer_are_exact(dtype, layer):
    """sl_conv1d_wgrad, sl_conv1d_wgrad_multi (bf16, layers whose channel counts it takes: 0, 1, 8, 9), sl_bias_grad and the
    RELU_MASK input gradient of ONE layer, operands written into buf.y / buf.g as test_single_layer_kernels_with_exact_operands
    does: {0, 1} inputs, gradients in [-3, 3], weights with two +1 and two -1 per INPUT channel (the columns of the
    input-gradient launch, |dx| <= 12).  Sums of at most 3 * 75 products of magnitude <= 3: exact in fp32.  The bias gradient in
    the ones-channel row of dW, the sl_bias_grad result and the reference are all three identical."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(70 + layer)
    case = make_case(b=3, t=150, seed=30)
    eng = make_engine(case, dtype)
    buf = eng.load_input(case["x"])
    buf.ensure_backward(eng)
    p = eng.plans[layer]
    s = p.spec
    t_out = buf.t_out
    ones_in = layer > 0 and eng._has_ones_output(eng.plans[layer - 1])
    if layer == 0:
        x_in = xi.family_a_input(rng, (3, 150, s.cin))
        eng.load_input(x_in.astype(np.float32))
    else:
        x_in = xi.family_a_input(rng, (3, t_out, s.cin))
        _store(eng, buf.y[layer - 1], t_out, x_in, ones=ones_in)
    g = rng.randint(-3, 4, size=(3, t_out, s.cout)).astype(np.int64)
    _store(eng, buf.g[layer], t_out, g, ones=False)
    w = xi.family_a_weights(rng, s.kernel_size, s.cin, s.cout, by_input=True)
    _set_layer(eng, layer, w, xi.family_a_bias(rng, s.cout))
    eng.repack_weights()
    st = torch.cuda.current_stream().cuda_stream
    dw_ref = xi.reference_weight_gradient(x_in, g, s.kernel_size, s.stride)
    db_ref = xi.reference_bias_gradient(g)
    assert np.abs(dw_ref).max() < xi.FP32_BUDGET and np.abs(db_ref).max() < xi.FP32_BUDGET
    x_ptr = (buf.x0 if layer == 0 else buf.y[layer - 1]).data_ptr()
    dw_v, db_v = eng.layer_param_views(eng.grads, p)
    where = "{} layer {} ".format(dtype, layer)

    def check_dw(what):
        full = dw_v.cpu().numpy()
        xi.assert_exact(full[:, :s.cin, :s.cout], dw_ref, where + what)
        assert not full[:, :, s.cout:].any(), (where + what, "padded output lanes")
        if ones_in:  # the row of the input's ones channel: at the tap that reads the frame itself it IS the bias gradient
            assert not full[:, s.cin:p.cin_pad - 1, :].any(), (where + what, "padded input lanes")
            xi.assert_exact(full[p.pad_left, p.cin_pad - 1, :s.cout], db_ref, where + what + " ones-channel row")
        else:
            assert not full[:, s.cin:, :].any(), (where + what, "padded input lanes")

    eng.lib.call("sl_conv1d_wgrad", x_ptr, buf.g[layer].data_ptr(), dw_v.data_ptr(), ctypes.byref(buf.wgrad_geom[layer]),
                 eng.dtype_code, 0, buf.wgrad_ws.data_ptr(), buf.wgrad_ws.numel(), st)
    eng.lib.call("sl_bias_grad", buf.g[layer].data_ptr(), db_v.data_ptr(), ctypes.byref(buf.wgrad_geom[layer]),
                 eng.dtype_code, buf.bias_ws.data_ptr(), buf.bias_ws.numel(), st)
    torch.cuda.synchronize()
    check_dw("sl_conv1d_wgrad")
    db = db_v.cpu().numpy()
    xi.assert_exact(db[:s.cout], db_ref, where + "sl_bias_grad")
    assert not db[s.cout:].any(), (where, "sl_bias_grad padded lanes")
    if ones_in:
        xi.assert_exact(dw_v[p.pad_left, p.cin_pad - 1, :s.cout].cpu().numpy(), db[:s.cout], where + "ones-channel row against sl_bias_grad")
    if dtype == "bf16" and p.cin_view % 256 == 0 and p.cout_pad % 256 == 0:
        dw_v.fill_(5)
        table = eng._wgrad_multi_table(buf, [layer])
        eng.lib.call("sl_conv1d_wgrad_multi", table, 1, eng.dtype_code, buf.wgrad_multi_ws.data_ptr(),
                     buf.wgrad_multi_ws.numel(), st)
        torch.cuda.synchronize()
        check_dw("sl_conv1d_wgrad_multi")
    else:
        assert dtype == "f32" or layer == 10  # (bf16 only; output_conv's 128 padded graphemes are no 256-wide tile)
    if layer > 0:
        dx_ref = xi.reference_input_gradient(g, w, mask=x_in)
        assert np.abs(dx_ref).max() <= 12
        buf.g[layer - 1].fill_(3)
        buf.g[layer - 1][:, :_halo()].zero_()
        buf.g[layer - 1][:, _halo() + t_out:].zero_()
        eng.lib.call("sl_conv1d_nt", buf.g[layer].data_ptr(), eng.w_dgrad[layer].data_ptr(), None,
                     buf.y[layer - 1].data_ptr(), buf.g[layer - 1].data_ptr(), ctypes.byref(buf.dgrad_geom[layer]),
                     _lib.EPI_RELU_MASK, eng.dtype_code, 0, 0, buf.nt_ws.data_ptr(), buf.nt_ws.numel(), st)
        torch.cuda.synchronize()
        _check_stored(buf.g[layer - 1], t_out, dx_ref, False, where + "RELU_MASK input gradient")


# ------------------------------------------------------------------------------------------ e. plane paths
def _store_planes(eng, tensor, t_out, values, ones):
    """values (B, t_out, C) as they are STORED (engine scales applied) into a plane tensor: rows [hi | lo | hi] of the padded
    channel count each, hi = rn(v), lo = rn(v - hi); the ones channel is hi = 1, lo = 0"""
    import torch
    h = _halo()
    cp = tensor.shape[2] // 3
    c = values.shape[2]
    v = torch.tensor(np.asarray(values, dtype=np.float32)).to(eng.device)
    hi = v.to(eng.torch_dtype)
    lo = (v - hi.float()).to(eng.torch_dtype)
    assert torch.equal(hi.double() + lo.double(), v.double())  # the planes hold the operand exactly
    full = torch.zeros_like(tensor)
    full[:, h:h + t_out, :c] = hi
    full[:, h:h + t_out, cp:cp + c] = lo
    full[:, h:h + t_out, 2 * cp:2 * cp + c] = hi
    if ones:
        full[:, h:h + t_out, cp - 1] = 1
        full[:, h:h + t_out, 3 * cp - 1] = 1
    tensor.copy_(full)
    return bool(lo.float().any())


def _check_planes(tensor, t_out, want_units, unit, ones, where):
    """a stored plane tensor: hi + lo (float64, exact) in multiples of `unit` equals the int64 reference on the real channels;
    the third plane repeats hi; halo rows, rows beyond t_out and padded channels are zero; the ones channel is hi = 1, lo = 0"""
    h = _halo()
    raw = tensor.double().cpu().numpy()
    cp = raw.shape[2] // 3
    hi, lo, hi2 = raw[:, :, :cp], raw[:, :, cp:2 * cp], raw[:, :, 2 * cp:]
    assert np.array_equal(hi, hi2), (where, "third plane is not the hi plane")
    c = want_units.shape[2]
    xi.assert_exact((hi + lo)[:, h:h + t_out, :c] / unit, want_units, where)
    assert not raw[:, :h].any() and not raw[:, h + t_out:].any(), (where, "halo rows / rows beyond t_out")
    last = cp - 1 if ones else cp
    assert not hi[:, h:h + t_out, c:last].any() and not lo[:, h:h + t_out, c:].any(), (where, "padded channels")
    if ones:
        assert (hi[:, h:h + t_out, -1] == 1).all(), (where, "ones channel")


def _plane_operands(fmt, variant, rng, s, t_out):
    """integer operands of one layer for a plane variant, each with the unit (a power of two) its values are multiples of:
    x, forward weights (two +1 / two -1 positions per output column), dgrad weights (per input channel) and gradient, and the
    gradient of the weight / bias-gradient launches.  A wide operand (lo != 0) only ever meets narrow ones: lo * lo = 0."""
    shape_x, shape_g = (3, t_out, s.cin), (3, t_out, s.cout)
    k = s.kernel_size
    ops = dict(x=(xi.family_a_input(rng, shape_x), 1.0),
               w_fwd=(xi.family_a_weights(rng, k, s.cin, s.cout), 1.0),
               w_dgrad=(xi.family_a_weights(rng, k, s.cin, s.cout, by_input=True), 1.0),
               g_dgrad=(rng.randint(-1, 2, size=shape_g).astype(np.int64), fmt.g_unit),
               g_wgrad=(rng.randint(-2, 3, size=shape_g).astype(np.int64), fmt.g_unit))
    if variant == "lo_second":  # the weights of the NT launches, the gradient of the weight-gradient launches
        for name in ("w_fwd", "w_dgrad"):
            ops[name] = (ops[name][0] * xi.wide_ints(rng, ops[name][0].shape, fmt.wide_bits), fmt.w_unit)
        ops["g_wgrad"] = (xi.wide_ints(rng, shape_g, fmt.g_wide_bits, signed=True), fmt.g_unit)
    elif variant == "lo_first":  # the activations of forward and weight gradient, the gradient of the input-gradient launch
        ops["x"] = (xi.wide_ints(rng, shape_x, fmt.wide_bits, density=0.5), fmt.act_unit)
        ops["g_dgrad"] = (xi.wide_ints(rng, shape_g, fmt.g_wide_bits, signed=True), fmt.g_unit)
        ops["g_wgrad"] = (xi.sparse_columns(rng, 3, t_out, s.cout, 8, [-1, 1]), fmt.g_unit)
    return ops


def _run_plane_layer(eng, buf, layer, ops, fmt, where, forward_only=False):
    """forward, input gradient, weight gradient and bias gradient of ONE layer of a plane engine with the engine's own launch
    sequence (engine_x3.py) on operands written into buf.y / buf.g; returns which operands had a non-zero lo plane"""
    import torch
    from speechless_amd import _lib
    p = eng.plans[layer]
    s = p.spec
    t_out = buf.t_out
    st = torch.cuda.current_stream().cuda_stream
    h = _halo()
    ones_in = eng._has_ones_output(eng.plans[layer - 1])
    (x, xu), (wf, wfu), (wd, wdu) = ops["x"], ops["w_fwd"], ops["w_dgrad"]
    bias = np.arange(s.cout) % 2
    lo_seen = {}

    def clear(t):
        t.fill_(3)
        t[:, :h].zero_()
        t[:, h + t_out:].zero_()

    # ---- forward: bias, ReLU and the split into planes in the NT kernel's epilogue
    lo_seen["x"] = _store_planes(eng, buf.y[layer - 1], t_out, x * xu, ones_in)
    _set_layer(eng, layer, wf * wfu, bias)
    eng.repack_weights()
    cp = p.cin_pad
    lo_seen["w"] = bool(eng.w_fwd[layer][:, :, 2 * cp:].float().any())
    clear(buf.y[layer])
    eng.lib.call("sl_conv1d_nt", buf.y[layer - 1].data_ptr(), eng.w_fwd[layer].data_ptr(),
                 eng.layer_param_views(eng.params, p)[1].data_ptr(), None, buf.y[layer].data_ptr(),
                 ctypes.byref(eng._plane_geom(buf, "fwd", layer, p.cout_pad)), _lib.EPI_BIAS_RELU, eng.dtype_code, 2, 0,
                 buf.nt_ws.data_ptr(), buf.nt_ws.numel(), st)
    torch.cuda.synchronize()
    unit = xu * wfu
    want = xi.reference_forward(x, wf, np.rint(bias / unit).astype(np.int64))
    assert np.abs(want).max() < 2 ** fmt.bits and fmt.planes_exact(want * unit)
    _check_planes(buf.y[layer], t_out, want, unit, eng._has_ones_output(p), where + " forward")
    if forward_only:
        return lo_seen
    # ---- input gradient: stored gradient planes hold g_scale * g, the ReLU mask is the hi plane of the layer's input
    g, gu = ops["g_dgrad"]
    _set_layer(eng, layer, wd * wdu, bias)
    eng.repack_weights()
    lo_seen["g"] = _store_planes(eng, buf.g[layer], t_out, g * gu * eng.g_scale, False)
    clear(buf.g[layer - 1])
    eng.lib.call("sl_conv1d_nt", buf.g[layer].data_ptr(), eng.w_dgrad[layer].data_ptr(), None, buf.y[layer - 1].data_ptr(),
                 buf.g[layer - 1].data_ptr(), ctypes.byref(eng._plane_geom(buf, "dgrad", layer, p.cin_pad)),
                 _lib.EPI_RELU_MASK, eng.dtype_code, 2, 0, buf.nt_ws.data_ptr(), buf.nt_ws.numel(), st)
    torch.cuda.synchronize()
    want = xi.reference_input_gradient(g, wd, mask=x)
    assert np.abs(want).max() < 2 ** fmt.bits and fmt.planes_exact(want * gu * wdu * eng.g_scale)
    _check_planes(buf.g[layer - 1], t_out, want, gu * wdu * eng.g_scale, False, where + " input gradient")
    # ---- weight gradient ([hi | lo] of x against g_hi, x_hi against g_lo, combined) and bias gradient
    g, gu = ops["g_wgrad"]
    lo_seen["g_wgrad"] = _store_planes(eng, buf.g[layer], t_out, g * gu * eng.g_scale, False)
    dw_v, db_v = eng.layer_param_views(eng.grads, p)
    wa, wb = buf.wgrad_geom[layer], buf.wgrad_geom_b[layer]
    ra = buf.wgrad_r
    rb = buf.wgrad_r[p.taps_view * wa.cin * p.cout_pad:]
    xp = buf.y[layer - 1].data_ptr()
    eng.lib.call("sl_conv1d_wgrad", xp, buf.g[layer].data_ptr(), ra.data_ptr(), ctypes.byref(wa), eng.dtype_code, 0,
                 buf.wgrad_ws.data_ptr(), buf.wgrad_ws.numel(), st)
    eng.lib.call("sl_conv1d_wgrad", xp, buf.g[layer].data_ptr() + p.cout_pad * 2, rb.data_ptr(), ctypes.byref(wb),
                 eng.dtype_code, 0, buf.wgrad_ws.data_ptr(), buf.wgrad_ws.numel(), st)
    args = (ra.data_ptr(), rb.data_ptr(), dw_v.data_ptr(), s.kernel_size, p.cin_pad, p.cout_pad, 1, 0, wa.cin, wb.cin, 0)
    if eng.x3_f16:
        eng.lib.call("sl_split3_wgrad_combine_scaled", *args, 1.0 / eng.g_scale, st)
    else:
        eng.lib.call("sl_split3_wgrad_combine", *args, st)
    ws = torch.empty((eng.lib.raw("sl_split3_bias_grad_workspace_bytes")(p.cout_pad),), dtype=torch.uint8, device=eng.device)
    bargs = (buf.g[layer].data_ptr(), db_v.data_ptr(), buf.batch, t_out, p.cout_pad, h, buf.rows * p.cout_pad * 3)
    eng.lib.call(eng._x3("sl_split3_bias_grad"), *bargs, *((1.0 / eng.g_scale,) if eng.x3_f16 else ()), ws.data_ptr(),
                 ws.numel(), st)
    torch.cuda.synchronize()
    dw_ref = xi.reference_weight_gradient(x, g, s.kernel_size)
    db_ref = xi.reference_bias_gradient(g)
    assert np.abs(dw_ref).max() < xi.FP32_BUDGET and np.abs(db_ref).max() < xi.FP32_BUDGET
    full = dw_v.double().cpu().numpy()
    xi.assert_exact(full[:, :s.cin, :s.cout] / (xu * gu), dw_ref, where + " weight gradient")
    assert not full[:, :, s.cout:].any(), (where, "weight gradient: padded output lanes")
    db = db_v.double().cpu().numpy()
    xi.assert_exact(db[:s.cout] / gu, db_ref, where + " bias gradient")
    if ones_in:
        assert not full[:, s.cin:p.cin_pad - 1, :].any(), (where, "weight gradient: padded input lanes")
        xi.assert_exact(full[p.pad_left, p.cin_pad - 1, :s.cout] / gu, db_ref, where + " bias gradient in the ones-channel row")
    return lo_seen


@pytest.mark.parametrize("variant", xi.PLANE_VARIANTS)
@pytest.mark.parametrize("layer", [1, 8])
@pytest.mark.parametrize("dtype", ["bf16x3", "f16x3"])
def test_plane_layer_is_exact(dtype, layer, variant):
    """the [hi | lo | hi] plane epilogues of both parity engines, layers 1 and 8: forward, input gradient, weight gradient and
    bias gradient on integers whose two-plane split is exact under the engine's own scales, in the three variants that keep
    the omitted lo * lo term zero -- no lo plane; only the second operand's; only the first operand's (one cross term each).
    Stored planes are compared as hi + lo, unscaled; weight and bias gradients as the fp32 values they are."""
    fmt = xi.PLANE_FORMATS[dtype]
    case = make_case(b=3, t=150, seed=30)
    eng = make_engine(case, dtype)
    assert (eng.w_scale, eng.g_scale) == (fmt.w_scale, fmt.g_scale)  # the scales the operand units were chosen for
    buf = eng.load_input(case["x"])
    buf.ensure_backward(eng)
    rng = np.random.RandomState(900 + 10 * layer + xi.PLANE_VARIANTS.index(variant))
    ops = _plane_operands(fmt, variant, rng, eng.specs[layer], buf.t_out)
    lo = _run_plane_layer(eng, buf, layer, ops, fmt, "{} layer {} {}".format(dtype, layer, variant))
    expect = {"lo_none": (False, False, False, False), "lo_second": (False, True, False, True),
              "lo_first": (True, False, True, False)}[variant]
    assert (lo["x"], lo["w"], lo["g"], lo["g_wgrad"]) == expect, lo  # the variant isolates the cross term it names


def test_f16x3_forward_keeps_denormal_weight_planes():
    """f16x3 forward with weights of magnitude 2^-10: 2^6 * w splits into a normal fp16 hi plane and a lo plane below 2^-14, in
    fp16's denormal range.  {0, 1, 2} inputs; the result (multiples of 2^-30 below 2^-7) is exact only if the MFMA keeps
    denormal inputs -- the claim of DESIGN.md section 1.  Compared before the plane split rounds it: through the fp32
    pre-activations, whose 23 significant bits hold every sum of four such weights."""
    import torch
    from speechless_amd import _lib
    fmt = xi.PLANE_FORMATS["f16x3"]
    layer = 1
    case = make_case(b=3, t=150, seed=30)
    eng = make_engine(case, "f16x3")
    buf = eng.load_input(case["x"])
    p = eng.plans[layer]
    s = p.spec
    t_out = buf.t_out
    rng = np.random.RandomState(77)
    w, n = xi.denormal_weights(rng, s.kernel_size, s.cin, s.cout)
    x = rng.randint(0, 3, size=(3, t_out, s.cin)).astype(np.int64)
    assert not _store_planes(eng, buf.y[layer - 1], t_out, x, True)
    _set_layer(eng, layer, w)
    eng.repack_weights()
    lo = eng.w_fwd[layer][:, :, 2 * p.cin_pad:].float()
    assert bool(lo.any()) and float(lo.abs().max()) < 2.0 ** -14  # the lo plane is there and denormal
    st = torch.cuda.current_stream().cuda_stream
    buf.stage32.fill_(3)
    eng.lib.call("sl_conv1d_nt", buf.y[layer - 1].data_ptr(), eng.w_fwd[layer].data_ptr(), None, None, buf.stage32.data_ptr(),
                 ctypes.byref(buf.fwd_geom[layer]), _lib.EPI_NONE, eng.dtype_code, 1, 0, buf.nt_ws.data_ptr(),
                 buf.nt_ws.numel(), st)
    torch.cuda.synchronize()
    want = xi.reference_preactivation(x, n, np.zeros(s.cout, dtype=np.int64))
    assert np.abs(want).max() < xi.FP32_BUDGET
    got = buf.stage32[:3 * buf.tt_pad * p.cout_pad].view(3, buf.tt_pad, p.cout_pad).double().cpu().numpy()
    xi.assert_exact(got[:, :t_out, :s.cout] * 2.0 ** 30, want, "f16x3 forward, denormal lo plane of the weights")
    assert not got[:, :t_out, s.cout:].any() and (got[:, t_out:] == 3).all()
