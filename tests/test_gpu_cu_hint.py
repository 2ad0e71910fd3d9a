"""GPU tests of sl_set_available_cus (the "CU hint" of data-parallel runs): the setter, each of the six
host-side launch choosers that read it -- through the C ABI, under hints that change their decision, against float64 -- and
the training step under Engine.comm_cus / GradBucketReducer(comm_cus=...) on one rank through the real RCCL backend.

Every test leaves the calling thread's setting at 0 (the autouse fixture below resets it whatever happens).
float64 references are plain per-tap matmuls in torch.float64 (they share nothing with the HIP kernels)."""
import contextlib
import ctypes
import os
import threading

import numpy as np
import pytest

from oracle import w2l_oracle as o
from test_gpu_parity import _bf16_exact, _nt_cfg, _report, make_case, make_engine, rel_l2, weights64

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, WORKSPACE_TOO_SMALL = -1, -3
GUARD_BYTES, GUARD_BYTE = 4096, 0xA5
HINTS = (64, 128, 192, 224)


@pytest.fixture(autouse=True)
def cu_hint_cleared(hip_lib):
    hip_lib.raw("sl_set_available_cus")(0)
    yield
    hip_lib.raw("sl_set_available_cus")(0)


@contextlib.contextmanager
def hinted(lib, cus):
    lib.call("sl_set_available_cus", cus)
    try:
        yield
    finally:
        lib.call("sl_set_available_cus", 0)


def _geom(batch, t_out, taps, cin, cout, x_row0, x_rs, x_bs, y_row0, y_rs, y_bs):
    from speechless_amd import _lib
    g = _lib.ConvGeom()
    g.batch, g.t_out, g.taps, g.cin, g.cout = batch, t_out, taps, cin, cout
    g.x_row0, g.x_row_stride, g.x_batch_stride = x_row0, x_rs, x_bs
    g.y_row0, g.y_row_stride, g.y_batch_stride = y_row0, y_rs, y_bs
    return g


# the first NT geometry of section 2: 32 taps x 384 channels = 192 steps in 6 chunks, 40 tiles of 256 x 256
NT_BATCH, NT_T, NT_TAPS, NT_CIN, NT_COUT, NT_HALO = 40, 70, 32, 384, 256, 48
NT_ROWS = NT_HALO + 256 + NT_HALO


def _nt_geom(y_planes=1):
    pad_l = (NT_TAPS - 1) // 2
    return _geom(NT_BATCH, NT_T, NT_TAPS, NT_CIN, NT_COUT, NT_HALO - pad_l, NT_CIN, NT_ROWS * NT_CIN, NT_HALO,
                 y_planes * NT_COUT, NT_ROWS * y_planes * NT_COUT)


def nt_split_k(lib):
    """the observable of the calling thread's setting: split-K count the NT chooser picks for the geometry above (host only)"""
    from speechless_amd import _lib
    need = lib.raw("sl_conv1d_nt_workspace_bytes")(ctypes.byref(_nt_geom()), _lib.SL_BF16, 0)
    per_split = NT_BATCH * 256 * NT_COUT * 4
    assert need % per_split == 0
    return need // per_split


class Workspace:
    """exactly `need` bytes for the library, a guard region of GUARD_BYTE behind them"""

    def __init__(self, need):
        import torch
        self.need = int(need)
        self.t = torch.empty((self.need + GUARD_BYTES,), dtype=torch.uint8, device="cuda:0")
        self.t[self.need:] = GUARD_BYTE
        self.ptr = self.t.data_ptr()

    def guard_intact(self):
        return bool((self.t[self.need:] == GUARD_BYTE).all())


def check_under_hints(lib, hints, need_fn, run_fn, check_fn, untouched_fn):
    """The protocol of section 2 of the issue for one launch.  need_fn() -> workspace bytes under the calling thread's setting;
    run_fn(ptr, nbytes) -> (status, outputs as numpy arrays), outputs pre-filled with a sentinel; check_fn(outputs, label)
    asserts a correct result; untouched_fn(outputs) asserts that nothing was written.  Returns {setting: bytes}."""
    need = {}
    for s in (0,) + tuple(hints):
        with hinted(lib, s):
            need[s] = int(need_fn())
            outs = []
            for _ in range(2):
                ws = Workspace(need[s])
                rc, out = run_fn(ws.ptr, ws.need)
                assert rc == 0, (s, rc, lib.last_error())
                assert ws.guard_intact(), ("wrote past the workspace it asked for", s, need[s])
                check_fn(out, "sized and launched under {}".format(s))
                outs.append(out)
            for a, b in zip(*outs):
                assert np.array_equal(a, b), ("not deterministic under", s)
    for h in hints:
        big = Workspace(max(need[0], need[h]))
        for s in (0, h):  # sized under one, launched under the other
            with hinted(lib, s):
                rc, out = run_fn(big.ptr, big.need)
            assert rc == 0 and big.guard_intact(), (h, s, rc, lib.last_error())
            check_fn(out, "workspace for {{0, {}}}, launched under {}".format(h, s))
        if need[h] != need[0]:  # too small for the active setting: an error, not a launch
            large, small = (h, need[0]) if need[h] > need[0] else (0, need[h])
            ws = Workspace(small)
            with hinted(lib, large):
                rc, out = run_fn(ws.ptr, ws.need)
            assert rc == WORKSPACE_TOO_SMALL, (h, rc)
            assert ws.guard_intact()
            untouched_fn(out)
    return need


def _f64(a):
    import torch
    return torch.as_tensor(np.asarray(a), device="cuda:0").double()


def _exact16(rng, shape, scale=1.0):
    """values exact in bf16 AND in fp16 (8 significant bits, nothing below fp16's normal range)"""
    v = _bf16_exact(rng, shape, scale)
    v[np.abs(v) < 2.0 ** -14] = 0
    assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
    return v


# ============================================================================================ 1. the setter
def test_setter_accepts_0_and_64_to_256_and_rejects_the_rest(hip_lib):
    """0 and 64 .. 256 are accepted (0 = 256); 1, 63, 257 and -1 come back as SL_ERR_INVALID_ARGUMENT with the range in
    sl_last_error() and leave the previous setting in force.  Observable: the NT chooser's split-K on 40 tiles x 6 chunks --
    6 splits while 240 work-groups fit one round (240 .. 256 CUs), 3 below."""
    setter = hip_lib.raw("sl_set_available_cus")
    assert nt_split_k(hip_lib) == 6
    for cus, want in ((64, 3), (128, 3), (239, 3), (240, 6), (256, 6), (224, 3), (0, 6)):
        assert setter(cus) == 0, cus
        assert nt_split_k(hip_lib) == want, (cus, nt_split_k(hip_lib))
    for previous, want in ((192, 3), (0, 6)):
        assert setter(previous) == 0
        for bad in (1, 63, 257, -1):
            assert setter(bad) == INVALID_ARGUMENT, bad
            assert "0 (all) or 64 .. 256" in hip_lib.last_error(), hip_lib.last_error()
            assert nt_split_k(hip_lib) == want, (previous, bad)


def test_setting_zero_equals_256(hip_lib):
    from speechless_amd import _lib
    answers = []
    for cus in (0, 256):
        with hinted(hip_lib, cus):
            g = _geom(6, 200, 7, 256, 256, 13, 256, 288 * 256, 16, 256, 288 * 256)
            answers.append((nt_split_k(hip_lib), hip_lib.raw("sl_conv1d_wgrad_workspace_bytes")(ctypes.byref(g), _lib.SL_BF16, 0)))
    assert answers[0] == answers[1] and answers[0][0] == 6


def test_setting_is_per_thread(hip_lib):
    """A hint set in a threading.Thread is not seen by the main thread, and a hint of the main thread not by a new thread."""
    seen = {}

    def worker():
        seen["fresh"] = nt_split_k(hip_lib)           # the main thread holds 192 at this point
        hip_lib.call("sl_set_available_cus", 64)
        seen["own"] = nt_split_k(hip_lib)
        go.set()
        done.wait(10)
        seen["own_later"] = nt_split_k(hip_lib)       # the main thread went back to 0 in between
        hip_lib.call("sl_set_available_cus", 0)

    go, done = threading.Event(), threading.Event()
    with hinted(hip_lib, 192):
        assert nt_split_k(hip_lib) == 3
        th = threading.Thread(target=worker)
        th.start()
        assert go.wait(10)
        assert nt_split_k(hip_lib) == 3
    assert nt_split_k(hip_lib) == 6                    # the worker's 64 is still set -- on ITS thread
    done.set()
    th.join(10)
    assert not th.is_alive()
    assert seen == {"fresh": 6, "own": 3, "own_later": 3}, seen


# ============================================================================================ 2. the choosers
_NT_OPERANDS = {}


def _nt_operands():
    """operands of the NT geometry (exact in bf16 and fp16) and the float64 sum, computed once"""
    if not _NT_OPERANDS:
        import torch
        rng = np.random.RandomState(32384)
        x = np.zeros((NT_BATCH, NT_ROWS, NT_CIN), dtype=np.float32)
        x[:, NT_HALO:NT_HALO + NT_T] = _exact16(rng, (NT_BATCH, NT_T, NT_CIN))
        w = _exact16(rng, (NT_TAPS, NT_CIN, NT_COUT), 0.05)
        bias = _bf16_exact(rng, (NT_COUT,), 0.1)
        mask = np.zeros((NT_BATCH, NT_ROWS, NT_COUT), dtype=np.float32)
        mask[:, NT_HALO:NT_HALO + NT_T] = _exact16(rng, (NT_BATCH, NT_T, NT_COUT))
        pad_l = (NT_TAPS - 1) // 2
        xd, wd = _f64(x), _f64(w)
        acc = torch.zeros((NT_BATCH, NT_T, NT_COUT), dtype=torch.float64, device="cuda:0")
        for tap in range(NT_TAPS):
            acc += xd[:, NT_HALO - pad_l + tap: NT_HALO - pad_l + tap + NT_T] @ wd[tap]
        _NT_OPERANDS.update(x=x, w=w, bias=bias, mask=mask, acc=acc.cpu().numpy())
    return _NT_OPERANDS


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_nt_split_k_chooser_under_hints_against_float64(hip_lib, dtype):
    """conv_nt_bf16.hip auto_cfg (compiled for bf16 and for f16): 40 tiles x 192 steps in 6 chunks.  Split-K 6 at 256 CUs (240
    work-groups, one round) -> 3 at 224, 192, 128 and 64.  Forward launches (bias / bias + ReLU) and input-gradient launches
    (ReLU mask) with cfg 0.  fp32 and plane outputs (hi + lo) against float64 at rel_l2 < 2e-6.  A bf16 output carries its own
    rounding: it is held to 3e-3 (the bound of test_single_layer_kernels_with_exact_operands for it), every element to one bf16
    ulp (2^-8 relative) of the float64 value, and the launch under a hint must equal bit for bit the launch at 256 CUs with the
    chosen split forced through the cfg word (the 8-wave interleaved slab tile with ksplit = 3) -- so the tail that reduces the
    partial tiles and applies the mask is the one the fp32 launches pin to 2e-6."""
    import torch
    from speechless_amd import _lib
    ops = _nt_operands()
    dev, st = "cuda:0", torch.cuda.current_stream().cuda_stream
    code, td = (_lib.SL_BF16, torch.bfloat16) if dtype == "bf16" else (_lib.SL_F16, torch.float16)
    xt = torch.tensor(ops["x"]).to(td).to(dev)
    wt = torch.tensor(ops["w"]).permute(2, 0, 1).contiguous().to(td).to(dev)   # packed [cout][taps][cin]
    bias_t = torch.tensor(ops["bias"]).to(dev)
    valid = slice(NT_HALO, NT_HALO + NT_T)
    acc, bias, mask = ops["acc"], ops["bias"].astype(np.float64), ops["mask"][:, valid]
    want = {_lib.EPI_BIAS: acc + bias, _lib.EPI_BIAS_RELU: np.maximum(acc + bias, 0), _lib.EPI_RELU_MASK: acc * (mask > 0)}
    if dtype == "bf16":
        launches = [(_lib.EPI_BIAS, 1, 2e-6), (_lib.EPI_BIAS_RELU, 0, 3e-3), (_lib.EPI_RELU_MASK, 0, 3e-3)]
    else:  # (the fp16 build serves the plane path: fp32 or [hi | lo | hi] plane outputs)
        launches = [(_lib.EPI_BIAS, 1, 2e-6), (_lib.EPI_BIAS_RELU, 2, 2e-6), (_lib.EPI_RELU_MASK, 2, 2e-6)]
    decisions = None
    for epi, out_f32, bound in launches:
        planes = 3 if out_f32 == 2 else 1
        geom = _nt_geom(planes)
        ydt = torch.float32 if out_f32 == 1 else td
        mask_t = None
        if epi == _lib.EPI_RELU_MASK:  # same geometry as y; plane outputs read the mask's hi plane
            m = torch.zeros((NT_BATCH, NT_ROWS, planes * NT_COUT), dtype=td, device=dev)
            m[:, :, :NT_COUT] = torch.tensor(ops["mask"]).to(td).to(dev)
            mask_t = m

        def need_fn():
            return hip_lib.raw("sl_conv1d_nt_workspace_bytes")(ctypes.byref(geom), code, 0)

        def run_fn(ptr, nbytes):
            y = torch.full((NT_BATCH, NT_ROWS, planes * NT_COUT), 7.0, dtype=ydt, device=dev)
            rc = hip_lib.raw("sl_conv1d_nt")(xt.data_ptr(), wt.data_ptr(), bias_t.data_ptr(),
                                             mask_t.data_ptr() if mask_t is not None else None, y.data_ptr(),
                                             ctypes.byref(geom), epi, code, out_f32, 0, ptr, nbytes, st)
            torch.cuda.synchronize()
            return rc, (y.float().cpu().numpy(),)

        def check_fn(out, label):
            y = out[0]
            got = y[:, valid].astype(np.float64)
            if planes == 3:
                assert np.array_equal(got[:, :, :NT_COUT], got[:, :, 2 * NT_COUT:]), label
                got = got[:, :, :NT_COUT] + got[:, :, NT_COUT:2 * NT_COUT]
            err = rel_l2(got, want[epi])
            assert err < bound, (dtype, epi, out_f32, label, err)
            if out_f32 == 0:  # one bf16 ulp per element (fp32 accumulation of 12288 terms of size ~0.05: 1e-5 absolute)
                assert (np.abs(got - want[epi]) <= 2.0 ** -8 * np.abs(want[epi]) + 1e-5).all(), (label, epi)
            if epi == _lib.EPI_RELU_MASK:
                assert not got[mask <= 0].any(), label
            assert (y[:, :NT_HALO] == 7.0).all() and (y[:, NT_HALO + NT_T:] == 7.0).all(), "rows outside [0, t_out) written"

        def untouched_fn(out):
            assert (out[0] == 7.0).all()

        hints = HINTS if out_f32 == 1 else (64, 224)  # (every hint once, the ends for the other epilogues)
        need = check_under_hints(hip_lib, hints, need_fn, run_fn, check_fn, untouched_fn)
        per_split = NT_BATCH * 256 * NT_COUT * 4
        decisions = {s: n // per_split for s, n in need.items()}
        assert decisions == dict([(0, 6)] + [(h, 3) for h in hints]), decisions  # not vacuous: the hints change the split
        if dtype == "bf16":  # cfg 0 under a hint == the same tile with the split forced, at 256 CUs
            for s, ks in ((224, 3), (0, 6)):
                ws = Workspace(NT_BATCH * 256 * NT_COUT * 4 * ks)
                with hinted(hip_lib, s):
                    rc, auto = run_fn(ws.ptr, ws.need)
                assert rc == 0
                y = torch.full((NT_BATCH, NT_ROWS, planes * NT_COUT), 7.0, dtype=ydt, device=dev)
                hip_lib.call("sl_conv1d_nt", xt.data_ptr(), wt.data_ptr(), bias_t.data_ptr(),
                             mask_t.data_ptr() if mask_t is not None else None, y.data_ptr(), ctypes.byref(geom), epi, code,
                             out_f32, _nt_cfg(2, 4, 10, ks, 8, 0, 0, 3), ws.ptr, ws.need, st)
                torch.cuda.synchronize()
                assert np.array_equal(auto[0], y.float().cpu().numpy()), (epi, out_f32, s, ks)
    print("NT split-K ({}): 256 CUs -> {}, under hints {}".format(dtype, decisions[0], decisions))


def _wgrad_case(rng, groups, batch, t_out, taps, cin, cout, halo=16):
    import torch
    rows = halo + ((t_out + 63) // 64) * 64 + halo
    pad_l = (taps - 1) // 2
    x = np.zeros((groups, batch, rows, cin), dtype=np.float32)
    g = np.zeros((groups, batch, rows, cout), dtype=np.float32)
    x[:, :, halo:halo + t_out] = _bf16_exact(rng, (groups, batch, t_out, cin))
    g[:, :, halo:halo + t_out] = _bf16_exact(rng, (groups, batch, t_out, cout), 0.05)
    geom = _geom(batch, t_out, taps, cin, cout, halo - pad_l, cin, rows * cin, halo, cout, rows * cout)
    xd, gd = _f64(x), _f64(g)
    want = torch.zeros((groups, taps, cin, cout), dtype=torch.float64, device="cuda:0")
    for q in range(groups):
        gq = gd[q, :, halo:halo + t_out].reshape(-1, cout)
        for tap in range(taps):
            want[q, tap] = xd[q, :, halo - pad_l + tap: halo - pad_l + tap + t_out].reshape(-1, cin).T @ gq
    xt = torch.tensor(x).to(torch.bfloat16).to("cuda:0")
    gt = torch.tensor(g).to(torch.bfloat16).to("cuda:0")
    return xt, gt, geom, want.cpu().numpy(), rows


@pytest.mark.parametrize("name,groups,batch,t_out,taps,cin,cout,hints,expect", [
    # 28 tiles of 128 x 128, target 512 work-groups: 6 splits; target 128 at 64 CUs: 3 (the tie goes to the smaller count)
    ("single", 1, 6, 200, 7, 256, 256, HINTS, {0: 6, 64: 3}),
    # three layers in one launch (as test_every_wgrad_tile_configuration_against_float64's grouped case)
    ("grouped", 3, 6, 130, 3, 256, 256, HINTS, None),
    # one column of tiles under a wide input (output_conv): 3-slot ring and HALF the chosen splits
    ("output_layer", 1, 16, 100, 1, 2048, 128, HINTS, {0: 8, 64: 4}),
])
def test_wgrad_batch_split_chooser_under_hints_against_float64(hip_lib, name, groups, batch, t_out, taps, cin, cout, hints, expect):
    """wgrad_tn_bf16.hip choose_splits through sl_conv1d_wgrad / sl_conv1d_wgrad_grouped with cfg 0: the batch-split count
    scales its work-group target with the CU count; the workspace query (splits x taps x cin x cout floats per group) shows the
    decision, which must differ from the one at 256 CUs under at least one hint."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(taps * 100 + batch + groups)
    xt, gt, geom, want, rows = _wgrad_case(rng, groups, batch, t_out, taps, cin, cout)
    st = torch.cuda.current_stream().cuda_stream
    n = taps * cin * cout
    dw_stride = n + 64

    def need_fn():
        if groups == 1:
            return hip_lib.raw("sl_conv1d_wgrad_workspace_bytes")(ctypes.byref(geom), _lib.SL_BF16, 0)
        return hip_lib.raw("sl_conv1d_wgrad_grouped_workspace_bytes")(ctypes.byref(geom), groups, 0)

    def run_fn(ptr, nbytes):
        dw = torch.full((groups * dw_stride,), 3.0, dtype=torch.float32, device="cuda:0")
        if groups == 1:
            rc = hip_lib.raw("sl_conv1d_wgrad")(xt.data_ptr(), gt.data_ptr(), dw.data_ptr(), ctypes.byref(geom), _lib.SL_BF16, 0,
                                                ptr, nbytes, st)
        else:
            rc = hip_lib.raw("sl_conv1d_wgrad_grouped")(xt.data_ptr(), gt.data_ptr(), dw.data_ptr(), ctypes.byref(geom), groups,
                                                        batch * rows * cin, batch * rows * cout, dw_stride, 0, ptr, nbytes, st)
        torch.cuda.synchronize()
        return rc, (dw.cpu().numpy().reshape(groups, dw_stride),)

    def check_fn(out, label):
        err = rel_l2(out[0][:, :n].reshape(groups, taps, cin, cout), want)
        assert err < 2e-6, (name, label, err)
        assert (out[0][:, n:] == 3.0).all(), "wrote past a group's weight block"

    def untouched_fn(out):
        assert (out[0] == 3.0).all()

    need = check_under_hints(hip_lib, hints, need_fn, run_fn, check_fn, untouched_fn)
    splits = {s: max(1, v // (groups * n * 4)) for s, v in need.items()}
    print("wgrad batch splits ({}): 256 CUs -> {}, under hints {}".format(name, splits[0], splits))
    assert any(splits[h] != splits[0] for h in hints), splits  # not vacuous
    for s, v in (expect or {}).items():
        assert splits[s] == v, splits
    if name == "output_layer":
        # the branch halves what choose_splits picks for 128 x 128 tiles; sl_conv1d_wgrad with an explicit 2 x 2 tile and
        # splits = 0 runs the same chooser without the halving
        for s in (0,) + tuple(hints):
            with hinted(hip_lib, s):
                full = hip_lib.raw("sl_conv1d_wgrad_workspace_bytes")(ctypes.byref(geom), _lib.SL_BF16, 2 | (2 << 4) | (2 << 8))
            chosen = max(1, full // (n * 4))
            assert splits[s] == (chosen // 2 if chosen >= 2 and chosen % 2 == 0 else chosen), (s, splits[s], chosen)


def _multi_plan(lib, table, n_jobs):
    from speechless_amd import _lib
    segs, workers = ctypes.c_int(-1), ctypes.c_int(-1)
    lib.call("sl_conv1d_wgrad_multi_plan", table, n_jobs, _lib.SL_BF16, ctypes.byref(segs), ctypes.byref(workers))
    return segs.value, workers.value


@pytest.mark.parametrize("name,shapes,batch,t_out,expect", [
    # the engine's mix: the striding layer's pair view (24 taps over 2 x 128 channels) and two inner layers: 38 tiles;
    # spt = 5 x 4 = 20 steps per tile.  segs = 2 * CUs / 38
    ("engine_mix", [(24, 256, 256), (7, 256, 256), (7, 256, 256)], 5, 200, {0: 13, 224: 11, 192: 10, 128: 6, 64: 3}),
    # the same jobs on 2 x 2 chunks: 13 segments clamped to spt = 4 at 256 CUs, 3 (odd, unclamped) at 64
    ("clamped_to_spt", [(24, 256, 256), (7, 256, 256), (7, 256, 256)], 2, 100, {0: 4, 128: 4, 64: 3}),
    # 140 tiles: 3 segments at 256 CUs, ONE where the tiles outnumber twice the CUs (128 and 64)
    ("one_segment", [(7, 512, 512)] * 5, 2, 100, {0: 3, 192: 2, 128: 1, 64: 1}),
    # a pair view of 640 channels (257 bins): three 256-wide tiles per tap, the last starting at 384 and overlapping its
    # neighbour; 72 + 7 = 79 tiles, spt = 3 x 3 = 9: even, odd and single segments
    ("overlapping_tile", [(24, 640, 256), (7, 256, 256)], 3, 130, {0: 6, 224: 5, 192: 4, 128: 3, 64: 1}),
])
def test_wgrad_multi_segment_chooser_under_hints_against_float64(hip_lib, name, shapes, batch, t_out, expect):
    """wgrad_tn_bf16.hip multi_fill through sl_conv1d_wgrad_multi: segs = 2 * CUs / tiles (even, odd >= 3 with its
    workers = pair_wgs + ceil(tiles / 2), 1, and clamped to the steps per tile), shown by sl_conv1d_wgrad_multi_plan.  Against
    float64 and against the per-layer sl_conv1d_wgrad launches (as test_wgrad_multi_against_the_per_layer_launches)."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(len(shapes) * 1000 + t_out)
    st = torch.cuda.current_stream().cuda_stream
    jobs = [_wgrad_case(rng, 1, batch, t_out, taps, cin, cout) for taps, cin, cout in shapes]
    sizes = [taps * cin * cout for taps, cin, cout in shapes]
    offs = np.concatenate([[0], np.cumsum([s + 64 for s in sizes])]).astype(np.int64)
    table = (_lib.WgradJob * len(jobs))()
    tiles = sum(taps * ((cin + 255) // 256) * (cout // 256) for taps, cin, cout in shapes)
    hints = tuple(h for h in expect if h)

    def fill(dw):
        for job, (xt, gt, geom, _, _), off in zip(table, jobs, offs):
            job.x, job.g, job.dw = xt.data_ptr(), gt.data_ptr(), dw.data_ptr() + int(off) * 4
            job.geom.copy_from(geom)

    def need_fn():
        fill(torch.empty((1,), device="cuda:0"))
        return hip_lib.raw("sl_conv1d_wgrad_multi_workspace_bytes")(table, len(jobs), _lib.SL_BF16)

    def run_fn(ptr, nbytes):
        dw = torch.full((int(offs[-1]),), 3.0, dtype=torch.float32, device="cuda:0")
        fill(dw)
        rc = hip_lib.raw("sl_conv1d_wgrad_multi")(table, len(jobs), _lib.SL_BF16, ptr, nbytes, st)
        torch.cuda.synchronize()
        return rc, (dw.cpu().numpy(),)

    def check_fn(out, label):
        for q, ((taps, cin, cout), (_, _, _, want, _)) in enumerate(zip(shapes, jobs)):
            got = out[0][offs[q]: offs[q] + sizes[q]].reshape(taps, cin, cout)
            err = rel_l2(got, want[0])
            assert err < 2e-6, (name, label, q, err)
            assert (out[0][offs[q] + sizes[q]: offs[q + 1]] == 3.0).all(), "wrote past a job's weight block"

    def untouched_fn(out):
        assert (out[0] == 3.0).all()

    plans = {}
    for s in (0,) + hints:
        with hinted(hip_lib, s):
            need_fn()  # (fills the job table)
            plans[s] = _multi_plan(hip_lib, table, len(jobs))
    print("wgrad multi ({}, {} tiles): (segs, workers) at 256 CUs {}, under hints {}".format(name, tiles, plans[0], plans))
    for s, segs in expect.items():
        assert plans[s][0] == segs, (s, plans)
        assert plans[s][1] == tiles * (segs // 2) + ((tiles + 1) // 2 if segs & 1 else 0), (s, plans)
    assert any(plans[h] != plans[0] for h in hints)  # not vacuous
    need = check_under_hints(hip_lib, hints, need_fn, run_fn, check_fn, untouched_fn)
    assert len(set(need.values())) == 1  # (a bound that does not depend on the segment count)
    ws = Workspace(16)  # too small under every setting: an error, not a launch
    rc, out = run_fn(ws.ptr, ws.need)
    assert rc == WORKSPACE_TOO_SMALL and ws.guard_intact()
    untouched_fn(out)
    # the per-layer launches it replaces
    with hinted(hip_lib, hints[-1]):
        big = Workspace(need[0])
        _, (multi,) = run_fn(big.ptr, big.need)
    for q, ((taps, cin, cout), (xt, gt, geom, _, _)) in enumerate(zip(shapes, jobs)):
        nbytes = hip_lib.raw("sl_conv1d_wgrad_workspace_bytes")(ctypes.byref(geom), _lib.SL_BF16, 0)
        ws = Workspace(nbytes)
        dw = torch.zeros((sizes[q],), dtype=torch.float32, device="cuda:0")
        hip_lib.call("sl_conv1d_wgrad", xt.data_ptr(), gt.data_ptr(), dw.data_ptr(), ctypes.byref(geom), _lib.SL_BF16, 0,
                     ws.ptr, ws.need, st)
        torch.cuda.synchronize()
        assert rel_l2(multi[offs[q]: offs[q] + sizes[q]], dw.cpu().numpy()) < 2e-6, (name, q)


@pytest.mark.parametrize("epilogue", ["relu", "elu"])
def test_output_layer_backward_split_chooser_under_hints_against_float64(hip_lib, epilogue):
    """conv1x1_bwd_bf16.hip pick_splits through sl_conv1d_backward_1x1 (and _part): cin 2048 = 16 column blocks, want =
    ceil(CUs / 16) frame ranges of 8 x 4 = 32 chunks: 16 splits at 256 CUs (2 chunks each), 11 at 192, 8 at 128, 4 at 64; the
    workspace is splits x cin x 32 floats.  k = 29 real classes: the padding columns of dw must come back zero.  dw (fp32) against
    float64 at 2e-6; dx is a bf16 output (3e-3, as test_fused_output_backward_against_float64_and_the_two_launches)."""
    import torch
    from speechless_amd import _lib
    rng = np.random.RandomState(2048)
    batch, t_out, cin, cout, k, halo = 8, 250, 2048, 128, 29, 16
    rows = halo + 256 + halo
    epi = _lib.EPI_RELU_MASK if epilogue == "relu" else _lib.EPI_ELU_MASK
    st = torch.cuda.current_stream().cuda_stream
    x = np.zeros((batch, rows, cin), dtype=np.float32)
    x[:, halo:halo + t_out] = _bf16_exact(rng, (batch, t_out, cin), 0.5)
    g = np.zeros((batch, rows, cout), dtype=np.float32)
    g[:, halo:halo + t_out, :k] = _bf16_exact(rng, (batch, t_out, k), 0.05)
    w = np.zeros((cin, 1, cout), dtype=np.float32)
    w[:, 0, :k] = _bf16_exact(rng, (cin, k), 0.05)
    xt, gt, wt = (torch.tensor(a).to(torch.bfloat16).to("cuda:0") for a in (x, g, w))
    geom = _geom(batch, t_out, 1, cin, cout, halo, cin, rows * cin, halo, cout, rows * cout)
    assert hip_lib.raw("sl_conv1d_backward_1x1_supported")(ctypes.byref(geom), k, _lib.SL_BF16) == 1
    xv, gv = _f64(x[:, halo:halo + t_out]), _f64(g[:, halo:halo + t_out])
    pre = gv @ _f64(w[:, 0]).T
    dx_ref = (pre * (xv > 0) if epilogue == "relu" else pre * torch.where(xv > 0, torch.ones_like(xv), xv + 1.0)).cpu().numpy()
    dw_ref = (xv.reshape(-1, cin).T @ gv.reshape(-1, cout)).cpu().numpy()
    t_written = ((t_out + 63) // 64) * 64

    def need_fn():
        return hip_lib.raw("sl_conv1d_backward_1x1_workspace_bytes")(ctypes.byref(geom), k, _lib.SL_BF16, 0)

    def run_fn(ptr, nbytes):
        dx = torch.full((batch, rows, cin), 7.0, dtype=torch.bfloat16, device="cuda:0")
        dw = torch.full((cin * cout + 64,), 3.0, dtype=torch.float32, device="cuda:0")
        rc = hip_lib.raw("sl_conv1d_backward_1x1")(xt.data_ptr(), gt.data_ptr(), wt.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                   ctypes.byref(geom), epi, k, _lib.SL_BF16, 0, ptr, nbytes, st)
        torch.cuda.synchronize()
        return rc, (dx.float().cpu().numpy(), dw.cpu().numpy())

    def check_fn(out, label):
        dx, dw = out
        assert rel_l2(dx[:, halo:halo + t_out], dx_ref) < 3e-3, (label, rel_l2(dx[:, halo:halo + t_out], dx_ref))
        assert not dx[:, halo + t_out:halo + t_written].any(), label   # written with the zeros of the layout invariant
        assert (dx[:, :halo] == 7.0).all() and (dx[:, halo + t_written:] == 7.0).all(), "rows outside the result written"
        got = dw[:cin * cout].reshape(cin, cout)
        assert rel_l2(got[:, :k], dw_ref[:, :k]) < 2e-6, (label, rel_l2(got[:, :k], dw_ref[:, :k]))
        assert not got[:, k:].any(), label                               # zeroed padding columns
        assert (dw[cin * cout:] == 3.0).all(), "wrote past dw"

    def untouched_fn(out):
        assert (out[0] == 7.0).all() and (out[1] == 3.0).all()

    need = check_under_hints(hip_lib, (64, 128, 192), need_fn, run_fn, check_fn, untouched_fn)
    splits = {s: v // (cin * 32 * 4) for s, v in need.items()}
    print("1x1 backward splits: 256 CUs -> {}, under hints {}".format(splits[0], splits))
    assert splits == {0: 16, 64: 4, 128: 8, 192: 11}, splits  # not vacuous
    # two uneven parts of the batch under a hint (the second accumulates) against the whole-batch call
    with hinted(hip_lib, 64):
        whole_ws = Workspace(need[64])
        _, (dx_whole, dw_whole) = run_fn(whole_ws.ptr, whole_ws.need)
        dx = torch.full((batch, rows, cin), 7.0, dtype=torch.bfloat16, device="cuda:0")
        dw = torch.full((cin * cout + 64,), 3.0, dtype=torch.float32, device="cuda:0")
        part_splits = []
        for first, count, accumulate in ((0, 3, 0), (3, 5, 1)):
            pg = geom.copy()
            pg.batch = count
            nbytes = hip_lib.raw("sl_conv1d_backward_1x1_workspace_bytes")(ctypes.byref(pg), k, _lib.SL_BF16, 0)
            part_splits.append(nbytes // (cin * 32 * 4))
            ws = Workspace(nbytes)
            hip_lib.call("sl_conv1d_backward_1x1_part", xt[first:].data_ptr(), gt[first:].data_ptr(), wt.data_ptr(),
                         dx[first:].data_ptr(), dw.data_ptr(), ctypes.byref(pg), epi, k, _lib.SL_BF16, 0, accumulate, ws.ptr,
                         ws.need, st)
            torch.cuda.synchronize()
            assert ws.guard_intact()
    assert np.array_equal(dx.float().cpu().numpy(), dx_whole)  # a frame's dx does not depend on the range it sits in
    check_fn((dx.float().cpu().numpy(), dw.cpu().numpy()), "two parts under 64")
    assert rel_l2(dw.cpu().numpy()[:cin * cout], dw_whole[:cin * cout]) < 2e-6
    print("1x1 backward, parts of 3 + 5 utterances under 64 CUs: splits", part_splits)


def test_chain_tile_rows_chooser_under_a_hint_is_bit_identical(hip_lib):
    """conv_chain_bf16.hip chain_tile_rows: 16 utterances x 256 frames are 64 work-groups of 64 frames or 96 of 48: 48-frame
    tiles at 256 CUs (one round either way, fewer MFMA tiles each), 64-frame tiles at 64 CUs (one round instead of two),
    shown by sl_conv1d_chain_plan.  An output row is the same sequence of accumulations in either tile
    (test_fused_inner_layers_with_48_frame_tiles_are_bit_identical), so both fused launches of the step repeated under the
    hint on the step's own buffers must reproduce activations and gradients bit for bit; each layer of the forward launch is
    also held to float64 on its stored bf16 input (3e-3: bf16 output, as test_single_layer_kernels_with_exact_operands)."""
    import torch
    from speechless_amd import _lib
    from speechless_amd.engine import HALO
    from test_gpu_parity import run_loss_and_grads
    case = make_case(b=16, t=512, seed=91)
    eng = make_engine(case, "bf16")
    eng.use_launch_lists = False
    run_loss_and_grads(eng, case)
    buf = eng.cur
    st = torch.cuda.current_stream().cuda_stream
    (s0, e0), = [r for r in eng.runs if r[1] - r[0] >= 1]
    layers = list(range(s0, e0 + 1))
    plan = lambda geom, n: hip_lib.raw("sl_conv1d_chain_plan")(ctypes.byref(geom), n, _lib.SL_BF16)  # noqa: E731
    rows = {0: plan(buf.fwd_geom[s0], len(layers))}
    with hinted(hip_lib, 64):
        rows[64] = plan(buf.fwd_geom[s0], len(layers))
    print("chain tile rows: 256 CUs -> {}, 64 CUs -> {}".format(rows[0], rows[64]))
    assert rows == {0: 48, 64: 64}, rows  # not vacuous
    try:
        hip_lib.call("sl_conv1d_chain_select", 64)
        assert plan(buf.fwd_geom[s0], len(layers)) == 64
    finally:
        hip_lib.call("sl_conv1d_chain_select", 0)
    dchain, _ = eng._dgrad_chains(buf, 0)
    (top, dlayers), = dchain.items()
    with hinted(hip_lib, 64):
        assert plan(buf.dgrad_geom[top], len(dlayers)) == 64
    assert plan(buf.dgrad_geom[top], len(dlayers)) == 48
    y_ref = [buf.y[i].clone() for i in layers]
    g_ref = [buf.g[i - 1].clone() for i in dlayers]
    for i in layers:
        buf.y[i].zero_()
    for i in dlayers:
        buf.g[i - 1].zero_()
    with hinted(hip_lib, 64):
        ys, ws, biases = eng._chain_table("fwd", layers, buf)
        hip_lib.call("sl_conv1d_chain", buf.y[s0 - 1].data_ptr(), ys, ws, biases, None, ctypes.byref(buf.fwd_geom[s0]),
                     len(layers), _lib.EPI_BIAS_RELU, _lib.SL_BF16, st)
        gs, wd, masks = eng._chain_table("dgrad", dlayers, buf)
        hip_lib.call("sl_conv1d_chain", buf.g[top].data_ptr(), gs, wd, None, masks, ctypes.byref(buf.dgrad_geom[top]),
                     len(dlayers), _lib.EPI_RELU_MASK, _lib.SL_BF16, st)
        torch.cuda.synchronize()
    for i, ref in zip(layers, y_ref):
        assert torch.equal(buf.y[i], ref), ("activation of layer", i)
    for i, ref in zip(dlayers, g_ref):
        assert torch.equal(buf.g[i - 1], ref), ("input gradient of layer", i)
    t_out = buf.t_out
    for i in layers:  # float64 on the stored (exact bf16) input, padded lanes and the ones channel included
        p = eng.plans[i]
        xin = buf.y[i - 1].double()
        w = eng.w_fwd[i].double()                                      # [cout][taps][cin]
        bias = eng.layer_param_views(eng.params, p)[1].double()
        acc = torch.zeros((buf.batch, t_out, p.cout_pad), dtype=torch.float64, device="cuda:0")
        for tap in range(p.spec.kernel_size):
            acc += xin[:, HALO - p.pad_left + tap: HALO - p.pad_left + tap + t_out] @ w[:, tap, :].T
        want = torch.relu(acc + bias).cpu().numpy()
        got = buf.y[i][:, HALO:HALO + t_out].float().cpu().numpy()
        assert rel_l2(got, want) < 3e-3, (i, rel_l2(got, want))


@pytest.mark.parametrize("ranges", [
    [(0, (1 << 20) + 5)],
    [(3, 16384 + 7), (40001, (1 << 20) + 5 - 40001 - 2)],        # two unaligned ranges, a gap between
    [(1, 600 * 16384 + 5)],                                      # 601 chunks: more than the 512 work-groups of 64 CUs
])
def test_squared_norm_under_hints_is_the_same_double(hip_lib, ranges):
    """optimizer.hip sl_grad_sqnorm: the partial-sum grid is min(chunks, 8 x CUs) work-groups that stride over the 16384-float
    chunks; a chunk's partial and the order of the final sum do not depend on the grid, so the result must be the SAME double
    under 64 and 192 CUs as at 256, within 1e-12 of float64 (test_squared_norm_reduction_matches_float64_and_repeats_bit_for_bit).
    (1 << 20) + 5 floats are 65 chunks -- one work-group each under every setting; the last case has 601 chunks, which
    64 CUs (512 work-groups, the formula restated: no query shows the grid) cover in two passes and 256 CUs in one."""
    import torch
    from test_gpu_optimizer_clip import run_sqnorm
    n = max(o_ + c for o_, c in ranges) + 3
    rng = np.random.RandomState(n % 1000)
    x = (rng.randn(n) * 10.0 ** rng.uniform(-20, 3, size=n)).astype(np.float32)
    dev = torch.tensor(x, device="cuda:0")
    want = sum(np.sum(x[o_:o_ + c].astype(np.float64) ** 2) for o_, c in ranges)
    base, _ = run_sqnorm(hip_lib, dev, ranges)
    assert abs(base - want) <= 1e-12 * want
    for cus in (64, 192):
        with hinted(hip_lib, cus):
            got, _ = run_sqnorm(hip_lib, dev, ranges)
            again, _ = run_sqnorm(hip_lib, dev, ranges)
        assert got.tobytes() == again.tobytes() == base.tobytes(), (cus, got, base)


# ============================================================================================ 3. the training step
@pytest.fixture(scope="module")
def rccl():
    """one rank, the real RCCL backend (as test_data_parallel_step_through_rccl_single_rank)"""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29541")
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl", rank=0, world_size=1)
    yield
    if created:
        dist.destroy_process_group()


_ORACLE = {}


def _oracle(case, key, mirror=False):
    k = (key, mirror)
    if k not in _ORACLE:
        args = (case["labels"], case["prediction_lengths"], case["label_lengths"])
        if mirror:
            _ORACLE[k] = o.loss_and_gradients(case["ospecs"], case["weights"], case["x"], *args, bf16_mirror=True)
        else:
            _ORACLE[k] = o.loss_and_gradients(case["ospecs"], weights64(case), case["x"].astype(np.float64), *args)
    return _ORACLE[k]


def _train(eng, case, reducer=None):
    return eng.train_step(case["x"], case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]),
                          reducer).cpu().numpy().copy()


def _reducer(eng, comm_cus, probes=None, lib=None, **kw):
    """GradBucketReducer(force=True, comm_cus=...) whose reduce_bucket also records the calling thread's setting (nt_split_k)"""
    from speechless_amd.parallel import GradBucketReducer
    red = GradBucketReducer(eng.grads, eng.bucket_ranges(), force=True, comm_cus=comm_cus, **kw)
    if probes is not None:
        inner = red.reduce_bucket
        red.reduce_bucket = lambda b, inner=inner: (probes.append((b, nt_split_k(lib))), inner(b))[1]
    return red


def _distances(grads, ref):
    return {i: (rel_l2(dw, rw), rel_l2(db, rb)) for i, ((dw, db), (rw, rb)) in enumerate(zip(grads, ref["grads"]))}


def _flat(grads):
    return np.concatenate([np.concatenate([w.ravel(), b.ravel()]) for w, b in grads]).astype(np.float64)


def _assert_against_float64(dtype, case, key, losses, grads, label):
    """loss and every gradient tensor against the float64 oracle at the bounds the suite already asserts for `dtype`:
    f32: test_loss_and_gradients_f32; bf16: test_loss_and_gradients_bf16 (no noisier than the storage scheme itself: 1.5 x the
    distance of the oracle's own bf16 mirror + 2e-3 -- bf16 gradients at random init do not meet 1e-3);
    bf16x3: test_bf16x3_loss_and_gradients_against_the_float64_oracle; f16x3: its f16x3 twin."""
    ref = _oracle(case, key)
    names = [s.name for s in case["specs"]]
    dist = _distances(grads, ref)
    if dtype == "bf16":
        mirror = _oracle(case, key, mirror=True)
        np.testing.assert_allclose(losses, ref["losses"], rtol=1e-3)
        for i, name in enumerate(names):
            scheme_w = rel_l2(mirror["grads"][i][0], ref["grads"][i][0])
            scheme_b = rel_l2(mirror["grads"][i][1], ref["grads"][i][1])
            assert dist[i][0] < 1.5 * scheme_w + 2e-3 and dist[i][1] < 1.5 * scheme_b + 2e-3, (label, name, dist[i], scheme_w)
    else:
        np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5)
        for i, name in enumerate(names):
            if dtype == "f32":
                bw = bb = 1e-4
            elif dtype == "bf16x3":
                bw = bb = 5e-3
            else:
                bw, bb = (2e-3 if name == "striding_conv" else 1e-3), 1e-3
            assert dist[i][0] < bw and dist[i][1] < bb, (label, name, dist[i])
    return rel_l2(_flat(grads), _flat(ref["grads"]))


def _ws_decisions(eng, lib, cus):
    """(NT workspace of big_conv_1's input gradient, weight-gradient workspaces per layer) of the engine's own geometries"""
    buf, first = eng.cur, eng.frozen_layer_count
    with hinted(lib, cus):
        big1 = [p.index for p in eng.plans if p.spec.name == "big_conv_1"][0]
        nt = lib.raw("sl_conv1d_nt_workspace_bytes")(ctypes.byref(buf.dgrad_geom[big1]), eng.dtype_code, 0)
        wg = [lib.raw("sl_conv1d_wgrad_workspace_bytes")(ctypes.byref(buf.wgrad_geom[p.index]), eng.dtype_code, 0)
              for p in eng.plans[first:]]
    return nt, wg


@pytest.mark.parametrize("dtype,comm_cus,b,t", [("bf16", 128, 20, 96), ("bf16x3", 128, 20, 96), ("f16x3", 128, 20, 96),
                                               ("bf16", 32, 30, 96), ("f32", 32, 3, 64)])
def test_hinted_training_step_against_the_float64_oracle(hip_lib, rccl, dtype, comm_cus, b, t):
    """One data-parallel step (world of one, RCCL) with GradBucketReducer(comm_cus=c): 2048 padded channels x 32 taps put
    big_conv_1's input gradient on split-K 8 for up to 32 tiles at 256 CUs; 20 utterances x 48 frames drop to 4 (6 on the
    plane paths' 3 x 2048 channels) at 128 CUs, 30 utterances at 224 CUs, and big_conv_2's weight gradient changes its batch
    split -- asserted through the workspace queries on the engine's own geometries.  From bucket 1 on the launches are enqueued
    under 256 - c (probed inside reduce_bucket).  The hinted step's loss and gradients are held to the float64 oracle at the
    dtype's existing bounds (_assert_against_float64); its distance to the unhinted step is recorded, not bounded.
    f32 is the control (the shape of test_loss_and_gradients_f32, whose 1e-4 it is held to): no chooser of that path reads the
    hint, the step must equal the unhinted one bit for bit.
    The three distances (flat gradient rel-L2) are printed, go into the parity report and are tabulated in DESIGN.md section 5."""
    import torch
    case = make_case(b=b, t=t, seed=5)
    key = ("step", b, t)
    plain = make_engine(case, dtype)
    loss0 = _train(plain, case)
    g0 = plain.get_gradients()
    eng = make_engine(case, dtype)
    probes = []
    red = _reducer(eng, comm_cus, probes, hip_lib)
    loss1 = _train(eng, case, red)
    torch.cuda.synchronize()
    g1 = eng.get_gradients()
    assert eng.comm_cus == comm_cus and eng._cu_hint_active == 0 and nt_split_k(hip_lib) == 6
    nb = len(eng.bucket_plan())
    assert probes == [(0, 6)] + [(i, 3) for i in range(1, nb)], probes   # bucket 0 closes unhinted, the rest under 256 - c
    if dtype == "f32":
        assert np.array_equal(loss0, loss1) and all(np.array_equal(a, c) and np.array_equal(bb, d)
                                                    for (a, bb), (c, d) in zip(g0, g1))
    else:
        nt0, wg0 = _ws_decisions(eng, hip_lib, 0)
        nt1, wg1 = _ws_decisions(eng, hip_lib, 256 - comm_cus)
        print("big_conv_1 dgrad split-K workspace {} -> {}; wgrad workspaces {} -> {}".format(nt0, nt1, wg0, wg1))
        assert nt0 > nt1 > 0, (nt0, nt1)
        assert wg0 != wg1, (wg0, wg1)
    d_hint = _assert_against_float64(dtype, case, key, loss1, g1, "hinted")
    d_plain = _assert_against_float64(dtype, case, key, loss0, g0, "unhinted")
    d_between = rel_l2(_flat(g1), _flat(g0))
    line = "hinted vs unhinted {:.3g}, hinted vs float64 {:.3g}, unhinted vs float64 {:.3g}".format(d_between, d_hint, d_plain)
    print(dtype, "comm_cus", comm_cus, "b", b, line)
    _report("cu_hint_grad_rel_l2_{}_c{}_b{}".format(dtype, comm_cus, b),
            dict(hinted_vs_unhinted=d_between, hinted_vs_float64=d_hint, unhinted_vs_float64=d_plain))
    assert np.isfinite(d_between), line


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3", "f16x3"])
def test_hinted_steps_through_launch_lists_equal_eager_steps(hip_lib, rccl, dtype):
    """The hint is a recorded op of a launch list: three hinted steps recorded / replayed train bit for bit like eager ones
    (as test_recorded_launch_lists_train_exactly_like_the_eager_path), and every replayed step sets and clears it."""
    import torch
    case = make_case(b=4, t=96, seed=5)
    results = []
    for use_lists in (True, False):
        eng = make_engine(case, dtype, lr=1e-3)
        eng.use_launch_lists = use_lists
        probes = []
        red = _reducer(eng, 32, probes, hip_lib)
        losses = [_train(eng, case, red) for _ in range(3)]
        torch.cuda.synchronize()
        nb = len(eng.bucket_plan())
        assert probes == ([(0, 6)] + [(i, 3) for i in range(1, nb)]) * 3, probes
        assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0
        if use_lists:
            assert eng.cur.launch_lists, "nothing was recorded"
        results.append((np.stack(losses), eng.params.clone()))
    assert np.array_equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])
    assert (results[0][0][2] != results[0][0][0]).any()


def _plain_twin_step(control, eng, case):
    """the same plain step on `control` (an engine that never saw a hint) from eng's weights: (loss, gradients) of both"""
    import torch
    control.set_weights(eng.get_weights())
    out = []
    for e in (control, eng):
        e.load_input(case["x"])
        e.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        e.set_comm_cus(0)
        e.forward(training=True)
        loss = e.ctc().cpu().numpy().copy()
        e.backward()
        torch.cuda.synchronize()
        out.append((loss, e.grads.clone()))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_plain_and_hinted_steps_alternate_on_one_engine(hip_lib, rccl, dtype):
    """plain, comm_cus = 32, plain, comm_cus = 128 ... at two batch lengths on ONE engine: set_comm_cus re-sizes the existing
    buffer sets and drops their launch lists; every step succeeds (a library error raises), the setting is back at 0 after each,
    and forward + backward of the plain steps equal, bit for bit, the same pass on an engine that never saw a hint."""
    import torch
    cases = {t: make_case(b=20, t=t, seed=40 + t) for t in (96, 600)}  # (two buffer sets: 48 and 300 output frames)
    eng = make_engine(cases[96], dtype)
    control = make_engine(cases[96], dtype)
    sequence = [(0, 96), (32, 96), (0, 600), (128, 600), (0, 96), (128, 96), (32, 600), (0, 600), (32, 96)]
    for comm_cus, t in sequence:
        case = cases[t]
        if comm_cus:
            loss = _train(eng, case, _reducer(eng, comm_cus))
            assert eng.comm_cus == comm_cus
        else:
            (lc, gc), (le, ge) = _plain_twin_step(control, eng, case)
            assert np.array_equal(lc, le) and torch.equal(gc, ge), (comm_cus, t)
            loss = _train(eng, case)
            assert eng.comm_cus == 0
        torch.cuda.synchronize()
        assert np.isfinite(loss).all()
        assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0, (comm_cus, t)


@pytest.mark.parametrize("dtype", ["bf16", "bf16x3"])
def test_hint_is_cleared_when_a_bucket_callback_raises(hip_lib, dtype):
    """Engine.backward(on_bucket_ready=...) with a Python callback that throws at bucket 0 and at the last bucket -- on the
    eager path, while a launch list is being recorded and while one is replayed: the calling thread's setting and the engine's
    record of it are back at 0, and the next plain pass equals the control's bit for bit.  set_comm_cus rejects 129 and -1."""
    import torch
    case = make_case(b=4, t=96, seed=5)
    eng = make_engine(case, dtype)
    control = make_engine(case, dtype)
    with pytest.raises(ValueError):
        eng.set_comm_cus(129)
    with pytest.raises(ValueError):
        eng.set_comm_cus(-1)
    assert eng.comm_cus == 0
    nb = len(eng.bucket_plan())

    def backward(callback):
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        eng.set_comm_cus(32)
        eng.forward(training=True)
        eng.ctc()
        eng.backward(on_bucket_ready=callback)

    for use_lists, replay in ((False, False), (True, False), (True, True)):
        eng.use_launch_lists = use_lists
        for at in (0, nb - 1):
            seen = []
            if replay:  # a complete recorded backward first: the raising one replays it
                eng.cur.launch_lists.clear()
                backward(seen.append)
                assert seen == list(range(nb)) and nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0
                assert eng.cur.launch_lists, "nothing was recorded"
                del seen[:]

            def boom(b, at=at, seen=seen):
                seen.append((b, nt_split_k(hip_lib)))
                if b == at:
                    raise RuntimeError("bucket {} failed".format(b))

            with pytest.raises(RuntimeError, match="bucket {} failed".format(at)):
                backward(boom)
            torch.cuda.synchronize()
            assert seen == [(0, 6)] + [(i, 3) for i in range(1, at + 1)], (use_lists, replay, at, seen)
            assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0, (use_lists, replay, at)
            (lc, gc), (le, ge) = _plain_twin_step(control, eng, case)
            assert np.array_equal(lc, le) and torch.equal(gc, ge), (use_lists, replay, at)
            assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0


def test_split_top_step_under_a_hint_against_the_whole_batch_step(hip_lib, rccl):
    """engine_split.py sizes the parts' NT workspace through _max_over_cu_hints: the split-top step under comm_cus = 32 at the
    smallest shape of test_split_top_step_against_the_whole_batch_step, against the whole-batch step under the same hint at
    that test's tolerances (losses 2e-5, gradients 5e-3)."""
    import torch
    case = make_case(b=2, t=64, seed=22)
    res = {}
    for split in (False, True):
        eng = make_engine(case, "bf16", lr=0.0)  # (every step the same pass: the weights do not move)
        eng.split_top, eng.split_min_tiles = split, 0
        eng.load_input(case["x"])
        eng.set_labels(case["labels"], np.array(case["label_lengths"]), np.array(case["prediction_lengths"]))
        probes = []
        red = _reducer(eng, 32, probes, hip_lib)
        for step in range(3):  # the first builds the buffers; then recorded and replayed
            loss = eng.train_step_resident(red).cpu().numpy().copy()
            torch.cuda.synchronize()
            assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0
            if step:
                assert eng.split_top_plan(eng.cur) == (1 if split else 0)
            res[split] = (loss, eng.grads.clone())
        assert [p for p in probes if p[0] > 0] and all(k == (6 if b_ == 0 else 3) for b_, k in probes), probes
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=2e-5)
    err = float(torch.linalg.norm(res[True][1] - res[False][1]) / torch.linalg.norm(res[False][1]))
    assert err < 5e-3, err


@pytest.mark.parametrize("dtype,option", [("bf16", "split_last_bucket"), ("bf16x3", "shard_optimizer"),
                                          ("bf16", "shard_optimizer")])
def test_optional_data_parallel_paths_under_a_hint(hip_lib, rccl, dtype, option):
    """split_last_bucket = True and shard_optimizer = True, one hinted step each (comm_cus = 128): loss and gradients against
    the float64 oracle at the dtype's existing bounds, like their unhinted twins; the distance between the two is recorded."""
    import torch
    case = make_case(b=3, t=64, seed=5)
    out = {}
    for comm_cus in (0, 128):
        eng = make_engine(case, dtype)
        eng.split_last_bucket = option == "split_last_bucket"
        probes = []
        red = _reducer(eng, comm_cus, probes, hip_lib, shard_optimizer=option == "shard_optimizer")
        loss = _train(eng, case, red)
        torch.cuda.synchronize()
        nb = len(eng.bucket_plan())
        assert nb == (4 if (option == "split_last_bucket" or dtype != "bf16") else 3)
        assert probes == [(i, 3 if (comm_cus and i) else 6) for i in range(nb)], probes
        assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0
        out[comm_cus] = (loss, eng.get_gradients())
        _assert_against_float64(dtype, case, ("optional", 3), loss, out[comm_cus][1], "{} comm_cus {}".format(option, comm_cus))
    print(dtype, option, "hinted vs unhinted", rel_l2(_flat(out[128][1]), _flat(out[0][1])))


def test_hinted_step_with_a_front_layer_against_the_float64_oracle(hip_lib, rccl):
    """An engine with a front_plan (raw-wave input: wave_conv in front of the stack) on the bf16x3 path: the front layer's
    launches close the last bucket and run under 256 - comm_cus, their workspaces sized for every setting in use.  One hinted
    step (comm_cus = 128) against the float64 oracle at the bounds of test_raw_wave_bf16x3_elu_against_the_float64_oracle
    (ELU: no decisions to flip; loss 2e-5, every gradient 2e-4)."""
    import torch
    from test_gpu_round4 import _wave_case
    from test_gpu_round5 import _wave_engine
    case = _wave_case(activation="elu")
    eng = _wave_engine(case, "bf16x3")
    assert eng.front_plan is not None
    probes = []
    red = _reducer(eng, 128, probes, hip_lib)
    loss = _train(eng, case, red)
    torch.cuda.synchronize()
    nb = len(eng.bucket_plan())
    assert eng.bucket_plan()[-1][0] == [eng.front_plan.index]
    assert probes == [(0, 6)] + [(i, 3) for i in range(1, nb)], probes
    assert nt_split_k(hip_lib) == 6 and eng._cu_hint_active == 0
    ref = o.loss_and_gradients(case["ospecs"], weights64(case), case["x"].astype(np.float64), case["labels"],
                               case["prediction_lengths"], case["label_lengths"])
    np.testing.assert_allclose(loss, ref["losses"], rtol=2e-5)
    errs = [max(rel_l2(dw, rw), rel_l2(db, rb)) for (dw, db), (rw, rb) in zip(eng.get_gradients(), ref["grads"])]
    assert max(errs) < 2e-4, errs
