"""The elementwise plane kernels (csrc/split3.hip: both formats, every activation / mask / dropout mode, input and weight
packing, the weight-gradient combine, the bias gradient) and their single-plane twins (csrc/misc.hip) against the numpy model
of tests/plane_ref.py, bit for bit (run with -m gpu on an MI355X).  Destinations are filled with a sentinel and hold spare
rows; everything outside the written rows must still be the sentinel.  NaNs are compared as NaNs, not by payload.

Not pinned here: what a NaN becomes in ReLU (fmaxf: mode 1, EPI_BIAS_RELU) and in ELU.  That belongs to the work on non-finite
values as a whole; this module only holds the plane CONVERSION to "NaN in, NaN out"."""
import ctypes

import numpy as np
import pytest

import plane_ref as pr

pytestmark = pytest.mark.gpu

S = pr.SENTINEL
ROW0, SPARE = 3, 2  # first written row of an utterance; rows left over behind the last one


def _name(fmt, tail=""):
    return ("sl_split3" if fmt == "bf16" else "sl_splitf16") + tail


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint16)


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _plane_buffer(batch, t_out, c, rows_value=None):
    """uint16 (batch, ROW0 + t_out + SPARE, 3 c) of sentinels, the rows ROW0 .. ROW0 + t_out - 1 set to rows_value"""
    a = np.full((batch, ROW0 + t_out + SPARE, 3 * c), S, dtype=np.uint16)
    if rows_value is not None:
        a[:, ROW0:ROW0 + t_out] = rows_value
    return a


def _assert_planes(got, want, fmt, what, zeros=False):
    got, want = pr.canonical(got, fmt), pr.canonical(want, fmt)
    if zeros:
        got, want = pr.zeros_by_value(got), pr.zeros_by_value(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        i = tuple(bad[0])
        raise AssertionError("{}: {} of {} words differ, first at {}: got {:#06x}, want {:#06x}".format(
            what, len(bad), got.size, i, int(got[i]), int(want[i])))


def _outside_is_sentinel(full, t_out):
    return (full[:, :ROW0] == S).all() and (full[:, ROW0 + t_out:] == S).all()


def _mask_values(shape, fmt, seed):
    """stored activations for the mask modes: edge and random values (shifted against the input's edge values so that the
    pairs differ), with +0, -0 and the smallest positive number of the format among them"""
    y = np.roll(pr.fill_values(shape, fmt, seed).reshape(-1), 5)
    tiny = 2.0 ** -24 if fmt == "f16" else 2.0 ** -133
    special = np.array([0.0, -0.0, tiny, -tiny, 0.5], dtype=np.float32)
    n = min(y.size, 45)
    y[-n:] = np.tile(special, 9)[:n]  # (period 5: all lanes)
    return y.reshape(shape)


def _run_split(lib, fmt, mode, v, mask_rows=None):
    """v float32 (batch, t_out, c) through sl_split3 / sl_splitf16 with spare source rows (src_batch_stride > t_out * c), ROW0
    and spare destination rows: (the whole destination, its written rows)"""
    import torch
    batch, t_out, c = v.shape
    src = np.full((batch, t_out + 2, c), np.nan, dtype=np.float32)
    src[:, :t_out] = v
    d_src, d_dst = _dev(src), _dev(_plane_buffer(batch, t_out, c))
    d_mask = _dev(_plane_buffer(batch, t_out, c, mask_rows)) if mask_rows is not None else None
    lib.call(_name(fmt), d_src.data_ptr(), d_dst.data_ptr(), d_mask.data_ptr() if d_mask is not None else None, batch, t_out, c,
             d_src.stride(0), ROW0, d_dst.stride(0), mode, _stream())
    torch.cuda.synchronize()
    full = _bits(d_dst)
    return full, full[:, ROW0:ROW0 + t_out]


SPLIT_SHAPES = [(1, 1, 8), (2, 37, 24), (3, 5, 256), (2, 129, 64)]


# ------------------------------------------------------------------------------------------ split
@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=str)
@pytest.mark.parametrize("mode", [0, 1, 3, 4])
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_split_modes_are_bit_exact(hip_lib, fmt, mode, shape):
    """modes 0 (none), 1 (ReLU; zeros by value), 3 (ReLU mask: the stored hi plane), 4 (ELU mask: hi + lo) on edge and random
    values; the last shape spans two blocks with a partial second one"""
    v = pr.fill_values(shape, fmt, seed=sum(shape) + mode)
    mask = pr.split(_mask_values(shape, fmt, seed=7 + mode), fmt) if mode >= 3 else None
    full, got = _run_split(hip_lib, fmt, mode, v, mask)
    _assert_planes(got, pr.act_split(v, mode, mask, fmt), fmt, "{} mode {} {}".format(fmt, mode, shape), zeros=mode == 1)
    assert _outside_is_sentinel(full, shape[1])
    if mode >= 3 and v.size > 500:  # both branches of the mask were taken
        y = pr.planes_value(mask, shape[2], fmt)
        assert (y > 0).mean() > 0.2 and (y <= 0).mean() > 0.2


def _ulp_key(x):
    i = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=str)
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_split_elu_mode_within_k_ulps(hip_lib, fmt, shape, capsys):
    """mode 2: bit-exact where v > 0; where v <= 0 the stored pair is split_planes(c) of a float32 c within k ulps of
    float32(expm1(float64 v)).  k = (the distance of the host libm's float32 expm1 from that reference on these inputs) + 2
    for the device libm being another implementation, and k <= 4 is asserted.

    Measured: numpy's float32 expm1 is 2 ulps from the reference on these inputs (0.7 % of the elements, |v| around 0.01;
    0 on the eight elements of the smallest shape), so k = 4 (k = 2 there); every pair the kernel stores on an MI355X is
    matched at a distance of at most 1 ulp, in both formats and all four shapes.  Each run prints its figures."""
    v = pr.fill_values(shape, fmt, seed=sum(shape) + 2)
    v = np.where(np.isnan(v), np.float32(-1), v)
    full, got = _run_split(hip_lib, fmt, 2, v)
    assert _outside_is_sentinel(full, shape[1])
    c = shape[2]
    center = pr.act_value(v, 2)
    neg = ~(v > 0)
    with np.errstate(all="ignore"):
        host = np.expm1(v.astype(np.float32)).astype(np.float32)
    host_dist = int(np.abs(_ulp_key(host) - _ulp_key(center))[neg].max()) if neg.any() else 0
    k = host_dist + 2
    assert k <= 4, host_dist
    want = pr.split(center, fmt)
    pos = np.concatenate([~neg] * 3, axis=-1)
    _assert_planes(np.where(pos, got, 0), np.where(pos, want, 0), fmt, "{} mode 2 {} where v > 0".format(fmt, shape))
    assert np.array_equal(got[..., :c], got[..., 2 * c:])
    dist = np.full(v.shape, 99, dtype=np.int64)
    for d in sorted(range(-k, k + 1), key=abs, reverse=True):
        cand = pr.canonical(pr.split(pr.step_ulps(center, d), fmt), fmt)
        g = pr.canonical(got, fmt)
        hit = (cand[..., :c] == g[..., :c]) & (cand[..., c:2 * c] == g[..., c:2 * c])
        dist[hit] = abs(d)
    worst = int(dist[neg].max()) if neg.any() else 0
    with capsys.disabled():
        print("\n[elu {} {}] host libm {} ulp, k = {}, kernel matched within {} ulp".format(fmt, shape, host_dist, k, worst))
    assert worst <= k, (worst, k, v[neg & (dist > k)][:8])


# ------------------------------------------------------------------------------------------ dropout
DROP_SHAPES = [(1, 8), (37, 24), (300, 256)]
RATES = (0.0, 0.25, 0.9)
SEEDS = (5, 2 ** 63 + 12345)


def _run_dropout(lib, fmt, src_planes, y_planes, c, mode, rate, seed, in_place):
    import torch
    rows = src_planes.shape[0]
    buf = np.full((rows + SPARE, 3 * c), S, dtype=np.uint16)
    d_dst = _dev(buf)
    if in_place:
        d_dst[:rows] = _dev(src_planes)
        d_src = d_dst
    else:
        d_src = _dev(src_planes)
    d_y = _dev(y_planes) if y_planes is not None else None
    lib.call(_name(fmt, "_dropout"), d_src.data_ptr(), d_dst.data_ptr(), d_y.data_ptr() if d_y is not None else None, rows, c,
             mode, rate, seed, _stream())
    torch.cuda.synchronize()
    full = _bits(d_dst)
    assert (full[rows:] == S).all()
    return full[:rows]


@pytest.mark.parametrize("shape", DROP_SHAPES, ids=str)
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_dropout_modes(hip_lib, fmt, mode, shape):
    """modes 0 (forward) and 1 (scale) bit-exact, mode 2 (ELU backward) equal to the fused or to the unfused candidate of
    m * keep_prob + 1 element by element; rates 0 / 0.25 / 0.9, a seed above 2^63; in place (as the engine calls it) and out of
    place agree bit for bit; rate 0 returns the input wherever re-splitting hi + lo does; the zero pattern of mode 0 is the
    complement of the keep decisions"""
    rows, c = shape
    if mode == 2:
        src, y = pr.mode2_inputs(rows, c, fmt)
    else:
        src, y = pr.split(pr.fill_values(shape, fmt, seed=rows + mode), fmt), None
    for rate in RATES:
        for seed in SEEDS:
            what = "{} mode {} {} rate {} seed {}".format(fmt, mode, shape, rate, seed)
            got = _run_dropout(hip_lib, fmt, src, y, c, mode, rate, seed, in_place=False)
            again = _run_dropout(hip_lib, fmt, src, y, c, mode, rate, seed, in_place=True)
            assert np.array_equal(got, again), what + ": in place differs from out of place"
            fused, unfused = pr.dropout_planes(src, y, c, mode, rate, seed, fmt)
            assert np.array_equal(got[:, :c], got[:, 2 * c:]), what
            if mode < 2:
                _assert_planes(got, fused, fmt, what)
            else:
                g, a, b = pr.canonical(got, fmt), pr.canonical(fused, fmt), pr.canonical(unfused, fmt)
                is_a = (g[:, :c] == a[:, :c]) & (g[:, c:2 * c] == a[:, c:2 * c])
                is_b = (g[:, :c] == b[:, :c]) & (g[:, c:2 * c] == b[:, c:2 * c])
                assert (is_a | is_b).all(), (what, int((~(is_a | is_b)).sum()), np.argwhere(~(is_a | is_b))[:4].tolist())
            if rate == 0.0 and mode < 2:
                same = fused == src  # (not where hi + lo is no number: bf16 planes of +-inf and of 3.4e38)
                assert (same.mean() > 0.9 or src.size < 500) and np.array_equal(got[same], src[same]), what
            if mode == 0:
                keep = pr._dropout_keep(seed, rows * c, rate).reshape(rows, c)
                kept_value = pr.dropout_planes(src, None, c, 1, rate, seed, fmt)[0]
                nonzero = ((kept_value[:, :c] & 0x7FFF) != 0) | ((kept_value[:, c:2 * c] & 0x7FFF) != 0)
                is_zero = (got[:, :c] == 0) & (got[:, c:2 * c] == 0)
                assert np.array_equal(is_zero[nonzero], ~keep[nonzero]), what
                assert nonzero.mean() > 0.5 or rows * c < 64


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_dropout_keeps_zero_rows_at_plus_zero(hip_lib, fmt):
    """x = +0 stays +0 in all three planes in every mode: kept (0 * scale, 0 * slope with the slope of a stored ELU output,
    m >= -1 / keep_prob, never negative) and dropped"""
    rows, c = 5, 24
    zeros = np.zeros((rows, 3 * c), dtype=np.uint16)
    rng = np.random.RandomState(3)
    m = -rng.rand(rows, c).astype(np.float32)  # above -1: a possible ELU output at every rate
    m.reshape(-1)[::3] = 0.75
    m.reshape(-1)[1::7] = -1.0
    y = pr.split(m, fmt)
    for mode in (0, 1, 2):
        for rate in RATES:
            got = _run_dropout(hip_lib, fmt, zeros, y if mode == 2 else None, c, mode, rate, SEEDS[1], in_place=True)
            assert not got.any(), (fmt, mode, rate)


@pytest.mark.parametrize("shape", DROP_SHAPES, ids=str)
def test_a_seed_draws_the_same_mask_on_every_path(hip_lib, shape):
    """sl_split3_dropout, sl_splitf16_dropout and sl_dropout (float32 and bf16 storage) on the same logical tensor of ones drop
    exactly the same elements: those the model drops"""
    import torch
    from speechless_amd import _lib
    rows, c = shape
    ones = np.ones((rows, c), dtype=np.float32)
    for rate in (0.25, 0.9):
        for seed in SEEDS:
            dropped = ~pr._dropout_keep(seed, rows * c, rate).reshape(rows, c)
            for fmt in pr.FORMATS:
                got = _run_dropout(hip_lib, fmt, pr.split(ones, fmt), None, c, 0, rate, seed, in_place=False)
                assert np.array_equal((got[:, :c] == 0) & (got[:, c:2 * c] == 0), dropped), (fmt, rate, seed)
            for code, data in ((_lib.SL_F32, ones), (_lib.SL_BF16, pr._round_bf16(ones)[1])):
                d_src = _dev(data)
                d_dst = torch.full_like(d_src, 7)
                hip_lib.call("sl_dropout", d_src.data_ptr(), d_dst.data_ptr(), rows * c, code, rate, seed, _stream())
                torch.cuda.synchronize()
                assert np.array_equal(d_dst.cpu().numpy().reshape(rows, c) == 0, dropped), (code, rate, seed)


# ------------------------------------------------------------------------------------------ misc.hip's single-plane twins
def _canon32(a):
    a = np.array(a, dtype=np.float32)
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.uint32)


def _same_stored(got, want, storage):
    if storage == "bf16":
        return pr.canonical(got, "bf16") == pr.canonical(want, "bf16")
    return _canon32(got) == _canon32(want)


@pytest.mark.parametrize("n", [1, 3, 1023, 1025, 4100])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_single_plane_twins(hip_lib, storage, n):
    """sl_dropout, sl_scale and sl_elu_dropout_backward on float32 and bf16 tensors of n elements (a thread takes 4, a block
    1024): bit-exact against the model, the ELU backward against either candidate of m * keep_prob + 1; the elements behind n
    are untouched"""
    import torch
    from speechless_amd import _lib
    code = _lib.SL_F32 if storage == "f32" else _lib.SL_BF16
    tail = 8
    x = pr.fill_values((n + tail,), "bf16", seed=n)
    m = _mask_values((n + tail,), "bf16", seed=n + 1)
    m[1::3] = -np.abs(np.random.RandomState(n).rand(len(m[1::3]))).astype(np.float32) / np.float32(0.75)
    if storage == "bf16":
        x, m = pr._round_bf16(x)[1], pr._round_bf16(m)[1]
    guard = x[n:].copy()
    st = _stream()
    for rate, seed in ((0.25, SEEDS[0]), (0.9, SEEDS[1]), (0.0, SEEDS[1])):
        what = (storage, n, rate, seed)
        d_src, d_dst = _dev(x), _dev(x)
        d_dst[:n] = 0
        hip_lib.call("sl_dropout", d_src.data_ptr(), d_dst.data_ptr(), n, code, rate, seed, st)
        d_g, d_y = _dev(x), _dev(m)
        hip_lib.call("sl_elu_dropout_backward", d_g.data_ptr(), d_y.data_ptr(), n, code, rate, seed, st)
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy().view(x.dtype)
        assert _same_stored(got[:n], pr.dropout_single(x[:n], rate, seed, storage), storage).all(), what
        assert np.array_equal(got[n:], guard), what
        got = d_g.cpu().numpy().view(x.dtype)
        a, b = pr.elu_dropout_backward_single(x[:n], m[:n], rate, seed, storage)
        ok = _same_stored(got[:n], a, storage) | _same_stored(got[:n], b, storage)
        assert ok.all(), (what, np.argwhere(~ok)[:4].tolist())
        assert np.array_equal(got[n:], guard), what
    for scale in (2.0 ** -7, 1.0 / 0.75):
        d_x = _dev(x)
        hip_lib.call("sl_scale", d_x.data_ptr(), n, code, scale, st)
        torch.cuda.synchronize()
        got = d_x.cpu().numpy().view(x.dtype)
        assert _same_stored(got[:n], pr.scale_single(x[:n], scale, storage), storage).all(), (storage, n, scale)
        assert np.array_equal(got[n:], guard)


# ------------------------------------------------------------------------------------------ packing
@pytest.mark.parametrize("batch,t_in,f,c", [(1, 7, 5, 8), (2, 33, 161, 192), (2, 9, 64, 64)])
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_pack_input(hip_lib, fmt, batch, t_in, f, c):
    """float32 (B, t_in, f) -> planes of c >= f channels at ROW0: bit-exact, the channels >= f zero in all three planes"""
    import torch
    x = pr.fill_values((batch, t_in, f), fmt, seed=t_in + f)
    d_x, d_dst = _dev(x), _dev(_plane_buffer(batch, t_in, c))
    hip_lib.call(_name(fmt, "_pack_input"), d_x.data_ptr(), d_dst.data_ptr(), batch, t_in, f, c, ROW0, d_dst.stride(0), _stream())
    torch.cuda.synchronize()
    full = _bits(d_dst)
    got = full[:, ROW0:ROW0 + t_in]
    _assert_planes(got, pr.pack_input_planes(x, c, fmt), fmt, "pack_input {}".format((fmt, batch, t_in, f, c)))
    assert _outside_is_sentinel(full, t_in)
    for p in range(3):
        assert not got[..., p * c + f:(p + 1) * c].any()


def _weights(k, cin, cout, seed):
    """randn * 10^U(-6, 1) per output channel, the edge values over the first elements of every tap"""
    rng = np.random.RandomState(seed)
    w = (rng.randn(k, cin, cout) * 10.0 ** rng.uniform(-6, 1, size=cout)).astype(np.float32)
    flat = w.reshape(k, -1)
    flat[:, :len(pr.EDGE_VALUES)] = pr.EDGE_VALUES
    return w


@pytest.mark.parametrize("with_dgrad", [True, False], ids=["dgrad", "fwd_only"])
@pytest.mark.parametrize("k,cin,cout", [(1, 32, 32), (3, 64, 32), (2, 32, 96)])
@pytest.mark.parametrize("fmt,scale", [("bf16", 1.0), ("f16", 1.0), ("f16", 64.0)])
def test_pack_weights(hip_lib, fmt, scale, k, cin, cout, with_dgrad):
    """master (k, cin, cout) -> w_fwd3 [cout][k][hi | hi | lo over cin] and w_dgrad3 [cin][k - 1 - tap][hi | hi | lo over cout]
    of scale * w, bit-exact; without the dgrad copy its buffer is untouched"""
    import torch
    w = _weights(k, cin, cout, seed=k + cin + cout)
    n = k * cin * cout * 3
    d_w = _dev(w)
    d_f, d_d = _dev(np.full(n + 8, S, dtype=np.uint16)), _dev(np.full(n + 8, S, dtype=np.uint16))
    args = (d_w.data_ptr(), d_f.data_ptr(), d_d.data_ptr() if with_dgrad else None, k, cin, cout)
    hip_lib.call(_name(fmt, "_pack_weights"), *args, *((scale,) if fmt == "f16" else ()), _stream())
    torch.cuda.synchronize()
    fwd, dgrad = pr.pack_weights_planes(w, scale, fmt)
    got_f, got_d = _bits(d_f), _bits(d_d)
    what = "pack_weights {}".format((fmt, scale, k, cin, cout))
    _assert_planes(got_f[:n].reshape(fwd.shape), fwd, fmt, what + " forward copy")
    assert (got_f[n:] == S).all()
    if with_dgrad:
        _assert_planes(got_d[:n].reshape(dgrad.shape), dgrad, fmt, what + " dgrad copy")
        assert (got_d[n:] == S).all()
    else:
        assert (got_d == S).all()
    # the model's own layout, spelled out once more: row [hi | hi | lo], taps of the dgrad copy reversed
    with np.errstate(over="ignore"):
        v = (w * np.float32(scale)).astype(np.float32)
    tap, ci, co = k - 1, cin - 3, cout - 5
    hi, lo = pr.split(v[tap, ci, co:co + 1], fmt)[:2]
    assert fwd[co, tap, ci] == hi == fwd[co, tap, cin + ci] and fwd[co, tap, 2 * cin + ci] == lo
    assert dgrad[ci, k - 1 - tap, co] == hi == dgrad[ci, k - 1 - tap, cout + co] and dgrad[ci, k - 1 - tap, 2 * cout + co] == lo


# ------------------------------------------------------------------------------------------ combine and bias gradient
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -7])
@pytest.mark.parametrize("taps,c_in,c_out,frames,fstride,rb_fstride,ra_cin,rb_cin",
                         [(3, 8, 12, 1, 0, 0, 16, 8), (4, 8, 12, 2, 24, 8, 43, 19), (4, 8, 12, 2, 24, 24, 43, 35)])
def test_wgrad_combine_on_integers(hip_lib, taps, c_in, c_out, frames, fstride, rb_fstride, ra_cin, rb_cin, scale):
    """dw = ((hh + hl) + lh) * scale on small integers (every fp32 sum exact: zero tolerance), one and two frames per row, the
    narrower RB window, operand rows longer than the minimum; the unscaled entry point at scale 1"""
    import torch
    rng = np.random.RandomState(taps + frames + rb_fstride)
    ra = rng.randint(-1000, 1001, size=(taps // frames, ra_cin, c_out)).astype(np.float32)
    rb = rng.randint(-1000, 1001, size=(taps // frames, rb_cin, c_out)).astype(np.float32)
    want = pr.wgrad_combine(ra, rb, taps, c_in, c_out, frames, fstride, ra_cin, rb_cin, rb_fstride, scale)
    # the model's index formula against a float64 loop over single elements
    for tap, ci, co in [(0, 0, 0), (taps - 1, c_in - 1, c_out - 1), (taps // 2, 3, 5)]:
        tv, f = divmod(tap, frames)
        s = float(ra[tv, f * fstride + ci, co]) + float(rb[tv, f * rb_fstride + ci, co]) + float(ra[tv, f * fstride + c_in + ci, co])
        assert float(want[tap, ci, co]) == s * scale
    n = taps * c_in * c_out
    entries = [("sl_split3_wgrad_combine_scaled", (scale,))] + ([("sl_split3_wgrad_combine", ())] if scale == 1.0 else [])
    for name, extra in entries:
        d_ra, d_rb = _dev(ra), _dev(rb)
        d_dw = _dev(np.full(n + 8, 12345.0, dtype=np.float32))
        hip_lib.call(name, d_ra.data_ptr(), d_rb.data_ptr(), d_dw.data_ptr(), taps, c_in, c_out, frames, fstride, ra_cin, rb_cin,
                     rb_fstride, *extra, _stream())
        torch.cuda.synchronize()
        got = d_dw.cpu().numpy()
        assert np.array_equal(got[:n].reshape(want.shape), want), name
        assert (got[n:] == 12345.0).all(), name


@pytest.mark.parametrize("batch,t_out,c", [(3, 1, 64), (2, 259, 128)])
@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_bias_gradient_on_integers(hip_lib, fmt, batch, t_out, c):
    """db = scale * sum over the valid frames of (g_hi + g_lo) on integer-valued planes with a non-zero lo plane, against the
    int64 sum with zero tolerance; 259 frames make the chunk loop of 4 x 64 frames wrap; the rows outside [ROW0, ROW0 + t_out)
    hold the sentinel (1.5e16 as bf16, 203.25 as fp16) and must not be read"""
    import torch
    rng = np.random.RandomState(t_out + c)
    wide = 2 ** 12 if fmt == "f16" else 2 ** 10  # beyond the 11 / 8 bits of one plane, within the two
    ints = rng.randint(-wide, wide + 1, size=(batch, t_out, c)).astype(np.int64)
    planes = pr.split(ints.astype(np.float32), fmt)
    assert planes[..., c:2 * c].any()
    rec = pr.planes_to_f32(planes[..., :c], fmt).astype(np.int64) + pr.planes_to_f32(planes[..., c:2 * c], fmt).astype(np.int64)
    assert np.array_equal(rec, ints)
    scale = 2.0 ** -7 if fmt == "f16" else 1.0
    want = ints.reshape(-1, c).sum(axis=0)
    assert np.array_equal(pr.bias_grad(planes, c, scale, fmt), want * scale)
    d_g = _dev(_plane_buffer(batch, t_out, c, planes))
    d_db = _dev(np.full(c + 4, 12345.0, dtype=np.float32))
    ws_bytes = hip_lib.raw("sl_split3_bias_grad_workspace_bytes")(c)
    d_ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    hip_lib.call(_name(fmt, "_bias_grad"), d_g.data_ptr(), d_db.data_ptr(), batch, t_out, c, ROW0, d_g.stride(0),
                 *((scale,) if fmt == "f16" else ()), d_ws.data_ptr(), ws_bytes, _stream())
    torch.cuda.synchronize()
    got = d_db.cpu().numpy()
    assert np.array_equal(got[:c].astype(np.float64), want * scale)
    assert (got[c:] == 12345.0).all()


# ------------------------------------------------------------------------------------------ NaN and inf
def _hi_lo(planes, c):
    return planes[..., :c], planes[..., c:2 * c], planes[..., 2 * c:]


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_nan_stays_nan_and_inf_follows_the_format(hip_lib, fmt):
    """a NaN input gives NaN in the hi AND lo planes on every path that passes a value on (split modes 0 / 3 / 4, dropout modes
    0..2 where kept, input and weight packing), in both formats; +-inf stays +-inf in bf16's hi plane and is clamped to +-65504
    in fp16's hi and lo planes (the documented design)"""
    import torch
    c = 8
    isnan = lambda p: np.isnan(pr.planes_to_f32(p, fmt))  # noqa: E731
    v = np.full((1, 2, c), np.nan, dtype=np.float32)
    v[0, 1, ::2] = -np.nan
    inf = np.tile(np.array([np.inf, -np.inf], dtype=np.float32), c // 2).reshape(1, 1, c)
    mask = pr.split(np.full((1, 2, c), 0.5, dtype=np.float32), fmt)
    for mode in (0, 3, 4):
        _, got = _run_split(hip_lib, fmt, mode, v, mask if mode >= 3 else None)
        assert isnan(got).all(), (fmt, mode, got)
    _, got = _run_split(hip_lib, fmt, 0, inf)
    hi, lo, hi2 = _hi_lo(got[0, 0], c)
    if fmt == "bf16":
        assert hi.tolist() == [0x7F80, 0xFF80] * (c // 2) and np.array_equal(hi, hi2)
    else:
        assert hi.tolist() == [0x7BFF, 0xFBFF] * (c // 2) and np.array_equal(hi, lo) and np.array_equal(hi, hi2)
    # dropout: NaN planes (hi = NaN, lo = NaN, as the split stores them) at rate 0 (all kept) and at 0.25 where kept
    src = pr.split(v[0], fmt)
    y = pr.split(np.array([[0.5] * c, [-0.5] * c], dtype=np.float32), fmt)
    for mode in (0, 1, 2):
        for rate in (0.0, 0.25):
            got = _run_dropout(hip_lib, fmt, src, y if mode == 2 else None, c, mode, rate, 5, in_place=True)
            keep = np.ones((2, c), dtype=bool) if mode == 1 else pr._dropout_keep(5, 2 * c, rate).reshape(2, c)
            hi, lo, hi2 = _hi_lo(got, c)
            assert isnan(hi)[keep].all() and isnan(lo)[keep].all() and isnan(hi2)[keep].all(), (fmt, mode, rate)
            assert not hi[~keep].any() and not lo[~keep].any()
    # input packing
    x = np.full((1, 2, 5), np.nan, dtype=np.float32)
    d_x, d_dst = _dev(x), _dev(_plane_buffer(1, 2, c))
    hip_lib.call(_name(fmt, "_pack_input"), d_x.data_ptr(), d_dst.data_ptr(), 1, 2, 5, c, ROW0, d_dst.stride(0), _stream())
    # weight packing
    w = np.full((1, 32, 32), np.nan, dtype=np.float32)
    d_w, d_f, d_d = _dev(w), _dev(np.zeros(3 * 1024, dtype=np.uint16)), _dev(np.zeros(3 * 1024, dtype=np.uint16))
    hip_lib.call(_name(fmt, "_pack_weights"), d_w.data_ptr(), d_f.data_ptr(), d_d.data_ptr(), 1, 32, 32,
                 *((64.0,) if fmt == "f16" else ()), _stream())
    torch.cuda.synchronize()
    got = _bits(d_dst)[:, ROW0:ROW0 + 2]
    for p in range(3):
        assert isnan(got[..., p * c:p * c + 5]).all() and not got[..., p * c + 5:(p + 1) * c].any(), (fmt, "pack_input")
    assert isnan(_bits(d_f)).all() and isnan(_bits(d_d)).all(), (fmt, "pack_weights")


def test_nan_through_the_nt_epilogue_plane_split():
    """plane_pack_hi / plane_pack_lo of the NT kernels' epilogue: the input-gradient launch of an f16x3 engine's layer 1
    (sl_conv1d_nt, plane output, EPI_RELU_MASK) with ONE NaN planted in the gradient under an all-positive mask.  Every output
    row a tap of the layer carries that element to holds NaN in its hi and lo planes; the rows beyond hold numbers."""
    import torch
    from speechless_amd import _lib
    from test_gpu_exact_ints import _halo, _store_planes
    from test_gpu_parity import make_case, make_engine
    case = make_case()
    eng = make_engine(case, "f16x3")
    buf = eng.load_input(case["x"])
    buf.ensure_backward(eng)
    layer = 1
    p = eng.plans[layer]
    s = p.spec
    t_out, h = buf.t_out, _halo()
    k = s.kernel_size
    assert t_out > 2 * k
    ones_in = eng._has_ones_output(eng.plans[layer - 1])
    _store_planes(eng, buf.y[layer - 1], t_out, np.ones((buf.batch, t_out, s.cin)), ones_in)
    rng = np.random.RandomState(4)
    _store_planes(eng, buf.g[layer], t_out, rng.randint(-1, 2, size=(buf.batch, t_out, s.cout)) * eng.g_scale, False)
    b0, t0, ch0 = 1, t_out // 2, 5
    buf.g[layer][b0, h + t0, ch0] = float("nan")                    # the hi plane (P0) and its copy (P2)
    buf.g[layer][b0, h + t0, 2 * p.cout_pad + ch0] = float("nan")
    buf.g[layer - 1].fill_(3)
    eng.lib.call("sl_conv1d_nt", buf.g[layer].data_ptr(), eng.w_dgrad[layer].data_ptr(), None, buf.y[layer - 1].data_ptr(),
                 buf.g[layer - 1].data_ptr(), ctypes.byref(eng._plane_geom(buf, "dgrad", layer, p.cin_pad)),
                 _lib.EPI_RELU_MASK, eng.dtype_code, 2, 0, buf.nt_ws.data_ptr(), buf.nt_ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = buf.g[layer - 1].float().cpu().numpy()
    cp = p.cin_pad
    hi, lo, hi2 = out[..., :s.cin], out[..., cp:cp + s.cin], out[..., 2 * cp:2 * cp + s.cin]
    nan_rows = np.isnan(hi[b0]).all(axis=1)
    assert nan_rows.sum() == k and nan_rows[t0 + h]                       # the k rows the NaN reaches, all real channels
    assert np.isnan(lo[b0][nan_rows]).all() and np.isnan(hi2[b0][nan_rows]).all()
    assert np.isfinite(hi[b0][~nan_rows]).all() and np.isfinite(lo[b0][~nan_rows]).all()
    other = [b for b in range(buf.batch) if b != b0]
    assert np.isfinite(out[other]).all()
