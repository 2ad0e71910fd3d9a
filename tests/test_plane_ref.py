"""The numpy model of the plane kernels (tests/plane_ref.py) against what DESIGN.md claims of the two formats, so that the model
cannot drift with the kernels it judges (tests/test_gpu_planes.py), and the host-side refusals of the plane entry points and
their single-plane twins (they come before any launch).  No GPU."""
import numpy as np
import pytest

import plane_ref as pr

SL_OK, SL_ERR_INVALID_ARGUMENT, SL_ERR_WORKSPACE_TOO_SMALL = 0, -1, -3


def _in_range(v, fmt):
    """finite values whose two planes are both normal-or-exactly-representable: fp16 |v| <= 65504; bf16 away from fp32's ends
    (hi overflows to inf above 2^127 (2 - 2^-8), lo leaves the normal range below 2^-126 * 2^17)"""
    a = np.abs(v.astype(np.float64))
    if fmt == "f16":
        return np.isfinite(v) & (a <= pr.F16_MAX)
    return np.isfinite(v) & ((a == 0) | ((a >= 2.0 ** -108) & (a <= 3.0e38)))


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_two_planes_reconstruct_the_value(fmt):
    """|hi + lo - v| <= 2^-17 |v| (bf16) and <= max(2^-22 |v|, 2^-25) (fp16) on the GPU tests' inputs, edge values included;
    the third plane equals the first"""
    v = pr.fill_values((4, 37, 64), fmt, seed=1)
    planes = pr.split(v, fmt)
    c = v.shape[-1]
    assert planes.shape == (4, 37, 3 * c) and planes.dtype == np.uint16
    assert np.array_equal(planes[..., :c], planes[..., 2 * c:])
    ok = _in_range(v, fmt)
    assert ok.sum() > 0.8 * v.size and (~ok).sum() > 0
    with np.errstate(invalid="ignore"):  # (inf - inf in the out-of-range elements)
        rec = pr.planes_to_f32(planes[..., :c], fmt).astype(np.float64) + pr.planes_to_f32(planes[..., c:2 * c], fmt).astype(np.float64)
    v64 = v.astype(np.float64)
    bound = 2.0 ** -17 * np.abs(v64) if fmt == "bf16" else np.maximum(2.0 ** -22 * np.abs(v64), 2.0 ** -25)
    err = np.abs(rec - v64)
    assert (err[ok] <= bound[ok]).all(), float((err[ok] / np.maximum(bound[ok], 1e-300)).max())
    for e in pr.EDGE_VALUES:  # every in-range edge value is among the checked elements
        if _in_range(np.float32(e), fmt):
            assert ((v == e) & ok).any(), e


def test_fp16_hi_is_clamped_and_the_boundary_is_65520():
    """|v| >= 65520 (the first value that would round to inf) gives hi = +-65504; below it hi rounds to nearest even; +-inf are
    clamped in hi and in lo"""
    big = 0x7BFF
    for v, hi in [(65504.0, big), (65519.9, big), (65520.0, big), (1e6, big), (3.4e38, big), (np.inf, big), (65488.0, 0x7BFE)]:
        for s, sign in ((1.0, 0), (-1.0, 0x8000)):
            p = pr.split(np.array([s * v], dtype=np.float32), "f16")
            assert p[0] == (hi | sign) and p[2] == p[0], (v, s, p)
    assert pr.split(np.array([np.inf], dtype=np.float32), "f16")[1] == big
    assert pr.split(np.array([-np.inf], dtype=np.float32), "f16")[1] == big | 0x8000
    assert pr.split(np.array([65519.9], dtype=np.float32), "f16")[1] == np.float16(np.float32(65519.9) - np.float32(65504)).view(np.uint16)
    # bf16 keeps the infinities in hi
    assert pr.split(np.array([np.inf, -np.inf], dtype=np.float32), "bf16")[[0, 1]].tolist() == [0x7F80, 0xFF80]


def test_value_edges_of_the_fp16_split():
    """denormal lo planes, the smallest fp16 denormal, its tie and a hi-plane tie, by hand"""
    f = np.float32

    def planes(v):
        p = pr.split(np.array([v], dtype=np.float32), "f16")
        return int(p[0]), int(p[1])
    assert planes(f(2.0 ** -14)) == (0x0400, 0)
    assert planes(f(2.0 ** -24)) == (0x0001, 0)
    assert planes(f(2.0 ** -25)) == (0x0000, 0)               # tie between 0 and 2^-24: to even, and lo sees the whole value again
    assert planes(f(1.5 * 2.0 ** -24)) == (0x0002, 0x8000)    # tie to even (2^-23); lo = -2^-25 ties to -0
    assert planes(f(1 + 2.0 ** -11)) == (0x3C00, 0x1000)      # hi tie to even (1.0), lo = 2^-11
    assert planes(f(1 + 3 * 2.0 ** -11)) == (0x3C02, 0x9000)  # hi tie to even (upwards), lo = -2^-11
    assert planes(f(2.0 ** -14 * (1 - 2.0 ** -11))) == (0x0400, 0x8000)  # 1023.5 denormal steps: up to the first normal number
    assert planes(f(2.0 ** -3 + 2.0 ** -16)) == (0x3000, 0x0100)         # lo = 2^-16: a denormal of fp16
    assert planes(f(-(1 + 2.0 ** -8))) == (0xBC04, 0)         # bf16's hi tie is exact in fp16


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_nan_gives_nan_in_both_planes(fmt):
    p = pr.split(pr.NAN_VALUES, fmt)
    assert np.isnan(pr.planes_to_f32(p, fmt)).all()
    c = pr.canonical(p, fmt)
    assert c[0] == c[1] == c[2]
    # and through every mode that passes a value on: 0, 3 under a positive mask, 4
    v = np.full((1, 8), np.nan, dtype=np.float32)
    mask = pr.split(np.full((1, 8), 0.5, dtype=np.float32), fmt)
    for mode in (0, 3, 4):
        assert np.isnan(pr.planes_to_f32(pr.act_split(v, mode, mask, fmt), fmt)).all(), mode
    src = pr.split(v, fmt)
    for mode in (0, 1, 2):
        a, b = pr.dropout_planes(src, mask, 8, mode, 0.0, 5, fmt)
        assert np.isnan(pr.planes_to_f32(a, fmt)).all() and np.isnan(pr.planes_to_f32(b, fmt)).all(), mode


def test_modes_by_hand():
    f = np.float32
    v = np.array([[-2.0, -0.5, 0.0, 0.5, 2.0, -1.0, 3.0, -3.0]], dtype=np.float32)
    y = np.array([[1.0, 0.0, -0.0, 6e-8, -0.25, -0.25, 2.0 ** -133, -1.0]], dtype=np.float32)
    for fmt in pr.FORMATS:
        mask = pr.split(y, fmt)
        ym = pr.planes_value(mask, 8, fmt)
        assert np.array_equal(pr.act_value(v, 1), np.maximum(v, 0))
        assert np.array_equal(pr.act_value(v, 3, mask, fmt), np.where(ym > 0, v, 0))
        want4 = np.where(ym > 0, v, v * (ym + f(1)))
        assert np.array_equal(pr.act_value(v, 4, mask, fmt), want4)
        assert pr.act_value(v, 4, mask, fmt)[0, 4] == f(1.5) and pr.act_value(v, 4, mask, fmt)[0, 7] == 0
        e = pr.act_value(v, 2)
        assert e[0, 4] == 2.0 and abs(float(e[0, 0]) - np.expm1(-2.0)) < 1e-7
    assert pr.planes_value(pr.split(y, "bf16"), 8, "bf16")[0, 6] == f(2.0 ** -133)  # the smallest positive bf16 is a mask
    assert pr.planes_value(pr.split(y, "f16"), 8, "f16")[0, 3] == f(2.0 ** -24)     # ... and the smallest positive fp16


def test_step_ulps_walks_the_float32_line():
    x = np.array([1.0, -1.0, 0.0, 2.0 ** -149, -2.0 ** -149], dtype=np.float32)
    assert np.array_equal(pr.step_ulps(x, 1), np.nextafter(x, np.float32(np.inf)))
    assert np.array_equal(pr.step_ulps(x, -1), np.nextafter(x, np.float32(-np.inf)))
    assert np.array_equal(pr.step_ulps(pr.step_ulps(x, 3), -3).view(np.uint32) & 0x7FFFFFFF, x.view(np.uint32) & 0x7FFFFFFF)


@pytest.mark.parametrize("rate", [0.25, 0.9, 0.0])
@pytest.mark.parametrize("seed", [5, 2 ** 63 + 12345, 2 ** 64 - 1])
def test_keep_fraction(rate, seed):
    """over 2^18 indices the keep fraction is within 4 sigma of 1 - rate; seeds up to 2^64 - 1"""
    n = 1 << 18
    keep = pr._dropout_keep(seed, n, rate)
    sigma = np.sqrt(rate * (1 - rate) / n)
    assert abs(keep.mean() - (1 - rate)) <= 4 * sigma, (keep.mean(), sigma)
    assert np.array_equal(keep[:1000], pr._dropout_keep(seed, 1000, rate))  # a pure function of (seed, index)


def test_dropout_bits_by_hand():
    """one value computed with Python integers"""
    m = (1 << 64) - 1
    for seed, idx in [(5, 0), (2 ** 63 + 12345, 77), (2 ** 64 - 1, 12)]:
        z = (seed + 0x9E3779B97F4A7C15 * (idx + 1)) & m
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
        z ^= z >> 31
        assert int(pr.dropout_bits(seed, idx + 1)[idx]) == z >> 32
    assert int(pr.dropout_threshold(0.25)) == 1 << 30 and int(pr.dropout_threshold(0.0)) == 0
    assert int(pr.dropout_threshold(0.9)) == int(float(np.float32(0.9)) * 2 ** 32)
    assert pr.dropout_scale(0.25) == np.float32(1) / np.float32(0.75)


@pytest.mark.parametrize("fmt", pr.FORMATS)
def test_the_two_mode2_candidates_rarely_differ(fmt):
    """fused and unfused m * keep_prob + 1 give different planes for at most 10 % of the elements (4.5 % on fp16 and 0.02 % on
    bf16 on plain randn gradients): the two-candidate rule of the GPU test still pins the others to one value"""
    c = 256
    g, m = pr.mode2_inputs(300, c, fmt)
    a, b = pr.dropout_planes(g, m, c, 2, 0.25, 5, fmt)
    differ = (a[:, :2 * c] != b[:, :2 * c]).reshape(-1, 2, c).any(axis=1)
    frac = differ.mean()
    print("mode 2 candidates differ on {:.3%} of the elements ({})".format(frac, fmt))
    assert frac <= 0.10
    dropped = ~pr._dropout_keep(5, g.shape[0] * c, 0.25).reshape(-1, c)
    assert not a[:, :c][dropped].any() and not a[:, c:2 * c][dropped].any()


def test_packing_layouts_by_hand():
    w = np.arange(2 * 32 * 64, dtype=np.float32).reshape(2, 32, 64) / 8  # exact in both formats' hi + lo
    for fmt in pr.FORMATS:
        fwd, dgrad = pr.pack_weights_planes(w, 2.0, fmt)
        assert fwd.shape == (64, 2, 96) and dgrad.shape == (32, 2, 192)
        val = lambda row, n: pr.planes_to_f32(row[:n], fmt) + pr.planes_to_f32(row[2 * n:], fmt)  # noqa: E731
        assert np.array_equal(val(fwd[5, 1], 32), 2 * w[1, :, 5]) and np.array_equal(fwd[5, 1, :32], fwd[5, 1, 32:64])
        assert np.array_equal(val(dgrad[7, 0], 64), 2 * w[1, 7, :]) and np.array_equal(dgrad[7, 0, :64], dgrad[7, 0, 64:128])
        x = np.arange(2 * 3 * 5, dtype=np.float32).reshape(2, 3, 5)
        p = pr.pack_input_planes(x, 8, fmt)
        assert p.shape == (2, 3, 24) and not p[..., 5:8].any() and not p[..., 13:16].any() and not p[..., 21:].any()
        assert np.array_equal(pr.planes_to_f32(p[..., :5], fmt), x)


def test_combine_and_bias_gradient_by_hand():
    taps, c_in, c_out, frames, fstride, rb_fstride = 4, 2, 4, 2, 6, 2
    ra_cin, rb_cin = fstride + 2 * c_in + 1, rb_fstride + c_in + 1
    ra = np.arange(2 * ra_cin * c_out, dtype=np.float32)
    rb = 1000 + np.arange(2 * rb_cin * c_out, dtype=np.float32)
    dw = pr.wgrad_combine(ra, rb, taps, c_in, c_out, frames, fstride, ra_cin, rb_cin, rb_fstride, 0.5)
    tap, ci, co = 3, 1, 2  # tv = 1, f = 1
    a = lambda r, col: ra[(1 * ra_cin + r) * c_out + col]  # noqa: E731
    assert dw[tap, ci, co] == 0.5 * (a(fstride + ci, co) + rb[(1 * rb_cin + rb_fstride + ci) * c_out + co] + a(fstride + c_in + ci, co))
    g = pr.split(np.array([[[1.0, 2.0]], [[1 + 2.0 ** -12, -4.0]]], dtype=np.float32), "f16")
    assert pr.bias_grad(g, 2, 0.5, "f16").tolist() == [1 + 2.0 ** -13, -1.0]


def test_single_plane_twins_by_hand():
    x = np.array([1.0, -2.0, 3.0, 0.0, 1 + 2.0 ** -8], dtype=np.float32)
    keep = pr._dropout_keep(5, 5, 0.25)
    s = np.float32(1) / np.float32(0.75)
    assert np.array_equal(pr.dropout_single(x, 0.25, 5, "f32"), np.where(keep, x * s, 0).astype(np.float32))
    bits = pr._round_bf16(x)[1]
    assert np.array_equal(pr.scale_single(bits, 2.0, "bf16"), pr._round_bf16(2 * pr.planes_to_f32(bits, "bf16"))[1])
    a, b = pr.elu_dropout_backward_single(x, np.array([1.0, -0.5, 0.0, -1.0, 2.0], dtype=np.float32), 0.0, 5, "f32")
    assert np.array_equal(a, b) and a.tolist() == [1.0, -1.0, 3.0, 0.0, float(x[4])]


# ------------------------------------------------------------------------------------------ refusals
def test_plane_refusals_come_before_any_launch(hip_lib):
    """valid HOST addresses: nothing may be launched on them.  Every refusal returns SL_ERR_INVALID_ARGUMENT (a too small
    bias-gradient workspace: SL_ERR_WORKSPACE_TOO_SMALL), names the function, and leaves the destination untouched."""
    src = np.zeros(4096, dtype=np.float32)
    dst = np.full(3 * 4096, pr.SENTINEL, dtype=np.uint16)
    other = np.zeros(3 * 4096, dtype=np.uint16)
    out32 = np.full(4096, 7.0, dtype=np.float32)
    S, D, O, F = src.ctypes.data, dst.ctypes.data, other.ctypes.data, out32.ctypes.data
    nan = float("nan")
    cases = []

    def refuse(name, args, rc=SL_ERR_INVALID_ARGUMENT, says=None):
        cases.append((name, args, rc, says or name))

    for tag in ("sl_split3", "sl_splitf16"):
        # src, dst, mask, batch, t_out, channels, src_batch_stride, dst_row0, dst_batch_stride, mode, stream
        refuse(tag, (S, D, None, 1, 4, 12, 48, 0, 144, 0, None))       # channels % 8
        refuse(tag, (S, D, None, 1, 4, 4, 16, 0, 48, 0, None))
        refuse(tag, (S, D, O, 1, 4, 8, 32, 0, 96, 5, None))            # mode out of range
        refuse(tag, (S, D, O, 1, 4, 8, 32, 0, 96, -1, None))
        refuse(tag, (S, D, None, 1, 4, 8, 32, 0, 96, 3, None))         # modes 3 / 4 without a mask
        refuse(tag, (S, D, None, 1, 4, 8, 32, 0, 96, 4, None))
        # src, dst, y, rows, channels, mode, rate, seed, stream
        drop = tag + "_dropout"
        refuse(drop, (O, D, None, 4, 12, 0, 0.25, 5, None))            # channels % 8
        refuse(drop, (O, D, O, 4, 8, 3, 0.25, 5, None))                # mode out of range
        refuse(drop, (O, D, O, 4, 8, -1, 0.25, 5, None))
        refuse(drop, (O, D, None, 4, 8, 2, 0.25, 5, None))             # mode 2 without y
        for rate in (-0.1, 1.0, nan):
            refuse(drop, (O, D, O, 4, 8, 0, rate, 5, None))
        # src, dst, batch, t_in, f, channels, dst_row0, dst_batch_stride, stream
        refuse(tag + "_pack_input", (S, D, 1, 4, 9, 8, 0, 96, None))   # channels < f
        # g, db, batch, t_out, channels, g_row0, g_batch_stride, [scale,] workspace, workspace_bytes, stream
        scale = (1.0,) if tag == "sl_splitf16" else ()
        bg = tag + "_bias_grad"
        refuse(bg, (O, F, 1, 4, 96) + (0, 1152) + scale + (S, 64 * 96 * 4, None))       # channels % 64
        refuse(bg, (O, F, 1, 4, 64) + (0, 768) + scale + (S, 64 * 64 * 4 - 1, None), SL_ERR_WORKSPACE_TOO_SMALL)
        refuse(bg, (O, F, 1, 4, 64) + (0, 768) + scale + (None, 64 * 64 * 4, None), SL_ERR_WORKSPACE_TOO_SMALL)
    # w_master, w_fwd3, w_dgrad3, k, cin_pad, cout_pad, [scale,] stream
    refuse("sl_split3_pack_weights", (S, D, None, 1, 48, 32, None))    # % 32
    refuse("sl_split3_pack_weights", (S, D, None, 1, 32, 16, None))
    refuse("sl_splitf16_pack_weights", (S, D, None, 1, 48, 32, 1.0, None))
    refuse("sl_splitf16_pack_weights", (S, D, None, 1, 32, 16, 1.0, None))
    refuse("sl_splitf16_pack_weights", (S, D, None, 1, 32, 32, 0.0, None))
    # ra, rb, dw, taps, c_in, c_out, frames, fstride, ra_cin, rb_cin, rb_fstride, [scale,] stream: both entry points report as
    # sl_split3_wgrad_combine
    for name, tail in (("sl_split3_wgrad_combine", (None,)), ("sl_split3_wgrad_combine_scaled", (1.0, None))):
        says = "sl_split3_wgrad_combine"
        refuse(name, (S, S, F, 4, 8, 10, 1, 0, 16, 8, 0) + tail, says=says)      # c_out % 4
        refuse(name, (S, S, F, 3, 8, 12, 3, 0, 48, 24, 0) + tail, says=says)     # frames = 3
        refuse(name, (S, S, F, 4, 8, 12, 2, 24, 39, 16, 8) + tail, says=says)    # ra_cin < fstride + 2 c_in
        refuse(name, (S, S, F, 4, 8, 12, 2, 24, 40, 15, 8) + tail, says=says)    # rb_cin < rb_fstride + c_in
        refuse(name, (S, S, F, 4, 8, 12, 1, 0, 15, 8, 0) + tail, says=says)      # frames = 1: ra_cin < 2 c_in
    refuse("sl_split3_wgrad_combine_scaled", (S, S, F, 4, 8, 12, 1, 0, 16, 8, 0, 0.0, None), says="sl_split3_wgrad_combine")
    # the single-plane twins: src, dst, n, dtype, rate, seed, stream
    for rate in (-0.1, 1.0, nan):
        refuse("sl_dropout", (S, F, 16, 1, rate, 5, None))
        refuse("sl_elu_dropout_backward", (F, S, 16, 1, rate, 5, None))
    refuse("sl_dropout", (S, F, 16, 2, 0.25, 5, None))                 # dtype: neither SL_BF16 nor SL_F32
    refuse("sl_elu_dropout_backward", (F, S, 16, 2, 0.25, 5, None))
    refuse("sl_scale", (F, 16, 2, 2.0, None))
    for name, args, rc, says in cases:
        got = hip_lib.raw(name)(*args)
        assert got == rc, (name, args, got, hip_lib.last_error())
        assert says in hip_lib.last_error(), (name, args, hip_lib.last_error())
    assert (dst == pr.SENTINEL).all() and (out32 == 7.0).all() and not other.any() and not src.any()
