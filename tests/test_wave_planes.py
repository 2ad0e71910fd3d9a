"""sl_wave_frames_planes without a GPU: the numpy restatement (tests/wave_planes_ref.py) against the bounds the f16x3 raw-wave
path rests on, and the entry point's host-side refusals (they come before any launch)."""
import numpy as np
import pytest

import wave_planes_ref as ref

SL_OK, SL_ERR_INVALID_ARGUMENT = 0, -1
SL_BF16, SL_F32, SL_F16 = 0, 1, 2
K, STRIDE = 250, 160


def _inputs():
    rng = np.random.RandomState(17)
    loud = rng.randn(2, 4001, 1).astype(np.float32)
    quiet = (loud * np.float32(2.0 ** -10)).astype(np.float32)
    edge = np.where(rng.rand(2, 4001, 1) < 0.5, -58.0, 58.0).astype(np.float32)
    return [("randn", loud, 1.0), ("quiet", quiet, 1.0), ("quiet_scaled", quiet, 1024.0), ("edge", edge, 1024.0)]


@pytest.mark.parametrize("name,x,scale", _inputs(), ids=[c[0] for c in _inputs()])
def test_fp16_planes_reconstruct_the_scaled_samples(name, x, scale):
    """|hi + lo - v| <= max(2^-22 |v|, 2^-25) element-wise with v = scale * x, the third plane equals the first, padding
    columns and the SAME padding are zero"""
    t_out, pad_l = ref.same_padding(x.shape[1], K, STRIDE)
    v = ref.gather_windows(x, K, STRIDE, pad_l, t_out, 256, scale)
    planes = ref.wave_frames_planes(x, K, STRIDE, pad_l, t_out, 256, scale, "f16")
    assert planes.shape == (2, t_out, 768) and planes.dtype == np.uint16
    hi, lo, hi2 = planes[..., :256], planes[..., 256:512], planes[..., 512:]
    assert np.array_equal(hi, hi2)
    rec = ref.planes_to_f32(hi).astype(np.float64) + ref.planes_to_f32(lo).astype(np.float64)
    v64 = v.astype(np.float64)
    bound = np.maximum(2.0 ** -22 * np.abs(v64), 2.0 ** -25)
    assert (np.abs(rec - v64) <= bound).all(), float((np.abs(rec - v64) / bound).max())
    assert not planes[..., 250:256].any() and not planes[..., 506:512].any()
    assert not planes[:, 0, :pad_l].any() and np.array_equal(v[:, 0, pad_l:250], np.float32(scale) * x[:, :250 - pad_l, 0])


def test_the_input_scale_is_exact():
    """scale 1024 on x * 2^-10 gives the planes of scale 1 on x -- and unscaled quiet samples lose what the scale keeps"""
    _, loud, _ = _inputs()[0]
    quiet = (loud * np.float32(2.0 ** -10)).astype(np.float32)
    t_out, pad_l = ref.same_padding(loud.shape[1], K, STRIDE)
    for fmt in ("f16", "bf16"):
        a = ref.wave_frames_planes(loud, K, STRIDE, pad_l, t_out, 256, 1.0, fmt)
        b = ref.wave_frames_planes(quiet, K, STRIDE, pad_l, t_out, 256, 1024.0, fmt)
        assert np.array_equal(a, b), fmt

    def rel_l2(planes, v, fmt):
        rec = ref.planes_to_f32(planes[..., :256], fmt).astype(np.float64) + ref.planes_to_f32(planes[..., 256:512], fmt)
        return float(np.linalg.norm(rec - v) / np.linalg.norm(v))
    v = ref.gather_windows(quiet, K, STRIDE, pad_l, t_out, 256).astype(np.float64)
    unscaled = rel_l2(ref.wave_frames_planes(quiet, K, STRIDE, pad_l, t_out, 256, 1.0, "f16"), v, "f16")
    bf16 = rel_l2(ref.wave_frames_planes(quiet, K, STRIDE, pad_l, t_out, 256, 1.0, "bf16"), v, "bf16")
    scaled = rel_l2(ref.wave_frames_planes(quiet, K, STRIDE, pad_l, t_out, 256, 1024.0, "f16"), 1024.0 * v, "f16")
    assert scaled < 2.0 ** -22 and bf16 < 2.0 ** -17 and unscaled > 100 * scaled, (unscaled, bf16, scaled)


def test_cin_2_windows_interleave_the_channels():
    rng = np.random.RandomState(3)
    x = rng.randn(1, 700, 2).astype(np.float32)
    t_out, pad_l = ref.same_padding(700, K, STRIDE)
    v = ref.gather_windows(x, K, STRIDE, pad_l, t_out, 512)
    assert v[0, 2, 2 * 7 + 1] == x[0, 2 * STRIDE + 7 - pad_l, 1] and not v[..., 500:].any()
    assert not v[0, t_out - 1, 2 * (700 - (t_out - 1) * STRIDE + pad_l):].any()


def test_refusals_come_before_any_launch(hip_lib):
    """valid HOST addresses: nothing may be launched on them.  Every refusal of include/speechless_hip.h returns
    SL_ERR_INVALID_ARGUMENT and names the function."""
    call = hip_lib.raw("sl_wave_frames_planes")
    audio = np.zeros((1, 400, 1), dtype=np.float32)
    dst = np.zeros((1, 3, 768), dtype=np.uint16)
    good = dict(audio=audio.ctypes.data, dst=dst.ctypes.data, batch=1, t_in=400, cin=1, k=250, stride=160, pad_left=85, t_out=3,
                channels=256, dst_batch_stride=3 * 768, scale=1024.0, dtype=SL_F16)

    def run(**change):
        a = dict(good, **change)
        return call(a["audio"], a["dst"], a["batch"], a["t_in"], a["cin"], a["k"], a["stride"], a["pad_left"], a["t_out"],
                    a["channels"], a["dst_batch_stride"], a["scale"], a["dtype"], None)

    refused = [dict(audio=None), dict(dst=None), dict(batch=0), dict(t_in=0), dict(t_in=-5), dict(cin=0), dict(k=0),
               dict(stride=0), dict(t_out=0), dict(channels=0), dict(pad_left=-1),
               dict(channels=248), dict(cin=2), dict(k=257),                    # k * cin > channels
               dict(dtype=SL_F32), dict(dtype=7), dict(dtype=-1),
               dict(scale=0.0), dict(scale=-1024.0), dict(scale=3.0), dict(scale=1000.0), dict(scale=float("inf")),
               dict(scale=float("nan")),
               dict(dst_batch_stride=3 * 768 - 8), dict(channels=252)]
    for change in refused:
        assert run(**change) == SL_ERR_INVALID_ARGUMENT, change
        assert "sl_wave_frames_planes" in hip_lib.last_error(), (change, hip_lib.last_error())
    assert not dst.any()
