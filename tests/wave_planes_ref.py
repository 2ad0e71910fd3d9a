"""numpy restatement of sl_wave_frames_planes (include/speechless_hip.h): the sample windows of wave_conv's output frames
(reference net.py:310-312) as the planes [hi | lo | hi] of scale * x -- fp16 through np.float16, bf16 through torch; both
conversions round to nearest even.  Shared by tests/test_wave_planes.py (CPU) and tests/test_gpu_wave_f16x3.py."""
import numpy as np

F16_MAX = 65504.0


def same_padding(t_in, k, stride):
    """TensorFlow's SAME rule: (output frames, left padding)"""
    t_out = -(-t_in // stride)
    pad = max((t_out - 1) * stride + k - t_in, 0)
    return t_out, pad // 2


def gather_windows(x, k, stride, pad_left, t_out, channels, scale=1.0):
    """x: float32 (B, T, Cin) -> float32 (B, t_out, channels): column j * Cin + c of row t is scale * x[b, t * stride + j -
    pad_left, c], zero outside [0, T) and in the columns >= k * Cin"""
    x = np.asarray(x, dtype=np.float32)
    batch, t_in, cin = x.shape
    assert k * cin <= channels
    padded = np.zeros((batch, pad_left + t_in + (t_out - 1) * stride + k, cin), dtype=np.float32)
    padded[:, pad_left:pad_left + t_in] = x * np.float32(scale)
    out = np.zeros((batch, t_out, channels), dtype=np.float32)
    for t in range(t_out):
        out[:, t, :k * cin] = padded[:, t * stride:t * stride + k].reshape(batch, k * cin)
    return out


def _round_f16(v):
    """(float32 value of the rounded number, its 16 bits); clamped to the largest finite fp16 as the kernels clamp"""
    h = np.clip(v, -F16_MAX, F16_MAX).astype(np.float16)
    return h.astype(np.float32), h.view(np.uint16)


def _round_bf16(v):
    import torch
    h = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16)
    return h.to(torch.float32).numpy(), h.view(torch.int16).numpy().view(np.uint16)


def split_planes(v, fmt="f16"):
    """float32 (..., C) -> uint16 (..., 3 C) rows [hi | lo | hi]: hi = cvt(v), lo = cvt(v - float(hi))"""
    rnd = {"f16": _round_f16, "bf16": _round_bf16}[fmt]
    v = np.asarray(v, dtype=np.float32)
    hi_f, hi = rnd(v)
    _, lo = rnd(v - hi_f)
    return np.concatenate([hi, lo, hi], axis=-1)


def planes_to_f32(bits, fmt="f16"):
    """uint16 planes -> their float32 values"""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if fmt == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def wave_frames_planes(x, k, stride, pad_left, t_out, channels, scale=1.0, fmt="f16"):
    """what sl_wave_frames_planes writes into the rows t < t_out: uint16 (B, t_out, 3 * channels)"""
    return split_planes(gather_windows(x, k, stride, pad_left, t_out, channels, scale), fmt)
