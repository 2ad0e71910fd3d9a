"""numpy model of the elementwise plane kernels (csrc/split3.hip) and their single-plane twins (csrc/misc.hip), in float32
arithmetic in the kernels' order of operations.  The two-plane split itself comes from wave_planes_ref.py.  Shared by
tests/test_plane_ref.py (CPU: the model against the bounds DESIGN.md claims) and tests/test_gpu_planes.py (the kernels against
the model, bit for bit).

Formats: "bf16" (sl_split3*) and "f16" (sl_splitf16*).  A plane tensor is uint16 (..., 3 C): [hi | lo | hi]."""
import numpy as np

from wave_planes_ref import F16_MAX, _round_bf16, _round_f16, planes_to_f32, split_planes  # noqa: F401  (re-exported)

FORMATS = ("bf16", "f16")
F32 = np.float32
SENTINEL = 0x5A5A


def _edge_values():
    p = [0.0, 2.0 ** -149, 2.0 ** -126, 2.0 ** -25, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -3,
         1 + 2.0 ** -23, 1 + 2.0 ** -11, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -12,
         65504.0, 65519.9, 65520.0, 1e6, 3.4e38, np.inf]
    return np.array([s * x for x in p for s in (1.0, -1.0)], dtype=np.float32)


EDGE_VALUES = _edge_values()   # both signs of every value edge of the two formats
NAN_VALUES = np.array([np.nan], dtype=np.float32)


def split(v, fmt):
    """split_planes without numpy's warnings on inf - inf (bf16 planes of +-inf: hi = +-inf, lo = NaN)"""
    with np.errstate(all="ignore"):
        return split_planes(np.asarray(v, dtype=np.float32), fmt)


def planes_value(planes, c, fmt):
    """float32(dec(hi) + dec(lo)) of a plane tensor (..., 3 c): the value every kernel here reads back"""
    with np.errstate(all="ignore"):
        return (planes_to_f32(planes[..., :c], fmt) + planes_to_f32(planes[..., c:2 * c], fmt)).astype(np.float32)


def canonical(bits, fmt):
    """plane bits with every NaN replaced by one pattern: NaNs are compared as NaNs, never by sign or payload"""
    bits = np.array(bits, dtype=np.uint16)
    bits[np.isnan(planes_to_f32(bits, fmt))] = 0x7E00 if fmt == "f16" else 0x7FC0
    return bits


def zeros_by_value(bits):
    """-0 -> +0 (mode 1 does not pin the sign of a zero result)"""
    bits = np.array(bits, dtype=np.uint16)
    bits[bits == 0x8000] = 0
    return bits


# ------------------------------------------------------------------------------------------ sl_split3 / sl_splitf16
def act_value(v, mode, mask_planes=None, fmt="f16"):
    """the float32 value split3_act_kernel splits, modes 0..4; mode 2 returns float32(expm1(float64 v)) where v <= 0 (the
    device's expm1f may differ from it in the last bits: the caller decides by how much)"""
    v = np.asarray(v, dtype=np.float32)
    c = v.shape[-1]
    with np.errstate(all="ignore"):
        if mode == 0:
            return v
        if mode == 1:
            return np.where(v > 0, v, F32(0))  # fmaxf(v, 0) for every v but NaN, which the tests keep out of mode 1
        if mode == 2:
            return np.where(v > 0, v, np.expm1(v.astype(np.float64)).astype(np.float32))
        if mode == 3:
            y = planes_to_f32(mask_planes[..., :c], fmt)
            return np.where(y > 0, v, F32(0))
        if mode == 4:
            y = planes_value(mask_planes, c, fmt)
            return np.where(y > 0, v, v * (y + F32(1)).astype(np.float32)).astype(np.float32)
    raise ValueError(mode)


def act_split(v, mode, mask_planes=None, fmt="f16"):
    """what sl_split3 / sl_splitf16 store for the rows of v: uint16 (..., 3 C)"""
    return split(act_value(v, mode, mask_planes, fmt), fmt)


def step_ulps(x, d):
    """float32 x moved by d units in the last place (across zero as well)"""
    x = np.asarray(x, dtype=np.float32)
    if d == 0:
        return x
    i = x.view(np.int32).astype(np.int64)
    key = np.where(i < 0, -(i & 0x7FFFFFFF), i) + d  # monotone integer line; -0 and +0 share the origin
    back = np.where(key < 0, (-key) | 0x80000000, key).astype(np.uint32)
    return back.view(np.float32)


# ------------------------------------------------------------------------------------------ dropout
def dropout_bits(seed, n):
    """numpy mirror of dropout_bits (csrc/common.h): splitmix64 finaliser of seed + golden * (index + 1), indices 0 .. n - 1;
    any seed below 2^64"""
    with np.errstate(over="ignore"):
        idx = np.arange(1, n + 1, dtype=np.uint64)
        z = np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF) + np.uint64(0x9E3779B97F4A7C15) * idx
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return (z >> np.uint64(32)).astype(np.uint32)


def dropout_threshold(rate):
    return np.uint32(int(float(np.float32(rate)) * 4294967296.0))


def _dropout_keep(seed, n, rate):
    """the keep decisions of the elements 0 .. n - 1: bits >= uint32(float64(float32(rate)) * 2^32)"""
    return dropout_bits(seed, n) >= dropout_threshold(rate)


def dropout_scale(rate):
    return F32(1) / (F32(1) - F32(rate))


def _elu_slope_candidates(m, keep_prob):
    """m * keep_prob + 1 in float32: as ONE fma (product and sum in float64 -- the product of two float32 is exact there --
    rounded once to float32) and as a rounded product followed by a rounded sum.  The kernels may form either."""
    m = np.asarray(m, dtype=np.float32)
    with np.errstate(all="ignore"):
        fused = (m.astype(np.float64) * np.float64(keep_prob) + 1.0).astype(np.float32)
        unfused = ((m * F32(keep_prob)).astype(np.float32) + F32(1)).astype(np.float32)
    return fused, unfused


def dropout_values(v, m, mode, rate, seed):
    """the float32 values split3_dropout_kernel splits for the logical tensor v (rows, c) -- element index r * c + ch -- as two
    candidates (they differ only in mode 2).  m: the stored activation's values (mode 2)."""
    v = np.asarray(v, dtype=np.float32)
    scale, keep_prob = dropout_scale(rate), F32(1) - F32(rate)
    keep = np.ones(v.shape, dtype=bool) if mode == 1 else _dropout_keep(seed, v.size, rate).reshape(v.shape)
    out = []
    with np.errstate(all="ignore"):
        if mode == 2:
            for e in _elu_slope_candidates(m, keep_prob):
                d = np.where(np.asarray(m) > 0, scale, (scale * e).astype(np.float32)).astype(np.float32)
                out.append(np.where(keep, (v * d).astype(np.float32), F32(0)))
        else:
            r = np.where(keep, (v * scale).astype(np.float32), F32(0))
            out = [r, r]
    return out[0], out[1]


def dropout_planes(src_planes, y_planes, c, mode, rate, seed, fmt):
    """what sl_split3_dropout / sl_splitf16_dropout store: (fused, unfused) plane tensors (rows, 3 c)"""
    v = planes_value(src_planes, c, fmt)
    m = planes_value(y_planes, c, fmt) if mode == 2 else None
    a, b = dropout_values(v, m, mode, rate, seed)
    return split(a, fmt), split(b, fmt)


# ------------------------------------------------------------------------------------------ packing
def pack_input_planes(x, c, fmt):
    """x float32 (B, t_in, f) -> planes (B, t_in, 3 c), channels >= f zero in all three planes"""
    x = np.asarray(x, dtype=np.float32)
    v = np.zeros(x.shape[:2] + (c,), dtype=np.float32)
    v[..., :x.shape[2]] = x
    return split(v, fmt)


def pack_weights_planes(w, scale, fmt):
    """master w float32 (k, cin, cout) -> (w_fwd3 (cout, k, 3 cin), w_dgrad3 (cin, k, 3 cout)): rows [hi | hi | lo] of scale * w,
    the taps of the dgrad copy reversed"""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(over="ignore"):
        v = (w * F32(scale)).astype(np.float32)

    def rows(a):  # (..., n) -> (..., 3 n) as [hi | hi | lo]
        n = a.shape[-1]
        p = split(a, fmt)
        return np.concatenate([p[..., :n], p[..., :n], p[..., n:2 * n]], axis=-1)
    fwd = rows(v.transpose(2, 0, 1).copy())                          # [co][tap][ci]
    dgrad = rows(v[::-1].transpose(1, 0, 2).copy())                  # [ci][k - 1 - tap][co]
    return fwd, dgrad


def wgrad_combine(ra, rb, taps, c_in, c_out, frames, fstride, ra_cin, rb_cin, rb_fstride, scale=1.0):
    """dw[tap][ci][co] = ((RA[tv][f * fstride + ci] + RB[tv][f * rb_fstride + ci]) + RA[tv][f * fstride + c_in + ci]) * scale,
    tap = frames * tv + f, float32 in that order"""
    ra = np.asarray(ra, dtype=np.float32).reshape(taps // frames, ra_cin, c_out)
    rb = np.asarray(rb, dtype=np.float32).reshape(taps // frames, rb_cin, c_out)
    dw = np.zeros((taps, c_in, c_out), dtype=np.float32)
    for tap in range(taps):
        tv, f = divmod(tap, frames)
        hh = ra[tv, f * fstride:f * fstride + c_in]
        hl = rb[tv, f * rb_fstride:f * rb_fstride + c_in]
        lh = ra[tv, f * fstride + c_in:f * fstride + 2 * c_in]
        dw[tap] = ((hh + hl).astype(np.float32) + lh).astype(np.float32) * F32(scale)
    return dw


def bias_grad(g_planes, c, scale, fmt):
    """float64 sum over every row of dec(hi) + dec(lo), times scale: g_planes (B, t_out, 3 c) holds the valid rows only"""
    g = np.asarray(g_planes)
    s = planes_to_f32(g[..., :c], fmt).astype(np.float64) + planes_to_f32(g[..., c:2 * c], fmt).astype(np.float64)
    return s.reshape(-1, c).sum(axis=0) * float(scale)


# ------------------------------------------------------------------------------------------ misc.hip's single-plane twins
def _load(x, storage):
    x = np.asarray(x)
    return planes_to_f32(x, "bf16") if storage == "bf16" else x.astype(np.float32)


def _store(v, storage):
    """float32 values as they are stored: float32, or bf16 bits"""
    v = np.asarray(v, dtype=np.float32)
    return _round_bf16(v)[1] if storage == "bf16" else v


def dropout_single(x, rate, seed, storage):
    """sl_dropout on the flat tensor x (float32 values, or uint16 bf16 bits): keep ? x / (1 - rate) : 0"""
    v = _load(x, storage).reshape(-1)
    keep = _dropout_keep(seed, v.size, rate)
    with np.errstate(all="ignore"):
        return _store(np.where(keep, (v * dropout_scale(rate)).astype(np.float32), F32(0)), storage)


def scale_single(x, scale, storage):
    """sl_scale: x * scale"""
    with np.errstate(all="ignore"):
        return _store((_load(x, storage).reshape(-1) * F32(scale)).astype(np.float32), storage)


def elu_dropout_backward_single(g, y, rate, seed, storage):
    """sl_elu_dropout_backward: keep ? (g * scale) * (m > 0 ? 1 : m * keep_prob + 1) : 0, as (fused, unfused) candidates"""
    gv, m = _load(g, storage).reshape(-1), _load(y, storage).reshape(-1)
    keep = _dropout_keep(seed, gv.size, rate)
    scale, keep_prob = dropout_scale(rate), F32(1) - F32(rate)
    out = []
    with np.errstate(all="ignore"):
        for e in _elu_slope_candidates(m, keep_prob):
            d = np.where(m > 0, F32(1), e).astype(np.float32)
            out.append(_store(np.where(keep, ((gv * scale).astype(np.float32) * d).astype(np.float32), F32(0)), storage))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------ inputs of the tests
def fill_values(shape, fmt, seed, edges=True):
    """float32 test input: randn * 10^U(-6, 1) (bf16) or randn * 2^U(-6, 3) (fp16: inside its range).  The first 8 * 39 of every
    1024 flat elements hold EDGE_VALUES at a period of 39 (odd, and 1024 is a multiple of 8: every value meets every lane 0..7
    of a thread's 8 channels; a smaller tensor takes what fits)."""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    mag = 10.0 ** rng.uniform(-6, 1, size=n) if fmt == "bf16" else 2.0 ** rng.uniform(-6, 3, size=n)
    v = (rng.randn(n) * mag).astype(np.float32)
    if edges:
        period = len(EDGE_VALUES) + 1
        assert period % 2 == 1
        pos = np.arange(n) % 1024
        put = (pos < 8 * period) & (pos % period < len(EDGE_VALUES))
        v[put] = EDGE_VALUES[pos[put] % period]
    return v.reshape(shape)


def mode2_inputs(rows, c, fmt, seed=11):
    """(gradient planes, stored-activation planes) of the ELU-backward dropout tests: g = randn with the edge values tiled in,
    m = -U(0, 1) / 0.75 (a kept ELU output behind rate 0.25) with every fourth element positive and +0, -0 and the smallest
    positive number of the format among them"""
    rng = np.random.RandomState(seed)
    g = fill_values((rows, c), fmt, seed + 1)
    plain = rng.randn(rows, c).astype(np.float32)
    g = np.where(np.arange(g.size).reshape(g.shape) % 1024 < 160, g, plain).astype(np.float32)  # (fewer edge values: 15 %)
    m = (-rng.rand(rows, c) / 0.75).astype(np.float32)
    flat = m.reshape(-1)
    flat[::4] = np.abs(flat[::4])
    special = np.array([0.0, -0.0, 2.0 ** -24 if fmt == "f16" else 2.0 ** -133, -1.0 / 0.75], dtype=np.float32)
    n = min(flat.size, 4 * 9)
    flat[:n] = np.tile(special, 9)[:n]  # period 4 against a stride of 9 slots: both lane parities, all of 0..7 over the run
    return split(g, fmt), split(m, fmt)
