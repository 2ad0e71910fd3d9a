"""Integer operands that make the convolution kernels' arithmetic EXACT, an integer reference and a comparator that points
at the tile row and channel block of a mismatch.  Plain helper module: numpy (and torch on the CPU for the plane round trips),
no GPU.  tests/test_exact_ints.py holds the generators' own conditions; the cases at the end of the file are what GPU tests
of the kernels are to run.

The bit-budget argument.  If every operand is a small integer (times a power of two), every product and every partial sum of a
kernel is an integer (times that power of two) below 2^24 in magnitude, i.e. exact in the fp32 accumulators in ANY order -- tile
shape, split-K, ring depth, MFMA shape and the order of the three plane terms do not matter.  If in addition every value a
kernel stores has at most 8 significant bits (bf16), 16 (bf16 hi + lo planes) or 22 (fp16 hi + lo planes), the output rounding
is the identity as well.  The kernel must then equal the integer reference in every element: tolerance zero, derived.

Families:
  A  dense {0, 1} input, sparse weights: every output column of a layer has exactly P weights +1 and N weights -1 at random
     (tap, cin) positions, biases in {0, 1}: max_out <= P * max_in + 1 by construction.
  B  impulse input (isolated 1s and 2s at the first / last frame, on both sides of every tile edge, in the last real channel
     and in the channel in front of the ones channel), dense weights in [-3, 3]: |out| <= 6 * (impulses in a receptive
     field) + 1.  Exercises EVERY (tap, cin) weight position, which family A does not.
  planes  integers whose hi + lo split is exact in the plane format, in three variants that leave the lo x lo term (which the
     scheme omits by design) zero: both operands lo = 0; only the second operand (weights; the gradient of a weight-gradient
     launch) lo != 0; only the first operand (activations; gradients) lo != 0.
"""
import numpy as np

FP32_BUDGET = 2 ** 24          # integers below this magnitude are exact in an fp32 accumulator
BF16_MAX_EXACT = 255           # every integer up to here has at most 8 significant bits
FAMILY_B_MAX_W = 3
FAMILY_B_MAX_X = 2
FAMILY_B_MAX_IMPULSES = BF16_MAX_EXACT // (FAMILY_B_MAX_W * FAMILY_B_MAX_X)  # per receptive field: floor(255 / 6) = 42


# ------------------------------------------------------------------------------------------ SAME padding (TF), as the engine
def same_padding(t_in, kernel_size, stride):
    t_out = -(-t_in // stride)
    pad_total = max((t_out - 1) * stride + kernel_size - t_in, 0)
    return t_out, pad_total // 2, pad_total - pad_total // 2


# ------------------------------------------------------------------------------------------ reference (int64)
def _as_int(a, what):
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        r = np.rint(a)
        if not np.array_equal(r, a):
            raise ValueError("{} is not integer-valued".format(what))
        a = r
    return a.astype(np.int64)


def _matmul_int(a, b):
    """a @ b for int64 arrays.  Evaluated by the float64 BLAS (an int64 matmul is a slow scalar loop) under the condition
    that makes it exact in any order -- sum |a| |b| < 2^53 -- which is checked, and returned as int64."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    bound = np.abs(a).max(initial=0) * np.abs(b).max(initial=0) * a.shape[-1]
    if bound >= 2 ** 53:
        raise OverflowError("integer reference: a partial sum may exceed 2^53")
    return (a.astype(np.float64) @ b.astype(np.float64)).astype(np.int64)


def _padded(x, taps, stride):
    b, t, c = x.shape
    t_out, pad_l, pad_r = same_padding(t, taps, stride)
    xp = np.zeros((b, pad_l + t + pad_r + stride, c), dtype=np.int64)
    xp[:, pad_l:pad_l + t] = x
    return xp, t_out, pad_l


def reference_preactivation(x, w, bias, stride=1):
    """z[b, t, co] = bias[co] + sum_{tap, ci} x[b, t * stride + tap - pad_left, ci] * w[tap, ci, co], TF 'SAME', int64"""
    x, w, bias = _as_int(x, "x"), _as_int(w, "w"), _as_int(bias, "bias")
    taps = w.shape[0]
    xp, t_out, _ = _padded(x, taps, stride)
    z = np.zeros((x.shape[0], t_out, w.shape[2]), dtype=np.int64)
    for tap in range(taps):
        z += _matmul_int(xp[:, tap: tap + stride * t_out: stride], w[tap])
    return z + bias


def reference_forward(x, w, bias, stride=1):
    """conv + bias + ReLU"""
    return np.maximum(reference_preactivation(x, w, bias, stride), 0)


def reference_accumulator_bound(x, w, bias=None, stride=1):
    """max over outputs of sum |x| |w| (+ |bias|): what the largest partial sum of ANY summation order is bounded by"""
    b0 = np.zeros(np.asarray(w).shape[2], dtype=np.int64) if bias is None else np.abs(_as_int(bias, "bias"))
    return int(reference_preactivation(np.abs(_as_int(x, "x")), np.abs(_as_int(w, "w")), b0, stride).max(initial=0))


def reference_input_gradient(g, w, mask=None):
    """dx[b, t, ci] = sum_{tap, co} g[b, t - tap + pad_left, co] * w[tap, ci, co] (stride 1), times (mask > 0) if given"""
    g, w = _as_int(g, "g"), _as_int(w, "w")
    taps = w.shape[0]
    # the input gradient of a stride-1 SAME convolution is the SAME-padded correlation with flipped taps and swapped channels
    # -- for an even tap count with the padding sides swapped, hence the explicit index arithmetic here
    _, pad_l, pad_r = same_padding(g.shape[1], taps, 1)
    b, t, _ = g.shape
    gp = np.zeros((b, pad_r + t + pad_l, g.shape[2]), dtype=np.int64)
    gp[:, pad_r:pad_r + t] = g
    dx = np.zeros((b, t, w.shape[1]), dtype=np.int64)
    for tap in range(taps):
        lo = pad_r + pad_l - tap  # row of gp that holds g[t - tap + pad_l] for t = 0
        dx += _matmul_int(gp[:, lo:lo + t], w[tap].T)
    if mask is not None:
        dx = dx * (np.asarray(mask) > 0)
    return dx


def reference_weight_gradient(x, g, taps, stride=1):
    """dw[tap, ci, co] = sum_{b, t} x[b, t * stride + tap - pad_left, ci] * g[b, t, co]"""
    x, g = _as_int(x, "x"), _as_int(g, "g")
    xp, t_out, _ = _padded(x, taps, stride)
    assert t_out == g.shape[1]
    g2 = g.reshape(-1, g.shape[2])
    dw = np.zeros((taps, x.shape[2], g.shape[2]), dtype=np.int64)
    for tap in range(taps):
        xs = xp[:, tap: tap + stride * t_out: stride].reshape(-1, x.shape[2])
        dw[tap] = _matmul_int(xs.T, g2)
    return dw


def reference_bias_gradient(g):
    g = _as_int(g, "g")
    return g.reshape(-1, g.shape[-1]).sum(axis=0)


# ------------------------------------------------------------------------------------------ comparator
class NotExact(AssertionError):
    pass


def mismatch_report(got, want, where):
    """None when got == want in every element (np.array_equal), else the text assert_exact raises with"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "{}: shape {} instead of {}".format(where, got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.argwhere(got != want)  # (NaN != anything: a NaN counts as a mismatch)
    lines = ["{}: {} of {} elements differ".format(where, len(bad), got.size)]
    names = "(b, t, c, got, want)" if got.ndim == 3 else "(index..., got, want)"
    lines.append("  first ten as {}:".format(names))
    for idx in bad[:10]:
        idx = tuple(int(i) for i in idx)
        lines.append("    {}".format(idx + (got[idx].item(), want[idx].item())))

    def histogram(values, label):
        keys, counts = np.unique(values, return_counts=True)
        lines.append("  by {}: {}".format(label, ", ".join("{}: {}".format(int(k), int(n)) for k, n in zip(keys, counts))))
    if got.ndim == 3:
        for m in (16, 48, 64):
            histogram(bad[:, 1] % m, "t mod {}".format(m))
    if got.ndim >= 1:
        histogram(bad[:, -1] // 64, "c // 64")
    return "\n".join(lines)


def assert_exact(got, want, where):
    """np.array_equal semantics; on failure: how many elements differ, the first ten, and histograms of the mismatches by
    t mod 16 / 48 / 64 (a tile row) and by c // 64 (a channel block)"""
    report = mismatch_report(got, want, where)
    if report is not None:
        raise NotExact(report)


# ------------------------------------------------------------------------------------------ family A
def family_a_input(rng, shape, density=0.5):
    return (rng.random_sample(shape) < density).astype(np.int64)


def family_a_weights(rng, taps, cin, cout, p=2, n=2, by_input=False):
    """(taps, cin, cout) with exactly p entries +1 and n entries -1 per OUTPUT COLUMN, at random (tap, cin) positions.
    by_input=True: per INPUT channel over (tap, cout) instead -- the columns of the input-gradient launch, whose output
    channels are the layer's inputs."""
    if by_input:
        return np.ascontiguousarray(family_a_weights(rng, taps, cout, cin, p, n).transpose(0, 2, 1))
    w = np.zeros((taps * cin, cout), dtype=np.int64)
    for co in range(cout):
        pos = rng.choice(taps * cin, size=p + n, replace=False)
        w[pos[:p], co] = 1
        w[pos[p:], co] = -1
    return w.reshape(taps, cin, cout)


def family_a_bias(rng, cout):
    return rng.randint(0, 2, size=cout).astype(np.int64)


def family_a_stack(seed, batch, t, layers=7, channels=250, taps=7, p=2, n=2, density=0.5):
    """input (batch, t, channels) and [(w, bias)] of a run of identical family-A layers"""
    rng = np.random.RandomState(seed)
    x = family_a_input(rng, (batch, t, channels), density)
    weights = [(family_a_weights(rng, taps, channels, channels, p, n), family_a_bias(rng, channels)) for _ in range(layers)]
    return x, weights


def run_stack(x, weights, strides=None):
    """[(pre-activation, activation)] of every layer, the activation of one the input of the next"""
    out = []
    for i, (w, b) in enumerate(weights):
        z = reference_preactivation(x, w, b, strides[i] if strides else 1)
        x = np.maximum(z, 0)
        out.append((z, x))
    return out


def run_stack_backward(g_top, weights, masks):
    """input gradients of a run from the top: g[i - 1] = dgrad(g[i], w[i]) * (masks[i - 1] > 0); returns [g[n - 2], ..., g[-1]]
    for weights = [w[0] .. w[n - 1]] and masks = [activation in front of layer 0, ..., in front of layer n - 1]"""
    out = []
    g = g_top
    for i in range(len(weights) - 1, -1, -1):
        g = reference_input_gradient(g, weights[i][0], masks[i])
        out.append(g)
    return out


# ------------------------------------------------------------------------------------------ family B
def tile_edge_frames(t_out, tiles=(48, 64)):
    """the first and last valid frame and the frames on both sides of every tile edge inside [0, t_out)"""
    frames = {0, t_out - 1}
    for tile in tiles:
        for edge in range(tile, t_out, tile):
            frames.update((edge - 1, edge))
    return sorted(f for f in frames if 0 <= f < t_out)


def family_b_input(rng, batch, t_out, channels, frames, impulse_channels):
    """zero except for impulses of value 1 or 2 at (every utterance, every frame of `frames`, every channel of
    `impulse_channels` plus one random channel per frame)"""
    x = np.zeros((batch, t_out, channels), dtype=np.int64)
    for b in range(batch):
        for f in frames:
            for c in list(impulse_channels) + [int(rng.randint(0, channels))]:
                x[b, f, c] = int(rng.randint(1, FAMILY_B_MAX_X + 1))
    return x


def family_b_weights(rng, taps, cin, cout):
    return rng.randint(-FAMILY_B_MAX_W, FAMILY_B_MAX_W + 1, size=(taps, cin, cout)).astype(np.int64)


def shift_weights(rng, taps, channels):
    """every output channel c copies input channel c from ONE random tap: values move in time (across tile edges, through
    the recomputed halo rows of a fused run) without growing"""
    w = np.zeros((taps, channels, channels), dtype=np.int64)
    w[rng.randint(0, taps, size=channels), np.arange(channels), np.arange(channels)] = 1
    return w


def max_impulses_in_field(x, taps):
    """the most non-zero input elements any window of `taps` consecutive frames (all channels) of one utterance holds"""
    per_frame = (np.asarray(x) != 0).sum(axis=2)
    csum = np.concatenate([np.zeros((per_frame.shape[0], 1), dtype=np.int64), np.cumsum(per_frame, axis=1)], axis=1)
    t = per_frame.shape[1]
    hi = np.minimum(np.arange(t) + taps, t)
    return int((csum[:, hi] - csum[:, :t]).max())


def family_b_stack(seed, batch, t_out, dense_at, layers=7, channels=250, taps=7, tiles=(48, 64)):
    """a run whose layer `dense_at` has family-B weights and whose other layers only shift channels in time (no bias, so
    nothing grows): impulses at both utterance ends and on both sides of every 48- and 64-row tile edge"""
    rng = np.random.RandomState(seed)
    x = family_b_input(rng, batch, t_out, channels, tile_edge_frames(t_out, tiles), (0, channels - 1))
    weights = []
    for i in range(layers):
        w = family_b_weights(rng, taps, channels, channels) if i == dense_at else shift_weights(rng, taps, channels)
        weights.append((w, np.zeros(channels, dtype=np.int64)))
    return x, weights


# ------------------------------------------------------------------------------------------ bf16 / plane formats
def is_bf16_exact(a):
    """every element survives a round trip through torch.bfloat16"""
    import torch
    t = torch.as_tensor(np.asarray(a, dtype=np.float64))
    return bool(torch.equal(t.to(torch.float32).to(torch.bfloat16).to(torch.float64), t))


class PlaneFormat:
    """hi + lo plane pair of one of the two parity engines.  Values are integers times `unit` powers of two; `wide` integers
    (bits - 3 of them, so that a family-A sum of two of them plus a bias still has at most `bits`) have a non-zero lo plane,
    `narrow` ones (|n| <= 2) do not.  The engine's own power-of-two scales: stored weight planes hold w_scale * w, stored
    gradient planes g_scale * g."""

    def __init__(self, name, bits, act_unit, w_unit, g_unit, w_scale, g_scale, g_wide_bits):
        self.name, self.bits = name, bits
        self.act_unit, self.w_unit, self.g_unit = act_unit, w_unit, g_unit
        self.w_scale, self.g_scale = w_scale, g_scale
        self.wide_bits = bits - 3
        self.g_wide_bits = g_wide_bits

    @property
    def torch_dtype(self):
        import torch
        return torch.bfloat16 if self.name == "bf16x3" else torch.float16

    def split(self, values):
        """(hi, lo) torch tensors in the plane dtype: hi = rn(v), lo = rn(v - hi)"""
        import torch
        v = torch.as_tensor(np.asarray(values, dtype=np.float64)).to(torch.float32)
        hi = v.to(self.torch_dtype)
        lo = (v - hi.to(torch.float32)).to(self.torch_dtype)
        return hi, lo

    def planes_exact(self, values):
        """hi + lo reconstructs every value after the round trip through the plane dtype, and nothing overflows"""
        import torch
        v = torch.as_tensor(np.asarray(values, dtype=np.float64))
        hi, lo = self.split(values)
        back = hi.to(torch.float64) + lo.to(torch.float64)
        return bool(torch.isfinite(back).all()) and bool(torch.equal(back, v))

    def lo_is_zero(self, values):
        return not bool(self.split(values)[1].float().any())


# bf16 planes: 8 + 8 bits, no scales, everything an integer.  fp16 planes: 11 + 11 bits; activations are integers times 2^-8
# (19-bit integers: below 2048), weights integers times 2^-14 (stored times 2^6: integers times 2^-8, below 2048 << 6e4),
# gradients integers times 2^-12 (stored times 2^12: plain integers, 13 bits so that a family-A sum stays below 65504).
PLANE_FORMATS = {
    "bf16x3": PlaneFormat("bf16x3", 16, 1.0, 1.0, 1.0, 1.0, 1.0, 13),
    "f16x3": PlaneFormat("f16x3", 22, 2.0 ** -8, 2.0 ** -14, 2.0 ** -12, 2.0 ** 6, 2.0 ** 12, 13),
}
PLANE_VARIANTS = ("lo_none", "lo_second", "lo_first")  # which operand of a launch has a non-zero lo plane


def wide_ints(rng, shape, bits, signed=False, density=1.0):
    """integers with the top bit of `bits` set (so the hi plane cannot hold them) and an odd low end (lo != 0)"""
    v = rng.randint(2 ** (bits - 1), 2 ** bits, size=shape).astype(np.int64) | 1
    if signed:
        v = v * rng.choice([-1, 1], size=shape)
    if density < 1.0:
        v = v * (rng.random_sample(shape) < density)
    return v


def sparse_columns(rng, batch, t, channels, per_channel, values):
    """(batch, t, channels) zero except `per_channel` entries per channel at random (b, t), drawn from `values`"""
    g = np.zeros((batch * t, channels), dtype=np.int64)
    for c in range(channels):
        pos = rng.choice(batch * t, size=per_channel, replace=False)
        g[pos, c] = rng.choice(values, size=per_channel)
    return g.reshape(batch, t, channels)


# ------------------------------------------------------------------------------------------ the cases for GPU tests of the kernels
NT_REAL, NT_PADDED = 250, 256  # channels as the engine lays them out: 250 real, 5 of zero padding, the ones channel last


def nt_case(family, taps, t_out, batch, seed, tiles=(16,)):
    """one sl_conv1d_nt launch in the engine's channel layout, as the kernel sees it (256 x 256 channels): x and mask
    (batch, t_out, 256), w (taps, 256, 256), bias (256,).  The ones channel (255) is 1 on every frame of x and of the mask,
    has zero weights and bias 1; output columns 250 .. 254 have zero weights and bias.  Family B puts its impulses on both
    sides of every multiple of `tiles` rows (16: every row-tile height of the kernel's variants is a multiple of it) in
    channels 0, 249 and 254 -- for the kernel channel 254 is one more contraction lane, the one in front of the ones."""
    rng = np.random.RandomState(seed)
    c = NT_PADDED
    x = np.zeros((batch, t_out, c), dtype=np.int64)
    w = np.zeros((taps, c, c), dtype=np.int64)
    bias = np.zeros(c, dtype=np.int64)
    if family == "A":
        x[:, :, :NT_REAL] = family_a_input(rng, (batch, t_out, NT_REAL))
        w[:, :NT_REAL, :NT_REAL] = family_a_weights(rng, taps, NT_REAL, NT_REAL)
        bias[:NT_REAL] = family_a_bias(rng, NT_REAL)
    else:
        x[:, :, :c - 1] = family_b_input(rng, batch, t_out, c - 1, tile_edge_frames(t_out, tiles), (0, NT_REAL - 1, c - 2))
        w[:, :c - 1, :NT_REAL] = family_b_weights(rng, taps, c - 1, NT_REAL)
        bias[:NT_REAL] = family_a_bias(rng, NT_REAL)
    x[:, :, c - 1] = 1
    bias[c - 1] = 1
    mask = np.zeros((batch, t_out, c), dtype=np.int64)
    mask[:, :, :NT_REAL] = rng.randint(0, 3, size=(batch, t_out, NT_REAL))
    mask[:, :, c - 1] = 1
    return dict(x=x, w=w, bias=bias, mask=mask)


def nt_expected(case):
    """{epilogue name: expected output} of nt_case for the three epilogues"""
    zero = np.zeros_like(case["bias"])
    acc = reference_preactivation(case["x"], case["w"], zero)
    return {"none": acc, "bias_relu": np.maximum(acc + case["bias"], 0), "relu_mask": acc * (case["mask"] > 0)}


ENGINE_LAYERS = [("striding_conv", 48, 2, None, 250)] + [("inner_conv_{}".format(i), 7, 1, 250, 250) for i in range(1, 8)] + \
    [("big_conv_1", 32, 1, 250, 2000), ("big_conv_2", 1, 1, 2000, 2000), ("output_conv", 1, 1, 2000, None)]


def engine_case(seed=0, batch=2, t_in=154, bins=128, graphemes=29, p=2, n=2):
    """family A through the whole Wav2Letter stack: input (batch, t_in, bins) in {0, 1}, [(w, bias)] of the eleven layers
    (the stride-2 first layer with 48 taps and the 2000-channel layers included) with P = p, N = n in every layer"""
    rng = np.random.RandomState(seed)
    x = family_a_input(rng, (batch, t_in, bins))
    weights, strides = [], []
    for _, taps, stride, cin, cout in ENGINE_LAYERS:
        cin, cout = cin or bins, cout or graphemes
        weights.append((family_a_weights(rng, taps, cin, cout, p, n), family_a_bias(rng, cout)))
        strides.append(stride)
    return x, weights, strides


def family_a_backward_run(seed, x, layers, channels=250, taps=7):
    """the input-gradient direction of a family-A run: (gradient at its top in {-1, 0, 1}, [(w, None)] with P = N = 2 per INPUT
    channel -- the output columns of that launch --, masks = the forward activations in front of every layer)"""
    rng = np.random.RandomState(seed)
    masks = [x] + [y for _, y in layers[:-1]]
    g_top = rng.randint(-1, 2, size=layers[-1][1].shape).astype(np.int64)
    wts = [(family_a_weights(rng, taps, channels, channels, by_input=True), None) for _ in layers]
    return g_top, wts, masks


def family_b_backward_run(seed, batch, t_out, dense_at, layers=7, channels=250, taps=7):
    """family B in the input-gradient direction: impulses in the gradient at the top of the run, one dense layer, shifting
    layers elsewhere, random masks in 0 .. 7 (one element in eight blocks the gradient: most impulses survive the run)"""
    g_top, weights = family_b_stack(seed, batch, t_out, dense_at, layers, channels, taps)
    rng = np.random.RandomState(seed + 1)
    masks = [rng.randint(0, 8, size=(batch, t_out, channels)).astype(np.int64) for _ in range(layers)]
    return g_top, [(w, None) for w, _ in weights], masks


def denormal_weights(rng, taps, cin, cout):
    """family-A positions and signs with magnitudes n * 2^-30, n = 2^20 + k, 0 < k < 512: about 2^-10, and 2^6 * w = n * 2^-24
    splits into a normal fp16 hi plane and a lo plane below 2^-14 -- fp16's denormal range.  Returns (w, n as signed int64)."""
    n = family_a_weights(rng, taps, cin, cout) * (2 ** 20 + rng.randint(1, 512, size=(taps, cin, cout)))
    return n * 2.0 ** -30, n
