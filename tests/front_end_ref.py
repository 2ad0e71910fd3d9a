"""The audio front end (speechless_amd/csrc/spectrogram.hip and the 1 x 1 mel projection) against float64, bin by bin
(TEST INFRASTRUCTURE ONLY, numpy only).

stft_cases()            the inputs and output layouts sl_stft_power_db is run at, shared by the CPU and GPU tests
stft_expected()         float64 amplitudes |D| per utterance and the per-frame error budget delta_t
compare_levels()        one utterance's slab of the level buffer against them: every bin, the floor, the layout
stft_f32_restatement()  the kernel's algorithm in numpy float32, with switches for the mistakes the case list must catch
mel_expected()          float64 projection of fp32 level rows and its accumulation-order-free bound
znorm_expected() / compare_znorm()   (x - mean) / std per utterance in float64

The error budget of a frame (worst case, component-wise; not a measurement):

    delta_t = 16 log2(n_fft) 2^-24 sum_n |x_t[n]| (w[n] + 2^-23)

x_t the reflect-padded frame, w the periodic Hann window.  Every bin is a sum over the frame taken through
log2(n_fft) - 1 butterfly stages and the real-split step; a stage costs a twiddle (<= 1 ulp), a complex multiply
(<= 2 sqrt 2 u) and an add (u): about 6 u.  16 leaves room for the split step and FMA contraction.  Levels are compared as
amplitudes, floored on both sides:  |10^(got/20) - max(a, floor)| <= delta_t + 1e-5 max(a, floor); the relative term is
four times what half an ulp of an fp32 level below 150 (7.6e-6 dB), a base-2 logarithm good to 1 ulp (1.2e-5 dB) and two
roundings of the power (5e-7 dB) come to (2e-5 dB = 2.3e-6 in amplitude)."""
from collections import namedtuple

import numpy as np

from oracle import spectrogram_oracle as so

SENTINEL = np.float32(-777.25)
RELATIVE = 1e-5
U = 2.0 ** -24

StftCase = namedtuple("StftCase", "name n_fft hop min_db utterances offsets max_frames row_stride batch_stride")


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ signals
def chirps(n, seed, gain=1.0, silence=None, sample_rate=16000):
    """tests/test_spectrogram.py's synthetic_audio for a sample count: four drifting tones over noise 40 dB down."""
    rng = np.random.RandomState(seed)
    seconds = n / sample_rate
    t = np.arange(n) / sample_rate
    y = 0.01 * rng.randn(n)
    for _ in range(4):
        f0, f1 = rng.uniform(100, 6000, size=2)
        y += rng.uniform(0.1, 0.4) * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / seconds))
    y *= np.hanning(n) ** 0.25
    if silence is not None:
        y[silence[0]:silence[1]] = 0.0
    return (y * gain).astype(np.float32)


def tone(n, n_fft, cycles_per_window, amplitude=0.5):
    """cycles_per_window an integer: exactly on a bin centre (deep nulls three bins away and beyond)."""
    return (amplitude * np.cos(2 * np.pi * cycles_per_window * np.arange(n) / n_fft + 0.3)).astype(np.float32)


def impulse(n, at):
    y = np.zeros(n, dtype=np.float32)
    y[at] = 1.0
    return y


def dc(n, level=0.75):
    return np.full(n, level, dtype=np.float32)


def nyquist(n, level=0.75):
    return (level * (1 - 2 * (np.arange(n) % 2))).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cases
def _case(name, n_fft, hop, utterances, min_db=-150.0, offsets=None, extra_frames=0, tight_rows=False, slack=0):
    bins = n_fft // 2 + 1
    lengths = [len(u) for u in utterances]
    assert min(lengths) > n_fft // 2 and max(lengths) <= 40 * hop and len(utterances) <= 8
    if offsets is None:
        offsets = np.concatenate([[0], np.cumsum(lengths[:-1])])
    max_frames = max(1 + n // hop for n in lengths) + extra_frames
    row_stride = bins + 1 if tight_rows else round_up(bins, 64)
    return StftCase(name, n_fft, hop, float(min_db), [np.asarray(u, dtype=np.float32) for u in utterances],
                    np.asarray(offsets, dtype=np.int64), max_frames, row_stride, max_frames * row_stride + slack)


_CASES = None


def stft_cases():
    """Every window length at hop = n_fft / 4 over the edge lengths and over the stationary / singular signals, n_fft = 512
    at hops 160, 256 and 512 (128 at 64), gains 2^-10 and 2^15, both floors, a ragged batch with odd offsets and gaps, and
    the output layouts (max_frames off a multiple of 16; whole work-groups of zero rows; bins + 1 columns; slack behind
    every utterance's rows).  Built once; the arrays are shared and must not be written."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []
    for n_fft in (64, 128, 256, 512, 1024):
        hop, half = n_fft // 4, n_fft // 2
        # minimum legal length and one more (both reflect branches in one frame); one sample either side of a multiple
        # of hop; 15, 16 and 17 frames: the edge of a work-group's 16 frames.  max_frames = 17: the break path.
        lengths = [half + 1, half + 2, 7 * hop - 1, 7 * hop, 7 * hop + 1, 14 * hop + 3, 15 * hop, 17 * hop - 1]
        cases.append(_case("n{}_lengths".format(n_fft), n_fft, hop,
                           [chirps(n, 100 + n_fft + i) for i, n in enumerate(lengths)]))
        # 33 frames; bins + 1 columns; 23 rows (one whole work-group and more) of zeros behind; 37 floats of slack
        n = 32 * hop + 5
        mid = 13 * hop + 1  # window positions 1 (where the window is 4e-5 at n_fft = 512), hop + 1, 2 hop + 1, 3 hop + 1
        cases.append(_case("n{}_signals".format(n_fft), n_fft, hop,
                           [tone(n, n_fft, n_fft // 8), tone(n, n_fft, n_fft / 8 + 0.5), impulse(n, 0), impulse(n, n - 1),
                            impulse(n, mid), dc(n), nyquist(n), chirps(n, 200 + n_fft, silence=(6 * hop, 19 * hop))],
                           extra_frames=23, tight_rows=True, slack=37))
    for n_fft, hop in ((512, 160), (512, 256), (512, 512), (128, 64)):
        half = n_fft // 2
        lengths = [half + 1, 9 * hop - 1, 9 * hop, 9 * hop + 1, 32 * hop + 7]
        n = 16 * hop + 11
        cases.append(_case("n{}_hop{}".format(n_fft, hop), n_fft, hop,
                           [chirps(m, 300 + hop + i) for i, m in enumerate(lengths)]
                           + [tone(n, n_fft, 40.5), impulse(n, 5 * hop + 3), nyquist(n)],
                           tight_rows=hop == 160, slack=64 if hop == 256 else 0))
    # gains: quiet (2^-10) and int16-scaled (2^15) audio; the -80 dB floor (amplitude 1e-4) cuts through the quiet noise
    lengths = [257, 5 * 128, 17 * 128 + 3]
    for name, gain, min_db in (("quiet", 2.0 ** -10, -150.0), ("quiet_floor80", 2.0 ** -10, -80.0),
                               ("int16", 2.0 ** 15, -150.0), ("int16_floor80", 2.0 ** 15, -80.0)):
        cases.append(_case("n512_" + name, 512, 128,
                           [chirps(n, 400 + i, gain=gain, silence=(900, 1700) if n > 2000 else None)
                            for i, n in enumerate(lengths)], min_db=min_db))
    # ragged: odd offsets, gaps of 1 .. 300 samples, the minimum length in the middle; 21 frames at most
    lengths = [1301, 257, 2600, 640, 258, 1999]
    offsets, at = [], 3
    for n, gap in zip(lengths, (1, 300, 7, 2, 129, 0)):
        offsets.append(at)
        at += n + gap
    cases.append(_case("n512_ragged", 512, 128, [chirps(n, 500 + i) for i, n in enumerate(lengths)], offsets=offsets))
    for c in cases:
        for u in c.utterances:
            u.setflags(write=False)
    _CASES = cases
    return cases


def stft_case(name):
    return {c.name: c for c in stft_cases()}[name]


def audio_buffer(case, fill=np.nan, tail=64):
    """The flat fp32 audio buffer of a case: `fill` before, between and behind the utterances."""
    end = max(int(o) + len(u) for o, u in zip(case.offsets, case.utterances))
    flat = np.full(end + tail, fill, dtype=np.float32)
    for o, u in zip(case.offsets, case.utterances):
        flat[o:o + len(u)] = u
    return flat


# ------------------------------------------------------------------------------------------------ expected
def stft_expected(case):
    """[(a, delta)] per utterance: a float64 (frames, bins) = |D| of oracle.spectrogram_oracle.stft over the fp32 samples
    widened to float64; delta float64 (frames,), the error budget of the module docstring."""
    out = []
    n_fft, hop, half = case.n_fft, case.hop, case.n_fft // 2
    w = so.hann_periodic(n_fft)
    for u in case.utterances:
        y = u.astype(np.float64)
        a = np.abs(so.stft(y, n_fft=n_fft, hop_length=hop)).T
        padded = np.abs(np.pad(y, half, mode="reflect"))
        frames = 1 + len(y) // hop
        assert a.shape == (frames, half + 1)
        idx = hop * np.arange(frames)[:, None] + np.arange(n_fft)[None, :]
        delta = 16 * np.log2(n_fft) * U * (padded[idx] * (w + 2.0 ** -23)[None, :]).sum(axis=1)
        out.append((a, delta))
    return out


def level_report(got_db, a, delta, min_db, max_frames, row_stride, sentinel=SENTINEL):
    """(worst ratio, [problems]) of one utterance's slab (1-D, batch_stride floats) of the level buffer."""
    got_db = np.asarray(got_db)
    frames, bins = a.shape
    problems = []
    if np.isnan(got_db).any():
        problems.append("{} NaN".format(int(np.isnan(got_db).sum())))
    if got_db.shape[0] < max_frames * row_stride or frames > max_frames or bins > row_stride:
        return np.inf, problems + ["slab of {} floats for {} rows of {}".format(got_db.shape[0], max_frames, row_stride)]
    rows = got_db[:max_frames * row_stride].reshape(max_frames, row_stride)
    rest = got_db[max_frames * row_stride:]
    if rest.size and not np.array_equal(rest.view(np.uint32), np.full(rest.shape, sentinel, np.float32).view(np.uint32)):
        problems.append("written behind row max_frames")
    if np.any(rows[:frames, bins:] != 0):
        problems.append("non-zero in columns >= bins")
    if np.any(rows[frames:] != 0):
        problems.append("non-zero in rows {} .. {}".format(frames, max_frames))
    got = rows[:frames, :bins].astype(np.float64)
    floor = 10.0 ** (min_db / 20)
    with np.errstate(over="ignore", invalid="ignore"):
        amp = 10.0 ** (got / 20)
    a_f = np.maximum(a, floor)
    d = delta[:, None]
    must_floor = a + d < floor
    if np.any(got[must_floor] != min_db):
        problems.append("{} bins under the floor are not exactly {}".format(int((got[must_floor] != min_db).sum()), min_db))
    excess = np.abs(amp - a_f) - RELATIVE * a_f
    excess = np.where(np.isnan(excess), np.inf, excess)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(excess > 0, excess / d, 0.0)  # (delta_t = 0: digital silence, where any excess is infinite)
    worst = float(ratio.max())
    if worst > 1:
        t, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        problems.append("frame {} bin {}: level {} for amplitude {} (error {:.3g}, delta {:.3g}): {:.3g} x the bound".format(
            t, k, got[t, k], a[t, k], abs(amp[t, k] - a_f[t, k]), delta[t], worst))
    return worst, problems


def compare_levels(got_db, a, delta, min_db, max_frames, row_stride, sentinel=SENTINEL):
    """Asserts the slab; returns the worst (|a^ - a_f| - 1e-5 a_f) / delta_t."""
    worst, problems = level_report(got_db, a, delta, min_db, max_frames, row_stride, sentinel)
    assert not problems, "; ".join(problems)
    return worst


def case_report(case, out_flat, expected=None, sentinel=SENTINEL):
    """level_report over every utterance of a case's whole output buffer (batch * batch_stride floats)."""
    expected = stft_expected(case) if expected is None else expected
    out_flat = np.asarray(out_flat).reshape(-1)
    worst, problems = 0.0, []
    for b, (a, delta) in enumerate(expected):
        slab = out_flat[b * case.batch_stride:(b + 1) * case.batch_stride]
        w, p = level_report(slab, a, delta, case.min_db, case.max_frames, case.row_stride, sentinel)
        worst = max(worst, w)
        problems += ["utterance {}: {}".format(b, x) for x in p]
    return worst, problems


def compare_case(case, out_flat, expected=None, sentinel=SENTINEL):
    worst, problems = case_report(case, out_flat, expected, sentinel)
    assert not problems, "{}: {}".format(case.name, "; ".join(problems))
    return worst


# ------------------------------------------------------------------------------------------------ the kernel, in numpy
MUTANTS = ("symmetric_window", "edge_repeating_reflect", "centre_shifted", "nyquist_twiddle", "last_stage_skipped", "no_floor",
           "cosine_window")


def window_f32(n_fft, symmetric=False, cosine=False):
    """sin^2(pi n / n_fft), the sine and the square rounded to fp32.  cosine=True: 0.5 - 0.5 cos(2 pi n / n_fft) with the
    cosine rounded to fp32, the form the kernel had first: equal in exact arithmetic, but the cosine next to 1 carries an
    absolute 2^-25, which one sample from the window's edge is 4e-4 of the window."""
    period = n_fft - 1 if symmetric else n_fft
    if cosine:
        return np.float32(0.5) - np.float32(0.5) * np.cos(2 * np.pi * np.arange(n_fft) / period).astype(np.float32)
    s = np.sin(np.pi * np.arange(n_fft) / period).astype(np.float32)
    return s * s


def stft_f32_restatement(case, mutant=None, sentinel=SENTINEL):
    """stft_power_db_kernel in numpy float32: window and twiddles rounded to fp32, half-length complex radix-2
    decimation-in-time transform over bit-reversed input, the real-split step, 3.0103 log2 with the floor.  Returns the
    whole output buffer (batch * batch_stride floats) as the kernel leaves it over a sentinel fill."""
    assert mutant is None or mutant in MUTANTS
    f32 = np.float32
    n_fft, hop, half = case.n_fft, case.hop, case.n_fft // 2
    log2h = int(np.log2(half))
    bins = half + 1
    win = window_f32(n_fft, symmetric=mutant == "symmetric_window", cosine=mutant == "cosine_window")
    ang = -2.0 * np.arange(half) / n_fft
    twr, twi = np.cos(np.pi * ang).astype(f32), np.sin(np.pi * ang).astype(f32)
    brev = np.array([int(format(n, "0{}b".format(log2h))[::-1], 2) for n in range(half)])
    out = np.full(len(case.utterances) * case.batch_stride, sentinel, dtype=f32)
    for b, y in enumerate(case.utterances):
        n_frames = 1 + len(y) // hop
        rows = out[b * case.batch_stride:b * case.batch_stride + case.max_frames * case.row_stride].reshape(
            case.max_frames, case.row_stride)
        rows[:] = 0
        idx = hop * np.arange(n_frames)[:, None] + np.arange(n_fft)[None, :] - half
        if mutant == "centre_shifted":
            idx = idx + 1
        if mutant == "edge_repeating_reflect":
            idx = np.where(idx < 0, -idx - 1, idx)
            idx = np.where(idx >= len(y), 2 * len(y) - 1 - idx, idx)
        else:
            idx = np.where(idx < 0, -idx, idx)
            idx = np.where(idx >= len(y), 2 * (len(y) - 1) - idx, idx)
        idx = np.clip(idx, 0, len(y) - 1)  # (the shifted mutant at the minimum length)
        x = win[None, :] * y[idx]
        zr, zi = np.empty((n_frames, half), f32), np.empty((n_frames, half), f32)
        zr[:, brev], zi[:, brev] = x[:, 0::2], x[:, 1::2]
        for s in range(1, log2h + 1):
            if mutant == "last_stage_skipped" and s == log2h and log2h % 2 == 1:
                continue
            mh = 1 << (s - 1)
            k = np.arange(mh) * (n_fft >> s)
            wr, wi = twr[k], twi[k]
            zr4, zi4 = zr.reshape(n_frames, -1, 2, mh), zi.reshape(n_frames, -1, 2, mh)
            ur, ui, vr, vi = zr4[:, :, 0], zi4[:, :, 0], zr4[:, :, 1], zi4[:, :, 1]
            pr, pi = wr * vr - wi * vi, wr * vi + wi * vr
            zr = np.stack([ur + pr, ur - pr], axis=2).reshape(n_frames, half)
            zi = np.stack([ui + pi, ui - pi], axis=2).reshape(n_frames, half)
        k = np.arange(bins)
        ka, kb = k & (half - 1), (half - k) & (half - 1)
        ar, ai, cr, ci = zr[:, ka], zi[:, ka], zr[:, kb], zi[:, kb]
        er, ei = f32(0.5) * (ar + cr), f32(0.5) * (ai - ci)
        dr, di = f32(0.5) * (ar - cr), f32(0.5) * (ai + ci)
        orr, oi = di, -dr
        wr = np.where(k == half, f32(1 if mutant == "nyquist_twiddle" else -1), twr[ka]).astype(f32)
        wi = np.where(k == half, f32(0), twi[ka]).astype(f32)
        xr, xi = er + wr * orr - wi * oi, ei + wr * oi + wi * orr
        pw = xr * xr + xi * xi
        with np.errstate(divide="ignore"):
            level = f32(3.0102999566398120) * np.log2(pw)
        if mutant != "no_floor":
            level = np.where(pw == 0, f32(case.min_db), np.maximum(level, f32(case.min_db)))
        assert level.dtype == f32
        rows[:n_frames, :bins] = level
    return out


# ------------------------------------------------------------------------------------------------ mel projection
def mel_expected(level_f32, bank_f32):
    """level_f32 (..., cin_pad) fp32 level rows as the kernel left them, bank_f32 (mel, cin_pad) the fp32 filter bank
    the projection holds.  Returns (want, bound): the float64 product and (cin_pad + 2) 2^-24 sum_j |w_ij| |level_j|,
    which holds for cin_pad fp32 multiply-adds in any order."""
    assert level_f32.dtype == np.float32 and bank_f32.dtype == np.float32
    level, bank = level_f32.astype(np.float64), bank_f32.astype(np.float64)
    cin_pad = level.shape[-1]
    return level @ bank.T, (cin_pad + 2) * U * (np.abs(level) @ np.abs(bank).T)


def compare_mel(got, level_f32, bank_f32):
    """Asserts |got - want| <= bound everywhere; returns the worst error / bound."""
    want, bound = mel_expected(level_f32, bank_f32)
    got = np.asarray(got)
    assert got.shape == want.shape and not np.isnan(got).any()
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(err <= bound), "mel projection: error {:.3g} over the bound at {}".format(
        float((err - bound).max()), np.unravel_index(int(np.argmax(err - bound)), err.shape))
    return float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0


# ------------------------------------------------------------------------------------------------ z-normalisation
def znorm_expected(src_f32, frames, f):
    """src_f32 (B, rows, stride >= f) fp32.  [(want, mean, std)] per utterance: (x - mean) / std in float64 over the first
    frames[b] rows and f columns (population standard deviation, as numpy's std)."""
    assert src_f32.dtype == np.float32
    out = []
    for b, n in enumerate(frames):
        x = src_f32[b, :n, :f].astype(np.float64)
        if n == 0:
            out.append((x, 0.0, 1.0))
            continue
        mean = x.mean()
        std = np.sqrt(((x - mean) ** 2).mean())
        with np.errstate(divide="ignore", invalid="ignore"):
            out.append(((x - mean) / std, float(mean), float(std)))
    return out


def znorm_report(got, src_f32, frames, f):
    """(worst error / tolerance, [problems]); got (B, max_frames, f).  Tolerance 2^-23 |want| + 1e-10 (1 + |mean| / std):
    one fp32 rounding of a double result, and double statistics over at most about 1e5 values."""
    got = np.asarray(got)
    problems, worst = [], 0.0
    if np.isnan(got).any():
        problems.append("{} NaN".format(int(np.isnan(got).sum())))
    for b, (want, mean, std) in enumerate(znorm_expected(src_f32, frames, f)):
        n = frames[b]
        if np.any(got[b, n:] != 0):
            problems.append("utterance {}: non-zero in rows >= {}".format(b, n))
        if n == 0:
            continue
        tol = 2.0 ** -23 * np.abs(want) + 1e-10 * (1 + abs(mean) / std)
        err = np.abs(got[b, :n].astype(np.float64) - want)
        err = np.where(np.isnan(err), np.inf, err)
        ratio = float((err / tol).max())
        worst = max(worst, ratio)
        if ratio > 1:
            problems.append("utterance {} ({} x {}): {:.3g} x the tolerance".format(b, n, f, ratio))
    return worst, problems


def compare_znorm(got, src_f32, frames, f):
    worst, problems = znorm_report(got, src_f32, frames, f)
    assert not problems, "; ".join(problems)
    return worst


ZNORM_VALUES = ("level", "near_constant", "large_spread")


def znorm_source(frames, f, stride, rows, values, seed, fill=np.nan):
    """(B, rows, stride) fp32 with `fill` in the padding columns and in the rows behind every utterance."""
    rng = np.random.RandomState(seed)
    src = np.full((len(frames), rows, stride), fill, dtype=np.float32)
    for b, n in enumerate(frames):
        if values == "level":
            x = -60 + 20 * rng.randn(n, f)
        elif values == "near_constant":
            x = -140 + 0.01 * rng.randn(n, f)
        else:
            x = rng.uniform(-1e4, 1e4, size=(n, f))
        src[b, :n, :f] = x
    return src
