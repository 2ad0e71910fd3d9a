"""sl_stft's power / amplitude / complex modes and sl_istft (speechless_amd/csrc/spectrogram.hip) against float64, value
by value (TEST INFRASTRUCTURE ONLY, numpy only).  The forward oracle, the case list and the frame
budget delta_t are tests/front_end_ref.py's; this module adds

forward_report()          one forward mode's whole output buffer against |D|, |D|^2 or D itself
stft_f32_modes()          the forward kernel in numpy float32 with a choice of output (front_end_ref's restatement emits levels only)
istft_f64()               librosa.istft(D, hop_length, win_length=n_fft) in float64: the expectation of the inverse
inverse_cases()           the spectra, layouts and output offsets sl_istft is run at
inverse_expected()        float64 samples and the per-sample bound
inverse_report()          the whole audio buffer against them: every sample, and the sentinel everywhere else
istft_f32_restatement()   the inverse kernel's algorithm in numpy float32, with a switch per mistake the case list must catch

The inverse, as librosa.istft states it with its defaults (window = periodic Hann of n_fft samples, center=True): frame t is
numpy.fft.irfft of its n_fft / 2 + 1 bins, multiplied by the window and added at sample t hop of a buffer of
n_fft + hop (frames - 1) samples; the buffer is divided by the sum of the SQUARED windows S[p] = sum_t w[p - t hop]^2
wherever S exceeds the smallest normal float32; n_fft / 2 samples are cut off both ends, which leaves hop (frames - 1).
The librosa of 2017 that the reference ran on cannot be imported here: this normalisation is taken from knowledge of librosa
and has not been verified against it.  What can be verified is: with it, the inverse of the forward oracle returns the audio
to 4.5e-16 wherever hop < n_fft (test_istft_ref.py).

The bound of output sample j, p = j + n_fft / 2 (worst case, component-wise; not a measurement):

    eps_t   = 16 log2(n_fft) 2^-24 (1 / n_fft) sum_k c_k |D_t[k]|,        c_k = 1 for the DC and Nyquist bins, 2 otherwise
    bound_j = ( sum_t w[p - t hop] eps_t  +  8 * 2^-24 sum_t |w[p - t hop] x_t[p - t hop]| ) / S[p]

both sums over the frames that cover p, x_t the float64 inverse transform of frame t; without the division where S[p] is
not above the smallest normal float32.  eps_t is front_end_ref's argument for the forward transform applied to the inverse:
a sample of x_t is a sum over the bins, sum_k c_k |D_t[k]| / n_fft bounds it term by term, and it passes through the
merge step and log2(n_fft) - 1 butterfly stages at about 6 u each, 16 for room.  The second term pays for the product with
the window (and the window's own rounding), the up to 8 adds in ascending frame order and the division, each at most u of
sum_t |w x_t|.

The forward modes, with a = |D| in float64 and delta_t of front_end_ref (component-wise on re and im):

    complex      |re^ - re|, |im^ - im| <= delta_t
    amplitude    |a^ - a|               <= delta_t + 1e-5 a
    power        |p^ - a^2|             <= 2 a delta_t + delta_t^2 + 1e-5 a^2

(|a^ - a| <= sqrt 2 delta_t would follow from the components alone; delta_t's 16 already holds the split step and the
modulus, as it does for the levels, which are compared as amplitudes under the same delta_t.)  Digital silence has
delta_t = 0 and a = 0: exact zeros in all three.
"""
from collections import namedtuple

import numpy as np

import front_end_ref as fr
from oracle import spectrogram_oracle as so

U = fr.U
SENTINEL = fr.SENTINEL
TINY = float(np.finfo(np.float32).tiny)
POWER, AMPLITUDE, COMPLEX, POWER_LEVEL = 0, 1, 2, 3   # SL_STFT_* of include/speechless_hip.h
MODE_NAMES = {POWER: "power", AMPLITUDE: "amplitude", COMPLEX: "complex"}


# ------------------------------------------------------------------------------------------------ forward modes
def forward_layout(case, mode):
    """(row_stride, batch_stride) a case is run at in `mode`: complex rows take twice the columns (and keep the slack)."""
    return (2 * case.row_stride, 2 * case.batch_stride) if mode == COMPLEX else (case.row_stride, case.batch_stride)


def complex_expected(case):
    """[D] per utterance: complex128 (frames, bins), the oracle's STFT of the fp32 samples widened to float64."""
    return [so.stft(u.astype(np.float64), n_fft=case.n_fft, hop_length=case.hop).T for u in case.utterances]


def forward_report(case, out_flat, mode, expected, spectra=None, sentinel=SENTINEL):
    """(worst error / bound, [problems]) of a whole forward output buffer.  expected: fr.stft_expected(case);
    spectra: complex_expected(case), needed for COMPLEX only."""
    out_flat = np.asarray(out_flat).reshape(-1)
    row_stride, batch_stride = forward_layout(case, mode)
    bins = case.n_fft // 2 + 1
    cols = 2 * bins if mode == COMPLEX else bins
    worst, problems = 0.0, []
    if out_flat.shape[0] != len(case.utterances) * batch_stride:
        return np.inf, ["buffer of {} floats for {} slabs of {}".format(out_flat.shape[0], len(case.utterances), batch_stride)]
    for b, (a, delta) in enumerate(expected):
        say = lambda text: problems.append("utterance {}: {}".format(b, text))
        slab = out_flat[b * batch_stride:(b + 1) * batch_stride]
        frames = a.shape[0]
        if np.isnan(slab).any():
            say("{} NaN".format(int(np.isnan(slab).sum())))
        rows = slab[:case.max_frames * row_stride].reshape(case.max_frames, row_stride)
        rest = slab[case.max_frames * row_stride:]
        if rest.size and not np.array_equal(rest.view(np.uint32), np.full(rest.shape, sentinel, np.float32).view(np.uint32)):
            say("written behind row max_frames")
        if np.any(rows[:frames, cols:] != 0):
            say("non-zero in columns >= {}".format(cols))
        if np.any(rows[frames:] != 0):
            say("non-zero in rows {} .. {}".format(frames, case.max_frames))
        got = rows[:frames, :cols].astype(np.float64)
        d = delta[:, None]
        if mode == COMPLEX:
            want = np.empty((frames, cols))
            want[:, 0::2], want[:, 1::2] = spectra[b].real, spectra[b].imag
            bound = np.broadcast_to(d, want.shape)
        elif mode == AMPLITUDE:
            want, bound = a, d + fr.RELATIVE * a
        else:
            want, bound = a * a, 2 * a * d + d * d + fr.RELATIVE * a * a
        err = np.abs(got - want)
        err = np.where(np.isnan(err), np.inf, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)  # (bound = 0: digital silence, where any error is infinite)
        w = float(ratio.max())
        worst = max(worst, w)
        if w > 1:
            t, k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            say("frame {} column {}: {} for {} (error {:.3g}, bound {:.3g}): {:.3g} x the bound".format(
                t, k, got[t, k], want[t, k], err[t, k], bound[t, k], w))
    return worst, problems


def _brev(half):
    log2h = int(np.log2(half))
    return np.array([int(format(n, "0{}b".format(log2h))[::-1], 2) for n in range(half)])


def _twiddles(n_fft):
    ang = -2.0 * np.arange(n_fft // 2) / n_fft
    return np.cos(np.pi * ang).astype(np.float32), np.sin(np.pi * ang).astype(np.float32)


def _fft_half_f32(zr, zi, n_fft, skip_lone_last_stage=False):
    """wave_fft_half: the radix-2 decimation-in-time stages over (frames, n_fft / 2) fp32 input in bit-reversed order."""
    half = n_fft // 2
    log2h = int(np.log2(half))
    twr, twi = _twiddles(n_fft)
    n_frames = zr.shape[0]
    for s in range(1, log2h + 1):
        if skip_lone_last_stage and s == log2h and log2h % 2 == 1:
            continue
        mh = 1 << (s - 1)
        k = np.arange(mh) * (n_fft >> s)
        wr, wi = twr[k], twi[k]
        zr4, zi4 = zr.reshape(n_frames, -1, 2, mh), zi.reshape(n_frames, -1, 2, mh)
        ur, ui, vr, vi = zr4[:, :, 0], zi4[:, :, 0], zr4[:, :, 1], zi4[:, :, 1]
        pr, pi = wr * vr - wi * vi, wr * vi + wi * vr
        zr = np.stack([ur + pr, ur - pr], axis=2).reshape(n_frames, half)
        zi = np.stack([ui + pi, ui - pi], axis=2).reshape(n_frames, half)
    assert zr.dtype == zi.dtype == np.float32
    return zr, zi


FORWARD_MUTANTS = tuple(m for m in fr.MUTANTS if m != "no_floor")  # (the floor belongs to the level mode alone)


def stft_f32_modes(case, mode, mutant=None, sentinel=SENTINEL):
    """stft_kernel<mode> in numpy float32 (front_end_ref.stft_f32_restatement with the kernel's other epilogues; POWER_LEVEL
    gives that function's buffer bit for bit).  Returns the whole output buffer over a sentinel fill."""
    assert mutant is None or mutant in fr.MUTANTS
    f32 = np.float32
    n_fft, hop, half = case.n_fft, case.hop, case.n_fft // 2
    bins = half + 1
    row_stride, batch_stride = forward_layout(case, mode)
    win = fr.window_f32(n_fft, symmetric=mutant == "symmetric_window", cosine=mutant == "cosine_window")
    twr, twi = _twiddles(n_fft)
    brev = _brev(half)
    out = np.full(len(case.utterances) * batch_stride, sentinel, dtype=f32)
    for b, y in enumerate(case.utterances):
        n_frames = 1 + len(y) // hop
        rows = out[b * batch_stride:b * batch_stride + case.max_frames * row_stride].reshape(case.max_frames, row_stride)
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
        idx = np.clip(idx, 0, len(y) - 1)
        x = win[None, :] * y[idx]
        zr, zi = np.empty((n_frames, half), f32), np.empty((n_frames, half), f32)
        zr[:, brev], zi[:, brev] = x[:, 0::2], x[:, 1::2]
        zr, zi = _fft_half_f32(zr, zi, n_fft, skip_lone_last_stage=mutant == "last_stage_skipped")
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
        if mode == COMPLEX:
            rows[:n_frames, 0:2 * bins:2], rows[:n_frames, 1:2 * bins:2] = xr, xi
        elif mode == POWER:
            rows[:n_frames, :bins] = pw
        elif mode == AMPLITUDE:
            rows[:n_frames, :bins] = np.sqrt(pw)
        else:
            with np.errstate(divide="ignore"):
                level = f32(3.0102999566398120) * np.log2(pw)
            if mutant != "no_floor":
                level = np.where(pw == 0, f32(case.min_db), np.maximum(level, f32(case.min_db)))
            rows[:n_frames, :bins] = level
    return out


# ------------------------------------------------------------------------------------------------ the inverse in float64
def window_sumsquare(n_fft, hop, frames, window=None):
    """S[p] = sum_t w[p - t hop]^2 over the n_fft + hop (frames - 1) samples of the untrimmed buffer."""
    w = so.hann_periodic(n_fft) if window is None else window
    s = np.zeros(n_fft + hop * (frames - 1))
    for t in range(frames):
        s[t * hop:t * hop + n_fft] += w * w
    return s


def istft_f64(spec, n_fft, hop):
    """spec complex (frames, n_fft / 2 + 1) -> float64 audio of hop (frames - 1) samples (module docstring)."""
    spec = np.asarray(spec, dtype=np.complex128)
    frames, half = spec.shape[0], n_fft // 2
    assert spec.shape[1] == half + 1 and frames >= 1
    w = so.hann_periodic(n_fft)
    y = np.zeros(n_fft + hop * (frames - 1))
    x = np.fft.irfft(spec, n=n_fft, axis=1)
    for t in range(frames):
        y[t * hop:t * hop + n_fft] += w * x[t]
    s = window_sumsquare(n_fft, hop, frames)
    y = np.where(s > TINY, y / np.where(s > TINY, s, 1.0), y)
    return y[half:len(y) - half]


InverseCase = namedtuple("InverseCase", "name n_fft hop spectra out_offsets out_total max_frames row_stride batch_stride source")


def resident_frames(n_fft):
    """Frames of n_fft floats a work-group of istft_kernel holds in 64 KiB of LDS beside the twiddles and the window (n_fft
    floats each), 16 at most."""
    return min(16384 // n_fft - 2, 16)


def tile_frames(n_fft, hop):
    """sl_istft_tile_frames: the frames of output a work-group owns.  A tile of T frames of output is covered by
    T + 2 ((n_fft / 2 - 1) // hop) + 1 frames."""
    return resident_frames(n_fft) - (2 * ((n_fft // 2 - 1) // hop) + 1)


def _inverse_case(name, n_fft, hop, spectra, gaps=None, extra_frames=0, row_slack=0, slack=0, source=None):
    """spectra: complex (frames, bins) per utterance, rounded to complex64 here (what the kernel is given)."""
    bins = n_fft // 2 + 1
    spectra = [np.ascontiguousarray(np.asarray(s).astype(np.complex64)) for s in spectra]
    assert all(s.shape[1] == bins and 1 <= s.shape[0] <= 41 for s in spectra) and len(spectra) <= 8
    assert all(np.isfinite(s.view(np.float32)).all() for s in spectra)
    lengths = [hop * (s.shape[0] - 1) for s in spectra]
    gaps = [0] * len(spectra) if gaps is None else gaps
    offsets, at = [], gaps[0]
    for n, gap in zip(lengths, list(gaps[1:]) + [0]):
        offsets.append(at)
        at += n + gap
    max_frames = max(s.shape[0] for s in spectra) + extra_frames
    row_stride = 2 * bins + row_slack
    for s in spectra:
        s.setflags(write=False)
    return InverseCase(name, n_fft, hop, spectra, np.asarray(offsets, dtype=np.int64), at + 64, max_frames, row_stride,
                       max_frames * row_stride + slack, source)


def random_spectra(frames, bins, seed):
    """Complex spectra that are the STFT of nothing, with imaginary parts in the DC and Nyquist bins as large as the rest."""
    rng = np.random.RandomState(seed)
    return (rng.randn(frames, bins) + 1j * rng.randn(frames, bins)) * rng.uniform(0.1, 4.0, size=(frames, 1))


_INVERSE_CASES = None


def inverse_cases():
    """Every case of front_end_ref.stft_cases() through the float64 oracle (its layout carried over: tight and padded
    rows, rows behind the longest utterance, slack; the ragged case with odd output offsets and gaps), and for the inverse
    alone: hop = n_fft / 8, frame counts one either side of one and of two tiles at 512 / 128 and at 1024 / 128 (the
    smallest tile), and random spectra.  Built once; the arrays are shared and must not be written."""
    global _INVERSE_CASES
    if _INVERSE_CASES is not None:
        return _INVERSE_CASES
    cases = []
    for c in fr.stft_cases():
        bins = c.n_fft // 2 + 1
        frames = max(1 + len(u) // c.hop for u in c.utterances)
        ragged = c.name == "n512_ragged"
        cases.append(_inverse_case("inv_" + c.name, c.n_fft, c.hop, complex_expected(c),
                                   gaps=(3, 1, 300, 7, 2, 129) if ragged else None, extra_frames=c.max_frames - frames,
                                   row_slack=2 * (c.row_stride - bins), slack=2 * (c.batch_stride - c.max_frames * c.row_stride),
                                   source=c.name))
    lengths = [257, 9 * 64 - 1, 9 * 64, 9 * 64 + 1, 40 * 64]
    hop64 = fr.StftCase("n512_hop64", 512, 64, -150.0, [fr.chirps(n, 600 + i) for i, n in enumerate(lengths)], None, 0, 0, 0)
    cases.append(_inverse_case("inv_n512_hop64", 512, 64, complex_expected(hop64), row_slack=1))
    for n_fft, hop in ((512, 128), (1024, 128)):
        tf = tile_frames(n_fft, hop)
        counts = [tf, tf + 1, tf + 2, 2 * tf, 2 * tf + 1, 2 * tf + 2]  # (frames - 1 = the frames of output: tf - 1 .. 2 tf + 1)
        src = fr.StftCase("tiles", n_fft, hop, -150.0, [fr.chirps((n - 1) * hop + 5 + i, 700 + n_fft + i)
                                                        for i, n in enumerate(counts)], None, 0, 0, 0)
        cases.append(_inverse_case("inv_n{}_hop{}_tile_edges".format(n_fft, hop), n_fft, hop, complex_expected(src)))
        cases.append(_inverse_case("inv_n{}_hop{}_random".format(n_fft, hop), n_fft, hop,
                                   [random_spectra(n, n_fft // 2 + 1, 800 + n_fft + i) for i, n in enumerate([1, 2] + counts)],
                                   gaps=(1, 0, 5, 0, 2, 77, 0, 3), extra_frames=3, row_slack=3, slack=11))
    tf = tile_frames(64, 8)
    cases.append(_inverse_case("inv_n64_hop8_random", 64, 8,
                               [random_spectra(n, 33, 900 + i) for i, n in enumerate([tf, tf + 1, tf + 2, 2 * tf + 1, 41])]))
    _INVERSE_CASES = cases
    return cases


def inverse_case(name):
    return {c.name: c for c in inverse_cases()}[name]


def spectrum_buffer(case, fill=np.nan):
    """The fp32 buffer sl_istft reads: `fill` in the padding columns, in the rows behind every utterance and in the slack."""
    buf = np.full((len(case.spectra), case.batch_stride), fill, dtype=np.float32)
    bins = case.n_fft // 2 + 1
    for b, s in enumerate(case.spectra):
        rows = buf[b, :case.max_frames * case.row_stride].reshape(case.max_frames, case.row_stride)
        rows[:s.shape[0], 0:2 * bins:2], rows[:s.shape[0], 1:2 * bins:2] = s.real, s.imag
    return buf.reshape(-1)


def inverse_expected(case):
    """[(want, bound)] per utterance: float64 (hop (frames - 1),) each (module docstring)."""
    out = []
    n_fft, hop, half = case.n_fft, case.hop, case.n_fft // 2
    w = so.hann_periodic(n_fft)
    c = np.full(half + 1, 2.0)
    c[0] = c[half] = 1.0
    for s in case.spectra:
        d = s.astype(np.complex128)
        frames = d.shape[0]
        want = istft_f64(d, n_fft, hop)
        x = np.fft.irfft(d, n=n_fft, axis=1)
        eps = 16 * np.log2(n_fft) * U / n_fft * (np.abs(d) * c[None, :]).sum(axis=1)
        num = np.zeros(n_fft + hop * (frames - 1))
        for t in range(frames):
            num[t * hop:t * hop + n_fft] += w * eps[t] + 8 * U * np.abs(w * x[t])
        ss = window_sumsquare(n_fft, hop, frames)
        bound = np.where(ss > TINY, num / np.where(ss > TINY, ss, 1.0), num)
        out.append((want, bound[half:len(bound) - half]))
        assert want.shape == out[-1][1].shape == (hop * (frames - 1),)
    return out


def inverse_report(case, audio_flat, expected=None, sentinel=SENTINEL):
    """(worst error / bound, [problems]) of the whole audio buffer (case.out_total floats) sl_istft wrote over `sentinel`."""
    expected = inverse_expected(case) if expected is None else expected
    audio_flat = np.asarray(audio_flat).reshape(-1)
    worst, problems = 0.0, []
    if audio_flat.shape[0] != case.out_total:
        return np.inf, ["buffer of {} floats, not {}".format(audio_flat.shape[0], case.out_total)]
    untouched = np.ones(case.out_total, dtype=bool)
    for b, (want, bound) in enumerate(expected):
        o = int(case.out_offsets[b])
        untouched[o:o + len(want)] = False
        if not len(want):
            continue
        got = audio_flat[o:o + len(want)].astype(np.float64)
        err = np.abs(got - want)
        err = np.where(np.isnan(err), np.inf, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        w = float(ratio.max())
        worst = max(worst, w)
        if w > 1:
            j = int(np.argmax(ratio))
            problems.append("utterance {} sample {}: {} for {} (error {:.3g}, bound {:.3g}): {:.3g} x the bound".format(
                b, j, got[j], want[j], err[j], bound[j], w))
    rest = audio_flat[untouched]
    if not np.array_equal(rest.view(np.uint32), np.full(rest.shape, sentinel, np.float32).view(np.uint32)):
        problems.append("{} floats written outside the utterances' samples".format(
            int((rest.view(np.uint32) != np.float32(sentinel).view(np.uint32)).sum())))
    return worst, problems


def compare_inverse(case, audio_flat, expected=None, sentinel=SENTINEL):
    worst, problems = inverse_report(case, audio_flat, expected, sentinel)
    assert not problems, "{}: {}".format(case.name, "; ".join(problems))
    return worst


# ------------------------------------------------------------------------------------------------ the inverse kernel, in numpy
INVERSE_MUTANTS = ("no_normalisation", "window_sum_not_squared", "trim_off_by_one", "halo_frame_dropped", "dc_nyquist_imag_used",
                   "conjugated", "symmetric_window")


def istft_f32_restatement(case, mutant=None, sentinel=SENTINEL, tile=None):
    """istft_kernel in numpy float32: X -> Z = E + i O of the half-length transform (the DC and Nyquist imaginary parts taken as
    zero), conj Z through the forward butterflies in bit-reversed order, x[2n] = Re / (N/2), x[2n+1] = -Im / (N/2), times the
    fp32 sin^2 window; per sample the covering frames added in ascending order, the squared windows likewise, one division.
    Returns the audio buffer (case.out_total floats) over a sentinel fill.  tile: frames of output per work-group, which only
    the halo mutant can see (it loses the first halo frame of every tile but the first, from both sums)."""
    assert mutant is None or mutant in INVERSE_MUTANTS
    f32 = np.float32
    n_fft, hop, half = case.n_fft, case.hop, case.n_fft // 2
    tile = tile_frames(n_fft, hop) if tile is None else tile
    reach = (half - 1) // hop
    win = fr.window_f32(n_fft, symmetric=mutant == "symmetric_window")
    twr, twi = _twiddles(n_fft)
    brev = _brev(half)
    inv = f32(1.0 / half)
    out = np.full(case.out_total, sentinel, dtype=f32)
    k = np.arange(half)
    kb = half - k
    for b, s in enumerate(case.spectra):
        frames = s.shape[0]
        re, im = s.real.astype(f32), s.imag.astype(f32)
        if mutant == "conjugated":
            im = -im
        ar, ai, br, bi = re[:, k], im[:, k].copy(), re[:, kb], im[:, kb].copy()
        if mutant != "dc_nyquist_imag_used":
            ai[:, 0] = 0
            bi[:, 0] = 0
        er, ei = f32(0.5) * (ar + br), f32(0.5) * (ai - bi)
        dr, di = f32(0.5) * (ar - br), f32(0.5) * (ai + bi)
        orr, oi = dr * twr + di * twi, di * twr - dr * twi
        zr, zi = np.empty((frames, half), f32), np.empty((frames, half), f32)
        zr[:, brev], zi[:, brev] = er - oi, -(ei + orr)
        zr, zi = _fft_half_f32(zr, zi, n_fft)
        x = np.empty((frames, n_fft), f32)
        x[:, 0::2], x[:, 1::2] = win[0::2] * (zr * inv), win[1::2] * (-zi * inv)
        acc = np.zeros(n_fft + hop * (frames - 1), f32)
        wsum = np.zeros_like(acc)
        p = np.arange(n_fft)
        for t in range(frames):
            keep = np.ones(n_fft, dtype=bool)
            if mutant == "halo_frame_dropped":
                owner = (t * hop + p - half) // (tile * hop)  # the tile of each sample this frame reaches
                keep = ~((owner >= 1) & (t == owner * tile - reach))
            acc[t * hop:t * hop + n_fft] += np.where(keep, x[t], f32(0))
            wsum[t * hop:t * hop + n_fft] += np.where(keep, win if mutant == "window_sum_not_squared" else win * win, f32(0))
        if mutant != "no_normalisation":
            acc = np.where(wsum > f32(TINY), acc / np.where(wsum > f32(TINY), wsum, f32(1)), acc)
        assert acc.dtype == f32
        n_out = hop * (frames - 1)
        start = half + (1 if mutant == "trim_off_by_one" else 0)
        o = int(case.out_offsets[b])
        out[o:o + n_out] = np.concatenate([acc, np.zeros(1, f32)])[start:start + n_out]
    return out
