"""tests/front_end_ref.py on the CPU: the float64 expectation against independent answers, the comparators against damage
they must reject, and the case list against the mistakes it must catch (a float32 restatement of the kernel with one switch
per mistake).  tests/test_gpu_front_end.py runs the HIP kernels through the same list and comparators."""
import numpy as np
import pytest

import front_end_ref as fr
from oracle import spectrogram_oracle as so

_EXPECTED = {}


def expected(case):
    if case.name not in _EXPECTED:
        _EXPECTED[case.name] = fr.stft_expected(case)
    return _EXPECTED[case.name]


def frame_counts(case):
    return [1 + len(u) // case.hop for u in case.utterances]


# ------------------------------------------------------------------------------------------------ the case list
def test_chirps_restate_the_synthetic_audio_of_test_spectrogram():
    from test_spectrogram import synthetic_audio
    assert np.array_equal(fr.chirps(800, 7), synthetic_audio(0.05, 7))
    assert np.array_equal(fr.chirps(4000, 9, silence=(100, 900)), synthetic_audio(0.25, 9, silence=(100, 900)))
    assert np.array_equal(fr.chirps(800, 7, gain=2.0 ** -10), synthetic_audio(0.05, 7) * np.float32(2.0 ** -10))


def test_case_list_covers_what_it_claims():
    cases = fr.stft_cases()
    assert len({c.name for c in cases}) == len(cases)
    for c in cases:
        bins = c.n_fft // 2 + 1
        assert len(c.utterances) <= 8 and all(c.n_fft // 2 < len(u) <= 40 * c.hop for u in c.utterances), c.name
        assert all(u.dtype == np.float32 and not u.flags.writeable for u in c.utterances)
        assert c.max_frames >= max(frame_counts(c)) and c.row_stride > bins - 1
        assert c.batch_stride >= c.max_frames * c.row_stride
        ends = [int(o) + len(u) for o, u in zip(c.offsets, c.utterances)]
        assert all(int(o) >= e for o, e in zip(c.offsets[1:], ends[:-1])), c.name  # no two utterances overlap
    quarter = {c.n_fft for c in cases if c.hop * 4 == c.n_fft}
    assert quarter == {64, 128, 256, 512, 1024}
    assert {(c.n_fft, c.hop) for c in cases} >= {(512, 160), (512, 256), (512, 512), (128, 64)}
    assert {c.min_db for c in cases} == {-150.0, -80.0}
    for n_fft in quarter:  # every edge length and frame count at every window length
        mine = [c for c in cases if c.n_fft == n_fft and c.hop * 4 == n_fft]
        hop, lengths = n_fft // 4, {len(u) for c in mine for u in c.utterances}
        assert {n_fft // 2 + 1, n_fft // 2 + 2} <= lengths
        assert any({m * hop - 1, m * hop, m * hop + 1} <= lengths for m in range(2, 40))
        assert {15, 16, 17, 33} <= {f for c in mine for f in frame_counts(c)}
    for c in cases:
        if c.hop * 4 != c.n_fft:
            lengths = {len(u) for u in c.utterances}
            assert c.n_fft // 2 + 1 in lengths and any({m * c.hop - 1, m * c.hop, m * c.hop + 1} <= lengths for m in range(2, 40))
    # layouts
    assert any(c.max_frames == max(frame_counts(c)) and c.max_frames % 16 for c in cases)
    assert any(c.max_frames >= max(frame_counts(c)) + 20 for c in cases)
    assert any(c.row_stride == fr.round_up(c.n_fft // 2 + 1, 64) for c in cases)
    assert any(c.row_stride == c.n_fft // 2 + 2 for c in cases)
    assert any(c.batch_stride > c.max_frames * c.row_stride for c in cases)
    ragged = fr.stft_case("n512_ragged")
    assert len(ragged.utterances) >= 5 and ragged.offsets[0] > 0 and any(int(o) % 2 for o in ragged.offsets)
    gaps = [int(o) - (int(p) + len(u)) for o, p, u in zip(ragged.offsets[1:], ragged.offsets[:-1], ragged.utterances[:-1])]
    assert min(gaps) >= 0 and sum(g > 0 for g in gaps) >= 4 and len(set(gaps)) > 3
    flat = fr.audio_buffer(ragged)
    assert np.isnan(flat[:ragged.offsets[0]]).all() and np.isnan(flat[-64:]).all()
    assert int(np.isnan(flat).sum()) == len(flat) - sum(len(u) for u in ragged.utterances)
    # gains: 2^-10 and 2^15 of the same signal; the -80 dB floor cuts the quiet one in two
    quiet, loud = fr.stft_case("n512_quiet"), fr.stft_case("n512_int16")
    assert np.array_equal(quiet.utterances[1] * np.float32(2.0 ** 25), loud.utterances[1])
    assert 1e-4 < np.abs(quiet.utterances[1]).max() < 1e-3 and 8192 < np.abs(loud.utterances[1]).max() < 65536
    for a, delta in expected(fr.stft_case("n512_quiet_floor80")):
        floored = (a + delta[:, None] < 1e-4).mean()
        assert 0.1 < floored < 0.9 and (a > 1e-4).mean() > 0.1
    # digital silence inside an utterance: whole frames of exact zeros
    for name in ("n512_signals", "n512_quiet", "n64_signals"):
        assert any((delta == 0).sum() >= 2 and (delta > 0).sum() >= 2 for _, delta in expected(fr.stft_case(name))), name


# ------------------------------------------------------------------------------------------------ stft_expected
@pytest.mark.parametrize("name", ["n64_lengths", "n512_hop160", "n1024_signals", "n512_ragged"])
def test_stft_expected_against_torch(name):
    import torch
    case = fr.stft_case(name)
    for u, (a, delta) in zip(case.utterances, expected(case)):
        ref = torch.stft(torch.from_numpy(u.astype(np.float64)), n_fft=case.n_fft, hop_length=case.hop,
                         window=torch.hann_window(case.n_fft, periodic=True, dtype=torch.float64), center=True,
                         pad_mode="reflect", return_complex=True).abs().numpy().T
        assert a.shape == ref.shape == (1 + len(u) // case.hop, case.n_fft // 2 + 1)
        assert np.abs(a - ref).max() <= 1e-12 * max(1.0, ref.max())
        assert delta.shape == (a.shape[0],) and (delta >= 0).all()


@pytest.mark.parametrize("n_fft", [64, 512, 1024])
def test_stft_expected_against_closed_forms(n_fft):
    """An impulse at window position p gives |X_k| = w[p] for every k; DC (which reflect padding leaves DC) gives sum w
    at k = 0, half of it at k = 1 and nothing beyond; the alternating sequence (which reflect padding leaves alternating)
    is its mirror image.  The budget of a DC frame is 16 log2 n u level (n / 2 + n 2^-23)."""
    case = fr.stft_case("n{}_signals".format(n_fft))
    hop, half = case.hop, n_fft // 2
    w = so.hann_periodic(n_fft)
    exp = expected(case)
    n = len(case.utterances[2])
    for b, at in ((2, 0), (3, n - 1), (4, 13 * hop + 1)):
        assert case.utterances[b][at] == 1 and np.count_nonzero(case.utterances[b]) == 1
        a, delta = exp[b]
        hit = 0
        for t in range(a.shape[0]):
            p = at + half - t * hop
            want = w[p] if 0 <= p < n_fft else 0.0
            hit += want > 0
            assert np.abs(a[t] - want).max() < 1e-13, (b, t)
            assert abs(delta[t] - 16 * np.log2(n_fft) * 2.0 ** -24 * (want + 2.0 ** -23) * (0 <= p < n_fft)) < 1e-20
        assert hit >= 2
    assert min(w[13 * hop + 1 + half - t * hop] for t in range(13, 16)) < 5e-3  # the mid impulse meets the window's edge
    for b, peak, side in ((5, 0, 1), (6, half, half - 1)):
        a, delta = exp[b]
        rest = np.ones(half + 1, dtype=bool)
        rest[[peak, side]] = False
        assert np.abs(a[:, peak] - 0.75 * n_fft / 2).max() < 1e-10 and np.abs(a[:, side] - 0.75 * n_fft / 4).max() < 1e-10
        assert a[:, rest].max() < 1e-11
        assert np.allclose(delta, 16 * np.log2(n_fft) * 2.0 ** -24 * 0.75 * (n_fft / 2 + n_fft * 2.0 ** -23), rtol=1e-12)
        # the nulls are what the bound must reach: 84 dB and more under the peak
        assert (0.75 * n_fft / 2) / delta.max() > 1.6e4


# ------------------------------------------------------------------------------------------------ restatement, mutants
def test_float32_restatement_stays_inside_a_twentieth_of_the_bound():
    """If the reference side alone came near the bound on some case, the bound would be too tight for that case."""
    worst = {}
    for case in fr.stft_cases():
        worst[case.name] = fr.compare_case(case, fr.stft_f32_restatement(case), expected(case))
    print("float32 restatement, worst error / bound:", worst)
    assert max(worst.values()) <= 0.05, worst
    assert max(worst.values()) > 1e-4  # (the restatement is float32, not the expectation again)


# mutant -> (a case that catches it, a case that cannot see it or None)
CAUGHT_BY = {
    "symmetric_window": ("n1024_lengths", None),
    "edge_repeating_reflect": ("n512_lengths", None),
    "centre_shifted": ("n512_lengths", None),
    "nyquist_twiddle": ("n512_signals", None),
    "last_stage_skipped": ("n256_lengths", "n512_lengths"),  # 512: an even number of stages, no lone last one
    "no_floor": ("n512_signals", "n512_lengths"),            # nothing reaches -150 dB without digital silence
    "cosine_window": ("n512_signals", "n512_lengths"),       # needs a frame that is all window edge
}


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_every_mutant_is_caught(mutant):
    catcher, blind = CAUGHT_BY[mutant]
    case = fr.stft_case(catcher)
    worst, problems = fr.case_report(case, fr.stft_f32_restatement(case, mutant), expected(case))
    assert problems and worst >= 10, (mutant, catcher, worst)
    with pytest.raises(AssertionError):
        fr.compare_case(case, fr.stft_f32_restatement(case, mutant), expected(case))
    if blind is not None:
        case = fr.stft_case(blind)
        assert fr.compare_case(case, fr.stft_f32_restatement(case, mutant), expected(case)) <= 0.05
    caught = [c.name for c in fr.stft_cases()
              if fr.case_report(c, fr.stft_f32_restatement(c, mutant), expected(c))[0] >= 10]
    print(mutant, "caught by", caught)
    assert catcher in caught
    if mutant in ("symmetric_window", "edge_repeating_reflect", "centre_shifted", "nyquist_twiddle"):
        assert len(caught) == len(fr.stft_cases())
    if mutant == "last_stage_skipped":
        assert {c.n_fft for c in fr.stft_cases() if c.name in caught} == {64, 256, 1024}
    if mutant == "cosine_window":
        assert "n1024_signals" in caught


def test_stationary_signals_alone_cannot_see_a_shifted_centre():
    """A tone on a bin centre and DC have the same amplitudes one sample later: away from the reflected edges the shifted
    mutant passes on them, and fails on the chirps of the same batch.  The case SET is what catches every mutant."""
    case = fr.stft_case("n512_signals")
    out = fr.stft_f32_restatement(case, "centre_shifted")
    exp = expected(case)
    inner = slice(2, 31)  # frames whose window does not reach the reflected samples
    for b, blind in ((0, True), (5, True), (7, False)):
        a, delta = exp[b]
        rows = out[b * case.batch_stride:][:case.max_frames * case.row_stride].reshape(case.max_frames, case.row_stride)
        got = rows[inner, :257]
        slab = np.concatenate([got, np.zeros((got.shape[0], 1), np.float32)], axis=1).reshape(-1)
        worst, problems = fr.level_report(slab, a[inner], delta[inner], case.min_db, got.shape[0], 258)
        assert (worst <= 0.05 and not problems) if blind else worst >= 10, (b, worst)


# ------------------------------------------------------------------------------------------------ comparator
def test_comparator_rejects_layout_damage_and_single_bins():
    case = fr.stft_case("n512_signals")
    exp = expected(case)
    good = fr.stft_f32_restatement(case)
    assert fr.compare_case(case, good, exp) <= 0.05
    b = 7
    a, delta = exp[b]
    frames, bins, rs = a.shape[0], a.shape[1], case.row_stride
    assert frames == 33 and case.max_frames == 56 and rs == bins + 1 and case.batch_stride == 56 * rs + 37
    base = b * case.batch_stride

    def rejected(index, value, word):
        bad = good.copy()
        bad[base + index] = value
        worst, problems = fr.case_report(case, bad, exp)
        assert problems and all(p.startswith("utterance {}:".format(b)) for p in problems), (index, value, problems)
        assert any(word in p for p in problems), (word, problems)
        with pytest.raises(AssertionError):
            fr.compare_levels(bad[base:base + case.batch_stride], a, delta, case.min_db, case.max_frames, rs)

    loud = int(np.argmax(a[3]))
    level = good[base + 3 * rs + loud]
    rejected(3 * rs + loud, level + np.float32(0.01), "x the bound")           # one bin, a hundredth of a decibel
    rejected(3 * rs + loud, level - np.float32(0.01), "x the bound")
    silent = int(np.nonzero(delta == 0)[0][0])
    assert good[base + silent * rs + 5] == -150.0
    rejected(silent * rs + 5, np.nextafter(np.float32(-150), np.float32(0)), "not exactly")  # one ulp above the floor
    rejected(silent * rs + 5, np.float32(-150.5), "not exactly")
    rejected(5 * rs + bins, np.float32(1e-30), "columns >= bins")              # the padding column
    rejected(frames * rs + 7, np.float32(-150), "rows 33 .. 56")                # a frame too many: the first zero row
    rejected((case.max_frames - 1) * rs, np.float32(1e-30), "rows 33 .. 56")
    rejected(case.max_frames * rs, np.float32(0), "behind row max_frames")     # sentinel overwritten, first and last
    rejected(case.batch_stride - 1, -fr.SENTINEL, "behind row max_frames")
    for index in (0, 5 * rs + bins, 40 * rs + 3, case.batch_stride - 2):        # a NaN anywhere
        rejected(index, np.float32(np.nan), "NaN")
    # a frame count off by one, either way: the last row missing, a row too many
    bad = good.copy()
    bad[base + (frames - 1) * rs:base + frames * rs] = 0
    assert fr.case_report(case, bad, exp)[1]
    bad = good.copy()
    bad[base + frames * rs:base + frames * rs + bins] = good[base + (frames - 1) * rs:base + (frames - 1) * rs + bins]
    assert fr.case_report(case, bad, exp)[1]
    # ... and the expectation of an utterance one hop longer does not fit this output
    longer = fr.StftCase("x", 512, 128, -150.0, [fr.chirps(len(case.utterances[7]) + 128, 712)], np.zeros(1, np.int64),
                         case.max_frames, rs, case.batch_stride)
    assert fr.case_report(longer, good[base:base + case.batch_stride])[1]
    # a slab that is too short is refused, not indexed
    assert fr.level_report(good[base:base + 100], a, delta, -150.0, case.max_frames, rs)[1]


def test_comparator_is_continuous_across_the_floor():
    """Floored on both sides: a bin whose true amplitude sits just under the floor may be reported just above it, and the
    other way round; only where a + delta is under the floor must the level be the floor exactly."""
    a = np.array([[0.9999e-4, 1.0001e-4, 0.5e-4, 1e-4]])
    delta = np.array([1e-7])
    row = lambda *levels: np.array(levels, dtype=np.float32)
    at = lambda amp: np.float32(20 * np.log10(amp))
    assert fr.compare_levels(row(-80, -80, -80, -80), a, delta, -80.0, 1, 4) <= 1
    assert fr.compare_levels(row(at(1.00005e-4), at(1.00005e-4), -80, at(1.00005e-4)), a, delta, -80.0, 1, 4) <= 1
    assert fr.level_report(row(-80, -80, at(0.5e-4), -80), a, delta, -80.0, 1, 4)[1]   # under the floor
    assert fr.level_report(row(-80, -80, at(1.002e-4), -80), a, delta, -80.0, 1, 4)[1]  # must floor, did not
    assert fr.level_report(row(at(1.003e-4), -80, -80, -80), a, delta, -80.0, 1, 4)[1]  # 2e-7 over: past delta + 1e-9


# ------------------------------------------------------------------------------------------------ z-normalisation
def test_znorm_comparator():
    frames, f = [0, 1, 2, 31, 64], 40
    for values in fr.ZNORM_VALUES:
        src = fr.znorm_source(frames, f, f + 7, 70, values, seed=3)
        assert np.isnan(src[:, :, f:]).all() and np.isnan(src[0]).all() and np.isnan(src[3, 31:]).all()
        got = np.zeros((5, 66, f), dtype=np.float32)
        for b, (want, mean, std) in enumerate(fr.znorm_expected(src, frames, f)):
            assert want.shape == (frames[b], f)
            if frames[b]:
                assert abs(want.mean()) < 1e-9 and abs(want.std() - 1) < 1e-9
                assert np.array_equal(want, so.z_normalize(src[b, :frames[b], :f].astype(np.float64)))
            got[b, :frames[b]] = want.astype(np.float32)
        assert fr.compare_znorm(got, src, frames, f) <= 0.5 + 1e-6  # half an ulp of 2^-23 |want|
        bad = got.copy()
        bad[3, 31, 0] = 1e-30
        assert fr.znorm_report(bad, src, frames, f)[1]
        bad = got.copy()
        bad[0, 0, 0] = np.nan
        assert fr.znorm_report(bad, src, frames, f)[1]
        bad = got.copy()
        t, c = np.unravel_index(int(np.argmax(np.abs(got[4]))), got[4].shape)
        bad[4, t, c] *= np.float32(1.00001)  # (near-constant: |mean| / std = 14000 allows 1.4e-6 absolute)
        assert fr.znorm_report(bad, src, frames, f)[1]


def test_znorm_comparator_rejects_a_one_pass_float32_variance():
    frames, f = [64, 257], 128
    src = fr.znorm_source(frames, f, f, 257, "near_constant", seed=4)
    got = np.zeros((2, 257, f), dtype=np.float32)
    for b, n in enumerate(frames):
        x = src[b, :n]
        mean = x.mean(dtype=np.float32)
        var = (x * x).mean(dtype=np.float32) - mean * mean  # 19600 +- 2e-3 for a variance of 1e-4
        with np.errstate(invalid="ignore", divide="ignore"):
            got[b, :n] = (x - mean) / np.sqrt(var)
    worst, problems = fr.znorm_report(got, src, frames, f)
    assert problems and worst > 100
    # the same one-pass formula passes in float64 on level-like values: the comparator is not simply strict
    src = fr.znorm_source(frames, f, f, 257, "level", seed=4)
    for b, n in enumerate(frames):
        x = src[b, :n].astype(np.float64)
        got[b, :n] = (x - x.mean()) / np.sqrt((x * x).mean() - x.mean() ** 2)
    assert fr.compare_znorm(got, src, frames, f) <= 1


@pytest.mark.parametrize("frames,f", [(1, 40), (2, 1), (64, 1), (2, 32), (1, 64)])
def test_znorm_comparator_rejects_the_sample_standard_deviation(frames, f):
    assert 1 < frames * f <= 64
    src = fr.znorm_source([frames], f, f, frames, "level", seed=5)
    x = src[0].astype(np.float64)
    got = ((x - x.mean()) / x.std(ddof=1)).astype(np.float32)[None]
    worst, problems = fr.znorm_report(got, src, [frames], f)
    assert problems and worst > 1000
    assert fr.compare_znorm(((x - x.mean()) / x.std()).astype(np.float32)[None], src, [frames], f) <= 0.5 + 1e-6


# ------------------------------------------------------------------------------------------------ mel projection
@pytest.mark.parametrize("n_fft,rate,mel", [(512, 16000, 128), (512, 16000, 40), (256, 8000, 40)])
def test_mel_bound_holds_for_numpy_float32_and_not_for_a_shifted_bank(n_fft, rate, mel):
    bins = n_fft // 2 + 1
    cin_pad = fr.round_up(bins, 64)
    case = fr.stft_case("n{}_lengths".format(n_fft))
    rows = fr.stft_f32_restatement(case)[:case.max_frames * case.row_stride].reshape(case.max_frames, case.row_stride)
    assert case.row_stride == cin_pad
    level = np.concatenate([rows[:3], np.full((1, cin_pad), -150, np.float32), np.full((1, cin_pad), 90, np.float32),
                            (90 - 240 * (np.arange(cin_pad) % 2)).astype(np.float32)[None]])
    level[:, bins:] = 0
    bank = np.zeros((mel, cin_pad), dtype=np.float32)
    bank[:, :bins] = so.mel_filter_bank(rate, n_fft, mel)
    want, bound = fr.mel_expected(level, bank)
    assert want.shape == bound.shape == (6, mel) and (bound > 0).all()
    assert np.abs(want[:3] - level[:3, :bins].astype(np.float64) @ so.mel_filter_bank(rate, n_fft, mel).T).max() \
        < 1e-6 * np.abs(want[:3]).max()  # (the fp32 rounding of the bank is all that separates the two)
    worst = fr.compare_mel(level @ bank.T, level, bank)
    assert 0 < worst <= 1
    shifted = np.roll(bank, 1, axis=1)
    with pytest.raises(AssertionError):
        fr.compare_mel(level[:3] @ shifted.T, level[:3], bank)
    with pytest.raises(AssertionError):  # ... and one value one part in 1e4 off
        bad = level @ bank.T
        bad[4, 7] *= np.float32(1.0001)
        fr.compare_mel(bad, level, bank)
