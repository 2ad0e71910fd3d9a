"""tests/istft_ref.py on the CPU: the float64 inverse against the forward oracle, the bound against a float32 restatement
of the inverse kernel, the inverse case list against the mistakes it must catch, the comparators of the three new forward
modes against the float32 restatement of the forward kernel and its mutants, and the host-only members of LabeledExample.
tests/test_gpu_istft.py runs the HIP kernels through the same lists and comparators."""
import numpy as np
import pytest

import front_end_ref as fr
import istft_ref as ir
from oracle import spectrogram_oracle as so

_EXPECTED, _SPECTRA, _INVERSE = {}, {}, {}


def expected(case):
    if case.name not in _EXPECTED:
        _EXPECTED[case.name] = fr.stft_expected(case)
    return _EXPECTED[case.name]


def spectra(case):
    if case.name not in _SPECTRA:
        _SPECTRA[case.name] = ir.complex_expected(case)
    return _SPECTRA[case.name]


def inverse_expected(case):
    if case.name not in _INVERSE:
        _INVERSE[case.name] = ir.inverse_expected(case)
    return _INVERSE[case.name]


# ------------------------------------------------------------------------------------------------ the float64 inverse
def test_float64_inverse_round_trips_the_forward_oracle():
    """Every case with hop < n_fft: the first hop (frames - 1) samples come back to 4.5e-16 (of full scale, or of the
    utterance's peak where that is larger)."""
    worst, seen = 0.0, 0
    for case in fr.stft_cases():
        if case.hop >= case.n_fft:
            continue
        for u, d in zip(case.utterances, spectra(case)):
            y = ir.istft_f64(d, case.n_fft, case.hop)
            assert y.shape == (case.hop * (len(u) // case.hop),)
            if len(y):
                worst = max(worst, np.abs(y - u[:len(y)].astype(np.float64)).max() / max(1.0, np.abs(u).max()))
                seen += 1
    print("float64 round trip, worst error:", worst)
    assert seen > 80 and worst <= 4.5e-16


def test_float64_inverse_against_direct_sums():
    """One frame count, written out sample by sample from the definition: irfft by a direct cosine sum, the overlap-add and
    the squared-window sum as plain loops.  Also: the DC and Nyquist imaginary parts do not matter, and S under four full
    overlaps is 4 * 3/8 (the mean of the squared Hann window)."""
    n_fft, hop, frames = 64, 16, 5
    d = ir.random_spectra(frames, 33, 1)
    n = np.arange(n_fft)
    w = so.hann_periodic(n_fft)
    c = np.full(33, 2.0)
    c[0] = c[32] = 1.0
    buf, s = np.zeros(n_fft + hop * (frames - 1)), np.zeros(n_fft + hop * (frames - 1))
    for t in range(frames):
        x = np.zeros(n_fft)
        for k in range(33):
            z = d[t, k].real if k in (0, 32) else d[t, k]
            x += c[k] * (z * np.exp(2j * np.pi * k * n / n_fft)).real / n_fft
        buf[t * hop:t * hop + n_fft] += w * x
        s[t * hop:t * hop + n_fft] += w ** 2
    assert (s[32:-32] > 1).all()
    want = buf[32:-32] / s[32:-32]
    got = ir.istft_f64(d, n_fft, hop)
    assert got.shape == (hop * (frames - 1),) and np.abs(got - want).max() < 1e-13
    real_edges = d.copy()
    real_edges[:, [0, 32]] = real_edges[:, [0, 32]].real
    assert np.array_equal(ir.istft_f64(real_edges, n_fft, hop), got)
    assert np.allclose(ir.window_sumsquare(n_fft, hop, 9)[n_fft:-n_fft], 1.5)
    # hop = n_fft: S touches 0 at every frame's first sample, where the sample is left as it is (0 times the window)
    s = ir.window_sumsquare(512, 512, 3)
    assert s[0] == s[512] == 0 and s[256] == 1
    lone = ir.istft_f64(ir.random_spectra(3, 257, 2), 512, 512)
    assert lone[256] == 0 and np.isfinite(lone).all()
    assert ir.istft_f64(ir.random_spectra(1, 257, 3), 512, 128).shape == (0,)


def test_window_sums_the_issue_quotes():
    def smallest(n_fft, hop):
        return ir.window_sumsquare(n_fft, hop, 12)[n_fft // 2:-(n_fft // 2)].min()
    assert abs(smallest(512, 128) - 1.25) < 1e-12 and abs(smallest(64, 16) - 1.25) < 1e-12
    assert smallest(512, 160) >= 1.095 and smallest(512, 256) >= 0.5 and smallest(512, 512) == 0


# ------------------------------------------------------------------------------------------------ the inverse case list
def test_inverse_case_list_covers_what_it_claims():
    cases = ir.inverse_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.source for c in cases if c.source} == {c.name for c in fr.stft_cases()}
    for c in cases:
        bins = c.n_fft // 2 + 1
        assert len(c.spectra) <= 8 and all(1 <= s.shape[0] <= 41 and s.shape[1] == bins for s in c.spectra), c.name
        assert all(s.dtype == np.complex64 and not s.flags.writeable for s in c.spectra)
        assert c.n_fft // 8 <= c.hop <= c.n_fft
        assert c.row_stride >= 2 * bins and c.batch_stride >= c.max_frames * c.row_stride
        assert c.max_frames >= max(s.shape[0] for s in c.spectra)
        ends = [int(o) + c.hop * (s.shape[0] - 1) for o, s in zip(c.out_offsets, c.spectra)]
        assert all(int(o) >= e for o, e in zip(c.out_offsets[1:], ends[:-1])) and c.out_total > ends[-1], c.name
        buf = ir.spectrum_buffer(c).reshape(len(c.spectra), -1)
        assert int(np.isnan(buf).sum()) == buf.size - sum(2 * s.size for s in c.spectra)
    assert {(c.n_fft, c.hop) for c in cases} >= {(512, 64), (64, 8), (1024, 128), (512, 160), (512, 256), (512, 512), (128, 64)}
    assert any(s.shape[0] == 1 for s in ir.inverse_case("inv_n512_hop512").spectra)  # no output samples
    for n_fft, hop in ((512, 128), (1024, 128)):
        tf = ir.tile_frames(n_fft, hop)
        for kind in ("tile_edges", "random"):
            c = ir.inverse_case("inv_n{}_hop{}_{}".format(n_fft, hop, kind))
            assert {tf - 1, tf, tf + 1, 2 * tf - 1, 2 * tf, 2 * tf + 1} <= {s.shape[0] - 1 for s in c.spectra}
    assert (ir.tile_frames(512, 128), ir.tile_frames(1024, 128), ir.tile_frames(1024, 1024), ir.tile_frames(64, 8)) == (13, 7, 13, 9)
    ragged = ir.inverse_case("inv_n512_ragged")
    gaps = [int(o) - (int(p) + 128 * (s.shape[0] - 1))
            for o, p, s in zip(ragged.out_offsets[1:], ragged.out_offsets[:-1], ragged.spectra[:-1])]
    assert ragged.out_offsets[0] % 2 == 1 and sum(g > 0 for g in gaps) >= 4 and any(int(o) % 2 for o in ragged.out_offsets[1:])
    rnd = ir.inverse_case("inv_n512_hop128_random")
    assert all(np.abs(s[:, [0, 256]].imag).min() > 0 for s in rnd.spectra) and rnd.row_stride % 2 == 1
    assert any(c.row_stride == 2 * (c.n_fft // 2 + 1) for c in cases) and any(c.batch_stride > c.max_frames * c.row_stride for c in cases)


def test_float32_restatement_of_the_inverse_stays_inside_a_twentieth_of_the_bound():
    """Worst error / bound of the restatement: DESIGN.md section 3.9 quotes it beside the GPU's."""
    worst = {}
    for case in ir.inverse_cases():
        worst[case.name] = ir.compare_inverse(case, ir.istft_f32_restatement(case), inverse_expected(case))
    print("float32 restatement of the inverse, worst error / bound:", worst)
    assert 1e-4 < max(worst.values()) <= 0.05, worst


def test_restatement_does_not_depend_on_the_tile():
    case = ir.inverse_case("inv_n512_hop128_random")
    assert np.array_equal(ir.istft_f32_restatement(case, tile=5).view(np.uint32), ir.istft_f32_restatement(case).view(np.uint32))


# mutant -> (a case that catches it, a case that cannot see it or None)
INVERSE_CAUGHT_BY = {
    "no_normalisation": ("inv_n512_lengths", None),
    "window_sum_not_squared": ("inv_n512_hop160", None),
    "trim_off_by_one": ("inv_n512_lengths", None),
    # a frame missing from BOTH sums still reconstructs a spectrum that is the STFT of something: x w^2 / w^2
    "halo_frame_dropped": ("inv_n512_hop128_random", "inv_n512_hop128_tile_edges"),
    "dc_nyquist_imag_used": ("inv_n512_hop128_random", "inv_n512_lengths"),  # an STFT's DC and Nyquist bins are real
    "conjugated": ("inv_n512_lengths", None),
    "symmetric_window": ("inv_n1024_lengths", None),
}


@pytest.mark.parametrize("mutant", ir.INVERSE_MUTANTS)
def test_every_inverse_mutant_is_caught(mutant):
    catcher, blind = INVERSE_CAUGHT_BY[mutant]
    case = ir.inverse_case(catcher)
    worst, problems = ir.inverse_report(case, ir.istft_f32_restatement(case, mutant), inverse_expected(case))
    print(mutant, catcher, "error / bound", worst)
    assert problems and worst >= 10, (mutant, catcher, worst)
    with pytest.raises(AssertionError):
        ir.compare_inverse(case, ir.istft_f32_restatement(case, mutant), inverse_expected(case))
    if blind is not None:
        case = ir.inverse_case(blind)
        assert ir.compare_inverse(case, ir.istft_f32_restatement(case, mutant), inverse_expected(case)) <= 0.05
    if mutant == "halo_frame_dropped":  # ... and a single tile has no halo to lose
        case = ir.inverse_case(catcher)
        one_tile = ir.istft_f32_restatement(case, mutant, tile=64)
        assert np.array_equal(one_tile.view(np.uint32), ir.istft_f32_restatement(case).view(np.uint32))


def test_inverse_comparator_rejects_single_samples_and_stray_writes():
    case = ir.inverse_case("inv_n512_ragged")
    exp = inverse_expected(case)
    good = ir.istft_f32_restatement(case)
    assert ir.compare_inverse(case, good, exp) <= 0.05
    o = int(case.out_offsets[2])
    n = 128 * (case.spectra[2].shape[0] - 1)
    loud = o + int(np.argmax(np.abs(exp[2][0])))
    for index, value in ((loud, good[loud] * np.float32(1.0001)), (o + 5, np.float32(np.nan)), (o - 1, np.float32(0)),
                         (o + n, good[o + n - 1]), (0, np.float32(0)), (case.out_total - 1, -ir.SENTINEL)):
        bad = good.copy()
        bad[index] = value
        assert ir.inverse_report(case, bad, exp)[1], index
    assert ir.inverse_report(case, good[:-1], exp)[1]


# ------------------------------------------------------------------------------------------------ forward modes
def test_power_level_mode_of_the_restatement_is_front_end_refs_restatement():
    for name in ("n64_lengths", "n512_signals", "n512_quiet_floor80"):
        case = fr.stft_case(name)
        assert np.array_equal(ir.stft_f32_modes(case, ir.POWER_LEVEL).view(np.uint32), fr.stft_f32_restatement(case).view(np.uint32))


@pytest.mark.parametrize("mode", sorted(ir.MODE_NAMES), ids=lambda m: ir.MODE_NAMES[m])
def test_forward_comparators_accept_the_float32_restatement(mode):
    worst = {}
    for case in fr.stft_cases():
        w, problems = ir.forward_report(case, ir.stft_f32_modes(case, mode), mode, expected(case), spectra(case))
        assert not problems, (case.name, problems)
        worst[case.name] = w
    print(ir.MODE_NAMES[mode], "float32 restatement, worst error / bound:", worst)
    assert 1e-4 < max(worst.values()) <= 0.05, worst
    # digital silence: exact zeros
    case = fr.stft_case("n512_signals")
    silent = np.nonzero(expected(case)[7][1] == 0)[0]
    row_stride, batch_stride = ir.forward_layout(case, mode)
    rows = ir.stft_f32_modes(case, mode)[7 * batch_stride:][:case.max_frames * row_stride].reshape(case.max_frames, row_stride)
    assert len(silent) >= 2 and not rows[silent].any()


FORWARD_CAUGHT_BY = {"symmetric_window": "n1024_lengths", "edge_repeating_reflect": "n512_lengths", "centre_shifted": "n512_lengths",
                     "nyquist_twiddle": "n512_signals", "last_stage_skipped": "n256_lengths", "cosine_window": "n512_signals"}


@pytest.mark.parametrize("mutant", ir.FORWARD_MUTANTS)
@pytest.mark.parametrize("mode", sorted(ir.MODE_NAMES), ids=lambda m: ir.MODE_NAMES[m])
def test_forward_comparators_reject_the_mutants(mode, mutant):
    case = fr.stft_case(FORWARD_CAUGHT_BY[mutant])
    worst, problems = ir.forward_report(case, ir.stft_f32_modes(case, mode, mutant), mode, expected(case), spectra(case))
    assert problems and worst >= 10, (mutant, worst)


@pytest.mark.parametrize("mode", sorted(ir.MODE_NAMES), ids=lambda m: ir.MODE_NAMES[m])
def test_forward_comparators_reject_layout_damage(mode):
    case = fr.stft_case("n512_signals")
    good = ir.stft_f32_modes(case, mode)
    row_stride, batch_stride = ir.forward_layout(case, mode)
    cols = (2 if mode == ir.COMPLEX else 1) * 257
    base = 7 * batch_stride
    assert row_stride > cols and batch_stride > case.max_frames * row_stride
    loud = 3 * row_stride + int(np.argmax(np.abs(good[base + 3 * row_stride:base + 3 * row_stride + cols])))
    for index, value in ((loud, good[base + loud] * np.float32(1.001)), (5 * row_stride + cols, np.float32(1e-30)),
                         (33 * row_stride + 7, np.float32(1e-30)), (case.max_frames * row_stride, np.float32(0)),
                         (batch_stride - 1, -ir.SENTINEL), (40 * row_stride + 3, np.float32(np.nan))):
        bad = good.copy()
        bad[base + index] = value
        problems = ir.forward_report(case, bad, mode, expected(case), spectra(case))[1]
        assert problems and all(p.startswith("utterance 7:") for p in problems), (index, problems)
    assert ir.forward_report(case, good[:-1], mode, expected(case), spectra(case))[1]


# ------------------------------------------------------------------------------------------------ the class, host side
def test_enums_carry_the_references_values():
    from speechless_amd.spectrogram import SpectrogramFrequencyScale, SpectrogramType
    assert {m.name: m.value for m in SpectrogramType} == {"power": "power", "amplitude": "amplitude", "power_level": "power level"}
    assert {m.name: m.value for m in SpectrogramFrequencyScale} == {"linear": "linear", "mel": "mel"}
    assert SpectrogramType("power level") is SpectrogramType.power_level


@pytest.mark.parametrize("rate,n_mels", [(16000, 128), (16000, 40), (8000, 64)])
def test_host_side_members_of_labeled_example(rate, n_mels):
    from speechless_amd.spectrogram import LabeledExample
    audio = fr.chirps(1000, 5)
    example = LabeledExample(lambda: audio, sample_rate=rate, mel_frequency_count=n_mels, label_with_tags="a <t> b <t>")
    assert np.array_equal(example.mel_frequencies(), so.mel_frequencies(n_mels + 2, fmax=rate / 2))
    assert example.highest_detectable_frequency() == rate / 2
    assert example.tag_count("<t>") == 2 and example.tag_count("<u>") == 0
    assert example.frequency_count_from_spectrogram(np.zeros((257, 8))) == 257
    assert example.time_step_count() == 1 + 1000 // 128 == 8
    assert example.time_step_rate() == 8 / (1000 / rate)
