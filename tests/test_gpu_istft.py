"""sl_stft (power, amplitude, complex, power level), sl_istft and the members of SpectrogramExtractor / LabeledExample built
on them, against float64 through tests/istft_ref.py: every value within the derived bounds, nothing
read outside an utterance's samples or rows (NaN everywhere else), nothing written outside the output (a sentinel around
it, bit for bit), and an utterance's result independent of the batch it sits in."""
import numpy as np
import pytest

import front_end_ref as fr
import istft_ref as ir
from oracle import spectrogram_oracle as so

pytestmark = pytest.mark.gpu

_EXPECTED, _SPECTRA, _INVERSE = {}, {}, {}
FORWARD_NAMES = [c.name for c in fr.stft_cases()]
SL_ERR_INVALID_ARGUMENT, SL_ERR_UNSUPPORTED = -1, -2


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run_forward(case, hip_lib, mode, entry="sl_stft"):
    """The bare launch: NaN before, between and behind the utterances, the sentinel all over the output."""
    import torch
    dev = torch.device("cuda:0")
    audio = torch.from_numpy(fr.audio_buffer(case)).to(dev)
    off = torch.from_numpy(case.offsets).to(dev)
    lengths = torch.tensor([len(u) for u in case.utterances], dtype=torch.int32, device=dev)
    batch = len(case.utterances)
    row_stride, batch_stride = ir.forward_layout(case, mode)
    out = torch.full((batch * batch_stride,), float(fr.SENTINEL), dtype=torch.float32, device=dev)
    head = (audio.data_ptr(), off.data_ptr(), lengths.data_ptr(), out.data_ptr(), batch, case.max_frames, case.n_fft, case.hop,
            row_stride, batch_stride)
    stream = torch.cuda.current_stream().cuda_stream
    if entry == "sl_stft":
        hip_lib.call("sl_stft", *head, mode, case.min_db, stream)
    else:
        hip_lib.call("sl_stft_power_db", *head, case.min_db, stream)
    return out.cpu().numpy()


def run_inverse(case, hip_lib, buffer=None):
    """The bare launch: NaN in the padding columns, behind every utterance's rows and in the slack; the sentinel all over
    the audio buffer."""
    import torch
    dev = torch.device("cuda:0")
    spec = torch.from_numpy(ir.spectrum_buffer(case) if buffer is None else buffer).to(dev)
    frames = torch.tensor([s.shape[0] for s in case.spectra], dtype=torch.int32, device=dev)
    off = torch.from_numpy(case.out_offsets).to(dev)
    audio = torch.full((case.out_total,), float(ir.SENTINEL), dtype=torch.float32, device=dev)
    hip_lib.call("sl_istft", spec.data_ptr(), frames.data_ptr(), audio.data_ptr(), off.data_ptr(), len(case.spectra),
                 case.max_frames, case.n_fft, case.hop, case.row_stride, case.batch_stride,
                 torch.cuda.current_stream().cuda_stream)
    return audio.cpu().numpy()


# ------------------------------------------------------------------------------------------------ sl_stft
@pytest.mark.parametrize("name", FORWARD_NAMES)
def test_forward_modes_within_the_bounds_at_every_value(name, hip_lib):
    """Worst error / bound measured on the MI355X: DESIGN.md section 3.9."""
    case = fr.stft_case(name)
    for mode in sorted(ir.MODE_NAMES):
        got = run_forward(case, hip_lib, mode)
        worst, problems = ir.forward_report(case, got, mode, expected(case), spectra(case))
        print("sl_stft", ir.MODE_NAMES[mode], name, "worst error / bound", worst)
        assert not problems, "{} {}: worst error / bound {}: {}".format(name, ir.MODE_NAMES[mode], worst, "; ".join(problems))
        assert worst <= 1


def test_forward_modes_give_exact_zeros_on_digital_silence(hip_lib):
    case = fr.stft_case("n512_signals")
    silent = np.nonzero(expected(case)[7][1] == 0)[0]
    assert len(silent) >= 2
    for mode in sorted(ir.MODE_NAMES):
        row_stride, batch_stride = ir.forward_layout(case, mode)
        rows = run_forward(case, hip_lib, mode)[7 * batch_stride:][:case.max_frames * row_stride].reshape(-1, row_stride)
        assert not rows[silent].any() and rows[:33].any()


def test_power_level_mode_is_sl_stft_power_db_bit_for_bit(hip_lib):
    for case in fr.stft_cases():
        new = run_forward(case, hip_lib, ir.POWER_LEVEL)
        old = run_forward(case, hip_lib, ir.POWER_LEVEL, entry="sl_stft_power_db")
        assert np.array_equal(bits(new), bits(old)), case.name
        fr.compare_case(case, new, expected(case))


def test_forward_rows_do_not_depend_on_the_batch(hip_lib):
    """Alone, inside the ragged batch, and at another position of it (the batch in reverse)."""
    case = fr.stft_case("n512_ragged")
    flipped = case._replace(name="flipped", utterances=case.utterances[::-1], offsets=case.offsets[::-1].copy())
    for mode in (ir.POWER, ir.AMPLITUDE, ir.COMPLEX, ir.POWER_LEVEL):
        _, batch_stride = ir.forward_layout(case, mode)
        together = run_forward(case, hip_lib, mode).reshape(-1, batch_stride)
        back = run_forward(flipped, hip_lib, mode).reshape(-1, batch_stride)
        assert np.array_equal(bits(back[::-1]), bits(together)), mode
        for b, u in enumerate(case.utterances):
            alone = case._replace(name="alone", utterances=[u], offsets=np.zeros(1, dtype=np.int64))
            assert np.array_equal(bits(run_forward(alone, hip_lib, mode)), bits(together[b])), (mode, b)
        assert np.count_nonzero(together[0]) >= 11 * 257


# ------------------------------------------------------------------------------------------------ sl_istft
def test_tile_frames_are_what_the_case_list_was_built_around(hip_lib):
    tile = hip_lib.raw("sl_istft_tile_frames")
    for n_fft in (64, 128, 256, 512, 1024):
        for hop in (n_fft // 8, n_fft // 4, n_fft // 2, n_fft, 5 * n_fft // 16):
            assert tile(n_fft, hop) == ir.tile_frames(n_fft, hop) >= 7, (n_fft, hop)
        assert tile(n_fft, n_fft // 8 - 1) == tile(n_fft, n_fft + 1) == tile(n_fft, 0) == 0
    assert tile(2048, 512) == tile(32, 8) == tile(384, 96) == 0


@pytest.mark.parametrize("name", [c.name for c in ir.inverse_cases()])
def test_inverse_within_the_bound_at_every_sample(name, hip_lib):
    """Worst error / bound measured on the MI355X: DESIGN.md section 3.9."""
    case = ir.inverse_case(name)
    got = run_inverse(case, hip_lib)
    worst, problems = ir.inverse_report(case, got, inverse_expected(case))
    print("sl_istft", name, "worst error / bound", worst)
    assert not problems, "{}: worst error / bound {}: {}".format(name, worst, "; ".join(problems))
    assert worst <= 1


def test_inverse_ignores_the_dc_and_nyquist_imaginary_parts(hip_lib):
    case = ir.inverse_case("inv_n512_hop128_random")
    buffer = ir.spectrum_buffer(case).reshape(len(case.spectra), -1)
    for b, s in enumerate(case.spectra):
        rows = buffer[b, :case.max_frames * case.row_stride].reshape(case.max_frames, case.row_stride)
        rows[:s.shape[0], [1, 513]] = np.nan
    assert np.array_equal(bits(run_inverse(case, hip_lib, buffer.reshape(-1))), bits(run_inverse(case, hip_lib)))


def test_inverse_does_not_depend_on_the_batch(hip_lib):
    """Alone (at offset 0, tight rows), inside the ragged batch, and at another position of it (the batch in reverse)."""
    for name in ("inv_n512_hop128_random", "inv_n1024_hop128_tile_edges", "inv_n512_ragged"):
        case = ir.inverse_case(name)
        together = run_inverse(case, hip_lib)
        ir.compare_inverse(case, together, inverse_expected(case))
        flipped = ir._inverse_case("flipped", case.n_fft, case.hop, case.spectra[::-1], extra_frames=2)
        back = run_inverse(flipped, hip_lib)
        for b, s in enumerate(case.spectra):
            n, o = case.hop * (s.shape[0] - 1), int(case.out_offsets[b])
            alone = ir._inverse_case("alone", case.n_fft, case.hop, [s])
            assert np.array_equal(bits(run_inverse(alone, hip_lib)[:n]), bits(together[o:o + n])), (name, b)
            fo = int(flipped.out_offsets[len(case.spectra) - 1 - b])
            assert np.array_equal(bits(back[fo:fo + n]), bits(together[o:o + n])), (name, b)


def test_unsupported_hops_and_bad_arguments_launch_nothing(hip_lib):
    import torch
    dev = torch.device("cuda:0")
    istft, stft = hip_lib.raw("sl_istft"), hip_lib.raw("sl_stft")
    spec = torch.zeros((4 * 514,), dtype=torch.float32, device=dev)
    frames = torch.tensor([4], dtype=torch.int32, device=dev)
    off = torch.zeros((1,), dtype=torch.int64, device=dev)
    audio = torch.full((4096,), float(ir.SENTINEL), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def inverse(n_fft=512, hop=128, spec_ptr=spec.data_ptr(), max_frames=4, row_stride=514, batch=1):
        return istft(spec_ptr, frames.data_ptr(), audio.data_ptr(), off.data_ptr(), batch, max_frames, n_fft, hop, row_stride,
                     max_frames * row_stride, stream)

    for hop in (63, 1, 513, 1024):
        assert inverse(hop=hop) == SL_ERR_UNSUPPORTED, hop
        assert "hop" in hip_lib.last_error()
    assert inverse(n_fft=64, hop=7) == SL_ERR_UNSUPPORTED and inverse(n_fft=256, hop=31) == SL_ERR_UNSUPPORTED
    for kwargs in ({"spec_ptr": None}, {"n_fft": 500}, {"n_fft": 2048, "hop": 512}, {"n_fft": 32, "hop": 8}, {"hop": 0}, {"hop": -128},
                   {"max_frames": 0}, {"row_stride": 513}, {"batch": 0}, {"batch": 65536}):
        assert inverse(**kwargs) == SL_ERR_INVALID_ARGUMENT, kwargs
    out = torch.full((8 * 514,), float(fr.SENTINEL), dtype=torch.float32, device=dev)
    wave = torch.zeros((1024,), dtype=torch.float32, device=dev)
    length = torch.tensor([1024], dtype=torch.int32, device=dev)
    for mode, row_stride in ((4, 514), (-1, 514), (ir.COMPLEX, 513), (ir.POWER, 256)):
        assert stft(wave.data_ptr(), off.data_ptr(), length.data_ptr(), out.data_ptr(), 1, 8, 512, 128, row_stride,
                    8 * row_stride, mode, -150.0, stream) == SL_ERR_INVALID_ARGUMENT, (mode, row_stride)
    torch.cuda.synchronize()
    sentinel = bits(np.float32(ir.SENTINEL).reshape(1))[0]
    assert (bits(audio.cpu().numpy()) == sentinel).all() and (bits(out.cpu().numpy()) == sentinel).all()
    assert inverse() == 0  # (and the arguments the refusals were variations of are accepted)
    assert not np.isnan(audio.cpu().numpy()[:384]).any() and not audio.cpu().numpy()[:384].any()


@pytest.mark.parametrize("name", [c.name for c in fr.stft_cases() if c.hop < c.n_fft])
def test_round_trip_returns_the_audio(name, hip_lib):
    """sl_istft(sl_stft(COMPLEX)) against the first hop (frames - 1) samples of every utterance.  The bound is the forward
    budget pushed through the inverse plus the inverse's own: re and im of a bin are each within delta_t, so the bin is
    within sqrt 2 delta_t, a sample of the frame's inverse transform within (1 / n_fft) sum_k c_k sqrt 2 delta_t =
    sqrt 2 delta_t, and sample j within sum_t w[p - t hop] sqrt 2 delta_t / S[p]; the inverse bound is taken over the
    spectrum the forward launch really wrote."""
    case = fr.stft_case(name)
    n_fft, hop, half, bins = case.n_fft, case.hop, case.n_fft // 2, case.n_fft // 2 + 1
    row_stride, batch_stride = ir.forward_layout(case, ir.COMPLEX)
    forward = run_forward(case, hip_lib, ir.COMPLEX).reshape(len(case.utterances), batch_stride)
    written = []
    for b, u in enumerate(case.utterances):
        rows = forward[b, :case.max_frames * row_stride].reshape(case.max_frames, row_stride)[:1 + len(u) // hop]
        written.append(rows[:, 0:2 * bins:2] + 1j * rows[:, 1:2 * bins:2])
    inverse = ir._inverse_case("rt_" + name, n_fft, hop, written, gaps=[1] * len(written), extra_frames=1, row_slack=1)
    got = run_inverse(inverse, hip_lib)
    own = ir.inverse_expected(inverse)
    ir.compare_inverse(inverse, got, own)
    w = so.hann_periodic(n_fft)
    worst = 0.0
    for b, (u, (_, delta)) in enumerate(zip(case.utterances, expected(case))):
        frames = len(delta)
        n, o = hop * (frames - 1), int(inverse.out_offsets[b])
        pushed = np.zeros(n_fft + hop * (frames - 1))
        for t in range(frames):
            pushed[t * hop:t * hop + n_fft] += w * np.sqrt(2.0) * delta[t]
        pushed = pushed[half:half + n] / ir.window_sumsquare(n_fft, hop, frames)[half:half + n]
        bound = pushed + own[b][1]
        err = np.abs(got[o:o + n].astype(np.float64) - u[:n].astype(np.float64))
        assert n == hop * (len(u) // hop) and not np.isnan(err).any()
        if n:
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(err > 0, err / bound, 0.0)
            worst = max(worst, float(ratio.max()))
    print("round trip", name, "worst error / bound", worst)
    assert worst <= 1


# ------------------------------------------------------------------------------------------------ the extractor
AUDIOS = [fr.chirps(n, 70 + i) for i, n in enumerate((1500, 257, 4099, 128 * 15, 903))]
PAIRS = [(t, s) for t in ("power", "amplitude", "power level") for s in ("linear", "mel")]


def direct(ext, hip_lib, mode, max_frames, row_stride):
    """One launch over AUDIOS into a sentinel-filled (5, max_frames, row_stride)."""
    flat, offsets, _ = ext.flatten(AUDIOS)
    case = fr.StftCase("direct", 512, 128, -150.0, AUDIOS, offsets, max_frames, row_stride, max_frames * row_stride)
    if mode == ir.COMPLEX:
        case = case._replace(row_stride=row_stride // 2, batch_stride=max_frames * row_stride // 2)
    entry = "sl_stft_power_db" if mode == ir.POWER_LEVEL else "sl_stft"
    return run_forward(case, hip_lib, mode, entry=entry).reshape(5, max_frames, row_stride)


@pytest.mark.parametrize("type,scale", PAIRS)
def test_spectrogram_batch_is_the_direct_launches_chained(type, scale, hip_lib):
    import torch
    from test_gpu_front_end import project
    from speechless_amd.spectrogram import SpectrogramExtractor, SpectrogramFrequencyScale, SpectrogramType, TIME_TILE
    ext = SpectrogramExtractor()
    mode = {"power": ir.POWER, "amplitude": ir.AMPLITUDE, "power level": ir.POWER_LEVEL}[type]
    x, frames = ext.spectrogram_batch(AUDIOS, SpectrogramType(type), SpectrogramFrequencyScale(scale))
    assert frames == [12, 3, 33, 16, 8] and x.dtype == torch.float32 and x.is_contiguous()
    got = x.cpu().numpy()
    if scale == "linear":
        want = direct(ext, hip_lib, mode, 33, 257)
    else:
        rows = direct(ext, hip_lib, mode, TIME_TILE, ext.bins_pad)
        mel = project(ext, torch.from_numpy(rows).to(ext.device), 33).cpu().numpy()
        bank = ext.mel_w[:128, 0, :].cpu().numpy()
        worst = fr.compare_mel(mel[:, :33, :128], rows[:, :33], bank)
        print("mel projection of", type, "worst error / bound", worst)
        assert worst <= 1
        want = mel[:, :33, :128]
    assert got.shape == want.shape == (5, 33, 257 if scale == "linear" else 128)
    assert np.array_equal(bits(got), bits(want))
    for b, n in enumerate(frames):
        assert not got[b, n:].any() and got[b, :n].any()


def test_stft_batch_and_istft_batch_are_the_direct_launches_chained(hip_lib):
    import torch
    from speechless_amd.spectrogram import SpectrogramExtractor
    ext = SpectrogramExtractor()
    spec, frames = ext.stft_batch(AUDIOS)
    assert spec.dtype == torch.complex64 and tuple(spec.shape) == (5, 33, 257) and frames == [12, 3, 33, 16, 8]
    rows = direct(ext, hip_lib, ir.COMPLEX, 33, 514)
    got = torch.view_as_real(spec).cpu().numpy().reshape(5, 33, 514)
    assert np.array_equal(bits(got), bits(rows))
    written = [rows[b, :n, 0::2] + 1j * rows[b, :n, 1::2] for b, n in enumerate(frames)]
    case = ir._inverse_case("chained", 512, 128, written, extra_frames=33 - max(frames))
    want = run_inverse(case, hip_lib, rows.reshape(-1).copy())
    pieces = ext.istft_batch(spec, frames)
    flat, offsets, lengths = ext.istft_batch(spec, frames, flat=True)
    assert list(lengths) == [128 * (n - 1) for n in frames] and list(offsets) == [int(o) for o in case.out_offsets]
    assert flat.dtype == torch.float32 and flat.shape[0] == int(lengths.sum()) and offsets.dtype == np.int64 and lengths.dtype == np.int32
    assert np.array_equal(bits(flat.cpu().numpy()), bits(want[:flat.shape[0]]))
    for piece, o, n in zip(pieces, offsets, lengths):
        assert piece.shape == (n,) and np.array_equal(bits(piece.cpu().numpy()), bits(want[o:o + n]))
    with pytest.raises(ValueError):
        ext.istft_batch(spec, [12, 3, 34, 16, 8])
    with pytest.raises(ValueError):
        ext.istft_batch(spec.real, frames)


# ------------------------------------------------------------------------------------------------ LabeledExample
def test_labeled_example_spectrograms_are_rows_of_the_batch(hip_lib):
    from speechless_amd.spectrogram import (LabeledExample, SpectrogramExtractor, SpectrogramFrequencyScale as Scale,
                                            SpectrogramType as Type)
    ext = SpectrogramExtractor()
    audio = AUDIOS[2]
    example = LabeledExample(lambda: audio)
    default = example.spectrogram()
    for type, scale in PAIRS:
        got = example.spectrogram(Type(type), Scale(scale))
        x, frames = ext.spectrogram_batch(AUDIOS, Type(type), Scale(scale))
        assert got.dtype == np.float32 and got.shape == (257 if scale == "linear" else 128, 33)
        assert np.array_equal(bits(got), bits(x[2].cpu().numpy().T)), (type, scale)
        assert example.frequency_count_from_spectrogram(got) == got.shape[0]
        if (type, scale) == ("power level", "linear"):
            assert np.array_equal(bits(got), bits(default))
    assert example.time_step_count() == default.shape[1] == 33
    assert example.time_step_rate() == 33 / (4099 / 16000)


def test_level_mel_spectrogram_z_normalised_is_the_nets_input(hip_lib):
    from test_gpu_front_end import run_znorm
    from speechless_amd.spectrogram import LabeledExample, SpectrogramFrequencyScale as Scale, SpectrogramType as Type
    for audio in AUDIOS:
        example = LabeledExample(lambda a=audio: a)
        mel = np.ascontiguousarray(example.spectrogram(Type.power_level, Scale.mel).T)
        frames = mel.shape[0]
        chained = run_znorm(hip_lib, mel[None], [frames], 128, frames, slack=0)[0]
        got = example.z_normalized_transposed_spectrogram()
        assert got.shape == (frames, 128) and np.array_equal(bits(got), bits(chained))


def test_power_mel_spectrogram_agrees_with_float64(hip_lib):
    """The reference's own test of this class (test/test_labeled_example.py:13-21: spectrogram(power, mel) against
    librosa.feature.melspectrogram), restated in float64: mel_filter_bank @ |stft|^2.  The bound is the projection's
    accumulation bound over the kernel's own fp32 power rows and fp32 bank, plus what the rows and the bank themselves may be
    off by, pushed through the bank: sum_j w_ij (power bound_j + 2^-24 a_j^2)."""
    from speechless_amd.spectrogram import (LabeledExample, SpectrogramExtractor, SpectrogramFrequencyScale as Scale,
                                            SpectrogramType as Type)
    ext = SpectrogramExtractor()
    bank32 = ext.mel_w[:128, 0, :].cpu().numpy()
    bank64 = so.mel_filter_bank(16000, 512, 128)
    worst = 0.0
    for i, audio in enumerate(AUDIOS):
        example = LabeledExample(lambda a=audio: a)
        got = example.spectrogram(Type.power, Scale.mel).T.astype(np.float64)
        rows = np.zeros((got.shape[0], ext.bins_pad), dtype=np.float32)
        rows[:, :257] = example.spectrogram(Type.power, Scale.linear).T
        _, accumulation = fr.mel_expected(rows, bank32)
        case = fr.StftCase("one", 512, 128, -150.0, [audio], np.zeros(1, np.int64), got.shape[0], 257, got.shape[0] * 257)
        a, delta = fr.stft_expected(case)[0]
        d = delta[:, None]
        rows_bound = 2 * a * d + d * d + fr.RELATIVE * a * a
        want = (a * a) @ bank64.T
        bound = accumulation + (rows_bound + fr.U * a * a) @ bank64.T
        err = np.abs(got - want)
        assert got.shape == want.shape == (1 + len(audio) // 128, 128) and (err <= bound).all(), (i, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print("spectrogram(power, mel) against float64, worst error / bound", worst)
    assert 0 < worst <= 1


def test_reconstructed_audio_matches_the_audio(hip_lib):
    from speechless_amd.spectrogram import LabeledExample
    w = so.hann_periodic(512)
    worst = 0.0
    for audio in AUDIOS:
        got = LabeledExample(lambda a=audio: a).reconstructed_audio_from_spectrogram()
        n = 128 * (len(audio) // 128)
        assert got.dtype == np.float32 and got.shape == (n,)
        if not n:
            continue
        case = fr.StftCase("one", 512, 128, -150.0, [audio], np.zeros(1, np.int64), 1 + n // 128, 257, (1 + n // 128) * 257)
        _, delta = fr.stft_expected(case)[0]
        inverse = ir._inverse_case("one", 512, 128, ir.complex_expected(case))
        frames = len(delta)
        pushed = np.zeros(512 + 128 * (frames - 1))
        for t in range(frames):
            pushed[t * 128:t * 128 + 512] += w * np.sqrt(2.0) * delta[t]
        pushed = pushed[256:256 + n] / ir.window_sumsquare(512, 128, frames)[256:256 + n]
        # The inverse bound is taken over the float64 spectrum here, and the inverse ran on the forward launch's: its
        # sum_k c_k |D[k]| may be larger by n_fft sqrt 2 delta_t = 6.2e-3 sum_n |x w|, and sum_k c_k |D[k]| >= sum_n |x w|
        # (Parseval and the two norm inequalities): 1.01 covers it.
        bound = pushed + 1.01 * ir.inverse_expected(inverse)[0][1]
        err = np.abs(got.astype(np.float64) - audio[:n].astype(np.float64))
        worst = max(worst, float((err / bound).max()))
    print("reconstructed audio, worst error / bound", worst)
    assert 0 < worst <= 1
