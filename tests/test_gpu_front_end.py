"""The three launches of the audio front end (sl_stft_power_db, the 1 x 1 fp32 mel projection on sl_conv1d_nt,
sl_z_normalize) against float64 through tests/front_end_ref.py: every bin of every frame within the derived budget, the
floor exact, the layout exact, nothing read outside an utterance (NaN around all of them), nothing written outside the
output (a sentinel around it), and an utterance's result independent of the batch it sits in."""
import ctypes

import numpy as np
import pytest

import front_end_ref as fr

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def expected(case):
    if case.name not in _EXPECTED:
        _EXPECTED[case.name] = fr.stft_expected(case)
    return _EXPECTED[case.name]


def run_stft(case, hip_lib):
    """The bare launch of a case: NaN before, between and behind the utterances, the sentinel all over the output."""
    import torch
    dev = torch.device("cuda:0")
    audio = torch.from_numpy(fr.audio_buffer(case)).to(dev)
    off = torch.from_numpy(case.offsets).to(dev)
    lengths = torch.tensor([len(u) for u in case.utterances], dtype=torch.int32, device=dev)
    batch = len(case.utterances)
    out = torch.full((batch * case.batch_stride,), float(fr.SENTINEL), dtype=torch.float32, device=dev)
    hip_lib.call("sl_stft_power_db", audio.data_ptr(), off.data_ptr(), lengths.data_ptr(), out.data_ptr(), batch,
                 case.max_frames, case.n_fft, case.hop, case.row_stride, case.batch_stride, case.min_db,
                 torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ sl_stft_power_db
@pytest.mark.parametrize("name", [c.name for c in fr.stft_cases()])
def test_stft_levels_within_the_budget_at_every_bin(name, hip_lib):
    """Worst (|a^ - a_f| - 1e-5 a_f) / delta_t measured on the MI355X: see DESIGN.md section 3.8."""
    case = fr.stft_case(name)
    got = run_stft(case, hip_lib)
    worst, problems = fr.case_report(case, got, expected(case))
    print("sl_stft_power_db", name, "worst error / bound", worst)
    assert not problems, "{}: worst error / bound {}: {}".format(name, worst, "; ".join(problems))
    assert worst <= 1


def test_stft_rows_do_not_depend_on_the_batch(hip_lib):
    case = fr.stft_case("n512_ragged")
    together = run_stft(case, hip_lib)
    for b, u in enumerate(case.utterances):
        alone = case._replace(name="alone", utterances=[u], offsets=np.zeros(1, dtype=np.int64))
        got = run_stft(alone, hip_lib)
        want = together[b * case.batch_stride:(b + 1) * case.batch_stride]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), b
    frames = 1 + len(case.utterances[0]) // case.hop
    assert np.count_nonzero(together[:frames * case.row_stride]) >= frames * 257


# ------------------------------------------------------------------------------------------------ mel projection
def project(ext, level, t_max):
    """The sl_conv1d_nt call of SpectrogramExtractor.batch_device over a level buffer (B, rows, bins_pad)."""
    import torch
    from speechless_amd import _lib
    b, rows = level.shape[0], level.shape[1]
    mel = torch.full((b, rows, ext.mel_pad), float(fr.SENTINEL), dtype=torch.float32, device=level.device)
    g = _lib.ConvGeom()
    g.batch, g.t_out, g.taps, g.cin, g.cout = b, t_max, 1, ext.bins_pad, ext.mel_pad
    g.x_row0, g.x_row_stride, g.x_batch_stride = 0, ext.bins_pad, rows * ext.bins_pad
    g.y_row0, g.y_row_stride, g.y_batch_stride = 0, ext.mel_pad, rows * ext.mel_pad
    ext.lib.call("sl_conv1d_nt", level.data_ptr(), ext.mel_w.data_ptr(), None, None, mel.data_ptr(), ctypes.byref(g),
                 _lib.EPI_NONE, _lib.SL_F32, 0, 0, None, 0, torch.cuda.current_stream().cuda_stream)
    return mel


@pytest.mark.parametrize("n_fft,rate,n_mels", [(512, 16000, 128), (512, 16000, 40), (256, 8000, 40)])
def test_mel_projection_within_the_accumulation_bound(n_fft, rate, n_mels):
    """The projection of the kernel's own level rows, and of hand-made rows at the extremes of the level range (the
    largest sum |w| |x|), against the float64 product: (cin_pad + 2) 2^-24 sum |w| |level|, any accumulation order."""
    import torch
    from speechless_amd.spectrogram import SpectrogramExtractor, TIME_TILE
    hop, bins = n_fft // 4, n_fft // 2 + 1
    ext = SpectrogramExtractor(sample_rate=rate, fourier_window_length=n_fft, hop_length=hop, mel_frequency_count=n_mels)
    bank = ext.mel_w[:n_mels, 0, :].cpu().numpy()
    assert bank.shape == (n_mels, ext.bins_pad) and not bank[:, bins:].any() and not ext.mel_w[n_mels:].any()
    audios = [fr.chirps(32 * hop + 9, 61), fr.chirps(14 * hop + 1, 62, silence=(3 * hop, 9 * hop)),
              fr.chirps(n_fft // 2 + 1, 63, gain=2.0 ** 15)]
    flat, offsets, lengths = ext.flatten(audios)
    dev = ext.device
    rows = TIME_TILE
    level = torch.full((3, rows, ext.bins_pad), float(fr.SENTINEL), dtype=torch.float32, device=dev)
    # (named, so that they outlive the launch: a temporary's memory is handed out again before the kernel reads it)
    flat_dev, off_dev, len_dev = (torch.from_numpy(a).to(dev) for a in (flat, offsets, lengths))
    ext.lib.call("sl_stft_power_db", flat_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(), level.data_ptr(), 3, rows,
                 n_fft, hop, ext.bins_pad, rows * ext.bins_pad, -150.0, torch.cuda.current_stream().cuda_stream)
    by_hand = np.zeros((3, rows, ext.bins_pad), dtype=np.float32)
    by_hand[0, :33, :bins] = -150
    by_hand[1, :33, :bins] = 90
    by_hand[2, :33, :bins] = np.where((np.arange(33)[:, None] + np.arange(bins)[None, :]) % 2, 90, -150)
    worst = {}
    for kind, buf in (("stft", level), ("by hand", torch.from_numpy(by_hand).to(dev))):
        rows_host = buf.cpu().numpy()
        if kind == "stft":
            assert (rows_host[0, :33, :bins] != 0).all() and not rows_host[1, 15:].any() and (rows_host[1, 5, :bins] == -150).all()
        for t_max in (1, 15, 33):
            got = project(ext, buf, t_max).cpu().numpy()
            worst[kind, t_max] = fr.compare_mel(got[:, :t_max, :n_mels], rows_host[:, :t_max], bank)
            assert not got[:, :t_max, n_mels:].any()  # (the padded output channels have zero weights)
    print("mel projection", (n_fft, rate, n_mels), "worst error / bound", worst)
    assert 0 < max(worst.values()) <= 1


# ------------------------------------------------------------------------------------------------ sl_z_normalize
ZFRAMES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 257]


def run_znorm(hip_lib, src, frames, f, max_frames, slack=13):
    """src (B, rows, stride) on the host.  The launch reads it from a buffer whose utterances lie rows * stride + slack
    apart (NaN in the slack) and writes into a sentinel-filled (B, max_frames, f)."""
    import torch
    dev = torch.device("cuda:0")
    b, rows, stride = src.shape
    spaced = np.full((b, rows * stride + slack), np.nan, dtype=np.float32)
    spaced[:, :rows * stride] = src.reshape(b, -1)
    src_dev = torch.from_numpy(spaced).to(dev)
    frames_dev = torch.tensor(frames, dtype=torch.int32, device=dev)
    dst = torch.full((b, max_frames, f), float(fr.SENTINEL), dtype=torch.float32, device=dev)
    ws = torch.empty((hip_lib.raw("sl_z_normalize_workspace_bytes")(b),), dtype=torch.uint8, device=dev)
    hip_lib.call("sl_z_normalize", src_dev.data_ptr(), frames_dev.data_ptr(), dst.data_ptr(), b, max_frames, f, stride,
                 rows * stride + slack, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    return dst.cpu().numpy()


@pytest.mark.parametrize("stride_kind", ["f", "f+7", "64s"])
@pytest.mark.parametrize("f", [1, 40, 128, 257])
def test_z_normalize_against_float64(f, stride_kind, hip_lib):
    """0, 1, 2 frames, one either side of the 32 chunks of the statistics (and of twice that), 257; mixed in one batch
    and each alone; NaN in the padding columns, in the rows behind every utterance and between utterances.  With f = 1 a
    single frame is a constant input (standard deviation 0), which is left out: three frames stand in its place."""
    stride = {"f": f, "f+7": f + 7, "64s": fr.round_up(f, 64)}[stride_kind]
    frames = [3 if (f == 1 and n == 1) else n for n in ZFRAMES]
    rows = max(frames) + 4
    worst = {}
    for values in fr.ZNORM_VALUES:
        src = fr.znorm_source(frames, f, stride, rows, values, seed=7 + f)
        assert stride == f or np.isnan(src[:, :, f:]).all()
        got = run_znorm(hip_lib, src, frames, f, max(frames))
        worst[values] = fr.compare_znorm(got, src, frames, f)
        assert not got[0].any() and np.abs(got[1:]).max() > 0.5
        # rows beyond the longest utterance (max_frames % 8 != 0 both times): the same values, zeros behind
        wider = run_znorm(hip_lib, src, frames, f, max(frames) + 4)
        assert np.array_equal(wider[:, :max(frames)].view(np.uint32), got.view(np.uint32)) and not wider[:, max(frames):].any()
        # the batch in reverse: every utterance at another position, bit for bit
        back = run_znorm(hip_lib, src[::-1].copy(), frames[::-1], f, max(frames))
        assert np.array_equal(back[::-1].view(np.uint32), got.view(np.uint32))
        # ... and alone
        for b, n in enumerate(frames):
            for max_frames in (max(n, 1), n + 3):
                alone = run_znorm(hip_lib, src[b:b + 1, :n + 3], [n], f, max_frames)
                fr.compare_znorm(alone, src[b:b + 1], [n], f)
                assert np.array_equal(alone[0, :n].view(np.uint32), got[b, :n].view(np.uint32)), (values, n, max_frames)
    print("sl_z_normalize f", f, "stride", stride, "worst error / tolerance", worst)
    assert max(worst.values()) <= 1


# ------------------------------------------------------------------------------------------------ the extractor
@pytest.mark.parametrize("n_mels", [128, None])
def test_extractor_is_the_three_launches_chained(n_mels, hip_lib):
    import torch
    from speechless_amd.spectrogram import SpectrogramExtractor, TIME_TILE
    ext = SpectrogramExtractor(mel_frequency_count=n_mels)
    audios = [fr.chirps(n, 70 + i) for i, n in enumerate((1500, 257, 4099, 128 * 15, 903))]
    x, frames = ext.batch(audios)
    assert frames == [1 + len(a) // 128 for a in audios] == [12, 3, 33, 16, 8]
    features = 257 if n_mels is None else n_mels
    assert x.shape == (5, 33, features) and x.dtype == torch.float32
    flat, offsets, lengths = ext.flatten(audios)
    case = fr.StftCase("chained", 512, 128, -150.0, audios, offsets, TIME_TILE, ext.bins_pad, TIME_TILE * ext.bins_pad)
    level = run_stft(case, hip_lib).reshape(5, TIME_TILE, ext.bins_pad)
    fr.compare_case(case, level, expected(case))
    src = level
    if n_mels is not None:
        src = project(ext, torch.from_numpy(level).to(ext.device), 33).cpu().numpy()
        fr.compare_mel(src[:, :33, :n_mels], level[:, :33], ext.mel_w[:n_mels, 0, :].cpu().numpy())
    chained = run_znorm(hip_lib, src, frames, features, 33, slack=0)
    fr.compare_znorm(chained, src[:, :33], frames, features)
    got = x.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), chained.view(np.uint32))
    for i, a in enumerate(audios):
        one = ext.one(a)
        assert one.shape == (frames[i], features) and np.array_equal(one.view(np.uint32), got[i, :frames[i]].view(np.uint32)), i
