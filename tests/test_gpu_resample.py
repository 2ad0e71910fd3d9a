"""sl_resample_polyphase and what is built on it (speechless_amd/resample.py, spectrogram.LabeledExampleFromFile, the staged
training and prediction from files at mixed sample rates) against the float64 restatement of tests/resample_ref.py."""
import struct
import wave

import numpy as np
import pytest

import resample_ref as rr
from oracle import spectrogram_oracle as so
from speechless_amd.resample import MAX_PHASES, MAX_TAPS, TILE, polyphase_bank, rate_ratio

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-777.25)
_BANKS = {}


def bank32(pair):
    if pair not in _BANKS:
        _BANKS[pair] = polyphase_bank(*pair)
    return _BANKS[pair]


def run_ragged(pair, utterances, gap=5):
    """The bare launch over utterances laid out with `gap` sentinel floats around every input and output.  Returns the
    per-utterance outputs and the whole output buffer with the outputs cut out (what must still be the sentinel)."""
    import torch
    from speechless_amd.resample import shared_resampler
    rs = shared_resampler(pair[0], pair[1], "cuda:0")
    lengths = np.array([len(u) for u in utterances], dtype=np.int32)
    out_lengths = np.array([rs.output_length(n) for n in lengths], dtype=np.int64)
    in_off = gap + np.concatenate([[0], np.cumsum(lengths[:-1] + gap)]).astype(np.int64)
    out_off = gap + np.concatenate([[0], np.cumsum(out_lengths[:-1] + gap)]).astype(np.int64)
    flat = np.full(int(in_off[-1] + lengths[-1] + gap), 1e30, dtype=np.float32)  # (a read outside an utterance shows)
    for u, o in zip(utterances, in_off):
        flat[o:o + len(u)] = u
    out = torch.full((int(out_off[-1] + out_lengths[-1] + gap),), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    rs.launch(torch.from_numpy(flat).cuda(), torch.from_numpy(in_off).cuda(), torch.from_numpy(lengths).cuda(), out,
              torch.from_numpy(out_off).cuda(), len(utterances))
    got = out.cpu().numpy()
    parts = [got[o:o + n].copy() for o, n in zip(out_off, out_lengths)]
    rest = got.copy()
    for o, n in zip(out_off, out_lengths):
        rest[o:o + n] = SENTINEL
    return parts, rest


def impulse_response(pair, n_in, m):
    """What the definition gives for x = 1.0 at sample m: one fp32 bank entry per output, exactly."""
    h, left, _ = bank32(pair)
    p, q = rate_ratio(*pair)
    n_out, n_res = rr.lengths(n_in, p, q)
    t = np.arange(n_out, dtype=np.int64)
    n, r = (t * p) // q, (t * p) % q
    j = m - n + left - 1
    ok = (j >= 0) & (j < h.shape[1]) & (t < n_res)
    want = np.zeros(n_out, dtype=np.float32)
    want[ok] = h[r[ok], j[ok]]
    return want


@pytest.mark.parametrize("pair", rr.RATE_PAIRS)
def test_impulses_select_the_banks_entries_bit_for_bit(pair):
    p, q = rate_ratio(*pair)
    long_in = -(-2 * TILE * p // q) + 301  # more than two tiles of outputs: the utterance spans three
    assert rr.lengths(long_in, p, q)[0] > 2 * TILE
    edge1, edge2 = TILE * p // q, 2 * TILE * p // q  # the input samples under the first outputs of tiles 1 and 2
    cases = [(long_in, 0), (long_in, long_in - 1), (long_in, edge1), (long_in, edge1 - 1), (long_in, edge2 + 1),
             (long_in, edge2 - 3), (1, 0), (37, 36), (37, 0), (TILE * p // q + 1, TILE * p // q)]
    utterances = []
    for n_in, m in cases:
        x = np.zeros(n_in, dtype=np.float32)
        x[m] = 1.0
        utterances.append(x)
    parts, rest = run_ragged(pair, utterances)
    assert np.all(rest == SENTINEL)
    for (n_in, m), got in zip(cases, parts):
        want = impulse_response(pair, n_in, m)
        assert got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (pair, n_in, m)
        assert n_in == 1 or np.count_nonzero(want) > 0


@pytest.mark.parametrize("pair", rr.RATE_PAIRS)
def test_noise_within_the_fma_bound(pair):
    """|got - want| <= (width + 2) 2^-24 mag: `width` fp32 FMAs in any order against the float64 sum over the same fp32 bank."""
    h, left, _ = bank32(pair)
    p, q = rate_ratio(*pair)
    width = h.shape[1]
    rng = np.random.RandomState(21)
    utterances = [rng.uniform(-1, 1, size=n).astype(np.float32) for n in (1, 37, 255, 256, 257, 4411, 14400)]
    utterances[5] = (utterances[5] * np.float32(2.0 ** -12)).astype(np.float32)
    parts, rest = run_ragged(pair, utterances)
    assert np.all(rest == SENTINEL)  # nothing outside the outputs is written
    worst = 0.0
    for x, got in zip(utterances, parts):
        want, mag = rr.fir(x, h, left, p, q)
        n_out, n_res = rr.lengths(len(x), p, q)
        assert got.shape == (n_out,)
        assert np.all(got[n_res:] == 0.0)  # the zero tail, exactly
        bound = (width + 2) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - want)
        worst = max(worst, float((err[mag > 0] / bound[mag > 0]).max()) if np.any(mag > 0) else 0.0)
        assert np.all(err <= bound), (pair, len(x), float((err - bound).max()))
    print(pair, "worst error / bound", worst)


def test_one_equals_its_slice_of_the_batch():
    import torch
    from speechless_amd.resample import Resampler
    rs = Resampler(44100, 16000, "cuda:0")
    rng = np.random.RandomState(22)
    audios = [rng.uniform(-1, 1, size=n).astype(np.float32) for n in (3000, 7001, 500)]
    lengths = np.array([len(a) for a in audios], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lengths[:-1])]).astype(np.int64)
    bufs = {}
    for _ in range(2):  # the second call reuses the caller's buffers
        flat, off, ln, lengths_out = rs.batch_device(torch.from_numpy(np.concatenate(audios)).cuda(),
                                                     torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda(),
                                                     lengths, bufs=bufs)
    kept = {k: v.data_ptr() for k, v in bufs.items()}
    flat, off, ln, lengths_out = rs.batch_device(torch.from_numpy(np.concatenate(audios)).cuda(),
                                                 torch.from_numpy(offsets).cuda(), torch.from_numpy(lengths).cuda(), lengths,
                                                 bufs=bufs)
    assert kept == {k: v.data_ptr() for k, v in bufs.items()}
    flat, off = flat.cpu().numpy(), off.cpu().numpy()
    assert list(ln.cpu().numpy()) == list(lengths_out) == [rs.output_length(n) for n in lengths]
    for a, o, n in zip(audios, off, lengths_out):
        one = rs.one(a)
        assert one.dtype == np.float32 and np.array_equal(one.view(np.uint32), flat[o:o + n].view(np.uint32))


# ---------------------------------------------------------------------------------------------- files
def write_pcm16(path, audio, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.round(np.clip(audio, -1, 1) * 32767).astype("<i2").tobytes())
    return path


def write_float32(path, audio, rate):
    payload = np.asarray(audio, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, rate, rate * 4, 4, 32)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload
    path.write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def synthetic_audio(seconds, seed, sample_rate):
    """Broadband noise with a few weak drifting tones below 6 kHz, at any rate.  The 2e-3 tolerance of the front end
    (test_spectrogram.py) is stated for bins well above fp32 round-off.  A converted signal has next to nothing left between the
    filter's cut-off (7.58 kHz) and 8 kHz, and fp32 SAMPLES carry round-off about 150 dB below the signal's level whatever
    produced them; under tones 25 dB above the noise, as in test_spectrogram.py, what the filter leaves of the noise up there is
    no more than that round-off.  So the noise is the louder part here, which keeps the top mel bins 20 dB and more above it."""
    rng = np.random.RandomState(seed)
    n = int(seconds * sample_rate)
    t = np.arange(n) / sample_rate
    y = 0.1 * rng.randn(n)
    for _ in range(4):
        f0, f1 = rng.uniform(100, 6000, size=2)
        y += rng.uniform(0.01, 0.03) * np.sin(2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / seconds))
    return (y * np.hanning(n) ** 0.25).astype(np.float32)


@pytest.mark.parametrize("rate,writer", [(44100, write_pcm16), (48000, write_float32)])
def test_labeled_example_from_file(tmp_path, rate, writer):
    from speechless_amd.alignment import PositionalLabel
    from speechless_amd.audio import read_wav
    from speechless_amd.resample import Resampler
    from speechless_amd.spectrogram import LabeledExample, LabeledExampleFromFile
    path = writer(tmp_path / "utt-7.wav", synthetic_audio(1.1, 31, rate), rate)
    example = LabeledExampleFromFile(path, label="abc de", positional_label=PositionalLabel([("abc", (0.1, 0.4)), ("de", (0.5, 0.9))]))
    assert isinstance(example, LabeledExample)
    assert example.id == "utt-7" and example.audio_file == path and example.audio_directory == tmp_path
    assert example.sample_rate == 16000 and example.original_sample_rate == rate == LabeledExampleFromFile.file_sample_rate(path)
    samples, file_rate = read_wav(path)
    assert file_rate == rate and example.duration_in_s == len(samples) / rate
    original, original_rate = example.get_original_audio()
    assert original_rate == rate and np.array_equal(original, samples)
    raw = example.get_raw_audio()
    assert np.array_equal(raw, Resampler(rate, 16000, "cuda:0").one(samples))
    # the spectrogram against the float64 oracle of the float64 filter output over the same fp32 bank
    h, left, _ = bank32((rate, 16000))
    want_audio, mag = rr.fir(samples, h, left, *rate_ratio(rate, 16000))
    assert np.all(np.abs(raw - want_audio) <= (h.shape[1] + 2) * 2.0 ** -24 * mag)
    want = so.z_normalized_transposed_spectrogram(want_audio)
    got = example.z_normalized_transposed_spectrogram()
    assert got.shape == want.shape and np.abs(got - want).max() < 2e-3
    sections = example.sections()
    assert [s.label for s in sections] == ["abc", "de"]
    for section, (start, end) in zip(sections, ((0.1, 0.4), (0.5, 0.9))):
        assert np.array_equal(section.get_raw_audio(), raw[int(start * 16000):int(end * 16000)]) and len(section.get_raw_audio()) > 4000
    assert sections[0].sample_rate == 16000 and sections[0].mel_frequency_count == 128
    assert LabeledExampleFromFile(path).sections() is None and LabeledExampleFromFile(path, id="x").id == "x"
    # a file at the net's rate is returned as it is
    same = write_pcm16(tmp_path / "same.wav", synthetic_audio(0.5, 32, 16000), 16000)
    assert np.array_equal(LabeledExampleFromFile(same).get_raw_audio(), read_wav(same)[0])


def test_training_and_prediction_from_files_at_mixed_rates(tmp_path):
    """Wav2Letter.train(from_audio=True) on LabeledExampleFromFile objects (16, 44.1 and 48 kHz mixed within a batch; converted
    in HBM in front of the front end) ends in the very weights of the same run on plain LabeledExample objects that return
    Resampler.one() of each file -- with the front end on the compute stream and on the copy stream."""
    from speechless_amd import Wav2Letter, english_frequent_characters
    from speechless_amd.audio import read_wav
    from speechless_amd.net import Adam
    from speechless_amd.resample import resample
    from speechless_amd.spectrogram import LabeledExample, LabeledExampleFromFile
    rng = np.random.RandomState(5)
    words = ["she", "wasn't", "three", "abc", "xyz", "a", "it's", "zoo"]
    rates = [16000, 44100, 48000]
    file_batches, plain_batches = [], []
    for j in range(9):
        files, plains = [], []
        for i in range(int(rng.randint(2, 5))):
            rate = rates[(j + i) % 3] if j != 4 else 16000  # (batch 4: nothing to convert)
            audio = synthetic_audio(float(rng.uniform(1.0, 1.6)), 100 + 10 * j + i, rate)
            path = (write_pcm16 if i % 2 else write_float32)(tmp_path / "b{}u{}.wav".format(j, i), audio, rate)
            label = " ".join(rng.choice(words, size=rng.randint(1, 4)))
            files.append(LabeledExampleFromFile(path, label=label))
            converted = resample(read_wav(path)[0], rate, 16000)
            plains.append(LabeledExample(lambda a=converted: a, id=files[-1].id, label=label))
        file_batches.append(files)
        plain_batches.append(plains)
    small = dict(main_filter_count=250, out_filter_count=256, inner_count=2)
    finals = []
    for batches, on_copy in ((plain_batches, False), (file_batches, False), (file_batches, True)):
        net = Wav2Letter(128, english_frequent_characters, optimizer=Adam(1e-3), seed=4, layer_sizes=small)
        net.train(batches, preview_labeled_spectrogram_batch=batches[0][:2], tensor_board_log_directory=None,
                  net_directory=tmp_path / "n{}".format(len(finals)), batches_per_epoch=3, from_audio=True,
                  front_end_on_copy_stream=on_copy)
        finals.append([w.copy() for w, _ in net.predictive_net.get_weights()])
    moved = 0.0
    for a, b, c in zip(*finals):
        assert np.array_equal(a, b) and np.array_equal(a, c)
        moved = max(moved, float(np.abs(a).max()))
    assert moved > 0
    originals = [x.get_original_audio() for x in file_batches[0]]
    got = net.predict_batch_greedily_from_audio([a for a, _ in originals], original_sample_rates=[r for _, r in originals])
    assert got == net.predict_batch_greedily_from_audio([x.get_raw_audio() for x in plain_batches[0]])
    assert got == net.predict_batch_greedily_from_audio([x.get_raw_audio() for x in plain_batches[0]],
                                                        original_sample_rates=[16000] * len(originals))
    # (a net this young transcribes nothing, so also what the conv stack is fed: the same spectrograms, bit for bit)
    import torch
    extractor = net._audio_extractor(file_batches[0][0])
    x_files, frames_files = net._front_end_at_mixed_rates(extractor, [a for a, _ in originals], [r for _, r in originals])
    x_plain, frames_plain = extractor.batch([x.get_raw_audio() for x in plain_batches[0]])
    assert frames_files == frames_plain and torch.equal(x_files, x_plain)


# ---------------------------------------------------------------------------------------------- the launcher's refusals
def test_launcher_rejections(hip_lib):
    import torch
    audio = torch.zeros(64, dtype=torch.float32, device="cuda:0")
    out = torch.full((64,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    off = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    ln = torch.full((1,), 16, dtype=torch.int32, device="cuda:0")
    bank = torch.zeros((MAX_PHASES + 1) * 8 + MAX_TAPS + 1, dtype=torch.float32, device="cuda:0")
    fn = hip_lib.raw("sl_resample_polyphase")

    def call(p, q, left, width, audio_ptr=None):
        return fn(audio.data_ptr() if audio_ptr is None else audio_ptr, off.data_ptr(), ln.data_ptr(), out.data_ptr(),
                  off.data_ptr(), bank.data_ptr(), 1, p, q, left, width, None)

    for args, word in (((3, 3, 2, 4), "p == q"), ((6, 2, 2, 4), "lowest terms"), ((3, 1, 5, 4), "left"), ((3, 1, 0, 4), "left"),
                       ((0, 1, 2, 4), "positive"), ((MAX_PHASES + 2, MAX_PHASES + 1, 2, 4), "limits"),
                       ((3, 1, 2, MAX_TAPS + 1), "limits"), ((64, 1, 2, 4), "LDS")):
        rc = call(*args)
        assert rc < 0, args
        assert word in hip_lib.last_error(), (args, hip_lib.last_error())
    assert call(3, 1, 2, 4, audio_ptr=0) < 0 and "null" in hip_lib.last_error()
    torch.cuda.synchronize()
    assert torch.all(out == float(SENTINEL))  # nothing was launched
    assert call(3, 1, 2, 4) == 0  # ... and the same call with good arguments runs
    torch.cuda.synchronize()
    assert torch.all(out[:6] == 0) and torch.all(out[6:] == float(SENTINEL))
