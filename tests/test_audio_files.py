"""speechless_amd.audio: the RIFF / WAVE parser.  PCM16 fixtures are written with the stdlib `wave` module, everything else
is assembled by hand (wav_bytes below), all into tmp_path."""
import struct
import wave

import numpy as np
import pytest

from speechless_amd.audio import read_wav, wav_duration_in_s, wav_sample_rate

PCM, FLOAT, EXTENSIBLE = 1, 3, 0xFFFE


def wav_bytes(payload, tag, bits, rate, channels=1, extensible=False, extra_chunks=(), data_size=None, riff=b"RIFF"):
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", EXTENSIBLE if extensible else tag, channels, rate, rate * block, block, bits)
    if extensible:  # cbSize 22: valid bits, channel mask, sub-format GUID (the tag, then the fixed tail)
        fmt += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt
    for chunk_id, chunk in extra_chunks:
        body += chunk_id + struct.pack("<I", len(chunk)) + chunk + (b"\0" if len(chunk) & 1 else b"")
    body += b"data" + struct.pack("<I", len(payload) if data_size is None else data_size) + payload
    return riff + struct.pack("<I", len(body)) + body


def write(tmp_path, name, data):
    path = tmp_path / name
    path.write_bytes(data)
    return path


def test_pcm16_written_by_the_wave_module(tmp_path):
    v = np.array([0, 1, -1, 32767, -32768, 12345, -20000], dtype="<i2")
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(44100)
        f.writeframes(v.tobytes())
    samples, rate = read_wav(path)
    assert rate == 44100 == wav_sample_rate(path)
    assert samples.dtype == np.float32 and np.array_equal(samples, v.astype(np.float32) / np.float32(32768))
    assert wav_duration_in_s(path) == len(v) / 44100


def test_every_accepted_format_at_its_scaling(tmp_path):
    u8 = np.array([0, 1, 127, 128, 129, 255], dtype=np.uint8)
    s, r = read_wav(write(tmp_path, "u8.wav", wav_bytes(u8.tobytes(), PCM, 8, 8000)))
    assert r == 8000 and np.array_equal(s, ((u8.astype(np.float64) - 128) / 128).astype(np.float32))

    v24 = np.array([0, 1, -1, 2 ** 23 - 1, -2 ** 23, 1234567, -7654321], dtype=np.int64)
    raw = b"".join(int(x & 0xFFFFFF).to_bytes(3, "little") for x in v24)
    s, r = read_wav(write(tmp_path, "s24.wav", wav_bytes(raw, PCM, 24, 48000)))
    assert r == 48000 and np.array_equal(s, (v24 / 2.0 ** 23).astype(np.float32))

    v32 = np.array([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 123456789], dtype="<i4")
    s, _ = read_wav(write(tmp_path, "s32.wav", wav_bytes(v32.tobytes(), PCM, 32, 22050)))
    assert np.array_equal(s, (v32.astype(np.float64) / 2.0 ** 31).astype(np.float32))

    f32 = np.array([0.0, 0.25, -1.0, 1e-7, 0.999], dtype="<f4")
    s, _ = read_wav(write(tmp_path, "f32.wav", wav_bytes(f32.tobytes(), FLOAT, 32, 48000)))
    assert np.array_equal(s, f32)

    f64 = np.array([0.0, 0.1, -0.3, 1.0 / 3], dtype="<f8")
    s, _ = read_wav(write(tmp_path, "f64.wav", wav_bytes(f64.tobytes(), FLOAT, 64, 16000)))
    assert s.dtype == np.float32 and np.array_equal(s, f64.astype(np.float32))


def test_stereo_is_the_mean_of_the_float32_channels(tmp_path):
    v = np.array([[100, 300], [-5, 5], [32767, 32767], [-32768, 0], [1, 2]], dtype="<i2")
    path = write(tmp_path, "st.wav", wav_bytes(v.tobytes(), PCM, 16, 44100, channels=2))
    s, r = read_wav(path)
    want = (v.astype(np.float32) / np.float32(32768)).T.mean(axis=0)  # librosa.to_mono on (channels, n) float32
    assert r == 44100 and s.shape == (5,) and np.array_equal(s, want)
    assert wav_duration_in_s(path) == 5 / 44100


@pytest.mark.parametrize("tag,bits,dtype", [(PCM, 16, "<i2"), (FLOAT, 32, "<f4")])
def test_extensible_header(tmp_path, tag, bits, dtype):
    v = np.array([0, 1, -1, 100], dtype=dtype)
    path = write(tmp_path, "x.wav", wav_bytes(v.tobytes(), tag, bits, 48000, extensible=True))
    s, r = read_wav(path)
    want = v.astype(np.float32) / np.float32(32768) if tag == PCM else v
    assert r == 48000 == wav_sample_rate(path) and np.array_equal(s, want)


def test_odd_list_chunk_in_front_of_data_and_streaming_sizes(tmp_path):
    v = np.array([5, -6, 7, -8], dtype="<i2")
    want = v.astype(np.float32) / np.float32(32768)
    odd = wav_bytes(v.tobytes(), PCM, 16, 22050, extra_chunks=[(b"LIST", b"INFOabc"), (b"fact", b"\x04\0\0\0")])
    path = write(tmp_path, "odd.wav", odd)
    s, r = read_wav(path)
    assert r == 22050 == wav_sample_rate(path) and np.array_equal(s, want)
    for i, size in enumerate((0, 0xFFFFFFFF)):
        s, _ = read_wav(write(tmp_path, "stream{}.wav".format(i), wav_bytes(v.tobytes(), PCM, 16, 22050, data_size=size)))
        assert np.array_equal(s, want)


def test_rejections_name_what_they_found(tmp_path):
    v = np.zeros(8, dtype="<i2").tobytes()
    with pytest.raises(ValueError, match="mu-law"):
        read_wav(write(tmp_path, "mulaw.wav", wav_bytes(v, 7, 8, 8000)))
    with pytest.raises(ValueError, match="MPEG"):
        wav_sample_rate(write(tmp_path, "mp3.wav", wav_bytes(v, 0x55, 16, 44100)))
    with pytest.raises(ValueError, match="PCM 12 bit"):
        read_wav(write(tmp_path, "p12.wav", wav_bytes(v, PCM, 12, 8000)))
    with pytest.raises(ValueError, match="A-law"):
        read_wav(write(tmp_path, "xalaw.wav", wav_bytes(v, 6, 8, 8000, extensible=True)))
    with pytest.raises(ValueError, match="FLAC"):
        read_wav(write(tmp_path, "a.flac", b"fLaC" + bytes(64)))
    with pytest.raises(ValueError, match="not a RIFF"):
        read_wav(write(tmp_path, "a.bin", b"RIFX" + bytes(64)))
    with pytest.raises(ValueError, match="truncated"):
        read_wav(write(tmp_path, "short.wav", wav_bytes(v, PCM, 16, 8000)[:30]))
    with pytest.raises(ValueError, match="truncated"):
        read_wav(write(tmp_path, "nodata.wav", wav_bytes(v, PCM, 16, 8000)[:36]))
    with pytest.raises(ValueError):
        read_wav(write(tmp_path, "empty.wav", b""))
