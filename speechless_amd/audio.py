"""WAV files without a decoder library: a RIFF parser on numpy.

`read_wav(path)` is what `librosa.load(path, sr=None)` returns for such a file -- float32 samples, several channels averaged
(librosa.to_mono) -- and `wav_sample_rate(path)` reads the header only.  Python's `wave` module rejects IEEE-float and
WAVE_FORMAT_EXTENSIBLE files; compressed codecs, FLAC and everything that is not RIFF / WAVE raise a ValueError that names
what was found (decoding them is out of scope: convert such a corpus to WAV once).
"""
import struct
from pathlib import Path

import numpy as np

WAVE_FORMAT_PCM = 1
WAVE_FORMAT_IEEE_FLOAT = 3
WAVE_FORMAT_EXTENSIBLE = 0xFFFE
_CODEC_NAMES = {2: "MS ADPCM", 6: "A-law", 7: "mu-law", 0x11: "IMA ADPCM", 0x31: "GSM 6.10", 0x55: "MPEG layer 3"}


class WavFormat:
    def __init__(self, format_tag, channels, sample_rate, block_align, bits):
        self.format_tag, self.channels, self.sample_rate = format_tag, channels, sample_rate
        self.block_align, self.bits = block_align, bits

    def describe(self):
        name = {WAVE_FORMAT_PCM: "PCM", WAVE_FORMAT_IEEE_FLOAT: "IEEE float"}.get(
            self.format_tag, _CODEC_NAMES.get(self.format_tag, "format tag 0x{:04x}".format(self.format_tag)))
        return "{} {} bit".format(name, self.bits)


def _parse_fmt(path, body):
    if len(body) < 16:
        raise ValueError("{}: truncated WAV header (fmt chunk of {} bytes)".format(path, len(body)))
    tag, channels, rate, _, block_align, bits = struct.unpack("<HHIIHH", body[:16])
    if tag == WAVE_FORMAT_EXTENSIBLE:  # cbSize, valid bits, channel mask, then a GUID whose first two bytes are the real tag
        if len(body) < 40:
            raise ValueError("{}: truncated WAV header (extensible fmt chunk of {} bytes)".format(path, len(body)))
        tag = struct.unpack("<H", body[24:26])[0]
    fmt = WavFormat(tag, channels, rate, block_align, bits)
    supported = (tag == WAVE_FORMAT_PCM and bits in (8, 16, 24, 32)) or (tag == WAVE_FORMAT_IEEE_FLOAT and bits in (32, 64))
    if not supported:
        raise ValueError("{}: unsupported WAV format: {} (PCM 8 / 16 / 24 / 32 bit and IEEE float 32 / 64 bit are read)".format(
            path, fmt.describe()))
    if channels < 1 or rate < 1:
        raise ValueError("{}: WAV header with {} channels at {} Hz".format(path, channels, rate))
    return fmt


def _open_riff(path, f):
    head = f.read(12)
    if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
        kind = "FLAC" if head[:4] == b"fLaC" else "Ogg" if head[:4] == b"OggS" else "not a RIFF / WAVE file"
        raise ValueError("{}: {} (first bytes {!r}); only WAV files are read".format(path, kind, head[:4]))


def _chunks(path, f):
    """(id, size, position of the body) of every chunk up to and including `data`; the file is left at the body of the last"""
    while True:
        head = f.read(8)
        if len(head) < 8:
            raise ValueError("{}: truncated WAV file (no data chunk)".format(path))
        size = struct.unpack("<I", head[4:])[0]
        yield head[:4], size
        if head[:4] == b"data":
            return


def _header(path, f):
    """(WavFormat, bytes of sample data, taken to the end of the file when the header leaves them open)"""
    _open_riff(path, f)
    fmt = None
    for chunk_id, size in _chunks(path, f):
        if chunk_id == b"fmt ":
            fmt = _parse_fmt(path, f.read(size))
            f.seek(size & 1, 1)
        elif chunk_id == b"data":
            if fmt is None:
                raise ValueError("{}: WAV data chunk without a fmt chunk in front of it".format(path))
            here = f.tell()
            rest = f.seek(0, 2) - here
            f.seek(here)
            if size in (0, 0xFFFFFFFF) or size > rest:  # streaming writers leave the size open; a cut file has less
                size = rest
            return fmt, size
        else:
            f.seek(size + (size & 1), 1)  # unknown chunk; odd sizes are padded to an even one
    raise ValueError("{}: truncated WAV file (no data chunk)".format(path))


def wav_sample_rate(path):
    with Path(path).open("rb") as f:
        return _header(path, f)[0].sample_rate


def wav_duration_in_s(path):
    with Path(path).open("rb") as f:
        fmt, size = _header(path, f)
    frame = fmt.channels * fmt.bits // 8
    return size // frame / fmt.sample_rate


def read_wav(path):
    """(float32 mono samples, sample rate).  PCM 8 bit unsigned: (v - 128) / 128; 16 / 24 / 32 bit: / 2^15, 2^23, 2^31; IEEE
    float 32 / 64: as stored, cast to float32.  Several channels: the mean of the float32 samples."""
    with Path(path).open("rb") as f:
        fmt, size = _header(path, f)
        frame = fmt.channels * fmt.bits // 8
        raw = f.read(size - size % frame)
    raw = raw[:len(raw) - len(raw) % frame]
    if fmt.format_tag == WAVE_FORMAT_IEEE_FLOAT:
        samples = np.frombuffer(raw, dtype="<f4" if fmt.bits == 32 else "<f8").astype(np.float32)
    elif fmt.bits == 8:
        samples = ((np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0).astype(np.float32)
    elif fmt.bits == 16:
        samples = np.frombuffer(raw, dtype="<i2").astype(np.float32) / np.float32(32768.0)
    elif fmt.bits == 24:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = v - ((v & 0x800000) << 1)  # sign extension
        samples = v.astype(np.float32) / np.float32(8388608.0)
    else:
        samples = (np.frombuffer(raw, dtype="<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    if fmt.channels > 1:
        samples = samples.reshape(-1, fmt.channels).mean(axis=1, dtype=np.float32)
    return np.ascontiguousarray(samples, dtype=np.float32), fmt.sample_rate
