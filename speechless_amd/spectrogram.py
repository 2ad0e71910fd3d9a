"""Audio -> z-normalised (mel) spectrogram on the MI355X (second half).

Mirrors the reference's speechless/labeled_example.py: `LabeledExample` with `get_raw_audio`, `sample_rate`,
`fourier_window_length` (512), `hop_length` (128), `mel_frequency_count` (128) and
`z_normalized_transposed_spectrogram() -> (frames, bins)` (labeled_example.py:74-140), which is what
`Wav2Letter` consumes (net.py:593).  The arithmetic the reference delegates to librosa / numpy runs in three launches:

    sl_stft_power_db   reflect-padded, Hann-windowed frames -> radix-2 FFT in LDS -> |D|^2 -> 10 log10 with the -150 floor
    sl_conv1d_nt       the mel projection of the LEVEL spectrogram (labeled_example.py:106-109, 114-129) as a 1 x 1
                       convolution on the exact-fp32 MFMA kernel (weights = librosa.filters.mel's matrix)
    sl_z_normalize     (a - mean) / std per utterance (labeled_example.py:28-29), zero rows behind short utterances

`SpectrogramExtractor.batch()` keeps the result in HBM as the zero-padded float32 (B, Tmax, F) batch that
`Engine.load_input` takes (net.py:578-587's layout), so a training or prediction step on raw audio never moves a
spectrogram over PCIe; `LabeledExample.z_normalized_transposed_spectrogram()` is the drop-in, numpy-returning form.

The rest of the reference's class (labeled_example.py:17-25, 96-171) stands on two more entry points: `sl_stft`, the same
Fourier kernel leaving |D|^2, |D| or D itself in the row (`spectrogram(type, frequency_scale)`, `spectrogram_batch`,
`stft_batch`), and `sl_istft`, librosa.istft as a gather (`reconstructed_audio_from_spectrogram`, `istft_batch`).
"""
import ctypes
import logging
from enum import Enum
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._lib import SL_TIME_TILE as TIME_TILE
from ._lib import ConvGeom, lib


class SpectrogramFrequencyScale(Enum):
    """labeled_example.py:17-19"""
    linear = "linear"
    mel = "mel"


class SpectrogramType(Enum):
    """labeled_example.py:22-25"""
    power = "power"
    amplitude = "amplitude"
    power_level = "power level"


_STFT_MODE = {SpectrogramType.power: _lib.STFT_POWER, SpectrogramType.amplitude: _lib.STFT_AMPLITUDE}


def _round_up(x, m):
    return (x + m - 1) // m * m


def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_hz / f_sp + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz, logstep = 200.0 / 3, 1000.0, np.log(6.4) / 27.0
    return np.where(m >= min_log_hz / f_sp, min_log_hz * np.exp(logstep * (m - min_log_hz / f_sp)), f_sp * m)


def mel_filter_bank(sample_rate, n_fft, n_mels):
    """The matrix librosa.filters.mel(sr, n_fft, n_mels) returns with its defaults (labeled_example.py:106-109): Slaney's
    mel scale between 0 and sr / 2, triangular filters on the FFT bin frequencies, each scaled by 2 / bandwidth."""
    bins = 1 + n_fft // 2
    fftfreqs = np.linspace(0, sample_rate / 2.0, bins)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(sample_rate / 2.0), n_mels + 2))
    widths = np.diff(edges)
    ramps = edges[:, None] - fftfreqs[None, :]
    bank = np.maximum(0, np.minimum(-ramps[:-2] / widths[:-1, None], ramps[2:] / widths[1:, None]))
    return bank * (2.0 / (edges[2:] - edges[:-2]))[:, None]


class SpectrogramExtractor:
    """Batched front end on one GPU.  mel_frequency_count=None keeps the linear frequency scale (1 + n_fft // 2 bins:
    the 257-bin power-level spectrograms of BASELINE config 5)."""

    def __init__(self, sample_rate=16000, fourier_window_length=512, hop_length=128, mel_frequency_count=128,
                 min_decibel=-150.0, device="cuda:0"):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("speechless_amd.spectrogram needs a ROCm GPU; there is no CPU fallback")
        self.lib = lib()
        self.device = torch.device(device)
        self.sample_rate = sample_rate
        self.n_fft = fourier_window_length
        self.hop = hop_length
        self.n_mels = mel_frequency_count
        self.min_decibel = float(min_decibel)
        self.bins = 1 + self.n_fft // 2
        self.bins_pad = _round_up(self.bins, 64)
        self.features = self.bins if mel_frequency_count is None else mel_frequency_count
        self.mel_w = None
        if mel_frequency_count is not None:
            self.mel_pad = _round_up(mel_frequency_count, 128)
            w = np.zeros((self.mel_pad, 1, self.bins_pad), dtype=np.float32)  # packed [cout][taps][cin] (sl_conv1d_nt)
            w[:mel_frequency_count, 0, :self.bins] = mel_filter_bank(sample_rate, self.n_fft, mel_frequency_count)
            self.mel_w = torch.from_numpy(w).to(self.device)

    def frame_count(self, sample_count):
        return 1 + sample_count // self.hop

    def batch(self, raw_audio_list):
        """raw_audio_list: 1-D float arrays (any float dtype).  Returns (x, frames): x float32 (B, Tmax, F) in HBM, every
        utterance z-normalised over its own frames and zero beyond them; frames int list."""
        flat, offsets, lengths = self.flatten(raw_audio_list)
        flat_dev = torch.from_numpy(flat).to(self.device, non_blocking=True)
        off_dev = torch.from_numpy(offsets).to(self.device, non_blocking=True)
        len_dev = torch.from_numpy(lengths).to(self.device, non_blocking=True)
        return self.batch_device(flat_dev, off_dev, len_dev, lengths)

    def flatten(self, raw_audio_list, out=None):
        """Host half of batch(): the utterances back to back as float32 (into `out`, a flat float32 array, if given),
        their start offsets (int64) and sample counts (int32)."""
        audios = [np.asarray(a).reshape(-1) for a in raw_audio_list]
        if not audios:
            raise ValueError("empty batch")
        lengths = np.array([a.shape[0] for a in audios], dtype=np.int32)
        if lengths.min() <= self.n_fft // 2:
            raise ValueError("audio shorter than {} samples cannot be reflect-padded (librosa.stft raises too)".format(
                self.n_fft // 2 + 1))
        offsets = np.zeros(len(audios), dtype=np.int64)
        offsets[1:] = np.cumsum(lengths[:-1])
        total = int(lengths.sum())
        flat = np.empty((total,), dtype=np.float32) if out is None else out[:total]
        for a, off, n in zip(audios, offsets, lengths):
            flat[off:off + n] = a  # (casts float64 / int16-scaled-by-the-reader input to float32)
        return flat, offsets, lengths

    def batch_device(self, flat_dev, off_dev, len_dev, lengths, frames_dev=None, bufs=None):
        """Device half of batch(): audio already in HBM (flat float32, int64 offsets, int32 sample counts; `lengths` the
        same counts on the host).  Everything is enqueued on the CURRENT stream -- the staged input pipeline calls this
        on its copy stream, right behind the H2D copy of the audio, so the front end of batch n + 1 runs under step n.
        bufs: a dict the caller owns (one per staging slot): intermediate and output tensors are kept there and reused, so
        that a steady-state call allocates nothing (allocations on a side stream whose results another stream reads make
        the caching allocator fall back to hipMalloc whenever the reader has not caught up: the staged run then jitters
        between 69 and 86 % of the resident rate)."""
        def tensor(name, shape, dtype):
            n = int(np.prod(shape))
            if bufs is None:
                return torch.empty(shape, dtype=dtype, device=self.device)
            flat = bufs.get(name)
            if flat is None or flat.numel() < n or flat.dtype != dtype:
                flat = bufs[name] = torch.empty((n,), dtype=dtype, device=self.device)
            return flat[:n].view(shape)

        frames = [self.frame_count(int(n)) for n in lengths]
        if frames_dev is None:  # (a pageable H2D copy: callers on the compute stream bring it along from their copy stream)
            frames_dev = torch.tensor(frames, dtype=torch.int32, device=self.device)
        b, t_max = len(frames), max(frames)
        rows = _round_up(t_max, TIME_TILE)  # sl_conv1d_nt reads whole time tiles
        st = torch.cuda.current_stream(self.device).cuda_stream
        level = tensor("level", (b, rows, self.bins_pad), torch.float32)
        self.lib.call("sl_stft_power_db", flat_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(), level.data_ptr(), b,
                      rows, self.n_fft, self.hop, self.bins_pad, rows * self.bins_pad, self.min_decibel, st)
        src, src_stride = level, self.bins_pad
        if self.mel_w is not None:
            mel = tensor("mel", (b, rows, self.mel_pad), torch.float32)
            self._mel_project(level, mel, t_max, st)
            src, src_stride = mel, self.mel_pad
        out = tensor("out", (b, t_max, self.features), torch.float32)
        ws = tensor("ws", (self.lib.raw("sl_z_normalize_workspace_bytes")(b),), torch.uint8)
        self.lib.call("sl_z_normalize", src.data_ptr(), frames_dev.data_ptr(), out.data_ptr(), b, t_max, self.features,
                      src_stride, rows * src_stride, ws.data_ptr(), ws.numel(), st)
        return out, frames

    def _mel_project(self, linear, mel, t_max, st):
        """The filter bank as a 1 x 1 fp32 convolution over the first t_max rows of linear (B, rows, bins_pad) into
        mel (B, rows, mel_pad)."""
        b, rows = linear.shape[0], linear.shape[1]
        g = ConvGeom()
        g.batch, g.t_out, g.taps, g.cin, g.cout = b, t_max, 1, self.bins_pad, self.mel_pad
        g.x_row0, g.x_row_stride, g.x_batch_stride = 0, self.bins_pad, rows * self.bins_pad
        g.y_row0, g.y_row_stride, g.y_batch_stride = 0, self.mel_pad, rows * self.mel_pad
        self.lib.call("sl_conv1d_nt", linear.data_ptr(), self.mel_w.data_ptr(), None, None, mel.data_ptr(), ctypes.byref(g),
                      _lib.EPI_NONE, _lib.SL_F32, 0, 0, None, 0, st)

    def one(self, raw_audio):
        x, frames = self.batch([raw_audio])
        return x[0, :frames[0]].cpu().numpy()

    def _to_device(self, raw_audio_list):
        flat, offsets, lengths = self.flatten(raw_audio_list)
        frames = [self.frame_count(int(n)) for n in lengths]
        return [torch.from_numpy(a).to(self.device) for a in (flat, offsets, lengths)], frames

    def _stft(self, dev, mode, out, max_frames, row_stride):
        """One launch over the (flat, offsets, lengths) device tensors of _to_device into out (B, max_frames, row_stride)."""
        flat_dev, off_dev, len_dev = dev
        st = torch.cuda.current_stream(self.device).cuda_stream
        args = (flat_dev.data_ptr(), off_dev.data_ptr(), len_dev.data_ptr(), out.data_ptr(), out.shape[0], max_frames,
                self.n_fft, self.hop, row_stride, max_frames * row_stride)
        if mode == _lib.STFT_POWER_LEVEL:
            self.lib.call("sl_stft_power_db", *args, self.min_decibel, st)
        else:
            self.lib.call("sl_stft", *args, mode, self.min_decibel, st)

    def spectrogram_batch(self, raw_audio_list, type=SpectrogramType.power_level,
                          frequency_scale=SpectrogramFrequencyScale.linear):
        """LabeledExample.spectrogram (labeled_example.py:120-134) of a batch, time-major: (x, frames) with x float32
        (B, Tmax, F) in HBM, zero behind short utterances; F = 1 + n_fft // 2 on the linear scale, mel_frequency_count on
        the mel scale, where the extractor's filter bank is applied to whichever of the three spectrograms was asked for
        (the reference projects the power LEVEL too: labeled_example.py:128-134).  Nothing is z-normalised."""
        type, frequency_scale = SpectrogramType(type), SpectrogramFrequencyScale(frequency_scale)
        mode = _STFT_MODE.get(type, _lib.STFT_POWER_LEVEL)
        dev, frames = self._to_device(raw_audio_list)
        b, t_max = len(frames), max(frames)
        if frequency_scale == SpectrogramFrequencyScale.linear:
            x = torch.empty((b, t_max, self.bins), dtype=torch.float32, device=self.device)
            self._stft(dev, mode, x, t_max, self.bins)
            return x, frames
        if self.mel_w is None:
            raise ValueError("this extractor was built with mel_frequency_count=None: it has no mel filter bank")
        rows = _round_up(t_max, TIME_TILE)  # sl_conv1d_nt reads whole time tiles
        st = torch.cuda.current_stream(self.device).cuda_stream
        linear = torch.empty((b, rows, self.bins_pad), dtype=torch.float32, device=self.device)
        self._stft(dev, mode, linear, rows, self.bins_pad)
        mel = torch.empty((b, rows, self.mel_pad), dtype=torch.float32, device=self.device)
        self._mel_project(linear, mel, t_max, st)
        return mel[:, :t_max, :self.n_mels].contiguous(), frames

    def stft_batch(self, raw_audio_list):
        """librosa.stft of a batch, time-major: (spec, frames) with spec complex64 (B, Tmax, 1 + n_fft // 2) in HBM, zero
        behind short utterances."""
        dev, frames = self._to_device(raw_audio_list)
        b, t_max = len(frames), max(frames)
        x = torch.empty((b, t_max, self.bins, 2), dtype=torch.float32, device=self.device)
        self._stft(dev, _lib.STFT_COMPLEX, x, t_max, 2 * self.bins)
        return torch.view_as_complex(x), frames

    def istft_batch(self, spec, frames, flat=False):
        """librosa.istft (hop_length, win_length = n_fft) of spec complex64 (B, Tmax, 1 + n_fft // 2) in HBM, utterance b
        over its first frames[b] rows.  Returns a list of float32 device tensors of hop * (frames[b] - 1) samples, or with
        flat=True (flat, offsets, lengths): the utterances back to back in one float32 device tensor, int64 start
        offsets and int32 sample counts on the host -- the layout of flatten()."""
        if spec.dtype != torch.complex64 or spec.dim() != 3 or spec.shape[2] != self.bins or len(frames) != spec.shape[0]:
            raise ValueError("spec must be complex64 (B, Tmax, {}) with one frame count per utterance".format(self.bins))
        frames = [int(n) for n in frames]
        if min(frames) < 1 or max(frames) > spec.shape[1]:
            raise ValueError("frame counts must lie in [1, {}]".format(spec.shape[1]))
        spec = spec.to(self.device).contiguous()
        rows = torch.view_as_real(spec)
        lengths = np.array([self.hop * (n - 1) for n in frames], dtype=np.int32)
        offsets = np.zeros(len(frames), dtype=np.int64)
        offsets[1:] = np.cumsum(lengths[:-1])
        out = torch.empty((max(int(lengths.sum()), 1),), dtype=torch.float32, device=self.device)  # (every sample is written)
        frames_dev = torch.tensor(frames, dtype=torch.int32, device=self.device)
        off_dev = torch.from_numpy(offsets).to(self.device)
        self.lib.call("sl_istft", rows.data_ptr(), frames_dev.data_ptr(), out.data_ptr(), off_dev.data_ptr(), len(frames),
                      spec.shape[1], self.n_fft, self.hop, 2 * self.bins, spec.shape[1] * 2 * self.bins,
                      torch.cuda.current_stream(self.device).cuda_stream)
        out = out[:int(lengths.sum())]
        if flat:
            return out, offsets, lengths
        return [out[o:o + n] for o, n in zip(offsets, lengths)]


_EXTRACTORS = {}


def shared_extractor(sample_rate, fourier_window_length, hop_length, mel_frequency_count, device="cuda:0"):
    key = (sample_rate, fourier_window_length, hop_length, mel_frequency_count, str(device))
    if key not in _EXTRACTORS:
        _EXTRACTORS[key] = SpectrogramExtractor(sample_rate, fourier_window_length, hop_length, mel_frequency_count,
                                                device=device)
    return _EXTRACTORS[key]


class LabeledExample:
    """Duck type of speechless.labeled_example.LabeledExample (labeled_example.py:74-140) whose spectrogram is computed
    on the GPU: same constructor arguments (the ones the net needs), `.id`, `.label`,
    `.z_normalized_transposed_spectrogram()` -> float32 ndarray (frames, mel_frequency_count)."""

    def __init__(self, get_raw_audio, sample_rate=16000, id=None, label="nolabel", fourier_window_length=512,
                 hop_length=128, mel_frequency_count=128, label_with_tags=None, positional_label=None, device="cuda:0"):
        self.get_raw_audio = get_raw_audio
        self.sample_rate = sample_rate
        self.id = id
        self.label = label
        self.fourier_window_length = fourier_window_length
        self.hop_length = hop_length
        self.mel_frequency_count = mel_frequency_count
        self.label_with_tags = label_with_tags
        self.positional_label = positional_label
        self._device = device

    def _extractor(self):
        return shared_extractor(self.sample_rate, self.fourier_window_length, self.hop_length, self.mel_frequency_count,
                                self._device)

    def z_normalized_transposed_spectrogram(self):
        return self._extractor().one(self.get_raw_audio())

    def spectrogram(self, type=SpectrogramType.power_level, frequency_scale=SpectrogramFrequencyScale.linear):
        """float32 ndarray (frequencies, frames): labeled_example.py:120-134."""
        x, _ = self._extractor().spectrogram_batch([self.get_raw_audio()], type, frequency_scale)
        return x[0].cpu().numpy().T

    def reconstructed_audio_from_spectrogram(self):
        """librosa.istft of the complex spectrogram (labeled_example.py:162-164): hop_length * (len // hop_length) samples."""
        extractor = self._extractor()
        spec, frames = extractor.stft_batch([self.get_raw_audio()])
        return extractor.istft_batch(spec, frames)[0].cpu().numpy()

    def tag_count(self, tag):
        return self.label_with_tags.count(tag)

    def mel_frequencies(self):
        """The mel_frequency_count + 2 band edges of the filter bank in Hz: librosa.mel_frequencies(n + 2, fmax=sr / 2)."""
        return _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(self.sample_rate / 2), self.mel_frequency_count + 2))

    def highest_detectable_frequency(self):
        return self.sample_rate / 2

    def frequency_count_from_spectrogram(self, spectrogram):
        return spectrogram.shape[0]

    def time_step_count(self):
        """The frame count of spectrogram(): 1 + samples // hop_length (no launch is needed to know it)."""
        return 1 + len(self.get_raw_audio()) // self.hop_length

    def time_step_rate(self):
        return self.time_step_count() / self.duration_in_s

    @property
    def duration_in_s(self):
        return len(self.get_raw_audio()) / self.sample_rate

    def __str__(self):
        return str(self.id) + (": {}".format(self.label) if self.label else "")


class LabeledExampleFromFile(LabeledExample):
    """Duck type of speechless.labeled_example.LabeledExampleFromFile (labeled_example.py:174-233) for WAV files: the file is
    parsed by speechless_amd.audio and brought to `sample_rate_to_convert_to` on the GPU (speechless_amd.resample), where the
    reference calls librosa.load(file, sr=...).  `get_original_audio()` is the extension the staged input pipeline uses: the
    samples at the file's own rate, to be converted in HBM together with the rest of their batch."""

    def __init__(self, audio_file, id=None, sample_rate_to_convert_to=16000, label="nolabel", fourier_window_length=512,
                 hop_length=128, mel_frequency_count=128, label_with_tags=None, positional_label=None, device="cuda:0"):
        self.audio_file = Path(audio_file)
        super().__init__(self._converted_audio, sample_rate=sample_rate_to_convert_to,
                         id=self.audio_file.stem if id is None else id, label=label,
                         fourier_window_length=fourier_window_length, hop_length=hop_length,
                         mel_frequency_count=mel_frequency_count, label_with_tags=label_with_tags,
                         positional_label=positional_label, device=device)
        self._original_sample_rate = None
        self._duration_in_s = None

    def get_original_audio(self):
        """(float32 mono samples, the file's sample rate)"""
        from .audio import read_wav
        return read_wav(self.audio_file)

    def _converted_audio(self):
        from .resample import resample
        samples, rate = self.get_original_audio()
        return resample(samples, rate, self.sample_rate, device=self._device)

    @property
    def audio_directory(self):
        return Path(self.audio_file.parent)

    @property
    def original_sample_rate(self):
        if self._original_sample_rate is None:
            self._original_sample_rate = LabeledExampleFromFile.file_sample_rate(self.audio_file)
        return self._original_sample_rate

    @staticmethod
    def file_sample_rate(audio_file):
        from .audio import wav_sample_rate
        return wav_sample_rate(audio_file)

    @property
    def duration_in_s(self):
        """From the header, without decoding; 0 for a file that cannot be read (labeled_example.py:211-217)."""
        if self._duration_in_s is None:
            from .audio import wav_duration_in_s
            try:
                self._duration_in_s = wav_duration_in_s(self.audio_file)
            except (OSError, ValueError) as e:
                logging.getLogger("speechless_amd").info("Failed to get duration of {}: {}".format(self.audio_file, e))
                self._duration_in_s = 0
        return self._duration_in_s

    def sections(self):
        """One LabeledExample per word timing of `positional_label` (seconds), cut from the converted audio; None without one."""
        if self.positional_label is None:
            return None
        audio = self.get_raw_audio()
        rate = self.sample_rate
        return [LabeledExample(lambda a=audio[int(start * rate):int(end * rate)]: a, sample_rate=rate, label=word,
                               fourier_window_length=self.fourier_window_length, hop_length=self.hop_length,
                               mel_frequency_count=self.mel_frequency_count, device=self._device)
                for word, (start, end) in self.positional_label.labeled_sections]
