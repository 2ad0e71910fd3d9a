"""Sample-rate conversion on the MI355X ("Resampling"): what `librosa.load(file, sr=16000)` does on the host for
the reference (speechless/labeled_example.py:193), as one launch of `sl_resample_polyphase` over a ragged batch in HBM.

The filter is resampy's `kaiser_best` as `librosa.resample` applies it, restated exactly: a Kaiser-windowed sinc sampled at
512 points per zero crossing, read with linear interpolation at a position that advances by sr_orig / sr_new per output.  The
position is kept as an exact rational here (resampy accumulates it in a float64), so the weights of output t depend on t only
through r = (t P) mod Q and the whole filter is a bank of Q rows of fp32 weights: `polyphase_bank`.
"""
import threading
from math import gcd

import numpy as np
import torch

from . import _lib
from ._lib import lib

PRECISION = 512                      # samples of the window per zero crossing
ZERO_CROSSINGS = 64
ROLLOFF = 0.9475937167399596
KAISER_BETA = 14.769656459379492
TILE = _lib.SL_RESAMPLE_TILE         # consecutive outputs of one utterance per work-group
MAX_PHASES = _lib.SL_RESAMPLE_MAX_PHASES
MAX_TAPS = _lib.SL_RESAMPLE_MAX_TAPS


def kaiser_best_window():
    """The right half of the interpolation window, float64, ZERO_CROSSINGS * PRECISION + 1 entries."""
    n = ZERO_CROSSINGS * PRECISION
    taper = np.kaiser(2 * n + 1, KAISER_BETA)[n:]
    return taper * ROLLOFF * np.sinc(ROLLOFF * np.arange(n + 1, dtype=np.float64) / PRECISION)


def rate_ratio(sr_orig, sr_new):
    """(P, Q): Q / P = sr_new / sr_orig in lowest terms."""
    sr_orig, sr_new = int(sr_orig), int(sr_new)
    if sr_orig <= 0 or sr_new <= 0:
        raise ValueError("sample rates must be positive, got {} -> {}".format(sr_orig, sr_new))
    g = gcd(sr_orig, sr_new)
    return sr_orig // g, sr_new // g


def output_length(n_in, p, q):
    return (int(n_in) * q + p - 1) // p


def polyphase_bank(sr_orig, sr_new):
    """(h, L, R): h float32 (Q, L + R); output t of the conversion is sum_j h[r][j] * x[n - (L - 1) + j] with
    n, r = divmod(t P, Q).  Built in float64, rounded to float32 once.  Wings shorter than the longest are zero-filled."""
    p, q = rate_ratio(sr_orig, sr_new)
    if p == q:
        raise ValueError("equal rates need no filter")
    n = ZERO_CROSSINGS * PRECISION
    w = min(1.0, q / p) * kaiser_best_window()
    delta = np.zeros_like(w)
    delta[:-1] = w[1:] - w[:-1]
    step = PRECISION * q // p if q < p else PRECISION
    d = p if q < p else q

    def wing(numerator):
        off, rem = divmod(PRECISION * numerator, d)
        idx = off + step * np.arange((n + 1 - off) // step)
        return w[idx] + (rem / d) * delta[idx]
    wings = [(wing(r), wing(q - r)) for r in range(q)]
    left = max(len(a) for a, _ in wings)
    right = max(len(b) for _, b in wings)
    h = np.zeros((q, left + right), dtype=np.float64)
    for r, (a, b) in enumerate(wings):
        h[r, left - len(a):left] = a[::-1]  # tap i of the left wing weighs x[n - i]
        h[r, left:left + len(b)] = b        # tap k of the right wing weighs x[n + 1 + k]
    return h.astype(np.float32), left, right


class Resampler:
    """One rate pair on one GPU; the bank stays in HBM."""

    def __init__(self, sr_orig, sr_new, device="cuda:0"):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("speechless_amd.resample needs a ROCm GPU; there is no CPU fallback")
        self.lib = lib()
        self.device = torch.device(device)
        self.sr_orig, self.sr_new = int(sr_orig), int(sr_new)
        self.p, self.q = rate_ratio(sr_orig, sr_new)
        h, self.left, right = polyphase_bank(sr_orig, sr_new)
        self.width = self.left + right
        self.bank = torch.from_numpy(h).to(self.device)
        # once per rate pair: the bank is read from whichever stream a later launch runs on
        torch.cuda.current_stream(self.device).synchronize()

    def output_length(self, n_in):
        return output_length(n_in, self.p, self.q)

    def launch(self, audio, in_off_dev, in_len_dev, out, out_off_dev, batch):
        """The bare call on the current stream: `audio` and `out` are the float32 tensors the int64 offsets count from."""
        st = torch.cuda.current_stream(self.device).cuda_stream
        self.lib.call("sl_resample_polyphase", audio.data_ptr(), in_off_dev.data_ptr(), in_len_dev.data_ptr(), out.data_ptr(),
                      out_off_dev.data_ptr(), self.bank.data_ptr(), batch, self.p, self.q, self.left, self.width, st)

    def batch_device(self, flat_dev, off_dev, len_dev, lengths, bufs=None):
        """Audio already in HBM in SpectrogramExtractor.batch_device's layout (flat float32, int64 offsets, int32 sample
        counts; `lengths` the same counts on the host) -> (flat_out, off_out, len_out, lengths_out) in that layout, the
        converted utterances back to back.  Enqueued on the CURRENT stream.  bufs: a dict the caller owns; the output tensors
        are kept there and reused, so that a steady-state call allocates nothing (see SpectrogramExtractor.batch_device)."""
        def tensor(name, n, dtype):
            if bufs is None:
                return torch.empty((n,), dtype=dtype, device=self.device)
            flat = bufs.get(name)
            if flat is None or flat.numel() < n or flat.dtype != dtype:
                flat = bufs[name] = torch.empty((n,), dtype=dtype, device=self.device)
            return flat[:n]

        lengths = np.asarray(lengths).reshape(-1)
        if lengths.size == 0 or lengths.min() < 1:
            raise ValueError("every utterance needs at least one sample")
        lengths_out = np.array([self.output_length(n) for n in lengths], dtype=np.int32)
        offsets_out = np.zeros(len(lengths), dtype=np.int64)
        offsets_out[1:] = np.cumsum(lengths_out[:-1], dtype=np.int64)
        b = len(lengths)
        flat_out = tensor("resampled", int(lengths_out.sum(dtype=np.int64)), torch.float32)
        off_out = tensor("resampled_off", b, torch.int64)
        len_out = tensor("resampled_len", b, torch.int32)
        off_out.copy_(torch.from_numpy(offsets_out))
        len_out.copy_(torch.from_numpy(lengths_out))
        self.launch(flat_dev, off_dev, len_dev, flat_out, off_out, b)
        return flat_out, off_out, len_out, lengths_out

    def one(self, audio):
        a = np.ascontiguousarray(np.asarray(audio).reshape(-1), dtype=np.float32)
        if a.shape[0] < 1:
            raise ValueError("empty audio")
        flat_dev = torch.from_numpy(a).to(self.device)
        off_dev = torch.zeros((1,), dtype=torch.int64, device=self.device)
        len_dev = torch.tensor([a.shape[0]], dtype=torch.int32, device=self.device)
        flat_out, _, _, _ = self.batch_device(flat_dev, off_dev, len_dev, [a.shape[0]])
        return flat_out.cpu().numpy()


_RESAMPLERS = {}
_RESAMPLERS_LOCK = threading.Lock()  # (the stager's worker threads ask for resamplers, too)


def shared_resampler(sr_orig, sr_new, device="cuda:0"):
    key = (int(sr_orig), int(sr_new), str(device))
    with _RESAMPLERS_LOCK:
        if key not in _RESAMPLERS:
            _RESAMPLERS[key] = Resampler(sr_orig, sr_new, device=device)
        return _RESAMPLERS[key]


def resample(audio, sr_orig, sr_new, device="cuda:0"):
    """librosa.resample(audio, sr_orig, sr_new) on the GPU; equal rates return the input itself, without a launch."""
    if int(sr_orig) == int(sr_new):
        return audio
    return shared_resampler(sr_orig, sr_new, device).one(audio)


class MixedRatePlan:
    """Host half of converting a batch whose utterances come at several rates: the converted utterances are laid out behind
    `in_total` staged samples of ONE device buffer, so that a single (offsets, lengths) pair describes the batch the front end
    reads -- utterances already at the target rate stay where the copy put them and never pass through the filter.

    offsets, lengths : int64 / int32 per utterance, what SpectrogramExtractor.batch_device takes
    total            : floats of the device buffer (staged samples + converted utterances)
    jobs             : one (rate, in_offsets, in_lengths, out_offsets) per distinct source rate to convert"""

    def __init__(self, in_offsets, in_lengths, rates, target_rate, in_total):
        in_offsets = np.asarray(in_offsets, dtype=np.int64)
        in_lengths = np.asarray(in_lengths, dtype=np.int32)
        rates = [int(r) for r in rates]
        if len(rates) != len(in_lengths):
            raise ValueError("{} sample rates for {} utterances".format(len(rates), len(in_lengths)))
        self.offsets = in_offsets.copy()
        self.lengths = in_lengths.copy()
        self.jobs = []
        cursor = int(in_total)
        for rate in sorted(set(rates) - {int(target_rate)}):
            p, q = rate_ratio(rate, target_rate)
            idx = np.array([i for i, r in enumerate(rates) if r == rate], dtype=np.int64)
            out_len = np.array([output_length(in_lengths[i], p, q) for i in idx], dtype=np.int32)
            out_off = cursor + np.concatenate([[0], np.cumsum(out_len[:-1], dtype=np.int64)]).astype(np.int64)
            cursor += int(out_len.sum(dtype=np.int64))
            self.offsets[idx] = out_off
            self.lengths[idx] = out_len
            self.jobs.append((rate, np.ascontiguousarray(in_offsets[idx]), np.ascontiguousarray(in_lengths[idx]), out_off))
        self.total = cursor
        self.target_rate = int(target_rate)

    def to_device(self, device):
        """The jobs' index arrays as device tensors (pageable H2D copies on the current stream)."""
        return [(rate, torch.from_numpy(a).to(device), torch.from_numpy(n).to(device), torch.from_numpy(o).to(device), len(n))
                for rate, a, n, o in self.jobs]

    def launch(self, jobs_dev, buffer, device):
        """One sl_resample_polyphase per distinct source rate, on the current stream, inside `buffer`."""
        for rate, in_off, in_len, out_off, count in jobs_dev:
            shared_resampler(rate, self.target_rate, device).launch(buffer, in_off, in_len, buffer, out_off, count)
