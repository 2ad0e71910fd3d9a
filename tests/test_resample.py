"""The resampler's definition ("Resampling") on the CPU: the two-wing loop against the polyphase form, the
product's fp32 bank against the float64 restatement, and properties of the filter that guard the restatement itself."""
import numpy as np
import pytest

import resample_ref as rr
from speechless_amd.resample import kaiser_best_window, output_length, polyphase_bank, rate_ratio, resample

_BANKS = {}


def ref_bank(pair):
    if pair not in _BANKS:
        _BANKS[pair] = rr.bank(*pair)
    return _BANKS[pair]


@pytest.mark.parametrize("pair", rr.RATE_PAIRS)
def test_direct_loop_equals_the_polyphase_form(pair):
    p, q = rate_ratio(*pair)
    h, left, right = ref_bank(pair)
    assert h.shape == rr.BANK_SHAPES[pair]
    rng = np.random.RandomState(11)
    for n_in in (37, 1000, 4411):
        x = rng.uniform(-1, 1, size=n_in)
        want = rr.direct(x, *pair)
        got, _ = rr.fir(x, h, left, p, q)
        assert got.shape == want.shape
        err = np.abs(got - want).max()
        print(pair, n_in, "direct vs fir", err)
        assert err <= 1e-14


@pytest.mark.parametrize("pair", rr.RATE_PAIRS)
def test_product_bank_is_the_restatement_rounded_to_fp32(pair):
    h64, left, right = ref_bank(pair)
    h, l, r = polyphase_bank(*pair)
    assert h.dtype == np.float32 and (l, r) == (left, right)
    assert np.array_equal(h.view(np.uint32), h64.astype(np.float32).view(np.uint32))
    # one rounding per coefficient: at most 2^-24 * mag[t] per output
    p, q = rate_ratio(*pair)
    x = np.random.RandomState(12).uniform(-1, 1, size=4411)
    exact, mag = rr.fir(x, h64, left, p, q)
    rounded, _ = rr.fir(x, h, left, p, q)
    ratio = (np.abs(rounded - exact)[mag > 0] / (2.0 ** -24 * mag[mag > 0])).max()
    print(pair, "bank rounding / bound", ratio)
    assert ratio <= 1.0


def test_window_is_the_definition():
    assert np.array_equal(kaiser_best_window(), rr.half_window())
    assert len(kaiser_best_window()) == 32769


def tone(freq, rate, n):
    return 0.5 * np.sin(2 * np.pi * freq * np.arange(n) / rate)


@pytest.mark.parametrize("sr_orig", [48000, 44100])
def test_downsampling_keeps_the_pass_band_and_removes_what_would_alias(sr_orig):
    pair = (sr_orig, 16000)
    p, q = rate_ratio(*pair)
    h, left, _ = ref_bank(pair)
    n_in = sr_orig // 4
    for freq in (1000.0, 3500.0, 7000.0):
        y, _ = rr.fir(tone(freq, sr_orig, n_in), h, left, p, q)
        err = np.abs(y - tone(freq, 16000, len(y)))[400:-400].max()
        print(pair, freq, err)
        assert err <= 3e-3
    y, _ = rr.fir(tone(12000.0, sr_orig, n_in), h, left, p, q)
    leak = np.abs(y)[400:-400].max()
    print(pair, 12000.0, leak)
    assert leak < 2e-4


def test_upsampling_interpolates_tones():
    pair = (8000, 16000)
    p, q = rate_ratio(*pair)
    h, left, _ = ref_bank(pair)
    for freq in (1000.0, 3500.0):
        y, _ = rr.fir(tone(freq, 8000, 2000), h, left, p, q)
        err = np.abs(y - tone(freq, 16000, len(y)))[400:-400].max()
        print(freq, err)
        assert err <= 1e-6


@pytest.mark.parametrize("pair", rr.RATE_PAIRS)
def test_output_length_and_zero_tail(pair):
    p, q = rate_ratio(*pair)
    h, left, _ = ref_bank(pair)
    for n_in in (p * 7, p * 7 + 1, p * 7 + p - 1, 1):
        n_out, n_res = rr.lengths(n_in, p, q)
        assert n_out == -(-n_in * q // p) == output_length(n_in, p, q)
        y, _ = rr.fir(np.ones(n_in), h, left, p, q)
        assert len(y) == n_out and n_out - n_res == (0 if (n_in * q) % p == 0 else 1)
        assert np.all(y[n_res:] == 0.0)
        if n_res:
            assert y[n_res - 1] != 0.0
        assert len(rr.direct(np.ones(n_in), *pair)) == n_out


def test_equal_rates_return_the_input_itself():
    a = np.arange(5, dtype=np.float32)
    assert resample(a, 16000, 16000) is a
    with pytest.raises(ValueError):
        polyphase_bank(16000, 16000)
