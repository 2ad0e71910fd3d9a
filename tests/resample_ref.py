"""Float64 restatement of the resampler's definition ("Resampling"), independent of speechless_amd/resample.py.

direct()  the two-wing loop of the definition, one output sample at a time
bank()    the same weights as a polyphase bank in float64
fir()     y[t] = sum_j h[r][j] x[n - (L - 1) + j] in float64 over any bank, and mag[t] = sum_j |h[r][j]| |x[..]|
"""
from math import gcd

import numpy as np

N = 64 * 512
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596

RATE_PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (32000, 16000), (16000, 8000)]
BANK_SHAPES = {(48000, 16000): (1, 383), (44100, 16000): (160, 354), (22050, 16000): (320, 176), (11025, 16000): (640, 128),
               (8000, 16000): (2, 127), (32000, 16000): (1, 255), (16000, 8000): (1, 255)}


def half_window():
    j = np.arange(N + 1, dtype=np.float64)
    return np.kaiser(2 * N + 1, BETA)[N:] * ROLLOFF * np.sinc(ROLLOFF * j / 512)


def setup(sr_orig, sr_new):
    g = gcd(sr_orig, sr_new)
    p, q = sr_orig // g, sr_new // g
    scale = min(1.0, q / p)
    w = scale * half_window()
    delta = np.zeros(N + 1)
    delta[:N] = w[1:] - w[:N]
    index_step = (512 * q) // p if q < p else 512
    d = p if q < p else q
    return p, q, w, delta, index_step, d


def lengths(n_in, p, q):
    """(n_out, n_res)"""
    return -((-n_in * q) // p), (n_in * q) // p


def direct(x, sr_orig, sr_new):
    x = np.asarray(x, dtype=np.float64)
    n_in = len(x)
    p, q, w, delta, index_step, d = setup(sr_orig, sr_new)
    n_out, n_res = lengths(n_in, p, q)
    y = np.zeros(n_out)
    for t in range(n_res):
        n, r = divmod(t * p, q)
        acc = 0.0
        off, rem = divmod(512 * r, d)
        for i in range((N + 1 - off) // index_step):
            if 0 <= n - i < n_in:
                k = off + i * index_step
                acc += (w[k] + (rem / d) * delta[k]) * x[n - i]
        off, rem = divmod(512 * (q - r), d)
        for k_ in range((N + 1 - off) // index_step):
            if 0 <= n + 1 + k_ < n_in:
                k = off + k_ * index_step
                acc += (w[k] + (rem / d) * delta[k]) * x[n + 1 + k_]
        y[t] = acc
    return y


def bank(sr_orig, sr_new):
    """(h float64 (Q, L + R), L, R)"""
    p, q, w, delta, index_step, d = setup(sr_orig, sr_new)
    rows = []
    for r in range(q):
        wings = []
        for num in (512 * r, 512 * (q - r)):
            off, rem = divmod(num, d)
            wings.append([w[off + i * index_step] + (rem / d) * delta[off + i * index_step]
                          for i in range((N + 1 - off) // index_step)])
        rows.append(wings)
    left = max(len(a) for a, _ in rows)
    right = max(len(b) for _, b in rows)
    h = np.zeros((q, left + right))
    for r, (a, b) in enumerate(rows):
        for i, v in enumerate(a):
            h[r, left - 1 - i] = v
        for k, v in enumerate(b):
            h[r, left + k] = v
    return h, left, right


def fir(x, h, left, p, q):
    """(y, mag) in float64; h may be the float64 bank or the fp32 one"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n_in, width = len(x), h.shape[1]
    n_out, n_res = lengths(n_in, p, q)
    xp = np.concatenate([np.zeros(width), x, np.zeros(width + 1)])
    y, mag = np.zeros(n_out), np.zeros(n_out)
    t = np.arange(n_res, dtype=np.int64)
    n, r = (t * p) // q, (t * p) % q
    start = n - (left - 1) + width  # index into xp of tap 0
    for phase in range(q):
        sel = np.nonzero(r == phase)[0]
        if sel.size == 0:
            continue
        win = xp[start[sel][:, None] + np.arange(width)[None, :]]
        y[sel] = win @ h[phase]
        mag[sel] = np.abs(win) @ np.abs(h[phase])
    return y, mag
