"""Shared by tests/test_audio_frontend_{cpu,gpu}.py: the float64 direct-form oracle of the audio front end's resampler (written from
the rule in include/fdm_hip.h, no scipy), the same sum evaluated in numpy float32 (the yardstick of the GPU bound), inputs and the
converted / downmixed float32 waveform.  tests/test_audio_frontend_cpu.py pins the oracle to scipy.signal.resample_poly at 1e-14."""
import functools
from math import gcd

import numpy as np

SR = 16000
CPU_RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000, 96000)
GPU_RATES = (48000, 44100, 22050, 11025, 8000, 24000, 96000)
TILE = 256            # csrc/audio_front.hpp FRONT_TILE: outputs per workgroup


def ratio(rate):
    g = gcd(int(rate), SR)
    return SR // g, int(rate) // g


def out_len(rate, frames):
    up, down = ratio(rate)
    return -(-(int(frames) * up) // down)


@functools.lru_cache(maxsize=None)
def taps64(up, down):
    """firwin(2 half + 1, 1 / m, window = ('kaiser', 5.0)) * up restated: sinc low-pass at 1 / m times the Kaiser window, unit DC gain."""
    m = max(up, down)
    half = 10 * m
    k = np.arange(2 * half + 1, dtype=np.float64) - half
    h = (1.0 / m) * np.sinc(k / m) * np.i0(5.0 * np.sqrt(np.maximum(0.0, 1.0 - (k / half) ** 2))) / np.i0(5.0)
    return h / h.sum() * up


def _direct(x, h, up, down, n_out, dtype):
    half = (len(h) - 1) // 2
    y = np.zeros(n_out, dtype=dtype)
    n = len(x)
    for j in range(n_out):
        c = j * down
        lo = max(-((half - c) // up), 0)             # ceil((c - half) / up)
        hi = min((c + half) // up, n - 1)
        if lo <= hi:
            i = np.arange(lo, hi + 1)
            y[j] = np.dot(x[lo:hi + 1], h[half + c - i * up])
    return y


def resample64(x, rate):
    """y[j] = sum_i x[i] h[half + j down - i up], zero padding outside the clip, everything in float64."""
    up, down = ratio(rate)
    x = np.asarray(x, dtype=np.float64)
    if up == down:
        return x.copy()
    return _direct(x, taps64(up, down), up, down, out_len(rate, len(x)), np.float64)


def resample32(x, rate):
    """The same sum with float32 taps and float32 input, np.dot per output in float32."""
    up, down = ratio(rate)
    x = np.asarray(x, dtype=np.float32)
    if up == down:
        return x.copy()
    return _direct(x, taps64(up, down).astype(np.float32), up, down, out_len(rate, len(x)), np.float32)


def lengths_for(rate, about=2000, tile=None):
    """Input lengths: 1, 2, down - 1, down, down + 1 frames, (with tile) the frames that give tile - 1, tile, tile + 1 outputs, and
    one that gives about `about` outputs."""
    up, down = ratio(rate)
    ns = {1, 2, max(down - 1, 1), down, down + 1}
    if tile:
        for n_out in (tile - 1, tile, tile + 1):      # (an upsampling ratio cannot give every count: the nearest on both sides)
            ns.update({max((n_out * down) // up, 1), -(-(n_out * down) // up)})
    ns.add(max((about * down) // up + 3, 1))
    return sorted(ns)


def noise(n, channels=1, seed=0):
    """N(0, 0.1) + 0.03 from a seeded CPU generator, float32 [n] or [n, channels]."""
    import torch
    g = torch.Generator().manual_seed(seed)
    shape = (n,) if channels == 1 else (n, channels)
    return (torch.randn(shape, generator=g) * 0.1 + 0.03).numpy().astype(np.float32)


def as_format(x, dtype):
    """float32 samples in [-1, 1) -> raw PCM of `dtype` (int16 / int32 / uint8 / float32) carrying about the same signal."""
    if dtype == np.float32:
        return x.astype(np.float32)
    if dtype == np.uint8:
        return np.clip(np.round(x * 128.0 + 128.0), 0, 255).astype(np.uint8)
    bits = np.iinfo(dtype).bits
    return np.clip(np.round(x.astype(np.float64) * 2.0 ** (bits - 1)), -2.0 ** (bits - 1), 2.0 ** (bits - 1) - 1).astype(dtype)


def mono32(pcm):
    """Items 1 and 2 of the rule as a float32 expression: convert, then ((c0 + c1) + c2 ...) / C."""
    pcm = np.asarray(pcm)
    if pcm.dtype == np.uint8:
        x = (pcm.astype(np.float32) - np.float32(128.0)) / np.float32(128.0)
    elif pcm.dtype.kind == "i":
        x = pcm.astype(np.float32) / np.float32(2.0 ** (np.iinfo(pcm.dtype).bits - 1))
    else:
        x = pcm.astype(np.float32)
    if x.ndim == 1:
        return x
    s = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        s = s + x[:, c]
    return (s / np.float32(x.shape[1])).astype(np.float32)


def normalize64(y, pad=0):
    """(y - mean) / sqrt(var + 1e-7) over the clip in float64, then `pad` zeros."""
    y = np.asarray(y, dtype=np.float64)
    out = (y - y.mean()) / np.sqrt(y.var() + 1e-7)
    return np.concatenate([out, np.zeros(pad)])


def ulp32(v):
    """One float32 unit in the last place of |v|."""
    return float(np.spacing(np.float32(abs(float(v)))))
