"""No GPU: the host side of the audio front end (include/fdm_hip.h, fdm_frontend_* and fdm_resample_*_host) -- the tap table against
scipy's firwin, lengths and ratios in 64 bits, the float64 oracle the GPU tests use against scipy.signal.resample_poly, and every
refusal that is decided before a launch."""
import ctypes as C

import numpy as np
import pytest

import audio_front_cases as AC
from fdm_amd import _lib, ops

ARG, SHAPE = -1, -2


def test_symbols_and_struct_are_bound():
    l = _lib.lib()
    for name in ("fdm_frontend_create", "fdm_frontend_samples", "fdm_frontend_forward", "fdm_frontend_destroy",
                 "fdm_resample_ratio_host", "fdm_resample_len_host", "fdm_resample_taps_host"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_abi_struct_size(b"fdm_pcm") == C.sizeof(_lib.Pcm) == 32
    assert _lib.STRUCTS["fdm_pcm"] is _lib.Pcm
    assert l.fdm_version() == 105
    assert (_lib.PCM_S16, _lib.PCM_S32, _lib.PCM_U8, _lib.PCM_F32) == (0, 1, 2, 3)


@pytest.mark.parametrize("up,down", [(1, 3), (160, 441), (2, 1), (320, 441), (640, 441), (1, 6), (2, 3)])
def test_taps_against_scipy_firwin(up, down):
    """Bound 1e-13 absolute: an independent double restatement agrees to 8e-16 and the taps are at most about up / m <= 1."""
    sig = pytest.importorskip("scipy.signal")
    m = max(up, down)
    want = sig.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    got = ops.resample_taps(up, down)
    assert got.shape == want.shape == (20 * m + 1,)
    err = float(np.abs(got - want).max())
    print(f"taps {up}/{down}: max |lib - firwin| = {err:.2e}, max |tap| = {np.abs(want).max():.3f}")
    assert err <= 1e-13
    assert float(np.abs(AC.taps64(up, down) - want).max()) <= 1e-13         # the oracle's own restatement


def test_ratios_and_lengths_in_64_bits():
    for rate in AC.CPU_RATES + (16000, 12000, 16000 * 2048, 125):          # (125 Hz: 128 / 1)
        up, down = AC.ratio(rate)
        assert ops.resample_ratio(rate) == (up, down)
        near = (2 ** 31) // down
        for frames in (1, 2, down - 1, down, down + 1, 1000, near - 1, near, near + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 40 + 12345):
            if frames < 1:
                continue
            assert ops.resample_len(rate, frames) == -(-(frames * up) // down), (rate, frames)
    l = _lib.lib()
    up, down = C.c_int(0), C.c_int(0)
    assert l.fdm_resample_ratio_host(0, C.byref(up), C.byref(down)) == ARG
    assert l.fdm_resample_ratio_host(-5, C.byref(up), C.byref(down)) == ARG
    assert l.fdm_resample_ratio_host(48000, None, C.byref(down)) == ARG
    assert l.fdm_resample_ratio_host(16000 * 2048, C.byref(up), C.byref(down)) == 0 and (up.value, down.value) == (1, 2048)
    assert l.fdm_resample_ratio_host(16000 * 2049, C.byref(up), C.byref(down)) == SHAPE and b"2048" in l.fdm_last_error()
    assert l.fdm_resample_ratio_host(16001, C.byref(up), C.byref(down)) == SHAPE            # 16000 / 16001
    assert l.fdm_resample_len_host(48000, 0) == SHAPE and l.fdm_resample_len_host(0, 10) == ARG
    assert l.fdm_resample_len_host(16001, 10) == SHAPE
    assert l.fdm_resample_taps_host(0, 1, None) == ARG and l.fdm_resample_taps_host(1, 3, None) == ARG
    buf = (C.c_double * 8)()
    assert l.fdm_resample_taps_host(1, 2049, buf) == SHAPE


@pytest.mark.parametrize("rate", AC.CPU_RATES)
def test_oracle_is_resample_poly_in_float64(rate):
    """The direct form of tests/audio_front_cases.py against scipy.signal.resample_poly on float64 input.  Bound 1e-14 (measured
    agreement 3e-16): this pins the oracle the GPU tests use, which therefore need no scipy."""
    sig = pytest.importorskip("scipy.signal")
    up, down = AC.ratio(rate)
    worst = 0.0
    for n in sorted({1, 2, max(down - 1, 1), down, down + 1, 1000, (2000 * down) // up + 3}):
        x = AC.noise(n, seed=n % 1000).astype(np.float64)
        want = sig.resample_poly(x, up, down)
        got = AC.resample64(x, rate)
        assert got.shape == want.shape == (AC.out_len(rate, n),), (rate, n)
        worst = max(worst, float(np.abs(got - want).max()))
    print(f"{rate} Hz: max |oracle - resample_poly| = {worst:.2e}")
    assert worst <= 1e-14


def test_float32_expression_of_convert_and_downmix_is_load_wav():
    """mono32 (what the GPU format tests compare with) is load_wav's arithmetic: astype / scale, then x.mean(axis=1), bit for bit.
    Up to 7 channels: numpy adds 8 values in pairs, the rule's sum is sequential (8 channels differ from load_wav in the last bit)."""
    for dtype in (np.int16, np.int32, np.uint8, np.float32):
        for ch in (1, 2, 3, 5, 7):
            pcm = AC.as_format(AC.noise(501, ch, seed=ch), dtype)
            if dtype == np.float32:
                x = pcm
            elif dtype == np.uint8:
                x = (pcm.astype(np.float32) - 128.0) / 128.0
            else:
                x = pcm.astype(np.float32) / float(np.iinfo(dtype).max + 1)
            x = x.astype(np.float32)
            want = x.mean(axis=1) if x.ndim > 1 else x
            assert want.dtype == np.float32 and np.array_equal(AC.mono32(pcm), want), (dtype, ch)


def _pcm(data=16, fmt=0, ch=1, rate=48000, frames=100):
    return _lib.Pcm(data, fmt, ch, rate, frames)


def test_frontend_samples():
    l = _lib.lib()
    n = C.c_longlong(-1)
    for rate, frames, pad in ((48000, 100, 0), (44100, 441, 16000), (16000, 5, 3), (8000, 7, 0), (44100, 2 ** 31 // 441 + 1, 16000)):
        assert l.fdm_frontend_samples(C.byref(_pcm(None, rate=rate, frames=frames)), pad, C.byref(n)) == 0
        assert n.value == AC.out_len(rate, frames) + pad
    assert l.fdm_frontend_samples(None, 0, C.byref(n)) == ARG
    assert l.fdm_frontend_samples(C.byref(_pcm()), 0, None) == ARG
    assert l.fdm_frontend_samples(C.byref(_pcm()), -1, C.byref(n)) == ARG
    assert l.fdm_frontend_samples(C.byref(_pcm(frames=0)), 0, C.byref(n)) == SHAPE
    assert l.fdm_frontend_samples(C.byref(_pcm(rate=0)), 0, C.byref(n)) == ARG
    assert l.fdm_frontend_samples(C.byref(_pcm(rate=16001)), 0, C.byref(n)) == SHAPE


def test_frontend_create_validation():
    l = _lib.lib()
    h = C.c_void_p()
    rates = (C.c_int * 3)(48000, 44100, 48000)
    assert l.fdm_frontend_create(rates, 3, None) == ARG
    assert l.fdm_frontend_create(None, 3, C.byref(h)) == ARG
    assert l.fdm_frontend_create(rates, -1, C.byref(h)) == ARG
    assert l.fdm_frontend_create((C.c_int * 2)(48000, 0), 2, C.byref(h)) == ARG
    assert l.fdm_frontend_create((C.c_int * 2)(48000, 16001), 2, C.byref(h)) == SHAPE and b"2048" in l.fdm_last_error()
    assert l.fdm_frontend_destroy(None) == 0


def test_frontend_forward_validation_precedes_any_launch():
    """Every refusal is decided before a launch (the data pointers below are never dereferenced).  The object itself needs no device:
    its tables are host work; a call that passes every check on a machine without a GPU ends in FDM_ERR_STATE, never in a fallback."""
    l = _lib.lib()
    h = C.c_void_p()
    assert l.fdm_frontend_create((C.c_int * 2)(48000, 44100), 2, C.byref(h)) == 0
    try:
        ns = (C.c_int * 4)()
        wav = 4096            # (a non-null output pointer: no call below gets as far as a launch)

        def fwd(clips, B=None, pad=0, n_max=100000, w=wav, n=ns, f=h):
            arr = (_lib.Pcm * max(len(clips), 1))(*clips)
            return l.fdm_frontend_forward(f, arr if clips else None, len(clips) if B is None else B, pad, 1, w, n_max, n, None)
        ok = _pcm()
        assert fwd([ok], f=None) == ARG and fwd([], B=1) == ARG and fwd([ok], w=None) == ARG and fwd([ok], n=None) == ARG
        assert fwd([_pcm(data=None)]) == ARG
        assert fwd([_pcm(fmt=4)]) == ARG and fwd([_pcm(fmt=-1)]) == ARG and b"format" in l.fdm_last_error()
        assert fwd([_pcm(rate=22050)]) == ARG and b"22050" in l.fdm_last_error()
        assert fwd([_pcm(rate=0)]) == ARG
        assert fwd([_pcm(ch=0)]) == ARG and fwd([_pcm(ch=9)]) == ARG and b"channels" in l.fdm_last_error()
        assert fwd([ok], pad=-1) == ARG
        assert fwd([_pcm(data=17)]) == ARG and fwd([_pcm(data=18, fmt=1)]) == ARG and b"aligned" in l.fdm_last_error()
        assert fwd([ok], B=0) == SHAPE and fwd([ok], B=-2) == SHAPE
        assert fwd([_pcm(frames=0)]) == SHAPE
        assert fwd([ok, _pcm(frames=30001)], n_max=10000) == SHAPE and b"clip 1" in l.fdm_last_error()      # 10001 samples
        assert fwd([_pcm(frames=30000)], pad=1, n_max=10000) == SHAPE                                        # the padding counts
        assert fwd([_pcm(rate=16000 * 4096)]) == ARG                     # not created for it (and over the ratio cap)
        assert list(ns) == [0, 0, 0, 0]                                  # a refused call writes no length
        if not l.fdm_device_ok():            # (with a device this call would launch on pointers that are not memory)
            assert fwd([ok, _pcm(rate=16000, fmt=3, ch=8), _pcm(rate=44100, fmt=2, data=17)]) == -4      # every check passed: no device
            assert b"no CPU fallback" in l.fdm_last_error()
    finally:
        assert l.fdm_frontend_destroy(h) == 0


def test_prepare_audio_refuses_cpu_tensors():
    import torch
    from fdm_amd import pipeline
    from fdm_amd.hubert import FrontendPlan
    with pytest.raises(_lib.FdmError):
        pipeline.prepare_audio(torch.zeros(100, dtype=torch.int16), 48000)
    with pytest.raises(_lib.FdmError):
        pipeline.prepare_audio_many([np.zeros(100, dtype=np.int16)], [48000], device="cpu")
    with pytest.raises(_lib.FdmError):
        FrontendPlan([48000], device="cpu")
    with pytest.raises(_lib.FdmError):
        ops.pcm_desc(torch.zeros(10, dtype=torch.int16), 48000)


@pytest.mark.parametrize("dtype,channels,rate", [(np.int16, 2, 44100), (np.int32, 1, 48000), (np.uint8, 1, 8000), (np.float32, 3, 22050)])
def test_load_pcm_returns_the_file_as_stored(tmp_path, dtype, channels, rate):
    wavfile = pytest.importorskip("scipy.io.wavfile")
    from fdm_amd import pipeline
    pcm = AC.as_format(AC.noise(321, channels, seed=channels), dtype)
    path = str(tmp_path / "clip.wav")
    wavfile.write(path, rate, pcm)
    got, r = pipeline.load_pcm(path)
    assert r == rate and isinstance(r, int) and got.dtype == pcm.dtype and got.shape == pcm.shape and np.array_equal(got, pcm)
    wavfile.write(path, rate, pcm.astype(np.float64) if dtype == np.float32 else pcm.astype(np.int64))
    if dtype == np.float32:
        with pytest.raises(ValueError):
            pipeline.load_pcm(path)              # float64 samples: not a format of the front end
