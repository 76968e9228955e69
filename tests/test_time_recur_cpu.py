"""CPU: the host side of the time filter's recurrences (include/fdm_hip.h, fdm_tfilter_recur_coeffs_host / _create_recur /
_forward_state): the constants against the float32 restatement (tests/time_recur_cases.py) exactly, every refusal, the plan's identity,
the pipeline keyword and the command-line flags, and the properties of the definition checked on the restatement.  Nothing here launches."""
import argparse
import ctypes as C

import numpy as np
import pytest

import time_recur_cases as RC
from fdm_amd import _lib, pipeline, presets, tfilter
from fdm_amd._lib import FdmError

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def test_constants_mirror_the_header():
    import os
    src = open(os.path.join(os.path.dirname(tfilter.__file__), "..", "csrc", "trecur.hpp")).read()
    for name, v in (("TR_VERTS", tfilter.RECUR_VERTS), ("TR_DEPTH", tfilter.PREFETCH_DEFAULT), ("TR_NCOEFF", _lib.TFILTER_NCOEFF)):
        assert f"constexpr int {name} = {v};" in src, name
    hdr = open(os.path.join(os.path.dirname(tfilter.__file__), "..", "..", "include", "fdm_hip.h")).read()
    for name, v in (("FDM_TFILTER_EMA", _lib.TFILTER_EMA), ("FDM_TFILTER_ONE_EURO", _lib.TFILTER_ONE_EURO), ("FDM_TFILTER_CAUSAL", _lib.TFILTER_CAUSAL),
                    ("FDM_TFILTER_ZERO_PHASE", _lib.TFILTER_ZERO_PHASE), ("FDM_TFILTER_NCOEFF", _lib.TFILTER_NCOEFF)):
        assert f"#define {name} {v}\n" in hdr, name


@pytest.mark.parametrize("fps", [30.0, 25.0, 60.0, 29.97, 1000.0, 0.5])
def test_coeffs_equal_the_restatement(fps):
    """The same IEEE operations on both sides: every bit"""
    for c in (0.05, 1.0, 1.7, 12.5, 400.0):
        assert np.array_equal(bits(tfilter.recur_coeffs("ema", fps, cutoff=c)), bits(RC.coeffs("ema", fps, cutoff=c)))
        for beta, dc in ((0.0, 1.0), (0.007, 1.0), (3.3, 0.3), (150.0, 7.0)):
            got = tfilter.recur_coeffs("one_euro", fps, min_cutoff=c, beta=beta, d_cutoff=dc)
            assert np.array_equal(bits(got), bits(RC.coeffs("one_euro", fps, min_cutoff=c, beta=beta, d_cutoff=dc))), (fps, c, beta, dc)
            assert got.dtype == F32 and got.shape == (8,) and 0 < got[5] < 1 and 0 < got[6] < 1 and got[7] == 0
    assert np.array_equal(tfilter.recur_coeffs("one_euro", fps, min_cutoff=1.0, beta=0.5), tfilter.recur_coeffs("one_euro", fps, min_cutoff=1.0, beta=0.5, d_cutoff=1.0))


def test_coeffs_refusals():
    nan, inf = float("nan"), float("inf")
    for kw in (dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=nan), dict(cutoff=inf), dict(cutoff=1e300), dict(cutoff=1e-300)):
        with pytest.raises(FdmError):
            tfilter.recur_coeffs("ema", 30.0, **kw)
    for fps in (0.0, -30.0, nan, inf, 1e300, 1e-300):
        with pytest.raises(FdmError):
            tfilter.recur_coeffs("ema", fps, cutoff=1.0)
        with pytest.raises(FdmError):
            tfilter.recur_coeffs("one_euro", fps, min_cutoff=1.0, beta=0.1)
    for kw in (dict(min_cutoff=0.0, beta=0.1), dict(min_cutoff=-2.0, beta=0.1), dict(min_cutoff=nan, beta=0.1), dict(min_cutoff=1.0, beta=-0.1),
               dict(min_cutoff=1.0, beta=nan), dict(min_cutoff=1.0, beta=inf), dict(min_cutoff=1.0, beta=1e300), dict(min_cutoff=1.0, beta=0.1, d_cutoff=0.0),
               dict(min_cutoff=1.0, beta=0.1, d_cutoff=-1.0), dict(min_cutoff=1.0, beta=0.1, d_cutoff=nan), dict(min_cutoff=1.0, beta=0.1, d_cutoff=inf)):
        with pytest.raises(FdmError):
            tfilter.recur_coeffs("one_euro", 30.0, **kw)
    # what belongs to the other kind, or is missing
    for kind, kw in (("ema", dict()), ("ema", dict(cutoff=1.0, beta=0.1)), ("ema", dict(min_cutoff=1.0)), ("one_euro", dict(min_cutoff=1.0)),
                     ("one_euro", dict(beta=0.1)), ("one_euro", dict(cutoff=1.0, min_cutoff=1.0, beta=0.1)), ("box", dict(cutoff=1.0))):
        with pytest.raises(ValueError):
            tfilter.recur_coeffs(kind, 30.0, **kw)
    with pytest.raises(ValueError):
        tfilter.recur_coeffs("ema", None, cutoff=1.0)
    L = _lib.lib()
    assert L.fdm_tfilter_recur_coeffs_host(_lib.TFILTER_EMA, 30.0, 1.0, 0.0, 1.0, None) != 0
    q = np.zeros(8, F32)
    assert L.fdm_tfilter_recur_coeffs_host(2, 30.0, 1.0, 0.0, 1.0, q.ctypes.data) != 0 and L.fdm_tfilter_recur_coeffs_host(-1, 30.0, 1.0, 0.0, 1.0, q.ctypes.data) != 0


def make(V, kind, q, strength=None, direction=_lib.TFILTER_CAUSAL):
    h = C.c_void_p()
    q = np.ascontiguousarray(q, dtype=F32)
    s = None if strength is None else np.ascontiguousarray(strength, dtype=F32)
    rc = _lib.lib().fdm_tfilter_create_recur(V, kind, None if q is None else q.ctypes.data, None if s is None else s.ctypes.data, direction, None, C.byref(h))
    return rc, h


def test_create_and_forward_refusals():
    """Every refusal of fdm_tfilter_create_recur and of fdm_tfilter_forward_state that is made before any device call"""
    L = _lib.lib()
    V, good = 5, tfilter.recur_coeffs("one_euro", 30.0, min_cutoff=1.0, beta=0.5)
    ema = tfilter.recur_coeffs("ema", 30.0, cutoff=1.0)
    h = C.c_void_p()
    assert L.fdm_tfilter_create_recur(V, 1, good.ctypes.data, None, 0, None, None) != 0
    assert L.fdm_tfilter_create_recur(V, 1, None, None, 0, None, C.byref(h)) != 0 and not h.value
    for Vbad in (0, -3):
        assert make(Vbad, 1, good)[0] != 0
    for kind in (-1, 2):
        assert make(V, kind, good)[0] != 0
    for direction in (-1, 2):
        assert make(V, 1, good, None, direction)[0] != 0
    for i, bad in ((0, 0.0), (0, -1.0), (0, np.nan), (1, 0.0), (1, -1.0), (1, np.inf), (2, -0.5), (2, np.nan), (3, 0.0), (3, -np.inf), (4, 0.0), (4, -30.0),
                   (4, np.nan), (5, 0.0), (5, np.nan), (6, 0.0), (6, np.inf), (7, np.nan)):
        q = good.copy()
        q[i] = bad
        assert make(V, 1, q)[0] != 0, (i, bad)
    q = ema.copy()
    q[2] = -1.0
    assert make(V, 0, q)[0] != 0
    assert make(V, 1, ema)[0] != 0            # one_euro needs cd and ad; ema does not
    for s in ([0, 0.5, 1, 1.0001, 0], [0, -0.1, 1, 1, 0], [0, np.nan, 1, 1, 0]):
        assert make(V, 1, good, s)[0] != 0
    rc, T = make(V, 1, good, [0, 0.5, 1, 1, 0])
    rc0, E = make(V, 0, ema)
    rcz, Z = make(V, 1, good, None, _lib.TFILTER_ZERO_PHASE)
    assert rc == 0 and rc0 == 0 and rcz == 0 and T.value and E.value and Z.value
    taps = np.array([0.5, 0.25], F32)
    F = C.c_void_p()
    assert L.fdm_tfilter_create(V, 1, taps.ctypes.data, None, 0, None, C.byref(F)) == 0
    x, y, st, seen = 0x100000, 0x200000, 0x300000, 0x400000        # never dereferenced: no call gets as far as a launch
    B, L_max = 3, 7
    lens = lambda *v: (C.c_int * B)(*v)  # noqa: E731
    fs = L.fdm_tfilter_forward_state
    assert fs(None, x, lens(7, 1, 4), B, L_max, st, seen, y) != 0
    assert fs(T, None, lens(7, 1, 4), B, L_max, st, seen, y) != 0
    assert fs(T, x, lens(7, 1, 4), B, L_max, None, seen, y) != 0
    assert fs(T, x, lens(7, 1, 4), B, L_max, st, None, y) != 0
    assert fs(T, x, lens(7, 1, 4), B, L_max, st, seen, None) != 0
    assert fs(F, x, lens(7, 1, 4), B, L_max, st, seen, y) != 0            # an FIR object
    with pytest.raises(FdmError, match="FIR"):
        _lib.check(fs(F, x, lens(7, 1, 4), B, L_max, st, seen, y))
    assert fs(Z, x, lens(7, 1, 4), B, L_max, st, seen, y) != 0            # zero-phase
    for bad in (lens(-1, 1, 4), lens(7, 1, 8)):
        assert fs(T, x, bad, B, L_max, st, seen, y) != 0
    assert fs(T, x, lens(7, 1, 4), 0, L_max, st, seen, y) != 0 and fs(T, x, None, B, 0, st, seen, y) != 0
    assert fs(T, x, lens(7, 1, 4), B, L_max, st, seen, x) != 0            # y overlaps x
    # all that is left is the device: L = 0 is a length here, and not in the stateless call
    state_err = fs(T, x, lens(7, 0, 4), B, L_max, st, seen, y)
    assert state_err != 0 and state_err == fs(E, x, None, B, L_max, st, seen, y) == L.fdm_tfilter_forward(T, x, lens(7, 1, 4), B, L_max, y)
    assert L.fdm_tfilter_forward(T, x, lens(7, 0, 4), B, L_max, y) not in (0, state_err)
    assert L.fdm_tfilter_set_prefetch(T, 4) == 0 and L.fdm_tfilter_set_prefetch(T, 3) != 0 and L.fdm_tfilter_set_prefetch(F, 4) != 0
    for o in (T, E, Z, F):
        assert L.fdm_tfilter_destroy(o) == 0


def test_plan_arguments_and_key():
    kw = dict(kind="one_euro", fps=30.0, min_cutoff=1.0, beta=0.5)
    a = tfilter.identity(5, **kw)
    assert a[:3] == (5, "one_euro", "zero_phase") and a == tfilter.identity(5, d_cutoff=1.0, direction="zero_phase", **kw)
    assert a == tfilter.identity(5, kind="one_euro", coeffs=tfilter.recur_coeffs("one_euro", 30.0, min_cutoff=1.0, beta=0.5))
    others = [tfilter.identity(6, **kw), tfilter.identity(5, **dict(kw, fps=25.0)), tfilter.identity(5, **dict(kw, min_cutoff=1.5)),
              tfilter.identity(5, **dict(kw, beta=0.25)), tfilter.identity(5, d_cutoff=2.0, **kw), tfilter.identity(5, direction="causal", **kw),
              tfilter.identity(5, strength=np.ones(5), **kw), tfilter.identity(5, strength=np.array([1, 1, 0, 1, 1.0]), **kw),
              tfilter.identity(5, kind="ema", fps=30.0, cutoff=1.0), tfilter.identity(5, kind="ema", fps=30.0, cutoff=2.0),
              tfilter.identity(5, kind="ema", fps=30.0, cutoff=1.0, direction="causal"), tfilter.identity(5, kind="gaussian", sigma=1.5)]
    assert len(set(others + [a])) == len(others) + 1
    for bad in (dict(kw, direction="both"), dict(kw, sigma=1.0), dict(kw, radius=3), dict(kw, edge="nearest"), dict(kw, taps=[1.0]), dict(kw, cutoff=1.0),
                dict(kind="one_euro", min_cutoff=1.0, beta=0.5), dict(kind="ema", fps=30.0), dict(kind="gaussian", sigma=1.0, fps=30.0),
                dict(kind="gaussian", sigma=1.0, direction="causal"), dict(kind="savgol", radius=3, order=2, cutoff=1.0)):
        with pytest.raises(ValueError):
            tfilter.identity(5, **bad)
    with pytest.raises(FdmError):
        tfilter.identity(5, strength=np.ones(4), **kw)
    with pytest.raises(FdmError):
        tfilter.TimeFilterPlan(5, device="cpu", **kw)


def test_outputs_resolve_fps_from_the_preset():
    p = presets.get("vocaset")
    o = pipeline._Outputs(p, "cpu", time_filter=dict(kind="one_euro", min_cutoff=1.0, beta=0.5))
    assert o.time_filter == dict(kind="one_euro", min_cutoff=1.0, beta=0.5, fps=float(p.fps), direction="zero_phase")
    assert pipeline._Outputs(p, "cpu", in_fps=60, time_filter=dict(kind="ema", cutoff=2.0, direction="causal")).time_filter == dict(
        kind="ema", cutoff=2.0, fps=60.0, direction="causal")
    assert pipeline._Outputs(None, "cpu", fps=(25, 50), time_filter=dict(kind="ema", cutoff=2.0)).time_filter["fps"] == 25.0
    assert pipeline._Outputs(None, "cpu", time_filter=dict(kind="ema", cutoff=2.0, fps=24)).time_filter["fps"] == 24
    with pytest.raises(ValueError, match="frame rate"):
        pipeline._Outputs(None, "cpu", time_filter=dict(kind="one_euro", min_cutoff=1.0, beta=0.5))
    for bad in (dict(kind="one_euro", min_cutoff=1.0, beta=0.5, sigma=1.0), dict(kind="ema", cutoff=1.0, edge="mirror"), dict(kind="ema", cutoff=1.0, seconds=0.1)):
        with pytest.raises(ValueError, match="time_filter= takes"):
            pipeline._Outputs(p, "cpu", time_filter=bad)
    # the resolved dict is what the plan's identity takes
    assert tfilter.identity(5, **o.time_filter) == tfilter.identity(5, kind="one_euro", fps=p.fps, min_cutoff=1.0, beta=0.5)


def test_command_line_flags(tmp_path):
    ap = argparse.ArgumentParser()
    pipeline.add_time_filter_arguments(ap)
    p = presets.get("vocaset")
    parse = lambda *v: pipeline.time_filter_arguments(ap.parse_args(list(v)), p)  # noqa: E731
    assert parse("--time_filter", "one_euro:1.5:0.25") == dict(kind="one_euro", min_cutoff=1.5, beta=0.25, direction="zero_phase")
    assert parse("--time_filter", "one_euro:1.5:0.25:2", "--time_filter_direction", "causal") == dict(
        kind="one_euro", min_cutoff=1.5, beta=0.25, d_cutoff=2.0, direction="causal")
    assert parse("--time_filter", "ema:3") == dict(kind="ema", cutoff=3.0, direction="zero_phase")
    idx = tmp_path / "idx.npy"
    np.save(idx, np.array([2, 3]))
    tf = parse("--time_filter", "ema:3", "--time_filter_keep", str(idx), "--time_filter_keep_strength", "0.25")
    assert tf["strength"].shape == (p.V3 // 3,) and list(tf["strength"][:5]) == [1, 1, 0.25, 0.25, 1]
    for bad in (["--time_filter", "one_euro:1"], ["--time_filter", "one_euro:1:2:3:4"], ["--time_filter", "ema"], ["--time_filter", "ema:1:2"],
                ["--time_filter", "ema:x"], ["--time_filter", "ema:1", "--time_filter_edge", "nearest"], ["--time_filter", "gaussian:1", "--time_filter_direction", "causal"],
                ["--time_filter_direction", "causal"], ["--time_filter_seconds", "0.1", "--time_filter_direction", "causal"]):
        with pytest.raises(ValueError):
            parse(*bad)
    with pytest.raises(SystemExit):
        ap.parse_args(["--time_filter_direction", "backward"])
    o = pipeline._Outputs(p, "cpu", time_filter=parse("--time_filter", "one_euro:1.5:0.25"))
    assert o.time_filter == dict(kind="one_euro", min_cutoff=1.5, beta=0.25, direction="zero_phase", fps=float(p.fps))


# ---- properties of the definition, on the restatement
KINDS = [("ema", dict(cutoff=1.5)), ("one_euro", dict(min_cutoff=1.5, beta=0.5, d_cutoff=1.0))]


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
@pytest.mark.parametrize("kind,kw", KINDS)
def test_a_constant_comes_back_bit_for_bit(kind, kw, direction):
    q = RC.coeffs(kind, 30.0, **kw)
    x = np.tile(np.random.default_rng(1).standard_normal((1, 15)).astype(F32), (40, 1))
    assert np.array_equal(bits(RC.filter_clip(x, kind, q, direction)), bits(x))
    s = np.array([0, 0.3, 1, 0.5, 0], F32)
    assert np.array_equal(bits(RC.filter_clip(x, kind, q, direction, s)), bits(x))


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
def test_one_euro_without_beta_is_ema(direction):
    x = RC.clip(50, 15, 2)
    e = RC.filter_clip(x, "ema", RC.coeffs("ema", 30.0, cutoff=1.5), direction)
    o = RC.filter_clip(x, "one_euro", RC.coeffs("one_euro", 30.0, min_cutoff=1.5, beta=0.0, d_cutoff=0.7), direction)
    assert np.array_equal(bits(e), bits(o)) and not np.array_equal(bits(e), bits(x))


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
@pytest.mark.parametrize("kind,kw", KINDS)
def test_it_filters(kind, kw, direction):
    """A slow sinusoid (0.05 Hz at 30 fps, amplitude 1, one period) plus seeded white jitter of sigma 0.1: the filtered signal is nearer
    the clean one than the input is.  The sizes come from the one-pole response at a 1.5 Hz cutoff, a = 1.5 / (1.5 + 30 / 2 pi) = 0.24:
    the causal lag leaves about (0.05 / 1.5) / sqrt(2) = 0.024 rms and the jitter about 0.1 sqrt(a / (2 - a)) = 0.037, together 0.044
    against the input's 0.1 (One Euro's cutoff rises with the jitter's own speed and keeps somewhat more of it)."""
    g = np.random.default_rng(7)
    t = np.arange(600, dtype=np.float64)[:, None]
    clean = np.sin(2.0 * np.pi * 0.05 * t / 30.0 + np.linspace(0, 1, 15)[None, :])
    x = (clean + 0.1 * g.standard_normal(clean.shape)).astype(F32)
    y = RC.filter_clip(x, kind, RC.coeffs(kind, 30.0, **kw), direction)
    rms = lambda a: float(np.sqrt(np.mean((a.astype(np.float64) - clean) ** 2)))  # noqa: E731
    print(f"{kind} {direction}: rms in {rms(x):.4f} out {rms(y):.4f}")
    assert rms(y) < rms(x)


def test_one_euro_follows_a_fast_ramp():
    """A clip at rest, one ramp of 1 mesh unit over 6 frames (5 units per second at 30 fps), at rest again.  min_cutoff = 1 Hz, beta = 4,
    d_cutoff = 1 Hz: at 5 units per second the cutoff rises towards 1 + 4 * 5 = 21 Hz, far above the ema's 1 Hz, so the One Euro output
    stays much nearer the input during the ramp (the values are chosen so that this holds with room: the bound asked is a factor 2)"""
    L, r0, r1 = 60, 20, 26
    x = np.zeros((L, 3), F32)
    x[r0:r1 + 1] = (np.arange(r1 - r0 + 1, dtype=F32) / F32(r1 - r0))[:, None]
    x[r1:] = 1.0
    e = RC.filter_clip(x, "ema", RC.coeffs("ema", 30.0, cutoff=1.0))
    o = RC.filter_clip(x, "one_euro", RC.coeffs("one_euro", 30.0, min_cutoff=1.0, beta=4.0, d_cutoff=1.0))
    dev = lambda y: float(np.abs(y - x)[r0:r1 + 1].max())  # noqa: E731
    print(f"largest deviation during the ramp: ema {dev(e):.4f}, one_euro {dev(o):.4f}")
    assert dev(o) < dev(e) and 2.0 * dev(o) < dev(e)


def test_state_and_zero_phase_on_the_restatement():
    """Chunks with a carried state give the whole clip's bits; zero_phase is flip(causal(flip(causal(x))))"""
    x = RC.clip(37, 15, 3)
    for kind, kw in KINDS:
        q = RC.coeffs(kind, 30.0, **kw)
        whole = RC.filter_clip(x, kind, q)
        st = RC.fresh_state(15)
        parts = [RC.filter_clip(x[a:b], kind, q, state=st) for a, b in ((0, 1), (1, 1), (1, 9), (9, 37))]
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole)) and st["seen"] == 37
        z = RC.filter_clip(x, kind, q, "zero_phase")
        assert np.array_equal(bits(z), bits(RC.filter_clip(whole[::-1], kind, q)[::-1]))
