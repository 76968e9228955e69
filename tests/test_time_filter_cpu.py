"""CPU: the host side of the time filter hand-off (include/fdm_hip.h, fdm_tfilter_*): the taps of fdm_tfilter_taps_host against the
float64 restatement and the exact rational (tolerances derived in tests/time_filter_cases.py), every refusal of create and forward,
the mirror index against short clips, the restatement's own float32 / float64 agreement, and the argument handling of the pipeline
keyword and of the command-line flags.  Nothing here launches."""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import time_filter_cases as TC
from fdm_amd import _lib, pipeline, presets, tfilter
from fdm_amd._lib import FdmError

F32 = np.float32


def test_constants_mirror_the_header():
    import os
    src = open(os.path.join(os.path.dirname(tfilter.__file__), "..", "csrc", "tfilter.hpp")).read()
    for name, v in (("TF_TILE", tfilter.FRAME_TILE), ("TF_CHUNK", tfilter.COLUMN_CHUNK), ("TF_RMAX", tfilter.RADIUS_MAX)):
        assert f"constexpr int {name} = {v};" in src, name
    assert (TC.FRAME_TILE, TC.COLUMN_CHUNK, TC.RADIUS_MAX) == (tfilter.FRAME_TILE, tfilter.COLUMN_CHUNK, tfilter.RADIUS_MAX)
    assert tfilter.COLUMN_CHUNK % 12 == 0


@pytest.mark.parametrize("sigma,R", TC.GAUSSIAN_CASES)
def test_gaussian_taps(sigma, R):
    h, ref = tfilter.gaussian(sigma, R), TC.gaussian_taps(sigma, R)
    gap = float(np.abs(h - ref).max())
    print(f"gaussian sigma {sigma} R {R}: gap {gap:.3e}, bound {TC.gaussian_tol(R):.3e}")
    assert h.shape == (R + 1,) and gap <= TC.gaussian_tol(R)
    assert abs(h[0] + 2.0 * h[1:].sum() - 1.0) <= (R + 2) * 2.0 ** -52 and (np.diff(h) <= 0).all()


def test_gaussian_default_radius():
    assert len(tfilter.gaussian(1.5)) == 6 and len(tfilter.gaussian(2.0)) == 7 and len(tfilter.gaussian(50.0)) == 33 and len(tfilter.gaussian(0.2)) == 2


@pytest.mark.parametrize("R,order", TC.SAVGOL_CASES)
def test_savgol_taps(R, order):
    h, ref = tfilter.savgol(R, order), TC.savgol_taps(R, order)
    gap = float(np.abs(h - ref).max())
    print(f"savgol R {R} order {order}: gap {gap:.3e}, bound {TC.savgol_tol(R, order):.3e}")
    assert gap <= TC.savgol_tol(R, order)
    if order in (2, 3):      # the closed form, exact rationals: one side's allowance
        exact = TC.savgol2_exact(R)
        gap = max(abs(float(a) - float(b)) for a, b in zip(exact, h))      # (the rational's conversion rounds once more: below u64 |h|)
        print(f"  against the rational: gap {gap:.3e}, bound {TC.savgol_tol(R, order, sides=1):.3e}")
        assert gap <= TC.savgol_tol(R, order, sides=1)
    pair = {2: 3, 3: 2, 4: 5, 5: 4}[order]
    if pair < 2 * R + 1:     # odd polynomials vanish at the centre: the orders share a row
        assert float(np.abs(tfilter.savgol(R, pair) - h).max()) <= TC.savgol_tol(R, max(order, pair))


def test_taps_refusals():
    h = np.zeros(40)
    taps = lambda kind, R, p, out=h.ctypes.data: _lib.lib().fdm_tfilter_taps_host(kind, R, C.c_double(p), out)  # noqa: E731
    assert taps(0, 4, 1.0) == 0
    assert taps(0, 4, 1.0, None) == -1 and b"null" in _lib.lib().fdm_last_error()
    for R in (-1, 33):
        assert taps(0, R, 1.0) == -1 and taps(1, R, 2.0) == -1
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        assert taps(0, 4, sigma) == -1
    for order in (0.0, 1.0, 6.0, 2.5, float("nan")):
        assert taps(1, 8, order) == -1
    assert taps(1, 1, 3.0) == -1 and taps(1, 2, 5.0) == -1 and taps(1, 0, 2.0) == -1 and b"window" in _lib.lib().fdm_last_error()      # order >= 2 R + 1
    assert taps(1, 1, 2.0) == 0 and taps(1, 2, 4.0) == 0
    assert taps(2, 4, 1.0) == -1 and b"kind" in _lib.lib().fdm_last_error()
    with pytest.raises(ValueError):
        tfilter.taps_host("box", 3, 1.0)
    with pytest.raises(FdmError):
        tfilter.savgol(1, 4)


def _create(V, R, taps, strength=None, edge=0):
    h = C.c_void_p()
    t = None if taps is None else np.ascontiguousarray(taps, dtype=F32)
    s = None if strength is None else np.ascontiguousarray(strength, dtype=F32)
    rc = _lib.lib().fdm_tfilter_create(V, R, None if t is None else t.ctypes.data, None if s is None else s.ctypes.data, edge, None, C.byref(h))
    return rc, h


def test_create_and_forward_refusals():
    l = _lib.lib()
    ok = np.array([0.5, 0.25], F32)
    assert l.fdm_tfilter_create(4, 1, ok.ctypes.data, None, 0, None, None) == -1
    for args in ((0, 1, ok), (-3, 1, ok), (4, -1, ok), (4, 33, np.zeros(34, F32)), (4, 1, None), (4, 1, [0.5, np.nan]), (4, 1, [np.inf, 0.25])):
        rc, h = _create(*args)
        assert rc == -1 and not h.value, args
    for s in ([0, 0.5, 1, 1.5], [0, -0.1, 1, 1], [0, np.nan, 1, 1], [np.inf, 0, 0, 0]):
        rc, h = _create(4, 1, ok, s)
        assert rc == -1 and not h.value and b"strength" in l.fdm_last_error()
    for edge in (-1, 2):
        rc, h = _create(4, 1, ok, None, edge)
        assert rc == -1 and b"edge" in l.fdm_last_error()
    for args in ((4, 1, ok, [0, 0.5, 1, 1], 1), (1, 0, [1.0]), (4, 32, np.full(33, 1 / 65, F32))):
        rc, h = _create(*args)
        assert rc == 0 and h.value
        assert l.fdm_tfilter_destroy(h) == 0
    assert l.fdm_tfilter_destroy(None) == 0
    rc, h = _create(4, 1, ok)
    assert rc == 0
    x, y, B, L = 0x10000, 0x20000, 3, 7              # never dereferenced: no call gets as far as a launch
    fr = lambda *a: (C.c_int * len(a))(*a)  # noqa: E731
    fwd = l.fdm_tfilter_forward
    assert fwd(None, x, fr(7, 1, 4), B, L, y) == -1 and fwd(h, None, fr(7, 1, 4), B, L, y) == -1 and fwd(h, x, fr(7, 1, 4), B, L, None) == -1
    assert fwd(h, x, fr(7, 1, 4), 0, L, y) == -2 and fwd(h, x, fr(7, 1, 4), -1, L, y) == -2 and fwd(h, x, None, B, 0, y) == -2
    for bad in (fr(7, 0, 4), fr(7, 8, 4), fr(-1, 1, 4)):
        assert fwd(h, x, bad, B, L, y) == -2 and b"frames" in l.fdm_last_error()
    n = B * L * 12 * 4                               # bytes of the batch
    for yy in (x, x + 4, x + n - 4, x - n + 4):
        assert fwd(h, x, fr(7, 1, 4), B, L, yy) == -1 and b"overlap" in l.fdm_last_error()
    if not l.fdm_device_ok():
        for yy in (x + n, x - n):                    # adjacent, not overlapping: as far as the device check
            assert fwd(h, x, fr(7, 1, 4), B, L, yy) == -4 and b"no gfx950 device" in l.fdm_last_error()
        assert fwd(h, x, None, B, L, y) == -4
    assert l.fdm_tfilter_destroy(h) == 0


def test_mirror_index_against_short_clips():
    """L in {1, 2, 3} with R = 32: every index lands inside the clip, the end sample is not repeated, and the filter of the
    restatement reads nothing else (NaN beyond the clip does not matter)"""
    i = np.arange(-40, 44)
    assert (TC.edge_index(i, 1) == 0).all()
    assert (TC.edge_index(i, 2) == np.abs(i) % 2).all()
    assert list(TC.edge_index(np.arange(-5, 8), 3)) == [1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1]
    assert list(TC.edge_index(np.arange(-3, 8), 5)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert list(TC.edge_index(np.arange(-3, 8), 5, "nearest")) == [0, 0, 0, 0, 1, 2, 3, 4, 4, 4, 4]
    h = TC.taps_for(32)
    for L in (1, 2, 3):
        x = TC.clip(L, 6, L)
        y = TC.filter_f32(x, h)
        assert y.shape == (L, 6) and np.isfinite(y).all()
        if L == 1:      # every tap reads the one frame
            want = TC.filter_f64(x, h)
            assert (np.abs(y - want) <= TC.bound(x, h)).all()


@pytest.mark.parametrize("R", [0, 1, 8, 32])
@pytest.mark.parametrize("edge", ["mirror", "nearest"])
def test_restatements_agree_within_the_derived_bound(R, edge):
    x, h = TC.clip(50, 12, R), TC.taps_for(R)
    s = np.array([0.0, 0.5, 1.0, 0.25], F32)
    for st in (None, s):
        y32, y64 = TC.filter_f32(x, h, edge, st), TC.filter_f64(x, h, edge, st)
        assert y32.dtype == F32 and (np.abs(y32.astype(np.float64) - y64) <= TC.bound(x, h, edge, st)).all()
    assert np.array_equal(TC.filter_f32(x, h, edge, s)[:, :3].view(np.uint32), x[:, :3].view(np.uint32))      # s = 0: the input bits
    rev = TC.filter_f32(x[::-1], h, edge)
    assert np.array_equal(rev[::-1].view(np.uint32), TC.filter_f32(x, h, edge).view(np.uint32))


def test_plan_arguments_and_key():
    a = tfilter.identity(5, kind="gaussian", sigma=1.5, radius=4)
    assert a == tfilter.identity(5, taps=tfilter.gaussian(1.5, 4)) and a[:3] == (5, 4, "mirror")
    assert a != tfilter.identity(5, kind="gaussian", sigma=1.5, radius=4, edge="nearest")
    assert a != tfilter.identity(5, kind="gaussian", sigma=1.5, radius=4, strength=np.ones(5))
    assert a != tfilter.identity(6, kind="gaussian", sigma=1.5, radius=4)
    assert tfilter.identity(5, kind="savgol", radius=4, order=2) == tfilter.identity(5, taps=tfilter.savgol(4, 2))
    for kw in (dict(), dict(kind="savgol", radius=3), dict(kind="savgol", order=2), dict(kind="box", sigma=1), dict(sigma=1.0, edge="wrap")):
        with pytest.raises(ValueError):
            tfilter.identity(5, **kw)
    with pytest.raises(FdmError):
        tfilter.identity(5, sigma=1.0, strength=np.ones(4))
    s = tfilter.strength_from_region(6, [1, 4], 0.25)
    assert s.dtype == F32 and list(s) == [1, 0.25, 1, 1, 0.25, 1]
    assert list(tfilter.strength_from_region(3, [0], 0.0, outside=0.5)) == [0, 0.5, 0.5]
    with pytest.raises(FdmError):
        tfilter.TimeFilterPlan(5, sigma=1.0, device="cpu")


def test_outputs_argument_handling():
    """_Outputs(..., time_filter=) on "cpu": the arguments are checked before anything runs; the keyword is the last one"""
    import inspect
    assert list(inspect.signature(pipeline._Outputs.__init__).parameters)[-1] == "time_filter"
    p = presets.get("vocaset")
    o = pipeline._Outputs(p, "cpu", time_filter=dict(kind="gaussian", seconds=0.05))
    assert o.time_filter == dict(kind="gaussian", sigma=0.05 * 30)
    assert pipeline._Outputs(p, "cpu", in_fps=60, time_filter=dict(seconds=0.05)).time_filter == dict(sigma=0.05 * 60)
    assert pipeline._Outputs(None, "cpu", fps=(25, 50), time_filter=dict(seconds=0.1)).time_filter == dict(sigma=0.1 * 25)
    assert pipeline._Outputs(p, "cpu").time_filter is None
    for bad, msg in ((dict(sigma=1.0, seconds=0.1), "not both"), (dict(sigma=1.0, cutoff=3), "time_filter= takes"), ("gaussian", "time_filter= takes"),
                     ([0.5, 0.25], "time_filter= takes")):
        with pytest.raises(ValueError, match=msg):
            pipeline._Outputs(p, "cpu", time_filter=bad)
    with pytest.raises(ValueError, match="frame rate"):
        pipeline._Outputs(None, "cpu", time_filter=dict(seconds=0.1))
    # a host tensor is refused as everywhere on the HIP path, in the hand-off's name
    with pytest.raises(FdmError, match="to_filtered"):
        pipeline._Outputs(p, "cpu", time_filter=dict(sigma=1.0))(torch.zeros(1, 4, p.V3))
    with pytest.raises(FdmError, match="to_filtered"):
        pipeline.to_filtered([torch.zeros(1, 4, 12), torch.zeros(1, 2, 12)], dict(sigma=1.0))
    for fn in (pipeline.animate, pipeline.animate_many, pipeline.animate_long, pipeline.SlotServer.__init__):
        assert inspect.signature(fn).parameters["time_filter"].default is None


def test_command_line_flags(tmp_path):
    ap = argparse.ArgumentParser()
    pipeline.add_time_filter_arguments(ap)
    p = presets.get("vocaset")
    assert pipeline.time_filter_arguments(ap.parse_args([]), p) is None
    assert pipeline.time_filter_arguments(ap.parse_args(["--time_filter", "gaussian:1.5"]), p) == dict(kind="gaussian", sigma=1.5, edge="mirror")
    assert pipeline.time_filter_arguments(ap.parse_args(["--time_filter", "savgol:4:2", "--time_filter_edge", "nearest"]), p) == dict(
        kind="savgol", radius=4, order=2, edge="nearest")
    assert pipeline.time_filter_arguments(ap.parse_args(["--time_filter_seconds", "0.05"]), p) == dict(kind="gaussian", seconds=0.05, edge="mirror")
    idx = tmp_path / "idx.npy"
    np.save(idx, np.array([2, 3]))
    tf = pipeline.time_filter_arguments(ap.parse_args(["--time_filter", "gaussian:2", "--time_filter_keep", str(idx), "--time_filter_keep_strength", "0.25"]), p)
    assert tf["strength"].shape == (p.V3 // 3,) and list(tf["strength"][:5]) == [1, 1, 0.25, 0.25, 1]
    assert float(pipeline.time_filter_arguments(ap.parse_args(["--time_filter", "gaussian:2", "--time_filter_keep", str(idx)]), p)["strength"][2]) == 0.0
    for bad in (["--time_filter", "box:3"], ["--time_filter", "gaussian"], ["--time_filter", "savgol:4"], ["--time_filter", "gaussian:1", "--time_filter_seconds", "0.1"],
                ["--time_filter_keep", str(idx)], ["--time_filter_edge", "nearest"], ["--time_filter", "gaussian:x"]):
        with pytest.raises(ValueError):
            pipeline.time_filter_arguments(ap.parse_args(bad), p)
    with pytest.raises(SystemExit):
        ap.parse_args(["--time_filter_edge", "wrap"])
    # what the flags give is what _Outputs takes
    o = pipeline._Outputs(p, "cpu", time_filter=pipeline.time_filter_arguments(ap.parse_args(["--time_filter_seconds", "0.05"]), p))
    assert o.time_filter == dict(kind="gaussian", sigma=1.5, edge="mirror")
