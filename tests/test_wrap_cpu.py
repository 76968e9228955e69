"""No GPU: the host side of the wrap hand-off (include/fdm_hip.h, fdm_wrap_*) -- fdm_wrap_coords_host against the float64 restatement
of tests/wrap_cases.py, the float32 search and follow restatements against their float64 forms (which also proves their inputs free
of subnormal intermediates), every refusal that is decided without a device, and a binding brought by the caller read back.

Measured here (numpy, these inputs) and recorded in DESIGN.md section 2 item 22:
  search   the float32 restatement picks another face than float64 brute force for 4 of 2214 target vertices; the largest float64
           distance excess of its choice is 2.7755575615628914e-17.  SEARCH_MARGIN is 4x that.
  follow   the largest |float32 - float64| of the follow restatement over rest reproduction and the rigid motion, sources x (own,
           lifted) targets, is 2.47558025412431e-07 (grid_extra, whose isolated vertex extrapolates 29 edge lengths).  FOLLOW_GATE is 4x that."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as MC
import wrap_cases as WC
from fdm_amd import _lib, wrap

ARG, SHAPE, STATE = -1, -2, -4
SEARCH_MARGIN = 4 * 2.7755575615628914e-17
FOLLOW_GATE = 4 * 2.47558025412431e-07


def test_symbols_are_bound_and_the_version_stays():
    l = _lib.lib()
    for name in ("fdm_wrap_coords_host", "fdm_wrap_create", "fdm_wrap_binding", "fdm_wrap_forward", "fdm_wrap_destroy"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_version() == _lib.LIB_VERSION == 105 and _lib.WRAP_OFFSETS == 1


def test_the_face_tile_the_cases_are_sized_by_is_the_kernels():
    import os
    import re
    hpp = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "csrc", "wrap_out.hpp")
    assert int(re.search(r"constexpr int WRAP_FT = (\d+);", open(hpp).read()).group(1)) == wrap.FACE_TILE


@pytest.mark.parametrize("cs", WC.SEARCH_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_search_restatement_against_float64_brute_force_and_host_coordinates(cs):
    """fdm_wrap_coords_host computes in fp64 in the header's order and rounds once: equality with the restatement after rounding to
    fp32 is attained (largest difference measured: 0)."""
    S, faces, T = WC.case(*cs)
    fi, d2, reg = WC.nearest(S, faces, T)
    assert (fi >= 0).all() and (WC.face_area2(S, faces)[fi] > 0).all()          # no vertex is left out; no face without area is chosen
    D = WC.all_dist2_f64(S, faces, T)
    mine, best = np.sqrt(D[np.arange(len(T)), fi]), np.sqrt(D.min(axis=1))
    print(f"{cs}: {int((fi != D.argmin(axis=1)).sum())} of {len(T)} choices differ from float64; largest excess {(mine - best).max():.3e}")
    assert ((mine - best) <= SEARCH_MARGIN).all()
    uvh, dist = wrap.coords(S, faces, T, fi)
    want_uvh, want_dist = WC.coords(S, faces, T, fi)
    assert np.array_equal(uvh.view(np.uint32), want_uvh.view(np.uint32)) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
    assert np.array_equal(dist, np.sqrt(D[np.arange(len(T)), fi]).astype(np.float32))
    # q = a + u e1 + v e2 + h nh
    a, b, c = (S[faces[fi, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    q = a + uvh[:, :1] * (b - a) + uvh[:, 1:2] * (c - a) + uvh[:, 2:] * n / np.linalg.norm(n, axis=1, keepdims=True)
    assert np.abs(q - T).max() <= 2.0 ** -22 * (1 + np.abs(uvh).max()) * np.abs(S).max()


def test_all_seven_regions_occur_and_are_the_ones_aimed_at():
    S, faces, T = WC.case("one_face", "regions", None)
    fi, _, reg = WC.nearest(S, faces, T)
    assert list(fi) == [0] * 7 and list(reg) == [0, 1, 2, 3, 4, 5, 6], [WC.REGIONS[r] for r in reg]


def test_a_tie_keeps_the_lowest_face_index():
    S, faces, T = WC.case("ridge", "ties", None)
    D = WC.all_dist2_f64(S, faces, T)
    assert (D[:, 0] == D[:, 1]).all()                   # both faces are exactly as far: the closest point is on the shared edge
    fi, d2, reg = WC.nearest(S, faces, T)
    assert list(fi) == [0] * len(T) and (reg == 2).all() and np.array_equal(d2.astype(np.float64), D[:, 0])
    # vertices of the source itself: every incident face ties at distance 0
    S, faces, T = WC.case("fan", "own", None)
    fi, d2, _ = WC.nearest(S, faces, T)
    assert (d2 == 0).all() and fi[0] == 0 and all(fi[v] == np.nonzero((faces == v).any(axis=1))[0][0] for v in range(len(T)))


def test_a_face_without_area_is_never_a_candidate_and_nan_never_wins():
    S, faces = WC.source("degenerate")
    f = MC.DEGENERATE["degenerate"]
    assert WC.face_area2(S, faces)[f] == 0
    T = S[faces[f, [0, 2]]].copy()                      # the two distinct vertices of the degenerate face
    fi, _, _ = WC.nearest(S, faces, T)
    assert (fi != f).all() and (fi >= 0).all()
    only = faces[f:f + 1]
    assert list(WC.nearest(S, only, T)[0]) == [-1, -1]  # nothing but a face without area: no candidate


def _rest_and_rigid(name, kind):
    S, faces = WC.source(name)
    T = WC.targets(name, kind)
    fi, _, _ = WC.nearest(S, faces, T)
    uvh, _ = WC.coords(S, faces, T, fi)
    R, t = WC.rotation()
    moved = (S.astype(np.float64) @ R.T + t).astype(np.float32)
    return S, faces, T, fi, uvh, R, t, moved


def _sensitivity(P, faces, fi, uvh):
    """per target vertex: how far y moves per unit the source vertices move (y is linear in a, b, c but for the unit normal)"""
    a, b, c = (P[faces[fi, k]].astype(np.float64) for k in range(3))
    n = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    u, v, h = (np.abs(uvh[:, k].astype(np.float64)) for k in range(3))
    return np.abs(1 - uvh[:, 0] - uvh[:, 1]) + u + v + h * 2 * (np.linalg.norm(b - a, axis=1) + np.linalg.norm(c - a, axis=1)) / n


@pytest.mark.parametrize("kind", ["own", "lifted"])
@pytest.mark.parametrize("name", WC.SOURCES)
def test_rest_reproduction_and_rigid_covariance(name, kind):
    """float32 against float64 under FOLLOW_GATE (4x the largest difference measured, module docstring).  Against T and R T + t
    themselves the float64 restatement is held to what the rounding of its float32 INPUTS allows: every source coordinate and
    coefficient is off by at most 2^-24 of its size, and y moves by `_sensitivity` times that; 4 covers the three components and
    the coefficients."""
    S, faces, T, fi, uvh, R, t, moved = _rest_and_rigid(name, kind)
    V = len(S)
    zero, tm = np.zeros((1, 1, 3 * V), np.float32), S.reshape(1, -1)
    y32 = WC.follow(zero, tm, [1], faces, fi, uvh, T)[0]
    y64 = WC.follow(zero, tm, [1], faces, fi, uvh, T, dt=np.float64)[0]
    r32 = WC.follow(moved.reshape(1, 1, -1), None, [1], faces, fi, uvh, T)[0]
    r64 = WC.follow(moved.reshape(1, 1, -1), None, [1], faces, fi, uvh, T, dt=np.float64)[0]
    want = (T.astype(np.float64) @ R.T + t)
    print(f"{name} {kind}: rest |f32 - f64| {np.abs(y32 - y64).max():.3e} |f32 - T| {np.abs(y32 - T.reshape(1, -1)).max():.3e}; "
          f"rigid |f32 - f64| {np.abs(r32 - r64).max():.3e} |f32 - (R T + t)| {np.abs(r32 - want.reshape(1, -1)).max():.3e}")
    assert np.abs(y32 - y64).max() <= FOLLOW_GATE and np.abs(r32 - r64).max() <= FOLLOW_GATE
    for y, P, exact in ((y64, S, T.astype(np.float64)), (r64, moved, want)):
        bound = 4 * 2.0 ** -24 * max(np.abs(P).max(), np.abs(exact).max()) * (1 + _sensitivity(P, faces, fi, uvh))
        assert (np.abs(y.reshape(-1, 3) - exact).max(axis=1) <= bound).all()
    # and float32 within both
    assert (np.abs(y32.reshape(-1, 3) - T).max(axis=1) <= FOLLOW_GATE + 4 * 2.0 ** -24 * np.abs(S).max() * (1 + _sensitivity(S, faces, fi, uvh))).all()


def test_weights_and_offsets_forms_of_the_restatement():
    S, faces, T, fi, uvh, _, _, _ = _rest_and_rigid("grid", "lifted")
    off, tm = MC.offsets("grid", 1, 2, seed=5), S.reshape(1, -1)
    w = np.linspace(0, 1, len(T)).astype(np.float32)
    y = WC.follow(off, tm, [2], faces, fi, uvh, T)[0].reshape(2, -1, 3)
    o = WC.follow(off, tm, [2], faces, fi, uvh, T, offsets_out=True)[0].reshape(2, -1, 3)
    yw = WC.follow(off, tm, [2], faces, fi, uvh, T, w)[0].reshape(2, -1, 3)
    ow = WC.follow(off, tm, [2], faces, fi, uvh, T, w, offsets_out=True)[0].reshape(2, -1, 3)
    assert np.array_equal(o, y - T[None]) and np.array_equal(ow, w[None, :, None] * o) and np.array_equal(yw, T[None] + ow)
    assert np.array_equal(yw[:, 0], np.broadcast_to(T[0], (2, 3))) and np.array_equal(ow[:, -1], o[:, -1])      # w = 0 stays at rest, w = 1 follows


def test_falloff_weights():
    w = wrap.falloff_weights(np.array([0.0, 0.5, 1.0, 1.5, 2.0]), 0.5, 1.5)
    assert w.dtype == np.float32 and list(w) == [1.0, 1.0, 0.5, 0.0, 0.0]
    assert list(wrap.falloff_weights(np.array([0.1, 0.3]), 0.2, 0.2)) == [1.0, 0.0]
    with pytest.raises(ValueError):
        wrap.falloff_weights(np.zeros(2), 1.0, 0.5)


def _arrays():
    S, faces, T = WC.case("degenerate", "lifted", 65)
    fi, _, _ = WC.nearest(S, faces, T)
    return np.ascontiguousarray(S), np.ascontiguousarray(faces), T, fi


def test_coords_refusals():
    l = _lib.lib()
    S, faces, T, fi = _arrays()
    uvh, dist = np.zeros((len(T), 3), np.float32), np.zeros(len(T), np.float32)

    def call(S=S, faces=faces, F=len(faces), V=len(S), T=T, Vt=len(T), fi=fi, uvh=uvh, dist=dist):
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return l.fdm_wrap_coords_host(p(S), p(faces), F, V, p(T), Vt, p(fi), p(uvh), p(dist))
    assert call() == 0
    for k in ("S", "faces", "T", "fi", "uvh", "dist"):
        assert call(**{k: None}) == ARG, k
    assert call(F=0) == ARG and call(V=0) == ARG and call(Vt=0) == ARG and call(F=-1) == ARG
    assert call(V=len(S) - 1) == ARG and b"names vertex" in l.fdm_last_error()
    bad = fi.copy()
    bad[3] = len(faces)
    assert call(fi=bad) == ARG and b"target vertex 3" in l.fdm_last_error()
    bad[3] = -1
    assert call(fi=bad) == ARG
    bad[3] = MC.DEGENERATE["degenerate"]
    assert call(fi=bad) == ARG and b"no area" in l.fdm_last_error()
    for arr, name in ((S, "S"), (T, "T")):
        for v in (np.nan, np.inf):
            x = arr.copy()
            x[2, 1] = v
            assert call(**{name: x}) == ARG and b"non-finite" in l.fdm_last_error()


def test_create_and_forward_refusals_precede_any_launch_and_the_binding_reads_back():
    """With face_idx given the object needs no device; a forward call that passes every check on a machine without a GPU ends in
    FDM_ERR_STATE, never in a fallback.  (The device pointers below are never dereferenced.)"""
    l = _lib.lib()
    S, faces, T, fi = _arrays()
    Vt = len(T)
    w = np.linspace(0, 1, Vt).astype(np.float32)
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731

    def create(h, S=S, faces=faces, F=len(faces), V=len(S), T=T, Vt=Vt, fi=fi, w=None):
        return l.fdm_wrap_create(p(S), p(faces), F, V, p(T), Vt, p(fi), p(w), h)
    h = C.c_void_p()
    assert l.fdm_wrap_create(p(S), p(faces), len(faces), len(S), p(T), Vt, p(fi), None, None) == ARG
    for k in ("S", "faces", "T"):
        assert create(C.byref(h), **{k: None}) == ARG and not h.value
    assert create(C.byref(h), Vt=0) == ARG and create(C.byref(h), V=3) == ARG
    for v in (-0.25, 1.5, np.nan, np.inf):
        bad = w.copy()
        bad[7] = v
        assert create(C.byref(h), w=bad) == ARG and b"target vertex 7" in l.fdm_last_error() and not h.value
    bad = fi.copy()
    bad[5] = len(faces)
    assert create(C.byref(h), fi=bad) == ARG and not h.value
    bad[5] = MC.DEGENERATE["degenerate"]
    assert create(C.byref(h), fi=bad) == ARG and b"no area" in l.fdm_last_error() and not h.value
    x = T.copy()
    x[0, 0] = np.nan
    assert create(C.byref(h), T=x) == ARG and not h.value
    if not l.fdm_device_ok():
        assert create(C.byref(h), fi=None) == STATE and b"no CPU fallback" in l.fdm_last_error() and not h.value
    assert create(C.byref(h), w=w) == 0 and h.value
    try:
        got_fi, got_uvh, got_dist = np.full(Vt, -7, np.int32), np.zeros((Vt, 3), np.float32), np.zeros(Vt, np.float32)
        assert l.fdm_wrap_binding(None, p(got_fi), p(got_uvh), p(got_dist)) == ARG
        assert l.fdm_wrap_binding(h, p(got_fi), None, None) == 0 and np.array_equal(got_fi, fi)
        assert l.fdm_wrap_binding(h, None, p(got_uvh), p(got_dist)) == 0
        want_uvh, want_dist = wrap.coords(S, faces, T, fi)
        assert np.array_equal(got_uvh, want_uvh) and np.array_equal(got_dist, want_dist)
        B, L_max = 3, 5
        X, Y = C.c_void_p(0x1000), C.c_void_p(0x2000)

        def fwd(hh=h, off=X, frames=(C.c_int * B)(5, 0, 2), B=B, L_max=L_max, tmpl=X, rows=1, flags=0, out=Y):
            return l.fdm_wrap_forward(hh, off, frames, B, L_max, tmpl, rows, flags, out, None)
        assert fwd(hh=None) == ARG and fwd(off=None) == ARG and fwd(out=None) == ARG
        assert fwd(flags=2) == ARG and b"flag" in l.fdm_last_error() and fwd(flags=-1) == ARG
        assert fwd(rows=2) == ARG and fwd(rows=-1) == ARG and fwd(tmpl=None) == ARG and fwd(tmpl=None, rows=B) == ARG
        assert fwd(B=0, rows=0) == SHAPE and fwd(L_max=0) == SHAPE
        assert fwd(L_max=4) == SHAPE and fwd(frames=(C.c_int * B)(5, -1, 2)) == SHAPE and fwd(frames=(C.c_int * B)(5, 6, 2)) == SHAPE
        if not l.fdm_device_ok():            # (with a device these calls would launch on pointers that are not memory)
            for kw in (dict(), dict(rows=0, tmpl=None), dict(rows=B), dict(flags=_lib.WRAP_OFFSETS), dict(frames=None)):
                assert fwd(**kw) == STATE and b"no CPU fallback" in l.fdm_last_error(), kw
    finally:
        assert l.fdm_wrap_destroy(h) == 0 and l.fdm_wrap_destroy(None) == 0


def test_plan_without_a_device_validates_and_reports_its_binding():
    S, faces, T, fi = _arrays()
    plan = wrap.WrapPlan(S, faces, T, face_idx=fi)
    got_fi, uvh, dist = plan.binding()
    want_uvh, want_dist = WC.coords(S, faces, T, fi)
    assert np.array_equal(got_fi, fi) and np.array_equal(uvh, want_uvh) and np.array_equal(dist, want_dist)
    assert plan.key == wrap.identity(S, faces, T, fi) != wrap.identity(S, faces, T, fi, np.ones(len(T), np.float32))
    with pytest.raises(_lib.FdmError):
        wrap.WrapPlan(S, faces, T, face_idx=fi[:-1])
    with pytest.raises(_lib.FdmError):
        wrap.WrapPlan(S, faces, T, face_idx=fi, weights=np.full(len(T), 2.0, np.float32))
