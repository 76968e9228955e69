"""No GPU: the host side of the mesh hand-off (include/fdm_hip.h, fdm_mesh_*) -- the incident-face lists against numpy, the frame
rule against its Python expression, every refusal that is decided before a launch, and the float32 oracle of tests/mesh_cases.py
against its float64 restatement (which also proves its inputs free of subnormal intermediates)."""
import ctypes as C

import numpy as np
import pytest

import mesh_cases as MC
from fdm_amd import _lib, mesh

ARG, SHAPE, STATE = -1, -2, -4


def test_symbols_are_bound():
    l = _lib.lib()
    for name in ("fdm_mesh_adjacency_host", "fdm_mesh_create", "fdm_mesh_frames", "fdm_mesh_forward", "fdm_mesh_destroy"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_version() == _lib.LIB_VERSION == 105
    assert (_lib.MESH_INTERLEAVED, _lib.MESH_F16, _lib.MESH_NORMALS) == (1, 2, 4)


@pytest.mark.parametrize("name", MC.SMALL + ["vocaset_size"])
def test_adjacency_against_numpy(name):
    faces, V, _ = MC.mesh(name)
    off, items = mesh.adjacency(faces, V)
    want_off, want_items = MC.adjacency(faces, V)
    assert off.dtype == np.int32 and np.array_equal(off, want_off) and np.array_equal(items, want_items)
    assert off[-1] == 3 * len(faces)
    for v in range(V):                     # ascending, one entry per corner
        row = items[off[v]:off[v + 1]]
        assert np.all(np.diff(row) >= 0) and len(row) == int((faces == v).sum())
    if name in MC.ISOLATED:
        v = MC.ISOLATED[name]
        assert off[v] == off[v + 1]
    if name in MC.DEGENERATE:
        f = MC.DEGENERATE[name]
        a = faces[f, 0]
        assert list(items[off[a]:off[a + 1]]).count(f) == 2
    if name == "fan":
        assert off[1] - off[0] == 40


def test_adjacency_refusals():
    l = _lib.lib()
    f = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    off, items = np.zeros(5, dtype=np.int32), np.zeros(6, dtype=np.int32)
    call = lambda fp, F, V, o=off.ctypes.data, i=items.ctypes.data: l.fdm_mesh_adjacency_host(fp, F, V, o, i)  # noqa: E731
    assert call(f.ctypes.data, 2, 4) == 0
    assert call(None, 2, 4) == ARG and call(f.ctypes.data, 2, 4, o=None) == ARG and call(f.ctypes.data, 2, 4, i=None) == ARG
    assert call(f.ctypes.data, -1, 4) == ARG and call(f.ctypes.data, 2, 0) == ARG and call(f.ctypes.data, 2, -3) == ARG
    assert call(f.ctypes.data, 2, 3) == ARG and b"vertex 3" in l.fdm_last_error()           # index == V
    g = f.copy()
    g[1, 0] = -1
    assert call(g.ctypes.data, 2, 4) == ARG
    assert call(f.ctypes.data, 0, 4) == 0 and np.array_equal(off, np.zeros(5))                # no faces: every list empty


def test_frames_rule():
    l = _lib.lib()
    n = C.c_int(-1)
    for fi, fo in MC.RATES:
        for L in range(1, 41):
            assert l.fdm_mesh_frames(L, float(fi), float(fo), C.byref(n)) == 0
            want = L if fi == fo else max(1, int(float(L) / fi * fo))
            assert n.value == want == MC.frames_out(L, (fi, fo)) == mesh.frames_out(L, fi, fo), (L, fi, fo)
    assert l.fdm_mesh_frames(7, 0.0, 0.0, C.byref(n)) == 0 and n.value == 7                   # no rates: pass through
    assert l.fdm_mesh_frames(7, 30.0, 0.0, C.byref(n)) == 0 and n.value == 7
    assert l.fdm_mesh_frames(0, 30.0, 60.0, C.byref(n)) == 0 and n.value == 0                 # no frames, no rows
    assert l.fdm_mesh_frames(7, 30.0, 60.0, None) == ARG and l.fdm_mesh_frames(-1, 30.0, 60.0, C.byref(n)) == ARG
    assert l.fdm_mesh_frames(7, -30.0, 60.0, C.byref(n)) == ARG and l.fdm_mesh_frames(7, 30.0, float("nan"), C.byref(n)) == ARG
    assert l.fdm_mesh_frames(2 ** 31 - 1, 1.0, 4.0, C.byref(n)) == SHAPE


def test_create_refusals_and_forward_validation_precede_any_launch():
    """Every refusal is decided before a launch (the device pointers below are never dereferenced).  The object needs no device; a
    call that passes every check on a machine without a GPU ends in FDM_ERR_STATE, never in a fallback."""
    l = _lib.lib()
    faces, V, _ = MC.mesh("grid")
    h = C.c_void_p()
    fp = faces.ctypes.data
    assert l.fdm_mesh_create(fp, len(faces), V, None) == ARG and l.fdm_mesh_create(None, len(faces), V, C.byref(h)) == ARG
    assert l.fdm_mesh_create(fp, -1, V, C.byref(h)) == ARG and l.fdm_mesh_create(fp, len(faces), 0, C.byref(h)) == ARG
    assert l.fdm_mesh_create(fp, len(faces), V - 1, C.byref(h)) == ARG                        # vertex 31 of 31
    assert l.fdm_mesh_destroy(None) == 0
    assert l.fdm_mesh_create(fp, len(faces), V, C.byref(h)) == 0
    try:
        B, L = 3, 7
        fr = (C.c_int * B)(7, 1, 4)
        got = (C.c_int * B)()
        N = _lib.MESH_NORMALS

        def fwd(m=h, off=4096, frames=fr, B=B, L_max=L, tmpl=8192, rows=1, fi=30.0, fo=60.0, flags=N, pos=12288, nrm=16384, Lo=14, out=got):
            return l.fdm_mesh_forward(m, off, frames, B, L_max, tmpl, rows, fi, fo, flags, pos, nrm, Lo, out, None)
        assert fwd(m=None) == ARG and fwd(off=None) == ARG and fwd(pos=None) == ARG
        assert fwd(rows=2) == ARG and b"tmpl_rows" in l.fdm_last_error()                      # 0, 1 or B
        assert fwd(rows=-1) == ARG and fwd(rows=1, tmpl=None) == ARG
        assert fwd(flags=8) == ARG and fwd(flags=N | 64) == ARG and b"flag" in l.fdm_last_error()
        assert fwd(flags=N | _lib.MESH_INTERLEAVED) == ARG and b"nrm" in l.fdm_last_error()   # interleaved takes nrm = NULL
        assert fwd(flags=_lib.MESH_INTERLEAVED, nrm=None) == ARG                             # and holds normals
        assert fwd(nrm=None) == ARG                                                          # planar normals need nrm
        assert fwd(fi=-1.0) == ARG and fwd(fo=float("inf")) == ARG
        assert fwd(B=0) == SHAPE and fwd(L_max=0) == SHAPE and fwd(Lo=0) == SHAPE
        assert fwd(Lo=13) == SHAPE and b"clip 0" in l.fdm_last_error()                        # 7 frames at 30 -> 60 fps are 14
        assert fwd(fi=0.0, fo=0.0, Lo=6) == SHAPE                                             # pass-through: 7
        assert fwd(L_max=6) == SHAPE and fwd(frames=(C.c_int * B)(7, -1, 4)) == SHAPE
        assert list(got) == [0, 0, 0]                                                         # a refused call writes no length
        if not l.fdm_device_ok():            # (with a device these calls would launch on pointers that are not memory)
            for kw in (dict(), dict(rows=0, tmpl=None), dict(rows=B), dict(flags=0, nrm=None), dict(flags=N | _lib.MESH_F16),
                       dict(flags=N | _lib.MESH_INTERLEAVED | _lib.MESH_F16, nrm=None), dict(frames=None, Lo=14), dict(fi=0.0, fo=0.0, Lo=7)):
                assert fwd(**kw) == STATE and b"no CPU fallback" in l.fdm_last_error(), kw
    finally:
        assert l.fdm_mesh_destroy(h) == 0


def test_python_layer_refuses_the_cpu():
    import torch
    from fdm_amd import pipeline
    faces, V, _ = MC.mesh("grid")
    with pytest.raises(_lib.FdmError):
        mesh.MeshOutPlan(faces, V, device="cpu")
    with pytest.raises(_lib.FdmError):
        pipeline.to_mesh(torch.zeros(1, 2, 3 * V), faces)
    from fdm_amd import presets
    assert presets.get("vocaset").fps == 30 and presets.get("biwi").fps == 25 and presets.get("vocaset_tiny").fps == 30
    assert pipeline._mesh_fps(presets.get("vocaset"), None, None) is None and pipeline._mesh_fps(presets.get("vocaset"), None, 60) == (30.0, 60.0)
    assert pipeline._mesh_fps(presets.get("mead"), 25, 60) == (25.0, 60.0)
    with pytest.raises(ValueError):
        pipeline._mesh_fps(presets.get("mead"), None, 60)


@pytest.mark.parametrize("name", MC.SMALL)
def test_float32_oracle_has_no_subnormals_and_follows_float64(name):
    """The generators' scales keep every float32 intermediate normal (the oracle asserts it), unit normals have unit length, and
    the float32 oracle stays within a few ulp of 1 of the float64 one (figures printed)."""
    faces, V, _ = MC.mesh(name)
    frames = [7, 1, 4]
    off, tmpl = MC.offsets(name, 3, 7, seed=3), MC.template(name, seed=3, rows=3)
    worst = 0.0
    for fps in [None] + MC.RATES:
        o32 = MC.oracle(off, tmpl, frames, fps, faces, V, np.float32)
        o64 = MC.oracle(off, tmpl, frames, fps, faces, V, np.float64)
        for b, L in enumerate(frames):
            p32, n32 = o32[b]
            p64, n64 = o64[b]
            assert p32.dtype == n32.dtype == np.float32 and p32.shape == n32.shape == (MC.frames_out(L, fps), V, 3)
            assert float(np.abs(p32 - p64).max()) <= 2e-7
            worst = max(worst, float(np.abs(n32 - n64).max()))
            length = np.sqrt((n32.astype(np.float64) ** 2).sum(-1))
            live = np.ones(V, dtype=bool)
            if name in MC.ISOLATED:
                live[MC.ISOLATED[name]] = False
                assert np.all(n32[:, MC.ISOLATED[name]] == 0)
            assert np.all(np.abs(length[:, live] - 1) <= 2 * 2.0 ** -23)
    print(f"{name}: max |normal32 - normal64| = {worst:.2e}")
    assert worst <= 1e-4            # conditioning of the thinnest triangles, not a merge bound of the kernels
