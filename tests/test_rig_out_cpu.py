"""No GPU: the host side of the rig hand-off (include/fdm_hip.h, fdm_rig_*) -- the Gram matrix and its Cholesky factor against numpy,
the float32 restatement of the solve (tests/rig_cases.py) against scipy's bounded least squares, every refusal that is decided
before a launch, and the Python layer's argument handling."""
import argparse
import ctypes as C

import numpy as np
import pytest

import rig_cases as RC
from fdm_amd import _lib, rig

ARG, SHAPE, STATE = -1, -2, -4


def test_symbols_are_bound():
    l = _lib.lib()
    for name in ("fdm_rig_gram_host", "fdm_rig_create", "fdm_rig_forward", "fdm_rig_destroy"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_version() == _lib.LIB_VERSION == 105
    assert l.fdm_abi_struct_size(b"fdm_rig") <= 0            # plain arguments: no public struct came with it


@pytest.mark.parametrize("K,V3,weighted", [(1, 3, True), (3, 15, False), (52, 288, True), (128, 1026, True)])
def test_gram_and_factor_against_numpy(K, V3, weighted):
    E, w, ridge = RC.random_rig(K, V3, seed=K, weighted=weighted)
    G, Lc = rig.gram(E, w, ridge)
    E64 = E.astype(np.float64)
    W = np.ones(V3) if w is None else np.repeat(w.astype(np.float64), 3)
    want = (E64 * W) @ E64.T + ridge * np.eye(K)
    mag = (np.abs(E64) * W) @ np.abs(E64).T + ridge * np.eye(K)
    err = np.abs(G - want)
    print(f"K = {K}, 3V = {V3}: max |G - numpy| = {err.max():.2e} (bound at that element {(K * V3 * 2.0 ** -53 * mag).flat[err.argmax()]:.2e})")
    assert np.all(err <= K * V3 * 2.0 ** -53 * mag)
    assert np.array_equal(G, G.T)
    ref = np.linalg.cholesky(want).astype(np.float32)
    assert Lc.dtype == np.float32 and np.all(np.triu(Lc, 1) == 0)
    ulp = np.spacing(np.abs(ref))
    assert np.all(np.abs(Lc.astype(np.float64) - ref.astype(np.float64)) <= ulp)


def _kkt(c, E, w, ridge, d, lo, hi, tol):
    """gradient of the objective at c in fp64, checked by sign against the bounds: >= -tol at lo, <= tol at hi, |.| <= tol inside."""
    E64 = E.astype(np.float64)
    W = np.ones(E.shape[1]) if w is None else np.repeat(w.astype(np.float64), 3)
    c64 = c.astype(np.float64)
    grad = ((c64 @ E64 - d.astype(np.float64)) * W) @ E64.T + ridge * c64
    at_lo, at_hi = c64 <= lo, c64 >= hi
    inside = ~at_lo & ~at_hi
    assert np.all(grad[at_lo] >= -tol) and np.all(grad[at_hi] <= tol) and np.all(np.abs(grad[inside]) <= tol)
    return int(at_lo.sum()), int(at_hi.sum()), int(inside.sum()), float(np.abs(grad[inside]).max())


def test_restatement_solves_the_bounded_problem():
    """K = 52, 3V = 288, random normal basis, ridge = 1e-2 tr(E W E^T) / K, bounds [0, 1], targets with coefficients on each bound:
    the float32 restatement against scipy.optimize.lsq_linear on the augmented system in fp64.  Measured on this case:
    max |c - c_scipy| = 4.2e-07 at 16 sweeps and the same at 64 (converged: what is left is float32 rounding).  The assertion is
    4 x that figure; the margin covers seed-to-seed spread of the rounding, it is not slack for non-convergence."""
    from scipy.optimize import lsq_linear
    K, V3, n = 52, 288, 12
    E, w, ridge = RC.random_rig(K, V3, seed=1)
    d = RC.targets_on_bounds(E, n, seed=1)
    G, Lc = rig.gram(E, w, ridge)
    P = (E.astype(np.float64) * np.repeat(w.astype(np.float64), 3)).astype(np.float32)
    r = (d.astype(np.float64) @ P.astype(np.float64).T).astype(np.float32)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    got = {S: RC.solve(r, G.astype(np.float32), Lc, lo, hi, S) for S in (16, 64)}
    sw = np.sqrt(np.repeat(w.astype(np.float64), 3))
    A = np.concatenate([sw[:, None] * E.astype(np.float64).T, np.sqrt(ridge) * np.eye(K)])
    ref = np.stack([lsq_linear(A, np.concatenate([sw * d[f].astype(np.float64), np.zeros(K)]), bounds=(0.0, 1.0), tol=1e-14).x for f in range(n)])
    e16, e64 = float(np.abs(got[16] - ref).max()), float(np.abs(got[64] - ref).max())
    scale = float(np.abs(G).max())
    # KKT tolerance from the number format: a coefficient in [0, 1] sits within 2^-23 of the fp64 solution's, which moves a gradient
    # component by at most sum_k |G_jk| 2^-23 <= K max|G| 2^-23 (measured: max |grad| inside 1.25e-04 against 2.1e-03)
    lows, highs, ins, gmax = _kkt(got[16], E, w, ridge, d, 0.0, 1.0, tol=K * 2.0 ** -23 * scale)
    print(f"max |c - scipy| = {e16:.2e} at 16 sweeps, {e64:.2e} at 64; {lows} at lo, {highs} at hi, {ins} inside (max |grad| inside {gmax:.2e}, G max {scale:.1f})")
    assert lows > 0 and highs > 0 and ins > 0
    assert e16 <= 4 * 4.2e-7 and e64 <= 4 * 4.2e-7         # measured 4.20e-07 at 16 sweeps, 4.20e-07 at 64


def test_restatement_without_bounds_is_the_normal_equations():
    K, V3 = 52, 288
    E, w, ridge = RC.random_rig(K, V3, seed=2)
    d = RC.targets_on_bounds(E, 5, seed=2)
    G, Lc = rig.gram(E, w, ridge)
    P = (E.astype(np.float64) * np.repeat(w.astype(np.float64), 3))
    r = d.astype(np.float64) @ P.T
    want = np.linalg.solve(G, r.T).T
    got = RC.solve(r.astype(np.float32), G.astype(np.float32), Lc)
    assert float(np.abs(got - want).max()) <= 1e-5
    assert np.array_equal(got, RC.solve(r.astype(np.float32), G.astype(np.float32), Lc, None, None, 0))


def test_create_refusals_and_forward_validation_precede_any_launch():
    """Every refusal is decided before a launch (the device pointers below are never dereferenced).  The object needs no device; a
    call that passes every check on a machine without a GPU ends in FDM_ERR_STATE, never in a fallback."""
    l = _lib.lib()
    K, V = 3, 5
    E, w, ridge = RC.random_rig(K, 3 * V, seed=3)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    h = C.c_void_p()

    def create(basis=E, K=K, V=V, w=w, ridge=ridge, lo=lo, hi=hi, sweeps=16, out=C.byref(h)):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        r = l.fdm_rig_create(p(basis), K, V, p(w), ridge, p(lo), p(hi), sweeps, out)
        if r == 0:
            assert l.fdm_rig_destroy(h) == 0
        return r
    assert create() == 0 and create(w=None) == 0 and create(lo=None, hi=None) == 0 and create(sweeps=0) == 0 and create(ridge=0.0) == 0
    assert create(basis=None) == ARG and create(out=None) == ARG
    assert create(K=0) == ARG and create(K=129) == ARG and create(V=0) == ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert create(ridge=bad) == ARG
        wb = w.copy()
        wb[2] = bad
        assert create(w=wb) == ARG and b"weight 2" in l.fdm_last_error()
    assert create(lo=None) == ARG and create(hi=None) == ARG and b"both" in l.fdm_last_error()
    assert create(lo=np.array([0, 2, 0], np.float32)) == ARG and b"coefficient 1" in l.fdm_last_error()
    assert create(hi=np.array([1, 1, np.inf], np.float32)) == ARG and create(lo=np.array([np.nan, 0, 0], np.float32)) == ARG
    assert create(sweeps=-1) == ARG
    twin = E.copy()
    twin[2] = twin[0]                         # two equal rows, no ridge: the Gram matrix is singular
    assert create(basis=twin, ridge=0.0) == ARG and b"basis is rank deficient under these weights: raise ridge" in l.fdm_last_error()
    assert create(basis=twin, ridge=1e-3) == 0
    assert create(w=np.zeros(V, np.float32), ridge=0.0) == ARG and b"rank deficient" in l.fdm_last_error()
    g, c = np.zeros((K, K)), np.zeros((K, K), np.float32)
    assert l.fdm_rig_gram_host(twin.ctypes.data, None, K, V, 0.0, g.ctypes.data, c.ctypes.data) == ARG
    assert l.fdm_rig_gram_host(E.ctypes.data, None, K, V, 0.0, None, c.ctypes.data) == ARG
    assert l.fdm_rig_gram_host(E.ctypes.data, None, K, V, 0.0, g.ctypes.data, None) == ARG
    assert l.fdm_rig_destroy(None) == 0

    assert l.fdm_rig_create(E.ctypes.data, K, V, w.ctypes.data, ridge, lo.ctypes.data, hi.ctypes.data, 16, C.byref(h)) == 0
    try:
        B, L = 3, 7
        fr = (C.c_int * B)(7, 1, 4)
        got = (C.c_int * B)()

        def fwd(r=h, off=4096, frames=fr, B=B, L_max=L, fi=30.0, fo=60.0, coef=8192, proj=12288, Lo=14, out=got):
            return l.fdm_rig_forward(r, off, frames, B, L_max, fi, fo, coef, proj, Lo, out, None)
        assert fwd(r=None) == ARG and fwd(off=None) == ARG and fwd(coef=None) == ARG
        assert fwd(fi=-1.0) == ARG and fwd(fo=float("inf")) == ARG and fwd(fi=float("nan")) == ARG
        assert fwd(B=0) == SHAPE and fwd(L_max=0) == SHAPE and fwd(Lo=0) == SHAPE
        assert fwd(Lo=13) == SHAPE and b"clip 0" in l.fdm_last_error()                        # 7 frames at 30 -> 60 fps are 14
        assert fwd(fi=0.0, fo=0.0, Lo=6) == SHAPE                                             # pass-through: 7
        assert fwd(L_max=6) == SHAPE and fwd(frames=(C.c_int * B)(7, -1, 4)) == SHAPE
        assert list(got) == [0, 0, 0]                                                         # a refused call writes no length
        if not l.fdm_device_ok():            # (with a device these calls would launch on pointers that are not memory)
            for kw in (dict(), dict(proj=None), dict(frames=None, Lo=14), dict(fi=0.0, fo=0.0, Lo=7), dict(out=None)):
                assert fwd(**kw) == STATE and b"no CPU fallback" in l.fdm_last_error(), kw
    finally:
        assert l.fdm_rig_destroy(h) == 0


def test_python_layer_argument_handling():
    import torch
    from fdm_amd import pipeline
    K, V = 4, 6
    E, w, ridge = RC.random_rig(K, 3 * V, seed=4)
    rf = rig.RigFrames(torch.zeros(1, 2, K), [2], ["a", "b", "c", "d"])
    assert rf.weights.shape == (1, 2, K) and rf.frames == [2] and rf.names[3] == "d" and rf._fields == ("weights", "frames", "names")
    with pytest.raises(_lib.FdmError):
        rig.RigPlan(E, device="cpu")
    with pytest.raises(_lib.FdmError):
        pipeline.to_rig(torch.zeros(1, 2, 3 * V), E)
    for bad in (E[:, :17], E.reshape(-1), np.zeros((0, 18), np.float32)):
        with pytest.raises(_lib.FdmError):
            rig.identity(bad)
    with pytest.raises(_lib.FdmError):
        rig.identity(E, weights=w[:-1])
    with pytest.raises(_lib.FdmError):
        rig.identity(E, names=["a"])
    with pytest.raises(_lib.FdmError):
        rig.RigPlan(E, bounds=(1.0, 0.0))                                  # lo > hi: the library refuses it
    a = rig.identity(E, w, ridge, (0, 1), 16, None)
    assert a == rig.identity(torch.from_numpy(E).reshape(K, V, 3), torch.from_numpy(w), ridge, (np.zeros(K), np.ones(K)), 16)
    assert a != rig.identity(E, w, ridge, (0, 1), 8) and a != rig.identity(E, None, ridge, (0, 1), 16) and a[:2] == (K, V)
    plan = rig.RigPlan(E, w, ridge, (0, 1), names="abcd")                  # no device needed to make (and validate) one
    assert plan.key == rig.identity(**plan.arguments()) and plan.names == ["a", "b", "c", "d"] and (plan.K, plan.V) == (K, V)
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            plan.forward(torch.zeros(1, 2, 3 * V))


def test_demo_flag_parser(tmp_path):
    from fdm_amd import pipeline
    K, V = 4, 6
    E, w, _ = RC.random_rig(K, 3 * V, seed=5)
    ap = argparse.ArgumentParser()
    pipeline.add_rig_arguments(ap)
    assert pipeline.rig_arguments(ap.parse_args([])) is None
    full, bare, half = tmp_path / "full.npz", tmp_path / "bare.npz", tmp_path / "half.npz"
    np.savez(full, basis=E, names=np.array(["jawOpen", "b", "c", "d"]), weights=w, lo=np.zeros(K, np.float32), hi=np.ones(K, np.float32))
    np.savez(bare, basis=E)
    np.savez(half, basis=E, lo=np.zeros(K, np.float32))
    kw = pipeline.rig_arguments(ap.parse_args(["--rig_file", str(full), "--rig_ridge", "0.5", "--rig_sweeps", "4"]))
    assert sorted(kw) == ["basis", "bounds", "names", "ridge", "sweeps", "weights"]
    assert np.array_equal(kw["basis"], E) and np.array_equal(kw["weights"], w) and kw["names"][0] == "jawOpen"
    assert kw["ridge"] == 0.5 and kw["sweeps"] == 4 and np.array_equal(kw["bounds"][1], np.ones(K))
    assert rig.identity(**kw) == rig.identity(E, w, 0.5, (0, 1), 4, ["jawOpen", "b", "c", "d"])
    kw = pipeline.rig_arguments(ap.parse_args(["--rig_file", str(bare)]))
    assert kw["weights"] is None and kw["bounds"] is None and kw["names"] is None and kw["ridge"] == 0.0 and kw["sweeps"] == 16
    with pytest.raises(ValueError):
        pipeline.rig_arguments(ap.parse_args(["--rig_file", str(half)]))
