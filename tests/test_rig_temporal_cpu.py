"""No GPU: the host side of the temporal rig fit (include/fdm_hip.h, fdm_rig_temporal_tables_host / fdm_rig_set_temporal; DESIGN.md
section 2 item 21) -- the Jacobi tables against numpy.linalg.eigh, their order and sign rule, every refusal, the float32 restatement
(tests/rig_temporal_cases.py) against fp64 solves of the stacked system, and that the fit smooths."""
import argparse
import ctypes as C

import numpy as np
import pytest

import rig_cases as RC
import rig_temporal_cases as TC
from fdm_amd import _lib, rig

ARG = -1
MUS = (0.1, 1.0, 10.0)                # x tr(G) / K


def case_gram(K, V3, seed):
    E, w, ridge = RC.random_rig(K, V3, seed=seed)
    G, _ = rig.gram(E, w, ridge)
    return E, w, ridge, G


def test_symbols_are_bound_and_the_version_stays():
    l = _lib.lib()
    for name in ("fdm_rig_temporal_tables_host", "fdm_rig_set_temporal"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_version() == _lib.LIB_VERSION == 105          # the feature is detected by the symbol


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,V3", [(1, 3), (3, 15), (52, 288), (128, 1026)])
def test_tables_against_eigh(K, V3, weighted):
    """max |Q^T G Q - diag(lam)| and max |Q^T M Q - I| relative to max |G|, against the same two quantities of numpy.linalg.eigh on
    D G D.  Jacobi and LAPACK are both backward stable; 16 x eigh's own figure covers their different constants.  Measured at
    mu = tr(G) / K, the first quantity then the second, the library's Jacobi | eigh (unweighted; weighted smoothing):
      K = 1    0, 3.9e-17 | 0, 3.9e-17;              0, 0 | 0, 0
      K = 3    1.3e-17, 1.4e-17 | 1.2e-17, 2.5e-17;  5.0e-17, 1.2e-17 | 5.0e-17, 2.5e-17
      K = 52   9.1e-18, 1.3e-18 | 4.4e-18, 4.1e-18;  9.2e-18, 1.6e-18 | 8.3e-18, 6.7e-18
      K = 128  3.5e-18, 9.5e-19 | 2.1e-18, 1.5e-18;  9.0e-18, 5.7e-19 | 2.3e-18, 2.3e-18"""
    _, _, _, G = case_gram(K, V3, seed=K)
    mu = float(np.trace(G)) / K
    m = (0.5 + np.random.default_rng(K).random(K)).astype(np.float32) if weighted else None
    lam, Q = rig.temporal_tables(G, mu, m)
    M = mu * np.diag(np.ones(K) if m is None else m.astype(np.float64))
    D = np.diag(1.0 / np.sqrt(np.diag(M)))
    lam_ref, U = np.linalg.eigh(D @ G @ D)
    Q_ref = D @ U
    scale = float(np.abs(G).max())

    def figures(lam, Q):
        return float(np.abs(Q.T @ G @ Q - np.diag(lam)).max()) / scale, float(np.abs(Q.T @ M @ Q - np.eye(K)).max()) / scale
    got, ref = figures(lam, Q), figures(lam_ref, Q_ref)
    print(f"K = {K}, weighted = {weighted}: Jacobi {got[0]:.2e}, {got[1]:.2e}; eigh {ref[0]:.2e}, {ref[1]:.2e}")
    assert got[0] <= 16 * ref[0] and got[1] <= 16 * ref[1]
    assert np.all(np.diff(lam) >= 0) and np.all(lam > 0)                               # ascending
    assert np.all(np.abs(lam - lam_ref) <= 1e-12 * lam_ref.max())
    U_got = Q / np.diag(D)[:, None]                                                     # sign: the largest-magnitude entry is positive
    big = np.abs(U_got).argmax(axis=0)
    assert np.all(U_got[big, np.arange(K)] > 0)


def test_refusals_and_set_temporal_without_a_device():
    l = _lib.lib()
    K, V = 3, 5
    E, w, ridge, G = case_gram(K, 3 * V, seed=3)
    lam, Q = np.zeros(K), np.zeros((K, K))
    m = np.ones(K, np.float32)

    def tables(gram=G, K=K, mu=1.0, m=m, lam=lam, Q=Q):
        p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return l.fdm_rig_temporal_tables_host(p(gram), K, mu, p(m), p(lam), p(Q))
    assert tables() == 0 and tables(m=None) == 0
    assert tables(gram=None) == ARG and tables(lam=None) == ARG and tables(Q=None) == ARG
    assert tables(K=0) == ARG and tables(K=129) == ARG
    for bad in (-1.0, float("nan"), float("inf"), 0.0):
        assert tables(mu=bad) == ARG
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        mb = m.copy()
        mb[1] = bad
        assert tables(m=mb) == ARG and b"weight 1" in l.fdm_last_error()
    assert tables(gram=-G) == ARG and b"eigenvalue" in l.fdm_last_error()               # not positive definite
    h = C.c_void_p()
    assert l.fdm_rig_create(E.ctypes.data, K, V, w.ctypes.data, ridge, None, None, 16, C.byref(h)) == 0
    try:
        assert l.fdm_rig_set_temporal(None, 1.0, None) == ARG
        assert l.fdm_rig_set_temporal(h, 1.0, None) == 0 and l.fdm_rig_set_temporal(h, 1.0, m.ctypes.data) == 0
        for bad in (-1.0, float("nan"), float("inf")):
            assert l.fdm_rig_set_temporal(h, bad, None) == ARG
        mb = m.copy()
        mb[2] = 0.0
        assert l.fdm_rig_set_temporal(h, 1.0, mb.ctypes.data) == ARG and l.fdm_rig_set_temporal(h, 0.0, mb.ctypes.data) == ARG
        assert l.fdm_rig_set_temporal(h, 1e-60, None) == ARG                              # eigenvalues past fp32
        assert l.fdm_rig_set_temporal(h, 0.0, None) == 0                                  # back to the per-frame path
    finally:
        assert l.fdm_rig_destroy(h) == 0


def test_python_layer_takes_the_new_keywords_last():
    import inspect
    from fdm_amd import pipeline
    K, V = 4, 6
    E, w, ridge = RC.random_rig(K, 3 * V, seed=4)
    for fn in (rig.identity, rig._arguments, rig.RigPlan.__init__, pipeline.to_rig):
        assert list(inspect.signature(fn).parameters)[-2:] == ["smooth", "smooth_weights"]
    base = rig.identity(E, w, ridge, (0, 1), 16, None)
    assert base == rig.identity(E, w, ridge, (0, 1), 16, None, 0.0, None)               # a per-frame rig keeps its identity
    a = rig.identity(E, w, ridge, (0, 1), 16, None, smooth=2.0)
    assert a != base and a != rig.identity(E, w, ridge, (0, 1), 16, None, smooth=3.0)
    assert a != rig.identity(E, w, ridge, (0, 1), 16, None, smooth=2.0, smooth_weights=np.full(K, 2.0))
    plan = rig.RigPlan(E, w, ridge, (0, 1), smooth=2.0, smooth_weights=np.ones(K))        # no device needed to make and validate one
    assert plan.key == rig.identity(**plan.arguments()) and plan.smooth == 2.0 and plan.arguments()["smooth_weights"].dtype == np.float32
    with pytest.raises(_lib.FdmError):
        rig.RigPlan(E, w, ridge, smooth=-1.0)
    with pytest.raises(_lib.FdmError):
        rig.RigPlan(E, w, ridge, smooth=1.0, smooth_weights=np.zeros(K))
    with pytest.raises(_lib.FdmError):
        rig.identity(E, smooth=1.0, smooth_weights=np.ones(K + 1))
    with pytest.raises(_lib.FdmError):
        plan.set_temporal(float("nan"))
    assert plan.smooth == 2.0                                                           # a refused call leaves the plan as it was
    plan.set_temporal(0.0)
    assert plan.key == base and plan.smooth == 0.0
    with pytest.raises(_lib.FdmError):
        rig.temporal_tables(np.zeros((3, 2)), 1.0)


def test_demo_flag_parser_takes_rig_smooth(tmp_path):
    from fdm_amd import pipeline
    K, V = 4, 6
    E, _, _ = RC.random_rig(K, 3 * V, seed=5)
    ap = argparse.ArgumentParser()
    pipeline.add_rig_arguments(ap)
    with_m, bare = tmp_path / "with_m.npz", tmp_path / "bare.npz"
    m = np.linspace(1, 2, K).astype(np.float32)
    np.savez(with_m, basis=E, smooth_weights=m)
    np.savez(bare, basis=E)
    kw = pipeline.rig_arguments(ap.parse_args(["--rig_file", str(with_m), "--rig_smooth", "0.5"]))
    assert kw["smooth"] == 0.5 and np.array_equal(kw["smooth_weights"], m)
    assert rig.identity(**kw) == rig.identity(E, smooth=0.5, smooth_weights=m)
    kw = pipeline.rig_arguments(ap.parse_args(["--rig_file", str(bare), "--rig_smooth", "0.5"]))
    assert kw["smooth"] == 0.5 and kw["smooth_weights"] is None
    assert "smooth" not in pipeline.rig_arguments(ap.parse_args(["--rig_file", str(with_m)]))


# ---- the restatement against fp64
def projections(E, w, d):
    P = (E.astype(np.float64) * np.repeat(w.astype(np.float64), 3)).astype(np.float32)
    return (d.astype(np.float64) @ P.astype(np.float64).T).astype(np.float32)


UNBOUNDED = {0.1: 6.3e-7, 1.0: 5.3e-7, 10.0: 1.6e-6}          # measured max |c - fp64| on the case below, O(1) coefficients


def test_restatement_without_bounds_is_the_stacked_solve():
    """K = 52, 3V = 288, Lo = 40: the float32 modal + tridiagonal solve against a dense fp64 solve of the stacked system built from
    the same float32 G and r.  The assertion is 4 x the measured figure (item 19's convention: the margin covers seed-to-seed spread
    of the rounding)."""
    K, V3, Lo = 52, 288, 40
    E, w, ridge, d = TC.smooth_case(K, V3, Lo, seed=1)
    G, _ = rig.gram(E, w, ridge)
    r = projections(E, w, d)
    G32 = G.astype(np.float32)
    for x, measured in UNBOUNDED.items():
        mu = x * float(np.trace(G)) / K
        got = TC.solve(r, G32, TC.tables32(G, mu))
        want = np.linalg.solve(TC.stacked(G32.astype(np.float64), mu * np.eye(K), Lo), r.astype(np.float64).reshape(-1)).reshape(Lo, K)
        err = float(np.abs(got - want).max())
        print(f"mu = {x} tr(G)/K: max |c - fp64| = {err:.2e} (max |c| = {np.abs(want).max():.2f})")
        assert err <= 4 * measured


BOUNDED = {(0.1, 16): 2.3e-7, (0.1, 64): 2.3e-7, (1.0, 16): 2.8e-5, (1.0, 64): 4.8e-7, (10.0, 16): 2.1e-2, (10.0, 64): 3.9e-4}      # measured


def test_restatement_with_bounds_against_scipy_on_the_stacked_system():
    """K = 12, 3V = 96, Lo = 24, bounds [0, 1], targets with coefficients on both bounds: the float32 restatement at S = 16 and 64
    against scipy.optimize.lsq_linear on the stacked system in fp64 (H = R^T R: minimise 1/2 |R c - R^-T r|^2).  The distances
    are the convergence table of DESIGN item 21: strong smoothing converges more slowly, and the figure at mu = 10 tr(G)/K is what
    the sweeps have left, not rounding.  Each assertion is 4 x its measured figure."""
    from scipy.optimize import lsq_linear
    K, V3, Lo = 12, 96, 24
    E, w, ridge, d = TC.smooth_case(K, V3, Lo, seed=2)
    G, _ = rig.gram(E, w, ridge)
    r = projections(E, w, d)
    G32 = G.astype(np.float32)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    for x in MUS:
        mu = x * float(np.trace(G)) / K
        R = np.linalg.cholesky(TC.stacked(G32.astype(np.float64), mu * np.eye(K), Lo)).T
        ref = lsq_linear(R, np.linalg.solve(R.T, r.astype(np.float64).reshape(-1)), bounds=(0.0, 1.0), tol=1e-14).x.reshape(Lo, K)
        assert (ref <= 1e-12).any() and (ref >= 1 - 1e-12).any()
        tables = TC.tables32(G, mu)
        for S in (16, 64):
            err = float(np.abs(TC.solve(r, G32, tables, lo, hi, S) - ref).max())
            print(f"mu = {x} tr(G)/K, {S} sweeps: max |c - scipy| = {err:.2e}")
            assert err <= 4 * BOUNDED[(x, S)]


def test_it_smooths():
    """The second-difference energy of the curves falls monotonically over mu = 0.1, 1, 10 x tr(G) / K and is below the per-frame
    fit's; the stacked objective at the temporal fit is below the per-frame solution's (it is that objective's minimiser)."""
    K, V3, Lo = 52, 288, 40
    E, w, ridge, d = TC.smooth_case(K, V3, Lo, seed=3)
    G, Lc = rig.gram(E, w, ridge)
    r = projections(E, w, d)
    G32 = G.astype(np.float32)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    for bounds in ((None, None), (lo, hi)):
        frame = RC.solve(r, G32, Lc, *bounds, 16)
        bends = [TC.bend(frame)]
        for x in MUS:
            mu = x * float(np.trace(G)) / K
            c = TC.solve(r, G32, TC.tables32(G, mu), *bounds, 16)
            M = mu * np.eye(K)
            assert TC.objective(c, r, G, M) < TC.objective(frame, r, G, M)
            bends.append(TC.bend(c))
        print(f"bounded = {bounds[0] is not None}: second-difference energy per-frame {bends[0]:.3g}, temporal {bends[1]:.3g}, {bends[2]:.3g}, {bends[3]:.3g}")
        assert bends[0] > bends[1] > bends[2] > bends[3]
