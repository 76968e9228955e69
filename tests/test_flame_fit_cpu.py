"""CPU: the numpy restatements of the parametric-head fit (tests/flame_fit_cases.py) against each other and against known parameters,
the Python argument refusals, and the binding table against the header.  No device is needed; the host tables come from the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import flame_fit_cases as K
from fdm_amd import _lib, flame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = ("v3_none", "v5_none", "v255_j2", "v257_jaw", "v513_all") + K.STEP_EXTRA      # the fp32 restatement walks the elements one by one: small V here


def _targets(name, dt=np.float64):
    c, m, r = K.truth_rows(name)
    y = K.forward(m, r["sh"], r["ex"], r["ps"], r["tr"] if c["transl"] else None, dt)["out"]
    return c, m, r, y


@pytest.mark.parametrize("name", K.SMALL + ("full",))
def test_fp64_restatement_recovers_known_parameters(name):
    """the condition on the choice of cases: within the default iters the vertex RMS is under 1e-6 of the bounding-box diagonal"""
    c, m, r, y = _targets(name)
    o = K.fit(m, y, r["sh"], r["p0"], c["free"], c["n_expr"], c["transl"], np.float64)
    assert o["status"].max() == 0
    print(name, "rms / diagonal", float(o["rms"].max() / K.bbox_diag(m)), "max |theta - truth|", float(np.abs(o["theta"] - r["theta"]).max()))
    assert o["rms"].max() < 1e-6 * K.bbox_diag(m)
    assert np.abs(o["theta"] - r["theta"]).max() < 1e-6


@pytest.mark.parametrize("name", CPU_CASES)
def test_fp32_and_fp64_restatements_agree_on_one_step(name):
    """H, g within step_bounds and delta within solve_bound, from a non-trivial theta (half way to the truth)"""
    c, m, r, y = _targets(name)
    free, ne, tr = c["free"], c["n_expr"], c["transl"]
    P, lam = K.n_params(c), K.step_lam(c)
    theta0 = K.join(np.zeros_like(r["ex"]), r["p0"], np.zeros_like(r["tr"]), free, tr).astype(np.float64)
    theta = (0.5 * (theta0 + r["theta"])).astype(np.float32)
    y32 = y.astype(np.float32)
    d64, s64, p64 = K.step(m, theta, y32, r["sh"], r["p0"], free, ne, tr, np.float64, lam=lam, parts=True)
    d32, s32, p32 = K.step(m, theta, y32, r["sh"], r["p0"], free, ne, tr, np.float32, lam=lam, parts=True)
    assert s64.max() == 0 and s32.max() == 0
    ex, ps, _ = K.split(theta, r["p0"], free, ne, tr)
    e_pose, e_deriv = K.deriv_bound(m, r["sh"], ex, ps, free, ne)
    dG = K.step_bounds(m, p64, y32.astype(np.float64), None, free, ne, tr, r["sh"].shape[1], e_pose, e_deriv)
    err = np.abs(np.triu(p32["G"].astype(np.float64) - p64["G"]))
    print(name, "max err / bound", float((err / np.maximum(np.triu(dG), 1e-300)).max()))
    assert np.all(err <= np.triu(dG))
    H64, g64 = K.full_sym(p64["G"], P)
    A64 = H64 + np.eye(P)[None] * lam
    dH, dg = K.full_sym(dG, P)
    bound = K.solve_bound(A64, -g64, d64, dH, dg, P)
    dd = np.linalg.norm(d32.astype(np.float64) - d64, axis=1)
    print(name, "max |delta32 - delta64| / bound", float((dd / bound).max()))
    assert np.all(dd <= bound)


def test_one_step_without_joints_is_the_normal_equations_solution():
    """no free joint, pose0 = 0, lambda = 0: F is affine in the expression, one step lands on the fp64 least-squares solution"""
    c, m, r = K.truth_rows("v5_none")
    p0 = np.zeros_like(r["p0"])
    ne = c["n_expr"]
    y = K.forward(m, r["sh"], r["ex"], p0, None, np.float64)["out"] + 1e-3 * np.random.default_rng(3).standard_normal((len(r["b"]), m.V, 3))
    theta = np.zeros((len(r["b"]), ne))
    d, st = K.step(m, theta, y, r["sh"], p0, (), ne, False, np.float64, lam=0.0)
    f0 = K.forward(m, r["sh"], np.zeros_like(r["ex"]), p0, None, np.float64)["out"]
    for i in range(len(r["b"])):
        cols = np.stack([(K.forward(m, r["sh"][i:i + 1], np.eye(ne)[k:k + 1], p0[i:i + 1], None, np.float64)["out"] - f0[i:i + 1]).reshape(-1) for k in range(ne)], 1)
        ref = np.linalg.lstsq(cols, (y[i] - f0[i]).reshape(-1), rcond=None)[0]
        assert np.abs(d[i] - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())


def test_degenerate_weights_fail_in_the_restatement():
    """all but one weight zero with lambda = rho = 0: rank 3 < P, the pivot rule flags every row and leaves theta"""
    c, m, r, y = _targets("v257_jaw")
    mw = np.zeros(m.V)
    mw[11] = 1.0
    o = K.fit(m, y, r["sh"], r["p0"], c["free"], c["n_expr"], c["transl"], np.float64, iters=2, mw=mw, lam=0.0)
    assert np.all(o["status"] > 0)
    assert np.array_equal(o["theta"], K.join(np.zeros_like(r["ex"]), r["p0"], np.zeros_like(r["tr"]), c["free"], c["transl"]).astype(np.float64))


def test_python_refusals():
    c, m, _ = K.case("v257_jaw")
    with pytest.raises(flame.FdmError, match="twice"):
        flame.fit_joints(("jaw", 2), 5)
    with pytest.raises(flame.FdmError, match="out of range"):
        flame.fit_joints((5,), 5)
    with pytest.raises(flame.FdmError, match="5-joint"):
        flame.fit_joints(("jaw",), 2)
    assert flame.fit_joints(("jaw", "neck"), 5) == (1, 2)
    plan = flame.FlamePlan(m)
    NE = m.NB - m.expr_at
    with pytest.raises(flame.FdmError, match="n_expr"):
        plan.fit_plan(n_expr=NE + 1)
    with pytest.raises(flame.FdmError, match="weights"):
        plan.fit_plan(n_expr=3, weights=np.zeros(m.V))
    with pytest.raises(flame.FdmError, match="weights"):
        plan.fit_plan(n_expr=3, weights=-np.ones(m.V))
    fp = plan.fit_plan(n_expr=3, joints=("jaw",))
    assert fp.P == 6 and fp.columns()[3] == ("pose", 6)
    for kw in (dict(iters=0), dict(lam=-1.0), dict(ridge_expr=-1e-3), dict(ridge_pose=float("inf"))):
        with pytest.raises(flame.FdmError):
            fp.set(**kw)
    big = flame.FlamePlan(K.case("v257_p128")[1])
    with pytest.raises(flame.FdmError, match="P = "):
        big.fit_plan(n_expr=111, joints=(0, 1, 2, 3, 4), transl=True)
    assert big.fit_plan(n_expr=110, joints=(0, 1, 2, 3, 4), transl=True).P == 128


def test_c_refusals_without_a_device():
    """fdm_flame_fit_create / _set validate on the host; the messages name the argument"""
    l = _lib.lib()
    c, m, _ = K.case("v257_jaw")
    plan = flame.FlamePlan(m)
    h = C.c_void_p()

    def create(joints, n_expr, transl, w=None):
        fj = (C.c_int * max(1, len(joints)))(*joints)
        return l.fdm_flame_fit_create(plan.h, fj, len(joints), n_expr, transl, None if w is None else w.ctypes.data, C.byref(h))
    assert create((2, 2), 3, 0) == -1 and b"twice" in l.fdm_last_error()
    assert create((7,), 3, 0) == -1 and b"out of range" in l.fdm_last_error()
    assert create((), m.NB - m.expr_at + 1, 0) == -1 and b"n_expr" in l.fdm_last_error()
    assert create((), 0, 0) == -1 and b"P = 0" in l.fdm_last_error()
    w = np.zeros(m.V, np.float32)
    assert create((2,), 3, 0, w) == -1 and b"all zero" in l.fdm_last_error()
    w[3] = -1
    assert create((2,), 3, 0, w) == -1 and b"vertex_weights[3]" in l.fdm_last_error()
    assert create((2,), 3, 1) == 0
    for key, v in ((b"iters", 0.0), (b"iters", 2.5), (b"lambda", -1.0), (b"ridge_expr", -1.0), (b"ridge_pose", float("nan")), (b"nope", 1.0)):
        assert l.fdm_flame_fit_set(h, key, v) == -1, key
    assert l.fdm_flame_fit_set(h, b"iters", 3.0) == 0 and l.fdm_flame_fit_set(h, b"lambda", 0.0) == 0
    assert l.fdm_flame_fit_destroy(h) == 0
    big = flame.FlamePlan(K.case("v257_p128")[1])
    fj = (C.c_int * 5)(0, 1, 2, 3, 4)
    assert l.fdm_flame_fit_create(big.h, fj, 5, 110, 1, None, C.byref(h)) == 0 and l.fdm_flame_fit_destroy(h) == 0      # P = 128: the edge
    assert l.fdm_flame_fit_create(big.h, fj, 5, 111, 1, None, C.byref(h)) == -1 and b"P = 129" in l.fdm_last_error()


def test_binding_matches_the_header():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fdm_hip.h")).read(), flags=re.S)
    for name in ("fdm_flame_fit_create", "fdm_flame_fit_set", "fdm_flame_fit_forward", "fdm_flame_fit_step", "fdm_flame_fit_destroy"):
        decl = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)", src).group(1)
        args = [a.strip() for a in decl.split(",")]
        res, types = _lib.SYMBOLS[name]
        assert res is _lib.ci and len(types) == len(args), name
        for a, t in zip(args, types):
            if "**" in a:
                assert t is C.POINTER(_lib.vp) or t == C.POINTER(_lib.vp), (name, a)
            elif "char" in a:
                assert t is C.c_char_p, (name, a)
            elif "*" in a:
                assert t is _lib.vp, (name, a)
            elif a.startswith("double"):
                assert t is C.c_double, (name, a)
            else:
                assert a.startswith("int ") and t is _lib.ci, (name, a)
    assert _lib.lib().fdm_version() == _lib.LIB_VERSION == 105          # the feature is detected by the symbols
