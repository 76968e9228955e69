"""No GPU: the host side of the parametric-head hand-off (include/fdm_hip.h, fdm_flame_*) -- the fp64 restatement of
tests/flame_cases.py against closed forms (so that the yardstick of the GPU tests is itself checked), fdm_flame_tables_host against
numpy, every refusal with its message, create without a device, and the Python layer (torch2mesh's pose mapping and rounding, the
reference-shaped FLAME class, FlameModel.load)."""
import ctypes as C
import inspect
import os
import pickle
import sys

import numpy as np
import pytest
import torch

import flame_cases as FC
from fdm_amd import _lib, flame

ARG, SHAPE, STATE = -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rotation(r):
    """exp of the skew matrix of r: scipy's from_rotvec if importable, else the series"""
    try:
        from scipy.spatial.transform import Rotation
        return Rotation.from_rotvec(np.asarray(r, np.float64)).as_matrix()
    except ImportError:
        x, y, z = (float(v) for v in r)
        K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
        out, term = np.eye(3), np.eye(3)
        for i in range(1, 60):
            term = term @ K / i
            out = out + term
        return out


def one_clip(m, pose, expr=None, shape=None):
    L = pose.shape[0]
    z = lambda n: np.zeros((1, L, n), np.float32)  # noqa: E731
    return dict(shape=np.zeros((1, 0), np.float32) if shape is None else shape.reshape(1, -1), expr=z(0) if expr is None else expr[None],
                pose=pose[None].astype(np.float32), transl=None, extra=None, frames=[L], lv=None, lb=None)


def test_symbols_and_struct_are_bound():
    l = _lib.lib()
    for name in ("fdm_flame_tables_host", "fdm_flame_create", "fdm_flame_forward", "fdm_flame_destroy"):
        assert name in _lib.SYMBOLS and hasattr(l, name)
    assert l.fdm_version() == _lib.LIB_VERSION == 105
    assert l.fdm_abi_struct_size(b"fdm_flame_model") == C.sizeof(_lib.FlameModelDesc) == 64


def test_zero_pose_gives_template_plus_blend_exactly():
    m = flame.FlameModel.synthetic(40, 5, 7, 4, seed=1)
    g = np.random.default_rng(2)
    sh, ex = g.standard_normal(4).astype(np.float32), g.standard_normal((3, 3)).astype(np.float32)
    r = FC.restate(m, one_clip(m, np.zeros((3, 15)), ex, sh), np.float64)
    D = FC.tables64(m)[0]
    want = m.v_template.reshape(1, -1).astype(np.float64) + sh.astype(np.float64) @ D[:4] + ex.astype(np.float64) @ D[4:7]
    assert np.array_equal(r["posefeat"], np.zeros((3, 36)))
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(12)
    assert np.abs(r["xforms"] - eye).max() <= 1e-15                # R = I exactly; t = Jf - I Jf
    wsum = np.repeat(m.lbs_weights.astype(np.float64).sum(1), 3)[None]   # float32 weights sum to 1 within 2^-24: T = (sum w) I
    assert np.abs(wsum - 1).max() <= 4 * 2.0 ** -24
    assert np.abs(r["verts"].reshape(3, -1) - wsum * want).max() <= 1e-15


@pytest.mark.parametrize("rot", [(0.3, -0.2, 0.5), (0.0, np.pi / 2, 0.0), (2.0, -2.5, 1.5)])
def test_all_weight_on_the_root_is_a_rigid_rotation_about_the_root_joint(rot):
    m = flame.FlameModel.synthetic(30, 3, 2, 1, seed=3, parents=[0, 0, 1])
    m.lbs_weights[:] = 0
    m.lbs_weights[:, 0] = 1
    m.posedirs[:] = 0
    pose = np.zeros((1, 9))
    pose[0, :3] = rot
    pose[0, 3:] = 0.4                                              # the other joints turn: with no weight they move nothing
    r = FC.restate(m, one_clip(m, pose), np.float64)
    J0 = m.j_regressor[0].astype(np.float64) @ m.v_template.astype(np.float64)
    R = rotation(np.asarray(rot, np.float32))
    want = (m.v_template.astype(np.float64) - J0) @ R.T + J0
    assert np.abs(r["verts"][0] - want).max() <= 1e-7             # (the rule's 1e-8 in the angle moves a unit-scale vertex by ~1e-8)


def test_two_joint_chain_is_the_hand_composition():
    m = flame.FlameModel.synthetic(20, 2, 0, 0, seed=4, parents=[0, 0])
    m.posedirs[:] = 0
    pose = np.array([[0.2, 0.1, -0.3, -0.5, 0.4, 0.1]])
    r = FC.restate(m, one_clip(m, pose), np.float64)
    vt, jr, w = (a.astype(np.float64) for a in (m.v_template, m.j_regressor, m.lbs_weights))
    J0, J1 = jr[0] @ vt, jr[1] @ vt
    R0, R1 = rotation(pose[0, :3].astype(np.float32)), rotation(pose[0, 3:].astype(np.float32))
    p0 = (vt - J0) @ R0.T + J0                                     # about the root
    p1 = ((vt - J1) @ R1.T + (J1 - J0)) @ R0.T + J0                # about the child, then carried by the root
    want = w[:, :1] * p0 + w[:, 1:] * p1
    assert np.abs(r["verts"][0] - want).max() <= 1e-7
    assert np.abs(r["posefeat"][0].reshape(3, 3) - (R1 - np.eye(3))).max() <= 1e-7


def test_folded_joints_equal_the_regressor_on_the_shaped_vertices():
    c, m, inp = FC.case("v771")
    D, JT, JD = FC.tables64(m)
    b, t, sh, ex, _ = FC._rows(m, inp)
    folded = JT.reshape(1, -1) + sh.astype(np.float64) @ JD[:sh.shape[1]] + ex.astype(np.float64) @ JD[m.expr_at:m.expr_at + ex.shape[1]]
    direct = FC.restate(m, inp, np.float64)["joints"]
    assert np.abs(folded - direct).max() <= 1e-13
    r32 = FC.restate(m, inp, np.float32)
    assert np.abs(r32["joints"] - direct).max() <= (sh.shape[1] + ex.shape[1] + 2) * 2.0 ** -24 * (np.abs(JT).max() + np.abs(sh).sum(1).max() * np.abs(JD).max() + np.abs(ex).sum(1).max() * np.abs(JD).max())


@pytest.mark.parametrize("name", ["v3", "v15", "v765", "v771"])
def test_tables_against_numpy(name):
    c, m, inp = FC.case(name)
    D, JT, JD = m.tables()
    D64, JT64, JD64 = FC.tables64(m)
    assert np.array_equal(D, D64.astype(np.float32))               # a transposition: exact
    for got, want in ((JT, JT64), (JD, JD64)):                      # fp64 sums in another order, rounded once: within one fp32 ulp
        w32 = want.astype(np.float32)
        assert got.shape == w32.shape and np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(w32)))
        assert got.size == 0 or np.mean(got == w32) > 0.99


def test_pose_error_table_is_current():
    """E of the docstring table of flame_cases.py, recomputed (the full-size case is left to the GPU file)."""
    for name in FC.CASES:
        c, m, inp = FC.case(name)
        e, _ = FC.pose_error(m, inp)
        print(f"{name}: E = {e:.2e}")
        assert FC.E_TABLE[name] / 2 <= e <= FC.E_TABLE[name] * 2


def _create(l, m, h, lv=None, lb=None, NL=0, **over):
    d = m.desc()
    for k, v in over.items():
        setattr(d, k, v)
    r = l.fdm_flame_create(C.byref(d), None if lv is None else lv.ctypes.data, None if lb is None else lb.ctypes.data, NL, C.byref(h))
    if r == 0:
        assert l.fdm_flame_destroy(h) == 0
    return r


def test_create_refusals_name_the_field():
    l = _lib.lib()
    m = flame.FlameModel.synthetic(12, 3, 5, 2, seed=5, parents=[0, 0, 1])
    h = C.c_void_p()
    assert _create(l, m, h) == 0
    for field in ("v_template", "shapedirs", "posedirs", "j_regressor", "parents", "lbs_weights"):
        assert _create(l, m, h, **{field: None}) == ARG and b"null " + field.encode() in l.fdm_last_error()
    d = m.desc()
    assert l.fdm_flame_create(C.byref(d), None, None, 0, None) == ARG and l.fdm_flame_create(None, None, None, 0, C.byref(h)) == ARG
    for over, msg in ((dict(J=0), b"J = 0"), (dict(J=9), b"J = 9"), (dict(NB=-1), b"NB = -1"), (dict(NB=513), b"NB = 513"), (dict(V=0), b"V = 0"),
                      (dict(expr_at=6), b"expr_at = 6"), (dict(expr_at=-1), b"expr_at")):
        assert _create(l, m, h, **over) == ARG and msg in l.fdm_last_error(), over
    for bad, msg in (([0, 1, 1], b"parents[1] = 1"), ([0, 0, 2], b"parents[2] = 2"), ([0, -1, 0], b"parents[1] = -1")):
        p = np.asarray(bad, np.int32)
        assert _create(l, m, h, parents=p.ctypes.data) == ARG and msg in l.fdm_last_error()
    for field in ("v_template", "shapedirs", "posedirs", "j_regressor", "lbs_weights"):
        for bad in (np.nan, np.inf):
            a = getattr(m, field).copy()
            a.reshape(-1)[3] = bad
            assert _create(l, m, h, **{field: a.ctypes.data}) == ARG and field.encode() + b" element 3" in l.fdm_last_error()
    lv, lb = np.array([[0, 1, 2], [3, 4, 11]], np.int32), np.full((2, 3), 1 / 3, np.float32)
    assert _create(l, m, h, lv, lb, 2) == 0
    assert _create(l, m, h, None, lb, 2) == ARG and _create(l, m, h, lv, None, 2) == ARG and b"lmk" in l.fdm_last_error()
    assert _create(l, m, h, lv, lb, 257) == ARG and _create(l, m, h, lv, lb, -1) == ARG and b"NL" in l.fdm_last_error()
    assert _create(l, m, h, np.array([[0, 1, 12]], np.int32), lb, 1) == ARG and b"lmk_verts element 2 = 12" in l.fdm_last_error()
    assert _create(l, m, h, lv, np.full((2, 3), np.nan, np.float32), 2) == ARG and b"lmk_bary" in l.fdm_last_error()
    D, JT, JD = np.zeros((5 + 18, 36), np.float32), np.zeros((3, 3), np.float32), np.zeros((5, 9), np.float32)
    assert l.fdm_flame_tables_host(C.byref(d), D.ctypes.data, None, JD.ctypes.data) == ARG
    assert l.fdm_flame_tables_host(None, D.ctypes.data, JT.ctypes.data, JD.ctypes.data) == ARG
    assert l.fdm_flame_destroy(None) == 0


def test_forward_validation_precedes_any_launch():
    """The object needs no device; every refusal is decided before a launch (the device pointers below are never dereferenced), and a
    call that passes every check without a GPU ends in FDM_ERR_STATE, never in a fallback."""
    l = _lib.lib()
    m = flame.FlameModel.synthetic(12, 3, 5, 2, seed=6, parents=[0, 0, 1])
    lv, lb = np.array([[0, 1, 2]], np.int32), np.full((1, 3), 1 / 3, np.float32)
    h, bare = C.c_void_p(), C.c_void_p()
    d = m.desc()
    assert l.fdm_flame_create(C.byref(d), lv.ctypes.data, lb.ctypes.data, 1, C.byref(h)) == 0
    assert l.fdm_flame_create(C.byref(d), None, None, 0, C.byref(bare)) == 0
    try:
        B, L = 3, 7
        fr = (C.c_int * B)(7, 0, 4)

        def fwd(f=h, shape=4096, NS=2, rows=1, expr=8192, NE=3, pose=12288, transl=None, extra=None, frames=fr, B=B, L=L, verts=16384, lmk=None):
            return l.fdm_flame_forward(f, shape, NS, rows, expr, NE, pose, transl, extra, frames, B, L, verts, lmk, None, None, None)
        assert fwd(f=None) == ARG and fwd(pose=None) == ARG and fwd(verts=None) == ARG
        assert fwd(shape=None) == ARG and b"shape" in l.fdm_last_error() and fwd(expr=None) == ARG and b"expr" in l.fdm_last_error()
        assert fwd(NS=3) == ARG and b"NS = 3" in l.fdm_last_error() and fwd(NS=-1) == ARG
        assert fwd(NE=4) == ARG and b"NE = 4" in l.fdm_last_error() and fwd(NE=-1) == ARG
        assert fwd(rows=2) == ARG and b"shape_rows" in l.fdm_last_error()
        assert fwd(f=bare, lmk=20480) == ARG and b"embedding" in l.fdm_last_error()
        assert fwd(B=0) == SHAPE and fwd(L=0) == SHAPE and fwd(L=6) == SHAPE and b"clip 0" in l.fdm_last_error()
        assert fwd(frames=(C.c_int * B)(7, -1, 4)) == SHAPE
        if not l.fdm_device_ok():            # (with a device these calls would launch on pointers that are not memory)
            for kw in (dict(), dict(shape=None, NS=0), dict(expr=None, NE=0), dict(frames=None), dict(rows=3), dict(lmk=20480), dict(transl=24576, extra=28672)):
                assert fwd(**kw) == STATE and b"no CPU fallback" in l.fdm_last_error(), kw
    finally:
        assert l.fdm_flame_destroy(h) == 0 and l.fdm_flame_destroy(bare) == 0


def test_python_layer_without_a_device(tmp_path):
    m = flame.FlameModel.synthetic(12, 5, 6, 3, seed=7)
    with pytest.raises(_lib.FdmError):
        flame.FlamePlan(m, device="cpu")
    plan = flame.FlamePlan(m)                                       # no device needed to make (and validate) one
    assert plan.key == flame.FlamePlan(flame.FlameModel.synthetic(12, 5, 6, 3, seed=7)).key and plan.key[:2] == (12, 5)
    assert plan.key != flame.FlamePlan(m, landmarks=(np.array([[0, 1, 2]]), np.array([[0.2, 0.3, 0.5]]))).key
    assert plan.key != flame.FlamePlan(flame.FlameModel.synthetic(12, 5, 6, 3, seed=8)).key
    bad = flame.FlameModel.synthetic(12, 5, 6, 3, seed=7)
    bad.parents[2] = 3
    with pytest.raises(_lib.FdmError, match="parents"):
        flame.FlamePlan(bad)
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            plan.forward(torch.zeros(1, 2, 15))
    E = m.expression_basis(2)
    assert E.shape == (2, 36) and np.array_equal(E[1].reshape(12, 3), m.shapedirs[:, :, 4])
    with pytest.raises(_lib.FdmError):
        m.expression_basis(4)
    # load: an .npz, and a pickled dict with a scipy-sparse regressor, the files' [V, 3, P] posedirs and a kintree table
    m.save(tmp_path / "head.npz")
    assert flame.FlameModel.load(tmp_path / "head.npz").digest == m.digest
    from scipy import sparse
    d = dict(v_template=m.v_template.astype(np.float64), shapedirs=m.shapedirs, posedirs=m.posedirs.T.reshape(12, 3, 36),
             J_regressor=sparse.csc_matrix(m.j_regressor), kintree_table=np.stack([np.array([2 ** 32 - 1, 0, 1, 1, 1], np.int64), np.arange(5)]),
             weights=m.lbs_weights)
    with open(tmp_path / "head.pkl", "wb") as fh:
        pickle.dump(d, fh)
    assert flame.FlameModel.load(tmp_path / "head.pkl", expr_at=3).digest == m.digest


def test_torch2mesh_pose_mapping_and_rounding():
    p6 = torch.arange(12, dtype=torch.float32).reshape(2, 6)
    full = flame.full_pose(p6)
    assert full.shape == (2, 15) and torch.equal(full[:, 0:3], p6[:, 0:3]) and torch.equal(full[:, 6:9], p6[:, 3:6])
    assert torch.count_nonzero(full[:, 3:6]) == 0 and torch.count_nonzero(full[:, 9:]) == 0
    with pytest.raises(_lib.FdmError):
        flame.full_pose(p6, J=2)
    v = torch.tensor([0.12344, 0.12346, -1.00005001, 2.5])
    assert torch.equal(flame.round4(v), torch.round(v, decimals=4)) and abs(float(flame.round4(v)[1]) - 0.1235) < 1e-7

    class Plan:                                                     # torch2mesh's own work: shapes in, rounding and shape out
        J, V = 5, 4

        def forward(self, pose, expression, landmarks=None):
            assert pose.shape == (1, 3, 15) and expression.shape == (1, 3, 50) and landmarks is False
            return flame.FlameFrames(torch.full((1, 3, 4, 3), 0.123456), None, [3])
    out = flame.torch2mesh(Plan(), torch.zeros(3, 50), torch.zeros(3, 6))
    assert out.shape == (1, 3, 12) and torch.equal(out, torch.full((1, 3, 12), 0.1235))


def test_flame_shim_has_the_reference_class_surface():
    sys.path.insert(0, os.path.join(ROOT, "face-diffusion-model_amd", "dropin"))
    try:
        from FLAME_PyTorch.FLAME import FLAME
    finally:
        sys.path.pop(0)
    assert list(inspect.signature(FLAME.__init__).parameters) == ["self", "config"]
    assert list(inspect.signature(FLAME.forward).parameters) == ["self", "shape_params", "expression_params", "pose_params", "neck_pose", "eye_pose", "transl"]
    assert all(p.default is None for n, p in inspect.signature(FLAME.forward).parameters.items() if n != "self")


def test_mead_names_flags_and_flame_argument_checks(tmp_path):
    import argparse
    from fdm_amd import metrics, pipeline
    assert metrics.mead_gt_name("M003_front_angry_level-1_001_ConditionEmotion_angry.npy") == ("M003", "M003-front-angry-level-1-001-ConditionEmotion_angry.npz")
    with pytest.raises(SystemExit):
        metrics.mead_main(["--pred_path", "x"])                           # --flame_model is required
    ap = argparse.ArgumentParser()
    pipeline.add_flame_arguments(ap)
    assert pipeline.flame_arguments(ap.parse_args([]), "cuda:0") is None
    with pytest.raises(ValueError, match="--flame_model"):
        pipeline.flame_arguments(ap.parse_args(["--template_params", "p.npy"]), "cuda:0")
    a = ap.parse_args(["--flame_model", "head.npz", "--flame_expr_at", "300"])
    assert a.flame_model == "head.npz" and a.flame_expr_at == 300 and a.template_params is None
    m = flame.FlameModel.synthetic(12, 5, 6, 3, seed=9)
    for bad in (dict(model=m), dict(pose=np.zeros((2, 15))), dict(model=m, pose=np.zeros((2, 15)), neck=1), [m]):
        with pytest.raises(ValueError, match="flame="):
            pipeline._flame_check(bad)
    pipeline._flame_check(dict(model=m, pose=np.zeros((2, 15)), shape=None, expression=None, transl=None))
    with pytest.raises(ValueError, match="rig="):                        # decided before anything touches a device
        pipeline._hand_off(torch.zeros(1, 2, 36), None, "cuda:0", rig=dict(basis=np.zeros((1, 36))), flame=dict(model=m, pose=np.zeros((2, 15))))
    with pytest.raises(ValueError, match="rig="):
        pipeline._hand_off_many([torch.zeros(1, 2, 36)], None, "cuda:0", rig=dict(basis=np.zeros((1, 36))), flame=dict(model=m, pose=np.zeros((2, 15))))
    if not torch.cuda.is_available():                                     # the evaluation itself has no CPU fallback
        m.save(tmp_path / "head.npz")
        for f in metrics.MEAD_REGIONS:
            np.save(tmp_path / f, np.arange(4))
        (tmp_path / "npy").mkdir()
        with pytest.raises(Exception):
            metrics.mead_evaluate(str(tmp_path / "npy"), str(tmp_path), str(tmp_path / "head.npz"), str(tmp_path), verbose=False)
