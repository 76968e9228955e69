"""Parametric head: parameters in, vertices out, on the device (include/fdm_hip.h, fdm_flame_*; kernels csrc/flame_out.hpp; DESIGN.md
section 2 item 20 is the definition).  A head of the SMPL / FLAME family: shape and expression blend shapes, pose correctives and
linear blend skinning; the decoder's offsets enter as `extra`.  No model file ships with the library (FLAME's is licensed):
FlameModel.load reads the user's, FlameModel.synthetic makes seeded ones for tests."""
import ctypes as C
import hashlib
from collections import namedtuple

import numpy as np
import torch

from ._lib import FdmError, FlameModelDesc, check, lib
from .handoff import HandoffPlan, cached_plan, frames_list

# vertices [B, L_max, V, 3] fp32 (rows at or past frames[b] are zeros), landmarks [B, L_max, NL, 3] or None, frames per clip
FlameFrames = namedtuple("FlameFrames", "vertices landmarks frames")

# expression [B, L_max, n_expr], pose [B, L_max, 3 J] (fixed joints carry pose0), transl [B, L_max, 3] (zeros unless fitted), rms [B, L_max],
# status [B, L_max] int32 (0, or 1 + the Cholesky column at which the row's step failed), frames per clip, vertices [B, L_max, V, 3] or None
FlameFit = namedtuple("FlameFit", "expression pose transl rms status frames vertices")
JOINT_NAMES = ("global", "neck", "jaw", "eye_l", "eye_r")      # the 5-joint FLAME chain
FIT_PMAX = 128
FIT_DEFAULTS = dict(iters=20, lam=1e-6, ridge_expr=0.0, ridge_pose=0.0, pivot_tol=2.0 ** -18)      # settings, not measurements

KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "parents", "lbs_weights")
FLAME_POSE = 15           # global, neck, jaw, left eye, right eye


def _dense(a):
    """numpy array of a plain array, a scipy-sparse matrix, or an object that carries its values in .r (read without its package)"""
    if hasattr(a, "toarray"):
        a = a.toarray()
    elif hasattr(a, "r") and not isinstance(a, np.ndarray):
        a = a.r
    return np.asarray(a)


class FlameModel:
    """Holder of the host arrays of fdm_flame_model: v_template [V, 3], shapedirs [V, 3, NB], posedirs [9 (J - 1), 3 V] (the model
    files' [V, 3, 9 (J - 1)] is accepted and transposed), j_regressor [J, V], parents [J], lbs_weights [V, J]; coefficients
    [0, expr_at) are shape, [expr_at, NB) expression."""

    def __init__(self, v_template, shapedirs, posedirs, j_regressor, parents, lbs_weights, expr_at):
        f = lambda a: np.ascontiguousarray(_dense(a), dtype=np.float32)  # noqa: E731
        self.v_template = f(v_template).reshape(-1, 3)
        self.V = int(self.v_template.shape[0])
        self.lbs_weights = f(lbs_weights).reshape(self.V, -1)
        self.J = int(self.lbs_weights.shape[1])
        sd = f(shapedirs) if shapedirs is not None else np.zeros((self.V, 3, 0), np.float32)
        self.shapedirs = np.ascontiguousarray(sd.reshape(self.V, 3, -1))
        self.NB = int(self.shapedirs.shape[2])
        P = 9 * (self.J - 1)
        if P:
            pd = f(posedirs)
            if pd.ndim == 3:                               # [V, 3, P] as the files store it -> [P, 3 V]
                pd = pd.reshape(-1, pd.shape[-1]).T
            if pd.shape != (P, 3 * self.V):
                raise FdmError(f"posedirs must be [{P}, {3 * self.V}] (or [V, 3, {P}]), got {pd.shape}")
            self.posedirs = np.ascontiguousarray(pd)
        else:
            self.posedirs = None
        self.j_regressor = f(j_regressor).reshape(-1, self.V)
        if self.j_regressor.shape[0] != self.J:
            raise FdmError(f"j_regressor has {self.j_regressor.shape[0]} rows for {self.J} joints")
        par = np.asarray(_dense(parents)).reshape(-1).astype(np.int64)
        if par.shape[0] != self.J:
            raise FdmError(f"{par.shape[0]} parents for {self.J} joints")
        par[0] = 0                                         # (files store -1 or 2^32 - 1 there; the entry is ignored)
        self.parents = np.ascontiguousarray(par.astype(np.int32))
        self.expr_at = int(expr_at)
        self.faces = None
        self._digest = None

    @classmethod
    def load(cls, path, expr_at=None):
        """An .npz with the keys v_template, shapedirs, posedirs, J_regressor (or j_regressor), parents (or kintree_table),
        lbs_weights (or weights) and optionally expr_at; or a pickled dict of plain numpy / scipy-sparse arrays with those keys.
        expr_at: where the expression coefficients start (FLAME: 300); default the file's, else NB."""
        if str(path).endswith(".npz"):
            with np.load(path, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        else:
            import pickle
            with open(path, "rb") as fh:
                d = dict(pickle.load(fh, encoding="latin1"))
        get = lambda *names: next((d[n] for n in names if n in d), None)  # noqa: E731
        par = get("parents")
        if par is None and "kintree_table" in d:
            par = _dense(d["kintree_table"])[0]
        need = dict(v_template=get("v_template"), j_regressor=get("J_regressor", "j_regressor"), parents=par, lbs_weights=get("lbs_weights", "weights"))
        missing = [k for k, v in need.items() if v is None]
        if missing:
            raise FdmError(f"{path}: missing {missing} (has {sorted(d)})")
        sd = get("shapedirs")
        if expr_at is None:
            expr_at = int(d["expr_at"]) if "expr_at" in d else (0 if sd is None else int(_dense(sd).shape[-1]))
        m = cls(need["v_template"], sd, get("posedirs"), need["j_regressor"], par, need["lbs_weights"], expr_at)
        m.faces = None if get("f") is None else np.asarray(_dense(get("f"))).astype(np.int64)      # the file's triangle list, if it has one
        return m

    def save(self, path):
        np.savez(path, v_template=self.v_template, shapedirs=self.shapedirs, posedirs=np.zeros((0, 3 * self.V), np.float32) if self.posedirs is None else self.posedirs,
                 J_regressor=self.j_regressor, parents=self.parents, lbs_weights=self.lbs_weights, expr_at=np.int32(self.expr_at))

    @classmethod
    def synthetic(cls, V, J, NB, expr_at, seed, parents=None):
        """A seeded model of the family's shape: a unit-scale template, directions two orders smaller, a sparse convex joint
        regressor, convex skinning weights.  parents: [J] or None (FLAME's tree cut to J: 0 <- 1 <- {2, 3, 4}, then a chain)."""
        g = np.random.default_rng(seed)
        vt = g.standard_normal((V, 3)).astype(np.float32) * np.float32(0.1)
        sd = (g.standard_normal((V, 3, NB)) * 1e-2).astype(np.float32)
        pd = (g.standard_normal((9 * (J - 1), 3 * V)) * 1e-2).astype(np.float32) if J > 1 else None
        jr = np.zeros((J, V), np.float64)
        for j in range(J):
            idx = g.choice(V, size=min(V, 8), replace=False)
            w = g.random(len(idx)) + 0.1
            jr[j, idx] = w / w.sum()
        w = g.random((V, J)) ** 4 + 1e-3
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
        if parents is None:
            parents = [0, 0, 1, 1, 1, 4, 5, 6][:J]
        return cls(vt, sd, pd, jr.astype(np.float32), np.asarray(parents), w, expr_at)

    def expression_basis(self, n=None):
        """[n, 3 V]: the first n expression directions, what rig.RigPlan(basis=...) takes."""
        n = self.NB - self.expr_at if n is None else int(n)
        if n < 1 or n > self.NB - self.expr_at:
            raise FdmError(f"{n} expression directions of {self.NB - self.expr_at}")
        return np.ascontiguousarray(self.shapedirs[:, :, self.expr_at:self.expr_at + n].reshape(3 * self.V, n).T)

    @property
    def digest(self):
        if self._digest is None:
            d = hashlib.sha1()
            for a in (self.v_template, self.shapedirs, self.posedirs, self.j_regressor, self.parents, self.lbs_weights):
                d.update(b"-" if a is None else a.tobytes())
            d.update(repr((self.V, self.J, self.NB, self.expr_at)).encode())
            self._digest = d.hexdigest()
        return self._digest

    def desc(self):
        p = lambda a: None if a is None or a.size == 0 else a.ctypes.data  # noqa: E731
        return FlameModelDesc(self.V, self.J, self.NB, self.expr_at, p(self.v_template), p(self.shapedirs), p(self.posedirs),
                              p(self.j_regressor), p(self.parents), p(self.lbs_weights))

    def tables(self):
        """(D [NB + 9 (J - 1), 3 V], JT [J, 3], JD [NB, 3 J]) float32 of fdm_flame_tables_host."""
        P = 9 * (self.J - 1)
        D = np.zeros((self.NB + P, 3 * self.V), np.float32)
        JT, JD = np.zeros((self.J, 3), np.float32), np.zeros((self.NB, 3 * self.J), np.float32)
        d = self.desc()
        check(lib().fdm_flame_tables_host(C.byref(d), D.ctypes.data, JT.ctypes.data, JD.ctypes.data))
        return D, JT, JD


def landmark_arrays(landmarks, V=None):
    """landmarks = (verts [NL, 3] ints, bary [NL, 3]) as contiguous host arrays, or (None, None)."""
    if landmarks is None:
        return None, None
    lv = np.ascontiguousarray(np.asarray(_dense(landmarks[0]), dtype=np.int32).reshape(-1, 3))
    lb = np.ascontiguousarray(np.asarray(_dense(landmarks[1]), dtype=np.float32).reshape(-1, 3))
    if lv.shape != lb.shape:
        raise FdmError(f"landmarks: {lv.shape[0]} vertex triples and {lb.shape[0]} weight triples")
    return lv, lb


def plan_key(model, landmarks=None):
    """FlamePlan(model, landmarks).key without making the plan: (V, J, digest of the model and the embedding)."""
    k = hashlib.sha1(model.digest.encode())
    for a in landmark_arrays(landmarks):
        k.update(b"-" if a is None else a.tobytes())
    return (model.V, model.J, k.hexdigest())


class FlamePlan(HandoffPlan):
    """Thin binding of fdm_flame_create / fdm_flame_forward for one model (and one static landmark embedding): the tables are formed
    and uploaded here, forward() only passes pointers.  A plan holds one scratch: it serves one stream at a time (pipeline.to_flame
    keeps them per (device, stream, model)).  Without a visible device the plan still validates and forward() raises."""

    _destroy = "fdm_flame_destroy"

    def __init__(self, model, landmarks=None, device="cuda:0"):
        super().__init__(device)
        self.model = model
        self.lv, self.lb = landmark_arrays(landmarks)
        self.NL = 0 if self.lv is None else int(self.lv.shape[0])
        self.V, self.J, self.NB = model.V, model.J, model.NB
        self.key = plan_key(model, landmarks)
        d = model.desc()
        self._create("fdm_flame_create", C.byref(d), None if self.lv is None else self.lv.ctypes.data, None if self.lb is None else self.lb.ctypes.data, self.NL)

    def _dev(self, x, what, last, B=None, L=None):
        """x as a contiguous float32 device tensor [B, L, last] ([L, last] gains the batch)"""
        x = torch.as_tensor(x).detach()
        if x.dim() == 2:
            x = x.unsqueeze(0)
        x = x.to(self.device, torch.float32).contiguous()
        if x.dim() != 3 or x.shape[2] != last or (B is not None and tuple(x.shape[:2]) != (B, L)):
            raise FdmError(f"{what} must be [{'B' if B is None else B}, {'L' if L is None else L}, {last}], got {tuple(x.shape)}")
        return x

    def forward(self, pose, expression=None, shape=None, transl=None, extra=None, frames=None, landmarks=None, xforms=False, out=None):
        """pose [B, L_max, 3 J] (or [L, 3 J]) axis-angle; expression [B, L_max, NE] or None; shape [NS] / [1, NS] / [B, NS] or None;
        transl [B, L_max, 3]; extra [B, L_max, 3 V] displacements added before skinning (the decoder's offsets); frames: L per clip
        (None: L_max).  landmarks: True / False (None: whether the plan has an embedding).  -> FlameFrames, or with xforms=True
        (FlameFrames, xforms [B, L_max, J, 12], posefeat [B, L_max, 9 (J - 1)]).  out: a vertices tensor to write."""
        dv = self.device
        pose = self._dev(pose, "pose", 3 * self.J)
        B, L = int(pose.shape[0]), int(pose.shape[1])
        ex, NE = None, 0
        if expression is not None:
            ex = torch.as_tensor(expression)
            ex = self._dev(ex, "expression", int(ex.shape[-1]), B, L)
            NE = int(ex.shape[2])
        sh, NS, srows = None, 0, 1
        if shape is not None:
            sh = torch.as_tensor(shape).detach().to(dv, torch.float32)
            sh = (sh.reshape(1, -1) if sh.dim() == 1 else sh).contiguous()
            NS, srows = int(sh.shape[1]), int(sh.shape[0])
        tr = None if transl is None else self._dev(transl, "transl", 3, B, L)
        xt = None
        if extra is not None:
            xt = torch.as_tensor(extra)
            xt = self._dev(xt.reshape(*xt.shape[:-2], -1) if (xt.shape[-1] == 3 and xt.shape[-2] == self.V) else xt, "extra", 3 * self.V, B, L)
        fr = frames_list(frames, B, L)
        if out is None:
            verts = torch.empty(B, L, self.V, 3, dtype=torch.float32, device=dv)
        else:
            verts = out
            if verts.dtype != torch.float32 or verts.device != dv or verts.numel() != B * L * self.V * 3 or not verts.is_contiguous():
                raise FdmError(f"out must be a contiguous float32 [{B}, {L}, {self.V}, 3] tensor on {dv}")
        want_l = bool(self.NL) if landmarks is None else bool(landmarks)
        lm = torch.empty(B, L, self.NL, 3, dtype=torch.float32, device=dv) if want_l else None
        xf = torch.empty(B, L, self.J, 12, dtype=torch.float32, device=dv) if xforms else None
        pf = torch.empty(B, L, 9 * (self.J - 1), dtype=torch.float32, device=dv) if xforms else None
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            check(lib().fdm_flame_forward(self.h, p(sh), NS, srows, p(ex), NE, pose.data_ptr(), p(tr), p(xt), fa, B, L, verts.data_ptr(), p(lm),
                                          p(xf), p(pf), torch.cuda.current_stream(dv).cuda_stream))
        self._keep = (pose, ex, sh, tr, xt)          # read asynchronously on this stream
        ff = FlameFrames(verts, lm, fr)
        return (ff, xf, pf) if xforms else ff

    def fit_plan(self, n_expr=50, joints=("jaw",), transl=False, weights=None):
        """The FlameFitPlan for one free set and weight vector, cached through handoff.cached_plan per (device, stream, MODEL digest, free
        set, weights) -- by the model, not by this head object.  A second FlamePlan of the same model on the same device and stream
        therefore gets the fit object bound to the FIRST head's native handle: the tables are the same, so the results are, but the
        first head's device memory stays pinned for the life of the process and the two heads share one scratch (one stream at a time
        for all of them)."""
        jt = fit_joints(joints, self.J)
        wk = None if weights is None else hashlib.sha1(np.ascontiguousarray(torch.as_tensor(weights).detach().cpu().numpy(), dtype=np.float32).tobytes()).hexdigest()
        # one fit object per (device, stream, model digest, free set): it holds this head (which must outlive it), the head holds nothing back
        return cached_plan((str(self.device), self.stream), "flame_fit", (self.key, int(n_expr), jt, bool(transl), wk),
                           lambda: FlameFitPlan(self, n_expr, jt, transl, weights))

    def _fit_inputs(self, target, shape, pose0, frames):
        dv = self.device
        y = torch.as_tensor(target).detach()
        if y.dim() >= 2 and y.shape[-1] == 3 and y.shape[-2] == self.V:
            y = y.reshape(*y.shape[:-2], -1)
        y = self._dev(y, "target", 3 * self.V)
        B, L = int(y.shape[0]), int(y.shape[1])
        sh, NS, srows = None, 0, 1
        if shape is not None:
            sh = torch.as_tensor(shape).detach().to(dv, torch.float32)
            sh = (sh.reshape(1, -1) if sh.dim() == 1 else sh).contiguous()
            NS, srows = int(sh.shape[1]), int(sh.shape[0])
        p0 = None if pose0 is None else self._dev(pose0, "pose0", 3 * self.J, B, L)
        return y, B, L, sh, NS, srows, p0, frames_list(frames, B, L)

    def fit(self, target, n_expr=50, joints=("jaw",), transl=False, shape=None, pose0=None, weights=None, iters=None, lam=None, ridge_expr=None,
            ridge_pose=None, frames=None, return_vertices=False, pivot_tol=None):
        """The reverse of forward() (fdm_flame_fit_forward): target [B, L_max, V, 3] or [B, L_max, 3 V] (or one
        clip without the batch) absolute vertex positions -> FlameFit.  n_expr: the first n expression coefficients; joints: the free
        joints by index or by name (JOINT_NAMES, 5-joint models); transl: fit a translation; shape as in forward (fixed); pose0
        [B, L_max, 3 J]: the start, and the rotation of the joints that stay fixed; weights [V] >= 0; iters, lam, ridge_expr, ridge_pose:
        pivot_tol (a row fails at a pivot not above pivot_tol x its damped diagonal; 0: the plain test pivot > 0): FIT_DEFAULTS (settings,
        not measurements)."""
        fp = self.fit_plan(n_expr, joints, transl, weights)
        fp.set(iters=iters, lam=lam, ridge_expr=ridge_expr, ridge_pose=ridge_pose, pivot_tol=pivot_tol)
        y, B, L, sh, NS, srows, p0, fr = self._fit_inputs(target, shape, pose0, frames)
        dv = self.device
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dv)  # noqa: E731
        ex, ps, tr, rms, st = new(B, L, fp.n_expr), new(B, L, 3 * self.J), new(B, L, 3), new(B, L), new(B, L, dt=torch.int32)
        verts = new(B, L, self.V, 3) if return_vertices else None
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            check(lib().fdm_flame_fit_forward(fp.h, y.data_ptr(), p(sh), NS, srows, p(p0), fa, B, L, ex.data_ptr(), ps.data_ptr(), tr.data_ptr(),
                                              rms.data_ptr(), p(verts), st.data_ptr(), torch.cuda.current_stream(dv).cuda_stream))
        self._keep = (y, sh, p0)                     # read asynchronously on this stream
        return FlameFit(ex, ps, tr, rms, st, fr, verts)

    def fit_step(self, target, expression, pose, transl=None, n_expr=50, joints=("jaw",), fit_transl=False, shape=None, pose0=None, weights=None,
                 lam=None, ridge_expr=None, ridge_pose=None, frames=None):
        """ONE Gauss-Newton step from given parameters (fdm_flame_fit_step; for tests and tools) -> dict(H [B, L, (P + 1)(P + 2) / 2],
        delta [B, L, P], dX, dE, xforms, status)."""
        fp = self.fit_plan(n_expr, joints, fit_transl, weights)
        fp.set(lam=lam, ridge_expr=ridge_expr, ridge_pose=ridge_pose)
        y, B, L, sh, NS, srows, p0, fr = self._fit_inputs(target, shape, pose0, frames)
        dv, J, P = self.device, self.J, fp.P
        ps = self._dev(pose, "pose", 3 * J, B, L)
        ex = self._dev(expression, "expression", fp.n_expr, B, L) if fp.n_expr else None
        tr = self._dev(transl, "transl", 3, B, L) if fp.transl else None
        new = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=dv)  # noqa: E731
        out = dict(H=new(B, L, (P + 1) * (P + 2) // 2), delta=new(B, L, P), dX=new(B, L, 3 * len(fp.joints), J, 12), dE=new(B, L, fp.n_expr, J, 3),
                   xforms=new(B, L, J, 12), status=new(B, L, dt=torch.int32))
        p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        fa = (C.c_int * B)(*fr)
        with torch.cuda.device(dv):
            check(lib().fdm_flame_fit_step(fp.h, y.data_ptr(), p(sh), NS, srows, p(p0), p(ex), ps.data_ptr(), p(tr), fa, B, L, out["H"].data_ptr(),
                                           out["delta"].data_ptr(), out["dX"].data_ptr(), out["dE"].data_ptr(), out["xforms"].data_ptr(),
                                           out["status"].data_ptr(), torch.cuda.current_stream(dv).cuda_stream))
        self._keep = (y, sh, p0, ps, ex, tr)
        return out


def fit_joints(joints, J):
    """joints: names of JOINT_NAMES (5-joint models) or indices -> ascending tuple of joint indices, refused when out of range or twice"""
    if joints is None:
        joints = ()
    if isinstance(joints, (str, int)):
        joints = (joints,)
    out = []
    for j in joints:
        if isinstance(j, str):
            if J != len(JOINT_NAMES) or j not in JOINT_NAMES:
                raise FdmError(f"joint name {j!r}: names {JOINT_NAMES} are those of a 5-joint model, this one has {J} joints")
            j = JOINT_NAMES.index(j)
        j = int(j)
        if j < 0 or j >= J:
            raise FdmError(f"joint index {j} out of range 0..{J - 1}")
        if j in out:
            raise FdmError(f"joint {j} is given twice")
        out.append(j)
    return tuple(sorted(out))


class FlameFitPlan(HandoffPlan):
    """fdm_flame_fit_create on a FlamePlan's head for one free set (n_expr, joints, transl, weights).  It uses the head's tables and
    scratch: one stream at a time for the pair.  It keeps the head alive; FlamePlan.fit_plan caches these through handoff.cached_plan."""

    _destroy = "fdm_flame_fit_destroy"

    def __init__(self, head, n_expr, joints, transl, weights):
        super().__init__(head.device)
        self.head = head
        self.n_expr, self.joints, self.transl = int(n_expr), fit_joints(joints, head.J), bool(transl)
        self.P = self.n_expr + 3 * len(self.joints) + 3 * int(self.transl)
        NE = head.NB - head.model.expr_at
        if self.n_expr < 0 or self.n_expr > NE:
            raise FdmError(f"n_expr = {self.n_expr}: the model has NE = {NE} expression coefficients")
        if self.P < 1 or self.P > FIT_PMAX:
            raise FdmError(f"P = {self.P} free parameters (1..{FIT_PMAX})")
        w = None
        if weights is not None:
            w = np.ascontiguousarray(torch.as_tensor(weights).detach().cpu().numpy(), dtype=np.float32).reshape(-1)
            if w.shape[0] != head.V:
                raise FdmError(f"weights must be [{head.V}], got {w.shape[0]}")
            if not np.all(np.isfinite(w)) or np.any(w < 0) or not np.any(w > 0):
                raise FdmError("weights must be finite, not negative and not all zero")
        self.weights = w
        fj = (C.c_int * max(1, len(self.joints)))(*self.joints)
        self._create("fdm_flame_fit_create", head.h, fj, len(self.joints), self.n_expr, int(self.transl), None if w is None else w.ctypes.data)
        self._set = {}

    def set(self, **kw):
        """iters, lam, ridge_expr, ridge_pose, pivot_tol (None: the default)"""
        for k, v in kw.items():
            v = FIT_DEFAULTS[k] if v is None else v
            if k == "iters":
                if int(v) != v or int(v) < 1:
                    raise FdmError(f"iters = {v} (a whole number >= 1)")
            elif not (float(v) >= 0.0) or float(v) == float("inf"):
                raise FdmError(f"{k} = {v} (finite and not negative)")
            if self._set.get(k) != v:
                check(lib().fdm_flame_fit_set(self.h, {"lam": b"lambda"}.get(k, k.encode()), float(v)))
                self._set[k] = v

    def columns(self):
        """what column q of theta is: ('expr', k) | ('pose', 3 j + c) | ('transl', c)"""
        return ([("expr", k) for k in range(self.n_expr)] + [("pose", 3 * j + c) for j in self.joints for c in range(3)] +
                [("transl", c) for c in range(3 * int(self.transl))])


def full_pose(pose6, J=5):
    """The reference's 6-number pose (global, jaw) -> [..., 3 J] with zero neck and eyes (FLAME's order: global, neck, jaw, eyes)."""
    pose6 = torch.as_tensor(pose6, dtype=torch.float32)
    if J < 3:
        raise FdmError(f"a (global, jaw) pose needs a model with a jaw joint, J = {J}")
    out = torch.zeros(*pose6.shape[:-1], 3 * J, dtype=torch.float32, device=pose6.device)
    out[..., 0:3] = pose6[..., 0:3]
    out[..., 6:9] = pose6[..., 3:6]
    return out


def round4(v):
    """torch.round(decimals=4) of the reference's torch2mesh, in torch"""
    return torch.round(v, decimals=4)


@torch.no_grad()
def torch2mesh(plan, expression, pose):
    """The reference's utiles/flame_utils.torch2mesh on the device: expression [L, NE] and pose [L, 6] (global, jaw) -> [1, L, 3 V]:
    zero shape, zero neck and eyes, vertices rounded to 4 decimals."""
    ps = full_pose(torch.as_tensor(pose, dtype=torch.float32).reshape(-1, 6), plan.J)
    L = int(ps.shape[0])
    ex = torch.as_tensor(expression, dtype=torch.float32).reshape(L, -1)
    ff = plan.forward(ps.unsqueeze(0), ex.unsqueeze(0) if ex.shape[1] else None, landmarks=False)
    return round4(ff.vertices).reshape(1, L, 3 * plan.V)
