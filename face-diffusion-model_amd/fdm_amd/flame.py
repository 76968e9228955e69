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
from .handoff import HandoffPlan, frames_list

# vertices [B, L_max, V, 3] fp32 (rows at or past frames[b] are zeros), landmarks [B, L_max, NL, 3] or None, frames per clip
FlameFrames = namedtuple("FlameFrames", "vertices landmarks frames")

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
