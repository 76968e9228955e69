"""Drop-in for FLAME_PyTorch/FLAME.py: the class surface of the reference's FLAME layer over the device hand-off (fdm_amd.flame,
include/fdm_hip.h fdm_flame_*).  config carries flame_model_path (an .npz or a pickled dict of plain arrays: FlameModel.load),
shape_params, expression_params, batch_size and optionally static_landmark_embedding_path (an .npz / pickle with lmk_faces_idx,
lmk_b_coords) with the model's faces under the key f.  The dynamic contour landmarks are not built: landmarks are the static
embedding's, or None without one."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _path  # noqa: E402,F401

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fdm_amd import flame as _flame  # noqa: E402


def _read(path):
    if str(path).endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    import pickle
    with open(path, "rb") as fh:
        return dict(pickle.load(fh, encoding="latin1"))


class FLAME(torch.nn.Module):
    def __init__(self, config):
        super().__init__()
        self.batch_size = int(getattr(config, "batch_size", 1))
        self.n_shape, self.n_expr = int(getattr(config, "shape_params", 100)), int(getattr(config, "expression_params", 50))
        self.device_name = getattr(config, "device", "cuda:0")
        self.model = _flame.FlameModel.load(config.flame_model_path, expr_at=getattr(config, "expr_at", None))
        landmarks = None
        emb = getattr(config, "static_landmark_embedding_path", None)
        if emb:
            e = _read(emb)
            if self.model.faces is None:
                raise _flame.FdmError(f"{config.flame_model_path}: a landmark embedding needs the faces under the key f")
            faces = self.model.faces
            landmarks = (faces[np.asarray(e["lmk_faces_idx"]).astype(np.int64)], np.asarray(e["lmk_b_coords"], dtype=np.float32))
        self.plan = _flame.FlamePlan(self.model, landmarks, self.device_name)

    def forward(self, shape_params=None, expression_params=None, pose_params=None, neck_pose=None, eye_pose=None, transl=None):
        """shape [N, n_shape], expression [N, n_expr], pose [N, 6] (global, jaw), neck [N, 3], eyes [N, 6], transl [N, 3]; whatever is
        None is zeros -> (vertices [N, V, 3], landmarks [N, NL, 3] or None).  Every row is its own clip of one frame."""
        given = [x for x in (shape_params, expression_params, pose_params, neck_pose, eye_pose, transl) if x is not None]
        N = int(given[0].shape[0]) if given else self.batch_size
        dv = self.plan.device
        z = lambda x, n: torch.zeros(N, n, device=dv) if x is None else torch.as_tensor(x, dtype=torch.float32).to(dv).reshape(N, n)  # noqa: E731
        p6, neck, eyes = z(pose_params, 6), z(neck_pose, 3), z(eye_pose, 6)
        pose = torch.cat([p6[:, :3], neck, p6[:, 3:], eyes], 1)[:, :3 * self.plan.J]
        sh = None if shape_params is None else z(shape_params, int(shape_params.shape[-1]))
        ex = None if expression_params is None else z(expression_params, int(expression_params.shape[-1])).unsqueeze(1)
        ff = self.plan.forward(pose.unsqueeze(1), ex, sh, None if transl is None else z(transl, 3).unsqueeze(1))
        return ff.vertices[:, 0], None if ff.landmarks is None else ff.landmarks[:, 0]
