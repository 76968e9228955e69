"""Vertex-error arithmetic of /root/reference metric/metric.py:115-138 (FVE / LVE / EME / all-vertex error) on the
MI355X.  The reference script derives its ground truth from FLAME parameters: mead_vertex_metrics takes vertex arrays
[F, 5023, 3], or gt_params=(expression, pose) with flame= a fdm_amd.flame.FlamePlan made from the user's model file
(dropin/FLAME_PyTorch/FLAME.py has the reference's class surface)."""
from fdm_amd.metrics import mead_evaluate, mead_main, mead_vertex_metrics, motion_std, vertex_error  # noqa: F401

if __name__ == "__main__":          # the reference's command line plus --flame_model file.npz
    mead_main()
