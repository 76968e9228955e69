"""GPU: the three consumers of interp_taps (csrc/handoff.hpp) agree bit for bit -- mesh_pos_kernel through the positions of a
one-vertex clip, rig_solve_kernel through the projections on an identity basis, and linear_interp_kernel on the same rows."""
import numpy as np
import pytest
import torch

from fdm_amd import mesh, ops, rig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("L,fps", [(1, (30, 60)), (2, (30, 25)), (7, (25, 30)), (7, (30, 24))])
def test_the_three_consumers_of_interp_taps_agree(L, fps):
    Lo = mesh.frames_out(L, *fps)
    x = torch.from_numpy(np.random.default_rng(L * 100 + fps[1]).standard_normal((1, L, 3)).astype(np.float32)).to(DEV)
    want = torch.full((1, Lo, 3), float("nan"), device=DEV)
    ops.linear_interp(x, want, 1, L, Lo, 3)
    mf = mesh.MeshOutPlan(np.zeros((0, 3), np.int32), 1, DEV).forward(x, [L], None, fps, normals=False)
    rf, proj = rig.RigPlan(np.eye(3, dtype=np.float32), device=DEV).forward(x, [L], fps, proj=True)
    assert mf.frames == [Lo] and rf.frames == [Lo]
    assert not torch.isnan(want).any()
    assert torch.equal(mf.positions.reshape(1, Lo, 3), want)
    assert torch.equal(proj, want)
