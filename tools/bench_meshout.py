"""Mesh hand-off: fdm_mesh_forward (mesh.MeshOutPlan) against the same arithmetic written in torch on the device -- the template add,
a gather of the face corners, the cross products and index_add_ over the corners -- on the same offsets.

    python tools/bench_meshout.py [--reps 20] [--warmup 3] [--limit 300]

Cases: 4 x 498 frames at V = 5023 (VOCASET) and 1 x 600 frames at V = 23370 (BIWI), a grid-like topology, normals on and off, fp32
and fp16 (eight cases).  The driver starts one child process per case under `timeout -k 10 <limit>` and stops at the first case that
fails or runs out of time; a child prints ONE JSON line:
  hip_ms            HIP events around MeshOutPlan.forward into outputs allocated before the loop (median, min, max)
  torch_ms          HIP events around the torch expression (its temporaries allocated by the caching allocator, warm)
  bytes             offsets + template read, outputs written, once each (the index lists and the gathers are not counted)
  floor_ms          bytes / 8 TB/s;  floor_fraction = floor_ms / hip_ms median
  max_abs_diff      normals against the torch expression (index_add_ adds in another order: agreement to a few ulp of 1, not bits)
Figures belong in profiles/mesh_out/README.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(B, L, V, n, h) for (B, L, V) in ((4, 498, 5023), (1, 600, 23370)) for n in (1, 0) for h in (0, 1)]
DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def grid_like(V):
    """Two triangles per cell of a rows x cols grid; vertices left over are isolated."""
    import numpy as np
    cols = int(V ** 0.5)
    rows = V // cols
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    a = (r * cols + c).reshape(-1)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int32)


def torch_path(off, tmpl, faces, V, normals, half):
    import torch
    p = (off + tmpl).reshape(off.shape[0], off.shape[1], V, 3)
    if not normals:
        return (p.half() if half else p), None
    pa, pb, pc = p[:, :, faces[:, 0]], p[:, :, faces[:, 1]], p[:, :, faces[:, 2]]
    n = torch.cross(pb - pa, pc - pa, dim=-1)
    s = torch.zeros_like(p)
    for k in range(3):
        s.index_add_(2, faces[:, k], n)
    d = (s * s).sum(-1, keepdim=True)
    nr = torch.where(d > 0, s / d.sqrt(), torch.zeros_like(s))
    return (p.half(), nr.half()) if half else (p, nr)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd.mesh import MeshOutPlan
    if not torch.cuda.is_available():
        raise SystemExit("bench_meshout needs the GPU (a CPU timing says nothing about it)")
    B, L, V, normals, half = a.case
    faces = grid_like(V)
    g = torch.Generator().manual_seed(1)
    off = (0.01 * torch.randn(B, L, 3 * V, generator=g)).to(DEV)
    cols = int(V ** 0.5)
    i = np.arange(V)
    tmpl = torch.from_numpy(np.stack([0.05 * (i % cols), 0.05 * (i // cols), 0.02 * np.sin(0.3 * i)], 1).astype(np.float32).reshape(1, -1)).to(DEV)
    plan = MeshOutPlan(faces, V, DEV)
    ft = torch.from_numpy(faces.astype(np.int64)).to(DEV)
    dt = torch.float16 if half else torch.float32
    out = (torch.empty(B, L, V, 3, dtype=dt, device=DEV), torch.empty(B, L, V, 3, dtype=dt, device=DEV) if normals else None)
    hip, ref = [], []
    for r in range(a.warmup + a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        mf = plan.forward(off, None, tmpl, None, bool(normals), False, bool(half), out=out)
        e1.record()
        tp, tn = torch_path(off, tmpl, ft, V, normals, half)
        e2.record()
        e2.synchronize()
        if r >= a.warmup:
            hip.append(e0.elapsed_time(e1))
            ref.append(e1.elapsed_time(e2))
    assert torch.equal(mf.positions, tp)
    diff = float((mf.normals.float() - tn.float()).abs().max()) if normals else 0.0
    nbytes = (B * L + 1) * 3 * V * 4 + B * L * 3 * V * (2 if half else 4) * (2 if normals else 1)
    floor = nbytes / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"B": B, "frames": L, "V": V, "F": int(len(faces)), "normals": bool(normals), "dtype": "fp16" if half else "fp32", "reps": a.reps,
                      "hip_ms": stats(hip), "torch_ms": stats(ref), "bytes": nbytes, "floor_ms": floor,
                      "floor_fraction": floor / statistics.median(hip), "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=5, default=None, metavar=("B", "FRAMES", "V", "NORMALS", "HALF"), help="run this case in this process")
    a = ap.parse_args()
    if a.case:
        return child(a)
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--case"] + [str(c) for c in case]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"case {case} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
