"""Wrap hand-off: fdm_wrap_forward (wrap.WrapPlan) against the same arithmetic written in torch on the device -- the template add, index
gathers of the bound faces' corners, cross, norm and the three scaled sums -- on the same offsets, and the create with the
nearest-face search.

    python tools/bench_wrap.py [--reps 20] [--warmup 3] [--limit 300]

Follow cases: 4 x 498 frames, V = 5023 to Vt = 5023 (the source's own vertices) and to Vt = 20000; 1 x 600 frames, V = 23370 to
Vt = 23370; a grid-like source, the binding found by the device search.  Create case: the search at Vt = 20000 over the 5023-vertex
grid-like mesh.  The driver starts one child process per case under `timeout -k 10 <limit>` and stops at the first case that fails or
runs out of time; a child prints ONE JSON line:
  hip_ms            HIP events around WrapPlan.forward into an output allocated before the loop, warm cache (median, min, max)
  torch_ms          HIP events around the torch expression (its temporaries allocated by the caching allocator, warm)
  bytes             offsets + template + binding records read, output written, once each (the gathers are not counted)
  floor_ms          bytes / 8 TB/s;  floor_fraction = floor_ms / hip_ms median
  max_abs_diff      against the torch expression (torch may contract and orders its sums its own way: a few ulp, not bits)
  create_ms         (create case) host clock around WrapPlan(...) with the search, which ends in a device-to-host copy: uploads, two
                    launches, the fp64 coordinates on the host and the record upload (median, min, max)
Figures belong in profiles/wrap_out/README.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (B, frames, V, Vt, create): Vt = V binds the source's own vertices; create = 1 times the create alone
CASES = [(4, 498, 5023, 5023, 0), (4, 498, 5023, 20000, 0), (1, 600, 23370, 23370, 0), (1, 1, 5023, 20000, 1)]
DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def grid_like(V):
    """(faces, rest): two triangles per cell of a rows x cols grid over a height field; vertices left over sit on the last row's line"""
    import numpy as np
    cols = int(V ** 0.5)
    rows = V // cols
    r, c = np.meshgrid(np.arange(rows - 1), np.arange(cols - 1), indexing="ij")
    a = (r * cols + c).reshape(-1)
    i = np.arange(V)
    rest = np.stack([0.05 * (i % cols), 0.05 * (i // cols), 0.02 * np.sin(0.3 * i)], 1).astype(np.float32)
    return np.concatenate([np.stack([a, a + 1, a + cols], 1), np.stack([a + 1, a + cols + 1, a + cols], 1)]).astype(np.int32), rest


def target(rest, faces, Vt):
    """the source's own vertices (Vt = V), or Vt seeded points over the faces lifted by up to half an edge"""
    import numpy as np
    if Vt == len(rest):
        return rest.copy()
    g = np.random.default_rng(7)
    f = faces[g.integers(0, len(faces), Vt)]
    w = g.dirichlet([1.0, 1.0, 1.0], Vt).astype(np.float32)
    q = (w[:, :, None] * rest[f]).sum(1)
    q[:, 2] += 0.025 * g.uniform(-1, 1, Vt).astype(np.float32)
    return q.astype(np.float32)


def torch_path(off, tmpl, V, ia, ib, ic, u, v, h):
    import torch
    p = (off + tmpl).reshape(off.shape[0], off.shape[1], V, 3)
    a, b, c = p[:, :, ia], p[:, :, ib], p[:, :, ic]
    e1, e2 = b - a, c - a
    n = torch.cross(e1, e2, dim=-1)
    d = torch.linalg.norm(n, dim=-1, keepdim=True)
    nh = torch.where(d > 0, n / d, torch.zeros_like(n))
    return (a + u * e1 + v * e2 + h * nh).reshape(off.shape[0], off.shape[1], -1)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd.wrap import WrapPlan
    if not torch.cuda.is_available():
        raise SystemExit("bench_wrap needs the GPU (a CPU timing says nothing about it)")
    B, L, V, Vt, create = a.case
    faces, rest = grid_like(V)
    T = target(rest, faces, Vt)
    torch.cuda.init()
    torch.zeros(1, device=DEV)
    if create:
        ms = []
        for r in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            plan = WrapPlan(rest, faces, T, device=DEV)
            if r >= a.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
            del plan
        print(json.dumps({"case": "create with search", "V": V, "F": int(len(faces)), "Vt": Vt, "reps": a.reps, "create_ms": stats(ms)}), flush=True)
        return
    plan = WrapPlan(rest, faces, T, device=DEV)
    fi, uvh, _ = plan.binding()
    g = torch.Generator().manual_seed(1)
    off = (0.01 * torch.randn(B, L, 3 * V, generator=g)).to(DEV)
    tmpl = torch.from_numpy(rest.reshape(1, -1)).to(DEV)
    ia, ib, ic = (torch.from_numpy(faces[fi, k].astype(np.int64)).to(DEV) for k in range(3))
    u, v, h = (torch.from_numpy(uvh[:, k:k + 1].copy()).to(DEV) for k in range(3))
    out = torch.empty(B, L, 3 * Vt, device=DEV)
    hip, ref = [], []
    for r in range(a.warmup + a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        y = plan.forward(off, None, tmpl, out=out)
        e1.record()
        yt = torch_path(off, tmpl, V, ia, ib, ic, u, v, h)
        e2.record()
        e2.synchronize()
        if r >= a.warmup:
            hip.append(e0.elapsed_time(e1))
            ref.append(e1.elapsed_time(e2))
    diff = float((y - yt).abs().max())
    nbytes = (B * L + 1) * 3 * V * 4 + Vt * 32 + B * L * 3 * Vt * 4
    floor = nbytes / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"case": "follow", "B": B, "frames": L, "V": V, "F": int(len(faces)), "Vt": Vt, "reps": a.reps, "hip_ms": stats(hip),
                      "torch_ms": stats(ref), "bytes": nbytes, "floor_ms": floor, "floor_fraction": floor / statistics.median(hip),
                      "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=5, default=None, metavar=("B", "FRAMES", "V", "VT", "CREATE"), help="run this case in this process")
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
