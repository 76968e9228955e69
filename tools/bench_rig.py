"""Rig hand-off: fdm_rig_forward (rig.RigPlan) against the same arithmetic written in torch on the device -- offsets @ P.T, then
cholesky_solve and a clamp -- on the same offsets.

    python tools/bench_rig.py [--reps 20] [--warmup 3] [--limit 300]

Cases: 4 x 498 frames at V = 5023 with K = 52 and bounds [0, 1], the same with K = 100 and no bounds (VOCASET / 3D-MEAD), and
1 x 600 frames at V = 23370 with K = 52 and bounds (BIWI); a random normal basis, ridge = 1e-2 tr(E E^T) / K, 16 sweeps.  The driver
starts one child process per case under `timeout -k 10 <limit>` and stops at the first case that fails or runs out of time; a child
prints ONE JSON line:
  hip_ms            HIP events around RigPlan.forward into an output allocated before the loop (median, min, max)
  torch_ms          HIP events around the torch expression (its temporaries allocated by the caching allocator, warm).  With bounds
                    it is the clamped unconstrained solution: cheaper than the bounded fit and not the same answer
  bytes             offsets read once plus coefficients written; floor_ms = bytes / 8 TB/s; floor_fraction = floor_ms / hip_ms median
  max_abs_diff      without bounds: coefficients against the torch expression (another summation order: agreement, not bits)
Figures belong in profiles/rig_out/README.md."""
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

CASES = [(4, 498, 5023, 52, 1), (4, 498, 5023, 100, 0), (1, 600, 23370, 52, 1)]      # B, frames, V, K, bounded
DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd.rig import RigPlan, gram
    if not torch.cuda.is_available():
        raise SystemExit("bench_rig needs the GPU (a CPU timing says nothing about it)")
    B, L, V, K, bounded = a.case
    g = np.random.default_rng(1)
    E = g.standard_normal((K, 3 * V)).astype(np.float32)
    ridge = 1e-2 * float((E.astype(np.float64) ** 2).sum()) / K
    coefs = g.uniform(-0.5, 1.5, size=(B * L, K)).astype(np.float32)
    off = (torch.from_numpy(coefs) @ torch.from_numpy(E)).reshape(B, L, 3 * V).to(DEV)
    plan = RigPlan(E, None, ridge, (0.0, 1.0) if bounded else None, 16, device=DEV)
    G, Lc = gram(E, None, ridge)
    Pt, Lt = torch.from_numpy(E).to(DEV), torch.from_numpy(Lc).to(DEV)
    out = torch.empty(B, L, K, device=DEV)
    hip, ref = [], []
    for r in range(a.warmup + a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        rf = plan.forward(off, out=out)
        e1.record()
        x = torch.cholesky_solve((off.reshape(B * L, -1) @ Pt.T).T, Lt).T
        if bounded:
            x = x.clamp(0.0, 1.0)
        e2.record()
        e2.synchronize()
        if r >= a.warmup:
            hip.append(e0.elapsed_time(e1))
            ref.append(e1.elapsed_time(e2))
    diff = None if bounded else float((rf.weights.reshape(B * L, K) - x).abs().max())
    nbytes = B * L * 3 * V * 4 + B * L * K * 4
    floor = nbytes / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"B": B, "frames": L, "V": V, "K": K, "bounded": bool(bounded), "sweeps": 16, "reps": a.reps, "hip_ms": stats(hip),
                      "torch_ms": stats(ref), "bytes": nbytes, "floor_ms": floor, "floor_fraction": floor / statistics.median(hip),
                      "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=5, default=None, metavar=("B", "FRAMES", "V", "K", "BOUNDED"), help="run this case in this process")
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
