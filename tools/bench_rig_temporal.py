"""Temporal rig fit: fdm_rig_forward on an object with fdm_rig_set_temporal(mu) against the SAME object's per-frame call (smooth = 0),
alternating in one process, and against the same arithmetic written in torch on the device.

    python tools/bench_rig_temporal.py [--reps 20] [--warmup 3] [--limit 300]

Cases: 4 x 498 frames at V = 5023 with K = 52 and bounds [0, 1] (16 sweeps), the same with K = 100 and no bounds (VOCASET / 3D-MEAD),
and 1 x 600 frames at V = 23370 with K = 52 and bounds (BIWI); a random normal basis, ridge = 1e-2 tr(E E^T) / K, mu = tr(G) / K.  The
driver starts one child process per case under `timeout -k 10 <limit>` and stops at the first case that fails or runs out of time; a
child prints ONE JSON line:
  temporal_ms       HIP events around RigPlan.forward with smooth = mu into an output allocated before the loop (median, min, max)
  frame_ms          the same object and output after set_temporal(0): the per-frame fit.  The two alternate rep by rep; set_temporal
                    (host work, a device wait) sits outside the events
  torch_ms          HIP events around the torch expression: offsets @ P.T, the modal transform, torch.linalg.solve of the K dense
                    tridiagonal [L, L] systems per clip, the transform back, a clamp with bounds (the clamped unconstrained solution:
                    cheaper than the bounded fit and not the same answer).  Temporaries come from the caching allocator, warm
  launches          kernels per temporal call: projection + 3 + 2 S with bounds
  max_abs_diff      without bounds: coefficients against the torch expression (another summation order: agreement, not bits)
Figures belong in profiles/rig_temporal/README.md."""
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
SWEEPS = 16


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd.rig import RigPlan, gram, temporal_tables
    if not torch.cuda.is_available():
        raise SystemExit("bench_rig_temporal needs the GPU (a CPU timing says nothing about it)")
    B, L, V, K, bounded = a.case
    g = np.random.default_rng(1)
    E = g.standard_normal((K, 3 * V)).astype(np.float32)
    ridge = 1e-2 * float((E.astype(np.float64) ** 2).sum()) / K
    coefs = g.uniform(-0.5, 1.5, size=(B * L, K)).astype(np.float32)
    off = (torch.from_numpy(coefs) @ torch.from_numpy(E)).reshape(B, L, 3 * V).to(DEV)
    G, _ = gram(E, None, ridge)
    mu = float(np.trace(G)) / K
    plan = RigPlan(E, None, ridge, (0.0, 1.0) if bounded else None, SWEEPS, device=DEV)
    lam, Q = temporal_tables(G, mu)
    Pt, Qt, lamt = torch.from_numpy(E).to(DEV), torch.from_numpy(Q.astype(np.float32)).to(DEV), torch.from_numpy(lam.astype(np.float32)).to(DEV)
    n = torch.full((L,), 2.0, device=DEV)
    n[0] = n[-1] = 1.0 if L > 1 else 0.0
    band = torch.diag(n) - torch.diag(torch.ones(L - 1, device=DEV), 1) - torch.diag(torch.ones(L - 1, device=DEV), -1)
    out = torch.empty(B, L, K, device=DEV)
    temporal, frame, ref = [], [], []
    for r in range(a.warmup + a.reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        plan.set_temporal(mu)
        e[0].record()
        rf = plan.forward(off, out=out)
        e[1].record()
        got = rf.weights.clone()
        plan.set_temporal(0.0)
        e[2].record()
        plan.forward(off, out=out)
        e[3].record()
        e[4].record()
        z = (off.reshape(B * L, -1) @ Pt.T) @ Qt                                    # [B L, K]: z_k = sum_j Q[j][k] r_j
        T = band[None] + torch.diag_embed(lamt[:, None].expand(K, L))               # [K, L, L]
        y = torch.linalg.solve(T[None], z.reshape(B, L, K).permute(0, 2, 1)[..., None])[..., 0]      # [B, K, L]
        x = y.permute(0, 2, 1) @ Qt.T
        if bounded:
            x = x.clamp(0.0, 1.0)
        e[5].record()
        e[5].synchronize()
        if r >= a.warmup:
            temporal.append(e[0].elapsed_time(e[1]))
            frame.append(e[2].elapsed_time(e[3]))
            ref.append(e[4].elapsed_time(e[5]))
    diff = None if bounded else float((got - x).abs().max())
    print(json.dumps({"B": B, "frames": L, "V": V, "K": K, "bounded": bool(bounded), "sweeps": SWEEPS, "mu_over_trG_K": 1.0, "reps": a.reps,
                      "temporal_ms": stats(temporal), "frame_ms": stats(frame), "torch_ms": stats(ref),
                      "launches": 1 + 3 + (2 * SWEEPS if bounded else 0), "max_abs_diff": diff}), flush=True)


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
