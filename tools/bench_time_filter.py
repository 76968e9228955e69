"""Time filter hand-off: fdm_tfilter_forward (tfilter.TimeFilterPlan) against its byte floor and against the same arithmetic written in
torch on the device -- conv1d over the transposed batch with mirrored padding, then the strength blend -- on the same offsets.

    python tools/bench_time_filter.py [--reps 20] [--warmup 3] [--limit 300]

Cases: 4 x 498 frames at V = 5023 and 1 x 600 frames at V = 23370, each at R in {4, 32}, with and without a per-vertex strength.  The
driver starts one child process per case under `timeout -k 10 <limit>` and stops at the first case that fails or runs out of time; a
child prints ONE JSON line:
  hip_ms            HIP events around TimeFilterPlan.forward into an output allocated before the loop, warm cache (median, min, max)
  torch_ms          HIP events around the torch expression (its temporaries allocated by the caching allocator, warm)
  bytes             the live rows read once and written once (halo rows read again from L2 are not counted)
  floor_ms          bytes / 8 TB/s;  floor_fraction = floor_ms / hip_ms median
  max_abs_diff      against the torch expression (torch orders its sums its own way and may contract: a few ulp, not bits)
Figures belong in profiles/time_filter/README.md.  No time is a merge condition."""
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

# (B, frames, V, R, strength)
CASES = [(B, L, V, R, s) for B, L, V in ((4, 498, 5023), (1, 600, 23370)) for R in (4, 32) for s in (0, 1)]
DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12


def torch_path(x, full, R, s3):
    """x [B, L, N], full [1, 1, 2 R + 1] -> the filter by conv1d over [B * N, 1, L] with mirrored padding (L > R), blended by s3 [N] or None"""
    import torch
    import torch.nn.functional as F
    B, L, N = x.shape
    xt = x.transpose(1, 2).reshape(B * N, 1, L)
    f = F.conv1d(F.pad(xt, (R, R), mode="reflect") if R else xt, full).reshape(B, N, L).transpose(1, 2)
    return f if s3 is None else torch.where(s3 == 0, x, x + s3 * (f - x))


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd import tfilter
    if not torch.cuda.is_available():
        raise SystemExit("bench_time_filter needs the GPU (a CPU timing says nothing about it)")
    B, L, V, R, with_s = a.case
    h = tfilter.gaussian(max(R, 1) / 2.5, R).astype(np.float32)
    s = np.random.default_rng(3).uniform(0, 1, V).astype(np.float32) if with_s else None
    if s is not None:
        s[::7] = 0.0
    torch.cuda.init()
    plan = tfilter.TimeFilterPlan(V, taps=h, strength=s, device=DEV)
    g = torch.Generator().manual_seed(1)
    x = (0.01 * torch.randn(B, L, 3 * V, generator=g)).to(DEV)
    full = torch.from_numpy(np.concatenate([h[:0:-1], h])).to(DEV).reshape(1, 1, -1)
    s3 = None if s is None else torch.from_numpy(np.repeat(s, 3)).to(DEV)
    out = torch.empty_like(x)
    hip, ref = [], []
    for r in range(a.warmup + a.reps):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        y = plan.forward(x, None, out=out)
        e1.record()
        yt = torch_path(x, full, R, s3)
        e2.record()
        e2.synchronize()
        if r >= a.warmup:
            hip.append(e0.elapsed_time(e1))
            ref.append(e1.elapsed_time(e2))
    diff = float((y - yt).abs().max())
    nbytes = 2 * B * L * 3 * V * 4
    floor = nbytes / HBM_BYTES_PER_S * 1e3
    print(json.dumps({"case": "time filter", "B": B, "frames": L, "V": V, "R": R, "strength": bool(with_s), "reps": a.reps, "hip_ms": stats(hip),
                      "torch_ms": stats(ref), "bytes": nbytes, "floor_ms": floor, "floor_fraction": floor / statistics.median(hip),
                      "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=5, default=None, metavar=("B", "FRAMES", "V", "R", "STRENGTH"), help="run this case in this process")
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
