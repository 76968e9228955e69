"""Time filter hand-off, the recurrences: fdm_tfilter_forward on an ema / one_euro plan (tfilter.TimeFilterPlan) against its byte floor,
against the FIR call at R = 4 on the same shape (for orientation) and against the same arithmetic written as a torch loop over frames.

    python tools/bench_time_recur.py [--reps 20] [--warmup 3] [--limit 300]

Cases: 4 x 498 frames at V = 5023 and 1 x 600 frames at V = 23370; in each, both kinds and both directions, each at every prefetch
depth of fdm_tfilter_set_prefetch.  The driver starts one child process per case under `timeout -k 10 <limit>` and stops at the first
case that fails or runs out of time; a child prints ONE JSON line per (kind, direction):
  hip_ms            per prefetch depth: HIP events around TimeFilterPlan.forward into an output allocated before the loop (median, min, max)
  bytes, floor_ms   one read and one write of the live rows per pass (zero_phase: two passes) / 8 TB/s;  floor_fraction at the default depth
  fir_ms            the Gaussian FIR plan at R = 4 on the same input
  torch_ms          the same arithmetic as a torch loop over frames (--torch_reps runs; it is thousands of launches)
  max_abs_diff      against that loop (torch may contract or order differently: a few ulp, not bits)
Figures belong in profiles/time_filter/README.md.  No time is a merge condition."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(4, 498, 5023), (1, 600, 23370)]      # (B, frames, V)
KINDS = {"ema": dict(cutoff=1.5), "one_euro": dict(min_cutoff=1.5, beta=0.5, d_cutoff=1.0)}
DEV = "cuda:0"
FPS = 30.0
HBM_BYTES_PER_S = 8e12


def torch_causal(x, kind, q):
    """x [B, L, N] -> the causal recurrence as a loop over frames of torch operations"""
    import torch
    k, c0, be, _, fr, ad, a0 = (float(v) for v in q[:7])
    B, L, N = x.shape
    out = torch.empty_like(x)
    y, xp, dh = x[:, 0].clone(), x[:, 0], torch.zeros_like(x[:, 0])
    out[:, 0] = y
    for t in range(1, L):
        xt = x[:, t]
        if kind == "one_euro":
            dh = dh + ad * ((xt - xp) * fr - dh)
            fc = c0 + be * dh.reshape(B, -1, 3).square().sum(-1).sqrt()
            a = (fc / (fc + k)).repeat_interleave(3, dim=1)
        else:
            a = a0
        y = y + a * (xt - y)
        xp = xt
        out[:, t] = y
    return out


def torch_path(x, kind, q, direction):
    import torch
    f = torch_causal(x, kind, q)
    return f if direction == "causal" else torch.flip(torch_causal(torch.flip(f, dims=[1]), kind, q), dims=[1])


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(fn, warmup, reps):
    import torch
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return stats(ms), y


def child(a):
    import torch
    from fdm_amd import tfilter
    if not torch.cuda.is_available():
        raise SystemExit("bench_time_recur needs the GPU (a CPU timing says nothing about it)")
    B, L, V = a.case
    torch.cuda.init()
    g = torch.Generator().manual_seed(1)
    t = torch.arange(L, dtype=torch.float32)[None, :, None]
    x = (0.01 * torch.sin(0.2 * t + 6.0 * torch.rand(B, 1, 3 * V, generator=g)) + 0.001 * torch.randn(B, L, 3 * V, generator=g)).to(DEV)
    out = torch.empty_like(x)
    fir = tfilter.TimeFilterPlan(V, kind="gaussian", sigma=4 / 2.5, radius=4, device=DEV)
    fir_ms, _ = timed(lambda: fir.forward(x, None, out=out), a.warmup, a.reps)
    for kind, kw in KINDS.items():
        q = tfilter.recur_coeffs(kind, FPS, **kw)
        for direction in ("causal", "zero_phase"):
            plan = tfilter.TimeFilterPlan(V, kind=kind, fps=FPS, direction=direction, device=DEV, **kw)
            hip = {}
            for depth in tfilter.PREFETCH_DEPTHS:
                plan.set_prefetch(depth)
                hip[str(depth)], y = timed(lambda: plan.forward(x, None, out=out), a.warmup, a.reps)
            plan.set_prefetch(tfilter.PREFETCH_DEFAULT)
            y = plan.forward(x, None).clone()
            ref_ms, yt = timed(lambda: torch_path(x, kind, q, direction), 1, a.torch_reps)
            diff = float((y - yt).abs().max())
            passes = 2 if direction == "zero_phase" else 1
            nbytes = passes * 2 * B * L * 3 * V * 4
            floor = nbytes / HBM_BYTES_PER_S * 1e3
            print(json.dumps({"case": "time recurrence", "B": B, "frames": L, "V": V, "kind": kind, "direction": direction, "reps": a.reps,
                              "waves": B * math.ceil(V / tfilter.RECUR_VERTS), "hip_ms": hip, "bytes": nbytes, "floor_ms": floor,
                              "floor_fraction": floor / hip[str(tfilter.PREFETCH_DEFAULT)]["median"], "fir_ms": fir_ms, "torch_ms": ref_ms,
                              "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch_reps", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=3, default=None, metavar=("B", "FRAMES", "V"), help="run this case in this process")
    a = ap.parse_args()
    if a.case:
        return child(a)
    for case in CASES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--torch_reps", str(a.torch_reps), "--case"] + [str(c) for c in case]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"case {case} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
