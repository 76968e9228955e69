"""Call times of the render hand-off (fdm_render_forward) on an MI355X, by HIP events, against the byte floor of a call: its outputs
written once plus one read of the positions.  One child process per case, each under its own `timeout -k 10`; a case that fails ends
the run (nothing more is started on the device after a fault).  Nothing here is a merge condition; until it has been run the figures
in profiles/render_out/README.md are listed as unmeasured.
  python tools/bench_render.py                      # all cases at one sample per pixel
  python tools/bench_render.py --samples 1 4 16     # every case at each sample count (a child process per case and count)
  python tools/bench_render.py --case 0 --samples 4 # one case, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# (name, clips, frames per clip, V, image side, seconds allowed)
CASES = [("4 x 498 frames, V = 5023, 800 x 800", 4, 498, 5023, 800, 300), ("1 x 600 frames, V = 23370, 800 x 800", 1, 600, 23370, 800, 300),
         ("4 x 498 frames, V = 5023, 256 x 256", 4, 498, 5023, 256, 200), ("1 x 600 frames, V = 23370, 256 x 256", 1, 600, 23370, 256, 200)]
HBM_TBPS = 8.0       # the MI355X's stated peak, for the floor only


def one(k, reps, samples=1):
    import numpy as np
    import torch
    import mesh_cases as MC
    from fdm_amd import render
    name, B, L, V, N, _ = CASES[k]
    faces, _, xyz = MC.grid_like(V)
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    xy = (xyz[:, :2] - (lo + hi) / 2) / (hi - lo).max() * 0.22
    P = np.concatenate([xy, 0.08 * np.cos(xy[:, :1] * 12) * np.cos(xy[:, 1:] * 12)], axis=1).astype(np.float32)
    g = torch.Generator().manual_seed(k)
    x = (2e-3 * torch.randn(B, L, 3 * V, generator=g)).to("cuda:0")
    tmpl = torch.from_numpy(P.reshape(1, -1)).to("cuda:0")
    plan = render.RenderPlan(faces, V, render.Camera.preset("vocaset").resized(N, N), samples=samples, device="cuda:0")
    out = (torch.empty(B, L, N, N, 3, dtype=torch.uint8, device="cuda:0"), None, None)
    plan.forward(x, None, tmpl, out=out)          # grows the scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.forward(x, None, tmpl, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    bytes_ = out[0].numel() + x.numel() * 4
    floor_ms = bytes_ / (HBM_TBPS * 1e12) * 1e3
    covered = float((out[0][0, 0].float().mean(-1) < 255).float().mean())
    print(json.dumps(dict(case=name, samples=samples, ms_min=min(ms), ms_median=sorted(ms)[len(ms) // 2], reps=reps, floor_ms=floor_ms,
                          floor_share=floor_ms / min(ms), us_per_frame=1e3 * min(ms) / (B * L), covered=covered)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1], choices=(1, 4, 16), help="coverage samples per pixel (one child per case and count)")
    a = ap.parse_args()
    if a.case is not None:
        for n in a.samples:
            one(a.case, a.reps, n)
        return 0
    for k, c in enumerate(CASES):
        for n in a.samples:
            r = subprocess.run(["timeout", "-k", "10", str(c[5]), sys.executable, os.path.abspath(__file__), "--case", str(k), "--reps", str(a.reps),
                                "--samples", str(n)])
            if r.returncode != 0:
                print(f"case {k} ({c[0]}) at {n} samples ended with status {r.returncode}: stopping here", file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
