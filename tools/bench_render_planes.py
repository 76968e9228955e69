"""Call times of the planes form of the render hand-off (fdm_render_forward_planes) on an MI355X, by HIP events, next to the same
build's fdm_render_forward (rgb only) on the same inputs, and against the byte floor of each output set: its outputs written once plus
one read of the positions.  Shapes: 4 x 498 frames of V = 5023 at 800 x 800, at 1 and 4 samples per pixel.  One child process per
case, each under its own `timeout -k 10`; a case that fails ends the run (nothing more is started on the device after a fault).
Nothing here is a merge condition; until it has been run the figures in profiles/render_out/README.md are listed as unmeasured.
  python tools/bench_render_planes.py                       # every output set at 1 and 4 samples (a child process per pair)
  python tools/bench_render_planes.py --case 1 --samples 4  # one pair, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

B, L, V, N = 4, 498, 5023, 800
SECONDS = 300        # allowed per child
# (name, outputs of the planes call); case 0 is the baseline: fdm_render_forward, rgb only
CASES = [("fdm_render_forward: rgb", None), ("planes: yuv", ("yuv",)), ("planes: rgb + alpha", ("rgb", "alpha")),
         ("planes: rgb + depth + face + alpha + yuv", ("rgb", "depth", "face_ids", "alpha", "yuv"))]
BYTES = dict(rgb=3, depth=4, face_ids=4, alpha=1, yuv=1.5)      # per pixel
HBM_TBPS = 8.0       # the MI355X's stated peak, for the floor only


def floor_bytes(names):
    """the least traffic of one call: every output written once, the positions read once"""
    return int(sum(BYTES[k] for k in names) * B * L * N * N) + B * L * 3 * V * 4


def one(k, reps, samples):
    import numpy as np
    import torch
    import mesh_cases as MC
    from fdm_amd import render
    name, names = CASES[k]
    dv = "cuda:0"
    faces, _, xyz = MC.grid_like(V)
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    xy = (xyz[:, :2] - (lo + hi) / 2) / (hi - lo).max() * 0.22
    P = np.concatenate([xy, 0.08 * np.cos(xy[:, :1] * 12) * np.cos(xy[:, 1:] * 12)], axis=1).astype(np.float32)
    x = (2e-3 * torch.randn(B, L, 3 * V, generator=torch.Generator().manual_seed(0))).to(dv)
    tmpl = torch.from_numpy(P.reshape(1, -1)).to(dv)
    plan = render.RenderPlan(faces, V, render.Camera.preset("vocaset").resized(N, N), samples=samples, device=dv)
    shape = dict(rgb=((N, N, 3), torch.uint8), depth=((N, N), torch.float32), face_ids=((N, N), torch.int32), alpha=((N, N), torch.uint8),
                 yuv=((3 * N * N // 2,), torch.uint8))
    if names is None:
        out = (torch.empty((B, L) + shape["rgb"][0], dtype=torch.uint8, device=dv), None, None)
    else:
        out = {n: torch.empty((B, L) + shape[n][0], dtype=shape[n][1], device=dv) for n in names}
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
    bytes_ = floor_bytes(names or ("rgb",))
    floor_ms = bytes_ / (HBM_TBPS * 1e12) * 1e3
    print(json.dumps(dict(case=name, samples=samples, ms_min=min(ms), ms_median=sorted(ms)[len(ms) // 2], reps=reps, floor_bytes=bytes_,
                          floor_ms=floor_ms, floor_share=floor_ms / min(ms), us_per_frame=1e3 * min(ms) / (B * L))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4], choices=(1, 4, 16), help="coverage samples per pixel (one child per case and count)")
    a = ap.parse_args()
    if a.case is not None:
        for n in a.samples:
            one(a.case, a.reps, n)
        return 0
    for n in a.samples:
        for k, c in enumerate(CASES):
            r = subprocess.run(["timeout", "-k", "10", str(SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(k), "--reps", str(a.reps),
                                "--samples", str(n)])
            if r.returncode != 0:
                print(f"case {k} ({c[0]}) at {n} samples ended with status {r.returncode}: stopping here", file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
