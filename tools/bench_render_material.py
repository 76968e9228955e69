"""Call times of the render hand-off's materials (fdm_render_set_material) on an MI355X, by HIP events: the four kinds -- base, vertex
colours, a 256-entry scalar map, a 1024 x 1024 bilinear texture -- on the scene of tools/bench_render_planes.py (4 x 498 frames of
V = 5023 at 800 x 800, rgb only), at 1 and 4 samples per pixel.  With --parent_tree DIR (a built checkout of the parent commit) the
base-material call is timed alternately on this build and on the parent's, parent first and last, so that the parent's own spread
over its repeats stands next to the difference.  One child process per case, each under its own `timeout -k 10`; a case that fails
ends the run (nothing more is started on the device after a fault).  Nothing here is a merge condition; the figures of its one
run are in profiles/render_out/README.md, its output in profiles/render_out/bench_material.jsonl.
  python tools/bench_render_material.py                            # every kind at 1 and 4 samples (a child process per pair)
  python tools/bench_render_material.py --parent_tree ../parent    # and base on parent, new, parent, new, parent
  python tools/bench_render_material.py --case 2 --samples 4       # one pair, in this process"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, L, V, N = 4, 498, 5023, 800
SECONDS = 300        # allowed per child
CASES = ["base", "vertex colours", "scalar map, 256 entries", "texture 1024 x 1024, bilinear"]


def one(k, reps, samples, tree):
    for p in (tree, os.path.join(tree, "face-diffusion-model_amd"), os.path.join(tree, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import mesh_cases as MC
    from fdm_amd import render
    dv = "cuda:0"
    faces, _, xyz = MC.grid_like(V)
    lo, hi = xyz[:, :2].min(0), xyz[:, :2].max(0)
    xy = (xyz[:, :2] - (lo + hi) / 2) / (hi - lo).max() * 0.22
    P = np.concatenate([xy, 0.08 * np.cos(xy[:, :1] * 12) * np.cos(xy[:, 1:] * 12)], axis=1).astype(np.float32)
    x = (2e-3 * torch.randn(B, L, 3 * V, generator=torch.Generator().manual_seed(0))).to(dv)
    tmpl = torch.from_numpy(P.reshape(1, -1)).to(dv)
    plan = render.RenderPlan(faces, V, render.Camera.preset("vocaset").resized(N, N), samples=samples, device=dv)
    g, kw = np.random.default_rng(0), {}
    if k == 1:
        plan.set_material(render.Material.vertex_colors(g.uniform(0, 1, (V, 3)).astype(np.float32)))
    if k == 2:
        plan.set_material(render.Material.scalar_map("heat", 0.0, 1.0))
        kw = dict(scalars=torch.rand(B, L, V, generator=torch.Generator().manual_seed(1)).to(dv))
    if k == 3:
        uv = (xy / 0.22 + 0.5).astype(np.float32)[np.asarray(faces)]          # the mesh's own (x, y) as its uv, per face corner
        plan.set_material(render.Material.texture(g.integers(0, 256, (1024, 1024, 3), dtype=np.uint8), uv))
    out = (torch.empty((B, L, N, N, 3), dtype=torch.uint8, device=dv), None, None)
    plan.forward(x, None, tmpl, out=out, **kw)          # grows the scratch
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.forward(x, None, tmpl, out=out, **kw)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    print(json.dumps(dict(case=CASES[k], tree=os.path.basename(os.path.abspath(tree)), samples=samples, ms_min=min(ms), ms_max=max(ms),
                          ms_median=sorted(ms)[len(ms) // 2], reps=reps, us_per_frame=1e3 * min(ms) / (B * L))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 4], choices=(1, 4, 16), help="coverage samples per pixel (one child per case and count)")
    ap.add_argument("--tree", default=ROOT, help="the checkout whose package and library a child times (this one)")
    ap.add_argument("--parent_tree", default=None, help="a built checkout of the parent commit: base is timed on parent, new, parent, new, parent")
    a = ap.parse_args()
    if a.case is not None:
        for n in a.samples:
            one(a.case, a.reps, n, a.tree)
        return 0
    runs = [(k, ROOT) for k in range(len(CASES))]
    if a.parent_tree:
        runs = [(0, t) for t in (a.parent_tree, ROOT, a.parent_tree, ROOT, a.parent_tree)] + runs[1:]
    for n in a.samples:
        for k, tree in runs:
            r = subprocess.run(["timeout", "-k", "10", str(SECONDS), sys.executable, os.path.abspath(__file__), "--case", str(k), "--reps", str(a.reps),
                                "--samples", str(n), "--tree", os.path.abspath(tree)])
            if r.returncode != 0:
                print(f"case {k} ({CASES[k]}) at {n} samples in {tree} ended with status {r.returncode}: stopping here", file=sys.stderr)
                return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
