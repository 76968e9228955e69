"""Per-step cost of the table-driven sampler (fdm_sample_graph kind 2) next to the DDPM and DDIM steps, and end-to-end frames/s of
DPM-Solver++ 2M at 20 steps next to the full DDPM chain, on one MI355X.  Two shapes: cfg2 (VOCASET, 4 clips x 200 frames, 800 rows,
no guidance: the update runs in the latent decoder's epilogue) and a shipped_mead-shaped call (3D-MEAD, 1 clip x 249 frames with
guidance, the single-clip plan setting: the update runs in sched_kernel).  Denoiser + scheduler only (no audio encoder, no VQ).

The yardstick for a change of the step is the PARENT commit's step at the same rows on the same box, taken in alternation
(DESIGN.md section 6).  --parent-tree <a built checkout of the parent commit> runs this file's DDPM / DDIM measurement in a child
process against that tree between the rounds of this one; without it only this build is measured.

  python tools/bench_samplers.py [--dtype bf16] [--rounds 3] [--parent-tree DIR] [--json out.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"cfg2": ("vocaset", 4, 200, False, {}), "shipped_mead": ("mead", 1, 249, True, {"ksplit.out": 2, "ksplit.ffn2": 4})}
DEV = "cuda:0"


def measure(tree, dtype_name, rounds):
    """ms per step of every sampler the tree at `tree` has, per shape: {shape: {sampler: [ms per round]}}."""
    sys.path.insert(0, os.path.join(tree, "face-diffusion-model_amd"))
    import torch
    from fdm_amd import schedule, synth
    from fdm_amd._lib import DTYPE_NAMES
    from fdm_amd.denoiser import DenoiserPlan
    res = {}
    for name, (preset, B, L, cfg, opts) in SHAPES.items():
        plan = DenoiserPlan(preset, synth.make_fdm_weights(preset), DTYPE_NAMES[dtype_name], DEV)
        for k, v in opts.items():
            plan.set(k, v)
        p = plan.p
        g = torch.Generator().manual_seed(0)
        hub = torch.randn(B, L * p.pair, p.audio_in // p.pair, generator=g)
        style = torch.eye(p.n_style)[:1].expand(B, -1)
        emo = torch.eye(p.n_emo)[4:5].expand(B, -1) if p.n_emo else None
        plan.prepare(hub, style, emo, L=L, cfg=cfg)
        x = torch.randn(B, L * p.G, p.c, generator=g).to(DEV)
        runs = {"ddpm": (100, lambda: plan.sample_ddpm(x, list(range(999, 899, -1)), seed=1)),
                "ddim": (99, lambda: plan.sample_ddim(x, 100))}
        if hasattr(plan, "sample_tables"):
            for kind, eta in (("dpmpp2m", 0.0), ("ddim_eta", 1.0)):
                t, tab = schedule.sampler_tables(kind, 100, eta)
                runs[kind] = (100, lambda t=t, tab=tab: plan.sample_tables(x, t, tab, seed=1))
            t20, tab20 = schedule.sampler_tables("dpmpp2m", 20)
            runs["e2e_2m_20"] = (1, lambda: plan.sample_tables(x, t20, tab20, seed=1))
            runs["e2e_ddpm_1000"] = (1, lambda: plan.sample_ddpm(x, list(range(999, -1, -1)), seed=1))
        out = {k: [] for k in runs}
        for fn in [r[1] for r in runs.values()]:          # graph capture and instantiation happen here
            fn()
        for _ in range(rounds):
            for k, (steps, fn) in runs.items():           # the samplers alternate inside a round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                out[k].append((time.perf_counter() - t0) * 1e3 / steps)
        out["frames"] = B * L
        res[name] = out
        del plan
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16", "f16x3", "f16"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a.child, a.dtype, a.rounds)))
        return
    trees = {"this": ROOT}
    if a.parent_tree:
        trees["parent"] = os.path.abspath(a.parent_tree)
    acc = {}
    for rnd in range(a.rounds):                             # the trees alternate (and swap places every round): one child process per tree and round
        for label, tree in (list(trees.items()) if rnd % 2 == 0 else list(trees.items())[::-1]):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree, "--dtype", a.dtype, "--rounds", "3"],
                                 capture_output=True, text=True, timeout=600)
            line = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
            if out.returncode != 0 or not line:
                raise SystemExit(f"{label} tree failed:\n{out.stdout[-2000:]}\n{out.stderr[-2000:]}")
            for shape, d in json.loads(line[0][7:]).items():
                for k, v in d.items():
                    acc.setdefault(shape, {}).setdefault(label, {}).setdefault(k, [])
                    acc[shape][label][k] += v if isinstance(v, list) else [v]
    report = {"dtype": a.dtype, "rounds": a.rounds, "shapes": {}}
    for shape, by_tree in acc.items():
        med = {label: {k: statistics.median(v) for k, v in d.items()} for label, d in by_tree.items()}
        r = {"ms_per_step": {label: {k: round(v, 4) for k, v in m.items() if not k.startswith("e2e") and k != "frames"} for label, m in med.items()}}
        this = med["this"]
        r["frames_per_s"] = {"dpmpp2m_20_steps": round(this["frames"] / (this["e2e_2m_20"] * 1e-3), 1),
                             "ddpm_1000_steps": round(this["frames"] / (this["e2e_ddpm_1000"] * 1e-3), 1)}
        base = med.get("parent", this)                      # without a parent tree: this build's own DDIM step
        r["vs_" + ("parent" if "parent" in med else "this") + "_ddim_step"] = {k: round(this[k] / base["ddim"], 4) for k in ("ddpm", "ddim", "dpmpp2m", "ddim_eta")}
        if "parent" in med:
            r["ddpm_vs_parent_ddpm_step"] = round(this["ddpm"] / base["ddpm"], 4)
        report["shapes"][shape] = r
    txt = json.dumps(report, indent=1)
    print(txt)
    if a.json:
        with open(a.json, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
