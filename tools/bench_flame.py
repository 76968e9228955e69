"""Call time of the parametric-head hand-off (fdm_flame_forward) against the same arithmetic in torch and against its byte floor.
One child process per case, each under its own `timeout -k 10`; HIP-event time of the whole call, warm; a case that fails or runs out
of time ends the run.  Seeded synthetic models (no FLAME file).
  python tools/bench_flame.py [--iters 50] [--out profiles/flame_out/bench.json]
The byte floor is D once + extra in + vertices out over 8 TB/s; torch is matmul for the blends and einsum for the skinning, fed the
library's own transforms and pose features (its pose stage is not timed for torch)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "face-diffusion-model_amd"))

CASES = {
    "mead_4x498": dict(B=4, L=498, V=5023, J=5, NB=400, expr_at=300, NS=100, NE=50, extra=False, NL=0),
    "mead_4x498_extra_lmk": dict(B=4, L=498, V=5023, J=5, NB=400, expr_at=300, NS=100, NE=50, extra=True, NL=68),
    "biwi_1x600_nb0": dict(B=1, L=600, V=23370, J=5, NB=0, expr_at=0, NS=0, NE=0, extra=True, NL=0),
}
HBM = 8.0e12


def child(name, iters):
    import numpy as np
    import torch
    from fdm_amd import flame
    c, dev = CASES[name], "cuda:0"
    m = flame.FlameModel.synthetic(c["V"], c["J"], c["NB"], c["expr_at"], seed=1)
    g = np.random.default_rng(2)
    lm = (g.integers(0, c["V"], size=(c["NL"], 3)), np.full((c["NL"], 3), 1 / 3, np.float32)) if c["NL"] else None
    plan = flame.FlamePlan(m, lm, dev)
    B, L, V, J = c["B"], c["L"], c["V"], c["J"]
    t = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32)).to(dev)  # noqa: E731
    pose, ex, sh = 0.3 * t(B, L, 3 * J), (t(B, L, c["NE"]) if c["NE"] else None), (t(c["NS"]) if c["NS"] else None)
    xt = 1e-2 * t(B, L, 3 * V) if c["extra"] else None
    out = torch.empty(B, L, V, 3, device=dev)
    _, xf, pf = plan.forward(pose, ex, sh, extra=xt, xforms=True, out=out)
    D = torch.from_numpy(m.tables()[0]).to(dev)
    vt, w = torch.from_numpy(m.v_template.reshape(-1)).to(dev), torch.from_numpy(m.lbs_weights).to(dev)

    def ours():
        plan.forward(pose, ex, sh, extra=xt, out=out)

    def ref():
        v = vt + (sh @ D[:c["NS"]] if sh is not None else 0)
        v = v + (ex @ D[c["expr_at"]:c["expr_at"] + c["NE"]] if ex is not None else 0) + pf @ D[c["NB"]:]
        v = (v + xt if xt is not None else v).reshape(B, L, V, 3)
        T = torch.einsum("vj,blje->blve", w, xf).reshape(B, L, V, 3, 4)
        return torch.einsum("blvca,blva->blvc", T[..., :3], v) + T[..., 3]

    def timed(fn):
        for _ in range(5):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters
    err = float((ref() - out).abs().max())
    P = 9 * (J - 1)
    floor_bytes = 4 * ((c["NE"] + P) * 3 * V + (B * L * 3 * V if c["extra"] else 0) + B * L * 3 * V)
    print(json.dumps(dict(case=name, ms=timed(ours), torch_ms=timed(ref), floor_ms=floor_bytes / HBM * 1e3, max_abs_vs_torch=err, **c)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.iters)
    rows = []
    for name in CASES:
        r = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(a.iters)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}\n{r.stdout}{r.stderr}")
            sys.exit(1)          # nothing more is started on the device after a failure
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        x = rows[-1]
        print(f"{name}: {x['ms']:.3f} ms, torch {x['torch_ms']:.3f} ms ({x['torch_ms'] / x['ms']:.2f}x), byte floor {x['floor_ms']:.3f} ms "
              f"({100 * x['floor_ms'] / x['ms']:.1f} %), max |ours - torch| {x['max_abs_vs_torch']:.2e}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
