"""Call time of the parametric-head fit (fdm_flame_fit_forward) against the same arithmetic in torch and against its byte floor.
One child process per case, each under its own `timeout -k 10`; HIP-event time of the whole call, warm; a case that fails or runs out
of time ends the run.  Seeded synthetic models (no FLAME file).
  python tools/bench_flame_fit.py [--reps 5] [--fit_iters 20] [--out profiles/flame_fit/bench.json]
The byte floor is one read of the targets and of the D rows the fit uses (expression and pose correctives) PER ITERATION over 8 TB/s.
The kernel does not meet that floor by construction: it reads the expression rows of D again once per live row of a tile
(profiles/flame_fit/README.md).  torch is, per iteration, the batched build of [J | r] from the library's own stage-1 tables (transforms,
dX, dE of fdm_flame_fit_step at the start: its pose and derivative stages are not timed for torch), Z^T Z by bmm and
torch.cholesky_solve, in row blocks that fit memory; it does not update the tables between iterations, so it is the cost of the
arithmetic, not a second solver.  No time is a merge condition; figures go to profiles/flame_fit/README.md."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "face-diffusion-model_amd"))

CASES = {
    "mead_4x498_jaw_neck": dict(B=4, L=498, V=5023, J=5, NB=400, expr_at=300, n_expr=50, joints=(1, 2)),
}
HBM = 8.0e12
ROW_BLOCK = 166      # rows per torch block: 166 x 15069 x 57 floats = 570 MB for Z


def child(name, reps, fit_iters):
    import numpy as np
    import torch
    from fdm_amd import flame
    c, dev = CASES[name], "cuda:0"
    m = flame.FlameModel.synthetic(c["V"], c["J"], c["NB"], c["expr_at"], seed=1)
    g = np.random.default_rng(2)
    plan = flame.FlamePlan(m, None, dev)
    B, L, V, J, ne, free = c["B"], c["L"], c["V"], c["J"], c["n_expr"], c["joints"]
    t = lambda *s: torch.from_numpy(g.standard_normal(s).astype(np.float32)).to(dev)  # noqa: E731
    pose = torch.zeros(B, L, 3 * J, device=dev)
    for j in free:
        pose[..., 3 * j:3 * j + 3] = 0.15 * t(B, L, 3)
    ex = t(B, L, ne).clamp(-2, 2)
    y = plan.forward(pose, ex, landmarks=False).vertices.clone()
    kw = dict(n_expr=ne, joints=free, iters=fit_iters)
    fit = plan.fit(y, **kw)
    torch.cuda.synchronize()
    rms, bad = float(fit.rms.max()), int((fit.status != 0).sum())

    # torch: the tables of one step at the start, then per iteration the J build, the Gram matrix and the solve
    z = torch.zeros(B, L, ne, device=dev)
    s1 = plan.fit_step(y, z, torch.zeros_like(pose), n_expr=ne, joints=free)
    R = B * L
    xf, dX, dE = s1["xforms"].reshape(R, J, 12), s1["dX"].reshape(R, 3 * len(free), J, 12), s1["dE"].reshape(R, ne, J, 3)
    D = torch.from_numpy(m.tables()[0]).to(dev)
    De = D[c["expr_at"]:c["expr_at"] + ne].reshape(ne, V, 3)
    vt, w = torch.from_numpy(m.v_template).to(dev), torch.from_numpy(m.lbs_weights).to(dev)
    yr = y.reshape(R, V, 3)
    P = ne + 3 * len(free)
    lam = flame.FIT_DEFAULTS["lam"]

    def ref():
        for _ in range(fit_iters):
            for r0 in range(0, R, ROW_BLOCK):
                sl = slice(r0, min(R, r0 + ROW_BLOCK))
                T = torch.einsum("vj,rje->rve", w, xf[sl]).reshape(-1, V, 3, 4)
                v = vt.unsqueeze(0).expand(T.shape[0], V, 3)
                Ze = torch.einsum("rvca,kva->rvck", T[..., :3], De) + torch.einsum("vj,rkjc->rvck", w, dE[sl])
                U = torch.einsum("vj,rqje->rqve", w, dX[sl]).reshape(-1, 3 * len(free), V, 3, 4)
                Zp = (torch.einsum("rqvca,rva->rvcq", U[..., :3], v) + U[..., 3].permute(0, 2, 3, 1))
                res = torch.einsum("rvca,rva->rvc", T[..., :3], v) + T[..., 3] - yr[sl]
                Z = torch.cat([Ze, Zp], -1).reshape(-1, 3 * V, P)
                H = torch.bmm(Z.transpose(1, 2), Z) + lam * torch.eye(P, device=dev)
                gr = torch.bmm(Z.transpose(1, 2), res.reshape(-1, 3 * V, 1))
                torch.cholesky_solve(-gr, torch.linalg.cholesky(H))

    def ours():
        plan.fit(y, **kw)

    def timed(fn, n):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n
    PF = 9 * (J - 1)
    floor_bytes = fit_iters * 4 * (B * L * 3 * V + (ne + PF) * 3 * V)
    print(json.dumps(dict(case=name, ms=timed(ours, reps), torch_ms=timed(ref, max(1, reps // 5)), floor_ms=floor_bytes / HBM * 1e3, fit_iters=fit_iters,
                          rms_max=rms, failed_rows=bad, P=P, **{k: (list(v) if isinstance(v, tuple) else v) for k, v in c.items()})))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fit_iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.reps, a.fit_iters)
    rows = []
    for name in CASES:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                            "--fit_iters", str(a.fit_iters)], capture_output=True, text=True)
        if r.returncode != 0:
            print(f"{name}: exit status {r.returncode}\n{r.stdout}{r.stderr}")
            sys.exit(1)          # nothing more is started on the device after a failure
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        x = rows[-1]
        print(f"{name}: {x['ms']:.3f} ms for {x['fit_iters']} iterations, torch {x['torch_ms']:.3f} ms ({x['torch_ms'] / x['ms']:.2f}x), byte floor "
              f"{x['floor_ms']:.3f} ms ({100 * x['floor_ms'] / x['ms']:.1f} %), rms max {x['rms_max']:.2e}, failed rows {x['failed_rows']}")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
