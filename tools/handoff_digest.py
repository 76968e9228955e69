"""One SHA-256 per case over every tensor the hand-offs return (mesh, rig, flame) and over ops.linear_interp, at the smallest shapes
that cross each edge of the shared device code (csrc/handoff.hpp): the frame-rate taps, the 16-byte peel at every row alignment, the
chunk and tile geometry.  Two builds compute the same bits when their outputs of this script are equal line by line:

    python tools/handoff_digest.py > digest.txt        (needs the GPU; a few seconds)

Inputs are seeded; padded input rows are NaN and new outputs come from the calls themselves."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        if t is None:
            h.update(b"-")
            continue
        a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
        h.update(repr((str(a.dtype), a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def padded(x, frames):
    x = x.copy()
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return torch.from_numpy(x).to(DEV)


def mesh_cases():
    import mesh_cases as MC
    from fdm_amd import mesh
    layouts = {"f32": dict(), "f16": dict(half=True), "inter": dict(interleaved=True)}
    for name in MC.SMALL:
        faces, V, _ = MC.mesh(name)
        plan = mesh.MeshOutPlan(faces, V, DEV)
        for frames, L_max, rates in (([0, 1, 7], 7, MC.RATES), ([1], 1, [(30, 60), (30, 25)])):
            x = padded(MC.offsets(name, len(frames), L_max), frames)
            for fps in rates:
                for lname, kw in layouts.items():
                    for tmpl in (None, MC.template(name)):
                        mf = plan.forward(x, frames, tmpl, fps, **kw)
                        yield f"mesh {name} frames={frames} fps={fps} {lname} template={tmpl is not None}", (mf.positions, mf.normals, mf.frames)


def rig_cases():
    import rig_cases as RC
    from fdm_amd import rig
    for K in (1, 65, 128):
        for V3 in (15, 771, 1539):
            E, w, ridge = RC.random_rig(K, V3, seed=K + V3)
            x = padded(RC.targets_on_bounds(E, 3 * RC.L_MAX, seed=K).reshape(3, RC.L_MAX, V3), RC.FRAMES)
            for bounds in (None, (0.0, 1.0)):
                for sweeps in (0, 16):
                    plan = rig.RigPlan(E, w, ridge, bounds, sweeps, device=DEV)
                    for fps in RC.RATES:
                        rf, proj = plan.forward(x, RC.FRAMES, fps, proj=True)
                        yield f"rig K={K} 3V={V3} bounded={bounds is not None} sweeps={sweeps} fps={fps}", (rf.weights, proj, rf.frames)


def flame_cases():
    import flame_cases as FC
    from fdm_amd import flame
    for name in ("v3", "v15", "v765", "v771"):
        c, m, inp = FC.case(name)
        lm = None if inp["lv"] is None else (inp["lv"], inp["lb"])
        plan = flame.FlamePlan(m, lm, DEV)
        B, L = inp["pose"].shape[:2]
        n = B * L * 3 * m.V
        extra = (1e-2 * np.random.default_rng(len(name)).standard_normal(n)).astype(np.float32)
        buf = torch.zeros(n + 5, device=DEV)                  # a fresh allocation is 16-byte aligned
        assert buf.data_ptr() % 16 == 0
        for shift in (0, 1):                                   # `extra` on a 16-byte boundary, and one float behind it
            xt = buf[shift:shift + n].view(B, L, 3 * m.V)
            xt.copy_(torch.from_numpy(extra).view(B, L, -1))
            assert xt.data_ptr() % 16 == 4 * shift
            ff, xf, pf = plan.forward(inp["pose"], inp["expr"] if c["NE"] else None, inp["shape"] if c["NS"] else None, inp["transl"], xt,
                                      inp["frames"], xforms=True)
            yield f"flame {name} extra at +{shift}", (ff.vertices, ff.landmarks, xf, pf, ff.frames)


def interp_cases():
    from fdm_amd import ops
    for Tin, Tout in ((1, 1), (2, 1), (7, 14), (7, 5), (50, 30)):
        x = torch.from_numpy(np.random.default_rng(Tin * 100 + Tout).standard_normal((2, Tin, 5)).astype(np.float32)).to(DEV)
        y = torch.full((2, Tout, 5), float("nan"), device=DEV)
        ops.linear_interp(x, y, 2, Tin, Tout, 5)
        yield f"linear_interp {Tin} -> {Tout}", (y,)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("handoff_digest needs the GPU")
    n = 0
    with torch.no_grad():
        for cases in (mesh_cases, rig_cases, flame_cases, interp_cases):
            for name, tensors in cases():
                print(f"{sha(*tensors)}  {name}", flush=True)
                n += 1
    print(f"# {n} cases", flush=True)


if __name__ == "__main__":
    main()
