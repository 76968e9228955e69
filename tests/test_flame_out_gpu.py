"""GPU: the parametric-head hand-off (include/fdm_hip.h, fdm_flame_*; kernels csrc/flame_out.hpp) -- the pose stage within 4 E of the
fp64 restatement (E measured on the CPU: tests/flame_cases.py), blend and skin within the a-priori bound (n + 2) 2^-24 S of fp64
evaluated from the device's own transforms, end to end against the full fp64 restatement, independence of the batch, the padding
and the optional outputs, one full-size case, animate(flame=) and the MEAD metrics and command lines, and a plain C++ client.  Outputs are NaN-filled before every call;
padded input rows are NaN.  (The blend uses fused multiply-adds, so there is no torch.equal against the float32 restatement.)"""
import functools

import numpy as np
import pytest
import torch

import flame_cases as FC
from fdm_amd import flame, metrics, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def nanpad(x, frames, L_max=None):
    """[B, L, n] host array -> device tensor with NaN in the rows past each clip's frames (and up to L_max)"""
    if x is None:
        return None
    x = x.copy() if L_max is None else np.concatenate([x, np.zeros((x.shape[0], L_max - x.shape[1], x.shape[2]), np.float32)], 1)
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return torch.from_numpy(x).to(DEV)


@functools.lru_cache(maxsize=None)
def plan_of(name):
    c, m, inp = FC.case(name)
    return flame.FlamePlan(m, None if inp["lv"] is None else (inp["lv"], inp["lb"]), DEV)


def run(name, clips=None, L_max=None, optional=True, extra="given"):
    """forward() into a NaN-filled output -> dict of host arrays [B, L, ...] (clips: a subset of the case's clips)"""
    c, m, inp = FC.case(name)
    sel = list(range(c["B"])) if clips is None else clips
    fr = [inp["frames"][b] for b in sel]
    cut = lambda k: None if inp[k] is None else inp[k][sel]  # noqa: E731
    sh = inp["shape"][sel] if inp["shape"].shape[0] > 1 else inp["shape"]
    L = inp["pose"].shape[1] if L_max is None else L_max
    xt = cut("extra")
    if extra == "zeros":
        xt = np.zeros((len(sel), inp["pose"].shape[1], 3 * m.V), np.float32)
    elif extra == "none":
        xt = None
    out = torch.full((len(sel), L, m.V, 3), float("nan"), device=DEV)
    plan = plan_of(name)
    args = (nanpad(cut("pose"), fr, L_max), nanpad(cut("expr"), fr, L_max) if c["NE"] else None, torch.from_numpy(sh) if c["NS"] else None,
            nanpad(cut("transl"), fr, L_max), nanpad(xt, fr, L_max), fr)
    if optional:
        ff, xf, pf = plan.forward(*args, xforms=True, out=out)
    else:
        ff, xf, pf = plan.forward(*args, landmarks=False, out=out), None, None
    assert ff.vertices is out and ff.frames == fr
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return dict(verts=host(out), lmk=host(ff.landmarks), xforms=host(xf), posefeat=host(pf), frames=fr)


@functools.lru_cache(maxsize=None)
def device_result(name):
    return run(name)


NAMES = list(FC.CASES) + ["full"]


@pytest.mark.parametrize("name", NAMES)
def test_pose_stage_within_four_times_the_float32_error(name):
    c, m, inp = FC.case(name)
    got, r64 = device_result(name), FC.restate(m, inp, np.float64)
    bound, e = FC.pose_bound(m, inp)
    assert FC.E_TABLE[name] / 2 <= e <= FC.E_TABLE[name] * 2          # the table of flame_cases.py is current
    xf, pf = FC.live(got["xforms"], got["frames"]), FC.live(got["posefeat"], got["frames"])
    ex = float(np.abs(xf.astype(np.float64) - r64["xforms"]).max()) if xf.size else 0.0
    ep = float(np.abs(pf.astype(np.float64) - r64["posefeat"]).max()) if pf.size else 0.0
    print(f"{name}: E = {e:.2e}, bound = {bound:.2e}, device |xforms - fp64| = {ex:.2e}, |posefeat - fp64| = {ep:.2e}")
    assert not np.isnan(xf).any() and not np.isnan(pf).any()
    assert ex <= bound and ep <= bound
    zero = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).reshape(12).astype(np.float32)
    first = [sum(got["frames"][:b]) for b in range(len(got["frames"])) if got["frames"][b]]
    assert np.array_equal(xf[first][:, :, [0, 1, 2, 4, 5, 6, 8, 9, 10]], np.broadcast_to(zero[[0, 1, 2, 4, 5, 6, 8, 9, 10]], (len(first), m.J, 9)))    # zero pose: R = I exactly
    assert np.all(pf[first] == 0)


@pytest.mark.parametrize("name", NAMES)
def test_blend_and_skin_within_the_a_priori_bound(name):
    """fp64 from the device's OWN fp32 transforms and pose features: what is left is stage B's rounding alone.  Every element."""
    c, m, inp = FC.case(name)
    got = device_result(name)
    D = m.tables()[0]
    xf, pf = FC.live(got["xforms"], got["frames"]), FC.live(got["posefeat"], got["frames"])
    want, S, n, _ = FC.blend_skin64(m, D, inp, xf, pf)
    v = FC.live(got["verts"], got["frames"])
    assert not np.isnan(v).any()
    err, bound = np.abs(v.astype(np.float64) - want), (n + 2) * FC.U * S
    print(f"{name}: n = {n}, worst err / bound = {float((err / bound).max()) if err.size else 0.0:.3f}")
    assert np.all(err <= bound)
    if got["lmk"] is not None:
        lm = FC.live(got["lmk"], got["frames"])
        lb, lv = inp["lb"].astype(np.float64), inp["lv"]
        v64 = v.astype(np.float64)                                    # from the device's own vertices: 3 terms
        wl = sum(lb[None, :, k, None] * v64[:, lv[:, k]] for k in range(3))
        Sl = sum(np.abs(lb[None, :, k, None] * v64[:, lv[:, k]]) for k in range(3))
        assert np.all(np.abs(lm.astype(np.float64) - wl) <= 5 * FC.U * Sl)


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_against_the_fp64_restatement(name):
    c, m, inp = FC.case(name)
    got, r64 = device_result(name), FC.restate(m, inp, np.float64)
    D = m.tables()[0]
    xf, pf = FC.live(got["xforms"], got["frames"]), FC.live(got["posefeat"], got["frames"])
    _, S, n, parts = FC.blend_skin64(m, D, inp, xf, pf)
    e4, _ = FC.pose_bound(m, inp)
    bound = (n + 2) * FC.U * S + FC.propagated(m, D, e4, parts)
    v = FC.live(got["verts"], got["frames"])
    err = np.abs(v.astype(np.float64) - r64["verts"])
    print(f"{name}: max |device - fp64| = {float(err.max()) if err.size else 0.0:.2e}, worst err / bound = {float((err / bound).max()) if err.size else 0.0:.3f}")
    assert np.all(err <= bound)
    if got["lmk"] is not None:
        lb = np.abs(inp["lb"].astype(np.float64))
        bl = sum(lb[None, :, k, None] * bound[:, inp["lv"][:, k]] for k in range(3)) + 5 * FC.U * sum(lb[None, :, k, None] * np.abs(r64["verts"][:, inp["lv"][:, k]]) for k in range(3))
        assert np.all(np.abs(FC.live(got["lmk"], got["frames"]).astype(np.float64) - r64["lmk"]) <= bl)


@pytest.mark.parametrize("name", ["v15", "v765", "v771"])
def test_a_clip_does_not_depend_on_the_batch_the_padding_or_the_optional_outputs(name):
    c, m, inp = FC.case(name)
    base = device_result(name)
    assert np.all(base["verts"][0] == 0) and np.all(base["xforms"][0] == 0)             # the 0-frame clip writes only zeros
    eq = lambda a, b: torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))  # noqa: E731
    wide = run(name, L_max=2 * FC.L_MAX + 1)
    bare = run(name, optional=False)
    assert eq(bare["verts"], base["verts"]) and bare["lmk"] is None
    for b, L in enumerate(base["frames"]):
        one = run(name, clips=[b])
        for got, i in ((one, 0), (wide, b)):
            for k in ("verts", "xforms", "posefeat") + (("lmk",) if base["lmk"] is not None else ()):
                assert eq(got[k][i, :L], base[k][b, :L]), (k, b)
                assert np.all(got[k][i, L:] == 0)
    if c["extra"]:
        assert not eq(run(name, extra="none")["verts"], base["verts"])
    assert eq(run(name, extra="zeros")["verts"], run(name, extra="none")["verts"])       # x + 0 = x: the rule makes this exact


# ---- the pipeline (tiny preset on the full VOCASET geometry, as tests/test_rig_out_gpu.py)
V_PIPE = 5023


@functools.lru_cache(maxsize=None)
def tiny_models():
    return pipeline.build_models("vocaset", None, DEV)


@functools.lru_cache(maxsize=None)
def pipe_head():
    return flame.FlameModel.synthetic(V_PIPE, 5, 12, 8, seed=21)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


def test_animate_with_flame_poses_the_offsets_it_decodes():
    diffusion, ae = tiny_models()
    m, wav = pipe_head(), tiny_audio(0.6, 1)
    tmpl = (1e-1 * np.random.default_rng(12).standard_normal((1, 3 * V_PIPE))).astype(np.float32)
    args = dict(ddim_steps=3, seed=2, device=DEV)
    offs, lat = pipeline.animate(diffusion, ae, wav, None, **args)
    want, _ = pipeline.animate(diffusion, ae, wav, tmpl, **args)
    same, _ = pipeline.animate(diffusion, ae, wav, tmpl, flame=None, **args)
    assert torch.equal(same, want)                                                     # flame=None: every path as before
    L = offs.shape[1]
    g = np.random.default_rng(13)
    pose = (0.2 * g.standard_normal((L + 3, 15))).astype(np.float32)
    fl = dict(model=m, pose=pose, shape=g.standard_normal(5).astype(np.float32), transl=g.standard_normal((L + 3, 3)).astype(np.float32))
    got, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, flame=fl, **args)
    ref = pipeline.to_flame(torch.from_numpy(pose[:L]).to(DEV), m, shape=fl["shape"], transl=torch.from_numpy(fl["transl"][None, :L]).to(DEV), extra=offs)
    assert torch.equal(lat, lat2) and got.shape == offs.shape and torch.equal(got, ref.vertices.reshape(offs.shape))
    assert float((got - want).abs().max()) > 1e-2                                      # posed, and the template argument is not read
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    mf, _ = pipeline.animate(diffusion, ae, wav, tmpl, flame=fl, faces=faces, **args)
    assert torch.equal(mf.positions.reshape(offs.shape), got)
    many, _ = pipeline.animate_many(diffusion, ae, [wav], None, flame=fl, **args)
    assert torch.equal(many[0], got)
    long, _ = pipeline.animate_long(diffusion, ae, wav, tmpl, flame=fl, **args)
    assert torch.equal(long, got)                                                      # (fits one window: animate()'s bits)


def test_mead_metrics_from_parameters_equal_the_call_with_torch2mesh_vertices():
    m = flame.FlameModel.synthetic(300, 5, 60, 10, seed=22)
    plan = flame.FlamePlan(m, device=DEV)
    g = np.random.default_rng(23)
    F = 6
    ex, p6 = g.standard_normal((F, 50)).astype(np.float32), (0.2 * g.standard_normal((F, 6))).astype(np.float32)
    gt = flame.torch2mesh(plan, ex, p6)
    assert gt.shape == (1, F, 900) and torch.equal(gt, torch.round(gt, decimals=4))
    ff = plan.forward(flame.full_pose(torch.from_numpy(p6)).unsqueeze(0), torch.from_numpy(ex).unsqueeze(0))
    assert torch.equal(gt.reshape(F, 300, 3), torch.round(ff.vertices[0], decimals=4))
    pred = gt.reshape(F, 300, 3).cpu() + torch.from_numpy((1e-3 * g.standard_normal((F, 300, 3))).astype(np.float32))
    regions = [list(range(0, 100)), list(range(50, 80)), list(range(200, 300))]
    a = metrics.mead_vertex_metrics(gt.reshape(F, 300, 3), pred, *regions, device=DEV)
    b = metrics.mead_vertex_metrics(None, pred, *regions, device=DEV, gt_params=(ex, p6), flame=plan)
    assert a == b and a["ALL"] > 0


def test_animate_with_flame_under_several_conditions_and_refusals():
    """S = 2 conditions per clip: a [L', 3 J] pose serves every row; a malformed flame= and flame= with rig= alone are refused."""
    diffusion, ae = tiny_models()
    m, wav = pipe_head(), tiny_audio(0.6, 1)
    args = dict(ddim_steps=2, seed=2, device=DEV)
    ids = torch.eye(8)[:2]
    offs, _ = pipeline.animate(diffusion, ae, wav, None, ids, **args)
    L = offs.shape[1]
    pose = (0.2 * np.random.default_rng(31).standard_normal((L, 15))).astype(np.float32)
    got, _ = pipeline.animate(diffusion, ae, wav, None, ids, flame=dict(model=m, pose=pose), **args)
    ref = pipeline.to_flame(torch.from_numpy(pose).to(DEV).expand(2, L, 15), m, extra=offs)
    assert got.shape == offs.shape == (2, L, 3 * V_PIPE) and torch.equal(got, ref.vertices.reshape(offs.shape))
    with pytest.raises(ValueError, match="flame="):
        pipeline.animate(diffusion, ae, wav, None, flame=dict(model=m), **args)
    with pytest.raises(ValueError, match="flame="):
        pipeline.animate(diffusion, ae, wav, None, flame=dict(model=m, pose=pose, jaw=1), **args)
    E = (1e-2 * np.random.default_rng(32).standard_normal((4, 3 * V_PIPE))).astype(np.float32)
    with pytest.raises(ValueError, match="rig="):
        pipeline.animate(diffusion, ae, wav, None, flame=dict(model=m, pose=pose), rig=dict(basis=E, ridge=1e-3), **args)


def test_c_client_poses_a_head_without_python(tmp_path):
    """tests/abi_c/flame_client.cpp: fdm_flame_create -> fdm_flame_forward with no Python in the process, checked in the program against
    the rule in fp64."""
    import os
    import shutil
    import subprocess
    from fdm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "flame_client")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", os.path.join(root, "tests", "abi_c", "flame_client.cpp"),
           "-I", os.path.join(root, "include"), "-L", libdir, "-lfdm_hip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flame_client ok" in r.stdout
    print(r.stdout.strip())


def _mead_set(tmp_path, m, seed):
    """A MEAD-shaped evaluation set for model m: predictions, ground-truth parameter files and region files under tmp_path"""
    g = np.random.default_rng(seed)
    plan = flame.FlamePlan(m, device=DEV)
    n_expr = m.NB - m.expr_at
    pred_dir, gt_dir, reg_dir = tmp_path / "npy", tmp_path / "gt", tmp_path / "region"
    for d in (pred_dir, gt_dir / "M003", reg_dir):
        d.mkdir(parents=True)
    regions = dict(face=np.arange(0, m.V, 2), lip=np.arange(10, 40), emotion=np.arange(m.V // 2, m.V))
    for k, r in regions.items():
        np.save(reg_dir / f"{k}_vertices.npy", r)
    names = ["M003_front_angry_level-1_001_ConditionEmotion_angry.npy", "M003_front_angry_level-2_007_ConditionEmotion_angry.npy",
             "M003_front_happy_level-1_002_ConditionEmotion_happy.npy", "M003_front_angry_level-3_009_ConditionEmotion_angry.npy"]
    want_gt, want_pred = [], []
    for i, name in enumerate(names):
        T, Tp = 5 + i, 6
        ex = g.standard_normal((T, n_expr)).astype(np.float32)
        pose = (0.2 * g.standard_normal((T, 6))).astype(np.float32)
        sub, gname = metrics.mead_gt_name(name)
        if i != 3:                                                  # the last prediction has no ground truth: skipped
            np.savez(gt_dir / sub / gname, expression=ex, pose=pose)
        p6 = np.concatenate([np.zeros((T, 3), np.float32), pose[:, 3:]], 1)     # the global rotation is dropped
        gt = flame.torch2mesh(plan, ex, p6).reshape(T, m.V, 3)
        pred = (gt[:1].cpu().expand(Tp, -1, -1) + torch.from_numpy((1e-3 * g.standard_normal((Tp, m.V, 3))).astype(np.float32))).numpy()
        np.save(pred_dir / name, pred.reshape(1, Tp, -1))
        if "angry" in name and i != 3:
            n = min(T, Tp)
            want_gt.append(gt[:n].cpu())
            want_pred.append(torch.from_numpy(pred[:n]))
    return plan, regions, torch.cat(want_gt), torch.cat(want_pred), (str(pred_dir), str(gt_dir), str(reg_dir))


def test_mead_evaluate_builds_the_ground_truth_from_parameter_files(tmp_path, capsys):
    m = flame.FlameModel.synthetic(300, 5, 60, 10, seed=24)
    m.save(tmp_path / "head.npz")
    plan, regions, gt, pred, (pp, gp, rp) = _mead_set(tmp_path, m, 25)
    res = metrics.mead_evaluate(pp, gp, str(tmp_path / "head.npz"), rp, DEV, verbose=False)
    want = metrics.mead_vertex_metrics(gt, pred, regions["face"], regions["lip"], regions["emotion"], DEV)
    assert res["frames"] == gt.shape[0] == 5 + 6 and len(res["files"]) == 2 and all("angry" in f for f in res["files"])
    assert {k: res[k] for k in want} == want and res["ALL"] > 0
    tmpl = flame.torch2mesh(plan, torch.zeros(1, 50), torch.zeros(1, 6)).reshape(300, 3)
    assert torch.equal(res["template"], tmpl)
    assert res["motion_std_gt"][0] == metrics.motion_std(gt[:5], tmpl, regions["emotion"], DEV)
    assert res["motion_std_pred"][1] == metrics.motion_std(pred[5:], tmpl, regions["emotion"], DEV)
    cli = metrics.mead_main(["--pred_path", pp, "--gt_path", gp, "--region_path", rp, "--flame_model", str(tmp_path / "head.npz"), "--device", DEV])
    assert {k: cli[k] for k in want} == want and "Face Vertex Error (FVE)" in capsys.readouterr().out
    every = metrics.mead_evaluate(pp, gp, plan, rp, DEV, pick=None, verbose=False)
    assert len(every["files"]) == 3 and every["frames"] == 5 + 6 + 6


def test_sampler_command_line_makes_the_template_from_flame_parameters(tmp_path):
    """The MEAD sampler command line with --flame_model (2M 3): the saved vertices are animate() with the template torch2mesh makes from the
    parameter file -- the neutral face without --template_params."""
    import importlib.util
    import os
    import sys
    from fdm_amd import presets
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sd = os.path.join(here, "face-diffusion-model_amd", "dropin", "samples")
    sys.path.insert(0, os.path.dirname(sd))
    spec = importlib.util.spec_from_file_location("sample_diffusion", os.path.join(sd, "sample_diffusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pm = presets.get("mead")
    m = flame.FlameModel.synthetic(pm.V3 // 3, 5, 56, 6, seed=26)
    m.save(tmp_path / "head.npz")
    prm = (0.3 * np.random.default_rng(27).standard_normal((1, 56))).astype(np.float32)
    np.save(tmp_path / "params.npy", prm)
    out = str(tmp_path / "mead")
    flags = ["--clips", "1", "--seconds", "1.0", "--sampler", "dpmpp2m", "--sampler_steps", "3", "--out", out, "--device", DEV]
    mod.main("mead", flags + ["--flame_model", str(tmp_path / "head.npz"), "--template_params", str(tmp_path / "params.npy")])
    plan = flame.FlamePlan(m, device=DEV)
    tmpl = flame.torch2mesh(plan, prm[:, :50], prm[:, 50:])[0]
    assert torch.equal(pipeline.flame_template(m, prm, DEV), tmpl) and tmpl.shape == (1, pm.V3)
    neutral = pipeline.flame_template(str(tmp_path / "head.npz"), None, DEV)
    assert float((neutral.cpu() - torch.from_numpy(m.v_template.reshape(1, -1))).abs().max()) <= 1e-4      # zero parameters: the template, to 4 decimals
    audio, _, one_hot_all, name = next(iter(mod.synthetic_loader(pm, 1, 1.0)))
    diffusion, ae = pipeline.build_models("mead", None, DEV, "", "", single_clip=True)
    ref, _ = pipeline.animate(diffusion, ae, audio, tmpl, one_hot_all[:, 0, :], torch.eye(7)[4:5], device=DEV, sampler="dpmpp2m", sampler_steps=3)
    files = [f for f in os.listdir(out) if f.endswith(".npy")]
    assert len(files) == 1 and torch.equal(torch.from_numpy(np.load(os.path.join(out, files[0]))), ref.cpu())
    with pytest.raises(ValueError, match="--flame_model"):
        mod.main("mead", flags + ["--template_params", str(tmp_path / "params.npy")])
