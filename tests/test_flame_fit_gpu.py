"""GPU: FlamePlan.fit / fdm_flame_fit_* against the fp64 restatement of tests/flame_fit_cases.py (bounds derived there), the round trip
through FlamePlan.forward, independence of rows and batches, and degenerate rows."""
import functools

import numpy as np
import pytest
import torch

import flame_cases as FC
import flame_fit_cases as K
from fdm_amd import flame

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _padded(tru, key, rows_nan=False):
    """[B, L, ...] float32 tensor of a truth array; rows at or past frames[b] are NaN when rows_nan"""
    x = np.array(tru[key], dtype=np.float32, copy=True)
    if rows_nan:
        for b, n in enumerate(tru["frames"]):
            x[b, n:] = np.nan
    return torch.from_numpy(x).to(DEV)


@pytest.fixture(scope="module")
def setup():
    cache = {}

    def get(name):
        if name not in cache:
            c, m, tru = K.case(name)
            plan = flame.FlamePlan(m, device=DEV)
            sh = torch.from_numpy(tru["shape"]).to(DEV) if c["NS"] else None
            ff = plan.forward(_padded(tru, "pose"), _padded(tru, "expr"), shape=sh, transl=_padded(tru, "transl") if c["transl"] else None,
                              frames=tru["frames"], landmarks=False)
            y = ff.vertices.clone()
            kw = dict(n_expr=c["n_expr"], joints=c["free"], transl=c["transl"], shape=sh, pose0=_padded(tru, "pose0"), frames=tru["frames"])
            cache[name] = (c, m, tru, plan, y, kw)
        return cache[name]
    return get


def _live(x, frames):
    return FC.live(x.detach().cpu().numpy(), frames)


@pytest.mark.parametrize("name", K.SMALL + K.STEP_EXTRA)
def test_one_step_per_element(setup, name):
    c, m, tru, plan, y, kw = setup(name)
    _, _, r = K.truth_rows(name)
    free, ne, tr, P, lam = c["free"], c["n_expr"], c["transl"], K.n_params(c), K.step_lam(c)
    theta0 = K.join(np.zeros_like(r["ex"]), r["p0"], np.zeros_like(r["tr"]), free, tr).astype(np.float64)
    theta = (0.5 * (theta0 + r["theta"])).astype(np.float32)
    ex, ps, t3 = K.split(theta, r["p0"], free, ne, tr)
    B, L = tru["pose"].shape[:2]

    def pad(a):
        out = np.zeros((B, L, a.shape[1]), np.float32)
        out[r["b"], r["t"]] = a
        return torch.from_numpy(out).to(DEV)
    got = plan.fit_step(y, pad(ex), pad(ps), pad(t3), n_expr=ne, joints=free, fit_transl=tr, shape=kw["shape"], pose0=kw["pose0"], lam=lam, frames=tru["frames"])
    torch.cuda.synchronize()
    yl = _live(y.reshape(B, L, m.V, 3), tru["frames"])
    d64, s64, p64 = K.step(m, theta, yl, r["sh"], r["p0"], free, ne, tr, np.float64, lam=lam, parts=True)
    assert s64.max() == 0 and int(got["status"].max()) == 0
    e_pose, e_deriv = K.deriv_bound(m, r["sh"], ex, ps, free, ne)
    for key, ref, e in (("xforms", p64["st"]["A"], e_pose), ("dX", p64["dX"], e_deriv), ("dE", p64["dE"], e_deriv)):
        if ref.size:
            err = float(np.abs(_live(got[key], tru["frames"]).astype(np.float64) - ref).max())
            print(name, key, "max err", err, "bound", e)
            assert err <= e
    G = K.unpack(_live(got["H"], tru["frames"]).astype(np.float64), P)
    dG = K.step_bounds(m, p64, yl.astype(np.float64), None, free, ne, tr, r["sh"].shape[1], e_pose, e_deriv)
    err = np.abs(np.triu(G - p64["G"]))
    print(name, "H, g max err / bound", float((err / np.maximum(np.triu(dG), 1e-300)).max()))
    assert np.all(err <= np.triu(dG))
    H64, g64 = K.full_sym(p64["G"], P)
    dH, dg = K.full_sym(dG, P)
    bound = K.solve_bound(H64 + np.eye(P)[None] * lam, -g64, d64, dH, dg, P)
    dd = np.linalg.norm(_live(got["delta"], tru["frames"]).astype(np.float64) - d64, axis=1)
    print(name, "delta max err / bound", float((dd / bound).max()))
    assert np.all(dd <= bound)


def _forward_floor(m, plan, c, tru, fit):
    """F [N]: the RMS over the vertices of the forward's own a-priori bound at the fitted parameters (flame_cases.blend_skin64 / propagated)"""
    ff, xf, pf = plan.forward(fit.pose, fit.expression, shape=None if not c["NS"] else torch.from_numpy(tru["shape"]).to(DEV),
                              transl=fit.transl if c["transl"] else None, frames=tru["frames"], landmarks=False, xforms=True)
    inp = dict(shape=tru["shape"], expr=fit.expression.cpu().numpy(), pose=fit.pose.cpu().numpy(), transl=fit.transl.cpu().numpy() if c["transl"] else None,
               extra=None, frames=tru["frames"], lv=None, lb=None)
    for k in ("expr", "pose", "transl"):
        if inp[k] is not None:
            inp[k] = np.nan_to_num(inp[k])
    D = m.tables()[0]
    _, S, n, parts = FC.blend_skin64(m, D, inp, _live(xf, tru["frames"]), _live(pf, tru["frames"]))
    e, _ = FC.pose_bound(m, inp)
    per = (n + 2) * 2.0 ** -24 * S + FC.propagated(m, D, e, parts)
    return np.sqrt((per ** 2).sum(-1).mean(-1))


@pytest.mark.parametrize("name", K.SMALL + ("full",))
def test_recovery_and_round_trip(setup, name):
    c, m, tru, plan, y, kw = setup(name)
    _, _, r = K.truth_rows(name)
    fit = plan.fit(y, return_vertices=True, **kw)
    again = plan.fit(y, return_vertices=True, **kw)
    torch.cuda.synchronize()
    for a, b in zip(fit[:5], again[:5]):
        assert torch.equal(a, b)                             # no atomics: two runs agree bit for bit
    assert int(fit.status.max()) == 0
    B, L = tru["pose"].shape[:2]
    yl = _live(y.reshape(B, L, m.V, 3), tru["frames"])
    ref = K.fit(m, yl, r["sh"], r["p0"], c["free"], c["n_expr"], c["transl"], np.float64)
    F = _forward_floor(m, plan, c, tru, fit)
    rms = _live(fit.rms, tru["frames"]).astype(np.float64)
    print(name, "rms device", rms.max(), "fp64", ref["rms"].max(), "floor F", F.max(), "excess / (margin F)", float(((rms - ref["rms"]) / (K.RMS_MARGIN * F)).max()))
    assert np.all(rms <= ref["rms"] + K.RMS_MARGIN * F)
    # parameters against truth through the restatement: the smallest singular value of the fp64 Jacobian at the truth
    _, _, p64 = K.step(m, r["theta"], yl, r["sh"], r["p0"], c["free"], c["n_expr"], c["transl"], np.float64, parts=True)
    P = K.n_params(c)
    Jm = p64["Z"][..., :P].reshape(len(F), 3 * m.V, P)
    smin = np.array([np.linalg.svd(Jm[i], compute_uv=False)[-1] for i in range(len(F))])
    th = K.join(_live(fit.expression, tru["frames"]), _live(fit.pose, tru["frames"]), _live(fit.transl, tru["frames"]), c["free"], c["transl"]).astype(np.float64)
    tol = K.RMS_MARGIN * F * np.sqrt(3 * m.V) / smin + np.abs(ref["theta"] - r["theta"]).max(1)
    dth = np.linalg.norm(th - r["theta"], axis=1)
    print(name, "max |theta - truth| / tol", float((dth / tol).max()))
    assert np.all(dth <= tol)
    # round trip: forward(fit(y)) is y within the same bound, and the returned vertices are the forward's own
    ff = plan.forward(fit.pose, fit.expression if c["n_expr"] else None, shape=kw["shape"], transl=fit.transl if c["transl"] else None,
                      frames=tru["frames"], landmarks=False)
    assert torch.equal(ff.vertices, fit.vertices)
    d = _live(ff.vertices, tru["frames"]).astype(np.float64) - yl
    back = np.sqrt((d ** 2).sum(-1).mean(-1))
    assert np.all(back <= ref["rms"] + K.RMS_MARGIN * F)
    for x in fit[:5] + (fit.vertices,):                      # rows at or past frames[b] are zeros
        FC.live(x.cpu().numpy(), tru["frames"])


def test_independence_and_padding(setup):
    c, m, tru, plan, y, kw = setup("v257_jaw")
    B, L = tru["pose"].shape[:2]
    base = plan.fit(y, **kw)
    # NaN in the targets' padding and in dead rows of pose0
    yn, pn = y.clone(), kw["pose0"].clone()
    for b, n in enumerate(tru["frames"]):
        yn[b, n:] = float("nan")
        pn[b, n:] = float("nan")
    nan = plan.fit(yn, **dict(kw, pose0=pn))
    for a, b in zip(base[:5], nan[:5]):
        assert torch.equal(a, b)
    # clip 1 alone, at its own L_max, against its rows inside the batch
    n1 = tru["frames"][1]
    sh = kw["shape"]
    alone = plan.fit(y[1:2, :n1].contiguous(), **dict(kw, shape=None if sh is None else sh[1:2], pose0=kw["pose0"][1:2, :n1].contiguous(), frames=[n1]))
    for a, b in zip(base[:5], alone[:5]):
        assert torch.equal(a[1, :n1], b[0])
    torch.cuda.synchronize()


def test_degenerate_rows(setup):
    """all but one weight zero, lambda = rho = 0: rank 3 < P = 10, every live row of THIS plan fails at a pivot, keeps its start and stays
    finite; a healthy fit on the same head before and after is unchanged"""
    c, m, tru, plan, y, kw = setup("v257_jaw")
    healthy = plan.fit(y, **kw)
    w = np.zeros(m.V, np.float32)
    w[11] = 1.0
    bad = plan.fit(y, weights=w, lam=0.0, ridge_expr=0.0, ridge_pose=0.0, iters=3, **kw)
    after = plan.fit(y, **kw)
    torch.cuda.synchronize()
    st = bad.status.cpu().numpy()
    for b, n in enumerate(tru["frames"]):
        assert np.all(st[b, :n] > 0) and np.all(st[b, n:] == 0)
    assert torch.equal(bad.expression, torch.zeros_like(bad.expression))
    p0 = kw["pose0"].clone()
    for b, n in enumerate(tru["frames"]):
        p0[b, n:] = 0
    assert torch.equal(bad.pose, p0)
    assert bool(torch.isfinite(bad.rms).all())
    for a, b in zip(healthy[:5], after[:5]):
        assert torch.equal(a, b)


def test_a_degenerate_row_beside_healthy_rows_in_one_launch():
    """One weight vector (all but one vertex zero), lambda = rho = 0, expression only (P = 2), a two-joint model whose expression
    directions do not move the joints (dE = 0) and whose weighted vertex is skinned half and half.  In frame 2 pose0 turns joint 1 by pi
    about x: the blended rotation (I + R) / 2 is then the projection on x up to sin(pi in fp32) ~ 1e-7, both columns are parallel,
    the second pivot is ~1e-14 of its diagonal and the row fails.  The other frames (small pose0) are healthy.  They share the row
    tile, the LDS block, the partials and the solve launch with the bad frame: their results are torch.equal to the same batch with
    the bad frame's pose0 replaced by a healthy one.  The failure rests on the default pivot_tol (2^-18): under pivot_tol = 0, the plain
    test pivot > 0, a pivot of ~1e-14 of its diagonal is decided by rounding noise and this frame may pass with a huge step."""
    from fdm_amd import flame as F
    base = F.FlameModel.synthetic(40, 2, 4, 1, seed=5, parents=[0, 0])
    sd = base.shapedirs.copy()
    used = np.nonzero(base.j_regressor.any(0))[0]
    sd[used] = 0                                           # JD = j_regressor . shapedirs = 0: the joints do not move with the coefficients
    vstar = int(np.setdiff1d(np.arange(40), used)[0])
    w = base.lbs_weights.copy()
    w[vstar] = [0.5, 0.5]
    m = F.FlameModel(base.v_template, sd, base.posedirs, base.j_regressor, base.parents, w, base.expr_at)
    plan = F.FlamePlan(m, device=DEV)
    g = np.random.default_rng(6)
    L = 5
    p0 = (0.05 * g.standard_normal((1, L, 6))).astype(np.float32)
    bad = p0.copy()
    bad[0, 2] = [0, 0, 0, np.pi, 0, 0]
    ex = g.uniform(-1, 1, (1, L, 2)).astype(np.float32)
    y = plan.forward(torch.from_numpy(p0).to(DEV), torch.from_numpy(ex).to(DEV), landmarks=False).vertices.clone()
    mw = np.zeros(40, np.float32)
    mw[vstar] = 1.0
    kw = dict(n_expr=2, joints=(), weights=mw, lam=0.0, ridge_expr=0.0, ridge_pose=0.0, iters=4)
    mixed = plan.fit(y, pose0=torch.from_numpy(bad).to(DEV), **kw)
    clean = plan.fit(y, pose0=torch.from_numpy(p0).to(DEV), **kw)
    torch.cuda.synchronize()
    st = mixed.status[0].cpu().numpy()
    print("status", st, "clean", clean.status[0].cpu().numpy())
    assert st[2] > 0 and np.all(st[[0, 1, 3, 4]] == 0) and int(clean.status.max()) == 0
    assert torch.equal(mixed.expression[0, 2], torch.zeros(2, device=DEV))                 # theta stays at the start
    assert torch.equal(mixed.pose[0, 2].cpu(), torch.from_numpy(bad[0, 2]))
    keep = torch.tensor([0, 1, 3, 4], device=DEV)
    for a, b in zip(mixed[:4], clean[:4]):
        assert torch.equal(a[0, keep], b[0, keep])
    assert bool(torch.isfinite(mixed.rms).all()) and bool(torch.isfinite(mixed.expression).all())


def test_joints_only_fit(setup):
    """n_expr = 0: no expression output is needed"""
    c, m, tru, plan, y, kw = setup("v257_jaw")
    ps = _padded(tru, "pose")
    yy = plan.forward(ps, None, shape=kw["shape"], frames=tru["frames"], landmarks=False).vertices
    fit = plan.fit(yy, return_vertices=True, **dict(kw, n_expr=0))
    assert fit.expression.shape[-1] == 0 and int(fit.status.max()) == 0
    back = plan.forward(fit.pose, None, shape=kw["shape"], frames=tru["frames"], landmarks=False)
    assert torch.equal(back.vertices, fit.vertices)
    assert float(fit.rms.max()) < float((yy - plan.forward(kw["pose0"], None, shape=kw["shape"], frames=tru["frames"], landmarks=False).vertices).pow(2).sum(-1).mean(-1).sqrt().max())


def test_linear_cross_check_against_the_rig_fit(setup):
    """no free joint, pose0 = 0, no shape: F = template + expr . D exactly (T = I: the weights sum to one only up to rounding, which the
    bound below carries), so the fit solves the normal equations (B B^T + rho I) c = B (y - template) that to_rig(offsets, basis,
    ridge=rho) solves.  Both are fp32 solutions of the same SPD system: each is within kappa_2 (C_P u + eA + eb) / (1 - ..) of the fp64
    solution (flame_fit_cases.solve_bound, with the per-element bound of a 3 V-term fp32 Gram sum, gamma_(3V + 2) sum |terms|, and the
    same for the right side, plus the skinning's own gamma_(2 J + 4) on the columns), so they are within the sum of the two bounds."""
    from fdm_amd import pipeline
    c, m, tru, plan, _, _ = setup("v257_jn")
    ne, rho = c["n_expr"], 1e-3
    g = np.random.default_rng(9)
    Bn, L = 2, 4
    Bs = m.expression_basis(ne).astype(np.float64)                                         # [ne, 3V]
    coef = g.uniform(-2, 2, (Bn, L, ne))
    offs = (coef @ Bs + 1e-3 * g.standard_normal((Bn, L, 3 * m.V))).astype(np.float32)
    offs_t = torch.from_numpy(offs).to(DEV)
    y = offs_t + torch.from_numpy(m.v_template.reshape(1, 1, -1)).to(DEV)
    fit = plan.fit(y, n_expr=ne, joints=(), lam=0.0, ridge_expr=rho, iters=1)
    rf = pipeline.to_rig(offs_t, m.expression_basis(ne), ridge=rho)
    torch.cuda.synchronize()
    assert int(fit.status.max()) == 0
    yo = (y.cpu().numpy().astype(np.float64) - m.v_template.reshape(1, 1, -1).astype(np.float64)).reshape(Bn * L, -1)
    A = Bs @ Bs.T + rho * np.eye(ne)
    rhs = yo @ Bs.T
    x64 = np.linalg.solve(A, rhs.T).T
    n, k = 3 * m.V, 2 * m.J + 4
    dH = (n + 2 + 2 * k) * K.U * (np.abs(Bs) @ np.abs(Bs).T)
    dg = (n + 2 + 2 * k) * K.U * ((np.abs(yo) + np.abs(m.v_template.reshape(1, -1))) @ np.abs(Bs).T)
    bound = K.solve_bound(np.broadcast_to(A, (Bn * L, ne, ne)), rhs, x64, np.broadcast_to(dH, (Bn * L, ne, ne)), dg, ne)
    e_fit = np.linalg.norm(fit.expression.cpu().numpy().reshape(Bn * L, ne).astype(np.float64) - x64, axis=1)
    e_rig = np.linalg.norm(rf.weights.cpu().numpy().reshape(Bn * L, ne).astype(np.float64) - x64, axis=1)
    d = np.linalg.norm((fit.expression - rf.weights.reshape(fit.expression.shape)).cpu().numpy().reshape(Bn * L, ne).astype(np.float64), axis=1)
    print("fit vs fp64 / bound", float((e_fit / bound).max()), "rig vs fp64 / bound", float((e_rig / bound).max()), "fit vs rig / 2 bound", float((d / (2 * bound)).max()))
    assert np.all(e_fit <= bound) and np.all(d <= 2 * bound)


def test_to_flame_params_forms(setup):
    from fdm_amd import pipeline
    c, m, tru, plan, y, kw = setup("v257_jaw")
    B, L = tru["pose"].shape[:2]
    tmpl = torch.from_numpy(m.v_template.reshape(1, -1)).to(DEV)
    offs = (y.reshape(B, L, -1) - tmpl.unsqueeze(1)).contiguous()
    args = dict(n_expr=c["n_expr"], joints=("jaw",), iters=6)
    a = pipeline.to_flame_params(offs, m, tmpl, frames=tru["frames"], **args)
    b = plan.fit((offs + tmpl.unsqueeze(1)).contiguous(), frames=tru["frames"], **args)
    for u, v in zip(a[:5], b[:5]):
        assert torch.equal(u, v)
    clips = [offs[i:i + 1, :n].contiguous() for i, n in enumerate(tru["frames"])]
    per = pipeline.to_flame_params(clips, m, [tmpl] * B, **args)
    for i, n in enumerate(tru["frames"]):
        assert per[i].frames == [n] and torch.equal(per[i].expression[0], a.expression[i, :n]) and torch.equal(per[i].pose[0], a.pose[i, :n])
    # fps: the targets are resampled by the mesh hand-off's frame rule before the fit
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    mf = pipeline.to_mesh(offs, faces, tmpl, frames=tru["frames"], fps=(30, 60), normals=False)
    r = pipeline.to_flame_params(offs, m, tmpl, frames=tru["frames"], fps=(30, 60), **args)
    assert r.frames == list(mf.frames)
    ref = plan.fit(mf.positions.reshape(B, -1, 3 * m.V).contiguous(), frames=list(mf.frames), **args)
    assert torch.equal(r.expression, ref.expression) and torch.equal(r.pose, ref.pose)



@functools.lru_cache(maxsize=None)
def _tiny():
    from fdm_amd import pipeline
    return pipeline.build_models("vocaset", None, DEV)


def test_pipeline_takes_flame_fit():
    from fdm_amd import pipeline
    diffusion, ae = _tiny()
    m = flame.FlameModel.synthetic(5023, 5, 12, 8, seed=21)
    wav = (0.1 * torch.randn(int(16000 * 0.6), generator=torch.Generator().manual_seed(1))).numpy()
    tmpl = m.v_template.reshape(1, -1).copy()
    args = dict(ddim_steps=3, seed=2, device=DEV)
    ffd = dict(model=m, n_expr=4, joints=("jaw",), iters=4)
    plain, lat = pipeline.animate(diffusion, ae, wav, tmpl, **args)
    same, _ = pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=None, **args)
    assert torch.equal(plain, same)
    got, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=ffd, **args)
    ref = pipeline.to_flame_params(plain, m, n_expr=4, joints=("jaw",), iters=4)
    assert isinstance(got, flame.FlameFit) and torch.equal(lat, lat2)
    for u, v in zip(got[:5], ref[:5]):
        assert torch.equal(u, v)
    many, _ = pipeline.animate_many(diffusion, ae, [wav], [tmpl], flame_fit=ffd, **args)
    long, _ = pipeline.animate_long(diffusion, ae, wav, tmpl, flame_fit=ffd, **args)
    for other in (many[0], long):
        assert torch.equal(other.expression.reshape(got.expression.shape), got.expression) and torch.equal(other.pose.reshape(got.pose.shape), got.pose)
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    mf, ff = pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=ffd, faces=faces, **args)[0]
    assert torch.equal(mf.positions.reshape(plain.shape), plain) and torch.equal(ff.expression, got.expression)
    with pytest.raises(ValueError, match="flame_fit= with flame="):
        pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=ffd, flame=dict(model=m, pose=np.zeros((40, 15), np.float32)), **args)
    with pytest.raises(ValueError, match="flame_fit= with wrap="):
        pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=ffd, wrap=dict(target=np.zeros((4, 3), np.float32)), **args)
    with pytest.raises(ValueError, match="flame_fit= takes"):
        pipeline.animate(diffusion, ae, wav, tmpl, flame_fit=dict(n_expr=4), **args)
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV)
    h = srv.submit_many([wav], [tmpl], seeds=1)
    v0 = {k: v for k, v, _ in srv.drain(2)}[h[0]]
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, flame_fit=ffd)
    h2 = srv.submit_many([wav], [tmpl], seeds=1)
    f2 = {k: v for k, v, _ in srv.drain(2)}[h2[0]]
    r2 = pipeline.to_flame_params(v0, m, n_expr=4, joints=("jaw",), iters=4)
    assert isinstance(f2, flame.FlameFit) and torch.equal(f2.expression, r2.expression) and torch.equal(f2.pose, r2.pose)


def test_demo_command_line_writes_the_flame_npz(tmp_path):
    """demo --flame_fit --flame_model file.npz --fit_joints jaw,neck --fit_expr 4 --fit_iters 3 on the tiny preset: <stem>_flame.npz holds
    the four keys with the documented shapes, equal to to_flame_params of the frames in <stem>.npy; <stem>.npy is what the command
    line writes without the flags."""
    from scipy.io import wavfile
    from fdm_amd import pipeline
    m = flame.FlameModel.synthetic(5023, 5, 12, 8, seed=21)
    wp, mp, tp = str(tmp_path / "hello.wav"), str(tmp_path / "head.npz"), str(tmp_path / "template.npy")
    wav = (0.1 * torch.randn(int(16000 * 0.5), generator=torch.Generator().manual_seed(3))).numpy()
    wavfile.write(wp, 16000, (wav * 20000).astype(np.int16))
    m.save(mp)
    np.save(tp, m.v_template.reshape(1, -1))
    base = ["--audio_file", wp, "--ddim_steps", "2", "--device", DEV, "--template_file", tp]
    plain = np.load(pipeline.demo_main("vocaset", base + ["--audio_path", str(tmp_path / "plain")]))
    dst = pipeline.demo_main("vocaset", base + ["--audio_path", str(tmp_path / "out"), "--flame_fit", "--flame_model", mp, "--fit_joints", "jaw,neck",
                                                "--fit_expr", "4", "--fit_iters", "3"])
    got = np.load(dst)
    assert np.array_equal(got, plain)
    z = np.load(dst[:-4] + "_flame.npz")
    L = got.shape[1]
    assert sorted(z.files) == ["expression", "pose", "rms", "transl"]
    assert z["expression"].shape == (1, L, 4) and z["pose"].shape == (1, L, 15) and z["transl"].shape == (1, L, 3) and z["rms"].shape == (1, L)
    ref = pipeline.to_flame_params(torch.from_numpy(got).to(DEV), flame.FlameModel.load(mp), n_expr=4, joints=("jaw", "neck"), iters=3)
    assert np.array_equal(z["expression"], ref.expression.cpu().numpy()) and np.array_equal(z["pose"], ref.pose.cpu().numpy())
    assert np.array_equal(z["rms"], ref.rms.cpu().numpy()) and not z["transl"].any()
    with pytest.raises(ValueError, match="--flame_fit needs --flame_model"):
        pipeline.demo_main("vocaset", base + ["--audio_path", str(tmp_path / "bad"), "--flame_fit"])


def test_c_client_fits_a_head_without_python(tmp_path):
    """tests/abi_c/flame_fit_client.cpp: fdm_flame_fit_create / _set / _forward with no Python in the process, under its own time limit;
    the Python call on the inputs it dumped returns the same bits in expr and pose."""
    import os
    import shutil
    import subprocess
    from fdm_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe, dump = str(tmp_path / "flame_fit_client"), str(tmp_path / "dump.bin")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", os.path.join(root, "tests", "abi_c", "flame_fit_client.cpp"),
           "-I", os.path.join(root, "include"), "-L", libdir, "-lfdm_hip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, dump], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "flame_fit_client ok" in r.stdout
    print(r.stdout.strip())
    raw = open(dump, "rb").read()
    V, J, NB, expr_at, NE, n_free, transl, B, L, iters = np.frombuffer(raw, np.int32, 10)
    at = 40

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(raw, dt, int(n), at).copy()
        at += 4 * int(n)
        return a
    free, frames, parents = take(np.int32, n_free), take(np.int32, B), take(np.int32, J)
    vt, sd, pd = take(np.float32, 3 * V), take(np.float32, 3 * V * NB), take(np.float32, 9 * (J - 1) * 3 * V)
    jr, w, y = take(np.float32, J * V), take(np.float32, V * J), take(np.float32, B * L * 3 * V)
    ex, ps, rms, st = take(np.float32, B * L * NE), take(np.float32, B * L * 3 * J), take(np.float32, B * L), take(np.int32, B * L)
    assert at == len(raw)
    m = flame.FlameModel(vt.reshape(V, 3), sd.reshape(V, 3, NB), pd.reshape(9 * (J - 1), 3 * V), jr.reshape(J, V), parents, w.reshape(V, J), int(expr_at))
    fit = flame.FlamePlan(m, device=DEV).fit(torch.from_numpy(y.reshape(B, L, 3 * V)).to(DEV), n_expr=int(NE), joints=tuple(int(j) for j in free),
                                             transl=bool(transl), iters=int(iters), frames=[int(f) for f in frames])
    assert torch.equal(fit.expression.cpu(), torch.from_numpy(ex.reshape(B, L, NE)))
    assert torch.equal(fit.pose.cpu(), torch.from_numpy(ps.reshape(B, L, 3 * J)))
    assert torch.equal(fit.rms.cpu(), torch.from_numpy(rms.reshape(B, L))) and torch.equal(fit.status.cpu(), torch.from_numpy(st.reshape(B, L)))
