"""GPU: the rig hand-off (include/fdm_hip.h, fdm_rig_*; kernels csrc/rig_out.hpp) -- the projection exactly on integers and within
the any-order bound on normal data, the solve bit for bit against the numpy restatement of tests/rig_cases.py fed the device's own
projections, exact recovery on a diagonal rig, independence of the batch and the padding, the frame rule on the projections, and
animate / animate_many / SlotServer with rig=.  Outputs are NaN-filled before every call; padded input rows are NaN."""
import functools

import numpy as np
import pytest
import torch

import rig_cases as RC
from fdm_amd import mesh, pipeline, rig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L_MAX, FRAMES = 3, RC.L_MAX, RC.FRAMES


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(d, frames, L_max=None):
    """[B, L_max, 3V] device tensor: clip b's rows, then NaN (input rows past frames[b] must never be read)"""
    x = d.copy() if L_max is None else np.concatenate([d, np.zeros((d.shape[0], L_max - d.shape[1], d.shape[2]), np.float32)], 1)
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return dev(x)


def run(plan, d, frames, fps=None, Lo_max=None, L_max=None):
    """forward() into NaN-filled outputs -> (coef, proj) on the host, [B, L_out_max, K]"""
    Lo = max([RC.frames_out(L, fps) for L in frames] + [1]) if Lo_max is None else Lo_max
    coef = torch.full((d.shape[0], Lo, plan.K), float("nan"), device=DEV)
    rf, proj = plan.forward(padded(d, frames, L_max), frames, fps, proj=True, out=coef)
    assert rf.frames == [RC.frames_out(L, fps) for L in frames] and rf.weights is coef
    return coef.cpu().numpy(), proj.cpu().numpy()


def live(x, frames_out):
    """the live rows of every clip, and a check that every other row is zero"""
    for b, n in enumerate(frames_out):
        assert np.all(x[b, n:] == 0)
    return np.concatenate([x[b, :n] for b, n in enumerate(frames_out)])


@pytest.mark.parametrize("V3", RC.V3S)
@pytest.mark.parametrize("K", RC.KS)
def test_projection_of_integers_is_exact(K, V3):
    P, d = RC.integer_case(K, V3, B, L_MAX, seed=K + V3)
    plan = rig.RigPlan(P, ridge=1.0, device=DEV)
    _, proj = run(plan, d, FRAMES)
    want = np.einsum("ki,bli->blk", P.astype(np.float64), d.astype(np.float64))
    assert float(np.abs(want).max()) < 2 ** 24
    for b, L in enumerate(FRAMES):
        assert torch.equal(torch.from_numpy(proj[b, :L]), torch.from_numpy(want[b, :L].astype(np.float32)))
        assert np.all(proj[b, L:] == 0)


@pytest.mark.parametrize("V3", RC.V3S)
@pytest.mark.parametrize("K", RC.KS)
def test_projection_within_the_any_order_bound(K, V3):
    """Random normal data against fp64 from the same fp32 P and d: per element |err| <= gamma_n sum_i |P_ki| |d_i| with
    n = 3V + chunks, the standard bound for a sum of n terms in any order.  Every element is checked."""
    E, w, ridge = RC.random_rig(K, V3, seed=K + V3)
    P = (E.astype(np.float64) * np.repeat(w.astype(np.float64), 3)).astype(np.float32)
    d = np.random.default_rng(K * V3).standard_normal((B, L_MAX, V3)).astype(np.float32)
    _, proj = run(rig.RigPlan(E, w, ridge, device=DEV), d, FRAMES)
    want = np.einsum("ki,bli->blk", P.astype(np.float64), d.astype(np.float64))
    mag = np.einsum("ki,bli->blk", np.abs(P).astype(np.float64), np.abs(d).astype(np.float64))
    n = V3 + RC.chunks(V3)
    gamma = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
    worst = 0.0
    for b, L in enumerate(FRAMES):
        err = np.abs(proj[b, :L].astype(np.float64) - want[b, :L])
        assert np.all(err <= gamma * mag[b, :L])
        worst = max(worst, float((err / (gamma * mag[b, :L])).max()) if L else 0.0)
    print(f"K = {K}, 3V = {V3}: worst err / bound = {worst:.3f}")


@pytest.mark.parametrize("K", RC.KS)
@pytest.mark.parametrize("sweeps", [0, 1, 16])
@pytest.mark.parametrize("bounded", [False, True])
def test_solve_equals_the_restatement_bit_for_bit(bounded, sweeps, K):
    V3 = 771                                                  # two chunks
    E, w, ridge = RC.random_rig(K, V3, seed=K)
    d = RC.targets_on_bounds(E, B * L_MAX, seed=K).reshape(B, L_MAX, V3)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    plan = rig.RigPlan(E, w, ridge, (lo, hi) if bounded else None, sweeps, device=DEV)
    coef, proj = run(plan, d, FRAMES)
    G, Lc = rig.gram(E, w, ridge)
    r = live(proj, FRAMES)
    want = RC.solve(r, G.astype(np.float32), Lc, lo if bounded else None, hi if bounded else None, sweeps)
    got = live(coef, FRAMES)
    assert not np.isnan(got).any() and torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    if bounded and sweeps == 16 and K >= 52:
        assert (got == 0).any() and (got == 1).any() and ((got > 0) & (got < 1)).any()


# every K at every 3V that can hold K rows of disjoint support (K <= 3V)
@pytest.mark.parametrize("K,V3", [(K, V3) for K in RC.KS for V3 in RC.V3S if RC.disjoint_rig(K, V3) is not None])
@pytest.mark.parametrize("bounded", [False, True])
def test_exact_recovery_on_a_diagonal_rig(bounded, K, V3):
    E = RC.disjoint_rig(K, V3)
    g = np.random.default_rng(K)
    c = (g.integers(1, 256, size=(B, L_MAX, K)) / 256.0).astype(np.float32)          # multiples of 2^-8 inside (0, 1)
    d = np.einsum("blk,ki->bli", c, E).astype(np.float32)
    plan = rig.RigPlan(E, ridge=0.0, bounds=(0, 1) if bounded else None, device=DEV)
    coef, _ = run(plan, d, FRAMES)
    for b, L in enumerate(FRAMES):
        assert torch.equal(torch.from_numpy(coef[b, :L]), torch.from_numpy(c[b, :L])) and np.all(coef[b, L:] == 0)


@pytest.mark.parametrize("V3", [15, 771, 1539])
@pytest.mark.parametrize("K", RC.KS)
def test_a_clip_does_not_depend_on_the_batch_or_the_padding(K, V3):
    E, w, ridge = RC.random_rig(K, V3, seed=7)
    d = RC.targets_on_bounds(E, B * L_MAX, seed=7).reshape(B, L_MAX, V3)
    plan = rig.RigPlan(E, w, ridge, (0, 1), device=DEV)
    coef, proj = run(plan, d, FRAMES)
    assert np.all(coef[0] == 0) and np.all(proj[0] == 0)                                # the 0-frame clip writes only zeros
    wide_c, wide_p = run(plan, d, FRAMES, L_max=2 * L_MAX, Lo_max=2 * L_MAX)
    for b, L in enumerate(FRAMES):
        one_c, one_p = run(plan, d[b:b + 1], [L])
        for got_c, got_p in ((one_c[0], one_p[0]), (wide_c[b], wide_p[b])):
            assert torch.equal(torch.from_numpy(got_c[:L]), torch.from_numpy(coef[b, :L]))
            assert torch.equal(torch.from_numpy(got_p[:L]), torch.from_numpy(proj[b, :L]))
            assert np.all(got_c[L:] == 0) and np.all(got_p[L:] == 0)
    clean = d.copy()
    for b, L in enumerate(FRAMES):
        clean[b, L:] = 0                                                                # zeros where run() puts NaN: nothing changes
    rf, pj = plan.forward(dev(clean), FRAMES, proj=True)
    assert torch.equal(rf.weights.cpu(), torch.from_numpy(coef)) and torch.equal(pj.cpu(), torch.from_numpy(proj))


@pytest.mark.parametrize("bounded", [False, True])
def test_a_non_finite_live_row_gives_nan_in_its_own_frame_only(bounded):
    """min / max keep a NaN operand (numpy's and the device's alike): the frame whose offsets hold a NaN gets NaN coefficients, never
    a bound, and every other frame keeps its bits."""
    K, V3 = 65, 771
    E, w, ridge = RC.random_rig(K, V3, seed=13)
    d = RC.targets_on_bounds(E, B * L_MAX, seed=13).reshape(B, L_MAX, V3)
    plan = rig.RigPlan(E, w, ridge, (0, 1) if bounded else None, device=DEV)
    coef0, _ = run(plan, d, FRAMES)
    bad = d.copy()
    bad[2, 3, 700] = np.nan
    coef, proj = run(plan, bad, FRAMES)
    assert np.isnan(coef[2, 3]).all() and np.isnan(proj[2, 3]).all()
    G, Lc = rig.gram(E, w, ridge)
    lo, hi = (np.zeros(K, np.float32), np.ones(K, np.float32)) if bounded else (None, None)
    with np.errstate(invalid="ignore"):
        assert np.isnan(RC.solve(proj[2, 3:4], G.astype(np.float32), Lc, lo, hi, 16)).all()
    keep = np.ones((B, L_MAX), bool)
    keep[2, 3] = False
    assert torch.equal(torch.from_numpy(coef[keep]), torch.from_numpy(coef0[keep]))


@pytest.mark.parametrize("fps", RC.RATES)
def test_frame_rate_is_the_lerp_of_the_native_projections(fps):
    K, V3 = 65, 1539
    E, w, ridge = RC.random_rig(K, V3, seed=9)
    d = RC.targets_on_bounds(E, B * L_MAX, seed=9).reshape(B, L_MAX, V3)
    lo, hi = np.zeros(K, np.float32), np.ones(K, np.float32)
    plan = rig.RigPlan(E, w, ridge, (lo, hi), device=DEV)
    coef0, proj0 = run(plan, d, FRAMES)
    coef, proj = run(plan, d, FRAMES, fps)
    G, Lc = rig.gram(E, w, ridge)
    for b, L in enumerate(FRAMES):
        Lo = RC.frames_out(L, fps)
        assert Lo == mesh.frames_out(L, *fps)
        want = RC.lerp(proj0[b], L, fps)
        assert torch.equal(torch.from_numpy(proj[b, :Lo]), torch.from_numpy(want)) and np.all(proj[b, Lo:] == 0)
        if Lo:
            assert torch.equal(torch.from_numpy(coef[b, :Lo]), torch.from_numpy(RC.solve(want, G.astype(np.float32), Lc, lo, hi, 16)))
    if fps[0] == fps[1]:                                                                # equal rates equal no rates
        assert torch.equal(torch.from_numpy(coef), torch.from_numpy(coef0)) and torch.equal(torch.from_numpy(proj), torch.from_numpy(proj0))


# ---- the pipeline
V_PIPE, K_PIPE = 5023, 8


@functools.lru_cache(maxsize=None)
def tiny_models():
    """The pipeline runs on the full VOCASET geometry only (tests/test_mesh_out_gpu.py, tiny_models()): half a second of audio and
    2-3 DDIM steps keep it short."""
    return pipeline.build_models("vocaset", None, DEV)


@functools.lru_cache(maxsize=None)
def pipe_rig():
    g = np.random.default_rng(11)
    E = (1e-2 * g.standard_normal((K_PIPE, 3 * V_PIPE))).astype(np.float32)
    return dict(basis=E, weights=None, ridge=1e-3, bounds=(-1.0, 1.0), sweeps=16, names=[f"shape{k}" for k in range(K_PIPE)])


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


def test_animate_with_rig_fits_the_offsets_it_decodes():
    diffusion, ae = tiny_models()
    kw, wav = pipe_rig(), tiny_audio(0.6, 1)
    tmpl = (1e-1 * np.random.default_rng(12).standard_normal((1, 3 * V_PIPE))).astype(np.float32)
    args = dict(ddim_steps=3, seed=2, device=DEV)
    offs, lat = pipeline.animate(diffusion, ae, wav, None, **args)                      # no template: the decoder's offsets
    want, _ = pipeline.animate(diffusion, ae, wav, tmpl, **args)
    same, _ = pipeline.animate(diffusion, ae, wav, tmpl, rig=None, **args)
    assert torch.equal(same, want)                                                     # rig=None: every path as before
    rf, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, rig=kw, **args)
    L = offs.shape[1]
    assert isinstance(rf, rig.RigFrames) and rf.frames == [L] and rf.weights.shape == (1, L, K_PIPE) and rf.names == kw["names"]
    assert torch.equal(lat, lat2)
    ref = pipeline.to_rig(offs, **kw)
    assert torch.equal(rf.weights, ref.weights) and float(ref.weights.abs().max()) > 0   # the offsets, not the templated vertices
    assert torch.equal(pipeline.to_rig(offs, rig.RigPlan(device=DEV, **kw)).weights, ref.weights)
    r2, _ = pipeline.animate(diffusion, ae, wav, tmpl, rig=kw, out_fps=60, **args)
    ref2 = pipeline.to_rig(offs, fps=(30, 60), **kw)
    assert r2.frames == [RC.frames_out(L, (30, 60))] and torch.equal(r2.weights, ref2.weights)
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)
    (mf, r3), _ = pipeline.animate(diffusion, ae, wav, tmpl, rig=kw, faces=faces, **args)
    assert torch.equal(r3.weights, ref.weights) and torch.equal(mf.positions.reshape(1, L, -1), want)
    long, _ = pipeline.animate_long(diffusion, ae, wav, tmpl, rig=kw, **args)
    assert torch.equal(long.weights, ref.weights)                                      # (fits one window: animate()'s bits)


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_rig_equal_the_per_clip_call(batch_stages):
    """batch_stages: the clips of a group / the clips that finish together go through ONE decode and ONE ragged rig call."""
    diffusion, ae = tiny_models()
    kw = pipe_rig()
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]                          # two clips of unequal length
    args = dict(ddim_steps=2, seed=1, device=DEV)
    offs, lats = pipeline.animate_many(diffusion, ae, wavs, None, **args)
    assert offs[0].shape[1] != offs[1].shape[1]
    got, lats2 = pipeline.animate_many(diffusion, ae, wavs, None, rig=kw, out_fps=25, batch_stages=batch_stages, **args)
    for b in range(2):
        ref = pipeline.to_rig(offs[b], fps=(30, 25), **kw)
        assert isinstance(got[b], rig.RigFrames) and got[b].frames == ref.frames and torch.equal(lats[b], lats2[b])
        assert torch.equal(got[b].weights, ref.weights)
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV)
    hs = srv.submit_many(wavs, None, seeds=1)
    plain = {h: v for h, v, _ in srv.drain(2)}
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, rig=kw, batch_stages=batch_stages)
    hs2 = srv.submit_many(wavs, None, seeds=1)
    fits = {h: v for h, v, _ in srv.drain(2)}
    assert isinstance(srv.rig, rig.RigPlan) and bool(srv.batched_decodes) == batch_stages      # the dict became a plan once
    for h, h2 in zip(hs, hs2):
        ref = pipeline.to_rig(plain[h], **kw)
        assert isinstance(fits[h2], rig.RigFrames) and fits[h2].frames == ref.frames and torch.equal(fits[h2].weights, ref.weights)
    faces = np.array([[0, 1, 2], [2, 1, 3]], dtype=np.int32)                              # with faces= too: the pair, from the same offsets
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, rig=kw, faces=faces, batch_stages=batch_stages)
    hs3 = srv.submit_many(wavs, None, seeds=1)
    both = {h: v for h, v, _ in srv.drain(2)}
    for h, h3 in zip(hs, hs3):
        mf, rf = both[h3]
        assert torch.equal(rf.weights, pipeline.to_rig(plain[h], **kw).weights) and torch.equal(mf.positions.reshape(plain[h].shape), plain[h])


def test_demo_command_line_with_rig_file(tmp_path):
    """demo --rig_file --out_fps 60 without --faces_file: <stem>_rig.npy holds to_rig of the decoded offsets at 60 fps, and <stem>.npy
    is what the command line writes without the flag (the template added, the model's frame rate)."""
    from scipy.io import wavfile
    diffusion, ae = tiny_models()
    kw = pipe_rig()
    wp, rp, tp = str(tmp_path / "hello.wav"), str(tmp_path / "rig.npz"), str(tmp_path / "template.npy")
    wavfile.write(wp, 16000, (tiny_audio(0.5, 3) * 20000).astype(np.int16))
    np.savez(rp, basis=kw["basis"], names=np.array(kw["names"]), lo=np.full(K_PIPE, -1, np.float32), hi=np.ones(K_PIPE, np.float32))
    np.save(tp, (1e-1 * np.random.default_rng(14).standard_normal((1, 3 * V_PIPE))).astype(np.float32))
    dst = pipeline.demo_main("vocaset", ["--audio_file", wp, "--ddim_steps", "2", "--device", DEV, "--template_file", tp, "--audio_path",
                                         str(tmp_path / "out"), "--rig_file", rp, "--rig_ridge", "1e-3", "--out_fps", "60"])
    wav = pipeline.processor_normalize(pipeline.load_wav(wp))
    base, _ = pipeline.animate(diffusion, ae, wav, np.load(tp), ddim_steps=2, device=DEV)
    offs, _ = pipeline.animate(diffusion, ae, wav, None, ddim_steps=2, device=DEV)
    ref = pipeline.to_rig(offs, fps=(30, 60), **kw)
    got, fit = np.load(dst), np.load(dst[:-4] + "_rig.npy")
    assert np.array_equal(got, base.cpu().numpy())
    assert fit.shape == (1, RC.frames_out(offs.shape[1], (30, 60)), K_PIPE) and np.array_equal(fit, ref.weights.cpu().numpy())
