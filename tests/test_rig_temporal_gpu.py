"""GPU: the temporal rig fit (include/fdm_hip.h, fdm_rig_set_temporal; kernels csrc/rig_out.hpp) -- the
coupled solve bit for bit against the numpy restatement of tests/rig_temporal_cases.py fed the device's own projections, independence
of the batch and the padding, the way back to the per-frame fit, NaN handling, and animate / animate_many with rig=dict(smooth=).
Outputs are NaN-filled before every call; padded input rows are NaN."""
import functools

import numpy as np
import pytest
import torch

import rig_cases as RC
import rig_temporal_cases as TC
from fdm_amd import pipeline, rig

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, L_MAX, FRAMES = 4, 9, [0, 1, 2, 9]          # every n_f (0; 1 and 1; 1, 2.., 1) and both parities
KS = [1, 3, 64, 65, 128]
MODES = [None, 0, 1, 4]                         # no bounds, or bounds with S sweeps
# (3V, rates) per call of one test: one chunk and two chunks, doubling, a ratio that is no integer, equal rates, no rates
CALLS = [(288, (30, 60)), (771, (25, 30)), (771, (30, 30)), (288, None)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def padded(d, frames):
    x = d.copy()
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return dev(x)


def zeroed(d, frames):
    x = d.copy()
    for b, L in enumerate(frames):
        x[b, L:] = 0
    return dev(x)


def run(plan, d, frames, fps=None, Lo_max=None, pad=padded):
    """forward() into NaN-filled outputs -> (coef, proj, frames out) on the host; rows at and past L_out[b] are checked to be zero"""
    fo = [RC.frames_out(L, fps) for L in frames]
    Lo = max(fo + [1]) if Lo_max is None else Lo_max
    coef = torch.full((d.shape[0], Lo, plan.K), float("nan"), device=DEV)
    rf, proj = plan.forward(pad(d, frames), frames, fps, proj=True, out=coef)
    assert rf.frames == fo and rf.weights is coef
    c, p = coef.cpu().numpy(), proj.cpu().numpy()
    for b, n in enumerate(fo):
        assert np.all(c[b, n:] == 0) and np.all(p[b, n:] == 0)
    return c, p, fo


def same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@functools.lru_cache(maxsize=None)
def case(K, V3, n):
    E, w, ridge = RC.random_rig(K, V3, seed=K)
    return E, w, ridge, RC.targets_on_bounds(E, n, seed=K), rig.gram(E, w, ridge)[0]


def smoothing(K, G, weighted, x=1.0):
    m = (0.5 + np.random.default_rng(K).random(K)).astype(np.float32) if weighted else None
    return x * float(np.trace(G)) / K, m


def check_against_restatement(plan, G, d, frames, fps, mode):
    K = plan.K
    lo, hi = (None, None) if mode is None else (np.zeros(K, np.float32), np.ones(K, np.float32))
    tables = TC.tables32(G, plan.smooth, plan.smooth_weights)
    coef, proj, fo = run(plan, d, frames, fps)
    for b, n in enumerate(fo):
        want = TC.solve(proj[b, :n], G.astype(np.float32), tables, lo, hi, mode or 0)
        assert not np.isnan(coef[b, :n]).any() and same(coef[b, :n], want), (b, n, fps)
    return coef


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K", KS)
def test_the_coupled_solve_equals_the_restatement_bit_for_bit(K, mode, weighted):
    for V3, fps in CALLS:
        E, w, ridge, d, G = case(K, V3, B * L_MAX)
        mu, m = smoothing(K, G, weighted)
        plan = rig.RigPlan(E, w, ridge, None if mode is None else (0, 1), mode or 0, device=DEV, smooth=mu, smooth_weights=m)
        coef = check_against_restatement(plan, G, d.reshape(B, L_MAX, V3), FRAMES, fps, mode)
        if mode == 4 and K >= 64:
            assert (coef == 1).any() and ((coef > 0) & (coef < 1)).any()


@pytest.mark.parametrize("K,V3,mode,x", [(3, 288, None, 10.0), (65, 771, 4, 0.1), (128, 288, 1, 1.0)])
def test_a_forty_frame_clip(K, V3, mode, x):
    E, w, ridge, d, G = case(K, V3, 40)
    mu, m = smoothing(K, G, True, x)
    plan = rig.RigPlan(E, w, ridge, None if mode is None else (0, 1), mode or 0, device=DEV, smooth=mu, smooth_weights=m)
    for fps in (None, (30, 60), (25, 30)):
        check_against_restatement(plan, G, d.reshape(1, 40, V3), [40], fps, mode)


@pytest.mark.parametrize("K,V3", [(3, 288), (65, 771), (128, 771)])
def test_a_clip_does_not_depend_on_the_batch_or_the_padding(K, V3):
    E, w, ridge, d, G = case(K, V3, B * L_MAX)
    d = d.reshape(B, L_MAX, V3)
    mu, m = smoothing(K, G, False)
    plan = rig.RigPlan(E, w, ridge, (0, 1), 4, device=DEV, smooth=mu)
    for fps in (None, (30, 60)):
        coef, proj, fo = run(plan, d, FRAMES, fps)
        assert np.all(coef[0] == 0) and np.all(proj[0] == 0)                            # the 0-frame clip writes only zeros
        wide_c, wide_p, _ = run(plan, d, FRAMES, fps, Lo_max=2 * max(fo) + 1)           # another L_out_max: other colours per launch
        zero_c, zero_p, _ = run(plan, d, FRAMES, fps, pad=zeroed)
        assert same(zero_c, coef) and same(zero_p, proj)                                # zeros where run() puts NaN: nothing changes
        for b, L in enumerate(FRAMES):
            one_c, one_p, _ = run(plan, d[b:b + 1], [L], fps)
            n = fo[b]
            assert same(one_c[0, :n], coef[b, :n]) and same(one_p[0, :n], proj[b, :n])
            assert same(wide_c[b, :n], coef[b, :n]) and same(wide_p[b, :n], proj[b, :n])


def test_set_temporal_zero_returns_to_the_per_frame_fit():
    K, V3 = 65, 771
    E, w, ridge, d, G = case(K, V3, B * L_MAX)
    d = d.reshape(B, L_MAX, V3)
    fresh, _, _ = run(rig.RigPlan(E, w, ridge, (0, 1), device=DEV), d, FRAMES, (30, 60))
    mu, m = smoothing(K, G, True)
    plan = rig.RigPlan(E, w, ridge, (0, 1), device=DEV, smooth=mu, smooth_weights=m)
    smooth, _, _ = run(plan, d, FRAMES, (30, 60))
    assert not same(smooth, fresh)
    plan.set_temporal(0.0)
    back, _, _ = run(plan, d, FRAMES, (30, 60))
    assert same(back, fresh) and plan.key == rig.identity(E, w, ridge, (0, 1))
    plan.set_temporal(mu, m)                                                            # and on again: the same tables, the same bits
    again, _, _ = run(plan, d, FRAMES, (30, 60))
    assert same(again, smooth)
    # the fit does what it is for: smoother curves than the per-frame fit on the 9-frame clip (18 output frames)
    assert TC.bend(smooth[3]) < TC.bend(fresh[3])


@pytest.mark.parametrize("mode", [None, 4])
def test_a_non_finite_live_row_gives_nan_in_its_own_clip_only(mode):
    """The frames of a clip are coupled: a NaN offset makes every coefficient of its clip NaN -- never a bound -- and every other clip
    keeps its bits."""
    K, V3 = 65, 771
    E, w, ridge, d, G = case(K, V3, B * L_MAX)
    d = d.reshape(B, L_MAX, V3)
    mu, _ = smoothing(K, G, False)
    plan = rig.RigPlan(E, w, ridge, None if mode is None else (0, 1), mode or 0, device=DEV, smooth=mu)
    coef0, _, _ = run(plan, d, FRAMES)
    bad = d.copy()
    bad[3, 4, 700] = np.nan
    coef, proj, _ = run(plan, bad, FRAMES)
    assert np.isnan(coef[3]).all() and np.isnan(proj[3, 4]).all() and not np.isnan(proj[3, :4]).any()
    assert same(coef[:3], coef0[:3])
    with np.errstate(invalid="ignore"):
        lo, hi = (None, None) if mode is None else (np.zeros(K, np.float32), np.ones(K, np.float32))
        assert np.isnan(TC.solve(proj[3], G.astype(np.float32), TC.tables32(G, mu), lo, hi, mode or 0)).all()


# ---- the pipeline
V_PIPE, K_PIPE = 5023, 8


@functools.lru_cache(maxsize=None)
def tiny_models():
    """The pipeline runs on the full VOCASET geometry only: half a second of audio and 2 DDIM steps keep it short."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


def test_animate_and_animate_many_with_a_smooth_rig_equal_to_rig_on_the_same_offsets():
    diffusion, ae = tiny_models()
    g = np.random.default_rng(11)
    E = (1e-2 * g.standard_normal((K_PIPE, 3 * V_PIPE))).astype(np.float32)
    G, _ = rig.gram(E, None, 1e-3)
    kw = dict(basis=E, weights=None, ridge=1e-3, bounds=(-1.0, 1.0), sweeps=4, names=None, smooth=float(np.trace(G)) / K_PIPE,
              smooth_weights=np.linspace(0.5, 2.0, K_PIPE).astype(np.float32))
    frame_kw = dict(kw, smooth=0.0, smooth_weights=None)
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]
    args = dict(ddim_steps=2, seed=1, device=DEV)
    offs, _ = pipeline.animate(diffusion, ae, wavs[0], None, **args)
    rf, _ = pipeline.animate(diffusion, ae, wavs[0], None, rig=kw, out_fps=60, **args)
    ref = pipeline.to_rig(offs, fps=(30, 60), **kw)
    assert rf.frames == ref.frames == [RC.frames_out(offs.shape[1], (30, 60))] and torch.equal(rf.weights, ref.weights)
    assert not torch.equal(ref.weights, pipeline.to_rig(offs, fps=(30, 60), **frame_kw).weights)
    assert torch.equal(pipeline.to_rig(offs, rig.RigPlan(device=DEV, **kw), fps=(30, 60)).weights, ref.weights)
    many, _ = pipeline.animate_many(diffusion, ae, wavs, None, **args)
    assert many[0].shape[1] != many[1].shape[1]
    got, _ = pipeline.animate_many(diffusion, ae, wavs, None, rig=kw, out_fps=25, batch_stages=True, **args)   # ONE ragged rig call
    for b in range(2):
        one = pipeline.to_rig(many[b], fps=(30, 25), **kw)
        assert got[b].frames == one.frames and torch.equal(got[b].weights, one.weights)
