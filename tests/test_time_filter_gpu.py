"""GPU: the time filter hand-off (include/fdm_hip.h, fdm_tfilter_*; csrc/tfilter.hpp) against its numpy restatement
(tests/time_filter_cases.py), bit for bit unless a test says otherwise: size edges at the kernel's own tile constants, ragged batches
with NaN padding, rows off a 16-byte boundary, the strength rule, exact properties that need no restatement, that it filters, and the
keyword through animate, animate_many, animate_long and SlotServer."""
import functools

import numpy as np
import pytest
import torch

import time_filter_cases as TC
from fdm_amd import pipeline, tfilter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TILE, CHUNK = tfilter.FRAME_TILE, tfilter.COLUMN_CHUNK


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def run(V, h, x, lens=None, edge="mirror", strength=None):
    plan = tfilter.TimeFilterPlan(V, taps=h, edge=edge, strength=strength, device=DEV)
    return plan.forward(dev(x), lens).cpu().numpy()


def check(x, lens, h, edge="mirror", strength=None):
    """The device result of the batch x [B, L_max, 3 V] equals the float32 restatement in every bit, padding rows (zeros) included"""
    V = x.shape[-1] // 3
    got = run(V, h, x, lens, edge, strength)
    want = TC.filter_batch(x, lens, h, edge, strength)
    assert np.array_equal(bits(got), bits(want)), (x.shape, lens, len(h) - 1, edge, np.abs(got - want).max())
    return got


@pytest.mark.parametrize("edge", ["mirror", "nearest"])
@pytest.mark.parametrize("R", [0, 1, 2, 8, 32])
def test_frame_count_edges(R, edge):
    """L in {1, 2, 3, R, R + 1, 2 R + 1, tile - 1, tile, tile + 1} as ONE ragged batch at V = 5 (N = 15, not a multiple of 4)"""
    Ls = sorted({1, 2, 3, max(R, 1), R + 1, 2 * R + 1, TILE - 1, TILE, TILE + 1})
    L_max, V = max(Ls), 5
    x = np.stack([TC.clip(L_max, 3 * V, 100 * R + L) for L in Ls])
    check(x, Ls, TC.taps_for(R), edge)


@pytest.mark.parametrize("V", [1, 2, 5, 86, 257, (CHUNK - 3) // 3, CHUNK // 3, (CHUNK + 3) // 3])
def test_column_count_edges(V):
    """N = 3 V not a multiple of 4, and at the column chunk - 3, exactly, + 3; two edge rules, a radius past the clip"""
    assert CHUNK % 3 == 0
    x = np.stack([TC.clip(19, 3 * V, V), TC.clip(19, 3 * V, V + 1)])
    check(x, [19, 5], TC.taps_for(8), "mirror")
    check(x, [4, 19], TC.taps_for(2), "nearest")


def test_ragged_batch_with_nan_padding():
    """B = 3 with lengths (L_max, 1, 7): NaN in the input's padding rows changes nothing, the output's padding rows are zeros, and every
    clip equals its own B = 1 call at another L_max"""
    V, L_max, lens, h = 86, TILE + 5, [TILE + 5, 1, 7], TC.taps_for(8)
    x = np.stack([TC.clip(L_max, 3 * V, s) for s in (1, 2, 3)])
    clean = check(x, lens, h)
    xn = x.copy()
    for b, L in enumerate(lens):
        xn[b, L:] = np.nan
    got = run(V, h, xn, lens)
    assert np.array_equal(bits(got), bits(clean))
    for b, L in enumerate(lens):
        assert not got[b, L:].any() and np.isfinite(got[b, :L]).all()
        solo = np.full((1, L + 3, 3 * V), np.nan, F32)
        solo[0, :L] = x[b, :L]
        assert np.array_equal(bits(run(V, h, solo, [L])[0, :L]), bits(got[b, :L]))


@pytest.mark.parametrize("V", [5, 86])
def test_rows_off_a_16_byte_boundary(V):
    """Input and output viewed one float into larger buffers"""
    B, L, N, h = 2, 21, 3 * V, TC.taps_for(8)
    x = np.stack([TC.clip(L, N, 7), TC.clip(L, N, 8)])
    big = torch.zeros(B * L * N + 5, device=DEV)
    xin = big[1:1 + B * L * N].view(B, L, N)
    xin.copy_(dev(x))
    obuf = torch.full((B * L * N + 5,), 7.0, device=DEV)
    out = obuf[1:1 + B * L * N].view(B, L, N)
    assert xin.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    plan = tfilter.TimeFilterPlan(V, taps=h, device=DEV)
    plan.forward(xin, [L, 9], out=out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(TC.filter_batch(x, [L, 9], h)))
    assert float(obuf[0]) == 7.0 and bool((obuf[1 + B * L * N:] == 7.0).all())      # nothing written outside the view


def test_strength():
    """s = 0 returns the input bits (-0.0 included); s = 1 goes through the three-operation rule: compared to the restatement"""
    V, L, h = 86, 40, TC.taps_for(8)
    x = TC.clip(L, 3 * V, 11)[None]
    x[0, ::3, ::5] = -0.0
    s = np.random.default_rng(5).uniform(0, 1, V).astype(F32)
    s[::4], s[1::4] = 0.0, 1.0
    got = check(x, [L], h, "mirror", s)
    keep = np.repeat(s == 0, 3)
    assert np.array_equal(bits(got[0][:, keep]), bits(x[0][:, keep]))
    check(x, [L], h, "nearest", np.ones(V, F32))
    check(x, [L - 3], h, "mirror", np.zeros(V, F32))


def test_dyadic_taps_are_exact():
    """Taps [1/2, 1/4] on small integers: the exact rational result, no rounding anywhere"""
    V, L = 5, 33
    x = np.random.default_rng(3).integers(-64, 65, (1, L, 3 * V)).astype(F32)
    got = run(V, np.array([0.5, 0.25], F32), x)
    e = TC.edge_index
    t = np.arange(L)
    want = 0.5 * x[0].astype(np.float64) + 0.25 * (x[0][e(t - 1, L)].astype(np.float64) + x[0][e(t + 1, L)])
    assert np.array_equal(got[0].astype(np.float64), want)


@pytest.mark.parametrize("edge", ["mirror", "nearest"])
def test_time_reversal(edge):
    """Reversing a clip in time reverses its result bit for bit (the pair is summed first); Gaussian taps, R = 8"""
    V, L, h = 86, TILE + 9, TC.gaussian_taps(2.5, 8).astype(F32)
    x = TC.clip(L, 3 * V, 4)[None]
    a = run(V, h, x, None, edge)
    b = run(V, h, x[:, ::-1].copy(), None, edge)
    assert np.array_equal(bits(a[0]), bits(b[0, ::-1]))


def test_radius_zero_is_a_copy():
    V, L_max = 86, 12
    x = np.stack([TC.clip(L_max, 3 * V, 1), TC.clip(L_max, 3 * V, 2)])
    got = run(V, np.array([1.0], F32), x, [L_max, 5])
    assert np.array_equal(bits(got[0]), bits(x[0])) and np.array_equal(bits(got[1, :5]), bits(x[1, :5])) and not got[1, 5:].any()


def test_it_filters():
    """A 64-frame clip of a slow sinusoid plus alternating-sign noise: in the interior the sinusoid is scaled by the gain
    h0 + 2 sum h_k cos(k w) (fp64) and the alternating component by the gain at w = pi, each to the derived bound"""
    V, L, R = 5, 64, 4
    h = TC.gaussian_taps(1.5, R).astype(F32)
    h64 = h.astype(np.float64)
    gain = lambda w: h64[0] + 2.0 * sum(h64[k] * np.cos(k * w) for k in range(1, R + 1))  # noqa: E731
    t = np.arange(L, dtype=np.float64)[:, None]
    w = 2.0 * np.pi / 32.0
    amp = np.linspace(0.5, 2.0, 3 * V)[None, :]
    phase = np.linspace(0.0, 1.0, 3 * V)[None, :]
    slow, alt = amp * np.sin(w * t + phase), 0.25 * amp * np.cos(np.pi * t)
    inner = slice(R, L - R)
    for part, g in ((slow, gain(w)), (alt, gain(np.pi)), (slow + alt, None)):
        x = part.astype(F32)
        got = run(V, h, x[None])[0].astype(np.float64)
        # the float32 input is what is filtered: it differs from the signal by at most u max|signal| per sample, which passes through
        # the full kernel's absolute sum |h0| + 2 sum |h_k| <= 2 sum_k |h_k|; 1e-15 covers the float64 sin / cos of the signal itself
        want = TC.filter_f64(x, h) if g is None else g * part
        tol = TC.bound(x, h) + (0 if g is None else TC.U32 * np.abs(h64).sum() * 2 * np.abs(part).max() + 1e-15)
        err = np.abs(got - want)[inner]
        print(f"gain {g}: max err {err.max():.3e}, bound min {tol[inner].min():.3e}")
        assert (err <= tol[inner]).all()
    assert abs(gain(np.pi)) < 0.02 < 0.9 < gain(w)      # the jitter goes, the motion stays


# ---- the pipeline
@functools.lru_cache(maxsize=None)
def tiny_models():
    """As tests/test_wrap_gpu.py: the pipeline decodes on the full VOCASET geometry only; short audio and 2-3 DDIM steps."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


FILTER = dict(kind="gaussian", sigma=1.5, radius=4)


def test_animate_with_time_filter():
    diffusion, ae = tiny_models()
    wav, kw = tiny_audio(0.6, 1), dict(ddim_steps=3, seed=2, device=DEV)
    offs, lat = pipeline.animate(diffusion, ae, wav, None, **kw)
    V = offs.shape[-1] // 3
    tmpl = np.random.default_rng(0).standard_normal((1, 3 * V)).astype(F32)
    got, lat2 = pipeline.animate(diffusion, ae, wav, None, time_filter=FILTER, **kw)
    want = pipeline.to_filtered(offs, FILTER)
    assert torch.equal(lat, lat2) and torch.equal(got, want) and not torch.equal(got, offs)
    assert np.array_equal(bits(got.cpu().numpy()), bits(TC.filter_batch(offs.cpu().numpy(), [offs.shape[1]], TC.gaussian_taps(1.5, 4).astype(F32))))
    # a plan, and seconds= by the preset's frame rate, are the same filter; a strength changes it
    plan = tfilter.TimeFilterPlan(V, device=DEV, **FILTER)
    fps = pipeline.presets.get("vocaset").fps
    for tf in (plan, dict(kind="gaussian", seconds=1.5 / fps, radius=4)):
        assert torch.equal(pipeline.animate(diffusion, ae, wav, None, time_filter=tf, **kw)[0], want)
    s = tfilter.strength_from_region(V, np.arange(0, V, 2), 0.0)
    part, _ = pipeline.animate(diffusion, ae, wav, None, time_filter=dict(FILTER, strength=s), **kw)
    p3 = part.reshape(1, -1, V, 3)
    assert torch.equal(p3[:, :, ::2], offs.reshape(1, -1, V, 3)[:, :, ::2]) and torch.equal(part, pipeline.to_filtered(offs, dict(FILTER, strength=s)))
    # the template is added after the filter; with faces= the mesh hand-off reads the filtered offsets
    with_t, _ = pipeline.animate(diffusion, ae, wav, tmpl, time_filter=FILTER, **kw)
    assert torch.equal(with_t, want + dev(tmpl).unsqueeze(1))
    faces = np.array([(k, k + 1, k + 2) for k in range(V - 2)], dtype=np.int32)
    mf, _ = pipeline.animate(diffusion, ae, wav, tmpl, faces=faces, out_fps=60, time_filter=FILTER, **kw)
    r = pipeline.to_mesh(want, faces, tmpl, fps=(fps, 60))
    assert mf.frames == r.frames and torch.equal(mf.positions, r.positions) and torch.equal(mf.normals, r.normals)
    # animate_long at 600 frames or fewer is animate()
    long, _ = pipeline.animate_long(diffusion, ae, wav, None, time_filter=FILTER, **kw)
    assert torch.equal(long, got)
    # time_filter=None: the call without the keyword
    none, _ = pipeline.animate(diffusion, ae, wav, None, time_filter=None, **kw)
    assert torch.equal(none, offs)


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_time_filter(batch_stages):
    diffusion, ae = tiny_models()
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]
    kw = dict(ddim_steps=2, seed=1, device=DEV)
    got, lats = pipeline.animate_many(diffusion, ae, wavs, None, batch_stages=batch_stages, time_filter=FILTER, **kw)
    plain, lats0 = pipeline.animate_many(diffusion, ae, wavs, None, batch_stages=batch_stages, **kw)
    solo = [pipeline.animate(diffusion, ae, wavs[b], None, time_filter=FILTER, **kw)[0] for b in range(2)]
    assert got[0].shape[1] != got[1].shape[1]
    for b in range(2):
        assert torch.equal(lats[b], lats0[b]) and got[b].shape == plain[b].shape
        assert torch.equal(got[b], solo[b]) and torch.equal(got[b], pipeline.to_filtered(plain[b], FILTER))
    listed = pipeline.to_filtered(plain, FILTER)      # the ragged list: one padded call, each clip its own call's bits
    assert all(torch.equal(a, b) for a, b in zip(listed, got))
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages, time_filter=FILTER)
    hs = srv.submit_many(wavs, None, seeds=1)
    res = {h: v for h, v, _ in srv.drain(2)}
    for b, h in enumerate(hs):
        assert torch.equal(res[h], solo[b])
