"""GPU: the recurrences of the time filter hand-off (include/fdm_hip.h, fdm_tfilter_create_recur / _forward_state; csrc/trecur.hpp)
against their numpy restatement (tests/time_recur_cases.py), bit for bit everywhere: frame and column edges at the kernel's own
constants, rows off a 16-byte boundary, both kinds and directions, the strength rule, ragged batches with NaN padding, the carried
state, every prefetch depth, and the keyword through animate, animate_many, animate_long and SlotServer."""
import functools

import numpy as np
import pytest
import torch

import time_filter_cases as TC
import time_recur_cases as RC
from fdm_amd import pipeline, tfilter
from fdm_amd._lib import FdmError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
VERTS, DEPTH = tfilter.RECUR_VERTS, tfilter.PREFETCH_DEFAULT
FPS = 30.0
KINDS = {"ema": dict(cutoff=1.5), "one_euro": dict(min_cutoff=1.5, beta=0.5, d_cutoff=1.0)}
FRAMES = [1, 2, 3, 17, 130]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def plan_for(V, kind, direction, strength=None):
    return tfilter.TimeFilterPlan(V, kind=kind, fps=FPS, direction=direction, strength=strength, device=DEV, **KINDS[kind])


def check(x, lens, kind, direction, strength=None, depth=None):
    """The device result of the batch x [B, L_max, 3 V] equals the restatement in every bit, padding rows (zeros) included"""
    V = x.shape[-1] // 3
    plan = plan_for(V, kind, direction, strength)
    if depth is not None:
        plan.set_prefetch(depth)
    got = plan.forward(dev(x), lens).cpu().numpy()
    want = RC.filter_batch(x, lens, kind, RC.coeffs(kind, FPS, **KINDS[kind]), direction, strength)
    assert np.array_equal(bits(got), bits(want)), (x.shape, lens, kind, direction, depth, np.abs(got - want).max())
    return got


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_frame_count_edges(kind, direction):
    """L in {1, 2, 3, 17, 130} and at the prefetch ring's own edges (depth - 1 .. 2 depth + 1) as ONE ragged batch at V = 5"""
    Ls = sorted(set(FRAMES) | {DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH - 1, 2 * DEPTH, 2 * DEPTH + 1})
    x = np.stack([RC.clip(max(Ls), 15, 10 + L) for L in Ls])
    check(x, Ls, kind, direction)
    for L in FRAMES:      # and each as a fixed batch of its own
        check(x[:2, :L], None, kind, direction)


@pytest.mark.parametrize("V", [1, 2, 5, 86, 257, VERTS - 1, VERTS, VERTS + 1])
def test_column_count_edges(V):
    """N = 3 V not a multiple of 4, and at the workgroup's vertex count - 1, exactly, + 1; both kinds and directions, with a strength"""
    x = np.stack([RC.clip(19, 3 * V, V), RC.clip(19, 3 * V, V + 1)])
    s = np.random.default_rng(V).uniform(0, 1, V).astype(F32)
    for kind in KINDS:
        check(x, [19, 5], kind, "causal")
        check(x, [4, 19], kind, "zero_phase")
        check(x, [19, 17], kind, "zero_phase", s)
        check(x, [3, 19], kind, "causal", s)


@pytest.mark.parametrize("V", [5, 86])
def test_rows_off_a_16_byte_boundary(V):
    """Input and output viewed one float into larger buffers"""
    B, L, N = 2, 21, 3 * V
    x = np.stack([RC.clip(L, N, 7), RC.clip(L, N, 8)])
    big = torch.zeros(B * L * N + 5, device=DEV)
    xin = big[1:1 + B * L * N].view(B, L, N)
    xin.copy_(dev(x))
    for kind in KINDS:
        for direction in ("causal", "zero_phase"):
            obuf = torch.full((B * L * N + 5,), 7.0, device=DEV)
            out = obuf[1:1 + B * L * N].view(B, L, N)
            assert xin.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
            plan_for(V, kind, direction).forward(xin, [L, 9], out=out)
            want = RC.filter_batch(x, [L, 9], kind, RC.coeffs(kind, FPS, **KINDS[kind]), direction)
            assert np.array_equal(bits(out.cpu().numpy()), bits(want))
            assert float(obuf[0]) == 7.0 and bool((obuf[1 + B * L * N:] == 7.0).all())      # nothing written outside the view


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_strength(kind, direction):
    """Entries of exactly 0 and 1 among others: s = 0 returns the input bits (-0.0 included), the rest goes through the three-operation rule"""
    V, L = 86, 40
    x = RC.clip(L, 3 * V, 11)[None]
    x[0, ::3, ::5] = -0.0
    s = np.random.default_rng(5).uniform(0, 1, V).astype(F32)
    s[::4], s[1::4] = 0.0, 1.0
    got = check(x, [L], kind, direction, s)
    keep = np.repeat(s == 0, 3)
    assert np.array_equal(bits(got[0][:, keep]), bits(x[0][:, keep])) and not np.array_equal(bits(got[0][:, ~keep]), bits(x[0][:, ~keep]))
    check(x, [L - 3], kind, direction, np.zeros(V, F32))
    check(x, [L], kind, direction, np.ones(V, F32))


@pytest.mark.parametrize("direction", ["causal", "zero_phase"])
@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_ragged_batch_with_nan_padding(kind, direction):
    """B = 3 with lengths (130, 1, 17): NaN in the input's padding rows changes nothing, the output's padding rows are zeros, and every
    clip equals its own B = 1 call at another L_max"""
    V, L_max, lens = 86, 130, [130, 1, 17]
    x = np.stack([RC.clip(L_max, 3 * V, s) for s in (1, 2, 3)])
    clean = check(x, lens, kind, direction)
    xn = x.copy()
    for b, L in enumerate(lens):
        xn[b, L:] = np.nan
    plan = plan_for(V, kind, direction)
    got = plan.forward(dev(xn), lens).cpu().numpy()
    assert np.array_equal(bits(got), bits(clean))
    for b, L in enumerate(lens):
        assert not got[b, L:].any() and np.isfinite(got[b, :L]).all()
        solo = np.full((1, L + 3, 3 * V), np.nan, F32)
        solo[0, :L] = x[b, :L]
        assert np.array_equal(bits(plan.forward(dev(solo), [L]).cpu().numpy()[0, :L]), bits(got[b, :L]))


@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_prefetch_depths_give_the_same_bits(kind):
    """Every depth of fdm_tfilter_set_prefetch against the restatement, at lengths around each ring's edges"""
    Ls = [1, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 130]
    x = np.stack([RC.clip(max(Ls), 15, 40 + L) for L in Ls])
    s = np.array([0, 0.3, 1, 0.5, 0.9], F32)
    for depth in tfilter.PREFETCH_DEPTHS:
        check(x, Ls, kind, "zero_phase", s, depth)
        check(x, Ls, kind, "causal", None, depth)
    with pytest.raises(FdmError):
        plan_for(5, kind, "causal").set_prefetch(3)


@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_state(kind):
    """A 130-frame clip fed as chunks of 1, as chunks of 7, and as (0, 130, 0) inside a batch whose other clip advances: each
    concatenation equals the one-shot causal call; the L = 0 clip's state is unchanged; reset() starts afresh"""
    V, L = 86, 130
    N = 3 * V
    x = np.stack([RC.clip(L, N, 21), RC.clip(L, N, 22)])
    s = np.random.default_rng(9).uniform(0, 1, V).astype(F32)
    s[::5] = 0.0
    for strength in (None, s):
        plan = plan_for(V, kind, "causal", strength)
        xd = dev(x)
        whole = plan.forward(xd)
        assert np.array_equal(bits(whole.cpu().numpy()), bits(RC.filter_batch(x, None, kind, RC.coeffs(kind, FPS, **KINDS[kind]), "causal", strength)))
        for step in (1, 7):
            st = plan.new_state(2)
            parts = [plan.forward(xd[:, a:a + step].contiguous(), state=st) for a in range(0, L, step)]
            assert torch.equal(torch.cat(parts, dim=1), whole) and st.seen.tolist() == [L, L]
        # clip 0 is fed as (0, 130, 0) frames while clip 1 advances by (50, 30, 50)
        st = plan.new_state(2)
        out0, out1, at = [], [], 0
        for l0, l1 in ((0, 50), (130, 30), (0, 50)):
            L_max = max(l0, l1)
            xin = torch.full((2, L_max, N), float("nan"), device=DEV)
            xin[0, :l0], xin[1, :l1] = xd[0, :l0], xd[1, at:at + l1]
            before = (st.st[0].clone(), int(st.seen[0]))
            y = plan.forward(xin, [l0, l1], state=st)
            if l0 == 0:
                assert torch.equal(st.st[0], before[0]) and int(st.seen[0]) == before[1] and not bool(y[0].any())
            assert not bool(y[1, l1:].any()) and not bool(y[0, l0:].any())
            out0.append(y[0, :l0])
            out1.append(y[1, :l1])
            at += l1
        assert torch.equal(torch.cat(out0), whole[0]) and torch.equal(torch.cat(out1), whole[1]) and st.seen.tolist() == [L, L]
        # reset: one clip, then all
        st.reset([1])
        assert st.seen.tolist() == [L, 0] and not bool(st.st[1].any()) and bool(st.st[0].any())
        y = plan.forward(xd[:, :9].contiguous(), [0, 9], state=st)
        assert torch.equal(y[1], whole[1, :9])
        st.reset()
        assert torch.equal(plan.forward(xd, state=st), whole)


def test_state_is_refused_where_there_is_none():
    V = 5
    x = dev(RC.clip(9, 15, 1)[None])
    causal = plan_for(V, "one_euro", "causal")
    st = causal.new_state(1)
    zero = plan_for(V, "one_euro", "zero_phase")
    fir = tfilter.TimeFilterPlan(V, kind="gaussian", sigma=1.5, device=DEV)
    for plan in (zero, fir):
        with pytest.raises(FdmError):
            plan.new_state(1)
        with pytest.raises(FdmError):
            plan.forward(x, state=st)
    with pytest.raises(FdmError):
        causal.forward(x, state=causal.new_state(2))
    with pytest.raises(FdmError):
        causal.forward(x, [0])            # L = 0 needs a state
    assert int(st.seen[0]) == 0


@pytest.mark.parametrize("kind", ["ema", "one_euro"])
def test_zero_phase_is_two_causal_calls(kind):
    """zero_phase == flip . causal . flip . causal through the device's own causal calls, each clip at its own length"""
    V, lens = 86, [130, 17]
    x = np.stack([RC.clip(130, 3 * V, 31), RC.clip(130, 3 * V, 32)])
    z = plan_for(V, kind, "zero_phase").forward(dev(x), lens)
    c = plan_for(V, kind, "causal")
    for b, L in enumerate(lens):
        f = c.forward(dev(x[b:b + 1, :L]))
        r = c.forward(torch.flip(f, dims=[1]).contiguous())
        assert torch.equal(torch.flip(r, dims=[1]), z[b:b + 1, :L])


def test_fir_plans_are_untouched():
    V, L, h = 86, 140, TC.gaussian_taps(1.5, 4).astype(F32)
    x = np.stack([TC.clip(L, 3 * V, 1), TC.clip(L, 3 * V, 2)])
    got = tfilter.TimeFilterPlan(V, kind="gaussian", sigma=1.5, radius=4, device=DEV).forward(dev(x), [L, 9]).cpu().numpy()
    assert np.array_equal(bits(got), bits(TC.filter_batch(x, [L, 9], h)))


# ---- the pipeline
@functools.lru_cache(maxsize=None)
def tiny_models():
    """As tests/test_time_filter_gpu.py: the pipeline decodes on the full VOCASET geometry only; short audio and 2-3 DDIM steps."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


FILTER = dict(kind="one_euro", min_cutoff=1.5, beta=0.5, d_cutoff=1.0)


def test_animate_with_one_euro():
    diffusion, ae = tiny_models()
    wav, kw = tiny_audio(0.6, 1), dict(ddim_steps=3, seed=2, device=DEV)
    offs, lat = pipeline.animate(diffusion, ae, wav, None, **kw)
    V = offs.shape[-1] // 3
    fps = pipeline.presets.get("vocaset").fps
    got, lat2 = pipeline.animate(diffusion, ae, wav, None, time_filter=FILTER, **kw)
    want = pipeline.to_filtered(offs, FILTER, fps=fps)
    assert torch.equal(lat, lat2) and torch.equal(got, want) and not torch.equal(got, offs)
    ref = RC.filter_batch(offs.cpu().numpy(), None, "one_euro", RC.coeffs("one_euro", fps, **KINDS["one_euro"]), "zero_phase")
    assert np.array_equal(bits(got.cpu().numpy()), bits(ref))
    # a plan, an explicit fps= and the default direction are the same filter; causal and ema are others
    plan = tfilter.TimeFilterPlan(V, fps=fps, direction="zero_phase", device=DEV, **FILTER)
    for tf in (plan, dict(FILTER, fps=fps), dict(FILTER, direction="zero_phase")):
        assert torch.equal(pipeline.animate(diffusion, ae, wav, None, time_filter=tf, **kw)[0], want)
    for tf in (dict(FILTER, direction="causal"), dict(kind="ema", cutoff=1.5)):
        other, _ = pipeline.animate(diffusion, ae, wav, None, time_filter=tf, **kw)
        assert torch.equal(other, pipeline.to_filtered(offs, tf, fps=fps)) and not torch.equal(other, want)
    s = tfilter.strength_from_region(V, np.arange(0, V, 2), 0.0)
    part, _ = pipeline.animate(diffusion, ae, wav, None, time_filter=dict(FILTER, strength=s), **kw)
    assert torch.equal(part.reshape(1, -1, V, 3)[:, :, ::2], offs.reshape(1, -1, V, 3)[:, :, ::2])
    assert torch.equal(part, pipeline.to_filtered(offs, dict(FILTER, strength=s), fps=fps))
    # animate_long at 600 frames or fewer is animate()
    long, lat3 = pipeline.animate_long(diffusion, ae, wav, None, time_filter=FILTER, **kw)
    assert torch.equal(long, got) and torch.equal(lat3, lat)


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_one_euro(batch_stages):
    diffusion, ae = tiny_models()
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]
    kw = dict(ddim_steps=2, seed=1, device=DEV)
    fps = pipeline.presets.get("vocaset").fps
    got, lats = pipeline.animate_many(diffusion, ae, wavs, None, batch_stages=batch_stages, time_filter=FILTER, **kw)
    plain, lats0 = pipeline.animate_many(diffusion, ae, wavs, None, batch_stages=batch_stages, **kw)
    assert got[0].shape[1] != got[1].shape[1]
    for b in range(2):
        assert torch.equal(lats[b], lats0[b]) and got[b].shape == plain[b].shape
        assert torch.equal(got[b], pipeline.to_filtered(plain[b], FILTER, fps=fps)) and not torch.equal(got[b], plain[b])
    listed = pipeline.to_filtered(plain, FILTER, fps=fps)      # the ragged list: one padded call, each clip its own call's bits
    assert all(torch.equal(a, b) for a, b in zip(listed, got))
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages, time_filter=FILTER)
    hs = srv.submit_many(wavs, None, seeds=1)
    res = {h: v for h, v, _ in srv.drain(2)}
    for b, h in enumerate(hs):
        assert torch.equal(res[h], got[b])
