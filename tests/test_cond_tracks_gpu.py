"""GPU: condition tracks (include/fdm_hip.h, "Condition tracks") -- one style / emotion vector per latent frame.

The conditions enter the denoiser through the addend table E0 only, so the bars are exact wherever no second implementation is
involved (torch.equal): the operator against fdm_op_small_linear + fdm_op_add_rows on every row's vectors; a track whose rows are all
equal against the per-clip call; the frames before a change against the run without the change (self-attention is causal, everything
else is row-local); a slot or a group admitted with tracks against its solo call.  Against the CPU oracle, fed the same [L, n] tracks,
the bars are the project's: 1e-4 in the fp32 and split-fp16 modes, tests/test_denoiser_gpu.py's 8e-2 (bf16) and 6e-3 (fp16) per call.
Tiny presets but for the operator, which runs at the real widths."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd import ops, schedule, tracks  # noqa: E402
from fdm_amd._lib import ACT_MISH, ACT_NONE, BF16, F16, F16X3, F32, SLOT_FINISHED  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan, window_starts  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"
ALL_MODES = [F32, BF16, F16X3, F16]
TOL = {F32: 1e-4, F16X3: 1e-4, BF16: 8e-2, F16: 6e-3}      # per denoiser call (tests/test_denoiser_gpu.py: TOL32, TOLBF, TOLF16)
DDPM_TS = [999, 500, 0]
PRESETS = [("vocaset_tiny", False), ("mead_tiny", True)]    # (preset, cfg): the style switches on VOCASET, the emotion on MEAD
_PLANS, _W, _IN = {}, {}, {}


def dv(t):
    return t.to(DEV)


def weights(preset):
    if preset not in _W:
        _W[preset] = W.make_fdm_weights(preset)
    return _W[preset]


def plan_for(preset, dtype):
    if (preset, dtype) not in _PLANS:
        _PLANS[(preset, dtype)] = DenoiserPlan(preset, weights(preset), dtype, DEV)
    return _PLANS[(preset, dtype)]


def inputs(preset, L, seed=5):
    if (preset, L, seed) not in _IN:
        _IN[(preset, L, seed)] = W.synth_inputs(preset, 1, L, seed=seed)
    return _IN[(preset, L, seed)]


def one_hot(n, i):
    return torch.eye(n)[i % n]


def cond_tracks(preset, L, keys):
    """(kwargs of the run with the first condition throughout, kwargs of the run with the switches at `keys`): the style switches on a
    preset without emotions, the emotion otherwise."""
    p = plan_for(preset, F32).p
    if p.n_emo:
        first = dict(style=one_hot(p.n_style, 3), emo=None, emotion_track=tracks.keyframes(L, [(0, one_hot(p.n_emo, 4))]))
        sw = dict(first, emotion_track=tracks.keyframes(L, [(0, one_hot(p.n_emo, 4))] + [(f, one_hot(p.n_emo, 1 + i)) for i, f in enumerate(keys)]))
    else:
        first = dict(style=None, emo=None, style_track=tracks.keyframes(L, [(0, one_hot(p.n_style, 3))]))
        sw = dict(first, style_track=tracks.keyframes(L, [(0, one_hot(p.n_style, 3))] + [(f, one_hot(p.n_style, 5 + i)) for i, f in enumerate(keys)]))
    return first, sw


def run(plan, x, sampler, windows=False, **kw):
    """One chain on a prepared plan; Philox noise for the samplers that draw."""
    if windows:
        if sampler == "ddim":
            return plan.sample_windows(x, kind="ddim", steps=4, **kw)
        if sampler == "ddpm":
            return plan.sample_windows(x, kind="ddpm", t_list=DDPM_TS, seed=11, clip0=2, **kw)
        t, tab = schedule.sampler_tables("dpmpp2m", 4)
        return plan.sample_windows(x, kind="tables", t_list=t, tables=tab, seed=11, clip0=2, **kw)
    if sampler == "ddim":
        return plan.sample_ddim(x, 4, **kw)
    if sampler == "ddpm":
        return plan.sample_ddpm(x, DDPM_TS, seed=11, clip0=2, **kw)
    t, tab = schedule.sampler_tables("dpmpp2m", 4)
    return plan.sample_tables(x, t, tab, seed=11, clip0=2, **kw)


def frames(x, G):
    """[B, L*G, c] -> [B, L, G*c]"""
    return x.reshape(x.shape[0], -1, G * x.shape[-1])


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,d,n_style,n_emo,cfg,act", [("vocaset", 1024, 8, 0, False, ACT_NONE), ("mead", 512, 25, 7, True, ACT_NONE),
                                                          ("biwi", 1024, 6, 0, False, ACT_MISH)])
@pytest.mark.parametrize("L,L_clip", [(1, 1), (7, 5), (33, 20), (33, 33)])
def test_op_cond_rows_equals_small_linear_and_add_rows(name, d, n_style, n_emo, cfg, act, L, L_clip):
    """Two clips in one launch, general (not one-hot) vectors per row, NaN in the caller's track rows beyond L_clip: every row of both
    halves has the bits of small_linear + add_rows on its vectors, the rows L_clip .. L are exactly zero."""
    B = 2
    g = torch.Generator().manual_seed(L * 100 + d + n_emo)
    pe, sw, sb = dv(torch.randn(40, d, generator=g)), dv(torch.randn(d, n_style, generator=g) * 0.3), dv(torch.randn(d, generator=g))
    ew, eb = (dv(torch.randn(d, n_emo, generator=g) * 0.3), dv(torch.randn(d, generator=g))) if n_emo else (None, None)
    st = torch.randn(B, L, n_style, generator=g)
    em = torch.randn(B, L, n_emo, generator=g) if n_emo else None
    st[:, L_clip:] = float("nan")
    if em is not None:
        em[:, L_clip:] = float("nan")
    st, em = dv(st), (dv(em) if em is not None else None)
    rows, M = B * L_clip, B * L
    out = torch.full((2 if cfg else 1, M, d), 7.0, device=DEV)
    ops.cond_rows(pe, st, em, sw, sb, ew, eb, out, B, L, L_clip, d, uncond_off=M * d if cfg else 0, act=act)
    # the per-clip path, every row its own "clip"
    xs = st[:, :L_clip].reshape(rows, n_style).contiguous()
    sty = torch.empty(rows, d, device=DEV)
    ops.small_linear(xs, sw, sb, sty, rows, n_style, d, act)
    e = eu = None
    if n_emo:
        e, eu = torch.empty(rows, d, device=DEV), torch.empty(rows, d, device=DEV)
        ops.small_linear(em[:, :L_clip].reshape(rows, n_emo).contiguous(), ew, eb, e, rows, n_emo, d)
        ops.small_linear(torch.zeros(rows, n_emo, device=DEV), ew, eb, eu, rows, n_emo, d)
    for half in range(2 if cfg else 1):
        ref = torch.empty(rows, d, device=DEV)
        ops.add_rows(ref, rows, d, pe, 1, L_clip, sty, 1, rows, (eu if half else e), 1, rows)
        got = out[half].reshape(B, L, d)
        assert torch.equal(got[:, :L_clip].reshape(rows, d), ref), (name, half)
        assert not got[:, L_clip:].any(), (name, half)          # exactly zero (and no NaN)
    assert torch.isfinite(out).all()


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_constant_track_is_the_per_clip_call(preset, cfg, dtype):
    """prepare(tracks with every row equal) + DDIM 4 / DDPM over 3 timesteps / DPM-Solver++ 2M 4 == prepare + the same sampler, two clips."""
    plan, L, B = plan_for(preset, dtype), 13, 2
    inp = W.synth_inputs(preset, B, L, seed=21)
    x, p = dv(inp["x"]), plan.p
    kw = dict(style_track=inp["style"].unsqueeze(1).expand(B, L, -1))
    if p.n_emo:
        kw["emotion_track"] = inp["emo"].unsqueeze(1).expand(B, L, -1)
    for sampler in ("ddim", "ddpm", "2m"):
        plan.prepare(inp["hub"], inp["style"], inp.get("emo"), L=L, cfg=cfg)
        ref = run(plan, x, sampler).clone()
        n0 = plan.get("launches_per_step")
        plan.prepare(inp["hub"], L=L, cfg=cfg, **kw)
        assert torch.equal(run(plan, x, sampler), ref), sampler
        assert plan.get("launches_per_step") == n0          # the same step program
    # one track alone: the other condition's per-clip vector is broadcast to frames
    if p.n_emo:
        plan.prepare(inp["hub"], inp["style"], L=L, cfg=cfg, emotion_track=kw["emotion_track"])
        assert torch.equal(run(plan, x, "2m"), ref)


@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_constant_track_is_the_per_clip_call_on_windows(preset, cfg, dtype):
    """The same on a windowed plan: window 24, overlap 8, 56 frames."""
    plan, LT = plan_for(preset, dtype), 56
    inp = inputs(preset, LT)
    x, p = dv(inp["x"]), plan.p
    kw = dict(style_track=inp["style"].expand(LT, -1))
    if p.n_emo:
        kw["emotion_track"] = inp["emo"].expand(LT, -1)
    for sampler in ("ddim", "ddpm", "2m"):
        plan.prepare_windows(inp["hub"], inp["style"], inp.get("emo"), L_total=LT, window=24, overlap=8, cfg=cfg)
        ref = run(plan, x, sampler, windows=True).clone()
        n0 = plan.get("launches_per_step")
        plan.prepare_windows(inp["hub"], L_total=LT, window=24, overlap=8, cfg=cfg, **kw)
        assert torch.equal(run(plan, x, sampler, windows=True), ref), sampler
        assert plan.get("launches_per_step") == n0


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_frames_before_a_switch_keep_their_bits(preset, cfg, dtype):
    """The acceptance test: 40 frames, the condition switches at frame 17 and again at 33 (neither a tile multiple).  After a DDIM 4
    chain and after a DDPM chain with Philox noise, the frames < 17 are torch.equal to the run with the first condition throughout,
    and the frames >= 17 differ from it."""
    plan, L, f0 = plan_for(preset, dtype), 40, 17
    inp = inputs(preset, L)
    x, G = dv(inp["x"]), plan.p.G
    first, sw = cond_tracks(preset, L, [f0, 33])
    for sampler in ("ddim", "ddpm"):
        plan.prepare(inp["hub"], L=L, cfg=cfg, **first)
        a = frames(run(plan, x, sampler), G).clone()
        plan.prepare(inp["hub"], L=L, cfg=cfg, **sw)
        b = frames(run(plan, x, sampler), G)
        assert torch.equal(a[:, :f0], b[:, :f0]), sampler
        assert (a[:, f0:] != b[:, f0:]).any(dim=-1).all(), sampler          # every later frame moved


@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_frames_before_a_switch_keep_their_bits_on_windows(preset, cfg, dtype):
    """The same on a windowed plan (window 24, overlap 8, 56 frames: windows at 0, 16, 32) with the switch at frame 29, and at frame
    34, which two windows cover: the frames before the switch keep their bits in the long buffer, the later ones move."""
    plan, LT = plan_for(preset, dtype), 56
    assert window_starts(LT, 24, 8) == [0, 16, 32]
    inp = inputs(preset, LT)
    x, G = dv(inp["x"]), plan.p.G
    for sampler in ("ddim", "ddpm"):
        first, _ = cond_tracks(preset, LT, [29])
        plan.prepare_windows(inp["hub"], L_total=LT, window=24, overlap=8, cfg=cfg, **first)
        a = frames(run(plan, x, sampler, windows=True), G).clone()
        for f0 in (29, 34):
            _, sw = cond_tracks(preset, LT, [f0])
            plan.prepare_windows(inp["hub"], L_total=LT, window=24, overlap=8, cfg=cfg, **sw)
            b = frames(run(plan, x, sampler, windows=True), G)
            assert torch.equal(a[:, :f0], b[:, :f0]), (sampler, f0)
            assert (a[:, f0:] != b[:, f0:]).any(dim=-1).all(), (sampler, f0)


# 4 ---------------------------------------------------------------------------------------------
def oracle_den(preset, cfg, hub, st, em):
    w = weights(preset)
    if cfg:
        return lambda x, t: FO.fdm_forward_cfg(w, preset, hub, t, x, st, em, 2.5, folded=True)
    return lambda x, t: FO.fdm_forward(w, preset, hub, t, x, st, em, folded=True)


@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_single_calls_with_tracks_match_the_oracle(preset, cfg, dtype):
    """One denoiser call with a track that differs on every frame (keyframes with a 3-frame ramp), L in {7, 31}, t in {0, 999}, against
    oracle.fdm_oracle fed the same [L, n] tracks."""
    plan = plan_for(preset, dtype)
    p = plan.p
    for L in (7, 31):
        inp = inputs(preset, L, seed=9)
        st = tracks.keyframes(L, [(0, one_hot(p.n_style, 1)), (L // 2, one_hot(p.n_style, 4)), (L - 1, one_hot(p.n_style, 2))], ramp=3)
        em = tracks.keyframes(L, [(0, one_hot(p.n_emo, 0)), (L // 3 + 1, one_hot(p.n_emo, 5))], ramp=3) if p.n_emo else None
        plan.prepare(inp["hub"], L=L, cfg=cfg, style_track=st, emotion_track=em)
        den = oracle_den(preset, cfg, inp["hub"], st.unsqueeze(0), em.unsqueeze(0) if em is not None else None)
        for t in (0, 999):
            err = float((plan.denoise(dv(inp["x"]), t, cfg_scale=2.5).cpu() - den(inp["x"], t)).abs().max())
            print(f"[cond tracks {preset} mode {dtype}] L={L} t={t}: max|hip - oracle| = {err:.3e} (bar {TOL[dtype]:.0e})")
            assert err < TOL[dtype], (L, t)


@pytest.mark.parametrize("dtype", [F32, F16X3])
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_ddim_chain_with_switches_matches_the_oracle(preset, cfg, dtype):
    """The DDIM 4 chain of the prefix test (40 frames, switches at 17 and 33) against the oracle's ddim_sample: 1e-4."""
    plan, L = plan_for(preset, dtype), 40
    inp = inputs(preset, L)
    _, sw = cond_tracks(preset, L, [17, 33])
    plan.prepare(inp["hub"], L=L, cfg=cfg, **sw)
    out = plan.sample_ddim(dv(inp["x"]), 4, cfg_scale=2.5).cpu()
    p = plan.p
    st = sw["style_track"] if "style_track" in sw else sw["style"].expand(L, -1)
    em = sw.get("emotion_track")
    den = oracle_den(preset, cfg, inp["hub"], st.unsqueeze(0), em.unsqueeze(0) if p.n_emo else None)
    err = float((out - FO.ddim_sample(den, inp["x"].clone(), 4)).abs().max())
    print(f"[cond tracks {preset} mode {dtype}] DDIM 4 chain: max|hip - oracle| = {err:.3e}")
    assert err < 1e-4


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_slot_admitted_with_tracks_equals_its_solo_call(preset, cfg, dtype):
    """A sampler-bank session with DDIM 4 (sampler 0) and DPM-Solver++ 2M 4: slot 0 is admitted per clip, two steps later slot 1 joins
    with tracks on the other sampler (13 of the slot's 20 frames).  Slot 1 == prepare(tracks) + sample_tables alone with the same x_T,
    seed and clip id; the slot, reused with a plain admit, gives that clip's solo result (no track rows left behind)."""
    plan, Ls, L = plan_for(preset, dtype), 20, 13
    t2m, tab = schedule.sampler_tables("dpmpp2m", 4)
    a, b = inputs(preset, L, seed=31), inputs(preset, Ls, seed=32)
    _, sw = cond_tracks(preset, L, [6])
    # the solo calls
    plan.prepare(b["hub"], L=L, cfg=cfg, **sw)
    solo_b = plan.sample_tables(dv(a["x"]), t2m, tab, seed=77, clip0=5).clone()
    plan.prepare(a["hub"], a["style"], a.get("emo"), L=L, cfg=cfg)
    solo_a = plan.sample_ddim(dv(a["x"]), 4).clone()
    emo = lambda c: c["emo"][0] if c.get("emo") is not None else None
    plan.open_slots(2, Ls, kind="ddim", steps=4, cfg=cfg, samplers=1, sampler_steps=len(t2m))
    sid = plan.add_sampler(kind="tables", t_list=t2m, tables=tab)
    plan.admit(0, a["hub"][0], a["style"][0], emo(a), a["x"][0], L=L, seed=1, clip_id=0)
    plan.run(2)
    n_slot = plan.get("launches_per_step")
    plan.admit(1, b["hub"][0][: L * plan.p.pair], x_T=a["x"][0], L=L, seed=77, clip_id=5, sampler=sid, **sw)
    while plan.slot_state(1)[2] != SLOT_FINISHED:
        plan.run(1)
    assert plan.get("launches_per_step") == n_slot          # the step program is the same however its slots are admitted
    assert plan.slot_state(0)[2] == SLOT_FINISHED
    assert torch.equal(plan.read_slot(1, L), solo_b)
    assert torch.equal(plan.read_slot(0, L), solo_a)
    # the slot again, per clip: nothing of the tracks is left in its rows
    plan.admit(1, a["hub"][0], a["style"][0], emo(a), a["x"][0], L=L, seed=1, clip_id=0)
    while plan.slot_state(1)[2] != SLOT_FINISHED:
        plan.run(1)
    assert torch.equal(plan.read_slot(1, L), solo_a)


@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_group_admitted_with_tracks_equals_sample_windows(preset, cfg, dtype):
    """admit_long(tracks) over the windows of a 56-frame recording (slots of 24 frames, overlap 8, switch at frame 29) ==
    prepare_windows(tracks) + sample_windows (DDPM, Philox)."""
    plan, LT, Ls = plan_for(preset, dtype), 56, 24
    inp = inputs(preset, LT)
    _, sw = cond_tracks(preset, LT, [29])
    starts = plan.prepare_windows(inp["hub"], L_total=LT, window=Ls, overlap=8, cfg=cfg, **sw)
    ref = plan.sample_windows(dv(inp["x"]), kind="ddpm", t_list=DDPM_TS, seed=9, clip0=4).clone()
    n = len(starts)
    plan.open_slots(n + 1, Ls, kind="ddpm", t_list=DDPM_TS, cfg=cfg, long_frames=LT, long_groups=1)
    plan.admit_long(list(range(1, n + 1)), inp["hub"][0], x_T=inp["x"][0], L_total=LT, overlap=8, seed=9, clip_id=4, **sw)
    plan.run(len(DDPM_TS))
    assert torch.equal(plan.read_long(1), ref)


# window rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_MODES)
@pytest.mark.parametrize("preset,cfg", PRESETS)
def test_overlapping_window_rows_stay_equal_across_windows(preset, cfg, dtype):
    """After a chain with a switch inside an overlap (frame 34 of 56; windows of 24 at 0, 16, 32), every frame that two windows cover
    holds the same bits in both windows' rows, the long buffer's (fdm_window_peek)."""
    plan, LT, W_ = plan_for(preset, dtype), 56, 24
    inp = inputs(preset, LT)
    _, sw = cond_tracks(preset, LT, [34])
    starts = plan.prepare_windows(inp["hub"], L_total=LT, window=W_, overlap=8, cfg=cfg, **sw)
    G = plan.p.G
    for sampler in ("ddim", "ddpm"):
        out = frames(run(plan, dv(inp["x"]), sampler, windows=True), G)[0]
        rows = plan.peek_windows()[0].reshape(len(starts), W_, -1)
        for w, s in enumerate(starts):
            assert torch.equal(rows[w], out[s:s + W_]), (sampler, w)
        for (w0, s0), (w1, s1) in zip(enumerate(starts[:-1]), enumerate(starts[1:], 1)):
            n = s0 + W_ - s1
            assert n > 0 and torch.equal(rows[w0, W_ - n:], rows[w1, :n]), (sampler, w0)


# 6 ---------------------------------------------------------------------------------------------
def vq_plan(dtype=F32):
    from fdm_amd.vq import VQPlan
    if ("vq", dtype) not in _PLANS:
        _PLANS[("vq", dtype)] = VQPlan("mead", W.make_vq_weights("mead"), dtype, DEV)
    return _PLANS[("vq", dtype)]


def test_quant_with_an_emotion_track_is_the_per_emotion_quant_stitched():
    """MEAD (G = 8 latent vectors per frame, 7 codebooks): a constant track == quant(one-hot); three segments (frames 0-4 emotion 4,
    5-10 emotion 1, 11-12 emotion 6; 5 * 8 and 11 * 8 rows lie inside a 64-row workgroup range) == the three per-emotion calls
    stitched by frame; a cross-fade row goes by the argmax rule; quant_full's statistics take the same books."""
    vq = vq_plan()
    p, L, B = vq.p, 13, 2
    z = dv(torch.randn(B, L * p.G, p.c, generator=torch.Generator().manual_seed(3)))
    e = torch.eye(p.n_emo)
    per = {i: vq.quant(z, e[i]) for i in (1, 4, 6)}
    per = {i: (a.clone(), b.clone()) for i, (a, b) in per.items()}
    zq, idx = vq.quant(z, emotion_track=e[4].expand(L, -1))
    assert torch.equal(zq, per[4][0]) and torch.equal(idx, per[4][1])
    full_c = vq.quant_full(z, emotion_track=e[4].expand(L, -1))
    full_p = vq.quant_full(z, e[4])
    assert torch.equal(full_c[1], full_p[1]) and torch.equal(full_c[2][0], full_p[2][0]) and torch.equal(full_c[2][1], full_p[2][1])
    tr = tracks.keyframes(L, [(0, e[4]), (5, e[1]), (11, e[6])])
    zq, idx = vq.quant(z, emotion_track=tr)
    book = tracks.book_of(tr)
    assert book.tolist() == [4] * 5 + [1] * 6 + [6] * 2
    idx, G = idx.reshape(B, L, p.G), p.G
    for l in range(L):
        k = int(book[l])
        assert torch.equal(zq[:, :, l * G:(l + 1) * G], per[k][0][:, :, l * G:(l + 1) * G]), l
        assert torch.equal(idx[:, l], per[k][1].reshape(B, L, G)[:, l]), l
    # a cross-fade: frames 4, 5, 6 carry 0.25 / 0.5 / 0.75 of emotion 1; the tie at frame 5 goes to the first maximum, index 1
    tr = tracks.keyframes(L, [(0, e[4]), (5, e[1])], ramp=3)
    zq2, _ = vq.quant(z, emotion_track=tr)
    for l in range(L):
        k = 4 if l < 5 else 1
        assert torch.equal(zq2[:, :, l * G:(l + 1) * G], per[k][0][:, :, l * G:(l + 1) * G]), l


# 7 ---------------------------------------------------------------------------------------------
def test_pipeline_takes_tracks_in_animate_and_the_slot_server():
    """MEAD with guidance, DPM-Solver++ 2M 4: animate(emotion_track=constant) == animate(emotion_one_hot=); SlotServer.submit(track) ==
    animate(track); submit_long(track) == animate_long(track) on a recording of three windows."""
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    g = torch.Generator().manual_seed(23)
    wav, wav_long = [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in (12000, 64000)]
    diffusion, ae = pipeline.build_models("mead", device=DEV)
    e = torch.eye(7)
    kw = dict(sampler="dpmpp2m", sampler_steps=4, device=DEV)
    ref = pipeline.animate(diffusion, ae, wav, emotion_one_hot=e[5:6], seed=3, **kw)
    L = ref[1].shape[1] // 8
    con = pipeline.animate(diffusion, ae, wav, seed=3, emotion_track=e[5].expand(L, -1), **kw)
    assert torch.equal(con[1], ref[1]) and torch.equal(con[0], ref[0])
    tr = tracks.keyframes(L, [(0, e[4]), (L // 2, e[5])])
    a = pipeline.animate(diffusion, ae, wav, seed=3, emotion_track=tr, **kw)
    assert torch.equal(frames(a[1], 8)[:, :L // 2], frames(pipeline.animate(diffusion, ae, wav, emotion_one_hot=e[4:5], seed=3, **kw)[1], 8)[:, :L // 2])
    lref = pipeline.animate_long(diffusion, ae, wav_long, seed=4, window=40, overlap=10, sampler="dpmpp2m", sampler_steps=4, device=DEV)
    LT = lref[1].shape[1] // 8
    ltr = tracks.keyframes(LT, [(0, e[4]), (LT // 2 + 3, e[1])])
    b = pipeline.animate_long(diffusion, ae, wav_long, seed=4, window=40, overlap=10, sampler="dpmpp2m", sampler_steps=4, device=DEV, emotion_track=ltr)
    assert not torch.equal(b[1], lref[1])
    srv = pipeline.SlotServer(diffusion, ae, slots=4, max_frames=40, sampler="dpmpp2m", sampler_steps=4, device=DEV, long_frames=120,
                              long_groups=1, overlap=10)
    h0 = srv.submit(wav, seed=3, emotion_track=tr)
    h1 = srv.submit_long(wav_long, seed=4, emotion_track=ltr)
    got = {h: (v, lat) for h, v, lat in srv.drain(1)}
    for h, r in ((h0, a), (h1, b)):
        assert torch.equal(got[h][1], r[1]), h
        assert torch.equal(got[h][0], r[0]), h


def test_batch_calls_take_one_track_per_clip():
    """animate_many(emotion_track=[track, None, track]) == animate() per clip with that clip's track (or none), per clip and with
    batch_stages; SlotServer.submit_many with the same list == submit() in a loop.  MEAD with DPM-Solver++ 2M 4, clips of unequal length."""
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    g = torch.Generator().manual_seed(29)
    wavs = [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in (12000, 9000, 15000)]
    diffusion, ae = pipeline.build_models("mead", device=DEV)
    e = torch.eye(7)
    kw = dict(sampler="dpmpp2m", sampler_steps=4, device=DEV)
    trs = [tracks.keyframes(30, [(0, e[4]), (7, e[1])]), None, tracks.keyframes(30, [(0, e[2]), (5, e[6]), (11, e[4])], ramp=2)]
    ids = [torch.eye(25)[3:4], torch.eye(25)[1:2], torch.eye(25)[7:8]]
    # (animate_many keys the Philox stream by the clip's position; DPM-Solver++ 2M draws none, so the solo calls are comparable)
    refs = [pipeline.animate(diffusion, ae, w, id_one_hot=i, seed=5, emotion_track=t, **kw) for w, i, t in zip(wavs, ids, trs)]
    for stages in (False, True):
        verts, lats = pipeline.animate_many(diffusion, ae, wavs, id_one_hots=ids, seed=5, emotion_track=trs, batch_stages=stages, **kw)
        for b in range(3):
            assert torch.equal(lats[b], refs[b][1]), (stages, b)
            assert torch.equal(verts[b], refs[b][0]), (stages, b)
    for stages in (False, True):
        srv = pipeline.SlotServer(diffusion, ae, slots=3, max_frames=40, sampler="dpmpp2m", sampler_steps=4, device=DEV, batch_stages=stages)
        hs = srv.submit_many(wavs, id_one_hots=ids, seeds=5, emotion_track=trs)
        got = {h: (v, lat) for h, v, lat in srv.drain(1)}
        for b, h in enumerate(hs):
            assert torch.equal(got[h][1], refs[b][1]), (stages, b)
            assert torch.equal(got[h][0], refs[b][0]), (stages, b)


def test_demo_command_line_takes_a_style_track(tmp_path):
    """demo --style_track "0:0,0.5:3" (VOCASET, DDIM 3) == animate(style_track=tracks.from_spec(...))."""
    import numpy as np
    from scipy.io import wavfile
    from fdm_amd import pipeline, presets
    wav = (np.random.default_rng(2).standard_normal(16000) * 3000).astype(np.int16)
    wp = str(tmp_path / "hello.wav")
    wavfile.write(wp, 16000, wav)
    dst = pipeline.demo_main("vocaset", ["--audio_file", wp, "--audio_path", str(tmp_path / "result"), "--ddim_steps", "3",
                                         "--style_track", "0:0,0.5:3"])
    p = presets.get("vocaset")
    diffusion, ae = pipeline.build_models("vocaset", None, DEV)
    x = pipeline.processor_normalize(pipeline.load_wav(wp))
    st = tracks.from_spec(p, 600, "0:0,0.5:3", [str(i) for i in range(8)])
    assert tracks.book_of(st)[:30].tolist() == [0] * 25 + [3] * 5
    ref, _ = pipeline.animate(diffusion, ae, x, ddim_steps=3, device=DEV, style_track=st)
    plain, _ = pipeline.animate(diffusion, ae, x, ddim_steps=3, device=DEV)
    arr = torch.from_numpy(np.load(dst))
    assert torch.equal(arr, ref.cpu()) and not torch.equal(arr, plain.cpu())


def test_sampler_command_line_takes_an_emotion_track(tmp_path):
    """The sampler command line with --emotion_track "0:happy,0.4:sad" --track_ramp 0.2 (MEAD, 2M 3) == animate(emotion_track=...) on
    the loader's clip; the flag is refused on a model without emotions and together with --all_styles."""
    import importlib.util
    import os
    import sys
    import numpy as np
    from fdm_amd import pipeline, presets
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sd = os.path.join(here, "face-diffusion-model_amd", "dropin", "samples")
    sys.path.insert(0, os.path.dirname(sd))
    spec = importlib.util.spec_from_file_location("sample_diffusion", os.path.join(sd, "sample_diffusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "mead")
    flags = ["--clips", "1", "--seconds", "1.0", "--sampler", "dpmpp2m", "--sampler_steps", "3", "--out", out, "--device", DEV]
    mod.main("mead", flags + ["--emotion_track", "0:happy,0.4:sad", "--track_ramp", "0.2"])
    pm = presets.get("mead")
    audio, template, one_hot_all, name = next(iter(mod.synthetic_loader(pm, 1, 1.0)))
    diffusion, ae = pipeline.build_models("mead", None, DEV, "", "", single_clip=True)
    et = tracks.from_spec(pm, pm.max_len, "0:happy,0.4:sad", pipeline.EMOTIONS, ramp=0.2)
    assert et[0].argmax() == 4 and et[20].argmax() == 5 and 0 < float(et[10, 5]) < 1
    ref, _ = pipeline.animate(diffusion, ae, audio, template, one_hot_all[:, 0, :], torch.eye(7)[4:5], device=DEV, sampler="dpmpp2m",
                              sampler_steps=3, emotion_track=et)
    files = [f for f in os.listdir(out) if f.endswith(".npy")]
    assert len(files) == 1
    assert torch.equal(torch.from_numpy(np.load(os.path.join(out, files[0]))), ref.cpu())
    with pytest.raises(SystemExit):
        mod.main("vocaset", ["--emotion_track", "0:happy"])                        # no such flag on a model without emotions
    with pytest.raises(SystemExit):
        mod.main("mead", flags + ["--emotion_track", "0:happy", "--all_styles"])
