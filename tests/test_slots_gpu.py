"""GPU: in-flight batching (include/fdm_hip.h, "Slots"): clips at different diffusion steps in one step program.

The bar is bit identity (torch.equal): a clip admitted into a slot at any step boundary, beside clips of other lengths at other
steps, ends with the latent its solo sample_* call returns on a (1, L_clip) plan with the same weights, x_T, seed and
clip0 = clip_id -- in every arithmetic mode, for DDIM, DDPM with Philox noise and the table-driven sampler (history), with and
without guidance.  Operators first (the per-clip LayerNorm form, fdm_op_slot_sched), then staggered chains, slot reuse, frozen /
idle slots, the oracle (1e-4, not through the solo GPU path), validation, launch counts and the pipeline's SlotServer.  Tiny
presets; L = 33 / 31 cross the period-30 positional table and one 32-key tile."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd import ops, schedule  # noqa: E402
from fdm_amd._lib import BF16, F16, F16X3, F32, SLOT_FINISHED, SLOT_IDLE, SLOT_RUNNING, FdmError  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"
TOL32 = 1e-4                     # the contract's bar for the fp32 and split-fp16 modes (tests/test_denoiser_gpu.py)
ALL_MODES = [F32, BF16, F16X3, F16]
_PLANS, _CLIPS, _REFS = {}, {}, {}

DDPM_TS = [999, 800, 600, 400, 200, 50, 1, 0]          # ends at t = 0: the no-noise branch
SAMPLERS = {
    "ddim": lambda: dict(kind="ddim", steps=6),
    "ddpm": lambda: dict(kind="ddpm", t_list=DDPM_TS),
    "2m": lambda: dict(zip(("kind", "t_list", "tables"), ("tables",) + tuple(schedule.sampler_tables("dpmpp2m", 5)))),
}


def dv(t):
    return t.to(DEV)


def plan_for(preset, dtype):
    if (preset, dtype) not in _PLANS:
        _PLANS[(preset, dtype)] = DenoiserPlan(preset, W.make_fdm_weights(preset), dtype, DEV)
    return _PLANS[(preset, dtype)]


def clip(preset, L, i):
    """Clip i: its own audio features, one-hots, x_T, Philox seed and clip id."""
    if (preset, L, i) not in _CLIPS:
        c = W.synth_inputs(preset, 1, L, seed=50 + i)
        c.update(L=L, seed=100 + 7 * i, clip_id=(3, 0, 7, 2)[i % 4])
        _CLIPS[(preset, L, i)] = c
    return _CLIPS[(preset, L, i)]


def solo(plan, preset, c, sampler, cfg=False, scale=2.5):
    """The clip alone on a (1, L_clip) shape of the same plan: the existing samplers (fused epilogue without guidance)."""
    key = (preset, plan.dtype, c["L"], c["seed"], sampler, cfg)
    if key not in _REFS:
        plan.prepare(c["hub"], c["style"], c.get("emo"), L=c["L"], cfg=cfg)
        kw, x = SAMPLERS[sampler](), dv(c["x"])
        if sampler == "ddim":
            out = plan.sample_ddim(x, kw["steps"], cfg_scale=scale)
        elif sampler == "ddpm":
            out = plan.sample_ddpm(x, kw["t_list"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
        else:
            out = plan.sample_tables(x, kw["t_list"], kw["tables"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
        _REFS[key] = out.clone()
    return _REFS[key]


def admit(plan, slot, c):
    plan.admit(slot, c["hub"][0], c["style"][0], c["emo"][0] if c.get("emo") is not None else None, c["x"][0], L=c["L"],
               seed=c["seed"], clip_id=c["clip_id"])


def run_staggered(plan, admits, pieces, on_piece=None):
    """admits: [(at_step, slot, clip)]; pieces: run() sizes, cycled until every admitted clip has been read.  A clip is admitted at
    the first piece boundary at or after at_step.  Returns {id(clip): latent}."""
    todo, where, out, done, i = sorted(admits, key=lambda a: a[0]), {}, {}, 0, 0
    while todo or where:
        while todo and todo[0][0] <= done:
            _, slot, c = todo.pop(0)
            admit(plan, slot, c)
            where[slot] = c
        n = pieces[i % len(pieces)]
        plan.run(n)
        done, i = done + n, i + 1
        for slot in list(where):
            if plan.slot_state(slot)[2] == SLOT_FINISHED:
                c = where.pop(slot)
                out[id(c)] = plan.read_slot(slot, c["L"])
        if on_piece:
            on_piece(done)
        assert i < 64
    return out


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("two_stage", [True, False])
@pytest.mark.parametrize("wrap", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_layernorm_per_clip_table_row(dtype, wrap, two_stage):
    """3 clips x 7 rows (x 2 halves with wrap), d = 256, three step words: each clip's rows equal the single-word call on its slice."""
    d, rows, clips = 256, 7, 3
    half = rows * clips
    M = half * (2 if wrap else 1)
    g = torch.Generator().manual_seed(3)
    x, add = dv(torch.randn(M, d, generator=g)), dv(torch.randn(M, d, generator=g))
    tab = dv(torch.randn(10, d, generator=g))
    ga, be, ga2, be2 = [dv(torch.randn(d, generator=g)) for _ in range(4)]
    words = [5, 0, 9]
    state = torch.zeros(clips, 4, dtype=torch.int32)
    state[:, 1] = torch.tensor(words)
    state[:, 0] = torch.tensor([77, 78, 79])                    # the other words of the state are not the gather's business
    state = dv(state)
    kw = dict(add_mat=add, add_tab=tab, dtype=dtype)
    if two_stage:
        kw.update(gamma2=ga2, beta2=be2)
    y, yt = torch.zeros(M, d, device=DEV), torch.zeros(M, d, device=DEV, dtype=ops.tdtype(dtype))
    ops.layernorm(x, ga, be, M, d, y_f32=y, y_t=yt if dtype != F32 else None, clip_step=state[:, 1:], clip_step_stride=4, clip_rows=rows,
                  clip_wrap=half if wrap else 0, **kw)
    for h in range(2 if wrap else 1):
        for c in range(clips):
            r0 = h * half + c * rows
            step = torch.tensor([words[c]], dtype=torch.int32, device=DEV)
            ry, ryt = torch.zeros(rows, d, device=DEV), torch.zeros(rows, d, device=DEV, dtype=ops.tdtype(dtype))
            k1 = dict(kw, add_mat=add[r0:r0 + rows])
            ops.layernorm(x[r0:r0 + rows], ga, be, rows, d, y_f32=ry, y_t=ryt if dtype != F32 else None, tab_step=step, **k1)
            assert torch.equal(y[r0:r0 + rows], ry), (h, c)
            if dtype != F32:
                assert torch.equal(yt[r0:r0 + rows], ryt), (h, c)
    assert not torch.equal(y[:rows], y[rows:2 * rows])


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_op_slot_sched_equals_sched_step_per_live_clip(mode, cfg):
    """3 clips x 7 frames, states {live k = 0, live k = last with t = 0, not live}: the live clips get fdm_op_sched_step's bits at
    their own k (seed and clip id of the slot), the third keeps a sentinel in x, every operand copy and x0_hist."""
    d, frames, clips = 64, 7, 3
    npc, n = frames * d, frames * d * clips
    g = torch.Generator().manual_seed(20 + mode)
    x0, x0u, x, hist0 = [torch.randn(n, generator=g) * 2 for _ in range(4)]
    tseq = torch.tensor([999, 500, 0], dtype=torch.int32)
    ks = [0, 2, 1]
    state = dv(torch.tensor([[0, 999, 1, 1], [2, 0, 1, 1], [1, 500, 0, 1]], dtype=torch.int32))
    seeds, ids = [1234, 2 ** 40 + 5, 99], [3, 0, 8]
    keys = dv(torch.tensor([[s, c] for s, c in zip(seeds, ids)], dtype=torch.int64))
    c1, c2, sg = schedule.ddpm_tables(schedule.make_buffers(1000))
    buf = schedule.make_buffers(1000)
    tabs = {}
    if mode == 0:
        tabs = dict(c1=dv(c1), c2=dv(c2), sigma=dv(sg))
    elif mode == 1:
        tabs = dict(sra=dv(buf["sqrt_recip_alphas_cumprod"]), srm1=dv(buf["sqrt_recipm1_alphas_cumprod"]),
                    sqrt_an=dv(torch.tensor([0.3, 0.6, 0.9])), c_n=dv(torch.tensor([0.95, 0.8, 0.43])))
    else:      # step 0: no history, noise; step 2: history and noise
        tabs = dict(lm_a=dv(torch.tensor([0.9518, 0.853, 0.7313])), lm_b=dv(torch.tensor([0.3067, 0.3352, 0.5269])),
                    lm_c=dv(torch.tensor([0.0, -0.013, -0.1491])), lm_s=dv(torch.tensor([0.25, 0.0, 0.4338])))
    SENT = 7.5

    def outs(count, rows_extra=0):
        o = dict(f32=torch.full((count,), SENT, device=DEV), bf16=torch.full((count,), SENT, device=DEV, dtype=torch.bfloat16),
                 f16=torch.full((count,), SENT, device=DEV, dtype=torch.float16),
                 split=ops.Split(torch.full((2, count // d + rows_extra, d), SENT, device=DEV, dtype=torch.float16), F16X3))
        return o
    common = dict(x0u=dv(x0u) if cfg else None, cfg_scale=2.5, **tabs)
    got, got_hist = outs(n, rows_extra=5), {}                    # (the split copy's plane distance is 5 rows larger than n)
    assert got["split"].lo_off > n
    for name in ("bf16", "f16", "split", None):
        o = got["f32"] if name is None else torch.full((n,), SENT, device=DEV)
        hist = dv(hist0.clone())
        hist[2 * npc:] = SENT
        ops.slot_sched(mode, dv(x0), dv(x), o, n, state, keys, clips, n_per_clip=npc, x_out_t=got[name] if name else None,
                       x0_hist=hist if mode == 3 else None, **common)
        got_hist[name] = hist
        if name is not None:
            assert torch.equal(o[2 * npc:], torch.full((npc,), SENT, device=DEV)), name
    for c in range(2):
        sl = slice(c * npc, (c + 1) * npc)
        step = torch.tensor([ks[c]], dtype=torch.int32, device=DEV)
        ref = outs(npc)
        for name in ("bf16", "f16", "split", None):
            hist = dv(hist0[sl].clone())
            o = ref["f32"] if name is None else torch.zeros(npc, device=DEV)
            ops.sched_step(mode, dv(x0[sl]), dv(x[sl]), o, npc, x0u=dv(x0u[sl]) if cfg else None, cfg_scale=2.5, n_per_clip=npc,
                           tseq=dv(tseq), step=step, seed=seeds[c], clip0=ids[c], x_out_t=ref[name] if name else None,
                           x0_hist=hist if mode == 3 else None, **tabs)
            if mode == 3:
                assert torch.equal(got_hist[name][sl], hist), (c, name)
        assert torch.equal(got["f32"][sl], ref["f32"]), c
        assert torch.equal(got["bf16"][sl], ref["bf16"]) and torch.equal(got["f16"][sl], ref["f16"]), c
        for pl in range(2):
            assert torch.equal(got["split"].planes[pl].reshape(-1)[sl], ref["split"].planes[pl].reshape(-1)), (c, pl)
        assert not torch.equal(got["f32"][sl], torch.full((npc,), SENT, device=DEV))
    # the clip that is not live: nothing of it was stored
    dead = slice(2 * npc, 3 * npc)
    assert torch.equal(got["f32"][dead], torch.full((npc,), SENT, device=DEV))
    for name in ("bf16", "f16"):
        assert torch.equal(got[name][dead].float(), torch.full((npc,), SENT, device=DEV)), name
    for pl in range(2):
        assert torch.equal(got["split"].planes[pl].reshape(-1)[dead].float(), torch.full((npc,), SENT, device=DEV))
        assert torch.equal(got["split"].planes[pl].reshape(-1)[3 * npc:].float(), torch.full((5 * d,), SENT, device=DEV))     # past n: untouched
    if mode == 3:
        for name, h in got_hist.items():
            assert torch.equal(h[dead], torch.full((npc,), SENT, device=DEV)), name
    if mode != 1:      # the two live clips drew different noise streams / the t = 0 step drew none
        assert not torch.equal(got["f32"][:npc], got["f32"][npc:2 * npc])


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
@pytest.mark.parametrize("dtype", ALL_MODES)
def test_staggered_chains_equal_solo_chains(dtype, sampler):
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    clips = [clip(preset, 33, 0), clip(preset, 31, 1), clip(preset, 7, 2)]
    refs = [solo(plan, preset, c, sampler) for c in clips]
    plan.open_slots(3, L, **SAMPLERS[sampler]())
    assert plan.get("slots") == 3
    out = run_staggered(plan, [(0, 0, clips[0]), (2, 1, clips[1]), (5, 2, clips[2])], [2, 3, 1])
    for c, r in zip(clips, refs):
        assert torch.equal(out[id(c)], r), (c["L"], sampler)
    assert not torch.equal(refs[0][:, :7 * plan.p.G], refs[2])


@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_staggered_chains_with_guidance(dtype, sampler):
    preset, L = "mead_tiny", 8
    plan = plan_for(preset, dtype)
    clips = [clip(preset, 7, 0), clip(preset, 8, 1)]
    refs = [solo(plan, preset, c, sampler, cfg=True, scale=1.7) for c in clips]
    plan.open_slots(2, L, cfg=True, cfg_scale=1.7, **SAMPLERS[sampler]())
    out = run_staggered(plan, [(0, 1, clips[0]), (2, 0, clips[1])], [2, 3, 1])
    for c, r in zip(clips, refs):
        assert torch.equal(out[id(c)], r), (c["L"], sampler)


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddpm", "2m"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_slot_reuse_resets_history_and_state(dtype, sampler):
    """Slot 0 finishes and is read; another clip and seed go into it while slot 1 is mid-chain."""
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    a, b, c = clip(preset, 31, 1), clip(preset, 33, 0), clip(preset, 7, 2)
    refs = [solo(plan, preset, k, sampler) for k in (a, b, c)]
    n = plan.open_slots(2, L, **SAMPLERS[sampler]())
    admit(plan, 0, a)
    plan.run(3)
    admit(plan, 1, b)
    plan.run(n - 3)
    assert plan.slot_state(0) == (n, n, SLOT_FINISHED) and plan.slot_state(1) == (n - 3, n, SLOT_RUNNING)
    got_a = plan.read_slot(0, a["L"])
    admit(plan, 0, c)                                        # slot 1 has 3 steps to go
    plan.run(3)
    assert plan.slot_state(1)[2] == SLOT_FINISHED and plan.slot_state(0) == (3, n, SLOT_RUNNING)
    plan.run(n)                                              # more than slot 0 needs: it freezes at its end
    got_b, got_c = plan.read_slot(1, b["L"]), plan.read_slot(0, c["L"])
    for got, r in zip((got_a, got_b, got_c), refs):
        assert torch.equal(got, r)


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_frozen_idle_read_and_run_splitting(dtype):
    preset, L, sampler = "vocaset_tiny", 33, "ddpm"
    plan = plan_for(preset, dtype)
    a, b = clip(preset, 7, 2), clip(preset, 31, 1)
    ref_a, ref_b = solo(plan, preset, a, sampler), solo(plan, preset, b, sampler)

    def session(pieces, use_graph=True):
        n = plan.open_slots(3, L, use_graph=use_graph, graph_steps=3, **SAMPLERS[sampler]())
        admit(plan, 0, a)
        plan.run(2)
        admit(plan, 1, b)
        for p in pieces:
            plan.run(p)
        return n, [plan.peek_slot(s) for s in range(3)]
    n, rows_34 = session([3, 4])
    _, rows_7 = session([7])
    _, rows_eager = session([7], use_graph=False)
    for s in range(3):
        assert torch.equal(rows_34[s], rows_7[s]) and torch.equal(rows_eager[s], rows_7[s]), s
    # after 9 steps: slot 0 finished at step 8 and has been frozen for one step, slot 1 is at step 7, slot 2 never admitted
    assert n == 8
    assert plan.slot_state(0) == (8, 8, SLOT_FINISHED) and plan.slot_state(1) == (7, 8, SLOT_RUNNING) and plan.slot_state(2) == (0, 8, SLOT_IDLE)
    G = plan.p.G
    assert torch.equal(rows_7[0][:, :a["L"] * G], ref_a)
    assert not rows_7[2].any()                               # the idle slot holds zeros
    # (the padding rows L_clip .. L of a live slot are updated with the slot, as the tail rows of animate_many's end padding are:
    #  they start at zero, stay finite, never reach the clip's own frames -- the denoiser is causal -- and are not read out)
    assert torch.isfinite(rows_7[0]).all()
    with pytest.raises(FdmError, match="-4"):                # reading a running slot
        plan.read_slot(1, b["L"])
    with pytest.raises(FdmError, match="-4"):                # ... or an idle one
        plan.read_slot(2, 7)
    plan.run(5)                                              # slot 1 ends after one more step; slot 0 stays frozen
    assert torch.equal(plan.peek_slot(0), rows_7[0]) and not plan.peek_slot(2).any()
    assert torch.equal(plan.read_slot(0, a["L"]), ref_a)
    assert plan.slot_state(0) == (0, 8, SLOT_IDLE)
    with pytest.raises(FdmError, match="-4"):                # a second read
        plan.read_slot(0, a["L"])
    assert torch.equal(plan.read_slot(1, b["L"]), ref_b)


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16X3])
def test_staggered_ddim_against_the_oracle(dtype):
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    w = W.make_fdm_weights(preset)
    clips = [clip(preset, 33, 0), clip(preset, 31, 1), clip(preset, 7, 2)]
    plan.open_slots(3, L, **SAMPLERS["ddim"]())
    out = run_staggered(plan, [(0, 0, clips[0]), (2, 1, clips[1]), (5, 2, clips[2])], [2, 3, 1])
    for c in clips:
        key = ("oracle", c["L"])
        if key not in _REFS:
            den = lambda x, t, c=c: FO.fdm_forward(w, preset, c["hub"], t, x, c["style"], None, folded=True)
            _REFS[key] = FO.ddim_sample(den, c["x"].clone(), 6)
        err = float((out[id(c)].cpu().double() - _REFS[key].double()).abs().max())
        print(f"[slots ddim dtype {dtype} L {c['L']}] vs the oracle {err:.2e}")
        assert err < TOL32


# 6 ---------------------------------------------------------------------------------------------
def test_validation_and_return_to_plain_mode():
    preset, L = "vocaset_tiny", 33
    fresh = DenoiserPlan(preset, W.make_fdm_weights(preset), F32, DEV)
    with pytest.raises(FdmError, match="-4"):                # run before open
        fresh.run(1)
    a, b = clip(preset, 31, 1), clip(preset, 7, 2)
    fresh.prepare(a["hub"], a["style"], L=a["L"])
    ref = fresh.sample_ddpm(dv(a["x"]), DDPM_TS, seed=5)
    with pytest.raises(FdmError, match="-4"):                # still plain
        fresh.run(1)
    plan = plan_for(preset, F32)
    plan.open_slots(2, 8, **SAMPLERS["ddim"]())
    with pytest.raises(FdmError, match="-2"):                # L_clip > L
        admit(plan, 0, a)
    plan.open_slots(2, L, **SAMPLERS["ddim"]())
    admit(plan, 0, a)
    with pytest.raises(FdmError, match="-4"):                # busy: running
        admit(plan, 0, b)
    for slot in (-1, 2):
        with pytest.raises(FdmError, match="-1"):
            admit(plan, slot, b)
    plan.run(5)
    with pytest.raises(FdmError, match="-4"):                # busy: finished and not read
        admit(plan, 0, b)
    plan._check_x = lambda x: x.to(DEV)                       # (the binding's own shape check is not under test)
    try:
        with pytest.raises(FdmError, match="-4"):            # the plain samplers refuse a slot-mode plan
            plan.sample_ddim(dv(a["x"]), 6)
    finally:
        del plan._check_x
    assert plan.get("slots") == 2
    plan.prepare(a["hub"], a["style"], L=a["L"])             # back to plain mode
    assert plan.get("slots") == 0
    assert torch.equal(plan.sample_ddpm(dv(a["x"]), DDPM_TS, seed=5), ref)
    with pytest.raises(FdmError, match="-4"):
        plan.run(1)


# 7 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
def test_launch_counts(sampler):
    preset, n_layers = "vocaset_tiny", 2
    plan = plan_for(preset, BF16)
    assert plan.p.n_layers == n_layers
    a = clip(preset, 7, 2)
    plan.open_slots(2, 33, **SAMPLERS[sampler]())
    admit(plan, 0, a)
    plan.run(1)
    assert plan.get("launches_per_step") == 2 + 7 * n_layers + 2        # advance + chain (decoder unfused) + the slot pass
    plan.prepare(a["hub"], a["style"], L=a["L"])
    plan.sample_ddim(dv(a["x"]), 6)
    assert plan.get("launches_per_step") == 2 + 7 * n_layers


# 8 ---------------------------------------------------------------------------------------------
def test_pipeline_slot_server_equals_animate():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "dropin"))
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    # (the VQ stage fixes G * c = 1024, so the pipeline has no tiny preset: the full VOCASET geometry on about a second of audio)
    g = torch.Generator().manual_seed(9)
    wavs = [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in (16000, 11000, 13500)]
    seeds = [4, 5, 6]
    diffusion, ae = pipeline.build_models("vocaset", device=DEV)
    refs = [pipeline.animate(diffusion, ae, w, ddim_steps=4, seed=s, device=DEV) for w, s in zip(wavs, seeds)]
    assert len({r[1].shape[1] for r in refs}) == 3
    srv = pipeline.SlotServer(diffusion, ae, slots=2, ddim_steps=4, device=DEV)
    assert srv.chain == 3
    h0 = srv.submit(wavs[0], seed=seeds[0])
    srv.step(1)
    h1 = srv.submit(wavs[1], seed=seeds[1])
    h2 = srv.submit(wavs[2], seed=seeds[2])                   # both slots are busy: it waits in the queue
    assert srv.pending == 3 and len(srv._queue) == 1
    srv.step(1)
    assert srv.results() == []
    got = {h: (v, lat) for h, v, lat in srv.drain(1)}
    assert sorted(got) == [h0, h1, h2] and srv.pending == 0
    for h, r in zip((h0, h1, h2), refs):
        assert torch.equal(got[h][1], r[1]), h
        assert torch.equal(got[h][0], r[0]), h
