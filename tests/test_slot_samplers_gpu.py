"""GPU: samplers per request in slot mode (include/fdm_hip.h, "Samplers per request in slot mode"): the slots of one step program run
DIFFERENT samplers and guidance scales.

The bar is bit identity per request (torch.equal): a slot's latent is the solo sample_* call on a (1, L_clip) plan with that request's
sampler and scale, a group's latent is sample_windows with them -- whatever the other slots run.  The operator first
(fdm_op_slot_sched_bank against fdm_op_sched_step per live clip), then mixed chains in all four arithmetic modes, same-kind samplers
of different lengths (offsets), guidance scales, the bank's life cycle, a long group on a non-default sampler, compatibility with
the plain slot program, the CPU oracle (1e-4, not through the solo GPU path) and the pipeline's SlotServer.  Tiny presets."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd import ops, schedule  # noqa: E402
from fdm_amd._lib import BF16, F16, F16X3, F32, SLOT_FINISHED, SLOT_RUNNING, FdmError  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan, window_starts  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"
TOL32 = 1e-4                     # the contract's bar for the fp32 and split-fp16 modes (tests/test_denoiser_gpu.py)
ALL_MODES = [F32, BF16, F16X3, F16]
_PLANS, _CLIPS, _REFS = {}, {}, {}

DDPM_TS = [999, 800, 600, 400, 200, 50, 1, 0]          # ends at t = 0: the no-noise branch
DEFS = {
    "ddim4": lambda: dict(kind="ddim", steps=4),
    "ddim6": lambda: dict(kind="ddim", steps=6),
    "ddim9": lambda: dict(kind="ddim", steps=9),
    "ddpm": lambda: dict(kind="ddpm", t_list=DDPM_TS),
    "2m": lambda: dict(zip(("kind", "t_list", "tables"), ("tables",) + tuple(schedule.sampler_tables("dpmpp2m", 5)))),
}
STEPS = {"ddim4": 3, "ddim6": 5, "ddim9": 8, "ddpm": 8, "2m": 5}      # live steps of a chain (DDIM: the dead last pair is skipped)


def dv(t):
    return t.to(DEV)


def plan_for(preset, dtype):
    if (preset, dtype) not in _PLANS:
        _PLANS[(preset, dtype)] = DenoiserPlan(preset, W.make_fdm_weights(preset), dtype, DEV)
    return _PLANS[(preset, dtype)]


def clip(preset, L, i):
    """Clip i: its own audio features, one-hots, x_T, Philox seed and clip id."""
    if (preset, L, i) not in _CLIPS:
        c = W.synth_inputs(preset, 1, L, seed=90 + i)
        c.update(L=L, seed=300 + 7 * i, clip_id=(3, 0, 7, 2)[i % 4])
        _CLIPS[(preset, L, i)] = c
    return _CLIPS[(preset, L, i)]


def solo(plan, preset, c, name, cfg=False, scale=2.5, window=None, overlap=10):
    """The clip alone with sampler `name`: on a (1, L_clip) plain plan, or (window given) on a B = 1 windowed plan."""
    key = (preset, plan.dtype, c["L"], c["seed"], name, cfg, scale, window)
    if key not in _REFS:
        kw, x = DEFS[name](), dv(c["x"])
        if window:
            plan.prepare_windows(c["hub"], c["style"], c.get("emo"), L_total=c["L"], window=window, overlap=overlap, cfg=cfg)
            out = plan.sample_windows(x, kind=kw["kind"], steps=kw.get("steps"), t_list=kw.get("t_list"), tables=kw.get("tables"),
                                      seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
        else:
            plan.prepare(c["hub"], c["style"], c.get("emo"), L=c["L"], cfg=cfg)
            if kw["kind"] == "ddim":
                out = plan.sample_ddim(x, kw["steps"], cfg_scale=scale)
            elif kw["kind"] == "ddpm":
                out = plan.sample_ddpm(x, kw["t_list"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
            else:
                out = plan.sample_tables(x, kw["t_list"], kw["tables"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
        _REFS[key] = out.clone()
    return _REFS[key]


def admit(plan, slot, c, sampler=0, cfg_scale=None):
    plan.admit(slot, c["hub"][0], c["style"][0], c["emo"][0] if c.get("emo") is not None else None, c["x"][0], L=c["L"],
               seed=c["seed"], clip_id=c["clip_id"], sampler=sampler, cfg_scale=cfg_scale)


def open_bank(plan, slots, L, default, others, **kw):
    """Open with sampler 0 = `default` and add `others`; returns {name: bank id}."""
    n = plan.open_slots(slots, L, samplers=max(len(others), 1), sampler_steps=max(sum(STEPS[o] for o in others), 1), **DEFS[default](), **kw)
    assert n == STEPS[default] and plan.get("slot_samplers") == max(len(others), 1)
    ids = {default: 0}
    for o in others:
        ids[o] = plan.add_sampler(**DEFS[o]())
        assert ids[o] >= 1 and plan.sampler_info(ids[o])[1] == STEPS[o]
    return ids


def run_mixed(plan, admits, pieces):
    """admits: [(at_step, slot, clip, sampler id, steps of its chain, cfg_scale)]; pieces: run() sizes, cycled until every clip has been
    read.  A clip is admitted at the first piece boundary at or after at_step.  Returns {id(clip): latent}."""
    todo, where, out, done, i = sorted(admits, key=lambda a: a[0]), {}, {}, 0, 0
    while todo or where:
        while todo and todo[0][0] <= done:
            _, slot, c, sid, total, scale = todo.pop(0)
            admit(plan, slot, c, sid, scale)
            assert plan.slot_state(slot) == (0, total, SLOT_RUNNING)          # the slot's OWN total
            where[slot] = (c, total)
        n = pieces[i % len(pieces)]
        plan.run(n)
        done, i = done + n, i + 1
        for slot in list(where):
            d, t, st = plan.slot_state(slot)
            assert t == where[slot][1] and d <= t
            if st == SLOT_FINISHED:
                c = where.pop(slot)[0]
                out[id(c)] = plan.read_slot(slot, c["L"])
        assert i < 64
    return out


def f32_bits(v):
    return int(torch.tensor(v, dtype=torch.float32).view(torch.int32))


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [False, True])
def test_op_slot_sched_bank_equals_sched_step_per_live_clip(cfg):
    """4 clips x 7 frames, d = 64, one launch: a DDPM slot at its final t = 0, a DDIM slot, a table-driven slot at a step with
    c[k] != 0 and a slot that is not live, each with its own scale.  Every live clip gets fdm_op_sched_step's bits on its slice with
    its mode, tables, k, seed, clip id and scale, in fp32 and in every operand kind of x_out_t; the dead clip keeps a sentinel in x,
    every operand copy and its history; the history rows of the DDPM and DDIM slots are untouched."""
    d, frames, clips = 64, 7, 4
    npc, n = frames * d, frames * d * clips
    g = torch.Generator().manual_seed(31)
    x0, x0u, x, hist0 = [torch.randn(n, generator=g) * 2 for _ in range(4)]
    buf = schedule.make_buffers(1000)
    c1, c2, sg = schedule.ddpm_tables(buf)
    shared = dict(c1=dv(c1), c2=dv(c2), sigma=dv(sg), sra=dv(buf["sqrt_recip_alphas_cumprod"]), srm1=dv(buf["sqrt_recipm1_alphas_cumprod"]))
    # the bank: sampler 0 DDPM over [999, 500, 0]; sampler 1 DDIM, 3 steps; sampler 2 table-driven, 3 steps; padding between the ranges
    tl = {0: [999, 500, 0], 1: [900, 500, 100], 2: [950, 450, 0]}
    san, cn = [0.3, 0.6, 0.9], [0.95, 0.8, 0.43]
    lm = dict(lm_a=[0.9518, 0.853, 0.7313], lm_b=[0.3067, 0.3352, 0.5269], lm_c=[0.0, -0.013, -0.1491], lm_s=[0.25, 0.0, 0.4338])
    PAD = 77.0
    bank_t = torch.tensor(tl[0] + [5000] + tl[1] + [-3, -3] + tl[2], dtype=torch.int32)
    coef = torch.tensor([PAD] * 4 + san + cn + [PAD] * 2 + lm["lm_a"] + lm["lm_b"] + lm["lm_c"] + lm["lm_s"] + [PAD])
    desc = torch.tensor([[0, 3, 0, 0], [1, 3, 4, 4], [3, 3, 9, 12]], dtype=torch.int32)
    modes, ks, ts = [0, 1, 3, 1], [2, 1, 2, 1], [0, 500, 0, 500]
    scales = [1.5, 2.5, 3.5, 4.5]
    seeds, ids = [1234, 2 ** 40 + 5, 99, 7], [3, 0, 8, 1]
    state = dv(torch.tensor([[2, 0, 1, 1], [1, 500, 1, 1], [2, 0, 1, 1], [1, 500, 0, 1]], dtype=torch.int32))
    keys = dv(torch.tensor([[s, c] for s, c in zip(seeds, ids)], dtype=torch.int64))
    req = dv(torch.tensor([[sid, f32_bits(sc), 0, 0] for sid, sc in zip([0, 1, 2, 1], scales)], dtype=torch.int32))
    bank = dict(req=req, desc=dv(desc), t=dv(bank_t), coef=dv(coef))
    SENT = 7.5

    def outs(count, rows_extra=0):
        return dict(f32=torch.full((count,), SENT, device=DEV), bf16=torch.full((count,), SENT, device=DEV, dtype=torch.bfloat16),
                    f16=torch.full((count,), SENT, device=DEV, dtype=torch.float16),
                    split=ops.Split(torch.full((2, count // d + rows_extra, d), SENT, device=DEV, dtype=torch.float16), F16X3))
    got, got_hist = outs(n, rows_extra=5), {}
    for name in ("bf16", "f16", "split", None):
        o = got["f32"] if name is None else torch.full((n,), SENT, device=DEV)
        hist = dv(hist0.clone())
        hist[3 * npc:] = SENT
        ops.slot_sched_bank(dv(x0), dv(x), o, n, state, keys, clips, n_per_clip=npc, x0u=dv(x0u) if cfg else None,
                            x_out_t=got[name] if name else None, x0_hist=hist, **shared, **bank)
        got_hist[name] = hist
        if name is not None:
            assert torch.equal(o[3 * npc:], torch.full((npc,), SENT, device=DEV)), name
    step_tabs = {0: {}, 1: dict(sqrt_an=dv(torch.tensor(san)), c_n=dv(torch.tensor(cn))), 3: {k: dv(torch.tensor(v)) for k, v in lm.items()}}
    for c in range(3):
        sl = slice(c * npc, (c + 1) * npc)
        step = torch.tensor([ks[c]], dtype=torch.int32, device=DEV)
        tseq = dv(torch.tensor(tl[c], dtype=torch.int32))
        assert tl[c][ks[c]] == ts[c]
        ref = outs(npc)
        for name in ("bf16", "f16", "split", None):
            hist = dv(hist0[sl].clone())
            o = ref["f32"] if name is None else torch.zeros(npc, device=DEV)
            ops.sched_step(modes[c], dv(x0[sl]), dv(x[sl]), o, npc, x0u=dv(x0u[sl]) if cfg else None, cfg_scale=scales[c], n_per_clip=npc,
                           tseq=tseq, step=step, seed=seeds[c], clip0=ids[c], x_out_t=ref[name] if name else None,
                           x0_hist=hist if modes[c] == 3 else None, **shared, **step_tabs[modes[c]])
            # mode 3 rewrote its history rows as the solo call does; modes 0 and 1 never touched theirs
            assert torch.equal(got_hist[name][sl], hist if modes[c] == 3 else dv(hist0[sl])), (c, name)
        assert torch.equal(got["f32"][sl], ref["f32"]), c
        assert torch.equal(got["bf16"][sl], ref["bf16"]) and torch.equal(got["f16"][sl], ref["f16"]), c
        for pl in range(2):
            assert torch.equal(got["split"].planes[pl].reshape(-1)[sl], ref["split"].planes[pl].reshape(-1)), (c, pl)
        assert not torch.equal(got["f32"][sl], torch.full((npc,), SENT, device=DEV))
    assert lm["lm_c"][ks[2]] != 0.0
    dead = slice(3 * npc, 4 * npc)
    assert torch.equal(got["f32"][dead], torch.full((npc,), SENT, device=DEV))
    for name in ("bf16", "f16"):
        assert torch.equal(got[name][dead].float(), torch.full((npc,), SENT, device=DEV)), name
    for pl in range(2):
        assert torch.equal(got["split"].planes[pl].reshape(-1)[dead].float(), torch.full((npc,), SENT, device=DEV))
        assert torch.equal(got["split"].planes[pl].reshape(-1)[4 * npc:].float(), torch.full((5 * d,), SENT, device=DEV))     # past n: untouched
    for name, h in got_hist.items():
        assert torch.equal(h[dead], torch.full((npc,), SENT, device=DEV)), name
    if cfg:      # the scale is the slot's own: the same launch with every scale equal gives other bits for the slots that had another
        o2 = torch.full((n,), SENT, device=DEV)
        req2 = req.clone()
        req2[:, 1] = f32_bits(2.5)
        ops.slot_sched_bank(dv(x0), dv(x), o2, n, state, keys, clips, n_per_clip=npc, x0u=dv(x0u), x0_hist=dv(hist0.clone()), **shared,
                            **dict(bank, req=req2))
        assert torch.equal(o2[npc:2 * npc], got["f32"][npc:2 * npc]) and not torch.equal(o2[:npc], got["f32"][:npc])


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_op_slot_group_sched_bank_equals_slot_group_sched(mode, cfg):
    """The two forms of the group pass against each other, byte for byte: fdm_op_slot_group_sched_bank with a bank whose sampler 0
    holds exactly the tables and the scale given to fdm_op_slot_group_sched.  4 slots x 8 frames, d = 8: slot 0 plain and live,
    slot 1 idle (NaN rows), slots 3 and 2 -- in that order, the leader is not the lowest slot -- a group of two windows over
    L_total = 12 with overlap 4, inside a larger arena.  Every slot is at k = 1 of a 3-step sampler: the DDIM offsets are not zero,
    the DDPM step draws noise (t = 500) and the table-driven step reads its history (c[1] != 0) and draws noise (s[1] != 0).
    Compared: x_out, the operand copy in every kind, the arena, x0_hist and hist_long, and the rows neither may touch."""
    from test_slot_long_gpu import bits, group_tables
    slots, Lw, d, F, NE, first, e0 = 4, 8, 8, 16, 20, 2, 3
    npc, n = Lw * d, slots * Lw * d
    PLAIN, IDLE, GROUP, LT = 0, 1, [3, 2], 12
    (member, frames, ents, gdesc), starts = group_tables([(GROUP, LT, 4, first, e0)], slots, F, NE, L=Lw)
    assert [list(s) for s in starts] == [[0, 4]]
    g = torch.Generator().manual_seed(50 + mode)
    x0, x0u, hist_p, xs0 = [torch.randn(n, generator=g) * 2 for _ in range(4)]
    xs0[IDLE * npc:(IDLE + 1) * npc] = float("nan")
    xl0, hl0 = torch.randn(F * d, generator=g) * 2, torch.randn(F * d, generator=g) * 2
    tseq, san, cn = [999, 500, 0], [0.3, 0.6, 0.9], [0.95, 0.8, 0.43]
    lm = dict(lm_a=[0.9518, 0.853, 0.7313], lm_b=[0.3067, 0.3352, 0.5269], lm_c=[0.0, -0.013, -0.1491], lm_s=[0.25, 0.125, 0.4338])
    assert lm["lm_c"][1] != 0.0 and lm["lm_s"][1] != 0.0
    state = torch.tensor([[1, tseq[1], 1, 1], [0, 0, 0, 0], [1, tseq[1], 1, 1], [1, tseq[1], 1, 1]], dtype=torch.int32)
    keys = dv(torch.tensor([[99, 5], [77, 1], [1234, 3], [2 ** 40 + 5, 8]], dtype=torch.int64))      # the group's key is its leader's (slot 3)
    buf = schedule.make_buffers(1000)
    c1, c2, sg = schedule.ddpm_tables(buf)
    shared = dict(c1=dv(c1), c2=dv(c2), sigma=dv(sg), sra=dv(buf["sqrt_recip_alphas_cumprod"]), srm1=dv(buf["sqrt_recipm1_alphas_cumprod"]))
    own = {0: {}, 1: dict(sqrt_an=dv(torch.tensor(san)), c_n=dv(torch.tensor(cn))), 3: {k: dv(torch.tensor(v)) for k, v in lm.items()}}[mode]
    coef = {0: [], 1: san + cn, 3: lm["lm_a"] + lm["lm_b"] + lm["lm_c"] + lm["lm_s"]}[mode]
    bank = dict(req=dv(torch.tensor([[0, f32_bits(2.5), 0, 0]] * slots, dtype=torch.int32)),
                desc=dv(torch.tensor([[mode, 3, 0, 0]], dtype=torch.int32)), t=dv(torch.tensor(tseq, dtype=torch.int32)),
                coef=dv(torch.tensor(coef, dtype=torch.float32)))
    SENT = 7.5

    def copy_out(name):
        if name == "split":      # (plane distance 5 rows larger than n)
            return ops.Split(torch.full((2, n // d + 5, d), SENT, device=DEV, dtype=torch.float16), F16X3)
        return torch.full((n,), SENT, device=DEV, dtype={"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[name])

    def planes(t):
        return [t.planes[0].reshape(-1), t.planes[1].reshape(-1)] if isinstance(t, ops.Split) else [t]

    def run(name, with_bank):
        xs, xl, hl, hp, ot = dv(xs0.clone()), dv(xl0.clone()), dv(hl0.clone()), dv(hist_p.clone()), copy_out(name)
        common = dict(member=member, frames=frames, entries=ents, groups=gdesc, x_long=xl, hist_long=hl, L=Lw, d=d, n_per_clip=npc,
                      x0u=dv(x0u) if cfg else None, x_out_t=ot, x0_hist=hp)
        if with_bank:
            ops.slot_group_sched_bank(dv(x0), xs, xs, n, dv(state), keys, slots, **bank, **shared, **common)
        else:
            ops.slot_group_sched(mode, dv(x0), xs, xs, n, dv(state), keys, slots, cfg_scale=2.5, **shared, **own, **common)
        return [xs, xl, hl, hp] + planes(ot)

    def rows(t, s):
        return t[s * npc:(s + 1) * npc]

    for name in ("f32", "bf16", "f16", "split"):
        plain, banked = run(name, False), run(name, True)
        for i, (a, b) in enumerate(zip(plain, banked)):
            assert torch.equal(bits(a), bits(b)), (name, i)
        xs, xl, hl, hp, *ot = banked
        # both did the work: the plain slot, both member slots and the group's arena frames moved ...
        for s in [PLAIN] + GROUP:
            assert not torch.equal(rows(xs, s), dv(rows(xs0, s))), (name, s)
            for t in ot:
                assert not torch.equal(rows(t, s).float(), torch.full((npc,), SENT, device=DEV)), (name, s)
        a0, a1 = first * d, (first + LT) * d
        assert not torch.equal(xl[a0:a1], dv(xl0[a0:a1]))
        # ... the seam frames hold one value in both member slots (window starts 0 and 4: frames 4..7 of the long clip)
        assert torch.equal(rows(xs, GROUP[0])[4 * d:], rows(xs, GROUP[1])[:4 * d])
        assert torch.equal(rows(xs, GROUP[0])[4 * d:], xl[a0 + 4 * d:a0 + 8 * d])
        # ... and neither touched the idle slot (x keeps its NaN bits, the copy its sentinel), the free arena frames, or a history
        # that the mode does not write (mode 3: the plain slot's rows of x0_hist and the group's frames of hist_long only)
        assert torch.equal(bits(rows(xs, IDLE)), bits(dv(rows(xs0, IDLE))))
        for t in ot:
            assert torch.equal(rows(t, IDLE).float(), torch.full((npc,), SENT, device=DEV)), name
        for t, t0 in ((xl, xl0), (hl, hl0)):
            assert torch.equal(t[:a0], dv(t0[:a0])) and torch.equal(t[a1:], dv(t0[a1:])), name
        for s in range(slots):
            assert torch.equal(rows(hp, s), dv(rows(hist_p, s))) == (mode != 3 or s != PLAIN), (name, s)
        assert torch.equal(hl[a0:a1], dv(hl0[a0:a1])) == (mode != 3), name


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL_MODES)
def test_mixed_chains_equal_their_solo_chains(dtype):
    """DDIM 6 (sampler 0), DPM-Solver++ 2M and DDPM side by side, admitted at steps 0, 2 and 5."""
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    clips = [clip(preset, 33, 0), clip(preset, 31, 1), clip(preset, 7, 2)]
    names = ["ddim6", "2m", "ddpm"]
    refs = [solo(plan, preset, c, nm) for c, nm in zip(clips, names)]
    ids = open_bank(plan, 3, L, "ddim6", ["2m", "ddpm"])
    out = run_mixed(plan, [(at, s, c, ids[nm], STEPS[nm], None) for at, s, c, nm in zip((0, 2, 5), (0, 1, 2), clips, names)], [2, 3, 1])
    for c, r, nm in zip(clips, refs, names):
        assert torch.equal(out[id(c)], r), (c["L"], nm)


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_same_kind_different_lengths_and_a_frozen_slot(dtype):
    """DDIM 4, 6 and 9 in three slots, staggered: a wrong t_off / c_off / n_steps shows here.  The 4-step slot ends first and stays
    frozen bit for bit while the others go on."""
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    a, b, c = clip(preset, 31, 1), clip(preset, 33, 0), clip(preset, 7, 2)
    refs = [solo(plan, preset, a, "ddim4"), solo(plan, preset, b, "ddim9"), solo(plan, preset, c, "ddim6")]
    ids = open_bank(plan, 3, L, "ddim6", ["ddim4", "ddim9"])
    admit(plan, 0, a, ids["ddim4"])
    plan.run(1)
    admit(plan, 1, b, ids["ddim9"])
    plan.run(1)
    admit(plan, 2, c)                                        # the old admit: sampler 0
    plan.run(1)
    assert plan.slot_state(0) == (3, 3, SLOT_FINISHED) and plan.slot_state(1) == (2, 8, SLOT_RUNNING) and plan.slot_state(2) == (1, 5, SLOT_RUNNING)
    frozen = plan.peek_slot(0)
    plan.run(3)
    assert torch.equal(plan.peek_slot(0), frozen)
    plan.run(4)                                              # more than either needs
    assert plan.slot_state(1) == (8, 8, SLOT_FINISHED) and plan.slot_state(2) == (5, 5, SLOT_FINISHED)
    assert torch.equal(plan.peek_slot(0), frozen)
    got = [plan.read_slot(0, a["L"]), plan.read_slot(1, b["L"]), plan.read_slot(2, c["L"])]
    for g_, r in zip(got, refs):
        assert torch.equal(g_, r)
    assert not torch.equal(solo(plan, preset, a, "ddim6"), refs[0])


# 4 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_guidance_scale_per_request(dtype):
    preset, L = "mead_tiny", 8
    plan = plan_for(preset, dtype)
    a, b = clip(preset, 7, 0), clip(preset, 8, 1)
    ref_a, ref_b = solo(plan, preset, a, "ddpm", cfg=True, scale=1.7), solo(plan, preset, b, "2m", cfg=True, scale=3.0)
    ids = open_bank(plan, 3, L, "ddpm", ["2m"], cfg=True, cfg_scale=2.5)
    out = run_mixed(plan, [(0, 1, a, 0, 8, 1.7), (2, 0, b, ids["2m"], 5, 3.0), (2, 2, a, 0, 8, 3.0)], [2, 3, 1])
    assert torch.equal(out[id(b)], ref_b)
    # clip a ran twice on sampler 0: at 1.7 (slot 1, read first) and at 3.0 (slot 2, admitted later: it overwrites the entry)
    assert torch.equal(out[id(a)], solo(plan, preset, a, "ddpm", cfg=True, scale=3.0))
    assert not torch.equal(ref_a, solo(plan, preset, a, "ddpm", cfg=True, scale=3.0))
    # ... and alone at 1.7 beside the other request
    ids = open_bank(plan, 2, L, "ddpm", ["2m"], cfg=True, cfg_scale=2.5)
    out = run_mixed(plan, [(0, 1, a, 0, 8, 1.7), (2, 0, b, ids["2m"], 5, 3.0)], [2, 3, 1])
    assert torch.equal(out[id(a)], ref_a) and torch.equal(out[id(b)], ref_b)
    assert not torch.equal(out[id(a)], out[id(b)][:, :a["L"] * plan.p.G])


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bank_life_cycle(dtype):
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    a, b, c = clip(preset, 31, 1), clip(preset, 33, 0), clip(preset, 7, 2)
    ref_a2m, ref_b6, ref_c9 = solo(plan, preset, a, "2m"), solo(plan, preset, b, "ddim6"), solo(plan, preset, c, "ddim9")
    plan.open_slots(2, L, samplers=1, sampler_steps=8, **DEFS["ddim6"]())
    assert plan.sampler_info(0) == (1, 5)
    s2m = plan.add_sampler(**DEFS["2m"]())
    assert s2m == 1 and plan.sampler_info(1) == (2, 5)
    with pytest.raises(FdmError, match="-4"):                # a full bank: nothing changes
        plan.add_sampler(**DEFS["ddim4"]())
    assert plan.sampler_info(1) == (2, 5)
    for bad in (0, 2, -1):
        with pytest.raises(FdmError, match="-1"):
            plan.drop_sampler(bad)
    with pytest.raises(FdmError, match="-1"):                # an unknown sampler: nothing changes
        admit(plan, 0, a, sampler=2)
    assert plan.slot_state(0)[2] == 0
    admit(plan, 0, a, s2m)
    plan.run(2)
    with pytest.raises(FdmError, match="-4"):                # in use: running
        plan.drop_sampler(s2m)
    plan.run(3)
    with pytest.raises(FdmError, match="-4"):                # in use: finished and not read
        plan.drop_sampler(s2m)
    assert torch.equal(plan.read_slot(0, a["L"]), ref_a2m)
    plan.drop_sampler(s2m)
    with pytest.raises(FdmError, match="-1"):
        plan.sampler_info(s2m)
    # slot 1 mid-chain on sampler 0 while a new sampler goes into the freed range and slot 0 runs it (2M, then DDIM)
    admit(plan, 1, b)
    plan.run(2)
    s9 = plan.add_sampler(**DEFS["ddim9"]())
    assert s9 == 1 and plan.sampler_info(1) == (1, 8)
    admit(plan, 0, c, s9)
    plan.run(3)
    assert plan.slot_state(1) == (5, 5, SLOT_FINISHED) and plan.slot_state(0) == (3, 8, SLOT_RUNNING)
    assert torch.equal(plan.read_slot(1, b["L"]), ref_b6)
    plan.run(5)
    assert torch.equal(plan.read_slot(0, c["L"]), ref_c9)
    # ... and 2M again in the same slot: the history starts at zero
    plan.drop_sampler(s9)
    s2m = plan.add_sampler(**DEFS["2m"]())
    admit(plan, 0, a, s2m)
    plan.run(5)
    assert torch.equal(plan.read_slot(0, a["L"]), ref_a2m)


# 6 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_long_group_on_a_non_default_sampler(dtype):
    """75 frames as 3 windows of 40 (overlap 10) on DPM-Solver++ 2M, beside a plain clip on sampler 0 (DDIM 6) at another step."""
    preset, L, O = "vocaset_tiny", 40, 10
    plan = plan_for(preset, dtype)
    long, a = clip(preset, 75, 3), clip(preset, 33, 1)
    assert len(window_starts(75, L, O)) == 3
    ref_long, ref_a = solo(plan, preset, long, "2m", window=L, overlap=O), solo(plan, preset, a, "ddim6")
    plan.open_slots(4, L, long_frames=80, long_groups=1, samplers=1, sampler_steps=5, **DEFS["ddim6"]())
    s2m = plan.add_sampler(**DEFS["2m"]())
    admit(plan, 0, a)
    plan.run(2)
    plan.admit_long([3, 1, 2], long["hub"][0], long["style"][0], None, long["x"][0], L_total=75, overlap=O, seed=long["seed"],
                    clip_id=long["clip_id"], sampler=s2m)
    assert plan.slot_state(3) == (0, 5, SLOT_RUNNING) and plan.slot_state(0) == (2, 5, SLOT_RUNNING)
    plan.run(3)
    assert torch.equal(plan.read_slot(0, a["L"]), ref_a)
    plan.run(2)
    assert plan.slot_state(3) == (5, 5, SLOT_FINISHED)
    assert torch.equal(plan.read_long(3), ref_long)


# 7 ---------------------------------------------------------------------------------------------
def test_compatibility_with_the_plain_slot_program():
    preset, L, n_layers = "vocaset_tiny", 33, 2
    plan = plan_for(preset, BF16)
    a = clip(preset, 31, 1)
    outs, counts = [], []
    for cap in (0, 2):
        plan.open_slots(2, L, samplers=cap, sampler_steps=4 * cap, **DEFS["ddpm"]())
        assert plan.get("slot_samplers") == cap and plan.get("slot_sampler_steps") == 4 * cap
        plan.admit(1, a["hub"][0], a["style"][0], None, a["x"][0], L=a["L"], seed=a["seed"], clip_id=a["clip_id"])      # the old admit
        plan.run(8)
        counts.append(plan.get("launches_per_step"))
        outs.append(plan.read_slot(1, a["L"]))
        if not cap:
            with pytest.raises(FdmError, match="-4"):        # no bank: fails cleanly
                plan.add_sampler(**DEFS["ddim4"]())
            with pytest.raises(FdmError, match="-1"):
                admit(plan, 0, a, sampler=1)
            assert plan.sampler_info(0) == (0, 8)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], solo(plan, preset, a, "ddpm"))
    assert counts == [2 + 7 * n_layers + 2] * 2               # advance + chain (decoder unfused) + the slot pass, bank or not


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16X3])
def test_mixed_ddim_against_the_oracle(dtype):
    preset, L = "vocaset_tiny", 33
    plan = plan_for(preset, dtype)
    w = W.make_fdm_weights(preset)
    a, b = clip(preset, 31, 1), clip(preset, 7, 2)
    ids = open_bank(plan, 2, L, "ddim4", ["ddim9"])
    out = run_mixed(plan, [(0, 0, a, ids["ddim9"], 8, None), (2, 1, b, 0, 3, None)], [2, 3, 1])
    for c, steps in ((a, 9), (b, 4)):
        key = ("oracle", c["L"], steps)
        if key not in _REFS:
            den = lambda x, t, c=c: FO.fdm_forward(w, preset, c["hub"], t, x, c["style"], None, folded=True)
            _REFS[key] = FO.ddim_sample(den, c["x"].clone(), steps)
        err = float((out[id(c)].cpu().double() - _REFS[key].double()).abs().max())
        print(f"[slot samplers ddim {steps} dtype {dtype} L {c['L']}] vs the oracle {err:.2e}")
        assert err < TOL32


# 9 ---------------------------------------------------------------------------------------------
def test_pipeline_slot_server_with_a_sampler_per_request():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "dropin"))
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    g = torch.Generator().manual_seed(9)
    wavs = [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in (16000, 11000, 13500, 12000)]
    seeds = [4, 5, 6, 7]
    reqs = [dict(ddim_steps=6), dict(sampler="dpmpp2m", sampler_steps=5), dict(sampler="ddim_eta", eta=0.5, sampler_steps=6), dict(ddim_steps=4)]
    diffusion, ae = pipeline.build_models("vocaset", device=DEV)
    refs = [pipeline.animate(diffusion, ae, w, seed=s, device=DEV, **r) for w, s, r in zip(wavs, seeds, reqs)]
    plain = pipeline.SlotServer(diffusion, ae, slots=2, ddim_steps=6, device=DEV)
    with pytest.raises(ValueError):
        plain.submit(wavs[0], ddim_steps=4)
    srv = pipeline.SlotServer(diffusion, ae, slots=3, ddim_steps=9, device=DEV, samplers=2, bank_steps=16)
    hs = [srv.submit(w, seed=s, **r) for w, s, r in zip(wavs[:3], seeds[:3], reqs[:3])]
    assert len(srv._defs) == 3 and srv.pending == 3          # DDIM 9 (the server's) and two of the three requests' definitions ...
    assert len(srv._queue) == 1                              # ... the third waits: both bank rows are held by running slots
    srv.step(1)
    hs.append(srv.submit(wavs[3], seed=seeds[3], **reqs[3]))
    got = {h: (v, lat) for h, v, lat in srv.drain(2)}
    assert sorted(got) == sorted(hs) and srv.pending == 0
    assert ("ddim", 6) not in srv._defs or ("tables", "dpmpp2m", 5, 0.0) not in srv._defs       # a definition was evicted
    for h, r in zip(hs, refs):
        assert torch.equal(got[h][1], r[1]), h
        assert torch.equal(got[h][0], r[0]), h
