"""GPU: long requests in slot mode (include/fdm_hip.h, fdm_slot_admit_long): a recording longer than a slot rides the slot program
as a GROUP of slots, one window each, blended every step over a long arena.

The bar is bit identity (torch.equal): a group's latent is what sample_windows returns for the clip alone on a B = 1 windowed plan
(window = the slot capacity, the same overlap, x_T, seed, clip0 = clip_id), whatever the other slots hold and whenever it was
admitted; plain slots beside it keep their own guarantee.  The operator first (fdm_op_slot_group_sched against fdm_op_sched_step on
the torch blend and against fdm_op_slot_sched), then chains, two groups with reuse, seams, the oracle (1e-4, not through the solo
GPU path), noise keying, validation, launch counts and pipeline.SlotServer.submit_long.  8 slots of L = 40 on the tiny presets:
L_total = 100 with O = 10 is 3 windows with two-window overlaps, O = 30 is 7 windows with frames under three or more; L = 40 crosses
the period-30 positional table and one 32-key tile."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd import ops, schedule  # noqa: E402
from fdm_amd._lib import BF16, F16, F16X3, F32, SLOT_FINISHED, SLOT_IDLE, SLOT_RUNNING, FdmError, lib  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan, window_starts, window_weights  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402
from test_long_audio_cpu import windowed_denoiser  # noqa: E402

DEV = "cuda:0"
ALL_MODES = [F32, BF16, F16X3, F16]
SLOTS, L = 8, 40
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


def clip(preset, frames, i):
    """Clip i: its own audio features, one-hots, x_T, Philox seed and clip id."""
    if (preset, frames, i) not in _CLIPS:
        c = W.synth_inputs(preset, 1, frames, seed=70 + i)
        c.update(L=frames, seed=200 + 7 * i, clip_id=(3, 0, 7, 2)[i % 4])
        _CLIPS[(preset, frames, i)] = c
    return _CLIPS[(preset, frames, i)]


def sample_kw(sampler):
    kw = SAMPLERS[sampler]()
    return dict(kind=kw["kind"], steps=kw.get("steps"), t_list=kw.get("t_list"), tables=kw.get("tables"))


def solo(plan, preset, c, sampler, overlap=10, cfg=False, scale=2.5):
    """The clip alone: a long one on a B = 1 windowed plan (window = L), a short one on a (1, L_clip) plain plan."""
    key = (preset, plan.dtype, c["L"], c["seed"], sampler, overlap if c["L"] > L else None, cfg)
    if key not in _REFS:
        kw, x = SAMPLERS[sampler](), dv(c["x"])
        if c["L"] > L:
            plan.prepare_windows(c["hub"], c["style"], c.get("emo"), L_total=c["L"], window=L, overlap=overlap, cfg=cfg)
            out = plan.sample_windows(x, seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale, **sample_kw(sampler))
        else:
            plan.prepare(c["hub"], c["style"], c.get("emo"), L=c["L"], cfg=cfg)
            if sampler == "ddim":
                out = plan.sample_ddim(x, kw["steps"], cfg_scale=scale)
            elif sampler == "ddpm":
                out = plan.sample_ddpm(x, kw["t_list"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
            else:
                out = plan.sample_tables(x, kw["t_list"], kw["tables"], seed=c["seed"], clip0=c["clip_id"], cfg_scale=scale)
        _REFS[key] = out.clone()
    return _REFS[key]


def admit(plan, slots, c, overlap=10):
    emo = c["emo"][0] if c.get("emo") is not None else None
    if c["L"] > L:
        plan.admit_long(slots, c["hub"][0], c["style"][0], emo, c["x"][0], L_total=c["L"], overlap=overlap, seed=c["seed"], clip_id=c["clip_id"])
    else:
        plan.admit(slots[0], c["hub"][0], c["style"][0], emo, c["x"][0], L=c["L"], seed=c["seed"], clip_id=c["clip_id"])


def drive(plan, admits, pieces, overlap=10):
    """admits: [(at_step, slots, clip)]; pieces: run() sizes, cycled until every admitted clip has been read.  A clip (or group) is
    admitted at the first piece boundary at or after at_step.  Returns {id(clip): latent}."""
    todo, where, out, done, i = sorted(admits, key=lambda a: a[0]), {}, {}, 0, 0
    while todo or where:
        while todo and todo[0][0] <= done:
            _, slots, c = todo.pop(0)
            admit(plan, slots, c, overlap)
            where[slots[0]] = c
        n = pieces[i % len(pieces)]
        plan.run(n)
        done, i = done + n, i + 1
        for lead in list(where):
            if plan.slot_state(lead)[2] == SLOT_FINISHED:
                c = where.pop(lead)
                out[id(c)] = plan.read_long(lead) if c["L"] > L else plan.read_slot(lead, c["L"])
        assert i < 64
    return out


# 1 ---------------------------------------------------------------------------------------------
def group_tables(groups, n_slots, F, n_entries, L=L):
    """groups: [(slots, L_total, overlap, first arena frame, first entry)] -> device tables of fdm_slot_group_args (+ the starts);
    L = frames per slot."""
    member = np.full(n_slots, -1, np.int32)
    frames = np.full((F, 4), -1, np.int32)
    ents = np.zeros((n_entries, 4), np.int32)
    desc = np.zeros((len(groups), 4), np.int32)
    starts = []
    for gi, (slots, Lt, O, first, e0) in enumerate(groups):
        ids = (C.c_int * len(slots))(*slots)
        ne = len(slots) * L
        off, es, est, ew = np.zeros(Lt + 1, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.int32), np.zeros(ne, np.float32)
        assert lib().fdm_slot_group_table_host(Lt, L, O, ids, len(slots), off.ctypes.data, es.ctypes.data, est.ctypes.data, ew.ctypes.data, ne) == ne
        frames[first:first + Lt, 0], frames[first:first + Lt, 1], frames[first:first + Lt, 2], frames[first:first + Lt, 3] = gi, e0 + off[:-1], e0 + off[1:], 0
        ents[e0:e0 + ne, 0], ents[e0:e0 + ne, 1], ents[e0:e0 + ne, 2] = es, est, ew.view(np.int32)
        desc[gi] = (slots[0], Lt, first, 0)
        member[list(slots)] = gi
        starts.append(window_starts(Lt, L, O))
        assert len(starts[-1]) == len(slots)
    return [dv(torch.from_numpy(a)) for a in (member, frames, ents, desc)], starts


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


@pytest.mark.parametrize("cfg", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 3])
def test_op_slot_group_sched(mode, cfg):
    """Two groups (L_total 100 and 75, shuffled member slots, apart in the arena), a plain live slot and an idle slot full of NaN.
    Group rows: fdm_op_sched_step on the torch blend of the windows' (CFG-mixed) x0, the clip alone; plain slot: fdm_op_slot_sched."""
    d, F, NE = 64, 190, 256
    npc, n = L * d, SLOTS * L * d
    GROUPS = [([5, 1, 6], 100, 10, 4, 0), ([0, 7, 3], 75, 10, 110, 130)]
    PLAIN, IDLE = 2, 4
    (member, frames, ents, desc), starts = group_tables(GROUPS, SLOTS, F, NE)
    g = torch.Generator().manual_seed(40 + mode)
    x0, x0u, hist_p = [torch.randn(n, generator=g) * 2 for _ in range(3)]
    xs0 = torch.randn(n, generator=g) * 2
    xs0[IDLE * npc:(IDLE + 1) * npc] = float("nan")
    xl0, hl0 = torch.randn(F * d, generator=g) * 2, torch.randn(F * d, generator=g) * 2
    tseq = torch.tensor([999, 500, 0], dtype=torch.int32)
    word = {0: [0, 999, 1, 1], 1: [2, 0, 1, 1], "plain": [1, 500, 1, 1]}           # group 0 at k = 0, group 1 at the last step (t = 0)
    state = torch.zeros(SLOTS, 4, dtype=torch.int32)
    seeds, ids = [1234, 2 ** 40 + 5], [3, 8]
    keys = torch.zeros(SLOTS, 2, dtype=torch.int64)
    for gi, (slots, *_r) in enumerate(GROUPS):
        for s in slots:
            state[s] = torch.tensor(word[gi])
            keys[s] = torch.tensor([seeds[gi], ids[gi]])
    state[PLAIN], keys[PLAIN] = torch.tensor(word["plain"]), torch.tensor([99, 5])
    keys[IDLE] = torch.tensor([77, 1])
    buf = schedule.make_buffers(1000)
    c1, c2, sg = schedule.ddpm_tables(buf)
    if mode == 0:
        tabs = dict(c1=dv(c1), c2=dv(c2), sigma=dv(sg))
    elif mode == 1:
        tabs = dict(sra=dv(buf["sqrt_recip_alphas_cumprod"]), srm1=dv(buf["sqrt_recipm1_alphas_cumprod"]),
                    sqrt_an=dv(torch.tensor([0.3, 0.6, 0.9])), c_n=dv(torch.tensor([0.95, 0.8, 0.43])))
    else:
        tabs = dict(lm_a=dv(torch.tensor([0.9518, 0.853, 0.7313])), lm_b=dv(torch.tensor([0.3067, 0.3352, 0.5269])),
                    lm_c=dv(torch.tensor([0.0, -0.013, -0.1491])), lm_s=dv(torch.tensor([0.25, 0.0, 0.4338])))
    SENT = 7.5

    def copy_out(name, count, rows_extra=0):
        if name == "f32":
            return torch.full((count,), SENT, device=DEV)
        if name == "split":
            return ops.Split(torch.full((2, count // d + rows_extra, d), SENT, device=DEV, dtype=torch.float16), F16X3)
        return torch.full((count,), SENT, device=DEV, dtype=torch.bfloat16 if name == "bf16" else torch.float16)

    def planes(t):
        return [t.planes[0].reshape(-1), t.planes[1].reshape(-1)] if isinstance(t, ops.Split) else [t]

    def blended(gi):
        """torch, fp32, separate ops (no contraction): each window's CFG mix, then the weighted sum in ascending window order with
        fdm_window_weights_host's weights (tests/test_slot_long_cpu.py: the group table holds their bits)."""
        slots, Lt, O, first, e0 = GROUPS[gi]
        wts = window_weights(Lt, L, O)
        acc = torch.zeros(Lt, d)
        seen = torch.zeros(Lt, dtype=torch.bool)
        for w, (s, st) in enumerate(zip(slots, starts[gi])):
            rows = slice(s * npc, (s + 1) * npc)
            v = x0[rows].reshape(L, d)
            if cfg:
                u = x0u[rows].reshape(L, d)
                v = u + 2.5 * (v - u)
            term = wts[w].view(L, 1) * v
            fresh = ~seen[st:st + L]
            acc[st:st + L] = torch.where(fresh.view(L, 1), term, acc[st:st + L] + term)
            seen[st:st + L] = True
        assert bool(seen.all())
        return acc.reshape(-1)

    def reference(gi, name):
        slots, Lt, O, first, e0 = GROUPS[gi]
        nl = Lt * d
        step = torch.tensor([word[gi][0]], dtype=torch.int32, device=DEV)
        o, ot = torch.zeros(nl, device=DEV), copy_out(name, nl)
        hist = dv(hl0[first * d:first * d + nl].clone())
        ops.sched_step(mode, dv(blended(gi)), dv(xl0[first * d:first * d + nl].clone()), o, nl, n_per_clip=nl, tseq=dv(tseq), step=step,
                       seed=seeds[gi], clip0=ids[gi], x_out_t=ot, x0_hist=hist if mode == 3 else None, **tabs)
        return o, ot, hist

    def run(name, st):
        xs, xl, hl, hp = dv(xs0.clone()), dv(xl0.clone()), dv(hl0.clone()), dv(hist_p.clone())
        ot = copy_out(name, n, rows_extra=5)                      # (the split copy's plane distance is 5 rows larger than n)
        ops.slot_group_sched(mode, dv(x0), xs, xs, n, dv(st), dv(keys), SLOTS, member=member, frames=frames, entries=ents, groups=desc,
                             x_long=xl, hist_long=hl if mode == 3 else None, L=L, d=d, n_per_clip=npc, x0u=dv(x0u) if cfg else None,
                             cfg_scale=2.5, x_out_t=ot, x0_hist=hp if mode == 3 else None, **tabs)
        return xs, xl, hl, hp, ot

    def slot_rows(t, s):
        return t[s * npc:(s + 1) * npc]

    for name in ("f32", "bf16", "f16", "split"):
        xs, xl, hl, hp, ot = run(name, state)
        for gi, (slots, Lt, O, first, e0) in enumerate(GROUPS):
            ro, rot, rh = reference(gi, name)
            a0, nl = first * d, Lt * d
            assert torch.equal(xl[a0:a0 + nl], ro), (name, gi)
            if mode == 3:
                assert torch.equal(hl[a0:a0 + nl], rh), (name, gi)
            for s, st in zip(slots, starts[gi]):
                assert torch.equal(slot_rows(xs, s), ro[st * d:(st + L) * d]), (name, gi, s)
                for got, want in zip(planes(ot), planes(rot)):
                    assert torch.equal(slot_rows(got, s), want[st * d:(st + L) * d]), (name, gi, s)
        # free arena frames: untouched
        for a, b in ((0, 4), (104, 110), (185, 190)):
            assert torch.equal(bits(xl[a * d:b * d]), bits(dv(xl0[a * d:b * d]))) and torch.equal(bits(hl[a * d:b * d]), bits(dv(hl0[a * d:b * d])))
        # the plain slot: fdm_op_slot_sched's bits (x, operand copy, history)
        pxs, php, pot = dv(xs0.clone()), dv(hist_p.clone()), copy_out(name, n, rows_extra=5)
        ops.slot_sched(mode, dv(x0), pxs, pxs, n, dv(state), dv(keys), SLOTS, n_per_clip=npc, x0u=dv(x0u) if cfg else None, cfg_scale=2.5,
                       x_out_t=pot, x0_hist=php if mode == 3 else None, **tabs)
        assert torch.equal(slot_rows(xs, PLAIN), slot_rows(pxs, PLAIN)) and not torch.equal(slot_rows(xs, PLAIN), dv(slot_rows(xs0, PLAIN)))
        for got, want in zip(planes(ot), planes(pot)):
            assert torch.equal(slot_rows(got, PLAIN), slot_rows(want, PLAIN)), name
        if mode == 3:
            assert torch.equal(slot_rows(hp, PLAIN), slot_rows(php, PLAIN))
            for s in range(SLOTS):                               # member slots never touch the plain history
                if s != PLAIN:
                    assert torch.equal(slot_rows(hp, s), dv(slot_rows(hist_p, s))), s
        # the idle slot: its NaN rows keep their bits, its operand copy keeps the sentinel
        assert torch.equal(bits(slot_rows(xs, IDLE)), bits(dv(slot_rows(xs0, IDLE))))
        for got in planes(ot):
            assert torch.equal(slot_rows(got, IDLE).float(), torch.full((npc,), SENT, device=DEV)), name
    # a group that is not live is skipped whole -- also when its members' own words say live (only the leader's word counts) --
    # and a member slot is never updated as a plain slot
    st2 = state.clone()
    st2[GROUPS[1][0][0], 2] = 0
    xs, xl, hl, hp, ot = run("f32", st2)
    slots, Lt, O, first, e0 = GROUPS[1]
    assert torch.equal(xl[first * d:(first + Lt) * d], dv(xl0[first * d:(first + Lt) * d]))
    assert torch.equal(hl[first * d:(first + Lt) * d], dv(hl0[first * d:(first + Lt) * d]))
    for s in slots:
        assert torch.equal(slot_rows(xs, s), dv(slot_rows(xs0, s))) and torch.equal(slot_rows(ot, s), torch.full((npc,), SENT, device=DEV)), s
    ro, _, _ = reference(0, "f32")
    assert torch.equal(xl[4 * d:104 * d], ro)                    # the live group beside it is unaffected
    # init form: the arena goes into the window rows (+ copy), nothing else moves and the state is not looked at
    xs, xl = dv(xs0.clone()), dv(xl0.clone())
    ot = copy_out("bf16", n)
    ops.slot_group_sched(2, None, None, xs, n, dv(torch.zeros_like(state)), dv(keys), SLOTS, member=member, frames=frames, entries=ents,
                         groups=desc, x_long=xl, L=L, d=d, n_per_clip=npc, x_out_t=ot, frame0=4, frame1=104, plain=0, init=1)
    assert torch.equal(xl, dv(xl0))
    for s, st in zip(GROUPS[0][0], starts[0]):
        want = dv(xl0[(4 + st) * d:(4 + st + L) * d])
        assert torch.equal(slot_rows(xs, s), want) and torch.equal(slot_rows(ot, s), ops.to_operand(want.contiguous(), BF16)), s
    for s in GROUPS[1][0] + [PLAIN]:
        assert torch.equal(slot_rows(xs, s), dv(slot_rows(xs0, s))), s


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
@pytest.mark.parametrize("dtype", ALL_MODES)
def test_group_beside_plain_clips_equals_the_solo_runs(dtype, sampler):
    """A 100-frame recording (7 windows at O = 30: frames under three and more windows) admitted at step 3 into shuffled slots,
    beside a plain clip of 33 frames admitted at step 0; a clip of 31 frames takes that slot when it has been read, while the
    group is mid-chain or just finished (the eighth slot is the only one outside the group)."""
    preset, O = "vocaset_tiny", 30
    plan = plan_for(preset, dtype)
    long, a, b = clip(preset, 100, 0), clip(preset, 33, 1), clip(preset, 31, 2)
    refs = [solo(plan, preset, c, sampler, overlap=O) for c in (long, a, b)]
    n = plan.open_slots(SLOTS, L, long_frames=120, long_groups=2, **SAMPLERS[sampler]())
    assert plan.get("slots") == SLOTS and plan.get("slot_long_frames") == 120 and plan.get("slot_long_groups") == 2
    members = [6, 2, 7, 0, 5, 3, 4]
    assert len(window_starts(100, L, O)) == 7
    # (slot 1 is the only slot outside the group: clip b follows clip a into it once a has been read)
    out = drive(plan, [(0, [1], a), (3, members, long), (max(5, n), [1], b)], [3, 2, 1, 3], overlap=O)
    for c, r in zip((long, a, b), refs):
        assert torch.equal(out[id(c)], r), (c["L"], sampler)
    assert refs[0].shape == (1, 100 * plan.p.G, plan.p.c)


@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
@pytest.mark.parametrize("dtype", ALL_MODES)
def test_group_of_three_windows_between_two_plain_clips(dtype, sampler):
    """O = 10: 3 windows, two-window overlaps; the plain clips run at other steps of their chains in other slots all the while."""
    preset = "vocaset_tiny"
    plan = plan_for(preset, dtype)
    long, a, b = clip(preset, 100, 0), clip(preset, 33, 1), clip(preset, 31, 2)
    refs = [solo(plan, preset, c, sampler) for c in (long, a, b)]
    plan.open_slots(SLOTS, L, long_frames=100, long_groups=1, **SAMPLERS[sampler]())
    out = drive(plan, [(0, [4], a), (3, [7, 0, 2], long), (5, [1], b)], [3, 2, 1, 3])
    for c, r in zip((long, a, b), refs):
        assert torch.equal(out[id(c)], r), (c["L"], sampler)
    assert plan.slot_state(7) == (0, plan.slot_state(0)[1], SLOT_IDLE) and plan.slot_group(7) == (-1, 0, 0)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_group_with_guidance_mead(dtype):
    preset = "mead_tiny"
    plan = plan_for(preset, dtype)
    long, a = clip(preset, 100, 0), clip(preset, 33, 1)
    for sampler in ("ddim", "ddpm"):
        refs = [solo(plan, preset, c, sampler, cfg=True, scale=1.7) for c in (long, a)]
        plan.open_slots(SLOTS, L, cfg=True, cfg_scale=1.7, long_frames=100, long_groups=1, **SAMPLERS[sampler]())
        out = drive(plan, [(0, [3], a), (2, [5, 1, 6], long)], [2, 3, 1])
        for c, r in zip((long, a), refs):
            assert torch.equal(out[id(c)], r), (c["L"], sampler)


# 3 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddpm", "2m"])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_two_groups_at_once_and_reuse(dtype, sampler):
    """L_total 100 and 75 side by side, admitted at different steps; when the first has been read a third long request takes its
    slots, its arena range and its descriptor while the second is mid-chain."""
    preset = "vocaset_tiny"
    plan = plan_for(preset, dtype)
    a, b, c = clip(preset, 100, 0), clip(preset, 75, 3), clip(preset, 90, 4)
    refs = [solo(plan, preset, k, sampler) for k in (a, b, c)]
    n = plan.open_slots(SLOTS, L, long_frames=180, long_groups=2, **SAMPLERS[sampler]())
    sa, sb = [2, 6, 0], [7, 1, 4]
    admit(plan, sa, a)
    plan.run(2)
    admit(plan, sb, b)
    assert plan.slot_group(6) == (2, 3, 100) and plan.slot_group(4) == (7, 3, 75) and plan.slot_group(3) == (-1, 0, 0)
    with pytest.raises(FdmError, match="-4"):                # no descriptor, no arena range: wait
        admit(plan, [3, 5, 2], c)
    plan.run(n - 2)
    assert plan.slot_state(0) == (n, n, SLOT_FINISHED) and plan.slot_state(1) == (n - 2, n, SLOT_RUNNING)
    with pytest.raises(FdmError, match="-4"):                # slot 0 is finished and not read
        admit(plan, [0, 3, 5], c)
    got_a = plan.read_long(2)
    assert plan.slot_group(2) == (-1, 0, 0) and plan.slot_state(6)[2] == SLOT_IDLE
    admit(plan, [0, 2, 6], c)                                # group b has 2 steps to go
    plan.run(2)
    got_b = plan.read_long(7)
    plan.run(n)                                              # more than c needs: it freezes at its end
    got_c = plan.read_long(0)
    for got, r in zip((got_a, got_b, got_c), refs):
        assert torch.equal(got, r)


# 4 ---------------------------------------------------------------------------------------------
def test_seams_are_bitwise_equal_across_member_slots():
    preset, O = "vocaset_tiny", 30
    plan = plan_for(preset, BF16)
    long = clip(preset, 100, 0)
    plan.open_slots(SLOTS, L, long_frames=100, long_groups=1, **SAMPLERS["ddpm"]())
    members = [6, 2, 7, 0, 5, 3, 4]
    admit(plan, members, long, overlap=O)
    starts = window_starts(100, L, O)

    def check():
        rows = [plan.peek_slot(s).reshape(L, -1) for s in members]
        for i in range(len(starts)):
            for j in range(i + 1, len(starts)):
                ov = starts[i] + L - starts[j]
                if ov > 0:
                    assert torch.equal(rows[i][L - ov:], rows[j][:ov]), (i, j)
        return rows
    before = check()                                         # x_T scattered by the init form
    assert torch.equal(before[0], dv(long["x"]).reshape(100, -1)[:L])
    plan.run(2)
    after = check()
    assert not torch.equal(after[0], before[0])


# 5 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16X3])
def test_group_against_the_windowed_oracle(dtype):
    preset = "vocaset_tiny"
    plan = plan_for(preset, dtype)
    w = W.make_fdm_weights(preset)
    long, a = clip(preset, 100, 0), clip(preset, 33, 1)
    plan.open_slots(SLOTS, L, long_frames=100, long_groups=1, **SAMPLERS["ddim"]())
    out = drive(plan, [(0, [3], a), (2, [5, 1, 6], long)], [2, 3, 1])
    if "oracle" not in _REFS:
        _REFS["oracle"] = FO.ddim_sample(windowed_denoiser(w, preset, long["hub"], long["style"], None, 100, L, 10), long["x"].clone(), 6)
    err = float((out[id(long)].cpu().double() - _REFS["oracle"].double()).abs().max())
    print(f"[slot group ddim dtype {dtype}] vs the windowed oracle {err:.2e}")
    assert err <= 1e-4


# 6 ---------------------------------------------------------------------------------------------
def test_group_noise_is_keyed_by_the_long_clip():
    """c1 = c2 = 0, sigma = 1: one DDPM step returns its noise draw z.  One step of a group equals the plain sampler's draw for the
    same (seed, clip_id) on an L_total-frame clip: one draw per long-clip element, whatever its place in the arena."""
    preset = "vocaset_tiny"
    plan = DenoiserPlan(preset, W.make_fdm_weights(preset), F32, DEV)
    for name, v in (("sched.c1", 0.0), ("sched.c2", 0.0), ("sched.sigma", 1.0)):
        t = torch.full((1000,), v)
        assert lib().fdm_plan_set_weights(plan.h, name.encode(), t.data_ptr(), 1000, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    long, other = clip(preset, 100, 0), clip(preset, 75, 3)
    plan.prepare(long["hub"], long["style"], L=100)
    z = plan.sample_ddpm(dv(long["x"]), [500], seed=11, clip0=3)
    assert float(z.std()) > 0.5
    plan.open_slots(SLOTS, L, kind="ddpm", t_list=[500], long_frames=180, long_groups=2)
    admit(plan, [7, 1, 4], other)                            # takes the arena's first 75 frames: the group under test starts at 75
    plan.admit_long([2, 6, 0], long["hub"][0], long["style"][0], None, long["x"][0], L_total=100, overlap=10, seed=11, clip_id=3)
    plan.run(1)
    assert torch.equal(plan.read_long(2), z)


# 7 ---------------------------------------------------------------------------------------------
def test_validation_and_state():
    preset = "vocaset_tiny"
    fresh = DenoiserPlan(preset, W.make_fdm_weights(preset), F32, DEV)
    long, a, short = clip(preset, 100, 0), clip(preset, 33, 1), clip(preset, 31, 2)
    for call in (lambda: admit(fresh, [0, 1, 2], long), lambda: fresh.read_long(0), lambda: fresh.slot_group(0)):
        with pytest.raises(FdmError, match="-4"):            # not in slot mode
            call()
    assert fresh.get("slot_long_frames") == 0 and fresh.get("slot_long_groups") == 0
    plan = plan_for(preset, F32)
    plan.open_slots(SLOTS, L, **SAMPLERS["ddim"]())         # no long capacity
    with pytest.raises(FdmError, match="-1"):
        admit(plan, [0, 1, 2], long)
    n = plan.open_slots(SLOTS, L, long_frames=150, long_groups=2, **SAMPLERS["ddim"]())
    admit(plan, [4], a)
    before = [plan.peek_slot(s) for s in range(SLOTS)]
    with pytest.raises(FdmError, match="-2"):                # wrong n
        admit(plan, [0, 1], long)
    with pytest.raises(FdmError, match="-2"):
        admit(plan, [0, 1, 2, 3], long)
    with pytest.raises(FdmError, match="-4"):                # a busy slot
        admit(plan, [0, 4, 2], long)
    with pytest.raises(FdmError, match="-1"):                # a duplicate
        admit(plan, [0, 2, 2], long)
    with pytest.raises(FdmError, match="-1"):                # outside [0, B)
        admit(plan, [0, 2, SLOTS], long)
    with pytest.raises(FdmError, match="-2"):                # L_total <= L: one window, fdm_slot_admit's business
        plan.admit_long([0], short["hub"][0], short["style"][0], None, short["x"][0], L_total=31, overlap=10)
    with pytest.raises(FdmError, match="-2"):                # more frames than the features hold
        plan.admit_long([0, 1, 2], long["hub"][0, :90], long["style"][0], None, long["x"][0], L_total=100, overlap=10)
    with pytest.raises(FdmError, match="-1"):                # overlap >= L
        plan.admit_long([0, 1, 2], long["hub"][0], long["style"][0], None, long["x"][0], L_total=100, overlap=L)
    admit(plan, [0, 1, 2], long)
    with pytest.raises(FdmError, match="-4"):                # arena full (150 frames, 100 taken): wait -- and the plan is unchanged
        admit(plan, [3, 5, 6], clip(preset, 75, 3))
    assert [plan.slot_state(s)[2] for s in range(SLOTS)] == [SLOT_RUNNING] * 3 + [SLOT_IDLE, SLOT_RUNNING] + [SLOT_IDLE] * 3
    assert plan.slot_group(5) == (-1, 0, 0) and plan.slot_group(1) == (0, 3, 100)
    for s in (3, 5, 6, 7):
        assert torch.equal(plan.peek_slot(s), before[s]) and not plan.peek_slot(s).any(), s
    assert torch.equal(plan.peek_slot(4), before[4])
    plan.run(2)
    assert plan.slot_state(1) == (2, n, SLOT_RUNNING) and plan.slot_state(2) == plan.slot_state(0)
    with pytest.raises(FdmError, match="-4"):                # read_long before the group finishes
        plan.read_long(0)
    plan.run(n)
    with pytest.raises(FdmError, match="-4"):                # read_slot on a member
        plan.read_slot(1, L)
    with pytest.raises(FdmError, match="-4"):                # read_long on a member that does not lead, and on a plain slot
        plan.read_long(1)
    with pytest.raises(FdmError, match="-4"):
        plan.read_long(4)
    assert plan.read_long(0).shape == (1, 100 * plan.p.G, plan.p.c)
    with pytest.raises(FdmError, match="-4"):                # a second read
        plan.read_long(0)
    assert torch.equal(plan.read_slot(4, a["L"]), solo(fresh, preset, a, "ddim"))
    # an fdm_audio_prepare call ends slot mode cleanly, and the next session starts empty
    plan.open_slots(SLOTS, L, long_frames=150, long_groups=2, **SAMPLERS["ddim"]())
    admit(plan, [0, 1, 2], long)
    plan.prepare(a["hub"], a["style"], L=a["L"])
    assert plan.get("slots") == 0
    with pytest.raises(FdmError, match="-4"):
        plan.read_long(0)
    assert torch.equal(plan.sample_ddim(dv(a["x"]), 6), solo(fresh, preset, a, "ddim"))
    plan.open_slots(SLOTS, L, long_frames=150, long_groups=2, **SAMPLERS["ddim"]())
    assert plan.slot_group(0) == (-1, 0, 0) and plan.slot_state(0)[2] == SLOT_IDLE


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "ddpm", "2m"])
def test_launch_counts_and_graph_modes(sampler):
    preset, n_layers = "vocaset_tiny", 2
    plan = plan_for(preset, BF16)
    long, a = clip(preset, 100, 0), clip(preset, 33, 1)
    plan.open_slots(SLOTS, L, **SAMPLERS[sampler]())
    admit(plan, [0], a)
    plan.run(1)
    assert plan.get("launches_per_step") == 2 + 7 * n_layers + 2        # no long capacity: today's program
    outs = []
    for kw in (dict(), dict(use_graph=False), dict(graph_steps=1)):
        plan.open_slots(SLOTS, L, long_frames=100, long_groups=1, **kw, **SAMPLERS[sampler]())
        outs.append(drive(plan, [(0, [3], a), (2, [5, 1, 6], long)], [2, 3, 1]))
        # with capacity: the group update rides the slot scheduler pass -- the same count
        assert plan.get("launches_per_step") == 2 + 7 * n_layers + 2
    for o in outs[1:]:
        assert torch.equal(o[id(long)], outs[0][id(long)]) and torch.equal(o[id(a)], outs[0][id(a)])
    assert torch.equal(outs[0][id(long)], solo(plan, preset, long, sampler))


# 9 ---------------------------------------------------------------------------------------------
def test_pipeline_submit_long_equals_animate_long():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "dropin"))
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    # (the VQ stage fixes G * c = 1024, so the pipeline has no tiny preset: the full VOCASET geometry, slots of 40 frames)
    g = torch.Generator().manual_seed(19)
    wavs = [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in (32400, 9000, 11000, 12000)]
    seeds = [4, 5, 6, 7]
    diffusion, ae = pipeline.build_models("vocaset", device=DEV)
    ref_long = pipeline.animate_long(diffusion, ae, wavs[0], ddim_steps=4, seed=seeds[0], window=40, overlap=10, device=DEV)
    ref_one = pipeline.animate_long(diffusion, ae, wavs[3], ddim_steps=4, seed=seeds[3], window=40, overlap=10, device=DEV)
    refs = [pipeline.animate(diffusion, ae, w, ddim_steps=4, seed=s, device=DEV) for w, s in zip(wavs[1:3], seeds[1:3])]
    L_total = ref_long[1].shape[1] // 16
    assert 95 <= L_total <= 105 and ref_one[1].shape[1] // 16 <= 40
    srv = pipeline.SlotServer(diffusion, ae, slots=4, max_frames=40, ddim_steps=4, device=DEV, long_frames=120, long_groups=1, overlap=10)
    h1 = srv.submit(wavs[1], seed=seeds[1])
    srv.step(1)
    h0 = srv.submit_long(wavs[0], seed=seeds[0])             # 3 windows into the 3 idle slots, beside a clip at step 1
    h2 = srv.submit(wavs[2], seed=seeds[2])                  # waits
    h3 = srv.submit_long(wavs[3], seed=seeds[3])             # fits a slot: an ordinary request, behind h2
    assert srv.pending == 4 and [r["handle"] for r in srv._queue] == [h2, h3]
    with pytest.raises(ValueError):
        srv.submit_long(np.concatenate([wavs[0], wavs[0]]), seed=1)      # ~200 frames: more than the arena holds
    got = {h: (v, lat) for h, v, lat in srv.drain(1)}
    assert sorted(got) == [h1, h0, h2, h3] and srv.pending == 0
    for h, r in ((h0, ref_long), (h3, ref_one), (h1, refs[0]), (h2, refs[1])):
        assert torch.equal(got[h][1], r[1]), h
        assert torch.equal(got[h][0], r[0]), h
