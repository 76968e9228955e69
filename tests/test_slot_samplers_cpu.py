"""CPU: samplers per request in slot mode (include/fdm_hip.h, fdm_slot_sampler_add / fdm_slot_admit_as) -- the exported symbols and
their bindings, the new struct's size, the pinned version, the argument errors that need no device, the host validation of the two
bank operators (recorded, never launched here), and the policy of pipeline.SlotServer with the plan stubbed: how a request's sampler
is resolved, what is refused at submit, the {definition: id} map, least-recently-used eviction and the wait at the head of the queue."""
import ctypes as C
import types

import pytest
import torch

from fdm_amd import _lib, pipeline, presets
from fdm_amd._lib import FdmError, SampleArgs, SchedArgs, SlotBankArgs, SlotGroupArgs

ERR_ARG, ERR_SHAPE, ERR_STATE = -1, -2, -4
NEW_SYMBOLS = ["fdm_slot_sampler_add", "fdm_slot_sampler_drop", "fdm_slot_sampler_info", "fdm_slot_admit_as", "fdm_slot_admit_long_as",
               "fdm_op_slot_sched_bank", "fdm_op_slot_group_sched_bank"]


def test_new_symbols_are_exported_and_bound_and_the_version_is_pinned():
    l = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(l, n) and n in _lib.SYMBOLS, n
    assert l.fdm_abi_struct_size(b"fdm_slot_bank_args") == C.sizeof(SlotBankArgs) == 48
    assert _lib.STRUCTS["fdm_slot_bank_args"] is SlotBankArgs
    assert l.fdm_version() == _lib.LIB_VERSION == 105
    # the existing public structs keep their layout
    assert C.sizeof(SchedArgs) == l.fdm_abi_struct_size(b"fdm_sched_args") and C.sizeof(SampleArgs) == l.fdm_abi_struct_size(b"fdm_sample_args")


def test_null_plan_and_null_args_are_argument_errors():
    l = _lib.lib()
    a = SampleArgs()
    a.kind, a.ddim_steps = 1, 6
    assert l.fdm_slot_sampler_add(None, C.byref(a), None) == ERR_ARG and b"null plan" in l.fdm_last_error()
    assert l.fdm_slot_sampler_add(None, None, None) == ERR_ARG and b"null sampler" in l.fdm_last_error()
    assert l.fdm_slot_sampler_drop(None, 1) == ERR_ARG
    assert l.fdm_slot_admit_as(None, 0, 16, 10, 1024, 16, None, 5, 16, 0, 0, 1, 2.5, None) == ERR_ARG
    ids = (C.c_int * 3)(0, 1, 2)
    assert l.fdm_slot_admit_long_as(None, ids, 3, 16, 100, 1024, 16, None, 100, 10, 16, 0, 0, 1, 2.5, None) == ERR_ARG
    assert l.fdm_op_slot_sched_bank(None, None, None, 1, None, None) == ERR_ARG
    assert l.fdm_op_slot_group_sched_bank(None, None, None, 1, None, None, None) == ERR_ARG
    sa, g, b = SchedArgs(), SlotGroupArgs(), SlotBankArgs()
    sa.x0 = sa.x = sa.x_out = 16
    assert l.fdm_op_slot_sched_bank(C.byref(sa), 16, 16, 1, None, None) == ERR_ARG and b"bank" in l.fdm_last_error()
    assert l.fdm_op_slot_sched_bank(C.byref(sa), 16, 16, 1, C.byref(b), None) == ERR_ARG           # the bank's own pointers are NULL
    assert l.fdm_op_slot_group_sched_bank(C.byref(sa), 16, 16, 1, C.byref(g), None, None) == ERR_ARG
    assert l.fdm_op_slot_group_sched_bank(C.byref(sa), 16, 16, 1, None, C.byref(b), None) == ERR_ARG


def test_sampler_add_refuses_noise_and_record():
    l = _lib.lib()
    for field in ("noise", "record"):
        a = SampleArgs()
        a.kind, a.ddim_steps = 1, 6
        setattr(a, field, 16)
        assert l.fdm_slot_sampler_add(None, C.byref(a), None) == ERR_ARG
        assert b"noise and record" in l.fdm_last_error(), field


def test_sampler_info_leaves_its_outputs_on_error():
    l = _lib.lib()
    k, n = C.c_int(7), C.c_int(7)
    assert l.fdm_slot_sampler_info(None, 0, C.byref(k), C.byref(n)) == ERR_ARG
    assert (k.value, n.value) == (7, 7)


def test_bank_operator_validation_without_a_device():
    l = _lib.lib()

    def args(**kw):
        sa, g, b = SchedArgs(), SlotGroupArgs(), SlotBankArgs()
        sa.x0 = sa.x = sa.x_out = 16
        sa.n, sa.n_per_clip = 2 * 8 * 64, 8 * 64
        sa.c1 = sa.c2 = sa.sigma = sa.sra = sa.srm1 = 16
        g.member = g.frames = g.entries = g.groups = g.x_long = 16
        g.arena_frames, g.n_entries, g.n_groups, g.L, g.d, g.frame0, g.frame1, g.plain = 20, 16, 1, 8, 64, 0, 20, 1
        b.req = b.desc = b.t = b.coef = 16
        b.n_samplers, b.n_t, b.n_coef = 2, 12, 48
        for k, v in kw.items():
            setattr(b if hasattr(b, k) else (g if hasattr(g, k) else sa), k, v)
        return sa, g, b

    def plain(**kw):
        sa, _, b = args(**kw)
        return l.fdm_op_slot_sched_bank(C.byref(sa), 16, 16, 2, C.byref(b), None)

    def group(**kw):
        sa, g, b = args(**kw)
        return l.fdm_op_slot_group_sched_bank(C.byref(sa), 16, 16, 2, C.byref(g), C.byref(b), None)
    h = C.c_void_p()
    assert l.fdm_prog_create(C.byref(h)) == 0 and l.fdm_prog_begin(h) == 0     # recorded, never launched on this machine
    try:
        for call in (plain, group):
            assert call() == 0
            assert call(n_coef=0, coef=None) == 0                               # a bank of DDPM samplers holds no coefficients
            assert call(n_samplers=0) == ERR_SHAPE
            assert call(n_t=0) == ERR_SHAPE
            assert call(n_coef=8, coef=None) == ERR_SHAPE
            assert call(desc=None) == ERR_ARG
            assert call(req=24) == ERR_ARG                                      # alignment of the 16-byte rows
            assert call(desc=20) == ERR_ARG
            assert call(noise=16) == ERR_ARG
            assert call(n_per_clip=8 * 64 + 2) == ERR_SHAPE
            assert call(x_out=24) == ERR_ARG
        assert group(init=1, plain=0) == 0
        assert group(init=1) == ERR_ARG
        assert group(frame1=21) == ERR_SHAPE and group(L=7) == ERR_SHAPE
        assert l.fdm_prog_end(h) == 0 and l.fdm_prog_num_ops(h) == 5
    finally:
        l.fdm_prog_destroy(h)


# ---- SlotServer policy, plan stubbed ---------------------------------------------------------------
class StubPlan:
    """A bank of `rows` samplers beyond sampler 0: add_sampler answers FDM_ERR_STATE when every row is taken."""

    def __init__(self, n_slots, rows):
        self.n_slots, self.rows, self.calls, self.bank = n_slots, rows, [], {}

    def get(self, key):
        return self.n_slots

    def add_sampler(self, kind, steps=None, t_list=None, tables=None):
        free = [i for i in range(1, self.rows + 1) if i not in self.bank]
        if not free:
            e = FdmError("libfdm_hip error -4: slot_sampler_add: all bank rows are in use")
            e.code = ERR_STATE
            raise e
        self.bank[free[0]] = (kind, steps if kind == "ddim" else len(t_list))
        self.calls.append(("add", free[0]) + self.bank[free[0]])
        return free[0]

    def drop_sampler(self, id):
        del self.bank[id]
        self.calls.append(("drop", id))

    def admit(self, slot, hub, ids, emo, x_T, L, seed, clip_id, **own):
        self.calls.append(("admit", slot, L, own.get("sampler", "old"), own.get("cfg_scale")))


def stub_server(n_slots=3, rows=2, bank_steps=40, cfg=False, n_emo=0):
    srv = object.__new__(pipeline.SlotServer)
    p = presets.get("mead_tiny" if n_emo else "vocaset_tiny")
    enc = lambda wav: types.SimpleNamespace(last_hidden_state=torch.zeros(1, wav.shape[1] * p.pair, 4))
    srv.p, srv.device, srv.model = p, "cpu", types.SimpleNamespace(audio_encoder=enc)
    srv.diffusion = types.SimpleNamespace(num_timesteps=1000, full_chain=True)
    srv.n_slots, srv.L, srv.long_frames, srv.overlap = n_slots, 40, 0, 10
    srv.cfg, srv.scale = cfg, 2.5
    srv.bank_samplers, srv.bank_steps = rows, bank_steps
    srv.plan = StubPlan(n_slots, rows)
    srv.default = srv._definition(6, None, 20, 0.0)
    srv._defs, srv._lru = {srv.default: 0}, []
    srv._next, srv._queue, srv._slot, srv._done = 0, [], [None] * n_slots, []
    return srv


def test_a_request_resolves_its_sampler_as_animate_does():
    srv = stub_server()
    assert srv.default == ("ddim", 6)
    assert srv._request(None, None, None, None, None) == (None, None)                  # names nothing: the server's own, the old admit
    assert srv._request(6, None, None, None, None) == (None, None)                     # names the server's definition: the same
    assert srv._request(9, None, None, None, None) == (("ddim", 9), None)
    assert srv._request(9, "dpmpp2m", None, None, None) == (("tables", "dpmpp2m", 20, 0.0), None)      # sampler= wins, 20 steps by default
    assert srv._request(None, "ddim_eta", 5, 0.5, None) == (("tables", "ddim_eta", 5, 0.5), None)
    assert srv._request(None, None, None, None, 1.7) == (None, None)                   # cfg_scale without guidance is ignored
    mead = stub_server(cfg=True, n_emo=7)
    assert mead._definition(6, None, 20, 0.0) == ("ddpm",)                             # animate() ignores ddim_steps on an emotion preset
    assert mead._request(None, None, None, None, 2.5) == (None, None)                  # the server's own scale
    assert mead._request(None, None, None, None, 1.7) == (mead.default, 1.7)


def test_submit_refuses_what_can_never_fit():
    srv = stub_server(rows=0, bank_steps=0)
    with pytest.raises(ValueError, match="without a sampler bank"):
        srv.submit(torch.zeros(10), ddim_steps=9)
    srv.submit(torch.zeros(10), ddim_steps=6)                                          # the default by name is fine
    srv.submit(torch.zeros(10))
    assert srv.plan.calls == [("admit", 0, 10, "old", None), ("admit", 1, 10, "old", None)]
    srv = stub_server(bank_steps=8)
    with pytest.raises(ValueError, match="9 steps"):
        srv.submit(torch.zeros(10), sampler="dpmpp2m", sampler_steps=9)
    with pytest.raises(ValueError, match="steps"):
        srv.submit_many([torch.zeros(10), torch.zeros(12)], ddim_steps=[4, 100])       # DDIM 100 has 99 live pairs
    assert srv._queue == [] and srv.plan.calls == [] and srv._next == 0
    srv.submit(torch.zeros(10), ddim_steps=9)                                          # 8 live pairs: fits
    assert srv.plan.calls == [("add", 1, "ddim", 9), ("admit", 0, 10, 1, None)]


def test_definitions_are_mapped_once_and_the_lru_sampler_is_dropped():
    srv = stub_server(n_slots=3, rows=2)
    h0 = srv.submit(torch.zeros(10), ddim_steps=4)
    h1 = srv.submit(torch.zeros(11), sampler="dpmpp2m", sampler_steps=5)
    h2 = srv.submit(torch.zeros(12), ddim_steps=4)                                     # known: no second add
    assert srv.plan.calls == [("add", 1, "ddim", 4), ("admit", 0, 10, 1, None), ("add", 2, "tables", 5), ("admit", 1, 11, 2, None),
                              ("admit", 2, 12, 1, None)]
    assert srv._defs == {("ddim", 6): 0, ("ddim", 4): 1, ("tables", "dpmpp2m", 5, 0.0): 2} and srv._lru == [2, 1]
    h3 = srv.submit(torch.zeros(13), ddim_steps=9)                                     # no slot: queued, the bank untouched
    assert len(srv.plan.calls) == 5 and [r["handle"] for r in srv._queue] == [h3]
    srv._slot[1] = None                                                                # the 2M request leaves; DDIM 4 is still held twice
    srv._fill()
    assert srv.plan.calls[5:] == [("drop", 2), ("add", 2, "ddim", 9), ("admit", 1, 13, 2, None)]
    assert ("tables", "dpmpp2m", 5, 0.0) not in srv._defs and srv._defs[("ddim", 9)] == 2
    assert {h0, h1, h2, h3} == {0, 1, 2, 3}


def test_a_full_bank_in_use_keeps_the_request_at_the_head():
    srv = stub_server(n_slots=4, rows=1)
    srv.submit(torch.zeros(10), ddim_steps=4)
    h1 = srv.submit(torch.zeros(11), ddim_steps=9)                                     # the only row is held by slot 0: waits
    h2 = srv.submit(torch.zeros(12))                                                   # a slot is idle, but it may not pass h1
    assert srv.plan.calls == [("add", 1, "ddim", 4), ("admit", 0, 10, 1, None)]
    assert [r["handle"] for r in srv._queue] == [h1, h2]
    srv._slot[0] = None
    srv._fill()
    assert srv.plan.calls[2:] == [("drop", 1), ("add", 1, "ddim", 9), ("admit", 0, 11, 1, None), ("admit", 1, 12, "old", None)]
    assert srv._queue == []


def test_a_request_with_its_own_scale_rides_sampler_zero():
    srv = stub_server(cfg=True, n_emo=7)
    srv.submit(torch.zeros(10), cfg_scale=1.7)
    srv.submit(torch.zeros(10), cfg_scale=2.5)
    assert srv.plan.calls == [("admit", 0, 10, 0, 1.7), ("admit", 1, 10, "old", None)]
