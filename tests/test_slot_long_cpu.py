"""CPU: long requests in slot mode (include/fdm_hip.h, fdm_slot_admit_long) -- the host table of a group
(fdm_slot_group_table_host), the argument errors that need no device, the pinned version, and the queue policy of
pipeline.SlotServer.submit_long with the plan stubbed (strict FIFO: nothing passes a long request that waits)."""
import ctypes as C
import math
import random
import types

import numpy as np
import pytest
import torch

from fdm_amd import _lib, pipeline, presets
from fdm_amd._lib import FdmError, SchedArgs, SlotGroupArgs

ERR_ARG, ERR_SHAPE, ERR_STATE = -1, -2, -4
CASES = [(100, 40, 10), (100, 40, 30), (41, 40, 0), (75, 40, 39)]          # (L_total, L, overlap)
LONG_SYMBOLS = ["fdm_slot_admit_long", "fdm_slot_group", "fdm_slot_read_long", "fdm_slot_group_table_host", "fdm_op_slot_group_sched"]


def group_table(L_total, L, O, slots):
    l = _lib.lib()
    ids = (C.c_int * len(slots))(*slots)
    ne = l.fdm_slot_group_table_host(L_total, L, O, ids, len(slots), None, None, None, None, 0)
    assert ne == len(slots) * L
    off, es, est = np.full(L_total + 1, -7, np.int32), np.full(ne, -7, np.int32), np.full(ne, -7, np.int32)
    ew = np.full(ne, np.nan, np.float32)
    assert l.fdm_slot_group_table_host(L_total, L, O, ids, len(slots), off.ctypes.data, es.ctypes.data, est.ctypes.data, ew.ctypes.data, ne) == ne
    return off, es, est, ew


def layout(L_total, L, O):
    l = _lib.lib()
    n = l.fdm_window_layout_host(L_total, L, O, None, 0)
    st = (C.c_int * n)()
    assert l.fdm_window_layout_host(L_total, L, O, st, n) == n
    w = np.empty((n, min(L, L_total)), np.float32)
    assert l.fdm_window_weights_host(L_total, L, O, w.ctypes.data) == n
    return list(st), w


def test_long_symbols_are_exported_and_the_version_is_pinned():
    l = _lib.lib()
    for n in LONG_SYMBOLS:
        assert hasattr(l, n) and n in _lib.SYMBOLS, n
    assert l.fdm_version() == 105
    assert l.fdm_abi_struct_size(b"fdm_slot_group_args") == C.sizeof(SlotGroupArgs)


@pytest.mark.parametrize("L_total,L,O", CASES)
def test_group_table_host(L_total, L, O):
    starts, w = layout(L_total, L, O)
    n = len(starts)
    slots = list(range(3, 3 + n))
    random.Random(L_total + O).shuffle(slots)
    if n > 1:
        assert slots != sorted(slots) or n == 2
    off, es, est, ew = group_table(L_total, L, O, slots)
    assert off[0] == 0 and off[-1] == n * L
    assert (np.diff(off) >= 1).all()                                       # monotone, and every frame has at least one entry
    for f in range(L_total):
        ws = [k for k in range(n) if starts[k] <= f < starts[k] + L]       # the covering windows, ascending
        j0, j1 = off[f], off[f + 1]
        assert j1 - j0 == len(ws), f
        assert list(est[j0:j1]) == [starts[k] for k in ws], f              # ascending window order
        assert list(es[j0:j1]) == [slots[k] for k in ws], f                # slot ids follow the list
        want = np.array([w[k, f - starts[k]] for k in ws], np.float32)
        assert ew[j0:j1].tobytes() == want.tobytes(), f                    # fdm_window_weights_host's bits
        s = math.fsum(float(v) for v in ew[j0:j1])                          # the exact sum of the fp32 weights (up to 36 of them here)
        assert abs(s - 1.0) <= 2 * float(np.spacing(np.float32(1.0))), (f, s)


def test_group_table_host_errors():
    l = _lib.lib()
    ids = (C.c_int * 8)(*range(8))
    assert l.fdm_slot_group_table_host(100, 40, 10, None, 3, None, None, None, None, 0) == ERR_ARG
    assert l.fdm_slot_group_table_host(100, 40, 40, ids, 3, None, None, None, None, 0) == ERR_ARG       # overlap >= L
    assert l.fdm_slot_group_table_host(40, 40, 10, ids, 1, None, None, None, None, 0) == ERR_SHAPE      # one window: no group
    assert l.fdm_slot_group_table_host(100, 40, 10, ids, 4, None, None, None, None, 0) == ERR_SHAPE     # 3 windows, 4 slots
    off = np.full(101, -7, np.int32)
    buf = np.full(120, -7, np.int32)
    assert l.fdm_slot_group_table_host(100, 40, 10, ids, 3, off.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 119) == 120
    assert (off == -7).all() and (buf == -7).all()                         # cap too small: the count, nothing written


def test_calls_on_a_null_plan():
    l = _lib.lib()
    ids = (C.c_int * 3)(0, 1, 2)
    a, n, lt = C.c_int(7), C.c_int(7), C.c_int(7)
    assert l.fdm_slot_admit_long(None, ids, 3, 16, 100, 1024, 16, None, 100, 10, 16, 0, 0, None) == ERR_ARG
    assert l.fdm_slot_group(None, 0, C.byref(a), C.byref(n), C.byref(lt)) == ERR_ARG
    assert (a.value, n.value, lt.value) == (7, 7, 7)
    assert l.fdm_slot_read_long(None, 0, 16, None) == ERR_ARG
    assert l.fdm_op_slot_group_sched(None, None, None, 1, None, None) == ERR_ARG
    sa, g = SchedArgs(), SlotGroupArgs()
    assert l.fdm_op_slot_group_sched(C.byref(sa), None, None, 1, C.byref(g), None) == ERR_ARG
    assert b"null" in l.fdm_last_error()


def test_op_argument_validation_without_a_device():
    l = _lib.lib()

    def args(**kw):
        sa, g = SchedArgs(), SlotGroupArgs()
        sa.x0 = sa.x = sa.x_out = 16
        sa.n, sa.n_per_clip, sa.mode = 2 * 8 * 64, 8 * 64, 1
        sa.sra = sa.srm1 = sa.sqrt_an = sa.c_n = 16
        g.member = g.frames = g.entries = g.groups = g.x_long = 16
        g.arena_frames, g.n_entries, g.n_groups, g.L, g.d, g.frame0, g.frame1, g.plain = 20, 16, 1, 8, 64, 0, 20, 1
        for k, v in kw.items():
            setattr(g if hasattr(g, k) else sa, k, v)
        return sa, g

    def call(**kw):
        sa, g = args(**kw)
        return l.fdm_op_slot_group_sched(C.byref(sa), 16, 16, 2, C.byref(g), None)
    h = C.c_void_p()
    assert l.fdm_prog_create(C.byref(h)) == 0 and l.fdm_prog_begin(h) == 0     # recorded, never launched on this machine
    try:
        assert call() == 0
        assert call(init=1, plain=0) == 0
        assert call(init=1) == ERR_ARG                                          # init loads window rows only
        assert call(frame1=21) == ERR_SHAPE
        assert call(L=7) == ERR_SHAPE                                           # L * d != n_per_clip
        assert call(d=62) == ERR_SHAPE
        assert call(noise=16) == ERR_ARG
        assert call(mode=3) == ERR_ARG                                          # no tables / histories
        assert call(x_long=24) == ERR_ARG                                       # alignment
        assert call(frames=None) == ERR_ARG
        assert l.fdm_prog_end(h) == 0 and l.fdm_prog_num_ops(h) == 2
    finally:
        l.fdm_prog_destroy(h)


# ---- SlotServer queue policy, plan stubbed ---------------------------------------------------------
class StubPlan:
    """Counts what SlotServer asks of the plan; `arena_free` = False makes admit_long answer FDM_ERR_STATE (arena busy)."""

    def __init__(self, n_slots):
        self.n_slots, self.calls, self.arena_free = n_slots, [], True

    def get(self, key):
        return self.n_slots

    def admit(self, slot, hub, ids, emo, x_T, L, seed, clip_id):
        self.calls.append(("admit", slot, L))

    def admit_long(self, slots, hub, ids, emo, x_T, L_total, overlap, seed, clip_id):
        if not self.arena_free:
            e = FdmError("libfdm_hip error -4: slot_admit_long: no free arena range")
            e.code = ERR_STATE
            raise e
        assert x_T.shape[1] == L_total * 16 and hub.shape[1] == L_total
        self.calls.append(("admit_long", tuple(slots), L_total, overlap))


def stub_server(n_slots=4, L=40, long_frames=200, overlap=10):
    srv = object.__new__(pipeline.SlotServer)
    p = presets.get("vocaset_tiny")
    enc = lambda wav: types.SimpleNamespace(last_hidden_state=torch.zeros(1, wav.shape[1], 4))      # one frame per sample
    srv.p, srv.device, srv.model = p, "cpu", types.SimpleNamespace(audio_encoder=enc)
    srv.n_slots, srv.L, srv.long_frames, srv.overlap = n_slots, L, long_frames, overlap
    srv.plan = StubPlan(n_slots)
    srv._next, srv._queue, srv._slot, srv._done = 0, [], [None] * n_slots, []
    return srv


def test_submit_long_refuses_what_can_never_fit():
    srv = stub_server(n_slots=2, long_frames=200)
    with pytest.raises(ValueError, match="windows"):
        srv.submit_long(torch.zeros(100))                    # 3 windows of 40, 2 slots
    with pytest.raises(ValueError, match="arena"):
        srv.submit_long(torch.zeros(201))
    assert srv._queue == [] and srv.plan.calls == [] and srv._next == 0
    plain = stub_server(long_frames=0)
    with pytest.raises(ValueError, match="arena"):
        plain.submit_long(torch.zeros(41))
    plain.submit_long(torch.zeros(40))                       # fits a slot: an ordinary request
    assert plain.plan.calls == [("admit", 0, 40)]


def test_queue_is_fifo_and_nothing_passes_a_waiting_long_request():
    srv = stub_server(n_slots=4)
    h0 = srv.submit_long(torch.zeros(30))                    # short: slot 0
    h1 = srv.submit_long(torch.zeros(25))                    # short: slot 1
    assert srv.plan.calls == [("admit", 0, 30), ("admit", 1, 25)]
    h2 = srv.submit_long(torch.zeros(100))                   # 3 windows, 2 idle slots: waits
    h3 = srv.submit_long(torch.zeros(20))                    # a slot is idle, but it may not pass h2
    assert [r["handle"] for r in srv._queue] == [h2, h3] and len(srv.plan.calls) == 2
    assert srv.pending == 4
    srv._slot[0] = None                                      # h0 leaves: 3 idle slots
    srv._fill()
    assert srv.plan.calls[2] == ("admit_long", (0, 2, 3), 100, 10)
    assert [r["handle"] for r in srv._queue] == [h3] and srv.pending == 3        # the group counts once
    assert srv._slot[0] is srv._slot[2] is srv._slot[3] and srv._slot[0]["slots"] == [0, 2, 3]
    srv._slot[1] = None                                      # h1 leaves: h3 gets its slot
    srv._fill()
    assert srv.plan.calls[3] == ("admit", 1, 20) and srv._queue == []
    assert {h0, h1, h2, h3} == {0, 1, 2, 3}


def test_a_busy_arena_keeps_the_long_request_at_the_head():
    srv = stub_server(n_slots=4)
    srv.plan.arena_free = False
    h0 = srv.submit_long(torch.zeros(100))                   # slots are idle, the arena is not: waits, plan untouched
    h1 = srv.submit_long(torch.zeros(10))
    assert srv.plan.calls == [] and [r["handle"] for r in srv._queue] == [h0, h1] and srv._slot == [None] * 4
    srv.plan.arena_free = True
    srv._fill()
    assert srv.plan.calls == [("admit_long", (0, 1, 2), 100, 10), ("admit", 3, 10)] and srv._queue == []


def test_without_long_requests_fill_is_todays():
    """Plain requests: admitted in order into the lowest idle slots, the rest queued -- what _fill did before long requests."""
    srv = stub_server(n_slots=2)
    for n in (11, 12, 13):
        srv._queue.append(dict(handle=srv._next, hub=torch.zeros(1, n, 4), L=n, ids=None, emo=None, x_T=torch.zeros(1, n * 16, 16), seed=0, template=None))
        srv._next += 1
        srv._fill()
    assert srv.plan.calls == [("admit", 0, 11), ("admit", 1, 12)] and len(srv._queue) == 1
    srv._slot[1] = None
    srv._fill()
    assert srv.plan.calls[-1] == ("admit", 1, 13) and srv.pending == 2
