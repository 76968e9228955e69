"""CPU: the C surface of in-flight batching (fdm_slots_open / fdm_slot_admit / fdm_slots_run / fdm_slot_state / fdm_slot_read,
fdm_op_slot_sched, fdm_ln_args.clip_step) -- exported symbols, struct mirrors, the pinned version and the argument errors that
need no device."""
import ctypes as C

from fdm_amd import _lib
from fdm_amd._lib import LnArgs, SampleArgs, SchedArgs

ERR_ARG = -1
SLOT_SYMBOLS = ["fdm_slots_open", "fdm_slot_admit", "fdm_slots_run", "fdm_slot_state", "fdm_slot_read", "fdm_op_slot_sched"]


def test_slot_symbols_are_exported_and_bound():
    l = _lib.lib()
    for n in SLOT_SYMBOLS:
        assert hasattr(l, n), n
        assert n in _lib.SYMBOLS, n


def test_struct_sizes_match_their_mirrors_and_the_version_is_pinned():
    l = _lib.lib()
    assert l.fdm_version() == 105
    for cname, mirror in _lib.STRUCTS.items():
        assert l.fdm_abi_struct_size(cname.encode()) == C.sizeof(mirror), cname
    # the per-clip fields sit at the END of fdm_ln_args: a zero-filled mirror keeps the single step word
    names = [f[0] for f in LnArgs._fields_]
    assert names[-4:] == ["clip_step", "clip_step_stride", "clip_rows", "clip_wrap"]
    assert names.index("x_plane_stride") == len(names) - 5


def test_null_arguments():
    l = _lib.lib()
    a = SampleArgs()
    a.kind, a.ddim_steps = 1, 4
    assert l.fdm_slots_open(None, 2, 8, 0, C.byref(a), None) == ERR_ARG
    assert l.fdm_slots_open(None, 2, 8, 0, None, None) == ERR_ARG
    assert l.fdm_slot_admit(None, 0, None, 1, 1, None, None, 1, None, 0, 0, None) == ERR_ARG
    assert l.fdm_slots_run(None, 1, None) == ERR_ARG
    assert l.fdm_slot_read(None, 0, None, None) == ERR_ARG
    assert l.fdm_op_slot_sched(None, None, None, 1, None) == ERR_ARG
    sa = SchedArgs()
    assert l.fdm_op_slot_sched(C.byref(sa), None, None, 1, None) == ERR_ARG
    assert b"null" in l.fdm_last_error()


def test_slots_open_refuses_injected_noise_and_record():
    l = _lib.lib()
    buf = (C.c_float * 4)()
    for field in ("noise", "record"):
        a = SampleArgs()
        a.kind, a.ddim_steps = 1, 4
        setattr(a, field, C.cast(buf, C.c_void_p))
        assert l.fdm_slots_open(None, 2, 8, 0, C.byref(a), None) == ERR_ARG
        assert b"noise and record" in l.fdm_last_error()


def test_slot_state_on_a_null_plan():
    l = _lib.lib()
    d, t, s = C.c_int(7), C.c_int(7), C.c_int(7)
    assert l.fdm_slot_state(None, 0, C.byref(d), C.byref(t), C.byref(s)) == ERR_ARG
    assert (d.value, t.value, s.value) == (7, 7, 7)
