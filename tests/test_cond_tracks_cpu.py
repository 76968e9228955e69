"""CPU: condition tracks (include/fdm_hip.h, "Condition tracks") -- the exported symbols and their bindings, the pinned version, the
argument errors that need no device (fdm_op_cond_rows recorded into a program, never launched here; the plan-level entry points on
their null checks), and the host helpers of fdm_amd.tracks: frame placement, cross-fades that sum to 1, the argmax rule of a
cross-fade row, times at the preset's latent frame rate."""
import ctypes as C

import pytest
import torch

from fdm_amd import _lib, tracks

ERR_ARG, ERR_SHAPE = -1, -2
NEW_SYMBOLS = ["fdm_op_argmax_rows", "fdm_op_vq_quant_rows", "fdm_op_vq_stats_rows", "fdm_vq_quant_tracks", "fdm_vq_quant_stats_tracks",
               "fdm_window_peek", "fdm_op_cond_rows", "fdm_audio_prepare_tracks", "fdm_audio_prepare_windows_tracks", "fdm_slot_admit_tracks",
               "fdm_slot_admit_long_tracks"]


def test_new_symbols_are_exported_and_bound_and_the_version_is_pinned():
    l = _lib.lib()
    for n in NEW_SYMBOLS:
        assert hasattr(l, n) and n in _lib.SYMBOLS, n
    assert l.fdm_version() == _lib.LIB_VERSION == 105
    for cname, mirror in _lib.STRUCTS.items():          # no public struct changed
        assert l.fdm_abi_struct_size(cname.encode()) == C.sizeof(mirror), cname


def test_null_tracks_and_null_plans_are_argument_errors():
    l = _lib.lib()
    ids = (C.c_int * 3)(0, 1, 2)
    # a null style track, whatever else is passed
    assert l.fdm_audio_prepare_tracks(None, 16, 1, 10, 1024, None, 16, 5, 0, None) == ERR_ARG
    assert l.fdm_audio_prepare_windows_tracks(None, 16, 1, 100, 1024, None, 16, 50, 24, 8, 0, None) == ERR_ARG
    assert b"null style track" in l.fdm_last_error()
    assert l.fdm_slot_admit_tracks(None, 0, 16, 10, 1024, None, 16, 5, 16, 0, 0, 0, 2.5, None) == ERR_ARG and b"null style track" in l.fdm_last_error()
    assert l.fdm_slot_admit_long_tracks(None, ids, 3, 16, 100, 1024, None, 16, 50, 8, 16, 0, 0, 0, 2.5, None) == ERR_ARG
    assert b"null style track" in l.fdm_last_error()
    # a null plan
    assert l.fdm_audio_prepare_tracks(None, 16, 1, 10, 1024, 16, 16, 5, 0, None) == ERR_ARG
    assert l.fdm_audio_prepare_windows_tracks(None, 16, 1, 100, 1024, 16, 16, 50, 24, 8, 0, None) == ERR_ARG
    assert l.fdm_slot_admit_tracks(None, 0, 16, 10, 1024, 16, 16, 5, 16, 0, 0, 0, 2.5, None) == ERR_ARG
    assert l.fdm_slot_admit_long_tracks(None, ids, 3, 16, 100, 1024, 16, 16, 50, 8, 16, 0, 0, 0, 2.5, None) == ERR_ARG


def test_op_cond_rows_validation_without_a_device():
    l = _lib.lib()
    base = dict(pe=16, style=16, emo=16, sw=16, sb=16, ew=16, eb=16, out=16, uncond_off=0, B=2, L=7, L_clip=5, L_track=7, d=512,
                n_style=25, n_emo=7, act=0)

    def call(**kw):
        a = dict(base, **kw)
        return l.fdm_op_cond_rows(a["pe"], a["style"], a["emo"], a["sw"], a["sb"], a["ew"], a["eb"], a["out"], a["uncond_off"], a["B"], a["L"],
                                  a["L_clip"], a["L_track"], a["d"], a["n_style"], a["n_emo"], a["act"], None)
    h = C.c_void_p()
    assert l.fdm_prog_create(C.byref(h)) == 0 and l.fdm_prog_begin(h) == 0          # recorded, never launched on this machine
    try:
        assert call() == 0
        assert call(emo=None, ew=None, eb=None, n_emo=0) == 0                       # a model without emotions
        assert call(sb=None, eb=None) == 0                                          # biases are optional, as in fdm_op_small_linear
        assert call(uncond_off=2 * 7 * 512) == 0 and call(uncond_off=5 * 7 * 512) == 0      # a slot's rows inside a larger table
        assert call(L_clip=7) == 0 and call(L_track=5) == 0
        for null in ("pe", "style", "sw", "out"):
            assert call(**{null: None}) == ERR_ARG, null
        assert call(ew=None) == ERR_ARG and b"emotion" in l.fdm_last_error()
        assert call(act=9) == ERR_ARG
        assert call(B=0) == ERR_SHAPE and call(L=0) == ERR_SHAPE and call(d=0) == ERR_SHAPE
        assert call(L_clip=0) == ERR_SHAPE and call(L_clip=8) == ERR_SHAPE           # outside [1, L]
        assert call(L_track=4) == ERR_SHAPE                                          # the track is shorter than the clip
        assert call(n_style=0) == ERR_SHAPE and call(n_style=129) == ERR_SHAPE and call(n_emo=129) == ERR_SHAPE
        assert call(uncond_off=-512) == ERR_SHAPE and call(uncond_off=2 * 7 * 512 + 4) == ERR_SHAPE
        assert call(uncond_off=7 * 512) == ERR_SHAPE                                 # would overlap the cond half
        assert call(B=1 << 20, L=1 << 12) == ERR_SHAPE                               # rows beyond a 32-bit grid
        assert l.fdm_prog_end(h) == 0 and l.fdm_prog_num_ops(h) == 7                 # one launch each
    finally:
        l.fdm_prog_destroy(h)


def test_keyframes_place_frames_piecewise_constant():
    a, b, c = torch.eye(7)[4], torch.eye(7)[1], torch.eye(7)[0]
    t = tracks.keyframes(40, [(0, a), (17, b), (33, c)])
    assert t.shape == (40, 7) and t.dtype == torch.float32
    assert (t[:17] == a).all() and (t[17:33] == b).all() and (t[33:] == c).all()
    # the first keyframe also covers the frames before it
    t = tracks.keyframes(10, [(4, a), (6, b)])
    assert (t[:6] == a).all() and (t[6:] == b).all()
    for bad in ([], [(0, a), (0, b)], [(5, a), (3, b)], [(0, a), (40, b)], [(-1, a)], [(0, a), (3, torch.eye(6)[0])]):
        with pytest.raises(ValueError):
            tracks.keyframes(40, bad)
    with pytest.raises(ValueError):
        tracks.keyframes(0, [(0, a)])
    with pytest.raises(ValueError):
        tracks.keyframes(10, [(0, a)], ramp=-1)


def test_ramps_are_convex_mixes_that_sum_to_one():
    a, b = torch.eye(7)[4], torch.eye(7)[1]
    t = tracks.keyframes(40, [(0, a), (20, b)], ramp=4)
    assert torch.allclose(t.sum(-1), torch.ones(40), atol=1e-6) and (t >= 0).all()
    assert (t[:18] == a).all() and (t[22:] == b).all()                               # 4 frames centred on frame 20: 18 .. 21
    w = t[18:22, 1]
    assert torch.allclose(w, torch.tensor([0.2, 0.4, 0.6, 0.8]), atol=1e-6) and torch.allclose(t[18:22, 4], 1 - w, atol=1e-6)
    # ramp 0 is the jump; a fade never reaches past its neighbouring keyframes or the ends of the track
    assert torch.equal(tracks.keyframes(40, [(0, a), (20, b)], ramp=0), tracks.keyframes(40, [(0, a), (20, b)]))
    t = tracks.keyframes(6, [(0, a), (1, b), (5, a)], ramp=6)
    assert t.shape == (6, 7) and (t[0] == a).all() and torch.allclose(t.sum(-1), torch.ones(6), atol=1e-6)


def test_the_book_of_a_ramp_row_is_its_first_maximum():
    a, b = torch.eye(7)[4], torch.eye(7)[1]
    t = tracks.keyframes(40, [(0, a), (20, b)], ramp=3)          # frames 19, 20, 21 carry 0.25, 0.5, 0.75 of the new emotion
    book = tracks.book_of(t)
    assert book.tolist() == [4] * 20 + [1] * 20                   # the tie at frame 20 goes to the first maximum: index 1 < 4
    t = tracks.keyframes(40, [(0, b), (20, a)], ramp=3)
    assert tracks.book_of(t).tolist() == [1] * 21 + [4] * 19      # ... here too: the tie stays with index 1
    assert torch.equal(tracks.book_of(t), torch.argmax(t, dim=-1))


def test_from_seconds_uses_the_latent_frame_rate():
    assert tracks.frame_rate("vocaset") == 50.0 and tracks.frame_rate("mead") == 25.0 and tracks.frame_rate("biwi") == 25.0
    e = torch.eye(7)
    t = tracks.from_seconds("mead", 1500, [(0, e[4]), (21.0, e[1]), (40.0, e[4])])
    assert tracks.book_of(t).tolist() == [4] * 525 + [1] * 475 + [4] * 500
    assert torch.equal(t, tracks.keyframes(1500, [(0, e[4]), (525, e[1]), (1000, e[4])]))
    t = tracks.from_seconds("vocaset", 200, [(0, torch.eye(8)[0]), (2.0, torch.eye(8)[3])], ramp=0.2)
    assert torch.equal(t, tracks.keyframes(200, [(0, torch.eye(8)[0]), (100, torch.eye(8)[3])], ramp=10))


def test_parse_reads_the_command_line_form():
    names = ["angry", "contempt", "disgusted", "fear", "neutral", "happy", "sad"]
    keys = tracks.parse("0:neutral,21.0:happy,40.0:neutral", names)
    assert [k[0] for k in keys] == [0.0, 21.0, 40.0] and [int(k[1].argmax()) for k in keys] == [4, 5, 4]
    assert [int(k[1].argmax()) for k in tracks.parse("0:2, 3.5:6", names)] == [2, 6]
    with pytest.raises(ValueError):
        tracks.parse("0:9", names)


def test_rowbook_operators_and_quant_tracks_validation_without_a_device():
    l = _lib.lib()
    assert l.fdm_vq_quant_tracks(None, 16, 16, 1, 8, 16, 16, None) == ERR_ARG
    assert l.fdm_vq_quant_stats_tracks(None, 16, 16, 16, 1, 8, 0.25, None, 16, None) == ERR_ARG
    assert l.fdm_window_peek(None, 16, None) != 0
    h = C.c_void_p()
    assert l.fdm_prog_create(C.byref(h)) == 0 and l.fdm_prog_begin(h) == 0          # recorded, never launched on this machine
    try:
        assert l.fdm_op_argmax_rows(16, 16, 26, 7, 8, 7, None) == 0
        # an argmax over more columns than the codebook has slices could name a book outside it: refused on the host
        assert l.fdm_op_argmax_rows(16, 16, 26, 8, 8, 7, None) == ERR_SHAPE and b"outside" in l.fdm_last_error()
        assert l.fdm_op_argmax_rows(16, 16, 26, 7, 8, 0, None) == ERR_SHAPE
        assert l.fdm_op_argmax_rows(None, 16, 26, 7, 8, 7, None) == ERR_ARG and l.fdm_op_argmax_rows(16, 16, 0, 7, 8, 7, None) == ERR_SHAPE
        assert l.fdm_op_vq_quant_rows(16, 16, 16, 7, 2, 104, 64, 256, 16, 16, None) == 0
        assert l.fdm_op_vq_quant_rows(16, 16, None, 7, 2, 104, 64, 256, 16, 16, None) == ERR_ARG
        assert l.fdm_op_vq_quant_rows(16, 16, 16, 0, 2, 104, 64, 256, 16, 16, None) == ERR_SHAPE
        assert l.fdm_op_vq_quant_rows(16, 16, 16, 7, 2, 104, 129, 256, 16, 16, None) == ERR_SHAPE
        assert l.fdm_op_vq_stats_rows(16, 16, 16, 7, 16, 2, 104, 64, 256, 0.25, None, 16, 16, 16, None) == 0
        assert l.fdm_op_vq_stats_rows(16, 16, None, 7, 16, 2, 104, 64, 256, 0.25, None, 16, 16, 16, None) == ERR_ARG
        assert l.fdm_op_vq_stats_rows(16, 16, 16, 0, 16, 2, 104, 64, 256, 0.25, None, 16, 16, 16, None) == ERR_SHAPE
        assert l.fdm_prog_end(h) == 0 and l.fdm_prog_num_ops(h) == 3
    finally:
        l.fdm_prog_destroy(h)


def test_from_spec_is_the_command_line_form():
    names = ["angry", "contempt", "disgusted", "fear", "happy", "sad", "surprised"]
    t = tracks.from_spec("mead", 100, "0:happy,2.0:sad,30.0:angry", names)          # 30 s lies past the 100 frames (4 s): dropped
    assert tracks.book_of(t).tolist() == [4] * 50 + [5] * 50
    t = tracks.from_spec("vocaset", 600, "0:0,0.5:3", [str(i) for i in range(8)], ramp=0.1)
    assert t.shape == (600, 8) and tracks.book_of(t)[20] == 0 and tracks.book_of(t)[30] == 3 and 0 < float(t[25, 3]) < 1
