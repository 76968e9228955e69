"""CPU: the entry points for clips of unequal length (include/fdm_hip.h: fdm_attn_args.lens, fdm_vq_decode_ragged and the
length-aware operators under it) are exported, the attention struct's mirror has the new last field, and every validation
failure is reported before a device is touched (there is none here)."""
import ctypes as C

from fdm_amd import _lib

ARG, SHAPE = -1, -2


def test_ragged_symbols_are_exported_and_bound():
    l = _lib.lib()
    for n in ("fdm_hubert_forward_ragged", "fdm_vq_decode_ragged", "fdm_op_set_ints", "fdm_op_mask_samples", "fdm_op_group_pad_lens",
              "fdm_op_time_groupnorm_lens", "fdm_op_pad_rows_lens", "fdm_op_leaky_instnorm_lens", "fdm_op_zero_pad_rows"):
        assert hasattr(l, n) and n in _lib.SYMBOLS, n


def test_attn_args_gains_lens_as_its_last_field():
    l = _lib.lib()
    assert l.fdm_abi_struct_size(b"fdm_attn_args") == C.sizeof(_lib.AttnArgs)
    name, _ = _lib.AttnArgs._fields_[-1]
    assert name == "lens"
    assert _lib.AttnArgs.lens.offset + C.sizeof(C.c_void_p) == C.sizeof(_lib.AttnArgs)      # nothing after it, nothing moved behind it
    assert _lib.AttnArgs.kv_lo_off.offset + 8 == _lib.AttnArgs.lens.offset
    assert l.fdm_version() == _lib.LIB_VERSION == 105


def _attn():
    a = _lib.AttnArgs()
    a.Q = a.Kp = a.Vp = a.O = 16
    a.ldq = a.ldo = 128
    a.B, a.H, a.L, a.hd, a.Lpad, a.dtype, a.scale, a.period = 2, 2, 40, 64, 64, _lib.F32, 0.125, 1
    a.lens = 16
    return a


def test_attention_lens_validation():
    l = _lib.lib()
    a = _attn()
    a.causal = 1
    assert l.fdm_op_attention(C.byref(a), None) == ARG and b"per-clip lengths" in l.fdm_last_error()
    a = _attn()
    a.hd, a.ldq, a.ldo = 256, 512, 512
    assert l.fdm_op_attention(C.byref(a), None) == ARG and b"per-clip lengths" in l.fdm_last_error()


def test_length_aware_operators_refuse_null_lengths():
    l = _lib.lib()
    assert l.fdm_op_pad_rows_lens(16, 16, 2, 8, 64, 2, _lib.F32, None, None) == ARG
    assert l.fdm_op_leaky_instnorm_lens(16, 16, None, 2, 8, 64, 1e-5, _lib.F32, None, None) == ARG
    assert l.fdm_op_zero_pad_rows(16, 2, 8, 64, None, None) == ARG
    assert l.fdm_op_zero_pad_rows(None, 2, 8, 64, 16, None) == ARG


def _vq(G=8, c=128, pre=0):
    l = _lib.lib()
    h = C.c_void_p()
    desc = _lib.VqDesc(G, c, 256, 1, 15069, pre)
    assert l.fdm_vq_create(C.byref(desc), _lib.F32, C.byref(h)) == 0
    return l, h


def test_vq_decode_ragged_validation_precedes_any_launch():
    l, h = _vq()
    try:
        ok = (C.c_int * 3)(2, 5, 12)
        R = 12 * 8
        assert l.fdm_vq_decode_ragged(None, 16, ok, 3, R, 16, None) == ARG
        assert l.fdm_vq_decode_ragged(h, None, ok, 3, R, 16, None) == ARG
        assert l.fdm_vq_decode_ragged(h, 16, None, 3, R, 16, None) == ARG
        assert l.fdm_vq_decode_ragged(h, 16, ok, 3, R, None, None) == ARG
        assert l.fdm_vq_decode_ragged(h, 16, ok, 0, R, 16, None) == SHAPE
        assert l.fdm_vq_decode_ragged(h, 16, ok, 3, R + 1, 16, None) == SHAPE                   # R_max % G
        for bad in ((2, 1, 12), (2, 5, 13), (0, 5, 12), (2, -3, 12)):                            # below the minimum, above R_max / G
            assert l.fdm_vq_decode_ragged(h, 16, (C.c_int * 3)(*bad), 3, R, 16, None) == SHAPE, bad
            assert b"frames" in l.fdm_last_error()
    finally:
        l.fdm_vq_destroy(h)


def test_hubert_forward_ragged_validation_precedes_any_launch():
    l = _lib.lib()
    for kind in (0, 1):
        h = C.c_void_p()
        assert l.fdm_hubert_create(kind, 2, _lib.F32, C.byref(h)) == 0
        try:
            ok, nf = (C.c_int * 2)(4000, 16000), (C.c_int * 2)()
            assert l.fdm_hubert_forward_ragged(None, 16, ok, 2, 16000, 16, nf, None) == ARG
            assert l.fdm_hubert_forward_ragged(h, None, ok, 2, 16000, 16, nf, None) == ARG
            assert l.fdm_hubert_forward_ragged(h, 16, None, 2, 16000, 16, nf, None) == ARG
            assert l.fdm_hubert_forward_ragged(h, 16, ok, 2, 16000, None, nf, None) == ARG
            assert l.fdm_hubert_forward_ragged(h, 16, ok, 2, 16000, 16, None, None) == ARG
            assert l.fdm_hubert_forward_ragged(h, 16, ok, 0, 16000, 16, nf, None) == SHAPE
            assert l.fdm_hubert_forward_ragged(h, 16, (C.c_int * 2)(4000, 399), 2, 16000, 16, nf, None) == SHAPE     # below the minimum
            assert b"too short" in l.fdm_last_error()
            assert l.fdm_hubert_forward_ragged(h, 16, (C.c_int * 2)(4000, 16001), 2, 16000, 16, nf, None) == SHAPE   # n_samples[b] > n_max
            assert b"wide" in l.fdm_last_error()
        finally:
            l.fdm_hubert_destroy(h)


def test_binding_frame_arithmetic_is_fdm_hubert_frames():
    from fdm_amd.hubert import num_frames
    l = _lib.lib()
    for n in list(range(400, 2000)) + [3999, 4000, 16000, 16001, 48000, 123455, 160000]:
        assert num_frames(n) == l.fdm_hubert_frames(n), n
