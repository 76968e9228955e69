"""ctypes binding of libfdm_hip.so (include/fdm_hip.h).  The product path has no CPU fallback:
if the library is missing or a call fails, this module raises."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FDM_LIB_PATH: load another build of the same library (the AddressSanitizer host build, csrc `make asan`)
LIB_PATH = os.environ.get("FDM_LIB_PATH") or os.path.join(_HERE, "libfdm_hip.so")

F32, BF16, F16X3, F16 = 0, 1, 2, 3      # include/fdm_hip.h FDM_*: operand kinds (F16X3 is a split plane pair; F16 its hi plane alone: denoiser only)
DTYPE_NAMES = {"f32": F32, "bf16": BF16, "f16x3": F16X3, "f16": F16}
SAMPLER_DPMPP_2M, SAMPLER_DDIM = 0, 1    # fdm_sampler_tables_host kinds
SLOT_IDLE, SLOT_RUNNING, SLOT_FINISHED = 0, 1, 2     # fdm_slot_state status
SAMPLER_NAMES = {"dpmpp2m": SAMPLER_DPMPP_2M, "ddim_eta": SAMPLER_DDIM}
ACT_NONE, ACT_RELU, ACT_MISH, ACT_GELU_ERF, ACT_GELU_TANH, ACT_LEAKY02 = range(6)

vp, ll, ci, cf = C.c_void_p, C.c_longlong, C.c_int, C.c_float


class SchedArgs(C.Structure):
    _fields_ = [("x0", vp), ("x0u", vp), ("cfg_scale", cf), ("x", vp), ("x_out", vp),
                ("n", ll), ("n_per_clip", ll), ("tseq", vp), ("step", vp), ("advance", ci),
                ("c1", vp), ("c2", vp), ("sigma", vp), ("sra", vp), ("srm1", vp),
                ("sqrt_an", vp), ("c_n", vp), ("noise", vp), ("noise_stride", ll), ("x_out_t", vp), ("out_dtype", ci), ("arrive", vp),
                ("seed", C.c_ulonglong), ("clip0", ci),
                ("mode", ci), ("x_out_t_lo_off", ll), ("seed_dev", vp),
                ("lm_a", vp), ("lm_b", vp), ("lm_c", vp), ("lm_s", vp), ("x0_hist", vp)]


class GemmArgs(C.Structure):
    _fields_ = [("A", vp), ("lda", ll), ("a_batch_stride", ll),
                ("W", vp), ("ldw", ll), ("w_batch_stride", ll),
                ("M", ci), ("N", ci), ("K", ci), ("batch", ci), ("dtype", ci),
                ("bias", vp), ("bias_batch_stride", ll), ("act", ci),
                ("resid", vp), ("ldr", ll), ("resid_row_mod", ci),
                ("out_f32", vp), ("ldo_f32", ll), ("out_t", vp), ("ldo_t", ll),
                ("out_batch_stride", ll),
                ("out_kp", vp), ("kp_col0", ci), ("out_vp", vp), ("vp_col0", ci),
                ("kv_L", ci), ("kv_Lpad", ci), ("kv_hd", ci),
                ("stat_out", vp), ("ln_stat_in", vp), ("ln_nparts", ci), ("ln_dim", ci), ("ln_eps", cf),
                ("ln_colsum", vp), ("rln_gamma", vp), ("rln_beta", vp), ("incr_counter", vp), ("incr_table", vp), ("tile", ci),
                ("sched_fuse", ci), ("sched", SchedArgs),
                ("a_lo_off", ll), ("w_lo_off", ll), ("out_t_lo_off", ll), ("kv_lo_off", ll),
                ("ksplit", ci), ("ksplit_stride", ll), ("batch2", ci), ("a_batch_stride2", ll), ("out_batch_stride2", ll)]


# the eight tiles of include/fdm_hip.h, and the retired ids (accepted: they resolve to a live tile)
TILE_AUTO, TILE_64x64, TILE_128x64, TILE_128x128, TILE_64x64_S2, TILE_32x64_S3, TILE_256x128_PP, TILE_80x128, TILE_64x128 = 0, 1, 2, 3, 8, 9, 10, 11, 12
TILE_96x128, TILE_256x128, TILE_64x64_S3, TILE_128x64_S3 = 4, 5, 6, 7


class ModelDesc(C.Structure):
    _fields_ = [(n, ci) for n in ("d", "n_head", "n_layers", "ffn", "G", "c", "n_style", "n_emo", "audio_in", "pair",
                                  "pe_periodic", "period", "latent_mish", "style_mish", "max_len")]


class SampleArgs(C.Structure):
    _fields_ = [("kind", ci), ("x_T", vp), ("out", vp), ("t_list", vp), ("n_steps", ci), ("ddim_steps", ci), ("noise", vp),
                ("seed", C.c_ulonglong), ("clip0", ci), ("cfg_scale", cf), ("eager", ci), ("record", vp), ("graph_steps", ci),
                ("lm_tables", vp)]


class VqDesc(C.Structure):
    _fields_ = [(n, ci) for n in ("G", "c", "K", "n_books", "V3", "pre")]


class AttnArgs(C.Structure):
    _fields_ = [("Q", vp), ("ldq", ll), ("Kp", vp), ("Vp", vp), ("Lpad", ci),
                ("O", vp), ("ldo", ll), ("B", ci), ("H", ci), ("L", ci), ("hd", ci), ("dtype", ci),
                ("scale", cf), ("causal", ci), ("slopes", vp), ("period", ci), ("o_split", ci), ("o_lo_off", ll), ("q_lo_off", ll), ("kv_lo_off", ll),
                ("lens", vp)]


class LnArgs(C.Structure):
    _fields_ = [("x", vp), ("M", ci), ("d", ci), ("add_mat", vp), ("add_tab", vp),
                ("tab_index", vp), ("tab_step", vp), ("gamma", vp), ("beta", vp), ("eps", cf),
                ("act", ci), ("y_f32", vp), ("y_t", vp), ("dtype", ci), ("gamma2", vp), ("beta2", vp), ("y_t_lo_off", ll),
                ("add_mat_L", ci), ("add_mat_group", ci), ("add_mat_wrap", ci), ("x_planes", ci), ("x_plane_stride", ll),
                ("clip_step", vp), ("clip_step_stride", ci), ("clip_rows", ci), ("clip_wrap", ci)]


class SlotGroupArgs(C.Structure):
    _fields_ = [("member", vp), ("frames", vp), ("entries", vp), ("groups", vp), ("x_long", vp), ("hist_long", vp),
                ("arena_frames", ci), ("n_entries", ci), ("n_groups", ci), ("L", ci), ("d", ci), ("frame0", ci), ("frame1", ci),
                ("plain", ci), ("init", ci)]


class SlotBankArgs(C.Structure):
    _fields_ = [("req", vp), ("desc", vp), ("t", vp), ("coef", vp), ("n_samplers", ci), ("n_t", ci), ("n_coef", ci), ("reserved", ci)]


class Pcm(C.Structure):
    _fields_ = [("data", vp), ("format", ci), ("channels", ci), ("rate", ci), ("frames", ll)]


class RenderPlanes(C.Structure):          # fdm_render_planes: the outputs of fdm_render_forward_planes, null where none is written
    _fields_ = [("rgb", vp), ("depth", vp), ("face", vp), ("alpha", vp), ("yuv", vp)]


class RenderMaterial(C.Structure):        # fdm_render_material: what fdm_render_set_material reads (HOST arrays, not kept)
    _fields_ = [("kind", ci), ("unlit", ci), ("colors", vp), ("lut", vp), ("n_lut", ci), ("lo", cf), ("hi", cf), ("uv", vp), ("texture", vp),
                ("tex_w", ci), ("tex_h", ci), ("filter", ci)]


class FlameModelDesc(C.Structure):
    _fields_ = [("V", ci), ("J", ci), ("NB", ci), ("expr_at", ci), ("v_template", vp), ("shapedirs", vp), ("posedirs", vp),
                ("j_regressor", vp), ("parents", vp), ("lbs_weights", vp)]


PCM_S16, PCM_S32, PCM_U8, PCM_F32 = range(4)      # fdm_pcm.format
MESH_INTERLEAVED, MESH_F16, MESH_NORMALS = 1, 2, 4      # fdm_mesh_forward flags
WRAP_OFFSETS = 1      # fdm_wrap_forward flags
TFILTER_GAUSSIAN, TFILTER_SAVGOL = 0, 1      # fdm_tfilter_taps_host kinds
TFILTER_MIRROR, TFILTER_NEAREST = 0, 1       # fdm_tfilter_create edge rules
TFILTER_EMA, TFILTER_ONE_EURO = 0, 1         # fdm_tfilter_create_recur kinds
TFILTER_CAUSAL, TFILTER_ZERO_PHASE = 0, 1    # fdm_tfilter_create_recur directions
TFILTER_NCOEFF = 8                           # floats of fdm_tfilter_recur_coeffs_host

# public structs of include/fdm_hip.h -> their mirrors (sizes checked against the loaded library in lib())
STRUCTS = {"fdm_sched_args": SchedArgs, "fdm_gemm_args": GemmArgs, "fdm_attn_args": AttnArgs, "fdm_ln_args": LnArgs,
           "fdm_model_desc": ModelDesc, "fdm_sample_args": SampleArgs, "fdm_vq_desc": VqDesc, "fdm_slot_group_args": SlotGroupArgs,
           "fdm_slot_bank_args": SlotBankArgs, "fdm_pcm": Pcm, "fdm_flame_model": FlameModelDesc, "fdm_render_planes": RenderPlanes,
           "fdm_render_material": RenderMaterial}

# every symbol include/fdm_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "fdm_last_error": (C.c_char_p, []),
    "fdm_version": (ci, []),
    "fdm_abi_struct_size": (ci, [C.c_char_p]),
    "fdm_device_ok": (ci, []),
    "fdm_op_gemm": (ci, [C.POINTER(GemmArgs), vp]),
    "fdm_gemm_heuristic_tile": (ci, [C.POINTER(GemmArgs)]),
    "fdm_op_attention": (ci, [C.POINTER(AttnArgs), vp]),
    "fdm_op_pack_kv": (ci, [vp, ll, vp, ll, vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "fdm_op_layernorm": (ci, [C.POINTER(LnArgs), vp]),
    "fdm_op_sched_step": (ci, [C.POINTER(SchedArgs), vp]),
    "fdm_op_slot_sched": (ci, [C.POINTER(SchedArgs), vp, vp, ci, vp]),
    "fdm_op_slot_group_sched": (ci, [C.POINTER(SchedArgs), vp, vp, ci, C.POINTER(SlotGroupArgs), vp]),
    "fdm_op_slot_sched_bank": (ci, [C.POINTER(SchedArgs), vp, vp, ci, C.POINTER(SlotBankArgs), vp]),
    "fdm_op_slot_group_sched_bank": (ci, [C.POINTER(SchedArgs), vp, vp, ci, C.POINTER(SlotGroupArgs), C.POINTER(SlotBankArgs), vp]),
    "fdm_op_cast": (ci, [vp, vp, ll, ci, vp]),
    "fdm_op_vertex_err": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]),
    "fdm_op_motion_std": (ci, [vp, vp, vp, ci, ci, ci, vp, vp, vp]),
    "fdm_op_linear_interp": (ci, [vp, vp, ci, ci, ci, ci, vp]),
    "fdm_op_bias_act": (ci, [vp, vp, vp, ll, ci, ci, vp]),
    "fdm_op_add_rows": (ci, [vp, ci, ci, vp, ci, ci, vp, ci, ci, vp, ll, ci, vp]),
    "fdm_op_small_linear": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, vp]),
    "fdm_op_pad_rows": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "fdm_op_pad_rows_lens": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, vp]),
    "fdm_op_zero_pad_rows": (ci, [vp, ci, ci, ci, vp, vp]),
    "fdm_op_group_pad": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp]),
    "fdm_op_set_ints": (ci, [vp, vp, ci, vp]),
    "fdm_op_mask_samples": (ci, [vp, vp, ci, ci, vp, vp]),
    "fdm_op_group_pad_lens": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]),
    "fdm_op_conv0": (ci, [vp, vp, vp, vp, ci, ci, ci, vp]),
    "fdm_op_conv0_ln_gelu": (ci, [vp, vp, vp, vp, vp, vp, ll, ci, ci, ci, cf, ci, vp]),
    "fdm_op_leaky_instnorm": (ci, [vp, vp, vp, ci, ci, ci, cf, ci, vp]),
    "fdm_op_leaky_instnorm_lens": (ci, [vp, vp, vp, ci, ci, ci, cf, ci, vp, vp]),
    "fdm_op_adain": (ci, [vp, vp, vp, ci, ci, ci, cf, vp]),
    "fdm_op_mean_diff": (ci, [vp, vp, vp, vp, ll, ci, vp]),
    "fdm_op_time_groupnorm": (ci, [vp, vp, vp, vp, vp, ll, ci, ci, ci, cf, ci, ci, vp, ll, vp]),
    "fdm_op_time_groupnorm_lens": (ci, [vp, vp, vp, vp, vp, ll, ci, ci, ci, cf, ci, ci, vp, ll, vp, vp]),
    "fdm_op_vq_quant": (ci, [vp, vp, vp, ci, ci, ci, ci, vp, vp, vp]),
    "fdm_op_vq_stats": (ci, [vp, vp, vp, vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, vp]),
    "fdm_prog_create": (ci, [C.POINTER(vp)]),
    "fdm_prog_destroy": (ci, [vp]),
    "fdm_prog_begin": (ci, [vp]),
    "fdm_prog_end": (ci, [vp]),
    "fdm_prog_run": (ci, [vp, vp]),
    "fdm_prog_instantiate": (ci, [vp, vp]),
    "fdm_prog_replay": (ci, [vp, ci, vp]),
    "fdm_prog_num_ops": (ci, [vp]),
    "fdm_model_preset": (ci, [C.c_char_p, C.POINTER(ModelDesc)]),
    "fdm_plan_create": (ci, [C.POINTER(ModelDesc), ci, ci, ci, ci, C.POINTER(vp)]),
    "fdm_plan_reserve": (ci, [vp, ci, ci, ci]),
    "fdm_plan_destroy": (ci, [vp]),
    "fdm_plan_set_weights": (ci, [vp, C.c_char_p, vp, ll, vp]),
    "fdm_plan_commit": (ci, [vp, vp]),
    "fdm_audio_prepare": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp]),
    "fdm_audio_prepare_conds": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, vp]),
    "fdm_denoise_step": (ci, [vp, vp, ci, cf, vp, vp, vp]),
    "fdm_sample_graph": (ci, [vp, C.POINTER(SampleArgs), vp]),
    "fdm_window_layout_host": (ci, [ci, ci, ci, vp, ci]),
    "fdm_window_weights_host": (ci, [ci, ci, ci, vp]),
    "fdm_audio_prepare_windows": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
    "fdm_sample_windows": (ci, [vp, C.POINTER(SampleArgs), vp]),
    "fdm_slots_open": (ci, [vp, ci, ci, ci, C.POINTER(SampleArgs), vp]),
    "fdm_slot_admit": (ci, [vp, ci, vp, ci, ci, vp, vp, ci, vp, C.c_ulonglong, ci, vp]),
    "fdm_slots_run": (ci, [vp, ci, vp]),
    "fdm_slot_state": (ci, [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
    "fdm_slot_read": (ci, [vp, ci, vp, vp]),
    "fdm_slot_peek": (ci, [vp, ci, vp, vp]),
    "fdm_slot_admit_long": (ci, [vp, vp, ci, vp, ci, ci, vp, vp, ci, ci, vp, C.c_ulonglong, ci, vp]),
    "fdm_slot_group": (ci, [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]),
    "fdm_slot_read_long": (ci, [vp, ci, vp, vp]),
    "fdm_slot_group_table_host": (ci, [ci, ci, ci, vp, ci, vp, vp, vp, vp, ci]),
    "fdm_slot_sampler_add": (ci, [vp, C.POINTER(SampleArgs), vp]),
    "fdm_slot_sampler_drop": (ci, [vp, ci]),
    "fdm_slot_sampler_info": (ci, [vp, ci, C.POINTER(ci), C.POINTER(ci)]),
    "fdm_slot_admit_as": (ci, [vp, ci, vp, ci, ci, vp, vp, ci, vp, C.c_ulonglong, ci, ci, cf, vp]),
    "fdm_slot_admit_long_as": (ci, [vp, vp, ci, vp, ci, ci, vp, vp, ci, ci, vp, C.c_ulonglong, ci, ci, cf, vp]),
    "fdm_op_cond_rows": (ci, [vp, vp, vp, vp, vp, vp, vp, vp, ll, ci, ci, ci, ci, ci, ci, ci, ci, vp]),
    "fdm_audio_prepare_tracks": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp]),
    "fdm_audio_prepare_windows_tracks": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, ci, ci, vp]),
    "fdm_slot_admit_tracks": (ci, [vp, ci, vp, ci, ci, vp, vp, ci, vp, C.c_ulonglong, ci, ci, cf, vp]),
    "fdm_slot_admit_long_tracks": (ci, [vp, vp, ci, vp, ci, ci, vp, vp, ci, ci, vp, C.c_ulonglong, ci, ci, cf, vp]),
    "fdm_window_peek": (ci, [vp, vp, vp]),
    "fdm_op_argmax_rows": (ci, [vp, vp, ll, ci, ci, ci, vp]),
    "fdm_op_vq_quant_rows": (ci, [vp, vp, vp, ci, ci, ci, ci, ci, vp, vp, vp]),
    "fdm_op_vq_stats_rows": (ci, [vp, vp, vp, ci, vp, ci, ci, ci, ci, cf, vp, vp, vp, vp, vp]),
    "fdm_vq_quant_tracks": (ci, [vp, vp, vp, ci, ci, vp, vp, vp]),
    "fdm_vq_quant_stats_tracks": (ci, [vp, vp, vp, vp, ci, ci, cf, vp, vp, vp]),
    "fdm_plan_tune": (ci, [vp, vp]),
    "fdm_plan_get": (ci, [vp, C.c_char_p, C.POINTER(ll)]),
    "fdm_plan_set": (ci, [vp, C.c_char_p, ll]),
    "fdm_hubert_create": (ci, [ci, ci, ci, C.POINTER(vp)]),
    "fdm_hubert_set_weights": (ci, [vp, C.c_char_p, vp, ll, vp]),
    "fdm_hubert_forward": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, C.POINTER(ci), vp]),
    "fdm_hubert_frames": (ci, [ci]),
    "fdm_hubert_forward_ragged": (ci, [vp, vp, vp, ci, ci, vp, vp, vp]),
    "fdm_hubert_destroy": (ci, [vp]),
    "fdm_frontend_create": (ci, [vp, ci, C.POINTER(vp)]),
    "fdm_frontend_samples": (ci, [C.POINTER(Pcm), ci, C.POINTER(ll)]),
    "fdm_frontend_forward": (ci, [vp, C.POINTER(Pcm), ci, ci, ci, vp, ll, vp, vp]),
    "fdm_frontend_destroy": (ci, [vp]),
    "fdm_mesh_adjacency_host": (ci, [vp, ci, ci, vp, vp]),
    "fdm_mesh_create": (ci, [vp, ci, ci, C.POINTER(vp)]),
    "fdm_mesh_frames": (ci, [ci, C.c_double, C.c_double, C.POINTER(ci)]),
    "fdm_mesh_forward": (ci, [vp, vp, vp, ci, ci, vp, ci, C.c_double, C.c_double, ci, vp, vp, ci, vp, vp]),
    "fdm_mesh_destroy": (ci, [vp]),
    "fdm_rig_gram_host": (ci, [vp, vp, ci, ci, C.c_double, vp, vp]),
    "fdm_rig_create": (ci, [vp, ci, ci, vp, C.c_double, vp, vp, ci, C.POINTER(vp)]),
    "fdm_rig_forward": (ci, [vp, vp, vp, ci, ci, C.c_double, C.c_double, vp, vp, ci, vp, vp]),
    "fdm_rig_destroy": (ci, [vp]),
    "fdm_rig_temporal_tables_host": (ci, [vp, ci, C.c_double, vp, vp, vp]),
    "fdm_rig_set_temporal": (ci, [vp, C.c_double, vp]),
    "fdm_flame_tables_host": (ci, [C.POINTER(FlameModelDesc), vp, vp, vp]),
    "fdm_flame_create": (ci, [C.POINTER(FlameModelDesc), vp, vp, ci, C.POINTER(vp)]),
    "fdm_flame_forward": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp]),
    "fdm_flame_destroy": (ci, [vp]),
    "fdm_flame_fit_create": (ci, [vp, vp, ci, ci, ci, vp, C.POINTER(vp)]),
    "fdm_flame_fit_set": (ci, [vp, C.c_char_p, C.c_double]),
    "fdm_flame_fit_forward": (ci, [vp, vp, vp, ci, ci, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]),
    "fdm_flame_fit_step": (ci, [vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]),
    "fdm_flame_fit_destroy": (ci, [vp]),
    "fdm_wrap_coords_host": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, vp]),
    "fdm_wrap_create": (ci, [vp, vp, ci, ci, vp, ci, vp, vp, C.POINTER(vp)]),
    "fdm_wrap_binding": (ci, [vp, vp, vp, vp]),
    "fdm_wrap_forward": (ci, [vp, vp, vp, ci, ci, vp, ci, ci, vp, vp]),
    "fdm_wrap_destroy": (ci, [vp]),
    "fdm_tfilter_taps_host": (ci, [ci, ci, C.c_double, vp]),
    "fdm_tfilter_create": (ci, [ci, ci, vp, vp, ci, vp, C.POINTER(vp)]),
    "fdm_tfilter_forward": (ci, [vp, vp, vp, ci, ci, vp]),
    "fdm_tfilter_destroy": (ci, [vp]),
    "fdm_tfilter_recur_coeffs_host": (ci, [ci, C.c_double, C.c_double, C.c_double, C.c_double, vp]),
    "fdm_tfilter_create_recur": (ci, [ci, ci, vp, vp, ci, vp, C.POINTER(vp)]),
    "fdm_tfilter_forward_state": (ci, [vp, vp, vp, ci, ci, vp, vp, vp]),
    "fdm_tfilter_set_prefetch": (ci, [vp, ci]),
    "fdm_render_create": (ci, [vp, ci, ci, ci, ci, vp, vp, vp, vp, ci, cf, vp, vp, C.POINTER(vp)]),
    "fdm_render_set_view": (ci, [vp, vp, vp, vp, vp, ci, cf]),
    "fdm_render_set": (ci, [vp, C.c_char_p, ll]),
    "fdm_render_sample_pattern_host": (ci, [ci, vp]),
    "fdm_render_forward": (ci, [vp, vp, vp, ci, ci, vp, ci, C.c_double, C.c_double, vp, vp, vp, vp, ci, vp, vp]),
    "fdm_render_forward_planes": (ci, [vp, vp, vp, ci, ci, vp, ci, C.c_double, C.c_double, vp, C.POINTER(RenderPlanes), ci, vp, vp]),
    "fdm_render_yuv_coeffs_host": (ci, [ci, ci, vp]),
    "fdm_render_set_material": (ci, [vp, C.POINTER(RenderMaterial)]),
    "fdm_render_forward_material": (ci, [vp, vp, vp, ci, ci, vp, ci, C.c_double, C.c_double, vp, C.POINTER(RenderPlanes), ci, vp, vp, vp]),
    "fdm_op_vertex_dist": (ci, [vp, vp, vp, ci, ci, vp]),
    "fdm_render_destroy": (ci, [vp]),
    "fdm_vq_create": (ci, [C.POINTER(VqDesc), ci, C.POINTER(vp)]),
    "fdm_vq_set_weights": (ci, [vp, C.c_char_p, vp, ll, vp]),
    "fdm_vq_quant": (ci, [vp, vp, vp, ci, ci, vp, vp, vp]),
    "fdm_vq_quant_stats": (ci, [vp, vp, vp, vp, ci, ci, cf, vp, vp, vp]),
    "fdm_vq_decode": (ci, [vp, vp, ci, ci, vp, vp]),
    "fdm_vq_decode_ragged": (ci, [vp, vp, vp, ci, ci, vp, vp]),
    "fdm_vq_encode": (ci, [vp, vp, vp, ci, ci, vp, vp]),
    "fdm_vq_destroy": (ci, [vp]),
    "fdm_schedule_host": (ci, [ci, vp]),
    "fdm_ddim_schedule_host": (ci, [ci, ci, vp, vp, vp, vp]),
    "fdm_sampler_tables_host": (ci, [ci, ci, ci, C.c_double, vp, vp, vp, vp, vp]),
    "fdm_alibi_slopes_host": (ci, [ci, vp]),
    "fdm_pe_table_host": (ci, [ci, ci, ci, ci, vp]),
    "fdm_resample_ratio_host": (ci, [ci, C.POINTER(ci), C.POINTER(ci)]),
    "fdm_resample_len_host": (ll, [ci, ll]),
    "fdm_resample_taps_host": (ci, [ci, ci, vp]),
}

_lib = None
LIB_VERSION = 105      # include/fdm_hip.h as this binding mirrors it (fdm_version()): struct layouts AND entry-point signatures


class FdmError(RuntimeError):
    pass


def lib():
    """Load (once) and return the bound library; raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FdmError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the product path)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        # a signature changed in place under an old symbol name would corrupt arguments silently: the build must be the one this
        # binding was written for
        if l.fdm_version() != LIB_VERSION:
            raise FdmError(f"{LIB_PATH}: fdm_version() = {l.fdm_version()}, this binding is for {LIB_VERSION}: rebuild the library "
                           "(python -c 'import __graft_entry__ as g; g.build()')")
        # the ctypes mirrors above must be the structs this build was compiled with (a stale .so or a header edit that
        # missed this file would otherwise corrupt arguments silently)
        for cname, mirror in STRUCTS.items():
            n = l.fdm_abi_struct_size(cname.encode())
            if n != C.sizeof(mirror):
                raise FdmError(f"{LIB_PATH}: sizeof({cname}) = {n} in the library, {C.sizeof(mirror)} in fdm_amd/_lib.py: rebuild the "
                               "library (python -c 'import __graft_entry__ as g; g.build()') or update the binding")
        _lib = l
    return _lib


def check(code):
    if code != 0:
        err = FdmError(f"libfdm_hip error {code}: {lib().fdm_last_error().decode()}")
        err.code = code              # FDM_ERR_*: a caller that waits on FDM_ERR_STATE (SlotServer) reads it here
        raise err
