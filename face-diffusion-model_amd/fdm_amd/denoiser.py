"""Denoiser + scheduler plan: a thin binding of the library's plan layer (include/fdm_hip.h: fdm_plan_create,
fdm_plan_set_weights, fdm_audio_prepare, fdm_denoise_step, fdm_sample_graph; implementation csrc/plan.hip, with the tile
tuner in csrc/tune.hip and the host tables -- schedules, sampler tables, window layout -- in csrc/host_tables.hip).

The per-step FDM forward (models/fdm_vocaset.py:54-91, models/fdm_vqvae_mead.py:65-104) and the sampling loops
(diffusion_BIWI_encoder_decoder.py:649-710, diffusion_mead_encoder_decoder.py:649-667) live in C++ / HIP:
  * commit (once per model): operand-kind weight copies; tau table = Mish(W_t[:, t] + b_t) for all 1000 t (the one-hot
    GEMV of :71-72 is a column gather); per-layer time tables TT_l[t] = Wo_l (Wv_l tau_t) of the folded cross-attention.
  * prepare (once per batch of clips): AF = audio_extract(audio-encoder features); per-layer tables
    C1_l = Wo_l (Wv_l AF + bv_l) + bo_l; E0 = PE[l] + style[b] (+ emotion[b]).  The cross-attention's memory mask leaves
    exactly one key per query (models/fdm_vocaset.py:119-127), so CA_l(h, AF + tau)[i] = C1_l[i] + TT_l[t] exactly.
  * step program (recorded once, captured into a hipGraph, `graph_steps` diffusion steps per graph launch; t comes from a
    device counter): latent_encoder GEMM(+bias+Mish+E0) -> n_layers x { QKV GEMM (K / V written fragment-packed) -> fused
    causal-ALiBi attention -> out-proj GEMM(+bias+residual) -> fused LN1+LN2(+C1_l + TT_l[t]) -> FFN1 GEMM(+bias+ReLU) ->
    FFN2 GEMM(+bias+residual) -> LN3 } -> latent_decoder GEMM with the scheduler update (DDPM / DDIM, Philox or injected
    noise) in its epilogue; CFG plans run cond + uncond rows through the same launches and mix in the scheduler kernel.
This module only moves pointers: torch owns the caller-side tensors and the stream."""
import ctypes as C

import torch

from . import presets, schedule
from ._lib import F32, FdmError, ModelDesc, SampleArgs, check, lib

TILE_SITES = ("enc", "qkv", "qkv_ln", "out", "out_ln", "ffn1", "ffn2", "ffn2_stat", "dec", "dec_ln")


def _dev(t, device):
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def model_desc(p):
    """fdm_model_desc of a presets.Preset (the reference constructors' numbers)."""
    return ModelDesc(p.d, p.n_head, p.n_layers, p.ffn, p.G, p.c, p.n_style, p.n_emo, p.audio_in, p.pair,
                     1 if p.pe == "periodic" else 0, p.period, int(p.latent_mish), int(p.style_mish), p.max_len)


def window_starts(L_total, window, overlap=60):
    """Window starts of the windowed-sampling layout (fdm_window_layout_host; include/fdm_hip.h states the rule)."""
    n = lib().fdm_window_layout_host(int(L_total), int(window), int(overlap), None, 0)
    if n < 0:
        check(n)
    buf = (C.c_int * n)()
    check(0 if lib().fdm_window_layout_host(int(L_total), int(window), int(overlap), buf, n) == n else -1)
    return list(buf)


def window_weights(L_total, window, overlap=60):
    """Normalised blend weights [n, min(window, L_total)] of that layout (fdm_window_weights_host), a float32 CPU tensor."""
    n = lib().fdm_window_weights_host(int(L_total), int(window), int(overlap), None)
    if n < 0:
        check(n)
    w = torch.empty(n, min(int(window), int(L_total)), dtype=torch.float32)
    check(0 if lib().fdm_window_weights_host(int(L_total), int(window), int(overlap), C.c_void_p(w.data_ptr())) == n else -1)
    return w


class DenoiserPlan:
    def __init__(self, preset, weights, dtype=F32, device="cuda:0"):
        self.p = presets.get(preset)
        self.dtype = dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise FdmError("DenoiserPlan runs on the HIP path only (no CPU fallback)")
        self.h = None
        self.B = self.L = self.M = 0
        self.S = 1
        self.cfg = False
        self._keep, self._inputs = [], None
        h = C.c_void_p()
        desc = model_desc(self.p)
        with torch.cuda.device(self.device):
            check(lib().fdm_plan_create(C.byref(desc), 1, 1, 0, dtype, C.byref(h)))
            self.h = h
            # schedule tables and the positional table as the reference computes them (torch fp64 -> fp32, torch fp32
            # sin / cos / exp), so that sampling is bit-identical to the reference's expressions; C-only callers get the
            # library's own (fdm_schedule_host, fdm_pe_table_host: within 1 ulp of these)
            buf = schedule.make_buffers(1000)
            c1, c2, sg = schedule.ddpm_tables(buf)
            tabs = {"sched.c1": c1, "sched.c2": c2, "sched.sigma": sg, "sched.sra": buf["sqrt_recip_alphas_cumprod"],
                    "sched.srm1": buf["sqrt_recipm1_alphas_cumprod"],
                    "PE.pe": schedule.positional_table(self.p.d, self.p.pe, self.p.period, self.p.max_len + 30)}
            keep = []
            for k, v in list(weights.items()) + list(tabs.items()):
                if k.startswith("audio_encoder.") or (k == "PE.pe" and v is not tabs["PE.pe"]):
                    continue        # (the PE buffer is rebuilt from the constructor's numbers, as the reference's __init__ does)
                t = v.detach().to(torch.float32).contiguous()       # host or device memory: the plan copies it
                keep.append(t)
                check(lib().fdm_plan_set_weights(h, k.encode(), t.data_ptr(), t.numel(), _stream()))
            torch.cuda.current_stream().synchronize()               # the copies read `keep`
            check(lib().fdm_plan_commit(h, _stream()))

    def __del__(self):
        try:
            if self.h:
                lib().fdm_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------
    def _track(self, what, n, B, L, vec, track):
        """One condition as a device track [B, L, n]: `track` ([L', n] or [B, L', n], L' >= L: the first L rows are taken), or the
        per-clip vector `vec` ([n] or [B, n]) broadcast to frames on the device."""
        if track is not None:
            t = torch.as_tensor(track)
            t = t.unsqueeze(0).expand(B, -1, -1) if t.dim() == 2 else t
            if t.dim() != 3 or t.shape[0] != B or t.shape[1] < L or t.shape[2] != n:
                raise FdmError(f"{what} track has shape {tuple(torch.as_tensor(track).shape)}, expected [{B}, >= {L}, {n}] (or [>= {L}, {n}])")
            return _dev(t[:, :L], self.device)
        if vec is None:
            raise FdmError(f"this preset needs a {what} vector or a {what} track")
        v = _dev(vec, self.device)
        v = v.unsqueeze(0).expand(B, -1) if v.dim() == 1 else v
        if v.shape != (B, n):
            raise FdmError(f"{what} has shape {tuple(v.shape)}, expected [{B}, {n}]")
        return v.unsqueeze(1).expand(B, L, n).contiguous()

    def _tracks(self, B, L, style, emo, style_track, emotion_track):
        p = self.p
        if emotion_track is not None and not p.n_emo:
            raise FdmError(f"preset {p.name} takes no emotion")
        return (self._track("style", p.n_style, B, L, style, style_track),
                self._track("emotion", p.n_emo, B, L, emo, emotion_track) if p.n_emo else None)

    def prepare(self, hub, style=None, emo=None, L=None, cfg=False, n_conds=1, style_track=None, emotion_track=None):
        """hub [B, N, fw] audio-encoder features; style [B, n_style]; emo [B, n_emo]; L latent frames.

        style_track [B, L, n_style] / emotion_track [B, L, n_emo] (or [L, n], shared by the clips): one vector per latent frame
        instead of one per clip (fdm_audio_prepare_tracks; tracks.keyframes builds them).  Either may be given alone: the other
        condition's per-clip vector is broadcast to frames.  Frames before a change keep the bits of the unchanged run.

        n_conds = S > 1: S conditions per clip in ONE step program (fdm_audio_prepare_conds) -- what the reference's
        samplers do as S sequential B = 1 calls with the same audio (samples/sample_diffusion_vocaset.py:71-83).  style
        [B*S, n_style] / emo [B*S, n_emo] in (clip, condition) order; the plan's batch becomes B*S row blocks (x_T, noise,
        outputs are [B*S, L*G, c]); the audio tables are computed once per clip and shared by its conditions."""
        p, dv = self.p, self.device
        hub = _dev(hub, dv)
        B, N, fw = hub.shape
        S = int(n_conds)
        if S < 1:
            raise FdmError(f"n_conds={S}")
        nfa = N // p.pair
        L = nfa if L is None else min(L, nfa)
        if L < 1 or L > p.max_len:
            raise FdmError(f"latent frames L={L} outside [1, {p.max_len}] (models/fdm_vocaset.py:44)")
        if style_track is not None or emotion_track is not None:
            if S != 1:
                raise FdmError("condition tracks are not available with n_conds > 1")
            st, et = self._tracks(B, L, style, emo, style_track, emotion_track)
            with torch.cuda.device(dv):
                check(lib().fdm_audio_prepare_tracks(self.h, hub.data_ptr(), B, N, fw, st.data_ptr(), et.data_ptr() if et is not None else None,
                                                     L, int(bool(cfg)), _stream()))
            self._inputs = (hub, st, et)
            self.B, self.L, self.M, self.cfg, self.S = B, L, B * L, bool(cfg), 1
            return L
        if style is None:
            raise FdmError("prepare needs style (or style_track)")
        if style.dim() == 1:
            style = style.unsqueeze(0).expand(B * S, -1)
        if style.shape[0] != B * S:
            raise FdmError(f"style has {style.shape[0]} rows, expected clips x conditions = {B * S}")
        style = _dev(style, dv)
        if p.n_emo:
            if emo is None:
                raise FdmError("this preset needs an emotion one-hot")
            if emo.dim() == 1:
                emo = emo.unsqueeze(0).expand(B * S, -1)
            if emo.shape[0] != B * S:
                raise FdmError(f"emotion one-hot has {emo.shape[0]} rows, expected clips x conditions = {B * S}")
            emo = _dev(emo, dv)
        with torch.cuda.device(dv):
            check(lib().fdm_audio_prepare_conds(self.h, hub.data_ptr(), B, N, fw, S, style.data_ptr(),
                                                emo.data_ptr() if p.n_emo else None, L, int(bool(cfg)), _stream()))
        # the library reads hub / style / emo asynchronously on this stream: keep them alive until the next prepare
        self._inputs = (hub, style, emo)
        self.B, self.L, self.M, self.cfg, self.S = B * S, L, B * S * L, bool(cfg), S
        return L

    def _check_x(self, x):
        if self.M == 0:
            raise FdmError("call prepare() first")
        if tuple(x.shape) != (self.B, self.L * self.p.G, self.p.c):
            raise FdmError(f"latent shape {tuple(x.shape)} != {(self.B, self.L * self.p.G, self.p.c)}")
        return _dev(x, self.device)

    # ------------------------------------------------------------------------------------------
    def denoise(self, x, t, cfg_scale=2.5, return_uncond=False):
        """One FDM.forward: x [B, L*G, c] -> x0_hat [B, L*G, c] (CFG-mixed when prepared with cfg=True)."""
        x = self._check_x(x)
        out = torch.empty_like(x)
        unc = torch.empty_like(x) if (return_uncond and self.cfg) else None
        with torch.cuda.device(self.device):
            check(lib().fdm_denoise_step(self.h, x.data_ptr(), int(t), float(cfg_scale), out.data_ptr(),
                                         unc.data_ptr() if unc is not None else None, _stream()))
        return (out, unc) if return_uncond else out

    def _sample(self, a, x_T):
        x = self._check_x(x_T)
        out = torch.empty_like(x)
        a.x_T, a.out = x.data_ptr(), out.data_ptr()
        with torch.cuda.device(self.device):
            check(lib().fdm_sample_graph(self.h, C.byref(a), _stream()))
        return out

    def sample_ddpm(self, x_T, t_list, noise=None, seed=0, clip0=0, cfg_scale=2.5, use_graph=True, record=None, graph_steps=0):
        """p_sample_loop over t_list (descending).  noise [len(t_list), B, L*G, c] injects z per step; otherwise z is
        drawn in-kernel (Philox keyed by seed, global clip index clip0 + b, step).  record (a list) receives the latent
        after every step."""
        a = SampleArgs()
        ts = (C.c_int * len(t_list))(*[int(t) for t in t_list])
        a.kind, a.t_list, a.n_steps = 0, C.cast(ts, C.c_void_p), len(t_list)
        a.seed, a.clip0, a.cfg_scale, a.eager, a.graph_steps = int(seed), int(clip0), float(cfg_scale), int(not use_graph), int(graph_steps)
        if noise is not None:
            nz = _dev(noise, self.device)
            if nz.numel() != len(t_list) * self.M * self.p.d:
                raise FdmError("noise must be [len(t_list), B, L*G, c]")
            self._keep = (self._keep + [nz])[-8:]          # recorded programs (at most 8) point at it
            a.noise = nz.data_ptr()
        rec = None
        if record is not None:
            rec = torch.empty(len(t_list), *x_T.shape, device=self.device)
            a.record = rec.data_ptr()
        out = self._sample(a, x_T)
        if rec is not None:
            record.extend(rec[i] for i in range(len(t_list)))
        return out

    def sample_ddim(self, x_T, steps, cfg_scale=2.5, use_graph=True, graph_steps=0, record=None):
        """ddim_sample (eta = 0).  The last pair (t, -1) never updates the latent in the reference (:695-696), so its
        denoiser call is skipped: exact.  record (a list) receives the latent after every live pair."""
        a = SampleArgs()
        a.kind, a.ddim_steps, a.cfg_scale, a.eager, a.graph_steps = 1, int(steps), float(cfg_scale), int(not use_graph), int(graph_steps)
        rec = None
        if record is not None:
            n_live = sum(1 for pr in schedule.ddim_time_pairs(int(steps)) if pr[1] >= 0)
            rec = torch.empty(max(n_live, 1), *x_T.shape, device=self.device)
            a.record = rec.data_ptr()
        out = self._sample(a, x_T)
        if rec is not None:
            record.extend(rec[i] for i in range(n_live))
        return out

    def _tables_args(self, a, t_list, tables):
        """kind 2 of fdm_sample_args: host timesteps + host [4, n_steps] tables (the library uploads both during the call)."""
        tab = torch.as_tensor(tables, dtype=torch.float32).detach().cpu().contiguous()
        if tab.dim() != 2 or tab.shape[0] != 4 or tab.shape[1] != len(t_list):
            raise FdmError(f"tables must be [4, len(t_list) = {len(t_list)}] (a, b, c, s), got {tuple(tab.shape)}")
        ts = (C.c_int * len(t_list))(*[int(t) for t in t_list])
        a.kind, a.t_list, a.n_steps, a.lm_tables = 2, C.cast(ts, C.c_void_p), len(t_list), tab.data_ptr()
        return ts, tab

    def sample_tables(self, x_T, t_list, tables, noise=None, seed=0, clip0=0, cfg_scale=2.5, use_graph=True, record=None, graph_steps=0):
        """Table-driven linear multistep sampler (fdm_sample_graph kind 2): step k runs the denoiser at t_list[k] and sets
        x <- a[k] x + b[k] x0 + c[k] x0_prev + s[k] z with tables = [a, b, c, s] ([4, len(t_list)], host), x0_prev the previous
        step's (guidance-mixed) prediction kept by the plan.  schedule.sampler_tables builds t_list and the tables of
        DPM-Solver++ 2M and of DDIM with eta.  noise / seed / clip0 / record / use_graph / graph_steps as sample_ddpm."""
        a = SampleArgs()
        held = self._tables_args(a, t_list, tables)
        a.seed, a.clip0, a.cfg_scale, a.eager, a.graph_steps = int(seed), int(clip0), float(cfg_scale), int(not use_graph), int(graph_steps)
        if noise is not None:
            nz = _dev(noise, self.device)
            if nz.numel() != len(t_list) * self.M * self.p.d:
                raise FdmError("noise must be [len(t_list), B, L*G, c]")
            self._keep = (self._keep + [nz])[-8:]
            a.noise = nz.data_ptr()
        rec = None
        if record is not None:
            rec = torch.empty(len(t_list), *x_T.shape, device=self.device)
            a.record = rec.data_ptr()
        out = self._sample(a, x_T)
        del held
        if rec is not None:
            record.extend(rec[i] for i in range(len(t_list)))
        return out

    # ------------------------------------------------------------------------------------------
    def prepare_windows(self, hub, style=None, emo=None, L_total=None, window=None, overlap=60, cfg=False, style_track=None, emotion_track=None):
        """Clips longer than max_len (fdm_audio_prepare_windows): hub [B, N, fw] features of B whole long clips, style [B, n_style],
        emo [B, n_emo]; L_total latent frames (default N // pair, no cap) as windows of `window` (default max_len) frames overlapping
        by >= `overlap`.  The plan's batch becomes B * n windows; sample_windows takes and returns latents in the long layout
        [B, L_total*G, c].  Returns the window starts (window_starts())."""
        p, dv = self.p, self.device
        hub = _dev(hub, dv)
        B, N, fw = hub.shape
        L_total = N // p.pair if L_total is None else int(L_total)
        window = p.max_len if window is None else int(window)
        starts = window_starts(L_total, window, overlap)
        if style_track is not None or emotion_track is not None:      # [B, L_total, n] per-frame conditions (fdm_audio_prepare_windows_tracks)
            st, et = self._tracks(B, L_total, style, emo, style_track, emotion_track)
            with torch.cuda.device(dv):
                check(lib().fdm_audio_prepare_windows_tracks(self.h, hub.data_ptr(), B, N, fw, st.data_ptr(), et.data_ptr() if et is not None else None,
                                                             L_total, window, int(overlap), int(bool(cfg)), _stream()))
            self._inputs = (hub, st, et)
            W = min(window, L_total)
            self.B, self.L, self.M, self.cfg, self.S = B * len(starts), W, B * len(starts) * W, bool(cfg), 1
            self.B_long, self.L_total, self.starts = B, L_total, starts
            return starts
        if style is None:
            raise FdmError("prepare_windows needs style (or style_track)")
        if style.dim() == 1:
            style = style.unsqueeze(0).expand(B, -1)
        style = _dev(style, dv)
        if p.n_emo:
            if emo is None:
                raise FdmError("this preset needs an emotion one-hot")
            emo = _dev(emo.unsqueeze(0).expand(B, -1) if emo.dim() == 1 else emo, dv)
        if style.shape[0] != B or (p.n_emo and emo.shape[0] != B):
            raise FdmError(f"one style / emotion row per long clip expected ({B})")
        with torch.cuda.device(dv):
            check(lib().fdm_audio_prepare_windows(self.h, hub.data_ptr(), B, N, fw, style.data_ptr(),
                                                  emo.data_ptr() if p.n_emo else None, L_total, window, int(overlap),
                                                  int(bool(cfg)), _stream()))
        self._inputs = (hub, style, emo)
        W = min(window, L_total)
        self.B, self.L, self.M, self.cfg, self.S = B * len(starts), W, B * len(starts) * W, bool(cfg), 1
        self.B_long, self.L_total, self.starts = B, L_total, starts
        return starts

    def sample_windows(self, x_T, kind="ddpm", t_list=None, steps=None, noise=None, seed=0, clip0=0, cfg_scale=2.5, record=None,
                       use_graph=True, graph_steps=0, tables=None):
        """fdm_sample_windows: x_T [B, L_total*G, c] -> [B, L_total*G, c].  kind "ddpm" over t_list (noise [len(t_list), B,
        L_total*G, c] injected, or Philox keyed by (seed, clip0 + long clip, step)), "ddim" with `steps`, or "tables" over t_list
        with `tables` [4, len(t_list)] (sample_tables; noise / seed as "ddpm").  record (a list) receives the long latent after
        every step."""
        if not self.get("windows"):
            raise FdmError("call prepare_windows() first")
        shape = (self.B_long, self.L_total * self.p.G, self.p.c)
        if tuple(x_T.shape) != shape:
            raise FdmError(f"latent shape {tuple(x_T.shape)} != {shape}")
        x = _dev(x_T, self.device)
        a = SampleArgs()
        a.cfg_scale, a.eager, a.graph_steps = float(cfg_scale), int(not use_graph), int(graph_steps)
        if kind in ("ddpm", "tables"):
            if kind == "tables":
                held = self._tables_args(a, t_list, tables)
                a.seed, a.clip0 = int(seed), int(clip0)
            else:
                ts = (C.c_int * len(t_list))(*[int(t) for t in t_list])
                a.kind, a.t_list, a.n_steps, a.seed, a.clip0 = 0, C.cast(ts, C.c_void_p), len(t_list), int(seed), int(clip0)
            n_rec = len(t_list)
            if noise is not None:
                nz = _dev(noise, self.device)
                if nz.numel() != len(t_list) * x.numel():
                    raise FdmError("noise must be [len(t_list), B, L_total*G, c]")
                self._keep = (self._keep + [nz])[-8:]
                a.noise = nz.data_ptr()
        elif kind == "ddim":
            a.kind, a.ddim_steps = 1, int(steps)
            n_rec = sum(1 for pr in schedule.ddim_time_pairs(int(steps)) if pr[1] >= 0)
        else:
            raise FdmError(f"kind {kind!r} (ddpm | ddim | tables)")
        rec = None
        if record is not None:
            rec = torch.empty(max(n_rec, 1), *shape, device=self.device)
            a.record = rec.data_ptr()
        out = torch.empty_like(x)
        a.x_T, a.out = x.data_ptr(), out.data_ptr()
        with torch.cuda.device(self.device):
            check(lib().fdm_sample_windows(self.h, C.byref(a), _stream()))
        if rec is not None:
            record.extend(rec[i] for i in range(n_rec))
        return out

    def peek_windows(self):
        """fdm_window_peek: the window rows of a windowed plan as they stand, [B, n_windows, W*G, c] (inspection; changes nothing)."""
        if not self.get("windows"):
            raise FdmError("call prepare_windows() first")
        out = torch.empty(self.B_long, len(self.starts), self.L * self.p.G, self.p.c, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().fdm_window_peek(self.h, out.data_ptr(), _stream()))
        return out

    # ------------------------------------------------------------------------------------------
    def _sampler_args(self, a, kind, steps=None, t_list=None, tables=None):
        """kind / steps / t_list / tables of a sampler definition into fdm_sample_args; returns what must stay alive during the call."""
        if kind == "ddim":
            a.kind, a.ddim_steps = 1, int(steps)
            return None
        if kind == "ddpm":
            held = (C.c_int * len(t_list))(*[int(t) for t in t_list])
            a.kind, a.t_list, a.n_steps = 0, C.cast(held, C.c_void_p), len(t_list)
            return held
        if kind == "tables":
            return self._tables_args(a, t_list, tables)
        raise FdmError(f"kind {kind!r} (ddpm | ddim | tables)")

    def open_slots(self, slots, L, kind="ddim", steps=None, t_list=None, tables=None, cfg=False, cfg_scale=2.5, use_graph=True, graph_steps=0,
                   long_frames=0, long_groups=0, samplers=0, sampler_steps=0):
        """In-flight batching (fdm_slots_open): `slots` slots of up to L latent frames, each a clip at its own step of ONE shared
        sampler -- kind "ddim" with `steps`, "ddpm" over t_list, or "tables" over t_list with `tables` [4, len(t_list)]
        (sample_tables).  Every slot starts idle; admit() / run() / slot_state() / read_slot() drive them.  Returns the number of
        steps of a chain.  long_frames / long_groups > 0 reserve capacity for long requests (admit_long): an arena of long_frames
        latent frames and long_groups group descriptors; 0 = the plain slot program.
        samplers / sampler_steps > 0 reserve a sampler BANK: `samplers` definitions beyond this one (sampler 0), holding
        `sampler_steps` steps in all (add_sampler); every admit then names its sampler and, with cfg, its own cfg_scale."""
        a = SampleArgs()
        a.cfg_scale, a.eager, a.graph_steps = float(cfg_scale), int(not use_graph), int(graph_steps)
        held = self._sampler_args(a, kind, steps, t_list, tables)
        self.set("slot_long_frames", int(long_frames))
        self.set("slot_long_groups", int(long_groups))
        self.set("slot_samplers", int(samplers))
        self.set("slot_sampler_steps", int(sampler_steps))
        with torch.cuda.device(self.device):
            check(lib().fdm_slots_open(self.h, int(slots), int(L), int(bool(cfg)), C.byref(a), _stream()))
        del held
        self._slot_inputs, self._slot_scale = {}, float(cfg_scale)
        self.B, self.L, self.M, self.cfg, self.S = int(slots), int(L), int(slots) * int(L), bool(cfg), 1
        return self.slot_state(0)[1]

    def add_sampler(self, kind, steps=None, t_list=None, tables=None):
        """fdm_slot_sampler_add: one more sampler definition into the bank, between steps (kind / steps / t_list / tables as
        open_slots).  Returns its id >= 1; FdmError with code -4 when the bank has no room (the plan is untouched).  Drains the stream once."""
        a = SampleArgs()
        held = self._sampler_args(a, kind, steps, t_list, tables)
        with torch.cuda.device(self.device):
            rc = lib().fdm_slot_sampler_add(self.h, C.byref(a), _stream())
        del held
        if rc < 0:
            check(rc)
        return rc

    def drop_sampler(self, id):
        """fdm_slot_sampler_drop: frees a bank row; FdmError -4 while a running or unread slot names it, -1 for id 0 / unknown."""
        check(lib().fdm_slot_sampler_drop(self.h, int(id)))

    def sampler_info(self, id):
        """fdm_slot_sampler_info: (kind 0 DDPM / 1 DDIM / 2 table-driven, steps of a chain) of a bank row (host only)."""
        k, n = C.c_int(), C.c_int()
        check(lib().fdm_slot_sampler_info(self.h, int(id), C.byref(k), C.byref(n)))
        return k.value, n.value

    def admit(self, slot, hub, style=None, emo=None, x_T=None, L=None, seed=0, clip_id=0, sampler=0, cfg_scale=None, style_track=None,
              emotion_track=None):
        """fdm_slot_admit: one clip into an idle slot, between steps.  hub [N, fw] (or [1, N, fw]) audio-encoder features, style
        [n_style], emo [n_emo], x_T [L_clip*G, c] (or [1, ...]); L = latent frames of the clip (default N // pair).  Its latent will
        equal the solo sample_* call on a (1, L_clip) plan with the same x_T, seed and clip0 = clip_id -- with the sampler the
        request names (a bank id; 0 = the session's) and its cfg_scale (None = the session's)."""
        p, dv = self.p, self.device
        hub = _dev(hub, dv).reshape(-1, hub.shape[-1])
        N, fw = hub.shape
        L = N // p.pair if L is None else int(L)
        x = _dev(x_T, dv).reshape(-1)
        if x.numel() != L * p.d:
            raise FdmError(f"x_T has {x.numel()} elements, expected L_clip*G*c = {L * p.d}")
        if style_track is not None or emotion_track is not None:      # [L_clip, n] per-frame conditions (fdm_slot_admit_tracks)
            st, et = self._tracks(1, L, None if style is None else torch.as_tensor(style).reshape(-1),
                                  None if emo is None else torch.as_tensor(emo).reshape(-1), style_track, emotion_track)
            scale = self._slot_scale if cfg_scale is None else float(cfg_scale)
            with torch.cuda.device(dv):
                check(lib().fdm_slot_admit_tracks(self.h, int(slot), hub.data_ptr(), N, fw, st.data_ptr(), et.data_ptr() if et is not None else None,
                                                  L, x.data_ptr(), int(seed), int(clip_id), int(sampler), scale, _stream()))
            self._slot_inputs[int(slot)] = (hub, st, et, x)
            return L
        style = _dev(style, dv).reshape(-1)
        emo = _dev(emo, dv).reshape(-1) if (p.n_emo and emo is not None) else None
        with torch.cuda.device(dv):
            if sampler == 0 and cfg_scale is None:
                check(lib().fdm_slot_admit(self.h, int(slot), hub.data_ptr(), N, fw, style.data_ptr(), emo.data_ptr() if emo is not None else None,
                                           L, x.data_ptr(), int(seed), int(clip_id), _stream()))
            else:
                scale = self._slot_scale if cfg_scale is None else float(cfg_scale)
                check(lib().fdm_slot_admit_as(self.h, int(slot), hub.data_ptr(), N, fw, style.data_ptr(), emo.data_ptr() if emo is not None else None,
                                              L, x.data_ptr(), int(seed), int(clip_id), int(sampler), scale, _stream()))
        self._slot_inputs[int(slot)] = (hub, style, emo, x)      # read asynchronously on this stream: kept until the slot is admitted again
        return L

    def admit_long(self, slots, hub, style=None, emo=None, x_T=None, L_total=None, overlap=60, seed=0, clip_id=0, sampler=0, cfg_scale=None,
                   style_track=None, emotion_track=None):
        """fdm_slot_admit_long: a recording of L_total > L latent frames into the idle slots `slots`, one window each (slots[0] leads
        the group); len(slots) must be the window count of window_starts(L_total, L, overlap).  hub [N, fw] (or [1, N, fw]) features
        of the whole recording, x_T [L_total*G, c] (or [1, ...]).  Its latent will equal sample_windows on a B = 1 windowed plan
        (window = L, the same overlap, x_T, seed, clip0 = clip_id).  Drains the stream once.  Returns L_total."""
        p, dv = self.p, self.device
        hub = _dev(hub, dv).reshape(-1, hub.shape[-1])
        N, fw = hub.shape
        L_total = N // p.pair if L_total is None else int(L_total)
        x = _dev(x_T, dv).reshape(-1)
        if x.numel() != L_total * p.d:
            raise FdmError(f"x_T has {x.numel()} elements, expected L_total*G*c = {L_total * p.d}")
        ids = (C.c_int * len(slots))(*[int(s) for s in slots])
        if style_track is not None or emotion_track is not None:      # [L_total, n] per-frame conditions (fdm_slot_admit_long_tracks)
            st, et = self._tracks(1, L_total, None if style is None else torch.as_tensor(style).reshape(-1),
                                  None if emo is None else torch.as_tensor(emo).reshape(-1), style_track, emotion_track)
            scale = self._slot_scale if cfg_scale is None else float(cfg_scale)
            with torch.cuda.device(dv):
                check(lib().fdm_slot_admit_long_tracks(self.h, C.cast(ids, C.c_void_p), len(slots), hub.data_ptr(), N, fw, st.data_ptr(),
                                                       et.data_ptr() if et is not None else None, L_total, int(overlap), x.data_ptr(),
                                                       int(seed), int(clip_id), int(sampler), scale, _stream()))
            self._slot_inputs[int(slots[0])] = (hub, st, et, x)
            return L_total
        style = _dev(style, dv).reshape(-1)
        emo = _dev(emo, dv).reshape(-1) if (p.n_emo and emo is not None) else None
        with torch.cuda.device(dv):
            if sampler == 0 and cfg_scale is None:
                check(lib().fdm_slot_admit_long(self.h, C.cast(ids, C.c_void_p), len(slots), hub.data_ptr(), N, fw, style.data_ptr(),
                                                emo.data_ptr() if emo is not None else None, L_total, int(overlap), x.data_ptr(),
                                                int(seed), int(clip_id), _stream()))
            else:      # the request's own sampler (a bank id) and cfg_scale (None = the session's)
                scale = self._slot_scale if cfg_scale is None else float(cfg_scale)
                check(lib().fdm_slot_admit_long_as(self.h, C.cast(ids, C.c_void_p), len(slots), hub.data_ptr(), N, fw, style.data_ptr(),
                                                   emo.data_ptr() if emo is not None else None, L_total, int(overlap), x.data_ptr(),
                                                   int(seed), int(clip_id), int(sampler), scale, _stream()))
        self._slot_inputs[int(slots[0])] = (hub, style, emo, x)      # read asynchronously on this stream: kept until the leader's slot is admitted again
        return L_total

    def slot_group(self, slot):
        """fdm_slot_group: (leader, members, L_total) of the long request a slot belongs to; (-1, 0, 0) for a plain or idle slot."""
        a, n, lt = C.c_int(), C.c_int(), C.c_int()
        check(lib().fdm_slot_group(self.h, int(slot), C.byref(a), C.byref(n), C.byref(lt)))
        return a.value, n.value, lt.value

    def read_long(self, leader):
        """fdm_slot_read_long: the finished group's latent [1, L_total*G, c]; its slots, arena range and descriptor are free afterwards."""
        L_total = self.slot_group(leader)[2]
        out = torch.empty(1, max(L_total, 1) * self.p.G, self.p.c, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().fdm_slot_read_long(self.h, int(leader), out.data_ptr(), _stream()))
        return out

    def run(self, n_steps):
        """fdm_slots_run: n_steps diffusion steps for every running slot (a chain that ends part-way freezes there)."""
        with torch.cuda.device(self.device):
            check(lib().fdm_slots_run(self.h, int(n_steps), _stream()))

    def slot_state(self, slot):
        """(steps_done, steps_total, status) of a slot from the host mirror; status _lib.SLOT_IDLE / SLOT_RUNNING / SLOT_FINISHED."""
        d, t, st = C.c_int(), C.c_int(), C.c_int()
        check(lib().fdm_slot_state(self.h, int(slot), C.byref(d), C.byref(t), C.byref(st)))
        return d.value, t.value, st.value

    def read_slot(self, slot, L):
        """fdm_slot_read: the finished slot's latent [1, L*G, c] (L = the clip's frames, as admitted); the slot is idle afterwards."""
        out = torch.empty(1, int(L) * self.p.G, self.p.c, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().fdm_slot_read(self.h, int(slot), out.data_ptr(), _stream()))
        return out

    def peek_slot(self, slot):
        """fdm_slot_peek: all L rows of a slot's latent [1, L*G, c], whatever its status (inspection; changes nothing)."""
        out = torch.empty(1, self.L * self.p.G, self.p.c, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().fdm_slot_peek(self.h, int(slot), out.data_ptr(), _stream()))
        return out

    # ------------------------------------------------------------------------------------------
    def tune(self):
        """Tune the GEMM tiles for the prepared shape now (plan-time work).  Nothing else tunes: get("needs_tune") says when a
        shape has run 2000 steps untuned; only a caller that set "tune_lazy" lets a sampling call tune (once per shape)."""
        with torch.cuda.device(self.device):
            check(lib().fdm_plan_tune(self.h, _stream()))

    def get(self, key):
        v = C.c_longlong()
        check(lib().fdm_plan_get(self.h, key.encode(), C.byref(v)))
        return v.value

    def set(self, key, value):
        check(lib().fdm_plan_set(self.h, key.encode(), int(value)))

    @property
    def tiles(self):
        """Tile chosen per GEMM call site of the step (0 = library heuristic)."""
        return {k: self.get("tile." + k) for k in TILE_SITES}

    @property
    def fuse_ln3(self):
        return bool(self.get("fuse_ln3"))
