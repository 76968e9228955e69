"""GPU: windowed sampling of clips longer than max_len (fdm_audio_prepare_windows / fdm_sample_windows, csrc/window.hpp) and the
audio encoders / VQ decoder at long-clip lengths.

A one-window plan is bit-identical to the plain sampler; a windowed plan matches the windowed CPU oracle of
tests/test_long_audio_cpu.py (fp32 / f16x3 within the 1e-4 contract, bf16 / fp16 at the project's per-mode bars); the noise is keyed
by the long clip; overlapping rows stay bitwise equal across windows; the pipeline animates the whole clip."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd._lib import BF16, F16, F16X3, F32, FdmError, lib  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan, window_starts  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402
from test_long_audio_cpu import windowed_denoiser  # noqa: E402

DEV = "cuda:0"
TOL = {F32: 1e-4, F16X3: 1e-4, BF16: 8e-2, F16: 6e-3}       # tests/test_denoiser_gpu.py: the per-mode bars
_PLANS = {}


def mad(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def plan_for(preset, dtype):
    if (preset, dtype) not in _PLANS:
        w = W.make_fdm_weights(preset)
        _PLANS[(preset, dtype)] = (DenoiserPlan(preset, w, dtype, DEV), w)
    return _PLANS[(preset, dtype)]


def stream():
    return torch.cuda.current_stream().cuda_stream


def gather_windows(x_long, starts, Wf, G):
    B = x_long.shape[0]
    xl = x_long.reshape(B, -1, G * x_long.shape[-1])
    return torch.stack([xl[b, s:s + Wf] for b in range(B) for s in starts]).reshape(B * len(starts), Wf * G, -1)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,dtype,L", [("vocaset_tiny", F32, 37), ("vocaset_tiny", BF16, 37), ("vocaset", F32, 100), ("vocaset", BF16, 100)])
def test_one_window_is_bit_identical_to_the_plain_sampler(preset, dtype, L):
    plan, _ = plan_for(preset, dtype)
    inp = W.synth_inputs(preset, 2, L, seed=21)
    x = inp["x"].to(DEV)
    ts = [999, 700, 400, 100, 1, 0]
    plan.prepare(inp["hub"], inp["style"], L=L)
    ref_p = plan.sample_ddpm(x, ts, seed=5, clip0=2)
    ref_d = plan.sample_ddim(x, 10)
    assert plan.get("launches_per_step") == (58 if preset == "vocaset" else 2 * 7 + 2)
    starts = plan.prepare_windows(inp["hub"], inp["style"], L_total=L)
    assert starts == [0] and plan.get("windows") == 1 and plan.get("window_len") == L and plan.get("L_total") == L
    assert torch.equal(plan.sample_windows(x, "ddpm", t_list=ts, seed=5, clip0=2), ref_p)
    assert torch.equal(plan.sample_windows(x, "ddim", steps=10), ref_d)
    assert plan.get("launches_per_step") == (59 if preset == "vocaset" else 2 * 7 + 3)


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F16X3, BF16, F16])
@pytest.mark.parametrize("window,overlap", [(40, 10), (40, 30)])
def test_windowed_ddpm_matches_the_windowed_oracle(dtype, window, overlap):
    preset, L_total, B = "vocaset_tiny", 100, 2
    plan, w = plan_for(preset, dtype)
    inp = W.synth_inputs(preset, B, L_total, seed=22)
    ts = list(range(999, 0, -50))[:19] + [0]                                # 20 steps, the last one noise-free
    noise = torch.randn(len(ts), *inp["x"].shape, generator=torch.Generator().manual_seed(3))
    starts = plan.prepare_windows(inp["hub"], inp["style"], L_total=L_total, window=window, overlap=overlap)
    assert starts == window_starts(L_total, window, overlap) and plan.B == B * len(starts)
    out = plan.sample_windows(inp["x"].to(DEV), "ddpm", t_list=ts, noise=noise)
    ref = FO.p_sample_loop(windowed_denoiser(w, preset, inp["hub"], inp["style"], None, L_total, window, overlap),
                           inp["x"].clone(), noise, ts)
    err = mad(out, ref)
    print(f"[windowed ddpm dtype {dtype} W {window} O {overlap}] max-abs vs oracle {err:.2e}")
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", [F32, F16X3])
def test_windowed_cfg_ddim_matches_the_windowed_oracle_mead(dtype):
    preset, L_total, window, overlap = "mead_tiny", 100, 40, 10
    plan, w = plan_for(preset, dtype)
    inp = W.synth_inputs(preset, 1, L_total, seed=23)
    plan.prepare_windows(inp["hub"], inp["style"], inp["emo"], L_total=L_total, window=window, overlap=overlap, cfg=True)
    out = plan.sample_windows(inp["x"].to(DEV), "ddim", steps=8, cfg_scale=2.5)
    den = windowed_denoiser(w, preset, inp["hub"], inp["style"], inp["emo"], L_total, window, overlap, cfg_scale=2.5)
    err = mad(out, FO.ddim_sample(den, inp["x"].clone(), 8))
    print(f"[windowed cfg ddim mead_tiny dtype {dtype}] max-abs vs oracle {err:.2e}")
    assert err < 1e-4


# 3 ---------------------------------------------------------------------------------------------
def test_noise_is_keyed_by_the_long_clip():
    """c1 = c2 = 0, sigma = 1: one DDPM step returns its noise draw z.  The windowed plan's long output equals a plain plan's on
    the same long clips (L_total <= max_len) bit for bit: one draw per long-clip element, keyed like the plain sampler's."""
    preset, L_total, B = "vocaset_tiny", 100, 2
    plan = DenoiserPlan(preset, W.make_fdm_weights(preset), F32, DEV)
    for name, v in (("sched.c1", 0.0), ("sched.c2", 0.0), ("sched.sigma", 1.0)):
        t = torch.full((1000,), v)
        assert lib().fdm_plan_set_weights(plan.h, name.encode(), t.data_ptr(), 1000, stream()) == 0
    torch.cuda.synchronize()
    inp = W.synth_inputs(preset, B, L_total, seed=24)
    x = inp["x"].to(DEV)
    plan.prepare(inp["hub"], inp["style"], L=L_total)
    z = plan.sample_ddpm(x, [500], seed=11, clip0=3)
    assert float(z.std()) > 0.5 and not torch.equal(z[0], z[1])
    plan.prepare_windows(inp["hub"], inp["style"], L_total=L_total, window=40, overlap=10)
    assert plan.get("windows") == 3
    assert torch.equal(plan.sample_windows(x, "ddpm", t_list=[500], seed=11, clip0=3), z)


# 4 ---------------------------------------------------------------------------------------------
def test_seams_bitwise_equal_and_graph_modes_agree():
    preset, L_total, window, overlap = "vocaset_tiny", 100, 40, 30
    plan, _ = plan_for(preset, BF16)
    inp = W.synth_inputs(preset, 2, L_total, seed=25)
    x = inp["x"].to(DEV)
    starts = plan.prepare_windows(inp["hub"], inp["style"], L_total=L_total, window=window, overlap=overlap)
    ts = list(range(990, -1, -90))[:11] + [0]
    rec = []
    ref = plan.sample_windows(x, "ddpm", t_list=ts, seed=4, record=rec)
    assert len(rec) == len(ts) and torch.equal(rec[-1], ref)
    for kw in (dict(use_graph=False), dict(graph_steps=1), dict(graph_steps=10)):
        assert torch.equal(plan.sample_windows(x, "ddpm", t_list=ts, seed=4, **kw), ref), kw
    G = plan.p.G
    # the windows' rows of every recorded step are gathers of the long latent, so their overlaps agree bit for bit; the
    # per-window denoiser view (fdm_denoise_step, plan layout, no blend) equals a plain plan's call on the same window rows
    xs = gather_windows(rec[3], starts, window, G)
    for i, s in enumerate(starts[1:], 1):
        ov = starts[i - 1] + window - s
        a = xs[i - 1].reshape(window, -1)[window - ov:]
        b = xs[i].reshape(window, -1)[:ov]
        assert torch.equal(a, b)
    x0w = plan.denoise(xs, ts[4])
    plain = DenoiserPlan(preset, W.make_fdm_weights(preset), BF16, DEV)
    hub = torch.stack([inp["hub"][b, s:s + window] for b in range(2) for s in starts])
    plain.prepare(hub, inp["style"].repeat_interleave(len(starts), 0), L=window)
    assert torch.equal(plain.denoise(xs, ts[4]), x0w)


# 5 ---------------------------------------------------------------------------------------------
def test_full_size_27s_bf16_ddim():
    import time
    preset, L_total = "vocaset", 1350
    plan, _ = plan_for(preset, BF16)
    g = torch.Generator().manual_seed(26)
    hub = torch.randn(1, L_total, 1024, generator=g)
    style = torch.eye(8)[:1]
    x = torch.randn(1, L_total * 16, 64, generator=g)
    starts = plan.prepare_windows(hub, style, L_total=L_total)
    assert len(starts) == 3 and plan.get("rows") == 1800
    plan.sample_windows(x, "ddim", steps=10)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = plan.sample_windows(x, "ddim", steps=10)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert out.shape == x.shape and bool(torch.isfinite(out).all())
    assert plan.get("launches_per_step") == 59
    print(f"[full vocaset L_total {L_total}, 3 windows, bf16] DDIM 10 in {dt * 1e3:.1f} ms ({dt * 1e2:.2f} ms / step)")
    plan.prepare(hub, style, L=600)
    plan.sample_ddim(x[:, :600 * 16], 2)
    assert plan.get("launches_per_step") == 58 and plan.get("windows") == 0


# 6 ---------------------------------------------------------------------------------------------
def test_hubert_45s_vs_oracle():
    from fdm_amd.hubert import HubertPlan
    from oracle import hubert_oracle as HO
    w = W.make_hubert_weights(2)
    wav = HO.processor_normalize(torch.randn(45 * 16000, generator=torch.Generator().manual_seed(27)) * 0.1)
    ref = HO.hubert_forward(w, wav.unsqueeze(0), n_layers=2)[0]
    assert ref.shape[0] >= 2240
    for dtype in (F32, F16X3):
        out = HubertPlan(w, 2, dtype, DEV).forward(wav)[0]
        err = mad(out, ref)
        print(f"[hubert 2 layers, 45 s = {ref.shape[0]} frames, dtype {dtype}] max-abs vs oracle {err:.2e}")
        assert out.shape == ref.shape and err < 1e-4


def test_vq_decode_1350_frames_vs_oracle():
    from fdm_amd.vq import VQPlan
    from oracle import vq_oracle as VO
    w = W.make_vq_weights("vocaset")
    z = torch.randn(1, 1350 * 16, 64, generator=torch.Generator().manual_seed(28)) * (1.5 / 256)
    zq, _ = VO.quant(w, "vocaset", z)
    ref = VO.decode(w, "vocaset", zq)
    out = VQPlan("vocaset", w, F32, DEV).decode(zq.to(DEV))
    err = mad(out, ref)
    print(f"[vq decode L 1350] max-abs vs oracle {err:.2e}")
    assert out.shape == ref.shape == (1, 1350, 15069) and err < 1e-4


# 7 ---------------------------------------------------------------------------------------------
def test_pipeline_animate_long(tmp_path):
    from scipy.io import wavfile
    from fdm_amd import pipeline
    diffusion, ae = pipeline.build_models("vocaset", None, DEV)
    g = torch.Generator().manual_seed(29)
    wav30 = pipeline.processor_normalize((torch.randn(30 * 16000, generator=g) * 0.1).numpy(), pad_seconds=0)
    v_long, lat_long = pipeline.animate_long(diffusion, ae, wav30, ddim_steps=4, seed=1, device=DEV)
    hub_frames = diffusion.denoise_fn.audio_features(torch.as_tensor(wav30, device=DEV).unsqueeze(0)).shape[1]
    assert hub_frames // 1 > 600 and v_long.shape == (1, hub_frames, 15069) and lat_long.shape == (1, hub_frames * 16, 64)
    assert bool(torch.isfinite(v_long).all())
    v_crop, _ = pipeline.animate(diffusion, ae, wav30, ddim_steps=4, seed=1, device=DEV)
    assert v_crop.shape == (1, 600, 15069)                                    # animate() keeps the reference's crop
    wav5 = pipeline.processor_normalize((torch.randn(5 * 16000, generator=g) * 0.1).numpy(), pad_seconds=0)
    a, la = pipeline.animate(diffusion, ae, wav5, ddim_steps=5, seed=2, device=DEV)
    b, lb = pipeline.animate_long(diffusion, ae, wav5, ddim_steps=5, seed=2, device=DEV)
    assert torch.equal(la, lb) and torch.equal(a, b)
    a2, _ = pipeline.animate(diffusion, ae, wav5, ddim_steps=5, seed=2, device=DEV)     # the cached plan state was left behind cleanly
    assert torch.equal(a2, a)
    pcm = (np.random.default_rng(1).standard_normal(14 * 16000) * 3000).astype(np.int16)
    wp = str(tmp_path / "long.wav")
    wavfile.write(wp, 16000, pcm)
    dst = pipeline.demo_main("vocaset", ["--audio_file", wp, "--audio_path", str(tmp_path / "result"), "--ddim_steps", "3",
                                         "--long_audio", "window", "--window_overlap", "40"])
    arr = np.load(dst)
    # 14 s + 1 s of zero pad = 240000 samples -> 748 HuBERT frames, all of them animated (truncate would keep 600)
    assert arr.shape == (1, 748, 15069) and np.isfinite(arr).all()


# 8 ---------------------------------------------------------------------------------------------
def test_validation_and_mode_switches():
    preset = "vocaset_tiny"
    plan, _ = plan_for(preset, F32)
    inp = W.synth_inputs(preset, 1, 80, seed=30)
    hub, style = inp["hub"].to(DEV), inp["style"].to(DEV)
    l, s = lib(), stream()
    assert l.fdm_audio_prepare_windows(plan.h, hub.data_ptr(), 1, 80, 1024, style.data_ptr(), None, 80, 601, 60, 0, s) == -2
    assert l.fdm_audio_prepare_windows(plan.h, hub.data_ptr(), 1, 80, 1024, style.data_ptr(), None, 80, 40, 40, 0, s) == -1
    assert l.fdm_audio_prepare_windows(plan.h, hub.data_ptr(), 1, 80, 1024, style.data_ptr(), None, 81, 40, 10, 0, s) == -2
    plan.prepare_windows(inp["hub"], inp["style"], L_total=80, window=40, overlap=10)
    assert plan.get("windows") == 3
    with pytest.raises(FdmError, match="windowed"):
        plan.sample_ddim(torch.zeros(3, 40 * 16, 16, device=DEV), 4)
    plan.prepare(inp["hub"], inp["style"], L=80)
    assert plan.get("windows") == 0 and plan.get("L_total") == 80
    assert plan.sample_ddim(inp["x"].to(DEV), 4).shape == inp["x"].shape
    with pytest.raises(FdmError, match="prepare_windows"):
        plan.sample_windows(inp["x"].to(DEV), "ddim", steps=4)
