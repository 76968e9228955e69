"""GPU: the table-driven multistep sampler (fdm_sched_args mode 3, fdm_sample_args kind 2: DPM-Solver++ 2M and DDIM with eta).

x' = a[k] x + b[k] x0 + c[k] x0_prev + s[k] z in sched_kernel, in the latent-decoder GEMM's fused epilogue and in
window_sched_kernel: bit-equal to the same expression in torch fp32 at the operator, bit-equal to the DDPM sampler when given
DDPM's coefficients, within the project's 1e-4 contract of the CPU oracle over whole chains (fp32 and split-fp16 modes), and
without any effect on the DDPM / DDIM programs of the same plan.  Tiny presets and short clips throughout (L = 31 crosses the
period-30 positional table and ALiBi mask); one full-size case."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fdm_amd import ops, schedule  # noqa: E402
from fdm_amd._lib import BF16, F16, F16X3, F32  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from oracle import fdm_oracle as FO  # noqa: E402
from oracle import weights as W  # noqa: E402
from test_long_audio_cpu import windowed_denoiser  # noqa: E402

DEV = "cuda:0"
TOL32 = 1e-4                     # the contract's bar (tests/test_denoiser_gpu.py); the existing chains sit at 3 to 7e-6
PARITY_MODES = [F32, F16X3]
_PLANS, _REFS = {}, {}


def mad(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def plan_for(preset, dtype):
    if (preset, dtype) not in _PLANS:
        w = W.make_fdm_weights(preset)
        _PLANS[(preset, dtype)] = (DenoiserPlan(preset, w, dtype, DEV), w)
    return _PLANS[(preset, dtype)]


def tables_loop(den, x_T, t_list, tab, noise=None):
    """The sampler restated: fp32 torch on the CPU, the library's expression order.  Returns the latent after every step."""
    x, prev, rec = x_T.clone(), torch.zeros_like(x_T), []
    a, b, c, s = tab
    for k, t in enumerate(t_list):
        x0 = den(x, int(t))
        o = b[k] * x0 + a[k] * x
        if float(c[k]) != 0:
            o = o + c[k] * prev
        if float(s[k]) != 0:
            o = o + s[k] * noise[k]
        x, prev = o, x0
        rec.append(x.clone())
    return torch.stack(rec)


def oracle_den(w, preset, inp, scale=None):
    if scale is not None:
        return lambda x, t: FO.fdm_forward_cfg(w, preset, inp["hub"], t, x, inp["style"], inp["emo"], scale, folded=True)
    return lambda x, t: FO.fdm_forward(w, preset, inp["hub"], t, x, inp["style"], inp.get("emo"), folded=True)


# 1 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 2 * 1028])
def test_op_sched_step_mode3_is_bit_equal_to_the_torch_expression(n):
    g = torch.Generator().manual_seed(12)
    x0, x0u, x, h = [torch.randn(n, generator=g) * 2 for _ in range(4)]
    noise = torch.randn(3, n, generator=g)
    # step 0: c = 0, s = 0; step 1: c != 0; step 2: c != 0 and s != 0 (injected noise)
    a, b = torch.tensor([0.9518, 0.853, 0.7313]), torch.tensor([0.3067, 0.3352, 0.5269])
    c, s = torch.tensor([0.0, -0.013, -0.1491]), torch.tensor([0.0, 0.0, 0.4338])
    dv = lambda t: t.to(DEV)
    for k in range(3):
        for cfg in (False, True):
            for adv in (0, 1):
                step = torch.tensor([k], dtype=torch.int32, device=DEV)
                hist, out = dv(h.clone()), torch.zeros(n, device=DEV)
                ops.sched_step(3, dv(x0), dv(x), out, n, x0u=dv(x0u) if cfg else None, cfg_scale=2.5, n_per_clip=n // 2, step=step,
                               advance=adv, lm_a=dv(a), lm_b=dv(b), lm_c=dv(c), lm_s=dv(s), x0_hist=hist, noise=dv(noise))
                mix = x0u + 2.5 * (x0 - x0u) if cfg else x0
                ref = b[k] * mix + a[k] * x
                if float(c[k]) != 0:
                    ref = ref + c[k] * h
                if float(s[k]) != 0:
                    ref = ref + s[k] * noise[k]
                torch.cuda.synchronize()
                assert torch.equal(out.cpu(), ref), (k, cfg, adv)
                assert torch.equal(hist.cpu(), mix), (k, cfg, adv)           # the history holds the (mixed) x0 afterwards
                assert int(step[0]) == k + adv


# 2 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PARITY_MODES)
@pytest.mark.parametrize("preset,cfg", [("vocaset_tiny", False), ("mead_tiny", True)])
def test_ddpm_through_the_tables_is_ddpm(preset, cfg, dtype):
    """a = c2[t], b = c1[t], c = 0, s = sigma[t] (0 at t = 0): the fused epilogue (no guidance) and sched_kernel (guidance)."""
    plan, _ = plan_for(preset, dtype)
    L = 7
    inp = W.synth_inputs(preset, 2, L, seed=31)
    plan.prepare(inp["hub"], inp["style"], inp.get("emo"), L=L, cfg=cfg)
    ts = list(range(9, -1, -1))
    c1, c2, sg = schedule.ddpm_tables(schedule.make_buffers(1000))
    idx = torch.tensor(ts)
    s = sg[idx].clone()
    s[-1] = 0.0
    tab = torch.stack([c2[idx], c1[idx], torch.zeros(len(ts)), s])
    noise = torch.randn(len(ts), *inp["x"].shape, generator=torch.Generator().manual_seed(2))
    ref = plan.sample_ddpm(inp["x"].to(DEV), ts, noise=noise)
    n_ddpm = plan.get("launches_per_step")
    assert cfg or n_ddpm == 2 * 7 + 2
    out = plan.sample_tables(inp["x"].to(DEV), ts, tab, noise=noise)
    assert plan.get("launches_per_step") == n_ddpm                           # DDPM's launch count (one more under guidance)
    assert torch.equal(out, ref)


# 3, 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PARITY_MODES)
def test_ddim_eta0_tracks_sample_ddim_and_eta1_the_restatement(dtype):
    preset, L = "vocaset_tiny", 7
    plan, w = plan_for(preset, dtype)
    inp = W.synth_inputs(preset, 2, L, seed=32)
    plan.prepare(inp["hub"], inp["style"], L=L)
    x = inp["x"].to(DEV)
    rec_ref, rec = [], []
    plan.sample_ddim(x, 3, record=rec_ref)
    t, tab = schedule.sampler_tables("ddim_eta", 3, 0.0)
    plan.sample_tables(x, t, tab, record=rec)
    assert len(rec_ref) == 2 and len(rec) == 3
    err = mad(torch.stack(rec[:2]), torch.stack(rec_ref))
    print(f"[ddim eta=0 dtype {dtype}] first 2 latents vs sample_ddim {err:.2e}")
    assert err < TOL32
    t, tab = schedule.sampler_tables("ddim_eta", 4, 1.0)
    noise = torch.randn(4, *inp["x"].shape, generator=torch.Generator().manual_seed(5))
    if "eta1" not in _REFS:
        _REFS["eta1"] = tables_loop(oracle_den(w, preset, inp), inp["x"], t, tab, noise)
    rec = []
    plan.sample_tables(x, t, tab, noise=noise, record=rec)
    err = mad(torch.stack(rec), _REFS["eta1"])
    print(f"[ddim eta=1 dtype {dtype}] every step vs the restatement {err:.2e}")
    assert err < TOL32


# 5 ---------------------------------------------------------------------------------------------
CASES_2M = [("vocaset_tiny", 7, 3, None), ("vocaset_tiny", 7, 8, None), ("vocaset_tiny", 31, 3, None), ("vocaset_tiny", 31, 8, None),
            ("mead_tiny", 7, 8, 2.5), ("vocaset", 30, 3, None)]


@pytest.mark.parametrize("dtype", PARITY_MODES + [BF16, F16])
@pytest.mark.parametrize("preset,L,steps,scale", CASES_2M)
def test_dpmpp_2m_against_the_oracle(preset, L, steps, scale, dtype):
    plan, w = plan_for(preset, dtype)
    B = 1 if preset == "vocaset" else 2
    inp = W.synth_inputs(preset, B, L, seed=33 + L)
    t, tab = schedule.sampler_tables("dpmpp2m", steps)
    key = (preset, L, steps)
    if key not in _REFS:
        _REFS[key] = tables_loop(oracle_den(w, preset, inp, scale), inp["x"], t, tab)
    plan.prepare(inp["hub"], inp["style"], inp.get("emo"), L=L, cfg=scale is not None)
    rec = []
    out = plan.sample_tables(inp["x"].to(DEV), t, tab, cfg_scale=scale or 2.5, record=rec)
    assert torch.equal(out, rec[-1])
    err = mad(torch.stack(rec), _REFS[key])
    print(f"[2M {preset} L {L} steps {steps} dtype {dtype}] every step vs the oracle {err:.2e}")
    if dtype in PARITY_MODES:
        assert err < TOL32
    else:
        assert torch.isfinite(out).all()


# 6, 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_graph_equals_eager_and_clips_are_batch_independent(dtype):
    preset, L = "vocaset_tiny", 31
    plan, _ = plan_for(preset, dtype)
    inp = W.synth_inputs(preset, 2, L, seed=34)
    x = inp["x"].to(DEV)
    runs = [schedule.sampler_tables("dpmpp2m", 8), schedule.sampler_tables("ddim_eta", 8, 0.5)]      # the second draws Philox noise
    plan.prepare(inp["hub"], inp["style"], L=L)
    both = []
    for t, tab in runs:
        a = plan.sample_tables(x, t, tab, seed=11, graph_steps=3)          # 2 launches of 3 steps + a remainder of 2
        assert plan.get("graph_launches") == 4
        b = plan.sample_tables(x, t, tab, seed=11, use_graph=False)
        assert torch.equal(a, b)
        assert torch.equal(a, plan.sample_tables(x, t, tab, seed=11))      # one graph launch of 8 steps
        both.append(a)
    assert not torch.equal(both[1], plan.sample_tables(x, *runs[1], seed=12))
    for i in range(2):
        plan.prepare(inp["hub"][i:i + 1], inp["style"][i:i + 1], L=L)
        for (t, tab), full in zip(runs, both):
            one = plan.sample_tables(x[i:i + 1], t, tab, seed=11, clip0=i)
            assert torch.equal(one[0], full[i]), i


# 8 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PARITY_MODES)
def test_constant_predictor_chain_ends_in_the_constant(dtype):
    """latent_decoder.weight = 0, bias = beta: every x0 prediction is beta, and the final pair (a = 0, b = 1) returns it bit
    for bit -- after four steps that mixed the history in."""
    preset, L = "vocaset_tiny", 7
    w = dict(W.make_fdm_weights(preset))
    beta = torch.randn(w["latent_decoder.bias"].shape, generator=torch.Generator().manual_seed(8))
    w["latent_decoder.weight"] = torch.zeros_like(w["latent_decoder.weight"])
    w["latent_decoder.bias"] = beta
    plan = DenoiserPlan(preset, w, dtype, DEV)
    inp = W.synth_inputs(preset, 2, L, seed=35)
    plan.prepare(inp["hub"], inp["style"], L=L)
    t, tab = schedule.sampler_tables("dpmpp2m", 5)
    rec = []
    out = plan.sample_tables(inp["x"].to(DEV), t, tab, record=rec)
    assert torch.equal(out.cpu().reshape(2, L, -1), beta.expand(2, L, -1))
    assert not torch.equal(rec[3].cpu().reshape(2, L, -1), beta.expand(2, L, -1))      # still on the way at step 4
    # the same chain in fp32 torch, with the constant predictor: the history indexing is what the restatement's is
    ref = tables_loop(lambda x, tt: beta.expand(2, L, -1).reshape(x.shape), inp["x"], t, tab)
    assert torch.equal(torch.stack(rec).cpu(), ref)


# 9 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", PARITY_MODES)
def test_windows(dtype):
    preset = "vocaset_tiny"
    plan, w = plan_for(preset, dtype)
    L = 31
    inp = W.synth_inputs(preset, 2, L, seed=36)
    x = inp["x"].to(DEV)
    runs = [schedule.sampler_tables("dpmpp2m", 5), schedule.sampler_tables("ddim_eta", 5, 0.5)]
    plan.prepare(inp["hub"], inp["style"], L=L)
    plain = [plan.sample_tables(x, t, tab, seed=3, clip0=1) for t, tab in runs]
    assert plan.prepare_windows(inp["hub"], inp["style"], L_total=L) == [0]
    for (t, tab), ref in zip(runs, plain):                                  # one window: the plain sampler, bit for bit
        assert torch.equal(plan.sample_windows(x, "tables", t_list=t, tables=tab, seed=3, clip0=1), ref)
    assert plan.get("launches_per_step") == 2 * 7 + 3
    L_total, window, overlap = 40, 24, 8
    inp = W.synth_inputs(preset, 2, L_total, seed=37)
    t, tab = runs[0]
    if "win" not in _REFS:
        _REFS["win"] = tables_loop(windowed_denoiser(w, preset, inp["hub"], inp["style"], None, L_total, window, overlap), inp["x"], t, tab)
    starts = plan.prepare_windows(inp["hub"], inp["style"], L_total=L_total, window=window, overlap=overlap)
    assert len(starts) == 2
    rec = []
    plan.sample_windows(inp["x"].to(DEV), "tables", t_list=t, tables=tab, record=rec)
    err = mad(torch.stack(rec), _REFS["win"])
    print(f"[2M windows dtype {dtype}] every step vs the blended restatement {err:.2e}")
    assert err < TOL32


# 10 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,cfg", [("vocaset_tiny", False), ("mead_tiny", True)])
def test_ddpm_and_ddim_programs_are_untouched_by_a_table_call(preset, cfg):
    plan, _ = plan_for(preset, F32)
    L = 31
    inp = W.synth_inputs(preset, 2, L, seed=38)
    x = inp["x"].to(DEV)
    plan.prepare(inp["hub"], inp["style"], inp.get("emo"), L=L, cfg=cfg)
    ts = [999, 600, 300, 1, 0]
    before = (plan.sample_ddpm(x, ts, seed=9), plan.sample_ddim(x, 5))
    t, tab = schedule.sampler_tables("ddim_eta", 6, 1.0)
    assert torch.isfinite(plan.sample_tables(x, t, tab, seed=77, clip0=3)).all()
    assert torch.equal(plan.sample_ddpm(x, ts, seed=9), before[0])
    assert torch.equal(plan.sample_ddim(x, 5), before[1])


# 11 --------------------------------------------------------------------------------------------
def test_pipeline_sampler_keyword():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "dropin"))
    from fdm_amd import pipeline
    from oracle import hubert_oracle as HO
    wav = HO.processor_normalize(torch.randn(16000, generator=torch.Generator().manual_seed(6)) * 0.1).numpy()
    # (the VQ stage fixes G * c = 1024, so the pipeline has no tiny preset: the full VOCASET geometry on one second of audio)
    diffusion, ae = pipeline.build_models("vocaset", device=DEV)
    out, lat = pipeline.animate(diffusion, ae, wav, seed=4, device=DEV, sampler="dpmpp2m", sampler_steps=8)
    # the manual composition: plan -> table sampler -> quant -> decode
    model, p = diffusion.denoise_fn, diffusion.denoise_fn.preset
    audio = torch.as_tensor(wav, dtype=torch.float32, device=DEV).unsqueeze(0)
    L = min(model.audio_features(audio).shape[1] // p.pair, p.max_len)
    ids = torch.eye(p.n_style)[:1].to(DEV)
    plan = model.prepare(audio, L, ids)
    t, tab = schedule.sampler_tables("dpmpp2m", 8)
    x_T = torch.randn((1, L * p.G, p.c), generator=torch.Generator(device="cpu").manual_seed(4))
    lat2 = plan.sample_tables(x_T, t, tab, seed=4)
    assert torch.equal(lat, lat2) and torch.isfinite(lat).all()
    assert torch.equal(out, ae.decode(ae.quant(lat2, stats=False)[0]))
    # without the keyword: today's path, and sampler=None is that path
    a = pipeline.animate(diffusion, ae, wav, ddim_steps=3, seed=4, device=DEV)
    b = pipeline.animate(diffusion, ae, wav, ddim_steps=3, seed=4, device=DEV, sampler=None)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], lat)
    c = pipeline.animate(diffusion, ae, wav, seed=4, device=DEV, sampler="ddim_eta", sampler_steps=4, eta=0.5)
    assert torch.isfinite(c[0]).all() and c[0].shape == out.shape
