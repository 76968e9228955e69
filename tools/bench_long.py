"""Long-audio throughput on one MI355X: 60 s of audio on the VOCASET preset (~3 000 latent frames) through windowed sampling
(fdm_audio_prepare_windows / fdm_sample_windows: windows of 600 frames, overlap 60) -> HuBERT once over the whole waveform ->
DDIM -> quant -> decode of the whole clip.  Per operand kind: frames/s end to end and per stage, ms per diffusion step of the
windowed plan next to a plain plan with the same rows (the blend pass's cost), and launches_per_step of both.

  python tools/bench_long.py [--secs 60] [--ddim 100] [--dtypes bf16,f16x3] [--json out.json]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "face-diffusion-model_amd"))
from fdm_amd import schedule, synth  # noqa: E402
from fdm_amd._lib import BF16, F16X3, F32  # noqa: E402
from fdm_amd.denoiser import DenoiserPlan  # noqa: E402
from fdm_amd.hubert import HubertPlan  # noqa: E402
from fdm_amd.vq import VQPlan  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) / reps


def run(dtype_name, secs, ddim, window, overlap):
    dt = {"bf16": BF16, "f16x3": F16X3, "f32": F32}[dtype_name]
    hub_plan = HubertPlan(synth.make_hubert_weights(24), 24, dt, DEV)
    den = DenoiserPlan("vocaset", synth.make_fdm_weights("vocaset"), dt, DEV)
    vq = VQPlan("vocaset", synth.make_vq_weights("vocaset"), F32 if dt == F16X3 else dt, DEV)
    g = torch.Generator().manual_seed(0)
    wav = (torch.randn(1, int(secs * 16000), generator=g) * 0.1).to(DEV)
    hub_plan.forward(wav)                                                  # warm-up (workspaces)
    hub, t_h = timed(lambda: hub_plan.forward(wav))
    L_total = hub.shape[1]
    sty = torch.eye(8)[:1]
    den.prepare_windows(hub, sty, L_total=L_total, window=window, overlap=overlap)
    starts, t_p = timed(lambda: den.prepare_windows(hub, sty, L_total=L_total, window=window, overlap=overlap))
    n, rows = len(starts), den.get("rows")
    xT = torch.randn(1, L_total * 16, 64, generator=g).to(DEV)
    den.sample_windows(xT, "ddim", steps=ddim)                             # graph instantiation
    lat, t_s = timed(lambda: den.sample_windows(xT, "ddim", steps=ddim))
    lps_win = den.get("launches_per_step")
    steps = sum(1 for pr in schedule.ddim_time_pairs(ddim) if pr[1] >= 0)     # live DDIM pairs (the dead last pair is skipped)
    lat = lat * (1.5 / 256 / 4)
    vq.decode(vq.quant(lat)[0])
    (zq, _), t_q = timed(lambda: vq.quant(lat))
    verts, t_d = timed(lambda: vq.decode(zq))
    assert verts.shape[1] == L_total and bool(torch.isfinite(verts).all())
    # a plain plan with the same rows: the windows' audio as ordinary clips, no blend pass (the scheduler fused into the decoder GEMM)
    hw = torch.cat([hub[:, s:s + window] for s in starts])
    den.prepare(hw, sty.expand(n, -1), L=window)
    xw = torch.randn(n, window * 16, 64, generator=g).to(DEV)
    den.sample_ddim(xw, ddim)
    _, t_plain = timed(lambda: den.sample_ddim(xw, ddim))
    lps_plain = den.get("launches_per_step")
    tot = t_h + t_p + t_s + t_q + t_d
    res = dict(dtype=dtype_name, secs=secs, L_total=L_total, windows=n, window=window, overlap=overlap, rows=rows, ddim=ddim,
               live_steps=steps,
               ms=dict(hubert=t_h * 1e3, prepare=t_p * 1e3, sample=t_s * 1e3, quant=t_q * 1e3, decode=t_d * 1e3, total=tot * 1e3),
               frames_per_s=dict(end_to_end=L_total / tot, hubert=L_total / t_h, prepare=L_total / t_p, sample=L_total / t_s,
                                 quant=L_total / t_q, decode=L_total / t_d),
               ms_per_step_windowed=t_s * 1e3 / steps, ms_per_step_plain_same_rows=t_plain * 1e3 / steps,
               launches_per_step_windowed=lps_win, launches_per_step_plain=lps_plain)
    print(f"[{dtype_name}] {secs:.0f} s audio -> L_total {L_total} frames, {n} windows x {window} (overlap >= {overlap}) = {rows} rows, DDIM {ddim}")
    for k in ("hubert", "prepare", "sample", "quant", "decode", "total"):
        fps = res["frames_per_s"]["end_to_end" if k == "total" else k]
        print(f"  {k:10s} {res['ms'][k]:10.2f} ms   {fps:12.1f} frames/s")
    print(f"  per diffusion step: windowed {res['ms_per_step_windowed']:.3f} ms ({lps_win} launches), plain plan at {rows} rows "
          f"{res['ms_per_step_plain_same_rows']:.3f} ms ({lps_plain} launches)")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--secs", type=float, default=60.0)
    ap.add_argument("--ddim", type=int, default=100)
    ap.add_argument("--window", type=int, default=600)
    ap.add_argument("--overlap", type=int, default=60)
    ap.add_argument("--dtypes", type=str, default="bf16,f16x3")
    ap.add_argument("--json", type=str, default=None)
    a = ap.parse_args()
    out = [run(d, a.secs, a.ddim, a.window, a.overlap) for d in a.dtypes.split(",")]
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
