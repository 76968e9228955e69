"""Clips of unequal length: ONE ragged call against the per-clip loop of the same build, same process, alternating, HIP events.

    python tools/bench_ragged.py [--stage encoders,vq,e2e] [--dtypes bf16,f16x3] [--reps 20] [--warmup 3]

Eight clips of 3 ... 10 s at unequal lengths.  One JSON line per measurement: median and min..max in ms of both forms.
  encoders  HuBERT-large (24 layers) and wav2vec2-base (12): HubertPlan.forward_ragged against forward() per clip
  vq        VQPlan.decode_ragged against decode() per clip, on the clips' latent frame counts (30 per second)
  e2e       pipeline.animate_many on the eight waveforms, sampler="dpmpp2m" (20 steps) and DDIM 100, batch_stages on against off.
            On a build whose animate_many has no batch_stages argument (the parent commit) only the off path is timed: run this
            file from the new tree against the old one with PYTHONPATH to show that the off path did not move."""
import argparse
import inspect
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd"), os.path.join(ROOT, "face-diffusion-model_amd", "dropin")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SECONDS = [3.0, 4.1, 5.3, 6.2, 7.4, 8.0, 9.1, 10.0]
DEV = "cuda:0"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(forms, reps, warmup):
    """forms: {name: callable}; every repetition runs each form once, in turn.  -> {name: {median, min, max}} in ms."""
    for _ in range(warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(reps):
        for k, fn in forms.items():
            t[k].append(timed(fn))
    return {k + "_ms": {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in t.items()}


def waveforms():
    g = torch.Generator().manual_seed(1)
    return [torch.randn(int(s * 16000), generator=g) * 0.1 for s in SECONDS]


def encoders(a):
    from fdm_amd._lib import DTYPE_NAMES
    from fdm_amd.hubert import WAV2VEC2_BASE, HubertPlan
    from oracle import weights as W
    wavs = [w.to(DEV) for w in waveforms()]
    for name, make, layers, cfg in (("hubert-large", W.make_hubert_weights, 24, None), ("wav2vec2-base", W.make_wav2vec_weights, 12, WAV2VEC2_BASE)):
        w = make(layers)
        for dt in a.dtypes.split(","):
            plan = HubertPlan(w, layers, DTYPE_NAMES[dt], DEV, **({"cfg": cfg} if cfg else {}))
            res = alternate({"ragged": lambda: plan.forward_ragged(wavs), "per_clip": lambda: [plan.forward(x) for x in wavs]}, a.reps, a.warmup)
            print(json.dumps({"stage": name, "dtype": dt, "seconds": SECONDS, "reps": a.reps, **res}), flush=True)
            del plan


def vq(a):
    from fdm_amd import presets
    from fdm_amd._lib import DTYPE_NAMES
    from fdm_amd.vq import VQPlan
    from oracle import weights as W
    p = presets.get(a.preset)
    frames = [int(s * 30) for s in SECONDS]
    w = W.make_vq_weights(a.preset)
    for dt in a.dtypes.split(","):
        plan = VQPlan(a.preset, w, DTYPE_NAMES[dt], DEV)
        z = torch.randn(len(frames), max(frames) * p.G, p.c, generator=torch.Generator().manual_seed(1)) * (1.5 / 256)
        emo = torch.eye(7)[:1].expand(len(frames), -1) if p.n_books > 1 else None
        zq = plan.quant(z, emo)[0]
        solo = [zq[b:b + 1, :, :n * p.G].contiguous() for b, n in enumerate(frames)]
        res = alternate({"ragged": lambda: plan.decode_ragged(zq, frames), "per_clip": lambda: [plan.decode(s) for s in solo]}, a.reps, a.warmup)
        print(json.dumps({"stage": "vq_decode", "preset": a.preset, "dtype": dt, "frames": frames, "reps": a.reps, **res}), flush=True)


def e2e(a):
    from fdm_amd import pipeline
    wavs = [w.numpy() for w in waveforms()]
    has_switch = "batch_stages" in inspect.signature(pipeline.animate_many).parameters
    for dt in a.dtypes.split(","):
        diffusion, ae = pipeline.build_models(a.preset, device=DEV, dtype=dt)
        for label, kw in (("dpmpp2m20", dict(sampler="dpmpp2m", sampler_steps=20)), ("ddim100", dict(ddim_steps=100))):
            forms = {"off": lambda: pipeline.animate_many(diffusion, ae, wavs, device=DEV, **kw, **({"batch_stages": False} if has_switch else {}))}
            if has_switch:
                forms["on"] = lambda: pipeline.animate_many(diffusion, ae, wavs, device=DEV, batch_stages=True, **kw)
            res = alternate(forms, a.reps, a.warmup)
            print(json.dumps({"stage": "animate_many", "sampler": label, "preset": a.preset, "dtype": dt, "seconds": SECONDS, "reps": a.reps,
                              "has_batch_stages": has_switch, **res}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="encoders,vq,e2e")
    ap.add_argument("--preset", default="vocaset")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtypes", default="bf16,f16x3")
    a = ap.parse_args()
    for st in a.stage.split(","):
        {"encoders": encoders, "vq": vq, "e2e": e2e}[st](a)


if __name__ == "__main__":
    main()
