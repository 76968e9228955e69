"""Audio front end: the host path (load_wav's arithmetic + processor_normalize, numpy / scipy, one thread) against the device path
(pipeline.prepare_audio_many: fdm_frontend_forward) on the same raw audio.

    python tools/bench_frontend.py [--reps 10] [--warmup 2] [--limit 300]

Cases: 10 s and 60 s of stereo int16 at 44.1 and 48 kHz, B = 1 and 8 (eight cases).  The driver starts one child process per case
under `timeout -k 10 <limit>` and stops at the first case that fails or runs out of time; a child prints ONE JSON line:
  host_ms           wall clock of the host pass over the B clips, one after the other (median, min, max)
  device_ms         HIP events around fdm_frontend_forward alone, PCM already on the device
  device_e2e_ms     wall clock of prepare_audio_many from the host arrays to a synchronised stream (upload included)
  max_abs_diff      device against host waveform (float32 host arithmetic: agreement to a few 1e-6 of a unit-variance signal)
Figures belong in profiles/audio_frontend/README.md."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "face-diffusion-model_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CASES = [(sec, rate, B) for sec in (10, 60) for rate in (44100, 48000) for B in (1, 8)]
DEV = "cuda:0"


def host_path(pcm, rate):
    """pipeline.load_wav's arithmetic on an array already in memory, then processor_normalize."""
    import numpy as np
    from scipy.signal import resample_poly
    from fdm_amd import pipeline
    x = pcm.astype(np.float32) / float(np.iinfo(pcm.dtype).max + 1)
    x = x.mean(axis=1)
    g = np.gcd(int(rate), 16000)
    x = resample_poly(x, 16000 // g, int(rate) // g).astype(np.float32)
    return pipeline.processor_normalize(x)


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def child(a):
    import numpy as np
    import torch
    from fdm_amd import pipeline
    if not torch.cuda.is_available():
        raise SystemExit("bench_frontend needs the GPU (a CPU timing says nothing about it)")
    sec, rate, B = a.case
    rng = np.random.default_rng(1)
    pcms = [np.clip(rng.normal(0.03, 0.1, size=(int((sec - 0.37 * b / 8) * rate), 2)) * 32768.0, -32768, 32767).astype(np.int16) for b in range(B)]
    host = [[], None]
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        outs = [host_path(p, rate) for p in pcms]
        if r >= a.warmup:
            host[0].append((time.perf_counter() - t0) * 1e3)
        host[1] = outs
    plan = pipeline._frontend([rate], DEV)
    ts = [torch.from_numpy(p).to(DEV) for p in pcms]
    dev, e2e = [], []
    for r in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        wav, lens = plan.forward(ts, [rate] * B, pad=16000)
        e1.record()
        e1.synchronize()
        t0 = time.perf_counter()
        wav2, _ = pipeline.prepare_audio_many(pcms, rate, device=DEV)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if r >= a.warmup:
            dev.append(e0.elapsed_time(e1))
            e2e.append((t1 - t0) * 1e3)
    diff = max(float(np.abs(wav[b, :lens[b]].cpu().numpy() - host[1][b]).max()) for b in range(B))
    assert all(lens[b] == len(host[1][b]) for b in range(B)) and torch.equal(wav, wav2)
    print(json.dumps({"seconds": sec, "rate": rate, "B": B, "format": "int16 stereo", "reps": a.reps, "samples_out": lens,
                      "host_ms": stats(host[0]), "device_ms": stats(dev), "device_e2e_ms": stats(e2e), "max_abs_diff": diff}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=300, help="seconds a case may take (its own `timeout -k 10`)")
    ap.add_argument("--case", type=int, nargs=3, default=None, metavar=("SECONDS", "RATE", "B"), help="run this case in this process")
    a = ap.parse_args()
    if a.case:
        return child(a)
    for sec, rate, B in CASES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--warmup", str(a.warmup),
               "--case", str(sec), str(rate), str(B)]
        rc = subprocess.call(cmd)
        if rc != 0:
            raise SystemExit(f"case {sec} s, {rate} Hz, B = {B} ended with status {rc}: nothing more is started")


if __name__ == "__main__":
    main()
