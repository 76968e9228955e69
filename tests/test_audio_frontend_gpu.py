"""GPU: the audio front end (include/fdm_hip.h, fdm_frontend_*; csrc/audio_front.hpp) -- raw PCM in, the encoders' waveform out.

Resampler against the float64 direct-form oracle of tests/audio_front_cases.py (pinned to scipy.signal.resample_poly at 1e-14 by
tests/test_audio_frontend_cpu.py), conversion and downmix bit for bit, the normaliser against the reference's golden and a float64
oracle, batch invariance bit for bit, then the path into the encoder, animate() and SlotServer, and a plain C client.
Inputs are N(0, 0.1) + 0.03 from a seeded CPU generator."""
import functools
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import audio_front_cases as AC  # noqa: E402
from fdm_amd import pipeline  # noqa: E402
from fdm_amd.hubert import FrontendPlan  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


WIDE_RATE = 384000      # 1 / 24: a tile of 256 outputs spans 256 * 24 + 480 = 6624 inputs, more than one LDS pass of 4096


@functools.lru_cache(maxsize=None)
def plan():
    return FrontendPlan(AC.GPU_RATES + (WIDE_RATE,), DEV)


def run(pcms, rates, pad=0, normalize=False, n_max=None, fill=float("nan")):
    """One front-end call on a NaN-filled output -> (wav [B, n_max] on the CPU, n_samples)."""
    ts = [torch.from_numpy(np.ascontiguousarray(p)).to(DEV) for p in pcms]
    ns = [plan().samples(len(p), r, pad) for p, r in zip(pcms, rates)]
    out = torch.full((len(ts), max(ns) if n_max is None else n_max), fill, device=DEV)
    wav, got = plan().forward(ts, rates, pad=pad, normalize=normalize, out=out)
    torch.cuda.synchronize()
    assert wav.data_ptr() == out.data_ptr() and got == ns
    return wav.cpu(), got


def test_tile_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "face-diffusion-model_amd", "csrc", "audio_front.hpp")).read()
    assert f"constexpr int FRONT_TILE = {AC.TILE};" in src


@pytest.mark.parametrize("rate", AC.GPU_RATES)
def test_resampler_against_the_float64_oracle(rate):
    """normalize = 0, pad = 0.  Bound: max |gpu - oracle| <= 4 x max |numpy float32 evaluation of the same sum - oracle| + one fp32 ulp of
    max |y| (the factor covers a different summation order and nothing else).  All lengths of a rate go through ONE call.
    Measured on an MI355X: profiles/audio_frontend/README.md."""
    up, down = AC.ratio(rate)
    lens = AC.lengths_for(rate, about=2000, tile=AC.TILE)
    outs = [AC.out_len(rate, n) for n in lens]
    assert {1, 2, max(down - 1, 1), down, down + 1} <= set(lens)
    assert any(abs(o - AC.TILE) <= 1 for o in outs) and any(o > AC.TILE for o in outs) and max(outs) >= 2000
    xs = [AC.noise(n, seed=100 + i) for i, n in enumerate(lens)]
    wav, ns = run(xs, [rate] * len(xs))
    assert ns == outs
    for i, (x, n_out) in enumerate(zip(xs, outs)):
        want = AC.resample64(x, rate)
        got = wav[i, :n_out].numpy().astype(np.float64)
        e_gpu = float(np.abs(got - want).max())
        e_f32 = float(np.abs(AC.resample32(x, rate).astype(np.float64) - want).max())
        bound = 4.0 * e_f32 + AC.ulp32(np.abs(want).max())
        print(f"{rate} Hz, {len(x)} frames -> {n_out}: max|gpu - f64| = {e_gpu:.2e}, max|numpy f32 - f64| = {e_f32:.2e}, "
              f"bound {bound:.2e}, max|y| = {np.abs(want).max():.3f}")
        assert e_gpu <= bound, (rate, len(x))
        assert bool((wav[i, n_out:] == 0).all())


def test_span_longer_than_one_lds_pass():
    """384 kHz (1 / 24): every full tile walks its input span in two LDS passes (csrc/audio_front.hpp, FRONT_SPAN).  The bound of the
    test above at 255, 256, 257 and about 2000 outputs, and each clip inside the batch bit for bit its own B = 1 call."""
    src = open(os.path.join(ROOT, "face-diffusion-model_amd", "csrc", "audio_front.hpp")).read()
    assert "constexpr int FRONT_SPAN = 4096;" in src and AC.TILE * 24 + 480 > 4096
    lens = [255 * 24, 256 * 24, 257 * 24, 2001 * 24 - 5]
    xs = [AC.as_format(AC.noise(n, 2, seed=300 + i), np.int16) for i, n in enumerate(lens)]
    wav, ns = run(xs, [WIDE_RATE] * len(xs))
    assert ns == [255, 256, 257, 2001]
    for i, (p, n_out) in enumerate(zip(xs, ns)):
        x = AC.mono32(p)
        want = AC.resample64(x, WIDE_RATE)
        e_gpu = float(np.abs(wav[i, :n_out].numpy().astype(np.float64) - want).max())
        e_f32 = float(np.abs(AC.resample32(x, WIDE_RATE).astype(np.float64) - want).max())
        bound = 4.0 * e_f32 + AC.ulp32(np.abs(want).max())
        print(f"{WIDE_RATE} Hz, {len(x)} frames -> {n_out}: max|gpu - f64| = {e_gpu:.2e}, max|numpy f32 - f64| = {e_f32:.2e}, bound {bound:.2e}")
        assert e_gpu <= bound, len(x)
        solo, _ = run([p], [WIDE_RATE])
        assert torch.equal(wav[i, :n_out], solo[0]) and bool((wav[i, n_out:] == 0).all())


def test_forward_refuses_a_wrong_output_tensor_and_a_short_rate_list():
    from fdm_amd._lib import FdmError
    pcms = [torch.zeros(300, dtype=torch.int16, device=DEV), torch.zeros(200, dtype=torch.int16, device=DEV)]
    good = torch.full((2, 100), float("nan"), device=DEV)
    for out in (good.double(), good[:1], torch.full((2, 200), 0.0, device=DEV)[:, ::2], good.cpu(), good.reshape(-1)):
        with pytest.raises(FdmError):
            plan().forward(pcms, [48000, 48000], out=out)
    with pytest.raises(FdmError):
        plan().forward(pcms, [48000], out=good)
    with pytest.raises(FdmError):
        plan().forward(pcms, [48000, 48000], out=good, n_max=99)
    torch.cuda.synchronize()
    assert bool(torch.isnan(good).all())                  # nothing was launched
    wav, ns = plan().forward(pcms, [48000, 48000], out=good)
    torch.cuda.synchronize()
    assert ns == [100, 67] and bool((wav == 0).all())


def test_pipeline_keeps_one_plan_per_stream_that_grows_with_the_rates():
    x = AC.as_format(AC.noise(900, 1, seed=5), np.int16)
    pipeline._FRONTENDS.clear()
    a = pipeline.prepare_audio(x, 48000, device=DEV)
    b, _ = pipeline.prepare_audio_many([x, x], [44100, 48000], device=DEV)
    c = pipeline.prepare_audio(x, 16000, device=DEV)
    assert len(pipeline._FRONTENDS) == 1 and next(iter(pipeline._FRONTENDS.values())).rates == (44100, 48000)
    assert torch.equal(b[1, :a.numel()], a) and c.numel() == 900 + 16000


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.uint8, np.float32], ids=lambda d: np.dtype(d).name)
def test_formats_and_downmix_are_the_float32_expression(dtype):
    """rate 16000, normalize = 0: no filter, so the output is items 1 and 2 of the rule, bit for bit, for 1, 2, 3 and 8 channels (one
    call per format; 700 frames: three tiles, the last one partial)."""
    chans = (1, 2, 3, 8)
    pcms = [AC.as_format(AC.noise(700 + c, c, seed=c), dtype) for c in chans]
    wav, ns = run(pcms, [16000] * len(pcms))
    for i, p in enumerate(pcms):
        assert ns[i] == len(p)
        assert torch.equal(wav[i, :ns[i]], torch.from_numpy(AC.mono32(p))), (np.dtype(dtype).name, chans[i])
        assert bool((wav[i, ns[i]:] == 0).all())


def test_normaliser_against_the_reference_golden(golden):
    """tests/golden/audio_misc.npz: 8000 samples at 16 kHz through Wav2Vec2FeatureExtractor.  Bound: the one tests/test_norm_edges_cpu.py
    states for this fixture's float32 results, 8 x 2^-24 x max |want|."""
    g = golden("audio_misc")
    wav, ns = run([g["wav"].astype(np.float32)], [16000], normalize=True)
    want = g["normalized"].astype(np.float64)
    assert ns == [8000]
    err = float(np.abs(wav[0].numpy().astype(np.float64) - want).max())
    print(f"golden normaliser: max|gpu - reference| = {err:.2e}, max|want| = {np.abs(want).max():.3f}")
    assert err <= 8 * 2.0 ** -24 * float(np.abs(want).max())


def test_normaliser_against_a_float64_oracle_and_padding():
    """n in {1, 2, 3, 1000, 16001} in one call with pad = 37 and 1000 columns beyond the longest clip.  Bound per clip: 4 x the error of
    processor_normalize (host float32) on the same input + one ulp of max |out|.  The padding and everything up to n_max is exactly 0.0
    on an output pre-filled with NaN."""
    sizes, pad = (1, 2, 3, 1000, 16001), 37
    xs = [AC.noise(n, seed=40 + n % 7) for n in sizes]
    wav, ns = run(xs, [16000] * len(xs), pad=pad, normalize=True, n_max=max(sizes) + pad + 1000)
    for i, x in enumerate(xs):
        n = len(x)
        assert ns[i] == n + pad
        want = AC.normalize64(x)
        host = pipeline.processor_normalize(x, pad_seconds=0).astype(np.float64)
        e_gpu = float(np.abs(wav[i, :n].numpy().astype(np.float64) - want).max())
        e_host = float(np.abs(host - want).max())
        bound = 4.0 * e_host + AC.ulp32(np.abs(want).max())
        print(f"normalise n = {n}: max|gpu - f64| = {e_gpu:.2e}, max|host f32 - f64| = {e_host:.2e}, bound {bound:.2e}, max|out| = {np.abs(want).max():.2f}")
        assert e_gpu <= bound, n
        assert bool((wav[i, n:] == 0).all()) and not bool(torch.isnan(wav[i]).any())


def test_constant_clip_normalises_to_zeros():
    pcms = [np.full(n, v, dtype=np.float32) for n, v in ((1, 0.25), (777, -0.1), (5000, 0.03))]
    wav, ns = run(pcms, [16000] * 3, pad=5, normalize=True)
    assert ns == [6, 782, 5005] and bool((wav == 0).all())


def mixed_batch():
    """Five clips of mixed rate, format and channel count, of unequal length, one of them a single frame."""
    spec = [(48000, np.int16, 2, 9001), (44100, np.float32, 1, 1), (16000, np.uint8, 3, 3000), (8000, np.int32, 8, 2500), (22050, np.int16, 1, 7777)]
    pcms = [AC.as_format(AC.noise(n, c, seed=60 + i), d) for i, (r, d, c, n) in enumerate(spec)]
    return pcms, [s[0] for s in spec]


@pytest.mark.parametrize("normalize", [False, True])
def test_batch_invariance_bit_for_bit(normalize):
    pcms, rates = mixed_batch()
    pad = 123
    wav, ns = run(pcms, rates, pad=pad, normalize=normalize)
    assert ns == [AC.out_len(r, len(p)) + pad for p, r in zip(pcms, rates)] and len(set(ns)) == 5
    wide, ns_w = run(pcms, rates, pad=pad, normalize=normalize, n_max=max(ns) + 1000)
    again, _ = run(pcms, rates, pad=pad, normalize=normalize)
    assert ns_w == ns and torch.equal(again, wav)
    assert not bool(torch.isnan(wav).any()) and not bool(torch.isnan(wide).any())
    for b, (p, r) in enumerate(zip(pcms, rates)):
        solo, n1 = run([p], [r], pad=pad, normalize=normalize)
        assert n1 == [ns[b]] and solo.shape == (1, ns[b])
        assert torch.equal(wav[b, :ns[b]], solo[0]), b
        assert torch.equal(wide[b, :ns[b]], solo[0]), b
        assert bool((wav[b, ns[b]:] == 0).all()) and bool((wide[b, ns[b]:] == 0).all())
        assert bool((solo[0, ns[b] - pad:] == 0).all())


def test_more_clips_than_one_launch_group():
    """20 clips (a launch carries 16 descriptors): every clip still equals its own call."""
    pcms = [AC.as_format(AC.noise(300 + 41 * i, 1 + i % 2, seed=i), np.int16) for i in range(20)]
    rates = [(48000, 44100, 16000, 8000)[i % 4] for i in range(20)]
    wav, ns = run(pcms, rates, pad=3, normalize=True)
    for b in (0, 15, 16, 17, 19):
        solo, _ = run([pcms[b]], [rates[b]], pad=3, normalize=True)
        assert torch.equal(wav[b, :ns[b]], solo[0]), b


def test_prepare_audio_many_into_the_encoder():
    """prepare_audio_many then encode_many (a 2-layer encoder) gives, per clip, the bits of its own prepare_audio then forward."""
    from fdm_amd.modules import HubertModel
    enc = HubertModel(n_layers=2)
    spec = [(48000, np.int16, 2, 30000), (44100, np.float32, 1, 22050), (16000, np.int16, 1, 9000)]
    pcms = [AC.as_format(AC.noise(n, c, seed=80 + i), d) for i, (r, d, c, n) in enumerate(spec)]
    rates = [s[0] for s in spec]
    wav, lens = pipeline.prepare_audio_many(pcms, rates, pad_seconds=0.25, device=DEV)
    assert wav.shape == (3, max(lens)) and lens == [AC.out_len(r, len(p)) + 4000 for p, r in zip(pcms, rates)]
    hubs = enc.encode_many([wav[b, :lens[b]] for b in range(3)], DEV)
    for b in range(3):
        own = pipeline.prepare_audio(pcms[b], rates[b], pad_seconds=0.25, device=DEV)
        assert torch.equal(own, wav[b, :lens[b]])
        assert torch.equal(enc(own.unsqueeze(0)).last_hidden_state, hubs[b]), b


@functools.lru_cache(maxsize=None)
def models():
    sys.path.insert(0, os.path.join(ROOT, "face-diffusion-model_amd", "dropin"))
    return pipeline.build_models("vocaset", device=DEV)


def test_animate_with_rate_is_animate_on_prepare_audio():
    diffusion, ae = models()
    pcm = AC.as_format(AC.noise(24000, 2, seed=90), np.int16)             # 0.5 s of 48 kHz stereo
    got = pipeline.animate(diffusion, ae, pcm, ddim_steps=2, seed=3, device=DEV, rate=48000)
    want = pipeline.animate(diffusion, ae, pipeline.prepare_audio(pcm, 48000, device=DEV), ddim_steps=2, seed=3, device=DEV)
    assert got[0].shape[1] >= 20 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    many = pipeline.animate_many(diffusion, ae, [pcm], ddim_steps=2, seed=3, device=DEV, rate=48000)
    assert torch.equal(many[0][0], want[0]) and torch.equal(many[1][0], want[1])
    long, lat = pipeline.animate_long(diffusion, ae, pcm, ddim_steps=2, seed=3, device=DEV, rate=48000)
    assert torch.equal(long, want[0]) and torch.equal(lat, want[1])          # (fits one window: animate()'s bits)


def test_demo_command_line_with_device_audio(tmp_path):
    """demo --device_audio on a 44.1 kHz stereo int16 file == animate(prepare_audio(*load_pcm(file))), and differs from the host path's
    result only as the two front ends differ (float32 host arithmetic), never in shape."""
    from scipy.io import wavfile
    pcm = AC.as_format(AC.noise(22050, 2, seed=92), np.int16)
    wp = str(tmp_path / "hello.wav")
    wavfile.write(wp, 44100, pcm)
    got_pcm, rate = pipeline.load_pcm(wp)
    assert rate == 44100 and got_pcm.dtype == np.int16 and np.array_equal(got_pcm, pcm)
    dst = pipeline.demo_main("vocaset", ["--audio_file", wp, "--audio_path", str(tmp_path / "result"), "--ddim_steps", "2", "--device_audio",
                                         "--device", DEV])
    diffusion, ae = pipeline.build_models("vocaset", None, DEV)
    ref, _ = pipeline.animate(diffusion, ae, pipeline.prepare_audio(got_pcm, rate, device=DEV), ddim_steps=2, device=DEV)
    arr = torch.from_numpy(np.load(dst))
    assert torch.equal(arr, ref.cpu())
    host = pipeline.processor_normalize(pipeline.load_wav(wp))
    assert len(host) == pipeline.prepare_audio(got_pcm, rate, device=DEV).numel()


def _sampler_module():
    import importlib.util
    sd = os.path.join(ROOT, "face-diffusion-model_amd", "dropin", "samples")
    sys.path.insert(0, os.path.dirname(sd))
    spec = importlib.util.spec_from_file_location("sample_diffusion", os.path.join(sd, "sample_diffusion.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("batch", [1, 2])
def test_sampler_command_line_with_device_audio(tmp_path, batch):
    """The sampler command line with --device_audio, in its default one-clip mode and with --batch 2 (animate_many): every file equals
    animate(prepare_audio(the loader's raw 48 kHz stereo int16 clip))."""
    mod = _sampler_module()
    from fdm_amd import presets
    out = str(tmp_path / "out")
    mod.main(None, ["--dataset", "vocaset", "--clips", "2", "--seconds", "0.5", "--ddim_steps", "2", "--out", out, "--device", DEV,
                    "--device_audio", "--batch", str(batch)])
    p = presets.get("vocaset")
    diffusion, ae = pipeline.build_models("vocaset", None, DEV, "", "", single_clip=batch <= 1)
    clips = list(mod.synthetic_loader(p, 2, 0.5, raw=True))
    assert all(isinstance(c[0], np.ndarray) and c[0].dtype == np.int16 and c[0].shape == (24000, 2) for c in clips)
    for pcm, template, one_hot_all, name in clips:
        ref, _ = pipeline.animate(diffusion, ae, pipeline.prepare_audio(pcm, mod.RAW_RATE, device=DEV), template, one_hot_all[:, 0, :], None,
                                  ddim_steps=2, device=DEV)
        got = torch.from_numpy(np.load(os.path.join(out, mod.save_name("vocaset", name, 0) + ".npy")))
        assert torch.equal(got, ref.cpu()), (batch, name)


def test_slot_server_submit_with_rate():
    diffusion, ae = models()
    pcm = AC.as_format(AC.noise(22050, 1, seed=91), np.int16)             # 0.5 s at 44.1 kHz
    res = []
    for raw in (True, False):
        srv = pipeline.SlotServer(diffusion, ae, slots=1, sampler="dpmpp2m", sampler_steps=2, device=DEV)
        if raw:
            h = srv.submit(pcm, rate=44100, seed=0)
        else:
            h = srv.submit(pipeline.prepare_audio(pcm, 44100, device=DEV), seed=0)
        (hh, v, lat), = srv.drain(2)
        assert hh == h
        res.append((v, lat))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    srv = pipeline.SlotServer(diffusion, ae, slots=1, sampler="dpmpp2m", sampler_steps=2, device=DEV)
    h, = srv.submit_many([pcm], rate=44100, seeds=0)
    (_, v, lat), = srv.drain(2)
    assert torch.equal(v, res[1][0]) and torch.equal(lat, res[1][1])


def test_c_client_prepares_its_own_audio(tmp_path):
    """tests/abi_c/frontend_smoke.cpp: int16 stereo 48 kHz -> fdm_frontend_forward -> fdm_hubert_forward_ragged (2 layers), no Python in
    the process; Python only writes the encoder's seeded weights by state-dict name and starts it."""
    from fdm_amd import _lib
    from oracle import weights as W
    wfile = str(tmp_path / "weights.bin")
    with open(wfile, "wb") as f:
        for name, t in W.make_hubert_weights(2).items():
            if not name.startswith(("feature_extractor.", "feature_projection.", "encoder.")):
                continue
            a =np.ascontiguousarray(t.numpy().astype(np.float32)).reshape(-1)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)) + nb + struct.pack("<Q", a.size) + a.tobytes())
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "frontend_smoke")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "abi_c", "frontend_smoke.cpp"),
           "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lfdm_hip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, wfile], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "frontend_smoke ok" in r.stdout
    print(r.stdout.strip())
