"""GPU: clips of unequal length in one call (include/fdm_hip.h: fdm_attn_args.lens, fdm_hubert_forward_ragged, fdm_vq_decode_ragged).

The bar is bit identity (torch.equal): inside a batch padded to the longest clip, every clip's own rows are what today's call
returns for that clip alone (B = 1, its own length), in every arithmetic mode; rows beyond a clip's length are exactly zero;
and nothing the caller leaves in the padding -- NaN included -- changes a bit.  Attention on its own first (operands of
tests/attn_cases.py; lengths around both key-tile widths, a single key, and both sides of the switch to two query sub-tiles at
L = 384), then the audio encoders (waveform padding, time GroupNorm in both of its forms, positional-conv padding, attention),
the VQ decoder (replicate padding, instance statistics, attention), then the pipeline's batch_stages switch and
SlotServer.submit_many."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_cases as AC  # noqa: E402
from attn_cases import BF16, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402
from fdm_amd.hubert import WAV2VEC2_BASE, HubertPlan, conv_lengths, num_frames  # noqa: E402
from fdm_amd.vq import VQPlan  # noqa: E402
from oracle import weights as W  # noqa: E402

DEV = "cuda:0"
KIND_IDS = lambda k: AC.KIND_NAMES[k]  # noqa: E731

# ---------------------------------------------------------------------------------------------------------------------
# attention alone
# ---------------------------------------------------------------------------------------------------------------------
B, H, LPAD = 3, 2, 400
# every length of {1, 15, 16, 17, 31, 32, 33, 383, 384, 400}: one fp32 (16) and one 16-bit (32) key tile and their neighbours, a
# single key, and solo launches on both sides of the two-sub-tile switch (384) inside a padded launch that is past it
LENS = [(1, 15, 16), (17, 31, 32), (33, 383, 384), (400, 1, 384)]


@functools.lru_cache(maxsize=None)
def full_operands(kind, hd):
    return AC.operands(kind, *AC.gaussian(B, H, LPAD, hd, seed=11), device=DEV)


def clip_operands(opnd, b, n):
    """Clip b's first n positions as a problem of its own."""
    return AC.Operands(opnd.kind, tuple(p[..., b:b + 1, :, :n, :].contiguous() for p in opnd.planes))


def poisoned(opnd, lens):
    """The same operands with NaN in K and V from the first 32-key tile wholly beyond each clip's length (whole 32-key tiles are
    whole 16-key tiles of the fp32 kind too)."""
    q, k, v = (p.clone() for p in opnd.planes)
    for b, n in enumerate(lens):
        k[..., b, :, (n + 31) // 32 * 32:, :] = float("nan")
        v[..., b, :, (n + 31) // 32 * 32:, :] = float("nan")
    return AC.Operands(opnd.kind, (q, k, v))


def new_output(kind, rows, cols, fill):
    if kind == F16X3:
        return ops.Split(torch.full((2, rows, cols), fill, device=DEV, dtype=torch.float16), F16X3)
    return torch.full((rows, cols), fill, device=DEV, dtype=AC.plane_dtype(kind))


def bits(t):
    return t.planes if isinstance(t, ops.Split) else t


def launch(opnd, lens=None):
    """One launch -> the output bits [(2,) B*L, d]; the output buffer starts as 7.0 everywhere."""
    d = opnd.H * opnd.hd
    Q, Kp, Vp, Lpad = opnd.device_inputs(DEV, 0.0)
    O = new_output(opnd.kind, opnd.B * opnd.L, d, 7.0)
    lv = torch.tensor(lens, dtype=torch.int32, device=DEV) if lens is not None else None
    ops.attention(Q, Kp, Vp, O, B=opnd.B, H=opnd.H, L=opnd.L, hd=opnd.hd, ldq=d, ldo=d, Lpad=Lpad, scale=1.0 / opnd.hd ** 0.5,
                  causal=False, lens=lv)
    torch.cuda.synchronize()
    return bits(O)


@functools.lru_cache(maxsize=None)
def solo(kind, hd, b, n):
    opnd = full_operands(kind, hd)
    return launch(clip_operands(opnd, b, n)).clone()


@pytest.mark.parametrize("lens", LENS, ids=lambda t: "-".join(map(str, t)))
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_attention_with_lengths_is_each_clips_solo_launch(kind, hd, lens):
    opnd = full_operands(kind, hd)
    d = H * hd
    got = launch(opnd, lens)
    rows = got.reshape(got.shape[:-2] + (B, LPAD, d))
    for b, n in enumerate(lens):
        assert torch.equal(rows[..., b, :n, :], solo(kind, hd, b, n).reshape(got.shape[:-2] + (n, d))), (b, n)
        assert bool((rows[..., b, n:, :] == 0).all()), f"clip {b}: a row at or beyond {n} is not zero"
    # K / V of key tiles wholly beyond a clip's length are never fetched: NaN there changes nothing
    assert torch.equal(launch(poisoned(opnd, lens), lens), got)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("kind", AC.KINDS, ids=KIND_IDS)
def test_attention_without_lengths_is_unchanged(kind, hd):
    """lens = NULL runs the kernels of the uniform form; full lengths through the new form give the same bits, and each clip of
    the uniform launch is its solo launch."""
    opnd = full_operands(kind, hd)
    plain = launch(opnd)
    assert torch.equal(launch(opnd, (LPAD,) * B), plain)
    d = H * hd
    rows = plain.reshape(plain.shape[:-2] + (B, LPAD, d))
    for b in range(B):
        assert torch.equal(rows[..., b, :, :], solo(kind, hd, b, LPAD).reshape(plain.shape[:-2] + (LPAD, d)))


# ---------------------------------------------------------------------------------------------------------------------
# VQ decode
# ---------------------------------------------------------------------------------------------------------------------
VQ_FRAMES = [2, 5, 12, 33, 100]
_VQ = {}


def vq_plan(preset, dtype):
    if (preset, dtype) not in _VQ:
        _VQ[(preset, dtype)] = VQPlan(preset, W.make_vq_weights(preset), dtype, DEV)
    return _VQ[(preset, dtype)]


@functools.lru_cache(maxsize=None)
def vq_codes(preset):
    """Quantised latents [5, c, 100*G] of five seeded clips (mead: five emotions), from the fp32 object's quantiser."""
    p = W.PRESETS[preset]
    n = len(VQ_FRAMES)
    z = torch.randn(n, max(VQ_FRAMES) * p["G"], p["c"], generator=torch.Generator().manual_seed(71)) * (1.5 / 256)
    emo = torch.eye(7)[[0, 6, 3, 5, 1]] if p["n_books"] > 1 else None
    return vq_plan(preset, F32).quant(z, emo)[0].clone()


@pytest.mark.parametrize("dtype", [F32, BF16, F16X3], ids=KIND_IDS)
@pytest.mark.parametrize("preset", ["vocaset", "mead"])
def test_vq_decode_ragged_is_each_clips_solo_decode(preset, dtype):
    G = W.PRESETS[preset]["G"]
    plan, zq = vq_plan(preset, dtype), vq_codes(preset)
    got = plan.decode_ragged(zq, VQ_FRAMES).clone()
    assert got.shape[:2] == (len(VQ_FRAMES), max(VQ_FRAMES))
    for b, n in enumerate(VQ_FRAMES):
        alone = plan.decode(zq[b:b + 1, :, :n * G].contiguous())
        assert torch.equal(got[b, :n], alone[0]), (b, n)
        assert bool((got[b, n:] == 0).all()), f"clip {b}: a row at or beyond {n} is not zero"
    # what the latent holds beyond a clip's frames never matters
    bad = zq.clone()
    for b, n in enumerate(VQ_FRAMES):
        bad[b, :, n * G:] = float("nan")
    assert torch.equal(plan.decode_ragged(bad, VQ_FRAMES), got)
    # equal lengths through the ragged entry: the uniform batched decode
    same = plan.decode_ragged(zq[:, :, :33 * G].contiguous(), [33] * len(VQ_FRAMES)).clone()
    assert torch.equal(same, plan.decode(zq[:, :, :33 * G].contiguous()))


def test_vq_decode_ragged_refuses_bad_lengths():
    from fdm_amd._lib import FdmError
    plan, zq = vq_plan("vocaset", F32), vq_codes("vocaset")
    for frames in ([2, 5, 12, 33, 101], [1, 5, 12, 33, 100]):
        with pytest.raises(FdmError, match="frames"):
            plan.decode_ragged(zq, frames)
    with pytest.raises(FdmError):
        plan.decode_ragged(zq, [2, 5, 12])


# ---------------------------------------------------------------------------------------------------------------------
# audio encoders
# ---------------------------------------------------------------------------------------------------------------------
# conv-stack lengths T6 of the clips of one call: 2 (the shortest the encoder takes), 32, 33 (odd: the even crop drops a frame, 32
# frames come out), 100 and 384 (attention past the two-sub-tile switch).  wav2vec2-base normalises conv 0 over time: the clips of
# T6 <= 33 have fewer than 4096 conv-0 frames (three-pass form), those of 100 and 384 take the chunked form with 7 and 25 chunks.
HUB_T6 = [2, 32, 33, 100, 384]
_HUB = {}


def samples_for(t6):
    n = 320 * t6
    while conv_lengths(n)[-1] < t6:
        n += 1
    return n


def hub_plan(kind, dtype, layers=2):
    if (kind, dtype, layers) not in _HUB:
        if kind == 0:
            _HUB[(kind, dtype, layers)] = HubertPlan(W.make_hubert_weights(layers), layers, dtype, DEV)
        else:
            _HUB[(kind, dtype, layers)] = HubertPlan(W.make_wav2vec_weights(layers), layers, dtype, DEV, cfg=WAV2VEC2_BASE)
    return _HUB[(kind, dtype, layers)]


@functools.lru_cache(maxsize=None)
def hub_wavs():
    g = torch.Generator().manual_seed(23)
    return tuple(torch.randn(samples_for(t), generator=g) * 0.1 for t in HUB_T6)


def check_clips(plan, wavs, out, lens):
    assert out.shape[1] == max(lens)
    for b, w in enumerate(wavs):
        alone = plan.forward(w)
        assert lens[b] == alone.shape[1] == num_frames(w.numel())
        assert torch.equal(out[b, :lens[b]], alone[0]), (b, lens[b])
        assert bool((out[b, lens[b]:] == 0).all()), f"clip {b}: a row at or beyond {lens[b]} is not zero"


@pytest.mark.parametrize("dtype", [F32, BF16, F16X3], ids=KIND_IDS)
@pytest.mark.parametrize("kind", [0, 1], ids=["hubert", "wav2vec2"])
def test_encoder_ragged_is_each_clips_solo_forward(kind, dtype):
    plan, wavs = hub_plan(kind, dtype), hub_wavs()
    assert [conv_lengths(w.numel())[-1] for w in wavs] == HUB_T6
    out, lens = plan.forward_ragged(wavs)
    out = out.clone()
    assert lens == [2, 32, 32, 100, 384]
    check_clips(plan, wavs, out, lens)
    # what the waveform batch holds beyond a clip's samples never matters
    ns = [w.numel() for w in wavs]
    bad = torch.full((len(wavs), max(ns)), float("nan"))
    for b, w in enumerate(wavs):
        bad[b, :ns[b]] = w
    out2, lens2 = plan.forward_padded(bad.to(DEV), ns)
    assert lens2 == lens and torch.equal(out2, out)
    # four clips of one length through the ragged entry: the uniform batched forward
    same = torch.stack([torch.roll(wavs[2], 17 * i) for i in range(4)]).to(DEV)
    out3, lens3 = plan.forward_padded(same, [same.shape[1]] * 4)
    out3 = out3.clone()
    assert lens3 == [32] * 4 and torch.equal(out3, plan.forward(same))


def test_hubert_large_full_depth_ragged_bf16():
    plan = hub_plan(0, BF16, layers=24)
    g = torch.Generator().manual_seed(29)
    wavs = [torch.randn(n, generator=g) * 0.1 for n in (32000, 48000)]
    out, lens = plan.forward_ragged(wavs)
    check_clips(plan, wavs, out.clone(), lens)


def test_encoder_ragged_refuses_bad_lengths():
    from fdm_amd._lib import FdmError
    plan = hub_plan(0, F32)
    wav = torch.zeros(2, 4000, device=DEV)
    for ns in ([4000, 399], [4000, 4001]):
        with pytest.raises(FdmError, match="samples"):
            plan.forward_padded(wav, ns)


# ---------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------
def _wavs(sizes, seed):
    from oracle import hubert_oracle as HO
    g = torch.Generator().manual_seed(seed)
    return [HO.processor_normalize(torch.randn(n, generator=g) * 0.1).numpy() for n in sizes]


@functools.lru_cache(maxsize=None)
def models(preset, cfg):
    """(presets.py has vocaset_tiny / mead_tiny for the denoiser, G * c = 128 / 256; the VQ decoder takes the latent as its 1024-wide
    input (vocaset: no pre-embedding, fdm_vq_create refuses G * c != 1024) and its hidden width is fixed, so the pipeline -- encoder,
    denoiser, quantiser, decoder -- runs on the full geometry only, as in tests/test_slots_gpu.py: about a second of audio per clip.)"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "face-diffusion-model_amd", "dropin"))
    from fdm_amd import pipeline
    return pipeline.build_models(preset, device=DEV, **(dict(cfg_level=2.5) if cfg else {}))


@pytest.mark.parametrize("form", ["ddim", "ddpm", "dpmpp2m"])
def test_animate_many_batch_stages_equals_the_per_clip_path(form, monkeypatch):
    """Five clips of different durations: one encoder call, and one padded quant and one decode per group, against the per-clip
    loops.  DDPM runs a 10-step chain through the sampler's own t_range argument."""
    from fdm_amd import pipeline
    diffusion, ae = models("vocaset", False)
    audios = _wavs((16000, 24400, 11300, 20000, 8000), 3)
    kw = dict(ddim=dict(ddim_steps=6), ddpm=dict(), dpmpp2m=dict(sampler="dpmpp2m", sampler_steps=5))[form]
    if form == "ddpm":
        full = diffusion.sample
        monkeypatch.setattr(diffusion, "sample", lambda *a, **k: full(*a, t_range=(999, 989), **k))
    tmpl = [torch.full((1, 15069), 0.01 * i) for i in range(5)]
    v0, l0 = pipeline.animate_many(diffusion, ae, audios, tmpl, device=DEV, max_batch=3, batch_stages=False, **kw)
    v1, l1 = pipeline.animate_many(diffusion, ae, audios, tmpl, device=DEV, max_batch=3, batch_stages=True, **kw)
    assert len({v.shape[1] for v in v0}) == 5
    for b in range(5):
        assert torch.equal(l0[b], l1[b]) and torch.equal(v0[b], v1[b]), b


@pytest.mark.parametrize("preset,cfg", [("vocaset", False), ("mead", True)])
def test_slot_server_submit_many_equals_submit_in_a_loop(preset, cfg):
    """submit_many (one encoder call) on a server that decodes the clips finishing together in one call, against submit() in a loop
    on a per-clip server; and each of the two alone against it."""
    from fdm_amd import pipeline
    diffusion, ae = models(preset, cfg)
    wavs, seeds = _wavs((16000, 11000, 13500), 9), [4, 5, 6]
    emos = [torch.eye(7)[i:i + 1] for i in (2, 5, 0)] if preset == "mead" else None
    got = {}
    for many, on in ((False, False), (True, False), (False, True), (True, True)):
        srv = pipeline.SlotServer(diffusion, ae, slots=3, sampler="dpmpp2m", sampler_steps=4, device=DEV, batch_stages=on)
        if many:
            hs = srv.submit_many(wavs, emotion_one_hots=emos, seeds=seeds)
        else:
            hs = [srv.submit(w, emotion_one_hot=emos[i] if emos else None, seed=s) for i, (w, s) in enumerate(zip(wavs, seeds))]
        res = {h: (v, lat) for h, v, lat in srv.drain(2)}
        assert srv.batched_decodes == ([3] if on else [])          # admitted together, they finish in one step(): one decode of three
        got[(many, on)] = [res[h] for h in hs]
    assert len({v.shape[1] for v, _ in got[(False, False)]}) == 3
    for key in ((True, False), (False, True), (True, True)):
        for (va, la), (vb, lb) in zip(got[(False, False)], got[key]):
            assert torch.equal(la, lb) and torch.equal(va, vb), key
