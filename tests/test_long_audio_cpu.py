"""CPU: windowed sampling of clips longer than max_len -- the layout and blend weights of the library's host functions
(fdm_window_layout_host, fdm_window_weights_host; include/fdm_hip.h states the rules) and a windowed CPU oracle built from
oracle.fdm_oracle.  tests/test_long_audio_gpu.py compares the HIP path with that oracle.  No device is touched."""
import ctypes as C

import pytest
import torch

from fdm_amd import _lib
from fdm_amd.denoiser import window_starts, window_weights
from oracle import fdm_oracle as FO
from oracle import weights as W

SWEEP = [(L, Wn, O) for L in (1, 7, 40, 41, 99, 100, 101, 599, 600, 601, 1350, 3000)
         for (Wn, O) in ((40, 10), (40, 0), (40, 39), (40, 30), (600, 60), (600, 0), (1, 0), (7, 3))]


def coverage(L, Wn, O):
    st = window_starts(L, Wn, O)
    Wf = min(Wn, L)
    cnt = torch.zeros(L, dtype=torch.int64)
    for s in st:
        cnt[s:s + Wf] += 1
    return st, Wf, cnt


@pytest.mark.parametrize("L,Wn,O", SWEEP)
def test_layout_properties(L, Wn, O):
    st, Wf, cnt = coverage(L, Wn, O)
    assert (cnt >= 1).all(), "every frame is covered"
    assert st[0] == 0 and st[-1] + Wf == L, "windows are exactly W' frames, the first starts at 0 and the last ends at L_total"
    assert all(0 <= s and s + Wf <= L for s in st)
    assert (len(st) == 1) == (L <= Wn), "one window iff L_total <= W"
    assert Wf == (L if L <= Wn else Wn)
    assert st == sorted(st) and len(set(st)) == len(st)
    for a, b in zip(st, st[1:]):
        assert a + Wf - b >= O, f"overlap {a + Wf - b} < {O}"
    if len(st) > 1:
        import math
        assert len(st) == math.ceil((L - O) / (Wn - O))


def test_triple_overlap_exists_and_is_blended():
    L, Wn, O = 100, 40, 30                 # stride 10 < W / 2: up to four windows cover a frame
    st, Wf, cnt = coverage(L, Wn, O)
    assert int(cnt.max()) >= 3
    w = window_weights(L, Wn, O)
    tot = torch.zeros(L, dtype=torch.float64)
    for i, s in enumerate(st):
        tot[s:s + Wf] += w[i].double()
    assert float((tot - 1).abs().max()) < 1e-6


def test_layout_argument_errors():
    l = _lib.lib()
    assert l.fdm_window_layout_host(100, 0, 0, None, 0) == -1
    assert l.fdm_window_layout_host(100, 40, 40, None, 0) == -1          # overlap >= window
    assert l.fdm_window_layout_host(100, 40, -1, None, 0) == -1
    assert l.fdm_window_layout_host(0, 40, 10, None, 0) == -2
    assert l.fdm_window_weights_host(0, 40, 10, None) == -2
    assert l.fdm_window_weights_host(100, 40, 50, None) == -1
    n = l.fdm_window_layout_host(100, 40, 10, None, 0)                   # starts = NULL: the needed cap
    buf = (C.c_int * n)(*([-7] * n))
    assert l.fdm_window_layout_host(100, 40, 10, buf, n - 1) == n and list(buf) == [-7] * n      # too small: nothing written
    assert l.fdm_window_layout_host(100, 40, 10, buf, n) == n and list(buf) == [0, 30, 60]


@pytest.mark.parametrize("L,Wn,O", [(100, 40, 10), (100, 40, 30), (3000, 600, 60), (1350, 600, 60), (601, 600, 60), (77, 40, 0), (500, 600, 60)])
def test_weights_partition_of_unity_and_taper(L, Wn, O):
    st = window_starts(L, Wn, O)
    w = window_weights(L, Wn, O)
    Wf = min(Wn, L)
    assert w.shape == (len(st), Wf) and (w > 0).all()
    tot = torch.zeros(L, dtype=torch.float64)
    for i, s in enumerate(st):
        tot[s:s + Wf] += w[i].double()
    assert float((tot - 1).abs().max()) < 1e-6
    # 1 where a single window covers the frame; continuous through each overlap (steps of at most 1 / O between frames)
    _, _, cnt = coverage(L, Wn, O)
    for i, s in enumerate(st):
        for f in range(s, s + Wf):
            if cnt[f] == 1:
                assert float(w[i, f - s]) == 1.0
        if O > 0:        # (three or more covering windows: the normalisation steepens the ramps, within 2 / O)
            bound = (1.0 if int(cnt.max()) <= 2 else 2.0) / O
            assert float((w[i, 1:] - w[i, :-1]).abs().max()) <= bound + 1e-6
    if O > 0 and len(st) > 1:
        assert float(w[0, 0]) == 1.0 and float(w[-1, -1]) == 1.0          # no taper at the long clip's ends
        assert float(w[1, 0]) < 0.5 / O + 1e-6                             # a later window enters from ~0


def test_weights_O0_average_the_covering_windows():
    L, Wn = 77, 40
    st = window_starts(L, Wn, 0)
    w = window_weights(L, Wn, 0)
    _, _, cnt = coverage(L, Wn, 0)
    for i, s in enumerate(st):
        for f in range(s, s + Wn):
            assert abs(float(w[i, f - s]) - 1.0 / int(cnt[f])) < 1e-7


# ---------------------------------------------------------------------------------------------
# windowed CPU oracle
# ---------------------------------------------------------------------------------------------
def windowed_denoiser(w, preset, hub, style, emo, L_total, window, overlap, cfg_scale=None):
    """denoise(x, t) of the windowed sampler: x [B, L_total*G, c] -> the blended x0 [B, L_total*G, c] (each window's CFG mix
    first, then sum_w w_hat_w(f) x0_w(f - s_w) in ascending window order, fp32)."""
    p = W.PRESETS[preset]
    G, c, pair = p["G"], p["c"], p["pair"]
    st = window_starts(L_total, window, overlap)
    wt = window_weights(L_total, window, overlap)
    Wf = min(window, L_total)

    def den(x, t):
        B = x.shape[0]
        xl = x.reshape(B, L_total, G * c)
        acc = torch.zeros_like(xl)
        seen = torch.zeros(L_total, dtype=torch.bool)
        for i, s in enumerate(st):
            xw = xl[:, s:s + Wf].reshape(B, Wf * G, c).contiguous()
            hw = hub[:, s * pair:(s + Wf) * pair]
            if cfg_scale is not None:
                x0 = FO.fdm_forward_cfg(w, preset, hw, t, xw, style, emo, cfg_scale, folded=True)
            else:
                x0 = FO.fdm_forward(w, preset, hw, t, xw, style, emo, folded=True)
            term = wt[i].view(1, Wf, 1) * x0.reshape(B, Wf, G * c)
            first = ~seen[s:s + Wf]
            acc[:, s:s + Wf] = torch.where(first.view(1, Wf, 1), term, acc[:, s:s + Wf] + term)
            seen[s:s + Wf] = True
        return acc.reshape(B, L_total * G, c)
    return den


def test_one_window_oracle_reproduces_the_plain_oracle():
    preset, L = "vocaset_tiny", 12
    w = W.make_fdm_weights(preset)
    inp = W.synth_inputs(preset, 2, L, seed=5)
    ts = [999, 500, 3, 0]
    noise = torch.randn(len(ts), *inp["x"].shape, generator=torch.Generator().manual_seed(1))
    plain = lambda x, t: FO.fdm_forward(w, preset, inp["hub"], t, x, inp["style"], None, folded=True)
    win = windowed_denoiser(w, preset, inp["hub"], inp["style"], None, L, 40, 10)
    assert torch.equal(FO.p_sample_loop(win, inp["x"].clone(), noise, ts), FO.p_sample_loop(plain, inp["x"].clone(), noise, ts))
    assert torch.equal(FO.ddim_sample(win, inp["x"].clone(), 4), FO.ddim_sample(plain, inp["x"].clone(), 4))


def test_windowed_oracle_seams_are_blends_of_the_windows():
    """Two windows: outside the overlap the blended x0 is the covering window's own prediction; inside it lies between them."""
    preset, L, Wn, O = "vocaset_tiny", 30, 20, 10
    w = W.make_fdm_weights(preset)
    inp = W.synth_inputs(preset, 1, L, seed=6)
    G, c = W.PRESETS[preset]["G"], W.PRESETS[preset]["c"]
    x0 = windowed_denoiser(w, preset, inp["hub"], inp["style"], None, L, Wn, O)(inp["x"], 400).reshape(1, L, G * c)
    st = window_starts(L, Wn, O)
    assert st == [0, 10]
    xl = inp["x"].reshape(1, L, G * c)
    a = FO.fdm_forward(w, preset, inp["hub"][:, :20], 400, xl[:, :20].reshape(1, 20 * G, c), inp["style"], folded=True).reshape(1, 20, -1)
    b = FO.fdm_forward(w, preset, inp["hub"][:, 10:30], 400, xl[:, 10:30].reshape(1, 20 * G, c), inp["style"], folded=True).reshape(1, 20, -1)
    assert torch.equal(x0[:, :10], a[:, :10]) and torch.equal(x0[:, 20:], b[:, 10:])
    lo, hi = torch.minimum(a[:, 10:], b[:, :10]), torch.maximum(a[:, 10:], b[:, :10])
    assert bool(((x0[:, 10:20] >= lo - 1e-6) & (x0[:, 10:20] <= hi + 1e-6)).all())
