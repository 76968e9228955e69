"""MI355X: the mesh hand-off (include/fdm_hip.h, fdm_mesh_*; csrc/mesh_out.hpp) -- positions bit for bit against torch's own add and
the existing linear_interp op, normals bit for bit against the float32 oracle of tests/mesh_cases.py (sign of zero aside), ragged
and batch invariance, layouts, then animate / animate_many / SlotServer with faces= and a plain C client.  Outputs are NaN-filled
before every call."""
import functools
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import mesh_cases as MC
from fdm_amd import _lib, mesh, ops, pipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP1 = 2.0 ** -23


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def plan(name):
    faces, V, _ = MC.mesh(name)
    return mesh.MeshOutPlan(faces, V, DEV)


def padded(off, frames, L_max=None):
    """[B, L_max, 3V] device tensor: clip b's rows, then NaN (input rows past frames[b] must never be read)"""
    x = off.copy() if L_max is None else np.concatenate([off, np.zeros((off.shape[0], L_max - off.shape[1], off.shape[2]), np.float32)], 1)
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return dev(x)


def run(name, off, frames, tmpl=None, fps=None, Lo_max=None, normals=True, interleaved=False, half=False, L_max=None):
    """forward() into NaN-filled outputs"""
    _, V, _ = MC.mesh(name)
    B = off.shape[0]
    Lo = max([MC.frames_out(L, fps) for L in frames] + [1]) if Lo_max is None else Lo_max
    dt = torch.float16 if half else torch.float32
    pos = torch.full((B, Lo, V, 6 if interleaved else 3), float("nan"), dtype=dt, device=DEV)
    nrm = None if interleaved else torch.full((B, Lo, V, 3), float("nan"), dtype=dt, device=DEV)
    mf = plan(name).forward(padded(off, frames, L_max), frames, None if tmpl is None else dev(tmpl), fps, normals, interleaved, half,
                            out=(pos, nrm))
    assert mf.frames == [MC.frames_out(L, fps) for L in frames]
    return pos, nrm, mf


def same_bits_but_zero_sign(got, want):
    """torch.equal up to the sign of zero (equal as values, no NaN on either side)"""
    return got.shape == want.shape and not torch.isnan(got).any() and bool((got == want).all())


@pytest.mark.parametrize("rows", [0, 1, 3])
def test_pass_through_positions_are_the_torch_add(rows):
    name, frames = "grid", [7, 7, 7]
    off = MC.offsets(name, 3, 7, seed=1)
    tmpl = MC.template(name, seed=1, rows=rows) if rows else None
    pos, _, _ = run(name, off, frames, tmpl)
    want = dev(off) if tmpl is None else dev(off) + dev(tmpl).reshape(-1, 1, off.shape[-1])
    assert torch.equal(pos.reshape(3, 7, -1), want)
    pos, _, _ = run(name, off, frames, tmpl, fps=(30, 30))           # equal rates: pass through as well
    assert torch.equal(pos.reshape(3, 7, -1), want)


@pytest.mark.parametrize("fps", [r for r in MC.RATES if r[0] != r[1]])
def test_resampled_positions_are_linear_interp_of_the_templated_clip(fps):
    name, frames = "grid_extra", [1, 2, 7, 16]
    _, V, _ = MC.mesh(name)
    off, tmpl = MC.offsets(name, 4, 16, seed=2), MC.template(name, seed=2, rows=4)
    pos, _, mf = run(name, off, frames, tmpl, fps, normals=False)
    for b, L in enumerate(frames):
        Lo = MC.frames_out(L, fps)
        x = (dev(off[b, :L]) + dev(tmpl[b])).contiguous()
        y = torch.full((Lo, 3 * V), float("nan"), device=DEV)
        ops.linear_interp(x, y, 1, L, Lo, 3 * V)
        assert torch.equal(pos[b, :Lo].reshape(Lo, -1), y), (b, L, Lo)
        assert not pos[b, Lo:].any()
    assert MC.frames_out(1, fps) in (1, 2) and mf.frames[0] == MC.frames_out(1, fps)


@pytest.mark.parametrize("name", MC.SMALL)
def test_normals_equal_the_float32_oracle_bit_for_bit(name):
    """Every mesh, with and without resampling: torch.equal to the float32 oracle up to the sign of zero.  The isolated vertex and the
    degenerate face contribute exact zeros; every other normal is within 2 ulp of unit length."""
    faces, V, _ = MC.mesh(name)
    frames = [5, 3]
    off, tmpl = MC.offsets(name, 2, 5, seed=4), MC.template(name, seed=4, rows=1)
    for fps in (None, (30, 25), (30, 60)):
        pos, nrm, _ = run(name, off, frames, tmpl, fps)
        want = MC.oracle(off, tmpl, frames, fps, faces, V)
        for b, L in enumerate(frames):
            Lo = MC.frames_out(L, fps)
            wp, wn = want[b]
            assert same_bits_but_zero_sign(pos[b, :Lo].cpu(), torch.from_numpy(wp)), (name, fps, b)
            err = float((nrm[b, :Lo].cpu() - torch.from_numpy(wn)).abs().max())
            print(f"{name} fps={fps} clip {b}: max |gpu - float32 oracle| = {err:.3e}")
            assert same_bits_but_zero_sign(nrm[b, :Lo].cpu(), torch.from_numpy(wn)), (name, fps, b, err)
            length = nrm[b, :Lo].double().pow(2).sum(-1).sqrt().cpu()
            live = torch.ones(V, dtype=torch.bool)
            if name in MC.ISOLATED:
                live[MC.ISOLATED[name]] = False
                assert not nrm[b, :Lo, MC.ISOLATED[name]].any()
            assert bool(((length[:, live] - 1).abs() <= 2 * ULP1).all())
    if name in MC.DEGENERATE:        # the face without area adds nothing: the mesh without it gives the same normals
        f = MC.DEGENERATE[name]
        assert f == len(faces) - 1 and np.array_equal(faces[:f], MC.mesh("grid")[0])
        _, other, _ = run("grid", off, frames, tmpl, None)
        _, nrm, _ = run(name, off, frames, tmpl, None)
        assert same_bits_but_zero_sign(nrm, other)


def test_ragged_batch_equals_each_clip_alone_whatever_the_padding():
    name, frames, fps = "strip", [7, 1, 4], (30, 25)
    off, tmpl = MC.offsets(name, 3, 7, seed=5), MC.template(name, seed=5, rows=3)
    for rate in (None, fps):
        pos, nrm, mf = run(name, off, frames, tmpl, rate)
        big_p, big_n, _ = run(name, off, frames, tmpl, rate, Lo_max=pos.shape[1] + 5, L_max=12)
        for b, L in enumerate(frames):
            Lo = mf.frames[b]
            p1, n1, m1 = run(name, off[b:b + 1, :L], [L], tmpl[b:b + 1], rate)
            assert m1.frames == [Lo]
            assert torch.equal(pos[b, :Lo], p1[0]) and torch.equal(nrm[b, :Lo], n1[0])
            assert torch.equal(big_p[b, :Lo], p1[0]) and torch.equal(big_n[b, :Lo], n1[0])
            for t in (pos, nrm, big_p, big_n):
                assert not t[b, Lo:].any() and not torch.isnan(t[b, Lo:]).any()
    # a clip without frames gives no rows
    pos, nrm, mf = run(name, off, [7, 0, 4], tmpl, None)
    assert mf.frames == [7, 0, 4] and not pos[1].any() and not nrm[1].any() and not torch.isnan(pos).any()


def test_vocaset_sized_rows():
    """V = 5023 (20 vertex blocks, 15 position tiles, rows of 15069 floats: not a multiple of 4), L = 3, resampled and not."""
    name, frames = "vocaset_size", [3, 2]
    faces, V, _ = MC.mesh(name)
    off, tmpl = MC.offsets(name, 2, 3, seed=6), MC.template(name, seed=6)
    for fps in (None, (30, 60)):
        pos, nrm, mf = run(name, off, frames, tmpl, fps)
        want = MC.oracle(off, tmpl, frames, fps, faces, V)
        for b in range(2):
            Lo = mf.frames[b]
            assert same_bits_but_zero_sign(pos[b, :Lo].cpu(), torch.from_numpy(want[b][0]))
            assert same_bits_but_zero_sign(nrm[b, :Lo].cpu(), torch.from_numpy(want[b][1]))
            p1, n1, _ = run(name, off[b:b + 1, :frames[b]], [frames[b]], tmpl, fps)
            assert torch.equal(pos[b, :Lo], p1[0]) and torch.equal(nrm[b, :Lo], n1[0])
            assert not pos[b, Lo:].any() and not nrm[b, Lo:].any()


@pytest.mark.parametrize("fps", [None, (30, 25)])
def test_layouts(fps):
    name, frames = "fan", [6, 3]
    off, tmpl = MC.offsets(name, 2, 6, seed=7), MC.template(name, seed=7, rows=2)
    pos, nrm, _ = run(name, off, frames, tmpl, fps)
    inter, none, mf = run(name, off, frames, tmpl, fps, interleaved=True)
    assert none is None and mf.normals is None and inter.shape[-1] == 6
    assert torch.equal(inter[..., :3], pos) and torch.equal(inter[..., 3:], nrm)
    hp, hn, _ = run(name, off, frames, tmpl, fps, half=True)
    assert hp.dtype == hn.dtype == torch.float16 and torch.equal(hp, pos.half()) and torch.equal(hn, nrm.half())
    hi, _, _ = run(name, off, frames, tmpl, fps, interleaved=True, half=True)
    assert torch.equal(hi, inter.half())
    for half in (False, True):          # normals=False: positions only, nrm untouched
        p2, n2, mf = run(name, off, frames, tmpl, fps, normals=False, half=half)
        assert mf.normals is None and torch.isnan(n2).all() and torch.equal(p2, pos.half() if half else pos)
    auto = plan(name).forward(padded(off, frames), frames, dev(tmpl), fps)          # outputs of the call's own making
    assert torch.equal(auto.positions, pos) and torch.equal(auto.normals, nrm)


PIPE_MESH = "vocaset_size"


@functools.lru_cache(maxsize=None)
def tiny_models():
    """The pipeline runs on the full VOCASET geometry only (fdm_vq_create refuses G * c != 1024 without a pre-embedding, so the tiny
    presets cannot be decoded; tests/test_ragged_gpu.py, models()): half a second of audio and 2-3 DDIM steps keep it short, and
    the mesh is the V = 5023 grid-like one."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


def test_animate_with_faces_returns_todays_vertices():
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    tmpl = MC.template(PIPE_MESH, seed=8)
    wav = tiny_audio(0.6, 1)
    want, lat = pipeline.animate(diffusion, ae, wav, tmpl, ddim_steps=3, seed=2, device=DEV)
    mf, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, ddim_steps=3, seed=2, device=DEV, faces=faces)
    L = want.shape[1]
    assert torch.equal(lat, lat2) and mf.frames == [L] and mf.positions.shape == (1, L, V, 3)
    assert torch.equal(mf.positions.reshape(1, L, -1), want)
    ref = pipeline.to_mesh(want, faces)
    assert torch.equal(ref.positions, mf.positions) and torch.equal(ref.normals, mf.normals)
    wn = MC.normals(want[0].cpu().numpy(), faces, V)
    assert same_bits_but_zero_sign(mf.normals[0].cpu(), torch.from_numpy(wn))
    # out_fps: the preset's 30 fps -> 60, interleaved fp16 through the mesh= options
    m2, _ = pipeline.animate(diffusion, ae, wav, tmpl, ddim_steps=3, seed=2, device=DEV, faces=faces, out_fps=60, mesh=dict(interleaved=True, half=True))
    r2 = pipeline.to_mesh(want, faces, fps=(30, 60))
    assert m2.frames == [MC.frames_out(L, (30, 60))] and torch.equal(m2.positions[..., :3], r2.positions.half())
    long, _ = pipeline.animate_long(diffusion, ae, wav, tmpl, ddim_steps=3, seed=2, device=DEV, faces=faces)
    assert torch.equal(long.positions, mf.positions) and torch.equal(long.normals, mf.normals)       # (fits one window: animate()'s bits)


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_faces_equal_to_mesh_of_the_default(batch_stages):
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4, 0.5))]
    tmpls = [MC.template(PIPE_MESH, seed=20 + i) for i in range(3)]
    kw = dict(ddim_steps=2, seed=1, device=DEV)
    verts, lats = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, **kw)
    for fps_kw, fps in ((dict(), None), (dict(out_fps=25), (30, 25))):
        got, lats2 = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, faces=faces, **fps_kw, **kw)
        for b in range(3):
            ref = pipeline.to_mesh(verts[b], faces, fps=fps)
            assert torch.equal(lats[b], lats2[b]) and got[b].frames == ref.frames
            assert torch.equal(got[b].positions, ref.positions) and torch.equal(got[b].normals, ref.normals)
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages)
    hs = srv.submit_many(wavs, tmpls, seeds=1)
    plain = {h: v for h, v, _ in srv.drain(2)}
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages, faces=faces, out_fps=60)
    hs2 = srv.submit_many(wavs, tmpls, seeds=1)
    meshes = {h: v for h, v, _ in srv.drain(2)}
    for h, h2 in zip(hs, hs2):
        ref = pipeline.to_mesh(plain[h], faces, fps=(30, 60))
        assert isinstance(meshes[h2], mesh.MeshFrames) and meshes[h2].frames == ref.frames
        assert torch.equal(meshes[h2].positions, ref.positions) and torch.equal(meshes[h2].normals, ref.normals)


def test_slot_server_batched_decode_with_a_template_on_one_request_only():
    """batch_stages: two requests finish in the same step() and share one decode; one has a template and one has none, so the mesh
    hand-off takes them clip by clip, and each result is bit for bit its own animate(..., faces=) call's."""
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    wavs = [tiny_audio(0.6, 0), tiny_audio(0.4, 1)]
    tmpls = [MC.template(PIPE_MESH, seed=20), None]
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=True, faces=faces)
    hs = srv.submit_many(wavs, tmpls, seeds=1)
    meshes = {h: v for h, v, _ in srv.drain(2)}
    assert srv.batched_decodes == [2]
    for h, wav, tmpl in zip(hs, wavs, tmpls):
        ref, _ = pipeline.animate(diffusion, ae, wav, tmpl, ddim_steps=2, seed=1, device=DEV, faces=faces)
        assert isinstance(meshes[h], mesh.MeshFrames) and meshes[h].frames == ref.frames
        assert torch.equal(meshes[h].positions, ref.positions) and torch.equal(meshes[h].normals, ref.normals)


def test_demo_command_line_with_faces_file(tmp_path):
    """demo --faces_file --out_fps 60 --save_normals: <stem>.npy keeps the reference's name and [1, L_out, 3V] shape and holds
    to_mesh(animate(...)) at 60 fps, <stem>_normals.npy its normals (one command-line run: each one builds the models)."""
    from scipy.io import wavfile
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    wp, fp, tp = str(tmp_path / "hello.wav"), str(tmp_path / "tri.npy"), str(tmp_path / "template.npy")
    wavfile.write(wp, 16000, (tiny_audio(0.5, 3) * 20000).astype(np.int16))
    np.save(fp, faces.astype(np.int64))
    np.save(tp, MC.template(PIPE_MESH, seed=9))
    dst = pipeline.demo_main("vocaset", ["--audio_file", wp, "--ddim_steps", "2", "--device", DEV, "--template_file", tp, "--audio_path",
                                         str(tmp_path / "out"), "--faces_file", fp, "--out_fps", "60", "--save_normals"])
    base, _ = pipeline.animate(diffusion, ae, pipeline.processor_normalize(pipeline.load_wav(wp)), np.load(tp), ddim_steps=2, device=DEV)
    ref = pipeline.to_mesh(base, faces, fps=(30, 60))
    Lo = MC.frames_out(base.shape[1], (30, 60))
    got, nr = np.load(dst), np.load(dst[:-4] + "_normals.npy")
    assert os.path.basename(dst) == "hello.npy" and got.shape == nr.shape == (1, Lo, 3 * V)
    assert np.array_equal(got, ref.positions.reshape(1, Lo, -1).cpu().numpy()) and np.array_equal(nr, ref.normals.reshape(1, Lo, -1).cpu().numpy())


def test_c_client_decodes_and_hands_off(tmp_path):
    """tests/abi_c/mesh_client.cpp: fdm_vq_decode_ragged -> fdm_mesh_forward with no Python in the process; Python writes the decoder's
    seeded weights by state-dict name, the inputs and the positions and normals its own path gives, which the client compares bit for bit."""
    diffusion, ae = tiny_models()
    faces, V, _ = MC.mesh(PIPE_MESH)
    vp = ae.plan(DEV)
    p, frames, fps = vp.p, [5, 3], (30.0, 25.0)
    zq = torch.randn(2, p.c, 5 * p.G, generator=torch.Generator().manual_seed(11)).to(DEV)
    tmpl = MC.template(PIPE_MESH, seed=11, rows=2)
    offs = ae.decode_many(zq, frames)
    mf = pipeline.to_mesh(offs, faces, tmpl, frames, fps)
    wfile, cfile = str(tmp_path / "weights.bin"), str(tmp_path / "case.bin")
    with open(wfile, "wb") as f:
        for name, t in ae.state_dict().items():
            if not name.startswith(("quantize.", "decoder.")) or name.endswith(".pe"):
                continue
            a = np.ascontiguousarray(t.detach().cpu().numpy().astype(np.float32)).reshape(-1)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)) + nb + struct.pack("<Q", a.size) + a.tobytes())
    Lo = mf.positions.shape[1]
    with open(cfile, "wb") as f:
        f.write(struct.pack("<14i", p.G, p.c, p.K, p.n_books, p.V3, int(p.vq_pre), vp.dtype, 2, 5, frames[0], frames[1], len(faces), V, Lo))
        f.write(struct.pack("<2d", *fps) + struct.pack("<2i", *mf.frames))
        for a in (zq.cpu().numpy(), tmpl, faces, mf.positions.cpu().numpy(), mf.normals.cpu().numpy()):
            f.write(np.ascontiguousarray(a).tobytes())
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "mesh_client")
    cmd = [hipcc, "-O2", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "abi_c", "mesh_client.cpp"),
           "-I", os.path.join(ROOT, "include"), "-L", libdir, "-lfdm_hip", "-Wl,-rpath," + libdir, "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    r = subprocess.run([exe, wfile, cfile], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mesh_client ok" in r.stdout
    print(r.stdout.strip())
