"""MI355X: the wrap hand-off (include/fdm_hip.h, fdm_wrap_*; csrc/wrap_out.hpp) -- the nearest-face search array_equal to the float32
restatement of tests/wrap_cases.py on every target set, the follow step bit for bit against it (uint32 views), batch and tile
invariance, then animate / animate_many / SlotServer with wrap=.  Outputs are NaN-filled before every call."""
import functools

import numpy as np
import pytest
import torch

import mesh_cases as MC
import wrap_cases as WC
from fdm_amd import pipeline, wrap

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def searched(name, kind, k):
    """the plan whose binding the device searched, and the float32 restatement's"""
    S, faces, T = WC.case(name, kind, k)
    return wrap.WrapPlan(S, faces, T, device=DEV), WC.nearest(S, faces, T)


@pytest.mark.parametrize("cs", WC.SEARCH_CASES, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_search_is_the_float32_restatement_and_coordinates_are_the_hosts(cs):
    S, faces, T = WC.case(*cs)
    plan, (want_fi, _, _) = searched(*cs)
    fi, uvh, dist = plan.binding()
    assert np.array_equal(fi, want_fi)
    want_uvh, want_dist = wrap.coords(S, faces, T, fi)
    assert np.array_equal(bits(uvh), bits(want_uvh)) and np.array_equal(bits(dist), bits(want_dist))


def test_a_vertex_gets_the_same_face_alone_and_among_257():
    S, faces, T = WC.case("vocaset_size", "lifted", 257)
    among = searched("vocaset_size", "lifted", 257)[0].binding()[0]
    for j in (0, 63, 64, 200, 256):
        alone = wrap.WrapPlan(S, faces, T[j:j + 1], device=DEV).binding()[0]
        assert list(alone) == [among[j]]
    S, faces, T = WC.case("tile+1", "lifted", 65)
    among = searched("tile+1", "lifted", 65)[0].binding()[0]
    assert [wrap.WrapPlan(S, faces, T[j:j + 1], device=DEV).binding()[0][0] for j in (0, 64)] == [among[0], among[64]]


def test_no_candidate_fails_the_create_and_names_the_vertex():
    S, faces = WC.source("degenerate")
    f = MC.DEGENERATE["degenerate"]
    with pytest.raises(wrap.FdmError, match="target vertex 0 has no candidate"):
        wrap.WrapPlan(S, faces[f:f + 1], WC.targets("degenerate", "own")[:3], device=DEV)


def padded(off, frames, L_max=None):
    """[B, L_max, 3V] device tensor: clip b's rows, then NaN (input rows past frames[b] must never be read)"""
    x = off.copy() if L_max is None else np.concatenate([off, np.zeros((off.shape[0], L_max - off.shape[1], off.shape[2]), np.float32)], 1)
    for b, L in enumerate(frames):
        x[b, L:] = np.nan
    return dev(x)


def run(plan, off, frames, tmpl, offsets_out, L_max=None):
    B, L = off.shape[0], off.shape[1] if L_max is None else L_max
    out = torch.full((B, L, 3 * plan.Vt), float("nan"), device=DEV)
    got = plan.forward(padded(off, frames, L_max), frames, None if tmpl is None else dev(tmpl), offsets_out, out=out)
    assert got is out
    return out.cpu().numpy()


def check_rows(got, want, frames):
    for b, L in enumerate(frames):
        assert np.array_equal(bits(got[b, :L]), bits(want[b])), f"clip {b}"
        assert np.array_equal(bits(got[b, L:]), np.zeros_like(bits(got[b, L:]))), f"padding of clip {b}"       # exactly +0


FOLLOW_SETS = list(dict.fromkeys([(s, "own", None) for s in WC.SOURCES] + [(s, "lifted", 257) for s in WC.SOURCES] + [("grid", "lifted", k) for k in WC.CUTS]))


@pytest.mark.parametrize("cs", FOLLOW_SETS, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_follow_bit_for_bit(cs):
    """B = 3, frames = [5, 0, 2], L_max = 5, NaN in every input row past a clip's frames; tmpl_rows 0, 1 and B; weights absent and
    present (0 and 1 among them); both flag values."""
    name = cs[0]
    S, faces, T = WC.case(*cs)
    fi, uvh, _ = searched(*cs)[0].binding()
    frames, B = [5, 0, 2], 3
    off = MC.offsets(name, B, 5, seed=11)
    w = np.linspace(0, 1, len(T)).astype(np.float32) if len(T) > 1 else np.ones(1, np.float32)
    for weights in (None, w):
        plan = searched(*cs)[0] if weights is None else wrap.WrapPlan(S, faces, T, face_idx=fi, weights=weights, device=DEV)
        for rows in (0, 1, B):
            tmpl = MC.template(name, seed=0, rows=rows) if rows else None
            x = off + (S.reshape(1, 1, -1) if tmpl is None else 0)          # without a template the offsets are the vertices themselves
            x = x.astype(np.float32)
            for offsets_out in (False, True):
                want = WC.follow(x, tmpl, frames, faces, fi, uvh, T, weights, offsets_out)
                check_rows(run(plan, x, frames, tmpl, offsets_out), want, frames)


def test_follow_on_a_face_that_loses_its_area_in_a_frame():
    name = "degenerate"
    S, faces, T = WC.case(name, "lifted", 257)
    plan = searched(name, "lifted", 257)[0]
    fi, uvh, _ = plan.binding()
    f = int(fi[0])
    off = (MC.offsets(name, 1, 3, seed=12) + S.reshape(1, 1, -1)).astype(np.float32)       # vertices: no template
    tmpl = None
    p = off[0, 1].reshape(-1, 3)                                    # (a view) frame 1: the face's three vertices meet in one point
    p[faces[f, 1]] = p[faces[f, 2]] = p[faces[f, 0]]
    got = run(plan, off, [3], tmpl, False)
    want = WC.follow(off, tmpl, [3], faces, fi, uvh, T)
    on_f = np.nonzero(fi == f)[0]
    y = got[0, 1].reshape(-1, 3)
    a = p[faces[f, 0]]
    assert len(on_f) and np.isfinite(got).all()
    assert np.array_equal(bits(y[on_f]), bits(np.broadcast_to(a, (len(on_f), 3))))      # nh = 0, e1 = e2 = 0: y = a
    check_rows(got, want, [3])


def test_batch_and_length_independence():
    name = "strip"
    S, faces, T = WC.case(name, "lifted", 257)
    plan = searched(name, "lifted", 257)[0]
    frames = [4, 7, 0, 1]
    off, tmpl = MC.offsets(name, 4, 7, seed=13), MC.template(name, seed=0, rows=4)
    got = run(plan, off, frames, tmpl, False)
    for b, L in enumerate(frames):
        assert not got[b, L:].any()
        if L:
            solo = run(plan, off[b:b + 1, :L], [L], tmpl[b:b + 1], False)
            longer = run(plan, off[b:b + 1], [L], tmpl[b:b + 1], False, L_max=12)
            assert np.array_equal(bits(solo[0]), bits(got[b, :L])) and np.array_equal(bits(longer[0, :L]), bits(got[b, :L]))
            assert not longer[0, L:].any()
    auto = plan.forward(padded(off, frames), frames, dev(tmpl))                    # an output of the call's own making
    assert np.array_equal(bits(auto.cpu().numpy()), bits(got))


def test_full_width():
    """V = 5023 -> Vt = 5024 (the source's vertices and one more), 2 frames.  The binding is brought by the caller (the lowest face
    at each vertex; wrap_cases.incident_binding): the restatement of the search at 5024 x 9.9k pairs would take the suite the better part of a minute,
    and the search at this face count is checked at Vt = 257 above."""
    S, faces = WC.source("vocaset_size")
    T = np.concatenate([S + np.float32(0.01), S[:1] - np.float32(0.02)])
    fi = np.concatenate([WC.incident_binding(faces, len(S)), [0]]).astype(np.int32)
    plan = wrap.WrapPlan(S, faces, T, face_idx=fi, device=DEV)
    _, uvh, _ = plan.binding()
    off = MC.offsets("vocaset_size", 2, 2, seed=14)
    tmpl = S.reshape(1, -1)
    check_rows(run(plan, off, [2, 1], tmpl, False), WC.follow(off, tmpl, [2, 1], faces, fi, uvh, T), [2, 1])
    check_rows(run(plan, off, [2, 1], tmpl, True), WC.follow(off, tmpl, [2, 1], faces, fi, uvh, T, None, True), [2, 1])


# ---- the pipeline
PIPE_MESH = "vocaset_size"


@functools.lru_cache(maxsize=None)
def tiny_models():
    """As tests/test_mesh_out_gpu.py: the pipeline decodes on the full VOCASET geometry only; short audio and 2-3 DDIM steps."""
    return pipeline.build_models("vocaset", None, DEV)


def tiny_audio(seconds, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.1 * torch.randn(int(16000 * seconds), generator=g)).numpy()


@functools.lru_cache(maxsize=None)
def pipe_plan():
    """257 lifted points over the V = 5023 mesh, with a strip of triangles over them as the target's own topology"""
    plan = searched(PIPE_MESH, "lifted", 257)[0]
    faces_t = np.array([(k, k + 1, k + 2) for k in range(255)], dtype=np.int32)
    return plan, faces_t


def test_animate_with_wrap():
    diffusion, ae = tiny_models()
    plan, faces_t = pipe_plan()
    S, _ = WC.source(PIPE_MESH)
    tmpl = S.reshape(1, -1)
    wav = tiny_audio(0.6, 1)
    kw = dict(ddim_steps=3, seed=2, device=DEV)
    offs, lat = pipeline.animate(diffusion, ae, wav, None, **kw)
    got, lat2 = pipeline.animate(diffusion, ae, wav, tmpl, wrap=plan, **kw)
    L = offs.shape[1]
    assert torch.equal(lat, lat2) and got.shape == (1, L, 3 * plan.Vt)
    want = pipeline.to_wrap(offs, plan, tmpl)
    assert torch.equal(got, want) and torch.isfinite(got).all()
    fi, uvh, _ = plan.binding()
    ref = WC.follow(offs.cpu().numpy(), tmpl, [L], plan.faces, fi, uvh, plan.dst_rest)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(ref[0]))
    # the dict of the plan's arguments is the same binding
    got_d, _ = pipeline.animate(diffusion, ae, wav, tmpl, wrap=plan.arguments(), **kw)
    assert torch.equal(got_d, got)
    # faces= is the target's triangle list; out_fps applies to the wrapped frames
    mf, _ = pipeline.animate(diffusion, ae, wav, tmpl, wrap=plan, faces=faces_t, out_fps=60, **kw)
    r = pipeline.to_mesh(want, faces_t, None, fps=(30, 60))
    assert mf.frames == r.frames and torch.equal(mf.positions, r.positions) and torch.equal(mf.normals, r.normals)
    long, _ = pipeline.animate_long(diffusion, ae, wav, tmpl, wrap=plan, **kw)
    assert torch.equal(long, got)                                   # (fits one window: animate()'s bits)
    # wrap=None: the parent behaviour
    a, _ = pipeline.animate(diffusion, ae, wav, tmpl, **kw)
    b, _ = pipeline.animate(diffusion, ae, wav, tmpl, wrap=None, **kw)
    assert torch.equal(a, b) and torch.equal(a, offs + dev(tmpl).unsqueeze(1))
    with pytest.raises(ValueError, match="wrap= with rig="):
        pipeline._hand_off(offs, tmpl, DEV, rig=dict(basis=np.zeros((1, offs.shape[-1]), np.float32)), wrap=plan)


@pytest.mark.parametrize("batch_stages", [False, True])
def test_animate_many_and_slot_server_with_wrap(batch_stages):
    diffusion, ae = tiny_models()
    plan, _ = pipe_plan()
    S, _ = WC.source(PIPE_MESH)
    wavs = [tiny_audio(s, i) for i, s in enumerate((0.6, 0.4))]
    tmpls = [S.reshape(1, -1), MC.template(PIPE_MESH, seed=21)]
    kw = dict(ddim_steps=2, seed=1, device=DEV)
    got, lats = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, wrap=plan, **kw)
    plain, lats0 = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, **kw)
    plain_none, _ = pipeline.animate_many(diffusion, ae, wavs, tmpls, batch_stages=batch_stages, wrap=None, **kw)
    solo = [pipeline.animate(diffusion, ae, wavs[b], tmpls[b], wrap=plan, **kw)[0] for b in range(2)]
    assert got[0].shape[1] != got[1].shape[1]
    for b in range(2):
        assert torch.equal(lats[b], lats0[b]) and torch.equal(plain[b], plain_none[b])
        assert got[b].shape == (1, plain[b].shape[1], 3 * plan.Vt) and torch.equal(got[b], solo[b])
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=64, ddim_steps=2, device=DEV, batch_stages=batch_stages, wrap=plan)
    hs = srv.submit_many(wavs, tmpls, seeds=1)
    res = {h: v for h, v, _ in srv.drain(2)}
    for b, h in enumerate(hs):
        assert torch.equal(res[h], solo[b])
