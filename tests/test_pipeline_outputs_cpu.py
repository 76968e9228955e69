"""No GPU: the chain that turns decoded offsets into what animate / animate_many / animate_long / SlotServer return, characterised
with every device stage replaced by a stub that records what it was handed.  All 32 combinations of faces / rig / flame / wrap / render,
in the batch form and in the ragged form, against a table written out here from the definition in the chain's docstring (_hand_off
and _hand_off_many are the chain for a caller that holds fps itself): the refusal, or the stages in order with what each received, and
the kind of thing that comes back."""
import itertools
import types

import numpy as np
import pytest
import torch

from fdm_amd import pipeline, presets

V3, VT3 = 12, 9                                   # the model's 4 vertices, the wrap target's 3
FPS = (30.0, 60.0)
FACES = np.array([[0, 1, 2], [0, 2, 3]])
POSED, WRAPPED = 2.0, 3.0                         # what the head and wrap stubs fill their vertices with


def keywords():
    """One valid value per output keyword (the dicts are real ones: their identity is digested where a plan is looked up)."""
    g = np.random.default_rng(0)
    return dict(faces=FACES, rig=dict(basis=g.standard_normal((2, V3)).astype(np.float32)), flame=dict(model=object(), pose=np.zeros((5, 15), np.float32)),
                wrap=dict(src_rest=g.standard_normal((4, 3)).astype(np.float32), faces=FACES, dst_rest=g.standard_normal((3, 3)).astype(np.float32)),
                render=dict(camera="vocaset"))


REFUSALS = {"render": "render= needs faces=: the triangle list of the mesh that is drawn (after wrap=, the target's)",
            "flame": "flame= with rig= and no faces=: the call would return the fit of the un-posed offsets alone and never pose anything",
            "wrap": "wrap= with rig= and no faces=: the call would return the fit of the model's own offsets alone and never wrap anything"}

# Keys: F faces, R rig, H flame (the head), W wrap, I render (images).  A value is the refusals that apply, in the batch form's
# order, or (stages, what comes back): a stage is name<what it received, +T where the template goes in with it.  rig always reads
# the offsets; after the head or the wrap nothing takes a template; the vertices that come back bare are offsets + T, or the posed
# or wrapped ones as they are.
TABLE = {
    "": ("", "offsets+T"),
    "F": ("mesh<offsets+T", "mesh"),
    "R": ("rig<offsets", "rig"),
    "FR": ("rig<offsets mesh<offsets+T", "mesh,rig"),
    "H": ("flame<offsets", "posed"),
    "FH": ("flame<offsets mesh<posed", "mesh"),
    "RH": ["flame"],
    "FRH": ("rig<offsets flame<offsets mesh<posed", "mesh,rig"),
    "W": ("wrap<offsets+T", "wrapped"),
    "FW": ("wrap<offsets+T mesh<wrapped", "mesh"),
    "RW": ["wrap"],
    "FRW": ("rig<offsets wrap<offsets+T mesh<wrapped", "mesh,rig"),
    "HW": ("flame<offsets wrap<posed", "wrapped"),
    "FHW": ("flame<offsets wrap<posed mesh<wrapped", "mesh"),
    "RHW": ["flame", "wrap"],
    "FRHW": ("rig<offsets flame<offsets wrap<posed mesh<wrapped", "mesh,rig"),
    "I": ["render"],
    "FI": ("render<offsets+T", "render"),
    "RI": ["render"],
    "FRI": ("rig<offsets render<offsets+T", "render,rig"),
    "HI": ["render"],
    "FHI": ("flame<offsets render<posed", "render"),
    "RHI": ["render", "flame"],
    "FRHI": ("rig<offsets flame<offsets render<posed", "render,rig"),
    "WI": ["render"],
    "FWI": ("wrap<offsets+T render<wrapped", "render"),
    "RWI": ["render", "wrap"],
    "FRWI": ("rig<offsets wrap<offsets+T render<wrapped", "render,rig"),
    "HWI": ["render"],
    "FHWI": ("flame<offsets wrap<posed render<wrapped", "render"),
    "RHWI": ["render", "flame", "wrap"],
    "FRHWI": ("rig<offsets flame<offsets wrap<posed render<wrapped", "render,rig"),
}
LETTERS = dict(F="faces", R="rig", H="flame", W="wrap", I="render")


class Tag:
    """What a stubbed hand-off returns: its name and, in the ragged form, the clip."""

    def __init__(self, name, clip=None):
        self.name, self.clip = name, clip


def pack(offsets, frames, device, who):
    """pipeline._pack_offsets without its refusal of host tensors: the zero-padded batch of a ragged list, a tensor as it is."""
    if not isinstance(offsets, (list, tuple)):
        return offsets, frames, False
    frames = [int(c.shape[-2]) for c in offsets]
    x = torch.zeros(len(offsets), max(frames), offsets[0].shape[-1])
    for b, c in enumerate(offsets):
        x[b, :frames[b]] = c.reshape(-1, c.shape[-1])
    return x, frames, True


class Stages:
    """The five device stages as stubs.  calls: (stage, what it was handed, whether a template came with it, fps) in call order."""

    def __init__(self, monkeypatch, offsets):
        self.offsets, self.calls, self.rig_input, self.flame_seen, self.plans = offsets, [], None, None, []
        for name in ("to_rig", "to_wrap", "to_mesh", "to_images", "_flame_posed"):
            monkeypatch.setattr(pipeline, name, getattr(self, name))
        monkeypatch.setattr(pipeline, "_pack_offsets", pack)
        # no device here: a plan that is looked up is a placeholder, and the look-ups are counted
        monkeypatch.setattr(pipeline, "_on_stream", lambda device: (torch.device("cpu"), ("cpu", 0)))
        monkeypatch.setattr(pipeline, "cached_plan", lambda at, kind, identity, make, given=None: self.plans.append(kind) or Tag(kind + " plan"))

    def origin(self, x):
        """Which vertices a stage was handed: the decoder's offsets, the posed head's or the wrapped mesh's."""
        many = isinstance(x, (list, tuple))
        clips, mine = (list(x), list(self.offsets)) if many else ([x], [self.offsets])
        if isinstance(self.offsets, (list, tuple)) and not many:      # the ragged head call takes the packed batch
            mine = [pack(self.offsets, None, None, None)[0]]
        if len(clips) == len(mine) and all(c.shape == m.shape and torch.equal(c, m) for c, m in zip(clips, mine)):
            return "offsets"
        for value, name in ((POSED, "posed"), (WRAPPED, "wrapped")):
            if all(bool((c == value).all()) for c in clips):
                return name
        return "?"

    def result(self, name, x):
        return [Tag(name, b) for b in range(len(x))] if isinstance(x, (list, tuple)) else Tag(name)

    def to_rig(self, offsets, basis, frames=None, fps=None, **kw):
        self.calls.append(("rig", self.origin(offsets), False, fps))
        self.rig_input = offsets
        return self.result("rig", offsets)

    def _flame_posed(self, out, flame, device, frames=None, S=1, B=1):
        self.calls.append(("flame", self.origin(out), False, None))
        self.flame_seen = (flame, frames)
        return torch.full_like(out, POSED)

    def to_wrap(self, offsets, wrap, template=None, frames=None, offsets_out=False, device=None):
        self.calls.append(("wrap", self.origin(offsets), template is not None, None))
        if isinstance(offsets, (list, tuple)):
            return [torch.full((1, c.shape[-2], VT3), WRAPPED) for c in offsets]
        return torch.full(tuple(offsets.shape[:2]) + (VT3,), WRAPPED)

    def to_mesh(self, offsets, faces, template=None, frames=None, fps=None, **options):
        self.calls.append(("mesh", self.origin(offsets), template is not None, fps))
        return self.result("mesh", offsets)

    def to_images(self, offsets, faces, render, template=None, frames=None, fps=None, device=None, **options):
        self.calls.append(("render", self.origin(offsets), template is not None, fps))
        return self.result("render", offsets)


def expected_calls(stages):
    """'rig<offsets mesh<offsets+T' -> the records Stages keeps: rig, mesh and render are handed the frame rates, the others none."""
    out = []
    for s in stages.split():
        name, src = s.split("<")
        out.append((name, src.replace("+T", ""), src.endswith("+T"), FPS if name in ("rig", "mesh", "render") else None))
    return out


def check_result(got, kind, ragged, offsets, templates):
    """What comes back: bare vertices (a tensor, or a list with one per clip), a hand-off's object, or the pair with the fit."""
    clips = list(got) if ragged else [got]
    assert (isinstance(got, list) and len(got) == len(offsets)) if ragged else not isinstance(got, list)
    for b, c in enumerate(clips):
        mine = offsets[b] if ragged else offsets
        if kind == "offsets+T":
            tp = templates[b] if ragged else templates
            assert torch.equal(c, mine + tp.reshape(-1, 1, V3))
        elif kind in ("posed", "wrapped"):        # as they are: no template is added to them
            width, value = (V3, POSED) if kind == "posed" else (VT3, WRAPPED)
            assert c.shape == mine.shape[:2] + (width,) and bool((c == value).all())
        elif "," in kind:
            assert isinstance(c, tuple) and [t.name for t in c] == kind.split(",") and all(t.clip == (b if ragged else None) for t in c)
        else:
            assert isinstance(c, Tag) and c.name == kind and c.clip == (b if ragged else None)


@pytest.mark.parametrize("ragged", [False, True], ids=["batch", "ragged"])
@pytest.mark.parametrize("key", list(TABLE), ids=[k or "none" for k in TABLE])
def test_the_chain_for_every_combination_of_outputs(key, ragged, monkeypatch):
    assert len(TABLE) == 32 and set(TABLE) == {"".join(c for c, on in zip("FRHWI", bits) if on) for bits in itertools.product([0, 1], repeat=5)}
    g = torch.Generator().manual_seed(11)
    kw = {LETTERS[c]: keywords()[LETTERS[c]] for c in key}
    fps = FPS if ("faces" in kw or "rig" in kw) else None          # as every entry point states it: only with faces= or rig=
    if ragged:
        offsets = [torch.randn(1, L, V3, generator=g) for L in (3, 5)]
        templates = [torch.randn(1, V3, generator=g) for _ in offsets]
        if "flame" in kw:      # one pose per clip, each of its own length
            kw["flame"] = dict(kw["flame"], pose=[np.ones((L, 15), np.float32) for L in (3, 5)])
        call = lambda: pipeline._hand_off_many(offsets, templates, "cpu", fps=fps, **kw)  # noqa: E731
    else:
        offsets, templates = torch.randn(2, 5, V3, generator=g), torch.randn(1, V3, generator=g)
        call = lambda: pipeline._hand_off(offsets, templates, "cpu", fps=fps, **kw)  # noqa: E731
    st = Stages(monkeypatch, offsets)
    want = TABLE[key]
    if isinstance(want, list):
        with pytest.raises(ValueError) as e:
            call()
        # the batch form's order is render, flame, wrap; where two apply the ragged form has raised either of them
        assert str(e.value) in ([REFUSALS[r] for r in want] if ragged else [REFUSALS[want[0]]]) and not st.calls
        return
    got = call()
    calls = expected_calls(want[0])
    if ragged:      # the fit reads nothing another stage writes, and the ragged form has made its one fit call last: its place is not held
        assert [c for c in st.calls if c[0] == "rig"] == [c for c in calls if c[0] == "rig"]
        assert [c for c in st.calls if c[0] != "rig"] == [c for c in calls if c[0] != "rig"]
    else:
        assert st.calls == calls
    if "R" in key:              # fitted on the original offsets: the very object, whatever the head or the wrap made of them since
        assert st.rig_input is offsets
    assert all(not with_template for name, src, with_template, _ in st.calls if src != "offsets")      # none after the head or the wrap
    if ragged and "H" in key:   # the per-clip poses padded into one batch for the one head call
        flame, frames = st.flame_seen
        assert frames == [3, 5] and tuple(flame["pose"].shape) == (2, 5, 15) and bool((flame["pose"][0, 3:] == 0).all()) and bool((flame["pose"][0, :3] == 1).all())
    check_result(got, want[1], ragged, offsets, templates)


def test_nothing_asked_for_returns_the_very_offsets(monkeypatch):
    clips = [torch.zeros(1, 3, V3), torch.zeros(1, 5, V3)]
    Stages(monkeypatch, clips)
    assert pipeline._hand_off_many(clips, None, "cpu") is clips and pipeline._hand_off(clips[0], None, "cpu") is clips[0]


# ---- a rig= dict becomes a plan once per animate_many call and once per SlotServer ----------------
def fake_models(p):
    """(diffusion, autoencoder) that run nowhere: an encoder that returns zeros of the right length, a decoder that returns zeros."""
    hidden = lambda w: types.SimpleNamespace(last_hidden_state=torch.zeros(1, p.pair * max(w.shape[-1] // 100, 1), 4))  # noqa: E731
    plan = types.SimpleNamespace(open_slots=lambda *a, **k: object())
    model = types.SimpleNamespace(preset=p, audio_encoder=hidden, _hub_key=None, _hub=None, _prep_key=None, set_audio_features=lambda hub: None,
                                  plan=lambda device: plan)
    ae = types.SimpleNamespace(decode=lambda z: torch.zeros(1, z.shape[1] // p.G, p.V3))
    return types.SimpleNamespace(denoise_fn=model, num_timesteps=1000, full_chain=True), ae


def test_a_rig_dict_is_resolved_once_per_call_and_once_per_server(monkeypatch):
    p = presets.get("vocaset_tiny")
    diffusion, ae = fake_models(p)
    st = Stages(monkeypatch, None)
    st.origin = lambda x: None
    monkeypatch.setattr(pipeline, "_sample", lambda diffusion, key, audio, shape, *a, **k: torch.zeros(shape))
    monkeypatch.setattr(pipeline, "_quantise", lambda ae, p, latent, *a, **k: latent)
    rig = dict(basis=np.zeros((2, p.V3), np.float32))
    fits, lats = pipeline.animate_many(diffusion, ae, [np.zeros(100 * n, np.float32) for n in (2, 3, 4)], rig=rig, out_fps=60, device="cpu", max_batch=1,
                                       ddim_steps=2)
    assert st.plans == ["rig"] and len(st.calls) == 3                      # three groups, three ragged rig calls, one plan
    assert [f.name for f in fits] == ["rig"] * 3 and [tuple(x.shape) for x in lats] == [(1, n * p.G, p.c) for n in (2, 3, 4)]
    assert all(c[3] == (float(p.fps), 60.0) for c in st.calls)
    del st.plans[:], st.calls[:]
    srv = pipeline.SlotServer(diffusion, ae, slots=2, max_frames=8, ddim_steps=2, device="cpu", rig=rig)
    for h in range(2):
        srv._finish_one([], torch.zeros(1, 2 * p.G, p.c), dict(handle=h, template=None, emo=None))
    assert st.plans == ["rig"] and len(st.calls) == 2 and [v.name for _, v, _ in srv.results()] == ["rig"] * 2
