"""No GPU: the pure helpers of pipeline.py's one request path -- conditions, the start noise, the sampler resolver and its plan
arguments, the template add of the batch hand-off and the ragged packing up to its refusal.  Every expectation is written out here
as the expression the entry points used to spell out themselves; nothing of the code under test forms one."""
import itertools
import types

import pytest
import torch

from fdm_amd import pipeline, presets
from fdm_amd._lib import FdmError

PRESETS = ["vocaset_tiny", "mead_tiny"]


def one_hot(n, i):
    return torch.eye(n)[i]


# ---- conditions ------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", PRESETS)
@pytest.mark.parametrize("rows", [1, 3])
def test_condition_defaults_are_style_row_0_and_emotion_row_4(preset, rows):
    p = presets.get(preset)
    assert (pipeline._STYLE_DEFAULT, pipeline._EMOTION_DEFAULT) == (0, 4)
    got = pipeline._condition(None, p.n_style, pipeline._STYLE_DEFAULT, rows)
    assert got.dtype == torch.float32 and torch.equal(got, torch.eye(p.n_style)[:1].expand(rows, -1))
    if p.n_emo:
        got = pipeline._condition(None, p.n_emo, pipeline._EMOTION_DEFAULT, rows)
        assert got.dtype == torch.float32 and torch.equal(got, torch.eye(p.n_emo)[4:5].expand(rows, -1))
        assert got.argmax(dim=1).tolist() == [4] * rows and pipeline.EMOTIONS[4] == "happy"


@pytest.mark.parametrize("preset", PRESETS)
def test_condition_shapes_come_back_as_rows_by_width(preset):
    p = presets.get(preset)
    rows = 3
    for n in [p.n_style] + ([p.n_emo] if p.n_emo else []):
        v = one_hot(n, 1)
        want = v.reshape(1, n).expand(rows, -1)
        for given in (v, v.reshape(1, n), v.double(), v.numpy()):                      # [n], [1, n], another dtype, an array
            got = pipeline._condition(given, n, 0, rows)
            assert got.dtype == torch.float32 and got.shape == (rows, n) and torch.equal(got, want)
        full = torch.stack([one_hot(n, i % n) for i in range(rows)])                  # [rows, n]: as it is
        got = pipeline._condition(full, n, 0, rows)
        assert got.dtype == torch.float32 and torch.equal(got, full)
        assert torch.equal(pipeline._condition(full.reshape(-1), n, 0, rows), full)   # any shape of rows * n numbers
        assert pipeline._condition(v, n, 0, 1).shape == (1, n)


# ---- start noise -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 32, 16), (3, 32, 16)])
@pytest.mark.parametrize("seed", [0, 7])
def test_start_noise_is_one_cpu_draw_of_the_shape(shape, seed):
    got = pipeline._start_noise(shape, seed)
    assert got.device.type == "cpu" and got.dtype == torch.float32
    assert torch.equal(got, torch.randn(shape, generator=torch.Generator(device="cpu").manual_seed(seed)))


def test_a_batch_draw_is_not_the_per_clip_draws():
    """[B, n, c] from one generator is not B draws of [1, n, c] from fresh generators: every caller keeps its own shape."""
    batch = pipeline._start_noise((3, 32, 16), 5)
    singles = torch.cat([pipeline._start_noise((1, 32, 16), 5) for _ in range(3)])
    assert torch.equal(singles[0], singles[1]) and torch.equal(singles[0], singles[2])  # a fresh generator each: the same draw
    assert not torch.equal(batch, singles) and not torch.equal(batch[1], batch[0])


# ---- sampler resolver ------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,ddim_steps,sampler,on_emotion",
                         itertools.product(PRESETS, [None, 6], [None, "dpmpp2m", "ddim_eta"], [False, True]))
def test_sampler_definition_table(preset, ddim_steps, sampler, on_emotion):
    p = presets.get(preset)
    if sampler:
        want = ("tables", sampler, 20, 0.5)                                            # sampler= wins on every preset
    elif ddim_steps and (on_emotion or not p.n_emo):
        want = ("ddim", 6)
    else:
        want = ("ddpm",)                                                               # ddim_steps ignored on an emotion preset
    got = pipeline._sampler_definition(p, ddim_steps, sampler, 20, 0.5, ddim_on_emotion=on_emotion)
    assert got == want and hash(got) == hash(want)
    if not on_emotion:
        assert pipeline._sampler_definition(p, ddim_steps, sampler, 20, 0.5) == want   # the default: as animate() chooses


@pytest.mark.parametrize("full_chain,T", [(True, 1000), (True, 50), (False, 1000)])
def test_ddpm_definition_gives_the_step_list(full_chain, T):
    d = types.SimpleNamespace(num_timesteps=T, full_chain=full_chain)
    a = pipeline._sampler_args(("ddpm",), d)
    assert a == dict(kind="ddpm", t_list=list(range(T - 1, -1, -1)) if full_chain else list(range(999, 499, -1)))
    assert a["t_list"][0] == (T - 1 if full_chain else 999) and a["t_list"][-1] == (0 if full_chain else 500)


def test_ddim_and_tables_definitions_give_their_plan_arguments():
    from fdm_amd import schedule
    d = types.SimpleNamespace(num_timesteps=1000, full_chain=True)
    assert pipeline._sampler_args(("ddim", 6), d) == dict(kind="ddim", steps=6)
    a = pipeline._sampler_args(("tables", "dpmpp2m", 5, 0.0), d)
    t_list, tables = schedule.sampler_tables("dpmpp2m", 5, 0.0, 1000)
    assert a["kind"] == "tables" and list(a["t_list"]) == list(t_list) and torch.equal(torch.as_tensor(a["tables"]), torch.as_tensor(tables))


# ---- batch hand-off, template only ----------------------------------------------------------------
def test_hand_off_adds_the_template():
    g = torch.Generator().manual_seed(3)
    V3, L = 12, 5
    out = torch.randn(1, L, V3, generator=g)
    tmpl = torch.randn(1, V3, generator=g)
    assert pipeline._hand_off(out, None, "cpu") is out
    for given in (tmpl, tmpl.reshape(-1), tmpl.numpy(), tmpl.double()):
        got = pipeline._hand_off(out, given, "cpu")
        assert torch.equal(got, out + torch.as_tensor(tmpl, dtype=torch.float32).reshape(-1, 1, V3))


def test_hand_off_repeats_a_per_clip_template_per_condition():
    g = torch.Generator().manual_seed(4)
    V3, L, B, S = 12, 5, 2, 2
    out = torch.randn(B * S, L, V3, generator=g)                                       # rows in (clip, condition) order
    per_clip = torch.randn(B, V3, generator=g)
    got = pipeline._hand_off(out, per_clip, "cpu", S=S, B=B)
    assert torch.equal(got, out + per_clip.reshape(-1, 1, V3).repeat_interleave(S, dim=0))
    for row in range(B * S):
        assert torch.equal(got[row], out[row] + per_clip[row // S])
    single = torch.randn(1, V3, generator=g)                                           # one template: broadcast over every row
    got = pipeline._hand_off(out, single, "cpu", S=S, B=B)
    assert torch.equal(got, out + single.reshape(-1, 1, V3))
    rows = torch.randn(B * S, V3, generator=g)                                         # one per (clip, condition): row by row
    assert torch.equal(pipeline._hand_off(out, rows, "cpu", S=S, B=B), out + rows.reshape(-1, 1, V3))


# ---- ragged packing --------------------------------------------------------------------------------
@pytest.mark.parametrize("who", ["to_mesh", "to_rig"])
def test_packing_refuses_host_tensors_in_the_callers_name(who):
    clips = [torch.zeros(1, 4, 6), torch.zeros(7, 6)]
    for offsets, device in ((clips, None), (clips, "cuda:0"), (torch.zeros(2, 4, 6), None), (torch.zeros(4, 6), "cpu")):
        with pytest.raises(FdmError, match=f"^{who} runs on the HIP path only"):
            pipeline._pack_offsets(offsets, None, device, who)


def test_the_public_hand_offs_name_themselves():
    with pytest.raises(FdmError, match="^to_mesh runs on the HIP path only"):
        pipeline.to_mesh([torch.zeros(1, 4, 6)], [[0, 1, 2]])
    with pytest.raises(FdmError, match="^to_rig runs on the HIP path only"):
        pipeline.to_rig(torch.zeros(1, 4, 6), torch.zeros(2, 6))
