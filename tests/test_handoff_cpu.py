"""CPU: what the hand-off plans share in Python (fdm_amd/handoff.py) -- the frame list, the fps pair, L_out_max of new outputs, the
offsets check, and the one plan cache's get-or-make with its reuse / remake-elsewhere rule, on a stub factory (no device)."""
import pytest
import torch

import mesh_cases as MC
from fdm_amd import handoff, mesh
from fdm_amd._lib import FdmError


def test_frames_list_and_fps_pair():
    assert handoff.frames_list(None, 3, 7) == [7, 7, 7]
    assert handoff.frames_list((0, 1.0, torch.tensor(7)), 3, 7) == [0, 1, 7]
    with pytest.raises(FdmError, match="2 frame counts for 3 clips"):
        handoff.frames_list([1, 2], 3, 7)
    assert handoff.fps_pair(None) == (0.0, 0.0)
    assert handoff.fps_pair((30, 25)) == (30.0, 25.0) and all(isinstance(f, float) for f in handoff.fps_pair((30, 25)))
    assert handoff.fps_pair((None, 60)) == (0.0, 60.0) and handoff.fps_pair((30, 0)) == (30.0, 0.0)


def test_frames_out_is_the_library_rule_and_stays_importable_from_mesh():
    assert mesh.frames_out is handoff.frames_out
    for fps in MC.RATES + [(0, 60), (30, 0)]:
        for L in (0, 1, 2, 7, 498):
            assert handoff.frames_out(L, *fps) == MC.frames_out(L, fps)
    for fps in MC.RATES:
        fr = [0, 1, 7]
        assert handoff.frames_out_max(fr, *map(float, fps)) == max(MC.frames_out(L, fps) for L in fr)
    assert handoff.frames_out_max([0, 0], 30.0, 60.0) == 1          # an output is at least one row long
    assert handoff.frames_out_max([1], 30.0, 25.0) == 1             # L_out = max(1, int(1 / 30 * 25))


def test_offsets_batch():
    dv = torch.device("cpu")
    x = torch.zeros(7, 6)
    assert tuple(handoff.offsets_batch(x, 2, dv).shape) == (1, 7, 6)
    y = torch.zeros(2, 7, 12)[:, :, ::2]
    got = handoff.offsets_batch(y, 2, dv)
    assert got.is_contiguous() and tuple(got.shape) == (2, 7, 6)
    for bad in (torch.zeros(2, 7, 5), torch.zeros(2, 7, 6, dtype=torch.float64), torch.zeros(1, 2, 7, 6)):
        with pytest.raises(FdmError, match=r"offsets must be float32 \[B, L, 6\] on cpu"):
            handoff.offsets_batch(bad, 2, dv)
    with pytest.raises(FdmError, match=r"on cuda:0, got torch.float32 \(2, 7, 6\) on cpu"):
        handoff.offsets_batch(torch.zeros(2, 7, 6), 2, torch.device("cuda:0"))


class Stub:
    made = 0

    def __init__(self, device, stream):
        self.device, self.stream = torch.device(device), stream
        Stub.made += 1


def test_cached_plan_get_or_make(monkeypatch):
    monkeypatch.setattr(handoff, "_PLANS", {})
    Stub.made = 0
    at, other, elsewhere = ("cuda:0", 11), ("cuda:0", 12), ("cuda:1", 11)
    make = lambda a: (lambda: Stub(*a))  # noqa: E731
    p = handoff.cached_plan(at, "mesh", ("id", 1), make(at))
    assert handoff.cached_plan(at, "mesh", ("id", 1), make(at)) is p and Stub.made == 1           # a hit makes nothing
    # the key is (device, stream, kind, identity): each of them apart is another plan
    q = [handoff.cached_plan(other, "mesh", ("id", 1), make(other)), handoff.cached_plan(elsewhere, "mesh", ("id", 1), make(elsewhere)),
         handoff.cached_plan(at, "rig", ("id", 1), make(at)), handoff.cached_plan(at, "mesh", ("id", 2), make(at))]
    assert len({id(x) for x in q + [p]}) == 5 and Stub.made == 5 and len(handoff._PLANS) == 5
    assert set(handoff._PLANS) >= {at + ("mesh", ("id", 1)), at + ("rig", ("id", 1))}


def test_cached_plan_uses_a_given_plan_where_it_was_made_and_remakes_it_elsewhere(monkeypatch):
    monkeypatch.setattr(handoff, "_PLANS", {})
    Stub.made = 0
    at, other, elsewhere = ("cuda:0", 11), ("cuda:0", 12), ("cuda:1", 11)
    mine = Stub(*at)
    never = lambda: pytest.fail("a plan made for this device and stream is used as it is")  # noqa: E731
    assert handoff.cached_plan(at, "rig", "k", never, mine) is mine and Stub.made == 1
    for where in (other, elsewhere):                            # another stream, another device: made again from its arguments
        got = handoff.cached_plan(where, "rig", "k", lambda: Stub(*where), mine)
        assert got is not mine and (str(got.device), got.stream) == where
        assert handoff.cached_plan(where, "rig", "k", never, mine) is got         # and kept
    assert Stub.made == 3
    twin = Stub(*at)                                            # a second plan of the same identity: the cached one serves
    assert handoff.cached_plan(at, "rig", "k", never, twin) is mine
    host = Stub("cuda:0", None)                                 # made without a visible device: never taken as it is
    assert handoff.cached_plan(at, "flame", "k", lambda: Stub(*at), host) is not host
