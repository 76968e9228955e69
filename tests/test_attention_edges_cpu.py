"""CPU: the per-element attention bound and the case list of tests/attn_cases.py, proven before a GPU is involved.

emulate() restates the algorithm of csrc/attention.hpp in torch fp32, in the kernel's own order: key tiles of 16 (fp32) or 32
(16-bit kinds) keys dealt round-robin to four partial (m, l, O) states, a running maximum with the rescale, the periodic ALiBi
step rebuilt from (D, rem, j) per lane group, the mask, the probabilities rounded to the kind, the merge, O rounded to the kind.
The clean emulation stays inside bound() on every case the GPU file runs; each seeded defect (the mistakes this kernel invites)
breaks the bound on at least one case, for every kind it applies to -- so the inputs can see those mistakes."""
import functools
import math

import pytest
import torch

import attn_cases as AC
from attn_cases import BF16, F16, F16X3, F32

LOG2E = 1.4426950408889634
DEFECTS = ["rem_ge", "pads_unmasked", "no_rescale", "goff_4g", "causal_wide"]
PAD_FILL = 64.0


def _round(kind, x):
    """fp32 -> the value the kind stores."""
    if kind == BF16:
        return x.bfloat16().float()
    if kind == F16:
        return x.clamp(-65504.0, 65504.0).half().float()
    if kind == F16X3:
        pl = AC.split_host(x)
        return pl[0].float() + pl[1].float() / AC.SPLIT_SCALE
    return x


def _pad_keys(x, Lpad, fill):
    B, H, L, hd = x.shape
    out = torch.full((B, H, Lpad, hd), fill, dtype=x.dtype)
    out[:, :, :L] = x
    return out


def emulate(kind, opnd, scale, causal, slopes, period, pad_fill=PAD_FILL, defect=None):
    B, H, L, hd = opnd.B, opnd.H, opnd.L, opnd.hd
    Lpad = AC.kv_pad(L)
    f32 = torch.float32
    if kind == F16X3:      # three passes: hi.hi + (hi.lo + lo.hi) / 2^11
        qh, ql = opnd.planes[0][0].float(), opnd.planes[0][1].float()
        kh, kl = (_pad_keys(opnd.planes[1][p].float(), Lpad, pad_fill) for p in (0, 1))
        vh, vl = (_pad_keys(opnd.planes[2][p].float(), Lpad, pad_fill) for p in (0, 1))
    else:
        qh = opnd.planes[0].float()
        kh, vh = _pad_keys(opnd.planes[1].float(), Lpad, pad_fill), _pad_keys(opnd.planes[2].float(), Lpad, pad_fill)
    KT = 16 if kind == F32 else 32
    GK = KT // 4                                             # keys per lane group: goff = GK * g, j < GK
    fast = kind in (BF16, F16)                               # log2 domain, exp2
    LG = torch.tensor(LOG2E if fast else 1.0, dtype=f32)
    ex = torch.exp2 if fast else torch.exp
    sc_mul = torch.tensor(scale, dtype=f32) * LG
    slope = (slopes.float() * LG).view(1, H, 1, 1) if slopes is not None else None
    inv_period = torch.tensor(1.0, dtype=f32) / torch.tensor(float(period), dtype=f32)
    fastbias = slopes is None or period >= 8
    qi = torch.arange(L).view(L, 1)
    sub0 = (qi // 16) * 16                                   # first query of the 16-query sub-tile
    NEG = float("-inf")
    m = [torch.full((B, H, L), NEG) for _ in range(4)]
    l = [torch.zeros(B, H, L) for _ in range(4)]
    o = [torch.zeros(B, H, L, hd) for _ in range(4)]
    for kt in range((L + KT - 1) // KT):
        w, kbase = kt % 4, kt * KT
        proc = (kbase <= sub0 + 15) if causal else torch.ones(L, 1, dtype=torch.bool)       # [L, 1]: the causal tile skip
        if not bool(proc.any()):
            continue
        kk = slice(kbase, kbase + KT)
        s = torch.einsum("bhid,bhjd->bhij", qh, kh[:, :, kk])
        if kind == F16X3:
            s = s + (torch.einsum("bhid,bhjd->bhij", qh, kl[:, :, kk]) + torch.einsum("bhid,bhjd->bhij", ql, kh[:, :, kk])) * (1.0 / AC.SPLIT_SCALE)
        s = s * sc_mul
        wk = torch.arange(KT).view(1, KT)
        g, j = wk // GK, wk % GK
        key = kbase + wk
        if slope is not None:
            goff = (4 if (defect == "goff_4g" and kind != F32) else GK) * g
            D = qi - kbase - goff                            # [L, KT]
            if fastbias:
                f0 = torch.floor((D.float() + 0.5) * inv_period)
                rem = D - f0.int() * period
                b0 = slope * f0
                b1 = b0 - slope
                s = s - torch.where((j >= rem) if defect == "rem_ge" else (j > rem), b1, b0)
            else:
                s = s - slope * torch.floor(((D - j).float() + 0.5) * inv_period)
        vis = key <= (L - 1 if defect != "pads_unmasked" else Lpad)
        if causal:
            vis = vis & (key <= qi + (1 if defect == "causal_wide" else 0))
        s = s.masked_fill(~vis, NEG)
        mx = s.amax(-1)
        m_new = torch.maximum(m[w], mx)
        safe = torch.where(torch.isfinite(m_new), m_new, torch.zeros_like(m_new))
        alpha = ex(m[w] - safe)
        p = ex(s - safe.unsqueeze(-1))
        l_new = l[w] * alpha + p.sum(-1)
        if kind == F16X3:
            ph = p.half().float()
            pl_ = ((p - ph) * AC.SPLIT_SCALE).half().float()
            pv = torch.einsum("bhij,bhjd->bhid", ph, vh[:, :, kk]) + (torch.einsum("bhij,bhjd->bhid", pl_, vh[:, :, kk]) + torch.einsum("bhij,bhjd->bhid", ph, vl[:, :, kk])) * (1.0 / AC.SPLIT_SCALE)
        else:
            pv = torch.einsum("bhij,bhjd->bhid", _round(kind, p), vh[:, :, kk])
        o_new = (o[w] if defect == "no_rescale" else o[w] * alpha.unsqueeze(-1)) + pv
        pr = proc.view(1, 1, L)
        m[w] = torch.where(pr, m_new, m[w])
        l[w] = torch.where(pr, l_new, l[w])
        o[w] = torch.where(pr.unsqueeze(-1), o_new, o[w])
    ms = torch.stack(m).amax(0)
    lsum, acc = torch.zeros(B, H, L), torch.zeros(B, H, L, hd)
    for w in range(4):
        sw = ex(m[w] - ms)
        lsum = lsum + sw * l[w]
        acc = acc + o[w] * sw.unsqueeze(-1)
    return _round(kind, acc * (1.0 / lsum).unsqueeze(-1))


@functools.lru_cache(maxsize=None)
def prepared(kind, case):
    """Operands, reference and bound of one (kind, case): computed once, shared by the clean run and the defects, never modified."""
    opnd = AC.operands(kind, *case.inputs())
    ref = AC.reference(opnd.q, opnd.k, opnd.v, case.scale, case.causal, case.slope_values(), case.period)
    return opnd, ref, AC.bound(kind, ref, case.hd)


def ratio(kind, case, defect=None):
    opnd, ref, bnd = prepared(kind, case)
    out = emulate(kind, opnd, case.scale, case.causal, case.slope_values(), case.period, defect=defect)
    return AC.worst(out, ref, bnd)


@pytest.mark.parametrize("kind", AC.KINDS, ids=lambda k: AC.KIND_NAMES[k])
def test_clean_emulation_is_inside_the_bound_on_every_case(kind):
    bad = []
    for case in AC.CASES:
        r, idx, err, bnd = ratio(kind, case)
        if not r <= 1.0:
            bad.append(f"{case.id}: error / bound = {r:.3g} at (b, h, i, e) = {idx} (|err| {err:.3g}, bound {bnd:.3g})")
    assert not bad, "\n".join(bad)


def _applies(defect, kind, case):
    if defect == "rem_ge":
        return case.slopes != "none" and case.period >= 8
    if defect == "goff_4g":
        return kind != F32 and case.slopes != "none"
    if defect == "causal_wide":
        return case.causal
    return True


@pytest.mark.parametrize("kind", AC.KINDS, ids=lambda k: AC.KIND_NAMES[k])
@pytest.mark.parametrize("defect", DEFECTS)
def test_seeded_defect_breaks_the_bound(defect, kind):
    """j >= rem for j > rem in the periodic step; pad keys (holding 64) left unmasked; the rescale of O skipped; the 16-bit lane
    group offset 8g taken as 4g in the bias only; a causal mask one key too wide."""
    if defect == "goff_4g" and kind == F32:
        return      # the fp32 kind's lane groups hold 4 keys: 4g IS its offset, there is nothing to seed
    caught = []
    for case in AC.CASES:
        if _applies(defect, kind, case):
            r = ratio(kind, case, defect)[0]
            if not r <= 1.0:
                caught.append((case.id, r))
                if len(caught) >= 3:
                    break
    assert caught, f"defect {defect} survives every case for kind {AC.KIND_NAMES[kind]}"


def test_inputs_are_what_they_claim():
    """peaked_late: scores reach about 60 and the row maximum sits at the last visible key tile; peaked_early: in the first one;
    fp16 operands of every builder stay finite; skewed_v spans six decades between columns."""
    q, k, v = AC.peaked_late(1, 1, 130, 64)
    s = torch.einsum("id,jd->ij", q[0, 0].double(), k[0, 0].double()) / 8.0
    assert 45.0 < float(s.max()) < 80.0
    assert int(s[-1].argmax()) >= 130 - 32 and int(s[-1, :98].argmax()) >= 64      # still moving in every tile
    q, k, v = AC.peaked_early(1, 1, 130, 64)
    s = torch.einsum("id,jd->ij", q[0, 0].double(), k[0, 0].double()) / 8.0
    assert 45.0 < float(s.max()) < 80.0 and int(s[-1].argmax()) < 32
    for name, fn in AC.BUILDERS.items():
        for t in fn(1, 3, 65, 64):
            assert torch.isfinite(t.half().float()).all(), name
    v = AC.skewed_v(1, 1, 17, 64)[2]
    assert float(v[..., 5].abs().mean()) > 1e5 * float(v[..., 6].abs().mean())


def test_pack_host_pad_fill_and_split_planes():
    """pad_fill lands on exactly the pad keys' slots; a split kind is packed plane by plane in the 16-bit layout."""
    g = torch.Generator().manual_seed(1)
    k, v = torch.randn(2, 3, 17, 64, generator=g), torch.randn(2, 3, 17, 64, generator=g)
    for kind in (F32, BF16):
        k0, v0 = AC.pack_host(k, v, 32, kind, 0.0)
        k1, v1 = AC.pack_host(k, v, 32, kind, 64.0)
        for a, b in ((k0, k1), (v0, v1)):
            diff = a != b
            assert int(diff.sum()) == 6 * (32 - 17) * 64 and bool((b[diff] == 64.0).all())
    pl = AC.split_host(k), AC.split_host(v)
    ks, vs = AC.pack_host(pl[0], pl[1], 32, F16X3, 0.0)
    for p in (0, 1):
        kb, vb = AC.pack_host(pl[0][p], pl[1][p], 32, BF16, 0.0)
        assert torch.equal(ks[p], kb) and torch.equal(vs[p], vb)
    assert float((AC.exact(F16X3, pl[0]) - k.double()).abs().max()) <= 2.0 ** -22 * float(k.abs().max())


def test_case_list_meets_every_edge():
    cs = AC.CASES
    assert {c.hd for c in cs} == {64, 128, 256}
    assert {1, 15, 16, 17, 31, 32, 33, 47, 65, 130, 383, 384, 385, 415} <= {c.L for c in cs} and max(c.L for c in cs) <= 415
    assert all(c.B * c.H == 1 for c in cs if c.L > 130)
    assert {(1, 1), (1, 3), (3, 3), (2, 8)} <= {(c.B, c.H) for c in cs}
    assert {1, 3, 7, 8, 9, 25, 30, 1000} <= {c.period for c in cs if c.slopes == "pow2" and c.causal}
    assert {c.builder for c in cs} == set(AC.BUILDERS)
    assert any(c.slopes != "none" and not c.causal for c in cs) and any(c.slopes == "none" and not c.causal for c in cs)
    assert {c.L % 32 for c in cs if not c.causal} >= {1, 15, 16, 17, 31}
    assert all(math.isclose(c.scale, c.hd ** -0.5) for c in cs)
