"""GPU: the GEMM against the exact reference of tests/gemm_cases.py -- every element of every output equal, no tolerance.

Every (kind, case) is launched through ops.gemm into sentinel-filled buffers (NaN for fp32 outputs, a fixed value for 16-bit
ones) with guard rows, guard columns and guard planes, on tile 1, on every other tile id its form allows, on the heuristic's
tile, and with FDM_TILE_GENERAL / FDM_TILE_LOCKSTEP or-ed in (include/fdm_hip.h).  The whole buffer must equal the reference laid
into the same sentinels: the reference's values inside the window, the untouched sentinel everywhere else.  A difference names
its first element.  tests/test_gemm_exact_cpu.py shows that the inputs make equality legitimate and that the cases see the
mistakes these kernels invite.

Packed K / V contract (fdm_gemm_args; ops.kv_buffers): row m of a QKV launch is key l = m % kv_L of clip b = m / kv_L; the GEMM
writes the kv_L keys of every (clip, head) block and nothing else, so the pad keys l in [kv_L, kv_Lpad) keep the (finite) value
the buffer was filled with -- here the sentinel, where the product path zeroes them."""
import functools
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as GC  # noqa: E402
from gemm_cases import BF16, F16, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402
from fdm_amd._lib import FdmError  # noqa: E402

DEV = "cuda:0"
KIND_IDS = lambda k: GC.KIND_NAMES[k]  # noqa: E731


def _header_flag(name):
    """The value include/fdm_hip.h gives `name` (fdm_amd._lib mirrors the tile ids, not these two test flags)."""
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdm_hip.h")) as f:
        m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)\s", f.read(), re.M)
    assert m, f"include/fdm_hip.h does not define {name}"
    return int(m.group(1), 0)


TILE_GENERAL, TILE_LOCKSTEP, TILE_ID_MASK = (_header_flag(n) for n in ("FDM_TILE_GENERAL", "FDM_TILE_LOCKSTEP", "FDM_TILE_ID_MASK"))
assert TILE_GENERAL & TILE_ID_MASK == 0 and TILE_LOCKSTEP & TILE_ID_MASK == 0 and TILE_GENERAL != TILE_LOCKSTEP
LIVE = (1, 2, 3, 8, 9, 10, 11, 12)              # the tile ids that are not retired aliases


def tiles_of(case):
    """Tile 1 first, then everything else the form allows (fdm_gemm_args: ksplit and batch2 run on three tiles each; ksplit
    refuses FDM_TILE_GENERAL)."""
    if case.S > 1:
        ids = (1, 8, 9)
        return list(ids) + [0] + [t | TILE_LOCKSTEP for t in ids]
    ids = (1, 8, 2) if case.C else tuple(range(1, 13))
    live = [t for t in ids if t in LIVE]
    return list(ids) + [0] + [t | TILE_GENERAL for t in live] + [t | TILE_LOCKSTEP for t in live if t != 10]


def _opnd(kind, planes, off=0):
    """Host [planes, n] (storage type) -> what ops.gemm takes, starting `off` elements into the buffer."""
    t = planes.to(DEV)
    if kind == F16X3:
        return ops.Split(t.view(2, 1, -1), F16X3, 0, off)
    return t[0, off:]


@functools.lru_cache(maxsize=None)
def prepared(kind, case):
    """Problem, device operands, device sentinel buffers and the device copy of the expected buffers of one (kind, case):
    built once, shared among the launches, never modified."""
    p = GC.problem(kind, case)
    dt = GC.plane_dtype(kind)
    d = dict(A=_opnd(kind, p.A.to(dt)), W=_opnd(kind, p.W.to(dt)),
             bias=p.bias.to(DEV) if p.bias is not None else None, resid=p.resid.to(DEV) if p.resid is not None else None)
    blank = {n: t.to(DEV) for n, t in GC.blank(p).items()}
    want = {n: t.to(DEV) for n, t in GC.expected(kind, case).items()}
    return p, d, blank, want


def launch(kind, case, tile):
    p, d, blank, _ = prepared(kind, case)
    out = {n: t.clone() for n, t in blank.items()}
    view = lambda name, off: _view(kind, out[name], off) if name in out else None  # noqa: E731
    kw = {}
    if case.G:
        kw.update(batch=p.G, a_bs=p.a_bs, w_bs=p.w_bs, bias_bs=p.bias_bs, out_bs=p.out_bs)
    if case.C:
        kw.update(batch2=p.C, a_bs2=p.a_bs2, out_bs2=p.out_bs2)
    if case.S > 1:
        kw.update(ksplit=p.S, ksplit_stride=p.ks_stride)
    if case.kv:
        kw.update(out_kp=view("kp", 0), kp_col0=p.d, out_vp=view("vp", 0), vp_col0=2 * p.d, kv_L=p.L, kv_Lpad=p.Lpad, kv_hd=p.hd)
    if case.stat:
        kw.update(stat_out=out["stat"][0, p.stat_base:])
    ops.gemm(d["A"], d["W"], p.M, p.N, p.K, lda=p.lda, ldw=p.ldw, bias=d["bias"], act=case.act, resid=d["resid"], ldr=p.ldr,
             resid_row_mod=case.rmod, out_f32=out["f32"][0, p.base:] if "f32" in out else None, ldo_f32=p.ldo,
             out_t=view("t", p.base), ldo_t=p.ldo, tile=tile, **kw)
    torch.cuda.synchronize()
    return out


def _view(kind, buf, off):
    if kind == F16X3:
        return ops.Split(buf.view(2, 1, -1), F16X3, 0, off)
    return buf[0, off:]


def first_difference(p, name, got, want):
    """Where and what: the first element of buffer `name` that differs, in the coordinates of the kernel -- (z, m, n) of an
    output window, (clip b, head h, key l, element e) of a packed K / V block, (column group n / 64, row m, sum | sum of squares)
    of stat_out -- or its place outside them."""
    g, w = got.cpu(), want.cpu()
    diff = GC.differing(g, w)
    pl, i = (int(x) for x in diff.nonzero()[0])
    gv, wv = float(g[pl, i]), float(w[pl, i])
    where = f"flat element {i}"
    if name in ("f32", "t"):
        for s in range(p.S):
            hit = (p.off + s * p.ks_stride == i).nonzero()
            if len(hit):
                c, gr, m, n = (int(x) for x in hit[0])
                where = f"(z, m, n) = ({c * p.G + gr}, {m}, {n})" + (f" of K-slice plane {s}" if p.S > 1 else "")
                break
        else:
            where += f" = row {i // p.ldo - GC.R0}, column {i % p.ldo - p.C0} of the buffer: outside the output window"
    elif name in ("kp", "vp"):
        blk = p.Lpad * p.hd
        bh, r = divmod(i, blk)
        l_, e_ = torch.arange(p.Lpad).view(-1, 1), torch.arange(p.hd).view(1, -1)
        offs = (GC._kp_off if name == "kp" else GC._vp_off)(l_, e_, p.hd, GC.epc(p.kind))
        hit = (offs == r).nonzero()
        if bh < p.B * p.H and len(hit):
            l, e = (int(x) for x in hit[0])
            where = f"(b, h, l, e) = ({bh // p.H}, {bh % p.H}, {l}, {e})" + (" (a pad key)" if l >= p.L else "")
        else:
            where += ": behind the last (clip, head) block"
    elif name == "stat":
        r = i - p.stat_base
        if 0 <= r < (p.N // 64) * p.M * 2:
            where = f"(n / 64, m, which) = ({r // (2 * p.M)}, {r % (2 * p.M) // 2}, {'sum of squares' if r % 2 else 'sum'})"
        else:
            where += ": outside the statistics"
    return f"{name} plane {pl}, {where}: got {gv!r}, want {wv!r}, difference {gv - wv!r} ({int(diff.sum())} elements differ)"


def check(kind, case, tile, out):
    p, _, _, want = prepared(kind, case)
    for name, w in want.items():
        if not GC.identical(out[name], w):
            raise AssertionError(f"{GC.KIND_NAMES[kind]} {case.id} tile {tile:#x}: {first_difference(p, name, out[name], w)}")


@pytest.mark.parametrize("case", GC.CASES, ids=lambda c: c.id)
@pytest.mark.parametrize("kind", GC.KINDS, ids=KIND_IDS)
def test_gemm_is_bit_exact_on_every_tile(kind, case):
    """Tile 1 equals the exact reference and leaves every sentinel; so does every other tile the form allows, the heuristic's
    choice, the general (edge-handling) kernel and the lockstep k loop."""
    for tile in tiles_of(case):
        check(kind, case, tile, launch(kind, case, tile))


@pytest.mark.parametrize("kind", GC.KINDS, ids=KIND_IDS)
def test_gemm_refuses_what_the_header_forbids(kind):
    """Beside test_gemm_split_k_argument_checks (tests/test_ops_gpu.py): batch2 on a tile that is not one of its three, and K
    that is not a multiple of the kind's k-tile."""
    ku, e, dt = GC.k_unit(kind), GC.epc(kind), GC.plane_dtype(kind)
    K = 2 * ku
    A, W = _opnd(kind, torch.zeros(GC.planes_of(kind), 64 * K, dtype=dt)), _opnd(kind, torch.zeros(GC.planes_of(kind), 64 * K, dtype=dt))
    out = torch.zeros(64, 64, device=DEV)
    b2 = dict(out_f32=out, batch=2, a_bs=32 * K, batch2=2, a_bs2=16 * K, out_bs2=16 * 64)
    for tile in (0, 1, 8, 2):                                                       # (the form itself is accepted on its three tiles)
        ops.gemm(A, W, 16, 64, K, tile=tile, **b2)
    for tile in (3, 9, 10, 11, 12):
        with pytest.raises(FdmError, match="batch2 runs on the 64-column tiles"):
            ops.gemm(A, W, 16, 64, K, tile=tile, **b2)
    for good in (ku, 2 * ku):                                                       # (the same launch with whole k-tiles is accepted)
        ops.gemm(A, W, 16, 64, good, lda=K, ldw=K, out_f32=out)
    for bad in (ku - e, ku + e, ku // 2):
        with pytest.raises(FdmError, match=f"K={bad} not a multiple of {ku}"):
            ops.gemm(A, W, 16, 64, bad, lda=K, ldw=K, out_f32=out)
    torch.cuda.synchronize()
