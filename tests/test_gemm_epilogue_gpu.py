"""GPU: the GEMM's inexact epilogue forms (Mish, GELU(erf), GELU(tanh)) and act_apply's other callers (ops.bias_act,
ops.small_linear), through fdm_amd.ops, on a pre-activation value known bit for bit (tests/epilogue_cases.py): every element of
every output finite and within its counted bound of the fp64 activation, NaN-filled outputs between sentinel guards, on the
heuristic's tile and tile 1, with FDM_TILE_GENERAL, and bit for bit the same on every other tile.  One EPI_RATIO line per
(form, kind class) carries the worst error-to-bound ratio measured."""
import functools
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

import epilogue_cases as EC  # noqa: E402
import gemm_cases as GC  # noqa: E402
import norm_cases as NC  # noqa: E402
from epilogue_cases import ACT_LEAKY02, ACT_RELU, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402

DEV = "cuda:0"
GUARD, SENT, NAN = 64, -7.0, float("nan")
TILE_GENERAL, TILE_LOCKSTEP = 0x100, 0x200
KIND_IDS = lambda k: EC.KIND_NAMES[k]  # noqa: E731
ACT_IDS = lambda a: EC.ACT_NAMES[a]  # noqa: E731
LIVE = (1, 2, 3, 8, 9, 10, 11, 12)
OTHER_TILES = [t for t in range(2, 13)] + [t | TILE_GENERAL for t in LIVE] + [t | TILE_LOCKSTEP for t in LIVE if t != 10]
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """One EPI_RATIO line per (form, kind class), after the module's last test."""
    yield
    for key in sorted(WORST, key=str):
        print(f"EPI_RATIO {' '.join(key)}: worst error / bound {WORST[key]:.4f}")


def test_tile_flags_are_the_headers():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fdm_hip.h")) as f:
        text = f.read()
    for name, val in (("FDM_TILE_GENERAL", TILE_GENERAL), ("FDM_TILE_LOCKSTEP", TILE_LOCKSTEP)):
        m = re.search(rf"^#define\s+{name}\s+(0x[0-9a-fA-F]+|\d+)\s", text, re.M)
        assert m and int(m.group(1), 0) == val, name
    # LIVE / OTHER_TILES name every tile id: a new id in the header has to be added here (and to tests/test_gemm_exact_gpu.py)
    ids = {n: int(v) for n, v in re.findall(r"^#define\s+FDM_TILE_(\w+)\s+(\d+)\s", text, re.M)}
    assert ids["MAX"] == 12 and max(v for n, v in ids.items() if n != "MAX") == 12
    assert {ids[n] for n in ("64x64", "128x64", "128x128", "64x64_S2", "32x64_S3", "256x128_PP", "80x128", "64x128")} == set(LIVE)


class Out:
    """A [rows, cols] output of `kind` (F32 for out_f32) filled with NaN, sentinel elements (whole sentinel rows for a plane pair) on
    each side of it -- of each plane (the buffers of tests/test_norm_edges_gpu.py)."""

    def __init__(self, kind, rows, cols):
        self.kind, self.rows, self.cols = kind, rows, cols
        dt = ops.tdtype(kind)
        if kind == F16X3:
            self.gr = gr = (GUARD + cols - 1) // cols
            self.buf = torch.full((2, rows + 2 * gr, cols), SENT, device=DEV, dtype=dt)
            self.buf[:, gr:gr + rows] = NAN
            self.arg = ops.Split(self.buf, F16X3, row0=gr)
        else:
            self.buf = torch.full((GUARD + rows * cols + GUARD,), SENT, device=DEV, dtype=dt)
            self.buf[GUARD:GUARD + rows * cols] = NAN
            self.arg = self.buf[GUARD:GUARD + rows * cols].view(rows, cols)

    def bits(self):
        b = self.buf[:, self.gr:self.gr + self.rows] if self.kind == F16X3 else self.arg
        return b.view(torch.int16 if b.element_size() == 2 else torch.int32)

    def guards_intact(self):
        if self.kind == F16X3:
            g = torch.cat([self.buf[:, :self.gr].reshape(-1), self.buf[:, self.gr + self.rows:].reshape(-1)])
        else:
            g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.rows * self.cols:]])
        return bool((g == SENT).all())

    def values(self):
        b = (self.buf[:, self.gr:self.gr + self.rows] if self.kind == F16X3 else self.arg).cpu()
        return (b[0].float() + b[1].float() / GC.SPLIT_SCALE) if self.kind == F16X3 else b.float()


def _opnd(kind, planes):
    t = planes.to(DEV)
    return ops.Split(t.view(2, 1, -1), F16X3, 0, 0) if kind == F16X3 else t[0]


@functools.lru_cache(maxsize=None)
def prepared(kind, shape, launch):
    p, bias, v, resid = EC.act_problem(kind, shape, launch)
    dt = GC.plane_dtype(kind)
    return p, _opnd(kind, p.A.to(dt)), _opnd(kind, p.W.to(dt)), bias.to(DEV), resid.to(DEV).contiguous()


def launch(kind, act, shape, name, outs, resid, tile):
    p, A, W, bias, r = prepared(kind, shape, name)
    o = {}
    if outs in ("f32", "both"):
        o["f32"] = Out(F32, p.M, p.N)
    if outs in ("t", "both"):
        o["t"] = Out(kind, p.M, p.N)
    ops.gemm(A, W, p.M, p.N, p.K, lda=p.lda, ldw=p.ldw, bias=bias, act=act, resid=r if resid else None, ldr=p.N,
             out_f32=o["f32"].arg if "f32" in o else None, ldo_f32=p.N, out_t=o["t"].arg if "t" in o else None, ldo_t=p.N, tile=tile)
    torch.cuda.synchronize()
    return o


def check(tag, kind, o, reference, key, pure=False):
    top = 0.0
    for name, out in o.items():
        assert out.guards_intact(), f"{tag} out_{name}: a guard element was written"
        got = out.values()
        assert bool(torch.isfinite(got).all()), f"{tag} out_{name}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
        ref, bnd = reference(name)
        r, idx, err, b = EC.worst(got.reshape(ref.shape), ref, bnd)
        assert r <= 1.0, f"{tag} out_{name}: error / bound = {r:.4g} at {idx}: |gpu - ref| = {err:.4g}, bound = {b:.4g}, ref = {float(ref[idx]):.6g}"
        top = max(top, r)
        if name == "f32" and pure:                                  # the activation alone: no residual add, no output rounding
            WORST[key + ("activation alone",)] = max(WORST.get(key + ("activation alone",), 0.0), r)
    WORST[key] = max(WORST.get(key, 0.0), top)
    return top


@pytest.mark.parametrize("act", EC.HEAVY, ids=ACT_IDS)
@pytest.mark.parametrize("kind", EC.KINDS, ids=KIND_IDS)
def test_gemm_activation_is_inside_its_bound_on_every_element(kind, act):
    """Mish / GELU(erf) / GELU(tanh) x out_f32 | out_t | both x residual or none x interior, interior + FDM_TILE_GENERAL, ragged x
    the grid launch and the special-value launch: per-element check on tile 0 and tile 1; every other tile gives tile 1's bits."""
    key = ("gemm " + EC.ACT_NAMES[act], EC.kind_class(kind))
    for shape, name, outs, resid in itertools.product(EC.SHAPES, ("grid", "special"), ("f32", "t", "both"), (False, True)):
        ref = lambda out: EC.gemm_reference(kind, act, shape, name, resid, out)  # noqa: E731
        tiles = (0, 1) + ((TILE_GENERAL, 1 | TILE_GENERAL) if shape == "interior" else ())
        base = None
        for tile in tiles:
            o = launch(kind, act, shape, name, outs, resid, tile)
            check(f"{EC.KIND_NAMES[kind]} {EC.ACT_NAMES[act]} {shape} {name} {outs} resid={resid} tile {tile:#x}", kind, o, ref, key, pure=not resid)
            if tile == 1:
                base = o
        if outs == "both":                                         # (the other tile ids once per (shape, launch, residual))
            for tile in OTHER_TILES:
                o = launch(kind, act, shape, name, outs, resid, tile)
                for n_, out in o.items():
                    assert out.guards_intact() and torch.equal(out.bits(), base[n_].bits()), \
                        f"{EC.KIND_NAMES[kind]} {EC.ACT_NAMES[act]} {shape} {name} resid={resid}: tile {tile:#x} differs from tile 1 in out_{n_}"


@pytest.mark.parametrize("act", (ACT_RELU, ACT_LEAKY02), ids=ACT_IDS)
def test_gemm_exact_controls(act):
    """ReLU and LeakyReLU(0.2) over the same launches: bit for bit the one-rounding reference (no residual: gemm_cases' rule for leaky)."""
    for kind, shape, name in itertools.product(EC.KINDS, EC.SHAPES, ("grid", "special")):
        _, _, v, _ = EC.act_problem(kind, shape, name)
        want = EC.act_twin(kind, act, v)
        assert torch.equal(want.double(), EC.act64(v, act).float().double())
        for tile in (0, 1, 1 | TILE_GENERAL):
            o = launch(kind, act, shape, name, "both", False, tile)
            assert o["f32"].guards_intact() and o["t"].guards_intact()
            got = o["f32"].values()
            assert not bool(GC.differing(got, want).any()), (EC.KIND_NAMES[kind], shape, name, tile)
            key = ("gemm " + EC.ACT_NAMES[act], EC.kind_class(kind))
            check(f"{EC.KIND_NAMES[kind]} {EC.ACT_NAMES[act]} {shape} {name} tile {tile:#x}", kind, {"t": o["t"]},
                  lambda out: EC.finish(kind, "t", torch.full(v.shape, 1e-30, dtype=torch.float64), want.double()), key)


@pytest.mark.parametrize("act", EC.ALL_ACTS, ids=ACT_IDS)
def test_bias_act_and_small_linear_are_inside_their_bounds(act):
    """act_apply's other callers over the whole value list, d = 67, below and above one block; small_linear with K = 1 and K = 8."""
    key = ("flat " + EC.ACT_NAMES[act], "f32-class")
    for size, vec in itertools.product(("small", "large"), (False, True)):
        x, w, v = EC.bias_act_problem(size, vec)
        o = Out(F32, *x.shape)
        ops.bias_act(x.to(DEV), w.to(DEV) if vec else None, o.arg, x.shape[0], x.shape[1], act)
        torch.cuda.synchronize()
        check(f"bias_act {EC.ACT_NAMES[act]} {size} vec={vec}", F32, {"f32": o}, lambda out: EC.flat_reference(act, v), key)
    for size, K in itertools.product(("small", "large"), (1, 8)):
        x, W, bias, v = EC.small_linear_problem(size, K)
        o = Out(F32, *v.shape)
        ops.small_linear(x.to(DEV), W.to(DEV), bias.to(DEV), o.arg, v.shape[0], K, v.shape[1], act)
        torch.cuda.synchronize()
        check(f"small_linear {EC.ACT_NAMES[act]} {size} K={K}", F32, {"f32": o}, lambda out: EC.flat_reference(act, v), key)


# ---------------------------------------------------------------------------------------------------------------------
# the LayerNorm fold
# ---------------------------------------------------------------------------------------------------------------------
CHECKED_TILES = (0, 1, 1 | TILE_GENERAL)


def opnd(kind, mat32):
    """Host fp32 [rows, cols] of values -> the GEMM operand of `kind` on the device."""
    t = GC.to_kind(kind, mat32).to(DEV).contiguous()
    return ops.Split(t, F16X3) if kind == F16X3 else t[0]


def same_bits(a, b):
    return all(torch.equal(a[n].bits(), b[n].bits()) and a[n].guards_intact() for n in a)


def run_producer(kind, p, tile):
    o = {"f32": Out(F32, p.M, p.D), "t": Out(kind, p.M, p.D), "stat": Out(F32, p.nparts * p.M, 2)}
    ops.gemm(opnd(kind, p.A0), opnd(kind, p.W0), p.M, p.D, p.K0, resid=p.R0.to(DEV), ldr=p.D, out_f32=o["f32"].arg, out_t=o["t"].arg,
             stat_out=o["stat"].arg, tile=tile)
    torch.cuda.synchronize()
    return o


def check_producer(tag, kind, p, o):
    for n, out in o.items():
        assert out.guards_intact(), f"{tag} {n}: a guard element was written"
    x = o["f32"].values()
    assert not bool(GC.differing(x, p.x).any()), f"{tag}: out_f32 is not fl32(acc + resid)"
    assert not bool(GC.differing(o["t"].values(), NC.round_kind(kind, p.x)).any()), f"{tag}: out_t is not the kind's rounding of out_f32"
    st = o["stat"].values().view(p.nparts, p.M, 2)
    assert bool(torch.isfinite(st).all()), f"{tag}: {int((~torch.isfinite(st)).sum())} statistics not written"
    ref, bnd = EC.producer_reference(x)
    r, idx, err, b = EC.worst(st, ref, bnd)
    assert r <= 1.0, f"{tag}: partial (part, row, which) = {idx}: error / bound = {r:.4g}, |gpu - ref| = {err:.4g}, bound = {b:.4g}"
    if not p.real:
        assert torch.equal(st.double(), ref), f"{tag}: integer sums below 2^24 are exact"
    key = ("fold producer", EC.kind_class(kind))
    WORST[key] = max(WORST.get(key, 0.0), r)
    return x, st


def run_consumer(kind, p, prod, N, tile, form):
    """form 'colsum': LN(x) W'^T + b from the raw rows; 'rln': A2 W2^T + b2 + LN(x) on the residual."""
    nn = N if form == "colsum" else p.D
    o = {"f32": Out(F32, p.M, nn), "t": Out(kind, p.M, nn)}
    kw = dict(out_f32=o["f32"].arg, out_t=o["t"].arg, ln_stat_in=prod["stat"].arg, ln_nparts=p.nparts, ln_dim=p.D, tile=tile)
    if form == "colsum":
        ops.gemm(prod["t"].arg, opnd(kind, p.W1[:N]), p.M, N, p.D, bias=p.b1[:N].to(DEV), ln_colsum=p.cs[:N].to(DEV), **kw)
    else:
        ops.gemm(opnd(kind, p.A2), opnd(kind, p.W2), p.M, p.D, p.K0, bias=p.b2.to(DEV), resid=prod["f32"].arg, ldr=p.D,
                 rln_gamma=p.gamma.to(DEV), rln_beta=p.beta.to(DEV), **kw)
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("nparts", EC.NPARTS)
@pytest.mark.parametrize("kind", EC.KINDS, ids=KIND_IDS)
def test_layernorm_fold_is_inside_its_bounds_on_every_element(kind, nparts):
    """Producer partials against the fp64 sums of the out_f32 the launch wrote; the ln_colsum consumer (N = 64, 68) and the rln
    residual against fp64 of the partials and rows they read; M = 1, 63, 65; tile 0, tile 1 and FDM_TILE_GENERAL per element, every
    other tile id (M = 65) bit for bit tile 1; a producer with real-valued rows for the partials' bound."""
    kn = EC.KIND_NAMES[kind]
    for M in EC.FOLD_M:
        p = EC.fold_problem(kind, nparts, M)
        prods = {}
        for tile in CHECKED_TILES:
            prods[tile] = run_producer(kind, p, tile)
            check_producer(f"{kn} producer nparts={nparts} M={M} tile {tile:#x}", kind, p, prods[tile])
        pr = EC.fold_problem(kind, nparts, M, real=True)
        check_producer(f"{kn} real producer nparts={nparts} M={M}", kind, pr, run_producer(kind, pr, 1))
        prod = prods[1]
        st = prod["stat"].values().view(nparts, M, 2)
        forms = [("colsum", N) for N in EC.FOLD_N] + [("rln", 0)]
        for form, N in forms:
            ref = (lambda out: EC.colsum_reference(kind, out, p, N, st)) if form == "colsum" else (lambda out: EC.rln_reference(kind, out, p, st))  # noqa: E731
            base = None
            for tile in CHECKED_TILES:
                o = run_consumer(kind, p, prod, N, tile, form)
                check(f"{kn} {form} nparts={nparts} M={M} N={N} tile {tile:#x}", kind, o, ref, ("fold " + form, EC.kind_class(kind)))
                base = o if tile == 1 else base
            if M == 65:
                for tile in OTHER_TILES:
                    assert same_bits(run_consumer(kind, p, prod, N, tile, form), base), f"{kn} {form} nparts={nparts} N={N}: tile {tile:#x} differs from tile 1"
        if M == 65:
            for tile in OTHER_TILES:
                assert same_bits(run_producer(kind, p, tile), prod), f"{kn} producer nparts={nparts}: tile {tile:#x} differs from tile 1"


@pytest.mark.parametrize("nparts", EC.NPARTS)
@pytest.mark.parametrize("kind", (F32, F16X3), ids=KIND_IDS)
def test_layernorm_fold_chain_against_fp64_layernorm(kind, nparts):
    """Producer (real-valued rows) then the ln_colsum consumer against fp64 LN(x) W^T + b of the fp32 x the producer wrote."""
    for M in EC.FOLD_M:
        p = EC.fold_problem(kind, nparts, M, real=True)
        prod = run_producer(kind, p, 0)
        x, st = check_producer(f"{EC.KIND_NAMES[kind]} chain producer nparts={nparts} M={M}", kind, p, prod)
        for N, tile in itertools.product(EC.FOLD_N, (0, 1)):
            o = run_consumer(kind, p, prod, N, tile, "colsum")
            check(f"{EC.KIND_NAMES[kind]} chain nparts={nparts} M={M} N={N} tile {tile:#x}", kind, o,
                  lambda out: EC.colsum_reference(kind, out, p, N, st, x=x, chain=True), ("fold chain", EC.kind_class(kind)))
