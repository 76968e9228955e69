"""GPU: every kernel that computes a mean and a variance (csrc/elementwise.hpp), called through fdm_amd.ops, against the fp64
reference of what it reads, element by element inside the bound derived in tests/norm_cases.py -- at offset, size and length edges,
in every operand kind, for y_f32 alone, y_t alone and both.  Every output buffer is pre-filled with NaN between two 64-element
sentinel guards: all of it must be finite afterwards and no guard may change.  tests/test_norm_edges_cpu.py shows that the cases
see the mistakes these kernels invite."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_cases as NC  # noqa: E402
from norm_cases import ACT_GELU_ERF, ACT_NONE, BF16, F16, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402
from fdm_amd._lib import FdmError  # noqa: E402

DEV = "cuda:0"
GUARD, SENT = 64, -7.0
KIND_IDS = lambda k: NC.KIND_NAMES[k]  # noqa: E731
CASE_IDS = lambda c: c.id  # noqa: E731
NAN = float("nan")


class Out:
    """A [rows, cols] output of `kind` (F32 for y_f32) filled with NaN, 64 sentinel elements (whole sentinel rows for a plane pair)
    on each side of it -- of each plane."""

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
        """The written region as stored (planes for the split kind)."""
        return self.buf[:, self.gr:self.gr + self.rows] if self.kind == F16X3 else self.arg

    def guards_intact(self):
        if self.kind == F16X3:
            g = torch.cat([self.buf[:, :self.gr].reshape(-1), self.buf[:, self.gr + self.rows:].reshape(-1)])
        else:
            g = torch.cat([self.buf[:GUARD], self.buf[GUARD + self.rows * self.cols:]])
        return bool((g == SENT).all())

    def values(self):
        """fp32 CPU [rows, cols] of what the buffer holds."""
        b = self.bits().cpu()
        return (b[0].float() + b[1].float() / NC.SPLIT_SCALE) if self.kind == F16X3 else b.float()


def outputs(kind, mode, rows, cols):
    """mode 'f32' | 't' | 'both' -> {'f32': Out, 't': Out} (the ones asked for)."""
    o = {}
    if mode in ("f32", "both"):
        o["f32"] = Out(F32, rows, cols)
    if mode in ("t", "both"):
        o["t"] = Out(kind, rows, cols)
    return o


def arg(o, name):
    return o[name].arg if name in o else None


@functools.lru_cache(maxsize=None)
def dev(op, case):
    """The case's inputs on the device (shared, never modified)."""
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in host(op, case).items()}


@functools.lru_cache(maxsize=None)
def host(op, case):
    return case.inputs()


@functools.lru_cache(maxsize=None)
def reference(op, kind, out, case):
    """(y_ref, bound) of one (kind, output, case): computed once, shared among the tests, never modified."""
    inp = host(op, case)
    if op == "ln":
        return NC.ln_reference(kind, out, case, inp)
    if op == "conv0":
        return NC.conv0_reference(case, inp)
    if op == "conv_ln":
        return NC.conv_ln_reference(kind, case, inp)
    if op == "instnorm":
        return NC.instnorm_reference(kind, out, case, inp)
    if op == "groupnorm":
        return NC.groupnorm_reference(kind, out, case, inp)
    return NC.adain_reference(case, inp)


WORST = {}


def check(op, kind, case, o, what=""):
    """Guards, finiteness and the per-element bound of every output in o."""
    top = 0.0
    for name, out in o.items():
        tag = f"{op} {NC.KIND_NAMES[kind]} {what}{case.id} {'y_' + name}"
        assert out.guards_intact(), f"{tag}: a guard element was written"
        got = out.values()
        assert bool(torch.isfinite(got).all()), f"{tag}: {int((~torch.isfinite(got)).sum())} elements not written (or not finite)"
        ref, bnd = reference(op, kind, "t" if (name == "t" or (op == "conv_ln" and kind != F32)) else "f32", case)
        r, idx, err, b = NC.worst(got.reshape(ref.shape), ref, bnd)
        top = max(top, r)
        assert r <= 1.0, (f"{tag}: error / bound = {r:.4g} at {idx}: |gpu - ref| = {err:.4g}, bound = {b:.4g}, ref = {float(ref[idx]):.6g}")
    key = (op, "f32-class" if kind in (F32, F16X3) else "16-bit")
    WORST[key] = max(WORST.get(key, 0.0), top)
    print(f"NORM_RATIO {op} {NC.KIND_NAMES[kind]} {what}{case.id} {top:.4f} (worst so far {key[1]}: {WORST[key]:.4f})")


def same_bits(a, b):
    return torch.equal(a.bits().view(torch.int16 if a.bits().element_size() == 2 else torch.int32),
                       b.bits().view(torch.int16 if b.bits().element_size() == 2 else torch.int32))


def check_t_is_rounding_of_f32(kind, o, tag):
    """y_t is the kind's rounding of y_f32 (store_opnd* / from_f32: round to nearest even, fp16 clamped at 65504), bit for bit;
    the split pair: hi plane bit for bit, the pair reproduces y_f32 to 2^-21 relative."""
    y = o["f32"].bits()
    t = o["t"].bits()
    if kind == F32:
        assert torch.equal(t.view(torch.int32), y.view(torch.int32)), tag
    elif kind == BF16:
        assert torch.equal(t.view(torch.int16), y.bfloat16().view(torch.int16)), tag
    elif kind == F16:
        assert torch.equal(t.view(torch.int16), y.clamp(-65504.0, 65504.0).half().view(torch.int16)), tag
    else:
        assert torch.equal(t[0].view(torch.int16), y.clamp(-65504.0, 65504.0).half().view(torch.int16)), tag
        pair = t[0].float() + t[1].float() / NC.SPLIT_SCALE
        assert bool(((pair - y).abs() <= 2.0 ** -21 * y.abs() + 2.0 ** -36).all()), tag


def all_modes(op, kind, case, launch, rows, cols):
    """y_f32 alone, y_t alone, both (twice): each inside the bound; the same bits whichever outputs are asked for and on a second
    launch; y_t the rounding of y_f32."""
    runs = {}
    for mode in ("f32", "t", "both", "again"):
        o = outputs(kind, "both" if mode == "again" else mode, rows, cols)
        launch(o)
        torch.cuda.synchronize()
        runs[mode] = o
        if mode != "again":
            check(op, kind, case, o, mode + " ")
    tag = f"{op} {NC.KIND_NAMES[kind]} {case.id}"
    assert same_bits(runs["f32"]["f32"], runs["both"]["f32"]) and same_bits(runs["t"]["t"], runs["both"]["t"]), tag + ": outputs depend on which are asked for"
    assert same_bits(runs["again"]["f32"], runs["both"]["f32"]) and same_bits(runs["again"]["t"], runs["both"]["t"]), tag + ": not repeatable"
    check_t_is_rounding_of_f32(kind, runs["both"], tag)
    return runs["both"]


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def ln_x(case):
    """x with its planes plane_stride apart (one flat buffer)."""
    inp = dev("ln", case)
    npl = inp["x"].shape[0]
    if npl == 1:
        return inp["x"][0].contiguous()
    buf = torch.full((npl * case.plane_stride,), 1e4, device=DEV)
    for p in range(npl):
        buf[p * case.plane_stride:p * case.plane_stride + case.M * case.d] = inp["x"][p].reshape(-1)
    return buf


def ln_launch(kind, case, o, rows=None):
    """rows: launch only that row range (plain cases: batch independence)."""
    inp = dev("ln", case)
    x = ln_x(case)
    M = case.M
    if rows is not None:
        x, M = x[rows[0]:rows[1]].contiguous(), rows[1] - rows[0]
    kw = {k: inp[k] for k in ("add_mat", "add_tab", "tab_index", "tab_step", "gamma2", "beta2", "clip_step", "clip_step_stride", "clip_rows",
                              "clip_wrap", "add_mat_group", "add_mat_wrap", "add_mat_L") if k in inp}
    if case.planes:
        kw.update(x_planes=case.planes, x_plane_stride=case.plane_stride)
    ops.layernorm(x, inp["gamma"], inp["beta"], M, case.d, eps=inp["eps"], act=case.act, y_f32=arg(o, "f32"), y_t=arg(o, "t"), dtype=kind, **kw)


@pytest.mark.parametrize("case", NC.LN_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", NC.KINDS, ids=KIND_IDS)
def test_layernorm_within_per_element_bound(kind, case):
    all_modes("ln", kind, case, lambda o: ln_launch(kind, case, o), case.M, case.d)


@pytest.mark.parametrize("d", [256, 512, 768, 1024])
@pytest.mark.parametrize("kind", NC.KINDS, ids=KIND_IDS)
def test_layernorm_row_does_not_depend_on_its_batch(kind, d):
    """'A clip's result never depends on the batch it is computed in' (csrc/elementwise.hpp): row r of the M = 5 launch has the
    bits of the M = 1 launch of that row."""
    for builder in ("row_scales", "wave_skew", "offset100"):
        case = NC.LnCase(builder, 5, d, "plain", ACT_NONE)
        full = outputs(kind, "both", 5, d)
        ln_launch(kind, case, full)
        for r in range(5):
            one = outputs(kind, "both", 1, d)
            ln_launch(kind, case, one, rows=(r, r + 1))
            torch.cuda.synchronize()
            for name in ("f32", "t"):
                a, b = full[name].bits(), one[name].bits()
                a = a[:, r:r + 1] if kind == F16X3 and name == "t" else a[r:r + 1]
                assert torch.equal(a.float(), b.float()) and one[name].guards_intact(), f"{case.id} row {r} y_{name}"


def test_layernorm_constant_rows_give_beta():
    """Variance exactly 0: y = beta within the bound's first term, 2 |g| r (s + 1) u a1 (the mean's rounding alone)."""
    for d in (256, 768):
        case = NC.LnCase("constant", 5, d, "plain", ACT_NONE)
        o = outputs(F32, "f32", 5, d)
        ln_launch(F32, case, o)
        torch.cuda.synchronize()
        inp = host("ln", case)
        a1 = inp["x"][0].double().abs().mean(1, keepdim=True)
        first = 2.0 * inp["gamma"].double().abs() * (1.0 / NC.EPS ** 0.5) * (9 + d // 256 + 1) * NC.U * a1 + 4.0 * NC.U * inp["beta"].double().abs() + 1e-30
        assert bool(((o["f32"].values().double() - inp["beta"].double()).abs() <= first).all())


# ---------------------------------------------------------------------------------------------------------------------
# conv0, conv0 + LayerNorm(512) + GELU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.CONV_CASES, ids=CASE_IDS)
def test_conv0_within_per_element_bound(case):
    inp = dev("conv0", case)
    runs = []
    for _ in range(2):
        o = {"f32": Out(F32, case.B * case.T0, 512)}
        ops.conv0(inp["wav"], inp["w"], inp["bias"], o["f32"].arg, case.B, case.n, case.T0)
        torch.cuda.synchronize()
        check("conv0", F32, case, o)
        runs.append(o["f32"])
    assert same_bits(*runs)


@pytest.mark.parametrize("case", NC.CONV_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", NC.KINDS, ids=KIND_IDS)
def test_conv0_ln_gelu_within_per_element_bound(kind, case):
    inp = dev("conv_ln", case)
    if kind == F16:       # refused, not skipped
        with pytest.raises(FdmError):
            ops.conv0_ln_gelu(inp["wav"], inp["w"], inp["bias"], inp["gamma"], inp["beta"], Out(F16, case.B * case.T0, 512).arg, case.B, case.n, case.T0)
        return
    runs = []
    for _ in range(2):
        out = Out(kind, case.B * case.T0, 512)
        ops.conv0_ln_gelu(inp["wav"], inp["w"], inp["bias"], inp["gamma"], inp["beta"], out.arg, case.B, case.n, case.T0, eps=inp["eps"])
        torch.cuda.synchronize()
        check("conv_ln", kind, case, {"f32" if kind == F32 else "t": out})
        runs.append(out)
    assert same_bits(*runs)


# ---------------------------------------------------------------------------------------------------------------------
# LeakyReLU + instance norm
# ---------------------------------------------------------------------------------------------------------------------
def in_launch(kind, case, o, x=None, L=None, lens=None):
    x = dev("instnorm", case)["x"] if x is None else x
    B, L = x.shape[0], (case.L if L is None else L)
    if lens is not None:
        ops.leaky_instnorm_lens(x, B, L, case.d, lens, y_f32=arg(o, "f32"), y_t=arg(o, "t"), eps=NC.EPS, dtype=kind)
    else:
        ops.leaky_instnorm(x, B, L, case.d, y_f32=arg(o, "f32"), y_t=arg(o, "t"), eps=NC.EPS, dtype=kind)


def dev_lens(case):
    return torch.tensor(case.lens, dtype=torch.int32, device=DEV) if case.lens else None


def check_pad_frames_are_plus_zero(o, case, L, cols):
    for name, out in o.items():
        b = out.bits()
        b = b.reshape((2, len(case.lens), L, cols) if out.kind == F16X3 else (len(case.lens), L, cols))
        for i, Lb in enumerate(case.lens):
            pad = b[..., i, Lb:, :]
            assert int(pad.view(torch.int16 if pad.element_size() == 2 else torch.int32).count_nonzero()) == 0, f"{case.id} clip {i} y_{name}: pad frames are not +0.0"


@pytest.mark.parametrize("case", NC.IN_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", NC.KINDS, ids=KIND_IDS)
def test_leaky_instnorm_within_per_element_bound(kind, case):
    lens = dev_lens(case)
    if kind in (F16, F16X3):       # refused, not skipped
        with pytest.raises(FdmError):
            in_launch(kind, case, {"t": Out(F16, case.nb * case.L, case.d)}, lens=lens)
        return
    both = all_modes("instnorm", kind, case, lambda o: in_launch(kind, case, o, lens=lens), case.nb * case.L, case.d)
    if case.L == 1:
        assert float(both["f32"].values().abs().max()) == 0.0 and float(both["t"].values().abs().max()) == 0.0      # one frame: exactly 0
    if case.builder == "constant":       # variance 0: 0 within the bound's first term (the mean's rounding alone)
        x = host("instnorm", case)["x"].double()
        first = 2.0 * (1.0 / NC.EPS ** 0.5) * (NC.s_time(case.L) + 1 + 1.25) * NC.U * NC.leaky64(x).abs().mean(1, keepdim=True) + 1e-30
        assert bool((both["f32"].values().double().reshape(x.shape).abs() <= first).all())
    if case.lens:
        check_pad_frames_are_plus_zero(both, case, case.L, case.d)
        x = dev("instnorm", case)["x"]
        for i, Lb in enumerate(case.lens):       # each clip of the ragged batch has the bits of its own launch
            solo = outputs(kind, "both", Lb, case.d)
            in_launch(kind, case, solo, x=x[i:i + 1, :Lb].contiguous(), L=Lb)
            torch.cuda.synchronize()
            for name in ("f32", "t"):
                rag = both[name].bits().reshape(len(case.lens), case.L, case.d)[i, :Lb]
                assert torch.equal(rag.float(), solo[name].bits().float()) and solo[name].guards_intact(), f"{case.id} clip {i} y_{name}"


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm(groups = C) over time
# ---------------------------------------------------------------------------------------------------------------------
def gn_scratch(case, B, T):
    need = NC.scratch_bytes(B, T, case.C)
    if need == 0 or case.scratch == "none":
        return None
    return torch.empty((need - (16 if case.scratch == "small" else 0)) // 8, dtype=torch.float64, device=DEV)


def gn_launch(kind, case, o, x=None, lens=None):
    inp = dev("groupnorm", case)
    x = inp["x"] if x is None else x
    B, T = x.shape[:2]
    scratch = gn_scratch(case, B, T)
    yt = arg(o, "t")
    if lens is not None:
        ops.time_groupnorm_lens(x, inp["gamma"], inp["beta"], B, T, case.C, lens, y_f32=arg(o, "f32"), y_t=yt, eps=inp["eps"], act=case.act, dtype=kind, scratch=scratch)
    else:
        ops.time_groupnorm(x, inp["gamma"], inp["beta"], B, T, case.C, y_f32=arg(o, "f32"), y_t=yt, eps=inp["eps"], act=case.act, dtype=kind, scratch=scratch)
    return scratch      # (kept alive by the caller until the synchronize)


@pytest.mark.parametrize("case", NC.GN_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", NC.KINDS, ids=KIND_IDS)
def test_time_groupnorm_within_per_element_bound(kind, case):
    lens = dev_lens(case)
    if kind == F16:       # refused, not skipped
        with pytest.raises(FdmError):
            gn_launch(kind, case, {"t": Out(F16, case.B * case.T, case.C)}, lens=lens)
        return
    keep = []
    both = all_modes("groupnorm", kind, case, lambda o: keep.append(gn_launch(kind, case, o, lens=lens)), case.B * case.T, case.C)
    if case.lens:
        check_pad_frames_are_plus_zero(both, case, case.T, case.C)
        x = dev("groupnorm", case)["x"]
        for i, Tb in enumerate(case.lens):       # each clip has the bits of its own launch with the same scratch choice
            solo = outputs(kind, "both", Tb, case.C)
            keep.append(gn_launch(kind, case, solo, x=x[i:i + 1, :Tb].contiguous()))
            torch.cuda.synchronize()
            for name in ("f32", "t"):
                rag, sb = both[name].bits(), solo[name].bits()
                rag = rag.reshape((2, len(case.lens), case.T, case.C) if rag.dim() == 3 else (len(case.lens), case.T, case.C))[..., i, :Tb, :]
                assert torch.equal(rag.float().reshape(-1), sb.float().reshape(-1)) and solo[name].guards_intact(), f"{case.id} clip {i} y_{name}"


@pytest.mark.parametrize("T", [4096, 4097])
def test_chunked_and_three_pass_groupnorm_share_one_reference(T):
    """With and without scratch at the switch: two kernels families, each inside its own bound of the same fp64 reference -- and they
    are two forms (the statistics differ in the last bits somewhere), so the scratch really selects the chunk pair."""
    got = {}
    for scratch in ("full", "none"):
        case = NC.GnCase("offset100", T, 8, scratch, True, ACT_NONE, None)
        o = outputs(F32, "f32", case.B * T, 8)
        keep = gn_launch(F32, case, o)
        torch.cuda.synchronize()
        check("groupnorm", F32, case, o, "forms ")
        got[scratch] = o["f32"].values()
        del keep
    ref_a = reference("groupnorm", F32, "f32", NC.GnCase("offset100", T, 8, "full", True, ACT_NONE, None))[0]
    ref_b = reference("groupnorm", F32, "f32", NC.GnCase("offset100", T, 8, "none", True, ACT_NONE, None))[0]
    assert torch.equal(ref_a, ref_b) and not torch.equal(got["full"], got["none"])


# ---------------------------------------------------------------------------------------------------------------------
# AdaIN
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", NC.ADA_CASES, ids=CASE_IDS)
def test_adain_within_per_element_bound(case):
    inp = dev("adain", case)
    runs = []
    for _ in range(2):
        o = {"f32": Out(F32, case.NC, case.Lc)}
        ops.adain(inp["content"], inp["style"], o["f32"].arg, case.NC, case.Lc, case.Ls, eps=inp["eps"])
        torch.cuda.synchronize()
        check("adain", F32, case, o)
        runs.append(o["f32"])
    assert same_bits(*runs)


def test_worst_ratios_are_reported():
    """Not a check of its own: prints the largest error / bound each operator reached in this session (pytest -s)."""
    for (op, cls), r in sorted(WORST.items()):
        print(f"NORM_WORST {op} {cls} {r:.4f}")
    assert all(r <= 1.0 for r in WORST.values())
