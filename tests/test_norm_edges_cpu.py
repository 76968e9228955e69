"""CPU: the per-element bounds, references, builders and case lists of tests/norm_cases.py, proven before a GPU is involved.

The clean twin of every kernel (fp32 torch in the kernel's summation order) stays inside the bound on every element of every case the
GPU file runs, in every kind; each seeded defect (the mistakes these kernels invite) breaks the bound on at least one case of every
operator it is seeded in -- so the inputs can see those mistakes.  The ratios are printed (pytest -s)."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC
from norm_cases import ACT_GELU_ERF, ACT_NONE, ACT_RELU, BF16, F16, F16X3, F32

KIND_IDS = lambda k: NC.KIND_NAMES[k]  # noqa: E731
OPS = ["ln", "conv0", "conv_ln", "instnorm", "groupnorm", "adain"]
CASES = {"ln": NC.LN_CASES, "conv0": NC.CONV_CASES, "conv_ln": NC.CONV_CASES, "instnorm": NC.IN_CASES, "groupnorm": NC.GN_CASES,
         "adain": NC.ADA_CASES}
# the kinds an operator writes (the others are refused by its entry point)
OP_KINDS = {"ln": NC.KINDS, "conv0": [F32], "conv_ln": [F32, BF16, F16X3], "instnorm": [F32, BF16], "groupnorm": [F32, BF16, F16X3],
            "adain": [F32]}


@functools.lru_cache(maxsize=None)
def inputs(op, case):
    return case.inputs()


@functools.lru_cache(maxsize=None)
def reference(op, kind, out, case):
    """(y_ref, bound): computed once, shared by the clean run and the defects, never modified."""
    inp = inputs(op, case)
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


@functools.lru_cache(maxsize=None)
def twin(op, kind, case, defect=None):
    """The twin's fp32 result before the output rounding."""
    inp = inputs(op, case)
    if op == "ln":
        return NC.ln_twin(kind, case, inp, defect)
    if op == "conv0":
        return NC.conv_twin(case, inp, defect)
    if op == "conv_ln":
        return NC.conv_ln_twin(kind, case, inp, defect)
    if op == "instnorm":
        return NC.instnorm_twin(case, inp, defect)
    if op == "groupnorm":
        return NC.groupnorm_twin(kind, case, inp, defect)
    return NC.adain_twin(case, inp, defect)


def outs_of(op, kind):
    if op in ("conv0", "adain"):
        return ["f32"]
    if op == "conv_ln":
        return ["f32" if kind == F32 else "t"]
    return ["f32", "t"]


def ratio(op, kind, case, defect=None):
    """Worst error / bound over the outputs of one (kind, case)."""
    y = twin(op, kind, case, defect)
    worst = (0.0, None, 0.0, 0.0)
    for out in outs_of(op, kind):
        ref, bnd = reference(op, kind, out, case)
        got = NC.round_kind(kind, y) if out == "t" else y
        w = NC.worst(got.reshape(ref.shape), ref, bnd)
        if not w[0] <= worst[0]:
            worst = w
    return worst


@pytest.mark.parametrize("op", OPS)
def test_clean_twin_is_inside_the_bound_on_every_case(op):
    bad, top = [], {}
    for kind in OP_KINDS[op]:
        for case in CASES[op]:
            if op == "groupnorm" and case.T > 5000 and kind != F32:
                continue      # (the 65537-frame twin is a 4097-step loop: once)
            r, idx, err, bnd = ratio(op, kind, case)
            top[kind] = max(top.get(kind, 0.0), r)
            if not r <= 1.0:
                bad.append(f"{NC.KIND_NAMES[kind]} {case.id}: error / bound = {r:.3g} at {idx} (|err| {err:.3g}, bound {bnd:.3g})")
    print(f"NORM_CLEAN {op} " + " ".join(f"{NC.KIND_NAMES[k]}={v:.3f}" for k, v in top.items()))
    assert not bad, "\n".join(bad)
    assert max(top.values()) < 1.0


def _applies(defect, op, case):
    if op == "ln":
        return {"third_wave_dropped": case.d == 768, "addend_row_mod_group": case.form == "shared",
                "table_row_k": case.form in ("addends", "two_add", "clip"), "addend_before_stage1": case.form == "two_add",
                "one_pass_var": case.builder.startswith("offset"), "eps_left_out": case.builder in ("tiny", "constant"),
                "eps_outside_sqrt": case.builder == "tiny"}.get(defect, True)
    if op in ("instnorm", "groupnorm"):
        L = case.L if op == "instnorm" else case.T
        return {"divide_by_L": bool(case.lens), "chunk_frame_twice": op == "groupnorm" and (case.chunked or bool(case.lens)) and L >= 4096,
                "chunk_frame_dropped": op == "groupnorm" and (case.chunked or bool(case.lens)) and L >= 4096,
                "one_pass_var": case.builder.startswith("offset") and L > 1 and not (op == "groupnorm" and case.chunked),
                "eps_left_out": case.builder in ("tiny", "constant"), "eps_outside_sqrt": case.builder == "tiny",
                "biased_unbiased_swap": L > 1, "leaky_skipped": case.builder != "constant",
                "leaky_after_norm": case.builder != "constant" and L > 1}.get(defect, True)
    if op == "adain":
        return {"one_pass_var": case.content.startswith("offset") or case.style.startswith("offset"),
                "eps_left_out": "tiny" in (case.content, case.style) or case.content == "constant",
                "eps_outside_sqrt": "tiny" in (case.content, case.style) or case.content == "constant"}.get(defect, True)
    if op == "conv_ln" and defect == "one_pass_var":
        return True
    return case.T0 > 1 if defect == "conv_stride_4" else True


@pytest.mark.parametrize("defect,op", [(d, op) for d, where in NC.DEFECTS.items() for op in where])
def test_seeded_defect_breaks_the_bound(defect, op):
    caught, tried = [], 0
    for kind in OP_KINDS[op]:
        hit = None
        for case in CASES[op]:
            if not _applies(defect, op, case) or (op == "groupnorm" and case.T > 5000):
                continue
            tried += 1
            r = ratio(op, kind, case, defect)[0]
            if not r <= 1.0:
                hit = (case.id, r)
                break
        assert hit, f"defect {defect} survives every {op} case for kind {NC.KIND_NAMES[kind]}"
        caught.append(f"{NC.KIND_NAMES[kind]}: {hit[0]} {hit[1]:.3g}")
    print(f"NORM_DEFECT {defect} {op} " + "; ".join(caught))
    assert tried


def test_one_pass_variance_is_far_outside_the_bound_at_offset():
    """The defect today's relative-to-max test passes: E[x^2] - mean^2 in fp32.  Tens of bounds at mean = 100 std."""
    rs = [ratio("ln", F32, c, "one_pass_var")[0] for c in NC.LN_CASES if c.form == "plain" and c.act == ACT_NONE and c.M == 5
          and c.builder in ("offset100", "offset1000")]
    print("NORM_ONE_PASS ln " + " ".join(f"{r:.3g}" for r in rs))
    assert len(rs) == 8 and min(rs) > 1.0


def rel64(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))      # (normalised outputs are O(1), or 0 for a constant row)


def centred(t, dim):
    """t minus its (fp32-rounded, so exactly subtracted) mean over dim: a normalisation does not see the shift, and torch's
    float64 functionals then carry no conditioning error of their own at mean = 1000 std."""
    return t - t.mean(dim, keepdim=True).float().double()


def test_references_agree_with_torch_functional_in_float64():
    tol = 1e-12
    for case in NC.LN_CASES:
        if case.form != "plain":
            continue
        inp = inputs("ln", case)
        y, _ = reference("ln", F32, "f32", case)
        want = F.layer_norm(centred(inp["x"][0].double(), 1), (case.d,), inp["gamma"].double(), inp["beta"].double(), NC.EPS)
        want = {ACT_RELU: F.relu, ACT_GELU_ERF: F.gelu, ACT_NONE: lambda t: t}[case.act](want)
        assert rel64(y, want) < tol, case.id
    # two stages with addends, by hand from F.layer_norm
    case = next(c for c in NC.LN_CASES if c.form == "two_add" and c.act == ACT_NONE)
    inp = inputs("ln", case)
    h = F.layer_norm(inp["x"][0].double(), (case.d,), inp["gamma"].double(), inp["beta"].double(), NC.EPS)
    h = h + inp["add_mat"].double() + inp["add_tab"].double()[int(inp["tab_index"][int(inp["tab_step"][0])])]
    want = F.layer_norm(h, (case.d,), inp["gamma2"].double(), inp["beta2"].double(), NC.EPS)
    assert rel64(reference("ln", F32, "f32", case)[0], want) < tol
    for case in NC.CONV_CASES:
        inp = inputs("conv0", case)
        b = inp["bias"].double() if inp["bias"] is not None else None
        conv = F.conv1d(inp["wav"].double().unsqueeze(1), inp["w"].double().unsqueeze(1), b, stride=5).transpose(1, 2)
        assert conv.shape[1] == case.T0
        assert rel64(reference("conv0", F32, "f32", case)[0], conv) < tol, case.id
        want = F.gelu(F.layer_norm(centred(conv, 2), (512,), inp["gamma"].double(), inp["beta"].double(), NC.EPS))
        assert rel64(reference("conv_ln", F32, "f32", case)[0], want) < tol, case.id
    for case in NC.IN_CASES:
        x = inputs("instnorm", case)["x"].double()
        y, _ = reference("instnorm", F32, "f32", case)
        for b in range(x.shape[0]):
            Lb = case.lens[b] if case.lens else case.L
            if Lb > 1:
                want = F.instance_norm(centred(F.leaky_relu(x[b:b + 1, :Lb], 0.2), 1).transpose(1, 2), eps=NC.EPS).transpose(1, 2)
                assert rel64(y[b:b + 1, :Lb], want) < tol, case.id
            else:
                assert float(y[b, :Lb].abs().max()) == 0.0      # (F.instance_norm refuses one frame: the definition gives 0)
            assert float(y[b, Lb:].abs().sum()) == 0.0
    for case in NC.GN_CASES:
        inp = inputs("groupnorm", case)
        x = inp["x"].double()
        y, _ = reference("groupnorm", F32, "f32", case)
        g = inp["gamma"].double() if inp["gamma"] is not None else None
        bt = inp["beta"].double() if inp["beta"] is not None else None
        for b in range(x.shape[0]):
            Tb = case.lens[b] if case.lens else case.T
            if Tb > 1:
                want = F.group_norm(centred(x[b:b + 1, :Tb], 1).transpose(1, 2), case.C, g, bt, NC.EPS).transpose(1, 2)
            else:       # (F.group_norm refuses one frame: the definition gives beta)
                want = (bt if bt is not None else torch.zeros(case.C, dtype=torch.float64)).view(1, 1, case.C)
            want = F.gelu(want) if case.act == ACT_GELU_ERF else want
            assert rel64(y[b:b + 1, :Tb], want) < tol, case.id
            assert float(y[b, Tb:].abs().sum()) == 0.0


def test_adain_reference_agrees_with_the_golden():
    """tests/golden/audio_misc.npz holds the reference implementation's fp32 result: the fp64 reference agrees to fp32 rounding
    (the golden's own precision), and to 1e-12 with the definition written with torch.var in float64."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "audio_misc.npz"))
    c, s = torch.from_numpy(z["adain_c"]).reshape(12, 11), torch.from_numpy(z["adain_s"]).reshape(12, 9)
    y, _ = NC.adain_reference(NC.AdaCase("golden", "golden", 12, 11, 9), {"content": c, "style": s, "eps": NC.EPS})
    want = torch.from_numpy(z["adain_out"]).reshape(12, 11).double()
    assert float((y - want).abs().max()) <= 8 * 2.0 ** -24 * float(want.abs().max())
    for case in NC.ADA_CASES:
        inp = inputs("adain", case)
        c, s = inp["content"].double(), inp["style"].double()
        want = (c - c.mean(1, keepdim=True)) / (c.var(1, keepdim=True) + NC.EPS).sqrt() * (s.var(1, keepdim=True) + NC.EPS).sqrt() + s.mean(1, keepdim=True)
        assert rel64(reference("adain", F32, "f32", case)[0], want) < 1e-12, case.id


def test_gelu_fast_formula_error_is_the_recorded_constant():
    e = NC.gelu_fast_formula_error()
    print(f"NORM_GELU_FAST formula error {e:.4g} on linspace{NC.GELU_FAST_GRID}")
    assert 0.5 * NC.GELU_FAST_FORMULA_ERR < e <= NC.GELU_FAST_FORMULA_ERR
    v = torch.linspace(-8.0, 8.0, 4001, dtype=torch.float64)
    assert rel64(NC.gelu64(v), F.gelu(v)) < 1e-12
    assert float(((NC.gelu64(v + 1e-6) - NC.gelu64(v)) / 1e-6).abs().max()) < NC.GELU_LIP


def test_builders_are_what_they_claim():
    R, n = 6, 1024
    sl = torch.arange(n) // 256
    for name, k in (("offset100", 100.0), ("offset1000", 1000.0)):
        x = NC.build(name, R, n).double()
        ratio_ = x.mean(1) / x.std(1)
        assert bool(((ratio_ > 0.9 * k) & (ratio_ < 1.1 * k)).all()), name
    x = NC.build("centred", R, n).double()
    assert float(x.mean(1).abs().max()) < 0.15 and 0.9 < float(x.std(1).min())
    x = NC.build("tiny", R, n).double()
    assert float(x.var(1).max()) < 1e-2 * NC.EPS
    x = NC.build("constant", R, n)
    assert float((x - x[:, :1]).abs().max()) == 0.0 and float(x.double().var(1).max()) == 0.0 and x[:, 0].unique().numel() == R
    x = NC.build("outlier", R, n)
    assert float(x.abs().max()) == 1e4 and int((x.abs() > 10).sum()) == R
    x = NC.build("wave_skew", R, n, sl).double().view(R, 4, 256)
    m, sd = x.mean(2), x.std(2)
    assert float((m[:, 1:] - m[:, :-1]).abs().min()) > 5.0 and float(sd.max() / sd.min()) > 6.0
    xt = NC.build("wave_skew", 4, 64, torch.arange(64) % 16).double().view(4, 4, 16)           # time kernels: one mean per time-lane
    assert torch.unique(xt.mean(1).round(), dim=1).shape[1] == 16
    x = NC.build("row_scales", R, n).double().std(1)
    assert float(x.max() / x.min()) > 5e5
    x = NC.build("negative_heavy", R, n)
    assert float((x < 0).float().mean()) > 0.85


def test_case_lists_meet_every_edge():
    ln = NC.LN_CASES
    plain = {(c.d, c.M, c.builder) for c in ln if c.form == "plain" and c.act == ACT_NONE}
    assert plain == {(d, M, b) for d in (256, 512, 768, 1024) for M in (1, 5) for b in NC.BUILDERS}
    assert {c.form for c in ln} == set(NC.LN_FORMS)
    assert {c.planes for c in ln} >= {2, 3, 4} and all(c.plane_stride > c.M * c.d and c.plane_stride % 4 == 0 for c in ln)
    assert {c.act for c in ln} == {ACT_NONE, ACT_RELU, ACT_GELU_ERF}
    assert any(c.form in ("two", "two_add") and c.act == ACT_GELU_ERF for c in ln)            # two stages with an activation
    assert {c.d for c in ln if c.form != "plain"} == {256, 512, 768, 1024}
    sh = [c for c in ln if c.form == "shared"]
    assert all(c.M == 24 and (i["add_mat_L"], i["add_mat_group"], i["add_mat_wrap"]) == (3, 6, 12) for c in sh for i in [c.inputs()])
    cl = next(c for c in ln if c.form == "clip").inputs()
    assert cl["clip_step_stride"] > 1 and cl["clip_wrap"] > 0 and all(int(cl["tab_index"][k]) != k for k in range(10))
    ins = NC.IN_CASES
    assert {c.L for c in ins} == {1, 2, 15, 16, 17, 33} and {c.d for c in ins} == {8, 64, 72} and all(c.B == 2 for c in ins)
    assert {(c.L, c.d) for c in ins if not c.lens} >= {(L, d) for L in (1, 33) for d in (8, 64, 72)}
    assert any(c.lens and c.lens[0] == 1 and 1 < c.lens[1] < c.L and c.lens[2] == c.L for c in ins)
    assert any(c.builder == "negative_heavy" for c in ins)
    gn = NC.GN_CASES
    assert {c.T for c in gn if c.scratch == "none" and not c.lens} >= {1, 15, 16, 17, 300} and {c.C for c in gn} == {8, 96}
    assert {c.T for c in gn if c.scratch == "full" and not c.lens} == {4095, 4096, 4097, 5000, 65537}
    assert all(c.C == 8 for c in gn if c.T >= 4095) and max(c.T * c.C * c.B for c in gn) <= 65537 * 8
    assert any(c.scratch == "small" and c.T >= 4096 for c in gn)
    assert {c.T for c in gn if c.scratch == "none"} >= {4096, 4097}                            # three-pass beside chunked
    assert any(not c.affine for c in gn) and {c.act for c in gn} == {ACT_NONE, ACT_GELU_ERF}
    assert any(c.lens == (1, 4095, 4096, 4097) and c.T == 4097 for c in gn)
    assert NC.chunks_of(65537)[0] == 64 and NC.chunks_of(65537)[0] * 1024 < 65537              # more frames than 64 chunks of 1024
    ad = NC.ADA_CASES
    assert {c.NC for c in ad} == {1, 5} and {c.Lc for c in ad} == set(NC._L6) and {c.Ls for c in ad} == set(NC._L6)
    assert any(c.style == "offset100" for c in ad) and any(c.content == "constant" for c in ad)
    cv = NC.CONV_CASES
    assert {c.T0 for c in cv} == {1, 7, 8, 9, 15, 16, 17, 31, 32, 33} and {c.extra for c in cv} == {0, 4} and all(c.B == 2 for c in cv)
    assert {c.bias for c in cv} == {True, False} and all((c.n - 10) // 5 + 1 == c.T0 for c in cv)
    w = cv[0].inputs()["w"]
    assert float((w - 1.0).abs().max()) < 0.5
    assert all(op in OPS for where in NC.DEFECTS.values() for op in where) and len(NC.DEFECTS) >= 14
