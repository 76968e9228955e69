"""GPU: the scheduler's Philox noise and its updates, element by element against the host model of tests/sched_cases.py (never
against another GPU path): which value enters which counter and key word, the fp32 uniforms, the hardware log / sine / cosine inside
the tolerance derived there, the indexing over clips, steps and the grid-stride loop; the three update forms with DRAWN noise bit
for bit against their unfused fp32 expression; the operand copies in every kind; the in-kernel step advance with tables that
differ at every step.  Outputs sit between 64-element sentinel guards.  tests/test_sched_noise_cpu.py shows that the model's cases
see the defects this code invites."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import norm_cases as NC  # noqa: E402
import sched_cases as SC  # noqa: E402
from attn_cases import split_host  # noqa: E402
from norm_cases import BF16, F16, F16X3, F32  # noqa: E402
from fdm_amd import ops  # noqa: E402

DEV = "cuda:0"
GUARD, SENT = 64, -7.0
NAN = float("nan")
NT = 16                                       # rows of every table here (t and k stay below it)
CASE_IDS = lambda c: c.id  # noqa: E731
KIND_IDS = lambda k: NC.KIND_NAMES[k]  # noqa: E731
# the worst |device - model| of sections A and B in this session: absolute, as the sine / cosine error |dz| / ra, and as a
# ratio to the tolerance (printed by test_noise_worst_is_reported)
WORST = {"abs": 0.0, "trig": 0.0, "ratio": 0.0, "where": ""}


class Buf:
    """n elements filled with `fill` between two guards of 64 sentinel elements."""

    def __init__(self, n, fill=NAN, dtype=torch.float32):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT, device=DEV, dtype=dtype)
        self.arg = self.buf[GUARD:GUARD + n]
        if torch.is_tensor(fill):
            self.arg.copy_(fill)
        else:
            self.arg.fill_(fill)

    def guards_intact(self):
        return bool((torch.cat([self.buf[:GUARD], self.buf[GUARD + self.n:]]) == SENT).all())

    def cpu(self):
        return self.arg.cpu()


def dev(v, dtype=torch.float32):
    return torch.as_tensor(v, dtype=dtype).to(DEV)


def table(entries, fill=NAN):
    """A device fp32 table of NT rows: `entries` {row: value}, every other row `fill` (NaN: a wrong row shows)."""
    t = torch.full((NT,), fill)
    for i, v in entries.items():
        t[i] = v
    return t.to(DEV)


def step_word(k):
    return dev([k], torch.int32)


TSEQ_DEV = None


def tseq_dev():
    global TSEQ_DEV
    if TSEQ_DEV is None:
        TSEQ_DEV = dev(SC.TSEQ, torch.int32)
    return TSEQ_DEV


def draw(case, seed_dev=False):
    """The identity launch: mode 0 with x0 = x = 0, c1 = c2 = 0, sigma = 1 -- 0 + 1 * z is z bit for bit -> fp32 CPU [n]."""
    n = case.n
    zeros = torch.zeros(n, device=DEV)
    out = Buf(n)
    key = ({"seed_dev": dev([SC.as_i64(case.seed), case.clip0], torch.int64)} if seed_dev
           else {"seed": case.seed, "clip0": case.clip0})
    ops.sched_step(0, zeros, zeros, out.arg, n, n_per_clip=case.n_per_clip, tseq=tseq_dev(), step=step_word(case.k),
                   c1=table({}, 0.0), c2=table({}, 0.0), sigma=table({}, 1.0), **key)
    torch.cuda.synchronize()
    assert out.guards_intact()
    return out.cpu()


def hold_to_model(got, z, ra, where):
    """Record the worst figures, then assert every element inside the tolerance."""
    got = got.double().numpy()
    assert np.isfinite(got).all(), where
    err = np.abs(got - z)
    i = int(err.argmax())
    with np.errstate(divide="ignore", invalid="ignore"):
        trig = np.where(ra > 0.0, err / ra, 0.0)
    ratio = err / SC.noise_bound(z, ra)
    if err[i] > WORST["abs"]:
        WORST["abs"], WORST["where"] = float(err[i]), f"{where} element {i}"
    WORST["trig"] = max(WORST["trig"], float(trig.max()))
    WORST["ratio"] = max(WORST["ratio"], float(ratio.max()))
    assert err[i] <= SC.NOISE_ERR_CONDITION, (where, i, float(err[i]))
    j = int(ratio.argmax())
    assert ratio[j] <= 1.0, (where, j, float(got[j]), float(z[j]), float(err[j]), float(ratio[j]))


# ---------------------------------------------------------------------------------------------------------------------
# A. the noise per element
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.noise_cases(), ids=CASE_IDS)
def test_noise_per_element_against_the_model(case):
    got = draw(case)
    if case.t == 0:                           # mode 0 draws nothing at t = 0: exact zeros
        assert torch.equal(got, torch.zeros(case.n))
        return
    z, ra, _ = SC.noise_reference(case.seed, case.clip0, case.k, case.n, case.n_per_clip)
    hold_to_model(got, z, ra, case.id)


def test_tail_quads_take_the_edge_inputs():
    """u0 = 1: the radius is +-0 and the pair exactly 0.  The smallest u0 of the search: |z| beyond 4."""
    one = draw(SC.NoiseCase(SC.TAIL_SEED_U0_ONE, 0, 0, 4, 4))
    assert float(one[0]) == 0.0 and float(one[1]) == 0.0 and bool(torch.isfinite(one).all())
    small = draw(SC.NoiseCase(SC.TAIL_SEED_U0_SMALL, 0, 0, 4, 4))
    assert float(small[:2].abs().max()) > 4.0


@pytest.mark.parametrize("seed", SC.SEEDS + SC.tail_seeds(), ids=hex)
def test_seed_high_word_reaches_the_key(seed):
    a = draw(SC.NoiseCase(seed, 5, 1, 24, 8))
    b = draw(SC.NoiseCase((seed + 2 ** 32) % 2 ** 64, 5, 1, 24, 8))
    assert not bool((a == b).any())


@pytest.mark.parametrize("case", [SC.NoiseCase(0xDEADBEEF00000000, 2 ** 31 - 4, 9, 24, 8), SC.NoiseCase(2 ** 64 - 1, 5, 1, 24, 8),
                                  SC.NoiseCase(SC.TAIL_SEED_U0_SMALL, 0, 0, 4, 4)], ids=CASE_IDS)
def test_device_seed_words_give_the_host_seed_bits(case):
    assert torch.equal(draw(case, seed_dev=True), draw(case))


@pytest.mark.parametrize("case", SC.grid_cases(), ids=CASE_IDS)
def test_noise_over_the_grid_stride_loop(case):
    """More quads than the capped grid has lanes: the elements from 2^21 on are the second trip of the loop."""
    assert case.n // 4 > SC.GRID_QUADS
    got = draw(case)
    z, ra, _ = SC.noise_reference(case.seed, case.clip0, case.k, case.n, case.n_per_clip)
    hold_to_model(got, z, ra, case.id)


# ---------------------------------------------------------------------------------------------------------------------
# B. slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 3])
def test_slot_noise_against_the_model(mode):
    """Three slots at their own (k, t) and key, one of them not live: the live rows hold the model's noise for THEIR key and step,
    nothing of the dead slot is stored (x_out, x_out_t, x0_hist), no guard moves."""
    npc, ns = SC.SLOT_N_PER_CLIP, len(SC.SLOT_KEYS)
    n = npc * ns
    g = torch.Generator().manual_seed(31)
    x0, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    out, out_t, hist = Buf(n), Buf(n), Buf(n, fill=3.0)
    state = dev(SC.SLOT_STATE, torch.int32)
    keys = dev([[SC.as_i64(s), c] for s, c in SC.SLOT_KEYS], torch.int64)
    if mode == 0:                             # 0 * x0 + 0 * x + 1 * z
        kw = {"c1": table({}, 0.0), "c2": table({}, 0.0), "sigma": table({}, 1.0)}
    else:
        kw = {"lm_a": table({}, 0.0), "lm_b": table({}, 0.0), "lm_c": table({}, 0.0), "lm_s": table({}, 1.0), "x0_hist": hist.arg}
    ops.slot_sched(mode, x0.to(DEV), x.to(DEV), out.arg, n, state, keys, ns, n_per_clip=npc, x_out_t=out_t.arg, **kw)
    torch.cuda.synchronize()
    assert out.guards_intact() and out_t.guards_intact() and hist.guards_intact()
    got, got_t, h = out.cpu().view(ns, npc), out_t.cpu().view(ns, npc), hist.cpu().view(ns, npc)
    for s, ((seed, clip), (k, t, live, _)) in enumerate(zip(SC.SLOT_KEYS, SC.SLOT_STATE)):
        if not live:
            assert bool(torch.isnan(got[s]).all()) and bool(torch.isnan(got_t[s]).all()) and bool((h[s] == 3.0).all())
            continue
        z, ra, _ = SC.noise_reference(seed, clip, k, npc, npc)
        hold_to_model(got[s], z, ra, f"slot{s}-mode{mode}")
        assert torch.equal(got_t[s], got[s])
        assert torch.equal(h[s], x0.view(ns, npc)[s]) if mode == 3 else bool((h[s] == 3.0).all())
    assert torch.equal(state.cpu(), torch.tensor(SC.SLOT_STATE, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------------------------
# C. the updates with drawn noise, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
N_UPD = 4 * 257                               # two blocks, the second with one active lane
UPD_KEY = dict(seed=2 ** 32 + 1, clip0=5)
UPD_K = 3                                     # t = TSEQ[3] = 5


def _operands(mix):
    op = SC.update_operands(N_UPD)
    kw = {"x0u": op["x0u"].to(DEV), "cfg_scale": SC.CFG_SCALE} if mix else {}
    x0m = SC.cfg_mix(op["x0"], op["x0u"], SC.CFG_SCALE) if mix else op["x0"]
    return op, kw, x0m


def _drawn(k=UPD_K):
    return draw(SC.NoiseCase(UPD_KEY["seed"], UPD_KEY["clip0"], k, N_UPD, N_UPD))


def _lm_tables(coefs, k):
    a, b, c, s = coefs
    return {"lm_a": table({k: a}), "lm_b": table({k: b}), "lm_c": table({k: c}), "lm_s": table({k: s})}


@pytest.mark.parametrize("mix", [False, True], ids=["nomix", "cfg"])
def test_mode0_update_with_drawn_noise_bit_exact(mix):
    c1, c2, sg, t = SC.MODE0_COEFS["t5"]
    assert t == SC.TSEQ[UPD_K]
    op, kw, x0m = _operands(mix)
    out = Buf(N_UPD)
    ops.sched_step(0, op["x0"].to(DEV), op["x"].to(DEV), out.arg, N_UPD, n_per_clip=N_UPD, tseq=tseq_dev(), step=step_word(UPD_K),
                   c1=table({t: c1}), c2=table({t: c2}), sigma=table({t: sg}), **UPD_KEY, **kw)
    torch.cuda.synchronize()
    assert out.guards_intact()
    assert torch.equal(out.cpu(), SC.update_mode0(c1, c2, sg, t, x0m, op["x"], _drawn()))


@pytest.mark.parametrize("mix", [False, True], ids=["nomix", "cfg"])
def test_mode3_update_with_drawn_noise_bit_exact(mix):
    coefs = SC.MODE3_COEFS["all"]
    op, kw, x0m = _operands(mix)
    out, hist = Buf(N_UPD), Buf(N_UPD, fill=op["h"])
    ops.sched_step(3, op["x0"].to(DEV), op["x"].to(DEV), out.arg, N_UPD, n_per_clip=N_UPD, tseq=tseq_dev(), step=step_word(UPD_K),
                   x0_hist=hist.arg, **_lm_tables(coefs, UPD_K), **UPD_KEY, **kw)
    torch.cuda.synchronize()
    assert out.guards_intact() and hist.guards_intact()
    assert torch.equal(out.cpu(), SC.update_mode3(*coefs, x0m, op["x"], op["h"], _drawn()))
    assert torch.equal(hist.cpu(), x0m)                                   # the history now holds the (mixed) x0


def test_mode3_zero_history_coefficient_never_reads_the_history():
    coefs = SC.MODE3_COEFS["no_hist"]
    op, kw, x0m = _operands(True)
    out, hist = Buf(N_UPD), Buf(N_UPD, fill=NAN)
    ops.sched_step(3, op["x0"].to(DEV), op["x"].to(DEV), out.arg, N_UPD, n_per_clip=N_UPD, tseq=tseq_dev(), step=step_word(UPD_K),
                   x0_hist=hist.arg, **_lm_tables(coefs, UPD_K), **UPD_KEY, **kw)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isfinite(got).all()) and out.guards_intact() and hist.guards_intact()
    assert torch.equal(got, SC.update_mode3(*coefs, x0m, op["x"], None, _drawn()))
    assert torch.equal(hist.cpu(), x0m)


def test_mode3_zero_noise_coefficient_never_reads_the_noise():
    coefs = SC.MODE3_COEFS["no_noise"]
    op, kw, x0m = _operands(False)
    k = 1
    out, hist = Buf(N_UPD), Buf(N_UPD, fill=op["h"])
    noise = torch.full((k + 1, N_UPD), NAN, device=DEV)
    ops.sched_step(3, op["x0"].to(DEV), op["x"].to(DEV), out.arg, N_UPD, tseq=tseq_dev(), step=step_word(k), noise=noise,
                   x0_hist=hist.arg, **_lm_tables(coefs, k))
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isfinite(got).all()) and out.guards_intact() and hist.guards_intact()
    assert torch.equal(got, SC.update_mode3(*coefs, x0m, op["x"], op["h"], None))


@pytest.mark.parametrize("mode", [0, 3])
def test_injected_noise_stride(mode):
    """Row k of an injected noise buffer whose rows lie n + 8 elements apart, against the default stride (n)."""
    op, _, x0 = _operands(False)
    k, stride = 2, N_UPD + 8
    wide = torch.randn(k + 1, stride, generator=torch.Generator().manual_seed(8))
    z = wide[k, :N_UPD].contiguous()
    outs = []
    for noise, st in ((wide, stride), (wide[:, :N_UPD].contiguous(), 0)):
        out, hist = Buf(N_UPD), Buf(N_UPD, fill=op["h"])
        if mode == 0:
            c1, c2, sg, t = SC.MODE0_COEFS["t5"]
            tseq = dev([9, 9, t], torch.int32)
            ops.sched_step(0, x0.to(DEV), op["x"].to(DEV), out.arg, N_UPD, tseq=tseq, step=step_word(k), noise=noise.to(DEV),
                           noise_stride=st, c1=table({t: c1}), c2=table({t: c2}), sigma=table({t: sg}))
            want = SC.update_mode0(c1, c2, sg, t, x0, op["x"], z)
        else:
            coefs = SC.MODE3_COEFS["all"]
            ops.sched_step(3, x0.to(DEV), op["x"].to(DEV), out.arg, N_UPD, tseq=tseq_dev(), step=step_word(k), noise=noise.to(DEV),
                           noise_stride=st, x0_hist=hist.arg, **_lm_tables(coefs, k))
            want = SC.update_mode3(*coefs, x0, op["x"], op["h"], z)
        torch.cuda.synchronize()
        assert out.guards_intact() and hist.guards_intact()
        outs.append(out.cpu())
        assert torch.equal(outs[-1], want)
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------------
# D. operand copies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, N_UPD])
@pytest.mark.parametrize("kind,gap", [(F32, 0), (BF16, 0), (F16, 0), (F16X3, 0), (F16X3, 72)],
                         ids=["f32", "bf16", "f16", "f16x3-lo_n", "f16x3-lo_n+72"])
def test_operand_copy_is_the_rounded_output(kind, gap, n):
    """x_out_t = round_kind(kind, x_out) bit for bit (mode 3 with drawn noise, so x0_hist is written too); the split kind with its
    lo plane n and n + 72 elements after the hi plane.  Every output between guards that stay."""
    coefs = SC.MODE3_COEFS["all"]
    op = SC.update_operands(n, seed=1)
    op["x"] = op["x"] * 300.0                                             # |x_out| up to ~1000: several binades of every kind
    out, hist = Buf(n), Buf(n, fill=op["h"])
    dt = ops.tdtype(kind)
    if kind == F16X3:
        out_t = Buf(2 * n + gap, fill=SENT if gap else NAN, dtype=dt)     # hi | gap (keeps the sentinel) | lo
        arg = ops.Split(out_t.buf.view(1, 1, -1), F16X3, 0, GUARD)
        arg.lo_off = n + gap
    else:
        out_t = Buf(n, dtype=dt)
        arg = out_t.arg
    ops.sched_step(3, op["x0"].to(DEV), op["x"].to(DEV), out.arg, n, n_per_clip=n, tseq=tseq_dev(), step=step_word(UPD_K),
                   x0_hist=hist.arg, x_out_t=arg, **_lm_tables(coefs, UPD_K), **UPD_KEY)
    torch.cuda.synchronize()
    assert out.guards_intact() and out_t.guards_intact() and hist.guards_intact()
    got = out.cpu()
    z = draw(SC.NoiseCase(UPD_KEY["seed"], UPD_KEY["clip0"], UPD_K, n, n))
    assert torch.equal(got, SC.update_mode3(*coefs, op["x0"], op["x"], op["h"], z))
    assert torch.equal(hist.cpu(), op["x0"])
    t = out_t.cpu()
    if kind == F16X3:
        planes = split_host(got)
        assert torch.equal(t[:n], planes[0]) and torch.equal(t[n + gap:], planes[1])
        assert bool((t[n:n + gap] == SENT).all())
        assert torch.equal(t[:n].float() + t[n + gap:].float() / NC.SPLIT_SCALE, NC.round_kind(F16X3, got))
    else:
        assert torch.equal(t.float(), NC.round_kind(kind, got))
        assert float(got.abs().max()) > 100.0


# ---------------------------------------------------------------------------------------------------------------------
# E. the in-kernel advance with tables that differ at every step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ticket", [True, False], ids=["ticket", "advance_launch"])
@pytest.mark.parametrize("n", [4 * 256 * 64, 2 ** 21])
def test_advance_with_step_dependent_tables(n, ticket):
    """16 launches back to back, none synchronised with the host; launch k writes row k with the coefficients of t = tseq[k]:
    c1[t] = 1 + t / 64 and c2[t] = 2^-t (exact in fp32), tseq a permutation.  A wave that read the step word of another launch
    writes other bits.  ticket: the last block advances the word inside the kernel; else the separate advance launch."""
    K = 16
    perm = [11, 3, 14, 0, 7, 9, 1, 15, 5, 12, 2, 8, 13, 6, 10, 4]
    c1 = torch.tensor([1.0 + t / 64.0 for t in range(K)])
    c2 = torch.tensor([2.0 ** -t for t in range(K)])
    g = torch.Generator().manual_seed(n)
    x0, x = torch.randn(n, generator=g), torch.randn(n, generator=g)
    x0d, xd = x0.to(DEV), x.to(DEV)
    tseq, step = dev(perm, torch.int32), dev([0], torch.int32)
    arrive = dev([0], torch.int32) if ticket else None
    noise = torch.zeros(K, n, device=DEV)
    out = torch.full((K, n), NAN, device=DEV)
    c1d, c2d, sg = c1.to(DEV), c2.to(DEV), torch.zeros(K, device=DEV)
    for k in range(K):
        ops.sched_step(0, x0d, xd, out[k], n, tseq=tseq, step=step, advance=1, c1=c1d, c2=c2d, sigma=sg, noise=noise, arrive=arrive)
    torch.cuda.synchronize()
    assert int(step[0]) == K and (arrive is None or int(arrive[0]) == 0)
    got = out.cpu()
    for k in range(K):
        t = perm[k]
        assert torch.equal(got[k], c1[t] * x0 + c2[t] * x), (k, t)


# ---------------------------------------------------------------------------------------------------------------------
# F. report
# ---------------------------------------------------------------------------------------------------------------------
def test_noise_worst_is_reported():
    """Not a check of its own: prints the worst |device - model| that A and B reached in this session (pytest -s) -- absolute, as
    the error of the sine / cosine (|dz| / ra, what E_TRIG_MEASURED of tests/sched_cases.py records) and as a ratio to the
    tolerance."""
    print(f"NOISE_WORST abs {WORST['abs']:.4e} at {WORST['where']}")
    print(f"NOISE_WORST trig {WORST['trig']:.4e} (E_TRIG {SC.E_TRIG})")
    print(f"NOISE_WORST ratio {WORST['ratio']:.4f}")
    assert WORST["abs"] <= SC.NOISE_ERR_CONDITION and WORST["ratio"] <= 1.0
