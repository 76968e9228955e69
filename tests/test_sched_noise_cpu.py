"""Host checks of tests/sched_cases.py, the model tests/test_sched_noise_gpu.py holds the scheduler kernels to: Philox4x32-10 against
its published known answers, the statistics of the modelled noise, every defect twin caught on its case, the tail seeds, and the
fp32 update expressions against fp64 within their rounding counts.  No GPU."""
import numpy as np
import pytest
import torch

import sched_cases as SC


def test_philox_known_answers_scalar_and_vectorised():
    for counter, key, want in SC.PHILOX_KAT:
        assert SC.philox4x32_10_scalar(counter, key) == want
        assert tuple(int(v) for v in SC.philox4x32_10(counter, key)) == want
    # the vectorised form over an array of counters and of keys is the scalar form element by element
    c0 = np.array([0, 1, 0xFFFFFFFF, 0x243f6a88], dtype=np.uint64)
    k0 = np.array([0, 0xFFFFFFFF, 5, 0xa4093822], dtype=np.uint64)
    got = SC.philox4x32_10((c0, 7, 0xFFFFFFFE, 0), (k0, 0x299f31d0))
    for i in range(4):
        assert tuple(int(v) for v in got[i]) == SC.philox4x32_10_scalar((int(c0[i]), 7, 0xFFFFFFFE, 0), (int(k0[i]), 0x299f31d0))


def test_uniforms_are_the_kernels_fp32_values():
    r = np.array([[0, 0, 2 ** 32 - 1, 2 ** 32 - 1], [2 ** 32 - 128, 2 ** 24 + 1, 2 ** 32 - 129, 2 ** 31]], dtype=np.uint64)
    u0, u1, u2, u3 = SC.uniforms(r)
    assert all(u.dtype == np.float32 for u in (u0, u1, u2, u3))
    assert float(u0[0]) == 2.0 ** -33 and float(u1[0]) == 0.0            # the smallest log argument the code can form
    assert float(u2[0]) == 1.0 and float(u3[0]) == 1.0                   # f32(2^32 - 1) = 2^32: one whole turn
    assert float(u0[1]) == 1.0                                           # 2^32 - 128 is a tie: to even, 2^32
    assert float(u2[1]) == 1.0 - 2.0 ** -24                              # 2^32 - 129 rounds down to 2^32 - 256
    assert float(u1[1]) == 2.0 ** -8 and float(u3[1]) == 0.5             # 2^24 + 1 is a tie: to even, 2^24
    z = SC.normals64(0, 0, 0, 0)
    assert z.shape == (4,) and np.all(np.isfinite(z))
    assert SC.RA_MAX == pytest.approx(6.7638, abs=1e-4)


def test_model_statistics():
    """2^20 draws: every interval is +- 5 standard errors of its estimator at this sample size (unit normal: var z = 1,
    var z^2 = 2, var z^4 = 96, var of a product of two uncorrelated draws = 1)."""
    n, npc, seed, k = 2 ** 20, 2 ** 16, 0x9E3779B97F4A7C15, 3
    z = SC.noise_model(seed, 11, k, n, npc)
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)
    assert abs((z * z).mean() - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs((z ** 4).mean() - 3.0) <= 5.0 * np.sqrt(96.0 / n)

    def corr_ok(a, b):
        return abs((a * b).mean()) <= 5.0 / np.sqrt(a.size)
    q = z.reshape(-1, 4)
    assert corr_ok(q[:, :3].reshape(-1), q[:, 1:].reshape(-1))            # neighbouring lanes of a quad
    assert corr_ok(q[:-1].reshape(-1), q[1:].reshape(-1))                 # neighbouring quads
    assert corr_ok(z, SC.noise_model(seed, 11, k + 1, n, npc))            # steps k and k + 1 of one element
    c = z.reshape(-1, npc)
    assert corr_ok(c[:-1].reshape(-1), c[1:].reshape(-1))                 # the same element of neighbouring clips


@pytest.mark.parametrize("defect", SC.DEFECTS)
def test_defect_twin_is_caught(defect):
    """Each defect moves >= 99 % of the elements it can reach in its case by more than the noise tolerance -- and by more than the
    1e-4 condition, so the exact tolerance is uncritical."""
    dc = SC.defect_cases()[defect]
    cs = dc.case
    z, ra = SC._model(cs.seed, cs.clip0, cs.k, cs.n, cs.n_per_clip)
    zd = SC.noise_model(cs.seed, cs.clip0, cs.k, cs.n, cs.n_per_clip, defect=defect, t=cs.t)
    tol = np.maximum(SC.noise_bound(z, ra), SC.NOISE_ERR_CONDITION)
    with np.errstate(invalid="ignore"):
        diff = np.abs(zd - z)
    caught = ~(diff <= tol)                                               # a non-finite twin value counts as caught
    sl = slice(dc.lo, dc.hi)
    assert caught[sl].mean() >= 0.99, (defect, float(caught[sl].mean()))
    assert not caught[:dc.lo].any() or dc.lo == 0                         # the elements before `lo` are those the defect leaves alone


def test_defects_cover_the_list():
    assert set(SC.defect_cases()) == set(SC.DEFECTS)


def test_tail_seeds_have_the_stated_r0():
    assert SC.first_r0(SC.TAIL_SEED_U0_ONE) == SC.TAIL_R0_U0_ONE >= 2 ** 32 - 128
    assert SC.first_r0(SC.TAIL_SEED_U0_SMALL) == SC.TAIL_R0_U0_SMALL < 2 ** 12
    z, ra = SC._model(SC.TAIL_SEED_U0_ONE, 0, 0, 4, 4)
    assert ra[0] == 0.0 and z[0] == 0.0 and z[1] == 0.0                   # u0 rounds to 1: the radius is exactly 0
    z, ra = SC._model(SC.TAIL_SEED_U0_SMALL, 0, 0, 4, 4)
    assert ra[0] > 6.0 and max(abs(z[0]), abs(z[1])) > 4.0                # the far tail: |z| beyond 4 sigma
    # a chunk of the search, re-run: no earlier key of it reaches the top range
    s = np.arange(SC.TAIL_SEED_U0_ONE - 4096, SC.TAIL_SEED_U0_ONE + 1, dtype=np.uint64)
    r0 = SC.philox4x32_10((0, 0, 0, 0), (s, 0))[..., 0]
    assert np.nonzero(r0 >= 2 ** 32 - 128)[0].tolist() == [4096]


def _check32(o32, o64, bound):
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64
    err = (o32.double() - o64).abs()
    assert bool((err <= bound + 1e-30).all()), float((err / (bound + 1e-30)).max())
    assert float(err.max()) > 0.0                                         # the fp32 form does round: the bound is not vacuous


@pytest.mark.parametrize("mix", [False, True], ids=["nomix", "cfg"])
@pytest.mark.parametrize("n", [4, 4 * 257])
def test_update_expressions_fp32_within_rounding_count_of_fp64(n, mix):
    op = SC.update_operands(n)
    d = {k: v.double() for k, v in op.items()}
    x0, x0d, e_x0 = op["x0"], d["x0"], None
    if mix:
        x0, x0d = SC.cfg_mix(op["x0"], op["x0u"], SC.CFG_SCALE), SC.cfg_mix(d["x0"], d["x0u"], SC.CFG_SCALE)
        e_x0 = SC.mix_bound(op["x0"], op["x0u"], SC.CFG_SCALE)
        _check32(x0, x0d, e_x0)
    for c in SC.MODE0_COEFS.values():
        _check32(SC.update_mode0(*c, x0, op["x"], op["z"]), SC.update_mode0(*c, x0d, d["x"], d["z"]),
                 SC.mode0_bound(*c, x0d, op["x"], op["z"], e_x0))
    for c in SC.MODE1_COEFS.values():
        _check32(SC.update_mode1(*c, x0, op["x"]), SC.update_mode1(*c, x0d, d["x"]), SC.mode1_bound(*c, x0d, op["x"], e_x0))
    for c in SC.MODE3_COEFS.values():
        _check32(SC.update_mode3(*c, x0, op["x"], op["h"], op["z"]), SC.update_mode3(*c, x0d, d["x"], d["h"], d["z"]),
                 SC.mode3_bound(*c, x0d, op["x"], op["h"], op["z"], e_x0))


def test_update_bounds_count_three_and_five_roundings():
    x = torch.ones(4)
    c1, c2, sg = 1.0, 1.0, 1.0
    assert torch.allclose(SC.mode0_bound(c1, c2, sg, 0, x, x, x), torch.full((4,), SC.gamma(3) * 2.0, dtype=torch.float64))
    assert torch.allclose(SC.mode0_bound(c1, c2, sg, 5, x, x, x), torch.full((4,), SC.gamma(5) * 3.0, dtype=torch.float64))
    assert SC.gamma(3) == pytest.approx(3 * SC.U, rel=1e-6) and SC.gamma(5) == pytest.approx(5 * SC.U, rel=1e-6)


def test_noise_tolerance_constants():
    assert SC.E_REL == 8.0 * SC.U
    assert SC.E_TRIG == SC.E_TRIG_MARGIN * SC.E_TRIG_MEASURED and SC.E_TRIG_MARGIN == 4.0
    assert SC.RA_MAX * SC.E_TRIG + SC.RA_MAX * SC.E_REL < SC.NOISE_ERR_CONDITION      # the bound never reaches the condition
