"""CPU: the host tables of the table-driven multistep sampler (fdm_sampler_tables_host: DPM-Solver++ 2M and DDIM with eta)
against an fp64 restatement of the published formulas, against the library's existing DDIM tables, and on a closed-form
problem that shows the order of the shipped 2M tables; argument validation of the host function and of fdm_sample_graph
kind 2.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

from fdm_amd import _lib, schedule

T = 1000


def abar64(n=T):
    """alphas_cumprod of the cosine schedule in fp64 (the expression order of schedule.cosine_beta_schedule)."""
    x = np.linspace(0, n, n + 1, dtype=np.float64)
    ac = np.cos(((x / n) + 0.008) / 1.008 * np.pi * 0.5) ** 2
    ac = ac / ac[0]
    return np.cumprod(1.0 - np.clip(1.0 - ac[1:] / ac[:-1], 0, 0.9999))


AB = abar64()


def grid(steps):
    times = np.linspace(-1, T - 1, steps + 1).astype(np.int32)[::-1].tolist()
    return list(zip(times[:-1], times[1:]))


def restate(kind, steps, eta=0.0):
    """t [steps], tables [4, steps] in fp64, from the formulas of include/fdm_hip.h."""
    t, tab = [], np.zeros((4, steps))
    h_prev = None
    for k, (tc, tn) in enumerate(grid(steps)):
        t.append(tc)
        if tn < 0:                                       # alpha_bar(-1) := 1: the step lands on the x0 prediction
            tab[:, k] = (0.0, 1.0, 0.0, 0.0)
            continue
        ab, abn = AB[tc], AB[tn]
        if kind == "ddim_eta":
            sg = eta * np.sqrt((1 - abn) / (1 - ab)) * np.sqrt(1 - ab / abn)
            a = np.sqrt(1 - abn - sg * sg) / np.sqrt(1 - ab)
            tab[:, k] = (a, np.sqrt(abn) - a * np.sqrt(ab), 0.0, sg)
            continue
        lam = lambda v: np.log(np.sqrt(v) / np.sqrt(1 - v))
        h = lam(abn) - lam(ab)
        phi = np.sqrt(abn) * (1 - np.exp(-h))
        if k == 0:
            b, c = phi, 0.0
        else:
            r = h_prev / h
            b, c = phi * (1 + 1 / (2 * r)), -phi / (2 * r)
        tab[:, k] = (np.sqrt(1 - abn) / np.sqrt(1 - ab), b, c, 0.0)
        h_prev = h
    return t, tab


CASES = [("dpmpp2m", 0.0)] + [("ddim_eta", e) for e in (0.0, 0.5, 1.0)]


@pytest.mark.parametrize("steps", [1, 2, 3, 20, 50])
@pytest.mark.parametrize("kind,eta", CASES)
def test_tables_against_the_fp64_restatement(kind, eta, steps):
    t, tab = schedule.sampler_tables(kind, steps, eta)
    rt, rtab = restate(kind, steps, eta)
    assert t == rt                                       # exact
    tab = tab.numpy().astype(np.float64)
    err = np.abs(tab - rtab) / np.maximum(np.abs(rtab), 1e-300)
    err[rtab == 0] = np.abs(tab[rtab == 0])             # exact zeros stay exact zeros
    assert err.max() <= 1e-6, (kind, eta, steps, err.max())
    assert tab[:, -1].tolist() == [0.0, 1.0, 0.0, 0.0]   # the final pair (t_last, -1) goes to data
    if steps == 1:
        assert t == [T - 1]
    if kind == "dpmpp2m":
        assert tab[2, 0] == 0.0 and not tab[3].any()
        if steps > 2:
            assert (tab[2, 1:-1] < 0).all()
    elif eta == 0:
        assert not tab[3].any()
    else:
        assert (tab[3, :-1] > 0).all() or steps == 1


@pytest.mark.parametrize("steps", [2, 3, 20, 50])
def test_ddim_eta0_matches_the_existing_host_schedule(steps):
    """The eta = 0 tables are the library's own DDIM update, x0 sqrt_an + c_n (sra x - x0) / srm1, written as a x + b x0.
    (The step counts of the table test above.  fdm_ddim_schedule_host forms c_n = sqrt(1 - abar_next) in fp32 from the fp32
    abar_next: near t = 0 that difference keeps ~1e-5 of relative accuracy, which is the 1e-5 bar; denser grids than these end
    closer to t = 0 and measure that rounding of the OLD table, not the new one, which is built in fp64.)"""
    l = _lib.lib()
    buf = np.zeros((12, T), np.float32)
    assert l.fdm_schedule_host(T, buf.ctypes.data) == 0
    sra, srm1 = buf[6].astype(np.float64), buf[7].astype(np.float64)
    tt, tn = np.zeros(steps, np.int32), np.zeros(steps, np.int32)
    san, cn = np.zeros(steps, np.float32), np.zeros(steps, np.float32)
    n = l.fdm_ddim_schedule_host(steps, T, tt.ctypes.data, tn.ctypes.data, san.ctypes.data, cn.ctypes.data)
    assert n == steps - 1
    t, tab = schedule.sampler_tables("ddim_eta", steps, 0.0)
    assert t[:n] == tt[:n].tolist()
    tab = tab.numpy().astype(np.float64)
    a_ref = cn[:n].astype(np.float64) * sra[tt[:n]] / srm1[tt[:n]]
    b_ref = san[:n].astype(np.float64) - cn[:n].astype(np.float64) / srm1[tt[:n]]
    assert np.max(np.abs(tab[0, :n] - a_ref) / np.abs(a_ref)) <= 1e-5
    assert np.max(np.abs(tab[1, :n] - b_ref) / np.abs(b_ref)) <= 1e-5


@pytest.mark.parametrize("steps", [1, 2, 3, 5, 20, 50, 100])
def test_2m_coefficients_amplify_nothing(steps):
    _, tab = schedule.sampler_tables("dpmpp2m", steps)
    assert float(tab[:3].abs().max()) == 1.0              # the final pair's b; everything else is below


def _chain_error(tab, t, s):
    """Scalar data N(0, s^2): the exact x0 predictor is alpha s^2 / (alpha^2 s^2 + sigma^2) x and the exact probability-flow
    solution x_t = x_T sqrt((abar_t s^2 + 1 - abar_t) / (abar_T s^2 + 1 - abar_T)).  Runs the first steps - 1 steps from
    x_T = 1 and returns the relative error at t_last."""
    x, prev = 1.0, 0.0
    n = len(t)
    for k in range(n - 1):
        ab = AB[t[k]]
        x0 = np.sqrt(ab) * s * s / (ab * s * s + 1 - ab) * x
        x, prev = tab[0, k] * x + tab[1, k] * x0 + tab[2, k] * prev, x0
    exact = np.sqrt((AB[t[n - 1]] * s * s + 1 - AB[t[n - 1]]) / (AB[t[0]] * s * s + 1 - AB[t[0]]))
    return abs(x - exact) / exact


@pytest.mark.parametrize("s", [0.5, 2.0])
def test_shipped_2m_tables_are_second_order(s):
    """First order = DDIM at eta = 0.  With fp64 tables: s = 0.5: 6.1e-2 | 1.3e-2 at 20 steps, 3.4e-2 | 6.7e-3 at 40,
    1.8e-2 | 2.5e-3 at 80; s = 2: 7.3e-2 | 2.3e-2, 3.7e-2 | 7.3e-3, 1.9e-2 | 2.3e-3 (ratios 5.1 to 8.3 at 40 and 80 steps)."""
    for steps in (5, 10, 20, 40, 80):
        t1, d1 = schedule.sampler_tables("ddim_eta", steps, 0.0)
        t2, d2 = schedule.sampler_tables("dpmpp2m", steps)
        e1 = _chain_error(d1.numpy().astype(np.float64), t1, s)
        e2 = _chain_error(d2.numpy().astype(np.float64), t2, s)
        print(f"s={s} steps={steps}: first order {e1:.3e} | 2M {e2:.3e} (ratio {e1 / e2:.2f})")
        assert e2 < e1, (s, steps, e1, e2)
        if steps in (40, 80):
            assert e2 <= e1 / 3, (s, steps, e1, e2)


def test_argument_validation_without_a_device():
    l = _lib.lib()
    n = 8
    t = (C.c_int * n)()
    f = [(C.c_float * n)() for _ in range(4)]
    ok = lambda kind, steps, Tn, eta, *out: l.fdm_sampler_tables_host(kind, steps, Tn, eta, *(out or (t, *f)))
    assert ok(_lib.SAMPLER_DPMPP_2M, 4, T, 0.0) == 0 and ok(_lib.SAMPLER_DDIM, 4, T, 1.0) == 0
    assert ok(_lib.SAMPLER_DDIM, 8, 8, 0.0) == 0                           # steps == T
    for bad in ((_lib.SAMPLER_DPMPP_2M, 0, T, 0.0), (_lib.SAMPLER_DDIM, -1, T, 0.0), (_lib.SAMPLER_DDIM, 9, 8, 0.0),
                (_lib.SAMPLER_DDIM, 4, T, -0.1), (_lib.SAMPLER_DDIM, 4, T, 1.5), (_lib.SAMPLER_DDIM, 4, T, float("nan")),
                (_lib.SAMPLER_DPMPP_2M, 4, T, 0.5), (2, 4, T, 0.0), (-1, 4, T, 0.0)):
        assert ok(*bad) == -1, bad
        assert b"sampler_tables_host" in l.fdm_last_error()
    for i in range(5):                                                      # each output pointer
        out = [t, *f]
        out[i] = None
        assert ok(_lib.SAMPLER_DPMPP_2M, 4, T, 0.0, *out) == -1 and b"null output" in l.fdm_last_error()
    with pytest.raises(_lib.FdmError):
        schedule.sampler_tables("ddim_eta", 0)
    with pytest.raises(ValueError):
        schedule.sampler_tables("heun", 4)
    # fdm_sample_graph / fdm_sample_windows kind 2: the sampler's own arguments are checked before the plan is looked at
    ts = (C.c_int * 4)(999, 700, 400, 100)
    tab = (C.c_float * 16)()
    for fn in (l.fdm_sample_graph, l.fdm_sample_windows):
        a = _lib.SampleArgs()
        a.kind, a.x_T, a.out, a.t_list, a.n_steps = 2, 16, 16, C.cast(ts, C.c_void_p), 4
        assert fn(None, C.byref(a), None) == -1 and b"lm_tables" in l.fdm_last_error()          # null tables
        a.lm_tables = C.cast(tab, C.c_void_p)
        a.n_steps = 0
        assert fn(None, C.byref(a), None) == -1 and b"lm_tables" in l.fdm_last_error()          # n_steps < 1
        a.n_steps, a.t_list = 4, None
        assert fn(None, C.byref(a), None) == -1 and b"lm_tables" in l.fdm_last_error()
        a.t_list = C.cast(ts, C.c_void_p)
        assert fn(None, C.byref(a), None) == -1 and b"null plan" in l.fdm_last_error()          # well-formed: the plan is what is missing
    # mode 3 of the operator: tables and history are required
    s = _lib.SchedArgs()
    s.x0, s.x, s.x_out, s.n, s.mode, s.noise = 16, 16, 16, 8, 3, 16
    assert l.fdm_op_sched_step(C.byref(s), None) == -1 and b"lm_a" in l.fdm_last_error()
    s.mode = 4
    assert l.fdm_op_sched_step(C.byref(s), None) == -1 and b"bad mode" in l.fdm_last_error()
